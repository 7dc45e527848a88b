"""not gpu: the token policy loss pinned on the host -- the numpy emulation of tests/token_policy_cases.py against its brute-force second formulation, what the
case table claims, the planted mistakes and how far each moves a case, logprob / lse / entropy against the SCORER's and the LOSS's emulations bit for bit, every
output against torch fp64 autograd of the textbook loss under derived bounds, the C entry against the ctypes table, the kernels' resource budget, the host-side
refusals, token_policy_loss's bookkeeping over a stub of ops and group_advantages against numpy."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import token_policy_cases as PC
import token_sample_cases as TC
import token_score_cases as SC
import token_xent_cases as XC
from selftoktokenizer_amd import _lib, losses, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "selftok_policy_rows"
f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64
NAMES = [c.name for c in PC.CASES]


def _values(c, grad):
    """a gradient buffer as fp32 values"""
    return TC.widen_bf16(grad) if c.dtype == "bf16" else grad


def _bits(c, grad):
    return grad.view(np.uint16 if c.dtype == "bf16" else u32)


@pytest.mark.parametrize("name", NAMES)
def test_emulation_equals_the_brute_force_formulation(name):
    c = PC.BY_NAME[name]
    a, b = PC.reference(name), PC.reference(name, brute=True)
    assert len(a.logprob) == PC.rows_of(c) and PC.same(name, a, b), PC.differing_rows(name, a, b)[:3]
    live = ~a.bad & ~a.ignored
    for out in (a.logprob, a.lse, a.ratio, a.kl, a.coef) + (() if a.entropy is None else (a.entropy,)):
        assert np.isnan(out[a.bad]).all()
    assert (a.flags[~live] == 0).all() and np.isfinite(a.lse[~a.bad]).all() and (a.ratio[live] >= 0).all() and (a.logprob[live] <= 0).all()
    for out in (a.logprob, a.ratio, a.kl, a.coef) + (() if a.entropy is None else (a.entropy,)):
        assert (out[a.ignored].view(u32) == 0).all()                # +0, bit for bit
    assert (a.entropy is None) == (c.entc == 0 and not c.went)
    v = _values(c, a.grad)
    assert (v[:, c.V:] == PC.SENT).all() and (v[:, :c.offset] == 0).all() and (v[:, c.offset + c.C:c.V] == 0).all()       # pad columns untouched, the rest written
    assert (v[~live, :c.V].view(u32) == 0).all()


def test_the_case_table_holds_what_it_claims():
    cs = PC.CASES
    assert {1, 2, 3, 4, 5} | set(PC.GEOMETRY_C) <= {c.C for c in cs} and {1, 3, 5, 64, PC.GRID_X + 1} <= {PC.rows_of(c) for c in cs}
    steps = {(c.S, PC.id_geometry(c)[3]) for c in cs}
    assert {s for s, _ in steps} >= {1, 3, 40} and {st for s, st in steps if s > 1} == {1, -1, 2, -2}
    assert {c.ids for c in cs} == {"int32", "int64"} and {c.dtype for c in cs} == {"f32", "bf16"} and {0, PC.OFFSET_VLM} <= {c.offset for c in cs}
    assert any(c.row > c.V for c in cs) and any(c.V > c.offset + c.C for c in cs) and {c.scale for c in cs} == {None, "const", "rows"}
    assert 0.0 in XC.ROW_SCALES and min(XC.ROW_SCALES) < 0
    ent = lambda c: c.entc != 0 or c.went
    kernels = [lambda c: c.C <= PC.SMALL_C and not ent(c), lambda c: c.C <= PC.SMALL_C and ent(c), lambda c: PC.SMALL_C < c.C <= PC.REG_C and not ent(c),
               lambda c: PC.SMALL_C < c.C <= PC.ENT_C and ent(c), lambda c: c.C > PC.REG_C and not ent(c), lambda c: c.C > PC.ENT_C and ent(c)]
    for mine in ([c for c in cs if k(c)] for k in kernels):        # every instance: both dtypes, a reference, bad rows of both kinds, ignored rows
        assert {c.dtype for c in mine} == {"f32", "bf16"} and {"badtargets", "ignored"} <= {c.tk for c in mine}, [c.name for c in mine]
        assert any(c.old == "badops" for c in mine) and any(c.ref is not None for c in mine) and any(c.scale == "rows" for c in mine), [c.name for c in mine]
    assert {(c.klc != 0, c.entc != 0) for c in cs} == {(False, False), (True, False), (False, True), (True, True)}
    assert all(c.offset % 4 == 0 and c.row % 4 == 0 and c.offset + c.C <= c.V <= c.row for c in cs)
    neg_zero = []
    for c in cs:
        d, ref = PC.make(c.name), PC.reference(c.name)
        full = TC.widen_bf16(d["logits"]) if c.dtype == "bf16" else d["logits"]
        outside = np.ones(c.row, bool)
        outside[c.offset:c.offset + c.C] = False
        assert np.isnan(full[:, outside]).all() and np.array_equal(PC.gather_targets(c, d), d["targets"])
        assert (d["ids"] == PC.POISON).sum() == d["ids"].size - PC.rows_of(c)
        live = ~ref.bad & ~ref.ignored
        lo, hi = PC.clip_bounds(c)
        if c.old == "edge":                                         # the six ratios exactly, each with A > 0, A < 0 and A = 0
            want = np.asarray(PC.edge_targets(c), f32)[np.arange(18) % 6]
            assert np.array_equal(ref.ratio.view(u32), want.view(u32)) and d["adv"].tolist() == [1.25] * 6 + [-0.5] * 6 + [0.0] * 6
            assert ref.flags.tolist() == [0, 0, 0, 0, 0, 1] + [2, 0, 0, 0, 0, 0] + [0] * 6 and not ref.bad.any()
            assert (ref.coef[[5, 6]] == 0).all() == (c.klc == 0) and (ref.coef[12:] == 0).all() == (c.klc == 0)
        if c.old == "eq":                                           # on policy: a difference of exactly 0
            assert (ref.ratio[live] == 1).all() and (ref.flags == 0).all()
            if c.ref == "eq":
                assert (ref.kl[live].view(u32) == 0).all() and (ref.e[live] == 0).all()
        if c.old == "huge":                                         # a ratio above the fp32 range: clipped with A > 0, a policy term of -inf with A < 0, 0 with A = 0
            assert np.isinf(ref.ratio).all() and ref.flags.tolist() == [1, 0, 0] * 2 and (ref.coef[1::3] == -np.inf).all() and np.isfinite(ref.coef[0::3]).all()
            assert np.isfinite(ref.coef[2::3]).all() and not ref.bad.any()
        if c.tk == "neginf":                                        # a target at -inf: ratio 0 with a finite old_logprob, bad against -inf
            assert ref.bad.sum() == 1 and (ref.ratio[[0] if c.ref else [0, 4]] == 0).all() and (ref.logprob[[0]] == -np.inf).all() and ref.bad[4 if c.ref else 2]
        if c.tk == "lowest":
            t = d["targets"]
            assert (ref.q[np.arange(len(t)), t] == 0).all() and np.isfinite(ref.logprob).all() and (ref.logprob < -24).all()
        if c.tk == "ignored":
            assert ref.ignored.tolist() == [False, True, True] * (PC.rows_of(c) // 3) and not ref.bad.any()
        if c.tk == "badtargets":
            assert ref.bad.tolist() == [False, True, True, True, False, True, False, True, False]
        if c.old == "badops":
            assert ref.bad.tolist() == [False, True, True, True, False, True, True, True, False]
        if c.adv == "neg" and c.kind == "gauss8" and c.entc == 0:   # negative coefficients over codes without mass: -0.0 in the gradient, which an added +0 would lose
            neg_zero.append(bool((_bits(c, ref.grad)[:, c.offset:c.offset + c.C] == (0x8000 if c.dtype == "bf16" else 0x80000000)).any()))
    assert any(neg_zero), neg_zero


MIN_MOVED = {"ratio_from_f64_lp": 30, "clip_ge": 3, "clipped_keeps_coef": 20, "k3_sign": 15, "kl_missing_from_coef": 15, "target_p_minus_1": 20, "ent_grad_without_H": 15,
             "ent_added_at_zero": 4, "scale_not_on_ent": 5, "ignored_unwritten": 5, "tail_chunk_dropped": 15}


def moved_by(name, mut):
    """the largest change a mistake makes to any output of a case, in units of that output's GATE in tests/test_token_policy_gpu.py: logprob, lse, entropy and
    flags are compared exactly (any change is infinitely many gates), ratio to one fp32 ulp, kl and coef to `kl_gate` / `coef_gate`, and the gradient exactly at
    the coefficient the row got (so a row whose coefficient did not move must keep every gradient bit)"""
    c, d = PC.BY_NAME[name], PC.make(name)
    ref, got = PC.reference(name), PC.reference(name, mut=mut)
    worst = 0.0
    with np.errstate(all="ignore"):
        exact = [(ref.logprob, got.logprob), (ref.lse, got.lse)] + ([] if ref.entropy is None else [(ref.entropy, got.entropy)])
        for a, b in exact:
            if not ((a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))).all():
                return np.inf
        if not np.array_equal(ref.flags, got.flags):
            return np.inf
        for a, b, gate in ((ref.ratio, got.ratio, PC.ratio_gate(d, ref)), (ref.kl, got.kl, PC.kl_gate(ref)), (ref.coef, got.coef, PC.coef_gate(c, d, ref))):
            same = (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))
            r = np.where(same, 0.0, np.where(np.isfinite(a) & np.isfinite(b) & np.isfinite(gate) & (gate > 0), np.abs(a.astype(f64) - b.astype(f64)) / np.where(gate > 0, gate, 1.0), np.inf))
            worst = max(worst, float(r.max()))
        kept = ref.coef.view(u32) == got.coef.view(u32)
        if not np.array_equal(_bits(c, ref.grad)[kept | ref.bad | ref.ignored], _bits(c, got.grad)[kept | ref.bad | ref.ignored]):
            return np.inf
    return worst


@pytest.mark.parametrize("mut", PC.MUTS)
def test_each_planted_mistake_changes_exactly_the_cases_it_names(mut):
    """the emulation with a mistake planted moves a case if and only if `applies` -- the brute-force formulation with the same mistake written a second time --
    says so, only where `needs` allows it, and then by at least 1000 gates of the GPU comparison.  One exception, stated: the ratio taken from the UNROUNDED
    logprob differs from the record by |logprob| / 2 ulps at the most -- a handful -- which is of the size of the one-ulp allowance the device's exp needs; it is
    held to 1000 gates where the comparison has no allowance, the on-policy cases (old_logprob = logprob: a ratio of exactly 1.0f), and must move every one of them"""
    moved = strict = 0
    for c in PC.CASES:
        got = not PC.same(c.name, PC.reference(c.name), PC.reference(c.name, mut=mut))
        assert got == PC.applies(mut, c.name), (mut, c.name)
        assert not got or PC.needs(mut, c), (mut, c.name)
        if got and (mut != "ratio_from_f64_lp" or c.old == "eq"):
            assert moved_by(c.name, mut) >= 1000.0, (mut, c.name, moved_by(c.name, mut))
            strict += 1
        elif got:                                                   # the stated exception: seen all the same -- some row's ratio at least a whole ulp off, the size of the gate
            assert moved_by(c.name, mut) >= 1.0, (mut, c.name, moved_by(c.name, mut))
        moved += got
    assert moved >= MIN_MOVED[mut] and strict >= (2 if mut == "ratio_from_f64_lp" else moved), (mut, moved, strict)
    assert len(PC.MUTS) >= 10 and set(MIN_MOVED) == set(PC.MUTS)


@pytest.mark.parametrize("name", NAMES)
def test_logprob_lse_and_entropy_are_the_scorers_and_the_losses(name):
    """logprob and entropy: the scorer's emulation, bit for bit; lse and -logprob: the loss's; and with ent_coef = 0 the whole gradient is the loss's emulation
    run with row_scale = this emulation's coefficient"""
    c, d = PC.BY_NAME[name], PC.make(name)
    mine = PC.reference(name)
    l, t = PC.window(name), d["targets"]
    theirs = SC.score_rows(l, None, t)
    live = ~mine.bad & ~mine.ignored
    assert np.array_equal(mine.q_total[~theirs.bad], theirs.q_total[~theirs.bad]) and not (theirs.bad & ~mine.bad).any()
    assert np.array_equal(mine.logprob[live].view(u32), theirs.logprob[live].view(u32))
    if mine.entropy is not None:
        assert np.array_equal(mine.entropy[live].view(u32), theirs.entropy[live].view(u32)) and live.any()
    ok = np.isfinite(mine.coef) | mine.bad                          # the loss's emulation takes any scale; keep the comparison to rows it was built for
    loss = XC.xent_rows(l, np.where(mine.bad & ~theirs.bad, -1, t), scale=np.where(mine.bad, f32(0), mine.coef), V=c.V, offset=c.offset, row=c.row, bf16=c.dtype == "bf16")
    good = ~loss.bad
    assert np.array_equal(mine.lse[good & ~mine.bad].view(u32), loss.lse[good & ~mine.bad].view(u32))
    assert np.array_equal(mine.logprob[live].view(u32), loss.nll[live].view(u32) ^ u32(0x80000000))
    if c.entc == 0:
        assert np.array_equal(_bits(c, mine.grad)[ok], _bits(c, loss.grad)[ok])


def _textbook(l, t, old, A, ref, lo, hi, klc, entc, g):
    """the textbook loss of one row in torch fp64 on the fp32 values -> (loss pieces, gradient)"""
    x = torch.from_numpy(l.astype(f64)).requires_grad_(True)
    logp = torch.log_softmax(x, 0)
    lp = logp[int(t)]
    ratio = torch.exp(lp - float(old))
    surrogate = torch.minimum(ratio * float(A), torch.clamp(ratio, float(lo), float(hi)) * float(A))
    kl = torch.zeros((), dtype=torch.float64)
    if ref is not None:
        u = float(ref) - lp
        kl = torch.expm1(u) - u
    p = torch.exp(logp)
    H = -(p * torch.where(p > 0, logp, torch.zeros_like(logp))).sum()
    (float(g) * (-surrogate + klc * kl - entc * H)).backward()
    return float(torch.logsumexp(x.detach(), 0)), float(lp.detach()), float(ratio.detach()), float(kl.detach()), float(H.detach()), p.detach().numpy(), logp.detach().numpy(), x.grad.numpy()


def test_outputs_and_gradient_against_fp64_autograd_within_the_derived_bounds():
    """-min(ratio A, clamp(ratio, lo, hi) A) + kl_coef k3 - ent_coef H, scaled by g, and autograd, in fp64 on the same fp32 values.  The bounds are derived (DESIGN
    38.4), not measured: the loss's bounds for lp, lse and the softmax gradient, carried through exp and expm1 into the ratio, the k3 estimate and the
    coefficient, and the scorer's entropy bound into the entropy term.  A row whose ratio lies within its bound of a clip edge is left out of the coefficient
    and gradient comparison: there the textbook loss itself is not differentiable.  The largest shares are written to profiles/token_policy_bound.txt."""
    worst = {k: (0.0, "") for k in ("logprob", "lse", "ratio", "kl", "entropy", "coef", "grad")}
    rows = skipped = 0
    for c in PC.CASES:
        if PC.rows_of(c) > 64 or c.C > 20000:
            continue
        ref, d, l = PC.reference(c.name), PC.make(c.name), PC.window(c.name)
        lo, hi = PC.clip_bounds(c)
        klc, entc = float(c.klc), float(c.entc)
        v = _values(c, ref.grad)[:, c.offset:c.offset + c.C].astype(f64)
        for r in np.flatnonzero(~ref.bad & ~ref.ignored):
            A, old = float(d["adv"][r]), float(d["old"][r])
            rf = None if d["ref"] is None else float(d["ref"][r])
            if not (np.isfinite(ref.logprob[r]) and np.isfinite(ref.ratio[r]) and np.isfinite(old) and (rf is None or np.isfinite(rf))):
                continue                                            # a target at -inf, a ratio above the fp32 range: the textbook loss is inf or NaN
            g = 1.0 if d["scale"] is None else float(d["scale"][r])
            L, lp, ratio, kl, H, p, logp, grad = _textbook(l[r], d["targets"][r], old, A, rf, lo, hi, klc, entc, g)
            checks = [("lse", float(ref.lse[r]), L, PC.bound_row_scalar(c.C, L)), ("logprob", float(ref.logprob[r]), lp, PC.bound_row_scalar(c.C, lp)), ("ratio", float(ref.ratio[r]), ratio, PC.bound_ratio(c.C, lp, ratio))]
            if rf is not None:
                checks.append(("kl", float(ref.kl[r]), kl, PC.bound_k3(c.C, lp, rf - lp, kl)))
            if ref.entropy is not None:
                checks.append(("entropy", float(ref.entropy[r]), H, PC.bound_entropy(c.C, H)))
            for what, got, want, b in checks:
                assert abs(got - want) <= b, (c.name, r, what, got, want, b)
                worst[what] = max(worst[what], (abs(got - want) / b, c.name))
            b_ratio = PC.bound_ratio(c.C, lp, ratio)
            if A != 0 and min(abs(ratio - float(lo)), abs(ratio - float(hi))) <= b_ratio:
                skipped += 1
                continue
            clipped = (A > 0 and ratio > hi) or (A < 0 and ratio < lo)
            assert clipped == (ref.flags[r] != 0), (c.name, r)
            u = 0.0 if rf is None else rf - lp
            k64 = g * ((0.0 if clipped else A * ratio) + klc * math.expm1(u))
            bk = PC.bound_coef(c.C, lp, A, ratio, clipped, klc if rf is not None else 0.0, u, g, k64)
            assert abs(float(ref.coef[r]) - k64) <= bk, (c.name, r, "coef", float(ref.coef[r]), k64, bk)
            worst["coef"] = max(worst["coef"], (abs(float(ref.coef[r]) - k64) / bk, c.name))
            onehot = np.zeros(c.C)
            onehot[d["targets"][r]] = 1.0
            bg = PC.bound_softmax_grad(c.C, p, k64, k64, 0.0, 0.0, onehot) + bk * (p + onehot)
            if entc:
                bg = bg + PC.bound_entropy_grad(c.C, p, np.where(p > 0, logp, 0.0) + H, g * entc, H) + 2.0 ** -23 * np.abs(grad)
            if c.dtype == "bf16":
                bg = bg + (np.abs(grad) + bg) * 2.0 ** -8
            eg = np.abs(v[r] - grad)
            assert (eg <= bg).all(), (c.name, r, "grad", float((eg / bg).max()), int(np.argmax(eg / bg)))
            worst["grad"] = max(worst["grad"], (float((eg / bg).max()), c.name))
            rows += 1
    text = "token policy loss against torch fp64 autograd (tests/test_token_policy_cpu.py, DESIGN 38.4): %d rows, %d more at a clip edge compared without their " \
           "gradient; largest share of the derived bound -- " % (rows, skipped) + ", ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in worst.items())
    print("\n" + text)
    try:
        with open(os.path.join(ROOT, "profiles", "token_policy_bound.txt"), "w") as f:
            f.write(text + "\n")
    except OSError:
        pass
    assert rows >= 150 and skipped >= 6 and all(v[0] > 0 for k, v in worst.items())


def test_ext_header_declares_the_entry_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "float": C.c_float, "unsigned": C.c_uint}
    m = re.search(r"(\w+)\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and ENTRY in _lib.EXT_SIGNATURES and ENTRY not in _lib.SIGNATURES and not ENTRY.startswith("selftok_token_")
    args = [a.strip() for a in m.group(2).split(",")]
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
    res, got = _lib.EXT_SIGNATURES[ENTRY]
    assert got == want and res == ctype_of[m.group(1)] and len(got) == 32, args
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_policy_rows.argtypes == got


def test_token_policy_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 12 kernels (fp32 / bf16 each).  Without the entropy sum: 2 chunks 34 VGPRs, 16 chunks 92 - 94 VGPRs (5 waves per SIMD), streamed 27 - 28.
    With it: 2 chunks 44, 8 chunks 117 (4 waves per SIMD: two 512-thread workgroups per compute unit), streamed 36.  56 bytes of LDS each.  The 10-, 12- and
    16-chunk instances with the entropy sum spill (56 - 364 bytes) and are not built."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_policy.o")
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 12 and all("tok_policy_kernel" in k for k in kernels), kernels
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 128 and l <= 64 and o >= 4 for v, l, o in zip(vgprs, lds, occ)), (vgprs, lds, occ)
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(G.CSRC, "token_policy.hip")).read().splitlines())
    assert "asm" not in code and "expf" not in code and "fma" not in code and "hipMalloc" not in code and "atomicAdd(float" not in code
    assert '#include "token_shared.h"' in code and not re.search(r"\brintf\b", code) and "0x9E3779B9" not in code       # the mass is the shared header's, not restated


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(8192, 0x5A5A5A5A, u32)
    p = x.ctypes.data
    assert p % 16 == 0
    q = p + 4096 * 4                                                # a second buffer, disjoint from a 2-row x 128-code fp32 call's extents

    def call(logits=p, dtype=0, R=2, C=100, rs=128, off=0, ids=p, ib=8, S=1, seq=1, step=1, V=None, scale=None, old=p, adv=p, ref=None, clo=0.2, chi=0.2, klc=0.0, entc=0.0,
             lp=p, lse=p, ratio=p, kl=p, ent=None, coef=p, flags=p, grad=q, gs=128, bad=p, ign=p):
        return lib.selftok_policy_rows(logits, dtype, R, C, rs, off, ids, ib, S, seq, step, off + C if V is None else V, scale, old, adv, ref, clo, chi, klc, entc, lp, lse,
                                       ratio, kl, ent, coef, flags, grad, gs, bad, ign, None)

    for kw in (dict(clo=-0.1), dict(clo=1.0), dict(clo=float("nan")), dict(chi=-1.0), dict(chi=float("inf")), dict(chi=float("nan"))):
        assert call(**kw) == -1 and "clip" in err(), kw
    for kw in (dict(klc=-1.0, ref=p), dict(klc=float("nan"), ref=p), dict(klc=float("inf"), ref=p), dict(entc=-1e-30), dict(entc=float("inf")), dict(entc=float("nan"))):
        assert call(**kw) == -1 and "coef" in err(), kw
    assert call(klc=0.1) == -1 and "ref_logprob" in err() and call(klc=0.1, R=0) == -1
    for kw in (dict(V=99), dict(V=0), dict(off=8, C=100, V=104), dict(V=129), dict(V=128, gs=124), dict(V=1 << 40)):      # V < offset + C, V > row_stride, V > grad_stride
        assert call(**kw) == -1 and "V" in err(), kw
    for kw in (dict(grad=p + 16), dict(grad=p + 128 * 4), dict(grad=p + 224 * 4), dict(logits=q + 64, grad=q), dict(grad=p, gs=132, rs=128), dict(grad=p, gs=124)):
        assert call(**kw) == -1 and ("overlap" in err() or "V" in err()), (kw, err())
    assert call(grad=p + 16) == -1 and "overlap" in err() and call(grad=p, gs=256, rs=128, V=100) == -1 and "overlap" in err()
    for C in (0, -1, 65537, 1 << 20):
        assert call(C=C, rs=1 << 21, V=1 << 21, gs=1 << 21) == -1 and "C" in err(), C
    for dt in (-1, 2, 16):
        assert call(dtype=dt) == -1 and "dtype" in err(), dt
    for ib in (0, 2, 3, 16):
        assert call(ib=ib) == -1 and "id_bytes" in err(), ib
    for S in (0, -1):
        assert call(S=S) == -1 and "rows_per_seq" in err(), S
    for kw in (dict(logits=None), dict(ids=None), dict(old=None), dict(adv=None), dict(lp=None), dict(lse=None), dict(ratio=None), dict(kl=None), dict(coef=None), dict(flags=None),
               dict(bad=None), dict(ign=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(logits=p + 4), dict(logits=p + 8), dict(grad=q + 4), dict(grad=q + 8), dict(off=2, rs=132, gs=132), dict(rs=130), dict(gs=130), dict(dtype=1, logits=p + 2),
               dict(dtype=1, grad=q + 4)):
        assert call(**kw) == -1 and "misaligned" in err(), kw
    for kw in (dict(ids=p + 4), dict(ib=4, ids=p + 2), dict(lp=p + 2), dict(lse=p + 1), dict(scale=p + 2), dict(old=p + 2), dict(adv=p + 1), dict(ref=p + 2), dict(ratio=p + 2),
               dict(kl=p + 2), dict(ent=p + 2), dict(coef=p + 2), dict(bad=p + 2), dict(ign=p + 2)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(C=100, rs=96), dict(C=100, off=32, rs=128), dict(off=-4), dict(rs=-1), dict(R=-1), dict(off=256, rs=128)):
        assert call(**kw) == -1 and "window" in err(), kw
    assert call(R=0, logits=None, ids=None, old=None, adv=None, lp=None, lse=None, ratio=None, kl=None, coef=None, flags=None, grad=None, bad=None, ign=None) == 0
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves its outputs untouched
    z = torch.zeros(2)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_policy(torch.zeros(2, 128), torch.zeros(2, dtype=torch.int64), z, z)


class _StubOps:
    """records every call and plays the kernel's part on the host: logprob = -(target + 1), ratio = 2 where the advantage is positive, else 0.5, clipped wherever
    the advantage is not 0 (clip 0.2), kl = 1, entropy = 3, coef = 7, the gradient row filled with the row's scale (1 without one); rows with a negative target
    ignored: +0 outputs, a zero row"""

    def __init__(self):
        self.calls = []

    def token_policy(self, logits, ids, old, adv, *, reverse_steps=False, **kw):
        B, S, V = logits.shape
        self.calls.append(dict(kw, reverse_steps=reverse_steps, old=old.clone(), adv=adv.clone(), ids_shape=tuple(ids.shape), ids_stride=tuple(ids.stride()),
                               ids_offset=ids.storage_offset()))
        t = (ids.flip(1) if reverse_steps else ids).to(torch.int64)
        ign = t < 0
        zero = torch.zeros(())
        a = adv.reshape(B, S)
        lp = torch.where(ign, zero, -(t.float() + 1))
        ratio = torch.where(ign, zero, torch.where(a > 0, torch.full((), 2.0), torch.full((), 0.5)))
        flags = torch.where(ign | (a == 0), torch.zeros((), dtype=torch.uint8), torch.where(a > 0, torch.ones((), dtype=torch.uint8), torch.full((), 2, dtype=torch.uint8)))
        g = torch.ones(B, S) if kw["row_scale"] is None else kw["row_scale"].reshape(B, S)
        grad = logits if kw["inplace"] else torch.empty_like(logits)
        grad.copy_(torch.where(ign, zero, g).unsqueeze(-1).expand(B, S, V))
        ent = torch.where(ign, zero, torch.full((), 3.0)) if kw["want_entropy"] else None
        return ops.PolicyOut(lp, torch.full((B, S), 2.0), ratio, torch.where(ign, zero, torch.ones(())), ent, torch.where(ign, zero, torch.full((), 7.0)), flags, grad,
                             torch.zeros(1, dtype=torch.int32), torch.tensor([int(ign.sum())], dtype=torch.int32))


def test_token_policy_loss_bookkeeping_over_an_ops_stub():
    B, K, S, V = 2, 6, 4, 16
    ids = torch.tensor([[10, 11, 12, 13, 14, 15], [20, 21, -1, 23, 24, 25]])
    new = lambda: torch.zeros(B, S, V, requires_grad=True)
    stub = _StubOps()
    adv_b = torch.tensor([1.0, -2.0])
    old_k = torch.arange(B * K, dtype=torch.float32).reshape(B, K)
    lg = new()
    loss, st = losses.token_policy_loss(lg, ids, old_k, adv_b, C=8, offset=4, ops=stub, return_stats=True)
    call = stub.calls[0]
    # AR step s meets position K - 1 - s: the view and direction of token_cross_entropy; [B, K] log-probabilities gathered to row order; [B] advantages broadcast
    assert call["reverse_steps"] and call["ids_offset"] == K - S and call["ids_stride"] == (K, 1) and (call["C"], call["offset"], call["inplace"]) == (8, 4, False)
    assert call["old"].tolist() == [[5.0, 4.0, 3.0, 2.0], [11.0, 10.0, 9.0, 8.0]] and call["adv"].tolist() == [[1.0] * 4, [-2.0] * 4] and call["ref_logprob"] is None
    assert call["clip"] == (0.2, 0.2) and call["kl_coef"] == 0.0 and call["ent_coef"] == 0.0 and call["want_entropy"]
    lo, hi = float(np.float32(1) - np.float32(0.2)), float(np.float32(1) + np.float32(0.2))
    rows = [-hi * 1.0] * 4 + [lo * 2.0] * 3                          # every scored row clipped: -surrogate = -hi A (A > 0), -lo A (A < 0)
    assert float(loss.detach()) == pytest.approx(sum(rows) / 7) and torch.allclose(call["row_scale"], torch.full((B, S), 1 / 7)) and loss.dim() == 0
    assert st.logprob.tolist() == [[-16.0, -15.0, -14.0, -13.0], [-26.0, -25.0, -24.0, 0.0]] and int(st.ignored[0]) == 1 and float(st.clip_frac[0]) == 1.0
    assert st.entropy is not None and st.flags.dtype == torch.uint8 and st.coef.tolist()[1] == [7.0, 7.0, 7.0, 0.0]
    (loss * 3).backward()                                           # the upstream gradient reaches every element
    want = torch.full((B, S, V), 3 / 7)
    want[1, 3] = 0.0
    assert torch.allclose(lg.grad, want)
    # the kl and entropy terms, [B, S] operands in row order, sum / none / seq_mean
    adv_bs = torch.tensor([[1.0, 0.0, -1.0, 1.0], [0.0, 0.0, 2.0, 5.0]])
    old_bs = torch.full((B, S), -1.0)
    lg = new()
    loss = losses.token_policy_loss(lg, ids, old_bs, adv_bs, ref_logprob=old_bs, kl_coef=0.5, ent_coef=0.25, clip=(0.1, 0.3), reduction="sum", ops=stub)
    call = stub.calls[-1]
    lo, hi = float(np.float32(1) - np.float32(0.1)), float(np.float32(1) + np.float32(0.3))
    per = lambda a: (-hi * a if a > 0 else -lo * a if a < 0 else 0.0) + 0.5 * 1.0 - 0.25 * 3.0
    rows = [per(a) for a in (1.0, 0.0, -1.0, 1.0, 0.0, 0.0, 2.0)]
    assert float(loss.detach()) == pytest.approx(sum(rows)) and call["row_scale"] is None and call["clip"] == (0.1, 0.3) and call["kl_coef"] == 0.5 and call["ent_coef"] == 0.25
    assert torch.equal(call["ref_logprob"], old_bs) and torch.equal(call["adv"], adv_bs) and call["want_entropy"]
    lg = new()
    loss = losses.token_policy_loss(lg, ids, old_bs, adv_bs, reduction="none", ops=stub)
    assert loss.shape == (B, S) and loss.tolist()[1] == pytest.approx([0.0, 0.0, -hi * 0 - float(np.float32(1.2)) * 2.0, 0.0]) and not stub.calls[-1]["want_entropy"]
    up = torch.arange(8.0).reshape(B, S)
    loss.backward(up)                                               # per-row upstream gradients
    assert torch.equal(lg.grad[..., 0], torch.where(torch.tensor([[True] * 4, [True] * 3 + [False]]), up, torch.zeros(())))
    loss = losses.token_policy_loss(new(), ids, old_bs, adv_bs, reduction="seq_mean", steps=[4, 2], ops=stub)       # rows past a sequence's count are ignored
    h2 = float(np.float32(1.2))
    assert float(loss.detach()) == pytest.approx(((-h2 * 1 + 0 + float(np.float32(0.8)) * 1 - h2 * 1) / 4 + 0.0 / 2) / 2)
    assert torch.allclose(stub.calls[-1]["row_scale"], torch.tensor([[1 / 8] * 4, [1 / 4] * 4])) and not stub.calls[-1]["reverse_steps"]
    loss = losses.token_policy_loss(new(), ids, old_bs, adv_bs, reduction="seq_mean", steps=[4, 0], ops=stub)       # a sequence without scored rows is not counted
    assert float(loss.detach()) == pytest.approx((-h2 * 1 + 0 + float(np.float32(0.8)) * 1 - h2 * 1) / 4)
    for red in ("mean", "seq_mean", "sum", "none"):                 # no scored row at all: loss 0 and finite row scales, not 0 / 0
        lg = new()
        loss = losses.token_policy_loss(lg, ids, old_bs, adv_bs, reduction=red, steps=[0, 0], ops=stub)
        assert float(loss.detach().abs().sum()) == 0.0 and (stub.calls[-1]["row_scale"] is None or bool(torch.isfinite(stub.calls[-1]["row_scale"]).all()))
        loss.sum().backward()
        assert float(lg.grad.abs().sum()) == 0.0
    # weights by TOKENIZER position: row s carries weights[K - 1 - s]
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    loss = losses.token_policy_loss(new(), ids, old_bs, adv_b, weights=w, ops=stub)
    wr = [6.0, 5.0, 4.0, 3.0]
    tot = sum(wr) + sum(wr[:3])
    assert float(loss.detach()) == pytest.approx((sum(wr) * -h2 + sum(wr[:3]) * float(np.float32(0.8)) * 2) / tot)
    assert torch.allclose(stub.calls[-1]["row_scale"], (torch.tensor(wr) / tot).expand(B, S))
    loss = losses.token_policy_loss(new(), ids, old_k, adv_b, ar_order=False, reduction="sum", weights=torch.ones(B, S), ops=stub)      # tokenizer order: row s meets position s
    assert not stub.calls[-1]["reverse_steps"] and stub.calls[-1]["old"].tolist() == [[0.0, 1.0, 2.0, 3.0], [6.0, 7.0, 8.0, 9.0]]
    # in place: the gradient IS the logits tensor; a second backward is refused, so is a double backward
    raw = torch.zeros(B, S, V, requires_grad=True)
    lg = raw * 1.0
    loss = losses.token_policy_loss(lg, ids, old_bs, adv_b, inplace=True, ops=stub)
    assert stub.calls[-1]["inplace"] and torch.allclose(lg.detach()[0, 0], torch.full((V,), 1 / 7))
    loss.backward(retain_graph=True)
    assert torch.allclose(raw.grad[0], torch.full((S, V), 1 / 7))
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    lg = new()
    loss = losses.token_policy_loss(lg, ids, old_bs, adv_b, ops=stub)
    (gr,) = torch.autograd.grad(loss, lg, create_graph=True)
    if gr.requires_grad:                                            # once_differentiable: differentiating a second time is an error
        with pytest.raises(RuntimeError):
            gr.sum().backward()
    for kw in (dict(reduction="max"), dict(clip=1.0), dict(clip=(0.2, float("inf"))), dict(kl_coef=0.1), dict(kl_coef=-1.0, ref_logprob=old_bs), dict(ent_coef=float("nan")),
               dict(weights=torch.ones(3)), dict(logprob_layout="columns")):
        with pytest.raises(ValueError):
            losses.token_policy_loss(new(), ids, old_bs, adv_b, ops=stub, **kw)
    for bad_old, bad_adv in ((torch.zeros(B, S + 1), adv_b), (old_bs, torch.zeros(B + 1)), (old_bs, torch.zeros(S))):
        with pytest.raises(ValueError):
            losses.token_policy_loss(new(), ids, bad_old, bad_adv, ops=stub)
    sq = torch.zeros(B, K, V, requires_grad=True)                   # S == K in AR order: [B, S] and [B, K] coincide and the orders differ
    with pytest.raises(ValueError, match="logprob_layout"):
        losses.token_policy_loss(sq, ids, old_k, adv_b, ops=stub)
    losses.token_policy_loss(sq, ids, old_k, adv_b, logprob_layout="tokens", ops=stub)
    assert stub.calls[-1]["old"].tolist()[0] == [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]
    losses.token_policy_loss(sq, ids, old_k, adv_b, logprob_layout="rows", ops=stub)
    assert stub.calls[-1]["old"].tolist()[0] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
    with pytest.raises(ValueError, match="S <= K"):
        losses.token_policy_loss(torch.zeros(B, K + 1, V), ids, old_bs, adv_b, ops=stub)


def test_group_advantages_match_numpy_fp64():
    rng = np.random.default_rng(38)
    r = rng.standard_normal(6 * 8) * 3 + 1
    r[8:16] = 2.5                                                   # a group whose rewards are all equal: advantage 0, not NaN
    got = losses.group_advantages(torch.from_numpy(r), 8)
    g = r.reshape(6, 8)
    want = ((g - g.mean(1, keepdims=True)) / (g.std(1, keepdims=True) + 1e-6)).reshape(-1)
    assert got.dtype == torch.float32 and got.shape == (48,) and np.array_equal(got.numpy(), want.astype(f32)) and (got[8:16] == 0).all()
    got = losses.group_advantages(torch.from_numpy(r.astype(f32)), 4, eps=1e-3, normalize_std=False)
    g = r.astype(f32).astype(f64).reshape(12, 4)
    assert np.array_equal(got.numpy(), (g - g.mean(1, keepdims=True)).reshape(-1).astype(f32))
    got = losses.group_advantages(torch.from_numpy(r), 6, eps=0.5)
    g = r.reshape(8, 6)
    assert np.allclose(got.numpy(), ((g - g.mean(1, keepdims=True)) / (g.std(1, keepdims=True) + 0.5)).reshape(-1), rtol=1e-6, atol=1e-7)
    assert losses.group_advantages(torch.tensor([3.0, 4.0]), 1).tolist() == [0.0, 0.0]
    for n in (5, 0, 7):
        with pytest.raises(ValueError):
            losses.group_advantages(torch.from_numpy(r), n)
    with pytest.raises(ValueError):
        losses.group_advantages(torch.zeros(2, 4), 4)
