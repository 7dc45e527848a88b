"""not gpu: the token loss pinned on the host -- the numpy emulation of tests/token_xent_cases.py against its brute-force second formulation, what the case
table claims, the planted mistakes and how far each moves a case, nll and Q_total against the SCORER's emulation bit for bit, nll, lse and the gradient against
torch fp64 autograd under a derived bound, the gradient rows' sums, the C entry against the ctypes table, the kernels' resource budget, the host-side refusals
and token_cross_entropy's bookkeeping over a stub of ops."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_sample_cases as TC
import token_score_cases as SC
import token_xent_cases as XC
from selftoktokenizer_amd import _lib, losses, ops, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "selftok_xent_rows"
f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64


def _values(c, grad):
    """a gradient buffer as fp32 values"""
    return TC.widen_bf16(grad) if c.dtype == "bf16" else grad


@pytest.mark.parametrize("name", [c.name for c in XC.CASES])
def test_emulation_equals_the_brute_force_formulation(name):
    c = XC.BY_NAME[name]
    a, b = XC.reference(name), XC.reference(name, brute=True)
    assert len(a.nll) == XC.rows_of(c) and XC.same(name, a, b), [r for r in XC.brute_rows(c) if XC.row_tuple(a, r) != XC.brute_tuple(b[r])][:3]
    good = ~a.bad
    sc = good & ~a.ignored
    assert (a.q_total[good] >= TC.ONE).all() and (a.q_total[good] < 1 << 49).all() and (a.nll[sc] >= 0).all() and np.isnan(a.nll[a.bad]).all() and np.isnan(a.lse[a.bad]).all()
    v = _values(c, a.grad)
    assert (v[:, c.V:] == XC.SENT).all() and (v[:, :c.offset] == 0).all() and (v[:, c.offset + c.C:c.V] == 0).all()       # pad columns untouched, the rest written
    assert (v[~sc, :c.V].view(u32) == 0).all() and (a.nll[a.ignored].view(u32) == 0).all() and np.isfinite(a.lse[good]).all()      # +0, bit for bit


def test_the_case_table_holds_what_it_claims():
    cs = XC.CASES
    assert {1, 2, 3, 4, 5} | set(XC.GEOMETRY_C) <= {c.C for c in cs} and {1, 3, 5, 64} | set(XC.GEOMETRY_R) <= {XC.rows_of(c) for c in cs}
    steps = {(c.S, XC.id_geometry(c)[3]) for c in cs}
    assert {s for s, _ in steps} >= {1, 3, 40} and {st for s, st in steps if s > 1} == {1, -1, 2, -2} and {(40, 1), (40, -1), (40, -2), (3, 2), (3, -2)} <= steps
    assert {c.ids for c in cs} == {"int32", "int64"} and {c.dtype for c in cs} == {"f32", "bf16"} and {0, XC.OFFSET_VLM} <= {c.offset for c in cs}
    assert any(c.row > c.V for c in cs) and any(c.V > c.offset + c.C for c in cs) and any((c.V - c.offset - c.C) % 4 for c in cs)
    assert {float(c.z) for c in cs} == {0.0, float(XC.Z_SMALL), float(XC.Z_BIG)} and {c.scale for c in cs} == {None, "const", "rows"}
    assert 0.0 in XC.ROW_SCALES and min(XC.ROW_SCALES) < 0
    assert {"four", "zeros", "dominant", "gauss1", "gauss8", "neginf", "gauss_neginf", "bad"} <= {c.kind for c in cs}
    for kernel_of in (lambda C: C <= XC.SMALL_C, lambda C: XC.SMALL_C < C <= XC.REG_C, lambda C: C > XC.REG_C):      # every kernel: both dtypes, z, bad, ignored rows
        mine = [c for c in cs if kernel_of(c.C)]
        assert {c.dtype for c in mine} == {"f32", "bf16"} and {c.z != 0 for c in mine} == {True, False} and {"badtargets", "ignored"} <= {c.tk for c in mine}
        assert any(c.offset == XC.OFFSET_VLM for c in mine) and any(c.scale == "rows" for c in mine)
    assert all(c.offset % 4 == 0 and c.row % 4 == 0 and c.offset + c.C <= c.V <= c.row for c in cs)
    for c in cs:
        d, ref = XC.make(c.name), XC.reference(c.name)
        l, t = XC.window(c.name), d["targets"]
        full = TC.widen_bf16(d["logits"]) if c.dtype == "bf16" else d["logits"]
        outside = np.ones(c.row, bool)
        outside[c.offset:c.offset + c.C] = False
        assert np.isnan(full[:, outside]).all() and np.array_equal(XC.gather_targets(c, d), t)        # NaN outside the window: it must make no row bad
        assert (d["ids"] == XC.POISON).sum() == d["ids"].size - XC.rows_of(c)
        key = TC.key_of(np.where(np.isnan(l), f32(-np.inf), l))
        if c.kind == "four":
            for r in range(XC.rows_of(c)):
                assert len(set(l[r].tolist())) == 4 and len(np.flatnonzero(l[r] == l[r, t[r]])) > 10
        if c.kind == "zeros":
            assert {bool(np.signbit(l[r, t[r]])) for r in range(6)} == {True, False} and len(set(ref.nll.tolist())) == 1
        if c.kind == "dominant":                                    # every other mass 0: p is a one-hot, the gradient a (onehot_max) - g (onehot_t)
            assert (ref.q_total == TC.ONE).all() and (ref.nll[0::2] == 0).all() and (ref.nll[1::2] == 30).all() and ((ref.p != 0).sum(1) == 1).all()
        if c.tk == "neginf":
            assert (ref.nll[0::2] == np.inf).all() and np.isfinite(ref.nll[1::2]).all() and not ref.bad.any() and np.isfinite(_values(c, ref.grad)[:, :c.V]).all()
        if c.tk == "neginf_one":
            assert (ref.nll[0::2] == 0).all() and (ref.nll[1::2] == np.inf).all() and (ref.q_total == TC.ONE).all()
        if c.tk == "ignored":
            assert ref.ignored.tolist() == [False, True, True] * (XC.rows_of(c) // 3) and set(t[ref.ignored].tolist()) == {-1, -100} and not ref.bad.any()
        if c.tk == "badtargets":
            assert ref.bad.tolist() == [False, True, True, True, False, True, False, True, False] and t[2] == c.C and t[7] == (2 ** 31 + 5 if c.ids == "int64" else c.C + 1)
        else:
            assert not ref.bad.any()
        if c.tk == "mix" and XC.rows_of(c) >= 3:                    # a target at the maximum, one at rank C - 1, the rest anywhere
            rank = lambda r: int((key[r] > key[r, t[r]]).sum() + ((key[r] == key[r, t[r]]) & (np.arange(c.C) < t[r])).sum())
            assert rank(2) == 0 and rank(1) == c.C - 1
        if c.kind in ("gauss1", "gauss8") and c.tk == "mix":        # gated gaussian cases: at least half the targets away from the maximum
            away = np.mean([l[r, t[r]] != l[r].max() for r in range(XC.rows_of(c))])
            assert away >= 0.5, (c.name, away)
        if c.kind == "gauss8":                                      # sigma 8: at least half the codes lie more than 24 below the maximum and have mass 0
            assert (ref.p == 0).mean() >= 0.5 and (ref.p[np.arange(len(t)), t] == 0).any()      # ... a target among them: q_t = 0, a finite nll
            assert np.isfinite(ref.nll).all()


MIN_MOVED = {"target_p_minus_1": 10, "z_without_2": 12, "lse_without_m": 30, "p_unnormalised": 30, "scale_on_p_only": 12, "target_without_offset": 5,
             "step_not_reversed": 5, "ignored_unwritten": 3, "outside_unwritten": 8, "bf16_truncated": 8, "tail_chunk_dropped": 15}


def _ulps_gate(x):
    return np.spacing(np.abs(np.asarray(x, f32)).astype(f32)).astype(f64)


def moved_by(name, mut):
    """the largest |change| a mistake makes to any output of a case, in units of that output's GATE in tests/test_token_xent_gpu.py: one fp32 ulp for nll and
    lse; for a gradient element the spread of the rows the GPU test accepts (the emulation with the factor of `a` one ulp either way, z_coef != 0 only) -- 0
    for most elements, where any change at all is infinitely many gates"""
    c = XC.BY_NAME[name]
    ref, got = XC.reference(name), XC.reference(name, mut=mut)
    worst = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for a, b in ((ref.nll, got.nll), (ref.lse, got.lse)):
            same = (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))
            r = np.where(same, 0.0, np.where(np.isfinite(a) & np.isfinite(b), np.abs(a.astype(f64) - b.astype(f64)) / _ulps_gate(a), np.inf))
            worst = max(worst, float(r.max()))
        va, vb = _values(c, ref.grad).astype(f64), _values(c, got.grad).astype(f64)
        gate = np.zeros_like(va)
        if c.z != 0:
            for u in (-1, 1):
                gate = np.maximum(gate, np.abs(_values(c, XC.reference(name, factor_ulps=u).grad).astype(f64) - va))
        diff = np.abs(va - vb)
        diff = np.where(np.isnan(diff), np.inf, diff)
        bits = ref.grad.view(np.uint16 if c.dtype == "bf16" else u32) == got.grad.view(np.uint16 if c.dtype == "bf16" else u32)     # -0 for +0 is a change
        r = np.where(bits, 0.0, np.where(gate == 0, np.inf, diff / np.where(gate == 0, 1.0, gate)))
        worst = max(worst, float(r.max()))
    return worst


@pytest.mark.parametrize("mut", XC.MUTS)
def test_each_planted_mistake_changes_exactly_the_cases_it_names(mut):
    """the emulation with a mistake planted moves a case if and only if `applies` -- the brute-force formulation with the same mistake written a second time --
    says so, only where `needs` allows it, and then by at least 1000 gates of the GPU comparison"""
    moved = 0
    for c in XC.CASES:
        got = not XC.same(c.name, XC.reference(c.name), XC.reference(c.name, mut=mut))
        assert got == XC.applies(mut, c.name), (mut, c.name)
        assert not got or XC.needs(mut, c), (mut, c.name)
        if got:
            assert moved_by(c.name, mut) >= 1000.0, (mut, c.name, moved_by(c.name, mut))
        moved += got
    assert moved >= MIN_MOVED[mut], (mut, moved)
    assert len(XC.MUTS) >= 10 and set(MIN_MOVED) == set(XC.MUTS)


@pytest.mark.parametrize("name", [c.name for c in XC.CASES])
def test_nll_is_the_scorers_logprob_with_the_sign_turned(name):
    """nll bits = the scorer's emulated logprob bits with the sign bit turned, and one Q_total: on every case of this table (nll and Q_total do not see z_coef)"""
    c, d = XC.BY_NAME[name], XC.make(name)
    mine = XC.reference(name)
    theirs = SC.score_rows(XC.window(name), None, d["targets"])
    assert np.array_equal(mine.bad, theirs.bad) and np.array_equal(mine.ignored, theirs.ignored) and np.array_equal(mine.q_total, theirs.q_total)
    sc = ~mine.bad & ~mine.ignored
    assert np.array_equal(mine.nll[sc].view(u32), theirs.logprob[sc].view(u32) ^ u32(0x80000000))
    if c.z == 0:
        assert np.array_equal(mine.a[sc], np.ones(sc.sum(), f32) if d["scale"] is None else d["scale"][sc])       # z_coef 0: the factor is exactly 1


@pytest.mark.parametrize("name", [c.name for c in SC.CASES if c.T == 1.0 and not c.guided and SC.rows_of(c) <= 64])
def test_the_scorers_own_table_at_temperature_one(name):
    lc, _ = SC.windows(name)
    theirs = SC.reference(name)
    mine = XC.xent_rows(lc, SC.make(name)["targets"])
    assert np.array_equal(mine.bad, theirs.bad) and np.array_equal(mine.ignored, theirs.ignored) and np.array_equal(mine.q_total, theirs.q_total)
    sc = ~mine.bad & ~mine.ignored
    assert np.array_equal(mine.nll[sc].view(u32), theirs.logprob[sc].view(u32) ^ u32(0x80000000)) and sc.any() == (~theirs.bad & ~theirs.ignored).any()


def test_nll_lse_and_gradient_against_fp64_autograd_within_the_derived_bound():
    """F.cross_entropy(reduction="none") + z logsumexp^2, scaled by g, and autograd, in fp64 on the same fp32 values; the bound is derived, not
    measured: the largest share of it that any case reaches is printed and written to profiles/token_xent_bound.txt.  With z_coef = 0 every scored fp32
    gradient row sums, in fp64, to within the sum of its elements' bounds of 0."""
    worst = {"nll": (0.0, ""), "lse": (0.0, ""), "grad": (0.0, ""), "rowsum": (0.0, "")}
    rows = 0
    for c in XC.CASES:
        if XC.rows_of(c) > 64:
            continue
        ref, d, l = XC.reference(c.name), XC.make(c.name), XC.window(c.name)
        t, z = d["targets"], float(c.z)
        v = _values(c, ref.grad)[:, c.offset:c.offset + c.C].astype(f64)
        for r in np.flatnonzero(~ref.bad):
            x = torch.from_numpy(l[r].astype(f64)).requires_grad_(True)
            L = torch.logsumexp(x, 0)
            Lf = float(L.detach())
            e, b = abs(float(ref.lse[r]) - Lf), XC.bound_row_scalar(c.C, Lf)
            assert e <= b, (c.name, r, "lse", e, b)
            worst["lse"] = max(worst["lse"], (e / b, c.name))
            if ref.ignored[r] or not np.isfinite(ref.nll[r]):
                continue
            g = 1.0 if d["scale"] is None else float(d["scale"][r])
            ce = F.cross_entropy(x.unsqueeze(0), torch.tensor([int(t[r])]), reduction="none")[0]
            (g * (ce + z * L * L)).backward()
            e, b = abs(float(ref.nll[r]) - float(ce.detach())), XC.bound_row_scalar(c.C, float(ce.detach()))
            assert e <= b, (c.name, r, "nll", e, b)
            worst["nll"] = max(worst["nll"], (e / b, c.name))
            p = torch.softmax(x.detach(), 0).numpy()
            onehot = np.zeros(c.C)
            onehot[t[r]] = 1.0
            bg = XC.bound_grad(c.C, p, g * (1 + 2 * z * Lf), g, z, Lf, onehot, bf16=c.dtype == "bf16")
            eg = np.abs(v[r] - x.grad.numpy())
            assert (eg <= bg).all(), (c.name, r, "grad", float((eg / bg).max()))
            worst["grad"] = max(worst["grad"], (float((eg / bg).max()), c.name))
            if z == 0 and c.dtype == "f32" and g != 0:
                s = abs(float(v[r].sum())) / float(bg.sum())
                assert s <= 1.0, (c.name, r, "row sum", s)
                worst["rowsum"] = max(worst["rowsum"], (s, c.name))
            rows += 1
    text = "token loss against torch fp64 autograd (tests/test_token_xent_cpu.py, DESIGN 35.4): %d scored rows; largest share of the derived bound -- " % rows + \
           ", ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in worst.items())
    print("\n" + text)
    try:
        with open(os.path.join(ROOT, "profiles", "token_xent_bound.txt"), "w") as f:
            f.write(text + "\n")
    except OSError:
        pass
    assert rows >= 100 and all(v[0] > 0 for v in worst.values())


def test_ext_header_declares_the_entry_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "float": C.c_float, "unsigned": C.c_uint}
    m = re.search(r"(\w+)\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and ENTRY in _lib.EXT_SIGNATURES and ENTRY not in _lib.SIGNATURES and not ENTRY.startswith("selftok_token_")
    args = [a.strip() for a in m.group(2).split(",")]
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
    res, got = _lib.EXT_SIGNATURES[ENTRY]
    assert got == want and res == ctype_of[m.group(1)] and len(got) == 21, args
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_xent_rows.argtypes == got


def test_token_xent_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 6 kernels (2 chunks / 16 chunks in registers / streamed, fp32 / bf16).  16 chunks: 90 VGPRs, 5 waves per SIMD -- two
    512-thread workgroups per compute unit; 2 chunks: 30 - 34 VGPRs, streamed: 31 - 32 VGPRs, 8 waves per SIMD; 32 bytes of LDS each."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_xent.o")
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 6 and all("tok_xent_kernel" in k for k in kernels), kernels
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 128 and l <= 64 and o >= 4 for v, l, o in zip(vgprs, lds, occ)), (vgprs, lds, occ)
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(G.CSRC, "token_xent.hip")).read().splitlines())
    assert "asm" not in code and "expf" not in code and "fma" not in code and "hipMalloc" not in code and "atomicAdd(float" not in code


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(8192, 0x5A5A5A5A, u32)
    p = x.ctypes.data
    assert p % 16 == 0
    q = p + 4096 * 4                                                # a second buffer, disjoint from a 2-row x 128-code fp32 call's extents

    def call(logits=p, dtype=0, R=2, C=100, rs=128, off=0, ids=p, ib=8, S=1, seq=1, step=1, V=None, scale=None, z=0.0, nll=p, lse=p, grad=q, gs=128, bad=p, ign=p):
        return lib.selftok_xent_rows(logits, dtype, R, C, rs, off, ids, ib, S, seq, step, off + C if V is None else V, scale, z, nll, lse, grad, gs, bad, ign, None)

    for z in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert call(z=z) == -1 and "z_coef" in err(), z
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
    for kw in (dict(logits=None), dict(ids=None), dict(nll=None), dict(lse=None), dict(grad=None), dict(bad=None), dict(ign=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(logits=p + 4), dict(logits=p + 8), dict(grad=q + 4), dict(grad=q + 8), dict(off=2, rs=132, gs=132), dict(rs=130), dict(gs=130), dict(dtype=1, logits=p + 2),
               dict(dtype=1, grad=q + 4)):
        assert call(**kw) == -1 and "misaligned" in err(), kw
    for kw in (dict(ids=p + 4), dict(ib=4, ids=p + 2), dict(nll=p + 2), dict(lse=p + 1), dict(scale=p + 2), dict(bad=p + 2), dict(ign=p + 2)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(C=100, rs=96), dict(C=100, off=32, rs=128), dict(off=-4), dict(rs=-1), dict(R=-1), dict(off=256, rs=128)):
        assert call(**kw) == -1 and "window" in err(), kw
    assert call(R=0, logits=None, ids=None, nll=None, lse=None, grad=None, bad=None, ign=None) == 0       # no rows: nothing launched
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves its outputs untouched
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_xent(torch.zeros(2, 128), torch.zeros(2, dtype=torch.int64))


class _StubOps:
    """records every call and plays the kernels' part on the host: nll = target + 1, lse = 2, the gradient row filled with the row's scale (1 without one);
    rows with a negative target ignored: nll 0, a zero row"""

    def __init__(self):
        self.calls = []

    def _record(self, ids, kw, reverse_steps):
        self.calls.append(dict(kw, reverse_steps=reverse_steps, ids_shape=tuple(ids.shape), ids_stride=tuple(ids.stride()), ids_offset=ids.storage_offset()))
        return (ids.flip(1) if reverse_steps else ids).to(torch.int64)

    def token_xent(self, logits, ids, *, reverse_steps=False, **kw):
        B, S, V = logits.shape
        t = self._record(ids, kw, reverse_steps)
        ign = t < 0
        nll = torch.where(ign, torch.zeros(()), t.float() + 1)
        g = torch.ones(B, S) if kw["row_scale"] is None else kw["row_scale"].reshape(B, S)
        grad = logits if kw["inplace"] else torch.empty_like(logits)
        grad.copy_(torch.where(ign, torch.zeros(()), g).unsqueeze(-1).expand(B, S, V))
        return nll, torch.full((B, S), 2.0), grad, torch.zeros(1, dtype=torch.int32), torch.tensor([int(ign.sum())], dtype=torch.int32)

    def token_score(self, logits, ids, *, reverse_steps=False, **kw):
        B, S, _ = logits.shape
        self._record(ids, kw, reverse_steps)
        z = torch.zeros(B, S)
        return z, torch.zeros(B, S, 2, dtype=torch.int64), z.int(), z.int(), z, torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)


def test_token_cross_entropy_bookkeeping_over_an_ops_stub():
    B, K, S, V = 2, 6, 4, 16
    ids = torch.tensor([[10, 11, 12, 13, 14, 15], [20, 21, -1, 23, 24, 25]])
    new = lambda: torch.zeros(B, S, V, requires_grad=True)
    stub = _StubOps()
    lg = new()
    loss, st = losses.token_cross_entropy(lg, ids, C=8, offset=4, ops=stub, return_stats=True)
    call = stub.calls[0]
    # AR step s meets position K - 1 - s: row 0 gets ids 15, 14, 13, 12; row 1 gets 25, 24, 23, -1 (ignored): the view and direction of score_tokens
    sampling.score_tokens(lg.detach(), ids, C=8, offset=4, ops=stub)
    for k in ("reverse_steps", "ids_shape", "ids_stride", "ids_offset", "C", "offset"):
        assert call[k] == stub.calls[1][k], k
    assert call["reverse_steps"] and call["ids_offset"] == K - S and call["ids_stride"] == (K, 1) and (call["C"], call["offset"], call["z_coef"], call["inplace"]) == (8, 4, 0.0, False)
    nll = [16.0, 15.0, 14.0, 13.0, 26.0, 25.0, 24.0]
    assert st.nll.tolist() == [nll[:4], nll[4:] + [0.0]] and int(st.ignored[0]) == 1 and loss.dtype == torch.float32 and loss.dim() == 0
    assert float(loss.detach()) == pytest.approx(sum(nll) / 7) and torch.allclose(call["row_scale"], torch.full((B, S), 1 / 7))
    (loss * 3).backward()                                           # the upstream gradient reaches every element
    want = torch.full((B, S, V), 3 / 7)
    want[1, 3] = 0.0
    assert torch.allclose(lg.grad, want)
    # sum and none, the z term, an ignored row's lse kept out
    lg = new()
    loss = losses.token_cross_entropy(lg, ids, reduction="sum", z_loss=0.5, ops=stub)
    assert float(loss.detach()) == pytest.approx(sum(nll) + 7 * 0.5 * 4.0) and stub.calls[-1]["row_scale"] is None and stub.calls[-1]["z_coef"] == 0.5
    lg = new()
    loss = losses.token_cross_entropy(lg, ids, reduction="none", z_loss=0.5, ops=stub)
    assert loss.shape == (B, S) and loss.tolist() == [[18.0, 17.0, 16.0, 15.0], [28.0, 27.0, 26.0, 0.0]]
    up = torch.arange(8.0).reshape(B, S)
    loss.backward(up)                                               # per-row upstream gradients
    assert torch.equal(lg.grad[..., 0], torch.where(torch.tensor([[True] * 4, [True] * 3 + [False]]), up, torch.zeros(())))
    # weights by TOKENIZER position: row s carries weights[K - 1 - s]
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    lg = new()
    loss = losses.token_cross_entropy(lg, ids, weights=w, ops=stub)
    wr = [6.0, 5.0, 4.0, 3.0]
    tot = sum(wr) + sum(wr[:3])
    assert float(loss.detach()) == pytest.approx((sum(a * b for a, b in zip(wr, nll[:4])) + sum(a * b for a, b in zip(wr, nll[4:]))) / tot)
    assert torch.allclose(stub.calls[-1]["row_scale"], (torch.tensor(wr) / tot).expand(B, S))
    loss = losses.token_cross_entropy(new(), ids, weights=w, ar_order=False, reduction="sum", ops=stub)      # tokenizer order: row s meets position s
    assert not stub.calls[-1]["reverse_steps"] and stub.calls[-1]["ids_offset"] == 0 and torch.equal(stub.calls[-1]["row_scale"], w[:S].expand(B, S))
    assert float(loss.detach()) == pytest.approx(1 * 11 + 2 * 12 + 3 * 13 + 4 * 14 + 1 * 21 + 2 * 22 + 4 * 24)
    wb = torch.tensor([[1.0, 0.0, 2.0, 1.0], [1.0, 1.0, 1.0, 5.0]])                                            # [B, S]: by row of the logits
    loss = losses.token_cross_entropy(new(), ids, weights=wb, ops=stub)
    assert float(loss.detach()) == pytest.approx((16 + 2 * 14 + 13 + 26 + 25 + 24) / 7.0)
    # a step count per sequence: the rows past it are ignored, and the mean counts the rest
    loss, st = losses.token_cross_entropy(new(), ids, steps=[4, 2], ops=stub, return_stats=True)
    assert st.nll.tolist() == [[16.0, 15.0, 14.0, 13.0], [26.0, 25.0, 0.0, 0.0]] and int(st.ignored[0]) == 2 and float(loss.detach()) == pytest.approx((58 + 51) / 6)
    assert not stub.calls[-1]["reverse_steps"] and torch.allclose(stub.calls[-1]["row_scale"], torch.full((B, S), 1 / 6))
    # in place: the gradient IS the logits tensor; a second backward is refused, so is a double backward
    raw = torch.zeros(B, S, V, requires_grad=True)
    lg = raw * 1.0
    loss = losses.token_cross_entropy(lg, ids, inplace=True, ops=stub)
    assert stub.calls[-1]["inplace"] and torch.allclose(lg.detach()[0, 0], torch.full((V,), 1 / 7))
    loss.backward(retain_graph=True)
    assert torch.allclose(raw.grad[0], torch.full((S, V), 1 / 7))
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    lg = new()
    loss = losses.token_cross_entropy(lg, ids, ops=stub)
    (gr,) = torch.autograd.grad(loss, lg, create_graph=True)
    if gr.requires_grad:                                            # once_differentiable: differentiating a second time is an error
        with pytest.raises(RuntimeError):
            gr.sum().backward()
    for kw in (dict(reduction="max"), dict(z_loss=-1.0), dict(weights=torch.ones(3))):
        with pytest.raises(ValueError):
            losses.token_cross_entropy(new(), ids, ops=stub, **kw)
    with pytest.raises(ValueError, match="S <= K"):
        losses.token_cross_entropy(torch.zeros(B, K + 1, V), ids, ops=stub)
