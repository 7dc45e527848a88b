"""not gpu: the token distillation pinned on the host -- the numpy emulation of tests/token_distill_cases.py against its brute-force second formulation, what
the case table claims, the planted mistakes and how far each moves a case, the teacher's entropy against the SCORER's emulation and the one-hot-teacher
gradient against the LOSS's emulation bit for bit, all four outputs and the gradient against torch fp64 (kl_div + autograd) under derived bounds, the C entry
against the ctypes table, the kernels' resource budget, the host-side refusals and token_distillation's bookkeeping over a stub of ops."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_distill_cases as DC
import token_sample_cases as TC
import token_score_cases as SC
import token_xent_cases as XC
from selftoktokenizer_amd import _lib, losses, ops, sampling

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "selftok_distill_rows"
f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64
OUTPUTS = ("kl", "ce", "h", "lse")


def _values(c, grad):
    """a gradient buffer as fp32 values"""
    return TC.widen_bf16(grad) if c.sd == "bf16" else grad


@pytest.mark.parametrize("name", [c.name for c in DC.CASES])
def test_emulation_equals_the_brute_force_formulation(name):
    c = DC.BY_NAME[name]
    a, b = DC.reference(name), DC.reference(name, brute=True)
    assert len(a.kl) == c.R and DC.same(name, a, b), [r for r in DC.brute_rows(c) if DC.row_tuple(a, r) != DC.brute_tuple(b[r])][:3]
    good = ~a.bad & ~a.ignored
    for k in OUTPUTS:
        o = getattr(a, k)
        assert np.isnan(o[a.bad]).all() and (o[a.ignored].view(u32) == 0).all() and not np.isnan(o[good]).any(), k      # NaN on bad rows, +0.0 on ignored ones
    assert all(TC.ONE <= int(q) < 1 << 49 for q in list(a.qa[good]) + list(a.qb[good])) and all(int(v) < 1 << 48 for v in list(a.slo[good]) + list(a.shi[good]))
    assert np.isinf(a.kl[a.overflow]).all() and np.isinf(a.ce[a.overflow]).all() and np.isfinite(a.h[good]).all() and np.isfinite(a.lse[good]).all()
    v = _values(c, a.grad)
    assert (v[:, c.V:] == DC.SENT).all() and (v[:, :c.offset].view(u32) == 0).all() and (v[:, c.offset + c.C:c.V].view(u32) == 0).all()     # pad columns untouched
    assert (v[~good, :c.V].view(u32) == 0).all() and np.isfinite(v[good, :c.V]).all()                 # +0, bit for bit; an overflow row's gradient is finite


def test_the_case_table_holds_what_it_claims():
    cs = DC.CASES
    assert {1, 2, 3, 4, 5} | set(DC.GEOMETRY_C) | {DC.SMALL_C, DC.REG_C} <= {c.C for c in cs} and {1, 3, 5, 64} | set(DC.GEOMETRY_R) <= {c.R for c in cs}
    assert {(c.sd, c.td) for c in cs} == {("f32", "f32"), ("f32", "bf16"), ("bf16", "f32"), ("bf16", "bf16")} and {0, DC.OFFSET_VLM} <= {c.offset for c in cs}
    assert any(c.row != c.trow for c in cs) and any(c.row > c.V for c in cs) and any((c.V - c.offset - c.C) % 4 for c in cs)
    assert {None if c.s is None else float(c.s) for c in cs} == {None, 0.0, 1.0, 3.0} and {c.scale for c in cs} == {None, "const", "rows"}
    assert 0.0 in DC.ROW_SCALES and min(DC.ROW_SCALES) < 0
    assert {"four", "zeros", "gauss1", "gauss8", "same", "onehot", "sneginf", "sneginf0", "under", "over", "bad"} <= {c.kind for c in cs}
    for kernel_of in (lambda C: C <= DC.SMALL_C, lambda C: DC.SMALL_C < C <= DC.REG_C, lambda C: C > DC.REG_C):      # every kernel: dtypes, guidance, bad, ignored rows
        mine = [c for c in cs if kernel_of(c.C)]
        assert {c.sd for c in mine} == {"f32", "bf16"} == {c.td for c in mine} and {c.s is None for c in mine} == {True, False}
        assert {"bad", "same"} <= {c.kind for c in mine} and any(c.mask for c in mine) and any(c.scale == "rows" for c in mine)
        assert {c.s is None for c in mine if c.kind == "bad"} == {True, False} and any(c.C % 4 for c in mine) and any(c.offset == DC.OFFSET_VLM for c in mine)
    assert all(c.offset % 4 == 0 and c.row % 4 == 0 and c.trow % 4 == 0 and c.offset + c.C <= c.V <= c.row and c.offset + c.C <= c.trow for c in cs)
    for c in cs:
        d, ref = DC.make(c.name), DC.reference(c.name)
        lc, lu, b = DC.windows(c.name)
        for arr, dt, rowlen in ((d["student"], c.sd, c.row), (d["teacher"], c.td, c.trow), (d["uncond"], c.td, c.trow)):
            if arr is not None:
                full = TC.widen_bf16(arr) if dt == "bf16" else arr
                outside = np.ones(rowlen, bool)
                outside[c.offset:c.offset + c.C] = False
                assert np.isnan(full[:, outside]).all()             # NaN outside the window: it must make no row bad
        if c.kind != "same":                                        # the student on its grid: b - mB is exact in fp32
            fin = b[np.isfinite(b)]
            assert (fin * f32(DC.GRID) == np.rint(fin * f32(DC.GRID))).all() and (np.abs(fin) < 2.0 ** 13).all() or c.kind in ("under", "over")
        if c.mask:
            ign = np.arange(c.R) % 3 == 1
            assert np.array_equal(ref.ignored, ign) and np.isnan(b[ign]).all() and np.isnan(lc[ign]).all() and not ref.bad.any()
        if c.kind == "bad":
            assert ref.bad.tolist() == [False, True, c.s is not None, True, False, True, False, True, False]
        else:
            assert not ref.bad.any()
        if c.kind == "same":
            assert np.array_equal(lc.view(u32), b.view(u32)) and (np.abs(ref.kl) < 1e-6).all() and (ref.kl != 0).any()
            assert (_values(c, ref.grad)[:, c.offset:c.offset + c.C] == 0).all()
        if c.kind == "onehot":
            assert all(int(q) == TC.ONE for q in ref.qa) and ((ref.pa != 0).sum(1) == 1).all() and (ref.h == 0).all()
        if c.kind == "sneginf":
            assert ref.overflow.all() and np.isfinite(_values(c, ref.grad)[:, :c.V]).all()
        if c.kind == "sneginf0":
            assert not ref.overflow.any() and np.isinf(b).any() and np.isfinite(ref.kl).all()
        if c.kind == "under":
            assert not ref.overflow.any() and all(int(v) > 1 << 30 for v in ref.shi) and (ref.kl > 600).all()
        if c.kind == "over":
            assert ref.overflow.all() and (b == f32(-32768.0)).any()
        if c.kind == "zeros":
            assert {bool(np.signbit(v)) for v in b[b == 0]} == {True, False} and len({ref.lse.tobytes()}) == 1 and len(set(ref.lse.tolist())) == 1
        if c.kind == "four":
            assert all(len(set(b[r].tolist())) == 4 and len(set(lc[r].tolist())) == 4 for r in range(c.R))
        if c.kind == "gauss8":                                      # sigma 8: most codes lie more than 24 below the maximum and have mass 0
            assert (ref.pa == 0).mean() >= 0.5 and (ref.pb == 0).mean() >= 0.5
        if c.kind in ("gauss1", "gauss8", "four", "under"):
            assert all(int(v) > 0 for v in ref.shi[~ref.ignored])  # the high limb carries weight nearly everywhere


MIN_MOVED = {"pa_minus_pb": 30, "x_from_d32": 3, "cross_over_zero_mass": 2, "ex_over_qb": 30, "la_lb_swapped": 30, "guidance_from_cond": 12, "scale_before_diff": 12,
             "ignored_unwritten": 6, "outside_unwritten": 8, "bf16_truncated": 10, "tail_chunk_dropped": 15, "s_hi_dropped": 35}


def moved_by(name, mut):
    """the largest |change| a mistake makes to any output of a case, in units of that output's GATE in tests/test_token_distill_gpu.py: one fp32 ulp for the
    four row outputs; none at all for a gradient element, where any changed bit is infinitely many gates"""
    c = DC.BY_NAME[name]
    ref, got = DC.reference(name), DC.reference(name, mut=mut)
    worst = 0.0
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for k in OUTPUTS:
            a, b = getattr(ref, k), getattr(got, k)
            same = (a.view(u32) == b.view(u32)) | (np.isnan(a) & np.isnan(b))
            gate = np.spacing(np.abs(a).astype(f32)).astype(f64)
            r = np.where(same, 0.0, np.where(np.isfinite(a) & np.isfinite(b), np.abs(a.astype(f64) - b.astype(f64)) / gate, np.inf))
            worst = max(worst, float(r.max()))
    if ref.grad.tobytes() != got.grad.tobytes():
        worst = math.inf
    return worst


@pytest.mark.parametrize("mut", DC.MUTS)
def test_each_planted_mistake_changes_exactly_the_cases_it_names(mut):
    """the emulation with a mistake planted moves what a caller sees of a case if and only if `applies` -- the brute-force formulation with the same mistake
    written a second time -- says so, only where `needs` allows it, and then by at least 1000 gates of the GPU comparison"""
    moved = 0
    for c in DC.CASES:
        got = not DC.same(c.name, DC.reference(c.name), DC.reference(c.name, mut=mut), sums=False)
        assert got == DC.applies(mut, c.name), (mut, c.name)
        assert DC.same(c.name, DC.reference(c.name, mut=mut), DC.reference(c.name, mut=mut, brute=True)), (mut, c.name)       # the two mistaken formulations agree too
        assert not got or DC.needs(mut, c), (mut, c.name)
        if got:
            assert moved_by(c.name, mut) >= 1000.0, (mut, c.name, moved_by(c.name, mut))
        moved += got
    assert moved >= MIN_MOVED[mut], (mut, moved)
    assert len(DC.MUTS) >= 12 and set(MIN_MOVED) == set(DC.MUTS)


@pytest.mark.parametrize("name", [c.name for c in DC.CASES if c.R <= 64])
def test_teacher_entropy_is_the_scorers_entropy(name):
    """h_teacher bits = the scorer's emulated entropy bits of the teacher row, guided rows included (and one Q_total, one S_h)"""
    c = DC.BY_NAME[name]
    lc, lu, _ = DC.windows(name)
    mine = DC.reference(name)
    rows = np.flatnonzero(~mine.bad & ~mine.ignored)
    theirs = SC.score_rows(lc[rows], None if lu is None else lu[rows], np.zeros(rows.size, np.int64), s=1.0 if c.s is None else float(c.s))
    assert not theirs.bad.any() and np.array_equal(theirs.entropy.view(u32), mine.h[rows].view(u32)), name
    assert [int(v) for v in theirs.q_total] == [int(v) for v in mine.qa[rows]] and [int(v) for v in theirs.s_h] == [int(v) for v in mine.sa[rows]]


@pytest.mark.parametrize("name", ["onehot", "onehot_reg_bf16"])
def test_one_hot_teacher_gives_the_losses_gradient_and_nll(name):
    """a teacher with one finite code is a hard label: without a row scale the gradient row is the loss's emulated gradient bit for bit, lse its lse, and ce
    is within one fp32 ulp of its nll (one is LB + X / (65536 QA), the other -((l_t - m) - LB))"""
    c = DC.BY_NAME[name]
    lc, _, b = DC.windows(name)
    t = np.argmax(lc, axis=1).astype(np.int64)
    mine = DC.distill_rows(lc, None, b, V=c.V, offset=c.offset, row=c.row, bf16=c.sd == "bf16")
    theirs = XC.xent_rows(b, t, V=c.V, offset=c.offset, row=c.row, bf16=c.sd == "bf16")
    assert mine.grad.tobytes() == theirs.grad.tobytes() and mine.lse.tobytes() == theirs.lse.tobytes() and not mine.bad.any()
    apart = np.abs(mine.ce.view(np.int32).astype(np.int64) - theirs.nll.view(np.int32).astype(np.int64))
    assert (apart <= 1).all() and (mine.kl.view(u32) == mine.ce.view(u32)).all()        # LA = 0 and E_A = 0: kl is ce


def _fp64_row(a32, b32, g):
    """torch fp64 on the same fp32 values: kl_div + autograd where the student is finite, the same sums over p > 0 otherwise -> dict of Python floats and arrays"""
    s = torch.from_numpy(b32.astype(f64)).requires_grad_(True)
    t = torch.from_numpy(a32.astype(f64))
    logq, p = torch.log_softmax(s, 0), torch.softmax(t, 0)
    on = p > 0
    zero = torch.zeros((), dtype=torch.float64)
    if bool(torch.isfinite(s).all()):
        kl = F.kl_div(logq, p, reduction="none").sum()
    else:
        kl = torch.where(on, p * (torch.log(torch.where(on, p, zero + 1)) - logq), zero).sum()
    ce = -torch.where(on, p * logq, zero).sum()
    h = -torch.where(on, p * torch.log(torch.where(on, p, zero + 1)), zero).sum()
    q = torch.softmax(s.detach(), 0)
    grad = g * (q - p)
    if bool(torch.isfinite(kl)):
        (g * kl).backward()
        assert torch.allclose(s.grad, grad, rtol=1e-9, atol=1e-15)
        grad = s.grad
    x = (s.detach().max() - s.detach())
    y = (t.max() - t)
    far = y > 22.0                                                  # codes whose mass the kernel may have dropped (it drops below 32 ln 2 = 22.18)
    px, py = torch.where(on, p * x, zero), torch.where(on, p * y, zero)
    near = on & (y < 22.5)                                          # codes the kernel gives mass for certain lie inside y <= 22; between 22 and 22.5 either may be
    return dict(kl=float(kl.detach()), ce=float(ce.detach()), h=float(h), lse=float(torch.logsumexp(s.detach(), 0)), grad=grad.numpy(), p=p.numpy(), q=q.numpy(),
                EX=float(px[~far].sum()), EA=float(py.sum()), tail_x=float(px[far].sum()), tail_a=float(py[far].sum()), x_max=float(x[on & ~far].max()),
                x_max_near=float(x[near].max()))


def test_outputs_and_gradient_against_fp64_within_the_derived_bounds():
    """the bounds are derived, not measured: the largest share of each that any case reaches is printed and written to
    profiles/token_distill_bound.txt.  A row the kernel reports as overflowing must have a weighted code 32768 or more below the student's maximum."""
    worst = {k: (0.0, "") for k in ("kl", "ce", "h", "lse", "grad")}
    rows = over = dropped = 0
    for c in DC.CASES:
        if c.R > 64:
            continue
        ref, d = DC.reference(c.name), DC.make(c.name)
        lc, lu, b = DC.windows(c.name)
        a = DC.guided(lc, lu, c.s)
        v = _values(c, ref.grad)[:, c.offset:c.offset + c.C].astype(f64)
        for r in np.flatnonzero(~ref.bad & ~ref.ignored):
            g = 1.0 if d["scale"] is None else float(d["scale"][r])
            w = _fp64_row(a[r], b[r], g)
            got = {k: float(getattr(ref, k)[r]) for k in DC.Out._fields[:4]}
            bounds = {"lse": DC.bound_lse(c.C, w["lse"]), "h": DC.bound_h(c.C, w["h"], w["EA"], w["tail_a"])}
            if ref.overflow[r]:
                assert w["x_max"] >= DC.X_LIMIT and got["kl"] == math.inf and got["ce"] == math.inf, (c.name, r)
                over += 1
            elif not math.isfinite(w["tail_x"]):                   # the student at -inf (or 32768 below) only where the teacher's mass is below e^-22: the
                assert w["x_max_near"] < DC.X_LIMIT and math.isfinite(got["kl"]) and w["kl"] == math.inf, (c.name, r)      # kernel drops that mass, fp64 does not
                dropped += 1
            else:
                assert w["x_max_near"] < DC.X_LIMIT and math.isfinite(w["kl"]), (c.name, r)
                bounds["ce"] = DC.bound_ce(c.C, w["ce"], w["EX"], w["tail_x"])
                bounds["kl"] = DC.bound_kl(c.C, w["kl"], w["EX"], w["EA"], w["tail_x"], w["tail_a"])
            for k, bd in bounds.items():
                e = abs(got[k] - w[k])
                assert e <= bd, (c.name, r, k, e, bd)
                worst[k] = max(worst[k], (e / bd, c.name))
            bg = DC.bound_grad(c.C, w["p"], w["q"], g, bf16=c.sd == "bf16")
            eg = np.abs(v[r] - w["grad"])
            assert (eg <= bg).all(), (c.name, r, "grad", float((eg / bg).max()))
            worst["grad"] = max(worst["grad"], (float((eg / bg).max()), c.name))
            rows += 1
    text = "token distillation against torch fp64 kl_div + autograd (tests/test_token_distill_cpu.py, DESIGN 36.4): %d rows, %d of them overflow rows, %d rows where fp64 is infinite through teacher mass "\
           "below e^-22 alone; largest share of the derived bound -- " % (rows, over, dropped) + ", ".join("%s %.3f (%s)" % (k, v[0], v[1]) for k, v in worst.items())
    print("\n" + text)
    try:
        with open(os.path.join(ROOT, "profiles", "token_distill_bound.txt"), "w") as f:
            f.write(text + "\n")
    except OSError:
        pass
    assert rows >= 150 and over >= 6 and dropped >= 2 and all(v[0] > 0 for v in worst.values())


def test_ext_header_declares_the_entry_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "float": C.c_float, "unsigned": C.c_uint}
    m = re.search(r"(\w+)\s+" + ENTRY + r"\s*\(([^)]*)\)\s*;", hdr)
    assert m and ENTRY in _lib.EXT_SIGNATURES and ENTRY not in _lib.SIGNATURES and not ENTRY.startswith("selftok_token_")
    args = [a.strip() for a in m.group(2).split(",")]
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
    res, got = _lib.EXT_SIGNATURES[ENTRY]
    assert got == want and res == ctype_of[m.group(1)] and len(got) == 23, args
    assert hasattr(C.CDLL(_lib.LIB_PATH), ENTRY), f"{ENTRY} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_distill_rows.argtypes == got


def test_token_distill_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 24 kernels (2 chunks / 4 chunks in registers / streamed; student fp32 / bf16, teacher fp32 / bf16, guided or not).  2 chunks:
    78 - 80 VGPRs, 6 waves per SIMD; 4 chunks: 110 - 113 VGPRs, 4 waves per SIMD -- two 512-thread workgroups per compute unit; streamed: 49 - 62 VGPRs, 8
    waves per SIMD; 80 bytes of LDS each."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_distill.o")
    assert "-ffp-contract=off" in cmd
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 24 and all("tok_distill_kernel" in k for k in kernels), kernels
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v <= 128 and l <= 128 and o >= 4 for v, l, o in zip(vgprs, lds, occ)), (vgprs, lds, occ)
    code = "\n".join(l.split("//")[0] for l in open(os.path.join(G.CSRC, "token_distill.hip")).read().splitlines())
    assert "asm" not in code and "expf" not in code and "fma" not in code and "hipMalloc" not in code and "atomicAdd(float" not in code


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(16384, 0x5A5A5A5A, u32)
    p = x.ctypes.data
    assert p % 16 == 0
    q, t, u = p + 4096 * 4, p + 8192 * 4, p + 12288 * 4            # grad, teacher, teacher_uncond: disjoint from a 2-row x 128-code fp32 call's extents

    def call(student=p, dtype=0, teacher=t, uncond=None, tdtype=0, R=2, C=100, rs=128, ts=128, off=0, s=1.0, V=None, scale=None, mask=None, kl=p, ce=p, h=p, lse=p,
             grad=q, gs=128, bad=p, ign=p):
        return lib.selftok_distill_rows(student, dtype, teacher, uncond, tdtype, R, C, rs, ts, off, s, off + C if V is None else V, scale, mask, kl, ce, h, lse, grad, gs,
                                        bad, ign, None)

    for s in (float("nan"), float("inf"), -float("inf")):
        assert call(uncond=u, s=s) == -1 and "cfg_scale" in err(), s
    for kw in (dict(V=99), dict(V=0), dict(off=8, C=100, V=104), dict(V=129), dict(V=128, gs=124), dict(V=1 << 40)):      # V < offset + C, V > row_stride, V > grad_stride
        assert call(**kw) == -1 and "V" in err(), kw
    for kw in (dict(grad=p + 16), dict(grad=p + 128 * 4), dict(grad=p + 224 * 4), dict(student=q + 64, grad=q), dict(grad=p, gs=132, rs=128), dict(grad=p, gs=124)):
        assert call(**kw) == -1 and ("overlap" in err() or "V" in err()), (kw, err())
    assert call(grad=p + 16) == -1 and "student overlap" in err() and call(grad=p, gs=256, rs=128, V=100) == -1 and "student overlap" in err()
    for kw in (dict(grad=t), dict(grad=t + 16), dict(grad=t + 224 * 4), dict(teacher=q + 112 * 4), dict(teacher=p, grad=p), dict(uncond=u, grad=u + 64),
               dict(uncond=q), dict(tdtype=1, teacher=q + 904), dict(ts=256, teacher=q - 300 * 4)):
        assert call(**kw) == -1 and "teacher overlap" in err(), (kw, err())
    for C in (0, -1, 65537, 1 << 20):
        assert call(C=C, rs=1 << 21, ts=1 << 21, V=1 << 21, gs=1 << 21) == -1 and "C" in err(), C
    for kw in (dict(dtype=-1), dict(dtype=2), dict(tdtype=2), dict(tdtype=16)):
        assert call(**kw) == -1 and "dtype" in err(), kw
    for kw in (dict(student=None), dict(teacher=None), dict(kl=None), dict(ce=None), dict(h=None), dict(lse=None), dict(bad=None), dict(ign=None)):
        assert call(**kw) == -1 and "null" in err(), kw
    for kw in (dict(student=p + 4), dict(student=p + 8), dict(grad=q + 4), dict(teacher=t + 8), dict(uncond=u + 4), dict(off=2, rs=132, gs=132, ts=132), dict(rs=130),
               dict(gs=130), dict(ts=130), dict(dtype=1, student=p + 2), dict(dtype=1, grad=q + 4), dict(tdtype=1, teacher=t + 4)):
        assert call(**kw) == -1 and "misaligned" in err(), kw
    for kw in (dict(kl=p + 2), dict(ce=p + 1), dict(h=p + 2), dict(lse=p + 1), dict(scale=p + 2), dict(bad=p + 2), dict(ign=p + 2)):
        assert call(**kw) == -1 and "aligned" in err(), kw
    for kw in (dict(C=100, rs=96), dict(C=100, ts=96), dict(C=100, off=32, rs=128), dict(off=-4), dict(rs=-1), dict(ts=-1), dict(R=-1), dict(off=256, rs=128)):
        assert call(**kw) == -1 and "window" in err(), kw
    assert call(R=0, student=None, teacher=None, kl=None, ce=None, h=None, lse=None, grad=None, bad=None, ign=None) == 0       # no rows: nothing launched
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves its outputs untouched
    # the Python layer: shapes, dtypes and the guided teacher's pairing are refused before the device is asked for
    st, te = torch.zeros(2, 128), torch.zeros(2, 128, dtype=torch.bfloat16)
    for kw, word in ((dict(teacher_uncond=torch.zeros(2, 128)), "teacher_uncond"), (dict(teacher_uncond=torch.zeros(2, 64, dtype=torch.bfloat16)), "teacher_uncond"),
                     (dict(teacher_uncond=te, cfg_scale=float("nan")), "cfg_scale"), (dict(teacher_uncond=te, cfg_scale=float("inf")), "cfg_scale"), (dict(C=129), "window"),
                     (dict(offset=-1), "window")):
        with pytest.raises(_lib.SelftokHipError, match=word):
            ops.token_distill(st, te, **kw)
    for bad_t in (torch.zeros(2, 128, dtype=torch.float16), torch.zeros(2, 64), torch.zeros(3, 128)):
        with pytest.raises(_lib.SelftokHipError, match="teacher"):
            ops.token_distill(st, bad_t)
    with pytest.raises(_lib.SelftokHipError, match="student"):
        ops.token_distill(torch.zeros(2, 128, dtype=torch.float16), te)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_distill(st, te)


class _StubOps:
    """records every call and plays the kernel's part on the host: kl = 1 + the row's index, the gradient row filled with the row's scale (1 without one); rows
    the mask switches off: kl 0, a zero row"""

    def __init__(self):
        self.calls = []

    def token_distill(self, student, teacher, **kw):
        B, S, V = student.shape
        self.calls.append(dict(kw, teacher=teacher))
        live = torch.ones(B, S, dtype=torch.bool) if kw.get("row_mask") is None else kw["row_mask"].reshape(B, S) != 0
        kl = torch.where(live, torch.arange(1.0, B * S + 1).reshape(B, S), torch.zeros(()))
        grad = None
        if kw.get("want_grad", True):
            g = torch.ones(B, S) if kw["row_scale"] is None else kw["row_scale"].reshape(B, S)
            grad = student if kw["inplace"] else torch.empty_like(student)
            grad.copy_(torch.where(live, g, torch.zeros(())).unsqueeze(-1).expand(B, S, V))
        z = torch.zeros(1, dtype=torch.int32)
        return kl, kl + 10, kl + 20, kl + 30, grad, z, torch.tensor([int((~live).sum())], dtype=torch.int32)


def test_token_distillation_bookkeeping_over_an_ops_stub():
    B, S, V = 2, 4, 16
    new = lambda: torch.zeros(B, S, V, requires_grad=True)
    teacher = torch.zeros(B, S, V, dtype=torch.bfloat16, requires_grad=True)
    stub = _StubOps()
    lg = new()
    loss, st = losses.token_distillation(lg, teacher, C=8, offset=4, ops=stub, return_stats=True)
    call = stub.calls[0]
    assert (call["C"], call["offset"], call["inplace"], call["row_mask"], call["teacher_uncond"], call["cfg_scale"]) == (8, 4, False, None, None, 1.0)
    assert not call["teacher"].requires_grad and torch.allclose(call["row_scale"], torch.full((B, S), 1 / 8))
    assert float(loss.detach()) == pytest.approx(36 / 8) and loss.dtype == torch.float32 and loss.dim() == 0 and st.ce[0, 0] == 11 and st.h_teacher[1, 3] == 28
    (loss * 3).backward()                                           # the upstream gradient reaches every element; the teacher gets none
    assert torch.allclose(lg.grad, torch.full((B, S, V), 3 / 8)) and teacher.grad is None
    # a step count per sequence: AR row s is live while s < steps[b]; the mean counts the live rows
    loss, st = losses.token_distillation(new(), teacher, steps=[4, 2], ops=stub, return_stats=True)
    assert stub.calls[-1]["row_mask"].tolist() == [[1, 1, 1, 1], [1, 1, 0, 0]] and stub.calls[-1]["row_mask"].dtype == torch.uint8
    assert int(st.ignored[0]) == 2 and float(loss.detach()) == pytest.approx((1 + 2 + 3 + 4 + 5 + 6) / 6) and torch.allclose(stub.calls[-1]["row_scale"], torch.full((B, S), 1 / 6))
    # sum and none
    lg = new()
    loss = losses.token_distillation(lg, teacher, reduction="sum", ops=stub)
    assert float(loss.detach()) == 36.0 and stub.calls[-1]["row_scale"] is None
    lg = new()
    loss = losses.token_distillation(lg, teacher, reduction="none", steps=[4, 3], ops=stub)
    assert loss.tolist() == [[1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 0.0]]
    up = torch.arange(8.0).reshape(B, S)
    loss.backward(up)                                               # per-row upstream gradients
    assert torch.equal(lg.grad[..., 0], torch.where(torch.tensor([[True] * 4, [True] * 3 + [False]]), up, torch.zeros(())))
    # weights by TOKENIZER position: AR row s carries weights[S - 1 - s]; by row; in tokenizer order
    w = torch.tensor([1.0, 2.0, 3.0, 4.0])
    loss = losses.token_distillation(new(), teacher, weights=w, ops=stub)
    wr = [4.0, 3.0, 2.0, 1.0]
    assert float(loss.detach()) == pytest.approx(sum(a * b for a, b in zip(wr + wr, range(1, 9))) / 20) and torch.allclose(stub.calls[-1]["row_scale"], (torch.tensor(wr) / 20).expand(B, S))
    loss = losses.token_distillation(new(), teacher, weights=w, ar_order=False, reduction="sum", ops=stub)
    assert torch.equal(stub.calls[-1]["row_scale"], w.expand(B, S)) and float(loss.detach()) == pytest.approx(sum(a * b for a, b in zip([1, 2, 3, 4] * 2, range(1, 9))))
    wb = torch.tensor([[1.0, 0.0, 2.0, 1.0], [1.0, 1.0, 1.0, 5.0]])
    loss = losses.token_distillation(new(), teacher, weights=wb, steps=[4, 3], ops=stub)
    assert float(loss.detach()) == pytest.approx((1 + 6 + 4 + 5 + 6 + 7) / 7.0)
    # the guided teacher is handed through, detached
    unc = torch.zeros(B, S, V, dtype=torch.bfloat16, requires_grad=True)
    losses.token_distillation(new(), teacher, teacher_uncond=unc, cfg_scale=3.0, ops=stub)
    assert stub.calls[-1]["cfg_scale"] == 3.0 and stub.calls[-1]["teacher_uncond"] is not None and not stub.calls[-1]["teacher_uncond"].requires_grad
    # in place: the gradient IS the student tensor; a second backward is refused, so is a double backward
    raw = torch.zeros(B, S, V, requires_grad=True)
    lg = raw * 1.0
    ver = lg._version
    loss = losses.token_distillation(lg, teacher, inplace=True, ops=stub)
    assert stub.calls[-1]["inplace"] and torch.allclose(lg.detach()[0, 0], torch.full((V,), 1 / 8)) and lg._version > ver
    loss.backward(retain_graph=True)
    assert torch.allclose(raw.grad[0], torch.full((S, V), 1 / 8))
    with pytest.raises(RuntimeError, match="second time"):
        loss.backward()
    lg = new()
    loss = losses.token_distillation(lg, teacher, ops=stub)
    (gr,) = torch.autograd.grad(loss, lg, create_graph=True)
    if gr.requires_grad:                                            # once_differentiable: differentiating a second time is an error
        with pytest.raises(RuntimeError):
            gr.sum().backward()
    for kw in (dict(reduction="max"), dict(weights=torch.ones(3)), dict(cfg_scale=2.0)):
        with pytest.raises(ValueError):
            losses.token_distillation(new(), teacher, ops=stub, **kw)
    with pytest.raises(ValueError, match="one shape"):
        losses.token_distillation(new(), torch.zeros(B, S, V + 1), ops=stub)
    # token_kl: q is the student side, p the (guided) teacher; no gradient is asked for; the reductions per tokenizer position
    out = sampling.token_kl(teacher.detach(), new().detach(), uncond_p=unc.detach(), cfg_scale=2.0, steps=[4, 2], ops=stub)
    call = stub.calls[-1]
    assert call["want_grad"] is False and call["cfg_scale"] == 2.0 and call["teacher"].dtype == torch.bfloat16 and call["row_mask"].tolist() == [[1, 1, 1, 1], [1, 1, 0, 0]]
    assert out._fields == ("kl", "ce", "entropy_p", "bad", "ignored") and float(out.mean()) == pytest.approx(21 / 6) and float(out.mean("ce")) == pytest.approx(21 / 6 + 10)
    assert out.per_position().tolist() == [4.0, 3.0, 4.0, 3.0]     # AR row s is tokenizer position S - 1 - s: rows (1, 5), (2, 6), 3, 4 -> positions 3, 2, 1, 0
