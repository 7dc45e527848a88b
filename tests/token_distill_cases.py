"""The token distillation's arithmetic of record in numpy float32 / uint64 / float64 (include/selftok_hip_ext.h states it; csrc/token_distill.hip runs it), a
second, brute-force formulation (a Python loop per row, Python integers for every sum, its own address arithmetic into the flat student, teacher and gradient
buffers), the case table and the planted mistakes -- shared by tests/test_token_distill_cpu.py and tests/test_token_distill_gpu.py.

The key, the maximum and the integer mass are the sampler's and are IMPORTED from tests/token_sample_cases.py, not restated.  What is this entry's own: the
guided teacher, the teacher's entropy term, the cross term and its two limbs, the four fp64 outputs, p = q / Q on either side, the gradient row with its zero
columns, its bf16 rounding and the row kinds.

Launch geometry the table is built around (csrc/token_distill.hip): 512 threads own a row, a thread owns 4-code chunks t, t + 512, .. of both rows; C <= 4096
runs the 2-chunk kernel, C <= 8192 the 4-chunk kernel, above that the streamed one, which reads every chunk three times; the up to three codes past the last
whole chunk (C % 4) are thread 0's; the grid is min(R, 65536) x ceil(R / 65536) workgroups.  Edges named below: GEOMETRY_C and GEOMETRY_R.

One rule of the data: the STUDENT logits of every case but the "same" ones lie on the grid of multiples of 2^-10 (Gaussian draws rounded to it; bf16 rounding
keeps a value on it), so that the fp32 difference b - mB is exact and the planted mistake "x from the fp32 d" moves nothing there; the "same" cases (teacher ==
student, raw Gaussian floats on both sides, in every kernel instance) are where it must move kl by far more than 1000 gates -- kl is the cancellation
E_X - E_A there.  The TEACHER logits are raw floats everywhere."""
import math
from collections import namedtuple

import numpy as np

import token_sample_cases as TC
from token_sample_cases import OFFSET_VLM, to_bf16_bits, weight, widen_bf16

f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64
NT, SMALL_C, REG_C, GRID_X = 512, 4096, 8192, 65536
GEOMETRY_C = (2047, 2048, 2049,                                     # one whole chunk per thread, +- 1 (4 * NT)
              2050,                                                 # a partial chunk of two codes
              4095, 4096, 4097,                                     # 2-chunk kernel | 4-chunk kernel
              8191, 8192, 8193,                                     # 4-chunk kernel | streamed kernel
              65536)                                                # 32 chunk rounds
GEOMETRY_R = (GRID_X + 1,)                                          # one workgroup into the second grid row
SENT = f32(-768.0)                                                  # what the gradient buffer holds before the call (exact in bf16)
NAN32 = f32("nan")
ROW_SCALES = (0.5, 0.0, -1.5, 2.0, 1.0 / 3.0)                       # per-row scales: a zero and a negative one among them
X_LIMIT = 32768.0
GRID = 1024.0                                                       # the student's grid: multiples of 1 / 1024

Out = namedtuple("Out", "kl ce h lse grad bad ignored overflow qa qb sa slo shi pa pb g")     # grad: [R, row] fp32 or bf16 bits, None without a gradient


def narrow(x, truncate=False):
    """fp32 -> bf16 bits: to nearest even, once"""
    x = np.asarray(x, dtype=f32)
    return (x.view(u32) >> u32(16)).astype(np.uint16) if truncate else to_bf16_bits(x)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind R C sd td offset V row trow s scale mask")


def _case(name, kind, R, C, sd="f32", td="f32", offset=0, vpad=0, pad=0, tpad=0, s=None, scale=None, mask=False):
    V = offset + C + vpad
    row = V + pad
    row += (-row) % 4
    trow = offset + C + tpad
    trow += (-trow) % 4
    return Case(name, kind, R, C, sd, td, offset, V, row, trow, None if s is None else f32(s), scale, mask)


CASES = [
    _case("c1", "small", 1, 1),
    _case("c2_rows_s1", "small", 3, 2, scale="rows", s=1.0),
    _case("c3_R5_mixed", "small", 5, 3, td="bf16"),
    _case("c4_const", "small", 5, 4, scale="const", sd="bf16"),
    _case("c5_mask_s3", "small", 6, 5, s=3.0, mask=True, tpad=8),
    _case("c255_bf16_both", "gauss1", 5, 255, sd="bf16", td="bf16", scale="rows"),
    _case("c2047_s0", "gauss1", 3, 2047, s=0.0),
    _case("c2048_bf16_f32", "gauss1", 3, 2048, sd="bf16", scale="const"),
    _case("c2049_g8", "gauss8", 3, 2049, scale="rows", td="bf16"),
    _case("c2050_pads", "gauss1", 3, 2050, vpad=3, pad=5, tpad=12, s=3.0),
    _case("c4095_stride", "gauss1", 3, 4095, offset=4, vpad=1, pad=4, mask=True),
    _case("c4096_R64", "gauss1", 64, 4096, scale="rows"),
    _case("c4097_bf16_both_s3", "gauss1", 3, 4097, sd="bf16", td="bf16", s=3.0, tpad=4),
    _case("c8191_g8_s1", "gauss8", 3, 8191, s=1.0, scale="rows"),
    _case("c8192_vlm", "gauss1", 3, 8192, offset=OFFSET_VLM, scale="const", mask=True),
    _case("c8192_f32_bf16", "gauss8", 3, 8192, td="bf16"),
    _case("c8193_rows", "gauss1", 3, 8193, scale="rows"),
    _case("c8193_bf16_f32_s3", "gauss1", 2, 8193, sd="bf16", vpad=2, pad=8, s=3.0),
    _case("c8194_vlm_bf16_both", "gauss1", 2, 8194, sd="bf16", td="bf16", offset=OFFSET_VLM, vpad=5, pad=3, tpad=8),
    _case("c65536_g8", "gauss8", 3, 65536, scale="rows"),
    _case("c65536_bf16_both_s1", "gauss1", 2, 65536, sd="bf16", td="bf16", pad=8, s=1.0),
    _case("c1000_vlm_mixed_s3", "gauss1", 5, 1000, td="bf16", offset=OFFSET_VLM, vpad=6, pad=24, tpad=16, s=3.0, scale="rows"),
    _case("four", "four", 9, 1000, scale="const"),
    _case("four_bf16_reg", "four", 6, 4097, sd="bf16", td="bf16"),
    _case("zeros_pair", "zeros", 6, 5),
    _case("same_small", "same", 5, 1000, scale="rows"),
    _case("same_reg", "same", 3, 6000),
    _case("same_stream", "same", 3, 9001),
    _case("onehot", "onehot", 4, 257),
    _case("onehot_reg_bf16", "onehot", 4, 4097, sd="bf16", scale="rows"),
    _case("student_neginf_weighted", "sneginf", 4, 257, scale="rows"),
    _case("student_neginf_unweighted", "sneginf0", 4, 300),
    _case("student_neginf_unweighted_stream", "sneginf0", 2, 8197, td="bf16", scale="rows"),
    _case("under_limit", "under", 3, 300),
    _case("over_limit", "over", 3, 300, scale="const"),
    _case("over_limit_stream", "over", 3, 8200),
    _case("masked_bf16", "gauss1", 6, 300, sd="bf16", offset=8, mask=True, scale="rows"),
    _case("masked_reg_s1", "gauss1", 3, 5000, mask=True, s=1.0, td="bf16"),
    _case("masked_stream", "gauss1", 3, 8195, mask=True),
    _case("bad_rows_small", "bad", 9, 1000, scale="rows"),
    _case("bad_rows_small_s3", "bad", 9, 256, sd="bf16", offset=8, vpad=2, pad=4, s=3.0),
    _case("bad_rows_reg", "bad", 9, 4100, vpad=1, scale="const", td="bf16"),
    _case("bad_rows_reg_s1", "bad", 9, 4100, s=1.0),
    _case("bad_rows_stream", "bad", 9, 8198, offset=4, vpad=3),
    _case("bad_rows_stream_s3", "bad", 9, 8198, s=3.0, sd="bf16", td="bf16"),
    _case("grid_second_row", "small", GRID_X + 1, 5, scale="const"),
]
BY_NAME = {c.name: c for c in CASES}
FOUR = TC.FOUR
_CACHE = {}


def row_scales(c):
    """fp32 [R], or None"""
    if c.scale is None:
        return None
    if c.scale == "const":
        return np.full(c.R, 0.25, f32)
    return np.asarray(ROW_SCALES, f32)[np.arange(c.R) % len(ROW_SCALES)]


def _on_grid(x):
    return (np.rint(np.asarray(x, f64) * GRID) / GRID).astype(f32)


def _pack(c, w, rowlen, dtype):
    buf = np.full((c.R, rowlen), np.nan, f32)
    buf[:, c.offset:c.offset + c.C] = w
    return to_bf16_bits(buf) if dtype == "bf16" else buf


def make(name):
    """-> dict(student: host array [R, row], teacher: [R, trow], uncond: [R, trow] or None -- NaN outside the window, bf16 as uint16 bits; scale: fp32 [R] or None;
    mask: uint8 [R] or None).  Built once per case and shared: treat as read-only."""
    if name in _CACHE:
        return _CACHE[name]
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 36)
    R, C = c.R, c.C
    sigma = 8.0 if c.kind == "gauss8" else 1.0
    b = _on_grid(rng.standard_normal((R, C)) * sigma)
    a = (rng.standard_normal((R, C)) * sigma).astype(f32)
    if c.kind == "four":
        b = np.asarray(FOUR, f32)[rng.integers(0, 4, size=(R, C))]
        a = np.asarray(FOUR, f32)[rng.integers(0, 4, size=(R, C))]
    elif c.kind == "zeros":
        b = np.stack([np.roll(np.asarray([-1.0, -0.0, 0.0, -0.0, -2.0], f32), r // 3) for r in range(R)])
        a = np.stack([np.roll(np.asarray([0.0, -0.0, -1.0, -0.0, -3.0], f32), r % 3) for r in range(R)])
    elif c.kind == "same":
        b = a.copy()                                                # raw floats on both sides
    elif c.kind == "onehot":                                        # the teacher: one finite code, the rest -inf
        hot = np.asarray([0, C // 2, C - 1, 7])[np.arange(R) % 4]
        a = np.full((R, C), -np.inf, f32)
        a[np.arange(R), hot] = f32(1.5)
    elif c.kind in ("sneginf", "sneginf0"):                         # the student at -inf on every fifth code; the teacher weights those codes, or gives them no mass
        b[:, ::5] = -np.inf
        if c.kind == "sneginf0":
            a[:, ::5] = np.where(np.arange(R)[:, None] % 2 == 0, f32(-np.inf), f32(-60.0))
    elif c.kind in ("under", "over"):                               # a weighted code just under / at / over 32768 below the student's maximum (0 at code 0)
        b = -np.abs(b)
        b[:, 0] = 0.0
        far = {"under": (-32767.5, -32767.0, -30000.25), "over": (-32768.0, -32768.5, -40000.0)}[c.kind]
        for r in range(R):
            b[r, 7 + r] = far[r % 3]
            a[r, 7 + r] = a[r].max() + f32(1.0 if r != 1 else 0.0)  # the teacher's maximum (row 1: a tie with it)
    if c.kind == "bad":                                             # good rows between the bad ones (rows 1, 3, 5, 7; row 2 when guided)
        b[1, C // 3] = np.nan
        a[3, C - 1] = np.inf
        b[5, :] = -np.inf
        a[7, :] = -np.inf
    lu = None
    if c.s is not None:
        lu = (a - f32(0.5) * rng.standard_normal((R, C)).astype(f32)).astype(f32)
        if c.kind == "four":
            lu = np.asarray(FOUR, f32)[rng.integers(0, 4, size=(R, C))]
        if c.kind == "bad":
            lu[7, :] = f32(0.0)                                     # -inf - 0 = -inf, s * -inf = -inf, 0 + -inf: nothing above -inf
            a[2, 5], lu[2, 5] = -np.inf, -np.inf                    # -inf in both inputs: the guidance gives NaN
            lu[3, :] = f32(0.25)
    mask = None
    if c.mask:                                                      # every third row (1, 4, ..) is padding, and its logits are NaN on both sides
        mask = (np.arange(R) % 3 != 1).astype(np.uint8)
        b[mask == 0], a[mask == 0] = np.nan, np.nan
        if lu is not None:
            lu[mask == 0] = np.nan
    d = {"student": _pack(c, b, c.row, c.sd), "teacher": _pack(c, a, c.trow, c.td), "uncond": None if lu is None else _pack(c, lu, c.trow, c.td),
         "scale": row_scales(c), "mask": mask}
    _CACHE[name] = d
    return d


def _window(c, arr, dtype):
    return None if arr is None else (widen_bf16(arr) if dtype == "bf16" else arr)[:, c.offset:c.offset + c.C]


def windows(name):
    """(teacher lc, uncond lu or None, student b): the fp32 windows [R, C] of a case, widened"""
    c, d = BY_NAME[name], make(name)
    return _window(c, d["teacher"], c.td), _window(c, d["uncond"], c.td), _window(c, d["student"], c.sd)


def guided(lc, lu, s, mut=None):
    """the teacher's logit: the sampler's step 1 -- difference, product, sum, each rounded to fp32"""
    lc = np.asarray(lc, f32)
    if lu is None:
        return lc
    with np.errstate(invalid="ignore", over="ignore"):
        diff = (lc - lu).astype(f32)
        prod = (f32(s) * diff).astype(f32)
        return ((lc if mut == "guidance_from_cond" else lu) + prod).astype(f32)


def _log_q(q):
    return math.log(q * 2.0 ** -32) if q else -math.inf


def _quot(x, y):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(f64(x) / f64(y))


def _row_outputs(ma, mb, QA, QB, SA, SLO, SHI, over, mut):
    """the four fp32 outputs of one good row from its integer sums: Python floats (fp64), one rounding each"""
    LA, LB = _log_q(QA), _log_q(QB)
    if mut == "la_lb_swapped":
        LA, LB = LB, LA
    EA = _quot(float(SA), 65536.0 * float(QA))
    X = float(SLO) if mut == "s_hi_dropped" else float(SHI) * 4294967296.0 + float(SLO)
    EX = _quot(X, 65536.0 * float(QB if mut == "ex_over_qb" else QA))
    with np.errstate(invalid="ignore", over="ignore"):
        lse, h = f32(f64(mb) + f64(LB)), f32(f64(LA) + f64(EA))
        ce, kl = f32(f64(LB) + f64(EX)), f32((f64(LB) - f64(LA)) + f64(EX) - f64(EA))
    if over:
        ce = kl = f32(np.inf)
    return kl, ce, h, lse


# ---- the emulation: all rows of a case at once ------------------------------------------------------------------------------------------------------
def distill_rows(lc, lu, b, *, s=1.0, scale=None, mask=None, V=None, offset=0, row=None, bf16=False, mut=None, with_grad=True):
    """lc, lu (or None), b fp32 [R, C] (the windows); scale fp32 [R] or None; mask uint8 [R] or None -> Out.  The gradient buffer [R, row] starts as SENT
    everywhere; columns [0, V) of every row are written."""
    lc, b = np.asarray(lc, f32), np.asarray(b, f32)
    R, C = b.shape
    V = offset + C if V is None else V
    row = V if row is None else row
    ignored = np.zeros(R, bool) if mask is None else np.asarray(mask) == 0
    a = guided(lc, lu, s, mut)
    with np.errstate(invalid="ignore"):
        poisoned = lambda t: np.isnan(t).any(1) | (t == np.inf).any(1)
        bad = poisoned(lc) | poisoned(a) | poisoned(b) | (a == -np.inf).all(1) | (b == -np.inf).all(1)
        if lu is not None:
            bad |= poisoned(np.asarray(lu, f32))
    bad &= ~ignored
    nan, zi = np.full(R, NAN32, f32), np.zeros(R, object)
    kl, ce, h, lse = nan.copy(), nan.copy(), nan.copy(), nan.copy()
    for o in (kl, ce, h, lse):
        o[ignored] = 0.0
    qa_t, qb_t, sa_t, slo_t, shi_t = zi.copy(), zi.copy(), zi.copy(), zi.copy(), zi.copy()
    overflow = np.zeros(R, bool)
    pa_out, pb_out, g_out = np.zeros((R, C), f32), np.zeros((R, C), f32), np.zeros(R, f32)
    grad = np.full((R, row), SENT, f32)
    n_live = C - C % 4 if mut == "tail_chunk_dropped" else C       # the codes a kernel without its partial chunk would see
    grad[bad if mut == "ignored_unwritten" else bad | ignored, :V] = 0.0
    gi = np.flatnonzero(~bad & ~ignored)
    if gi.size:
        ag, bg = np.where(a[gi] == 0, f32(0.0), a[gi]), np.where(b[gi] == 0, f32(0.0), b[gi])       # -0.0 counts as +0.0
        ma, mb = ag.max(1), bg.max(1)
        with np.errstate(invalid="ignore"):
            da, db = (ag - ma[:, None]).astype(f32), (bg - mb[:, None]).astype(f32)
            _, qa = weight(da)
            _, qb = weight(db)
        qa, qb = qa.copy(), qb.copy()
        qa[:, n_live:] = 0
        qb[:, n_live:] = 0
        QA, QB = qa.sum(1, dtype=u64), qb.sum(1, dtype=u64)
        qad = qa.astype(f64)
        dda = np.where(qa > 0, da, f32(0.0))
        ha = np.trunc(qad * (-dda).astype(f64) * 65536.0).astype(u64)
        with np.errstate(invalid="ignore"):
            x = (-db).astype(f64) if mut == "x_from_d32" else mb.astype(f64)[:, None] - bg.astype(f64)
            live = np.ones_like(qa, bool) if mut == "cross_over_zero_mass" else qa > 0
            live[:, n_live:] = False
            fits = x < X_LIMIT
            over = (live & ~fits).any(1)
            cv = np.trunc((qad * np.where(live & fits, x, 0.0)) * 65536.0).astype(u64)
        SA, SLO, SHI = ha.sum(1, dtype=u64), (cv & u64(0xFFFFFFFF)).sum(1, dtype=u64), (cv >> u64(32)).sum(1, dtype=u64)
        for j, r in enumerate(gi):
            kl[r], ce[r], h[r], lse[r] = _row_outputs(ma[j], mb[j], int(QA[j]), int(QB[j]), int(SA[j]), int(SLO[j]), int(SHI[j]), over[j], mut)
            qa_t[r], qb_t[r], sa_t[r], slo_t[r], shi_t[r] = int(QA[j]), int(QB[j]), int(SA[j]), int(SLO[j]), int(SHI[j])
        overflow[gi] = over
        g = np.ones(gi.size, f32) if scale is None else np.asarray(scale, f32)[gi]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            pa = (qad * np.divide(1.0, QA.astype(f64))[:, None]).astype(f32)
            pb = (qb.astype(f64) * np.divide(1.0, QB.astype(f64))[:, None]).astype(f32)
            if mut == "pa_minus_pb":
                vals = (g[:, None] * (pa - pb).astype(f32)).astype(f32)
            elif mut == "scale_before_diff":
                vals = ((g[:, None] * pb).astype(f32) - (g[:, None] * pa).astype(f32)).astype(f32)
            else:
                vals = (g[:, None] * (pb - pa).astype(f32)).astype(f32)
        pa_out[gi], pb_out[gi], g_out[gi] = pa, pb, g
        if mut != "outside_unwritten":
            grad[gi, :offset] = 0.0
            grad[gi, offset + C:V] = 0.0
        grad[gi, offset:offset + n_live] = vals[:, :n_live]
    if bf16:
        grad = narrow(grad, truncate=mut == "bf16_truncated")
    return Out(kl, ce, h, lse, grad if with_grad else None, bad, ignored, overflow, qa_t, qb_t, sa_t, slo_t, shi_t, pa_out, pb_out, g_out)


# ---- the second formulation: one row, Python integers and floats, flat buffers -------------------------------------------------------------------------
def _round32(xs):
    return np.asarray(xs, dtype=f64).astype(f32)


def _cut(flat, at, C, dtype):
    piece = flat[at:at + C]
    return (widen_bf16(piece) if dtype == "bf16" else piece).astype(f32)


def distill_row_brute(c, d, r, mut=None):
    """-> (kl, ce, h, lse fp32, (QA, QB, S_A, S_lo, S_hi), the row of the gradient buffer as fp32 values or bf16 bits [row], bad, ignored, overflow).  Every
    address is computed here, from the flat buffers; every sum is a Python integer sum over Python lists; the per-code products go through Python floats
    (fp64).  The planted mistakes are written a second time, independently."""
    C, off, V, rowlen = c.C, c.offset, c.V, c.row
    buf = [float(SENT)] * rowlen

    def finish(outs, sums, is_bad, ign, over):
        arr = np.asarray(buf, dtype=f64).astype(f32)
        if c.sd == "bf16":
            arr = (arr.view(u32) >> u32(16)).astype(np.uint16) if mut == "bf16_truncated" else to_bf16_bits(arr)
        return tuple(f32(v) for v in outs) + (sums, arr, is_bad, ign, over)

    if d["mask"] is not None and int(d["mask"].reshape(-1)[r]) == 0:           # nothing of the row is read
        if mut != "ignored_unwritten":
            buf[:V] = [0.0] * V
        return finish((0.0, 0.0, 0.0, 0.0), (0, 0, 0, 0, 0), False, True, False)
    bv = _cut(d["student"].reshape(-1), r * rowlen + off, C, c.sd)
    lcv = _cut(d["teacher"].reshape(-1), r * c.trow + off, C, c.td)
    inputs = [bv.tolist(), lcv.tolist()]
    av = lcv
    if d["uncond"] is not None:
        luv = _cut(d["uncond"].reshape(-1), r * c.trow + off, C, c.td)
        inputs.append(luv.tolist())
        with np.errstate(invalid="ignore", over="ignore"):
            step = f32(c.s) * (lcv - luv)                           # fp32 arrays: each operation rounds once
            av = (lcv + step) if mut == "guidance_from_cond" else (luv + step)
    inputs.append(av.tolist())
    is_bad = any(math.isnan(v) or v == math.inf for vs in inputs for v in vs) or all(v == -math.inf for v in inputs[0]) or all(v == -math.inf for v in inputs[-1])
    if is_bad:
        buf[:V] = [0.0] * V
        return finish((NAN32,) * 4, (0, 0, 0, 0, 0), True, False, False)
    al, bl = [0.0 if v == 0 else v for v in av.tolist()], [0.0 if v == 0 else v for v in bv.tolist()]
    ma, mb = max(al), max(bl)
    with np.errstate(invalid="ignore"):
        da = (np.asarray(al, f32) - f32(ma)).astype(f32)
        db = (np.asarray(bl, f32) - f32(mb)).astype(f32)
        qa = [int(v) for v in weight(da)[1].tolist()]
        qb = [int(v) for v in weight(db)[1].tolist()]
    live_n = C // 4 * 4 if mut == "tail_chunk_dropped" else C
    QA, QB = sum(qa[:live_n]), sum(qb[:live_n])
    dal, dbl = da.tolist(), db.tolist()
    SA = SLO = SHI = 0
    over = False
    for i in range(live_n):
        if qa[i] > 0:
            SA += int(float(qa[i]) * -dal[i] * 65536.0)
        if qa[i] > 0 or mut == "cross_over_zero_mass":
            x = -dbl[i] if mut == "x_from_d32" else mb - bl[i]
            if x >= X_LIMIT:
                over = True
            else:
                cc = int(float(qa[i]) * x * 65536.0)
                SLO += cc % (1 << 32)
                SHI += cc // (1 << 32)
    la, lb = (math.log(QA / 2 ** 32) if QA else -math.inf), (math.log(QB / 2 ** 32) if QB else -math.inf)        # Q < 2^53: the quotient is exact
    if mut == "la_lb_swapped":
        lb, la = la, lb
    e_a = _quot(SA, 65536.0 * QA)
    big = SLO if mut == "s_hi_dropped" else float(SHI) * 2.0 ** 32 + float(SLO)
    e_x = _quot(big, 65536.0 * (QB if mut == "ex_over_qb" else QA))
    with np.errstate(invalid="ignore", over="ignore"):
        k_l = f64(lb) - f64(la) + f64(e_x) - f64(e_a)
        outs = (math.inf if over else k_l, math.inf if over else f64(lb) + f64(e_x), f64(la) + f64(e_a), f64(mb) + f64(lb))
    g = 1.0 if d["scale"] is None else float(d["scale"][r])
    inv_a, inv_b = _quot(1.0, float(QA)), _quot(1.0, float(QB))
    with np.errstate(invalid="ignore", over="ignore"):
        pa, pb = _round32([q * inv_a for q in qa]), _round32([q * inv_b for q in qb])
        if mut == "pa_minus_pb":
            vals = f32(g) * (pa - pb)
        elif mut == "scale_before_diff":
            vals = f32(g) * pb - f32(g) * pa
        else:
            vals = f32(g) * (pb - pa)
    if mut != "outside_unwritten":
        for i in list(range(0, off)) + list(range(off + C, V)):
            buf[i] = 0.0
    vl = vals.astype(f32).tolist()
    for i in range(live_n):
        buf[off + i] = vl[i]
    return finish(outs, (QA, QB, SA, SLO, SHI), False, False, over)


def brute_rows(c):
    """the rows the second formulation walks: all of them up to 64 (two of them where a row is longer than 20000 codes), else the first, the last and a spread"""
    R = c.R
    if c.C > 20000:
        return sorted({0, R - 1})
    if R <= 64:
        return list(range(R))
    return sorted(set(list(range(8)) + list(range(R - 8, R)) + [GRID_X - 1, min(GRID_X, R - 1)] + list(range(0, R, R // 8))))


_REF = {}


def reference(name, mut=None, brute=False):
    """the emulation: Out over all rows.  brute=True: {row: tuple} over brute_rows.  Computed once and shared: treat as read-only."""
    k = (name, mut, brute)
    if k in _REF:
        return _REF[k]
    c, d = BY_NAME[name], make(name)
    if not brute:
        lc, lu, b = windows(name)
        out = distill_rows(lc, lu, b, s=c.s, scale=d["scale"], mask=d["mask"], V=c.V, offset=c.offset, row=c.row, bf16=c.sd == "bf16", mut=mut)
    else:
        out = {r: distill_row_brute(c, d, r, mut) for r in brute_rows(c)}
    _REF[k] = out
    return out


def _fb(v):
    return f32(v).tobytes()


def row_tuple(out, r, sums=True):
    t = (_fb(out.kl[r]), _fb(out.ce[r]), _fb(out.h[r]), _fb(out.lse[r]), out.grad[r].tobytes(), bool(out.bad[r]), bool(out.ignored[r]), bool(out.overflow[r]))
    return t + ((int(out.qa[r]), int(out.qb[r]), int(out.sa[r]), int(out.slo[r]), int(out.shi[r])),) if sums else t


def brute_tuple(t, sums=True):
    u = (_fb(t[0]), _fb(t[1]), _fb(t[2]), _fb(t[3]), t[5].tobytes(), bool(t[6]), bool(t[7]), bool(t[8]))
    return u + (tuple(int(v) for v in t[4]),) if sums else u


def same(name, a, b, sums=True):
    """two results of a case over the rows the brute force walks (either kind each): every output equal, floats bit for bit, the whole gradient buffer row;
    sums=False leaves the five integer sums out: what a caller of the kernel can see"""
    rows = brute_rows(BY_NAME[name])
    ta = [brute_tuple(a[r], sums) if isinstance(a, dict) else row_tuple(a, r, sums) for r in rows]
    tb = [brute_tuple(b[r], sums) if isinstance(b, dict) else row_tuple(b, r, sums) for r in rows]
    return ta == tb


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------------------------
MUTS = ("pa_minus_pb", "x_from_d32", "cross_over_zero_mass", "ex_over_qb", "la_lb_swapped", "guidance_from_cond", "scale_before_diff", "ignored_unwritten",
        "outside_unwritten", "bf16_truncated", "tail_chunk_dropped", "s_hi_dropped")


def needs(mut, c):
    """what a case must have for a mistake to be able to move it at all (necessary, not sufficient)"""
    return {"pa_minus_pb": c.kind != "same", "x_from_d32": c.kind == "same", "cross_over_zero_mass": c.kind in ("sneginf0", "onehot", "over", "under"),
            "ex_over_qb": c.kind != "same", "la_lb_swapped": c.kind != "same", "guidance_from_cond": c.s is not None, "scale_before_diff": c.scale is not None,
            "ignored_unwritten": c.mask, "outside_unwritten": c.offset != 0 or c.V > c.offset + c.C, "bf16_truncated": c.sd == "bf16",
            "tail_chunk_dropped": c.C % 4 != 0, "s_hi_dropped": True}[mut]


def applies(mut, name):
    """does the mistake move what a caller can see of the case?  Decided by the brute-force formulation, where every mistake is written a second time."""
    return not same(name, reference(name, brute=True), reference(name, mut=mut, brute=True), sums=False)


# ---- the derived bounds against fp64 -----------------------------------------------------------------------------------------------------
DQ_CODE = 2.0 ** -21 + 24 * 2.0 ** -24                              # one mass against exp(d) 2^32: the polynomial, and the fp32 rounding of d (|d| <= 24)


def delta_q(C):
    """the relative error of a sum of masses (the loss's): DQ_CODE on each mass, under one unit of truncation per code against Q >= 2^32, and the
    tail below -24 dropped (e^-24 per code against a sum >= 1)"""
    return DQ_CODE + C * (2.0 ** -32 + math.exp(-24.0))


def bound_lse(C, value):
    dq = delta_q(C)
    return dq / (1 - dq) + abs(value) * 2.0 ** -24 + 1e-12


def bound_expectation(C, E, tail):
    """|S / (65536 Q) - sum p_i y_i| for y >= 0 (y = -dA for the entropy, x for the cross term), E the fp64 value: the relative error of every q_i and of Q,
    the fp32 rounding of y where it is one (2^-24 relative), one unit of truncation per code against 65536 Q >= 2^48, and `tail`: what the codes contribute to
    the fp64 value whose mass the kernel may have dropped (the caller sums p_i y_i over the codes more than 22 below the teacher's maximum)"""
    dq = delta_q(C)
    return E * ((DQ_CODE + dq) / (1 - dq) + 2.0 ** -24) + C * 2.0 ** -48 + tail


def bound_h(C, H, EA, tail):
    dq = delta_q(C)
    return dq / (1 - dq) + bound_expectation(C, EA, tail) + abs(H) * 2.0 ** -24 + 1e-12


def bound_ce(C, ce, EX, tail):
    dq = delta_q(C)
    return dq / (1 - dq) + bound_expectation(C, EX, tail) + abs(ce) * 2.0 ** -24 + 1e-12


def bound_kl(C, kl, EX, EA, tail_x, tail_a):
    """kl = (LB - LA) + E_X - E_A: the two logarithms' errors, and the two expectations' errors ADDED -- each is relative to its own size, not to the
    difference's, which is what the cancellation in E_X - E_A costs"""
    dq = delta_q(C)
    return 2 * dq / (1 - dq) + bound_expectation(C, EX, tail_x) + bound_expectation(C, EA, tail_a) + abs(kl) * 2.0 ** -24 + 1e-12


def bound_grad(C, pa, pb, g, bf16=False):
    """elementwise |grad_i - g (pB_i - pA_i)| for one row; pa, pb [C] the fp64 softmaxes.  p = q / Q on either side as in the loss; then the fp32
    difference and the fp32 product, half an ulp each of a value of at most pA + pB; bf16 output: half an ulp of bf16, at most 2^-8 of the value and its error."""
    dq = delta_q(C)
    dp = lambda p: p * ((DQ_CODE + dq) / (1 - dq) + 2.0 ** -24) + 2.0 ** -32 + math.exp(-24.0)
    size = abs(g) * np.abs(pb - pa)
    e = abs(g) * (dp(pa) + dp(pb)) + 2 * abs(g) * (pa + pb) * 2.0 ** -24 + 1e-12
    return e + ((size + e) * 2.0 ** -8 if bf16 else 0.0)
