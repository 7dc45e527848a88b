"""The token loss's arithmetic of record in numpy float32 / uint64 / float64 (include/selftok_hip_ext.h states it; csrc/token_xent.hip runs it), a second,
brute-force formulation (a Python loop per row over Python integers and floats, with its own address arithmetic into the flat logits, id and gradient
buffers), the case table and the planted mistakes -- shared by tests/test_token_xent_cpu.py and tests/test_token_xent_gpu.py.

Steps 1 - 4 (the key, the maximum, the integer mass) are the sampler's and are IMPORTED from tests/token_sample_cases.py, not restated.  What is the loss's
own: the target's address, nll and lse in fp64, the factor a, p = q / Q_total, the gradient row with its zero columns, its bf16 rounding and the row kinds.

Launch geometry the table is built around (csrc/token_xent.hip, the scorer's): 512 threads own a row, a thread owns 4-code chunks t, t + 512, ..; C <= 4096
runs the 2-chunk kernel, C <= 32768 the 16-chunk kernel, above that the streamed one, which reads every chunk three times; the up to three codes past the
last whole chunk (C % 4) are thread 0's; the grid is min(R, 65536) x ceil(R / 65536) workgroups.  Edges named below: GEOMETRY_C and GEOMETRY_R."""
import math
from collections import namedtuple

import numpy as np

import token_sample_cases as TC
from token_sample_cases import OFFSET_VLM, key_of, to_bf16_bits, weight, widen_bf16

f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64
NT, SMALL_C, REG_C, GRID_X = 512, 4096, 32768, 65536
GEOMETRY_C = (2047, 2048, 2049,                                     # one whole chunk per thread, +- 1 (4 * NT)
              2050,                                                 # a partial chunk of two codes
              4095, 4096, 4097,                                     # 2-chunk kernel | 16-chunk kernel
              32767, 32768, 32769,                                  # 16-chunk kernel | streamed kernel
              65536)                                                # 32 chunk rounds
GEOMETRY_R = (GRID_X + 1,)                                          # one workgroup into the second grid row
POISON = 2 ** 31 - 1                                                # what the id buffers hold where no target lives: read by mistake, it makes the row bad
SENT = f32(-768.0)                                                  # what the gradient buffer holds before the call (exact in bf16)
NAN32 = f32("nan")
Z_SMALL, Z_BIG = f32(1e-4), f32(0.5)
ROW_SCALES = (0.5, 0.0, -1.5, 2.0, 1.0 / 3.0)                       # per-row scales: a zero and a negative one among them

Out = namedtuple("Out", "nll lse q_total grad bad ignored a p")     # grad: [R, row] fp32, or uint16 bf16 bits; a [R] fp32, p [R, C] fp32 (for the bounds)


def from_key(key):
    key = np.asarray(key, dtype=u32)
    return np.where(key & u32(0x80000000), key & u32(0x7FFFFFFF), ~key).astype(u32).view(f32)


def narrow(x, truncate=False):
    """fp32 -> bf16 bits: to nearest even, once"""
    x = np.asarray(x, dtype=f32)
    return (x.view(u32) >> u32(16)).astype(np.uint16) if truncate else to_bf16_bits(x)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind B S C dtype offset V row step ids wide tk z scale")


def _case(name, kind, B, C, S=1, dtype="f32", offset=0, vpad=0, pad=0, step=1, ids="int64", wide=False, tk="mix", z=0.0, scale=None):
    V = offset + C + vpad
    row = V + pad
    row += (-row) % 4
    return Case(name, kind, B, S, C, dtype, offset, V, row, step, ids, wide, tk, f32(z), scale)


CASES = [
    _case("c1", "small", 1, 1, tk="argmax"),
    _case("c2_zbig_rows", "small", 3, 2, z=Z_BIG, scale="rows"),
    _case("c3_R3", "small", 3, 3),
    _case("c4_int32", "small", 5, 4, ids="int32", scale="const"),
    _case("c5_S3_rev_zbig", "small", 2, 5, S=3, step=-1, z=Z_BIG),
    _case("c255_S40", "gauss1", 1, 255, S=40, scale="rows"),
    _case("c257_bf16_zbig", "gauss1", 3, 257, dtype="bf16", z=Z_BIG, scale="rows"),
    _case("c2047_z", "gauss1", 3, 2047, z=Z_SMALL),
    _case("c2048_bf16", "gauss1", 3, 2048, dtype="bf16", scale="const"),
    _case("c2049_g8", "gauss8", 3, 2049, scale="rows"),
    _case("c2050_int32_wide", "gauss1", 2, 2050, S=3, ids="int32", wide=True, vpad=3, pad=5),
    _case("c4095_stride_z", "gauss1", 3, 4095, offset=4, vpad=1, pad=4, z=Z_SMALL),
    _case("c4096_R64", "gauss1", 64, 4096, scale="rows"),
    _case("c4096_S40_rev_z", "gauss1", 1, 4096, S=40, step=-1, z=Z_SMALL),
    _case("c4097_bf16_S40_wide_rev", "gauss1", 1, 4097, S=40, dtype="bf16", ids="int32", wide=True, step=-1),
    _case("c32767_g8_z", "gauss8", 3, 32767, z=Z_SMALL, scale="rows"),
    _case("c32768_vlm_z", "gauss1", 1, 32768, S=3, step=-1, offset=OFFSET_VLM, scale="const", z=Z_SMALL),
    _case("c32768_bf16_g8", "gauss8", 3, 32768, dtype="bf16"),
    _case("c32769_zbig", "gauss1", 3, 32769, scale="rows", z=Z_BIG),
    _case("c32769_bf16_z", "gauss1", 1, 32769, dtype="bf16", vpad=2, pad=8, z=Z_SMALL),
    _case("c32770_vlm", "gauss1", 1, 32770, S=3, offset=OFFSET_VLM, vpad=5, pad=3),
    _case("c65536_g8", "gauss8", 3, 65536, scale="rows"),
    _case("c65536_bf16_z", "gauss1", 1, 65536, dtype="bf16", pad=8, z=Z_SMALL),
    _case("c1000_bf16_vlm_wide_rev_zbig", "gauss1", 2, 1000, S=3, step=-1, dtype="bf16", offset=OFFSET_VLM, vpad=6, pad=24, wide=True, z=Z_BIG, scale="rows"),
    _case("four", "four", 9, 1000, tk="tie", scale="const"),
    _case("four_bf16_z", "four", 6, 4097, dtype="bf16", tk="tie", z=Z_SMALL),
    _case("zeros_pair", "zeros", 6, 5, tk="zeros"),
    _case("dominant_zbig", "dominant", 4, 1000, tk="dominant", z=Z_BIG),
    _case("target_neginf", "gauss_neginf", 4, 257, tk="neginf", scale="rows"),
    _case("neginf_but_one", "neginf", 4, 257, tk="neginf_one"),
    _case("neginf_but_one_bf16", "neginf", 4, 4097, dtype="bf16", tk="neginf_one", z=Z_SMALL),
    _case("ignored_z", "gauss1", 2, 1000, S=3, tk="ignored", z=Z_SMALL, vpad=4),
    _case("ignored_int32_rev_bf16", "gauss1", 2, 300, S=3, step=-1, ids="int32", dtype="bf16", tk="ignored", scale="rows", offset=8),
    _case("ignored_c5000_bf16", "gauss1", 1, 5000, S=3, dtype="bf16", tk="ignored", z=Z_SMALL),
    _case("ignored_stream", "gauss1", 1, 32771, S=3, tk="ignored"),
    _case("bad_rows_c4100", "bad", 9, 4100, vpad=1, tk="badtargets", scale="const"),
    _case("bad_rows_z", "bad", 9, 1000, tk="badtargets", z=Z_SMALL, scale="rows"),
    _case("bad_rows_bf16", "bad", 9, 256, dtype="bf16", offset=8, vpad=2, pad=4, tk="badtargets"),
    _case("bad_rows_stream", "bad", 9, 32770, offset=4, vpad=3, tk="badtargets", ids="int32"),
    _case("grid_second_row", "small", 1, 5, S=GRID_X + 1, step=-1, scale="const"),
]
BY_NAME = {c.name: c for c in CASES}
FOUR = TC.FOUR
_CACHE = {}


def rows_of(c):
    return c.B * c.S


def id_geometry(c):
    """(buffer length, base element, seq stride, step stride) of a case's id buffer; `wide`: every other element of a row, rows three elements further apart"""
    a = 2 if c.wide else 1
    seq = a * c.S + (3 if c.wide else 0)
    base = 2 + (a * (c.S - 1) if c.step < 0 else 0)
    return 2 + c.B * seq + 2, base, seq, a * c.step


def row_scales(c):
    """fp32 [R], or None"""
    R = rows_of(c)
    if c.scale is None:
        return None
    if c.scale == "const":
        return np.full(R, 0.25, f32)
    return np.asarray(ROW_SCALES, f32)[np.arange(R) % len(ROW_SCALES)]


def make(name):
    """-> dict(logits: host array [R, row], NaN outside the window, bf16 as uint16 bits; ids: the 1-D id buffer (POISON where no target lives); targets int64
    [R]: the target of row r; scale: fp32 [R] or None).  Built once per case and shared: treat as read-only."""
    if name in _CACHE:
        return _CACHE[name]
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 35)
    R, C = rows_of(c), c.C
    if c.kind in ("gauss1", "bad", "small", "gauss_neginf"):
        w = rng.standard_normal((R, C)).astype(f32)
    elif c.kind == "gauss8":
        w = (rng.standard_normal((R, C)) * 8.0).astype(f32)
    elif c.kind == "four":
        w = np.asarray(FOUR, f32)[rng.integers(0, 4, size=(R, C))]
    elif c.kind == "dominant":
        w = np.full((R, C), -30.0, f32)
        w[np.arange(R), rng.integers(0, C, size=R)] = 0.0
    elif c.kind == "zeros":
        w = np.stack([np.roll(np.asarray([-1.0, -0.0, 0.0, -0.0, -2.0], f32), r // 3) for r in range(R)])
    elif c.kind == "neginf":
        w = np.full((R, C), -np.inf, f32)
        w[np.arange(R), np.asarray([0, C // 2, C - 1, 7])[np.arange(R) % 4]] = f32(1.5)
    if c.kind == "gauss_neginf":
        w[:, ::5] = -np.inf
    if c.kind == "bad":                                             # good rows between a NaN, a +inf and an all -inf row (rows 1, 3, 5)
        w[1, C // 3] = np.nan
        w[3, C - 1] = np.inf
        w[5, :] = -np.inf
    buf = np.full((R, c.row), np.nan, f32)
    buf[:, c.offset:c.offset + C] = w
    d = {"logits": to_bf16_bits(buf) if c.dtype == "bf16" else buf}
    l = _window(c, d)
    t = rng.integers(0, C, size=R).astype(np.int64)
    safe = np.where(np.isnan(l), -np.inf, l)
    k = key_of(np.where(safe == 0, f32(0.0), safe))
    am = np.argmax(k, axis=1)
    amin = C - 1 - np.argmin(k[:, ::-1], axis=1)                    # the LAST index at the lowest key: rank C - 1
    r = np.arange(R)
    if c.tk == "argmax":
        t = am.astype(np.int64)
    elif c.tk == "mix":                                             # r % 4: 0 and 3 anywhere, 1 the last of the order, 2 the first
        t = np.where(r % 4 == 2, am, np.where(r % 4 == 1, amin, t))
    elif c.tk == "tie":                                             # first, middle and last of the target's group of equal logits
        for i in range(R):
            grp = np.flatnonzero(l[i] == l[i, t[i]])
            t[i] = grp[[0, len(grp) // 2, len(grp) - 1][i % 3]]
    elif c.tk == "zeros":
        for i in range(R):
            t[i] = np.flatnonzero(l[i] == 0)[i % 3]
    elif c.tk == "dominant":                                        # the dominant code, and a code 30 below it: q_t = 0, a finite nll
        t = np.where(r % 2 == 0, am, (am + 1 + r) % C)
    elif c.tk == "neginf":
        t = np.where(r % 2 == 0, (t // 5) * 5, np.where(t % 5 == 0, t + 1, t))          # every fifth code is -inf: on it, and beside it
    elif c.tk == "neginf_one":
        t = np.where(r % 2 == 0, am, (am + 1) % C)
    elif c.tk == "ignored":
        t = np.where(r % 3 == 1, -1, np.where(r % 3 == 2, -100, t))
    elif c.tk == "badtargets":
        t[2], t[7] = C, 2 ** 31 + 5
        if c.ids == "int32":
            t[7] = C + 1
    n, base, seq, step = id_geometry(c)
    ids = np.full(n, POISON, np.int32 if c.ids == "int32" else np.int64)
    ids[base + (r // c.S) * seq + (r % c.S) * step] = t
    d["ids"], d["targets"], d["scale"] = ids, t, row_scales(c)
    _CACHE[name] = d
    return d


def _window(c, d):
    a = d["logits"]
    return (widen_bf16(a) if c.dtype == "bf16" else a)[:, c.offset:c.offset + c.C]


def window(name):
    """the fp32 window [R, C] of a case, widened"""
    return _window(BY_NAME[name], make(name))


def gather_targets(c, d, mut=None):
    """the emulation's reading of the id buffer: numpy index arithmetic"""
    _, base, seq, step = id_geometry(c)
    r = np.arange(rows_of(c))
    if mut == "step_not_reversed" and step < 0:
        base, step = base + (c.S - 1) * step, -step
    return d["ids"][base + (r // c.S) * seq + (r % c.S) * step].astype(np.int64)


# ---- the emulation: all rows of a case at once ------------------------------------------------------------------------------------------------------
def xent_rows(l, targets, *, z=0.0, scale=None, V=None, offset=0, row=None, bf16=False, mut=None, factor_ulps=0):
    """l fp32 [R, C] (the window); targets int64 [R]; scale fp32 [R] or None -> Out.  The gradient buffer [R, row] starts as SENT everywhere; columns [0, V) of
    every row are written.  factor_ulps moves the fp32 factor (float) (1 + 2 z L) by that many units in the last place: what a device logarithm one place off
    before the one rounding could give."""
    l = np.asarray(l, dtype=f32)
    R, C = l.shape
    V = offset + C if V is None else V
    row = V if row is None else row
    z = f32(z)
    t = np.asarray(targets, dtype=np.int64)
    bad = np.isnan(l).any(1) | (l == np.inf).any(1) | (l == -np.inf).all(1) | (t >= C)
    ignored = ~bad & (t < 0)
    grad = np.full((R, row), SENT, f32)
    nll, lse, q_total = np.full(R, NAN32, f32), np.full(R, NAN32, f32), np.zeros(R, u64)
    a_out, p_out = np.zeros(R, f32), np.zeros((R, C), f32)
    n_live = C - C % 4 if mut == "tail_chunk_dropped" else C       # the codes a kernel without its partial chunk would see
    grad[bad if mut == "ignored_unwritten" else bad | ignored, :V] = 0.0
    gi = np.flatnonzero(~bad)
    if gi.size:
        lg = np.where(l[gi] == 0, f32(0.0), l[gi])                  # -0.0 counts as +0.0
        m = lg.max(1)
        with np.errstate(invalid="ignore"):
            _, q = weight((lg - m[:, None]).astype(f32))
        q = q.copy()
        q[:, n_live:] = 0
        Q = q.sum(1, dtype=u64)
        log_z = np.asarray([math.log(int(v) * 2.0 ** -32) if v else -math.inf for v in Q], f64)      # the one library call, a scalar at a time (Q = 0: a planted mistake only)
        L = log_z if mut == "lse_without_m" else m.astype(f64) + log_z
        lse[gi], q_total[gi] = L.astype(f32), Q
        tg = t[gi]
        sc = tg >= 0
        ti, rows = np.where(sc, tg, 0), np.arange(gi.size)
        lt = lg[rows, ti]
        nll[gi] = np.where(sc, (-((lt.astype(f64) - m.astype(f64)) - log_z)).astype(f32), f32(0.0))
        g = np.ones(gi.size, f32) if scale is None else np.asarray(scale, f32)[gi]
        twice = (1.0 if mut == "z_without_2" else 2.0) * float(z)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            factor = (1.0 + twice * L).astype(f32)
            if factor_ulps:
                factor = np.nextafter(factor, f32(np.inf if factor_ulps > 0 else -np.inf))
            a = (g * factor).astype(f32)
            inv = np.full(gi.size, 2.0 ** -32) if mut == "p_unnormalised" else np.divide(1.0, Q.astype(f64))
            p = (q.astype(f64) * inv[:, None]).astype(f32)
            row_g = (a[:, None] * p).astype(f32)
            at = row_g[rows, ti]
            if mut == "scale_on_p_only":                            # g reaches the softmax term, the one-hot stays unscaled
                row_g[rows, ti] = at - f32(1.0)
            elif mut == "target_p_minus_1":
                row_g[rows, ti] = (p[rows, ti] - f32(1.0)) * a
            elif mut != "target_without_offset":
                row_g[rows, ti] = at - g
            a_out[gi], p_out[gi] = a, p
            si = gi[sc]                                             # the scored rows: the formula's
            if mut != "outside_unwritten":
                grad[si, :offset] = 0.0
                grad[si, offset + C:V] = 0.0
            grad[si, offset:offset + n_live] = row_g[sc][:, :n_live]
            if mut == "target_without_offset":                      # the one-hot lands at buffer column t, not offset + t
                grad[si, ti[sc]] = grad[si, ti[sc]] - g[sc]
    if bf16:
        grad = narrow(grad, truncate=mut == "bf16_truncated")
    return Out(nll, lse, q_total, grad, bad, ignored, a_out, p_out)


# ---- the second formulation: one row, Python integers and floats, flat buffers -------------------------------------------------------------------------
def _round32(xs):
    return np.asarray(xs, dtype=f64).astype(f32)


def xent_row_brute(c, d, r, mut=None):
    """-> (nll fp32, lse fp32, Q_total, the row of the gradient buffer as fp32 values or bf16 bits [row], bad, ignored).  Every address is computed here, from
    the flat buffers; Q_total is a Python integer sum; p, a p and the factor go through Python floats (fp64) and ONE conversion to fp32 each -- the product of
    two fp32 values is exact in fp64, so that conversion is the fp32 product's rounding.  The planted mistakes are written a second time, independently."""
    C, off, V, rowlen = c.C, c.offset, c.V, c.row
    flat = d["logits"].reshape(-1)
    cut = flat[r * rowlen + off:r * rowlen + off + C]
    vals = (widen_bf16(cut) if c.dtype == "bf16" else cut).astype(f32)
    _, base, seq, step = id_geometry(c)
    b, st = divmod(r, c.S)
    if mut == "step_not_reversed" and step < 0:
        st = c.S - 1 - st
    t = int(d["ids"][base + b * seq + st * step])
    buf = [float(SENT)] * rowlen
    pv = vals.tolist()
    is_bad = any(math.isnan(v) or v == math.inf for v in pv) or all(v == -math.inf for v in pv) or t >= C

    def finish(nll, lse, Q, ign):
        arr = np.asarray(buf, dtype=f64).astype(f32)
        if c.dtype == "bf16":
            arr = (arr.view(u32) >> u32(16)).astype(np.uint16) if mut == "bf16_truncated" else to_bf16_bits(arr)
        return (f32(nll), f32(lse), Q, arr, is_bad, ign)

    if is_bad or (t < 0 and mut != "ignored_unwritten"):
        buf[:V] = [0.0] * V
    if is_bad:
        return finish(NAN32, NAN32, 0, False)
    m = max(0.0 if v == 0 else v for v in pv)
    with np.errstate(invalid="ignore"):
        _, qq = weight((np.where(vals == 0, f32(0.0), vals) - f32(m)).astype(f32))
    q = [int(v) for v in qq.tolist()]
    live = C // 4 * 4 if mut == "tail_chunk_dropped" else C
    Q = sum(q[:live])
    log_z = math.log(Q / 2 ** 32) if Q else -math.inf             # Q = 0: under a planted mistake only
    L = log_z + (0.0 if mut == "lse_without_m" else m)
    if t < 0:
        return finish(0.0, L, Q, True)
    lt = 0.0 if pv[t] == 0 else pv[t]
    nll = -((lt - m) - log_z)
    g = 1.0 if d["scale"] is None else float(d["scale"][r])
    zz = float(c.z)
    factor = float(f32(1.0 + (zz if mut == "z_without_2" else 2.0 * zz) * L))
    a = float(f32(g * factor))
    inv = 1.0 / float(Q) if Q else math.inf
    p = _round32([qi * (2.0 ** -32 if mut == "p_unnormalised" else inv) for qi in q]).tolist()
    ap = _round32([a * pi for pi in p])
    with np.errstate(invalid="ignore", over="ignore"):
        if mut == "target_p_minus_1":
            ap[t] = f32(f32(p[t]) - f32(1.0)) * f32(a)
        elif mut == "scale_on_p_only":
            ap[t] = ap[t] - f32(1.0)
        elif mut != "target_without_offset":
            ap[t] = ap[t] - f32(g)
    if mut != "outside_unwritten":
        for i in list(range(0, off)) + list(range(off + C, V)):
            buf[i] = 0.0
    apl = ap.tolist()
    for i in range(live):
        buf[off + i] = apl[i]
    if mut == "target_without_offset":
        buf[t] = float(f32(buf[t]) - f32(g))
    return finish(nll, L, Q, False)


BRUTE_BIG_ROWS = 2


def brute_rows(c):
    """the rows the second formulation walks: all of them up to 64 (two of them where a row is longer than 20000 codes), else the first, the last and a spread"""
    R = rows_of(c)
    if c.C > 20000:
        return sorted({0, R - 1})
    if R <= 64:
        return list(range(R))
    return sorted(set(list(range(8)) + list(range(R - 8, R)) + [GRID_X - 1, min(GRID_X, R - 1)] + list(range(0, R, R // 8))))


_REF = {}


def reference(name, mut=None, brute=False, factor_ulps=0):
    """the emulation: Out over all rows.  brute=True: {row: tuple} over brute_rows.  Computed once and shared: treat as read-only."""
    k = (name, mut, brute, factor_ulps)
    if k in _REF:
        return _REF[k]
    c, d = BY_NAME[name], make(name)
    if not brute:
        out = xent_rows(window(name), gather_targets(c, d, mut), z=c.z, scale=d["scale"], V=c.V, offset=c.offset, row=c.row, bf16=c.dtype == "bf16", mut=mut,
                        factor_ulps=factor_ulps)
    else:
        out = {r: xent_row_brute(c, d, r, mut) for r in brute_rows(c)}
    _REF[k] = out
    return out


def row_tuple(out, r):
    return (f32(out.nll[r]).tobytes(), f32(out.lse[r]).tobytes(), int(out.q_total[r]), out.grad[r].tobytes(), bool(out.bad[r]), bool(out.ignored[r]))


def brute_tuple(t):
    return (f32(t[0]).tobytes(), f32(t[1]).tobytes(), int(t[2]), t[3].tobytes(), bool(t[4]), bool(t[5]))


def same(name, a, b):
    """two results of a case over the rows the brute force walks (either kind each): every output equal, floats bit for bit, the whole gradient buffer row"""
    rows = brute_rows(BY_NAME[name])
    ta = [brute_tuple(a[r]) if isinstance(a, dict) else row_tuple(a, r) for r in rows]
    tb = [brute_tuple(b[r]) if isinstance(b, dict) else row_tuple(b, r) for r in rows]
    return ta == tb


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------------------------
MUTS = ("target_p_minus_1", "z_without_2", "lse_without_m", "p_unnormalised", "scale_on_p_only", "target_without_offset", "step_not_reversed",
        "ignored_unwritten", "outside_unwritten", "bf16_truncated", "tail_chunk_dropped")


def needs(mut, c):
    """what a case must have for a mistake to be able to move it at all (necessary, not sufficient)"""
    return {"target_p_minus_1": True, "z_without_2": c.z != 0, "lse_without_m": True, "p_unnormalised": True, "scale_on_p_only": c.scale is not None,
            "target_without_offset": c.offset != 0, "step_not_reversed": c.step < 0 and c.S > 1, "ignored_unwritten": c.tk == "ignored",
            "outside_unwritten": c.offset != 0 or c.V > c.offset + c.C, "bf16_truncated": c.dtype == "bf16", "tail_chunk_dropped": c.C % 4 != 0}[mut]


def applies(mut, name):
    """does the mistake move the case?  Decided by the brute-force formulation, where every mistake is written a second time."""
    return not same(name, reference(name, brute=True), reference(name, mut=mut, brute=True))


# ---- the derived bounds against fp64 -----------------------------------------------------------------------------------------------------
def delta_q(C):
    """the relative error of Q_total: 2^-21 on each mass, the fp32 rounding of d = l - m (|d| <= 24, so 24 * 2^-24 on exp(d)), under one unit of truncation per
    code against Q >= 2^32, and the tail below -24 dropped (e^-24 per code against a sum >= 1) -- the scorer's"""
    return 2.0 ** -21 + 24 * 2.0 ** -24 + C * (2.0 ** -32 + math.exp(-24.0))


def bound_row_scalar(C, value):
    """|nll - fp64| and |lse - fp64|: the relative error of Q through the logarithm, the one rounding to fp32, 1e-12 for the fp64 log and the reference's sums"""
    dq = delta_q(C)
    return dq / (1 - dq) + abs(value) * 2.0 ** -24 + 1e-12


def bound_grad(C, p, a, g, z, L, onehot, bf16=False):
    """elementwise |grad_i - fp64| for one row; p [C], a, g, L the fp64 values.  p_i = q_i / Q: the mass's 2^-21 and the rounding of d on q_i, the relative
    error of Q on the quotient, one truncation unit 2^-32 and the dropped tail e^-24 absolutely, the rounding to fp32.  a = g (1 + 2 z L): 2 z times the error
    of L, the rounding of the factor, the fp32 product.  Then the fp32 product a p and the fp32 difference, half an ulp each of a value of at most |a| p + |g|;
    bf16 output: half an ulp of bf16, at most 2^-8 of the value and its error."""
    dq = delta_q(C)
    dl = dq / (1 - dq)
    dp = p * ((2.0 ** -21 + 24 * 2.0 ** -24 + dq) / (1 - dq) + 2.0 ** -24) + 2.0 ** -32 + math.exp(-24.0)
    da = abs(g) * (2 * z * dl + abs(1 + 2 * z * L) * 2.0 ** -24) + abs(a) * 2.0 ** -24
    size = abs(a) * p + abs(g) * onehot
    e = abs(a) * dp + da * (p + dp) + 2 * size * 2.0 ** -24 + 1e-12
    return e + ((size + e) * 2.0 ** -8 if bf16 else 0.0)
