"""The token policy loss's arithmetic of record in numpy float32 / uint64 / float64 (include/selftok_hip_ext.h states it; csrc/token_policy.hip runs it), a
second, brute-force formulation (a Python loop per row over Python integers and floats, math.exp / math.expm1, its own address arithmetic into the flat
logits, id and gradient buffers), the case table and the planted mistakes -- shared by tests/test_token_policy_cpu.py and tests/test_token_policy_gpu.py.

The key, the maximum and the integer mass are the sampler's and are IMPORTED from tests/token_sample_cases.py; the id addressing, the row scales, the bf16
rounding and the bounds of the softmax gradient are the loss's and are imported from tests/token_xent_cases.py.  What is the policy loss's own: the ratio, the
clip, the k3 estimate, the coefficient, the entropy term of the gradient and the row kinds.

Launch geometry the table is built around: 512 threads own a row, a thread owns 4-code chunks t, t + 512, ..; C <= 4096 runs the 2-chunk kernels; WITHOUT the
entropy sum C <= 32768 runs the 16-chunk kernel, WITH it C <= 16384 the 8-chunk kernel; above that the streamed ones; the up to three codes past the last
whole chunk are thread 0's; the grid is min(R, 65536) x ceil(R / 65536) workgroups."""
import math
from collections import namedtuple

import numpy as np

import token_sample_cases as TC
import token_xent_cases as XC
from token_sample_cases import OFFSET_VLM, to_bf16_bits, weight, widen_bf16
from token_xent_cases import GRID_X, NAN32, POISON, SENT, gather_targets, id_geometry, narrow, row_scales

f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64
SMALL_C, ENT_C, REG_C = 4096, 16384, 32768
GEOMETRY_C = (2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385, 32767, 32768, 32769, 65536)
INF = float("inf")
ADV_CYCLE = (1.25, -0.5, 0.0)                                       # the advantages of the edge rows: A > 0, A < 0, A = 0

Case = namedtuple("Case", "name kind B S C dtype offset V row step ids wide tk scale old adv ref clip klc entc went")
Out = namedtuple("Out", "logprob lse ratio kl entropy coef flags grad bad ignored q q_total d E e u kH sc")


def _case(name, kind, B, C, S=1, dtype="f32", offset=0, vpad=0, pad=0, step=1, ids="int64", wide=False, tk="any", scale=None, old="near", adv="mix", ref=None,
          clip=(0.2, 0.2), klc=0.0, entc=0.0, went=False):
    V = offset + C + vpad
    row = V + pad
    row += (-row) % 4
    return Case(name, kind, B, S, C, dtype, offset, V, row, step, ids, wide, tk, scale, old, adv, ref, (f32(clip[0]), f32(clip[1])), f32(klc), f32(entc), went)


KL, EN = 0.04, 0.01
CASES = [
    _case("c1", "small", 1, 1, old="eq"),
    _case("c2_kl_rows", "small", 3, 2, ref="near", klc=KL, scale="rows"),
    _case("c3_R3_ent", "small", 3, 3, entc=EN),
    _case("c4_int32", "small", 5, 4, ids="int32", scale="const", ref="near", klc=KL, entc=EN),
    _case("c5_S3_rev", "small", 2, 5, S=3, step=-1, went=True),
    _case("c255_S40_kl_ent", "gauss1", 1, 255, S=40, scale="rows", ref="near", klc=KL, entc=EN),
    _case("c257_bf16_ent", "gauss1", 3, 257, dtype="bf16", entc=EN, scale="rows"),
    _case("c2047_kl", "gauss1", 3, 2047, ref="near", klc=KL),
    _case("c2048_bf16", "gauss1", 3, 2048, dtype="bf16", scale="const"),
    _case("c2049_g8_ent", "gauss8", 3, 2049, scale="rows", entc=EN, adv="neg"),
    _case("c2050_int32_wide", "gauss1", 2, 2050, S=3, ids="int32", wide=True, vpad=3, pad=5, adv="neg"),
    _case("c4095_stride_ent", "gauss1", 3, 4095, offset=4, vpad=1, pad=4, entc=EN, ref="near", klc=KL),
    _case("c4096_R64", "gauss1", 64, 4096, scale="rows", ref="near", klc=KL),
    _case("c4096_S40_rev_ent", "gauss1", 1, 4096, S=40, step=-1, entc=EN),
    _case("c4097_bf16_S40_wide_rev", "gauss1", 1, 4097, S=40, dtype="bf16", ids="int32", wide=True, step=-1),
    _case("c4097_ent_kl", "gauss1", 3, 4097, entc=EN, ref="near", klc=KL, scale="rows"),
    _case("c16383_ent", "gauss1", 3, 16383, entc=EN, scale="rows"),
    _case("c16384_bf16_ent_kl", "gauss1", 3, 16384, dtype="bf16", entc=EN, ref="near", klc=KL),
    _case("c16385_ent", "gauss8", 3, 16385, entc=EN, adv="neg"),
    _case("c16385_went", "gauss1", 1, 16385, went=True),
    _case("c32767_g8_kl", "gauss8", 3, 32767, ref="near", klc=KL, scale="rows", adv="neg"),
    _case("c32768_vlm", "gauss1", 1, 32768, S=3, step=-1, offset=OFFSET_VLM, scale="const"),
    _case("c32768_bf16_g8_ent", "gauss8", 3, 32768, dtype="bf16", entc=EN),
    _case("c32769_kl", "gauss1", 3, 32769, scale="rows", ref="near", klc=KL),
    _case("c32769_bf16_ent", "gauss1", 1, 32769, dtype="bf16", vpad=2, pad=8, entc=EN),
    _case("c32770_vlm_ent", "gauss1", 1, 32770, S=3, offset=OFFSET_VLM, vpad=5, pad=3, entc=EN, ref="near", klc=KL),
    _case("c65536_g8", "gauss8", 3, 65536, scale="rows", adv="neg"),
    _case("c65536_bf16_ent", "gauss1", 1, 65536, dtype="bf16", pad=8, entc=EN),
    _case("c1000_bf16_vlm_wide_rev", "gauss1", 2, 1000, S=3, step=-1, dtype="bf16", offset=OFFSET_VLM, vpad=6, pad=24, wide=True, scale="rows", ref="near", klc=KL, entc=EN),
    _case("edge", "boost", 18, 1000, tk="any", old="edge", adv="cycle", ref="near", klc=KL),
    _case("edge_asym_ent", "boost", 18, 4100, tk="any", old="edge", adv="cycle", clip=(0.1, 0.28), entc=EN, scale="rows"),
    _case("edge_bf16", "boost", 18, 300, dtype="bf16", tk="any", old="edge", adv="cycle"),
    _case("on_policy", "gauss1", 6, 1000, old="eq", ref="eq", klc=KL, scale="rows"),
    _case("on_policy_ent_bf16", "gauss1", 6, 4097, dtype="bf16", old="eq", ref="eq", klc=KL, entc=EN),
    _case("ratio_overflows", "gauss1", 6, 1000, old="huge", adv="cycle", ref="near", klc=KL),
    _case("target_neginf", "gauss_neginf", 6, 257, tk="neginf", scale="rows", old="neginf_ops", adv="cycle"),
    _case("target_neginf_ref", "gauss_neginf", 6, 257, tk="neginf", old="neginf_ops", adv="cycle", ref="neginf_ops", klc=KL, entc=EN),
    _case("target_neginf_c32768", "gauss_neginf", 6, 32768, tk="neginf", old="neginf_ops", adv="cycle", scale="rows"),
    _case("target_neginf_ref_stream_ent_bf16", "gauss_neginf", 6, 16392, dtype="bf16", tk="neginf", old="neginf_ops", adv="cycle", ref="neginf_ops", klc=KL, entc=EN),
    _case("target_far_below", "gauss8", 6, 2049, tk="lowest", entc=EN, adv="cycle"),
    _case("ignored_kl", "gauss1", 2, 1000, S=3, tk="ignored", vpad=4, ref="near", klc=KL),
    _case("ignored_int32_rev_bf16_ent", "gauss1", 2, 300, S=3, step=-1, ids="int32", dtype="bf16", tk="ignored", scale="rows", offset=8, entc=EN),
    _case("ignored_c5000_ent", "gauss1", 1, 5000, S=3, tk="ignored", entc=EN),
    _case("ignored_c5000", "gauss1", 1, 5000, S=3, dtype="bf16", tk="ignored"),
    _case("ignored_stream", "gauss1", 1, 32771, S=3, tk="ignored"),
    _case("ignored_stream_ent", "gauss1", 1, 16390, S=3, tk="ignored", entc=EN),
    _case("bad_rows_c4100", "bad", 9, 4100, vpad=1, tk="badtargets", scale="const", ref="near", klc=KL),
    _case("bad_rows_ent", "bad", 9, 1000, tk="badtargets", entc=EN, scale="rows"),
    _case("bad_rows_ent_c5000", "bad", 9, 5000, tk="badtargets", entc=EN, ref="near", klc=KL, scale="rows"),
    _case("bad_rows_bf16", "bad", 9, 256, dtype="bf16", offset=8, vpad=2, pad=4, tk="badtargets"),
    _case("bad_rows_stream", "bad", 9, 32770, offset=4, vpad=3, tk="badtargets", ids="int32"),
    _case("bad_rows_stream_ent", "bad", 9, 16388, tk="badtargets", entc=EN),
    _case("bad_operands", "gauss1", 9, 1000, old="badops", ref="badops", klc=KL, scale="rows"),
    _case("bad_operands_ent_c5000", "gauss1", 9, 5000, old="badops", entc=EN),
    _case("bad_operands_stream_bf16", "gauss1", 9, 32772, dtype="bf16", old="badops", ref="badops", klc=KL),
    _case("bad_operands_ent_c300_bf16", "gauss1", 9, 300, dtype="bf16", old="badops", ref="badops", klc=KL, entc=EN, scale="rows"),
    _case("bad_operands_c5000", "gauss1", 9, 5000, old="badops"),
    _case("bad_operands_stream_ent", "gauss1", 9, 16392, old="badops", entc=EN, scale="rows"),
    _case("grid_second_row", "small", 1, 5, S=GRID_X + 1, step=-1, scale="const", ref="near", klc=KL),
]
BY_NAME = {c.name: c for c in CASES}
_CACHE = {}


def rows_of(c):
    return c.B * c.S


def clip_bounds(c):
    """(lo, hi) in fp32, as the kernel forms them"""
    return f32(1.0) - f32(c.clip[0]), f32(1.0) + f32(c.clip[1])


def edge_targets(c):
    """the six ratios an edge case places: one fp32 ulp below lo, lo, one above; one below hi, hi, one above"""
    lo, hi = clip_bounds(c)
    return [np.nextafter(lo, f32(0)), lo, np.nextafter(lo, f32(2)), np.nextafter(hi, f32(0)), hi, np.nextafter(hi, f32(2))]


def _step_ulps(x, k):
    """fp32 x moved by k units in the last place (x != 0, no sign change in the table's use)"""
    return (np.asarray(x, f32).view(np.int32) + np.int32(k if x > 0 else -k)).view(f32)


def find_old(lp, rho):
    """an fp32 old_logprob whose exactly representable difference to the fp32 lp gives (float) exp(lp - old) == rho, by search on the emulation's exp"""
    base = f32(float(lp) - math.log(float(rho)))
    for k in sorted(range(-400, 401), key=abs):
        cand = f32(_step_ulps(base, k)) if base != 0 else f32(k * 2.0 ** -40)
        if f32(math.exp(float(lp) - float(cand))) == rho:
            return cand
    raise AssertionError(("no old_logprob gives the ratio", float(lp), float(rho)))


def make(name):
    """-> dict(logits [R, row] (NaN outside the window, bf16 as uint16 bits), ids (the 1-D id buffer), targets int64 [R], scale, old, adv, ref fp32 [R] or None).
    Built once per case and shared: treat as read-only."""
    if name in _CACHE:
        return _CACHE[name]
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 38)
    R, C = rows_of(c), c.C
    sigma = 8.0 if c.kind == "gauss8" else 1.0
    w = (rng.standard_normal((R, C)) * sigma).astype(f32)
    t = rng.integers(0, C, size=R).astype(np.int64)
    r = np.arange(R)
    if c.kind == "boost":                                           # the target holds most of the mass: |logprob| < 1, so an fp32 step of old_logprob moves the ratio by less than its ulp
        w[r, t] += f32(12.0)
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
    if c.tk == "neginf":
        t = np.where(r % 2 == 0, (t // 5) * 5, np.where(t % 5 == 0, (t + 1) % C, t))        # every fifth code is -inf: on it, and beside it
        t = np.where((r % 2 == 1) & (t % 5 == 0), 1, t)
    elif c.tk == "lowest":                                          # the lowest logit of the row: more than 24 below the maximum at sigma 8
        t = np.argmin(l, axis=1).astype(np.int64)
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
    # the row operands: built around the emulation's own logprob
    with np.errstate(all="ignore"):
        lp = _scalars(l, t)["lp"]
    lp0 = np.where(np.isfinite(lp), lp, f32(-3.0)).astype(f32)
    if c.adv == "cycle":
        adv = np.asarray(ADV_CYCLE, f32)[(r // 6 if c.old == "edge" else r) % 3]
    else:
        adv = rng.standard_normal(R).astype(f32)
        if c.adv == "neg":                                          # mostly negative coefficients: -0.0 wherever a code has no mass
            adv = -np.abs(adv)
        adv[r % 5 == 3] = 0.0
    old = (lp0 - (rng.standard_normal(R) * 0.25).astype(f32)).astype(f32)
    if c.old == "eq":
        old = lp0.copy()
    elif c.old == "edge":
        tg = edge_targets(c)
        old = np.asarray([find_old(lp0[i], tg[i % 6]) for i in range(R)], f32)
    elif c.old == "huge":                                           # exp(100) is above the fp32 range
        old = (lp0 - f32(100.0)).astype(f32)
    ref = None
    if c.ref is not None:
        ref = lp0.copy() if c.ref == "eq" else (lp0 + (rng.standard_normal(R) * 0.2).astype(f32)).astype(f32)
    if c.old == "neginf_ops":                                       # rows 0, 2, 4 have their target at -inf: a finite old (ratio 0), then -inf against -inf
        old[2] = -np.inf
        if ref is not None:
            old[2], ref[4] = f32(-2.0), -np.inf
    if c.old == "badops":
        adv[1], adv[3], old[2], old[5] = np.nan, -np.inf, np.nan, np.inf
        if ref is not None:
            ref[6], ref[7] = np.nan, np.inf
        else:
            adv[6], old[7] = np.inf, np.nan
    d["old"], d["adv"], d["ref"] = old, adv.astype(f32), ref
    _CACHE[name] = d
    return d


def _window(c, d):
    a = d["logits"]
    return (widen_bf16(a) if c.dtype == "bf16" else a)[:, c.offset:c.offset + c.C]


def window(name):
    return _window(BY_NAME[name], make(name))


# ---- the emulation: all rows of a case at once ------------------------------------------------------------------------------------------------------
def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def _expm1(x):
    try:
        return math.expm1(x)
    except OverflowError:
        return INF


def _scalars(l, t, n_live=None):
    """steps 3 - 4 and the two fp64 row values every output starts from -> dict over all rows (NaN / 0 on rows the LOSS calls bad)"""
    l = np.asarray(l, f32)
    R, C = l.shape
    n_live = C if n_live is None else n_live
    bad = np.isnan(l).any(1) | (l == np.inf).any(1) | (l == -np.inf).all(1) | (t >= C)
    lz = np.where(l == 0, f32(0.0), l)                              # -0.0 counts as +0.0
    m = np.where(bad, f32(0.0), np.where(np.isnan(lz), -np.inf, lz).max(1)).astype(f32)
    with np.errstate(invalid="ignore"):
        d = (lz - m[:, None]).astype(f32)
        _, q = weight(d)
    q = q.copy()
    q[:, n_live:] = 0
    q[bad] = 0
    Q = q.sum(1, dtype=u64)
    dd = np.where(q > 0, d, f32(0.0))
    h = np.trunc(q.astype(f64) * (-dd).astype(f64) * 65536.0).astype(u64)
    S = h.sum(1, dtype=u64)
    Lq = np.asarray([math.log(int(v) * 2.0 ** -32) if v else -INF for v in Q], f64)
    E = np.asarray([float(int(s)) / (65536.0 * float(int(v))) if v else 0.0 for s, v in zip(S, Q)], f64)
    ti = np.where((t >= 0) & ~bad, t, 0)
    lt = lz[np.arange(R), ti]
    with np.errstate(invalid="ignore"):
        lp64 = (lt.astype(f64) - m.astype(f64)) - Lq
    return dict(bad=bad, m=m, d=d, q=q, Q=Q, Lq=Lq, E=E, lt=lt, lp64=lp64, lp=lp64.astype(f32), lse=(m.astype(f64) + Lq).astype(f32), H=(Lq + E).astype(f32))


def coef_of(adv, ratio, flags, klc, e, g, mut=None):
    """k = g * (float) W for one row, from the ratio and the clip outcome GIVEN (the GPU test hands in the device's)"""
    clipped = flags != 0 and mut != "clipped_keeps_coef"
    with np.errstate(all="ignore"):
        policy = 0.0 if (clipped or adv == 0) else float(adv) * float(ratio)
        W = policy + (0.0 if mut == "kl_missing_from_coef" else float(klc)) * e
        return f32(f32(g) * f32(W))


def flags_of(adv, ratio, lo, hi, mut=None):
    c_hi = (adv >= 0 if mut == "clip_ge" else adv > 0) and ratio > hi
    c_lo = adv < 0 and ratio < lo
    return int(c_hi) | int(c_lo) << 1


def gradient(c, sc, targets, k, kH, live, bad, ignored, mut=None):
    """the gradient buffer [R, row] (fp32, or bf16 bits) of a case from the row coefficients GIVEN: k, kH fp32 [R]; sc the dict of `_scalars`; live: the
    scored rows.  Starts as SENT everywhere; columns [0, V) of every row are written."""
    R, C = sc["q"].shape
    grad = np.full((R, c.row), SENT, f32)
    n_live = C - C % 4 if mut == "tail_chunk_dropped" else C
    grad[bad if mut == "ignored_unwritten" else bad | ignored, :c.V] = 0.0
    si = np.flatnonzero(live)
    if si.size:
        q, Q, d = sc["q"][si], sc["Q"][si], sc["d"][si]
        t = targets[si]
        rows = np.arange(si.size)
        kk, hh = np.asarray(k, f32)[si], np.asarray(kH, f32)[si]
        with np.errstate(all="ignore"):
            pd = q.astype(f64) * np.divide(1.0, Q.astype(f64))[:, None]
            p = pd.astype(f32)
            x = (kk[:, None] * p).astype(f32)
            if mut == "target_p_minus_1":
                x[rows, t] = ((p[rows, t] - f32(1.0)).astype(f32) * kk).astype(f32)
            else:
                x[rows, t] = (x[rows, t] - kk).astype(f32)
            if c.entc != 0 or mut == "ent_added_at_zero":
                shift = -sc["Lq"][si] if mut == "ent_grad_without_H" else sc["E"][si]
                tt = np.where(q > 0, (pd * (d.astype(f64) + shift[:, None])).astype(f32), f32(0.0))
                x = (x + (hh[:, None] * tt).astype(f32)).astype(f32)
        grad[si, :c.offset] = 0.0
        grad[si, c.offset + C:c.V] = 0.0
        grad[si, c.offset:c.offset + n_live] = x[:, :n_live]
    return narrow(grad) if c.dtype == "bf16" else grad


def policy_rows(c, d, mut=None, want_grad=True):
    """the emulation of one case -> Out"""
    l = _window(c, d)
    R, C = l.shape
    t = gather_targets(c, d)
    sc = _scalars(l, t, C - C % 4 if mut == "tail_chunk_dropped" else C)
    old, adv, ref = d["old"], d["adv"], d["ref"]
    has_t = ~sc["bad"] & (t >= 0)
    lp_ninf = has_t & (sc["lt"] == -np.inf)
    bad_ops = ~np.isfinite(adv) | np.isnan(old) | (old == np.inf) | (lp_ninf & (old == -np.inf))
    if ref is not None:
        bad_ops |= np.isnan(ref) | (ref == np.inf) | (lp_ninf & (ref == -np.inf))
    bad = sc["bad"] | (has_t & bad_ops)
    ignored = ~bad & (t < 0)
    live = ~bad & ~ignored
    lo, hi = clip_bounds(c)
    g = np.ones(R, f32) if d["scale"] is None else d["scale"]
    nan = np.full(R, NAN32, f32)
    logprob, lse, ratio, kl, ent, coef = (np.where(bad, nan, f32(0.0)).astype(f32) for _ in range(6))
    lse = np.where(bad, nan, sc["lse"]).astype(f32)
    flags, e_all, u_all = np.zeros(R, np.uint8), np.zeros(R, f64), np.zeros(R, f64)
    kH = np.zeros(R, f32)
    with np.errstate(all="ignore"):
        for r in np.flatnonzero(live):
            lp = sc["lp"][r]
            diff = (float(sc["lp64"][r]) if mut == "ratio_from_f64_lp" else float(lp)) - float(old[r])
            rt = f32(_exp(diff))
            fl = flags_of(adv[r], rt, lo, hi, mut)
            e = u = 0.0
            k3 = f32(0.0)
            if ref is not None:
                u = (float(lp) - float(ref[r])) if mut == "k3_sign" else (float(ref[r]) - float(lp))
                e = _expm1(u)
                k3 = f32(e - u)
            logprob[r], ratio[r], kl[r], flags[r], e_all[r], u_all[r] = lp, rt, k3, fl, e, u
            coef[r] = coef_of(adv[r], rt, fl, c.klc, e, g[r], mut)
            kH[r] = f32(c.entc) if mut == "scale_not_on_ent" else f32(g[r] * f32(c.entc))
            ent[r] = sc["H"][r]
    entropy = ent if (c.entc != 0 or c.went) else None
    grad = gradient(c, sc, t, coef, kH, live, bad, ignored, mut) if want_grad else None
    return Out(logprob, lse, ratio, kl, entropy, coef, flags, grad, bad, ignored, sc["q"], sc["Q"], sc["d"], sc["E"], e_all, u_all, kH, sc)


# ---- the second formulation: one row, Python integers and floats, flat buffers -------------------------------------------------------------------------
def _r32(x):
    with np.errstate(all="ignore"):
        return float(f32(x))


def policy_row_brute(c, d, r, mut=None):
    """-> (logprob, lse, ratio, kl, entropy or None, coef -- fp32 -- flags, the row of the gradient buffer as fp32 values or bf16 bits [row], bad, ignored).  Every
    address is computed here from the flat buffers; Q and S are Python integer sums; every fp32 operation is a Python float (fp64) operation on fp32 values --
    exact for a product, and for a sum of two fp32 values within 2^53 of each other's scale, else computed in numpy fp32 -- and ONE conversion to fp32.  The planted
    mistakes are written a second time, independently."""
    C, off, V, rowlen = c.C, c.offset, c.V, c.row
    flat = d["logits"].reshape(-1)
    cut = flat[r * rowlen + off:r * rowlen + off + C]
    vals = (widen_bf16(cut) if c.dtype == "bf16" else cut).astype(f32)
    _, base, seq, step = id_geometry(c)
    b, st = divmod(r, c.S)
    t = int(d["ids"][base + b * seq + st * step])
    buf = [float(SENT)] * rowlen
    pv = vals.tolist()
    want_ent = c.entc != 0 or c.went
    A, old = float(d["adv"][r]), float(d["old"][r])
    ref = None if d["ref"] is None else float(d["ref"][r])
    is_bad = any(math.isnan(v) or v == INF for v in pv) or all(v == -INF for v in pv) or t >= C
    if not is_bad and t >= 0:
        is_bad = math.isnan(A) or math.isinf(A) or math.isnan(old) or old == INF or (ref is not None and (math.isnan(ref) or ref == INF))
        if pv[t] == -INF and (old == -INF or ref == -INF):
            is_bad = True

    def finish(lp, lse, ratio, kl, H, k, fl, ign):
        arr = np.asarray(buf, dtype=f64).astype(f32)
        if c.dtype == "bf16":
            arr = to_bf16_bits(arr)
        return (f32(lp), f32(lse), f32(ratio), f32(kl), f32(H) if want_ent else None, f32(k), fl, arr, is_bad, ign)

    if is_bad or (t < 0 and mut != "ignored_unwritten"):
        buf[:V] = [0.0] * V
    if is_bad:
        return finish(NAN32, NAN32, NAN32, NAN32, NAN32, NAN32, 0, False)
    m = max(0.0 if v == 0 else v for v in pv)
    with np.errstate(invalid="ignore"):
        dv = (np.where(vals == 0, f32(0.0), vals) - f32(m)).astype(f32)
        _, qq = weight(dv)
    live = C // 4 * 4 if mut == "tail_chunk_dropped" else C
    q = [int(v) for v in qq.tolist()[:live]] + [0] * (C - live)
    dl = dv.tolist()
    Q = sum(q)
    S = sum(int(float(qi) * -di * 65536.0) for qi, di in zip(q, dl) if qi > 0)
    Lq = math.log(Q / 2 ** 32) if Q else -INF                       # Q = 0: under a planted mistake only
    E = S / (65536.0 * Q) if Q else 0.0
    lse = m + Lq
    if t < 0:
        return finish(0.0, lse, 0.0, 0.0, 0.0, 0.0, 0, True)
    lt = 0.0 if pv[t] == 0 else pv[t]
    lp64 = (lt - m) - Lq
    lp = _r32(lp64)
    ratio = _r32(_exp((lp64 if mut == "ratio_from_f64_lp" else lp) - old))
    lo, hi = (float(v) for v in clip_bounds(c))
    c_hi = (A >= 0 if mut == "clip_ge" else A > 0) and ratio > hi
    c_lo = A < 0 and ratio < lo
    e = u = kl = 0.0
    with np.errstate(all="ignore"):
        if ref is not None:
            u = lp - ref if mut == "k3_sign" else ref - lp
            e = _expm1(u)
            kl = e - u if not (math.isinf(e) and math.isinf(u)) else math.nan
        clipped = (c_hi or c_lo) and mut != "clipped_keeps_coef"
        policy = 0.0 if (clipped or A == 0) else A * ratio
        kterm = (0.0 if mut == "kl_missing_from_coef" else float(c.klc)) * e if not (math.isinf(e) and (mut == "kl_missing_from_coef" or c.klc == 0)) else math.nan
        W = policy + kterm
        g = 1.0 if d["scale"] is None else float(d["scale"][r])
        k = _r32(g * _r32(W))
        kH = float(c.entc) if mut == "scale_not_on_ent" else _r32(g * float(c.entc))
        inv = 1.0 / float(Q) if Q else INF
        pd = [qi * inv for qi in q]
        p = np.asarray(pd, f64).astype(f32)
        x = (f32(k) * p).astype(f32)
        if mut == "target_p_minus_1":
            x[t] = f32(f32(p[t] - f32(1.0)) * f32(k))
        else:
            x[t] = f32(x[t] - f32(k))
        if c.entc != 0 or mut == "ent_added_at_zero":
            shift = -Lq if mut == "ent_grad_without_H" else E
            tt = np.asarray([pi * (di + shift) if qi > 0 else 0.0 for pi, di, qi in zip(pd, dl, q)], f64).astype(f32)
            x = (x + (f32(kH) * tt).astype(f32)).astype(f32)
    for i in list(range(0, off)) + list(range(off + C, V)):
        buf[i] = 0.0
    xl = x.astype(f64).tolist()
    for i in range(live):
        buf[off + i] = xl[i]
    return finish(lp, lse, ratio, kl, Lq + E, k, int(c_hi) | int(c_lo) << 1, False)


def brute_rows(c):
    """the rows the second formulation walks: all of them up to 64 (two where a row is longer than 20000 codes), else the first, the last and a spread"""
    R = rows_of(c)
    if c.C > 20000:
        return sorted({0, R - 1})
    if R <= 64:
        return list(range(R))
    return sorted(set(list(range(8)) + list(range(R - 8, R)) + [GRID_X - 1, min(GRID_X, R - 1)] + list(range(0, R, R // 8))))


_REF = {}


def reference(name, mut=None, brute=False):
    """the emulation: Out over all rows.  brute=True: {row: tuple} over brute_rows.  Computed once and shared: treat as read-only."""
    k = (name, mut, brute)
    if k not in _REF:
        c, d = BY_NAME[name], make(name)
        _REF[k] = {r: policy_row_brute(c, d, r, mut) for r in brute_rows(c)} if brute else policy_rows(c, d, mut)
    return _REF[k]


def _fb(v):
    return None if v is None else f32(v).tobytes()


def row_tuple(out, r):
    return (_fb(out.logprob[r]), _fb(out.lse[r]), _fb(out.ratio[r]), _fb(out.kl[r]), None if out.entropy is None else _fb(out.entropy[r]), _fb(out.coef[r]), int(out.flags[r]),
            out.grad[r].tobytes(), bool(out.bad[r]), bool(out.ignored[r]))


def brute_tuple(t):
    return (_fb(t[0]), _fb(t[1]), _fb(t[2]), _fb(t[3]), _fb(t[4]), _fb(t[5]), int(t[6]), t[7].tobytes(), bool(t[8]), bool(t[9]))


def _canon(tp):
    """NaN payloads and signs are not part of the record"""
    nan = lambda b: b if b is None or not np.isnan(np.frombuffer(b, f32)[0]) else b"nan"
    return tuple(nan(v) if isinstance(v, bytes) and len(v) == 4 else v for v in tp)


def same(name, a, b):
    """two results of a case over the rows the brute force walks (either kind each): every output equal, floats bit for bit, the whole gradient buffer row"""
    rows = brute_rows(BY_NAME[name])
    ta = [_canon(brute_tuple(a[r]) if isinstance(a, dict) else row_tuple(a, r)) for r in rows]
    tb = [_canon(brute_tuple(b[r]) if isinstance(b, dict) else row_tuple(b, r)) for r in rows]
    return ta == tb


def differing_rows(name, a, b):
    rows = brute_rows(BY_NAME[name])
    return [r for r in rows if _canon(brute_tuple(a[r]) if isinstance(a, dict) else row_tuple(a, r)) != _canon(brute_tuple(b[r]) if isinstance(b, dict) else row_tuple(b, r))]


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------------------------
MUTS = ("ratio_from_f64_lp", "clip_ge", "clipped_keeps_coef", "k3_sign", "kl_missing_from_coef", "target_p_minus_1", "ent_grad_without_H", "ent_added_at_zero",
        "scale_not_on_ent", "ignored_unwritten", "tail_chunk_dropped")


def needs(mut, c):
    """what a case must have for a mistake to be able to move it at all (necessary, not sufficient)"""
    return {"ratio_from_f64_lp": True, "clip_ge": True, "clipped_keeps_coef": True, "k3_sign": c.ref is not None, "kl_missing_from_coef": c.klc != 0,
            "target_p_minus_1": True, "ent_grad_without_H": c.entc != 0, "ent_added_at_zero": c.entc == 0, "scale_not_on_ent": c.entc != 0 and c.scale is not None,
            "ignored_unwritten": c.tk == "ignored", "tail_chunk_dropped": c.C % 4 != 0}[mut]


def applies(mut, name):
    """does the mistake move the case?  Decided by the brute-force formulation, where every mistake is written a second time."""
    return not same(name, reference(name, brute=True), reference(name, mut=mut, brute=True))


# ---- the allowances of the GPU comparison (the device's fp64 exp / expm1 may differ from libm's in the last place) ---------------------------------------
def ulp32(x):
    with np.errstate(all="ignore"):
        return np.spacing(np.abs(np.asarray(x, f32)).astype(f32)).astype(f64)


def ratio_gate(d, out):
    """one fp32 ulp; NOTHING on a row whose old_logprob is the logprob's own bits: exp(0) is 1 on every device"""
    return np.where(d["old"].view(u32) == out.logprob.view(u32), 0.0, ulp32(out.ratio))


def kl_gate(out):
    """one fp32 ulp plus 2^-52 (|e| + |u|); NOTHING on a row with u = 0 (and without a reference): expm1(0) is 0 on every device"""
    with np.errstate(all="ignore"):
        return np.where(out.u == 0, 0.0, ulp32(out.kl) + 2.0 ** -52 * (np.abs(out.e) + np.abs(out.u)))


def coef_gate(c, d, out):
    """what the two allowances above leave for k = g (float) (A ratio + kl_coef e): |A| ulp(ratio) on an unclipped policy term, kl_coef 2^-52 (|e| + |u|) on the
    other, through the rounding of W (one ulp of the result may follow) and the fp32 product with g (another); NOTHING where neither allowance applies, and
    nothing on a coefficient of 0 (a clipped row without a KL term, a row scale of 0): its sign is part of the record"""
    g = np.ones(len(out.coef), f32) if d["scale"] is None else d["scale"]
    with np.errstate(all="ignore"):
        dW = np.abs(d["adv"].astype(f64)) * np.where(out.flags != 0, 0.0, ratio_gate(d, out)) + float(c.klc) * np.where(out.u == 0, 0.0, 2.0 ** -52 * (np.abs(out.e) + np.abs(out.u)))
        return np.where((dW == 0) | (out.coef == 0), 0.0, np.abs(g.astype(f64)) * dW + 2.0 * ulp32(out.coef))


# ---- the derived bounds against fp64 ------------------------------------------------------------------------------------------------------
delta_q, bound_row_scalar, bound_softmax_grad = XC.delta_q, XC.bound_row_scalar, XC.bound_grad


def bound_entropy(C, H):
    """the scorer's: log Z's error, E's denominator by the same relative error (E <= ln C), E's numerator by 2^-21 on each mass, x |1 - x| 2^-24 <=
    552 * 2^-24 from the rounding of d in x e^-x, one unit of q truncated per code times x <= 24 against Q >= 2^32, 2^-16 unit per term, and the codes of mass 0
    (x > 22.1) dropped; then the final rounding"""
    dq = delta_q(C)
    lnc = math.log(max(C, 2))
    return (1 + lnc) * dq / (1 - dq) + lnc * 2.0 ** -21 + 552 * 2.0 ** -24 + 24 * C * 2.0 ** -32 + C * 2.0 ** -48 + C * 22.1 * math.exp(-22.1) + abs(H) * 2.0 ** -24 + 1e-12


def bound_ratio(C, lp, ratio):
    """ratio = exp(lp - old): the error b of lp (its fp32 rounding included) through the exponential, the rounding to fp32, 1e-12 relative for the fp64 exp"""
    b = bound_row_scalar(C, lp)
    return ratio * (math.expm1(b) + 2.0 ** -24 + 1e-12)


def bound_k3(C, lp, u, kl):
    """kl = expm1(u) - u, u = ref - lp: d kl / du = expm1(u), the second-order term exp(u + b) b^2 / 2 <= exp(u + b) b^2, the rounding to fp32"""
    b = bound_row_scalar(C, lp)
    return abs(math.expm1(u)) * b + math.exp(u + b) * b * b + abs(kl) * 2.0 ** -24 + 1e-12


def bound_coef(C, lp, A, ratio, clipped, klc, u, g, k):
    """k = g (A ratio [unclipped] + kl_coef expm1(u)): the ratio's bound, d expm1(u) / du = exp(u) over the error of lp (second order as above), the rounding of
    W to fp32 and the fp32 product with g"""
    b = bound_row_scalar(C, lp)
    dW = (0.0 if clipped or A == 0 else abs(A) * bound_ratio(C, lp, ratio)) + klc * (math.exp(u + b) * b + 1e-12 * abs(math.expm1(u)))
    return abs(g) * dW + 2 * abs(k) * 2.0 ** -24 + 1e-12


def bound_entropy_grad(C, p, logp_plus_H, kH, H):
    """elementwise |kH t_i - fp64|, t_i = p_i (log p_i + H) = p_i (d_i + E): the error of p_i as in the loss, of d_i = l_i - m (its fp32 rounding, |d| <= 24) and
    of E (the entropy's bound: E = H - Lq and both carry the error of Q), the rounding of t_i, the fp32 product with kH and the fp32 sum into the element; a code
    the kernel gives mass 0 (more than 22.1 below the maximum) contributes its whole fp64 term: at most 24 e^-22.1 + e^-22.1 H"""
    dq = delta_q(C)
    dp = p * ((2.0 ** -21 + 24 * 2.0 ** -24 + dq) / (1 - dq) + 2.0 ** -24) + 2.0 ** -32 + math.exp(-24.0)
    dshift = 24 * 2.0 ** -24 + bound_entropy(C, H) + dq / (1 - dq)
    t = np.abs(p * logp_plus_H)
    dropped = math.exp(-22.1) * (24 + abs(H))
    return abs(kH) * (dp * np.abs(logp_plus_H) + (p + dp) * dshift + 3 * t * 2.0 ** -24 + dropped) + 1e-12
