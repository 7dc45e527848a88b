"""The token sampler's arithmetic of record in numpy float32 / uint64 (include/selftok_hip_ext.h states it; csrc/token_sample.hip runs it), a second,
brute-force formulation (Python `sorted` on (-key, index), Python-integer running sums, a scalar Philox), the case table and the planted mistakes -- shared by
tests/test_token_sample_cpu.py and tests/test_token_sample_gpu.py.

numpy's float32 `*`, `+`, `-` round once per operation and never fuse, `np.rint` rounds half to even: the same operations the kernel is compiled to
(-ffp-contract=off).  Every sum of masses is an integer sum."""
import math
from collections import namedtuple

import numpy as np

f32, u32, u64 = np.float32, np.uint32, np.uint64
LOG2E, LN2_HI, LN2_LO = f32(1.4426950408889634), f32(0.693145751953125), f32(1.428606765330187045e-06)
C6, C5, C4, C3 = f32(1.0 / 720.0), f32(1.0 / 120.0), f32(1.0 / 24.0), f32(1.0 / 6.0)
ONE = 1 << 32                                                       # the mass of the row maximum
M32 = 0xFFFFFFFF

PHILOX_KNOWN = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                ((M32,) * 4, (M32,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


# ---- Philox4x32-10 --------------------------------------------------------------------------------------------------------------------------------
def philox(ctr, key):
    """vectorised: ctr [..., 4], key [..., 2] (anything that broadcasts) uint32 -> [..., 4] uint32; uint64 products, no Python integers"""
    c = [np.asarray(ctr)[..., i].astype(u64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(u64) for i in range(2)]
    for _ in range(10):
        p0, p1 = u64(0xD2511F53) * c[0], u64(0xCD9E8D57) * c[2]
        c = [(p1 >> u64(32)) ^ c[1] ^ k[0], p1 & u64(M32), (p0 >> u64(32)) ^ c[3] ^ k[1], p0 & u64(M32)]
        k = [(k[0] + u64(0x9E3779B9)) & u64(M32), (k[1] + u64(0xBB67AE85)) & u64(M32)]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(u32)


def philox_scalar(ctr, key):
    """the 12-line version: Python integers"""
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
        k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
    return tuple(c)


def mulhi64(u, q):
    """floor(u * q / 2^64) for uint64 arrays, by 32-bit limbs"""
    u, q = np.asarray(u, dtype=u64), np.asarray(q, dtype=u64)
    lo = u64(M32)
    s = u64(32)
    uh, ul, qh, ql = u >> s, u & lo, q >> s, q & lo
    mid = (ul * ql >> s) + (uh * ql & lo) + (ul * qh & lo)
    return uh * qh + (uh * ql >> s) + (ul * qh >> s) + (mid >> s)


# ---- the arithmetic of record ---------------------------------------------------------------------------------------------------------------------
def widen_bf16(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(u32) << u32(16)).view(f32)


def to_bf16_bits(x):
    """round to nearest even, for building inputs only"""
    b = np.asarray(x, dtype=f32).view(u32).astype(u64)
    r = ((b + u64(0x7FFF) + ((b >> u64(16)) & u64(1))) >> u64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def weight(d):
    """fp32 d <= 0 -> (w fp32 = exp(d) * 2^32 to 2^-21 relative, q uint64 = trunc(w)); q = 0 for d < -24, -inf and NaN"""
    d = np.asarray(d, dtype=f32)
    ok = d >= f32(-24.0)
    dd = np.where(ok, d, f32(0.0))
    n = np.rint(dd * LOG2E)
    r = (dd - n * LN2_HI) - n * LN2_LO
    p = C6 * r + C5
    p = p * r + C4
    p = p * r + C3
    p = p * r + f32(0.5)
    p = p * r + f32(1.0)
    p = p * r + f32(1.0)
    w = p * np.ldexp(f32(1.0), n.astype(np.int32) + 32).astype(f32)
    assert w.dtype == f32 and p.dtype == f32 and r.dtype == f32
    return np.where(ok, w, f32(0.0)), np.where(ok, w, f32(0.0)).astype(u64)


def scaled_logits(lc, lu, s, temperature, mut=None):
    """(l fp32 [C], inv_T): guidance as difference, product, sum; then the product with inv_T = 1 / T in fp32 (1 when greedy)"""
    inv_t = f32(1.0) if temperature == 0 else f32(1.0) / f32(temperature)
    l = np.asarray(lc, dtype=f32)
    if lu is not None:
        lu = np.asarray(lu, dtype=f32)
        with np.errstate(invalid="ignore", over="ignore"):
            l = (l + f32(s) * (l - lu)) if mut == "guidance_from_cond" else (lu + f32(s) * (l - lu))
    with np.errstate(invalid="ignore", over="ignore"):
        return (l if mut == "temperature_after" else l * inv_t).astype(f32), inv_t


def key_of(l):
    u = np.where(l == 0, f32(0.0), l).view(u32)                      # -0.0 counts as +0.0
    return np.where(u & u32(0x80000000), ~u, u | u32(0x80000000))


Row = namedtuple("Row", "id n_kept q_total q_kept q_id logprob bad detail")
BAD_ROW = Row(-1, 0, 0, 0, 0, float("nan"), True, None)


def sample_row(lc, lu, *, s=1.0, temperature=1.0, top_k=0, top_p=1.0, seed=0, ctr=(0, 0), mut=None):
    """one row of the window: the emulation.  numpy throughout: one stable sort of the 48-bit order words, uint64 cumulative sums."""
    C = len(lc)
    greedy = temperature == 0
    l, inv_t = scaled_logits(lc, lu, s, temperature, mut)
    if np.isnan(l).any() or (l == np.inf).any() or (l == -np.inf).all():
        return BAD_ROW
    l = np.where(l == 0, f32(0.0), l)
    key = key_of(l)
    m = l.max()
    with np.errstate(invalid="ignore"):
        w, q = weight(l - m)
    if mut == "mass_rounded":
        q = np.rint(w.astype(np.float64)).astype(u64)
    idx = np.arange(C, dtype=u64)
    word = ((~key).astype(u64) << u64(16)) | (u64(C - 1) - idx if mut == "ties_desc_index" else idx)
    order = np.argsort(word, kind="stable")
    q_total = int(q.sum(dtype=u64))
    kk = 1 if greedy else (min(top_k, C) if top_k > 0 else C)
    pre = order[:kk]
    cum = np.cumsum(q[pre], dtype=u64)
    q_k = int(cum[-1])
    n, T = kk, None
    if not greedy and 0.0 < top_p < 1.0:
        base = q_total if mut == "topp_unrenormalised" else q_k
        t = float(f32(top_p)) * float(base)
        T = int(math.floor(t)) if mut == "floor_T" else int(math.ceil(t))
        n = int(np.searchsorted(cum, u64(T), side="right" if mut == "gt_T" else "left")) + 1
        n = max(1, min(n, kk))
    kept = pre[:n]
    if mut == "temperature_after":                                   # the filters saw the unscaled logits; the draw sees the scaled ones
        l = (l * inv_t).astype(f32)
        l = np.where(l == 0, f32(0.0), l)
        m = l.max()
        w, q = weight(l - m)
        q_total = int(q.sum(dtype=u64))
    q_kept = int(q[kept].sum(dtype=u64))
    draw = kept if mut == "draw_sorted_order" else np.sort(kept)
    r = 0
    if not greedy:
        c = (ctr[1], ctr[0]) if mut == "ctr_swapped" else ctr
        out = philox(np.array([c[0], c[1], 0, 0], dtype=u32), np.array([seed & M32, (seed >> 32) & M32], dtype=u32))
        u = u64(out[0]) | (u64(out[1]) << u64(32))
        if mut == "u_shifted_right":
            u = u >> u64(32)                                         # `u >> 32` only: r is all but always 0
        r = int(mulhi64(u, u64(q_kept)))
    pick = int(np.searchsorted(np.cumsum(q[draw], dtype=u64), u64(r), side="right"))
    i = int(draw[min(pick, len(draw) - 1)])
    denom = q_kept if mut == "logprob_filtered" else q_total
    lp = f32((float(l[i]) - float(m)) - math.log(denom * 2.0 ** -32))
    return Row(i, n, q_total, q_kept, int(q[i]), float(lp), False, dict(order=order, key=key, q=q, kk=kk, n=n, T=T, q_k=q_k, cum=cum, l=l))


def sample_row_brute(lc, lu, *, s=1.0, temperature=1.0, top_k=0, top_p=1.0, seed=0, ctr=(0, 0), mut=None):
    """the second formulation: Python's sorted on (-key, index), Python integers for every sum, the scalar Philox.  The planted mistakes are written a
    second time here, independently, so that it can say which cases a mistake moves."""
    C = len(lc)
    greedy = temperature == 0
    inv_t = f32(1.0) if greedy else f32(1.0) / f32(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        l = np.asarray(lc, dtype=f32)
        if lu is not None:
            lu32 = np.asarray(lu, dtype=f32)
            diff = l - lu32
            l = (l if mut == "guidance_from_cond" else lu32) + f32(s) * diff
        l_filter = l if mut == "temperature_after" else l * inv_t
        l_draw = l * inv_t
    if any(math.isnan(v) or v == math.inf for v in l_filter.tolist()) or all(v == -math.inf for v in l_filter.tolist()):
        return BAD_ROW

    def masses(lv):
        lv = np.where(lv == 0, f32(0.0), lv).astype(f32)
        mm = max(lv.tolist())
        with np.errstate(invalid="ignore"):
            ww, qq = weight(lv - f32(mm))
        if mut == "mass_rounded":
            return lv, mm, [int(round(float(v))) for v in ww.tolist()]     # Python rounds half to even, as rint does
        return lv, mm, [int(v) for v in qq.tolist()]

    lf, _, qf = masses(l_filter)
    keys = key_of(lf).tolist()
    ordered = sorted(range(C), key=(lambda i: (-keys[i], -i)) if mut == "ties_desc_index" else (lambda i: (-keys[i], i)))
    kk = 1 if greedy else (min(top_k, C) if top_k > 0 else C)
    pre = ordered[:kk]
    n = kk
    if not greedy and 0.0 < top_p < 1.0:
        base = sum(qf) if mut == "topp_unrenormalised" else sum(qf[i] for i in pre)
        t = float(f32(top_p)) * float(base)
        T = math.floor(t) if mut == "floor_T" else math.ceil(t)
        run, n = 0, 0
        for i in pre:
            run += qf[i]
            n += 1
            if (run > T) if mut == "gt_T" else (run >= T):
                break
    kept = pre[:n]
    ld, m, qd = masses(l_draw)
    q_total, q_kept = sum(qd), sum(qd[i] for i in kept)
    r = 0
    if not greedy:
        c = (ctr[1], ctr[0]) if mut == "ctr_swapped" else ctr
        out = philox_scalar((int(c[0]), int(c[1]), 0, 0), (seed & M32, (seed >> 32) & M32))
        u = out[0] | (out[1] << 32)
        if mut == "u_shifted_right":
            u = out[1]
        r = (u * q_kept) >> 64
    run, chosen = 0, None
    for i in (kept if mut == "draw_sorted_order" else sorted(kept)):
        run += qd[i]
        if run > r:
            chosen = i
            break
    if chosen is None:
        chosen = kept[-1]
    denom = q_kept if mut == "logprob_filtered" else q_total
    lp = f32((float(ld[chosen]) - float(m)) - math.log(denom * 2.0 ** -32))
    return Row(chosen, n, q_total, q_kept, qd[chosen], float(lp), False, None)


# ---- the case table -------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind B C dtype offset row guided s T k P pos ids K seed")
OFFSET_VLM = 151936                                                 # the image codes of a vision-language vocabulary start here


def _case(name, kind, B, C, dtype="f32", offset=0, pad=0, guided=False, s=1.0, T=1.0, k=0, P=1.0, pos=False, ids="int64", K=8, seed=0x5E1F70C):
    row = offset + C + pad
    row += (-row) % 4
    return Case(name, kind, B, C, dtype, offset, row, guided, s, T, k, P, pos, ids, K, seed)


CASES = [
    _case("c1", "small", 1, 1),
    _case("c2_k1", "small", 3, 2, k=1),
    _case("c5_k2_p50_pos", "small", 5, 5, k=2, P=0.5, pos=True, ids="int32"),
    _case("c255_k50_p90", "gauss1", 3, 255, k=50, P=0.9),
    _case("c256_bf16_p50", "gauss1", 3, 256, "bf16", P=0.5),
    _case("c257_cfg_kCm1_p999", "gauss1", 3, 257, guided=True, s=3.0, k=256, P=0.999),
    _case("c1000_bf16_cfg_vlm", "gauss1", 5, 1000, "bf16", offset=OFFSET_VLM, pad=24, guided=True, s=1.5, T=0.7, k=50, P=0.9),
    _case("c4095_T4_stride", "gauss1", 3, 4095, offset=4, pad=1, T=4.0, P=0.9),
    _case("c4096_B64", "gauss1", 64, 4096, k=50, P=0.9, pos=True),
    _case("c4097_bf16_kCp1_p10", "gauss1", 3, 4097, "bf16", T=0.7, k=4098, P=0.1, ids="int32"),
    _case("c32767_kC_p50", "gauss8", 3, 32767, T=4.0, k=32767, P=0.5),
    _case("c32768_cfg_vlm_pos", "gauss1", 5, 32768, offset=OFFSET_VLM, guided=True, s=2.0, T=0.7, k=50, P=0.9, pos=True),
    _case("c32768_bf16_T4_p999", "gauss8", 3, 32768, "bf16", T=4.0, P=0.999),
    _case("c65536_k50_p90", "gauss1", 3, 65536, k=50, P=0.9),
    _case("c65536_bf16_cfg_p50", "gauss1", 1, 65536, "bf16", guided=True, s=2.0, P=0.5, pad=8),
    _case("greedy_four", "four_greedy", 3, 1000, T=0.0),
    _case("greedy_gauss_cfg", "gauss1g", 3, 4096, guided=True, s=2.0, T=0.0, k=50, P=0.9),
    _case("four_k300_p50", "four", 64, 1000, k=300, P=0.5),
    _case("four_bf16_T07", "four", 5, 4097, "bf16", T=0.7, k=1500, P=0.9),
    _case("four_cfg", "four", 5, 256, guided=True, s=2.0, k=100, P=0.9, pos=True, ids="int32"),
    _case("dominant", "dominant", 3, 1000, P=0.9),
    _case("zeros_pair_k2", "zeros", 3, 5, k=2),
    _case("zeros_pair_greedy", "zeros", 3, 5, T=0.0),
    _case("neginf_but_one", "neginf", 3, 257, P=0.9),
    _case("neginf_but_one_k50", "neginf", 3, 257, "bf16", k=50),
    _case("bad_rows", "bad", 7, 1000, k=50, P=0.9),
    _case("bad_rows_bf16_cfg", "bad", 7, 256, "bf16", guided=True, s=2.0, P=0.5, offset=8, pad=4),
    _case("exact_T", "exact_T", 3, 8, P=0.5),                        # the running mass meets T exactly: >= keeps two codes, > would keep three
    _case("half_T", "half_T", 3, 5, P=0.5),                          # P * Q_k = 2^32 + 1/2: ceil asks for a second code, floor would not
    _case("off_gauss", "gauss_off", 3, 1000),                        # no filter at all: the draw alone
]
BY_NAME = {c.name: c for c in CASES}
FOUR = (2.0, 1.0, 0.0, -1.0)                                        # exact in bf16, and after the guidance and temperatures of the table still four values

_CACHE = {}


def make(name):
    """-> dict(logits, uncond (or None), ctr uint32 [B, 2], pos int32 [B] or None): host arrays, rows of `row` elements, NaN outside the window; bf16 as uint16
    bits.  Built once per case and shared: treat as read-only."""
    if name in _CACHE:
        return _CACHE[name]
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)))
    B, C = c.B, c.C

    def window(second=False):
        if c.kind in ("gauss1", "gauss1g", "gauss_off", "bad"):
            w = rng.standard_normal((B, C)).astype(f32)
        elif c.kind == "gauss8":
            w = (rng.standard_normal((B, C)) * 8.0).astype(f32)
        elif c.kind == "small":
            w = rng.standard_normal((B, C)).astype(f32)
        elif c.kind in ("four", "four_greedy"):
            w = np.full((B, C), 0.5, f32) if second else np.asarray(FOUR, f32)[rng.integers(0, 4, size=(B, C))]
        elif c.kind == "dominant":
            w = np.full((B, C), -30.0, f32)
            w[np.arange(B), rng.integers(0, C, size=B)] = 0.0
        elif c.kind == "zeros":
            w = np.tile(np.asarray([-1.0, -0.0, 0.0, -0.0, -2.0], f32), (B, 1))
            for b in range(B):
                w[b] = np.roll(w[b], b)
        elif c.kind in ("exact_T", "half_T"):
            base = [0.0, 0.0, 0.0, 0.0, -30.0, -30.0, -30.0, -30.0] if c.kind == "exact_T" else [0.0, 0.0, -22.1, -30.0, -30.0]
            w = np.stack([np.roll(np.asarray(base, f32), 2 * b) for b in range(B)])
        elif c.kind == "neginf":
            w = np.full((B, C), -np.inf, f32)
            w[np.arange(B), [0, C // 2, C - 1]] = f32(1.5)
        if c.kind == "bad" and not second:                          # good rows 0, 2, 4, 6 between a NaN, a +inf and an all -inf row
            w[1, C // 3] = np.nan
            w[3, C - 1] = np.inf
            w[5, :] = -np.inf
        return w

    def full(w):
        buf = np.full((B, c.row), np.nan, f32)
        buf[:, c.offset:c.offset + C] = w
        return to_bf16_bits(buf) if c.dtype == "bf16" else buf

    d = {"logits": full(window()), "uncond": full(window(True)) if c.guided else None}
    d["ctr"] = np.stack([rng.integers(0, 1 << 32, size=B, dtype=np.uint64), rng.integers(0, 1024, size=B, dtype=np.uint64)], axis=1).astype(u32)
    d["pos"] = rng.integers(0, c.K, size=B).astype(np.int32) if c.pos else None
    _CACHE[name] = d
    return d


def windows(name):
    """the fp32 windows (cond, uncond or None) of a case, widened"""
    c, d = BY_NAME[name], make(name)
    cut = lambda a: None if a is None else (widen_bf16(a) if c.dtype == "bf16" else a)[:, c.offset:c.offset + c.C]
    return cut(d["logits"]), cut(d["uncond"])


_REF = {}


def reference(name, mut=None, brute=False):
    """[Row] * B for a case; the unmutated emulation is computed once and shared"""
    if mut is None and not brute and name in _REF:
        return _REF[name]
    c, d = BY_NAME[name], make(name)
    lc, lu = windows(name)
    fn = sample_row_brute if brute else sample_row
    eff_mut = None if mut == "offset_ignored" else mut
    if mut == "offset_ignored":                                     # the window read from element 0 of the row
        a = lambda t: None if t is None else (widen_bf16(t) if c.dtype == "bf16" else t)[:, :c.C]
        lc, lu = a(d["logits"]), a(d["uncond"])
    rows = [fn(lc[b], None if lu is None else lu[b], s=c.s, temperature=c.T, top_k=c.k, top_p=c.P, seed=c.seed, ctr=tuple(int(v) for v in d["ctr"][b]), mut=eff_mut)
            for b in range(c.B)]
    if mut is None and not brute:
        _REF[name] = rows
    return rows


def same(a, b):
    """two lists of rows: every output equal (logprob by its fp32 bits; NaN equals NaN)"""
    key = lambda r: (r.id, r.n_kept, r.q_total, r.q_kept, r.q_id, r.bad, None if math.isnan(r.logprob) else f32(r.logprob).tobytes())
    return [key(x) for x in a] == [key(y) for y in b]


# ---- planted mistakes -------------------------------------------------------------------------------------------------------------------------------
MUTS = ("ties_desc_index", "topp_unrenormalised", "gt_T", "floor_T", "draw_sorted_order", "u_shifted_right", "ctr_swapped", "temperature_after",
        "guidance_from_cond", "mass_rounded", "logprob_filtered", "offset_ignored")


def needs(mut, c):
    """what a case must have for a mistake to be able to move it at all (necessary, not sufficient: whether a given draw moves is the brute-force
    formulation's call, see applies)"""
    p_on, k_on, greedy = 0.0 < c.P < 1.0 and c.T != 0, 0 < c.k < c.C and c.T != 0, c.T == 0
    return {"ties_desc_index": c.C > 1,
            "topp_unrenormalised": p_on and k_on, "gt_T": p_on, "floor_T": p_on, "draw_sorted_order": not greedy, "u_shifted_right": not greedy,
            "ctr_swapped": not greedy, "temperature_after": c.T not in (0.0, 1.0), "guidance_from_cond": c.guided, "mass_rounded": True,
            "logprob_filtered": p_on or k_on or greedy, "offset_ignored": c.offset != 0}[mut]


def applies(mut, name):
    """does the mistake move the case?  Decided by the brute-force formulation, where every mistake is written a second time."""
    return not same(reference(name, brute=True), reference(name, mut=mut, brute=True))


def cut_inside_ties(name):
    """per good row: (the k cut falls strictly inside a group of equal keys, the P cut does)"""
    out = []
    for r in reference(name):
        if r.bad:
            continue
        d = r.detail
        ks = d["key"][d["order"]]
        inside = lambda n: 0 < n < len(ks) and ks[n - 1] == ks[n]
        out.append((inside(d["kk"]), inside(d["n"]) and d["n"] < d["kk"]))
    return out
