"""The token scorer's arithmetic of record in numpy float32 / uint64 / float64 (include/selftok_hip_ext.h states it; csrc/token_score.hip runs it), a second,
brute-force formulation (Python `sorted` on (-key, index) for the rank and the first code, Python integers for Q and S_h, its own address arithmetic for the
target), the case table and the planted mistakes -- shared by tests/test_token_score_cpu.py and tests/test_token_score_gpu.py.

Steps 1 - 4 (guidance, temperature, key, integer mass) are the sampler's and are IMPORTED from tests/token_sample_cases.py, not restated.  What is the
scorer's own: the target's address, the rank, the first code, the fp64 log-probability, the integer entropy sum S_h and the row kinds.

Launch geometry the table is built around (csrc/token_score.hip): 512 threads own a row, a thread owns 4-code chunks t, t + 512, ..; C <= 4096 runs the
2-chunk kernel, C <= 32768 the 16-chunk kernel, above that the streamed one; the up to three codes past the last whole chunk (C % 4) are thread 0's; the grid
is min(R, 65536) x ceil(R / 65536) workgroups.  Edges named below: GEOMETRY_C and GEOMETRY_R."""
import math
from collections import namedtuple

import numpy as np

import token_sample_cases as TC
from token_sample_cases import OFFSET_VLM, key_of, scaled_logits, to_bf16_bits, weight, widen_bf16

f32, u32, u64, f64 = np.float32, np.uint32, np.uint64, np.float64
NT, SMALL_C, REG_C, GRID_X = 512, 4096, 32768, 65536
GEOMETRY_C = (2047, 2048, 2049,                                     # one whole chunk per thread, +- 1 (4 * NT)
              2050,                                                 # a partial chunk of two codes (1 and 3 are 4097 / 4095 and their like)
              4095, 4096, 4097,                                     # 2-chunk kernel | 16-chunk kernel
              32767, 32768, 32769,                                  # 16-chunk kernel | streamed kernel (17 chunk rounds, the last all but empty)
              65536)                                                # 32 chunk rounds
GEOMETRY_R = (GRID_X, GRID_X + 1)                                   # one full grid row; one workgroup into the second
POISON = 2 ** 31 - 1                                                # what the id buffers hold where no target lives: read by mistake, it makes the row bad
NAN32 = f32("nan")

Out = namedtuple("Out", "logprob q_total q_t rank top_id entropy s_h bad ignored")


def _log_z(q_total):
    return math.log(q_total * 2.0 ** -32)


# ---- the emulation: all rows of a case at once ------------------------------------------------------------------------------------------------------
def score_rows(lc, lu, targets, *, s=1.0, temperature=1.0, mut=None):
    """lc, lu (or None) fp32 [R, C]; targets int64 [R] -> Out of arrays [R] (q_total, q_t, s_h uint64; logprob, entropy fp32; rank, top_id int32; bad,
    ignored bool).  numpy throughout; the two fp64 scalars per row through math.log, as the sampler's emulation takes them."""
    lc = np.asarray(lc, dtype=f32)
    R, C = lc.shape
    t = np.asarray(targets, dtype=np.int64).copy()
    l, inv_t = scaled_logits(lc, lu, s, temperature, "guidance_from_cond" if mut == "guidance_from_cond" else None)
    if mut == "temperature_after":                                  # the target's logit is read before the temperature is applied
        l_pre, _ = scaled_logits(lc, lu, s, 1.0)
    bad = np.isnan(l).any(1) | (l == np.inf).any(1) | (l == -np.inf).all(1) | (t >= C)
    ignored = ~bad & (t < 0)
    if mut == "ignored_as_bad":
        bad, ignored = bad | ignored, np.zeros(R, bool)
    out = Out(np.full(R, NAN32, f32), np.zeros(R, u64), np.zeros(R, u64), np.full(R, -1, np.int32), np.full(R, -1, np.int32), np.full(R, NAN32, f32),
              np.zeros(R, u64), bad, ignored)
    g = np.flatnonzero(~bad)
    if g.size == 0:
        return out
    lg = l[g]
    lg = np.where(lg == 0, f32(0.0), lg)                            # -0.0 counts as +0.0
    key = key_of(lg)
    if mut == "neg_zero_below":
        u = l[g].view(u32)
        key = np.where(u & u32(0x80000000), ~u, u | u32(0x80000000))
    m = lg.max(1)
    with np.errstate(invalid="ignore"):
        d = (lg - m[:, None]).astype(f32)
        _, q = weight(d)
    dd = np.where(q > 0, d, f32(0.0))
    prod = q.astype(f64) * (-dd).astype(f64) * 65536.0
    h = (np.rint(prod) if mut == "rint_h" else np.trunc(prod)).astype(u64)
    q_total, s_h = q.sum(1, dtype=u64), h.sum(1, dtype=u64)
    top = np.argmax(key, axis=1)                                    # the first maximum: the lowest index at the highest key
    tg = t[g]
    scored = tg >= 0
    ti = np.where(scored, tg, 0)
    rows = np.arange(g.size)
    tkey = key[rows, ti]
    if mut == "temperature_after":
        lp_ = np.where(l_pre[g] == 0, f32(0.0), l_pre[g])
        tkey = key_of(lp_)[rows, ti]
    idx = np.arange(C)[None, :]
    ahead = (key > tkey[:, None]).sum(1)
    if mut != "ties_by_value":                                      # equal keys: the lower index is ahead
        before = (idx <= ti[:, None]) if mut == "rank_counts_self" else (idx < ti[:, None])
        ahead = ahead + ((key == tkey[:, None]) & before).sum(1)
    lt = from_key(tkey)
    with np.errstate(invalid="ignore"):
        _, q_t = weight((lt - m).astype(f32))
    for j, r in enumerate(g):
        lz = _log_z(int(q_total[j]))
        out.q_total[r], out.s_h[r], out.top_id[r] = q_total[j], s_h[j], top[j]
        out.entropy[r] = f32(lz + float(int(s_h[j])) / (65536.0 * float(int(q_total[j]))))
        if scored[j]:
            out.logprob[r] = f32((float(lt[j]) - float(m[j])) - lz)
            out.rank[r], out.q_t[r] = ahead[j], q_t[j]
        else:
            out.logprob[r] = f32(0.0)
    return out


def from_key(key):
    """the fp32 value of a key (the inverse of key_of; -0.0 does not come back)"""
    key = np.asarray(key, dtype=u32)
    return np.where(key & u32(0x80000000), key & u32(0x7FFFFFFF), ~key).astype(u32).view(f32)


# ---- the second formulation: one row, Python integers and sorted() ----------------------------------------------------------------------------------
def score_row_brute(lc, lu, target, *, s=1.0, temperature=1.0, mut=None):
    """-> a tuple (logprob fp32, q_total, q_t, rank, top_id, entropy fp32, s_h, bad, ignored) of Python values.  The planted mistakes are written a
    second time here, independently."""
    C = len(lc)
    inv_t = f32(1.0) / f32(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        l = np.asarray(lc, dtype=f32)
        if lu is not None:
            lu32 = np.asarray(lu, dtype=f32)
            diff = l - lu32
            l = (l if mut == "guidance_from_cond" else lu32) + f32(s) * diff
        l_raw = l
        l = l * inv_t
    vals = l.tolist()
    target = int(target)
    BAD = (NAN32, 0, 0, -1, -1, NAN32, 0, True, False)
    if any(math.isnan(v) or v == math.inf for v in vals) or all(v == -math.inf for v in vals) or target >= C:
        return BAD
    if target < 0 and mut == "ignored_as_bad":
        return BAD
    canon = np.where(l == 0, f32(0.0), l).astype(f32)
    keys = key_of(l.copy() if mut == "neg_zero_below" else canon)
    if mut == "neg_zero_below":
        uu = l.view(u32)
        keys = np.where(uu & u32(0x80000000), ~uu, uu | u32(0x80000000))
    keys = keys.tolist()
    m = max(canon.tolist())
    with np.errstate(invalid="ignore"):
        d = (canon - f32(m)).astype(f32)
        _, qq = weight(d)
    q = [int(v) for v in qq.tolist()]
    dl = d.tolist()
    rnd = (lambda x: int(round(x))) if mut == "rint_h" else (lambda x: int(math.trunc(x)))     # Python rounds half to even, as rint does
    s_h = sum(rnd(float(q[i]) * float(-dl[i]) * 65536.0) for i in range(C) if q[i] > 0)
    q_total = sum(q)
    ordered = sorted(range(C), key=lambda i: (-keys[i], i))
    lz = math.log(q_total * 2.0 ** -32)
    ent = f32(lz + float(s_h) / (65536.0 * float(q_total)))
    if target < 0:
        return (f32(0.0), q_total, 0, -1, ordered[0], ent, s_h, False, True)
    tk = keys[target]
    lt = float(canon[target])
    if mut == "temperature_after":
        raw = np.where(l_raw == 0, f32(0.0), l_raw).astype(f32)
        tk, lt = int(key_of(raw)[target]), float(raw[target])
    if mut == "ties_by_value":
        rank = sum(1 for k in keys if k > tk)
    elif mut == "temperature_after":
        rank = sum(1 for i, k in enumerate(keys) if k > tk or (k == tk and i < target))
    else:
        rank = ordered.index(target) + (1 if mut == "rank_counts_self" else 0)
    with np.errstate(invalid="ignore"):
        q_t = int(weight(np.asarray([lt], f32) - f32(m))[1][0])
    return (f32((lt - float(m)) - lz), q_total, q_t, rank, ordered[0], ent, s_h, False, False)


# ---- the case table ----------------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "name kind B S C dtype offset row guided s T step ids wide tk")


def _case(name, kind, B, C, S=1, dtype="f32", offset=0, pad=0, guided=False, s=1.0, T=1.0, step=1, ids="int64", wide=False, tk="mix"):
    row = offset + C + pad
    row += (-row) % 4
    return Case(name, kind, B, S, C, dtype, offset, row, guided, s, T, step, ids, wide, tk)


CASES = [
    _case("c1", "small", 1, 1, tk="argmax"),
    _case("c3_R3", "small", 3, 3),
    _case("c4_int32", "small", 5, 4, ids="int32"),
    _case("c5_S3_rev", "small", 2, 5, S=3, step=-1),
    _case("c255_T07", "gauss1", 3, 255, T=0.7),
    _case("c256_bf16", "gauss1", 3, 256, dtype="bf16"),
    _case("c257_cfg", "gauss1", 3, 257, guided=True, s=3.0),
    _case("c2047", "gauss1", 3, 2047),
    _case("c2048_bf16_cfg", "gauss1", 3, 2048, dtype="bf16", guided=True, s=3.0, T=0.7),
    _case("c2049_T4", "gauss8", 3, 2049, T=4.0),
    _case("c2050_int32_wide", "gauss1", 2, 2050, S=3, ids="int32", wide=True),
    _case("c4095_stride", "gauss1", 3, 4095, offset=4, pad=1, T=4.0),
    _case("c4096_R64", "gauss1", 64, 4096),
    _case("c4096_S40_rev", "gauss1", 1, 4096, S=40, step=-1, T=0.7),
    _case("c4097_bf16_S40", "gauss1", 1, 4097, S=40, dtype="bf16", ids="int32"),
    _case("c32767_T4", "gauss8", 3, 32767, T=4.0),
    _case("c32768_cfg_vlm", "gauss1", 1, 32768, S=3, step=-1, offset=OFFSET_VLM, guided=True, s=3.0, T=0.7),
    _case("c32768_bf16_T4", "gauss8", 3, 32768, dtype="bf16", T=4.0),
    _case("c32769", "gauss1", 3, 32769),
    _case("c32769_bf16_cfg", "gauss1", 1, 32769, dtype="bf16", guided=True, s=3.0, pad=8),
    _case("c65536", "gauss8", 3, 65536),
    _case("c65536_bf16_cfg", "gauss1", 1, 65536, dtype="bf16", guided=True, s=3.0, pad=8),
    _case("c1000_bf16_cfg_vlm_wide_rev", "gauss1", 2, 1000, S=3, step=-1, dtype="bf16", offset=OFFSET_VLM, pad=24, guided=True, s=3.0, T=0.7, wide=True),
    _case("four", "four", 9, 1000, tk="tie"),
    _case("four_bf16_T07", "four", 6, 4097, dtype="bf16", T=0.7, tk="tie"),
    _case("four_cfg", "four", 6, 256, guided=True, s=3.0, ids="int32", tk="tie"),
    _case("zeros_pair", "zeros", 6, 5, tk="zeros"),
    _case("dominant", "dominant", 4, 1000, tk="dominant"),
    _case("target_neginf", "gauss_neginf", 4, 257, tk="neginf"),
    _case("neginf_but_one", "neginf", 4, 257, tk="neginf_one"),
    _case("neginf_but_one_bf16", "neginf", 4, 4097, dtype="bf16", tk="neginf_one"),
    _case("ignored", "gauss1", 2, 1000, S=3, tk="ignored"),
    _case("ignored_int32_rev", "gauss1", 2, 300, S=3, step=-1, ids="int32", tk="ignored"),
    _case("bad_rows", "bad", 9, 1000, tk="badtargets"),
    _case("bad_rows_bf16_cfg", "bad", 9, 256, dtype="bf16", guided=True, s=3.0, offset=8, pad=4, tk="badtargets"),
    _case("grid_row_full", "small", GRID_X, 4, ids="int32"),
    _case("grid_row_plus_one", "small", 1, 3, S=GRID_X + 1, step=-1),
]
BY_NAME = {c.name: c for c in CASES}
FOUR = TC.FOUR

_CACHE = {}


def rows_of(c):
    return c.B * c.S


def id_geometry(c):
    """(buffer length, base element, seq stride, step stride) of a case's id buffer; `wide`: every other element of a row, rows one element apart more"""
    a = 2 if c.wide else 1
    seq = a * c.S + (3 if c.wide else 0)
    base = 2 + (a * (c.S - 1) if c.step < 0 else 0)
    return 2 + c.B * seq + 2, base, seq, a * c.step


def make(name):
    """-> dict(logits, uncond (or None): host arrays [R, row], NaN outside the window, bf16 as uint16 bits; ids: the 1-D id buffer (POISON where no target
    lives); targets int64 [R]: what row r is to be scored against).  Built once per case and shared: treat as read-only."""
    if name in _CACHE:
        return _CACHE[name]
    c = BY_NAME[name]
    rng = np.random.default_rng(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + 17)
    R, C = rows_of(c), c.C

    def window(second=False):
        if c.kind in ("gauss1", "bad", "small", "gauss_neginf"):
            w = rng.standard_normal((R, C)).astype(f32)
        elif c.kind == "gauss8":
            w = (rng.standard_normal((R, C)) * 8.0).astype(f32)
        elif c.kind == "four":
            w = np.full((R, C), 0.5, f32) if second else np.asarray(FOUR, f32)[rng.integers(0, 4, size=(R, C))]
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
        if c.kind == "bad" and not second:                          # good rows between a NaN, a +inf and an all -inf row (rows 1, 3, 5)
            w[1, C // 3] = np.nan
            w[3, C - 1] = np.inf
            w[5, :] = -np.inf
        return w

    def full(w):
        buf = np.full((R, c.row), np.nan, f32)
        buf[:, c.offset:c.offset + C] = w
        return to_bf16_bits(buf) if c.dtype == "bf16" else buf

    d = {"logits": full(window()), "uncond": full(window(True)) if c.guided else None}
    lc, lu = _windows(c, d)
    with np.errstate(invalid="ignore", over="ignore"):
        l, _ = scaled_logits(lc, lu, c.s, c.T)
    t = rng.integers(0, C, size=R).astype(np.int64)
    safe = np.where(np.isnan(l), -np.inf, l)
    am = np.argmax(key_of(np.where(safe == 0, f32(0.0), safe)), axis=1)
    r = np.arange(R)
    if c.tk == "argmax":
        t = am.astype(np.int64)
    elif c.tk == "mix":
        t = np.where(r % 4 == 0, am, t)
    elif c.tk == "tie":                                             # first, middle and last of the target's group of equal logits
        for i in range(R):
            grp = np.flatnonzero(l[i] == l[i, t[i]])
            t[i] = grp[[0, len(grp) // 2, len(grp) - 1][i % 3]]
    elif c.tk == "zeros":                                           # each of the three zeros (-0.0, +0.0, -0.0) in turn
        for i in range(R):
            t[i] = np.flatnonzero(lc[i] == 0)[i % 3]
    elif c.tk == "dominant":                                        # the dominant code, and a code 30 below it: q_t = 0, a finite logprob
        t = np.where(r % 2 == 0, am, (am + 1 + r) % C)
    elif c.tk == "neginf":
        t = np.where(r % 2 == 0, (t // 5) * 5, t)
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
    d["ids"], d["targets"] = ids, t
    _CACHE[name] = d
    return d


def _windows(c, d, at=None):
    off = c.offset if at is None else at
    cut = lambda a: None if a is None else (widen_bf16(a) if c.dtype == "bf16" else a)[:, off:off + c.C]
    return cut(d["logits"]), cut(d["uncond"])


def windows(name):
    """the fp32 windows (cond, uncond or None) of a case, widened"""
    return _windows(BY_NAME[name], make(name))


BRUTE_ROWS = 24


def brute_rows(c):
    """the rows the second formulation walks: all of them up to 64, else the first, the last and a spread in between"""
    R = rows_of(c)
    if R <= 64:
        return list(range(R))
    return sorted(set(list(range(8)) + list(range(R - 8, R)) + [GRID_X - 1, min(GRID_X, R - 1)] + list(range(0, R, R // 8))))


def gather_targets(c, d, mut=None):
    """the emulation's reading of the id buffer: numpy index arithmetic"""
    _, base, seq, step = id_geometry(c)
    r = np.arange(rows_of(c))
    if mut == "step_not_reversed" and step < 0:
        base, step = base + (c.S - 1) * step, -step
    t = d["ids"][base + (r // c.S) * seq + (r % c.S) * step].astype(np.int64)
    if mut == "target_in_vocab":
        t = t - c.offset
    return t


_REF = {}


def reference(name, mut=None, brute=False):
    """the emulation: Out of arrays over all rows.  brute=True: {row: tuple} over brute_rows.  The unmutated results are computed once and shared."""
    k = (name, mut, brute)
    if k in _REF:
        return _REF[k]
    c, d = BY_NAME[name], make(name)
    lc, lu = windows(name)
    if not brute:
        out = score_rows(lc, lu, gather_targets(c, d, mut), s=c.s, temperature=c.T, mut=mut)
    else:
        _, base, seq, step = id_geometry(c)
        out = {}
        for r in brute_rows(c):
            b, st = divmod(r, c.S)
            if mut == "step_not_reversed" and step < 0:
                st = c.S - 1 - st
            t = int(d["ids"][base + b * seq + st * step])
            if mut == "target_in_vocab":
                t -= c.offset
            out[r] = score_row_brute(lc[r], None if lu is None else lu[r], t, s=c.s, temperature=c.T, mut=mut)
    if mut is None or len(_REF) < 4096:
        _REF[k] = out
    return out


def row_tuple(out, r):
    """row r of an Out, comparable: floats by their bits"""
    return (f32(out.logprob[r]).tobytes(), int(out.q_total[r]), int(out.q_t[r]), int(out.rank[r]), int(out.top_id[r]), f32(out.entropy[r]).tobytes(), int(out.s_h[r]),
            bool(out.bad[r]), bool(out.ignored[r]))


def brute_tuple(t):
    return (f32(t[0]).tobytes(), int(t[1]), int(t[2]), int(t[3]), int(t[4]), f32(t[5]).tobytes(), int(t[6]), bool(t[7]), bool(t[8]))


def same(name, a, b):
    """two results of a case over the rows the brute force walks (either kind each): every output equal, floats bit for bit"""
    rows = brute_rows(BY_NAME[name])
    ta = [brute_tuple(a[r]) if isinstance(a, dict) else row_tuple(a, r) for r in rows]
    tb = [brute_tuple(b[r]) if isinstance(b, dict) else row_tuple(b, r) for r in rows]
    return ta == tb


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------------------------
MUTS = ("ties_by_value", "rank_counts_self", "neg_zero_below", "target_in_vocab", "temperature_after", "guidance_from_cond", "step_not_reversed", "rint_h",
        "ignored_as_bad")


def needs(mut, c):
    """what a case must have for a mistake to be able to move it at all (necessary, not sufficient)"""
    return {"ties_by_value": c.C > 1, "rank_counts_self": True, "neg_zero_below": c.kind == "zeros", "target_in_vocab": c.offset != 0,
            "temperature_after": c.T != 1.0, "guidance_from_cond": c.guided, "step_not_reversed": c.step < 0 and c.S > 1, "rint_h": c.C > 1,
            "ignored_as_bad": c.tk == "ignored"}[mut]


def applies(mut, name):
    """does the mistake move the case?  Decided by the brute-force formulation, where every mistake is written a second time."""
    return not same(name, reference(name, brute=True), reference(name, mut=mut, brute=True))
