"""Case table and host emulation of the VQ top-k lookup (csrc/vq_topk.hip, include/selftok_hip_ext.h), shared by tests/test_vq_topk_cpu.py and
tests/test_vq_topk_gpu.py.

`topk_ref` is the arithmetic of record: oracle.clib.l2norm16 -> oracle.clib.vq_scores (the canonical k-ordered fp32 FMA chain) -> a STABLE
sort on (NaN first, score descending with -0.0 == +0.0, index ascending); a zero score is written as +0.0, a NaN score as 0x7FC00000.

How the kernel walks the codes, which is what the planted structure aims at: code c sits in 32-code tile c >> 5; inside a tile the codes with
bit 2 of (c & 31) clear belong to wave half 0, the others to half 1, so a "lane stream" of a row is (code split, half) and holds 16 codes of
every tile of its split; the code range is cut into up to 64 splits of whole tiles (SELFTOK_VQ_SPLIT overrides the count).  A wave holds 32
rows (times RT = 1, 2 or 4 row blocks), a workgroup four waves."""
from collections import namedtuple

import numpy as np

from oracle import clib

Case = namedtuple("Case", "name N C tags build")      # tags: "ties" = exact ties among a row's best codes (an all-NaN row included), "nan" = NaN scores next to numbers
KS = (1, 2, 3, 8)
QNAN = np.uint32(0x7FC00000)
MUT_TIES_DESC, MUT_NAN_LAST, MUT_UNSTABLE = "ties_descending_index", "nan_last", "unstable_sort"


def _unit(rng, n):
    v = rng.standard_normal((n, 16)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def _base(seed, N, C):
    rng = np.random.default_rng(seed)
    return rng, (_unit(rng, N) * rng.uniform(0.5, 4.0, (N, 1))).astype(np.float32), _unit(rng, C)


def _plain(seed):
    def build(N, C):
        _, z, cb = _base(seed, N, C)
        return z, cb, {}
    return build


def _spread(C, n):
    """n code indices spread over the whole range: the first tile, the last tile, both halves, and (C >= 2048) every one of 8 equal splits"""
    if C == 32:
        return [0, 1, 5, 8, 14, 18, 22, 27, 31][:n]
    step = (C - 1) / (n - 1)
    out = sorted({int(round(i * step)) for i in range(n)})
    assert len(out) == n
    return out


def _dups(seed, rows_at):
    """(a), (b): identical best codes.  Row rows_at[0]: two in one lane's 16 codes of a tile; [1]: in the two wave halves of a tile; [2]: in two tiles of
    one stream (C >= 64); [3]: in the first and the last code split (C >= 64); [4]: nine copies spread over every split -- k = 8 returns the 8 lowest"""
    def build(N, C):
        rng, z, cb = _base(seed, N, C)
        t = (C >> 5) - 1
        groups = [[2, 3], [32 * t + 9, 32 * t + 13]]
        if C >= 64:
            groups += [[32 * (t - 1) + 17, 32 * t + 17], [5, C - 6]]
        groups.append(_spread(C, 9))
        assert len({c for g in groups for c in g}) == sum(len(g) for g in groups)
        plan = {}
        for g, r in zip(groups, [r for r in rows_at if r < N] * 2):      # N == 1: every group lands on row 0, the last one (nine copies) wins the row
            v = _unit(rng, 1)[0]
            cb[g] = v
            z[r] = v * np.float32(3.0)
            plan[r] = g
        return z, cb, {"dups": plan}
    return build


def _one_stream(seed):
    """(c): the 8 best codes of row 0 all in one lane stream (tile 0, half 0), the 9th best in the LAST tile (another split whenever there are two),
    scores strictly decreasing; row 1 (if any): the same with the stream in the last tile's half 1 and the 9th in tile 0"""
    def build(N, C):
        rng, z, cb = _base(seed, N, C)
        last = 32 * ((C >> 5) - 1)
        for r, codes in ((0, [0, 1, 2, 3, 8, 9, 10, 11, last + 20 if C > 32 else 16]), (1, [last + c for c in (4, 5, 6, 7, 12, 13, 14, 15)] + [last - 8 if C > 32 else 17])):
            if r >= N:
                break
            v, w = _unit(rng, 1)[0], _unit(rng, 1)[0]
            for j, c in enumerate(rng.permutation(codes[:8]).tolist() + codes[8:]):
                e = v + np.float32(0.02 * (j + 1)) * w
                cb[c] = e / np.linalg.norm(e)
            z[r] = v * np.float32(2.0)
        return z, cb, {}
    return build


def _zero_row(seed, row):
    """(d): a zero row scores +0.0 or -0.0 against every code: ids 0 .. k - 1"""
    def build(N, C):
        _, z, cb = _base(seed, N, C)
        z[min(row, N - 1)] = 0.0
        return z, cb, {"zero_row": min(row, N - 1)}
    return build


def _nan_row(seed, row):
    """(e): one NaN row (its wave takes the exact scan, the other waves the fast one): every score NaN, ids 0 .. k - 1"""
    def build(N, C):
        _, z, cb = _base(seed, N, C)
        z[min(row, N - 1), 5] = np.nan
        return z, cb, {"nan_row": min(row, N - 1)}
    return build


def _nonfinite_codes(seed):
    """(e): a NaN code, a second NaN code before it in another stream, a +inf and a -inf code; a row whose element 3 is zero (0 * inf = NaN) and a NaN row"""
    def build(N, C):
        _, z, cb = _base(seed, N, C)
        cb[C - 3, 7] = np.nan
        cb[6, 0] = np.nan
        cb[C // 2 + 1, 3] = np.inf
        cb[C // 2 + 9, 3] = -np.inf
        z[0, 3] = 0.0
        if N > 2:
            z[N - 1, 11] = np.nan
        return z, cb, {"nan_codes": [6, C - 3]}
    return build


def _signed_zeros(seed):
    """(e): row 0 = (1e-25, 0, ..., 0, 1): code 5 and code C - 12 score -0.0 (every product is -0.0: the first underflows, the others are +0 x -0), code 9
    scores +0.0, every other code is negative: ids (5, 9, C - 12), all three written as +0.0"""
    def build(N, C):
        _, z, cb = _base(seed, N, C)
        cb[:, 15] = -np.abs(cb[:, 15]) - np.float32(0.5)
        z[0] = 0.0
        z[0, 0], z[0, 15] = 1e-25, 1.0
        neg = np.full(16, -0.0, np.float32)
        neg[0] = -1e-25
        cb[5], cb[C - 12], cb[9] = neg, neg, 0.0
        return z, cb, {"signed_zeros": [5, 9, C - 12]}
    return build


def _ulp_ties(seed):
    """(f): row r = a multiple of a unit axis, so score(c) = cb[c][axis] exactly: codes whose axis element is v, v + 1 ulp, v + 2 ulp, ... in one lane's 16
    codes, across the halves, across tiles and across splits -- the order must follow single ulps, and two codes at the same value tie by index"""
    def build(N, C):
        rng, z, cb = _base(seed, N, C)
        cb *= np.float32(0.8)                                   # every other score is below 0.8
        plan = {}
        for r in range(min(N, 3)):
            axis = (3, 0, 15)[r]
            z[r] = 0.0
            z[r, axis] = (1.0, 2.5, 0.75)[r]
            codes = _spread(C, 9) if r == 0 else sorted(rng.choice(C, 9, replace=False).tolist())
            v, vals = np.float32(0.9), []
            for j in range(9):
                vals.append(v)
                if j not in (3, 6):                             # two exact ties among the one-ulp steps
                    v = np.nextafter(v, np.float32(2.0))
            for c, val in zip(codes, rng.permutation(np.array(vals, np.float32))):
                cb[c, axis] = val
            plan[r] = codes
        return z, cb, {"ulp": plan}
    return build


def _table():
    cases = []

    def add(name, N, C, factory, tags=(), *args):
        cases.append(Case(f"{name}_N{N}_C{C}", N, C, frozenset(tags), factory(1000 + len(cases), *args)))

    for N, C in ((1, 32), (31, 64), (32, 8192), (33, 32768), (127, 64), (128, 8192), (129, 32), (513, 8192)):
        add("random", N, C, _plain)
    for N, C in ((1, 64), (33, 32), (129, 8192), (31, 32768)):
        add("dups", N, C, _dups, ("ties",), (0, N // 2, N - 1, 1, N // 3 + 2))
    for N, C in ((1, 32), (32, 64), (127, 8192), (2, 32768)):
        add("one_stream", N, C, _one_stream)
    for N, C in ((1, 32), (129, 64), (33, 8192)):
        add("zero_row", N, C, _zero_row, ("ties",), 40)
    for N, C in ((1, 64), (129, 8192), (513, 32)):
        add("nan_row", N, C, _nan_row, ("ties",), 70)
    for N, C in ((3, 64), (128, 8192), (1, 32768)):
        add("nonfinite_codes", N, C, _nonfinite_codes, ("nan",))
    for N, C in ((1, 32), (33, 64), (31, 8192)):
        add("signed_zeros", N, C, _signed_zeros, ("ties",))
    for N, C in ((2, 32), (32, 64), (128, 32768), (3, 8192)):
        add("ulp_ties", N, C, _ulp_ties, ("ties",))
    return cases


CASES = _table()
_made, _ref = {}, {}


def make(case):
    """(z [N,16], codebook [C,16], plan) of a case; built once, returned read-only"""
    if case.name not in _made:
        z, cb, plan = case.build(case.N, case.C)
        z, cb = np.ascontiguousarray(z, np.float32), np.ascontiguousarray(cb, np.float32)
        z.setflags(write=False); cb.setflags(write=False)
        _made[case.name] = (z, cb, plan)
    return _made[case.name]


def _hash(idx):
    return (idx.astype(np.uint64) * np.uint64(2654435761)) % np.uint64(1 << 32)


def topk_order(scores, k, mut=None):
    """[N, C] canonical scores -> (ids int64 [N, k], scores fp32 [N, k]) in the order of record: per row a stable sort (np.lexsort, so equal
    (NaN flag, score) pairs keep ascending index) of the entries that can reach the first k -- those not below the k-th largest.
    mut: one of the planted mistakes."""
    N, C = scores.shape
    nan = np.isnan(scores)
    v = np.where(nan, np.float32(0), scores) + np.float32(0)           # -0.0 + 0.0 = +0.0
    rank = np.where(nan, np.float32(-np.inf if mut == MUT_NAN_LAST else np.inf), v)
    kth = np.partition(rank, C - k, axis=1)[:, C - k]
    ids, out = np.empty((N, k), np.int64), np.empty((N, k), np.uint32)
    for r in range(N):
        cand = np.flatnonzero(rank[r] >= kth[r])
        tie = {None: cand, MUT_NAN_LAST: cand, MUT_TIES_DESC: -cand, MUT_UNSTABLE: _hash(cand)}[mut]
        first = nan[r, cand] if mut == MUT_NAN_LAST else ~nan[r, cand]
        sel = cand[np.lexsort((tie, -v[r, cand], first))[:k]]
        ids[r] = sel
        out[r] = np.where(nan[r, sel], QNAN, v[r, sel].view(np.uint32))
    return ids, out.view(np.float32)


def scores_of(z, cb, normalize=True):
    return clib.vq_scores(clib.l2norm16(z) if normalize else z, cb)


def topk_ref(z, cb, k, normalize=True, mut=None, block=512):
    """rows in blocks of `block` on a thread pool (the C scores and numpy's partition release the GIL; at most 16 threads): the [N, C] score
    matrix of a whole golden file would be 4 GiB"""
    z = np.ascontiguousarray(z, np.float32).reshape(-1, 16)
    if z.shape[0] <= block:
        return topk_order(scores_of(z, cb, normalize), k, mut)
    from concurrent.futures import ThreadPoolExecutor
    import os
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as ex:
        parts = list(ex.map(lambda i: topk_order(scores_of(z[i:i + block], cb, normalize), k, mut), range(0, z.shape[0], block)))
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def case_ref(case, k=8):
    """reference of a case for k <= 8: the first k columns of the k = 8 result (the order is total), computed once"""
    if case.name not in _ref:
        z, cb, _ = make(case)
        ids, sc = topk_ref(z, cb, 8)
        ids.setflags(write=False); sc.setflags(write=False)
        _ref[case.name] = (ids, sc)
    ids, sc = _ref[case.name]
    return ids[:, :k], sc[:, :k]


# ---- the kernel's list algorithm restated in Python (csrc/vq_topk.hip), on the oracle's scores: what it computes given canonical scores ----
_EMPTY = 0x007FFFFF00000000


def _orderable(v):
    u = int(np.float32(v).view(np.uint32))
    return (~u) & 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000


def _from_orderable(k):
    return np.uint32((k & 0x7FFFFFFF) if k & 0x80000000 else (~k) & 0xFFFFFFFF).view(np.float32)


def _key(s, c):
    hi = 0xFFFFFFFF if s != s else _orderable(np.float32(0) if s == 0 else s)
    return (hi << 32) | ((~c) & 0xFFFFFFFF)


def _insert(l, k):
    for i in range(len(l)):
        if k > l[i]:
            l[i], k = k, l[i]


def kernel_walk_row(s, K, split, exact):
    """one row's scores s [C] -> (ids, score bits) as the kernel forms them: per (code split, wave half) stream a sorted list of K keys fed in the order
    the lane meets its codes -- fast path: only scores strictly above the stream's K-th (after one compare against the tile maximum); exact path: every
    key --, then the merge of the two halves, then of the splits.  `split` is clamped and rounded as the entry does."""
    nt = s.shape[0] >> 5
    tps = -(-nt // max(1, min(split, nt, 64)))
    parts = []
    for first in range(0, nt, tps):
        halves = []
        for half in (0, 1):
            l, thr = [_EMPTY] * K, np.float32(-np.inf)
            for t in range(first, min(nt, first + tps)):
                codes = [t * 32 + (r & 3) + 8 * (r >> 2) + 4 * half for r in range(16)]
                if exact:
                    for c in codes:
                        k = _key(s[c], c)
                        if k > l[-1]:
                            _insert(l, k)
                elif s[codes].max() > thr:
                    for c in codes:
                        if s[c] > thr:
                            _insert(l, _key(s[c], c))
                            thr = _from_orderable(l[-1] >> 32)
            halves.append(l)
        for k in halves[1]:
            _insert(halves[0], k)
        parts.append(halves[0])
    l = parts[0]
    for p in parts[1:]:
        for k in p:
            if k > l[-1]:
                _insert(l, k)
    return [(~k) & 0xFFFFFFFF for k in l], [0x7FC00000 if (k >> 32) == 0xFFFFFFFF else int(_from_orderable(k >> 32).view(np.uint32)) for k in l]
