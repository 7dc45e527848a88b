"""The arithmetic of record of the token statistics (csrc/token_stats.hip, selftoktokenizer_amd/tokenstats.py) in numpy, the case tables and the planted mistakes.

  counts     np.add.at on [K, C] uint32; an id outside [0, C) only counts in `bad`.
  census     fp64: per position and for the POOLED counts (uint64 column sums) n, used, H = -sum p ln p over the non-zero counts, H_ref = -sum p ln(p + 1e-10)
             (the reference's get_group_perplexity expression before its exp), max_count; a row with n == 0 is all zeros.
  agreement  a loop over the rows.
  nearest    a loop over the queries; ties go to the lowest index; no candidate gives (-1, 0).
Every emulation takes `mut`, a planted mistake; `*_applies(mut, case)` names the cases that can see it.

The kernels' edges the tables are built around: tok_count_kernel and tok_to_u16_kernel walk the ids flat, 256 per workgroup (ROW_TILE ids); tok_nearest_kernel has
64 query rows per strip and 64 reference rows per tile (TILE), a chunk of 64 positions, an aligned path (K even) and a halfword path (K odd), and the automatic
split turns from 1 to 2 at 8 tiles = 512 reference rows.
"""
import collections
import math

import numpy as np

ROW_TILE = 256          # ids per workgroup of the flat kernels
TILE = 64               # query rows per strip, reference rows per tile
SPLITS = (1, 2, 3, 5, 64)
INT64_MIN = np.iinfo(np.int64).min

# --------------------------------------------------------------------------------------------------------------------------------------------------
# count / census
# --------------------------------------------------------------------------------------------------------------------------------------------------
CountCase = collections.namedtuple("CountCase", "name N K C dtype es rpad kind")


def _cc(N, K, C, dtype="int64", es=1, rpad=0, kind="random"):
    name = f"n{N}_k{K}_c{C}_{dtype}" + (f"_es{es}" if es != 1 else "") + (f"_pad{rpad}" if rpad else "") + ("" if kind == "random" else f"_{kind}")
    return CountCase(name, N, K, C, dtype, es, rpad, kind)


COUNT_CASES = [
    # N = 0, 1, 63, 64, 65 and the flat tile of 256 ids +- 1 (K = 1: ids = rows; K = 40: 6 rows = 240, 7 rows = 280 ids)
    _cc(0, 40, 64), _cc(1, 40, 64), _cc(63, 40, 64, "int32"), _cc(64, 40, 64, "uint16"), _cc(65, 40, 64),
    _cc(255, 1, 64, "uint16"), _cc(256, 1, 64, "int32"), _cc(257, 1, 64), _cc(6, 40, 5), _cc(7, 40, 5, "int32"),
    # every K and C, every width
    _cc(65, 512, 32768, "uint16"), _cc(3, 1024, 32768, "int32"), _cc(64, 512, 32768, "int64"), _cc(9, 1, 5, "uint16"), _cc(70, 40, 32768, "int64"),
    # strides: elem_stride 2 and 8 (column 0 of a top-k result), a row stride larger than K
    _cc(65, 40, 64, "int64", es=2), _cc(64, 40, 32768, "int64", es=8), _cc(33, 40, 64, "int32", es=2, rpad=5), _cc(65, 40, 64, "uint16", rpad=3),
    # worst contention; the ends of the code range
    _cc(4096, 1, 32768, "int64", kind="equal"), _cc(65, 40, 32768, "uint16", kind="ends"), _cc(65, 40, 5, "int32", kind="ends"),
    # bad ids: -1 and C (signed widths), C and 65535 (uint16 at C = 32768), 2^40 and INT64_MIN (int64)
    _cc(65, 40, 64, "int32", kind="bad"), _cc(65, 40, 32768, "uint16", kind="bad"), _cc(65, 40, 32768, "int64", kind="bad"), _cc(64, 40, 5, "int64", es=2, kind="bad"),
    # uniform counts (perplexity == C), one code only (H == 0 exactly), a position that only ever received bad ids (n == 0)
    _cc(64, 40, 64, "int32", kind="uniform"), _cc(32768, 1, 32768, "uint16", kind="uniform"), _cc(5, 512, 5, "int64", kind="uniform"),
    _cc(65, 40, 32768, "int64", kind="one_code"), _cc(65, 40, 64, "int64", kind="dead_pos"),
    # positions with different totals (bad ids in some): the pooled row is not the mean of the per-position distributions
    _cc(300, 3, 5, "int64", kind="skewed"),
    # beyond the issue's table: a code book past 2^15, so that a uint16 id has its top bit set and is still a good id
    _cc(300, 1, 65536, "uint16", kind="high"),
]
COUNT_BY_NAME = {c.name: c for c in COUNT_CASES}
_NP = {"uint16": np.uint16, "int32": np.int32, "int64": np.int64}


def make_ids(name):
    """(base [N, K * es + rpad], view = base[:, :K * es:es]) -- the view is what is counted, the rest of base is filler of valid, different ids"""
    c = COUNT_BY_NAME[name]
    rng = np.random.default_rng(abs(hash_name(name)))
    dt = _NP[c.dtype]
    width = c.K * c.es + c.rpad
    base = rng.integers(0, c.C, size=(c.N, width)).astype(dt)
    view = base[:, :c.K * c.es:c.es]
    N, K, C = c.N, c.K, c.C
    if c.kind == "equal":
        view[...] = 7
    elif c.kind == "one_code":
        view[...] = C - 2
    elif c.kind == "ends":
        view[...] = np.where(rng.integers(0, 2, size=(N, K)) == 1, C - 1, 0).astype(dt)
    elif c.kind == "uniform":
        view[...] = ((np.arange(N)[:, None] + 3 * np.arange(K)[None, :]) % C).astype(dt)
    elif c.kind == "high":
        view[...] = rng.integers(32768, 65536, size=(N, K)).astype(dt)
        view[0, 0] = 65535
    elif c.kind in ("bad", "dead_pos", "skewed"):
        if c.dtype == "uint16":
            bads = [C, 65535] if C < 65535 else []
        elif c.dtype == "int32":
            bads = [-1, C, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
        else:
            bads = [-1, C, 1 << 40, INT64_MIN, (1 << 32) + 3, -(1 << 32)]        # the last two: good ids in their low 32 bits
        if c.kind == "bad":
            hit = rng.random((N, K)) < 0.1
            hit[0, 0] = hit[N - 1, K - 1] = True
            pick = np.array(bads, dtype=dt)[rng.integers(0, len(bads), size=(N, K))]
            view[...] = np.where(hit, pick, view)
            for i, b in enumerate(bads):                                          # every kind at least once
                view[1 + i, 1 + i] = b
        elif c.kind == "dead_pos":
            view[:, 0] = np.array(bads, dtype=dt)[rng.integers(0, len(bads), size=N)]
        else:                                                                      # skewed: position 0 all code 0, position 1 half bad and the rest code 1, position 2 random
            view[:, 0] = 0
            view[:, 1] = np.where(np.arange(N) % 2 == 0, -1, 1)
    return base, view


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h + 1


def count(view, C, mut=None, base=None, es=1):
    """-> (counts uint32 [K, C], bad)"""
    N, K = view.shape
    ids = view
    if mut == "no_elem_stride":
        ids = base[:, :K]
    if mut == "u16_signed" and ids.dtype == np.uint16:
        ids = ids.view(np.int16)
    v = ids.astype(np.int64)
    if mut == "drop_tail":                                         # the last partial tile of 256 ids never runs
        keep = (N * K) // ROW_TILE * ROW_TILE
        live = (np.arange(N * K) < keep).reshape(N, K)
    else:
        live = np.ones((N, K), bool)
    good = (v >= 0) & (v < C)
    if mut == "clamp":
        v, good = np.clip(v, 0, C - 1), np.ones((N, K), bool)
    counts = np.zeros(K * C, np.uint32)
    kk = np.broadcast_to(np.arange(K)[None, :], (N, K))
    sel = good & live
    flat = v[sel] * K + kk[sel] if mut == "swapped" else kk[sel] * C + v[sel]
    np.add.at(counts, flat, 1)
    return counts.reshape(K, C), int((~good & live).sum())


def count_brute(view, C):
    """the second formulation: bincount of the good ids per position"""
    N, K = view.shape
    counts = np.zeros((K, C), np.uint32)
    bad = 0
    for k in range(K):
        col = [int(x) for x in view[:, k]]
        good = [x for x in col if 0 <= x < C]
        bad += len(col) - len(good)
        if good:
            counts[k] = np.bincount(np.array(good, np.int64), minlength=C).astype(np.uint32)
    return counts, bad


def count_applies(mut, c, view):
    v = view.astype(np.int64)
    if c.N == 0:
        return False
    if mut == "swapped":                                            # uniform counts fill every cell of [K, C] alike: any permutation of the cells is invisible
        return c.K > 1 and c.kind != "uniform"
    if mut == "clamp":
        return bool(((v < 0) | (v >= c.C)).any())
    if mut == "no_elem_stride":
        return c.es > 1
    if mut == "drop_tail":
        return (c.N * c.K) % ROW_TILE != 0
    if mut == "u16_signed":                                         # a uint16 id with its top bit set that is a GOOD id: 65535 at C = 32768 is bad either way
        return c.dtype == "uint16" and bool(((v >= 32768) & (v < c.C)).any())
    raise KeyError(mut)


COUNT_MUTS = ("swapped", "clamp", "no_elem_stride", "drop_tail", "u16_signed")


def to_u16(view, mut=None):
    """-> (uint16 [N, K], bad): an id outside [0, 65535] packs as 0"""
    ids = view.view(np.int16) if (mut == "u16_signed" and view.dtype == np.uint16) else view
    v = ids.astype(np.int64)
    good = (v >= 0) & (v <= 65535)
    return np.where(good, v, 0).astype(np.uint16), int((~good).sum())


def _row_stats(cnt, mut=None):
    cnt = np.asarray(cnt, np.uint64)
    n = int(cnt.sum())
    if n == 0:
        return (0.0, 0.0, 0.0, 0.0, 0.0)
    nz = cnt[cnt > 0].astype(np.float64)
    p = nz / float(n)
    log = np.log2 if mut == "log2" else np.log
    H = -(p * log(p + (1e-10 if mut == "eps_in_H" else 0.0))).sum()
    H_ref = -(p * log(p + (0.0 if mut == "no_eps_ref" else 1e-10))).sum()
    used = int((cnt > 1).sum()) if mut == "used_gt1" else int((cnt > 0).sum())
    return (float(n), float(used), float(H) + 0.0, float(H_ref) + 0.0, float(cnt.max()))


def census(counts, mut=None):
    """counts [K, C] -> fp64 [K + 1, 5]"""
    K, C = counts.shape
    out = np.zeros((K + 1, 5))
    for k in range(K):
        out[k] = _row_stats(counts[k], mut)
    pooled = counts.astype(np.uint64).sum(0)
    out[K] = _row_stats(pooled, mut)
    if mut == "pooled_mean" and pooled.sum() > 0:                  # the entropies of the MEAN of the per-position distributions (positions without a token left out)
        n_k = counts.astype(np.uint64).sum(1).astype(np.float64)
        live = n_k > 0
        p = (counts[live].astype(np.float64) / n_k[live, None]).mean(0)
        nz = p[p > 0]
        out[K, 2] = -(nz * np.log(nz)).sum() + 0.0
        out[K, 3] = -(nz * np.log(nz + 1e-10)).sum() + 0.0
    return out


def census_brute(counts):
    """the second formulation: math.log and math.fsum over the non-zero counts, one row at a time"""
    K, C = counts.shape
    rows = [[int(x) for x in counts[k]] for k in range(K)]
    rows.append([sum(rows[k][c] for k in range(K)) for c in range(C)] if K * C <= 1 << 16 else [int(x) for x in counts.astype(np.uint64).sum(0)])
    out = np.zeros((K + 1, 5))
    for i, row in enumerate(rows):
        n = sum(row)
        if n == 0:
            continue
        nz = [x for x in row if x]
        out[i] = (n, len(nz), -math.fsum(x / n * math.log(x / n) for x in nz) + 0.0, -math.fsum(x / n * math.log(x / n + 1e-10) for x in nz) + 0.0, max(nz))
    return out


CENSUS_MUTS = ("log2", "eps_in_H", "no_eps_ref", "pooled_mean", "used_gt1")
H_TOL = 1e-10            # nats, absolute: C = 32768 terms of magnitude <= 0.37, each a few fp64 ulps of log off, is <= 8e-12; the tree on a sum <= 10.4 adds ~ 2e-14
PPL_RTOL = 1e-10
MOVE = 1e-9              # a planted census mistake moves an entropy it applies to by at least this, ten times the tolerance


def census_applies(mut, counts):
    """what the mistake can move by more than MOVE, decided on the counts: (row mask [K + 1], columns)"""
    K, C = counts.shape
    good = census(counts)
    n, used, H = good[:, 0], good[:, 1], good[:, 2]
    if mut == "log2":                                              # H / ln 2: visible wherever H is
        return H > 10 * MOVE, (2, 3)
    if mut in ("eps_in_H", "no_eps_ref"):                          # the 1e-10 moves an entropy by about used * 1e-10
        return used >= 100, (2,) if mut == "eps_in_H" else (3,)
    if mut == "used_gt1":
        rows = np.array([(counts[k] == 1).any() for k in range(K)] + [(counts.astype(np.uint64).sum(0) == 1).any()])
        return rows, (1,)
    if mut == "pooled_mean":                                       # BLIND when every live position has the same n: the mean of the distributions is then the pooled one
        n_k = n[:K][n[:K] > 0]
        rows = np.zeros(K + 1, bool)
        rows[K] = len(n_k) > 0 and not (n_k == n_k[0]).all()
        return rows, (2, 3)
    raise KeyError(mut)


# --------------------------------------------------------------------------------------------------------------------------------------------------
# agreement
# --------------------------------------------------------------------------------------------------------------------------------------------------
AgreeCase = collections.namedtuple("AgreeCase", "name N K k_lo k_hi kind")
AGREE_CASES = [
    AgreeCase("equal_n65_k40", 65, 40, 0, 40, "equal"),
    AgreeCase("flip0_n65_k40", 65, 40, 0, 40, "flip0"),
    AgreeCase("flipend_n65_k40", 65, 40, 0, 40, "flipend"),
    AgreeCase("flipboth_n65_k40", 65, 40, 0, 40, "flipboth"),
    AgreeCase("flipboth_cut_lo", 65, 40, 1, 40, "flipboth"),       # k_lo cuts the flip at index 0 off
    AgreeCase("flipboth_cut_hi", 65, 40, 0, 39, "flipboth"),       # k_hi cuts the flip at K - 1 off
    AgreeCase("flipboth_cut_both", 65, 40, 1, 39, "flipboth"),
    AgreeCase("random_n257_k512", 257, 512, 0, 512, "random"),
    AgreeCase("random_n300_k40_r", 300, 40, 7, 33, "random"),
    AgreeCase("random_n5_k1024", 5, 1024, 0, 1024, "random"),
    AgreeCase("random_n70_k1", 70, 1, 0, 1, "random"),
    AgreeCase("random_n70_k41_empty", 70, 41, 20, 20, "random"),
    AgreeCase("n0_k40", 0, 40, 0, 40, "random"),
]
AGREE_BY_NAME = {c.name: c for c in AGREE_CASES}


def make_agree(name):
    c = AGREE_BY_NAME[name]
    rng = np.random.default_rng(hash_name(name))
    a = rng.integers(0, 32768, size=(c.N, c.K)).astype(np.uint16)
    b = a.copy()
    rows = np.arange(c.N) % 3 != 1                                 # two rows of three are touched, the third stays equal
    if c.kind in ("flip0", "flipboth"):
        b[rows, 0] ^= 1
    if c.kind in ("flipend", "flipboth"):
        b[rows, c.K - 1] ^= 0x4000
    if c.kind == "random" and c.N:
        hit = rng.random((c.N, c.K)) < 0.05
        hit[0] = False                                             # one equal row
        hit[c.N - 1] = True                                        # one row that differs everywhere
        b = np.where(hit, (a + 1 + rng.integers(0, 100, size=a.shape)).astype(np.uint16) % 32768, a).astype(np.uint16)
    return a, b


def agree(a, b, k_lo, k_hi, mut=None):
    """-> (match_pos uint32 [K], n_diff, first_diff, last_diff int32 [N])"""
    N, K = a.shape
    hi = min(K, k_hi + 1) if mut == "k_hi_inclusive" else k_hi
    match_pos = np.zeros(K, np.uint32)
    n_diff, first, last = np.zeros(N, np.int32), np.full(N, K, np.int32), np.full(N, -1, np.int32)
    for r in range(N):
        d = [k for k in range(k_lo, hi) if a[r, k] != b[r, k]]
        for k in range(k_lo, hi):
            if a[r, k] == b[r, k]:
                match_pos[k] += 1
        n_diff[r] = len(d)
        if d:
            first[r], last[r] = d[0], d[-1]
    if mut == "swap_first_last":
        first, last = last, first
    return match_pos, n_diff, first, last


def agree_brute(a, b, k_lo, k_hi):
    """the second formulation: whole-matrix numpy"""
    N, K = a.shape
    ne = a != b
    ne[:, :k_lo] = False
    ne[:, k_hi:] = False
    inr = np.zeros(K, bool)
    inr[k_lo:k_hi] = True
    match_pos = ((~ne) & inr[None, :]).sum(0).astype(np.uint32)
    n_diff = ne.sum(1).astype(np.int32)
    idx = np.arange(K)[None, :]
    first = np.where(ne, idx, K).min(1, initial=K).astype(np.int32)
    last = np.where(ne, idx, -1).max(1, initial=-1).astype(np.int32)
    return match_pos, n_diff, first, last


AGREE_MUTS = ("swap_first_last", "k_hi_inclusive")


def agree_applies(mut, c, a, b):
    if c.N == 0:
        return False
    if mut == "swap_first_last":                                   # a row with exactly one differing position has first == last: blind; an equal row (K, -1) is not
        nd = agree(a, b, c.k_lo, c.k_hi)[1]
        return bool((nd != 1).any())
    if mut == "k_hi_inclusive":
        return c.k_hi < c.K
    raise KeyError(mut)


# --------------------------------------------------------------------------------------------------------------------------------------------------
# nearest
# --------------------------------------------------------------------------------------------------------------------------------------------------
NearCase = collections.namedtuple("NearCase", "name M N K k_lo k_hi self kind")


def _nc(M, N, K, k_range=None, self_=False, kind="c4", tag=""):
    k_lo, k_hi = (0, K) if k_range is None else k_range
    name = f"m{M}_n{N}_k{K}" + (f"_r{k_lo}_{k_hi}" if k_range else "") + ("_self" if self_ else "") + ("" if kind == "c4" else f"_{kind}") + tag
    return NearCase(name, M, N, K, k_lo, k_hi, self_, kind)


NEAR_CASES = [
    # the strip of 64 queries and the tile of 64 reference rows +- 1; the automatic split's edge at 8 tiles = 512 rows +- 1
    _nc(63, 63, 40), _nc(64, 64, 40), _nc(65, 65, 40), _nc(1, 127, 40), _nc(129, 128, 40), _nc(2, 129, 40),
    _nc(70, 511, 40), _nc(66, 512, 40), _nc(65, 513, 40), _nc(30, 577, 40),
    # every K: one chunk of 64 positions, 8 and 16 chunks; K = 1 can only match 0 or 1 position
    _nc(70, 130, 1, kind="k1"), _nc(66, 200, 512), _nc(5, 70, 1024), _nc(65, 130, 41),                        # K = 41: the halfword path
    # a bit-copied row planted at two reference indices: match = K, the lowest index wins
    _nc(65, 300, 40, kind="planted"), _nc(10, 600, 512, kind="planted"),
    # the set against itself, with and without duplicates
    _nc(130, 130, 40, self_=True), _nc(130, 130, 40, self_=True, kind="dups"), _nc(1, 1, 40, self_=True), _nc(66, 66, 41, self_=True, kind="dups"),
    # k_range: odd and even bounds on either path, an empty range
    _nc(65, 130, 40, (3, 37)), _nc(65, 130, 40, (2, 40)), _nc(65, 130, 41, (5, 41)), _nc(65, 130, 512, (65, 300)), _nc(9, 70, 40, (20, 20)),
    # nothing to search, nothing to ask
    _nc(65, 0, 40), _nc(0, 65, 40),
]
NEAR_BY_NAME = {c.name: c for c in NEAR_CASES}
FREE = 40                # positions of a K >= 512 case that vary from row to row (the others hold one id per column): the match counts keep the spread of K = 40
PLANT = (17, 230)        # reference indices of the planted bit-copies of query 0 (N >= 300)


def make_near(name):
    """(q, ref) uint16, ids from a code book of 4"""
    c = NEAR_BY_NAME[name]
    rng = np.random.default_rng(hash_name(name))

    def rows(n):
        x = np.broadcast_to(col, (n, c.K)).copy()
        x[:, free] = rng.integers(0, 4, size=(n, len(free)))
        return x.astype(np.uint16)

    col = rng.integers(0, 4, size=(1, c.K))
    lo, hi = c.k_lo, c.k_hi
    if c.K >= 512:                                                 # the free positions sit inside the range, its two ends included
        inner = np.arange(lo, hi)
        free = np.unique(np.concatenate([[lo, hi - 1], rng.choice(inner, FREE - 2, replace=False)]))
    else:
        free = np.arange(c.K)
    ref = rows(c.N)
    q = ref if c.self else rows(c.M)
    if c.kind == "planted":
        ref[PLANT[0]] = ref[PLANT[1]] = q[0]
    if c.kind == "dups":
        ref[10] = ref[3]
        ref[c.N - 1] = ref[3]
        ref[20] = ref[21]
    return q, ref


def _merge(cands, mut=None):
    """candidates (match, idx) of the reference parts -> one: most matches, then the lowest index"""
    cands = [x for x in cands if x[0] >= 0]
    if not cands:
        return (-1, 0)
    if mut == "merge_by_index":
        return min(cands, key=lambda x: x[1])
    return min(cands, key=lambda x: (-x[0], x[1]))


def nearest(q, ref, k_lo, k_hi, exclude_self=False, mut=None, parts=2):
    """-> (best_match, best_idx) int32 [M]; `parts` only matters to the planted merge mistake (the reference tiles in that many runs)"""
    M, N = q.shape[0], ref.shape[0]
    best, idx = np.full(M, -1, np.int32), np.zeros(M, np.int32)
    ntiles = -(-N // TILE)
    per = -(-ntiles // parts) * TILE if ntiles else 1
    for i in range(M):
        m = (ref[:, k_lo:k_hi] == q[i:i + 1, k_lo:k_hi]).sum(1).astype(np.int64)
        if exclude_self and mut != "self_included" and i < N:
            m[i] = -1
        cands = []
        for j0 in range(0, N, per):
            part = m[j0:j0 + per]
            top = int(part.max())
            where = np.flatnonzero(part == top)
            cands.append((top, j0 + int(where[-1] if mut == "highest_index" else where[0])))
        if mut == "highest_index" and cands:                       # ... across the parts as well
            top = max(x[0] for x in cands)
            best[i], idx[i] = (top, max(x[1] for x in cands if x[0] == top)) if top >= 0 else (-1, 0)
        else:
            best[i], idx[i] = _merge(cands, mut)
    return best, idx


def nearest_brute(q, ref, k_lo, k_hi, exclude_self=False):
    """the second formulation: one position at a time into an [M, N] count matrix, then the maximum of match * (N + 1) + (N - j)"""
    M, N = q.shape[0], ref.shape[0]
    if M == 0 or N == 0:
        return np.full(M, -1, np.int32), np.zeros(M, np.int32)
    cnt = np.zeros((M, N), np.int64)
    for k in range(k_lo, k_hi):
        cnt += q[:, k][:, None] == ref[:, k][None, :]
    key = cnt * (N + 1) + (N - np.arange(N))[None, :]
    if exclude_self:
        key[np.arange(min(M, N)), np.arange(min(M, N))] = -1
    top = key.max(1)
    best = np.where(top < 0, -1, top // (N + 1)).astype(np.int32)
    idx = np.where(top < 0, 0, N - top % (N + 1)).astype(np.int32)
    return best, idx


def tied(q, ref, k_lo, k_hi, exclude_self=False):
    """bool [M]: more than one reference row attains the best"""
    out = np.zeros(q.shape[0], bool)
    for i in range(q.shape[0]):
        m = (ref[:, k_lo:k_hi] == q[i:i + 1, k_lo:k_hi]).sum(1)
        if exclude_self:
            m[i] = -1
        out[i] = ref.shape[0] > 0 and (m == m.max()).sum() > 1
    return out


NEAR_MUTS = ("highest_index", "self_included", "merge_by_index")


def near_applies(mut, c, q, ref):
    if c.M == 0 or c.N == 0:
        return False
    if mut == "self_included":
        return c.self
    if c.self and c.N == 1:
        return False
    if mut == "highest_index":
        return bool(tied(q, ref, c.k_lo, c.k_hi, c.self).any())
    if mut == "merge_by_index":                                    # two runs of tiles, the first run's candidate always wins: visible iff some query's best sits in the second
        first_run = -(-(-(-c.N // TILE)) // 2) * TILE
        return bool((nearest(q, ref, c.k_lo, c.k_hi, c.self)[1] >= first_run).any())
    raise KeyError(mut)
