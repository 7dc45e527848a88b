"""The definitions of record of density / coverage, the nearest-neighbour entry and KID (selftoktokenizer_amd/genmetrics.py, GEN_METRICS_DEFINITION) restated in
numpy fp64, the case tables the CPU and GPU tests walk, the derived error bounds, and the planted mistakes the tables must be able to see.  Restated from the
papers (Naeem et al. 2020, Binkowski et al. 2018) and from memory of prdc / torch-fidelity: unpinned against either package.

Count / nearest ride on tests/gen_metrics_cases.py: its cases (A the set, X the queries; for density / coverage A is the reference and X the generated set), its
fp64 d2 and its bound E(u, v) = (D + 5) 2^-24 (|u|^2 + |v|^2) on the device's d2.  The tests hand the SAME fp32 r2 array to the device and to the reference, so only d2
carries error:
    count     lo_i <= count_i <= hi_i, lo the pairs with d2 <= r2 - E, hi those with d2 <= r2 + E;
    nn_d2     within the row's largest E of the fp64 minimum (a minimum moves by at most the largest perturbation of its arguments);
    nn_idx    CLEAR when the fp64 runner-up is more than E_min + E_runner-up above the fp64 minimum: there the device must return the fp64 argmin;
    coverage  a reference row is DECIDED when |nn_d2 - r2| exceeds its largest E.
KID: the device's dot product c obeys |c - u.v| <= (D + 0.25) 2^-24 |u||v| (one fmaf chain of length D), so t = c / D + 1 carries delta = (D + 0.25) 2^-24 |u||v| / D and
a sum of P pairs taken in any fixed fp64 order lies within
    T = sum_pairs ((|t| + delta)^3 - |t|^3) + P 2^-52 sum |k|
of the real number; mmd2 is gated at (T_XX + T_YY) / (m (m - 1)) + 2 T_XY / m^2.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np

import gen_metrics_cases as GC

U24 = GC.U24
CAP = 0.01                                                        # of bracket width, unclear neighbours and undecided coverage rows on every random case
NN_CAP_EXEMPT = ("wide_n40_d2048_k3",)                            # one query of 40 (2.5 %) has an unclear neighbour and an undecided coverage row: held to its count claims only
MOVE = 100.0                                                      # a planted mistake moves a case that can see it by at least this many gates


# ---- count / nearest / density / coverage, numpy fp64 ----
def counts(X, A, r2, mut: Optional[str] = None) -> np.ndarray:
    """count[i] = #{ j : d2(x_i, a_j) <= r2[j] }, false against NaN"""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    if X.shape[0] == 0:
        return np.zeros(0, np.int64)
    d, r2 = GC.d2_matrix(X, A), np.asarray(r2, np.float64)
    with np.errstate(invalid="ignore"):
        inside = d < r2[None, :] if mut == "lt" else d <= r2[None, :]
    c = inside.sum(1).astype(np.int64)
    return np.minimum(c, 1) if mut == "any_flag" else c


def count_brackets(X, A, r2):
    """(lo, hi) int64 [M]: the pairs inside by more than E, and those not outside by more than E"""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    if X.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    d, e, r2 = GC.d2_matrix(X, A), GC.bound(X, A), np.asarray(r2, np.float64)[None, :]
    with np.errstate(invalid="ignore"):
        return (d <= r2 - e).sum(1).astype(np.int64), (d <= r2 + e).sum(1).astype(np.int64)


def nearest(X, A, mut: Optional[str] = None):
    """(nn_d2 fp64 [M], nn_idx int64 [M]): the smallest non-NaN distance and the lowest index that has it; NaN / -1 without one"""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    M = X.shape[0]
    nd, ni = np.full(M, np.nan), np.full(M, -1, np.int64)
    if M == 0:
        return nd, ni
    d = GC.d2_matrix(X, A)
    for i in range(M):
        ok = np.flatnonzero(~np.isnan(d[i]))
        if ok.size:
            v = d[i, ok].min()
            hits = ok[d[i, ok] == v]
            nd[i], ni[i] = v, (hits[-1] if mut == "highest_index" else hits[0])
    return nd, ni


def nearest_clear(X, A):
    """(clear bool [M], E_row [M]): the fp64 runner-up is more than E_min + E_runner-up above the fp64 minimum (a lone candidate is clear; a query with no
    non-NaN distance is clear: -1 is the only answer); E_row the largest E of the query's row"""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    M = X.shape[0]
    clear, e_row = np.ones(M, bool), np.zeros(M)
    if M == 0:
        return clear, e_row
    d, e = GC.d2_matrix(X, A), GC.bound(X, A)
    for i in range(M):
        ok = np.flatnonzero(~np.isnan(d[i]))
        if ok.size:
            e_row[i] = e[i, ok].max()
        if ok.size >= 2:
            order = ok[np.argsort(d[i, ok], kind="stable")]
            j0, j1 = order[0], order[1]
            clear[i] = d[i, j1] - d[i, j0] > e[i, j0] + e[i, j1]
    return clear, e_row


def density(ref, gen, r2_ref, k: int, mut: Optional[str] = None):
    """(density, density_count): queries the generated rows, candidates the reference rows with their radii"""
    c = counts(gen, ref, r2_ref, mut)
    total = int(c.sum())
    return total / ((1 if mut == "div_m" else k) * len(gen)), total


def coverage(ref, gen, r2_ref, k: int, mut: Optional[str] = None):
    """(coverage, coverage_count): the share of reference rows whose OWN ball holds a generated row"""
    nd, ni = nearest(ref, gen)
    r = np.asarray(r2_ref, np.float64)
    if mut == "candidate_radius":                                # the generated row's radius inside the generated set instead of the reference row's own
        rg = GC.radii(gen, k) if len(gen) > k else np.full(len(gen), np.nan)
        r = np.where(ni >= 0, rg[np.maximum(ni, 0)], np.nan)
    with np.errstate(invalid="ignore"):
        inside = nd < r if mut == "lt" else nd <= r
    return float(inside.mean()), int(inside.sum())


def coverage_decided(ref, gen, r2_ref) -> np.ndarray:
    """bool [N]: |nn_d2 - r2| exceeds the row's largest E (a row whose nn_d2 or r2 is NaN can never flip)"""
    nd, _ = nearest(ref, gen)
    _, e_row = nearest_clear(ref, gen)
    with np.errstate(invalid="ignore"):
        return ~(np.abs(nd - np.asarray(r2_ref, np.float64)) <= e_row)


def coverage_settled(ref, gen, r2_ref) -> np.ndarray:
    """bool [N], pair by pair: the row is outside whatever the device's error (every d2 - E > r2) or inside whatever it is (some d2 + E <= r2).  Every DECIDED
    row is settled (|min d2 - r2| > the largest E implies either); the reverse fails where one far generated row inflates the row's largest E, as on the cluster
    cases, whose integers are demanded outright on this criterion"""
    ref = np.asarray(ref, np.float64)
    d, e, r = GC.d2_matrix(ref, gen), GC.bound(ref, gen), np.asarray(r2_ref, np.float64)[:, None]
    with np.errstate(invalid="ignore"):
        return ~(d - e <= r).any(1) | (d + e <= r).any(1)


def counts_brute(X, A, r2) -> np.ndarray:
    d = GC.d2_brute(X, A)
    return np.array([sum(1 for j in range(d.shape[1]) if d[i, j] <= r2[j]) for i in range(d.shape[0])], np.int64)


def nearest_brute(X, A):
    d = GC.d2_brute(X, A)
    nd, ni = np.full(d.shape[0], np.nan), np.full(d.shape[0], -1, np.int64)
    for i in range(d.shape[0]):
        for j in range(d.shape[1]):
            if d[i, j] == d[i, j] and (ni[i] < 0 or d[i, j] < nd[i]):
                nd[i], ni[i] = d[i, j], j
    return nd, ni


@lru_cache(maxsize=None)
def r2_f32(name: str) -> np.ndarray:
    """the fp32 radii array BOTH sides of a count test read: the fp64 radii of the case's set, rounded once"""
    c = GC.BY_NAME[name]
    r = GC.radii(GC.make(name)[0], c.k).astype(np.float32)
    r.setflags(write=False)
    return r


DC_MUTS = ("lt", "candidate_radius", "div_m", "any_flag", "highest_index")


def dc_applies(mut: str, c) -> bool:
    """which count / nearest cases can see a planted mistake"""
    if c.M == 0 or c.kind == "nan":
        return False                                             # no query, or figures that are compared elsewhere
    if mut == "lt":
        return c.kind == "tie"                                   # only a distance EXACTLY on a radius tells <= from <
    if mut == "candidate_radius":
        return c.kind.startswith("clusters")                     # the two sets' radii must differ by orders of magnitude
    if mut == "div_m":
        return c.k > 1 and c.kind in ("random", "clusters_p1r0")          # k = 1 divides by the same number; a density of 0 stays 0
    if mut == "any_flag":
        return c.k > 1 and c.kind in ("random", "clusters_p1r0")          # needs queries inside more than one ball: k-NN balls overlap about k deep
    if mut == "highest_index":
        return c.kind == "dups"                                  # needs two candidates at a distance of equal bits: bit-copied rows
    return True


# ---- KID, numpy fp64 ----
def _kernel(G, D: int, mut: Optional[str]):
    g = G if mut == "gamma_1" else G / float(D)
    t = g if mut == "no_plus_1" else g + 1.0
    return t * t if mut == "degree_2" else t * t * t


def kid_sums64(xs, ys, S: int, m: int, mut: Optional[str] = None) -> np.ndarray:
    """fp64 [S, 3] = (XX, YY, XY) of the subsets' rows s m .. s m + m - 1: XX and YY without the positions i == j"""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    D = xs.shape[1]
    out = np.empty((S, 3))
    for s in range(S):
        x, y = xs[s * m:(s + 1) * m], ys[s * m:(s + 1) * m]
        if mut == "padded_by_value":                             # rows padded to the 128-row tile with zeros and never masked: (0 + 1)^3 = 1 per pair
            pad = np.zeros((-m % 128, D))
            x, y = np.concatenate([x, pad]), np.concatenate([y, pad])
        off = np.ones((len(x), len(x)), bool) if mut == "diag_included" else ~np.eye(len(x), dtype=bool)
        out[s] = [_kernel(x @ x.T, D, mut)[off].sum(), _kernel(y @ y.T, D, mut)[off].sum(), _kernel(x @ y.T, D, mut).sum()]
    return out


def kid_sums_brute(xs, ys, S: int, m: int) -> np.ndarray:
    """the double loop over positions"""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    D = xs.shape[1]
    k = lambda u, v: (float(np.dot(u, v)) / D + 1.0) ** 3
    out = np.zeros((S, 3))
    for s in range(S):
        x, y = xs[s * m:(s + 1) * m], ys[s * m:(s + 1) * m]
        for i in range(m):
            for j in range(m):
                if i != j:
                    out[s, 0] += k(x[i], x[j]); out[s, 1] += k(y[i], y[j])
                out[s, 2] += k(x[i], y[j])
    return out


def mmd2_of(sums, m: int, mut: Optional[str] = None) -> np.ndarray:
    sums = np.asarray(sums, np.float64)
    den = m * m if mut == "biased" else m * (m - 1)
    return (sums[:, 0] + sums[:, 1]) / den - 2.0 * sums[:, 2] / (m * m)


def kid_sum_bounds(xs, ys, S: int, m: int) -> np.ndarray:
    """T [S, 3] of the module docstring (NaN for a sum that holds a NaN row)"""
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    D = xs.shape[1]
    out = np.empty((S, 3))
    for s in range(S):
        x, y = xs[s * m:(s + 1) * m], ys[s * m:(s + 1) * m]
        nx, ny = np.sqrt((x * x).sum(1)), np.sqrt((y * y).sum(1))
        off = ~np.eye(m, dtype=bool)
        for w, (u, v, nu, nv, mask) in enumerate(((x, x, nx, nx, off), (y, y, ny, ny, off), (x, y, nx, ny, np.ones((m, m), bool)))):
            t = np.abs(u @ v.T / D + 1.0)[mask]
            delta = ((D + 0.25) * U24 * nu[:, None] * nv[None, :] / D)[mask]
            out[s, w] = ((t + delta) ** 3 - t ** 3).sum() + t.size * 2.0 ** -52 * (t ** 3).sum()
    return out


def mmd2_gate(T, m: int) -> np.ndarray:
    T = np.asarray(T, np.float64)
    return (T[:, 0] + T[:, 1]) / (m * (m - 1)) + 2.0 * T[:, 2] / (m * m)


def kid_draw(n_gen: int, n_ref: int, subsets: int, m: int, seed: int, mut: Optional[str] = None):
    """the host draw: per subset in order, the generated rows first, then the reference rows"""
    rng = np.random.RandomState(seed)
    gi, ri = [], []
    for _ in range(subsets):
        if mut == "draw_swapped":
            ri.append(rng.choice(n_ref, m, replace=False)); gi.append(rng.choice(n_gen, m, replace=False))
        else:
            gi.append(rng.choice(n_gen, m, replace=False)); ri.append(rng.choice(n_ref, m, replace=False))
    return np.array(gi), np.array(ri)


def kid64(ref, gen, subsets: int, m: int, seed: int, mut: Optional[str] = None):
    """{"kid", "kid_std", "mmd2", "gate"}: gate [subsets] the mmd2 gates of the drawn subsets"""
    gi, ri = kid_draw(len(gen), len(ref), subsets, m, seed, mut)
    xs, ys = np.asarray(gen)[gi.reshape(-1)], np.asarray(ref)[ri.reshape(-1)]
    v = mmd2_of(kid_sums64(xs, ys, subsets, m, mut), m, mut)
    return {"kid": float(np.mean(v)), "kid_std": float(np.std(v, ddof=1 if mut == "sample_std" else 0)), "mmd2": v,
            "gate": mmd2_gate(kid_sum_bounds(xs, ys, subsets, m), m)}


@dataclass(frozen=True)
class KidCase:
    name: str
    m: int
    D: int
    S: int
    kind: str = "random"      # "random"; "copies": bit-copied rows at two positions of a subset (they count: only POSITION i = j is excluded); "nan": a NaN row in one subset
    scale: float = 1.0
    dim: int = 8


def _kid_cases():
    out = []
    add = lambda *a, **kw: out.append(KidCase(*a, **kw))
    # the 128-row tile and its multiples +-1 (127 .. 130, 257), the smallest subsets (2, 5), every D of the parent's table, one and three subsets
    add("kid_m2_d16_s1", 2, 16, 1)
    add("kid_m5_d64_s3", 5, 64, 3)
    add("kid_m127_d16_s1", 127, 16, 1)
    add("kid_m128_d64_s1", 128, 64, 1)
    add("kid_m128_d2048_s1", 128, 2048, 1)
    add("kid_m129_d16_s3", 129, 16, 3)
    add("kid_m129_d2048_s3", 129, 2048, 3)
    add("kid_m130_d2048_s1", 130, 2048, 1)
    add("kid_m257_d64_s1", 257, 64, 1)
    add("kid_m257_d16_s3", 257, 16, 3)
    add("kid_copies_m129_d64_s1", 129, 64, 1, kind="copies")
    add("kid_nan_m130_d16_s3", 130, 16, 3, kind="nan")
    add("kid_scaled_m129_d64_s1", 129, 64, 1, scale=8.0)
    return out


KID_CASES = _kid_cases()
KID_BY_NAME = {c.name: c for c in KID_CASES}
NAN_SUBSET = 1                                                    # of the "nan" case: the subset whose x rows hold the NaN
KID_SUM_MUTS = ("diag_included", "padded_by_value", "biased", "degree_2", "no_plus_1", "gamma_1")
KID_FIGURE_MUTS = ("sample_std", "draw_swapped")
KID_MUTS = KID_SUM_MUTS + KID_FIGURE_MUTS
# whole figures: (n_ref, n_gen, D, subsets, m) -- rows of sets() below, subsets drawn by the host rule
KID_SET_CASES = ((300, 257, 64, 4, 130), (230, 200, 16, 3, 150), (140, 150, 2048, 2, 129))


def sets(n_ref: int, n_gen: int, D: int, dim: int = 8, scale: float = 1.0, seed_name: str = "kid_sets"):
    """(ref [n_ref, D], gen [n_gen, D]) fp32: unit-scale rows of one `dim`-dimensional subspace, the reference N(0, I) and the generated 1.5 N(0, I) + 1 in its basis"""
    g = np.random.default_rng(GC._seed(f"{seed_name}_{n_ref}_{n_gen}_{D}"))
    ref, basis = GC._subspace_rows(g, n_ref, D, dim)
    gen, _ = GC._subspace_rows(g, n_gen, D, dim, basis)
    gen = (1.5 * gen.astype(np.float64) + basis.sum(1)[None, :]).astype(np.float32)
    ref, gen = ref * np.float32(scale), gen * np.float32(scale)
    return ref, gen


@lru_cache(maxsize=None)
def kid_make(name: str):
    """(xs, ys) fp32 [S m, D] of a case: xs the generated rows, ys the reference rows, subset s in rows s m .. s m + m - 1"""
    c = KID_BY_NAME[name]
    ys, xs = sets(c.S * c.m, c.S * c.m, c.D, c.dim, c.scale, name)
    if c.kind == "copies":
        xs[7] = xs[3]; xs[c.m - 1] = xs[3]; ys[c.m - 2] = ys[0]
    elif c.kind == "nan":
        xs[NAN_SUBSET * c.m + 4, 2] = np.nan
    xs.setflags(write=False); ys.setflags(write=False)
    return xs, ys


def kid_applies(mut: str, c: KidCase) -> bool:
    """which KID cases can see a planted mistake"""
    if c.kind == "nan":
        return False                                             # its figures are compared elsewhere
    if mut == "padded_by_value":
        return c.m % 128 != 0 and c.scale == 1.0                 # a subset that fills its tiles has no padded row; at 8 x the kernel values are in the thousands and a padded pair adds 1
    return True


def kid_figure_applies(mut: str, case) -> bool:
    """which rows of KID_SET_CASES can see a mistake in the figure's tail (KID_FIGURE_MUTS): both show through the SPREAD of mmd2 between subsets, which shrinks
    like 1 / D while the gate (an absolute error of t = c / D + 1 near 1) does not: at D = 2048 the spread is a few gates"""
    n_ref, n_gen, D, subsets, m = case
    return subsets > 1 and m < min(n_ref, n_gen) and D <= 64
