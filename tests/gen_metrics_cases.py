"""The definitions of record of selftoktokenizer_amd/genmetrics.py (GEN_METRICS_DEFINITION) restated in numpy fp64, the case table the CPU and GPU tests walk,
the error bound of the device's squared distance, and the planted mistakes the table must be able to see.

Squared distance: d2(u, v) = |u|^2 + |v|^2 - 2 u.v clamped at 0 -- never square-rooted.  The device takes the norms in fp64 (rounded to fp32 once) and the dot
product as one fp32 fmaf chain of length D, so against the real number
    |d2_device - d2| <= E(u, v) = (D + C_ERR) * 2^-24 * (|u|^2 + |v|^2),   C_ERR = 5.
The k-th order statistic of a row moves by at most the largest perturbation of any of its distances, so E (its largest value over the row) bounds a radius too.
A membership is DECIDED by the fp64 reference when every pair of the query is further than E from its radius, min_j (|d2 - r2_j| - E_ij) > 0; the other queries
are undecided, and the table is built so that they are at most 1 % of every random case, in both directions precision / recall walk
(tests/test_gen_metrics_cpu.py asserts it on the reference alone).  The planted cases (bit-copies, the exact tie, clusters, NaN rows) put queries ON radii on
purpose: they are held to agreement on their decided queries, the cluster cases to equal counts outright.
"""
from dataclasses import dataclass
from functools import lru_cache
from typing import Optional

import numpy as np

U24 = 2.0 ** -24
C_ERR = 5
CLASSES = 1008
UNDECIDED_MAX = 0.01


# ---- the definitions, numpy fp64 ----
def d2_matrix(X, A) -> np.ndarray:
    """the real number |u|^2 + |v|^2 - 2 u.v = sum_k (u_k - v_k)^2, taken in fp64 in the form without cancellation: a pair's value depends on its two rows
    alone (one numpy reduction per pair, whatever the matrices around it), it is symmetric, and bit-copies are exactly 0 apart.  A NaN is handed on."""
    X, A = np.asarray(X, np.float64), np.asarray(A, np.float64)
    out = np.empty((X.shape[0], A.shape[0]))
    for i in range(X.shape[0]):
        out[i] = ((A - X[i]) ** 2).sum(1)
    return out


def d2_brute(X, A) -> np.ndarray:
    """the double loop over pairs, in the definition's own form: |u|^2 + |v|^2 - 2 u.v clamped at 0, every sum a python loop over k"""
    X, A = np.asarray(X, np.float64), np.asarray(A, np.float64)
    out = np.empty((X.shape[0], A.shape[0]))
    nx = [sum(float(v) * float(v) for v in x) for x in X]
    na = [sum(float(v) * float(v) for v in a) for a in A]
    for i in range(X.shape[0]):
        for j in range(A.shape[0]):
            d = nx[i] + na[j] - 2.0 * float(np.dot(X[i], A[j]))
            out[i, j] = d if d != d else max(d, 0.0)
    return out


def bound(X, A) -> np.ndarray:
    """E[i, j] of the module docstring (NaN rows give NaN)"""
    X, A = np.asarray(X, np.float64), np.asarray(A, np.float64)
    return (X.shape[1] + C_ERR) * U24 * ((X * X).sum(1)[:, None] + (A * A).sum(1)[None, :]) + 1e-30


def kth_of_rows(d: np.ndarray, k: int, skip_self: bool) -> np.ndarray:
    """the k-th smallest non-NaN entry of every row (k counts from 1), the diagonal skipped BY INDEX when asked; NaN where a row has fewer than k"""
    d = np.array(d, np.float64)
    if skip_self:
        d[np.arange(d.shape[0]), np.arange(d.shape[0])] = np.nan
    d = np.sort(d, axis=1)                                       # NaNs last
    if k > d.shape[1]:
        return np.full(d.shape[0], np.nan)
    return d[:, k - 1].copy()


def radii(A, k: int, mut: Optional[str] = None) -> np.ndarray:
    d = d2_matrix(A, A)
    if mut == "self_included":
        return kth_of_rows(d, k, False)
    return kth_of_rows(d, k + 1 if mut == "k_plus_1" else k, True)


def members(X, A, r2, mut: Optional[str] = None, k: int = 3) -> np.ndarray:
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    if X.shape[0] == 0:
        return np.zeros(0, bool)
    d = d2_matrix(X, A)
    r2 = np.asarray(r2, np.float64)
    with np.errstate(invalid="ignore"):
        if mut == "lt":
            return (d < r2[None, :]).any(1)
        if mut == "query_radius":                                # the query's own radius inside its own set instead of the set member's
            return (d <= radii(X, k)[:, None]).any(1)
        if mut == "sqrt_radius":
            return (d <= np.sqrt(r2)[None, :]).any(1)
        return (d <= r2[None, :]).any(1)


def decided(X, A, r2) -> np.ndarray:
    """bool [M]: every pair of the query is further than E from its radius (pairs with a NaN on either side can never flip: NaN compares false)"""
    X = np.asarray(X, np.float64).reshape(-1, np.asarray(A).shape[1])
    if X.shape[0] == 0:
        return np.zeros(0, bool)
    with np.errstate(invalid="ignore"):
        gap = np.abs(d2_matrix(X, A) - np.asarray(r2, np.float64)[None, :]) - bound(X, A)
        return ~(gap <= 0.0).any(1)


def kth_neighbour(A, j: int, k: int):
    """(index of row j's k-th nearest other row, clear): clear when the k-th distance is more than 2 E away from the (k - 1)-th and the (k + 1)-th, so that
    the device, whose distances carry E each, must pick the same row"""
    d = d2_matrix(A[j:j + 1], A)[0]
    e = bound(A[j:j + 1], A)[0].max()
    d[j] = np.inf
    order = np.argsort(d, kind="stable")
    v = d[order]
    clear = (k < 2 or v[k - 1] - v[k - 2] > 2 * e) and (k >= len(A) - 1 or v[k] - v[k - 1] > 2 * e)
    return int(order[k - 1]), bool(clear)


def precision_recall(ref, gen, k: int = 3, mut: Optional[str] = None):
    pm = members(gen, ref, radii(ref, k, mut), mut, k)
    rm = members(ref, gen, radii(gen, k, mut), mut, k)
    if mut == "swapped":
        pm, rm = rm, pm
    return {"precision": float(pm.mean()), "recall": float(rm.mean()), "precision_count": int(pm.sum()), "recall_count": int(rm.sum()),
            "n_ref": len(ref), "n_gen": len(gen), "k": k}


def softmax64(logits) -> np.ndarray:
    x = np.asarray(logits, np.float32).astype(np.float64)
    e = np.exp(x - x.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def kl_rows(p: np.ndarray, q: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore", invalid="ignore"):
        t = p * (np.log(p) - np.log(q)[None, :])
    return np.where(p == 0.0, 0.0, t).sum(1)


def inception_score(logits, split_size: int = 5000, mut: Optional[str] = None) -> float:
    p = softmax64(logits)
    N = p.shape[0]
    los = list(range(0, N, split_size))
    if mut == "drop_partial" and N % split_size and N > split_size:
        los = los[:-1]
    kls = [kl_rows(p[lo:lo + split_size], (p if mut == "global_marginal" else p[lo:lo + split_size]).mean(0)).mean() for lo in los]
    if mut == "mean_before_exp":
        return float(np.exp(np.mean(kls)))
    return float(np.mean(np.exp(kls)))


def inception_score_brute(logits, split_size: int) -> float:
    """the double loop over rows and classes"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    N, C = x.shape
    p = np.empty_like(x)
    for n in range(N):
        e = [np.exp(x[n, y] - x[n].max()) for y in range(C)]
        z = sum(e)
        p[n] = [v / z for v in e]
    scores = []
    for lo in range(0, N, split_size):
        rows = range(lo, min(lo + split_size, N))
        q = [sum(p[n, y] for n in rows) / len(rows) for y in range(C)]
        kl = [sum(p[n, y] * (np.log(p[n, y]) - np.log(q[y])) for y in range(C) if p[n, y] != 0.0) for n in rows]
        scores.append(np.exp(sum(kl) / len(rows)))
    return float(sum(scores) / len(scores))


def is_tolerance(logits, split_size: int) -> float:
    """|device - numpy| allowed on the score: exp and log are within 2 ulp on either side, the row sums run over C terms and the column sums over at most
    split_size rows, each in another order on either side: every p, q carries (C + rows + 8) * 2^-53 relative, log p - log q that much absolute plus
    2^-52 * (|log p| + |log q|), and the score is exp(mean kl): relative error = absolute error of the mean kl.  A factor 4 covers both sides and the means."""
    p = softmax64(logits)
    rows = min(split_size, p.shape[0])
    with np.errstate(divide="ignore"):
        big = float(np.abs(np.log(np.maximum(p, 1e-300))).max())
    return 4.0 * ((p.shape[1] + rows + 8) * 2.0 ** -53 * (2.0 + big)) * inception_score(logits, split_size)


# ---- the case table ----
@dataclass(frozen=True)
class Case:
    name: str
    kind: str                 # "random": rows in a low-dimensional subspace; "dups", "tie", "clusters_p1r0", "clusters_p0r1", "nan": planted
    N: int                    # rows of the set A (the reference side of precision / recall)
    M: int                    # queries X (the generated side)
    D: int
    k: int
    dim: int = 3              # intrinsic dimension of the random rows
    scale: float = 1.0        # of the rows: squared radii far above 1 are where a square-rooted radius shows
    margin: bool = True       # the membership of this case is held to the <= 1 % undecided condition: every random case; the planted ones have their own claims


def _seed(name: str) -> int:
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def _subspace_rows(g, n, D, dim, basis=None):
    if basis is None:
        basis, _ = np.linalg.qr(g.standard_normal((D, dim)))
    return (g.standard_normal((n, dim)) @ basis.T).astype(np.float32), basis


@lru_cache(maxsize=None)
def make(name: str):
    """(A [N, D], X [M, D]) fp32 of a case"""
    c = BY_NAME[name]
    g = np.random.default_rng(_seed(name))
    A, basis = _subspace_rows(g, c.N, c.D, c.dim)
    X, _ = _subspace_rows(g, c.M, c.D, c.dim, basis)
    A, X = A * np.float32(c.scale), X * np.float32(c.scale)
    if c.kind == "dups":                                         # every third row a bit-copy of its predecessor, and queries that are bit-copies of rows
        A[2::3] = A[1:-1:3][: len(A[2::3])]
        X[::2] = A[: len(X[::2])]
    elif c.kind == "tie":                                        # query 0 is a bit-copy of the row that DEFINES row 0's radius: d2(x_0, a_0) = r2[0] exactly
        d = d2_matrix(A, A)
        d[np.arange(c.N), np.arange(c.N)] = np.inf
        X[0] = A[np.argsort(d[0], kind="stable")[c.k - 1]]
        X[1:] = X[1:] * 0.01 + (30.0 * basis[:, 0]).astype(np.float32)      # every other query far outside
    elif c.kind in ("clusters_p1r0", "clusters_p0r1"):
        # one side: two WIDE clusters 40 apart; the other side: one TIGHT cluster (1e-3) on the first one's centre.  Every tight row lies inside a wide row's
        # ball, no wide row inside a tight row's ball: reference wide / generated tight is precision 1, recall 0, and the reverse the other way round.
        far = (40.0 * basis[:, 0]).astype(np.float32)
        if c.kind == "clusters_p1r0":
            A[c.N // 2:] += far
            X = (X * np.float32(1e-3)).astype(np.float32)
        else:
            X[c.M // 2:] += far
            A = (A * np.float32(1e-3)).astype(np.float32)
    elif c.kind == "nan":
        A[5, 3] = np.nan; A[c.N - 1, 0] = np.nan
        if c.M > 2:
            X[2, 1] = np.nan
    A.setflags(write=False); X.setflags(write=False)
    return A, X


def _cases():
    out = []
    add = lambda *a, **kw: out.append(Case(*a, **kw))
    # the row / column tile (128) and its multiples, +-1; the automatic split's edge (9 tiles -> 2 splits of 5 and 4 tiles: column 640) and N = k + 1
    for n in (127, 128, 129, 255, 256, 257, 639, 640, 641):
        add(f"edge_n{n}_d16_k3", "random", n, 130, 16, 3)
    add("edge_n1100_d16_k3", "random", 1100, 300, 16, 3)
    add("small_n2_d16_k1", "random", 2, 5, 16, 1)
    add("small_n4_d16_k3", "random", 4, 5, 16, 3)
    add("small_n9_d64_k8", "random", 9, 5, 64, 8)
    add("k1_n300_d64", "random", 300, 257, 64, 1)
    add("k8_n300_d64", "random", 300, 129, 64, 8)
    add("scaled_n300_d64_k3", "random", 300, 257, 64, 3, scale=8.0)
    add("scaled_n129_d2048_k3", "random", 129, 40, 2048, 3, scale=8.0)
    add("m0_n129_d16_k3", "random", 129, 0, 16, 3)
    add("m1_n129_d64_k3", "random", 129, 1, 64, 3)
    add("wide_n40_d2048_k3", "random", 40, 40, 2048, 3)
    # at D = 2048 the bound is 2.4e-4 of the norms: the intrinsic dimension of these rows is the one at which the fp64 reference leaves <= 1 % undecided both ways
    add("wide_n300_d2048_k3", "random", 300, 129, 2048, 3, dim=5)
    add("wide_n129_d2048_k8", "random", 129, 64, 2048, 8, dim=8)
    add("wide_n257_d2048_k1", "random", 257, 257, 2048, 1, dim=5)
    add("dups_n130_d16_k3", "dups", 130, 40, 16, 3, margin=False)
    add("dups_n130_d2048_k1", "dups", 130, 40, 2048, 1, margin=False)
    add("tie_n257_d64_k3", "tie", 257, 33, 64, 3, margin=False)
    add("tie_n129_d2048_k8", "tie", 129, 9, 2048, 8, margin=False)
    add("clusters_p1r0_d64", "clusters_p1r0", 200, 150, 64, 3, margin=False)
    add("clusters_p0r1_d2048", "clusters_p0r1", 150, 130, 2048, 3, margin=False)
    add("nan_n200_d64_k3", "nan", 200, 70, 64, 3, margin=False)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
MUTS = ("self_included", "k_plus_1", "lt", "query_radius", "swapped", "sqrt_radius")


def mut_visible(mut: str, c: Case) -> bool:
    """which cases can see a planted mistake (the others are blind to it by construction, for the reason given)"""
    if c.M == 0 or c.kind == "nan":
        return False                                             # no query, or fractions that are compared elsewhere
    if mut == "lt":
        return c.kind == "tie"                                   # only a distance EXACTLY on a radius tells <= from <
    if mut == "swapped":
        return c.kind.startswith("clusters")                     # needs precision != recall by a margin
    if mut in ("self_included", "k_plus_1"):
        return True                                              # every radius changes (checked on the radii themselves)
    if mut == "query_radius":
        return c.M > c.k and c.kind.startswith("clusters")       # the two sets' radii must differ by orders of magnitude
    if mut == "sqrt_radius":
        return c.scale > 1.0                                     # squared radii far above 1, where the square root shrinks them across the distances
    return True


# ---- Inception Score cases: (N, split_size, C); every N with a split size that leaves a partial split ----
IS_CASES = ((2, 5000, CLASSES), (17, 5, CLASSES), (300, 128, CLASSES), (300, 299, 16), (1100, 512, CLASSES), (1100, 700, CLASSES))
IS_MUTS = ("drop_partial", "mean_before_exp", "global_marginal")


@lru_cache(maxsize=None)
def make_logits(N: int, C: int) -> np.ndarray:
    g = np.random.default_rng(_seed(f"logits_{N}_{C}"))
    x = (3.0 * g.standard_normal((N, C)) + np.linspace(0.0, 4.0, N)[:, None] * g.standard_normal(C)[None, :]).astype(np.float32)      # the rows drift: splits differ
    x.setflags(write=False)
    return x


def is_mut_visible(mut: str, N: int, split_size: int) -> bool:
    return N > split_size                                        # every planted mistake needs a second split (with N % split_size != 0 it is a partial one)
