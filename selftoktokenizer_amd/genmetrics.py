"""Generative-model metrics beside FID: improved precision / recall (Kynkaanniemi et al. 2019, as the ADM evaluator computes them) on pool3 features and
the Inception Score on the 1008-way fc logits, on the project's own kernels (csrc/gen_metrics.hip): the N x N distance matrix is never stored, every
pairwise squared distance is a function of its two rows alone, bit for bit, and every reduction runs in a fixed order.

GEN_METRICS_DEFINITION states the metrics; tests/gen_metrics_cases.py restates them in numpy fp64.  Like the rFID figure (fid.py) the implementation is held
to the published definitions, not to the ADM evaluator or the published weights, neither of which is reachable here: unpinned against the evaluator.
sFID is not offered: its tap is an internal tensor of the TensorFlow graph (mixed_6/conv:0) whose counterpart in the pt_inception-2015-12-05 layout cannot
be established without either package or weights, and a guessed definition is worse than none.

Beside them, on the same features and the same pair arithmetic (csrc/gen_metrics_kdc.hip): density and coverage (Naeem et al. 2020), the nearest reference row of
every generated row, and the Kernel Inception Distance (Binkowski et al. 2018) with the polynomial kernel, the unbiased figure for small sample sets.  Their
definitions are restated from the papers and from memory of torch-fidelity / prdc: unpinned against either package.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops

K_DEFAULT = 3
K_MAX = 8
SPLIT_SIZE = 5000
CLASSES = 1008
KID_SUBSETS = 100
KID_SUBSET_SIZE = 1000
KID_SEED = 2020
KID_CHUNK_BYTES = 256 << 20

GEN_METRICS_DEFINITION = {
    "distance": "d2(u, v) = |u|^2 + |v|^2 - 2 u.v on fp32 rows, clamped at 0; SQUARED, never square-rooted: radii and tests are all in d2; the bits of d2(u, v) are "
                "a function of the two rows alone (one fp64 chain per norm rounded to fp32 once, one k-ascending fmaf chain per dot product, csrc/gen_metrics_shared.h)",
    "radius": "r2[j] = the k-th smallest d2(a_j, a_i) over i != j, the row's own index excluded by index, not by value (= entry k of the sorted row with self "
              "included); a NaN distance is never a neighbour; a row holding a NaN gets radius NaN and changes no other radius; N <= k is refused",
    "k": K_DEFAULT, "k_max": K_MAX,
    "membership": "member[i] = any_j d2(x_i, a_j) <= r2[j]: the set member's radius, <= (a point exactly on a radius is inside), false against NaN",
    "precision": "mean membership of the generated features in the reference manifold (reference radii)",
    "recall": "mean membership of the reference features in the generated manifold (generated radii)",
    "features": "pool3 of fid.FID_DEFINITION",
    "logits": "pool3 . W^T + b in fp32, 1008 classes, a 1 x 1 convolution on a 1 x 1 map on the fp32 convolution entry (its stated arithmetic)", "classes": CLASSES,
    "inception_score": "p = softmax(logits) in fp64 from the fp32 logits; consecutive splits of split_size rows, the last partial split included; per split "
                       "exp(mean_n sum_y p_ny (ln p_ny - ln mean_n p_ny)); the score is the mean over splits (no standard deviation is part of the figure)",
    "split_size": SPLIT_SIZE,
    "sfid": "not offered: the tap mixed_6/conv:0 of the TF graph has no established counterpart in the pt_inception-2015-12-05 layout",
    "pinned": "unpinned against the ADM evaluator and the published weights",
    "count": "count[i] = #{ j : d2(x_i, a_j) <= r2[j] }: the set member's radius, <= as the membership entry uses (prdc compares with <: a point exactly on a "
             "radius counts here and not there), false against NaN; the d2 bits are the membership entry's, so count > 0 is membership bit for bit",
    "nearest": "nn_d2[i] = min_j d2(x_i, a_j) over the non-NaN distances, nn_idx[i] = the lowest j whose d2 has those bits (the minimum of (bits of d2 << 32) | j as "
               "an unsigned 64-bit integer: exact and order-free); no non-NaN distance: nn_d2 = NaN, nn_idx = -1",
    "density": "sum_i count[i] / (k * M): queries the M generated rows, candidates the reference rows with their k-NN radii",
    "coverage": "mean_j [ nn_d2(ref_j against the generated set) <= r2_ref[j] ]: the REFERENCE row's own radius (the share of reference balls that hold a generated "
                "row), compared in fp32 with <= on the device values; integer counts are reported beside both fractions",
    "radii": "one k serves precision, recall, density and coverage; the reference radii are computed once per compare_sets call",
    "kid": "k(u, v) = (u.v / D + 1)^3, the dot product the shared fp32 chain, t = (double)c / (double)D + 1.0 and t * t * t in fp64; per subset of m rows of each "
           "set XX = sum_{i != j} k(x_i, x_j) (position i = j excluded by position, not by value), YY likewise, XY = sum_{i, j} k(x_i, y_j) with nothing excluded, "
           "mmd2 = (XX + YY) / (m (m - 1)) - 2 XY / m^2 (the unbiased estimator); kid = the mean over subsets, kid_std the population standard deviation (ddof 0); "
           "subsets drawn on the host: rng = numpy.random.RandomState(seed), per subset in order rng.choice(n_gen, m, replace=False) then "
           "rng.choice(n_ref, m, replace=False); m < 2 or m > min(n_ref, n_gen) is refused",
    "kid_subsets": KID_SUBSETS, "kid_subset_size": KID_SUBSET_SIZE, "kid_seed": KID_SEED,
    "pinned_kdc": "unpinned against torch-fidelity and prdc: restated from the papers",
}


def knn_radii(X: torch.Tensor, k: int = K_DEFAULT) -> torch.Tensor:
    """X [N, D] fp32 on the device -> r2 [N] fp32: the squared distance of every row to its k-th nearest other row (ops.knn_radius).  1 <= k <= 8, N > k,
    D a multiple of 16 up to 2048."""
    return ops.knn_radius(X, k)


def manifold_members(X: torch.Tensor, A: torch.Tensor, r2: torch.Tensor) -> torch.Tensor:
    """X [M, D] queries, A [N, D] with its radii r2 [N] -> bool [M] on the device: X[i] lies inside some A[j]'s ball (ops.manifold_member)"""
    return ops.manifold_member(X, A, r2) != 0


def precision_recall(ref_feats: torch.Tensor, gen_feats: torch.Tensor, k: int = K_DEFAULT) -> Dict:
    """ref_feats [N, D], gen_feats [M, D] fp32 on the device -> {"precision", "recall", "precision_count", "recall_count", "n_ref", "n_gen", "k"}:
    precision = the share of generated rows inside the reference manifold, recall = the share of reference rows inside the generated manifold"""
    if ref_feats.dim() != 2 or gen_feats.dim() != 2 or ref_feats.shape[1] != gen_feats.shape[1]:
        raise _lib.SelftokHipError(f"precision_recall: expected ref [N, D] and gen [M, D], got {tuple(ref_feats.shape)} and {tuple(gen_feats.shape)}")
    n_ref, n_gen = ref_feats.shape[0], gen_feats.shape[0]
    pc = int(manifold_members(gen_feats, ref_feats, knn_radii(ref_feats, k)).sum().item())
    rc = int(manifold_members(ref_feats, gen_feats, knn_radii(gen_feats, k)).sum().item())
    return {"precision": pc / n_gen, "recall": rc / n_ref, "precision_count": pc, "recall_count": rc, "n_ref": int(n_ref), "n_gen": int(n_gen), "k": int(k)}


def inception_score(logits: torch.Tensor, split_size: int = SPLIT_SIZE) -> float:
    """logits [N, C] fp32 on the device -> the Inception Score of GEN_METRICS_DEFINITION: the per-row KL values come from the device in fp64
    (ops.is_colmean, ops.is_kl_rows); their mean per split, exp and the mean over splits are numpy fp64 on the host"""
    split_size = int(split_size)
    kl = ops.is_kl_rows(logits, ops.is_colmean(logits, split_size), split_size).cpu().numpy()
    return float(np.mean([np.exp(kl[lo:lo + split_size].mean()) for lo in range(0, kl.size, split_size)]))


def nearest_neighbours(X: torch.Tensor, A: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """X [M, D] queries, A [N, D] -> (nn_idx int32 [M], nn_d2 fp32 [M]) on the device: the nearest row of A to every query by squared distance, the lowest index
    on equal bits; -1 / NaN for a query with no non-NaN distance (ops.manifold_count_nn without radii)"""
    _, d2, idx = ops.manifold_count_nn(X, A)
    return idx, d2


def ball_counts(X: torch.Tensor, A: torch.Tensor, r2: torch.Tensor):
    """X [M, D] queries, A [N, D] with its radii r2 [N] -> (count int32 [M], nn_d2 [M], nn_idx [M]): how many of A's balls hold X[i], and its nearest row of A"""
    return ops.manifold_count_nn(X, A, r2)


def coverage_count(ref_feats: torch.Tensor, gen_feats: torch.Tensor, r2_ref: torch.Tensor) -> int:
    """the number of reference rows whose own ball holds a generated row: nn_d2(ref_j against the generated set) <= r2_ref[j], fp32 on the device"""
    _, d2, _ = ops.manifold_count_nn(ref_feats, gen_feats)
    return int((d2 <= r2_ref).sum().item())


def density_coverage(ref_feats: torch.Tensor, gen_feats: torch.Tensor, k: int = K_DEFAULT, r2_ref: Optional[torch.Tensor] = None) -> Dict:
    """ref_feats [N, D], gen_feats [M, D] fp32 on the device -> {"density", "coverage", "density_count", "coverage_count", "n_ref", "n_gen", "k"}: density =
    density_count / (k M), density_count = the number of (generated row, reference ball) incidences; coverage = coverage_count / N, coverage_count = the
    reference rows whose own ball holds a generated row.  r2_ref: the reference radii when the caller holds them already."""
    if ref_feats.dim() != 2 or gen_feats.dim() != 2 or ref_feats.shape[1] != gen_feats.shape[1] or gen_feats.shape[0] < 1:
        raise _lib.SelftokHipError(f"density_coverage: expected ref [N, D] and gen [M >= 1, D], got {tuple(ref_feats.shape)} and {tuple(gen_feats.shape)}")
    n_ref, n_gen = ref_feats.shape[0], gen_feats.shape[0]
    r2 = knn_radii(ref_feats, k) if r2_ref is None else r2_ref
    count, _, _ = ball_counts(gen_feats, ref_feats, r2)
    dc = int(count.sum(dtype=torch.int64).item())
    cc = coverage_count(ref_feats, gen_feats, r2)
    return {"density": dc / (int(k) * n_gen), "coverage": cc / n_ref, "density_count": dc, "coverage_count": cc, "n_ref": int(n_ref), "n_gen": int(n_gen), "k": int(k)}


def kid_subsets(n_gen: int, n_ref: int, subsets: int = KID_SUBSETS, subset_size: int = KID_SUBSET_SIZE, seed: int = KID_SEED) -> Tuple[np.ndarray, np.ndarray]:
    """the host draw of GEN_METRICS_DEFINITION["kid"] -> (gen_idx, ref_idx), int64 [subsets, subset_size] each"""
    n_gen, n_ref, S, m = int(n_gen), int(n_ref), int(subsets), int(subset_size)
    if S < 1 or m < 2 or m > min(n_ref, n_gen):
        raise ValueError(f"kid: need subsets >= 1 and 2 <= subset_size <= min(n_ref, n_gen), got {S} subsets of {m} rows from {n_ref} reference and {n_gen} generated rows")
    rng = np.random.RandomState(int(seed))
    gi, ri = np.empty((S, m), np.int64), np.empty((S, m), np.int64)
    for s in range(S):
        gi[s] = rng.choice(n_gen, m, replace=False)
        ri[s] = rng.choice(n_ref, m, replace=False)
    return gi, ri


def kid_chunk(subset_size: int, D: int) -> int:
    """subsets per device call: the two gathered matrices of a chunk stay under KID_CHUNK_BYTES together"""
    return max(1, KID_CHUNK_BYTES // (2 * int(subset_size) * int(D) * 4))


def kid_of_sums(sums: np.ndarray, m: int) -> Tuple[float, float, np.ndarray]:
    """sums fp64 [S, 3] = (XX, YY, XY) -> (kid, kid_std, mmd2 [S]) in numpy fp64"""
    sums = np.asarray(sums, np.float64)
    mmd2 = (sums[:, 0] + sums[:, 1]) / (m * (m - 1)) - 2.0 * sums[:, 2] / (m * m)
    return float(np.mean(mmd2)), float(np.std(mmd2)), mmd2


def kid(ref_feats: torch.Tensor, gen_feats: torch.Tensor, subsets: int = KID_SUBSETS, subset_size: int = KID_SUBSET_SIZE, seed: int = KID_SEED,
        chunk: Optional[int] = None) -> Dict:
    """ref_feats [N, D], gen_feats [M, D] fp32 on the device -> {"kid", "kid_std", "kid_subsets", "kid_subset_size", "kid_seed"}.  The subsets are gathered with
    index_select (a copy) `chunk` subsets at a time (default kid_chunk: under 256 MB per call) and summed by ops.kid_sums; a subset's sums depend on its own
    rows alone, so the result does not depend on the chunking.  The tail (mmd2 per subset, mean, np.std) is numpy fp64 on the host."""
    if ref_feats.dim() != 2 or gen_feats.dim() != 2 or ref_feats.shape[1] != gen_feats.shape[1]:
        raise _lib.SelftokHipError(f"kid: expected ref [N, D] and gen [M, D], got {tuple(ref_feats.shape)} and {tuple(gen_feats.shape)}")
    S, m = int(subsets), int(subset_size)
    gi, ri = kid_subsets(gen_feats.shape[0], ref_feats.shape[0], S, m, seed)
    chunk = kid_chunk(m, ref_feats.shape[1]) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError(f"kid: chunk must be >= 1, got {chunk}")
    parts = []
    for lo in range(0, S, chunk):
        n = min(chunk, S - lo)
        xs = gen_feats.index_select(0, torch.from_numpy(gi[lo:lo + n].reshape(-1)).to(gen_feats.device))
        ys = ref_feats.index_select(0, torch.from_numpy(ri[lo:lo + n].reshape(-1)).to(ref_feats.device))
        parts.append(ops.kid_sums(xs, ys, n, m).cpu().numpy())
    mean, std, _ = kid_of_sums(np.concatenate(parts), m)
    return {"kid": mean, "kid_std": std, "kid_subsets": S, "kid_subset_size": m, "kid_seed": int(seed)}
