"""Generative-model metrics beside FID: improved precision / recall (Kynkaanniemi et al. 2019, as the ADM evaluator computes them) on pool3 features and
the Inception Score on the 1008-way fc logits, on the project's own kernels (csrc/gen_metrics.hip): the N x N distance matrix is never stored, every
pairwise squared distance is a function of its two rows alone, bit for bit, and every reduction runs in a fixed order.

GEN_METRICS_DEFINITION states the metrics; tests/gen_metrics_cases.py restates them in numpy fp64.  Like the rFID figure (fid.py) the implementation is held
to the published definitions, not to the ADM evaluator or the published weights, neither of which is reachable here: unpinned against the evaluator.
sFID is not offered: its tap is an internal tensor of the TensorFlow graph (mixed_6/conv:0) whose counterpart in the pt_inception-2015-12-05 layout cannot
be established without either package or weights, and a guessed definition is worse than none.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib, ops

K_DEFAULT = 3
K_MAX = 8
SPLIT_SIZE = 5000
CLASSES = 1008

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
