"""The rFID arithmetic of record restated on the host, and the case tables of tests/test_fid_cpu.py / tests/test_fid_gpu.py.

The emulation is the FID InceptionV3 in plain torch-CPU float64 (`conv2d`, the UNFOLDED `batch_norm` with eps 1e-3, `avg_pool2d(count_include_pad=False)`,
`max_pool2d`, `interpolate`, `torch.cat`) on the fp32 input, numpy float64 statistics and the Frechet formula (fid.FID_DEFINITION in code).
`pool3(..., dtype=torch.float32)` computes the FEATURES with torch's own fp32 kernels: the comparator the device gates are measured on.  No project kernel
is used as a reference; only fid.InceptionNet.synthetic_tensors (the hash-generated weights) and fid.UNITS (the geometry table) are shared.  The
network's structure is written here a second time (`network`), over pluggable unit / pool operations, so that tests/test_fid_gpu.py can run the SAME
structure on the device entries with tight outputs and `torch.cat` -- the staged calls the slice-writing product path is held to, bit for bit.

Every input is a function of the case name (synth.hash_uniform with a crc32 seed), so it regenerates on any host.
"""
from __future__ import annotations

import functools
import zlib
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

import image_io_cases as IO
from selftoktokenizer_amd import fid as FD, synth

U32 = 2.0 ** -24                                # fp32 unit roundoff
U = 2.0 ** -53                                  # fp64 unit roundoff
MUTS = ("count_include_pad", "avg_in_7c", "bn_eps_1e-5", "align_corners", "swap_1x7_7x1", "concat_order")
TAIL_MUTS = ("cov_1_over_n", "trace_term_without_2")


class Case(NamedTuple):
    name: str
    H: int
    W: int
    B: int
    content: str
    bf16: bool
    signed: bool
    quantize: bool
    resize: bool


CONTENTS = ("noise", "smooth", "const")


def _cases():
    out, k = [], 0
    for H, W in ((75, 75), (76, 75), (91, 107)):                  # maps 7^2 / 3^2 / 1^2, one more row, ragged 9x11 / 4x5 / 1x2 against the 64-row tile
        for B in (1, 3):
            for content in CONTENTS:
                bf, sg, qz = bool(k & 1), bool(k & 2), bool(k & 4)
                out.append(Case(f"{H}x{W}_b{B}_{content}_{'b' if bf else 'f'}{'s' if sg else 'u'}{'q' if qz else 'x'}", H, W, B, content, bf, sg, qz, False))
                k += 3                                            # walks all 8 dtype / sign / quantize combinations
    out.append(Case("64x64_b3_noise_bux_resize", 64, 64, 3, "noise", True, False, False, True))
    out.append(Case("256x256_b1_noise_fsq_resize", 256, 256, 1, "noise", False, True, True, True))
    out.append(Case("299x299_b1_smooth_fsx_resize", 299, 299, 1, "smooth", False, True, False, True))
    out.append(Case("320x200_b1_smooth_bux_resize", 320, 200, 1, "smooth", True, False, False, True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _u(seed, shape, lo, hi):
    return synth.hash_uniform(seed & 0xFFFFFFFF, shape, lo, hi).numpy().astype(np.float32)


def _smooth(seed, B, H, W):
    g = torch.from_numpy(_u(seed, (B, 3, H // 8 + 2, W // 8 + 2), 0.0, 1.0))
    return F.interpolate(g, size=(H, W), mode="bilinear", align_corners=True).numpy().astype(np.float32)


def images(content: str, seed: int, B: int, H: int, W: int):
    """[B, 3, H, W] fp32 in [0, 1]"""
    shape = (B, 3, H, W)
    if content == "noise":
        return _u(seed, shape, 0.0, 1.0)
    if content == "smooth":
        return _smooth(seed, B, H, W)
    if content == "const":
        return np.broadcast_to(_u(seed, (B, 3, 1, 1), 0.0, 1.0), shape).copy()
    raise KeyError(content)


def make(case: Case, seed: int = 0):
    """the case's images as an fp32 array [B, 3, H, W], in [-1, 1] when case.signed else in [0, 1], representable in the dtype the case names"""
    unit = images(case.content, zlib.crc32(case.name.encode()) + 7919 * seed, case.B, case.H, case.W)
    x = (unit * np.float32(2) - np.float32(1)).astype(np.float32) if case.signed else unit
    return np.ascontiguousarray(_bf16(x) if case.bf16 else x, np.float32)


# ---- the input stage ----
def to_signed(x, bf16: bool, signed: bool, quantize: bool):
    """the image as fp32 in [-1, 1], before the resize"""
    f32 = np.float32
    x = np.asarray(x, f32)
    with np.errstate(invalid="ignore"):
        if quantize:
            if signed:
                b = IO.to_u8_f32(((x + f32(1)) / f32(2)).astype(f32))
            else:
                b = IO.to_u8_bf16(IO.bf16_bits(x)) if bf16 else IO.to_u8_f32(x)
            return (((b.astype(f32) / f32(255)).astype(f32) * f32(2)).astype(f32) - f32(1)).astype(f32)
        return x if signed else ((x * f32(2)).astype(f32) - f32(1)).astype(f32)


def taps(n_in: int, n_out: int):
    """the tap table of one axis restated: (i0, i1, lambda fp32) from fp64"""
    i0, i1, lam = [], [], []
    for d in range(n_out):
        src = max(0.0, (d + 0.5) * (float(n_in) / float(n_out)) - 0.5)
        a = min(int(np.floor(src)), n_in - 1)
        i0.append(a); i1.append(min(a + 1, n_in - 1)); lam.append(np.float32(src - a))
    return np.array(i0, np.int32), np.array(i1, np.int32), np.array(lam, np.float32)


def resize(x, dtype=torch.float64, mut=None, side: int = FD.SIDE):
    """[N, 3, H, W] fp32 -> [N, 3, side, side] of `dtype`: torch's bilinear interpolate; a side x side image passes through"""
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    if tuple(t.shape[2:]) == (side, side):
        return t
    return F.interpolate(t, size=(side, side), mode="bilinear", align_corners=mut == "align_corners")


def resize_tables_f64(x, side: int = FD.SIDE):
    """the same resize from the tap tables, in numpy fp64 (exact products and sums of fp32 values up to fp64 rounding): what the device blend is held to"""
    x = np.asarray(x, np.float64)
    y0, y1, ly = taps(x.shape[2], side)
    x0, x1, lx = taps(x.shape[3], side)
    lx, ly = lx.astype(np.float64), ly.astype(np.float64)[:, None]
    top = x[:, :, y0][..., x0] + lx * (x[:, :, y0][..., x1] - x[:, :, y0][..., x0])
    bot = x[:, :, y1][..., x0] + lx * (x[:, :, y1][..., x1] - x[:, :, y1][..., x0])
    return top + ly * (bot - top)


RESIZE_TOL = 24 * U32
"""|device blend - resize_tables_f64| for values in [-1, 1], derived from the operation count: b - a (|.| <= 2) errs by 2u, lambda * (.) adds 2u, a + (.) (|.| <= 1)
adds u: a horizontal blend carries 5u.  bot - top inherits 10u and adds 2u, lambda * (.) adds 2u, top + (.) inherits top's 5u and adds u: 20u.  The table's
lambda is the fp32 rounding of the fp64 one in resize_tables_f64's twin `resize` (torch): 2u per axis, 4u.  24u, u = 2^-24."""


# ---- the network ----
@functools.lru_cache(maxsize=None)
def state(dtype=torch.float64):
    return {k: v.to(dtype) for k, v in FD.InceptionNet.synthetic_tensors().items()}


class TorchOps:
    """the unit and the pools in torch-CPU `dtype`, BatchNorm unfolded"""

    def __init__(self, dtype=torch.float64, mut=None):
        self.sd, self.mut = state(dtype), mut
        self.cat = lambda ts: torch.cat(ts, 1)

    def unit(self, name, x):
        _, _, kh, kw, s, ph, pw = FD.UNITS[name]
        w = self.sd[name + ".conv.weight"]
        if self.mut == "swap_1x7_7x1" and name == "Mixed_6b.branch7x7_2":
            w, ph, pw = w.transpose(2, 3), pw, ph
        y = F.conv2d(x, w, None, stride=s, padding=(ph, pw))
        bn = lambda leaf: self.sd[f"{name}.bn.{leaf}"]
        y = F.batch_norm(y, bn("running_mean"), bn("running_var"), bn("weight"), bn("bias"), False, 0.0, 1e-5 if self.mut == "bn_eps_1e-5" else 1e-3)
        return F.relu(y)

    def avg(self, x):
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=self.mut == "count_include_pad")

    def max_s1(self, x):
        return F.max_pool2d(x, 3, 1, 1)

    def max_s2(self, x):
        return F.max_pool2d(x, 3, 2)


def network(x, o, keep=None):
    """x [N, 3, H, W] in [-1, 1] -> Mixed_7c's map [N, 2048, h, w] over the operations `o` (unit, avg, max_s1, max_s2, cat, mut)"""
    mut = getattr(o, "mut", None)
    u = o.unit
    x = u("Conv2d_2b_3x3", u("Conv2d_2a_3x3", u("Conv2d_1a_3x3", x)))
    x = o.max_s2(x)
    x = u("Conv2d_4a_3x3", u("Conv2d_3b_1x1", x))
    x = o.max_s2(x)
    if keep is not None:
        keep["stem"] = x
    for b in FD.BLOCKS:
        c = lambda leaf, t: u(f"{b}.{leaf}", t)
        if b[:7] == "Mixed_5":
            br = [c("branch1x1", x), c("branch5x5_2", c("branch5x5_1", x)), c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x))), c("branch_pool", o.avg(x))]
            if mut == "concat_order" and b == "Mixed_5b":
                br[0], br[1] = br[1], br[0]
        elif b == "Mixed_6a":
            br = [c("branch3x3", x), c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x))), o.max_s2(x)]
        elif b[:7] == "Mixed_6":
            br = [c("branch1x1", x), c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x))),
                  c("branch7x7dbl_5", c("branch7x7dbl_4", c("branch7x7dbl_3", c("branch7x7dbl_2", c("branch7x7dbl_1", x))))), c("branch_pool", o.avg(x))]
        elif b == "Mixed_7a":
            br = [c("branch3x3_2", c("branch3x3_1", x)), c("branch7x7x3_4", c("branch7x7x3_3", c("branch7x7x3_2", c("branch7x7x3_1", x)))), o.max_s2(x)]
        else:
            t3, td = c("branch3x3_1", x), c("branch3x3dbl_2", c("branch3x3dbl_1", x))
            pool = o.max_s1(x) if (b == "Mixed_7c" and mut != "avg_in_7c") else o.avg(x)
            br = [c("branch1x1", x), c("branch3x3_2a", t3), c("branch3x3_2b", t3), c("branch3x3dbl_3a", td), c("branch3x3dbl_3b", td), c("branch_pool", pool)]
        x = o.cat(br)
        if keep is not None:
            keep[b] = x
    return x


def pool3(x, bf16, signed, quantize, resize_on, dtype=torch.float64, mut=None, keep=None):
    """images (fp32 array as `make` gives them) -> pool3 features [B, 2048] as a numpy array of `dtype`"""
    s = to_signed(x, bf16, signed, quantize)
    t = resize(s, dtype, mut) if resize_on else torch.from_numpy(s).to(dtype)
    if keep is not None:
        keep["input"] = t
    return network(t, TorchOps(dtype, mut), keep).mean((2, 3)).numpy()


@functools.lru_cache(maxsize=None)
def case_features(name: str, dtype=torch.float64, mut=None):
    """pool3 [B, 2048] of a case under the emulation; computed once per (case, variant) and shared by the tests -- read-only"""
    case = BY_NAME[name]
    v = pool3(make(case), case.bf16, case.signed, case.quantize, case.resize, dtype, mut)
    v.setflags(write=False)
    return v


def rel_err(f, ref):
    """per image ||f - ref|| / ||ref||"""
    f, ref = np.asarray(f, np.float64), np.asarray(ref, np.float64)
    return np.linalg.norm(f - ref, axis=1) / np.linalg.norm(ref, axis=1)


@functools.lru_cache(maxsize=None)
def fp32_relative_error() -> float:
    """the largest per-image relative error of torch-CPU fp32 running the same emulation against fp64, over the whole table: the pool3 gate is 4 x this"""
    return max(float(rel_err(case_features(c.name, torch.float32), case_features(c.name)).max()) for c in CASES)


# ---- the second, independent formulation: folded weights, explicit im2col + einsum, numpy fp64 ----
class NumpyOps:
    mut = None

    def __init__(self):
        sd = state()
        self.w = {}
        for name in FD.UNITS:
            g = sd[f"{name}.bn.weight"].numpy() / np.sqrt(sd[f"{name}.bn.running_var"].numpy() + 1e-3)
            self.w[name] = (sd[f"{name}.conv.weight"].numpy() * g[:, None, None, None], sd[f"{name}.bn.bias"].numpy() - sd[f"{name}.bn.running_mean"].numpy() * g)
        self.cat = lambda ts: np.concatenate(ts, 1)

    def unit(self, name, x):
        _, _, KH, KW, s, ph, pw = FD.UNITS[name]
        w, b = self.w[name]
        N, C, H, W = x.shape
        xp = np.zeros((N, C, H + 2 * ph, W + 2 * pw))
        xp[:, :, ph:ph + H, pw:pw + W] = x
        OH, OW = (H + 2 * ph - KH) // s + 1, (W + 2 * pw - KW) // s + 1
        cols = np.empty((N, C, KH, KW, OH, OW))
        for i in range(KH):
            for j in range(KW):
                cols[:, :, i, j] = xp[:, :, i:i + s * (OH - 1) + 1:s, j:j + s * (OW - 1) + 1:s]
        return np.maximum(np.einsum("ncijyx,ocij->noyx", cols, w, optimize=True) + b.reshape(1, -1, 1, 1), 0.0)

    @staticmethod
    def _windows(x, s, p, fill):
        N, C, H, W = x.shape
        xp = np.full((N, C, H + 2 * p, W + 2 * p), fill)
        xp[:, :, p:p + H, p:p + W] = x
        OH, OW = (H + 2 * p - 3) // s + 1, (W + 2 * p - 3) // s + 1
        return [xp[:, :, i:i + s * (OH - 1) + 1:s, j:j + s * (OW - 1) + 1:s] for i in range(3) for j in range(3)]

    def avg(self, x):
        return sum(self._windows(x, 1, 1, 0.0)) / sum(self._windows(np.ones_like(x), 1, 1, 0.0))

    def max_s1(self, x):
        return functools.reduce(np.maximum, self._windows(x, 1, 1, -np.inf))

    def max_s2(self, x):
        return functools.reduce(np.maximum, self._windows(x, 2, 0, -np.inf))


# ---- statistics and distance ----
def statistics(X, mut=None):
    """numpy fp64: mu [D], sigma [D, D] with 1 / (N - 1)"""
    X = np.asarray(X, np.float64)
    mu = X.mean(0)
    A = X - mu
    return mu, (A.T @ A) / (X.shape[0] if mut == "cov_1_over_n" else X.shape[0] - 1)


STATS_C, STATS_K = 2.0, 5.0


def stats_tolerance(X):
    """(tol_mu [D], tol_sigma [D, D]): bounds on |device - numpy|, both in fp64 (u = 2^-53), derived from the operation counts, no tuned factor.
    mu: a sum of N terms in ANY order errs by at most (N - 1) u sum|x|, the division adds u: (N u) mean|x| a side, two sides.
    sigma[i, j] = sum_n a_ni a_nj / (N - 1), a = x - mu: each a carries one rounding (u; the error of mu itself enters only in second order, because the
    exact a of a column sum to zero: N e_i e_j with |e| <= N u mean|x|, below u sum|a_i||a_j| whenever mean|x| <= 1e3 rms(a), which test_fid_cpu asserts
    of the matrices used -- one unit of k), so a product carries 2u, the fma chain and the tree add the N terms in some order, (N - 1) u, the division u:
    (N - 1 + 2 + 1 + 1) u = (N + 4 - 1) u, plus the second-order unit: k = 5 with one to spare, per side.  Two sides: c = 2.
    tol_sigma = c (N + k) u sum_n |a_ni| |a_nj| / (N - 1)."""
    X = np.asarray(X, np.float64)
    N = X.shape[0]
    A = np.abs(X - X.mean(0))
    return 2.0 * N * U * np.abs(X).mean(0), STATS_C * (N + STATS_K) * U * (A.T @ A) / (N - 1)


def frechet(mu1, s1, mu2, s2, mut=None):
    """the formula restated: symmetric square root of s1 by eigendecomposition (eigenvalues clamped at 0), eigenvalues of S s2 S"""
    w, V = np.linalg.eigh(s1)
    S = (V * np.sqrt(np.clip(w, 0.0, None))) @ V.T
    M = S @ s2 @ S
    lam = np.linalg.eigvalsh(0.5 * (M + M.T))
    tr = np.sqrt(np.clip(lam, 0.0, None)).sum()
    return float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - (1.0 if mut == "trace_term_without_2" else 2.0) * tr)


def stats_matrix(N: int, D: int):
    """[N, D] fp32: ReLU-like features (half of them zero), columns of different scale"""
    s = zlib.crc32(f"fid_stats_{N}x{D}".encode())
    x = np.maximum(_u(s, (N, D), -1.0, 1.0), 0) * (np.float32(0.25) + _u(s + 1, (1, D), 0.0, 2.0))
    return np.ascontiguousarray(x, np.float32)


# ---- end to end: two sets of 24 images at 75 x 75 ----
SET_N, SET_SIDE = 24, 75


def set_images(which: str):
    """the originals ("smooth", signed fp32) and the reconstructions ("noise", [0, 1] bf16) of the end-to-end case"""
    s = zlib.crc32(f"fid_set_{which}".encode())
    amp, mid = _u(s + 1, (SET_N, 1, 1, 1), 0.2, 1.0), _u(s + 2, (SET_N, 3, 1, 1), 0.3, 0.7)      # a contrast and a colour per image: the sets have a spread of their own
    unit = np.clip(mid + amp * (images(which, s, SET_N, SET_SIDE, SET_SIDE) - np.float32(0.5)), 0.0, 1.0).astype(np.float32)
    return (unit * np.float32(2) - np.float32(1)).astype(np.float32) if which == "smooth" else _bf16(unit)


@functools.lru_cache(maxsize=None)
def set_features(which: str, dtype=torch.float64, quantize=False):
    v = pool3(set_images(which), which == "noise", which == "smooth", quantize, False, dtype)
    v.setflags(write=False)
    return v


def set_distance(dtype=torch.float64, quantize=False, mut=None):
    """d^2 of the two sets: features in `dtype`, the tail in fp64 -- dtype=float32 is the comparator of the end-to-end gate"""
    m1, s1 = statistics(set_features("smooth", dtype, quantize), mut)
    m2, s2 = statistics(set_features("noise", dtype, quantize), mut)
    return frechet(m1, s1, m2, s2, mut)
