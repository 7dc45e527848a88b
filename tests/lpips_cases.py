"""The LPIPS-AlexNet arithmetic of record restated on the host, and the case tables of tests/test_lpips_cpu.py / tests/test_lpips_gpu.py.

The emulation is plain torch-CPU `conv2d` / `max_pool2d` in float64 on the fp32 input of the scaling layer, then numpy float64 for the
distance (lpips.LPIPS_DEFINITION in code).  `emulate(..., dtype=torch.float32)` is the switch that computes the FEATURES in fp32 (torch's own
fp32 convolution) and everything after them in fp64: the comparator the end-to-end gate is measured on, and the form the distance stage is
fed.  No project kernel is used as a reference; only lpips.LpipsNet.synthetic_tensors (the hash-generated weights) is shared.

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
from selftoktokenizer_amd import synth
from selftoktokenizer_amd.lpips import LAYERS, LpipsNet

SHIFT = np.array([-0.030, -0.088, -0.188], np.float32)
SCALE = np.array([0.458, 0.448, 0.450], np.float32)
EPS = 1e-10
U = 2.0 ** -53                                  # fp64 unit roundoff

MUTS = ("eps_inside", "no_scaling", "pre_relu", "ceil_pool", "conv1_pad0", "spatial_sum", "normalize_after")


class Case(NamedTuple):
    name: str
    H: int
    W: int
    B: int
    content: str
    recon_bf16: bool
    orig_bf16: bool
    signed: bool
    quantize: bool


CONTENTS = ("noise", "smooth", "recon_noise", "identical", "const")
GATED_CONTENTS = ("noise", "smooth")            # cases whose EVERY pair must have d >= D_GATED (a condition on the table, checked by test_lpips_cpu)
D_GATED = 0.05                                  # the end-to-end relative gate applies to every pair of every case at or above this, `const` and
                                                # `recon_noise` pairs included (gated_pairs); below it the two stage gates cover the pair


def _cases():
    out = []
    geoms = [(31, 31, 1), (31, 31, 5), (35, 47, 3), (67, 95, 1), (64, 64, 3), (67, 95, 3), (35, 47, 5), (64, 64, 1)]
    k = 0
    for H, W, B in geoms:
        for content in CONTENTS:
            rb, ob, sg, qz = bool(k & 1), bool(k & 2), not (k & 4), bool(k & 8)
            if content == "identical" and qz and rb:
                rb = False                        # a bf16 image and its fp32 twin do not quantize to the same byte everywhere
            out.append(Case(f"{H}x{W}_b{B}_{content}_{'b' if rb else 'f'}{'b' if ob else 'f'}{'s' if sg else 'u'}{'q' if qz else 'x'}", H, W, B, content, rb, ob, sg, qz))
            k += 3                                # walks all 16 dtype / sign / quantize combinations
    out.append(Case("256x256_b2_noise_bfsx", 256, 256, 2, "noise", True, False, True, False))
    out.append(Case("256x256_b1_recon_noise_ffsq", 256, 256, 1, "recon_noise", False, False, True, True))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
GATED = [c for c in CASES if c.content in GATED_CONTENTS]


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _u(seed, shape, lo, hi):
    return synth.hash_uniform(seed & 0xFFFFFFFF, shape, lo, hi).numpy().astype(np.float32)


def _smooth(seed, B, H, W):
    g = torch.from_numpy(_u(seed, (B, 3, H // 8 + 2, W // 8 + 2), 0.0, 1.0))
    return F.interpolate(g, size=(H, W), mode="bilinear", align_corners=True).numpy().astype(np.float32)


def make(case: Case, seed: int = 0):
    """(recon [B, 3, H, W] in [0, 1], original in [-1, 1] when case.signed else in [0, 1]) as fp32 arrays, representable in the dtype the case names"""
    s = zlib.crc32(case.name.rsplit("_", 1)[0].encode()) + 7919 * seed
    shape = (case.B, 3, case.H, case.W)
    if case.content == "noise":
        recon, unit = _u(s, shape, 0.0, 1.0), _u(s + 1, shape, 0.0, 1.0)
    elif case.content == "smooth":
        recon, unit = _smooth(s, case.B, case.H, case.W), _smooth(s + 1, case.B, case.H, case.W)
    elif case.content == "recon_noise":
        unit = 0.5 * _smooth(s, case.B, case.H, case.W) + 0.5 * _u(s + 1, shape, 0.0, 1.0)
        recon = np.clip(unit + _u(s + 2, shape, -0.02, 0.02), 0.0, 1.0).astype(np.float32)
    elif case.content == "identical":
        unit = np.floor(_u(s, shape, 0.0, 256.0)).clip(0, 255).astype(np.float32) / np.float32(256)      # k / 256: v * 2 - 1 is exact, in bf16 too
        recon = unit.copy()
    elif case.content == "const":
        c = _u(s, (case.B, 3, 1, 1), 0.0, 1.0)
        unit = np.broadcast_to(c, shape).copy()
        recon = np.broadcast_to(_u(s + 1, (case.B, 3, 1, 1), 0.0, 1.0), shape).copy()
    else:
        raise KeyError(case.content)
    orig = (unit * np.float32(2) - np.float32(1)).astype(np.float32) if case.signed else unit
    if case.recon_bf16:
        recon = _bf16(recon)
    if case.orig_bf16:
        orig = _bf16(orig)
    return np.ascontiguousarray(recon, np.float32), np.ascontiguousarray(orig, np.float32)


# ---- the input stage ----
def to_signed(recon, orig, recon_bf16: bool, signed: bool, quantize: bool):
    """both images as fp32 in [-1, 1], before the scaling layer"""
    f32 = np.float32
    recon, orig = np.asarray(recon, f32), np.asarray(orig, f32)
    if quantize:
        bx = IO.to_u8_bf16(IO.bf16_bits(recon)) if recon_bf16 else IO.to_u8_f32(recon)
        with np.errstate(invalid="ignore"):
            o = ((orig + f32(1)) / f32(2)).astype(f32) if signed else orig
        by = IO.to_u8_f32(o)
        q = lambda b: ((b.astype(f32) / f32(255)).astype(f32) * f32(2)).astype(f32) - f32(1)
        return q(bx), q(by)
    with np.errstate(invalid="ignore"):
        x0 = (recon * f32(2)).astype(f32) - f32(1)
        x1 = orig if signed else (orig * f32(2)).astype(f32) - f32(1)
    return x0.astype(f32), x1.astype(f32)


def scaling_layer(x):
    with np.errstate(invalid="ignore"):
        return ((np.asarray(x, np.float32) - SHIFT.reshape(1, 3, 1, 1)).astype(np.float32) / SCALE.reshape(1, 3, 1, 1)).astype(np.float32)


def input_stage(recon, orig, recon_bf16, signed, quantize):
    """[2B, 3, H, W] fp32: the device input stage's output (recon images first), NCHW"""
    x0, x1 = to_signed(recon, orig, recon_bf16, signed, quantize)
    return scaling_layer(np.concatenate([x0, x1]))


# ---- the network ----
@functools.lru_cache(maxsize=None)
def weights(dtype=torch.float64):
    sd, lin = LpipsNet.synthetic_tensors()
    conv = [(sd[key + ".weight"].to(dtype), sd[key + ".bias"].to(dtype)) for _, key, *_ in LAYERS]
    return conv, [w.reshape(-1).double().numpy() for w in lin]


def features(x, dtype=torch.float64, mut=None):
    """x [N, 3, H, W] fp32 (the scaling layer's output) -> the five taps [N, C, h, w] as numpy arrays of `dtype`"""
    conv, _ = weights(dtype)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    taps = []
    for i, ((_, _, _, _, k, s, p, pool), (w, b)) in enumerate(zip(LAYERS, conv)):
        pre = F.conv2d(t, w, b, stride=s, padding=0 if (mut == "conv1_pad0" and i == 0) else p)
        t = F.relu(pre)
        taps.append((pre if mut == "pre_relu" else t).numpy())
        if pool:
            t = F.max_pool2d(t, 3, 2, ceil_mode=mut == "ceil_pool")
    return taps


def tap_distance(f0, f1, w, mut=None):
    """one tap's contribution per pair: f0, f1 [B, C, h, w], w [C]; numpy fp64"""
    f0, f1, w = np.asarray(f0, np.float64), np.asarray(f1, np.float64), np.asarray(w, np.float64).reshape(1, -1, 1, 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        if mut == "normalize_after":
            d = f0 - f1
            d = d / (np.sqrt((d * d).sum(1, keepdims=True)) + EPS)
        else:
            norm = (lambda f: np.sqrt((f * f).sum(1, keepdims=True) + EPS)) if mut == "eps_inside" else (lambda f: np.sqrt((f * f).sum(1, keepdims=True)) + EPS)
            d = f0 / norm(f0) - f1 / norm(f1)
        per_pixel = (w * (d * d)).sum(1)
    return per_pixel.sum((1, 2)) if mut == "spatial_sum" else per_pixel.mean((1, 2))


def distance(taps, mut=None):
    """taps: five [2B, C, h, w] arrays (recon images first) -> LPIPS per pair, the taps added in index order"""
    _, lin = weights()
    B = taps[0].shape[0] // 2
    total = np.zeros(B)
    for f, w in zip(taps, lin):
        total = total + tap_distance(f[:B], f[B:], w, mut)
    return total


def emulate(recon, orig, recon_bf16, signed, quantize, dtype=torch.float64, mut=None):
    x0, x1 = to_signed(recon, orig, recon_bf16, signed, quantize)
    x = np.concatenate([x0, x1])
    x = x if mut == "no_scaling" else scaling_layer(x)
    return distance(features(x, dtype, mut), mut)


@functools.lru_cache(maxsize=None)
def case_value(name: str, dtype=torch.float64, mut=None):
    """LPIPS [B] of a case under the emulation; computed once per (case, variant) and shared by the tests -- treat it as read-only"""
    case = BY_NAME[name]
    recon, orig = make(case)
    v = emulate(recon, orig, case.recon_bf16, case.signed, case.quantize, dtype, mut)
    v.setflags(write=False)
    return v


def gated_pairs(name: str):
    """bool [B]: the pairs of a case the end-to-end relative gate applies to -- d >= D_GATED under the fp64 emulation, whatever the content"""
    return case_value(name) >= D_GATED


@functools.lru_cache(maxsize=None)
def fp32_relative_error() -> float:
    """the largest relative error of the fp32-feature variant (torch-CPU fp32 convolutions) against the fp64 emulation over the GATED cases (noise and smooth:
    every pair at d >= D_GATED).  The const pairs the gate also applies to are left out of this maximum on purpose: torch's fp32 convolution of a constant
    image errs more (2.6e-7 on this table; presumably because equal products round the same way at every step of a sum and nothing averages out) and taking
    them in would widen the gate of every case 3.6 x.  No end-to-end case has a zero-norm pixel (a const image still leaves channels above zero after conv1's
    bias), so the eps is exercised by the crafted `tiny` features of FEAT_CASES alone."""
    return max(float((np.abs(case_value(c.name, torch.float32) - case_value(c.name)) / case_value(c.name)).max()) for c in GATED)


# ---- the second, independent formulation: explicit im2col + einsum, numpy fp64 ----
def _conv_im2col(x, w, b, stride, pad):
    N, C, H, W = x.shape
    Co, _, KH, KW = w.shape
    xp = np.zeros((N, C, H + 2 * pad, W + 2 * pad))
    xp[:, :, pad:pad + H, pad:pad + W] = x
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    cols = np.empty((N, C, KH, KW, OH, OW))
    for i in range(KH):
        for j in range(KW):
            cols[:, :, i, j] = xp[:, :, i:i + stride * (OH - 1) + 1:stride, j:j + stride * (OW - 1) + 1:stride]
    return np.einsum("ncijyx,ocij->noyx", cols, w, optimize=True) + b.reshape(1, -1, 1, 1)


def _pool_np(x):
    N, C, H, W = x.shape
    PH, PW = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = np.full((N, C, PH, PW), -np.inf)
    for i in range(3):
        for j in range(3):
            out = np.maximum(out, x[:, :, i:i + 2 * (PH - 1) + 1:2, j:j + 2 * (PW - 1) + 1:2])
    return out


def emulate_im2col(recon, orig, recon_bf16, signed, quantize):
    conv, lin = weights()
    x0, x1 = to_signed(recon, orig, recon_bf16, signed, quantize)
    t = scaling_layer(np.concatenate([x0, x1])).astype(np.float64)
    B = x0.shape[0]
    total = np.zeros(B)
    for (_, _, _, _, k, s, p, pool), (w, b), lw in zip(LAYERS, conv, lin):
        t = np.maximum(_conv_im2col(t, w.numpy(), b.numpy(), s, p), 0.0)
        n = t / (np.sqrt(np.einsum("nchw,nchw->nhw", t, t))[:, None] + EPS)
        d = n[:B] - n[B:]
        total = total + np.einsum("c,nchw->n", lw, d * d) / (t.shape[2] * t.shape[3])
        if pool:
            t = _pool_np(t)
    return total


# ---- the distance stage alone: crafted fp32 features ----
class FeatCase(NamedTuple):
    name: str
    B: int
    C: int
    h: int
    w: int
    content: str        # relu_noise | cancelling | tiny (pixels with norms around the eps, and all-zero pixels)


FEAT_CASES = [FeatCase("b1_c64_7x7_relu_noise", 1, 64, 7, 7, "relu_noise"), FeatCase("b3_c192_3x5_cancelling", 3, 192, 3, 5, "cancelling"),
              FeatCase("b5_c384_1x1_relu_noise", 5, 384, 1, 1, "relu_noise"), FeatCase("b2_c256_9x15_tiny", 2, 256, 9, 15, "tiny"),
              FeatCase("b3_c64_13x5_tiny", 3, 64, 13, 5, "tiny"), FeatCase("b2_c64_63x63_relu_noise", 2, 64, 63, 63, "relu_noise"),
              FeatCase("b1_c100_8x9_cancelling", 1, 100, 8, 9, "cancelling")]


def make_features(fc: FeatCase):
    """(feat [2B, C, h, w] fp32, w [C] fp32 >= 0)"""
    s = zlib.crc32(fc.name.encode())
    shape = (fc.B, fc.C, fc.h, fc.w)
    f0 = np.maximum(_u(s, shape, -1.0, 1.0), 0)
    if fc.content == "cancelling":
        f1 = (f0 * (np.float32(1) + _u(s + 1, shape, -1e-4, 1e-4))).astype(np.float32)
    else:
        f1 = np.maximum(_u(s + 1, shape, -1.0, 1.0), 0)
    if fc.content == "tiny":
        scale = np.float32(10.0) ** np.floor(_u(s + 2, (fc.B, 1, fc.h, fc.w), -13.0, -3.0))     # norms from 1e-13 to 1e-3: around the eps
        dead = _u(s + 3, (fc.B, 1, fc.h, fc.w), 0.0, 1.0) < 0.2                                   # all-zero pixels in one image
        f0, f1 = (f0 * scale).astype(np.float32), (f1 * scale).astype(np.float32)
        f1 = np.where(dead, np.float32(0), f1)
        f0 = np.where(np.roll(dead, 1, axis=-1), np.float32(0), f0)
    w = np.abs(_u(s + 4, (fc.C,), -1.0, 1.0)) * np.float32(np.sqrt(3.0 / fc.C))
    return np.ascontiguousarray(np.concatenate([f0, f1]), np.float32), w.astype(np.float32)


def distance_tolerance(value, C: int, npix: int, wmax: float):
    """bound on |device - emulation| of one tap's contribution, both in fp64 (u = 2^-53), derived, no tuned factor:
    the channel sum of squares is a sum of C non-negative terms, relative error <= (C + 1) u in any order; sqrt halves it and adds one rounding, + eps and the
    division add one each, one spare for a square root that is faithful rather than correctly rounded: a normalised component a = f / n carries
    |da| <= e |a|, e = (C / 2 + 4) u.  d = a - b then carries |dd| <= e (|a| + |b|) + u |d| and d^2 carries 2 |d| |dd| (second order dropped, < 1e-28):
    sum_c w_c 2 |d_c| e (|a_c| + |b_c|) <= 2 e wmax |d|_2 |(|a| + |b|)|_2 <= 8 e wmax, because normalised vectors have |a|_2, |b|_2 <= 1.
    Every remaining operation (w * d^2, the sums over channels, the pixels of a tile, the tiles, the division by npix) acts on non-negative terms and is
    relative: depth (C + npix + 8) u covers any summation order of either side.  Both sides err, hence the leading 2."""
    e = (C / 2 + 4) * U
    return 2.0 * (8.0 * e * wmax + (C + npix + 8) * U * np.asarray(value, np.float64))
