"""The LPIPS-VGG16 arithmetic of record restated on the host, and the case tables of tests/test_lpips_vgg_cpu.py / tests/test_lpips_vgg_gpu.py.

The emulation is plain torch-CPU `conv2d` / `max_pool2d` in float64 on the fp32 input of the scaling layer, then numpy float64 for the distance
(lpips.LPIPS_VGG_DEFINITION in code).  `emulate(..., dtype=torch.float32)` computes the FEATURES in fp32 (torch's own fp32 convolution) and
everything after them in fp64: the comparator the end-to-end gate is measured on.  The input stage, the image contents and the distance of one tap
are those of tests/lpips_cases.py (shared with the AlexNet definition); only the backbone, the taps and the pooling are restated here.  No project
kernel is used as a reference; only lpips.LpipsNet.synthetic_tensors("vgg") (the hash-generated weights) is shared."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

import lpips_cases as L
from selftoktokenizer_amd.lpips import VGG_LAYERS, LpipsNet

Case = L.Case
CONTENTS = L.CONTENTS
GATED_CONTENTS = L.GATED_CONTENTS
D_GATED = L.D_GATED

MUTS = ("pre_relu", "tap_first_conv", "tap_after_pool", "ceil_pool", "alex_pool", "reversed_weightings", "normalize_after")


def _cases():
    out = []
    geoms = [(31, 31, 1), (31, 31, 3), (32, 33, 3), (32, 33, 1), (47, 34, 1), (47, 34, 3), (64, 64, 3), (64, 64, 1)]
    k = 0
    for H, W, B in geoms:
        for content in CONTENTS:
            rb, ob, sg, qz = bool(k & 1), bool(k & 2), not (k & 4), bool(k & 8)
            if content == "identical" and qz and rb:
                rb = False                        # a bf16 image and its fp32 twin do not quantize to the same byte everywhere
            out.append(Case(f"vgg_{H}x{W}_b{B}_{content}_{'b' if rb else 'f'}{'b' if ob else 'f'}{'s' if sg else 'u'}{'q' if qz else 'x'}", H, W, B, content, rb, ob, sg, qz))
            k += 3                                # walks all 16 dtype / sign / quantize combinations
    out.append(Case("vgg_96x96_b1_noise_bfsx", 96, 96, 1, "noise", True, False, True, False))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
GATED = [c for c in CASES if c.content in GATED_CONTENTS]
make = L.make


@functools.lru_cache(maxsize=None)
def weights(dtype=torch.float64):
    sd, lin = LpipsNet.synthetic_tensors("vgg")
    conv = [(sd[key + ".weight"].to(dtype), sd[key + ".bias"].to(dtype)) for _, key, *_ in VGG_LAYERS]
    return conv, [w.reshape(-1).double().numpy() for w in lin]


def features(x, dtype=torch.float64, mut=None):
    """x [N, 3, H, W] fp32 (the scaling layer's output) -> the five taps [N, C, h, w] as numpy arrays of `dtype`"""
    conv, _ = weights(dtype)
    t = torch.from_numpy(np.ascontiguousarray(x)).to(dtype)
    taps, first = [], None
    for (name, _, _, _, tap, pool), (w, b) in zip(VGG_LAYERS, conv):
        pre = F.conv2d(t, w, b, stride=1, padding=1)
        t = F.relu(pre)
        if name.endswith("_1"):
            first = t
        if tap:
            kept = pre if mut == "pre_relu" else (first if mut == "tap_first_conv" else t)
        if pool:
            t = F.max_pool2d(t, 3, 2) if mut == "alex_pool" else F.max_pool2d(t, 2, 2, ceil_mode=mut == "ceil_pool")
            if mut == "tap_after_pool":
                kept = t
        if tap:
            taps.append(kept.numpy())
    return taps


def distance(taps, mut=None):
    """taps: five [2B, C, h, w] arrays (recon images first) -> LPIPS per pair, the taps added in index order"""
    _, lin = weights()
    if mut == "reversed_weightings":
        lin = _reversed(lin)
    B = taps[0].shape[0] // 2
    total = np.zeros(B)
    for f, w in zip(taps, lin):
        total = total + L.tap_distance(f[:B], f[B:], w, "normalize_after" if mut == "normalize_after" else None)
    return total


def _reversed(lin):
    """the five weightings applied in reversed tap order; a weighting of another channel count is cut or cyclically extended to the tap's"""
    return [np.resize(w, n.shape) for w, n in zip(lin[::-1], lin)]


def emulate(recon, orig, recon_bf16, signed, quantize, dtype=torch.float64, mut=None):
    x0, x1 = L.to_signed(recon, orig, recon_bf16, signed, quantize)
    return distance(features(L.scaling_layer(np.concatenate([x0, x1])), dtype, mut), mut)


@functools.lru_cache(maxsize=None)
def case_value(name: str, dtype=torch.float64, mut=None):
    """LPIPS [B] of a case under the emulation; computed once per (case, variant) and shared by the tests -- treat it as read-only"""
    case = BY_NAME[name]
    recon, orig = make(case)
    v = emulate(recon, orig, case.recon_bf16, case.signed, case.quantize, dtype, mut)
    v.setflags(write=False)
    return v


def gated_pairs(name: str):
    return case_value(name) >= D_GATED


@functools.lru_cache(maxsize=None)
def fp32_relative_error(const: bool = False) -> float:
    """the largest relative error of the fp32-feature variant (torch-CPU fp32 convolutions) against the fp64 emulation: over the GATED cases (noise and smooth),
    as lpips_cases.fp32_relative_error is for AlexNet -- or, with `const`, over the pairs at d >= D_GATED of the const cases.  The two are kept apart because
    the comparator itself differs 15 x between them on this backbone: 1.5e-8 on noise and smooth, 2.4e-7 on constant images (every pixel of a constant map
    carries the SAME rounding error through 13 convolutions, so the spatial mean averages nothing out).  One pooled figure would either hold the const pairs
    to a bound torch-CPU fp32 misses 4 x over, or loosen the bound of every textured pair 15 x; with two, each pair is held to 4 x the comparator's error on
    pairs of its own kind.  Both figures come from the comparator alone."""
    if const:
        worst = 0.0
        for c in CASES:
            if c.content == "const" and gated_pairs(c.name).any():
                m, v = gated_pairs(c.name), case_value(c.name)
                worst = max(worst, float((np.abs(case_value(c.name, torch.float32) - v)[m] / v[m]).max()))
        return worst
    return max(float((np.abs(case_value(c.name, torch.float32) - case_value(c.name)) / case_value(c.name)).max()) for c in GATED)


def relative_gate(name: str) -> float:
    """the end-to-end relative gate of a case's pairs at d >= D_GATED: 4 x torch-CPU fp32's relative error on pairs of its kind"""
    return 4.0 * fp32_relative_error(BY_NAME[name].content == "const" if name in BY_NAME else False)


# ---- the second, independent formulation: explicit im2col + einsum, numpy fp64 ----
def _pool2_np(x):
    PH, PW = x.shape[2] // 2, x.shape[3] // 2
    x = x[:, :, :2 * PH, :2 * PW]
    return np.maximum(np.maximum(x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2]), np.maximum(x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2]))


def emulate_im2col(recon, orig, recon_bf16, signed, quantize):
    conv, lin = weights()
    x0, x1 = L.to_signed(recon, orig, recon_bf16, signed, quantize)
    t = L.scaling_layer(np.concatenate([x0, x1])).astype(np.float64)
    B = x0.shape[0]
    total, i = np.zeros(B), 0
    for (_, _, _, _, tap, pool), (w, b) in zip(VGG_LAYERS, conv):
        t = np.maximum(L._conv_im2col(t, w.numpy(), b.numpy(), 1, 1), 0.0)
        if tap:
            n = t / (np.sqrt(np.einsum("nchw,nchw->nhw", t, t))[:, None] + L.EPS)
            d = n[:B] - n[B:]
            total = total + np.einsum("c,nchw->n", lin[i], d * d) / (t.shape[2] * t.shape[3])
            i += 1
        if pool:
            t = _pool2_np(t)
    return total
