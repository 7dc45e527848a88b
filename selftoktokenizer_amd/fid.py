"""rFID: the Frechet distance between InceptionV3 pool3 features of the originals and of the reconstructions, on the project's own kernels
(csrc/fid.hip): an image's 2048 features are a function of that image alone, bit for bit, whatever the batch around it, and the statistics
are taken in fp64 in a fixed order.

FID_DEFINITION states the metric: the `pytorch-fid` variant (FID InceptionV3, `pt_inception-2015-12-05` key layout, pool3).  tests/fid_cases.py
restates it in torch-CPU fp64 / numpy.  The published weight file is read by `InceptionNet.from_files`; `InceptionNet.synthetic` builds the same
architecture on hash-generated weights, which is what the tests run on.  The implementation is held to the published definition, not to the
`pytorch-fid` package: unpinned against the package.
"""
from __future__ import annotations

import math
import os
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib, ops, synth

BN_EPS = 1e-3
SIDE = 299                    # the network's own input side: what `resize=True` brings an image to
MIN_SIDE = 75                 # smallest H, W that leaves one pixel at the last map
FEATURES = 2048
CLASSES = 1008                # the fc head of the 2015 network: what the Inception Score reads (genmetrics.py)
CHUNK_BYTES = 1 << 30         # activations of one internal chunk of images stay below this (one image at 299 x 299 is 45 MB: 22 images)


def _units():
    """name -> (Cin, Cout, KH, KW, stride, pad_h, pad_w): the 94 BasicConv2d units (convolution without bias -> BatchNorm, eps 1e-3 -> ReLU)"""
    U = {}

    def u(name, cin, cout, k=1, s=1, p=0):
        kh, kw = (k, k) if isinstance(k, int) else k
        ph, pw = (p, p) if isinstance(p, int) else p
        U[name] = (cin, cout, kh, kw, s, ph, pw)

    u("Conv2d_1a_3x3", 3, 32, 3, 2); u("Conv2d_2a_3x3", 32, 32, 3); u("Conv2d_2b_3x3", 32, 64, 3, 1, 1); u("Conv2d_3b_1x1", 64, 80); u("Conv2d_4a_3x3", 80, 192, 3)
    for b, cin, pf in (("Mixed_5b", 192, 32), ("Mixed_5c", 256, 64), ("Mixed_5d", 288, 64)):
        u(f"{b}.branch1x1", cin, 64)
        u(f"{b}.branch5x5_1", cin, 48); u(f"{b}.branch5x5_2", 48, 64, 5, 1, 2)
        u(f"{b}.branch3x3dbl_1", cin, 64); u(f"{b}.branch3x3dbl_2", 64, 96, 3, 1, 1); u(f"{b}.branch3x3dbl_3", 96, 96, 3, 1, 1)
        u(f"{b}.branch_pool", cin, pf)
    u("Mixed_6a.branch3x3", 288, 384, 3, 2)
    u("Mixed_6a.branch3x3dbl_1", 288, 64); u("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1); u("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for b, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        u(f"{b}.branch1x1", 768, 192)
        u(f"{b}.branch7x7_1", 768, c7); u(f"{b}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3)); u(f"{b}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        u(f"{b}.branch7x7dbl_1", 768, c7); u(f"{b}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0)); u(f"{b}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        u(f"{b}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0)); u(f"{b}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        u(f"{b}.branch_pool", 768, 192)
    u("Mixed_7a.branch3x3_1", 768, 192); u("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    u("Mixed_7a.branch7x7x3_1", 768, 192); u("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3)); u("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    u("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for b, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        u(f"{b}.branch1x1", cin, 320)
        u(f"{b}.branch3x3_1", cin, 384); u(f"{b}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1)); u(f"{b}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        u(f"{b}.branch3x3dbl_1", cin, 448); u(f"{b}.branch3x3dbl_2", 448, 384, 3, 1, 1)
        u(f"{b}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1)); u(f"{b}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        u(f"{b}.branch_pool", cin, 192)
    return U


UNITS = _units()
BLOCKS = ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e", "Mixed_7a", "Mixed_7b", "Mixed_7c")
BN_LEAVES = ("weight", "bias", "running_mean", "running_var")

FID_DEFINITION = {
    "net": "FID InceptionV3 (pytorch-fid), pt_inception-2015-12-05 key layout", "features": "pool3", "dim": FEATURES,
    "input": "fp32 in [-1, 1]: float32(v) * 2 - 1 for a [0, 1] image, a signed image as it is; u8: byte / 255 * 2 - 1 of the byte save_image writes",
    "resize": "bilinear to 299 x 299, align_corners=False, no antialiasing: source coordinate max(0, (d + 0.5) * (in / out) - 0.5), i0 = floor, i1 = min(i0 + 1, in - 1), "
              "fp32 blend a + lambda * (b - a), horizontal pairs first, then vertical; a 299 x 299 image passes through bit for bit",
    "unit": "convolution without bias -> BatchNorm in eval mode, eps 1e-3 (folded on the host in fp64, rounded to fp32 once) -> ReLU", "bn_eps": BN_EPS,
    "pools": "max 3x3 / 2 after Conv2d_2b and Conv2d_4a and in Mixed_6a / Mixed_7a; branch pools 3x3 / 1 / pad 1: average with count_include_pad=False, "
             "except Mixed_7c: max-pool",
    "units": {k: list(v) for k, v in UNITS.items()},
    "pool3": "spatial mean of Mixed_7c's map",
    "statistics": "fp64 from the fp32 features on: mu = mean, sigma = covariance with 1 / (N - 1), two passes",
    "distance": "|mu1 - mu2|^2 + tr s1 + tr s2 - 2 sum_i sqrt(max(lambda_i, 0)), lambda the eigenvalues of S s2 S, S = s1^(1/2) by a symmetric eigendecomposition "
                "with eigenvalues clamped at 0 (= tr (s1 s2)^(1/2); defined for rank-deficient covariances); numpy fp64 on the host",
    "min_side": MIN_SIDE,
}


def resize_taps(n_in: int, n_out: int):
    """(i0 int32 [n_out], i1 int32 [n_out], lambda fp32 [n_out]) of one axis, from fp64: bilinear, align_corners=False, no antialiasing"""
    d = np.arange(n_out, dtype=np.float64)
    src = np.maximum(0.0, (d + 0.5) * (np.float64(n_in) / np.float64(n_out)) - 0.5)
    i0 = np.minimum(np.floor(src), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0.astype(np.int32), i1.astype(np.int32), (src - i0).astype(np.float32)


def resize_tables(H: int, W: int, device, side: int = SIDE):
    """the (ytab, xtab) int32 [3, side] device tensors ops.fid_input takes: rows i0, i1 and the bits of the fp32 lambda"""
    out = []
    for n in (H, W):
        i0, i1, lam = resize_taps(n, side)
        out.append(torch.from_numpy(np.stack([i0, i1, lam.view(np.int32)])).to(device))
    return tuple(out)


def fold_bn(w: torch.Tensor, bn: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma / sqrt(var + eps), in fp64, each rounded to fp32 once"""
    scale = bn["weight"].double() / torch.sqrt(bn["running_var"].double() + BN_EPS)
    return (w.double() * scale.view(-1, 1, 1, 1)).float(), (bn["bias"].double() - bn["running_mean"].double() * scale).float()


def state_shapes() -> Dict[str, Tuple[int, ...]]:
    out = {}
    for name, (cin, cout, kh, kw, _, _, _) in UNITS.items():
        out[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for leaf in BN_LEAVES:
            out[f"{name}.bn.{leaf}"] = (cout,)
    return out


def fc_shapes() -> Dict[str, Tuple[int, ...]]:
    """the fc head's two tensors (state_shapes() lists the 94 units only): read when a network is built with logits=True"""
    return {"fc.weight": (CLASSES, FEATURES), "fc.bias": (CLASSES,)}


class _Runner:
    """walks the network once: `dry` only sizes the activations (meta tensors), otherwise they come from `alloc` and the kernels run"""

    def __init__(self, net, alloc, dry=False):
        self.net, self.alloc, self.dry = net, alloc, dry

    def conv(self, name, x, out=None, co_off=0):
        cin, cout, kh, kw, s, ph, pw = UNITS[name]
        n, H, W, _ = x.shape
        if out is None:
            out = self.alloc((n, (H + 2 * ph - kh) // s + 1, (W + 2 * pw - kw) // s + 1, cout))
        if not self.dry:
            ops.fid_conv2d(x, self.net.packed[name], self.net.bias[name], cout, kh, kw, s, ph, pw, True, out=out, co_off=co_off)
        return out

    def pool(self, x, mode, out=None, co_off=0):
        n, H, W, C = x.shape
        if out is None:
            out = self.alloc((n, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C) if mode == "max_s2" else (n, H, W, C))
        if not self.dry:
            ops.fid_pool3(x, mode, out=out, co_off=co_off)
        return out


def _block(r: _Runner, b: str, x):
    """one Inception block: every branch writes its slice of the block's map, in the order FID_DEFINITION lists (no concatenation pass)"""
    n, H, W, _ = x.shape
    c = lambda leaf, t, out=None, off=0: r.conv(f"{b}.{leaf}", t, out, off)
    if b in ("Mixed_5b", "Mixed_5c", "Mixed_5d"):
        pf = UNITS[f"{b}.branch_pool"][1]
        y = r.alloc((n, H, W, 224 + pf))
        c("branch1x1", x, y, 0)
        c("branch5x5_2", c("branch5x5_1", x), y, 64)
        c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x)), y, 128)
        c("branch_pool", r.pool(x, "avg_s1p1"), y, 224)
    elif b == "Mixed_6a":
        y = r.alloc((n, (H - 3) // 2 + 1, (W - 3) // 2 + 1, 768))
        c("branch3x3", x, y, 0)
        c("branch3x3dbl_3", c("branch3x3dbl_2", c("branch3x3dbl_1", x)), y, 384)
        r.pool(x, "max_s2", y, 480)
    elif b in ("Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
        y = r.alloc((n, H, W, 768))
        c("branch1x1", x, y, 0)
        c("branch7x7_3", c("branch7x7_2", c("branch7x7_1", x)), y, 192)
        c("branch7x7dbl_5", c("branch7x7dbl_4", c("branch7x7dbl_3", c("branch7x7dbl_2", c("branch7x7dbl_1", x)))), y, 384)
        c("branch_pool", r.pool(x, "avg_s1p1"), y, 576)
    elif b == "Mixed_7a":
        y = r.alloc((n, (H - 3) // 2 + 1, (W - 3) // 2 + 1, 1280))
        c("branch3x3_2", c("branch3x3_1", x), y, 0)
        c("branch7x7x3_4", c("branch7x7x3_3", c("branch7x7x3_2", c("branch7x7x3_1", x))), y, 320)
        r.pool(x, "max_s2", y, 512)
    else:                                                         # Mixed_7b, Mixed_7c
        y = r.alloc((n, H, W, 2048))
        c("branch1x1", x, y, 0)
        t = c("branch3x3_1", x)
        c("branch3x3_2a", t, y, 320); c("branch3x3_2b", t, y, 704)
        t = c("branch3x3dbl_2", c("branch3x3dbl_1", x))
        c("branch3x3dbl_3a", t, y, 1088); c("branch3x3dbl_3b", t, y, 1472)
        c("branch_pool", r.pool(x, "max_s1p1" if b == "Mixed_7c" else "avg_s1p1"), y, 1856)      # the FID network's quirk: 7c pools with a maximum
    return y


def _walk(r: _Runner, x, keep: Optional[dict] = None):
    """x [n, H, W, 3] -> Mixed_7c's map [n, h, w, 2048]; `keep` collects the stem's and every block's output"""
    x = r.conv("Conv2d_2b_3x3", r.conv("Conv2d_2a_3x3", r.conv("Conv2d_1a_3x3", x)))
    x = r.pool(x, "max_s2")
    x = r.conv("Conv2d_4a_3x3", r.conv("Conv2d_3b_1x1", x))
    x = r.pool(x, "max_s2")
    if keep is not None:
        keep["stem"] = x
    for b in BLOCKS:
        x = _block(r, b, x)
        if keep is not None:
            keep[b] = x
    return x


def map_sizes(H: int, W: int) -> List[Tuple[int, int]]:
    """spatial size of the 35 / 17 / 8 maps (Mixed_5x, Mixed_6x, Mixed_7x) of an H x W network input"""
    keep = {}
    _walk(_Runner(None, lambda s: torch.empty(s, device="meta"), dry=True), torch.empty(1, H, W, 3, device="meta"), keep)
    return [tuple(keep[b].shape[1:3]) for b in ("Mixed_5d", "Mixed_6e", "Mixed_7c")]


class InceptionNet:
    """net.pool3(images, signed) -> fp32 [B, 2048] on the device.  Built from a state dict in the pt_inception-2015-12-05 key layout."""

    def __init__(self, state: Dict[str, torch.Tensor], device, source, logits: bool = False):
        self.device = torch.device(device)
        self.source = source
        self.chunk_images: Optional[int] = None                   # None: sized from CHUNK_BYTES; the tests set it to walk the chunk edges
        self.resize = True                                        # what pool3(resize=None) does, evaluate()'s route: False feeds the images straight in
        shapes = dict(state_shapes(), **(fc_shapes() if logits else {}))
        for key, shape in shapes.items():
            if key not in state:
                raise KeyError(f"FID InceptionV3: key {key!r} is missing")
            if tuple(state[key].shape) != tuple(shape):
                raise ValueError(f"FID InceptionV3: {key!r} has shape {tuple(state[key].shape)}, expected {tuple(shape)}")
        self.packed, self.bias, self._tables, self._plans = {}, {}, {}, {}
        for name in UNITS:
            w, b = fold_bn(state[f"{name}.conv.weight"].detach().cpu(), {leaf: state[f"{name}.bn.{leaf}"].detach().cpu() for leaf in BN_LEAVES})
            self.packed[name] = ops.lpips_pack_conv_weight(w).to(self.device)
            self.bias[name] = b.contiguous().to(self.device)
        self.fc_packed = self.fc_bias = None                      # logits=True: the fc head as a 1 x 1 convolution on the 1 x 1 pool3 map
        if logits:
            self.fc_packed = ops.lpips_pack_conv_weight(state["fc.weight"].detach().cpu().float().view(CLASSES, FEATURES, 1, 1)).to(self.device)
            self.fc_bias = state["fc.bias"].detach().cpu().float().contiguous().to(self.device)

    # ---- construction ----
    @staticmethod
    def synthetic_tensors() -> Dict[str, torch.Tensor]:
        """the state dict on the host, hash-generated by tensor name: convolution weights uniform in +-sqrt(2) * sqrt(3 / fan_in) (the gain keeps the features
        of different images apart: with the plain sqrt(3 / fan_in) recipe the network is bias-dominated), BatchNorm gamma and running_var in [0.9, 1.1], beta and
        running_mean in [-0.1, 0.1]"""
        sd = {}
        for key, shape in state_shapes().items():
            seed = synth.name_seed("fid.inception." + key)
            leaf = key.rsplit(".", 1)[-1]
            if key.endswith("conv.weight"):
                a = math.sqrt(2.0) * math.sqrt(3.0 / (shape[1] * shape[2] * shape[3]))
                sd[key] = synth.hash_uniform(seed, shape, -a, a)
            elif leaf in ("weight", "running_var"):
                sd[key] = synth.hash_uniform(seed, shape, 0.9, 1.1)
            else:
                sd[key] = synth.hash_uniform(seed, shape, -0.1, 0.1)
        return sd

    @staticmethod
    def synthetic_fc_tensors() -> Dict[str, torch.Tensor]:
        """the fc head, hash-generated like the units: weight uniform in +-4 * sqrt(3 / 2048) (the gain keeps the class probabilities of different images
        apart), bias in [-0.1, 0.1]"""
        a = 4.0 * math.sqrt(3.0 / FEATURES)
        return {"fc.weight": synth.hash_uniform(synth.name_seed("fid.inception.fc.weight"), (CLASSES, FEATURES), -a, a),
                "fc.bias": synth.hash_uniform(synth.name_seed("fid.inception.fc.bias"), (CLASSES,), -0.1, 0.1)}

    @classmethod
    def synthetic(cls, device, logits: bool = False) -> "InceptionNet":
        return cls(dict(cls.synthetic_tensors(), **(cls.synthetic_fc_tensors() if logits else {})), device, "synthetic", logits)

    @classmethod
    def from_files(cls, pth: str, device, logits: bool = False) -> "InceptionNet":
        """pytorch-fid's pt_inception-2015-12-05 state dict: keys <layer>.conv.weight and <layer>.bn.{weight,bias,running_mean,running_var} of the 94 units.
        A missing key or a wrong shape is an error; fc.*, AuxLogits.*, num_batches_tracked and any other key are ignored.  logits=True also reads
        fc.weight [1008, 2048] and fc.bias [1008] (missing or misshapen: an error), for net.logits / net.features."""
        return cls(torch.load(pth, map_location="cpu", weights_only=True), device, os.path.basename(pth), logits)

    # ---- the network ----
    def _check(self, images, resize):
        if images.dim() != 4 or images.shape[1] != 3:
            raise _lib.SelftokHipError(f"fid: expected a [B, 3, H, W] tensor, got {tuple(images.shape)}")
        if images.dtype not in (torch.bfloat16, torch.float32):
            raise _lib.SelftokHipError(f"fid: dtype {images.dtype}: expected bfloat16 or float32")
        B, _, H, W = images.shape
        if B < 1 or H < 1 or W < 1 or (not resize and (H < MIN_SIDE or W < MIN_SIDE)):
            raise _lib.SelftokHipError(f"fid: need B >= 1 and, without the resize, H, W >= {MIN_SIDE} (one pixel at the last map), got B {B}, {H} x {W}")
        ops._need_cuda(images)
        return B, H, W

    def _tables_for(self, H, W, resize):
        if not resize or (H, W) == (SIDE, SIDE):
            return None                                           # a 299 x 299 image passes through bit for bit
        key = (H, W, torch.cuda.current_device())
        if key not in self._tables:
            self._tables[key] = resize_tables(H, W, self.device)
        return self._tables[key]

    def _run(self, images, signed, quantize, resize, keep_stages: bool):
        B, H, W = self._check(images, resize)
        tables = self._tables_for(H, W, resize)
        IH, IW = (H, W) if tables is None else (SIDE, SIDE)
        align = lambda v: -(-v // 256) * 256
        if (IH, IW) not in self._plans:                           # bytes of one image's activations and their number, from a dry walk
            sizes = []
            _walk(_Runner(self, lambda s: (sizes.append(align(4 * math.prod(s[1:]))), torch.empty(s, device="meta"))[1], dry=True), torch.empty(1, IH, IW, 3, device="meta"))
            self._plans[(IH, IW)] = (align(4 * IH * IW * 3) + sum(sizes), len(sizes) + 1)
        per_image, buffers = self._plans[(IH, IW)]
        chunk = min(self.chunk_images or max(1, CHUNK_BYTES // per_image), B)
        out = torch.empty(B, FEATURES, dtype=torch.float32, device=images.device)
        stages = []
        arena = None if keep_stages else ops.eval_workspace(images.device, chunk * per_image + 256 * buffers)
        for b0 in range(0, B, chunk):
            b1 = min(b0 + chunk, B)
            off = [0]

            def alloc(shape):
                if arena is None:
                    return torch.empty(shape, dtype=torch.float32, device=images.device)
                nbytes = 4 * math.prod(shape)
                t = arena[off[0]:off[0] + nbytes].view(torch.float32).view(shape)
                off[0] += align(nbytes)
                return t
            keep = {} if keep_stages else None
            x = ops.fid_input(images[b0:b1], signed, quantize, tables, out=alloc((b1 - b0, IH, IW, 3)))
            if keep is not None:
                keep["input"] = x
            ops.fid_spatial_mean(_walk(_Runner(self, alloc), x, keep), out=out[b0:b1])
            stages.append(keep)
        return out, stages

    def pool3(self, images: torch.Tensor, signed: bool, quantize: bool = False, resize: Optional[bool] = None) -> torch.Tensor:
        """images [B, 3, H, W], in [-1, 1] when `signed` else in [0, 1], bf16 or fp32, on the device -> the pool3 features, fp32 [B, 2048] on the device.
        resize=False feeds H x W >= 75 x 75 straight in; None: self.resize (True unless set otherwise).  No synchronisation.  Large batches are walked in chunks
        of images; a value does not depend on the chunking."""
        return self._run(images, signed, quantize, self.resize if resize is None else resize, False)[0]

    def logits(self, pool3: torch.Tensor) -> torch.Tensor:
        """pool3 [B, 2048] fp32 on the device -> the fc logits, fp32 [B, 1008]: pool3 . W^T + b as a 1 x 1 convolution on a 1 x 1 map (ops.fid_conv2d, no ReLU),
        so a row's logits are a function of that row alone in the convolution's stated arithmetic.  Needs a network built with logits=True."""
        if self.fc_packed is None:
            raise _lib.SelftokHipError("fid: this network was built without the fc head: build it with logits=True (InceptionNet.synthetic / from_files)")
        if pool3.dim() != 2 or pool3.shape[1] != FEATURES or pool3.dtype != torch.float32:
            raise _lib.SelftokHipError(f"fid: logits expects float32 pool3 features [B, {FEATURES}], got {pool3.dtype} {tuple(pool3.shape)}")
        ops._need_cuda(pool3)
        B = pool3.shape[0]
        if B == 0:
            return torch.empty(0, CLASSES, dtype=torch.float32, device=pool3.device)
        return ops.fid_conv2d(pool3.contiguous().view(B, 1, 1, FEATURES), self.fc_packed, self.fc_bias, CLASSES, 1, 1, 1, 0, 0, relu=False).view(B, CLASSES)

    def features(self, images: torch.Tensor, signed: bool, quantize: bool = False, resize: Optional[bool] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """(pool3 [B, 2048], logits [B, 1008]) of one walk of the network: pool3() followed by logits()"""
        f = self.pool3(images, signed, quantize, resize)
        return f, self.logits(f)

    def stages(self, images: torch.Tensor, signed: bool, quantize: bool = False, resize: Optional[bool] = None) -> Dict[str, torch.Tensor]:
        """the network input, the stem's and every block's output as [B, C, h, w] fp32 and "pool3" [B, 2048]: what the tests compare stage by stage"""
        out, stages = self._run(images, signed, quantize, self.resize if resize is None else resize, True)
        res = {k: torch.cat([s[k] for s in stages]).permute(0, 3, 1, 2) for k in stages[0]}
        res["pool3"] = out
        return res


# ---- the dataset-level tail ----
def statistics(X: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """X [N, D] fp32 on the device -> (mu [D], sigma [D, D]) fp64 on the device (ops.fid_stats): N >= 2, D a multiple of 16"""
    return ops.fid_stats(X)


def _host64(a) -> np.ndarray:
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)


def frechet_distance(mu1, sigma1, mu2, sigma2) -> float:
    """d^2 of FID_DEFINITION["distance"], numpy fp64 on the host.  S sigma2 S is symmetrised ((M + M^T) / 2, a rounding-level step) before its eigenvalues
    are taken."""
    mu1, mu2, s1, s2 = _host64(mu1), _host64(mu2), _host64(sigma1), _host64(sigma2)
    if mu1.ndim != 1 or mu2.shape != mu1.shape or s1.shape != (mu1.size, mu1.size) or s2.shape != s1.shape:
        raise ValueError(f"frechet_distance: expected mu [D] and sigma [D, D] twice, got {mu1.shape}, {s1.shape}, {mu2.shape}, {s2.shape}")
    w, V = np.linalg.eigh(s1)
    S = (V * np.sqrt(np.maximum(w, 0.0))) @ V.T
    M = S @ s2 @ S
    lam = np.linalg.eigvalsh((M + M.T) / 2.0)
    d = mu1 - mu2
    return float(d @ d + np.trace(s1) + np.trace(s2) - 2.0 * np.sqrt(np.maximum(lam, 0.0)).sum())


def save_stats(path: str, mu, sigma) -> None:
    """an .npz with keys `mu` and `sigma`: the layout pytorch-fid users have, so a reference set can be precomputed"""
    with open(path, "wb") as f:
        np.savez(f, mu=_host64(mu), sigma=_host64(sigma))


def load_stats(path: str) -> Tuple[np.ndarray, np.ndarray]:
    with np.load(path) as z:
        for key in ("mu", "sigma"):
            if key not in z:
                raise KeyError(f"{path}: key {key!r} is missing")
        mu, sigma = np.asarray(z["mu"], np.float64), np.asarray(z["sigma"], np.float64)
    if mu.ndim != 1 or sigma.shape != (mu.size, mu.size):
        raise ValueError(f"{path}: expected mu [D] and sigma [D, D], got {mu.shape} and {sigma.shape}")
    return mu, sigma
