"""LPIPS (Zhang et al. 2018) with the v0.1 linear layers on the project's own kernels (csrc/lpips.hip, csrc/lpips_vgg.hip): the AlexNet backbone --
`lpips.LPIPS()`'s default -- and the VGG16 backbone (`net="vgg"`).  The value of an image pair is a function of that pair alone, bit for bit,
whatever the batch around it.

LPIPS_DEFINITION / LPIPS_VGG_DEFINITION state the metric; tests/lpips_cases.py and tests/lpips_vgg_cases.py restate it in torch-CPU fp64 / numpy.
The published weight files (torchvision's AlexNet / VGG16, the `lpips` package's alex.pth / vgg.pth) are read by `LpipsNet.from_files`;
`LpipsNet.synthetic` builds the same architecture on hash-generated weights, which is what the tests run on.  The implementation is held to the
published definition, not to the `lpips` package: unpinned against the package.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib, ops

# (name, torchvision key, Cout, Cin, kernel, stride, pad, max-pool after the tap)
LAYERS = (("conv1", "features.0", 64, 3, 11, 4, 2, True),
          ("conv2", "features.3", 192, 64, 5, 1, 2, True),
          ("conv3", "features.6", 384, 192, 3, 1, 1, False),
          ("conv4", "features.8", 256, 384, 3, 1, 1, False),
          ("conv5", "features.10", 256, 256, 3, 1, 1, False))
MIN_SIDE = 31

LPIPS_DEFINITION = {
    "net": "alex", "version": "0.1",
    "input": "both images fp32 in [-1, 1]: float32(v) * 2 - 1 for a [0, 1] image, a signed image as it is; u8: byte / 255 * 2 - 1 of the byte save_image writes",
    "shift": [-0.030, -0.088, -0.188], "scale": [0.458, 0.448, 0.450],
    "backbone": "torchvision AlexNet features, fp32, zero padding; taps after the ReLU of conv1..conv5; max-pool 3x3 stride 2 (floor) after taps 1 and 2",
    "layers": [{"name": n, "kernel": k, "stride": s, "pad": p, "channels": [ci, co]} for n, _, co, ci, k, s, p, _ in LAYERS],
    "normalize": "f / (sqrt(sum_c f_c^2) + 1e-10) per pixel", "eps": 1e-10,
    "distance": "sum over taps of the spatial mean of sum_c w_c (f0_c / n0 - f1_c / n1)^2, fp64 from the fp32 features on",
    "min_side": MIN_SIDE,
}


def _vgg_layers():
    out, idx, ci = [], 0, 3
    for stage, (co, n) in enumerate(((64, 2), (128, 2), (256, 3), (512, 3), (512, 3)), 1):
        for j in range(1, n + 1):
            out.append((f"conv{stage}_{j}", f"features.{idx}", co, ci, j == n, j == n and stage < 5))
            idx, ci = idx + 2, co                     # a ReLU follows every convolution
        idx += 1                                      # the MaxPool2d(2, 2) that closes the stage (indices 4, 9, 16, 23; the one at 30 is never reached)
    return tuple(out)


# (name, torchvision key, Cout, Cin, tap after its ReLU, 2 x 2 max-pool after the tap): all 3 x 3, stride 1, pad 1
VGG_LAYERS = _vgg_layers()
VGG_ARCH_MIN_SIDE = 16                                # four floor-mode halvings leave one pixel at relu5_3

LPIPS_VGG_DEFINITION = {
    "net": "vgg", "version": "0.1",
    "input": LPIPS_DEFINITION["input"], "shift": LPIPS_DEFINITION["shift"], "scale": LPIPS_DEFINITION["scale"],
    "backbone": "torchvision VGG16 features, fp32, 3x3 convolutions with zero padding 1 and stride 1, ReLU after each; taps after relu1_2, relu2_2, relu3_3, relu4_3, "
                "relu5_3; max-pool 2x2 stride 2 (floor: the last row / column of an odd map is dropped) after taps 1 to 4",
    "layers": [{"name": n, "key": key, "kernel": 3, "stride": 1, "pad": 1, "channels": [ci, co], "tap": tap} for n, key, co, ci, tap, _ in VGG_LAYERS],
    "pools": [4, 9, 16, 23],
    "normalize": LPIPS_DEFINITION["normalize"], "eps": 1e-10, "distance": LPIPS_DEFINITION["distance"],
    "min_side": MIN_SIDE,                             # the architecture needs 16; the one input stage both networks share refuses below 31 and is kept as it is
}

DEFINITIONS = {"alex": LPIPS_DEFINITION, "vgg": LPIPS_VGG_DEFINITION}
NETS = tuple(DEFINITIONS)

CHUNK_BYTES = 96 << 20        # activations of one internal chunk of pairs stay below this (one pair at 256 x 256 is 5.9 MB; on VGG16 134 MB, so one pair per chunk)


def _check_net(net: str) -> str:
    if net not in NETS:
        raise ValueError(f"LPIPS net {net!r}: expected one of {NETS}")
    return net


def tap_sizes(H: int, W: int, net: str = "alex") -> List[Tuple[int, int]]:
    """spatial size of the five taps of an H x W image"""
    out = []
    if _check_net(net) == "vgg":
        for _ in range(5):
            out.append((H, W))
            H, W = H // 2, W // 2
        return out
    for _, _, _, _, k, s, p, pool in LAYERS:
        H, W = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
        out.append((H, W))
        if pool:
            H, W = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    return out


def _check_shapes(what: str, tensors: Dict[str, torch.Tensor], want: Dict[str, Tuple[int, ...]]):
    for key, shape in want.items():
        if key not in tensors:
            raise KeyError(f"{what}: key {key!r} is missing")
        if tuple(tensors[key].shape) != tuple(shape):
            raise ValueError(f"{what}: {key!r} has shape {tuple(tensors[key].shape)}, expected {tuple(shape)}")


def _convs(net: str):
    """(name, torchvision key, Cout, Cin, kernel) of every convolution of a backbone"""
    if net == "vgg":
        return [(n, key, co, ci, 3) for n, key, co, ci, _, _ in VGG_LAYERS]
    return [(n, key, co, ci, k) for n, key, co, ci, k, _, _, _ in LAYERS]


def _tap_channels(net: str) -> List[int]:
    return [co for _, _, co, _, tap, _ in VGG_LAYERS if tap] if net == "vgg" else [co for _, _, co, *_ in LAYERS]


class LpipsNet:
    """net(recon, original) -> fp64 [B] on the device.  Built from a backbone state dict (torchvision AlexNet or VGG16 keys) and the five 1 x 1 weightings."""

    def __init__(self, backbone: Dict[str, torch.Tensor], linear: Sequence[torch.Tensor], device, source, net: str = "alex"):
        self.net = _check_net(net)
        self.definition = DEFINITIONS[net]
        self.device = torch.device(device)
        self.source = source
        self.chunk_pairs: Optional[int] = None            # None: sized from CHUNK_BYTES; the tests set it to walk the chunk edges
        convs, taps = _convs(net), _tap_channels(net)
        _check_shapes("LPIPS backbone", backbone, {f"{key}.{leaf}": ((co, ci, k, k) if leaf == "weight" else (co,))
                                                   for _, key, co, ci, k in convs for leaf in ("weight", "bias")})
        if len(linear) != len(taps):
            raise ValueError(f"LPIPS linear layers: expected {len(taps)} weightings, got {len(linear)}")
        self.packed, self.bias, self.lin = [], [], []
        for name, key, co, ci, k in convs:
            self.packed.append(ops.lpips_pack_conv_weight(backbone[key + ".weight"].detach().float().cpu()).to(self.device))
            self.bias.append(backbone[key + ".bias"].detach().float().contiguous().to(self.device))
        for i, (co, w) in enumerate(zip(taps, linear)):
            if w.numel() != co:
                raise ValueError(f"LPIPS linear layer of tap {i + 1}: {w.numel()} weights, expected {co}")
            self.lin.append(w.detach().float().reshape(co).contiguous().to(self.device))

    # ---- construction ----
    @staticmethod
    def synthetic_tensors(net: str = "alex"):
        """(backbone state dict, five [1, C, 1, 1] weightings) on the host: hash-generated by tensor name with weights._synth_tensor's recipe; the 1 x 1
        weights are non-negative, as the published ones are"""
        from . import weights as W
        sd = {}
        for _, key, co, ci, k in _convs(_check_net(net)):
            sd[key + ".weight"] = W._synth_tensor(f"lpips.{net}.{key}.weight", (co, ci, k, k), "cpu")
            sd[key + ".bias"] = W._synth_tensor(f"lpips.{net}.{key}.bias", (co,), "cpu")
        prefix = "lpips" if net == "alex" else f"lpips.{net}"
        lin = [W._synth_tensor(f"{prefix}.lin{i}.model.1.weight", (1, co, 1, 1), "cpu").abs() for i, co in enumerate(_tap_channels(net))]
        return sd, lin

    @classmethod
    def synthetic(cls, device, net: str = "alex") -> "LpipsNet":
        sd, lin = cls.synthetic_tensors(net)
        return cls(sd, lin, device, "synthetic", net=net)

    @classmethod
    def from_files(cls, backbone_pth: str, linear_pth: str, device, net: str = "alex") -> "LpipsNet":
        """torchvision's AlexNet state dict (keys features.{0,3,6,8,10}.{weight,bias}) and the lpips v0.1 alex.pth (keys lin{0..4}.model.1.weight, [1, C, 1, 1]);
        with net="vgg" torchvision's vgg16 state dict (features.{0,2,5,7,10,12,14,17,19,21,24,26,28}.{weight,bias}) and the package's vgg.pth (the same
        lin keys, C = 64, 128, 256, 512, 512).  A missing key or a wrong shape is an error; other keys (the classifier's among them) are ignored."""
        _check_net(net)
        sd = torch.load(backbone_pth, map_location="cpu", weights_only=True)
        ld = torch.load(linear_pth, map_location="cpu", weights_only=True)
        taps = _tap_channels(net)
        _check_shapes(f"LPIPS linear file {linear_pth}", ld, {f"lin{i}.model.1.weight": (1, co, 1, 1) for i, co in enumerate(taps)})
        return cls(sd, [ld[f"lin{i}.model.1.weight"] for i in range(len(taps))], device, [os.path.basename(backbone_pth), os.path.basename(linear_pth)], net=net)

    # ---- the network ----
    def _check(self, recon, original):
        if recon.dim() != 4 or recon.shape[1] != 3 or tuple(original.shape) != tuple(recon.shape):
            raise _lib.SelftokHipError(f"lpips: expected two [B, 3, H, W] tensors of one shape, got {tuple(recon.shape)} and {tuple(original.shape)}")
        B, _, H, W = recon.shape
        if B < 1 or H < MIN_SIDE or W < MIN_SIDE:
            raise _lib.SelftokHipError(f"lpips: need B >= 1 and H, W >= {MIN_SIDE} (one pixel at every tap), got B {B}, {H} x {W}")
        ops._need_cuda(recon, original)
        return B, H, W

    def _plan(self, n: int, H: int, W: int):
        """shapes of the activation buffers of n images.  AlexNet: every activation in the order it is produced (input, then per layer the tap and, where there
        is one, the pooled map).  VGG16: the input, the five taps and the two buffers every other map ping-pongs between (_vgg_steps says who writes where)."""
        if self.net == "vgg":
            return [(n,) + s for s in _vgg_steps(H, W)[0]]
        shapes = [(n, H, W, 3)]
        for (_, _, co, _, _, _, _, pool), (h, w) in zip(LAYERS, tap_sizes(H, W)):
            shapes.append((n, h, w, co))
            if pool:
                shapes.append((n, (h - 3) // 2 + 1, (w - 3) // 2 + 1, co))
        return shapes

    def _taps(self, recon, original, original_signed, quantize, bufs=None) -> List[torch.Tensor]:
        """the five taps [2B, h, w, C] of one chunk; `bufs`: preallocated activations in _plan's order"""
        if self.net == "vgg":
            return self._taps_vgg(recon, original, original_signed, quantize, bufs)
        it = iter(bufs) if bufs is not None else iter(lambda: None, 0)
        x = ops.lpips_input(recon, original, original_signed, quantize, out=next(it))
        taps = []
        for (_, _, co, _, k, s, p, pool), packed, bias in zip(LAYERS, self.packed, self.bias):
            x = ops.lpips_conv2d(x, packed, bias, co, k, k, s, p, True, out=next(it))
            taps.append(x)
            if pool:
                x = ops.lpips_maxpool3s2(x, out=next(it))
        return taps

    def _taps_vgg(self, recon, original, original_signed, quantize, bufs=None) -> List[torch.Tensor]:
        n = 2 * recon.shape[0]
        shapes, steps = _vgg_steps(recon.shape[2], recon.shape[3])
        if bufs is None:
            bufs = [torch.empty((n,) + s, dtype=torch.float32, device=recon.device) for s in shapes]
        held = {0: ops.lpips_input(recon, original, original_signed, quantize, out=bufs[0])}
        for kind, layer, src, dst, shape in steps:
            out = bufs[dst].reshape(-1)[:n * shape[0] * shape[1] * shape[2]].view((n,) + shape)      # a ping-pong buffer is viewed at the map's own shape
            if kind == "conv":
                held[dst] = ops.lpips_conv2d(held[src], self.packed[layer], self.bias[layer], shape[2], 3, 3, 1, 1, True, out=out)
            else:
                held[dst] = ops.lpips_maxpool2s2(held[src], out=out)
        return [held[1 + i] for i in range(5)]

    def features(self, recon: torch.Tensor, original: torch.Tensor, original_signed: bool = True, quantize: bool = False) -> List[torch.Tensor]:
        """the five taps as [2B, C, h, w] fp32 (recon images first, then the originals): what the distance stage is fed, for the tests"""
        self._check(recon, original)
        return [t.permute(0, 3, 1, 2) for t in self._taps(recon, original, original_signed, quantize)]

    def __call__(self, recon: torch.Tensor, original: torch.Tensor, original_signed: bool = True, quantize: bool = False) -> torch.Tensor:
        """recon [B, 3, H, W] in [0, 1], original [B, 3, H, W] in [-1, 1] (in [0, 1] with original_signed=False), bf16 or fp32 each, on the device -> LPIPS per
        pair, fp64 [B] on the device.  No synchronisation.  Large batches are walked in chunks of pairs; a value does not depend on the chunking."""
        B, H, W = self._check(recon, original)
        per_pair = 2 * 4 * sum(h * w * c for _, h, w, c in self._plan(1, H, W))
        chunk = self.chunk_pairs or max(1, CHUNK_BYTES // per_pair)
        chunk = min(chunk, B)
        shapes = self._plan(2 * chunk, H, W)
        lib = _lib.load()
        dist_bytes = lib.selftok_lpips_distance_workspace_bytes(chunk, max(h * w for h, w in tap_sizes(H, W, self.net)))
        if dist_bytes == 0:
            _lib.check(-1, "selftok_lpips_distance_workspace_bytes")
        align = lambda v: -(-v // 256) * 256
        sizes = [align(4 * n * h * w * c) for n, h, w, c in shapes]
        arena = ops.eval_workspace(recon.device, sum(sizes) + align(dist_bytes))
        out = torch.empty(B, dtype=torch.float64, device=recon.device)
        for b0 in range(0, B, chunk):
            b1 = min(b0 + chunk, B)
            n, off, bufs = 2 * (b1 - b0), 0, []
            for (_, h, w, c), size in zip(shapes, sizes):
                bufs.append(arena[off:off + 4 * n * h * w * c].view(torch.float32).view(n, h, w, c))
                off += size
            dist_ws = arena[off:off + align(dist_bytes)]
            taps = self._taps(recon[b0:b1], original[b0:b1], original_signed, quantize, bufs)
            for i, (t, w) in enumerate(zip(taps, self.lin)):          # taps in index order into out[b0:b1]
                ops.lpips_distance(t, w, out=out[b0:b1], accumulate=i > 0, workspace=dist_ws)
        return out


def _vgg_steps(H: int, W: int):
    """(per-image buffer shapes, steps) of the VGG16 route.  Buffers: 0 the input, 1 .. 5 the taps, 6 and 7 the ping-pong pair, each as large as the largest
    map written into it.  A step is (kind, layer index, source buffer, destination buffer, per-image output shape): a convolution that is tapped writes its tap
    buffer, every other convolution and every pool writes the ping-pong buffer it does not read."""
    shapes = [(H, W, 3)] + [None] * 5 + [(0, 0, 0), (0, 0, 0)]
    steps, src, tap, h, w = [], 0, 0, H, W
    grow = lambda dst, shape: shapes.__setitem__(dst, max(shapes[dst], shape, key=lambda s: s[0] * s[1] * s[2]))
    for layer, (_, _, co, _, is_tap, pool) in enumerate(VGG_LAYERS):
        dst = 1 + tap if is_tap else (7 if src == 6 else 6)
        if is_tap:
            shapes[dst] = (h, w, co)
            tap += 1
        else:
            grow(dst, (h, w, co))
        steps.append(("conv", layer, src, dst, (h, w, co)))
        src = dst
        if pool:
            h, w = h // 2, w // 2
            grow(6, (h, w, co))
            steps.append(("pool", None, src, 6, (h, w, co)))
            src = 6
    return shapes, steps
