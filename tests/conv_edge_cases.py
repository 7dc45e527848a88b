"""Case tables and references of record of tests/test_conv_edges_cpu.py and tests/test_conv_edges_gpu.py: the channels-last bf16
convolution of csrc/conv.hip in its five launch shapes, its weight packer, and GroupNorm [+ SiLU] in both layouts (csrc/conv.hip NHWC,
csrc/vae.hip NCHW), at the tile, halo, channel-block and pixel-range edges.  Nothing here touches a GPU.

Convolution, exact data.  x and w are integers in [-8, 8], the bias integers in [-64, 64], the residual integers in [-512, 512] rounded to
bf16 (odd integers above 256 are not bf16 values; every other operand is one as drawn).  Every product and every partial sum in any order
is then an integer below 2^24, so fp32 accumulation is exact whatever the matrix core's order, and the kernel's output must EQUAL
RNE_bf16(exact sum), with a residual RNE_bf16(fp32(RNE_bf16(sum)) + res).  The reference is torch.nn.functional.conv2d in float64 on the
CPU -- F.pad(x, (0, 1, 0, 1)) for stride 2, F.interpolate(mode="nearest", scale_factor=2) for the upsample -- and the rounding written
out on the bit pattern.  No project code is used as a reference.

Convolution, gaussian data (one case per launch shape): float64 accumulation rounded once, every element equal or an adjacent bf16 value
(|diff| <= 2^-12 below 2^-6, where an fp32 sum that cancels is noise), fewer than 1 % different: tests/test_cpu_twin_gpu.py's gate.

GroupNorm: two-pass float64 statistics on the bf16 inputs, g = RNE_bf16((x - m) / sqrt(v + eps) * w + b) from float64 in one rounding,
then RNE_bf16(g * sigmoid(g)) in float64 on the rounded g; `gn_gate` is the bracket gate and the count cap relative to torch-CPU's own bf16
F.group_norm on the same inputs.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.nn.functional as F

SENTINEL = 0xABCD            # what `out` holds before a call: a negative bf16 no case computes
NAN_BF16 = 0x7FC0            # guard bands
EPS = 1e-6


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


# ---------------------------------------------------------------------------------------------------------------------------------
# bf16 on the bit pattern
# ---------------------------------------------------------------------------------------------------------------------------------
RNE, TRUNC, TIES_AWAY = "rne", "trunc", "ties_away"


def f32_to_bf16_bits(a, how=RNE):
    """fp32 values -> bf16 bit patterns (uint16).  RNE: add 0x7FFF + the lowest kept bit, drop 16 bits.  TRUNC / TIES_AWAY: the planted mistakes."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    if how == RNE:
        u = u + 0x7FFF + ((u >> 16) & 1)
    elif how == TIES_AWAY:
        u = u + 0x8000
    return (u >> 16).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.ascontiguousarray(b, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f64_to_bf16_bits(a):
    """float64 -> bf16 in ONE rounding to nearest even (no trip through fp32): x / ulp is exact, rint is half-to-even"""
    a = np.asarray(a, dtype=np.float64)
    _, e = np.frexp(a)
    ulp = np.ldexp(1.0, e - 8)                       # |a| in [2^(e-1), 2^e): 8 significant bits
    v = np.rint(a / ulp) * ulp
    return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_ord(b):
    """bf16 bit patterns -> integers ordered like the values (+0 and -0 coincide): adjacent values differ by 1"""
    b = np.asarray(b, dtype=np.uint16).astype(np.int32)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


# ---------------------------------------------------------------------------------------------------------------------------------
# convolution cases
# ---------------------------------------------------------------------------------------------------------------------------------
ROWS, S2, N3, N1, P1 = "conv3x3_rows_kernel<1>", "<2,2,2,9,2>", "<4,1,1,9,1>", "<4,1,1,1,1>", "<2,4,1,1,1>"
LAUNCH_SHAPES = (ROWS, S2, N3, N1, P1)
TILE_H = {ROWS: 4, S2: 4, N3: 8, N1: 8, P1: 4}      # output rows per workgroup; every shape has 32 output columns
TILE_W = 32


@dataclass(frozen=True)
class ConvCase:
    name: str
    B: int
    H: int
    W: int
    Cin: int                     # the layer's input channels (what the image is packed with)
    Cout: int
    ks: int = 3
    stride: int = 1
    up: int = 0
    bn: int = 128
    resid: bool = False
    bias: bool = True
    cin_store: Optional[int] = None      # channels of x in memory (a multiple of 8 in the same 32-block count), default Cin
    cstore: Optional[int] = None         # default: Cout rounded up to 4
    ldo: Optional[int] = None            # default: Cstore
    rounding: bool = False               # claims to test the rounding (checked by rounding_stats)
    gauss: bool = False

    @property
    def cin_s(self):
        return self.cin_store or self.Cin

    @property
    def cs(self):
        return self.cstore or (self.Cout + 3) // 4 * 4

    @property
    def ld(self):
        return self.ldo or self.cs

    @property
    def Hi(self):
        return self.H << self.up

    @property
    def Wi(self):
        return self.W << self.up

    @property
    def Ho(self):
        return self.Hi // 2 if self.stride == 2 else self.Hi

    @property
    def Wo(self):
        return self.Wi // 2 if self.stride == 2 else self.Wi

    @property
    def taps(self):
        return self.ks * self.ks

    @property
    def ncb(self):
        return (self.Cin + 31) // 32

    @property
    def launch(self):
        """the launch shape selftok_conv2d_nhwc_bf16 picks for these arguments (csrc/conv.hip, the end of the entry)"""
        if self.bn == 32:
            return N3 if self.ks == 3 else N1
        if self.stride == 2:
            return S2
        return ROWS if self.ks == 3 else P1

    @property
    def channel_blocks(self):
        return (self.cs + self.bn - 1) // self.bn

    @property
    def block_bytes(self):
        """one channel block of the packed image"""
        return self.ncb * self.taps * self.bn * 32 * 2


def _c(*a, **k):
    return ConvCase(*a, **k)


CONV_EXACT = [
    # conv3x3_rows_kernel<1>: tile 4 x 32 x 128
    _c("rows_1x1x1_8to64", 1, 1, 1, 8, 64),
    _c("rows_3x5x33_40to132_res", 3, 5, 33, 40, 132, resid=True, rounding=True),                      # two channel blocks, the second 4 wide
    _c("rows_2x9x65_72to100_cs128_ldo136", 2, 9, 65, 72, 100, cstore=128, ldo=136, rounding=True),    # zero channels inside the block, pitch wider than the store
    _c("rows_1x4x32_32to128", 1, 4, 32, 32, 128, rounding=True),
    _c("rows_1x3x31_32to128", 1, 3, 31, 32, 128, rounding=True),
    _c("rows_1x2x2_512to512", 1, 2, 2, 512, 512, rounding=True),                                     # 16 input blocks x 4 channel blocks: both group parities, every tile pixel but four dead
    _c("rows_1x16x32_3to128_cin8", 1, 16, 32, 3, 128, cin_store=8),
    _c("rows_1x5x33_40to64_nobias", 1, 5, 33, 40, 64, bias=False, rounding=True),
    # <2,2,2,9,2>: stride 2, single halo buffer.  Odd sizes lose the last row / column, even ones read the padded one
    _c("s2_1x2x2_24to64", 1, 2, 2, 24, 64, stride=2),
    _c("s2_3x5x67_72to64", 3, 5, 67, 72, 64, stride=2, rounding=True),
    _c("s2_1x8x64_24to128", 1, 8, 64, 24, 128, stride=2, rounding=True),
    _c("s2_1x9x65_72to132", 1, 9, 65, 72, 132, stride=2, rounding=True),
    # <4,1,1,9,1>: bn 32, tile 8 x 32
    _c("n3_1x7x31_512to36", 1, 7, 31, 512, 36, bn=32, rounding=True),                                 # two blocks, the second 4 wide
    _c("n3_1x9x33_16to3_cs4", 1, 9, 33, 16, 3, bn=32, cstore=4),
    _c("n3_2x8x32_40to32", 2, 8, 32, 40, 32, bn=32, rounding=True),
    # <4,1,1,1,1>: 1 x 1, bn 32, four halo chunks per thread
    _c("n1_1x9x33_8to3", 1, 9, 33, 8, 3, ks=1, bn=32),
    _c("n1_2x1x1_72to32", 2, 1, 1, 72, 32, ks=1, bn=32),
    _c("n1_1x8x32_256to36", 1, 8, 32, 256, 36, ks=1, bn=32, rounding=True),                        # one whole tile; two blocks, the second 4 wide
    # <2,4,1,1,1>: 1 x 1, bn 128, the halo tile pipelined like the weights; ncb = 1, 2, 3 and 8
    _c("p1_2x4x32_32to256", 2, 4, 32, 32, 256, ks=1),
    _c("p1_1x5x33_40to64", 1, 5, 33, 40, 64, ks=1),
    _c("p1_1x1x1_8to128", 1, 1, 1, 8, 128, ks=1),
    _c("p1_1x5x33_72to64", 1, 5, 33, 72, 64, ks=1),
    _c("p1_1x5x33_256to64", 1, 5, 33, 256, 64, ks=1, rounding=True),
    # the nearest 2x upsample while staging
    _c("up_1x1x1_64to64", 1, 1, 1, 64, 64, up=1),
    _c("up_2x3x17_64to64", 2, 3, 17, 64, 64, up=1, rounding=True),                                    # Wo = 34
    _c("up_1x16x16_64to64", 1, 16, 16, 64, 64, up=1, rounding=True),                                  # 32 x 32 exactly
    _c("up_1x2x5_64to64_res", 1, 2, 5, 64, 64, up=1, resid=True, rounding=True),
]
CONV_GAUSS = [
    _c("gauss_rows_1x6x40_128to128_res", 1, 6, 40, 128, 128, resid=True, gauss=True),
    _c("gauss_s2_1x10x66_128to128", 1, 10, 66, 128, 128, stride=2, gauss=True),
    _c("gauss_n3_1x9x33_512to3", 1, 9, 33, 512, 3, bn=32, gauss=True),
    _c("gauss_n1_1x9x33_64to8", 1, 9, 33, 64, 8, ks=1, bn=32, gauss=True),
    _c("gauss_p1_1x5x33_512to128", 1, 5, 33, 512, 128, ks=1, gauss=True),
    _c("gauss_up_1x3x17_256to128", 1, 3, 17, 256, 128, up=1, gauss=True),
]
CONV_CASES = CONV_EXACT + CONV_GAUSS
CONV_BY_NAME = {c.name: c for c in CONV_CASES}
PACK_CASES = [(40, 24, 3, 32), (132, 40, 3, 128), (3, 8, 1, 32)]         # Cout, Cin, ksize, bn


_inputs = {}


def conv_inputs(case: ConvCase):
    """{x [B, H, W, cin_s], w [Cout, Cin, k, k], bias [Cout] | None, res [B, Ho, Wo, ldo] | None} as fp32 arrays of bf16 values, computed
    once and shared (read-only)"""
    if case.name in _inputs:
        return _inputs[case.name]
    r = np.random.default_rng(seed_of("conv_edges/" + case.name))
    xs, ws, rs = (case.B, case.H, case.W, case.cin_s), (case.Cout, case.Cin, case.ks, case.ks), (case.B, case.Ho, case.Wo, case.ld)
    if case.gauss:
        q = lambda a: bf16_bits_to_f32(f32_to_bf16_bits(a))
        d = dict(x=q(r.standard_normal(xs)), w=q(r.standard_normal(ws) / math.sqrt(case.Cin * case.taps)), bias=q(r.standard_normal(case.Cout)) if case.bias else None,
                 res=q(r.standard_normal(rs)) if case.resid else None)
    else:
        d = dict(x=r.integers(-8, 9, xs).astype(np.float32), w=r.integers(-8, 9, ws).astype(np.float32),
                 bias=r.integers(-64, 65, case.Cout).astype(np.float32) if case.bias else None,
                 res=bf16_bits_to_f32(f32_to_bf16_bits(r.integers(-512, 513, rs).astype(np.float32))) if case.resid else None)
    for v in d.values():
        if v is not None:
            assert np.array_equal(bf16_bits_to_f32(f32_to_bf16_bits(v)), v)       # bf16 values
            v.setflags(write=False)
    _inputs[case.name] = d
    return d


# planted mistakes
MUT_PAD_TOP_LEFT = "stride2_pad_top_left"
MUT_UP_ROUND = "upsample_source_rounds_up"
MUT_DYDX = "dy_dx_swapped"
MUT_CLAMP = "border_clamped"
MUT_TRUNC = "truncation"
MUT_TIES_AWAY = "ties_away_from_zero"
MUT_BIAS_AFTER = "bias_after_rounding"
MUT_ONE_ROUNDING = "one_rounding_for_x_plus_h"
MUT_CIN_TAIL = "cin_tail_dropped"
MUT_PARTIAL_TILE = "partial_tile_unwritten"
CONV_MISTAKES = (MUT_PAD_TOP_LEFT, MUT_UP_ROUND, MUT_DYDX, MUT_CLAMP, MUT_TRUNC, MUT_TIES_AWAY, MUT_BIAS_AFTER, MUT_ONE_ROUNDING, MUT_CIN_TAIL, MUT_PARTIAL_TILE)


def applies(case: ConvCase, mut: str):
    """can the planted mistake change this case's output?  True / False from the geometry and the arguments alone; None where the drawn data
    decides (a rounding mistake on a case that does not claim to test the rounding)"""
    if mut == MUT_PAD_TOP_LEFT:
        return case.stride == 2
    if mut == MUT_UP_ROUND:                          # (i + 1) >> 1 clamped to the source: a 1 x 1 source has one pixel to give
        return case.up == 1 and (case.H > 1 or case.W > 1)
    if mut == MUT_DYDX:                              # a 1 x 1 image under a padded 3 x 3 kernel meets the centre tap only
        return case.ks == 3 and (case.Hi > 1 or case.Wi > 1)
    if mut == MUT_CLAMP:                             # stride 2 on odd sizes never reads the padded row / column
        return case.ks == 3 and (case.stride == 1 or case.Hi % 2 == 0 or case.Wi % 2 == 0)
    if mut in (MUT_TRUNC, MUT_TIES_AWAY):
        return True if case.rounding else None
    if mut == MUT_BIAS_AFTER:
        return False if not case.bias else (True if case.rounding else None)
    if mut == MUT_ONE_ROUNDING:
        return False if not case.resid else (True if case.rounding else None)
    if mut == MUT_CIN_TAIL:
        return case.Cin % 32 != 0
    if mut == MUT_PARTIAL_TILE:
        return case.Wo % TILE_W != 0 or case.Ho % TILE_H[case.launch] != 0
    raise KeyError(mut)


def conv_sum(case: ConvCase, mut=None, with_bias=True, d=None):
    """float64 [B, Ho, Wo, Cout]: the convolution (+ bias) in float64 -- exact on the integer cases.  d: other operands than the case's own"""
    d = d or conv_inputs(case)
    x = torch.from_numpy(d["x"][..., :case.Cin].astype(np.float64)).permute(0, 3, 1, 2)
    w = torch.from_numpy(d["w"].astype(np.float64))
    if mut == MUT_CIN_TAIL:
        w = w.clone(); w[:, case.Cin // 32 * 32:] = 0
    if mut == MUT_DYDX:
        w = w.transpose(2, 3)
    if case.up:
        if mut == MUT_UP_ROUND:
            iy = torch.clamp((torch.arange(case.Hi) + 1) >> 1, max=case.H - 1); ix = torch.clamp((torch.arange(case.Wi) + 1) >> 1, max=case.W - 1)
            x = x[:, :, iy][:, :, :, ix]
        else:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
    bias = torch.from_numpy(d["bias"].astype(np.float64)) if (case.bias and with_bias) else None
    mode = dict(mode="replicate") if mut == MUT_CLAMP else {}
    if case.stride == 2:
        y = F.conv2d(F.pad(x, (1, 0, 1, 0) if mut == MUT_PAD_TOP_LEFT else (0, 1, 0, 1), **mode), w, bias, stride=2)
    elif case.ks == 3:
        y = F.conv2d(F.pad(x, (1, 1, 1, 1), **mode), w, bias)
    else:
        y = F.conv2d(x, w, bias)
    assert y.shape == (case.B, case.Cout, case.Ho, case.Wo)
    return np.ascontiguousarray(y.permute(0, 2, 3, 1).numpy())


def conv_abs_bound(case: ConvCase):
    """max over the outputs of sum |x| |w| + |b|: below 2^24, every partial sum in any order is an exact fp32 integer"""
    d = conv_inputs(case)
    return float(conv_sum(case, d=dict(x=np.abs(d["x"]), w=np.abs(d["w"]), bias=None if d["bias"] is None else np.abs(d["bias"]))).max())


def rounding_stats(case: ConvCase):
    """(share of the exact sums that are not bf16 values, number of exact ties) of an integer case"""
    s = conv_sum(case)
    low = s.astype(np.float32).view(np.uint32) & 0xFFFF
    return float((low != 0).mean()), int((low == 0x8000).sum())


_expected = {}


def conv_expected(case: ConvCase, mut=None):
    """uint16 [B, Ho, Wo, Cstore]: what the entry must store in channels [0, Cstore) (the reference of record; mut: a planted mistake)"""
    key = (case.name, mut)
    if mut is None and key in _expected:
        return _expected[key]
    d = conv_inputs(case)
    how = {MUT_TRUNC: TRUNC, MUT_TIES_AWAY: TIES_AWAY}.get(mut, RNE)
    s = conv_sum(case, mut, with_bias=mut != MUT_BIAS_AFTER)
    if case.gauss:
        assert mut is None
        h = f64_to_bf16_bits(s)
    else:
        assert np.array_equal(s, np.rint(s)) and np.abs(s).max() < 2 ** 24
        h = f32_to_bf16_bits(s.astype(np.float32), how)
        if mut == MUT_BIAS_AFTER and case.bias:
            h = f32_to_bf16_bits(bf16_bits_to_f32(h) + d["bias"], how)
    full = np.zeros((case.B, case.Ho, case.Wo, case.cs), np.uint16)         # channels [Cout, Cstore): zero weights, no bias
    full[..., :case.Cout] = h
    if case.resid:
        res = d["res"][..., :case.cs]
        if mut == MUT_ONE_ROUNDING:
            z = np.zeros(full.shape, np.float64); z[..., :case.Cout] = s
            full = f32_to_bf16_bits((z + res).astype(np.float32), how)
        elif case.gauss:
            full = f64_to_bf16_bits(bf16_bits_to_f32(full).astype(np.float64) + res)
        else:
            full = f32_to_bf16_bits(bf16_bits_to_f32(full) + res, how)        # fp32(bf16) + integer: exact in fp32
    if mut == MUT_PARTIAL_TILE:
        full = full.copy()
        full[:, case.Ho // TILE_H[case.launch] * TILE_H[case.launch]:] = SENTINEL
        full[:, :, case.Wo // TILE_W * TILE_W:] = SENTINEL
    if mut is None:
        full.setflags(write=False)
        _expected[key] = full
    return full


def gauss_gate(got, ref):
    """(ok, share different): every element equal or an adjacent bf16 value -- below 2^-6, where an fp32 sum that cancels is noise, within
    2^-12 -- and fewer than 1 % different (tests/test_cpu_twin_gpu.py's gate for bf16 outputs, tol 0)"""
    a, b = bf16_bits_to_f32(got), bf16_bits_to_f32(ref)
    near = np.where(np.abs(b) >= 2.0 ** -6, np.abs(bf16_ord(got) - bf16_ord(ref)) <= 1, np.abs(a - b) <= 2.0 ** -12)
    share = float((got != ref).mean())
    return bool(near.all()) and share < 0.01, share


def pack_expected(w_bits, Cout, Cin, ks, bn):
    """the documented image: [channel block][32-channel input block][tap][bn][32], zero padded (include/selftok_hip.h)"""
    taps, ncb, nb = ks * ks, (Cin + 31) // 32, (Cout + bn - 1) // bn
    p = np.zeros((nb, ncb, taps, bn, 32), np.uint16)
    w = w_bits.reshape(Cout, Cin, taps)
    for co in range(Cout):
        for c in range(Cin):
            p[co // bn, c // 32, :, co % bn, c % 32] = w[co, c]
    return p.reshape(-1)


def conv_call(lib, case: ConvCase, alloc, samples=None, out_fill=SENTINEL):
    """pack the weights and run the case on `lib` with buffers from alloc(uint16 or uint8 ndarray, name) -> object with .ptr / .numpy().
    Sizes of the packed image come from the library.  samples: a slice of the batch.  Returns (rc, out buffer, packed buffer)."""
    d = conv_inputs(case)
    sl = slice(None) if samples is None else samples
    x, res = d["x"][sl], (d["res"][sl] if case.resid else None)
    B = x.shape[0]
    nbytes = lib.selftok_conv2d_packed_bytes(case.Cout, case.Cin, case.ks, case.bn)
    assert nbytes == (case.Cout + case.bn - 1) // case.bn * case.block_bytes
    packed = alloc(np.full(nbytes // 2, NAN_BF16, np.uint16), "packed")
    wb = alloc(f32_to_bf16_bits(d["w"]), "w")
    rc = lib.selftok_conv2d_pack_weight_bf16(wb.ptr, packed.ptr, case.Cout, case.Cin, case.ks, case.bn, None)
    assert rc == 0, lib.selftok_last_error()
    out = alloc(np.full((B, case.Ho, case.Wo, case.ld), out_fill, np.uint16), "out")
    xb = alloc(f32_to_bf16_bits(x), "x")
    bb = alloc(f32_to_bf16_bits(d["bias"]), "bias") if case.bias else None
    rb = alloc(f32_to_bf16_bits(res), "res") if case.resid else None
    rc = lib.selftok_conv2d_nhwc_bf16(xb.ptr, packed.ptr, bb.ptr if bb else None, rb.ptr if rb else None, out.ptr, B, case.H, case.W, case.cin_s, case.Cout,
                                      case.cs, case.ld, case.ks, case.stride, case.up, case.bn, None)
    return rc, out, packed


# ---------------------------------------------------------------------------------------------------------------------------------
# GroupNorm cases
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GnCase:
    name: str
    layout: str                  # "nhwc": selftok_groupnorm_silu_nhwc_bf16 on [B, HW, C]; "nchw": selftok_groupnorm_silu_bf16 on [B, C, HW]
    B: int
    HW: int
    C: int
    groups: int
    content: str = "noise"       # noise: 2 N(0, 1) + 0.3; const: group 1 of every sample is constant 1.5; offset: 300 + N(0, 1)

    @property
    def nblk(self):
        """pixel ranges per sample of the NHWC statistics pass (gn_nblk, csrc/conv.hip)"""
        return min(max(self.HW // 256, 1), 32)

    @property
    def n(self):
        return self.B * self.HW * self.C


def _g(name, B, HW, C, groups, content="noise"):
    return GnCase("nhwc_" + name, "nhwc", B, HW, C, groups, content)


def _n(name, B, HW, C, groups, content="noise"):
    return GnCase("nchw_" + name, "nchw", B, HW, C, groups, content)


GN_CASES = (
    # pixel-range routes: 1 range; 2 equal; 2 ragged; 3 of 257, 257, 255; 6 x 267; 32 equal; 32 ragged
    [_g(f"hw{hw}_c128", 2 if hw < 8192 else 1, hw, 128, 32) for hw in (1, 255, 511, 512, 513, 769, 1600, 8192, 8193)] +
    # channel widths: one thread slot per chunk ... 256 chunks per pixel
    [_g("hw513_c8_g1", 2, 513, 8, 1), _g("hw513_c32_g8", 2, 513, 32, 8), _g("hw513_c512", 1, 513, 512, 32), _g("hw513_c1024", 1, 513, 1024, 32),
     _g("hw300_c2048", 1, 300, 2048, 32), _g("hw513_c256_g64", 1, 513, 256, 64),
     _g("b64_hw1100_c128", 64, 1100, 128, 32),                       # the apply pass's grid-stride loop: 69 blocks of chunks, 64 workgroups per sample
     _g("const_hw769_c128", 2, 769, 128, 32, "const"), _g("offset300_hw769_c128", 2, 769, 128, 32, "offset"), _g("b3_hw600_c256", 3, 600, 256, 32)] +
    [_n("hw8_c32", 2, 8, 32, 32),                                    # one channel per group: 511 idle threads
     _n("hw64_c64", 2, 64, 64, 32), _n("hw64_c512", 1, 64, 512, 32),  # 2 and 16 channels per group
     _n("hw520_c64", 2, 520, 64, 32), _n("hw4104_c128", 1, 4104, 128, 32),       # 130 and 2052 vectors per group: no multiple of the 512-thread block
     _n("const_hw520_c64", 2, 520, 64, 32, "const"), _n("offset300_hw520_c64", 2, 520, 64, 32, "offset"), _n("b3_hw64_c128", 3, 64, 128, 32)])
GN_BY_NAME = {c.name: c for c in GN_CASES}
CONST_VALUE, CONST_GROUP = 1.5, 1

_gn_inputs = {}


def gn_inputs(case: GnCase):
    """(x, w, b) bf16 bit patterns: x [B, HW, C] or [B, C, HW] in the case's layout, computed once and shared (read-only)"""
    if case.name not in _gn_inputs:
        r = np.random.default_rng(seed_of("conv_edges/gn/" + case.name))
        x = r.standard_normal((case.B, case.HW, case.C))            # drawn channels-last in both layouts
        x = 300.0 + x if case.content == "offset" else 2.0 * x + 0.3
        if case.content == "const":
            cpg = case.C // case.groups
            g = CONST_GROUP % case.groups
            x[:, :, g * cpg:(g + 1) * cpg] = CONST_VALUE
        if case.layout == "nchw":
            x = x.transpose(0, 2, 1)
        t = (f32_to_bf16_bits(np.ascontiguousarray(x, dtype=np.float32)), f32_to_bf16_bits(1 + 0.2 * r.standard_normal(case.C)), f32_to_bf16_bits(0.2 * r.standard_normal(case.C)))
        for v in t:
            v.setflags(write=False)
        _gn_inputs[case.name] = t
    return _gn_inputs[case.name]


def _as_bcp(case: GnCase, a):
    """the case's layout -> [B, C, HW]"""
    return a.transpose(0, 2, 1) if case.layout == "nhwc" else a


def silu64_bits(g_bits):
    g = bf16_bits_to_f32(g_bits).astype(np.float64)
    return f64_to_bf16_bits(g / (1.0 + np.exp(-g)))


_gn_ref = {}


def gn_reference(case: GnCase):
    """(g_ref, y_ref) uint16 in the case's layout: GroupNorm rounded once from float64, and SiLU of that rounded value rounded once"""
    if case.name not in _gn_ref:
        xb, wb, bb = gn_inputs(case)
        x = _as_bcp(case, bf16_bits_to_f32(xb).astype(np.float64)).reshape(case.B, case.groups, -1)
        m = x.mean(-1, keepdims=True)
        v = ((x - m) ** 2).mean(-1, keepdims=True)
        y = ((x - m) / np.sqrt(v + EPS)).reshape(case.B, case.C, case.HW)
        y = y * bf16_bits_to_f32(wb).astype(np.float64)[None, :, None] + bf16_bits_to_f32(bb).astype(np.float64)[None, :, None]
        g = np.ascontiguousarray(_as_bcp(case, f64_to_bf16_bits(y)))
        _gn_ref[case.name] = (g, silu64_bits(g))
        for a in _gn_ref[case.name]:
            a.setflags(write=False)
    return _gn_ref[case.name]


_gn_torch = {}


def gn_torch_counts(case: GnCase):
    """(plain, SiLU): how many elements of torch-CPU's own bf16 F.group_norm [+ F.silu] on the same inputs differ from the reference"""
    if case.name not in _gn_torch:
        xb, wb, bb = gn_inputs(case)
        t = lambda u: torch.from_numpy(u.view(np.int16).copy()).view(torch.bfloat16)
        x = t(np.ascontiguousarray(_as_bcp(case, xb)))
        g = F.group_norm(x, case.groups, t(wb), t(bb), EPS)
        bits = lambda a: np.ascontiguousarray(_as_bcp(case, a.contiguous().view(torch.int16).numpy().view(np.uint16)))
        g_ref, y_ref = gn_reference(case)
        _gn_torch[case.name] = (int((bits(g) != g_ref).sum()), int((bits(F.silu(g)) != y_ref).sum()))
    return _gn_torch[case.name]


def gn_cap(case: GnCase, silu: int):
    """the most elements that may differ from the reference: twice torch-CPU's own count, or the project's standing 99.95 % figure"""
    return max(2 * gn_torch_counts(case)[silu], math.ceil(5e-4 * case.n), 1)


def _gn_inside(case: GnCase, got, silu: int):
    g_ref, y_ref = gn_reference(case)
    if not silu:
        return np.abs(bf16_ord(got) - bf16_ord(g_ref)) <= 1
    # the kernel's rounded GroupNorm value may be g_ref or one of its two bf16 neighbours: SiLU of the three spans an interval; one output ulp beyond it
    o = bf16_ord(g_ref)
    unord = lambda v: np.where(v < 0, (-v) | 0x8000, v).astype(np.uint16)
    ys = np.stack([bf16_ord(silu64_bits(unord(o + k))) for k in (-1, 0, 1)])
    a = bf16_ord(got)
    return (a >= ys.min(0) - 1) & (a <= ys.max(0) + 1)


def gn_gate(case: GnCase, got, silu: int):
    """(every element inside its bracket, elements different from the reference, the cap on that number)"""
    ref = gn_reference(case)[silu]
    return bool(_gn_inside(case, got, silu).all()), int((got != ref).sum()), gn_cap(case, silu)


def gn_outside(case: GnCase, got, silu: int):
    """the elements outside the bracket, for a message: how many, the largest |reference| among them, the largest difference"""
    bad = ~_gn_inside(case, got, silu)
    if not bad.any():
        return "0 outside"
    a, b = bf16_bits_to_f32(got)[bad], bf16_bits_to_f32(gn_reference(case)[silu])[bad]
    return f"{int(bad.sum())} of {case.n} outside, |ref| <= {float(np.abs(b).max()):.1e}, off by <= {float(np.abs(a - b).max()):.1e}"


def gn_const_expected(case: GnCase, silu: int):
    """[cpg] bf16: what every element of the constant group's channels must hold: bf16(bias), through the reference SiLU if asked"""
    _, _, bb = gn_inputs(case)
    cpg = case.C // case.groups
    b = bb[(CONST_GROUP % case.groups) * cpg:(CONST_GROUP % case.groups + 1) * cpg]
    return silu64_bits(b) if silu else b


def gn_call(lib, case: GnCase, alloc, silu: int, samples=None, out_fill=SENTINEL):
    """run the case on `lib`; the workspace size comes from the library.  Returns (rc, out buffer)."""
    xb, wb, bb = gn_inputs(case)
    x = xb if samples is None else xb[samples]
    B = x.shape[0]
    out = alloc(np.full(x.shape, out_fill, np.uint16), "out")
    xd, wd, bd = alloc(x, "x"), alloc(wb, "w"), alloc(bb, "b")
    if case.layout == "nchw":
        return lib.selftok_groupnorm_silu_bf16(xd.ptr, wd.ptr, bd.ptr, out.ptr, B, case.C, case.HW, case.groups, EPS, silu, None), out
    ws = alloc(np.full(lib.selftok_groupnorm_nhwc_workspace_bytes(B, case.HW, case.C), 0xC0, np.uint8), "workspace")
    return lib.selftok_groupnorm_silu_nhwc_bf16(xd.ptr, wd.ptr, bd.ptr, out.ptr, ws.ptr, B, case.HW, case.C, case.groups, EPS, silu, None), out


# ---- refusals of selftok_conv2d_nhwc_bf16 ------------------------------------------------------------------------------------------------
EINVAL = -1
# (what, B, H, W, Cin, Cout, Cstore, ldo, ksize, stride, upsample, bn): launch nothing, write nothing.  The first four are new.
NEW_REFUSALS = [("cstore_opens_a_block_128", 1, 4, 4, 32, 128, 132, 132, 3, 1, 0, 128), ("cstore_opens_a_block_100_256", 1, 4, 4, 32, 100, 256, 256, 3, 1, 0, 128),
                ("cstore_opens_a_block_bn32", 1, 4, 4, 32, 32, 36, 36, 1, 1, 0, 32), ("cstore_opens_a_block_stride2", 1, 4, 4, 32, 128, 132, 132, 3, 2, 0, 128),
                ("empty_stride2_h1", 1, 1, 8, 32, 128, 128, 128, 3, 2, 0, 128), ("empty_stride2_w1", 2, 8, 1, 32, 128, 128, 128, 3, 2, 0, 128)]
OLD_REFUSALS = [("cin_not_8", 1, 4, 4, 12, 128, 128, 128, 3, 1, 0, 128), ("cstore_below_cout", 1, 4, 4, 32, 128, 124, 128, 3, 1, 0, 128),
                ("cstore_not_4", 1, 4, 4, 32, 126, 126, 128, 3, 1, 0, 128), ("ldo_below_cstore", 1, 4, 4, 32, 128, 128, 124, 3, 1, 0, 128),
                ("ksize_2", 1, 4, 4, 32, 128, 128, 128, 2, 1, 0, 128), ("stride2_1x1", 1, 4, 4, 32, 128, 128, 128, 1, 2, 0, 128),
                ("stride2_upsample", 1, 4, 4, 32, 128, 128, 128, 3, 2, 1, 128), ("stride2_bn32", 1, 4, 4, 32, 32, 32, 32, 3, 2, 0, 32),
                ("bn_64", 1, 4, 4, 32, 128, 128, 128, 3, 1, 0, 64), ("negative_batch", -1, 4, 4, 32, 128, 128, 128, 3, 1, 0, 128), ("h_zero", 1, 0, 4, 32, 128, 128, 128, 3, 1, 0, 128)]
NEW_MESSAGES = (b"Cstore opens a channel block", b"empty stride-2 output")


def refused_call(lib, alloc, r):
    """issue refusal case r with small live buffers; returns (rc, out bits)"""
    _, B, H, W, Cin, Cout, Cs, ldo, ks, stride, up, bn = r
    x = alloc(np.zeros(max(B, 1) * max(H, 1) * W * Cin * 4, np.uint16), "x")
    pk = alloc(np.zeros(max(lib.selftok_conv2d_packed_bytes(Cout, Cin, 3, 128), 2) // 2, np.uint16), "packed")
    out = alloc(np.full(max(B, 1) * max(H, 1) * 4 * W * 4 * max(ldo, 4), SENTINEL, np.uint16), "out")
    rc = lib.selftok_conv2d_nhwc_bf16(x.ptr, pk.ptr, None, None, out.ptr, B, H, W, Cin, Cout, Cs, ldo, ks, stride, up, bn, None)
    return rc, out.numpy()


class Host:
    """alloc for the CPU twin"""

    def __init__(self, a, name=""):
        self.a = np.ascontiguousarray(a).copy()
        self.ptr = self.a.ctypes.data

    def numpy(self):
        return self.a
