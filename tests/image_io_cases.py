"""The case table of tests/test_image_io_cpu.py / test_image_io_gpu.py and a numpy restatement of the arithmetic of record:
torchvision Resize(S) on a PIL image (Pillow's 8-bit ImagingResample: fp64 weights, 22-bit fixed-point coefficients, horizontal pass
first, uint8 between the passes) -> CenterCrop(S) (Python's round: half to even) -> NormalizeToTensor, and save_image's uint8 conversion.

Images are arithmetic (an integer hash of the pixel index, sawtooth ramps, 0 / 255 stripes), never an RNG stream.  The emulation only
computes the crop window; `MUT_*` switches plant the mistakes the table must be able to see.

    python tests/image_io_cases.py --write-golden      # re-records tests/golden/image_io.npz with the installed Pillow
"""
import math
import os
import zlib
from collections import namedtuple

import numpy as np

PB = 22
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_io.npz")

Case = namedtuple("Case", "name w h S content")

_GEOM13 = [(500, 375), (375, 500), (257, 256), (256, 999), (1024, 768), (300, 300), (255, 255), (100, 180), (640, 427), (3000, 2000), (256, 256),
           (511, 513), (77, 1031)]
_CONTENT = ["noise", "ramp", "stripes1", "noise", "noise", "noise", "stripes3", "ramp", "noise", "noise", "noise", "stripes3", "noise"]

CASES = [Case(f"g{w}x{h}", w, h, 256, c) for (w, h), c in zip(_GEOM13, _CONTENT)] + [
    Case("s128_500x375", 500, 375, 128, "noise"),
    Case("s128_97x131", 97, 131, 128, "stripes2"),
    Case("s320_640x427", 640, 427, 320, "noise"),
    Case("s320_1024x768", 1024, 768, 320, "ramp"),
    Case("crop_42p5_down", 500, 375, 256, "stripes1"),          # ow 341: (341 - 256) / 2 = 42.5 -> 42
    Case("crop_43p5_up", 686, 512, 256, "noise"),               # ow 343: 43.5 -> 44
    Case("crop_0p5_down_v", 256, 257, 256, "noise"),            # crop only, top 0.5 -> 0
    Case("crop_1p5_up_v", 512, 518, 256, "noise"),              # oh 259: 1.5 -> 2
    Case("side_is_S_w343", 343, 256, 256, "noise"),             # no pass at all, left 43.5 -> 44
    Case("side_is_S_h700", 256, 700, 256, "ramp"),
    Case("one_wide", 1, 5, 256, "noise"),
    Case("one_high", 7, 1, 256, "noise"),
    Case("one_pixel", 1, 1, 256, "noise"),
    Case("long_6100", 700, 6100, 256, "noise"),
    Case("taps49_6000", 6000, 6016, 256, "tiled"),              # 6000 / 256 = 23.4: 49 taps on both axes
]
BY_NAME = {c.name: c for c in CASES}
MIXED = [c for c in CASES if c.S == 256]                        # the batch that mixes all of them
TABLE_GEOMS = [(500, 341), (375, 256), (6000, 256)]             # (in, out) of the coefficient tables kept in the golden file


def _hash(x, y, c, seed):
    v = (x.astype(np.uint32) * np.uint32(0x9E3779B1)) ^ (y.astype(np.uint32) * np.uint32(0x85EBCA6B)) ^ (c.astype(np.uint32) * np.uint32(0xC2B2AE35)) ^ np.uint32(seed)
    v ^= v >> np.uint32(15); v *= np.uint32(0x2C1B3C6D); v ^= v >> np.uint32(12); v *= np.uint32(0x297A2D39); v ^= v >> np.uint32(15)
    return (v >> np.uint32(11)).astype(np.uint8)


def image(case, seed=0):
    """uint8 [h, w, 3], a function of the pixel index alone"""
    w, h, kind = case.w, case.h, case.content
    seed = (seed * 7919 + w * 31 + h * 17 + case.S) & 0x7FFFFFFF
    if kind == "tiled":
        t = image(Case("t", 509, 503, case.S, "noise"), seed)
        return np.ascontiguousarray(np.tile(t, ((h + 502) // 503, (w + 508) // 509, 1))[:h, :w])
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    if kind == "noise":
        return _hash(x, y, c, seed)
    if kind == "ramp":                                           # sawtooth: smooth inside a tooth, 7 / 13 levels per pixel
        return ((x * 7 + y * 13 + c * 85 + seed) % 256).astype(np.uint8)
    p = int(kind[-1])                                            # 0 / 255 stripes of period p along both axes, one phase per channel
    return (((x // p + y // p + c) % 2) * 255).astype(np.uint8)


# ---- the arithmetic of record ----
def target_size(w, h, S):
    if (w <= h and w == S) or (h <= w and h == S):
        return w, h
    return (S, int(S * h / w)) if w < h else (int(S * w / h), S)


def crop_offset(side, S, half_up=False):
    v = (side - S) / 2.0
    return int(math.floor(v + 0.5)) if half_up else int(round(v))


def tables(insz, outsz, first, count):
    """tap rows of output indices first .. first + count: (xmin [count], n [count], k [count, kmax] int64); the identity when no pass is needed"""
    if insz == outsz:
        return np.arange(first, first + count), np.ones(count, np.int64), np.full((count, 1), 1 << PB, np.int64)
    scale = insz / outsz
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    xx = np.arange(first, first + count, dtype=np.float64)
    center = (xx + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)              # astype truncates toward zero, as (int)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), insz) - xmin
    kmax = int(xmax.max())
    w = np.zeros((count, kmax))
    ww = np.zeros(count)
    for x in range(kmax):                                                        # left to right, as the C loop accumulates ww
        a = np.abs(((x + xmin) - center + 0.5) * ss)
        w[:, x] = np.where((a < 1.0) & (x < xmax), 1.0 - a, 0.0)
        ww = ww + w[:, x]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, (-0.5 + w * (1 << PB)).astype(np.int64), (0.5 + w * (1 << PB)).astype(np.int64))
    k[np.arange(kmax)[None, :] >= xmax[:, None]] = 0
    return xmin, xmax, k


MUT_NONE, MUT_XMIN, MUT_TRUNC, MUT_NO_U8, MUT_HALF_UP = range(5)


def _pass(a, tab, mut, keep_float=False, from_float=False):
    """resample axis 1 of [R, N, 3] with the tap rows `tab` -> [R, count, 3]"""
    xmin, n, k = tab
    out = np.empty((a.shape[0], len(xmin), 3), np.float64 if keep_float else np.uint8)
    src = a if from_float else a.astype(np.int64)
    half = 0 if mut == MUT_TRUNC else 1 << (PB - 1)
    for i in range(len(xmin)):
        x0, m = int(xmin[i]), int(n[i])
        s = np.tensordot(src[:, x0:x0 + m], k[i, :m].astype(src.dtype), axes=([1], [0]))
        if keep_float:
            out[:, i] = s / float(1 << PB)
        else:
            out[:, i] = np.clip(np.floor(s + half).astype(np.int64) >> PB if from_float else (half + s) >> PB, 0, 255)
    return out


def resize_crop(a, S, mut=MUT_NONE):
    """uint8 [h, w, 3] -> uint8 [S, S, 3]: CenterCrop(S)(Resize(S)(image)), the crop window only"""
    h, w, _ = a.shape
    ow, oh = target_size(w, h, S)
    left, top = crop_offset(ow, S, mut == MUT_HALF_UP), crop_offset(oh, S, mut == MUT_HALF_UP)
    th, tv = tables(w, ow, left, S), tables(h, oh, top, S)
    if mut == MUT_XMIN:                                           # one output index (the middle one) of every real pass reads one pixel off
        def shift(tab, insz):
            xmin, n, k = (t.copy() for t in tab)
            i = S // 2
            assert n[i] < insz
            xmin[i] += 1 if xmin[i] + n[i] < insz else -1
            return xmin, n, k
        th = shift(th, w) if w != ow and w > 1 else th
        tv = shift(tv, h) if h != oh and h > 1 else tv
    r0, r1 = int(tv[0].min()), int((tv[0] + tv[1]).max())         # the input rows the S output rows touch
    both = w != ow and h != oh
    if mut == MUT_NO_U8 and both:
        mid = _pass(a[r0:r1], th, mut, keep_float=True)
        out = _pass(mid.transpose(1, 0, 2), (tv[0] - r0, tv[1], tv[2]), mut, from_float=True)
    else:
        mid = _pass(a[r0:r1], th, mut)
        out = _pass(mid.transpose(1, 0, 2), (tv[0] - r0, tv[1], tv[2]), mut)
    return np.ascontiguousarray(out.transpose(1, 0, 2))


def applies(case, mut):
    """does the planted mistake change the arithmetic of this case at all?"""
    ow, oh = target_size(case.w, case.h, case.S)
    hp, vp = case.w != ow, case.h != oh
    if mut == MUT_XMIN:
        return (hp and case.w > 1) or (vp and case.h > 1)
    if mut == MUT_TRUNC:
        return (hp and case.w > 1) or (vp and case.h > 1)         # a 1-pixel side resamples to itself: every sum is v * 2^22 exactly
    if mut == MUT_NO_U8:
        return hp and vp and case.w > 1 and case.h > 1
    if mut == MUT_HALF_UP:
        return any(crop_offset(s, case.S) != crop_offset(s, case.S, True) for s in (ow, oh)) and min(case.w, case.h) > 1
    return False


def normalize_lut():
    """fp32 [256]: the very expression of pipeline.NormalizeToTensor on every uint8 value"""
    from selftoktokenizer_amd.pipeline import NormalizeToTensor
    return NormalizeToTensor()(np.arange(256, dtype=np.uint8).reshape(1, 256, 1)).numpy().reshape(256).copy()


def bf16_bits(f32):
    """fp32 array -> uint16 bf16 patterns, round to nearest even (no NaN here)"""
    u = np.ascontiguousarray(f32, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def to_tensor(u8, bf16):
    """uint8 [S, S, 3] -> CHW fp32 values, or their bf16 patterns as uint16"""
    t = normalize_lut()[u8.transpose(2, 0, 1)]
    return bf16_bits(t) if bf16 else t


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


# ---- save_image's uint8 conversion ----
def _rne_bf16(f32):
    u = f32.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def to_u8_bf16(bits):
    """uint16 bf16 patterns -> uint8: x * 255 rounded to bf16, + 0.5 rounded to bf16, clamp, truncate; NaN -> 0"""
    x = (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)
    nan = np.isnan(x)
    x = np.where(nan, np.float32(0), x)
    with np.errstate(over="ignore", invalid="ignore"):
        y = _rne_bf16(np.ascontiguousarray(x * np.float32(255)))
        y = _rne_bf16(np.ascontiguousarray(y + np.float32(0.5)))
    out = np.clip(y, 0, 255).astype(np.uint8)
    out[nan] = 0
    return out


def to_u8_f32(x):
    x = np.asarray(x, np.float32)
    nan = np.isnan(x)
    with np.errstate(over="ignore", invalid="ignore"):
        y = (np.where(nan, np.float32(0), x) * np.float32(255)).astype(np.float32) + np.float32(0.5)
    out = np.clip(y.astype(np.float32), 0, 255).astype(np.uint8)
    out[nan] = 0
    return out


def f32_samples():
    """fp32 inputs of the to_u8 test: every k / 255 and its neighbours, a dense sweep of [-0.1, 1.1], +-Inf, +-0, huge, tiny"""
    k = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    hk = ((np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255)).astype(np.float32)      # where the byte changes
    near = []
    for b in (k, hk):
        u = b.view(np.uint32)
        near += [b] + [(u + np.uint32(d)).view(np.float32) for d in (1, 2)] + [(np.maximum(u, 2) - np.uint32(d)).view(np.float32) for d in (1, 2)]
    sweep = (np.arange(-6553, 72090, dtype=np.float32) * np.float32(1.0 / 65536)).astype(np.float32)
    edge = np.array([np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30, 1e-40, -1e-40, 3.4e38, -3.4e38, 1.0, 2.0, 255.0, 256.0], np.float32)
    return np.concatenate(near + [sweep, edge])


# ---- golden ----
def make_golden():
    import PIL
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([c.name for c in CASES])}
    u8, bf = [], []
    for c in CASES:
        r = resize_crop(image(c), c.S)
        u8.append(crc(r)); bf.append(crc(to_tensor(r, True)))
    out["crc_u8"] = np.array(u8, np.uint32); out["crc_bf16"] = np.array(bf, np.uint32)
    for insz, outsz in TABLE_GEOMS:
        xmin, n, k = tables(insz, outsz, 0, outsz)
        out[f"tab_{insz}_{outsz}_xmin"] = xmin.astype(np.int32); out[f"tab_{insz}_{outsz}_n"] = n.astype(np.int32); out[f"tab_{insz}_{outsz}_k"] = k.astype(np.int32)
    return out


if __name__ == "__main__":
    import sys
    if "--write-golden" in sys.argv:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        np.savez_compressed(GOLDEN, **make_golden())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
