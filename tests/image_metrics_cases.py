"""The case table of tests/test_image_metrics_cpu.py / test_image_metrics_gpu.py and a numpy restatement of the arithmetic of record of the
device image metrics (csrc/image_metrics.hip): the SSIM of Wang et al. in the form the common libraries share (11 x 11 separable Gaussian
window of sigma 1.5, "valid" windows, population moments, C1 = 0.01^2, C2 = 0.03^2, data range 1) in fp64, and the mean squared error with
evaluate.psnr_each's operations -- on the float values, or (`quantize`) on the bytes save_image writes.

numpy only.  `MUT_*` switches plant the mistakes the table must be able to see.  Inputs are fp32 arrays whose values are representable in
the dtype the case names, so `.to(bfloat16)` of them is exact."""
from collections import namedtuple

import numpy as np

import image_io_cases as IO

KW, HALO = 11, 10
TILE_H, TILE_W = 16 + HALO, 32 + HALO          # the pixels of exactly one tile of the kernel (16 x 32 windows)
C1, C2 = 0.01 * 0.01, 0.03 * 0.03

Case = namedtuple("Case", "name H W B content recon_bf16 orig_bf16 signed quantize")

SIZES = [(11, 11), (11, 40), (12, 12), (TILE_H, TILE_W), (TILE_H + 1, TILE_W), (TILE_H, TILE_W + 1), (TILE_H + 1, TILE_W + 1), (75, 42), (256, 256)]
CONTENTS = ["noise", "recon_noise", "nearflat", "identical", "const01", "edges"]
TEXTURED = ("noise", "recon_noise", "edges")    # both images vary inside a window: every term of the SSIM expression is live


def _cases():
    out = []
    for i, (H, W) in enumerate(SIZES):
        for j, content in enumerate(CONTENTS):
            big = H * W >= 65536
            if big and content in ("identical", "const01", "edges"):
                continue
            B = (1, 3)[(i + j) % 2] if big else (1, 3, 5)[(i + j) % 3]
            n = 7 * i + j                           # walks the 16 dtype / range / quantize combinations; every content meets both parities
            rb, ob, signed, quant = bool(n & 1), bool(n & 2), not (n & 4), bool(n & 8)
            if content == "nearflat":               # 0.5 + 1e-4 * noise only exists in fp32, and its bytes are constant
                rb, quant = False, False
            out.append(Case(f"{H}x{W}_b{B}_{content}_{'bf16' if rb else 'f32'}_{'bf16' if ob else 'f32'}_{'s' if signed else 'u'}{'_u8' if quant else ''}",
                            H, W, B, content, rb, ob, signed, quant))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def window():
    """g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) normalised to sum 1, fp64 -- written out here; evaluate.ssim_window must give these bits"""
    i = np.arange(KW, dtype=np.float64) - 5.0
    g = np.exp(-(i * i) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _bf16(a):
    return IO._rne_bf16(np.ascontiguousarray(a, np.float32))


def make(case, seed=0):
    """(recon, original) fp32 [B, 3, H, W]; recon in (about) [0, 1], original in [-1, 1] when case.signed else [0, 1]"""
    rng = np.random.default_rng([seed, case.H, case.W, case.B, CONTENTS.index(case.content)])
    shape = (case.B, 3, case.H, case.W)
    u = lambda: rng.random(shape)
    if case.content == "identical":               # k / 128: exact in bf16, and (2 o - 1 + 1) / 2 gives it back exactly
        pool = np.arange(129) / 128.0
        if case.quantize and case.recon_bf16:     # x * 255 + 0.5 rounds differently in bf16: keep the values whose two bytes agree
            p32 = pool.astype(np.float32)
            pool = pool[IO.to_u8_bf16((p32.view(np.uint32) >> 16).astype(np.uint16)) == IO.to_u8_f32(p32)]
        o01 = pool[rng.integers(0, len(pool), shape)]
        x = o01
    elif case.content == "noise":
        o01, x = u(), u()
    elif case.content == "recon_noise":           # a low-contrast original (variance of the order of C2) and a slightly noisy copy
        o01 = 0.5 + 0.1 * (u() - 0.5)
        x = o01 + 0.04 * (u() - 0.5)
    elif case.content == "nearflat":
        o01 = np.full(shape, 0.5)
        x = 0.5 + 1e-4 * u()
    elif case.content == "const01":
        o01, x = np.ones(shape), np.zeros(shape)
    elif case.content == "edges":                 # 0, 1, just outside [0, 1] on both sides, the byte-rounding midpoints
        pool = np.array([0.0, 1.0, -1e-3, 1.0 + 1e-3, 0.5, 0.5 / 255, 254.5 / 255, 0.25])
        o01 = np.clip(pool[rng.integers(0, len(pool), shape)], 0.0, 1.0)
        x = pool[rng.integers(0, len(pool), shape)]
    else:
        raise ValueError(case.content)
    orig = (2.0 * o01 - 1.0) if case.signed else o01
    x, orig = x.astype(np.float32), orig.astype(np.float32)
    return (_bf16(x) if case.recon_bf16 else x), (_bf16(orig) if case.orig_bf16 else orig)


# ---- the arithmetic of record ----
MUT_NONE, MUT_SAMPLE_COV, MUT_BOX, MUT_SAME, MUT_K2, MUT_FP32 = range(6)


def to_unit(orig, signed):
    """fp32 original -> o in [0, 1], fp32: evaluate.psnr_each's expression"""
    orig = np.asarray(orig, np.float32)
    return ((orig + np.float32(1.0)) / np.float32(2.0)).astype(np.float32) if signed else orig


def quantized(recon, o, recon_bf16):
    """the bytes save_image writes: the reconstruction in its own type, o in fp32"""
    bx = IO.to_u8_bf16((np.ascontiguousarray(recon, np.float32).view(np.uint32) >> 16).astype(np.uint16)) if recon_bf16 else IO.to_u8_f32(recon)
    return bx, IO.to_u8_f32(o)


def _filter(a, g, axis):
    """"valid" correlation with the 11 taps along `axis`, taps ascending, every product and sum rounded on its own"""
    n = a.shape[axis] - HALO
    taps = lambda k: a[..., k:k + n] if axis == -1 else a[..., k:k + n, :]
    acc = np.zeros_like(taps(0))
    for k in range(KW):
        acc = acc + g[k] * taps(k)
    return acc


def smooth_separable(a, g):
    return _filter(_filter(a, g, -1), g, -2)                      # horizontal pass first, as the kernel


def smooth_direct2d(a, g):
    """the 121-tap 2-D form of the same window"""
    w2 = np.outer(g, g)
    h, w = a.shape[-2] - HALO, a.shape[-1] - HALO
    acc = np.zeros(a.shape[:-2] + (h, w))
    for i in range(KW):
        for j in range(KW):
            acc = acc + w2[i, j] * a[..., i:i + h, j:j + w]
    return acc


def ssim_map(x, y, g=None, smooth=smooth_separable, mut=MUT_NONE):
    """fp64 [..., H, W] x 2 -> the SSIM value of every valid window [..., H - 10, W - 10]"""
    g = window() if g is None else g
    c2 = 0.3 * 0.3 if mut == MUT_K2 else C2
    if mut == MUT_BOX:
        g = np.full(KW, 1.0 / KW)
    if mut == MUT_SAME:
        pad = [(0, 0)] * (x.ndim - 2) + [(HALO // 2, HALO // 2)] * 2
        x, y = np.pad(x, pad), np.pad(y, pad)
    if mut == MUT_FP32:
        x, y, g = x.astype(np.float32), y.astype(np.float32), g.astype(np.float32)
    mux, muy, sxx, syy, sxy = (smooth(m, g).astype(np.float64) for m in (x, y, x * x, y * y, x * y))
    vx, vy, vxy = sxx - mux * mux, syy - muy * muy, sxy - mux * muy
    if mut == MUT_SAMPLE_COV:
        n = float(KW * KW)
        vx, vy, vxy = vx * (n / (n - 1.0)), vy * (n / (n - 1.0)), vxy * (n / (n - 1.0))
    return ((2.0 * mux * muy + C1) * (2.0 * vxy + c2)) / ((mux * mux + muy * muy + C1) * (vx + vy + c2))


def metrics(recon, orig, recon_bf16=False, signed=True, quantize=False, smooth=smooth_separable, mut=MUT_NONE):
    """fp32 [B, 3, H, W] x 2 -> (mean SSIM [B], MSE [B]) fp64"""
    recon = np.asarray(recon, np.float32)
    o = to_unit(orig, signed)
    B = recon.shape[0]
    count = float(recon[0].size)
    if quantize:
        bx, by = quantized(recon, o, recon_bf16)
        d = bx.astype(np.int64) - by.astype(np.int64)
        mse = (d * d).reshape(B, -1).sum(axis=1).astype(np.float64) / (65025.0 * count)
        x, y = bx.astype(np.float64) / 255.0, by.astype(np.float64) / 255.0
    else:
        d = (recon - o).astype(np.float32)
        mse = (d * d).astype(np.float32).reshape(B, -1).astype(np.float64).sum(axis=1) / count
        x, y = recon.astype(np.float64), o.astype(np.float64)
    s = ssim_map(x, y, smooth=smooth, mut=mut)
    return s.reshape(B, -1).sum(axis=1) / float(s[0].size), mse


def case_metrics(case, **kw):
    recon, orig = make(case)
    return metrics(recon, orig, case.recon_bf16, case.signed, case.quantize, **kw)
