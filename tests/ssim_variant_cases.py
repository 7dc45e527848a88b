"""The case table of tests/test_ssim_variant_cpu.py / test_ssim_variant_gpu.py and a numpy restatement of the arithmetic of record of
selftok_img_ssim (csrc/image_ssim.hip): SSIM over "valid" windows with T separable fp64 window taps, a covariance normalisation `cov_norm` and a
data range of 1 ([0, 1] operands) or 2 ([-1, 1] operands), fp64 throughout, every operation rounded on its own.

Every case of the table is a generalisation of skimage.metrics.structural_similarity's defaults to T = 3, 7, 11: the uniform T x T window with the
sample covariance (cov_norm = T^2 / (T^2 - 1)); T = 7 is the package's own default.  The Gaussian / population reading is checked separately against
the emulation of tests/image_metrics_cases.py, whose contents and byte rules this module reuses.  numpy only; `mut=` plants the mistakes the table
must be able to see."""
from collections import namedtuple

import numpy as np

import image_metrics_cases as M

TILE_H, TILE_W = 16, 32                           # windows per tile of the kernel: a tile's pixels are (16 + T - 1) x (32 + T - 1)
TAPS = (3, 7, 11)
GPU_GATE = 1e-10                                  # |device - emulation| of tests/test_ssim_variant_gpu.py (derived in DESIGN.md section 30)

Case = namedtuple("Case", "name T H W B content recon_bf16 orig_bf16 orig_signed signed_range quantize")

MUTS = ("population_cov", "gaussian_window", "taps_11", "range_1_constants_on_signed", "range_2_constants_on_unsigned", "zero_padded_same", "fp32")


def sizes(T):
    th, tw = TILE_H + T - 1, TILE_W + T - 1
    return [(T, T), (T, T + 1), (th - 1, tw - 1), (th, tw), (th + 1, tw), (th, tw + 1), (th + 1, tw + 1), (64, 48), (256, 256)]


def _cases():
    out, n = [], 0
    for T in TAPS:
        for i, (H, W) in enumerate(sizes(T)):
            for j, content in enumerate(M.CONTENTS):
                big = H * W >= 65536
                if big and content in ("identical", "const01", "edges"):
                    continue
                B = (1, 2)[(i + j) % 2] if big else (1, 3, 5)[(i + j) % 3]
                rb, ob, osg, sr, qz = bool(n & 1), bool(n & 2), not (n & 4), not (n & 8), bool(n & 16)
                n += 7                              # walks all 32 dtype / original form / range / quantize combinations; each content meets both ranges
                if content == "nearflat":           # 0.5 + 1e-4 * noise only exists in fp32, and its bytes are constant
                    rb, qz = False, False
                name = f"t{T}_{H}x{W}_b{B}_{content}_{'bf16' if rb else 'f32'}_{'bf16' if ob else 'f32'}_{'s' if osg else 'u'}_{'R2' if sr else 'R1'}{'_u8' if qz else ''}"
                out.append(Case(name, T, H, W, B, content, rb, ob, osg, sr, qz))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
# an image of one or two windows of independent noise can have dS / d(cov_norm) near zero by chance (the derivative changes sign with the window's own
# covariance): the draw of that case is moved on until every planted mistake is visible in it -- the contents change, never the threshold
SEED_OFFSET = {(11, 11, 12, "noise"): 1}


def make(case, seed=0):
    """(recon, original) fp32 [B, 3, H, W]: image_metrics_cases' contents"""
    seed += SEED_OFFSET.get((case.T, case.H, case.W, case.content), 0)
    return M.make(M.Case(case.name, case.H, case.W, case.B, case.content, case.recon_bf16, case.orig_bf16, case.orig_signed, case.quantize), seed)


def uniform_window(T):
    return np.full(T, 1.0 / T)


def gaussian_window(T, sigma=1.5):
    i = np.arange(T, dtype=np.float64) - (T // 2)
    g = np.exp(-(i * i) / (2.0 * sigma ** 2))
    return g / g.sum()


def sample_cov_norm(T):
    return (T * T) / (T * T - 1.0)


def constants(signed_range):
    R = 2.0 if signed_range else 1.0
    return (0.01 * R) * (0.01 * R), (0.03 * R) * (0.03 * R)


def operands(recon, orig, recon_bf16, orig_signed, signed_range, quantize):
    """fp32 [.., H, W] x 2 -> the two fp64 operands of the SSIM expression"""
    recon, orig = np.asarray(recon, np.float32), np.asarray(orig, np.float32)
    if quantize:
        bx, by = M.quantized(recon, M.to_unit(orig, orig_signed), recon_bf16)
        x, y = bx.astype(np.float64) / 255.0, by.astype(np.float64) / 255.0
        return (2.0 * x - 1.0, 2.0 * y - 1.0) if signed_range else (x, y)
    if signed_range:
        return 2.0 * recon.astype(np.float64) - 1.0, orig.astype(np.float64) if orig_signed else 2.0 * orig.astype(np.float64) - 1.0
    return recon.astype(np.float64), M.to_unit(orig, orig_signed).astype(np.float64)


def _filter(a, g, axis):
    """"valid" correlation with the taps of g along `axis`, taps ascending from 0.0, every product and sum rounded on its own"""
    T = len(g)
    n = a.shape[axis] - (T - 1)
    taps = lambda k: a[..., k:k + n] if axis == -1 else a[..., k:k + n, :]
    acc = np.zeros_like(taps(0))
    for k in range(T):
        acc = acc + g[k] * taps(k)
    return acc


def smooth_separable(a, g):
    return _filter(_filter(a, g, -1), g, -2)                      # horizontal pass first, as the kernel


def smooth_direct2d(a, g):
    """the T^2-tap 2-D correlation with the outer product of the window, in numpy's extended precision (80-bit on x86-64): a naive fp64 sum of 121 equal terms
    is itself 12 ulp off on a constant image, which the signed const01 cases amplify by 4 / C2 to 3e-12 -- the comparator's own error, not the emulation's
    (2.5e-13 against this form)"""
    T = len(g)
    g, a = np.asarray(g, np.longdouble), np.asarray(a, np.longdouble)
    w2 = np.outer(g, g)
    h, w = a.shape[-2] - (T - 1), a.shape[-1] - (T - 1)
    acc = np.zeros(a.shape[:-2] + (h, w), np.longdouble)
    for i in range(T):
        for j in range(T):
            acc = acc + w2[i, j] * a[..., i:i + h, j:j + w]
    return acc


def ssim_map(x, y, g, cov_norm, signed_range, smooth=smooth_separable, mut=None):
    """fp64 [..., H, W] x 2 -> the SSIM value of every valid window [..., H - T + 1, W - T + 1]"""
    T = len(g)
    c1, c2 = constants(signed_range)
    if mut == "population_cov":
        cov_norm = 1.0
    elif mut == "gaussian_window":
        g = gaussian_window(T)
    elif mut == "taps_11":
        g, cov_norm = uniform_window(11), sample_cov_norm(11)
    elif mut in ("range_1_constants_on_signed", "range_2_constants_on_unsigned"):
        c1, c2 = constants(not signed_range)
    elif mut == "zero_padded_same":
        pad = [(0, 0)] * (x.ndim - 2) + [(T // 2, T // 2)] * 2
        x, y = np.pad(x, pad), np.pad(y, pad)
    elif mut == "fp32":
        x, y, g = x.astype(np.float32), y.astype(np.float32), g.astype(np.float32)
    elif mut is not None:
        raise KeyError(mut)
    ux, uy, uxx, uyy, uxy = (smooth(m, g).astype(np.float64) for m in (x, y, x * x, y * y, x * y))
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    return ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))


def ssim(recon, orig, g, cov_norm, signed_range, recon_bf16=False, orig_signed=True, quantize=False, smooth=smooth_separable, mut=None):
    """fp32 [B, 3, H, W] x 2 -> mean SSIM [B] fp64"""
    x, y = operands(recon, orig, recon_bf16, orig_signed, signed_range, quantize)
    s = ssim_map(x, y, np.asarray(g, np.float64), cov_norm, signed_range, smooth, mut)
    return s.reshape(s.shape[0], -1).sum(axis=1) / float(s[0].size)


_values = {}


def case_value(case, smooth=smooth_separable, mut=None):
    """mean SSIM [B] of a case; the plain emulation is computed once per case and shared -- read-only"""
    key = (case.name, mut) if smooth is smooth_separable else None
    if key is None or key not in _values:
        recon, orig = make(case)
        v = ssim(recon, orig, uniform_window(case.T), sample_cov_norm(case.T), case.signed_range, case.recon_bf16, case.orig_signed, case.quantize, smooth, mut)
        v.setflags(write=False)
        if key is None:
            return v
        _values[key] = v
    return _values[key]
