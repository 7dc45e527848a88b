"""The case table of tools/gen_ssim_bits.py and tests/test_ssim_bits_gpu.py: the smallest inputs that reach every path of the two SSIM entries
(csrc/image_metrics.hip, csrc/image_ssim.hip, the tile body of csrc/ssim_shared.h).  B = 2, so the finish kernel's per-image offset counts; T x T is one
window, (T + 16) x (T + 32) is 17 x 33 windows = 2 x 2 tiles whose last row and column hold one window each.  numpy only; inputs come from
image_metrics_cases.make (a numpy generator seeded by the shape)."""
from collections import namedtuple

import numpy as np

import image_metrics_cases as M

B = 2
FIXTURE = "ssim_bits.json"

SsimCase = namedtuple("SsimCase", "name T window cov_norm signed_range inputs")        # inputs: the image_metrics_cases.Case that makes the two tensors


def _shapes(T):
    return [(T, T), (T + 16, T + 32)]


def _inputs(H, W, n, quantize):
    """the dtype pair and `original_signed` walk with n, one step out of phase with the four (signed_range, quantize) settings of a shape"""
    k = n + n // 4
    rb, ob, signed = bool(k & 1), bool(k & 2), bool(k & 4)
    return M.Case(f"{H}x{W}_{'bf16' if rb else 'f32'}_{'bf16' if ob else 'f32'}_{'s' if signed else 'u'}{'_u8' if quantize else ''}", H, W, B, "noise", rb, ob, signed, quantize)


def metrics_cases():
    """image_metrics: both shapes x all four dtype pairs x quantize off / on, original_signed alternating"""
    out = []
    for H, W in _shapes(M.KW):
        for n in range(8):
            rb, ob, quantize = bool(n & 1), bool(n & 2), bool(n & 4)
            signed = (n + H) % 2 == 0
            out.append(M.Case(f"{H}x{W}_{'bf16' if rb else 'f32'}_{'bf16' if ob else 'f32'}_{'s' if signed else 'u'}{'_u8' if quantize else ''}", H, W, B, "noise", rb, ob, signed,
                              quantize))
    return out


def ssim_cases():
    """image_ssim: every instantiation T = 3 .. 11 with the uniform window and the sample covariance, T = 11 also with the Gaussian window and population
    moments, x signed_range off / on x quantize off / on x both shapes; the dtype pair and original_signed alternate"""
    out, n = [], 0
    for T, window, cov in [(T, "uniform", T * T / (T * T - 1.0)) for T in (3, 5, 7, 9, 11)] + [(11, "gaussian", 1.0)]:
        for H, W in _shapes(T):
            for signed_range in (False, True):
                for quantize in (False, True):
                    inp = _inputs(H, W, n, quantize)
                    out.append(SsimCase(f"t{T}_{window}_{'r2' if signed_range else 'r1'}_{inp.name}", T, window, cov, signed_range, inp))
                    n += 1
    return out


def window(case):
    return M.window() if case.window == "gaussian" else np.full(case.T, 1.0 / case.T, dtype=np.float64)


def hex_bits(a):
    """fp64 array -> its bit patterns, 16 hex digits each, row-major"""
    return [f"{int(v):016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64)]


def run(ops, torch, device):
    """{"image_metrics": {case: [bits]}, "image_ssim": {case: [bits]}} of the two entries on `device`"""
    def dev(a, bf16):
        t = torch.from_numpy(a).to(device)
        return t.to(torch.bfloat16) if bf16 else t                # the values are representable: the conversion is exact

    res = {"image_metrics": {}, "image_ssim": {}}
    for c in metrics_cases():
        recon, orig = M.make(c)
        res["image_metrics"][c.name] = hex_bits(ops.image_metrics(dev(recon, c.recon_bf16), dev(orig, c.orig_bf16), c.signed, c.quantize).cpu().numpy())
    for c in ssim_cases():
        i = c.inputs
        recon, orig = M.make(i)
        got = ops.image_ssim(dev(recon, i.recon_bf16), dev(orig, i.orig_bf16), window(c), c.cov_norm, c.signed_range, i.signed, i.quantize)
        res["image_ssim"][c.name] = hex_bits(got.cpu().numpy())
    return res
