"""-m gpu: every entry point of include/selftok_hip.h issued twice on the same inputs -- on the gfx950 library with device pointers
and on its CPU twin (oracle/libselftok_cpu.so, pinned to the reference's golden vectors by tests/test_cpu_twin.py) with host pointers.

`exact` cases must agree bit for bit (integer ids, layouts, every kernel whose fp32 operation order is defined: the VQ lookup, the fused
residual / LayerNorm / modulate pass incl. its shuffle-reduction order, splits, latent format, Euler step ...); the others within the
stated absolute tolerance relative to the output scale (hardware exp / rsq / sin / cos, matrix-core summation order, fp32 atomics);
bf16 outputs: fewer than 1 % of the elements differ, none by more than 2 * 2^-7 * max(|x|, 2^-6) -- one bf16 ulp, two through SiLU's second
rounding (measured: >= 99.95 % equal, profiles/r3_cpu_twin_vs_gpu.txt)."""
import os
import subprocess

import numpy as np
import pytest

import abi_cases as A
from selftoktokenizer_amd import _lib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libs():
    path = os.path.join(ROOT, "oracle", "libselftok_cpu.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return _lib.load(), A.bind(path)


def same_bits(a, b):
    if a.dtype.kind == "f":
        nan = np.isnan(a)
        return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))
    return np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(A.CASES))
def test_gpu_library_matches_cpu_twin(libs, name):
    gpu, twin = libs
    spec = A.CASES[name]
    g, c = A.run(gpu, name, A.Dev), A.run(twin, name, A.Host)
    worst = 0.0
    for k in g:
        if k.startswith("_"):
            continue
        a, b = g[k], c[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if k == "overflow" or a.dtype.kind in "iu" and not (k.endswith("blk") or k.endswith("bf16") or k in ("o0", "o1")):
            assert np.array_equal(a, b), (k, a[:8], b[:8])
            continue
        if spec["exact"]:
            assert same_bits(a, b), (k, np.argwhere(a != b)[:4])
            continue
        if k.endswith("bf16"):                                     # GroupNorm statistics / convolution sums in a different order: one
            fa, fb = A.from_bf16(a), A.from_bf16(b)                # bf16 ulp (two through SiLU's second rounding), or fp32-sum noise where a sum cancels to ~0
            assert (np.abs(fa - fb) <= np.maximum(2 * 2.0 ** -7 * np.maximum(np.abs(fb), 2.0 ** -6), spec["tol"])).all() and (a != b).mean() < 0.01, (k, float(np.abs(fa - fb).max()), float((a != b).mean()))
            worst = max(worst, float((a != b).mean()))
            continue
        if a.dtype == np.uint16:                                   # a split activation: compare the values it encodes
            rows, cols = (g.get("_rows"), g.get("_cols")) if "_rows" in g else g["_blk" + k[-1]]
            (ah, al), (bh, bl) = A.split_planes(a, rows, cols), A.split_planes(b, rows, cols)
            a, b = ah + al / 2048, bh + bl / 2048
        scale = max(1.0, float(np.abs(b).max()))
        err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) / scale
        worst = max(worst, err)
        assert err <= spec["tol"], (k, err)
    what = "bit-exact" if spec["exact"] else ("%.4f %% of the bf16 outputs differ (by one ulp)" % (100 * worst) if any(k.endswith("bf16") for k in g) else
                                             "max err %.2e of scale (tol %.0e)" % (worst, spec["tol"]))
    print(f"{name}: {what}")
