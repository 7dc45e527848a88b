"""not gpu: the arithmetic of record of the device image metrics (csrc/image_metrics.hip) pinned on the host -- the numpy emulation of
tests/image_metrics_cases.py against an independent 2-D formulation (and scipy when it is installed), its exact values on identical images,
its PSNR against evaluate.psnr_each, the byte recovery of the `quantize` mode, the planted mistakes the case table must be able to see, the
extension header against the ctypes table, the host-side refusals, and the kernels' LDS / scratch budget."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_io_cases as IO
import image_metrics_cases as M
from selftoktokenizer_amd import _lib, evaluate as E, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_img_metrics_workspace_bytes", "selftok_img_metrics"}
GPU_GATE = 1e-10                                # tests/test_image_metrics_gpu.py: |device SSIM - emulation|

_cache = {}


def emulated(case):
    if case.name not in _cache:
        _cache[case.name] = M.case_metrics(case)
    return _cache[case.name]


def test_case_table_covers_what_it_claims():
    assert {(c.H, c.W) for c in M.CASES} >= {(11, 11), (11, 40), (12, 12), (26, 42), (27, 42), (26, 43), (27, 43), (75, 42), (256, 256)}
    assert {c.B for c in M.CASES} == {1, 3, 5} and {c.content for c in M.CASES} == set(M.CONTENTS)
    combos = {(c.recon_bf16, c.orig_bf16, c.signed, c.quantize) for c in M.CASES}
    assert len(combos) == 16, sorted(combos)
    assert len({c.name for c in M.CASES}) == len(M.CASES)
    for c in M.CASES:                             # the inputs are representable in the dtype the case names
        recon, orig = M.make(c)
        assert recon.dtype == np.float32 and orig.dtype == np.float32 and recon.shape == (c.B, 3, c.H, c.W) == orig.shape
        if c.recon_bf16:
            assert not (recon.view(np.uint32) & 0xFFFF).any()
        if c.orig_bf16:
            assert not (orig.view(np.uint32) & 0xFFFF).any()
    edges = np.concatenate([M.make(c)[0].ravel() for c in M.CASES if c.content == "edges" and not c.recon_bf16])
    assert (edges < 0).any() and (edges > 1).any() and (edges == 0).any() and (edges == 1).any()


def test_window_is_the_normalised_gaussian():
    g = E.ssim_window()
    assert g.dtype == np.float64 and g.shape == (11,) and np.array_equal(g.view(np.uint64), M.window().view(np.uint64))
    assert abs(g.sum() - 1.0) <= 2.3e-16 and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1.0 / 4.5)) < 1e-15
    assert E.SSIM_DEFINITION == {"window": 11, "sigma": 1.5, "K1": 0.01, "K2": 0.03, "data_range": 1.0, "covariance": "population", "region": "valid"}


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_emulation_equals_the_independent_formulations(case):
    """separable, horizontal pass first == the direct 121-tap 2-D correlation == scipy's correlate1d cropped to the valid region"""
    ssim, mse = emulated(case)
    s2, m2 = M.case_metrics(case, smooth=M.smooth_direct2d)
    assert np.abs(ssim - s2).max() <= 1e-12 and np.array_equal(mse, m2)
    try:
        from scipy.ndimage import correlate1d
    except ImportError:
        return

    def smooth_scipy(a, g):
        a = correlate1d(correlate1d(np.asarray(a, np.float64), g, axis=-1, mode="constant"), g, axis=-2, mode="constant")
        return a[..., 5:-5, 5:-5]
    s3, _ = M.case_metrics(case, smooth=smooth_scipy)
    assert np.abs(ssim - s3).max() <= 1e-12


def test_identical_images_are_exact():
    """population moments and uncontracted products: numerator and denominator are the same bits, so SSIM == 1.0 and MSE == 0.0 exactly"""
    seen = 0
    for case in M.CASES:
        if case.content != "identical":
            continue
        ssim, mse = emulated(case)
        assert (ssim == 1.0).all() and (mse == 0.0).all(), case.name
        seen += 1
    assert seen >= 6
    for case in M.CASES:
        if case.content == "const01":
            ssim, mse = emulated(case)
            assert (mse == 1.0).all() and np.abs(ssim - M.C1 / (1.0 + M.C1)).max() < 1e-15, case.name


def test_psnr_equals_psnr_each():
    seen = 0
    for case in M.CASES:
        if not case.signed or case.quantize:
            continue                              # psnr_each takes the float values of a [-1, 1] original
        recon, orig = M.make(case)
        to = lambda a, bf: torch.from_numpy(a).to(torch.bfloat16) if bf else torch.from_numpy(a)
        want = E.psnr_each(to(recon, case.recon_bf16), to(orig, case.orig_bf16))
        got = E.psnr_of_mse(emulated(case)[1])
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(got)) and (got[~fin] == want[~fin]).all(), case.name
        assert np.abs(got[fin] - want[fin]).max(initial=0.0) <= 1e-9, case.name
        seen += 1
    assert seen >= 10


def test_quantize_recovers_the_bytes_of_a_preprocessed_original():
    u8 = np.arange(256, dtype=np.uint8)
    lut = IO.normalize_lut()                      # float32(u8) / 127.5 - 1: what the loader hands to the pipeline
    assert np.array_equal(IO.to_u8_f32(M.to_unit(lut, True)), u8)
    assert np.array_equal(IO.to_u8_f32((u8 / np.float32(255)).astype(np.float32)), u8)
    img = np.resize(u8, (1, 3, 16, 16))
    recon = (img / np.float32(255)).astype(np.float32)
    bx, by = M.quantized(recon, M.to_unit(lut[img], True), False)
    assert np.array_equal(bx, img) and np.array_equal(by, img)
    ssim, mse = M.metrics(recon, lut[img], False, True, True)
    assert ssim[0] == 1.0 and mse[0] == 0.0
    off = np.clip(img.astype(np.int64) + 3, 0, 255)                         # three levels off (two values clip): the exact integer MSE
    _, mse = M.metrics((off / np.float32(255)).astype(np.float32), lut[img], False, True, True)
    assert mse[0] == float(((off - img) ** 2).sum()) / (65025.0 * img.size)


MUTS = {"sample_covariance": M.MUT_SAMPLE_COV, "box_window": M.MUT_BOX, "zero_padded_same": M.MUT_SAME, "K2_0.3": M.MUT_K2}


@pytest.mark.parametrize("mut", list(MUTS), ids=list(MUTS))
def test_every_textured_case_sees_the_planted_mistake(mut):
    """each mistake moves the SSIM of every image of every case whose two images vary inside a window by >= 1000 x the GPU gate"""
    seen = 0
    for case in M.CASES:
        if case.content not in M.TEXTURED:
            continue
        d = np.abs(M.case_metrics(case, mut=MUTS[mut])[0] - emulated(case)[0])
        assert d.min() >= 1000 * GPU_GATE, f"{case.name}: {mut} moves the SSIM by only {d.min():.2e}"
        seen += 1
    assert seen >= 20


def test_near_flat_cases_see_fp32_accumulation():
    """sigma^2 = E[x^2] - mu^2 cancels eight digits on a near-flat image: fp32 anywhere in the moments is visible there (and almost not on noise)"""
    seen = 0
    for case in M.CASES:
        if case.content != "nearflat":
            continue
        d = np.abs(M.case_metrics(case, mut=M.MUT_FP32)[0] - emulated(case)[0])
        assert d.min() >= 1000 * GPU_GATE, f"{case.name}: fp32 accumulation moves the SSIM by only {d.min():.2e}"
        seen += 1
    assert seen >= 8


def test_ext_header_declares_the_metrics_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and names == set(_lib.EXT_SIGNATURES) and not (names & set(_lib.SIGNATURES))
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    for n in NEW_ENTRIES:
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want, (n, args)
        assert res == ctype_of[m.group(1)]
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_host_side_refusals_and_workspace_query_without_a_gpu():
    """every refusal is decided on the host before anything is launched, and the workspace query is host code"""
    lib = _lib.load()
    assert lib.selftok_img_metrics_workspace_bytes(1, 11, 11) == 3 * 16                    # one tile per plane, one pair of doubles each
    assert lib.selftok_img_metrics_workspace_bytes(1, 26, 42) == 3 * 16
    assert lib.selftok_img_metrics_workspace_bytes(2, 27, 43) == 2 * 3 * 4 * 16
    assert lib.selftok_img_metrics_workspace_bytes(64, 256, 256) == 64 * 3 * 16 * 8 * 16
    for (B, H, W), word in (((1, 10, 11), "H, W >= 11"), ((1, 11, 10), "H, W >= 11"), ((0, 11, 11), "B >= 1"), ((-1, 11, 11), "B >= 1"),
                            ((2731, 512, 512), "2^31"), ((1, 46341, 46341), "2^31"), ((2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), "2^31")):
        assert lib.selftok_img_metrics_workspace_bytes(B, H, W) == 0, (B, H, W)
        assert word in lib.selftok_last_error().decode(), (B, H, W, lib.selftok_last_error().decode())
    assert lib.selftok_img_metrics_workspace_bytes(2730, 512, 512) > 0                     # 2730 * 3 * 2^18 < 2^31 <= 2731 * 3 * 2^18
    x = np.zeros(3 * 11 * 11, np.float32)
    out, ws, g = np.zeros(2), np.zeros(6), E.ssim_window()
    p = lambda a: a.ctypes.data
    call = lambda recon, orig, win, o, w, wb, B, H, W: lib.selftok_img_metrics(recon, 0, orig, 0, 1, 0, win, o, w, wb, B, H, W, None)
    for args, word in (((None, p(x), p(g), p(out), p(ws), 48, 1, 11, 11), "null"), ((p(x), None, p(g), p(out), p(ws), 48, 1, 11, 11), "null"),
                       ((p(x), p(x), None, p(out), p(ws), 48, 1, 11, 11), "null"), ((p(x), p(x), p(g), None, p(ws), 48, 1, 11, 11), "null"),
                       ((p(x), p(x), p(g), p(out), None, 48, 1, 11, 11), "null"), ((p(x), p(x), p(g), p(out), p(ws), 47, 1, 11, 11), "workspace"),
                       ((p(x), p(x), p(g), p(out), p(ws), 48, 1, 10, 11), "H, W >= 11"), ((p(x), p(x), p(g), p(out), p(ws), 48, 1, 11, 10), "H, W >= 11"),
                       ((p(x), p(x), p(g), p(out), p(ws), 1 << 40, 2731, 512, 512), "2^31")):
        assert call(*args) == -1, word
        assert word in lib.selftok_last_error().decode(), (word, lib.selftok_last_error().decode())
    t = torch.zeros(1, 3, 16, 16)
    with pytest.raises(_lib.SelftokHipError):
        ops.image_metrics(t, t)                                                             # CPU tensors: there is no CPU fallback


def test_image_metrics_compiles_for_gfx950_within_its_budget(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "image_metrics.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(kernels) == 5 and len(scratch) == len(kernels) == len(lds), (kernels, scratch, lds)       # four dtype pairs of the main kernel + finish
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert max(lds) == 2 * 26 * 42 * 8 + 5 * 26 * 32 * 8 <= 65536, dict(zip(kernels, lds))
    src = open(os.path.join(G.CSRC, "image_metrics.hip")).read()
    assert "asm" not in src.replace("namespace", "") and "atomic" not in src.replace("No atomics", "")    # plain C++, no atomics of any kind
