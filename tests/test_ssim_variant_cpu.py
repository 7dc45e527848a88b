"""not gpu: the arithmetic of record of selftok_img_ssim (csrc/image_ssim.hip) pinned on the host -- the numpy emulation of
tests/ssim_variant_cases.py against scipy's uniform_filter cropped to the valid region (the pin available offline for scikit-image's filter) and a
direct T^2-tap correlation, the Gaussian / population preset against the emulation of tests/image_metrics_cases.py, the exact 1.0 of identical
images, the planted mistakes the table must be able to see, the new declarations against the ctypes table, the kernels' scratch / LDS budget, the
host-side refusals, and the argument check of evaluate()."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_metrics_cases as M
import ssim_variant_cases as S
from selftoktokenizer_amd import _lib, evaluate as E, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_img_ssim_workspace_bytes", "selftok_img_ssim"}
TEXTURED = M.TEXTURED


def test_case_table_covers_what_it_claims():
    assert {c.T for c in S.CASES} == {3, 7, 11} and {c.B for c in S.CASES} == {1, 2, 3, 5}
    for T in S.TAPS:
        th, tw = 16 + T - 1, 32 + T - 1
        assert {(c.H, c.W) for c in S.CASES if c.T == T} == {(T, T), (T, T + 1), (th - 1, tw - 1), (th, tw), (th + 1, tw), (th, tw + 1), (th + 1, tw + 1), (64, 48), (256, 256)}
        assert {c.content for c in S.CASES if c.T == T} == set(M.CONTENTS)
    assert len({(c.recon_bf16, c.orig_bf16, c.orig_signed, c.signed_range, c.quantize) for c in S.CASES}) == 32
    for content in M.CONTENTS:                    # every content meets both ranges, and both input forms where it has bytes of its own
        mine = [c for c in S.CASES if c.content == content]
        assert {c.signed_range for c in mine} == {True, False} and {c.orig_signed for c in mine} == {True, False}, content
        assert content == "nearflat" or {c.quantize for c in mine} == {True, False}, content
    assert len({c.name for c in S.CASES}) == len(S.CASES)
    assert np.array_equal(E.ssim_uniform_window(), S.uniform_window(7)) and E.ssim_uniform_window(3).shape == (3,) and abs(E.ssim_uniform_window(11).sum() - 1) < 1e-15
    for bad in (2, 1, 13, 8):
        with pytest.raises(ValueError):
            E.ssim_uniform_window(bad)
    win, cn = ops.ssim_preset("skimage")
    assert np.array_equal(win, S.uniform_window(7)) and cn == 49.0 / 48.0 == S.sample_cov_norm(7)
    win, cn = ops.ssim_preset("gaussian")
    assert np.array_equal(win, M.window()) and cn == 1.0
    with pytest.raises(ValueError):
        ops.ssim_preset("box")
    assert S.constants(False) == (M.C1, M.C2) and S.constants(True) == (0.02 * 0.02, 0.06 * 0.06)


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_emulation_equals_scipy_uniform_filter_and_the_direct_correlation(case):
    """separable, horizontal pass first == scipy.ndimage.uniform_filter(size=T) cropped by (T - 1) / 2 (scikit-image's filter and crop) == the T^2-tap 2-D form"""
    from scipy.ndimage import uniform_filter
    v = S.case_value(case)
    assert v.shape == (case.B,) and np.isfinite(v).all()
    assert np.abs(S.case_value(case, smooth=S.smooth_direct2d) - v).max() <= 1e-12
    h = case.T // 2

    def smooth_scipy(a, g):
        a = uniform_filter(np.asarray(a, np.float64), size=(1,) * (a.ndim - 2) + (case.T, case.T))      # its default mode is 'reflect', as scikit-image calls it
        return a[..., h:a.shape[-2] - h, h:a.shape[-1] - h]
    assert np.abs(S.case_value(case, smooth=smooth_scipy) - v).max() <= 1e-12


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_gaussian_population_unsigned_is_the_existing_ssim(case):
    """the 11 Gaussian weights, cov_norm 1.0 and the [0, 1] range: the same operations in the same order as image_metrics_cases.metrics -- the same bits"""
    recon, orig = M.make(case)
    want, _ = M.case_metrics(case)
    got = S.ssim(recon, orig, M.window(), 1.0, False, case.recon_bf16, case.signed, case.quantize)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_identical_images_are_exact():
    seen = 0
    for case in S.CASES:
        if case.content == "identical":
            assert (S.case_value(case) == 1.0).all(), case.name
            seen += 1
    assert seen >= 20 and {c.signed_range for c in S.CASES if c.content == "identical"} == {True, False}


def _visible(mut, case):
    if mut == "taps_11":
        return case.T != 11 and min(case.H, case.W) >= 11
    if mut == "gaussian_window":
        return True
    if mut == "range_1_constants_on_signed":
        return case.signed_range
    if mut == "range_2_constants_on_unsigned":
        return not case.signed_range
    return True


@pytest.mark.parametrize("mut", [m for m in S.MUTS if m != "fp32"])
def test_every_textured_case_that_can_see_a_planted_mistake_sees_it(mut):
    """each mistake moves the SSIM of every image of every textured case that can see it by >= 1000 x the GPU gate"""
    seen = 0
    for case in S.CASES:
        if case.content not in TEXTURED or not _visible(mut, case):
            continue
        d = np.abs(S.case_value(case, mut=mut) - S.case_value(case))
        assert d.min() >= 1000 * S.GPU_GATE, f"{case.name}: {mut} moves the SSIM by only {d.min():.2e}"
        seen += 1
    assert seen >= {"taps_11": 15, "range_1_constants_on_signed": 15, "range_2_constants_on_unsigned": 15}.get(mut, 60), seen


def test_near_flat_cases_see_fp32_accumulation():
    """sigma^2 = E[x^2] - mu^2 cancels eight digits where the mean is 0.5: on the [0, 1] range.  On the signed range the same image is 2e-4 * noise around
    zero, nothing cancels and fp32 is as good as fp64 there -- those cases cannot see the mistake"""
    seen = 0
    for case in S.CASES:
        if case.content != "nearflat" or case.signed_range:
            continue
        d = np.abs(S.case_value(case, mut="fp32") - S.case_value(case))
        assert d.min() >= 1000 * S.GPU_GATE, f"{case.name}: fp32 accumulation moves the SSIM by only {d.min():.2e}"
        seen += 1
    assert seen >= 10 and {c.T for c in S.CASES if c.content == "nearflat" and not c.signed_range} == {3, 7, 11}


def test_ext_header_declares_the_ssim_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and names == set(_lib.EXT_SIGNATURES)
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p, "double": C.c_double}
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


def test_image_ssim_compiles_for_gfx950_within_its_budget(tmp_path):
    """five window sizes and the finish kernel, 0 scratch, the LDS of a (16 + T - 1) x (32 + T - 1) tile: at T = 11 what image_metrics.hip holds"""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "image_ssim.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(kernels) == 6 and len(scratch) == len(lds) == 6, (kernels, scratch, lds)
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    want = sorted([0] + [8 * (2 * (15 + T) * (31 + T) + 5 * (15 + T) * 32) for T in (3, 5, 7, 9, 11)])
    assert sorted(lds) == want and max(lds) == 50752, dict(zip(kernels, lds))
    src = open(os.path.join(G.CSRC, "image_ssim.hip")).read()
    assert "asm" not in src.replace("namespace", "") and "atomic" not in src.replace("No atomics", "")


class _NoPipe:
    device = torch.device("cpu")


def test_host_side_refusals_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    q = lib.selftok_img_ssim_workspace_bytes
    assert q(1, 7, 7, 7) == 3 * 8 and q(1, 22, 38, 7) == 3 * 8 and q(2, 23, 39, 7) == 2 * 3 * 4 * 8 and q(1, 18, 34, 3) == 3 * 8 and q(1, 19, 35, 3) == 3 * 4 * 8
    assert q(64, 256, 256, 11) == 64 * 3 * 16 * 8 * 8 and q(64, 256, 256, 7) == 64 * 3 * 16 * 8 * 8 and q(2730, 512, 512, 7) > 0
    for (B, H, W, T), word in (((1, 6, 7, 7), "H, W >= taps"), ((1, 7, 6, 7), "H, W >= taps"), ((0, 7, 7, 7), "B >= 1"), ((1, 16, 16, 8), "odd"), ((1, 16, 16, 1), "odd"),
                               ((1, 16, 16, 13), "taps <= 11"), ((2731, 512, 512, 7), "2^31"), ((1, 46341, 46341, 3), "2^31")):
        assert q(B, H, W, T) == 0 and word in err(), (B, H, W, T, err())
    x = np.zeros(3 * 16 * 16, np.float32)
    out, ws, g = np.zeros(2), np.zeros(6), E.ssim_uniform_window(7)
    p = lambda a: a.ctypes.data
    call = lambda recon, orig, win, T, cn, o, w, wb, B, H, W: lib.selftok_img_ssim(recon, 0, orig, 0, 1, 0, win, T, cn, 1, o, w, wb, B, H, W, None)
    ok = (p(x), p(x), p(g), 7, 49 / 48, p(out), p(ws), 24, 1, 16, 16)
    swap = lambda i, v: ok[:i] + (v,) + ok[i + 1:]
    for args, word in ((swap(0, None), "null"), (swap(1, None), "null"), (swap(2, None), "null"), (swap(5, None), "null"), (swap(6, None), "null"),
                       (swap(7, 23), "workspace"), (swap(3, 6), "odd"), (swap(3, 13), "taps <= 11"), (swap(9, 6), "H, W >= taps"), (swap(10, 6), "H, W >= taps"),
                       (swap(4, 0.0), "cov_norm"), (swap(4, float("nan")), "cov_norm"), (swap(4, 2.5), "cov_norm"), (swap(6, p(ws) + 4), "aligned"),
                       ((p(x), p(x), p(g), 7, 1.0, p(out), p(ws), 1 << 40, 2731, 512, 512), "2^31")):
        assert call(*args) == -1 and word in err(), (word, err())
    t = torch.zeros(1, 3, 16, 16)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.image_ssim(t, t)
    with pytest.raises(ValueError, match="cov_norm"):
        ops.image_ssim(t, t, "skimage", 1.0)
    with pytest.raises(ValueError, match="cov_norm"):
        ops.image_ssim(t, t, np.full(7, 1 / 7))
    with pytest.raises(ValueError, match="preset"):
        ops.image_ssim(t, t, "box")


def test_evaluate_accepts_the_new_names_and_refuses_bad_ones():
    """the argument check runs before anything touches a device: an accepted call gets as far as the stand-in pipe's missing `encoding`"""
    t = torch.zeros(1, 3, 32, 32)
    load = lambda lo, hi: t
    with pytest.raises(AttributeError, match="encoding"):
        E.evaluate(_NoPipe(), load, 1, metrics=("psnr", "ssim_skimage"))
    with pytest.raises(AttributeError, match="encoding"):
        E.evaluate(_NoPipe(), load, 1, metrics=("ssim_skimage",), metrics_u8=True, ssim_skimage_signed=False)
    with pytest.raises(ValueError, match="ssim_sk"):
        E.evaluate(_NoPipe(), load, 1, metrics=("psnr", "ssim_sk"))
    with pytest.raises(ValueError, match="metrics_u8"):
        E.evaluate(_NoPipe(), load, 1, metrics=("psnr",), metrics_u8=True)
    d = E.ssim_skimage_definition(True, False)
    assert (d["window"], d["weights"], d["covariance"], d["data_range"], d["range"], d["on"], d["precision"]) == (7, "uniform", "sample", 2.0, "[-1, 1]", "float", "float64")
    d = E.ssim_skimage_definition(False, True)
    assert (d["data_range"], d["range"], d["on"]) == (1.0, "[0, 1]", "u8")
