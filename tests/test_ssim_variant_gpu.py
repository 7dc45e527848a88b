"""-m gpu: selftok_img_ssim (csrc/image_ssim.hip, ops.image_ssim) against the numpy emulation of tests/ssim_variant_cases.py on every case of its
table, the Gaussian / population / [0, 1] preset against column 0 of selftok_img_metrics BIT FOR BIT (the arithmetic order is shared), bit for bit
against itself (run to run, alone against inside a batch, any order, next to a NaN image), inside NaN-filled guard bands, replayed from a hipGraph,
and its refusals.

The gate is the existing entry's, by the same derivation: fp64 rounding 1.1e-16 x at most 121-term sums x at most
4 / C2 = 1.1e3 amplification (C2 relative to R^2 is the same number on both ranges) = 1.5e-11, with a few-fold margin -> 1e-10."""
import numpy as np
import pytest
import torch

import image_metrics_cases as M
import ssim_variant_cases as S
from selftoktokenizer_amd import _lib, evaluate as E, ops

pytestmark = pytest.mark.gpu
GATE = S.GPU_GATE


def dev(a, bf16):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(case, recon=None, orig=None):
    if recon is None:
        recon, orig = S.make(case)
    return ops.image_ssim(dev(recon, case.recon_bf16), dev(orig, case.orig_bf16), S.uniform_window(case.T), S.sample_cov_norm(case.T), case.signed_range,
                          original_signed=case.orig_signed, quantize=case.quantize).cpu().numpy()


@pytest.mark.parametrize("case", S.CASES, ids=lambda c: c.name)
def test_device_equals_the_emulation(case):
    got = run(case)
    want = S.case_value(case)
    d = np.abs(got - want).max()
    print(f"\n{case.name}: |dSSIM| {d:.2e} (gate {GATE:.0e})")
    assert got.shape == (case.B,) and got.dtype == np.float64 and d <= GATE
    if case.content == "identical":
        assert (got == 1.0).all()                                          # exactly: numerator and denominator are the same bits


def test_the_skimage_preset_is_t7_uniform_with_the_sample_covariance():
    for case in [c for c in S.CASES if c.T == 7 and (c.H, c.W) == (64, 48)]:
        recon, orig = S.make(case)
        got = ops.image_ssim(dev(recon, case.recon_bf16), dev(orig, case.orig_bf16), "skimage", None, case.signed_range, case.orig_signed, case.quantize).cpu().numpy()
        assert np.array_equal(bits(got), bits(run(case, recon, orig))), case.name
        assert np.abs(got - S.case_value(case)).max() <= GATE


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_gaussian_population_unsigned_is_column_0_of_image_metrics_bit_for_bit(case):
    recon, orig = M.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    old = ops.image_metrics(x, y, original_signed=case.signed, quantize=case.quantize).cpu().numpy()[:, 0]
    new = ops.image_ssim(x, y, E.ssim_window(), 1.0, False, original_signed=case.signed, quantize=case.quantize).cpu().numpy()
    preset = ops.image_ssim(x, y, "gaussian", None, False, original_signed=case.signed, quantize=case.quantize).cpu().numpy()
    assert np.array_equal(bits(new), bits(old)) and np.array_equal(bits(preset), bits(old))
    assert np.abs(new - M.case_metrics(case)[0]).max() <= GATE


BATCH5 = S.Case("t7_75x42_b5", 7, 75, 42, 5, "noise", False, False, True, True, False)


@pytest.mark.parametrize("quantize", [False, True], ids=["float", "u8"])
@pytest.mark.parametrize("signed_range", [True, False], ids=["R2", "R1"])
def test_bit_for_bit_run_to_run_alone_against_batch_and_any_order(quantize, signed_range):
    case = BATCH5._replace(quantize=quantize, recon_bf16=quantize, signed_range=signed_range)
    recon, orig = S.make(case)
    a, b = run(case, recon, orig), run(case, recon, orig)
    assert np.array_equal(bits(a), bits(b)) and np.abs(a - S.ssim(recon, orig, S.uniform_window(7), S.sample_cov_norm(7), signed_range, quantize, True, quantize)).max() <= GATE
    for i in range(case.B):
        alone = run(case, recon[i:i + 1], orig[i:i + 1])
        assert np.array_equal(bits(alone[0]), bits(a[i])), f"image {i} alone differs from the same image inside B = {case.B}"
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(bits(run(case, recon[perm], orig[perm])), bits(a[perm]))


def test_a_nan_image_poisons_only_its_own_value():
    recon, orig = S.make(BATCH5)
    clean = run(BATCH5, recon, orig)
    for where in ((2, 1, 40, 17), (4, 2, 74, 41), (0, 0, 0, 0)):
        bad = recon.copy()
        bad[where] = np.nan
        got = run(BATCH5, bad, orig)
        keep = [i for i in range(BATCH5.B) if i != where[0]]
        assert np.isnan(got[where[0]]) and np.array_equal(bits(got[keep]), bits(clean[keep])), where
    bad = orig.copy()
    bad[1] = np.nan
    got = run(BATCH5, recon, bad)
    assert np.isnan(got[1]) and np.array_equal(bits(got[[0, 2, 3, 4]]), bits(clean[[0, 2, 3, 4]]))


@pytest.mark.parametrize("T", S.TAPS)
def test_inputs_inside_nan_guard_bands(T):
    """both tensors are views inside larger NaN-filled allocations: a halo read that strays past a tensor turns an output into NaN"""
    th, tw = 16 + T - 1, 32 + T - 1
    seen = 0
    for case in [c for c in S.CASES if c.T == T and (c.H, c.W) in ((T, T), (th + 1, tw + 1), (64, 48), (256, 256)) and c.content in ("noise", "recon_noise")]:
        recon, orig = S.make(case)
        views = []
        for a, bf in ((recon, case.recon_bf16), (orig, case.orig_bf16)):
            t = dev(a, bf)
            guard = 2 * 11 * case.W + 64
            buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=t.dtype, device="cuda")
            buf[guard:guard + t.numel()] = t.reshape(-1)
            views.append(buf[guard:guard + t.numel()].view(t.shape))
        got = ops.image_ssim(views[0], views[1], S.uniform_window(T), S.sample_cov_norm(T), case.signed_range, case.orig_signed, case.quantize).cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(bits(got), bits(run(case, recon, orig))), case.name
        seen += 1
    assert seen >= 6


def test_hipgraph_replay_equals_eager():
    case = next(c for c in S.CASES if c.T == 7 and (c.H, c.W) == (64, 48) and c.content == "recon_noise")
    recon, orig = S.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    call = lambda: ops.image_ssim(x, y, "skimage", None, case.signed_range, case.orig_signed, case.quantize)
    eager = call().cpu().numpy()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(eager))
    recon2, orig2 = S.make(case, seed=1)
    x.copy_(dev(recon2, case.recon_bf16)); y.copy_(dev(orig2, case.orig_bf16))
    g.replay()
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert np.array_equal(bits(again), bits(call().cpu().numpy())) and not np.array_equal(bits(again), bits(eager))


def test_refusals():
    f = torch.zeros(2, 3, 16, 16, device="cuda")
    for recon, orig in ((f.double(), f), (f, f.half()), (f, f[:1]), (f[0], f[0]), (f[:, :2], f[:, :2]), (f[..., :6], f[..., :6]), (f[..., :6, :], f[..., :6, :]),
                        (f.cpu(), f), (f, f.cpu())):
        with pytest.raises(_lib.SelftokHipError):
            ops.image_ssim(recon, orig)
    for win, cn in ((np.full(8, 1 / 8), 1.0), (np.full(13, 1 / 13), 1.0), (np.ones(1), 1.0), (np.full(7, 1 / 7), 0.0), (np.full(7, 1 / 7), float("nan"))):
        with pytest.raises(_lib.SelftokHipError):
            ops.image_ssim(f, f, win, cn)
    lib = _lib.load()
    need = lib.selftok_img_ssim_workspace_bytes(2, 16, 16, 7)
    assert need == 2 * 3 * 8
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, dtype=torch.float64, device="cuda")
    g = E.ssim_uniform_window(7)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda wb: lib.selftok_img_ssim(f.data_ptr(), 0, f.data_ptr(), 0, 0, 0, g.ctypes.data, 7, 49 / 48, 0, out.data_ptr(), ws.data_ptr(), wb, 2, 16, 16, st)
    assert call(need - 1) == -1 and "workspace" in lib.selftok_last_error().decode()
    assert call(need) == 0                                                              # the exact size is enough
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 1.0).all()                                             # zeros against zeros
