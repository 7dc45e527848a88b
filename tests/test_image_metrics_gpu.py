"""-m gpu: the device image metrics (csrc/image_metrics.hip, ops.image_metrics, evaluate(metrics=...)) against the numpy emulation of
tests/image_metrics_cases.py, bit for bit against themselves (run to run, alone against inside a batch, next to a NaN image), inside
NaN-filled guard bands, through the evaluation harness, replayed from a hipGraph, and their refusals.

The SSIM gate is derived, not measured: fp64 rounding 1.1e-16 x 121-term sums x at most 1 / C2 = 1.1e3 amplification = 1.5e-11, with a
few-fold margin -> 1e-10.  A device value outside it means an fp32 step or a contraction, not noise."""
import numpy as np
import pytest
import torch

import image_metrics_cases as M
from selftoktokenizer_amd import _lib, evaluate as E, ops, synth

pytestmark = pytest.mark.gpu
SSIM_GATE, MSE_GATE = 1e-10, 1e-12

_ref = {}


def emulated(case):
    if case.name not in _ref:
        _ref[case.name] = M.case_metrics(case)
    return _ref[case.name]


def dev(a, bf16):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def run(case, recon=None, orig=None):
    if recon is None:
        recon, orig = M.make(case)
    return ops.image_metrics(dev(recon, case.recon_bf16), dev(orig, case.orig_bf16), original_signed=case.signed, quantize=case.quantize).cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.name)
def test_device_equals_the_emulation(case):
    got = run(case)
    ssim, mse = emulated(case)
    ds, dm = np.abs(got[:, 0] - ssim).max(), (np.abs(got[:, 1] - mse) / np.maximum(mse, 1e-12)).max()
    print(f"\n{case.name}: |dSSIM| {ds:.2e} (gate {SSIM_GATE:.0e}), |dMSE| / max(MSE, 1e-12) {dm:.2e} (gate {MSE_GATE:.0e})")
    assert got.shape == (case.B, 2) and got.dtype == np.float64
    assert ds <= SSIM_GATE and dm <= MSE_GATE
    if case.content == "identical":
        assert (got[:, 0] == 1.0).all() and (got[:, 1] == 0.0).all()       # exactly: numerator and denominator are the same bits
    if case.quantize:
        assert np.array_equal(bits(got[:, 1]), bits(mse))                  # an exact integer sum, one division


BATCH5 = M.Case("75x42_b5", 75, 42, 5, "noise", False, False, True, False)


@pytest.mark.parametrize("quantize", [False, True], ids=["float", "u8"])
def test_bit_for_bit_run_to_run_and_alone_against_batch(quantize):
    case = BATCH5._replace(quantize=quantize, recon_bf16=quantize)
    recon, orig = M.make(case)
    a, b = run(case, recon, orig), run(case, recon, orig)
    assert np.array_equal(bits(a), bits(b))
    for i in range(case.B):
        alone = run(case, recon[i:i + 1], orig[i:i + 1])
        assert np.array_equal(bits(alone[0]), bits(a[i])), f"image {i} alone differs from the same image inside B = {case.B}"
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(bits(run(case, recon[perm], orig[perm])), bits(a[perm]))


def test_a_nan_image_poisons_only_its_own_outputs():
    recon, orig = M.make(BATCH5)
    clean = run(BATCH5, recon, orig)
    for where in ((2, 1, 40, 17), (4, 2, 74, 41), (0, 0, 0, 0)):
        bad = recon.copy()
        bad[where] = np.nan
        got = run(BATCH5, bad, orig)
        b = where[0]
        assert np.isnan(got[b]).all(), where
        keep = [i for i in range(BATCH5.B) if i != b]
        assert np.array_equal(bits(got[keep]), bits(clean[keep])), where
    bad = orig.copy()
    bad[1] = np.nan
    got = run(BATCH5, recon, bad)
    assert np.isnan(got[1]).all() and np.array_equal(bits(got[[0, 2, 3, 4]]), bits(clean[[0, 2, 3, 4]]))


@pytest.mark.parametrize("name", ["11x11", "27x43", "75x42", "256x256"])
def test_inputs_inside_nan_guard_bands(name):
    """the tensors are views inside larger NaN-filled allocations: a halo read that strays past a tensor turns an output into NaN instead of
    provoking anything"""
    for case in [c for c in M.CASES if c.name.startswith(name + "_") and c.content in ("noise", "recon_noise")]:
        recon, orig = M.make(case)
        views = []
        for a, bf in ((recon, case.recon_bf16), (orig, case.orig_bf16)):
            t = dev(a, bf)
            guard = 2 * 11 * case.W + 64
            buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=t.dtype, device="cuda")
            buf[guard:guard + t.numel()] = t.reshape(-1)
            views.append(buf[guard:guard + t.numel()].view(t.shape))
            assert views[-1].is_contiguous() and views[-1].data_ptr() == buf.data_ptr() + guard * t.element_size()
        got = ops.image_metrics(views[0], views[1], original_signed=case.signed, quantize=case.quantize).cpu().numpy()
        assert np.isfinite(got).all(), case.name
        assert np.array_equal(bits(got), bits(run(case, recon, orig))), case.name


def test_the_entry_uses_the_window_it_is_given():
    """a box window through the raw entry gives the box-window SSIM: the weights are the caller's, the kernel has none of its own"""
    case = M.BY_NAME[next(c.name for c in M.CASES if c.name.startswith("27x43_") and c.content == "noise")]
    recon, orig = M.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    lib = _lib.load()
    n = lib.selftok_img_metrics_workspace_bytes(case.B, case.H, case.W)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = torch.empty(case.B, 2, dtype=torch.float64, device="cuda")
    box = np.full(11, 1.0 / 11)
    _lib.check(lib.selftok_img_metrics(x.data_ptr(), int(case.recon_bf16), y.data_ptr(), int(case.orig_bf16), int(case.signed), int(case.quantize), box.ctypes.data,
                                       out.data_ptr(), ws.data_ptr(), n, case.B, case.H, case.W, torch.cuda.current_stream().cuda_stream), "selftok_img_metrics")
    want, mse = M.case_metrics(case, mut=M.MUT_BOX)
    got = out.cpu().numpy()
    assert np.abs(got[:, 0] - want).max() <= SSIM_GATE and np.abs(want - emulated(case)[0]).min() > 1e-5
    assert (np.abs(got[:, 1] - mse) / np.maximum(mse, 1e-12)).max() <= MSE_GATE


class _PoolingPipe:
    """a stand-in tokenizer for the HARNESS tests (evaluate only needs .device, .encoding, .decoding*): 8 x 8 mean pooling to 16 levels and
    nearest-neighbour decoding, every image on its own, so a batch's composition cannot change a value"""
    device = torch.device("cuda")

    def encoding(self, imgs, device=None):
        p = torch.nn.functional.avg_pool2d(imgs.float(), 8)
        self.shape = tuple(p.shape[1:])
        return p.mul(7.5).add(7.5).round().clamp(0, 15).to(torch.int64).flatten(1)

    def decoding(self, ids, device=None, noise=None):
        t = torch.from_numpy(np.asarray(ids)).to(self.device).float().view(-1, *self.shape) / 15.0
        return torch.nn.functional.interpolate(t, scale_factor=8, mode="nearest").to(torch.bfloat16)

    def decoding_with_renderer(self, ids, device=None):
        return self.decoding(ids).float() * 0.75 + 0.125


def _smooth_images(lo, hi):
    """synthetic 128 x 128 images with structure at the scale of the window (the hash images of synth, pooled and scaled back up), in [-1, 1]"""
    a = torch.nn.functional.avg_pool2d(synth.synthetic_images(hi - lo, size=256, first_index=lo), 8)
    return torch.nn.functional.interpolate(a, scale_factor=4, mode="bilinear").mul(3.0).clamp(-1, 1)


def test_harness_metrics_option():
    pipe = _PoolingPipe()
    dec = ("diffusion", "renderer")
    base = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec)
    same = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec, metrics=("psnr",))
    assert same == base and list(base) == ["images", "ranks", "batch", "shard", "diffusion", "renderer", "token_ids_first_image"]
    assert list(base["diffusion"]) == ["psnr_mean_dB", "psnr_each_dB"]
    imgs = _smooth_images(0, 3).cuda()
    ids = pipe.encoding(imgs).cpu().numpy()
    today = E.psnr_each(pipe.decoding(ids), imgs)                           # the host route's own values
    assert base["diffusion"]["psnr_each_dB"] == [round(float(v), 6) for v in today] and base["diffusion"]["psnr_mean_dB"] == float(today.mean())

    both = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec, metrics=("psnr", "ssim"))
    assert both["metric_definition"] == {"window": 11, "sigma": 1.5, "K1": 0.01, "K2": 0.03, "data_range": 1.0, "covariance": "population", "region": "valid", "on": "float"}
    for d, rec in (("diffusion", pipe.decoding(ids)), ("renderer", pipe.decoding_with_renderer(ids))):
        assert list(both[d]) == ["psnr_mean_dB", "psnr_each_dB", "ssim_mean", "ssim_each"]
        ssim, psnr = E.metrics_each(rec, imgs)
        host = E.psnr_each(rec, imgs)
        print(f"\n{d}: PSNR device {psnr} host {host} |d| {np.abs(psnr - host).max():.2e} dB; SSIM {ssim}")
        assert np.abs(psnr - host).max() <= 1e-9                            # the same fp32 squares, only the fp64 summation order differs
        assert abs(both[d]["psnr_mean_dB"] - base[d]["psnr_mean_dB"]) <= 1e-9
        assert np.abs(np.array(both[d]["psnr_each_dB"]) - np.array(base[d]["psnr_each_dB"])).max() <= 1e-6 + 1e-9     # both lists are rounded to 1e-6
        assert both[d]["ssim_each"] == [round(float(v), 9) for v in ssim] and both[d]["ssim_mean"] == float(ssim.mean())
        want, _ = M.metrics(rec.float().cpu().numpy(), imgs.cpu().numpy(), rec.dtype == torch.bfloat16, True, False)
        assert np.abs(ssim - want).max() <= SSIM_GATE and 0.0 < ssim.min() and ssim.max() < 1.0
    ragged = E.evaluate(pipe, _smooth_images, 3, batch=2, decoders=dec, metrics=("psnr", "ssim"))
    assert ragged["batch"] == 2 and {k: v for k, v in ragged.items() if k != "batch"} == {k: v for k, v in both.items() if k != "batch"}

    u8 = E.evaluate(pipe, _smooth_images, 3, batch=3, metrics=("ssim",), metrics_u8=True)
    assert u8["metric_definition"]["on"] == "u8"
    want_s, want_m = M.metrics(pipe.decoding(ids).float().cpu().numpy(), imgs.cpu().numpy(), True, True, True)
    assert np.abs(np.array(u8["diffusion"]["ssim_each"]) - want_s).max() <= SSIM_GATE + 1e-9
    assert np.abs(np.array(u8["diffusion"]["psnr_each_dB"]) - E.psnr_of_mse(want_m)).max() <= 1e-6
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics=("lpips",))
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics_u8=True)


def test_hipgraph_replay_equals_eager():
    case = M.BY_NAME[next(c.name for c in M.CASES if c.name.startswith("75x42_") and c.content == "recon_noise")]
    recon, orig = M.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    call = lambda: ops.image_metrics(x, y, original_signed=case.signed, quantize=case.quantize)
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
    recon2, orig2 = M.make(case, seed=1)                                     # new pixels in the captured tensors: the replay reads them
    x.copy_(dev(recon2, case.recon_bf16)); y.copy_(dev(orig2, case.orig_bf16))
    g.replay()
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert np.array_equal(bits(again), bits(call().cpu().numpy())) and not np.array_equal(bits(again), bits(eager))


def test_refusals():
    f = torch.zeros(2, 3, 16, 16, device="cuda")
    for recon, orig in ((f.double(), f), (f, f.half()), (f, f[:1]), (f[0], f[0]), (f[:, :2], f[:, :2]), (f[..., :10], f[..., :10]), (f[..., :10, :], f[..., :10, :]),
                        (f.cpu(), f), (f, f.cpu())):
        with pytest.raises(_lib.SelftokHipError):
            ops.image_metrics(recon, orig)
    lib = _lib.load()
    ws = torch.empty(1024, dtype=torch.uint8, device="cuda")
    out = torch.empty(2, 2, dtype=torch.float64, device="cuda")
    g = E.ssim_window()
    st = torch.cuda.current_stream().cuda_stream
    call = lambda recon, orig, win, o, w, wb, B, H, W: lib.selftok_img_metrics(recon, 0, orig, 0, 1, 0, win, o, w, wb, B, H, W, st)
    p, gp = f.data_ptr(), g.ctypes.data
    need = lib.selftok_img_metrics_workspace_bytes(2, 16, 16)
    assert need == 2 * 3 * 16
    for args, word in (((None, p, gp, out.data_ptr(), ws.data_ptr(), 1024, 2, 16, 16), "null"), ((p, p, None, out.data_ptr(), ws.data_ptr(), 1024, 2, 16, 16), "null"),
                       ((p, p, gp, None, ws.data_ptr(), 1024, 2, 16, 16), "null"), ((p, p, gp, out.data_ptr(), None, 1024, 2, 16, 16), "null"),
                       ((p, p, gp, out.data_ptr(), ws.data_ptr(), need - 1, 2, 16, 16), "workspace"), ((p, p, gp, out.data_ptr(), ws.data_ptr(), 1024, 2, 10, 16), "H, W >= 11"),
                       ((p, p, gp, out.data_ptr(), ws.data_ptr(), 1024, 0, 16, 16), "B >= 1"), ((p, p, gp, out.data_ptr(), ws.data_ptr(), 1 << 40, 2731, 512, 512), "2^31")):
        assert call(*args) == -1, word
        assert word in lib.selftok_last_error().decode(), (word, lib.selftok_last_error().decode())
    assert call(p, p, gp, out.data_ptr(), ws.data_ptr(), need, 2, 16, 16) == 0         # the exact size is enough
    torch.cuda.synchronize()
    assert (out.cpu().numpy()[:, 1] == 0.25).all()                                      # zeros against a [-1, 1] zero = 0.5
