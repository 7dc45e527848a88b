"""-m gpu: both readings of the SSIM and LPIPS columns through the evaluation harness -- evaluate(metrics=("psnr", "ssim", "ssim_skimage", "lpips"),
lpips=[alex, vgg]) on a stand-in tokenizer with a ragged last batch: the new keys equal the direct calls, every existing key is what a run without
the new metrics gives, metrics_u8 is honoured -- and tools/eval_psnr.py --synthetic --ssim-skimage --lpips-vgg in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lpips_vgg_cases as V
import ssim_variant_cases as S
from selftoktokenizer_amd import evaluate as E, lpips as LP, ops, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _PoolingPipe:
    """a stand-in tokenizer (evaluate only needs .device, .encoding, .decoding*): 8 x 8 mean pooling to 16 levels and nearest-neighbour decoding, every image on
    its own, so a batch's composition cannot change a value"""
    device = torch.device("cuda")

    def encoding(self, imgs, device=None):
        p = F.avg_pool2d(imgs.float(), 8)
        self.shape = tuple(p.shape[1:])
        return p.mul(7.5).add(7.5).round().clamp(0, 15).to(torch.int64).flatten(1)

    def decoding(self, ids, device=None, noise=None):
        t = torch.from_numpy(np.asarray(ids)).to(self.device).float().view(-1, *self.shape) / 15.0
        return F.interpolate(t, scale_factor=8, mode="nearest").to(torch.bfloat16)

    def decoding_with_renderer(self, ids, device=None):
        return self.decoding(ids).float() * 0.75 + 0.125


def _smooth_images(lo, hi):
    a = F.avg_pool2d(synth.synthetic_images(hi - lo, size=128, first_index=lo), 8)
    return F.interpolate(a, scale_factor=4, mode="bilinear").mul(3.0).clamp(-1, 1)                   # 64 x 64


def _each(v):
    return [round(float(x), 9) for x in v]


def test_harness_reports_both_readings_of_both_columns():
    alex, vgg = LP.LpipsNet.synthetic("cuda"), LP.LpipsNet.synthetic("cuda", net="vgg")
    pipe = _PoolingPipe()
    dec = ("diffusion", "renderer")
    old = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec, metrics=("psnr", "ssim", "lpips"), lpips=alex)
    full = E.evaluate(pipe, _smooth_images, 3, batch=2, decoders=dec, metrics=("psnr", "ssim", "ssim_skimage", "lpips"), lpips=[alex, vgg])      # 2 + 1 images
    assert list(full) == list(old)
    new_keys = ["ssim_skimage_mean", "ssim_skimage_each", "lpips_alex_mean", "lpips_alex_each", "lpips_vgg_mean", "lpips_vgg_each"]
    assert list(full["diffusion"]) == ["psnr_mean_dB", "psnr_each_dB", "ssim_mean", "ssim_each"] + new_keys
    md = full["metric_definition"]
    assert md["lpips_alex"] == dict(LP.LPIPS_DEFINITION, weights="synthetic") == old["metric_definition"]["lpips"] and md["lpips_vgg"] == dict(LP.LPIPS_VGG_DEFINITION, weights="synthetic")
    assert md["ssim_skimage"] == E.ssim_skimage_definition(True, False) and "lpips" not in md
    assert {k: v for k, v in md.items() if k not in ("ssim_skimage", "lpips_alex", "lpips_vgg")} == {k: v for k, v in old["metric_definition"].items() if k != "lpips"}
    imgs = _smooth_images(0, 3).cuda()
    ids = pipe.encoding(imgs).cpu().numpy()
    for d, rec in (("diffusion", pipe.decoding(ids)), ("renderer", pipe.decoding_with_renderer(ids))):
        for k in ("psnr_mean_dB", "psnr_each_dB", "ssim_mean", "ssim_each"):                       # every existing key: what the run without the new metrics gives
            assert full[d][k] == old[d][k], (d, k)
        assert full[d]["lpips_alex_each"] == old[d]["lpips_each"] and full[d]["lpips_alex_mean"] == old[d]["lpips_mean"]
        sk = ops.image_ssim(rec, imgs, "skimage", None, True).cpu().numpy()
        lv = vgg(rec, imgs).cpu().numpy()
        assert full[d]["ssim_skimage_each"] == _each(sk) and full[d]["ssim_skimage_mean"] == float(sk.mean())
        assert full[d]["lpips_vgg_each"] == _each(lv) and full[d]["lpips_vgg_mean"] == float(lv.mean()) and lv.min() > 0
        want = S.ssim(rec.float().cpu().numpy(), imgs.cpu().numpy(), S.uniform_window(7), S.sample_cov_norm(7), True, rec.dtype == torch.bfloat16, True, False)
        assert np.abs(sk - want).max() <= S.GPU_GATE and -1.0 < sk.min() and sk.max() < 1.0
        want = V.emulate(rec.float().cpu().numpy(), imgs.cpu().numpy(), rec.dtype == torch.bfloat16, True, False)
        m = want >= V.D_GATED
        assert (np.abs(lv[m] - want[m]) <= 4.0 * V.fp32_relative_error() * want[m]).all(), (lv, want)
    # one network on its own keeps the `lpips_*` keys, whichever backbone it is; the definition names it
    only = E.evaluate(pipe, _smooth_images, 3, batch=3, metrics=("lpips",), lpips=vgg)
    assert only["diffusion"]["lpips_each"] == full["diffusion"]["lpips_vgg_each"] and only["metric_definition"]["lpips"]["net"] == "vgg"
    seq1 = E.evaluate(pipe, _smooth_images, 3, batch=3, metrics=("lpips",), lpips=[vgg])
    assert seq1["diffusion"]["lpips_vgg_each"] == full["diffusion"]["lpips_vgg_each"] and "lpips_each" not in seq1["diffusion"]
    # the [0, 1] reading and the bytes
    unsigned = E.evaluate(pipe, _smooth_images, 3, batch=2, metrics=("ssim_skimage",), ssim_skimage_signed=False)
    assert unsigned["metric_definition"]["ssim_skimage"] == E.ssim_skimage_definition(False, False)
    sk = ops.image_ssim(pipe.decoding(ids), imgs, "skimage", None, False).cpu().numpy()
    assert unsigned["diffusion"]["ssim_skimage_each"] == _each(sk) != full["diffusion"]["ssim_skimage_each"]
    u8 = E.evaluate(pipe, _smooth_images, 3, batch=2, metrics=("ssim", "ssim_skimage", "lpips"), metrics_u8=True, lpips=[alex, vgg])
    assert u8["metric_definition"]["on"] == "u8" and u8["metric_definition"]["ssim_skimage"]["on"] == "u8"
    rec = pipe.decoding(ids)
    sk, lv = ops.image_ssim(rec, imgs, "skimage", None, True, True, True).cpu().numpy(), vgg(rec, imgs, quantize=True).cpu().numpy()
    assert u8["diffusion"]["ssim_skimage_each"] == _each(sk) != full["diffusion"]["ssim_skimage_each"]
    assert u8["diffusion"]["lpips_vgg_each"] == _each(lv) != full["diffusion"]["lpips_vgg_each"]
    assert u8["diffusion"]["lpips_alex_each"] == _each(alex(rec, imgs, quantize=True).cpu().numpy())
    want = S.ssim(rec.float().cpu().numpy(), imgs.cpu().numpy(), S.uniform_window(7), S.sample_cov_norm(7), True, True, True, True)
    assert np.abs(sk - want).max() <= S.GPU_GATE
    # the default route is untouched
    base = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec)
    assert list(base) == ["images", "ranks", "batch", "shard", "diffusion", "renderer", "token_ids_first_image"] and list(base["diffusion"]) == ["psnr_mean_dB", "psnr_each_dB"]
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics=("psnr", "ssim_skimage2"))
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics=("lpips",), lpips=[alex, alex])


def test_eval_tool_prints_both_readings_in_one_run(tmp_path):
    tool = os.path.join(ROOT, "tools", "eval_psnr.py")
    out = tmp_path / "eval.json"
    r = subprocess.run([sys.executable, tool, "--synthetic", "2", "--batch", "2", "--ssim", "--ssim-skimage", "--lpips", "--lpips-vgg", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(out.read_text())
    d = line["diffusion"]
    for key in ("psnr_each_dB", "ssim_each", "ssim_skimage_each", "lpips_alex_each", "lpips_vgg_each"):
        assert len(d[key]) == 2 and all(np.isfinite(v) for v in d[key]), key
    assert d["ssim_each"] != d["ssim_skimage_each"] and d["lpips_alex_each"] != d["lpips_vgg_each"]
    assert line["metric_definition"]["ssim_skimage"]["data_range"] == 2.0 and line["metric_definition"]["lpips_vgg"]["net"] == "vgg"
    assert line["lpips_weights"] == "synthetic" and line["lpips_vgg_weights"] == "synthetic"
    assert json.loads(r.stdout.strip().splitlines()[-1]) == line
    r = subprocess.run([sys.executable, tool, "--synthetic", "2", "--lpips-vgg", "only_one.pth"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--lpips-vgg" in r.stderr
