"""What the reconstruction metrics of the evaluation harness cost on MI355X, B = 64 and B = 256 images of 256 x 256:

  (a) the device route: `ops.image_metrics` (SSIM + MSE in one call) timed by HIP events, and `evaluate.metrics_each` (the same call plus the
      read of its [B, 2] result) by the host clock around a synchronise;
  (b) the fp64 numpy emulation of the same arithmetic (tests/image_metrics_cases.py) on a 16-thread pool, images split over the threads;
  (c) today's host PSNR route `evaluate.psnr_each`, device-to-host copy of both tensors included (PSNR only: it has no SSIM);
  (d) one `evaluate()` batch of the one-step renderer (encoding + decoding_with_renderer, synthetic weights) and the share of a batch each
      metrics route would take next to it.

Same process for every variant, 3 warm-up runs + `--reps` repetitions (the emulation: 1 + 3), median and min..max.  Nothing is asserted about
speed; the device values are checked against the emulation before anything is timed.  Prints a text report and one JSON line.

    python tools/bench_image_metrics.py [--reps 15] [--no-pipeline] [--out profiles/image_metrics.txt]

--variant skimage: the same protocol for `ops.image_ssim` (csrc/image_ssim.hip) -- the "skimage" preset (uniform 7 x 7, sample covariance) on both ranges
and on the bytes, the uniform and the Gaussian 11-tap window -- next to `ops.image_metrics` on the same buffers, A / B alternating inside one loop; the values
are checked against the emulation of tests/ssim_variant_cases.py first, and the Gaussian reading against column 0 of image_metrics bit for bit.  One JSON object.

    python tools/bench_image_metrics.py --variant skimage [--reps 15] [--batches 64] [--out profiles/ssim_variants.json]"""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import image_metrics_cases as M
from selftoktokenizer_amd import evaluate as E, ops, synth, weights as W
from selftoktokenizer_amd.config import default_config

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--batches", default="64,256")
ap.add_argument("--no-pipeline", action="store_true")
ap.add_argument("--variant", default="gaussian", choices=["gaussian", "skimage"], help="skimage: time ops.image_ssim's readings next to ops.image_metrics instead")
ap.add_argument("--out", default=None, help="also write the report to this file")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
S, THREADS = 256, 16
pool = ThreadPoolExecutor(max_workers=THREADS)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": round(float(np.median(v)) * 1e3, 4), "min_ms": round(float(v.min()) * 1e3, 4), "max_ms": round(float(v.max()) * 1e3, 4), "n": len(v)}


def host_timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def event_timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e-3)
    return out


def emulation(recon, orig):
    """the numpy emulation, one slice of the batch per thread"""
    parts = [p for p in np.array_split(np.arange(recon.shape[0]), THREADS) if len(p)]
    res = list(pool.map(lambda p: M.metrics(recon[p], orig[p], True, True, False), parts))
    return np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])


def ssim_variants():
    import ssim_variant_cases as SV
    res = {"tool": "bench_image_metrics --variant skimage", "size": S, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "protocol": "one process, warm, 3 warm-up runs + reps repetitions, HIP events around one call, A / B alternating; median [min..max]"}
    for B in [int(b) for b in a.batches.split(",")]:
        orig = synth.synthetic_images(B, size=S).to(dev)
        recon = ((orig + 1) / 2 + 0.1 * (synth.synthetic_images(B, size=S, first_index=B).to(dev))).clamp_(0, 1).to(torch.bfloat16)
        recon_h, orig_h = recon.float().cpu().numpy(), orig.cpu().numpy()
        calls = {"image_metrics_ssim_and_mse": lambda: ops.image_metrics(recon, orig),
                 "ssim_t7_uniform_sample_signed": lambda: ops.image_ssim(recon, orig, "skimage", None, True),
                 "ssim_t7_uniform_sample_unsigned": lambda: ops.image_ssim(recon, orig, "skimage", None, False),
                 "ssim_t7_uniform_sample_signed_u8": lambda: ops.image_ssim(recon, orig, "skimage", None, True, True, True),
                 "ssim_t11_uniform_sample_signed": lambda: ops.image_ssim(recon, orig, SV.uniform_window(11), SV.sample_cov_norm(11), True),
                 "ssim_t11_gaussian_population_unsigned": lambda: ops.image_ssim(recon, orig, "gaussian", None, False)}
        n = min(B, 8)                                                                           # the emulation of the first images, one thread
        want = {"ssim_t7_uniform_sample_signed": SV.ssim(recon_h[:n], orig_h[:n], SV.uniform_window(7), SV.sample_cov_norm(7), True, True, True, False),
                "ssim_t7_uniform_sample_unsigned": SV.ssim(recon_h[:n], orig_h[:n], SV.uniform_window(7), SV.sample_cov_norm(7), False, True, True, False),
                "ssim_t7_uniform_sample_signed_u8": SV.ssim(recon_h[:n], orig_h[:n], SV.uniform_window(7), SV.sample_cov_norm(7), True, True, True, True),
                "ssim_t11_uniform_sample_signed": SV.ssim(recon_h[:n], orig_h[:n], SV.uniform_window(11), SV.sample_cov_norm(11), True, True, True, False)}
        r = {"checked_images": n}
        for k, w in want.items():
            got = calls[k]().cpu().numpy()
            r[k] = {"mean": float(got.mean()), "max_abs_d_vs_emulation": float(np.abs(got[:n] - w).max())}
            assert r[k]["max_abs_d_vs_emulation"] <= 1e-10, (k, r[k])
        old, new = calls["image_metrics_ssim_and_mse"]().cpu().numpy()[:, 0], calls["ssim_t11_gaussian_population_unsigned"]().cpu().numpy()
        r["ssim_t11_gaussian_population_unsigned"] = {"mean": float(new.mean()), "bit_equal_to_image_metrics_column_0": bool(np.array_equal(old.view(np.uint64), new.view(np.uint64)))}
        assert r["ssim_t11_gaussian_population_unsigned"]["bit_equal_to_image_metrics_column_0"]
        r["image_metrics_ssim_and_mse"] = {"mean": float(old.mean())}
        times = {k: [] for k in calls}
        for fn in calls.values():
            for _ in range(3):
                fn()
        for _ in range(a.reps):                                                                 # alternating
            for k, fn in calls.items():
                times[k] += event_timed(fn, 1, warm=0)
        for k in calls:
            r[k]["events"] = stats(times[k])
        r["gpixel_per_s_t7"] = round(B * 3 * S * S / (r["ssim_t7_uniform_sample_signed"]["events"]["median_ms"] * 1e-3) / 1e9, 2)
        res[f"B{B}"] = r
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if a.variant == "skimage":
    ssim_variants()
    pool.shutdown()
    sys.exit(0)

res = {"tool": "bench_image_metrics", "size": S, "reps": a.reps, "device": torch.cuda.get_device_name(0), "emulation_threads": THREADS}
for B in [int(b) for b in a.batches.split(",")]:
    orig = synth.synthetic_images(B, size=S).to(dev)                                            # fp32 in [-1, 1), as the loader hands it over
    recon = ((orig + 1) / 2 + 0.1 * (synth.synthetic_images(B, size=S, first_index=B).to(dev))).clamp_(0, 1).to(torch.bfloat16)
    recon_h, orig_h = recon.float().cpu().numpy(), orig.cpu().numpy()
    got = ops.image_metrics(recon, orig).cpu().numpy()
    want_s, want_m = emulation(recon_h, orig_h)
    r = {"max_abs_dssim_vs_emulation": float(np.abs(got[:, 0] - want_s).max()), "max_rel_dmse_vs_emulation": float((np.abs(got[:, 1] - want_m) / want_m).max()),
         "max_abs_dpsnr_dB_vs_psnr_each": float(np.abs(E.psnr_of_mse(got[:, 1]) - E.psnr_each(recon, orig)).max()), "ssim_mean": float(got[:, 0].mean())}
    assert r["max_abs_dssim_vs_emulation"] <= 1e-10 and r["max_rel_dmse_vs_emulation"] <= 1e-12, r
    r["a_device_call_events"] = stats(event_timed(lambda: ops.image_metrics(recon, orig), a.reps))
    r["a_device_call_u8_events"] = stats(event_timed(lambda: ops.image_metrics(recon, orig, quantize=True), a.reps))
    r["a_metrics_each_with_result_read"] = stats(host_timed(lambda: E.metrics_each(recon, orig), a.reps))
    r["b_numpy_emulation_16_threads"] = stats(host_timed(lambda: emulation(recon_h, orig_h), 3, warm=1))
    r["c_psnr_each_host_route_d2h_included"] = stats(host_timed(lambda: E.psnr_each(recon, orig), a.reps))
    res[f"B{B}"] = r
    del orig, recon
if not a.no_pipeline:
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    pipe = SelftokPipeline(cfg=default_config(512, renderer=True), ckpt_path=None, sd3_path=None, datasize=S, device=dev, verbose=False,
                           state_dict=W.synthetic_state_dict(W.expected_shapes(512, renderer=True), device=dev), vae_state_dict=W.synthetic_vae_state_dict(device=dev))
    for B in [int(b) for b in a.batches.split(",")]:
        imgs = synth.synthetic_images(B, size=S).to(dev)

        def batch():
            ids = pipe.encoding(imgs, device=dev).detach().cpu().numpy()
            return pipe.decoding_with_renderer(ids, device=dev)
        t = float(np.median(host_timed(batch, 3, warm=1)))
        r = res[f"B{B}"]
        r["d_renderer_batch_without_metrics_ms"] = round(t * 1e3, 2)
        for name, key in (("device", "a_metrics_each_with_result_read"), ("numpy_emulation", "b_numpy_emulation_16_threads"), ("psnr_each_psnr_only", "c_psnr_each_host_route_d2h_included")):
            m = r[key]["median_ms"] * 1e-3
            r[f"d_share_of_batch_{name}"] = round(m / (t + m), 5)
pool.shutdown()
lines = [f"{k}: {json.dumps(v)}" for k, v in res.items()] + [json.dumps(res)]
print("\n".join(lines), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")
