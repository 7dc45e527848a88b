"""What LPIPS (AlexNet, synthetic weights) costs on MI355X at B = 64 pairs of 256 x 256, one process, warm:

  (a) `LpipsNet.__call__` timed by HIP events, and every kernel of it on its own (input stage, the five convolutions, the two pools, the five
      distance stages) on the shapes of that batch;
  (b) the same network composed from torch.nn.functional on the GPU (MIOpen convolutions, fp32, NCHW; the distance in torch fp64), A / B
      alternating with (a) inside one loop;
  (c) one `evaluate()` batch of the one-step renderer (encoding + decoding_with_renderer, synthetic weights) and the share LPIPS adds to it.

3 warm-up runs + `--reps` repetitions, median and min..max.  Nothing is asserted about speed; the device values are checked against the fp64
emulation (tests/lpips_cases.py, on the first `--check` pairs) before anything is timed.  Writes one JSON object.

    python tools/bench_lpips.py [--reps 15] [--batch 64] [--no-pipeline] [--out profiles/lpips.json]

--net vgg: the same protocol for LPIPS on the VGG16 backbone (synthetic weights) -- `LpipsNet(net="vgg").__call__` and the AlexNet network's call A / B
alternating inside one loop on the same pairs, then every kernel of the VGG route on the shapes of one internal chunk: the 13 convolutions' share of the
call and their fraction of the fp32 matrix peak (157.3 TFLOP/s, v_mfma_f32_32x32x2_f32).  Values are checked against the fp64 emulation of
tests/lpips_vgg_cases.py (on the first `--check` pairs) first.

    python tools/bench_lpips.py --net vgg [--reps 15] [--batch 64] [--check 1] [--out profiles/lpips_vgg.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F
import lpips_cases as L
from selftoktokenizer_amd import ops, synth, weights as W
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.lpips import LAYERS, LpipsNet, tap_sizes

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--check", type=int, default=4, help="pairs checked against the fp64 emulation before timing")
ap.add_argument("--no-pipeline", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--net", default="alex", choices=["alex", "vgg"])
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
S, B = 256, a.batch


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": round(float(np.median(v)) * 1e3, 4), "min_ms": round(float(v.min()) * 1e3, 4), "max_ms": round(float(v.max()) * 1e3, 4), "n": len(v)}


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3


def event_timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    return [event_time(fn) for _ in range(reps)]


def bench_vgg():
    import lpips_vgg_cases as V
    from selftoktokenizer_amd import lpips as LP
    PEAK = 157.3                                                                                # TFLOP/s, fp32 matrix (MFMA f32 in / f32 accumulate)
    vgg, alex = LpipsNet.synthetic(dev, net="vgg"), LpipsNet.synthetic(dev)
    orig = synth.synthetic_images(B, size=S).to(dev)
    recon = ((synth.synthetic_images(B, size=S, first_index=B).to(dev) + 1) / 2).clamp_(0, 1).to(torch.bfloat16)
    n = min(a.check, B)
    got, got_alex = vgg(recon, orig).cpu().numpy(), alex(recon, orig).cpu().numpy()
    want = V.emulate(recon[:n].float().cpu().numpy(), orig[:n].cpu().numpy(), True, True, False)
    gate = 4.0 * V.fp32_relative_error()
    res = {"tool": "bench_lpips --net vgg", "size": S, "pairs": B, "reps": a.reps, "device": torch.cuda.get_device_name(0), "weights": vgg.source,
           "protocol": "one process, warm, 3 warm-up runs + reps repetitions, HIP events around one call, A / B alternating; median [min..max]",
           "lpips_vgg_mean": float(got.mean()), "lpips_alex_mean": float(got_alex.mean()), "checked_pairs": n,
           "max_rel_error_vs_fp64_emulation": float((np.abs(got[:n] - want) / want).max()), "gate": gate}
    assert res["max_rel_error_vs_fp64_emulation"] <= gate and want.min() >= 0.05, res
    tv, ta = [], []
    for _ in range(3):
        vgg(recon, orig); alex(recon, orig)
    for _ in range(a.reps):
        tv.append(event_time(lambda: vgg(recon, orig)))
        ta.append(event_time(lambda: alex(recon, orig)))
    res["vgg_call_events"], res["alex_call_events"] = stats(tv), stats(ta)
    per_pair = 2 * 4 * sum(h * w * c for _, h, w, c in vgg._plan(1, S, S))
    chunk = min(B, vgg.chunk_pairs or max(1, LP.CHUNK_BYTES // per_pair))
    chunks = -(-B // chunk)
    res["activation_bytes_per_pair"], res["chunk_pairs"], res["chunks_per_call"] = per_pair, chunk, chunks
    kern, conv_ms, conv_flop, tap = {}, 0.0, 0.0, 0
    x = ops.lpips_input(recon[:chunk], orig[:chunk])
    kern["input"] = stats(event_timed(lambda: ops.lpips_input(recon[:chunk], orig[:chunk]), a.reps))
    for (name, _, co, ci, is_tap, pool), packed, bias in zip(LP.VGG_LAYERS, vgg.packed, vgg.bias):
        xin = x
        t = stats(event_timed(lambda: ops.lpips_conv2d(xin, packed, bias, co, 3, 3, 1, 1, True), a.reps))
        flop = 2.0 * xin.shape[0] * xin.shape[1] * xin.shape[2] * co * ci * 9
        t["tflops"] = round(flop / (t["median_ms"] * 1e-3) / 1e12, 2)
        t["fraction_of_fp32_matrix_peak"] = round(t["tflops"] / PEAK, 4)
        kern[name] = t
        conv_ms, conv_flop = conv_ms + t["median_ms"], conv_flop + flop
        x = ops.lpips_conv2d(xin, packed, bias, co, 3, 3, 1, 1, True)
        if is_tap:
            cur, lw = x, vgg.lin[tap]
            kern["distance_" + name] = stats(event_timed(lambda: ops.lpips_distance(cur, lw), a.reps))
            tap += 1
        if pool:
            cur = x
            kern["pool_" + name] = stats(event_timed(lambda: ops.lpips_maxpool2s2(cur), a.reps))
            x = ops.lpips_maxpool2s2(cur)
    res["per_kernel_one_chunk"] = kern
    call = res["vgg_call_events"]["median_ms"]
    res["convolutions_ms_per_call"] = round(conv_ms * chunks, 3)
    res["convolutions_share_of_call"] = round(conv_ms * chunks / call, 4)
    res["convolutions_tflops"] = round(conv_flop * chunks / (conv_ms * chunks * 1e-3) / 1e12, 2)
    res["convolutions_fraction_of_fp32_matrix_peak"] = round(res["convolutions_tflops"] / PEAK, 4)
    res["call_tflops_convolution_flop_over_call_time"] = round(conv_flop * chunks / (call * 1e-3) / 1e12, 2)
    res["vgg_over_alex_call_time"] = round(call / res["alex_call_events"]["median_ms"], 2)
    print(json.dumps(res, indent=1), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(json.dumps(res, indent=1) + "\n")


if a.net == "vgg":
    bench_vgg()
    sys.exit(0)

net = LpipsNet.synthetic(dev)
orig = synth.synthetic_images(B, size=S).to(dev)                                                # fp32 in [-1, 1)
recon = ((synth.synthetic_images(B, size=S, first_index=B).to(dev) + 1) / 2).clamp_(0, 1).to(torch.bfloat16)     # independent pairs: d >= 0.05, where the relative gate means something

sd, lin = LpipsNet.synthetic_tensors()
tw = [(sd[k + ".weight"].to(dev), sd[k + ".bias"].to(dev)) for _, k, *_ in LAYERS]
tl = [w.to(dev).double().view(1, -1, 1, 1) for w in lin]
shift, scale = torch.tensor(L.SHIFT, device=dev).view(1, 3, 1, 1), torch.tensor(L.SCALE, device=dev).view(1, 3, 1, 1)


def torch_lpips(recon, orig):
    """the same network from torch.nn.functional: MIOpen fp32 convolutions on 2B images, the distance in torch fp64"""
    x = (torch.cat([recon.float() * 2 - 1, orig.float()]) - shift) / scale
    total = None
    for (_, _, _, _, k, s, p, pool), (w, b), lw in zip(LAYERS, tw, tl):
        x = F.relu(F.conv2d(x, w, b, stride=s, padding=p))
        f = x.double()
        f = f / (f.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
        d = (lw * (f[:B] - f[B:]).pow(2)).sum(1).mean((1, 2))
        total = d if total is None else total + d
        if pool:
            x = F.max_pool2d(x, 3, 2)
    return total


n = min(a.check, B)
got = net(recon, orig).cpu().numpy()
want = L.emulate(recon[:n].float().cpu().numpy(), orig[:n].cpu().numpy(), True, True, False)
gate = 4.0 * L.fp32_relative_error()
res = {"tool": "bench_lpips", "size": S, "pairs": B, "reps": a.reps, "device": torch.cuda.get_device_name(0), "weights": net.source,
       "lpips_mean": float(got.mean()), "checked_pairs": n, "max_rel_error_vs_fp64_emulation": float((np.abs(got[:n] - want) / want).max()), "gate": gate,
       "torch_functional_max_rel_diff_to_device": float((np.abs(torch_lpips(recon, orig).cpu().numpy() - got) / got).max())}
assert res["max_rel_error_vs_fp64_emulation"] <= gate and want.min() >= 0.05, res

own, lib = [], []
for _ in range(3):
    net(recon, orig); torch_lpips(recon, orig)
for _ in range(a.reps):                                                                         # A / B alternating
    own.append(event_time(lambda: net(recon, orig)))
    lib.append(event_time(lambda: torch_lpips(recon, orig)))
res["a_lpipsnet_call_events"], res["b_torch_functional_miopen_events"] = stats(own), stats(lib)

# per kernel, on the shapes of one internal chunk (what __call__ launches) -- and how many chunks a call walks
per_pair = 2 * 4 * sum(h * w * c for _, h, w, c in net._plan(1, S, S))
chunk = min(B, net.chunk_pairs or max(1, (96 << 20) // per_pair))
res["chunk_pairs"], res["chunks_per_call"] = chunk, -(-B // chunk)
kern = {}
x = ops.lpips_input(recon[:chunk], orig[:chunk])
kern["input"] = stats(event_timed(lambda: ops.lpips_input(recon[:chunk], orig[:chunk]), a.reps))
for (name, _, co, ci, k, s, p, pool), packed, bias, lw, (h, w) in zip(LAYERS, net.packed, net.bias, net.lin, tap_sizes(S, S)):
    xin = x
    t = stats(event_timed(lambda: ops.lpips_conv2d(xin, packed, bias, co, k, k, s, p, True), a.reps))
    flop = 2.0 * 2 * chunk * h * w * co * ci * k * k
    t["tflops"] = round(flop / (t["median_ms"] * 1e-3) / 1e12, 2)
    kern[name] = t
    x = ops.lpips_conv2d(xin, packed, bias, co, k, k, s, p, True)
    tap = x
    kern["distance_" + name] = stats(event_timed(lambda: ops.lpips_distance(tap, lw), a.reps))
    if pool:
        kern["pool_" + name] = stats(event_timed(lambda: ops.lpips_maxpool3s2(tap), a.reps))
        x = ops.lpips_maxpool3s2(tap)
res["a_per_kernel_one_chunk"] = kern

if not a.no_pipeline:
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    pipe = SelftokPipeline(cfg=default_config(512, renderer=True), ckpt_path=None, sd3_path=None, datasize=S, device=dev, verbose=False,
                           state_dict=W.synthetic_state_dict(W.expected_shapes(512, renderer=True), device=dev), vae_state_dict=W.synthetic_vae_state_dict(device=dev))
    imgs = synth.synthetic_images(B, size=S).to(dev)

    def batch():
        ids = pipe.encoding(imgs, device=dev).detach().cpu().numpy()
        return pipe.decoding_with_renderer(ids, device=dev)
    ts = []
    batch()
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        batch()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    m = res["a_lpipsnet_call_events"]["median_ms"] * 1e-3
    res["c_renderer_batch_without_metrics_ms"] = round(t * 1e3, 2)
    res["c_share_of_batch_lpips"] = round(m / (t + m), 5)
print(json.dumps(res, indent=1), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
