"""What rFID (FID InceptionV3 pool3, synthetic weights) costs on MI355X at B = 64 images of 256 x 256 resized to 299 x 299, one process, warm:

  (a) `InceptionNet.pool3` timed by HIP events, and every kernel launch of one internal chunk on its own (the input stage, the 94 convolutions, the
      14 pools, the spatial mean), summed per block;
  (b) the same network composed from torch.nn.functional on the GPU (MIOpen convolutions, fp32, NCHW, unfolded BatchNorm), A / B alternating with (a)
      inside one loop;
  (c) `fid.statistics` at N = 4096, D = 2048 (mean and covariance in fp64), next to torch's own fp64 `A.T @ A`;
  (d) one `evaluate()` batch of the one-step renderer (encoding + decoding_with_renderer, synthetic weights) and the share the two pool3 calls of a batch
      (originals, reconstructions) add to it.

3 warm-up runs + `--reps` repetitions, median and min..max.  Nothing is asserted about speed; the device features are checked against the fp64 emulation
(tests/fid_cases.py, on the first `--check` images) before anything is timed.  Writes one JSON object.

    python tools/bench_fid.py [--reps 10] [--batch 64] [--no-pipeline] [--out profiles/fid.json]"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import torch.nn.functional as F
import fid_cases as FC
from selftoktokenizer_amd import fid as FD, ops, synth, weights as W
from selftoktokenizer_amd.config import default_config

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--check", type=int, default=2, help="images checked against the fp64 emulation before timing")
ap.add_argument("--no-pipeline", action="store_true")
ap.add_argument("--out", default=None)
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


net = FD.InceptionNet.synthetic(dev)
recon = ((synth.synthetic_images(B, size=S).to(dev) + 1) / 2).clamp_(0, 1).to(torch.bfloat16)

tops = FC.TorchOps(torch.float32)
tops.sd = {k: v.to(dev) for k, v in tops.sd.items()}


def torch_pool3(x):
    """the same network from torch.nn.functional: bilinear interpolate, MIOpen fp32 convolutions, unfolded BatchNorm"""
    t = F.interpolate(x.float() * 2 - 1, size=(FD.SIDE, FD.SIDE), mode="bilinear", align_corners=False)
    return FC.network(t, tops).mean((2, 3))


n = min(a.check, B)
got = net.pool3(recon, False)
want = FC.pool3(recon[:n].float().cpu().numpy(), True, False, False, True)
gate = 4.0 * FC.fp32_relative_error()
res = {"tool": "bench_fid", "size": S, "side": FD.SIDE, "images": B, "reps": a.reps, "device": torch.cuda.get_device_name(0), "weights": net.source,
       "checked_images": n, "max_rel_error_vs_fp64_emulation": float(FC.rel_err(got[:n].cpu().numpy(), want).max()), "gate": gate,
       "torch_functional_max_rel_diff_to_device": float(FC.rel_err(torch_pool3(recon).cpu().numpy(), got.cpu().numpy()).max())}
assert res["max_rel_error_vs_fp64_emulation"] <= gate, res

own, lib = [], []
for _ in range(3):
    net.pool3(recon, False); torch_pool3(recon)
for _ in range(a.reps):                                                                         # A / B alternating
    own.append(event_time(lambda: net.pool3(recon, False)))
    lib.append(event_time(lambda: torch_pool3(recon)))
res["a_pool3_call_events"], res["b_torch_functional_miopen_events"] = stats(own), stats(lib)

# per kernel launch of one internal chunk: the ops entries wrapped with events for `reps` walks
sizes = []
FD._walk(FD._Runner(net, lambda s: (sizes.append(-(-4 * int(np.prod(s[1:])) // 256) * 256), torch.empty(s, device="meta"))[1], dry=True), torch.empty(1, FD.SIDE, FD.SIDE, 3, device="meta"))
per_image = -(-4 * FD.SIDE * FD.SIDE * 3 // 256) * 256 + sum(sizes)
chunk = min(B, net.chunk_images or max(1, FD.CHUNK_BYTES // per_image))
res["activation_bytes_per_image"], res["chunk_images"], res["chunks_per_call"] = per_image, chunk, -(-B // chunk)
marks = []
real = {k: getattr(ops, k) for k in ("fid_input", "fid_conv2d", "fid_pool3", "fid_spatial_mean")}
flops = {}


def wrapped(kind):
    def call(*args, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = real[kind](*args, **kw)
        e1.record()
        marks.append((e0, e1))
        return out
    return call


for k in real:
    setattr(ops, k, wrapped(k))
try:
    runs = []
    for _ in range(3 + a.reps):
        marks.clear()
        net.pool3(recon[:chunk], False)
        torch.cuda.synchronize()
        runs.append([e0.elapsed_time(e1) * 1e-3 for e0, e1 in marks])
finally:
    for k, f in real.items():
        setattr(ops, k, f)
per = np.median(np.asarray(runs[3:]), axis=0)                                                   # median per launch over the repetitions
# the launch order of one walk: input, then _walk's conv / pool calls, then the mean -- named by a dry walk that records them
order = ["input"]


class _Names(FD._Runner):
    def conv(self, name, x, out=None, co_off=0):
        order.append(name)
        y = super().conv(name, x, out, co_off)
        ci, co, kh, kw, _, _, _ = FD.UNITS[name]
        flops[name] = 2.0 * chunk * y.shape[1] * y.shape[2] * co * ci * kh * kw
        return y

    def pool(self, x, mode, out=None, co_off=0):
        order.append("pool:" + mode)
        return super().pool(x, mode, out, co_off)


keep = {}
r = _Names(net, lambda s: torch.empty(s, device="meta"), dry=True)
FD._walk(r, torch.empty(1, FD.SIDE, FD.SIDE, 3, device="meta"), keep)
order.append("spatial_mean")
assert len(order) == len(per), (len(order), len(per))
groups, cur = {}, "stem"
for name, t in zip(order, per):
    if name.startswith("Mixed_"):
        cur = name.split(".")[0]
    key = name if name in ("input", "spatial_mean") else cur
    g = groups.setdefault(key, {"ms": 0.0, "launches": 0, "conv_flop": 0.0})
    g["ms"] += float(t) * 1e3; g["launches"] += 1; g["conv_flop"] += flops.get(name, 0.0)
for g in groups.values():
    g["ms"] = round(g["ms"], 4)
    g["conv_tflops"] = round(g.pop("conv_flop") / max(g["ms"] * 1e-3, 1e-12) / 1e12, 2)
res["a_per_block_one_chunk"] = groups
conv_ms = sum(float(t) for nme, t in zip(order, per) if nme in flops) * 1e3
res["a_convolutions_one_chunk"] = {"ms": round(conv_ms, 4), "launches": len(flops), "gflop_per_image": round(sum(flops.values()) / chunk / 1e9, 3),
                                   "tflops": round(sum(flops.values()) / (conv_ms * 1e-3) / 1e12, 2)}
res["a_pools_one_chunk_ms"] = round(sum(float(t) for nme, t in zip(order, per) if nme.startswith("pool:")) * 1e3, 4)

# (c) the statistics
N, D = 4096, FD.FEATURES
X = torch.relu(torch.randn(N, D, device=dev, generator=torch.Generator(device=dev).manual_seed(0)))


def torch_stats(X):
    A = X.double() - X.double().mean(0)
    return A.t() @ A / (N - 1)


mu, sg = FD.statistics(X)
res["c_stats_max_abs_diff_to_torch_fp64"] = float((sg - torch_stats(X)).abs().max())
own, lib = [], []
for _ in range(2):
    FD.statistics(X); torch_stats(X)
for _ in range(a.reps):
    own.append(event_time(lambda: FD.statistics(X)))
    lib.append(event_time(lambda: torch_stats(X)))
res["c_stats_n4096_d2048"], res["c_torch_fp64_matmul"] = stats(own), stats(lib)
t0 = time.perf_counter()
d2 = FD.frechet_distance(mu, sg, mu + 0.01, sg)
res["c_frechet_distance_host_s"] = round(time.perf_counter() - t0, 3)

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
    m = 2 * res["a_pool3_call_events"]["median_ms"] * 1e-3                                      # originals + reconstructions
    res["d_renderer_batch_without_metrics_ms"] = round(t * 1e3, 2)
    res["d_share_of_batch_rfid_two_pool3_calls"] = round(m / (t + m), 5)
print(json.dumps(res, indent=1), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write(json.dumps(res, indent=1) + "\n")
