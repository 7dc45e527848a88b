"""Where the time of the image input stage goes on MI355X: 64 synthetic 500 x 375 uint8 arrays already in memory (no file decoding).

  (a) the host route: per image Resize -> CenterCrop -> NormalizeToTensor with PIL (`preprocess.load_image` without the file), torch.stack,
      .to(device), .to(bf16) -- in one thread, and the same PIL work on a 16-thread pool;
  (b) the device route (preprocess.DeviceLoader): pack into the pinned buffer, one H2D copy, the resize kernels -- split by HIP events;
  (c) encode-only images/s: `encoding` fed by (a) against `encoding_u8`, exact and fast / parity modes.

Same process for every variant, warm-up, >= 10 repetitions, median and min..max.  Prints a text report and one JSON line.

    python tools/bench_image_io.py [--reps 15] [--no-encode]"""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image
from selftoktokenizer_amd import preprocess, synth, weights as W
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.pipeline import NormalizeToTensor

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--no-encode", action="store_true")
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
B, S = a.batch, 256
arrays = synth.synthetic_u8_images(B, sizes=((500, 375),))


def one(arr):
    return NormalizeToTensor()(preprocess.center_crop(preprocess.resize_shorter_side(Image.fromarray(arr), S), S))


pool = ThreadPoolExecutor(max_workers=16)


def host_route(threads):
    ts = list(pool.map(one, arrays)) if threads > 1 else [one(x) for x in arrays]
    t1 = time.perf_counter()
    out = torch.stack(ts).to(dev).to(torch.bfloat16)
    torch.cuda.synchronize()
    return out, t1


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(float(v.min()) * 1e3, 3), "max_ms": round(float(v.max()) * 1e3, 3), "n": len(v)}


def timed(fn, reps, warm=3):
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


res = {"tool": "bench_image_io", "batch": B, "source": "500 x 375 uint8, in memory", "reps": a.reps}
# (a)
for th in (1, 16):
    pil, tail = [], []
    def run():
        t0 = time.perf_counter()
        _, t1 = host_route(th)
        pil.append(t1 - t0); tail.append(time.perf_counter() - t1)
    tot = timed(run, a.reps)
    res[f"a_host_{th}_threads"] = {"total": stats(tot), "pil_resize_crop_normalize": stats(pil[3:]), "stack_h2d_to_bf16": stats(tail[3:])}
# (b)
loader = preprocess.DeviceLoader(S, dev, dtype=torch.bfloat16, workers=1)
loader.timing = True
pack, h2d, kern = [], [], []
def run_b():
    out = loader.load(arrays)
    torch.cuda.synchronize()
    e0, e1, e2 = loader.last_events
    pack.append(loader.last_times["pack_s"]); h2d.append(e0.elapsed_time(e1) * 1e-3); kern.append(e1.elapsed_time(e2) * 1e-3)
    return out
tot = timed(run_b, a.reps)
res["b_device_route"] = {"total": stats(tot), "pack_into_pinned": stats(pack[3:]), "h2d_copy": stats(h2d[3:]), "resize_kernels": stats(kern[3:]),
                         "bytes_per_batch": loader.last_times["bytes"]}
same = bool(torch.equal(run_b(), host_route(1)[0]))
res["b_equals_a_bit_for_bit"] = same
# (c)
if not a.no_encode:
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device=dev)
    vsd = W.synthetic_vae_state_dict(device=dev)
    for label, kw in (("exact", dict(encoder_mode="exact", vae_mode="exact")), ("fast_parity", dict(encoder_mode="fast", vae_mode="parity"))):
        pipe = SelftokPipeline(default_config(512), None, None, device=dev, state_dict=sd, vae_state_dict=vsd, verbose=False, **kw)
        r = {}
        ids = {}
        for name, fn in (("encoding_fed_by_a_1_thread", lambda: pipe.encoding(host_route(1)[0], device=dev)),
                         ("encoding_fed_by_a_16_threads", lambda: pipe.encoding(host_route(16)[0], device=dev)),
                         ("encoding_u8", lambda: pipe.encoding_u8(arrays))):
            t = timed(lambda: ids.__setitem__(name, fn()), max(10, a.reps // 2 + 3), warm=2)
            r[name] = dict(stats(t), images_per_s=round(B / float(np.median(t)), 1))
        r["same_ids"] = bool(torch.equal(ids["encoding_u8"], ids["encoding_fed_by_a_1_thread"]))
        r["encode_alone"] = stats(timed(lambda x=host_route(1)[0]: pipe.encoding(x, device=dev), 10, warm=1))
        res[f"c_encode_{label}"] = r
        del pipe
        torch.cuda.empty_cache()
pool.shutdown()
loader.close()
for k, v in res.items():
    print(f"{k}: {json.dumps(v)}")
print(json.dumps(res), flush=True)
