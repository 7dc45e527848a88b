"""Where the time of an augmented image input stage goes on MI355X: 64 synthetic 500 x 375 uint8 arrays already in memory (no file decoding),
Resize(281) -> TenCrop(256): 640 views per batch.

  (a) the host route: per view `preprocess.apply_view_pil` (crop, PIL resize, crop, flip, NormalizeToTensor), torch.stack, .to(device), .to(bf16)
      -- in one thread, and the same PIL work on a 16-thread pool (one task per image);
  (b) the device route (preprocess.DeviceLoader.load(views=...)): pack the 64 sources into the pinned buffer, one H2D copy, the view kernels
      (csrc/image_views.hip) -- split by HIP events;
  (c) encode-only images/s: `encoding` fed by (a) against `encoding_u8(views=...)`, on the same 64 images, --encode-chunk images (ten views
      each) per encode call.

Same process for every variant, 3 warm-up + 15 repetitions, median and min..max.  Prints a text report and one JSON line, and writes the same
JSON to profiles/image_views.json (--out).  There is no speed gate: the file says what was measured, whichever route wins.

    python tools/bench_image_views.py [--reps 15] [--no-encode] [--out profiles/image_views.json]"""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from selftoktokenizer_amd import preprocess, synth, weights as W
from selftoktokenizer_amd.config import default_config

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--encode-chunk", type=int, default=8, help="images (ten views each) per encode call of the comparison (c)")
ap.add_argument("--no-encode", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_views.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
B, S, R = a.batch, 256, 281
arrays = synth.synthetic_u8_images(B, sizes=((500, 375),))
views = lambda w, h: preprocess.views_ten(w, h, R, S)


def one(arr):
    return [preprocess.apply_view_pil(arr, v) for v in views(arr.shape[1], arr.shape[0])]


pool = ThreadPoolExecutor(max_workers=16)


def host_route(threads, imgs=arrays):
    per = list(pool.map(one, imgs)) if threads > 1 else [one(x) for x in imgs]
    t1 = time.perf_counter()
    out = torch.stack([t for ts in per for t in ts]).to(dev).to(torch.bfloat16)
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


res = {"tool": "bench_image_views", "device": torch.cuda.get_device_name(dev), "batch": B, "source": "500 x 375 uint8, in memory",
       "recipe": f"Resize({R}) -> TenCrop({S})", "views_per_batch": 10 * B, "warmup": 3, "reps": a.reps}
# (a)
for th in (1, 16):
    pil, tail = [], []
    def run():
        t0 = time.perf_counter()
        _, t1 = host_route(th)
        pil.append(t1 - t0); tail.append(time.perf_counter() - t1)
    tot = timed(run, a.reps)
    res[f"a_host_{th}_threads"] = {"total": stats(tot), "pil_views_normalize": stats(pil[3:]), "stack_h2d_to_bf16": stats(tail[3:]),
                                   "views_per_s": round(10 * B / float(np.median(tot)), 1)}
# (b)
loader = preprocess.DeviceLoader(S, dev, dtype=torch.bfloat16, workers=1)
loader.timing = True
pack, h2d, kern = [], [], []
def run_b():
    out = loader.load(arrays, views=views)
    torch.cuda.synchronize()
    e0, e1, e2 = loader.last_events
    pack.append(loader.last_times["pack_s"]); h2d.append(e0.elapsed_time(e1) * 1e-3); kern.append(e1.elapsed_time(e2) * 1e-3)
    return out
tot = timed(run_b, a.reps)
res["b_device_route"] = {"total": stats(tot), "pack_into_pinned": stats(pack[3:]), "h2d_copy": stats(h2d[3:]), "view_kernels": stats(kern[3:]),
                         "bytes_per_batch": loader.last_times["bytes"], "views_per_s": round(10 * B / float(np.median(tot)), 1)}
res["b_equals_a_bit_for_bit"] = bool(torch.equal(run_b(), host_route(16)[0]))
# (c)
if not a.no_encode:
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device=dev)
    vsd = W.synthetic_vae_state_dict(device=dev)
    step = a.encode_chunk
    chunks = [arrays[i:i + step] for i in range(0, B, step)]                   # one repetition = all B images, `step` images (ten views each) per call
    for label, kw in (("exact", dict(encoder_mode="exact", vae_mode="exact")), ("fast_parity", dict(encoder_mode="fast", vae_mode="parity"))):
        pipe = SelftokPipeline(default_config(512), None, None, device=dev, state_dict=sd, vae_state_dict=vsd, verbose=False, **kw)
        r, ids = {"images": B, "views": 10 * B, "images_per_call": step}, {}
        for name, fn in (("encoding_fed_by_a_1_thread", lambda c: pipe.encoding(host_route(1, c)[0], device=dev)),
                         ("encoding_fed_by_a_16_threads", lambda c: pipe.encoding(host_route(16, c)[0], device=dev)),
                         ("encoding_u8_views", lambda c: pipe.encoding_u8(c, views=views))):
            t = timed(lambda: ids.__setitem__(name, torch.cat([fn(c) for c in chunks])), a.reps)
            r[name] = dict(stats(t), images_per_s=round(B / float(np.median(t)), 2), views_per_s=round(10 * B / float(np.median(t)), 1))
            print(f"c_encode_{label} {name}: {json.dumps(r[name])}", file=sys.stderr, flush=True)
        r["same_ids"] = bool(torch.equal(ids["encoding_u8_views"], ids["encoding_fed_by_a_1_thread"]))
        fed = [host_route(1, c)[0] for c in chunks]
        r["encode_alone"] = stats(timed(lambda: [pipe.encoding(x, device=dev) for x in fed], a.reps))
        res[f"c_encode_{label}"] = r
        del pipe
        torch.cuda.empty_cache()
pool.shutdown()
loader.close()
for k, v in res.items():
    print(f"{k}: {json.dumps(v)}")
print(json.dumps(res), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
