"""Where the time of the ADM image input (`center_crop_arr`: BOX halvings, one BICUBIC resize, centre crop) goes, and what the BICUBIC views
entry costs next to the BILINEAR one.  Uint8 arrays already in memory (no file decoding), S = 256.

  (a) the host route of record: per image `preprocess.center_crop_adm` + NormalizeToTensor, torch.stack [, .to(device), .to(bf16)] -- in one
      thread, and the PIL work on a 16-thread pool.  Needs no GPU: --host-only measures just this;
  (b) the device route (preprocess.DeviceLoader(preprocess="adm")): pack into the pinned buffer, one H2D copy, the kernels (csrc/image_filters.hip)
      -- split by HIP events; then the kernels alone, stage by stage: each BOX halving depth (ops.image_resize) and the BICUBIC views call;
  (c) the workload of profiles/image_views.json (64 x 500 x 375, Resize(281) -> TenCrop(256), 640 views) through the BILINEAR entry and through
      the BICUBIC one: the view kernels of each.

The ADM workload mixes three sizes, --sizes (default 500x375, 1000x750, 2000x1500: 0, 1 and 2 halvings).  Same process for every variant, 3 warm-up +
--reps repetitions, median and min..max.  Prints a text report and one JSON line and writes the same JSON to profiles/image_filters.json (--out).
There is no speed gate: the claim of the device route is equal bytes, and the file says what was measured, whichever route wins.

    python tools/bench_image_filters.py [--reps 15] [--host-only] [--out profiles/image_filters.json]"""
import argparse, json, os, sys, time
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image
from selftoktokenizer_amd import preprocess, synth

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--sizes", default="500x375,1000x750,2000x1500")
ap.add_argument("--host-only", action="store_true", help="only (a), without touching a GPU")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_filters.json"))
a = ap.parse_args()
B, S = a.batch, 256
sizes = tuple(tuple(int(v) for v in s.split("x")) for s in a.sizes.split(","))
arrays = synth.synthetic_u8_images(B, sizes=sizes)
dev = None
if not a.host_only:
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
norm = preprocess.NormalizeToTensor()
pool = ThreadPoolExecutor(max_workers=16)


def sync():
    if dev is not None:
        torch.cuda.synchronize()


def one(arr):
    return norm(preprocess.center_crop_adm(Image.fromarray(arr), S))


def host_route(threads):
    per = list(pool.map(one, arrays)) if threads > 1 else [one(x) for x in arrays]
    t1 = time.perf_counter()
    out = torch.stack(per)
    if dev is not None:
        out = out.to(dev).to(torch.bfloat16)
    sync()
    return out, t1


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": round(float(np.median(v)) * 1e3, 3), "min_ms": round(float(v.min()) * 1e3, 3), "max_ms": round(float(v.max()) * 1e3, 3), "n": len(v)}


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    out = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


plans = [preprocess.adm_plan(x.shape[1], x.shape[0], S) for x in arrays]
res = {"tool": "bench_image_filters", "device": torch.cuda.get_device_name(dev) if dev is not None else None, "host_cpus_used": 16, "batch": B,
       "source": f"{a.sizes} uint8, in memory", "recipe": f"center_crop_arr(S = {S}): BOX halvings, BICUBIC, centre crop",
       "halvings_per_image": sorted({len(p.frames) - 1 for p in plans}), "warmup": 3, "reps": a.reps}
# (a)
for th in (1, 16):
    pil, tail = [], []
    def run():
        t0 = time.perf_counter()
        _, t1 = host_route(th)
        pil.append(t1 - t0); tail.append(time.perf_counter() - t1)
    tot = timed(run, a.reps)
    res[f"a_host_{th}_threads"] = {"total": stats(tot), "pil_adm_normalize": stats(pil[3:]), "stack_h2d_to_bf16" if dev is not None else "stack": stats(tail[3:]),
                                   "images_per_s": round(B / float(np.median(tot)), 1)}
if dev is not None:
    from selftoktokenizer_amd import ops
    # (b)
    loader = preprocess.DeviceLoader(S, dev, dtype=torch.bfloat16, workers=1, preprocess="adm")
    loader.timing = True
    pack, h2d, kern = [], [], []
    def run_b():
        out = loader.load(arrays)
        torch.cuda.synchronize()
        e0, e1, e2 = loader.last_events
        pack.append(loader.last_times["pack_s"]); h2d.append(e0.elapsed_time(e1) * 1e-3); kern.append(e1.elapsed_time(e2) * 1e-3)
        return out
    tot = timed(run_b, a.reps)
    res["b_device_route"] = {"total": stats(tot), "pack_into_pinned": stats(pack[3:]), "h2d_copy": stats(h2d[3:]), "kernels": stats(kern[3:]),
                             "bytes_per_batch": loader.last_times["bytes"], "images_per_s": round(B / float(np.median(tot)), 1)}
    res["b_equals_a_bit_for_bit"] = bool(torch.equal(run_b(), host_route(16)[0]))
    # the kernels alone, stage by stage, on the batch as the loader staged it
    st = loader._stage(arrays, 0)
    front = st.rows.size + sum(c.size for c in st.chain)
    head = (front * 8 + 63) // 64 * 64
    buf = torch.empty(st.nbytes, dtype=torch.uint8, device=dev)
    buf[:st.copied].copy_(loader._pinned[0][:st.copied])
    pixels = buf[head:]
    stages = {f"box_halving_depth_{d + 1}": [] for d in range(len(st.chain))}
    stages["bicubic_views"] = []
    def run_stages():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(st.chain) + 2)]
        ev[0].record()
        for d, c in enumerate(st.chain):
            ops.image_resize(pixels, c, "box")
            ev[d + 1].record()
        ops.image_views(pixels, None, None, S, rows=st.rows, filter="bicubic")
        ev[-1].record()
        torch.cuda.synchronize()
        for d, key in enumerate(stages):
            stages[key].append(ev[d].elapsed_time(ev[d + 1]) * 1e-3)
    timed(run_stages, a.reps)
    res["b_kernel_stages"] = dict({k: stats(v[3:]) for k, v in stages.items()}, frames_per_depth=[int(c.shape[0]) for c in st.chain],
                                  note="each stage includes the copy of its small table to the device and its workspace allocation")
    loader.close()
    # (c)
    same = synth.synthetic_u8_images(B, sizes=((500, 375),))
    views = lambda w, h: preprocess.views_ten(w, h, 281, S)
    outs = {}
    for mode, label in (("reference", "bilinear"), ("bicubic", "bicubic")):
        ld = preprocess.DeviceLoader(S, dev, dtype=torch.bfloat16, workers=1, preprocess=mode)
        ld.timing = True
        k = []
        def run_c():
            outs[label] = ld.load(same, views=views)
            torch.cuda.synchronize()
            k.append(ld.last_events[1].elapsed_time(ld.last_events[2]) * 1e-3)
        tot = timed(run_c, a.reps)
        res[f"c_ten_crop_{label}"] = {"total": stats(tot), "view_kernels": stats(k[3:]), "views_per_batch": 10 * B}
        ld.close()
    host = torch.stack([preprocess.apply_view_pil(x, v, filter="bicubic") for x in same[:4] for v in views(500, 375)]).to(dev).to(torch.bfloat16)
    res["c_bicubic_equals_pillow_bit_for_bit"] = bool(torch.equal(outs["bicubic"][:40], host))
pool.shutdown()
for k, v in res.items():
    print(f"{k}: {json.dumps(v)}")
print(json.dumps(res), flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
