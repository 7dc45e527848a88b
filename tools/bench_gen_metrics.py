"""Times the precision / recall kernels (ops.knn_radius, ops.manifold_member) against the route a user would otherwise write with torch -- chunked fp32 matmul
plus topk / compare, never holding the N x N matrix -- alternating in ONE loop, warm, with HIP events: median [min .. max] per call, achieved TFLOP/s against
the 157.3 TFLOP/s fp32 matrix peak of MI355X, the largest |difference| between the two routes' radii, and what the new calls cost next to one evaluate() batch
of InceptionV3 features.  Writes profiles/gen_metrics.json.

    python tools/bench_gen_metrics.py [--reps 5] [--sizes 10000,50000] [--out profiles/gen_metrics.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import genmetrics, ops

PEAK_FP32_MATRIX_TFLOPS = 157.3
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--sizes", default="10000,50000", help="set sizes N of the radii runs (D = 2048)")
ap.add_argument("--member", default="50000x10000", help="queries x set rows of the membership run")
ap.add_argument("--dim", type=int, default=2048)
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--chunk", type=int, default=4096, help="rows per matmul of the torch route")
ap.add_argument("--features-batch", type=int, default=64, help="images of the evaluate() batch the new calls are set against (0: skip)")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gen_metrics.json"))
a = ap.parse_args()
torch.backends.cuda.matmul.allow_tf32 = False
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def rows(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, a.dim, device=dev, generator=g).abs_() * 0.5       # pool3-like: non-negative, norms far above the distances' spread


def torch_radii(A, k):
    na = (A * A).sum(1)
    out = torch.empty(A.shape[0], device=dev)
    for lo in range(0, A.shape[0], a.chunk):
        d = (na[lo:lo + a.chunk, None] + na[None, :] - 2.0 * (A[lo:lo + a.chunk] @ A.t())).clamp_min_(0.0)
        out[lo:lo + a.chunk] = torch.topk(d, k + 1, dim=1, largest=False).values[:, k]      # entry k of the sorted row, self included
    return out


def torch_member(X, A, r2):
    na, nx = (A * A).sum(1), (X * X).sum(1)
    out = torch.empty(X.shape[0], dtype=torch.bool, device=dev)
    for lo in range(0, X.shape[0], a.chunk):
        d = (nx[lo:lo + a.chunk, None] + na[None, :] - 2.0 * (X[lo:lo + a.chunk] @ A.t())).clamp_min_(0.0)
        out[lo:lo + a.chunk] = (d <= r2[None, :]).any(1)
    return out


def alternate(fns):
    """every function once per round, `reps` rounds after one warm round: {name: [ms]}"""
    times = {n: [] for n in fns}
    for r in range(a.reps + 1):
        for n, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if r:
                times[n].append(e0.elapsed_time(e1))
    return times


def stats(ms, flops):
    med = float(np.median(ms))
    return {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms)), "tflops": flops / med / 1e9, "of_fp32_matrix_peak": flops / med / 1e9 / PEAK_FP32_MATRIX_TFLOPS}


res = {"tool": "bench_gen_metrics", "device": torch.cuda.get_device_name(0), "dim": a.dim, "k": a.k, "reps": a.reps, "torch_chunk_rows": a.chunk,
       "peak_fp32_matrix_tflops": PEAK_FP32_MATRIX_TFLOPS, "timing": "HIP events around each call, routes alternating in one loop, one warm round dropped", "radii": [], "member": None}
for n in [int(v) for v in a.sizes.split(",") if v]:
    A = rows(n, n)
    t = alternate({"kernel": lambda: ops.knn_radius(A, a.k), "torch": lambda: torch_radii(A, a.k)})
    diff = (ops.knn_radius(A, a.k) - torch_radii(A, a.k)).abs().max().item()
    flops = 2.0 * n * n * a.dim
    res["radii"].append({"N": n, "kernel": stats(t["kernel"], flops), "torch": stats(t["torch"], flops), "speedup_median": float(np.median(t["torch"]) / np.median(t["kernel"])),
                         "max_abs_radius_difference": diff})
    print(json.dumps(res["radii"][-1]), flush=True)
    del A
m, n = (int(v) for v in a.member.split("x"))
X, A = rows(m, 1), rows(n, 2)
r2 = ops.knn_radius(A, a.k)
t = alternate({"kernel": lambda: ops.manifold_member(X, A, r2), "torch": lambda: torch_member(X, A, r2)})
flops = 2.0 * m * n * a.dim
agree = int(((ops.manifold_member(X, A, r2) != 0) == torch_member(X, A, r2)).sum().item())
res["member"] = {"M": m, "N": n, "kernel": stats(t["kernel"], flops), "torch": stats(t["torch"], flops), "speedup_median": float(np.median(t["torch"]) / np.median(t["kernel"])),
                 "queries_agreeing": agree}
print(json.dumps(res["member"]), flush=True)
if a.features_batch:
    from selftoktokenizer_amd.fid import InceptionNet
    net = InceptionNet.synthetic(dev)
    imgs = torch.rand(a.features_batch, 3, 256, 256, device=dev) * 2.0 - 1.0
    n0 = int(a.sizes.split(",")[0])
    R, G = rows(n0, 3), rows(n0, 4)
    t = alternate({"pool3": lambda: net.pool3(imgs, True), "precision_recall": lambda: genmetrics.precision_recall(R, G, a.k)})       # its four calls: two radii, two memberships
    batch_ms, pr_ms = float(np.median(t["pool3"])), float(np.median(t["precision_recall"]))
    features_ms = 2.0 * n0 / a.features_batch * batch_ms        # the pool3 batches of both sets, from the one batch timed
    res["evaluate_batch"] = {"images": a.features_batch, "pool3_ms_median": batch_ms, "N": n0, "precision_recall_ms_median": pr_ms,
                             "precision_recall_ms_min": float(min(t["precision_recall"])), "precision_recall_ms_max": float(max(t["precision_recall"])),
                             "precision_recall_over_one_pool3_batch": pr_ms / batch_ms, "feature_ms_for_both_sets_extrapolated": features_ms,
                             "share_of_the_evaluation_extrapolated": pr_ms / (pr_ms + features_ms)}
    print(json.dumps(res["evaluate_batch"]), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
