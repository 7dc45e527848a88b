"""Times the count / nearest entry (ops.manifold_count_nn) next to the membership entry (ops.manifold_member) ON THE SAME BUFFERS and against the route a user would
otherwise write with torch (chunked fp32 matmul + compare + sum + min, never holding the M x N matrix), the KID sums (ops.kid_sums behind genmetrics.kid)
against index_select + matmul + pow + sum in torch, and one whole genmetrics.density_coverage -- one process, warm, the routes alternating in ONE loop, HIP
events: median [min .. max] per call.  Writes profiles/gen_metrics_kdc.json.

    python tools/bench_gen_metrics_kdc.py [--reps 5] [--pairs 50000x10000] [--kid 100x1000] [--dc 10000] [--out profiles/gen_metrics_kdc.json]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import genmetrics, ops

PEAK_FP32_MATRIX_TFLOPS = 157.3
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pairs", default="50000x10000", help="queries x set rows of the count / nearest run")
ap.add_argument("--kid", default="100x1000", help="subsets x rows per subset of the KID run")
ap.add_argument("--dc", type=int, default=10000, help="rows of either set of the density_coverage run (0: skip)")
ap.add_argument("--dim", type=int, default=2048)
ap.add_argument("--k", type=int, default=3)
ap.add_argument("--chunk", type=int, default=4096, help="rows per matmul of the torch route")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "gen_metrics_kdc.json"))
a = ap.parse_args()
torch.backends.cuda.matmul.allow_tf32 = False
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)


def rows(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(n, a.dim, device=dev, generator=g).abs_() * 0.5       # pool3-like: non-negative, norms far above the distances' spread


def torch_count_nn(X, A, r2):
    na, nx = (A * A).sum(1), (X * X).sum(1)
    cnt = torch.empty(X.shape[0], dtype=torch.int64, device=dev)
    nd, ni = torch.empty(X.shape[0], device=dev), torch.empty(X.shape[0], dtype=torch.int64, device=dev)
    for lo in range(0, X.shape[0], a.chunk):
        d = (nx[lo:lo + a.chunk, None] + na[None, :] - 2.0 * (X[lo:lo + a.chunk] @ A.t())).clamp_min_(0.0)
        cnt[lo:lo + a.chunk] = (d <= r2[None, :]).sum(1)
        nd[lo:lo + a.chunk], ni[lo:lo + a.chunk] = d.min(1)
    return cnt, nd, ni


def torch_kid_sums(feats_x, feats_y, gi, ri, m):
    out = torch.empty(gi.shape[0], 3, dtype=torch.float64, device=dev)
    D = feats_x.shape[1]
    off = ~torch.eye(m, dtype=torch.bool, device=dev)
    for s in range(gi.shape[0]):
        x, y = feats_x.index_select(0, gi[s]), feats_y.index_select(0, ri[s])
        k = lambda u, v: ((u @ v.t()).double() / D + 1.0).pow(3)
        out[s, 0], out[s, 1], out[s, 2] = k(x, x)[off].sum(), k(y, y)[off].sum(), k(x, y).sum()
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


def stats(ms, flops=None):
    med = float(np.median(ms))
    out = {"ms_median": med, "ms_min": float(min(ms)), "ms_max": float(max(ms))}
    if flops:
        out.update({"tflops": flops / med / 1e9, "of_fp32_matrix_peak": flops / med / 1e9 / PEAK_FP32_MATRIX_TFLOPS})
    return out


res = {"tool": "bench_gen_metrics_kdc", "device": torch.cuda.get_device_name(0), "dim": a.dim, "k": a.k, "reps": a.reps, "torch_chunk_rows": a.chunk,
       "peak_fp32_matrix_tflops": PEAK_FP32_MATRIX_TFLOPS, "timing": "HIP events around each call, routes alternating in one loop, one warm round dropped"}
m, n = (int(v) for v in a.pairs.split("x"))
X, A = rows(m, 1), rows(n, 2)
r2 = ops.knn_radius(A, a.k)
t = alternate({"count_nn": lambda: ops.manifold_count_nn(X, A, r2), "nn_only": lambda: ops.manifold_count_nn(X, A), "member": lambda: ops.manifold_member(X, A, r2),
               "torch": lambda: torch_count_nn(X, A, r2)})
flops = 2.0 * m * n * a.dim
cnt, nd, ni = ops.manifold_count_nn(X, A, r2)
tc, td, ti = torch_count_nn(X, A, r2)
res["count_nn"] = {"M": m, "N": n, "count_nn": stats(t["count_nn"], flops), "nn_only": stats(t["nn_only"], flops), "member_same_buffers": stats(t["member"], flops),
                   "torch": stats(t["torch"], flops), "count_nn_over_member_median": float(np.median(t["count_nn"]) / np.median(t["member"])),
                   "speedup_over_torch_median": float(np.median(t["torch"]) / np.median(t["count_nn"])),
                   "queries_with_equal_count": int((cnt == tc).sum().item()), "queries_with_equal_index": int((ni == ti).sum().item()),
                   "count_positive_equals_member": bool(((cnt > 0) == (ops.manifold_member(X, A, r2) != 0)).all().item())}
print(json.dumps(res["count_nn"]), flush=True)
del X, A
S, mk = (int(v) for v in a.kid.split("x"))
n_set = max(2 * mk, 10000)
R, G = rows(n_set, 3), rows(n_set, 4) * 1.1
gi_np, ri_np = genmetrics.kid_subsets(n_set, n_set, S, mk, genmetrics.KID_SEED)
gi, ri = torch.from_numpy(gi_np).to(dev), torch.from_numpy(ri_np).to(dev)
xs, ys = G.index_select(0, gi.reshape(-1)[: genmetrics.kid_chunk(mk, a.dim) * mk]), R.index_select(0, ri.reshape(-1)[: genmetrics.kid_chunk(mk, a.dim) * mk])
Sc = xs.shape[0] // mk
t = alternate({"kid": lambda: genmetrics.kid(R, G, S, mk), "kid_sums_one_chunk": lambda: ops.kid_sums(xs, ys, Sc, mk), "torch": lambda: torch_kid_sums(G, R, gi, ri, mk)})
flops = 3.0 * 2.0 * S * mk * mk * a.dim
got = genmetrics.kid(R, G, S, mk)
want = genmetrics.kid_of_sums(torch_kid_sums(G, R, gi, ri, mk).cpu().numpy(), mk)
res["kid"] = {"subsets": S, "subset_size": mk, "set_rows": n_set, "chunk_subsets": Sc, "kid_whole_call": stats(t["kid"], flops),
              "kid_sums_one_chunk": stats(t["kid_sums_one_chunk"], flops * Sc / S), "torch": stats(t["torch"], flops),
              "speedup_over_torch_median": float(np.median(t["torch"]) / np.median(t["kid"])), "kid": got["kid"], "kid_torch_route": want[0],
              "abs_difference": abs(got["kid"] - want[0])}
print(json.dumps(res["kid"]), flush=True)
del R, G, xs, ys
if a.dc:
    R, G = rows(a.dc, 5), rows(a.dc, 6)
    t = alternate({"density_coverage": lambda: genmetrics.density_coverage(R, G, a.k), "precision_recall": lambda: genmetrics.precision_recall(R, G, a.k)})
    res["density_coverage"] = {"N": a.dc, "density_coverage": stats(t["density_coverage"]), "precision_recall_same_buffers": stats(t["precision_recall"]),
                               "calls": "one knn_radius, two manifold_count_nn (with and without radii)"}
    print(json.dumps(res["density_coverage"]), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
