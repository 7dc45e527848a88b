"""Timings of the token statistics on MI355X -> profiles/token_stats.json.  No gate: nothing here had been timed before.

    python tools/bench_token_stats.py [--quick] [--out profiles/token_stats.json]

  token_count    64 x 512 (the size a tokenisation loop passes per call) and 65536 x 512 ids, uniform and all-equal (worst contention), next to
                 torch.bincount on k * C + id (which builds the index tensor, counts into a fresh int64 tensor and adds it to the running counts).
  token_nearest  10 000 queries x 100 000 reference rows x 512 positions, the achieved id comparisons per second and their share of the VALU rate of the
                 inner loop; next to the chunked torch route (q[:, None] == ref[None]).sum(-1).max(-1) on 200 of the queries, both routes alternating in
                 one loop at THAT size (the torch route at the full size would run for minutes; its full-size time is extrapolated, and named so).
Warm, device events, median with minimum and maximum, the versions alternating in one loop.

The VALU rate the share refers to (MI355X_MICROARCH: a wave64 vector instruction issues over 2 cycles per SIMD, 4 SIMDs per CU, 256 CUs, 2.4 GHz):
the inner loop spends v_pk_sub, v_pk_min_u16 and v_pk_add_u16 on every 32-bit word of two ids, so a SIMD compares 64 lanes * 2 ids / (3 * 2 cycles)
= 21.33 ids per cycle, the chip 21 845 per cycle = 5.24e13 per second at the full clock.  The LDS reads (one ds_read_b128 per 24 of those instructions), the
staging and the epilogue are not in that figure, and neither is the clock the chip actually holds under load."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="a tenth of the nearest problem, fewer repetitions")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "token_stats.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
VALU_PEAK = 64 * 2 / (3 * 2) * 4 * 256 * 2.4e9


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warm=2):
    """{name: [ms]}: the versions take turns inside one loop"""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(timed(f))
    return out


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5), "reps": len(ms)}


res = {"tool": "bench_token_stats", "device": torch.cuda.get_device_name(0), "count": [], "valu_peak_comparisons_per_s": VALU_PEAK}
K, C = 512, 32768
g = torch.Generator(device=dev).manual_seed(1)
for N in (64, 65536):
    for kind in ("uniform", "all_equal"):
        ids = torch.randint(0, C, (N, K), device=dev, generator=g) if kind == "uniform" else torch.full((N, K), 7, dtype=torch.int64, device=dev)
        counts, bad = torch.zeros(K, C, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        run64 = torch.zeros(K * C, dtype=torch.int64, device=dev)
        offs = (torch.arange(K, device=dev) * C)[None, :]

        def hip():
            ops.token_count(ids, counts, bad)

        def bincount():
            run64.add_(torch.bincount((ids + offs).reshape(-1), minlength=K * C))

        t = alternate({"token_count": hip, "torch_bincount": bincount}, 10 if a.quick else 30)
        reps = len(t["token_count"]) + 2
        assert torch.equal(counts.to(torch.int64).reshape(-1), run64) and int(counts.sum()) == reps * N * K      # both routes counted the same thing
        res["count"].append({"rows": N, "K": K, "C": C, "ids": kind, "token_count": stats(t["token_count"]), "torch_bincount": stats(t["torch_bincount"]),
                             "speedup_median": round(statistics.median(t["torch_bincount"]) / statistics.median(t["token_count"]), 3)})
        print(json.dumps(res["count"][-1]), flush=True)

M, N = (1000, 100000) if a.quick else (10000, 100000)
q = torch.randint(0, C, (M, K), device=dev, generator=g)
ref = torch.randint(0, C, (N, K), device=dev, generator=g)
ref[12345] = q[3]                                                   # one planted copy: the answer is checked, not only timed
qd, rd = ops.token_to_u16(q), ops.token_to_u16(ref)
Ms = 200


def torch_route(qq, chunk=8):
    best, idx = [], []
    for i in range(0, qq.shape[0], chunk):
        m = (qq[i:i + chunk, None, :] == ref[None, :, :]).sum(-1)
        v, j = m.max(-1)
        best.append(v); idx.append(j)
    return torch.cat(best), torch.cat(idx)


small = alternate({"token_nearest": lambda: ops.token_nearest(qd[:Ms], rd), "torch_chunked": lambda: torch_route(q[:Ms])}, 3 if a.quick else 5, warm=1)
b0, i0 = ops.token_nearest(qd[:Ms], rd)
b1, i1 = torch_route(q[:Ms])
assert torch.equal(b0.long(), b1.long()) and int(b0[3]) == K and int(i0[3]) == 12345
full = [timed(lambda: ops.token_nearest(qd, rd)) for _ in range(2 if a.quick else 3)]
comparisons = float(M) * N * K
rate = comparisons / (statistics.median(full) * 1e-3)
rate_small = float(Ms) * N * K / (statistics.median(small["token_nearest"]) * 1e-3)
res["nearest"] = {"M": M, "N": N, "K": K, "comparisons": comparisons, "token_nearest": stats(full), "comparisons_per_s": rate, "share_of_valu_rate": round(rate / VALU_PEAK, 4),
                  "valu_rate_note": "3 packed 16-bit instructions per 2 ids, 2 cycles per wave64 instruction and SIMD, 1024 SIMDs, 2.4 GHz; LDS reads, staging and the held clock not included",
                  "small": {"M": Ms, "token_nearest": stats(small["token_nearest"]), "torch_chunked": stats(small["torch_chunked"]), "comparisons_per_s": rate_small,
                            "speedup_median": round(statistics.median(small["torch_chunked"]) / statistics.median(small["token_nearest"]), 2)},
                  "torch_chunked_full_size_extrapolated_s": round(statistics.median(small["torch_chunked"]) * 1e-3 * M / Ms, 2)}
print(json.dumps(res["nearest"]), flush=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out, flush=True)
