"""Timings of the token scorer on MI355X -> profiles/token_score.json.  No gate: nothing here had been timed before.

    python tools/bench_token_score.py [--quick] [--out profiles/token_score.json]

ops.token_score at R = 64, 4096 and 32768 rows x C = 32768 codes, fp32 and bf16 logits, with and without guidance, next to the torch route on the same
buffers in two forms: `ce`, the log-probability alone through F.cross_entropy(reduction="none") on the fp32 logits, and `full`, all four outputs
(log_softmax, gather, (l > l_t).sum, argmax, -(p * logp).sum).  Warm, device events, the three taking turns in one loop, median with minimum and maximum.
`hbm_fraction` / `copy_fraction`: the bytes of the kernel's one read of the logits (R * C * element size, twice that with guidance) over its median time, as a
share of the 8.0 TB/s the HBM3E is specified at and of the 6.29 TB/s a float4 copy reaches on this chip.  `valu_floor_ms`: the kernel's own instruction
stream -- VALU instructions per code counted in the ISA (csrc/token_score.hip, 16-chunk fp32 kernel: 13 in the first sweep, 16 with guidance, and 59 in the
second, 14 of them fp64), one wave64 instruction per 4 cycles per SIMD, 1024 SIMDs at 2.4 GHz.  `peak_extra_bytes`: what the comparator allocates on top of the inputs."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer repetitions, R = 64 and 4096 only")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "token_score.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
HBM_SPEC, COPY_RATE = 8.0e12, 6.29e12
C = 32768
VALU_PER_CODE = {False: 13 + 59, True: 16 + 59}                    # with guidance: a subtraction, a product and a sum more per code
SIMDS, CLOCK = 1024, 2.4e9


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warm=2):
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


def guided_logits(lc, lu, s):
    l = lc.float()
    if lu is not None:
        u = lu.float()
        l = u + s * (l - u)
    return l


def torch_ce(lc, lu, s, t):
    return -F.cross_entropy(guided_logits(lc, lu, s), t, reduction="none")


def torch_full(lc, lu, s, t):
    l = guided_logits(lc, lu, s)
    logp = torch.log_softmax(l, -1)
    lp = logp.gather(1, t.unsqueeze(1)).squeeze(1)
    rank = (l > l.gather(1, t.unsqueeze(1))).sum(-1)
    return lp, rank, l.argmax(-1), -(logp.exp() * logp).sum(-1)


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


res = {"tool": "bench_token_score", "device": torch.cuda.get_device_name(0), "C": C, "hbm_spec_bytes_per_s": HBM_SPEC, "copy_bytes_per_s": COPY_RATE,
       "valu_per_code": {"unguided": VALU_PER_CODE[False], "guided": VALU_PER_CODE[True]}, "rows": []}
g = torch.Generator(device=dev).manual_seed(1)
reps = 10 if a.quick else 30
for R in ((64, 4096) if a.quick else (64, 4096, 32768)):
    for dtype in (torch.float32, torch.bfloat16):
        lc = torch.randn(R, C, device=dev, generator=g).to(dtype)
        lu = torch.randn(R, C, device=dev, generator=g).to(dtype)
        t = torch.randint(0, C, (R,), device=dev, generator=g)
        outs = dict(logprob=torch.zeros(R, device=dev), mass=torch.zeros(R, 2, dtype=torch.int64, device=dev), rank=torch.zeros(R, dtype=torch.int32, device=dev),
                    top_id=torch.zeros(R, dtype=torch.int32, device=dev), entropy=torch.zeros(R, device=dev), bad=torch.zeros(1, dtype=torch.int32, device=dev),
                    ignored=torch.zeros(1, dtype=torch.int32, device=dev))
        for guided in (False, True):
            un = lu if guided else None
            fns = {"kernel": lambda: ops.token_score(lc, t, uncond_logits=un, cfg_scale=3.0, **outs),
                   "ce": lambda: torch_ce(lc, un, 3.0, t), "full": lambda: torch_full(lc, un, 3.0, t)}
            tm = alternate(fns, reps)
            k, ce, full = stats(tm["kernel"]), stats(tm["ce"]), stats(tm["full"])
            nbytes = R * C * lc.element_size() * (2 if guided else 1)
            rate = nbytes / (k["median_ms"] * 1e-3)
            row = {"R": R, "dtype": str(dtype).replace("torch.", ""), "guided": guided, "kernel": k, "torch_ce": ce, "torch_full": full,
                   "speedup_vs_ce": round(ce["median_ms"] / k["median_ms"], 2), "speedup_vs_full": round(full["median_ms"] / k["median_ms"], 2),
                   "logit_bytes": nbytes, "hbm_fraction": round(rate / HBM_SPEC, 4), "copy_fraction": round(rate / COPY_RATE, 4),
                   "valu_floor_ms": round(R * C * VALU_PER_CODE[guided] / 64 * 4 / SIMDS / CLOCK * 1e3, 4),
                   "peak_extra_bytes": {"ce": peak_extra(fns["ce"]), "full": peak_extra(fns["full"]), "kernel": peak_extra(fns["kernel"])}}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        assert int(outs["bad"].cpu()[0]) == 0
        del lc, lu
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
