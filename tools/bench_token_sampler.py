"""Timings of the token sampler on MI355X -> profiles/token_sampler.json.  No gate: nothing here had been timed before.

    python tools/bench_token_sampler.py [--quick] [--out profiles/token_sampler.json]

ops.token_sample at B = 1, 8, 64, 256 rows x C = 32768 codes, fp32 and bf16 logits, with and without guidance, for greedy, top-k 50, top-p 0.9 and both,
next to the torch route on the same buffers: (guidance,) softmax -> sort -> cumsum -> mask -> multinomial (top-k by torch.topk; greedy by argmax).  Warm,
device events, the two routes alternating in one loop, median with minimum and maximum.  `hbm_fraction` is the bytes of the kernel's one read of the
logits (B * C * element size, twice that with guidance) over its median time, as a share of the 8.0 TB/s the HBM3E is specified at (a float4 copy
reaches 6.29 TB/s on this chip).  At B = 64 only a quarter of the 256 compute units have a row, and the logits of a repeated call come from the caches: the
figure says how far the kernel is from a pure read, not what the memory delivers."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer repetitions, B = 1 and 64 only")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "token_sampler.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
HBM_SPEC = 8.0e12
C = 32768


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, reps, warm=3):
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


def torch_route(lc, lu, s, mode, gen):
    """what a user writes today; fp32 throughout"""
    l = lc.float()
    if lu is not None:
        u = lu.float()
        l = u + s * (l - u)
    if mode == "greedy":
        return l.argmax(-1)
    if mode in ("top_k", "both"):
        kth = torch.topk(l, 50, dim=-1).values[:, -1:]
        l = l.masked_fill(l < kth, float("-inf"))
    p = torch.softmax(l, -1)
    if mode in ("top_p", "both"):
        sp, si = torch.sort(p, dim=-1, descending=True)
        keep = (torch.cumsum(sp, -1) - sp) < 0.9
        p = torch.zeros_like(p).scatter_(1, si, sp * keep)
    return torch.multinomial(p, 1, generator=gen)


MODES = {"greedy": dict(temperature=0.0), "top_k": dict(top_k=50), "top_p": dict(top_p=0.9), "both": dict(top_k=50, top_p=0.9)}
res = {"tool": "bench_token_sampler", "device": torch.cuda.get_device_name(0), "C": C, "hbm_spec_bytes_per_s": HBM_SPEC, "rows": []}
g = torch.Generator(device=dev).manual_seed(1)
reps = 10 if a.quick else 30
for B in ((1, 64) if a.quick else (1, 8, 64, 256)):
    for dtype in (torch.float32, torch.bfloat16):
        lc = torch.randn(B, C, device=dev, generator=g).to(dtype)
        lu = torch.randn(B, C, device=dev, generator=g).to(dtype)
        ctr = torch.stack([torch.arange(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)], 1).contiguous()
        ids = torch.zeros(B, 1, dtype=torch.int64, device=dev)
        nk, mass = torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, 3, dtype=torch.int64, device=dev)
        lp, bad = torch.zeros(B, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        for guided in (False, True):
            for mode, kw in MODES.items():
                un = lu if guided else None
                fns = {"kernel": lambda: ops.token_sample(lc, ctr, ids, uncond_logits=un, cfg_scale=3.0, seed=1, n_kept=nk, mass=mass, logprob=lp, bad=bad, **kw),
                       "torch": lambda: torch_route(lc, un, 3.0, mode, g)}
                t = alternate(fns, reps)
                k, ref = stats(t["kernel"]), stats(t["torch"])
                nbytes = B * C * lc.element_size() * (2 if guided else 1)
                row = {"B": B, "dtype": str(dtype).replace("torch.", ""), "guided": guided, "mode": mode, "kernel": k, "torch": ref,
                       "speedup": round(ref["median_ms"] / k["median_ms"], 2), "logit_bytes": nbytes,
                       "hbm_fraction": round(nbytes / (k["median_ms"] * 1e-3) / HBM_SPEC, 4), "mean_n_kept": round(float(nk.float().mean()), 1)}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
        assert int(bad.cpu()[0]) == 0
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
