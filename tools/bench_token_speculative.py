"""Speculative token sampling on MI355X: acceptance on synthetic noise and the time of one verify round -> profiles/token_speculative.json.  No gate.

    python tools/bench_token_speculative.py --synthetic [--quick] [--C 32768] [--S 4] [--out profiles/token_speculative.json]

Synthetic logits only (--synthetic says so on the command line): target = gaussian, draft = target + gaussian noise at a few sigma.  The acceptance rates and
tokens per round are properties of that noise, not of any model.  Per configuration (B = 1 / 8 / 64; fp32, and bf16 with guidance on both sides; top-k 50
with top-p 0.9, and greedy), warm, device events, the three routes alternating in one loop, median of 30 runs with minimum and maximum:
 1. `verify`: ops.token_verify, the verify + commit pair;
 2. `torch`: the torch route on the same buffers -- two softmax -> sort -> cumsum -> mask chains, gather, rand, clamp, multinomial (greedy: two argmax);
 3. `sample_floor`: B * (S + 1) rows through ops.token_sample alone: a verify row does the sampler's work twice, so it cannot beat this."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--synthetic", action="store_true", help="required: the only logits this tool has are synthetic")
ap.add_argument("--quick", action="store_true", help="fewer repetitions, B = 1 and 64 only")
ap.add_argument("--C", type=int, default=32768)
ap.add_argument("--S", type=int, default=4)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "token_speculative.json"))
a = ap.parse_args()
if not a.synthetic:
    ap.error("pass --synthetic: there are no model logits here, and the acceptance rates below are properties of the noise")
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
C, S, K = a.C, a.S, 1024


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


def filtered(lc, lu, s, greedy):
    """what a user writes today, fp32 throughout: the filtered, renormalised distribution of every row"""
    l = lc.float()
    if lu is not None:
        u = lu.float()
        l = u + s * (l - u)
    if greedy:
        return torch.zeros_like(l).scatter_(-1, l.argmax(-1, keepdim=True), 1.0)
    kth = torch.topk(l, min(50, l.shape[-1]), dim=-1).values[..., -1:]
    p = torch.softmax(l.masked_fill(l < kth, float("-inf")), -1)
    sp, si = torch.sort(p, dim=-1, descending=True)
    keep = (torch.cumsum(sp, -1) - sp) < 0.9
    p = torch.zeros_like(p).scatter_(-1, si, sp * keep)
    return p / p.sum(-1, keepdim=True)


def torch_route(tl, tu, dl, du, x, s, greedy, gen):
    p, d = filtered(tl, tu, s, greedy), filtered(dl, du, s, greedy)
    px, dx = p[:, :S].gather(-1, x.unsqueeze(-1)).squeeze(-1), d.gather(-1, x.unsqueeze(-1)).squeeze(-1)
    accept = torch.rand(x.shape, device=x.device, generator=gen) * dx < px
    resid = (p[:, :S] - d).clamp_(min=0)
    resid = torch.where(resid.sum(-1, keepdim=True) > 0, resid, p[:, :S])
    repl = torch.multinomial(resid.reshape(-1, resid.shape[-1]), 1, generator=gen)
    bonus = torch.multinomial(p[:, S], 1, generator=gen)
    return accept, repl, bonus


res = {"tool": "bench_token_speculative", "device": torch.cuda.get_device_name(0), "C": C, "S": S, "logits": "synthetic: draft = target + sigma * gaussian",
       "rows": []}
g = torch.Generator(device=dev).manual_seed(1)
reps = 10 if a.quick else 30
for B in ((1, 64) if a.quick else (1, 8, 64)):
    for dtype, guided in ((torch.float32, False), (torch.bfloat16, True)):
        for mode, kw in (("top_k50_top_p90", dict(top_k=50, top_p=0.9)), ("greedy", dict(temperature=0.0))):
            for sigma in (0.1, 0.3, 1.0):
                tl = torch.randn(B, S + 1, C, device=dev, generator=g)
                dl = (tl[:, :S] + sigma * torch.randn(B, S, C, device=dev, generator=g)).to(dtype).contiguous()
                tl = tl.to(dtype)
                tu = (0.5 * torch.randn(B, S + 1, C, device=dev, generator=g)).to(dtype) if guided else None
                du = tu[:, :S].contiguous() if guided else None
                scale = dict(cfg_scale=2.0, draft_cfg_scale=2.0) if guided else {}
                ctr0 = torch.stack([torch.arange(B, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)], 1).contiguous()
                # the drafter: S sampler steps on the draft rows, counters (ticket, s)
                x = torch.zeros(B, S, dtype=torch.int64, device=dev)
                nk1, mass1, lp1, bad = (torch.zeros(B, dtype=torch.int32, device=dev), torch.zeros(B, 3, dtype=torch.int64, device=dev), torch.zeros(B, device=dev),
                                        torch.zeros(1, dtype=torch.int32, device=dev))
                ctr = ctr0.clone()
                for s in range(S):
                    ops.token_sample(dl[:, s], ctr, x, uncond_logits=None if du is None else du[:, s], cfg_scale=2.0, seed=1, col=s, n_kept=nk1, mass=mass1,
                                     logprob=lp1, bad=bad, **kw)
                    ctr[:, 1] += 1
                ids, lpm, nkm = torch.zeros(B, K, dtype=torch.int64, device=dev), torch.zeros(B, K, device=dev), torch.zeros(B, K, dtype=torch.int32, device=dev)
                foreign = torch.zeros(1, dtype=torch.int32, device=dev)
                ctr = ctr0.clone()
                out = ops.token_verify(tl, dl, x, ctr, ids, lpm, nkm, target_uncond=tu, draft_uncond=du, seed=1, foreign=foreign, bad=bad, **scale, **kw)
                n_foreign = int(foreign.cpu()[0])                   # of this one round: the counter accumulates over the timed calls below
                pre = {k: getattr(out, k) for k in ("accept", "repl_id", "mass", "logprob_x", "logprob_repl", "n_accept", "n_emit")}

                def verify():
                    ctr.copy_(ctr0)                                  # each timed call starts from step 0 (one 8 B-per-row copy, counted)
                    ops.token_verify(tl, dl, x, ctr, ids, lpm, nkm, target_uncond=tu, draft_uncond=du, seed=1, row_n_kept=out.n_kept, foreign=foreign, bad=bad, **scale,
                                     **kw, **pre)

                R = B * (S + 1)
                flat, flat_u = tl.reshape(R, C), None if tu is None else tu.reshape(R, C)
                ctr_r = torch.stack([torch.arange(R, dtype=torch.int32, device=dev), torch.zeros(R, dtype=torch.int32, device=dev)], 1).contiguous()
                ids_r, nk_r, mass_r, lp_r = (torch.zeros(R, 1, dtype=torch.int64, device=dev), torch.zeros(R, dtype=torch.int32, device=dev),
                                             torch.zeros(R, 3, dtype=torch.int64, device=dev), torch.zeros(R, device=dev))
                fns = {"verify": verify,
                       "torch": lambda: torch_route(tl, tu, dl, du, x, 2.0, mode == "greedy", g),
                       "sample_floor": lambda: ops.token_sample(flat, ctr_r, ids_r, uncond_logits=flat_u, cfg_scale=2.0, seed=1, n_kept=nk_r, mass=mass_r, logprob=lp_r,
                                                                bad=bad, **kw)}
                t = {k: stats(v) for k, v in alternate(fns, reps).items()}
                n_acc = out.n_accept.float()
                row = {"B": B, "dtype": str(dtype).replace("torch.", ""), "guided": guided, "mode": mode, "sigma": sigma, **t,
                       "verify_over_floor": round(t["verify"]["median_ms"] / t["sample_floor"]["median_ms"], 2),
                       "torch_over_verify": round(t["torch"]["median_ms"] / t["verify"]["median_ms"], 2),
                       "acceptance_rate": round(float(out.accept[:, :S].float().mean()), 4), "mean_accepted_prefix": round(float(n_acc.mean()), 3),
                       "tokens_per_round": round(float(out.n_emit.float().mean()), 3), "foreign": n_foreign}
                res["rows"].append(row)
                print(json.dumps(row), flush=True)
                assert int(bad.cpu()[0]) == 0
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
