"""Timings of the token policy loss on MI355X -> profiles/token_policy.json.

    python tools/bench_token_policy.py [--quick] [--out profiles/token_policy.json]

Three routes to the gradient of the clipped PPO / GRPO surrogate with a k3 KL penalty (and, in the `ent` rows, an entropy bonus) on the same values:
  (a) ops.token_policy: one launch -- in place and out of place;
  (b) what the kernels before it allow: ops.token_score for the log-probability, the ratio, clip and coefficient in torch, ops.token_xent(row_scale=coef);
      it cannot produce the entropy gradient, so the `ent` rows have no (b);
  (c) plain torch with autograd: log_softmax, gather, exp, clamp, min, the entropy, backward -- on a leaf holding the logits (on a sliced copy of the window for the
      window case, whose gradient then covers the window only).
R = 64, 4096 and 32768 rows x C = 32768 codes and one case over the window at offset 151936 of 184704-wide rows, fp32 and bf16 logits.  Values checked before
timing: (a) against (b) and against (c) to 1e-5 of the largest gradient element (2^-7 for bf16); whether (a) and (b) agree bit for bit is recorded -- they do
wherever torch's exp and expm1 round the coefficient as the kernel's do.  Warm,
device events, the contenders taking turns in one loop, median with minimum and maximum of 30 runs.  The in-place kernel destroys its logits, so every in-place
run works on the gradient its predecessor left -- finite values of the same size and layout; the arithmetic per code does not depend on the values.
REQUIREMENT (recorded as `requirement`): the median of (a) out of place lies below (b)'s and below (c)'s at 4096 and at 32768 fp32 rows without the entropy term."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer repetitions, R = 64 and 4096 only")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "token_policy.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
HBM_SPEC, COPY_RATE = 8.0e12, 6.29e12
C, OFFSET_VLM, V_VLM = 32768, 151936, 184704
CLIP, KL_COEF, ENT_COEF = (0.2, 0.2), 0.04, 0.01


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


res = {"tool": "bench_token_policy", "device": torch.cuda.get_device_name(0), "C": C, "clip": CLIP, "kl_coef": KL_COEF, "ent_coef": ENT_COEF,
       "hbm_spec_bytes_per_s": HBM_SPEC, "copy_bytes_per_s": COPY_RATE, "rows": []}
g = torch.Generator(device=dev).manual_seed(38)
reps = 10 if a.quick else 30
shapes = [(R, C, 0) for R in ((64, 4096) if a.quick else (64, 4096, 32768))] + [(256 if a.quick else 4096, V_VLM, OFFSET_VLM)]
gate = {}
for R, V, off in shapes:
    for dtype in (torch.float32, torch.bfloat16):
        name = str(dtype).replace("torch.", "")
        logits = torch.randn(R, V, device=dev, generator=g).to(dtype)
        t = torch.randint(0, C, (R,), device=dev, generator=g)
        adv = torch.randn(R, device=dev, generator=g)
        scale = torch.full((R,), 1.0 / R, device=dev)
        lp0 = ops.token_score(logits, t, C=C, offset=off)[0]
        old = (lp0 + 0.25 * torch.randn(R, device=dev, generator=g)).contiguous()            # ratios on both sides of the clip range
        ref = (lp0 + 0.2 * torch.randn(R, device=dev, generator=g)).contiguous()
        lo, hi = 1.0 - CLIP[0], 1.0 + CLIP[1]
        for ent in (0.0, ENT_COEF):
            work = logits.clone()                                   # the in-place kernel's buffer
            grad_a, grad_b = torch.empty_like(logits), torch.empty_like(logits)
            row = lambda dt=torch.float32: torch.zeros(R, dtype=dt, device=dev)
            outs = dict(logprob=row(), lse=row(), ratio=row(), kl=row(), coef=row(), flags=row(torch.uint8), bad=torch.zeros(1, dtype=torch.int32, device=dev),
                        ignored=torch.zeros(1, dtype=torch.int32, device=dev))
            if ent:
                outs["entropy"] = row()
            s_out = dict(logprob=row(), mass=torch.zeros(R, 2, dtype=torch.int64, device=dev), rank=row(torch.int32), top_id=row(torch.int32), entropy=row(),
                         bad=torch.zeros(1, dtype=torch.int32, device=dev), ignored=torch.zeros(1, dtype=torch.int32, device=dev))
            x_out = dict(nll=row(), lse=row(), bad=torch.zeros(1, dtype=torch.int32, device=dev), ignored=torch.zeros(1, dtype=torch.int32, device=dev))
            kw = dict(ref_logprob=ref, clip=CLIP, kl_coef=KL_COEF, ent_coef=ent, C=C, offset=off, row_scale=scale)
            leaf = logits.clone().requires_grad_(True)

            def route_a():
                return ops.token_policy(logits, t, old, adv, grad=grad_a, **kw, **outs)

            def route_a_in_place():
                return ops.token_policy(work, t, old, adv, inplace=True, **kw, **outs)

            def route_b():
                lp = ops.token_score(logits, t, C=C, offset=off, **s_out)[0]
                ratio = torch.exp(lp.double() - old.double()).float()
                clipped = ((adv > 0) & (ratio > hi)) | ((adv < 0) & (ratio < lo))
                w = torch.where(clipped, torch.zeros((), dtype=torch.float64, device=dev), adv.double() * ratio.double()) + KL_COEF * torch.expm1(ref.double() - lp.double())
                return ops.token_xent(logits, t, C=C, offset=off, row_scale=scale * w.float(), grad=grad_b, **x_out)

            def route_c():
                leaf.grad = None
                x = leaf if off == 0 else leaf[:, off:off + C].contiguous()
                logp = torch.log_softmax(x.float() if dtype != torch.float32 else x, -1)
                lp = logp.gather(1, t.unsqueeze(1)).squeeze(1)
                ratio = torch.exp(lp - old)
                u = ref - lp
                rows = -torch.minimum(ratio * adv, ratio.clamp(lo, hi) * adv) + KL_COEF * (torch.expm1(u) - u)
                if ent:
                    rows = rows + ent * (logp.exp() * logp).sum(-1)
                (rows * scale).sum().backward()
                return leaf.grad

            # values before timings
            route_a()
            gc = route_c()
            win = slice(off, off + C)
            top = float(gc[:, win].abs().max())
            err_c = float((grad_a[:, win].float() - gc[:, win].float()).abs().max()) / top
            tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
            assert err_c <= tol, (R, V, name, ent, "route (a) against torch autograd", err_c)
            fns = {"a_out_of_place": route_a, "a_in_place": route_a_in_place, "c_torch_autograd": route_c}
            same_as_b = None
            if not ent:
                route_b()
                same_as_b = bool(torch.equal(grad_a.view(torch.int16 if dtype == torch.bfloat16 else torch.int32), grad_b.view(torch.int16 if dtype == torch.bfloat16 else torch.int32)))
                err_b = float((grad_a[:, win].float() - grad_b[:, win].float()).abs().max()) / top
                assert err_b <= tol, (R, V, name, "route (a) against route (b)", err_b)      # torch's exp / expm1 may round a coefficient the other way: not held to bits
                fns["b_score_torch_xent"] = route_b
            assert int(outs["bad"].cpu()[0]) == 0
            tm = alternate(fns, reps)
            st = {k: stats(v) for k, v in tm.items()}
            es = logits.element_size()
            nbytes = 2 * R * V * es if not off else R * (C + V) * es
            ma = st["a_out_of_place"]["median_ms"]
            out = {"R": R, "V": V, "C": C, "offset": off, "dtype": name, "ent_coef": ent, **st, "max_rel_err_against_torch": err_c, "bits_equal_to_route_b": same_as_b,
                   "ratio_c_over_a": round(st["c_torch_autograd"]["median_ms"] / ma, 2), "ratio_c_over_a_in_place": round(st["c_torch_autograd"]["median_ms"] / st["a_in_place"]["median_ms"], 2),
                   "read_write_bytes": nbytes, "read_write_ms_at_copy_rate": round(nbytes / COPY_RATE * 1e3, 4),
                   "copy_fraction_in_place": round(nbytes / (st["a_in_place"]["median_ms"] * 1e-3) / COPY_RATE, 4),
                   "hbm_fraction_in_place": round(nbytes / (st["a_in_place"]["median_ms"] * 1e-3) / HBM_SPEC, 4)}
            if not ent:
                out["ratio_b_over_a"] = round(st["b_score_torch_xent"]["median_ms"] / ma, 2)
                if dtype == torch.float32 and off == 0 and R in (4096, 32768):
                    gate[f"R{R}"] = {"a_ms": ma, "b_ms": st["b_score_torch_xent"]["median_ms"], "c_ms": st["c_torch_autograd"]["median_ms"],
                                     "a_below_b": ma < st["b_score_torch_xent"]["median_ms"], "a_below_c": ma < st["c_torch_autograd"]["median_ms"]}
            res["rows"].append(out)
            print(json.dumps(out), flush=True)
            del work, grad_a, grad_b, leaf, gc
            torch.cuda.empty_cache()
        del logits
        torch.cuda.empty_cache()
res["requirement"] = {"text": "(a) out of place below (b) and below (c) at 4096 and 32768 fp32 rows, ent_coef = 0", "shapes": gate,
                      "met": bool(gate) and all(v["a_below_b"] and v["a_below_c"] for v in gate.values()) and (a.quick or len(gate) == 2)}
print(json.dumps(res["requirement"]), flush=True)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
