"""Timings of the token distillation on MI355X -> profiles/token_distill.json.  No gate: nothing here had been timed before.

    python tools/bench_token_distill.py [--quick] [--out profiles/token_distill.json]

ops.token_distill (kl, ce, teacher entropy, student lse and the whole gradient in one launch) at R = 64, 4096 and 32768 rows x C = 32768 codes, fp32 and bf16
logits on both sides, with and without a guided teacher (cfg_scale 3), out of place, in place and metrics only, and one case over the window at offset 151936
of 184704-wide rows, next to the torch route on the same values, forward + backward on a leaf holding the student: the guided teacher materialised,
F.kl_div(log_softmax(s), softmax(t), reduction="none").sum(-1).mean(), autograd (on sliced copies of the window for the window case, whose gradient then
covers the window only).  Warm, device events, the contenders taking turns in one loop, median with minimum and maximum.  The in-place kernel destroys its
student logits, so every in-place run works on the gradient its predecessor left -- finite values of the same size and layout; the arithmetic per code does
not depend on the values.
`floor_bytes`: one read of the student window, one of the teacher window (two when guided), one write of the gradient row; `copy_fraction` / `hbm_fraction`:
those bytes over the kernel's median time as a share of the 6.29 TB/s a float4 copy reaches on this chip and of the 8.0 TB/s the HBM3E is specified at.
`valu_floor_ms`: the kernel's own instruction stream -- VALU instructions per code counted in the ISA of the streamed kernels (csrc/token_distill.hip;
DESIGN 36.3), one wave64 instruction per 4 cycles per SIMD, 1024 SIMDs at 2.4 GHz.  `peak_extra_bytes`: what a call allocates on top of its inputs."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from selftoktokenizer_amd import ops

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="fewer repetitions, R = 64 and 4096 only")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "token_distill.json"))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: a timing taken anywhere else says nothing"
dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
HBM_SPEC, COPY_RATE = 8.0e12, 6.29e12
C, OFFSET_VLM, V_VLM = 32768, 151936, 184704
# VALU instructions per code of the streamed kernels, from the ISA: (sweep 1 keys, sweep 2 masses and fp64 terms, sweep 3 masses again, quotients, store)
VALU_PER_CODE = {("float32", False): (27, 100, 82), ("float32", True): (44, 104, 84), ("bfloat16", False): (26, 104, 91), ("bfloat16", True): (38, 106, 93)}
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


def peak_extra(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


res = {"tool": "bench_token_distill", "device": torch.cuda.get_device_name(0), "C": C, "hbm_spec_bytes_per_s": HBM_SPEC, "copy_bytes_per_s": COPY_RATE,
       "valu_per_code": {f"{k[0]}{'_guided' if k[1] else ''}": sum(v) for k, v in VALU_PER_CODE.items()}, "rows": []}
g = torch.Generator(device=dev).manual_seed(1)
reps = 10 if a.quick else 30
shapes = [(R, C, 0) for R in ((64, 4096) if a.quick else (64, 4096, 32768))] + [(256 if a.quick else 4096, V_VLM, OFFSET_VLM)]
for R, V, off in shapes:
    for dtype in (torch.float32, torch.bfloat16):
        for guided in (False, True):
            name = str(dtype).replace("torch.", "")
            student = torch.randn(R, V, device=dev, generator=g).to(dtype)
            teacher = torch.randn(R, V, device=dev, generator=g).to(dtype)
            uncond = (teacher.float() - 0.5 * torch.randn(R, V, device=dev, generator=g)).to(dtype) if guided else None
            s = 3.0 if guided else 1.0
            work = student.clone()                                  # the in-place kernel's buffer
            scale = torch.full((R,), 1.0 / R, device=dev)
            grad = torch.empty_like(student)
            outs = dict(kl=torch.zeros(R, device=dev), ce=torch.zeros(R, device=dev), h_teacher=torch.zeros(R, device=dev), lse_student=torch.zeros(R, device=dev),
                        bad=torch.zeros(1, dtype=torch.int32, device=dev), ignored=torch.zeros(1, dtype=torch.int32, device=dev))
            leaf = student.clone().requires_grad_(True)
            kw = dict(teacher_uncond=uncond, cfg_scale=s, C=C, offset=off, row_scale=scale)

            def torch_route():
                leaf.grad = None
                cut = lambda x: x if off == 0 else x[:, off:off + C].contiguous()      # the window case: sliced copies restrict the softmax
                t = cut(teacher).float()
                if guided:
                    u = cut(uncond).float()
                    t = u + s * (t - u)
                F.kl_div(torch.log_softmax(cut(leaf).float(), -1), torch.softmax(t, -1), reduction="none").sum(-1).mean().backward()
                return leaf.grad

            fns = {"out_of_place": lambda: ops.token_distill(student, teacher, grad=grad, **kw, **outs),
                   "in_place": lambda: ops.token_distill(work, teacher, inplace=True, **kw, **outs),
                   "metrics_only": lambda: ops.token_distill(student, teacher, want_grad=False, **kw, **outs),
                   "torch": torch_route}
            tm = alternate(fns, reps)
            ko, ki, km, tc = stats(tm["out_of_place"]), stats(tm["in_place"]), stats(tm["metrics_only"]), stats(tm["torch"])
            leaf.grad = None                                        # so that the route's gradient counts in its peak
            torch_peak = peak_extra(torch_route)
            es = student.element_size()
            nbytes = R * ((2 + guided) * C + V) * es                # the windows read once each, the gradient row written once
            valu = VALU_PER_CODE[(name, guided)]
            row = {"R": R, "V": V, "C": C, "offset": off, "dtype": name, "guided": guided, "out_of_place": ko, "in_place": ki, "metrics_only": km, "torch_kl_fwd_bwd": tc,
                   "speedup_out_of_place": round(tc["median_ms"] / ko["median_ms"], 2), "speedup_in_place": round(tc["median_ms"] / ki["median_ms"], 2),
                   "floor_bytes": nbytes, "floor_ms_at_copy_rate": round(nbytes / COPY_RATE * 1e3, 4),
                   "copy_fraction_out_of_place": round(nbytes / (ko["median_ms"] * 1e-3) / COPY_RATE, 4), "hbm_fraction_out_of_place": round(nbytes / (ko["median_ms"] * 1e-3) / HBM_SPEC, 4),
                   "valu_floor_ms": round(R * C * sum(valu) / 64 * 4 / SIMDS / CLOCK * 1e3, 4),
                   "valu_floor_ms_metrics_only": round(R * C * sum(valu[:2]) / 64 * 4 / SIMDS / CLOCK * 1e3, 4),
                   "peak_extra_bytes": {"torch": torch_peak, "out_of_place_new_grad": peak_extra(lambda: ops.token_distill(student, teacher, **kw)),
                                        "in_place": peak_extra(fns["in_place"]), "metrics_only": peak_extra(fns["metrics_only"])}}
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
            assert int(outs["bad"].cpu()[0]) == 0
            del student, teacher, uncond, work, grad, leaf
            torch.cuda.empty_cache()
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
