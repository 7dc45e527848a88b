"""GPU: what the single-pass fp16 Linear mode (gemm="f16", csrc/gemm_f16.hip) buys over f16x2 -> profiles/f16_mode.json.

1. Kernel time (device events, warm, alternating A / B inside every repeat) of selftok_linear_f16_split[_residual] and of
   selftok_linear_f16x2_split[_residual] at the four block-Linear shapes (qkv, proj, fc1 + GELU with split output, fc2 + fused residual) at
   22912 and 16384 rows; both entries read the SAME split activation and the SAME packed weights.
2. A 64-image, 512-token, 50-step `decoding` in f16 and in f16x2 mode, same process, alternating, with the spread of the repeats.

    python tools/bench_f16_mode.py [--repeats 3] [--iters 20] [--no-decode] [--out profiles/f16_mode.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from selftoktokenizer_amd import ops, synth, weights as W  # noqa: E402
from selftoktokenizer_amd.config import default_config  # noqa: E402

H = 1536
SHAPES = (("qkv", 3 * H, H), ("proj", H, H), ("fc1+gelu", 4 * H, H), ("fc2+residual", H, 4 * H))
ROWS = (22912, 16384)


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_cases(M, name, N, K):
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.02
    b = torch.randn(N, device="cuda", generator=g) * 0.1
    xs, packed = ops.split_f16x2(a.reshape(64, M // 64, K)), ops.linear_f16x2_pack(w)
    if name == "fc2+residual":
        resid = torch.randn(64, M // 64, N, device="cuda", generator=g)
        gate = torch.randn(64, N, device="cuda", generator=g)
        return (lambda: ops.linear_f16_split_residual(xs, packed, b, N, resid, gate=gate, gate_per_sample=True),
                lambda: ops.linear_f16x2_split_residual(xs, packed, b, N, resid, gate=gate, gate_per_sample=True))
    kw = dict(gelu=True, out_split=True) if name == "fc1+gelu" else {}
    return lambda: ops.linear_f16_split(xs, packed, b, N, **kw), lambda: ops.linear_f16x2_split(xs, packed, b, N, **kw)


def bench_kernels(repeats, iters):
    rows = []
    for M in ROWS:
        for name, N, K in SHAPES:
            f16, x2 = kernel_cases(M, name, N, K)
            for fn in (f16, x2):                    # warm both
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            t16, tx2 = [], []
            for _ in range(repeats):                # alternating A / B
                t16.append(event_ms(f16, iters))
                tx2.append(event_ms(x2, iters))
            flop = 2.0 * M * N * K
            row = {"shape": name, "M": M, "N": N, "K": K, "f16_ms": t16, "f16x2_ms": tx2, "f16_ms_median": sorted(t16)[len(t16) // 2], "f16x2_ms_median": sorted(tx2)[len(tx2) // 2],
                   "f16_slowest_over_f16x2_fastest": max(t16) / min(tx2)}
            row["speedup_median"] = row["f16x2_ms_median"] / row["f16_ms_median"]
            row["f16_tflops_median"] = flop / row["f16_ms_median"] * 1e-9
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def bench_decode(repeats, batch=64):
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    pipe = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd,
                           vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False, gemm="f16x2")
    ids, noise = synth.synthetic_token_ids(batch), synth.synthetic_noise(batch)
    times = {"f16": [], "f16x2": []}

    def once(mode):
        assert pipe.set_gemm(mode) == mode
        torch.cuda.synchronize()
        t = time.perf_counter()
        rec = pipe.decoding(ids, noise=noise)
        torch.cuda.synchronize()
        assert int(pipe.model.model.overflow.item()) == 0 and bool(torch.isfinite(rec.float()).all())
        return time.perf_counter() - t

    for mode in ("f16", "f16x2"):                   # warm both (first launches, the packed weights)
        pipe.set_gemm(mode)
        pipe.decoding(ids, noise=noise, max_steps=2)
    for _ in range(repeats):
        for mode in ("f16", "f16x2"):
            times[mode].append(once(mode))
            print(json.dumps({"decode_s": times[mode][-1], "gemm": mode}), flush=True)
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: max(v) - min(v) for m, v in times.items()}
    return {"images": batch, "tokens": 512, "steps": 50, "seconds": times, "median_s": med, "spread_s": spread, "speedup_median": med["f16x2"] / med["f16"],
            "faster_by_more_than_the_spread": max(times["f16"]) < min(times["f16x2"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_mode.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_f16_mode.py measures on the GPU; there is no fallback"
    out = {"tool": "bench_f16_mode", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters}
    if not a.no_kernels:
        out["kernels"] = bench_kernels(a.repeats, a.iters)
        out["f16_faster_on_every_shape"] = all(r["f16_slowest_over_f16x2_fastest"] < 1.0 for r in out["kernels"])
    if not a.no_decode:
        out["decode"] = bench_decode(a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
