"""GPU: what the single-pass fp16 joint attention (ops.ATTN_F16, csrc/attention_f16.hip) buys over attn64_f16x2_kernel inside the
lossy gemm="f16" mode -> profiles/f16_attention.json.

1. Kernel time (device events, warm, alternating A / B inside every repeat) of selftok_attn_f16 and of the f16x2 attention (mode 1) on
   the SAME buffers: B = 64, 24 heads, n_x = 256 image rows, n_ctx in {513, 358, 128, 20} context rows, with a prefix `kvis` (every key
   visible) and with a 50 % suffix `kmask`, fp32 and split-activation outputs.
2. A 64-image, 512-token, 50-step `decoding` in gemm="f16" with and without attention="f16", same process, alternating, with the
   spread of the repeats.

    python tools/bench_f16_attention.py [--repeats 3] [--iters 20] [--no-decode] [--no-kernels] [--out profiles/f16_attention.json]
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

B, NH, NX = 64, 24, 256
H = NH * 64
N_CTX = (513, 358, 128, 20)


def event_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_case(n, masked, split):
    """-> {mode: launch} on one set of q | k | v buffers"""
    g = torch.Generator(device="cuda").manual_seed(n)
    cqkv = torch.randn(B, n, 3 * H, device="cuda", generator=g)
    xqkv = torch.randn(B, NX, 3 * H, device="cuda", generator=g)
    kvis = kmask = None
    if masked:
        kmask = ops.pack_key_mask((torch.arange(n, device="cuda") >= n // 2)[None].expand(B, n))
    else:
        kvis = torch.full((B,), n - 1, dtype=torch.int32, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    mk = (lambda rows: ops.SplitAct((B, rows, H), "cuda", zero=True)) if split else (lambda rows: torch.zeros(B, rows, H, device="cuda"))
    oc, ox = mk(n), mk(NX)
    seg0 = (cqkv[..., :H], cqkv[..., H:2 * H], cqkv[..., 2 * H:], oc)
    seg1 = (xqkv[..., :H], xqkv[..., H:2 * H], xqkv[..., 2 * H:], ox)
    run = lambda mode: ops.attention(seg0, seg1, NH, 64, kvis=kvis, seg0_sees_seg1=True, mode=mode, overflow=flag, kmask=kmask)
    return {"f16": lambda: run(ops.ATTN_F16), "f16x2": lambda: run(ops.ATTN_F16X2)}, flag


def bench_kernels(repeats, iters):
    rows = []
    for n in N_CTX:
        for masked in (False, True):
            for split in (False, True):
                fns, flag = kernel_case(n, masked, split)
                for fn in fns.values():              # warm both
                    for _ in range(3):
                        fn()
                torch.cuda.synchronize()
                assert int(flag.item()) == 0
                t = {"f16": [], "f16x2": []}
                for _ in range(repeats):             # alternating A / B
                    for m in ("f16", "f16x2"):
                        t[m].append(event_ms(fns[m], iters))
                med = {m: sorted(v)[len(v) // 2] for m, v in t.items()}
                visible = (n - n // 2 if masked else n) + NX
                flop = 4.0 * B * NH * 64 * visible * ((n - n // 2 if masked else n) + NX)     # live rows x visible keys, two products
                row = {"n_ctx": n, "visibility": "kmask 50% suffix" if masked else "kvis prefix (all)", "output": "split" if split else "fp32",
                       "f16_ms": t["f16"], "f16x2_ms": t["f16x2"], "f16_ms_median": med["f16"], "f16x2_ms_median": med["f16x2"],
                       "spread_ms": {m: max(v) - min(v) for m, v in t.items()}, "speedup_median": med["f16x2"] / med["f16"],
                       "faster_by_more_than_the_spread": max(t["f16"]) < min(t["f16x2"]), "f16_tflops_median": flop / med["f16"] * 1e-9}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def bench_decode(repeats, batch=64):
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    pipe = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd,
                           vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False, gemm="f16")
    ids, noise = synth.synthetic_token_ids(batch), synth.synthetic_noise(batch)
    names = {"attention=f16": "f16", "split attention": None}
    times = {k: [] for k in names}

    def once(name):
        assert pipe.set_gemm("f16", attention=names[name]) == "f16"
        torch.cuda.synchronize()
        t = time.perf_counter()
        rec = pipe.decoding(ids, noise=noise)
        torch.cuda.synchronize()
        assert int(pipe.model.model.overflow.item()) == 0 and bool(torch.isfinite(rec.float()).all())
        return time.perf_counter() - t

    for name in names:                               # warm both
        pipe.set_gemm("f16", attention=names[name])
        pipe.decoding(ids, noise=noise, max_steps=2)
    for _ in range(repeats):
        for name in names:
            times[name].append(once(name))
            print(json.dumps({"decode_s": times[name][-1], "gemm": "f16", "attention": name}), flush=True)
    med = {m: sorted(v)[len(v) // 2] for m, v in times.items()}
    spread = {m: max(v) - min(v) for m, v in times.items()}
    return {"images": batch, "tokens": 512, "steps": 50, "gemm": "f16", "seconds": times, "median_s": med, "spread_s": spread,
            "speedup_median": med["split attention"] / med["attention=f16"],
            "faster_by_more_than_the_spread": max(times["attention=f16"]) < min(times["split attention"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_attention.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_f16_attention.py measures on the GPU; there is no fallback"
    out = {"tool": "bench_f16_attention", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "iters": a.iters}
    if not a.no_kernels:
        out["kernels"] = bench_kernels(a.repeats, a.iters)
        out["f16_faster_at_n_ctx_358_and_513"] = all(r["faster_by_more_than_the_spread"] for r in out["kernels"] if r["n_ctx"] in (358, 513))
    if not a.no_decode:
        out["decode"] = bench_decode(a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "kernels"}))


if __name__ == "__main__":
    main()
