"""GPU: what the split-K form of the single-pass fp16 Linear (set_gemm("f16", splitk="f16"), csrc/gemm_f16_splitk.hip) buys at one to four
images -> profiles/f16_splitk.json.  Reported, not gated.

1. Kernel time (partial + reduction launch) of ops.linear_f16_split[_residual]_k at ops.f16_ksplit against ops.linear_f16x2_split[_residual] at
   ops.f16x2_ksplit, the four block-Linear shapes (qkv, proj, fc1 + GELU with split output, fc2 + fused residual) at 256, 513, 769 and 1024 rows.
   Both read the SAME split activation; eight packed weight copies in rotation (the model streams its weights, nothing stays in L2 between
   uses); each measurement is a hipGraph of 20 calls replayed (eager timing of 5-20 us kernels measures the host); A / B alternating.
2. `decoding` of 1, 2 and 4 images (50 steps, K = 512, hipGraph) with splitk="f16", with splitk="f16" + attention="f16", and with the switch
   off (the f16x2 route), same process, alternating.
Every figure: median [min .. max] of the repeats.

    python tools/bench_f16_splitk.py [--repeats 5] [--no-decode] [--no-kernels] [--out profiles/f16_splitk.json]
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
ROWS = (256, 513, 769, 1024)
REP = 20


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1]}


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REP):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def replay_us(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / REP


def kernel_cases(M, name, N, K):
    g = torch.Generator(device="cuda").manual_seed(M + N + K)
    a = torch.randn(1, M, K, device="cuda", generator=g)
    w = torch.randn(N, K, device="cuda", generator=g) * 0.02
    b = torch.randn(N, device="cuda", generator=g) * 0.1
    xs, packs = ops.split_f16x2(a), [ops.linear_f16x2_pack(w) for _ in range(8)]
    s16, sx2 = ops.f16_ksplit(M, N, K), ops.f16x2_ksplit(M, N, K)
    i = [0]

    def nxt():
        i[0] = (i[0] + 1) & 7
        return packs[i[0]]

    if name == "fc2+residual":
        resid = torch.randn(1, M, N, device="cuda", generator=g)
        gate = torch.randn(1, N, device="cuda", generator=g)
        return (s16, sx2, lambda: ops.linear_f16_split_residual_k(xs, nxt(), b, N, resid, s16, gate=gate, gate_per_sample=True),
                lambda: ops.linear_f16x2_split_residual(xs, nxt(), b, N, resid, gate=gate, gate_per_sample=True, ksplit=sx2))
    kw = dict(gelu=True, out_split=True) if name == "fc1+gelu" else {}
    return s16, sx2, (lambda: ops.linear_f16_split_k(xs, nxt(), b, N, s16, **kw)), (lambda: ops.linear_f16x2_split(xs, nxt(), b, N, ksplit=sx2, **kw))


def bench_kernels(repeats):
    rows = []
    for M in ROWS:
        for name, N, K in SHAPES:
            s16, sx2, f16, x2 = kernel_cases(M, name, N, K)
            g16, gx2 = graph_of(f16), graph_of(x2)
            t16, tx2 = [], []
            for _ in range(repeats):                # alternating A / B
                t16.append(replay_us(g16))
                tx2.append(replay_us(gx2))
            row = {"shape": name, "M": M, "N": N, "K": K, "f16_ksplit": s16, "f16x2_ksplit": sx2, "f16_us": stats(t16), "f16x2_us": stats(tx2)}
            row["speedup_median"] = row["f16x2_us"]["median"] / row["f16_us"]["median"]
            row["faster_by_more_than_the_spread"] = max(t16) < min(tx2)
            rows.append(row)
            print(json.dumps(row), flush=True)
            del g16, gx2
    return rows


def bench_decode(repeats, batches=(1, 2, 4)):
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    pipe = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd,
                           vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False, gemm="f16")
    configs = (("splitk=f16", dict(splitk="f16")), ("splitk=f16 attention=f16", dict(splitk="f16", attention="f16")), ("switch off (f16x2 route)", {}))
    out = []
    for B in batches:
        ids, noise = synth.synthetic_token_ids(B), synth.synthetic_noise(B)
        times = {name: [] for name, _ in configs}

        def once(kw):
            assert pipe.set_gemm("f16", **kw) == "f16"
            torch.cuda.synchronize()
            t = time.perf_counter()
            rec = pipe.decoding(ids, noise=noise, use_graph=True)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            assert int(pipe.model.model.overflow.item()) == 0 and bool(torch.isfinite(rec.float()).all())
            return dt

        for _, kw in configs:                       # warm: first launches, graph capture
            once(kw)
        for _ in range(repeats):
            for name, kw in configs:
                times[name].append(once(kw))
        row = {"images": B, "tokens": 512, "steps": 50, "seconds": {k: stats(v) for k, v in times.items()}}
        base = row["seconds"]["switch off (f16x2 route)"]["median"]
        row["speedup_median"] = {k: base / v["median"] for k, v in row["seconds"].items()}
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-decode", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "f16_splitk.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_f16_splitk.py measures on the GPU; there is no fallback"
    out = {"tool": "bench_f16_splitk", "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "calls_per_graph": REP,
           "f16_splitk_cost": ops.F16_SPLITK_COST}
    if not a.no_kernels:
        out["kernels"] = bench_kernels(a.repeats)
    if not a.no_decode:
        out["decode"] = bench_decode(a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
