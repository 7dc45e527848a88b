"""What a decode-stream step costs on MI355X (SelftokPipeline.decode_stream, synthetic weights, 256 x 256), one process, warm, 3 warm-up runs +
`--reps` repetitions, device events around whole steps, the versions that are compared alternating inside one loop:

  (a) slots = 64, all requests in phase: `--steps` stream steps from step 0 in both context modes against the same steps of `p_sample_loop` on the
      same 64 requests, per step.  Prices the in-place key-mask route and the two kernels of csrc/decode_stream.hip.
  (b) slots = 64, phases spread uniformly over the 50 steps: one stream step.
  (c) slots = 1, 2, 4: the mean of 49 stream steps against decoding / 50 with and without use_graph (decoding's figure contains the token
      lookup and the VAE; the stream's does not).  Here the modulation table replaces 28 GEMMs per step.
  (d) DERIVED from (a) and (b), not measured: wait to the first step and completion latency of a request that arrives uniformly in time, for the stream
      (a slot is free; it starts at the next step boundary) against "start a batch of 64 when the previous one ends".

The bench sets the stream's step counters directly (device and mirror) to put the slots into a phase; nothing retires inside a timed region.
Nothing is asserted about speed.  Writes one JSON object.

    python tools/bench_decode_stream.py [--reps 15] [--steps 2] [--slots 64] [--small 1,2,4] [--modes fp32,f16x2] [--out profiles/decode_stream.json]"""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from selftoktokenizer_amd import synth, weights as W
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.pipeline import SelftokPipeline

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--steps", type=int, default=2)
ap.add_argument("--slots", type=int, default=64)
ap.add_argument("--small", default="1,2,4")
ap.add_argument("--modes", default="fp32,f16x2")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_stream.json"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
WARM = 3


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(v.min()), 3), "max_ms": round(float(v.max()), 3), "n": len(v)}


def event_time(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternating(fns, reps):
    """{name: fn} -> {name: [ms]}: the versions take turns inside one loop"""
    out = {k: [] for k in fns}
    for r in range(WARM + reps):
        for k, fn in fns.items():
            t = event_time(fn)
            if r >= WARM:
                out[k].append(t)
    return out


def set_phase(stream, steps):
    stream.sched.step = [int(s) for s in steps]
    stream.step_dev.copy_(torch.tensor(stream.sched.step, dtype=torch.int32))


def filled(pipe, slots, ids, noise, context):
    stream = pipe.decode_stream(slots, context=context)
    for b in range(slots):
        stream.submit(ids[b], noise=noise[b])
    return stream


def run_steps(stream, phase, n):
    def fn():
        set_phase(stream, phase)
        for _ in range(n):
            assert stream.step() == []
    return fn


sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
pipe = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"))
pipe.verbose = False
dit = pipe.model.model
S = a.slots
ids, noise = synth.synthetic_token_ids(S), synth.synthetic_noise(S)
noise_dev = noise.to(dev)
res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "warm": WARM, "slots": S, "steps_timed_in_a": a.steps, "modes": {}}
with torch.no_grad():
    for mode in a.modes.split(","):
        assert pipe.set_gemm(mode) == mode
        out = {}
        # ---- (a) in phase, (b) spread ----
        ehs = pipe._codes(ids)
        live, full = filled(pipe, S, ids, noise, "live"), filled(pipe, S, ids, noise, "full")
        zero = [0] * S
        t = alternating({"p_sample_loop": lambda: pipe.flow.p_sample_loop(dit, noise_dev, ehs, pipe.k_table, max_steps=a.steps),
                         "stream_live": run_steps(live, zero, a.steps), "stream_full": run_steps(full, zero, a.steps)}, a.reps)
        out["a_in_phase_per_step"] = {k: stats(np.asarray(v) / a.steps) for k, v in t.items()}
        print(mode, "(a)", json.dumps(out["a_in_phase_per_step"]), flush=True)
        spread = [(b * 49) // S for b in range(S)]                               # steps 0 .. 48: nobody retires inside the timed step
        t = alternating({"stream_live": run_steps(live, spread, 1), "stream_full": run_steps(full, spread, 1)}, a.reps)
        out["b_spread_one_step"] = {k: stats(v) for k, v in t.items()}
        del live, full
        # ---- (d) derived ----
        Tb = out["a_in_phase_per_step"]["p_sample_loop"]["median_ms"]
        Ts = out["b_spread_one_step"]["stream_live"]["median_ms"]
        out["d_derived_not_measured"] = {
            "assumption": "requests arrive uniformly in time; the stream has a free slot; 50 steps per request; VAE and token lookup left out of both",
            "batch_start_when_previous_ends": {"step_ms": Tb, "wait_mean_s": round(25 * Tb / 1e3, 3), "wait_worst_s": round(50 * Tb / 1e3, 3),
                                               "completion_mean_s": round(75 * Tb / 1e3, 3), "completion_worst_s": round(100 * Tb / 1e3, 3)},
            "stream": {"step_ms": Ts, "wait_mean_s": round(0.5 * Ts / 1e3, 4), "wait_worst_s": round(Ts / 1e3, 4),
                       "completion_mean_s": round(50.5 * Ts / 1e3, 3), "completion_worst_s": round(51 * Ts / 1e3, 3)}}
        # ---- (c) small slot counts ----
        out["c_small"] = {}
        for n in [int(v) for v in a.small.split(",") if v]:
            st = filled(pipe, n, ids, noise, "live")
            pipe.decoding(ids[:n], noise=noise[:n], use_graph=True)                # capture outside the timed loop
            t = alternating({"stream_49_steps": run_steps(st, [0] * n, 49), "decoding": lambda: pipe.decoding(ids[:n], noise=noise[:n]),
                             "decoding_graph": lambda: pipe.decoding(ids[:n], noise=noise[:n], use_graph=True)}, a.reps)
            out["c_small"][str(n)] = {"stream_step": stats(np.asarray(t["stream_49_steps"]) / 49), "decoding_over_50": stats(np.asarray(t["decoding"]) / 50),
                                      "decoding_graph_over_50": stats(np.asarray(t["decoding_graph"]) / 50)}
            print(mode, "(c)", n, json.dumps(out["c_small"][str(n)]), flush=True)
            del st
        pipe._graphs.clear()
        res["modes"][mode] = out
        print(mode, json.dumps(out), flush=True)
    pipe.set_gemm("fp32")
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(res, f, indent=1)
print("wrote", a.out)
