"""VQ top-k lookup (csrc/vq_topk.hip) at N = 32768 rows, C = 32768 codes, k = 1, 2, 8: HIP-event time of
  (a) ops.vq_topk, the new entry (main kernel + finalize);
  (b) the existing argmax entry, ops.vq_encode(packed=True) on the fp32-input MFMA kernel (the arithmetic (a) shares) and on the default f16 coarse pass;
  (c) the dense torch route (normalize(z) @ codebook.T).topk(k): a [N, C] fp32 score matrix of 4 GiB, written and read back.
One process, 3 warm-up + 15 timed repetitions each, median [min .. max] in ms.  Before anything is timed, (a) is checked against (b): column 0 must be its ids and
score bits.  Writes one JSON file (default profiles/vq_topk.json) and prints it; `requirement_met` says whether (a) beat (c) at k = 2 and k = 8, and the exit
status is 1 if it did not.

    python tools/bench_vq_topk.py [--out profiles/vq_topk.json] [--rows 32768] [--reps 15]"""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import ops, synth, weights as W

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "vq_topk.json"))
ap.add_argument("--rows", type=int, default=32768)
ap.add_argument("--reps", type=int, default=15)
a = ap.parse_args()

C = 32768
cb = W._synth_tensor("encoder.quantizer._codebook.embed", (1, C, 16), "cpu")[0].contiguous().cuda()
pk = ops.vq_pack_codebook(cb)
z = synth.synthetic_vq_rows(a.rows, device="cuda")


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e))
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


ids1, best = ops.vq_encode(z, pk, packed=True, return_best=True, coarse=False)
for k in (1, 2, 8):
    ids, sc = ops.vq_topk(z, pk, k)
    assert torch.equal(ids[:, 0], ids1) and torch.equal(sc[:, 0].contiguous().view(torch.int32), best.view(torch.int32)), f"k = {k}: column 0 is not the argmax entry's output"
dense_ids = (torch.nn.functional.normalize(z, dim=-1) @ cb.T).topk(2).indices
agree = float((dense_ids == ops.vq_topk(z, pk, 2)[0]).all(dim=1).float().mean())

out = {"tool": "bench_vq_topk", "device": torch.cuda.get_device_name(0), "N": a.rows, "C": C, "reps": a.reps,
       "protocol": "HIP events around one call, one process, 3 warm-up + reps timed, median [min .. max]; allocation of outputs and workspace included in every route",
       "rows_where_dense_top2_ids_equal_ours": agree,
       "argmax_fp32_mfma": timed(lambda: ops.vq_encode(z, pk, packed=True, return_best=True, coarse=False)),
       "argmax_default_f16_coarse": timed(lambda: ops.vq_encode(z, pk, packed=True, return_best=True)), "k": {}}
for k in (1, 2, 8):
    new = timed(lambda: ops.vq_topk(z, pk, k))
    dense = timed(lambda: (torch.nn.functional.normalize(z, dim=-1) @ cb.T).topk(k))
    out["k"][str(k)] = {"vq_topk": new, "dense_torch_topk": dense, "dense_over_vq_topk": round(dense["median_ms"] / new["median_ms"], 2),
                        "vq_topk_over_argmax_fp32_mfma": round(new["median_ms"] / out["argmax_fp32_mfma"]["median_ms"], 2),
                        "vq_topk_over_argmax_default": round(new["median_ms"] / out["argmax_default_f16_coarse"]["median_ms"], 2)}
# the one speed requirement: the new entry beats the dense route at k = 2 and k = 8 (its ratio to the argmax kernel is reported, not gated)
out["faster_than_dense"] = {k: out["k"][k]["vq_topk"]["median_ms"] < out["k"][k]["dense_torch_topk"]["median_ms"] for k in ("2", "8")}
out["requirement_met"] = all(out["faster_than_dense"].values())
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps(out))
sys.exit(0 if out["requirement_met"] else 1)
