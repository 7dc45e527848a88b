"""Teacher-forced scores of known token ids under an AR model's logits, on the GPU (sampling.score_tokens, csrc/token_score.hip).

    python tools/score_tokens.py --logits logits.npy --ids ids.npy [--uncond uncond.npy --cfg-scale 3.0] [--offset 151936 --codes 32768]
                                 [--temperature 1.0] [--tokenizer-order] [--json out.json]
    python tools/score_tokens.py --synthetic 4

logits: [B, S, V] fp32, or bf16 as its uint16 bits; ids: [B, K] int32 / int64 in tokenizer order, S <= K (.npy, or .npz with the arrays `logits`, `ids` and
optionally `uncond`).  By default logits row s is AR step s and scores tokenizer position K - 1 - s; --tokenizer-order scores row s against position s.  A
negative id is padding and is left out.  Prints NLL, perplexity, top-1 / top-5 accuracy, mean rank and mean entropy, pooled and per tokenizer position;
--json writes the same.  --synthetic N: N sequences of 16 positions over 1024 codes, ids drawn from the logits' own distribution (so NLL is near the entropy)."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import sampling


def load(path, key):
    a = np.load(path)
    return a[key] if hasattr(a, "files") else a


def to_device(x):
    x = np.ascontiguousarray(x)
    if x.dtype == np.uint16:
        return torch.from_numpy(x.view(np.int16)).cuda().view(torch.bfloat16)
    if x.dtype != np.float32:
        raise SystemExit(f"logits must be float32, or bf16 as uint16 bits, got {x.dtype}")
    return torch.from_numpy(x).cuda()


def synthetic(n):
    g = torch.Generator(device="cuda").manual_seed(20)
    B, K, V = n, 16, 1024
    lg = torch.randn(B, K, V, device="cuda", generator=g) * 2.0
    drawn = torch.multinomial(torch.softmax(lg.view(-1, V), -1), 1, generator=g).view(B, K)        # by AR step
    return lg, drawn.flip(1).contiguous()                           # ids in tokenizer order: AR step s is position K - 1 - s


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--logits"); ap.add_argument("--ids"); ap.add_argument("--uncond")
ap.add_argument("--cfg-scale", type=float, default=None)
ap.add_argument("--offset", type=int, default=0, help="first code of the window inside a logits row")
ap.add_argument("--codes", type=int, default=None, help="codes in the window (default: the rest of the row)")
ap.add_argument("--temperature", type=float, default=1.0)
ap.add_argument("--tokenizer-order", action="store_true", help="logits row s scores position s (default: AR order, position K - 1 - s)")
ap.add_argument("--allow-bad", action="store_true", help="summarise the rest when rows are bad (NaN / +inf logits, an id outside the window)")
ap.add_argument("--synthetic", type=int, default=0, metavar="N")
ap.add_argument("--json", default=None)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: there is no CPU fallback"
torch.cuda.set_device(0)
if a.synthetic:
    logits, ids = synthetic(a.synthetic)
    uncond = None
else:
    if not a.logits or not a.ids:
        raise SystemExit("need --logits and --ids, or --synthetic N")
    logits = to_device(load(a.logits, "logits"))
    ids = torch.from_numpy(np.ascontiguousarray(load(a.ids, "ids"))).cuda()
    uncond = to_device(load(a.uncond, "uncond")) if a.uncond else None
if ids.dtype not in (torch.int32, torch.int64):
    ids = ids.to(torch.int64)
sc = sampling.score_tokens(logits, ids, ar_order=not a.tokenizer_order, uncond_logits=uncond, cfg_scale=a.cfg_scale, C=a.codes, offset=a.offset,
                           temperature=a.temperature)
ok = a.allow_bad
scored = sc.rank >= 0
n_pos = scored.sum(0).double()
col = lambda x: (torch.where(scored, x.double(), torch.zeros((), dtype=torch.float64, device=x.device)).sum(0) / n_pos).cpu().tolist()
per = {"position": sc.positions.tolist(), "n": scored.sum(0).cpu().tolist(), "nll": col(-sc.logprob), "top1": col(sc.rank < 1), "top5": col(sc.rank < 5),
       "mean_rank": col(sc.rank), "mean_entropy": col(sc.entropy)}
res = {"rows": int(scored.numel()), "scored": int(scored.sum()), "ignored": int(sc.ignored.cpu()[0]), "bad": int(sc.bad.cpu()[0]),
       "nll": float(sc.nll(ok)), "perplexity": float(sc.perplexity(ok)), "top1": float(sc.topk_accuracy(1, ok)), "top5": float(sc.topk_accuracy(5, ok)),
       "mean_rank": float(sc.mean_rank(ok)), "mean_entropy": float(sc.mean_entropy(ok)), "sequence_logprob": sc.sequence_logprob(ok).cpu().tolist(),
       "per_position": per}
print(f"rows {res['rows']}  scored {res['scored']}  ignored {res['ignored']}  bad {res['bad']}")
print(f"NLL {res['nll']:.6f}  perplexity {res['perplexity']:.4f}  top-1 {res['top1']:.4f}  top-5 {res['top5']:.4f}  mean rank {res['mean_rank']:.2f}  "
      f"mean entropy {res['mean_entropy']:.6f}")
print("position      n        NLL    top-1    top-5  mean rank    entropy")
for i in np.argsort(per["position"]):
    print(f"{per['position'][i]:8d} {per['n'][i]:6d} {per['nll'][i]:10.6f} {per['top1'][i]:8.4f} {per['top5'][i]:8.4f} {per['mean_rank'][i]:10.2f} {per['mean_entropy'][i]:10.6f}")
if a.json:
    with open(a.json, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.json)
