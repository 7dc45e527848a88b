"""Statistics of token-id files on MI355X (selftoktokenizer_amd/tokenstats.py): what `tools/tokenize_folder.py --out` writes, the reference's int64 .npy
or the --uint16 form, [n, K] or [n, views, K] (views are counted as rows).

    python tools/token_stats.py --ids ids.rank0.npy                          # code-book usage, perplexity, dead codes
    python tools/token_stats.py --ids a.npy --against b.npy                  # how far two tokenisations of the same images disagree, and where they part
    python tools/token_stats.py --ids generated.npy --nearest-in train.npy   # is a generated sequence a near-copy of a training sequence
    python tools/token_stats.py --ids train.npy --dedup                      # near-duplicates inside one set (every row against every OTHER row)

Several --ids files are concatenated.  Prints ONE JSON line.  --codes C: the code-book size (default 32768); --k-range LO HI restricts --against,
--nearest-in and --dedup to the positions [LO, HI); --census-out saves the counts (.npz) for an offline merge."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import tokenstats as TS

ap = argparse.ArgumentParser()
ap.add_argument("--ids", nargs="+", required=True, help=".npy id files, int64 or uint16, [n, K] or [n, views, K]")
ap.add_argument("--against", nargs="+", default=None, help="a second tokenisation of the same rows")
ap.add_argument("--nearest-in", nargs="+", default=None, help="reference set: for every row of --ids the row with the most equal positions")
ap.add_argument("--dedup", action="store_true", help="--ids against itself, a row never its own candidate")
ap.add_argument("--codes", type=int, default=32768)
ap.add_argument("--k-range", type=int, nargs=2, default=None, metavar=("LO", "HI"))
ap.add_argument("--near", type=float, default=0.9, help="a row counts as a near-copy when at least this share of the positions is equal")
ap.add_argument("--census-out", default=None)
ap.add_argument("--device", type=int, default=0)
a = ap.parse_args()


def load(files):
    arrs = [np.load(f) for f in files]
    for f, x in zip(files, arrs):
        if x.ndim not in (2, 3) or not np.issubdtype(x.dtype, np.integer):
            sys.exit(f"{f}: expected integer ids [n, K] or [n, views, K], got {x.dtype} {x.shape}")
    arrs = [x.reshape(-1, x.shape[-1]) for x in arrs]
    if len({x.shape[1] for x in arrs}) != 1:
        sys.exit(f"{files}: K differs between the files")
    return np.concatenate(arrs) if len(arrs) > 1 else arrs[0]


def near_summary(best, idx, span, self_search):
    best, idx = best.cpu().numpy(), idx.cpu().numpy()
    have = best >= 0
    share = best[have] / span if span else np.ones(have.sum())
    top = np.argsort(-best, kind="stable")[:5]
    return {"rows": int(best.size), "positions": int(span), "against": "the other rows of the set" if self_search else "the reference set",
            "best_match_mean": float(best[have].mean()) if have.any() else None, "best_match_max": int(best.max()) if best.size else None,
            "exact_copies": int((best[have] == span).sum()), "near_copies": int((share >= a.near).sum()), "near_threshold": a.near,
            "closest": [{"row": int(i), "nearest": int(idx[i]), "equal_positions": int(best[i])} for i in top if best[i] >= 0]}


torch.cuda.set_device(a.device)
dev = torch.device("cuda", a.device)
ids = load(a.ids)
N, K = ids.shape
span = (a.k_range[1] - a.k_range[0]) if a.k_range else K
census = TS.TokenCensus(K, a.codes, dev)
for r0 in range(0, N, 1 << 16):                                     # one upload per 65536 rows
    census.update(ids[r0:r0 + (1 << 16)])
out = {"tool": "token_stats", "ids": a.ids, "rows": N, "tokens": K, "dtype": str(ids.dtype), "census": dict(census.summary(), dead_codes=int(census.dead_codes().size))}
if a.census_out:
    census.save(a.census_out)
if a.against:
    other = load(a.against)
    if other.shape != ids.shape:
        sys.exit(f"--against: {other.shape} rows against {ids.shape}")
    r = TS.token_agreement(ids, other, a.k_range)
    nd, first, last = r["n_diff"], r["first_diff"], r["last_diff"]
    differ = nd > 0
    out["agreement"] = {"against": a.against, "positions": r["positions"], "match_rate": r["match_rate"], "rows_equal": r["rows_equal"],
                        "n_diff_mean": float(nd.mean()) if N else None, "n_diff_max": int(nd.max()) if N else None,
                        "first_diff_mean": float(first[differ].mean()) if differ.any() else None, "last_diff_mean": float(last[differ].mean()) if differ.any() else None,
                        "worst_position": int(np.argmin(r["match_rate_pos"])) + (a.k_range[0] if a.k_range else 0) if r["positions"] else None,
                        "worst_position_match_rate": float(r["match_rate_pos"].min()) if r["positions"] else None}
if a.nearest_in:
    ref = load(a.nearest_in)
    out["nearest"] = dict(near_summary(*TS.nearest_sequences(ids, ref, a.k_range), span, False), reference=a.nearest_in, reference_rows=int(ref.shape[0]))
if a.dedup:
    dq = torch.from_numpy(np.ascontiguousarray(ids)).to(dev)
    out["dedup"] = near_summary(*TS.nearest_sequences(dq, dq, a.k_range, exclude_self=True), span, True)
print(json.dumps(out), flush=True)
