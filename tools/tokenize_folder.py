"""Tokenise an image folder on MI355X: files -> host decode (thread pool) -> pinned staging -> one H2D copy -> resize / crop / normalise on the
GPU (csrc/image_io.hip, the reference's PIL arithmetic bit for bit) -> `encoding` -> token ids.  Sharded over ranks under torchrun.

    python tools/tokenize_folder.py --images <dir> --yml-path configs/res256/256-eval.yml --pretrained tokenizer_512_ckpt.pth --sd3_pretrained <sd3 dir> --out ids
    python tools/tokenize_folder.py --synthetic 256 --out /tmp/ids          # hash-generated weights and mixed-size uint8 images

Every rank writes <out>.rank<r>.npy (int64 [n, K], what the reference script saves; --uint16 for the compact wire format) and rank 0 prints
ONE JSON line: images/s and where the time went (host decode, pack, H2D copy, resize kernels, encode).  --topk k also writes
<out>.rank<r>.topk.npz (`ids` uint16 [n, K, k]: the k best codes of every token, best first; `scores` fp32 [n, K, k]: their exact cosine scores)
and, for k >= 2, adds the near-tie census of the top-1 / top-2 margins to the JSON line; the .npy is the same bytes with and without it.

Augmented runs: --crops five | ten takes torchvision's FiveCrop / TenCrop(data_size) of the image resized to --resize R (shorter side, default
data_size), --flip adds the mirror image of every view; each view is the tensor torchvision gives on the PIL image, bit for bit
(csrc/image_views.hip, every file still crosses to the GPU once).  With more than one view per image the id file is int64 [n, views, K] (and the
top-k arrays [n, views, K, k]), views in torchvision's order, and the JSON line names the recipe; --batch counts images, not views.

--stats adds `token_census` to the JSON line (selftoktokenizer_amd.tokenstats.TokenCensus of this rank's ids: code-book usage, perplexity, dead codes)
and, with more than one view per image, `view_agreement`: every view against view 0 (match rate, mean number of differing positions).  Both accumulate
on the device, one read at the end; the id files are the same bytes with and without it."""
import argparse, json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mimogpt.infer.infer_utils import parse_args_from_yaml
from mimogpt.infer.SelftokPipeline import SelftokPipeline
from selftoktokenizer_amd import dist as D, evaluate as E, ops, preprocess, synth, tokens, tokenstats, weights as W
from selftoktokenizer_amd.config import default_config

ap = argparse.ArgumentParser()
ap.add_argument("--images", default=None, help="folder of images (searched recursively, sorted)")
ap.add_argument("--synthetic", type=int, default=0, help="N hash-generated mixed-size uint8 images + synthetic weights instead of files")
ap.add_argument("--limit", type=int, default=0)
ap.add_argument("--yml-path", default=None)
ap.add_argument("--pretrained", default=None)
ap.add_argument("--sd3_pretrained", default=None)
ap.add_argument("--data_size", type=int, default=256)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--workers", type=int, default=8, help="host decode threads (at most 16)")
ap.add_argument("--encoder-mode", default=None, choices=["exact", "fast"])
ap.add_argument("--vae-mode", default=None, choices=["exact", "parity", "fast", "miopen"])
ap.add_argument("--uint16", action="store_true", help="write tokens.to_uint16 ids instead of the reference's int64")
ap.add_argument("--topk", type=int, default=0, help="k in 1..8: also keep every token's k best codes and their scores (SelftokPipeline.encoding_topk); the margin census needs k >= 2")
ap.add_argument("--crops", default="center", choices=["center", "five", "ten"], help="views per image: the centre crop, FiveCrop or TenCrop of the resized image")
ap.add_argument("--resize", type=int, default=0, help="R >= data_size: shorter side of the resize before the crops (default: data_size)")
ap.add_argument("--flip", action="store_true", help="also emit the mirror image of every view")
ap.add_argument("--preprocess", default="reference", choices=["reference", "bicubic", "adm"], help="the reference's bilinear Resize; bicubic Resize (the views likewise); or the ADM protocol center_crop_arr, which is one centre crop per image (no --crops / --resize / --flip)")
ap.add_argument("--stats", action="store_true", help="add the code census of the ids (usage, perplexity) and, with several views per image, their agreement with view 0 to the JSON line")
ap.add_argument("--out", default=None, help="prefix of the id files; nothing is written without it")
a = ap.parse_args()
if not 0 <= a.topk <= 8:
    ap.error("--topk k: 1 <= k <= 8")
R = a.resize or a.data_size
if R < a.data_size:
    ap.error(f"--resize {R}: must be >= --data_size {a.data_size}")
views, nviews = None, 1                # None: the centre crop of Resize(data_size), the route without views
if a.crops != "center" or a.flip or R != a.data_size:
    S = a.data_size
    base = {"center": lambda w, h: [preprocess.views_five(w, h, R, S)[4]], "five": lambda w, h: preprocess.views_five(w, h, R, S),
            "ten": lambda w, h: preprocess.views_ten(w, h, R, S)}[a.crops]
    views = (lambda w, h: preprocess.mirrored(base(w, h))) if a.flip else base
    nviews = {"center": 1, "five": 5, "ten": 10}[a.crops] * (2 if a.flip else 1)
if views and a.preprocess == "adm":
    ap.error("--preprocess adm is one centre crop per image: it takes no --crops, --resize or --flip")

rank, world, local = D.init_from_env()
torch.cuda.set_device(local)
dev = torch.device("cuda", local)
cfg = parse_args_from_yaml(a.yml_path) if a.yml_path else default_config(512)
K = int(cfg.tokenizer.params.k)
kw = {}
if a.pretrained is None:
    kw = dict(state_dict=W.synthetic_state_dict(W.expected_shapes(K), device=dev), vae_state_dict=W.synthetic_vae_state_dict(device=dev))
pipe = SelftokPipeline(cfg=cfg, ckpt_path=a.pretrained, sd3_path=a.sd3_pretrained, datasize=a.data_size, device=dev, verbose=False,
                       encoder_mode=a.encoder_mode, vae_mode=a.vae_mode, **kw)
if a.synthetic:
    n, src = a.synthetic, f"{a.synthetic} hash-generated uint8 images (selftoktokenizer_amd.synth)"
    lo, hi = D.shard_range(n, rank, world)
    items = synth.synthetic_u8_images(hi - lo, first_index=lo)
else:
    assert a.images, "--images <dir> or --synthetic N"
    paths = E.list_images(a.images)
    paths = paths[:a.limit] if a.limit else paths
    assert paths, f"no image files under {a.images}"
    n, src = len(paths), f"{len(paths)} files under {a.images}"
    lo, hi = D.shard_range(n, rank, world)
    items = paths[lo:hi]

loader = preprocess.DeviceLoader(a.data_size, dev, dtype=torch.bfloat16, workers=a.workers, preprocess=a.preprocess)
loader.timing = True
topk_ids, topk_scores = [], []
census = tokenstats.TokenCensus(K, int(pipe.model.encoder.codebook.shape[0]), dev) if a.stats else None
view_match = torch.zeros(K, dtype=torch.int32, device=dev)           # rows of views 1.. that agree with view 0, per position
view_diff = torch.zeros(1, dtype=torch.int64, device=dev)            # differing positions over those rows
ids, split, marks = [], {"host_decode_s": 0.0, "pack_s": 0.0, "h2d_ms": 0.0, "resize_kernels_ms": 0.0, "encode_ms": 0.0}, []
torch.cuda.synchronize()
t0 = time.perf_counter()
for batch in (loader.batches(items, a.batch, views=views) if views else loader.batches(items, a.batch)):
    ev, lt = loader.last_events, loader.last_times
    e3 = torch.cuda.Event(enable_timing=True)
    if a.topk:
        tk_ids, tk_scores = pipe.encoding_topk(batch, k=a.topk, device=dev)
        tok = tk_ids[..., 0]
    else:
        tok = pipe.encoding(batch, device=dev)
    e3.record()
    marks.append(ev + (e3,))
    if a.stats:                                                      # after the encode mark: on the device, nothing read back
        census.update(tok)
        if nviews > 1:
            t3 = tok.reshape(-1, nviews, K)
            first = ops.token_to_u16(t3[:, :1].expand(-1, nviews - 1, -1).reshape(-1, K))
            rest = ops.token_to_u16(t3[:, 1:].reshape(-1, K))
            view_diff += ops.token_agree(first, rest, match_pos=view_match)[1].sum()
    split["host_decode_s"] += lt["decode_s"]; split["pack_s"] += lt["pack_s"]
    ids.append(tok.cpu().numpy())
    if a.topk:
        topk_ids.append(tk_ids.cpu().numpy()); topk_scores.append(tk_scores.cpu().numpy())
torch.cuda.synchronize()
wall = time.perf_counter() - t0
for e0, e1, e2, e3 in marks:
    split["h2d_ms"] += e0.elapsed_time(e1); split["resize_kernels_ms"] += e1.elapsed_time(e2); split["encode_ms"] += e2.elapsed_time(e3)
loader.close()
ids = np.concatenate(ids) if ids else np.zeros((0, K), np.int64)
if nviews > 1:
    ids = ids.reshape(-1, nviews, K)
if a.out:
    f = f"{a.out}.rank{rank}.npy"
    np.save(f, tokens.to_uint16(ids)) if a.uint16 else tokens.save_reference_npy(f, ids)
extra = {}
if a.topk:
    topk_ids = np.concatenate(topk_ids) if topk_ids else np.zeros((0, K, a.topk), np.int64)
    topk_scores = np.concatenate(topk_scores) if topk_scores else np.zeros((0, K, a.topk), np.float32)
    if nviews > 1:
        topk_ids, topk_scores = topk_ids.reshape(-1, nviews, K, a.topk), topk_scores.reshape(-1, nviews, K, a.topk)
    if a.out:
        np.savez(f"{a.out}.rank{rank}.topk.npz", ids=tokens.to_uint16(topk_ids), scores=topk_scores)
    extra = {"topk": a.topk}
    if a.topk >= 2:                  # the margin needs the runner-up
        m = tokens.margins(topk_scores)
        extra.update({"rank0_margin_below_1e-5": int((m < 1e-5).sum()), "rank0_margin_below_1e-4": int((m < 1e-4).sum()),
                      "rank0_min_margin": float(m.min()) if m.size else None})
if views:
    extra.update({"crops": a.crops, "resize": R, "flip": bool(a.flip), "views_per_image": nviews, "views": n * nviews,
                  "recipe": f"Resize({R}) -> {dict(center='CenterCrop', five='FiveCrop', ten='TenCrop')[a.crops]}({a.data_size})" + (" + mirror images" if a.flip else "")})
if a.stats:
    extra["rank0_token_census"] = census.summary()
    extra["rank0_token_census"]["dead_codes"] = int(census.dead_codes().size)
    if a.out:
        census.save(f"{a.out}.rank{rank}.census.npz")               # ranks combine offline: TokenCensus.load(...).merge(...)
    if nviews > 1:
        rows = int(ids.shape[0]) * (nviews - 1)
        match = int(view_match.cpu().numpy().view(np.uint32).astype(np.int64).sum())
        extra["rank0_view_agreement"] = {"against": "view 0", "rows": rows, "match_rate": match / (rows * K) if rows else None,
                                         "mean_n_diff": int(view_diff.item()) / rows if rows else None}
slowest = D.max_over_ranks(wall, dev)
D.barrier()
if rank == 0:
    print(json.dumps({"tool": "tokenize_folder", "source": src, "images": n, "ranks": world, "batch": a.batch, "workers": loader.workers, "tokens": K,
                      "data_size": a.data_size, "preprocess": a.preprocess, "vae": pipe.vae.mode, "encoder": pipe.model.encoder.mode, "wall_s": round(slowest, 4),
                      "images_per_s": round(n / slowest, 2) if slowest > 0 else None,
                      "rank0_split": {k: round(v, 4) for k, v in split.items()}, "rank0_shard": [lo, hi],
                      **extra,
                      "note": "host decode / pack of batch i + 1 overlap the GPU work of batch i, so the parts do not add up to wall_s"}), flush=True)
D.shutdown()
