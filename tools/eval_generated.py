"""FID, Inception Score, improved precision and recall of a set of generated images against a reference set, on MI355X (selftoktokenizer_amd/evaluate.py:
compare_sets; genmetrics.GEN_METRICS_DEFINITION and fid.FID_DEFINITION state the figures).  Sharded over ranks when launched under torchrun.

    python tools/eval_generated.py --ref <dir | ref.npz> --samples <dir | samples.npz> --fid-weights pt_inception-2015-12-05.pth
    python tools/eval_generated.py --ref <dir | ref.npz> --tokens ids.npy --yml-path configs/res256/256-eval.yml --pretrained tokenizer_512_ckpt.pth \\
                                   --sd3_pretrained <sd3 dir> --fid-weights pt_inception-2015-12-05.pth      # decode AR token ids first
    python tools/eval_generated.py --ref a.npz --samples b.npz --synthetic                                   # hash-generated InceptionV3: no weights reachable

With --tokens sequence i is decoded from the noise of a generator seeded --seed + i (evaluate.index_noise): the images do not depend on the sharding.  They are
the same bits for every batch size only with --gemm exact; the default fp32 sampler is not bit-reproducible across batch shapes.
--ref / --samples: a folder of image files (searched recursively, sorted, pre-processed to --data_size like eval_psnr.py) or an ADM-style .npz whose arr_0
is uint8 [N, H, W, 3].  Prints ONE JSON object on rank 0.  The figures are those of the published definitions on the weights given; nothing here is pinned
against the ADM evaluator (unpinned), and sFID is not offered (genmetrics.py says why).
--metrics also takes kid, density and coverage (evaluate.COMPARE_METRICS_EXTRA; unpinned against torch-fidelity and prdc): KID is the unbiased figure for sets
of a few thousand images, where FID is biased.  --nn-out FILE.npz writes, for every generated image, the index of its nearest reference image and the squared
pool3 distance to it (`index`, `d2`), and keeps both out of the JSON object."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from selftoktokenizer_amd import dist as D, evaluate as E, genmetrics as GM
from selftoktokenizer_amd.fid import InceptionNet

ap = argparse.ArgumentParser()
ap.add_argument("--ref", required=True, help="reference images: a folder or an .npz (arr_0 uint8 [N, H, W, 3])")
ap.add_argument("--samples", default=None, help="generated images: a folder or an .npz")
ap.add_argument("--tokens", default=None, help="ids.npy [N, K] of generated token ids: decoded through the checkpoint below instead of --samples")
ap.add_argument("--synthetic", action="store_true", help="hash-generated InceptionV3 (and, with --tokens, tokenizer) weights: the published definitions on synthetic weights")
ap.add_argument("--fid-weights", default=None, help="pytorch-fid's pt_inception-2015-12-05 state dict, with fc.weight / fc.bias for the Inception Score")
ap.add_argument("--k", type=int, default=GM.K_DEFAULT, help="neighbours of precision / recall")
ap.add_argument("--split-size", type=int, default=GM.SPLIT_SIZE, help="rows per Inception Score split")
ap.add_argument("--metrics", default=",".join(E.COMPARE_METRICS), help="any of " + ", ".join(E.COMPARE_METRICS + E.COMPARE_METRICS_EXTRA))
ap.add_argument("--kid-subsets", type=int, default=GM.KID_SUBSETS, help="subsets of the KID estimate")
ap.add_argument("--kid-subset-size", type=int, default=GM.KID_SUBSET_SIZE, help="rows of either set per KID subset")
ap.add_argument("--kid-seed", type=int, default=GM.KID_SEED, help="seed of the KID subset draw")
ap.add_argument("--nn-out", default=None, help="FILE.npz: the nearest reference image of every generated image (index, d2), rank 0")
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--data_size", type=int, default=256)
ap.add_argument("--preprocess", default="adm", choices=["reference", "bicubic", "adm"], help="how files of a folder become data_size x data_size images")
ap.add_argument("--no-resize", action="store_true", help="feed the images to the network as they are (>= 75 x 75) instead of resizing to 299 x 299")
ap.add_argument("--yml-path", default=None)
ap.add_argument("--pretrained", default=None)
ap.add_argument("--sd3_pretrained", default=None)
ap.add_argument("--gemm", default=None, choices=["fp32", "f16x2", "exact", "f16"])
ap.add_argument("--seed", type=int, default=1234, help="with --tokens: sequence i is decoded from the noise of a generator seeded seed + i")
ap.add_argument("--out", default=None, help="also write the JSON object to this file (rank 0)")
a = ap.parse_args()
if (a.samples is None) == (a.tokens is None):
    ap.error("exactly one of --samples and --tokens")
if not a.fid_weights and not a.synthetic:
    ap.error("--fid-weights FILE, or --synthetic: the published InceptionV3 weights are not shipped")

rank, world, local = D.init_from_env()
torch.cuda.set_device(local)
dev = torch.device("cuda", local)
metrics = tuple(m for m in a.metrics.split(",") if m)
net = InceptionNet.from_files(a.fid_weights, dev, logits="is" in metrics) if a.fid_weights else InceptionNet.synthetic(dev, logits="is" in metrics)
net.resize = not a.no_resize


def image_set(path):
    if path.endswith(".npz"):
        load, n = E.npz_loader(path)
        return load, n, f"{n} images of {path}"
    paths = E.list_images(path)
    assert paths, f"no image files under {path}"
    return E.folder_loader(paths, a.data_size, preprocess=a.preprocess), len(paths), f"{len(paths)} files under {path}"


load_ref, n_ref, src_ref = image_set(a.ref)
if a.tokens:
    from mimogpt.infer.infer_utils import parse_args_from_yaml
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    from selftoktokenizer_amd import weights as W
    from selftoktokenizer_amd.config import default_config
    cfg = parse_args_from_yaml(a.yml_path) if a.yml_path else default_config(512)
    kw = {}
    if a.pretrained is None:
        if not a.synthetic:
            ap.error("--tokens needs --pretrained (and --yml-path / --sd3_pretrained), or --synthetic")
        kw = dict(state_dict=W.synthetic_state_dict(W.expected_shapes(int(cfg.tokenizer.params.k)), device=dev), vae_state_dict=W.synthetic_vae_state_dict(device=dev))
    pipe = SelftokPipeline(cfg=cfg, ckpt_path=a.pretrained, sd3_path=a.sd3_pretrained, datasize=a.data_size, device=dev, gemm=a.gemm, verbose=False, **kw)
    ids = np.load(a.tokens)
    assert ids.ndim == 2, f"{a.tokens}: expected token ids [N, K], got {ids.shape}"
    noise = E.index_noise(a.seed, a.data_size // 8)             # per sequence index: the decoded images, and so every figure, do not depend on the sharding
    load_gen = lambda lo, hi: pipe.decoding(ids[lo:hi], device=dev, noise=noise(lo, hi)).float() * 2.0 - 1.0      # decoding returns [0, 1]
    n_gen, src_gen = int(ids.shape[0]), f"{ids.shape[0]} token sequences of {a.tokens}, decoded"
else:
    load_gen, n_gen, src_gen = image_set(a.samples)

res = E.compare_sets(load_ref, n_ref, load_gen, n_gen, fid=net, metrics=metrics, batch=a.batch, k=a.k, split_size=a.split_size, device=dev,
                     kid_subsets=a.kid_subsets, kid_subset_size=a.kid_subset_size, kid_seed=a.kid_seed, nearest=a.nn_out is not None)
D.barrier()
nn = res.pop("nearest", None)
if rank == 0:
    if a.nn_out:
        np.savez(a.nn_out, index=np.asarray(nn["index"], np.int32), d2=np.asarray(nn["d2"], np.float32))
        res["nn_out"] = a.nn_out
    line = {"tool": "eval_generated", "ref": src_ref, "samples": src_gen, "fid_weights": net.source, "pinned": GM.GEN_METRICS_DEFINITION["pinned"], **res}
    print(json.dumps(line), flush=True)
    if a.out:
        open(a.out, "w").write(json.dumps(line) + "\n")
D.shutdown()
