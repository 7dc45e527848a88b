"""Reconstruction-quality evaluation of a tokenizer checkpoint: images -> `encoding` -> `decoding` (50-step) and / or
`decoding_with_renderer` -> per-image PSNR against the pre-processed original, batch-sharded over the ranks of a torchrun job.

What it reproduces: the PSNR column of the reference's README table (README.md:89-94, 256 x 256: tokenizer_512_ckpt 21.86 dB / with
renderer 24.14 dB, tokenizer_1024_ckpt 23.06 dB / with renderer 26.30 dB) with the reference's own data flow (test.py:24-43: Resize -> CenterCrop ->
NormalizeToTensor -> encoding -> np.save / np.load -> decoding).  The published weights are not reachable offline; the harness is
pinned instead to the reference pipeline's own run on the synthetic weights (tests/golden/pipeline_b16.npz: psnr_ref of 16 images,
tests/test_eval_gpu.py), so the moment a checkpoint is reachable ONE command gives the README's number:

    python tools/eval_psnr.py --images <dir> --yml-path configs/res256/256-eval.yml --pretrained tokenizer_512_ckpt.pth \\
                              --sd3_pretrained <stable-diffusion-3-medium-diffusers> [--renderer-yml ... --renderer-pretrained ...]
"""
from __future__ import annotations

import os
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import dist as D

IMG_EXT = (".jpg", ".jpeg", ".png", ".bmp", ".webp", ".JPEG", ".JPG", ".PNG")


def list_images(folder: str) -> List[str]:
    """every image file under `folder` (recursive), sorted: the order defines the sharding, so it must be the same on every rank"""
    out = []
    for root, _, files in os.walk(folder):
        out += [os.path.join(root, f) for f in files if f.endswith(IMG_EXT)]
    return sorted(out)


def psnr_each(recon: torch.Tensor, original: torch.Tensor) -> np.ndarray:
    """recon [B,3,H,W] in [0,1] (any float dtype / device), original [B,3,H,W] in [-1,1] -> PSNR in dB per image (fp64 mean of the squared error,
    peak 1.0) -- the arithmetic the reference pipeline run's `psnr_ref` golden was made with"""
    o = (original.detach().float().cpu() + 1.0) / 2.0
    mse = ((recon.detach().float().cpu() - o) ** 2).reshape(o.shape[0], -1).double().mean(dim=1)
    return (10.0 * torch.log10(1.0 / mse)).numpy()


SSIM_DEFINITION = {"window": 11, "sigma": 1.5, "K1": 0.01, "K2": 0.03, "data_range": 1.0, "covariance": "population", "region": "valid"}


def ssim_window() -> np.ndarray:
    """the 11 fp64 weights of the SSIM window: g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised to sum 1 -- the one place they are computed (the device entry
    takes them as an argument, the emulation of the tests calls this)"""
    i = np.arange(SSIM_DEFINITION["window"], dtype=np.float64) - (SSIM_DEFINITION["window"] // 2)
    g = np.exp(-(i * i) / (2.0 * SSIM_DEFINITION["sigma"] ** 2))
    return np.ascontiguousarray(g / g.sum())


def ssim_uniform_window(T: int = 7) -> np.ndarray:
    """the T fp64 weights 1 / T of a uniform T x T window (T odd, 3 .. 11): scipy's uniform_filter, which skimage.metrics.structural_similarity applies by default
    with T = 7"""
    T = int(T)
    if T % 2 == 0 or not 3 <= T <= 11:
        raise ValueError(f"ssim_uniform_window: need an odd T, 3 <= T <= 11, got {T}")
    return np.full(T, 1.0 / T, dtype=np.float64)


def ssim_skimage_definition(signed: bool = True, quantize: bool = False) -> Dict:
    """what "ssim_skimage" computes: skimage.metrics.structural_similarity's defaults (uniform 7 x 7 window, sample covariance, K1 = 0.01, K2 = 0.03), in fp64
    (skimage >= 0.19 computes float32 input in float32; that path is not offered), on [-1, 1] data with data_range 2 or on [0, 1] data with data_range 1"""
    return {"window": 7, "weights": "uniform", "K1": 0.01, "K2": 0.03, "data_range": 2.0 if signed else 1.0, "range": "[-1, 1]" if signed else "[0, 1]",
            "covariance": "sample", "cov_norm": "49/48", "region": "valid", "precision": "float64", "on": "u8" if quantize else "float"}


def psnr_of_mse(mse: np.ndarray) -> np.ndarray:
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(1.0 / np.asarray(mse, dtype=np.float64))


def metrics_each(recon: torch.Tensor, original: torch.Tensor, quantize: bool = False):
    """recon [B,3,H,W] in [0,1], original [B,3,H,W] in [-1,1], both on the GPU (bf16 or fp32) -> (ssim [B], psnr_dB [B]) as numpy fp64, from ONE device call
    (ops.image_metrics: SSIM as SSIM_DEFINITION says, the MSE with psnr_each's operations).  `quantize`: on the bytes save_image would write."""
    from . import ops
    m = ops.image_metrics(recon.detach(), original.detach(), original_signed=True, quantize=quantize).cpu().numpy()
    return m[:, 0].copy(), psnr_of_mse(m[:, 1])


def evaluate(pipe, load_batch: Callable[[int, int], torch.Tensor], n_images: int, batch: int = 64, decoders: Sequence[str] = ("diffusion",),
             noise_fn: Optional[Callable[[int, int], torch.Tensor]] = None, seed: Optional[int] = 1234, renderer_pipe=None, verbose: bool = False,
             metrics: Sequence[str] = ("psnr",), metrics_u8: bool = False, lpips=None, fid=None, ssim_skimage_signed: bool = True) -> Dict:
    """PSNR of `n_images` images through `pipe` (and `renderer_pipe` for the one-step decoder), this rank's contiguous shard of them
    (dist.shard_range) in batches of `batch`; per-image values are gathered to every rank (one all_gather_into_tensor per decoder at the end).
    load_batch(lo, hi) -> float tensor [hi-lo, 3, H, W] in [-1, 1] (host or device).  noise_fn(lo, hi) -> [hi-lo, 16, h, w] replaces the
    reference's `torch.randn` draw (global CPU generator, seeded here with `seed` + rank when given).
    metrics (extension): ("psnr",) is the host route above.  With "ssim" in it both figures come from one device call per batch (ops.image_metrics, no host
    copy of the images, one read of the [n, 2] results at the end): every decoder's dict gains `ssim_mean` / `ssim_each` and the result says which SSIM it is
    (`metric_definition`).  metrics_u8: take both on the bytes `save_image` would write (needs "ssim": the host route has no such mode).
    "lpips" with `lpips=` an lpips.LpipsNet (the weights are not shipped, so there is no default network): the device route as for "ssim", every decoder's dict
    also gains `lpips_mean` / `lpips_each` and `metric_definition["lpips"]` states the definition and where the weights came from; metrics_u8 applies to it too.
    "rfid" with `fid=` a fid.InceptionNet (no default network either): the device route; the pool3 features of the originals (once) and of every decoder's
    reconstructions are collected per batch and gathered like the per-image values, and the statistics are taken of the GATHERED matrices, so the figure does
    not depend on the sharding.  Every decoder's dict gains `rfid`, `rfid_n` and `rfid_rank_deficient` (fewer than 2049 images: the covariances are singular
    and the figure is only comparable at the same N); `metric_definition["rfid"]` states the definition and the weights' source; metrics_u8 applies.
    "precision_recall" with `fid=` likewise: improved precision / recall (genmetrics.GEN_METRICS_DEFINITION, k = 3) on the same gathered pool3 features, the
    originals as the reference set against every decoder's reconstructions; every decoder's dict gains `precision`, `recall` and their integer counts, and
    `metric_definition["precision_recall"]` states the definition.  Needs more than 3 images.
    "ssim_skimage": skimage.metrics.structural_similarity's defaults (ops.image_ssim's "skimage" preset: uniform 7 x 7 window, sample covariance, fp64) on the
    device route; ssim_skimage_signed: on [-1, 1] data with data_range 2 (default) or on [0, 1] data with data_range 1.  Every decoder's dict gains
    `ssim_skimage_mean` / `ssim_skimage_each`, `metric_definition["ssim_skimage"]` states window, moments, range and quantisation; metrics_u8 applies.
    `lpips=` may also be a sequence of LpipsNets of different backbones: each then writes `lpips_<net>_mean` / `lpips_<net>_each` and
    `metric_definition["lpips_<net>"]`; one network given on its own writes the `lpips_*` keys above.
    "tokens" (beside any of the above): adds `token_census`, tokenstats.TokenCensus.summary() of the ids this RANK encoded anyway (code-book usage, perplexity of
    the pooled counts and the reference's 1e-10 form, per-position extremes, dead codes), counted on the device; every other key is what a run without it gives."""
    lpips_nets = None                                        # a sequence of networks: keys by backbone name
    if lpips is not None and not callable(lpips):
        lpips_nets = list(lpips)
        names = [getattr(n, "net", None) for n in lpips_nets]
        if not lpips_nets or None in names or len(set(names)) != len(names):
            raise ValueError(f"lpips=: expected one LpipsNet or a non-empty sequence of LpipsNets of different backbones, got backbones {names}")
    with_lpips = "lpips" in metrics and lpips is not None
    with_sk = "ssim_skimage" in metrics
    with_fid = "rfid" in metrics and fid is not None
    with_pr = "precision_recall" in metrics and fid is not None
    with_tokens = "tokens" in metrics
    bad = [m for m in metrics if m not in ("psnr", "ssim", "ssim_skimage", "tokens") and not (m == "lpips" and with_lpips) and not (m == "rfid" and with_fid) and not (m == "precision_recall" and with_pr)]
    if bad or not metrics:
        raise ValueError(f"metrics {tuple(metrics)!r}: expected a non-empty subset of ('psnr', 'ssim')" + (", or 'lpips' together with lpips=<LpipsNet>" if "lpips" in bad else "")
                         + (", or 'rfid' together with fid=<InceptionNet>" if "rfid" in bad else "")
                         + (", or 'precision_recall' together with fid=<InceptionNet>" if "precision_recall" in bad else ""))
    if with_fid and n_images < 2:
        raise ValueError(f"'rfid' needs at least 2 images (a covariance), got {n_images}")
    if with_pr:
        from . import genmetrics as GM
        if n_images <= GM.K_DEFAULT:
            raise ValueError(f"'precision_recall' needs more than k = {GM.K_DEFAULT} images (a k-th neighbour), got {n_images}")
    with_feats = with_fid or with_pr
    on_device = "ssim" in metrics or with_sk or with_lpips or with_feats
    if metrics_u8 and not on_device:
        raise ValueError("metrics_u8 needs 'ssim' in `metrics` (the device route); the host PSNR route is the float one")
    world, rank = D.world_size(), D.rank()       # the dist module's view: sharding and the gather below must agree
    lo, hi = D.shard_range(n_images, rank, world)
    counts = [D.shard_range(n_images, r, world)[1] - D.shard_range(n_images, r, world)[0] for r in range(world)]
    if seed is not None:
        torch.manual_seed(int(seed) + rank)
    vals = {d: [] for d in decoders}
    extra = {d: {} for d in decoders}            # "ssim_skimage" and the networks of a sequence: key -> fp64 [b] per batch, on the device
    feats = {d: [] for d in decoders}            # "rfid": pool3 features [b, 2048] fp32 per batch, the originals under None
    feats[None] = []
    ids_all = []
    census = None
    for b0 in range(lo, hi, batch):
        b1 = min(b0 + batch, hi)
        imgs = load_batch(b0, b1).to(pipe.device)
        tokens = pipe.encoding(imgs, device=pipe.device)
        ids = tokens.detach().cpu().numpy()                       # the reference round-trips the ids through a host .npy (test.py:38-39)
        ids_all.append(ids)
        if with_tokens:
            if census is None:
                from .tokenstats import TokenCensus
                census = TokenCensus(tokens.shape[-1], int(pipe.model.encoder.codebook.shape[0]), pipe.device)
            census.update(tokens.detach())
        if with_feats:
            feats[None].append(fid.pool3(imgs, signed=True, quantize=metrics_u8))
        for d in decoders:
            if d == "diffusion":
                kw = {} if noise_fn is None else {"noise": noise_fn(b0, b1)}
                rec = pipe.decoding(ids, device=pipe.device, **kw)
            elif d == "renderer":
                rec = (renderer_pipe or pipe).decoding_with_renderer(ids, device=pipe.device)
            else:
                raise ValueError(f"decoder {d!r}: expected 'diffusion' or 'renderer'")
            if on_device:
                from . import ops
                m = ops.image_metrics(rec.detach(), imgs, original_signed=True, quantize=metrics_u8)      # [b, 2] fp64, stays on the device
                if with_lpips and lpips_nets is None:
                    m = torch.cat([m, lpips(rec.detach(), imgs, original_signed=True, quantize=metrics_u8)[:, None]], dim=1)      # [b, 3]
                if with_sk:
                    extra[d].setdefault("ssim_skimage", []).append(ops.image_ssim(rec.detach(), imgs, "skimage", None, ssim_skimage_signed, True, metrics_u8))
                if with_lpips and lpips_nets is not None:
                    for one in lpips_nets:
                        extra[d].setdefault("lpips_" + one.net, []).append(one(rec.detach(), imgs, original_signed=True, quantize=metrics_u8))
                vals[d].append(m)
                if with_feats:
                    feats[d].append(fid.pool3(rec.detach(), signed=False, quantize=metrics_u8))
            else:
                vals[d].append(psnr_each(rec, imgs))
        if verbose and rank == 0:
            so_far = (lambda d: float(psnr_of_mse(torch.cat(vals[d])[:, 1].cpu().numpy()).mean())) if on_device else (lambda d: np.concatenate(vals[d]).mean())
            print(f"[eval] images {b0}..{b1 - 1} of shard {lo}..{hi - 1}: " + ", ".join(f"{d} {so_far(d):.4f} dB so far" for d in decoders), flush=True)
    out = {"images": int(n_images), "ranks": world, "batch": int(batch), "shard": [int(lo), int(hi)]}
    if with_feats:
        from . import fid as FD
        held = {}                                                 # every feature matrix is gathered ONCE, whichever figures read it

        def gathered(key):
            if key not in held:
                held[key] = D.all_gather_rows(torch.cat(feats[key]) if feats[key] else torch.zeros(0, FD.FEATURES, dtype=torch.float32, device=pipe.device), counts)
            return held[key]
    if with_fid:
        mu0, sigma0 = (t.cpu().numpy() for t in FD.statistics(gathered(None)))
    for d in decoders:
        if on_device:
            mine = torch.cat(vals[d]) if vals[d] else torch.zeros(0, 3 if with_lpips and lpips_nets is None else 2, dtype=torch.float64, device=pipe.device)
            allv = D.all_gather_rows(mine, counts).cpu().numpy()
            ssim, psnr = allv[:, 0], psnr_of_mse(allv[:, 1])
            out[d] = {"psnr_mean_dB": float(psnr.mean()) if psnr.size else float("nan"), "psnr_each_dB": [round(float(v), 6) for v in psnr],
                      "ssim_mean": float(ssim.mean()) if ssim.size else float("nan"), "ssim_each": [round(float(v), 9) for v in ssim]}
            if with_lpips and lpips_nets is None:
                out[d].update({"lpips_mean": float(allv[:, 2].mean()) if ssim.size else float("nan"), "lpips_each": [round(float(v), 9) for v in allv[:, 2]]})
            for key in (["ssim_skimage"] if with_sk else []) + (["lpips_" + one.net for one in lpips_nets] if with_lpips and lpips_nets is not None else []):
                col = extra[d].get(key, [])
                v = D.all_gather_rows((torch.cat(col) if col else torch.zeros(0, dtype=torch.float64, device=pipe.device))[:, None], counts).cpu().numpy()[:, 0]
                out[d].update({key + "_mean": float(v.mean()) if v.size else float("nan"), key + "_each": [round(float(x), 9) for x in v]})
            if with_fid:
                out[d].update({"rfid": FD.frechet_distance(*FD.statistics(gathered(d)), mu0, sigma0), "rfid_n": int(n_images), "rfid_rank_deficient": n_images <= FD.FEATURES})
            if with_pr:
                out[d].update({k: v for k, v in GM.precision_recall(gathered(None), gathered(d)).items() if k not in ("n_ref", "n_gen", "k")})
            continue
        mine = torch.from_numpy(np.concatenate(vals[d]) if vals[d] else np.zeros(0)).to(torch.float64)
        allv = D.all_gather_rows(mine.to(pipe.device), counts).cpu().numpy()      # returns `mine` when there is no exchange to perform
        out[d] = {"psnr_mean_dB": float(allv.mean()) if allv.size else float("nan"), "psnr_each_dB": [round(float(v), 6) for v in allv]}
    if on_device:
        out["metric_definition"] = dict(SSIM_DEFINITION, on="u8" if metrics_u8 else "float")
        if with_sk:
            out["metric_definition"]["ssim_skimage"] = ssim_skimage_definition(ssim_skimage_signed, metrics_u8)
        if with_lpips and lpips_nets is None:
            from .lpips import LPIPS_DEFINITION
            out["metric_definition"]["lpips"] = dict(getattr(lpips, "definition", LPIPS_DEFINITION), weights=lpips.source)
        elif with_lpips:
            for one in lpips_nets:
                out["metric_definition"]["lpips_" + one.net] = dict(one.definition, weights=one.source)
        if with_fid:
            out["metric_definition"]["rfid"] = dict(FD.FID_DEFINITION, weights=fid.source, resized=bool(fid.resize))
        if with_pr:
            out["metric_definition"]["precision_recall"] = dict(GM.GEN_METRICS_DEFINITION, weights=fid.source, resized=bool(fid.resize), n=int(n_images))
    out["token_ids_first_image"] = ids_all[0][0, :8].tolist() if ids_all else []
    if census is not None:
        out["token_census"] = dict(census.summary(), dead_codes=int(census.dead_codes().size), shard=[int(lo), int(hi)])
    return out


def folder_loader(paths: Sequence[str], size: int, device=None, preprocess: str = "reference") -> Callable[[int, int], torch.Tensor]:
    """load_batch for `evaluate`.  Default: `preprocess.load_image` per file on the host.  With a `device` (extension): the files are only
    decoded on the host and the resize / crop / normalise runs on that GPU (preprocess.DeviceLoader) -- the same fp32 values, bit for bit,
    already on the device (the PSNR is taken against them, so they stay fp32; `encoding` rounds to bf16 itself).
    preprocess: "reference" (load_image), "bicubic" (load_image(filter="bicubic")) or "adm" (load_image_adm), by either route."""
    from . import preprocess as P
    P._check_preprocess(preprocess)
    if device is not None:
        loader = P.DeviceLoader(size, device, dtype=torch.float32) if preprocess == "reference" else P.DeviceLoader(size, device, dtype=torch.float32, preprocess=preprocess)
        return lambda lo, hi: loader.load(paths[lo:hi])

    def load(lo: int, hi: int) -> torch.Tensor:
        if preprocess == "adm":
            return torch.stack([P.load_image_adm(p, size) for p in paths[lo:hi]])
        if preprocess == "bicubic":
            return torch.stack([P.load_image(p, size, filter="bicubic") for p in paths[lo:hi]])
        return torch.stack([P.load_image(p, size) for p in paths[lo:hi]])
    return load


COMPARE_METRICS = ("fid", "is", "precision", "recall")
COMPARE_METRICS_EXTRA = ("kid", "density", "coverage")


def compare_sets(load_ref: Callable[[int, int], torch.Tensor], n_ref: int, load_gen: Callable[[int, int], torch.Tensor], n_gen: int, fid=None,
                 metrics: Sequence[str] = COMPARE_METRICS, batch: int = 64, k: Optional[int] = None, split_size: Optional[int] = None, device=None,
                 kid_subsets: Optional[int] = None, kid_subset_size: Optional[int] = None, kid_seed: Optional[int] = None, nearest: bool = False) -> Dict:
    """Two image sets against each other, the figures of the ADM / LlamaGen protocol that this project defines: FID, Inception Score (of the generated set),
    improved precision and recall.  load_ref(lo, hi) / load_gen(lo, hi) -> float tensor [hi - lo, 3, H, W] in [-1, 1] (host or device; load_gen may decode
    token ids through a pipeline); each rank walks its contiguous shard (dist.shard_range) of either set in batches of `batch`, the pool3 features (and, for
    "is", the fc logits) are gathered to every rank and every figure is taken of the GATHERED matrices, so it does not depend on the sharding or the batch.
    `fid`: a fid.InceptionNet (no default network: the weights are not shipped), built with logits=True when "is" is asked for.  k: neighbours of
    precision / recall (default 3); split_size: rows per Inception Score split (default 5000).
    COMPARE_METRICS_EXTRA, on the same gathered features (genmetrics.GEN_METRICS_DEFINITION): "kid" (kid_subsets subsets of kid_subset_size rows drawn with
    kid_seed, defaults 100 x 1000, seed 2020: the unbiased figure for sets too small for FID) gives `kid`, `kid_std` and the three parameters; "density" and
    "coverage" give the fractions and `density_count` / `coverage_count`, with the k and the reference radii of precision (computed once per call; asked for
    together with density, precision is count > 0, the membership entry's bits).  nearest=True: out["nearest"] = {"index", "d2"}, for every generated image
    its nearest reference image by squared pool3 distance."""
    from . import fid as FD, genmetrics as GM
    metrics = tuple(metrics)
    bad = [m for m in metrics if m not in COMPARE_METRICS + COMPARE_METRICS_EXTRA]
    if bad or not metrics:
        raise ValueError(f"metrics {metrics!r}: expected a non-empty subset of {COMPARE_METRICS + COMPARE_METRICS_EXTRA}")
    if fid is None:
        raise ValueError("compare_sets needs fid=<InceptionNet> (the weights are not shipped, so there is no default network)")
    k = GM.K_DEFAULT if k is None else int(k)
    split_size = GM.SPLIT_SIZE if split_size is None else int(split_size)
    with_is, with_pr = "is" in metrics, "precision" in metrics or "recall" in metrics
    with_kid, with_dc = "kid" in metrics, "density" in metrics or "coverage" in metrics
    kid_subsets = GM.KID_SUBSETS if kid_subsets is None else int(kid_subsets)
    kid_subset_size = GM.KID_SUBSET_SIZE if kid_subset_size is None else int(kid_subset_size)
    kid_seed = GM.KID_SEED if kid_seed is None else int(kid_seed)
    if with_kid and (kid_subsets < 1 or kid_subset_size < 2 or kid_subset_size > min(n_ref, n_gen)):
        raise ValueError(f"'kid' needs kid_subsets >= 1 and 2 <= kid_subset_size <= min(n_ref, n_gen), got {kid_subsets} subsets of {kid_subset_size} rows, "
                         f"{n_ref} and {n_gen} images")
    if with_dc and (n_ref <= k or not 1 <= k <= GM.K_MAX):
        raise ValueError(f"'density' / 'coverage' need 1 <= k <= {GM.K_MAX} and more than k reference images, got k {k}, {n_ref} images")
    if with_is and fid.fc_packed is None:
        raise ValueError("compare_sets: 'is' needs a network built with logits=True")
    if "fid" in metrics and min(n_ref, n_gen) < 2:
        raise ValueError(f"'fid' needs at least 2 images per set (a covariance), got {n_ref} and {n_gen}")
    if with_pr and (min(n_ref, n_gen) <= k or not 1 <= k <= GM.K_MAX):
        raise ValueError(f"'precision' / 'recall' need 1 <= k <= {GM.K_MAX} and more than k images per set, got k {k}, {n_ref} and {n_gen} images")
    if n_gen < 1 or n_ref < 1 or split_size < 1 or batch < 1:
        raise ValueError(f"compare_sets: need n_ref, n_gen, batch, split_size >= 1, got {n_ref}, {n_gen}, {batch}, {split_size}")
    device = fid.device if device is None else torch.device(device)
    world, rank = D.world_size(), D.rank()

    def walk(load, n, want_logits):
        lo, hi = D.shard_range(n, rank, world)
        counts = [D.shard_range(n, r, world)[1] - D.shard_range(n, r, world)[0] for r in range(world)]
        f, lg = [], []
        for b0 in range(lo, hi, batch):
            b1 = min(b0 + batch, hi)
            f.append(fid.pool3(load(b0, b1).to(device), signed=True))
            if want_logits:
                lg.append(fid.logits(f[-1]))
        cat = lambda ts, width: D.all_gather_rows(torch.cat(ts) if ts else torch.zeros(0, width, dtype=torch.float32, device=device), counts)
        return cat(f, FD.FEATURES), (cat(lg, FD.CLASSES) if want_logits else None)

    fr, _ = walk(load_ref, n_ref, False)
    fg, lg = walk(load_gen, n_gen, with_is)
    out = {"n_ref": int(n_ref), "n_gen": int(n_gen), "ranks": world, "batch": int(batch)}
    definition = {"weights": fid.source, "resized": bool(fid.resize)}
    if "fid" in metrics:
        out["fid"] = FD.frechet_distance(*FD.statistics(fg), *FD.statistics(fr))
        out["fid_rank_deficient"] = min(n_ref, n_gen) <= FD.FEATURES
        definition["fid"] = FD.FID_DEFINITION
    if with_is:
        out["is"] = GM.inception_score(lg, split_size)
        out["split_size"] = split_size
    if with_pr and not with_dc:
        pr = GM.precision_recall(fr, fg, k)
        out.update({key: v for key, v in pr.items() if key.split("_")[0] in metrics or key == "k"})
    nn = None
    if with_dc:                                                   # one set of reference radii serves precision, density and coverage
        r2_ref = GM.knn_radii(fr, k)
        pr = {}
        if "density" in metrics:
            count, nn_d2, nn_idx = GM.ball_counts(fg, fr, r2_ref)
            nn = (nn_idx, nn_d2)
            dc = int(count.sum(dtype=torch.int64).item())
            pr.update({"density": dc / (k * n_gen), "density_count": dc})
            if "precision" in metrics:                            # count > 0 is the membership entry bit for bit
                pc = int((count > 0).sum().item())
                pr.update({"precision": pc / n_gen, "precision_count": pc})
        elif "precision" in metrics:
            pc = int(GM.manifold_members(fg, fr, r2_ref).sum().item())
            pr.update({"precision": pc / n_gen, "precision_count": pc})
        if "recall" in metrics:
            rc = int(GM.manifold_members(fr, fg, GM.knn_radii(fg, k)).sum().item())
            pr.update({"recall": rc / n_ref, "recall_count": rc})
        if "coverage" in metrics:
            cc = GM.coverage_count(fr, fg, r2_ref)
            pr.update({"coverage": cc / n_ref, "coverage_count": cc})
        order = ("precision", "recall", "density", "coverage", "precision_count", "recall_count", "density_count", "coverage_count")
        out.update({key: pr[key] for key in order if key in pr})
        out["k"] = k
    if with_kid:
        out.update(GM.kid(fr, fg, kid_subsets, kid_subset_size, kid_seed))
    if nearest:
        nn_idx, nn_d2 = GM.nearest_neighbours(fg, fr) if nn is None else nn
        out["nearest"] = {"index": [int(v) for v in nn_idx.cpu().numpy()], "d2": [float(v) for v in nn_d2.cpu().numpy()]}
    if with_is or with_pr or with_dc or with_kid or nearest:
        definition["gen_metrics"] = GM.GEN_METRICS_DEFINITION
    out["metric_definition"] = definition
    return out


def index_noise(seed: int, latent: int = 32) -> Callable[[int, int], torch.Tensor]:
    """noise_fn(lo, hi) -> [hi - lo, 16, latent, latent]: the decode-start noise of item i comes from a CPU generator seeded `seed + i`, so what item i decodes
    to depends on neither the batch nor the sharding (the global generator `evaluate` seeds with seed + rank does)"""
    return lambda lo, hi: torch.stack([torch.randn(16, latent, latent, generator=torch.Generator().manual_seed(int(seed) + i)) for i in range(lo, hi)]) \
        if hi > lo else torch.zeros(0, 16, latent, latent)


def npz_loader(path: str, key: str = "arr_0") -> "tuple[Callable[[int, int], torch.Tensor], int]":
    """(load_batch, n) over an ADM-style sample file: an .npz whose `arr_0` is uint8 [N, H, W, 3] -> float32 [b, 3, H, W] in [-1, 1], byte / 127.5 - 1 (the
    NormalizeToTensor expression of the folder route)"""
    with np.load(path) as z:
        if key not in z:
            raise KeyError(f"{path}: key {key!r} is missing")
        arr = np.asarray(z[key])
    if arr.dtype != np.uint8 or arr.ndim != 4 or arr.shape[3] != 3:
        raise ValueError(f"{path}: expected uint8 [N, H, W, 3], got {arr.dtype} {arr.shape}")
    return (lambda lo, hi: torch.from_numpy(arr[lo:hi]).permute(0, 3, 1, 2).float() / 127.5 - 1.0), int(arr.shape[0])
