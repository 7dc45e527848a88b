"""Reconstruction PSNR of a Selftok tokenizer checkpoint over an image folder, on MI355X (one command = the PSNR column of the reference's
README.md:89-94; see selftoktokenizer_amd/evaluate.py).  Sharded over ranks when launched under torchrun:

    python tools/eval_psnr.py --images <dir> --yml-path configs/res256/256-eval.yml --pretrained tokenizer_512_ckpt.pth --sd3_pretrained <sd3 dir>
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 tools/eval_psnr.py --images <dir> ... --renderer-yml configs/renderer/renderer-eval.yml --renderer-pretrained renderer_512_ckpt.pth
    python tools/eval_psnr.py --synthetic 16          # no checkpoint reachable: hash-generated weights / images / noise = the reference pipeline's golden run

Prints ONE JSON line on rank 0: per-image and mean PSNR for the 50-step `decoding` and, when a renderer checkpoint is given, `decoding_with_renderer`;
with --ssim also `ssim_mean` / `ssim_each` (the SSIM column of the reference's results table), computed on the GPU together with the PSNR;
with --lpips-backbone FILE --lpips-linear FILE (torchvision's AlexNet state dict and the lpips package's v0.1 alex.pth) also `lpips_mean` / `lpips_each`
(selftoktokenizer_amd/lpips.py).  `--lpips` alone is accepted with --synthetic only: the hash-generated LPIPS network, labelled "synthetic" in the line;
with --fid-weights FILE (pytorch-fid's pt_inception-2015-12-05 state dict) also `rfid` per decoder (selftoktokenizer_amd/fid.py: InceptionV3 pool3 features
and the fp64 statistics on the GPU, the Frechet distance on the host); `--fid` alone, like `--lpips`, with --synthetic only;
with --ssim-skimage [--ssim-range signed|unsigned] also `ssim_skimage_mean` / `ssim_skimage_each`: skimage.metrics.structural_similarity's defaults (uniform
7 x 7 window, sample covariance) in fp64, on [-1, 1] data with data_range 2 (signed, the default) or on [0, 1] data;
with --lpips-vgg BACKBONE.pth LINEAR.pth (torchvision's vgg16 state dict and the lpips package's v0.1 vgg.pth) also LPIPS on the VGG16 backbone; given
together with the AlexNet network the two are reported as `lpips_alex_*` and `lpips_vgg_*`.  `--lpips-vgg` without files: with --synthetic only.
One run with --ssim --ssim-skimage --lpips... --lpips-vgg... --fid... prints PSNR, both SSIM readings, both LPIPS readings and rFID."""
import argparse, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mimogpt.infer.infer_utils import parse_args_from_yaml
from mimogpt.infer.SelftokPipeline import SelftokPipeline
from selftoktokenizer_amd import dist as D, evaluate as E, synth, weights as W
from selftoktokenizer_amd.config import default_config

ap = argparse.ArgumentParser()
ap.add_argument("--images", default=None, help="folder of images (searched recursively, sorted)")
ap.add_argument("--synthetic", type=int, default=0, help="N hash-generated images + synthetic weights + hash noise instead of files")
ap.add_argument("--limit", type=int, default=0, help="evaluate only the first N images of the folder")
ap.add_argument("--yml-path", default=None)
ap.add_argument("--pretrained", default=None)
ap.add_argument("--sd3_pretrained", default=None)
ap.add_argument("--renderer-yml", default=None)
ap.add_argument("--renderer-pretrained", default=None)
ap.add_argument("--data_size", type=int, default=256)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--seed", type=int, default=1234)
ap.add_argument("--gemm", default=None, choices=["fp32", "f16x2", "exact", "f16"], help="exact: every operation in the reference's torch-CPU order (bit-equal pixels, the parity mode); f16: the lossy single-pass fp16 Linears (outside the 1e-3 dB of the other modes)")
ap.add_argument("--device-io", action="store_true", help="resize / crop / normalise the decoded files on the GPU (preprocess.DeviceLoader): the same values, bit for bit")
ap.add_argument("--preprocess", default="reference", choices=["reference", "bicubic", "adm"], help="how the files become data_size x data_size originals: the reference's Resize (bilinear) -> CenterCrop; Resize (bicubic) -> CenterCrop; or the ADM protocol center_crop_arr (BOX halvings, bicubic, floor-divided crop) that published ImageNet rFID / PSNR tables use.  By either loader route, bit for bit")
ap.add_argument("--ssim", action="store_true", help="also the SSIM of every image (11 x 11 Gaussian window, sigma 1.5, valid region); both figures then come from one device call per batch")
ap.add_argument("--metrics-u8", action="store_true", help="with --ssim: take PSNR and SSIM on the uint8 bytes save_image would write instead of the float tensors")
ap.add_argument("--lpips-backbone", default=None, help="torchvision AlexNet state dict (features.{0,3,6,8,10}.{weight,bias}); with --lpips-linear: also LPIPS (alex, v0.1) of every image, on the GPU")
ap.add_argument("--lpips-linear", default=None, help="the lpips package's v0.1 alex.pth (lin{0..4}.model.1.weight)")
ap.add_argument("--lpips", action="store_true", help="with --synthetic and no weight files: LPIPS on the hash-generated network (values of the published definition on synthetic weights)")
ap.add_argument("--ssim-skimage", action="store_true", help="also skimage.metrics.structural_similarity's default SSIM (uniform 7 x 7 window, sample covariance, fp64) of every image, on the GPU")
ap.add_argument("--ssim-range", default="signed", choices=["signed", "unsigned"], help="with --ssim-skimage: on [-1, 1] data with data_range 2 (signed) or on [0, 1] data with data_range 1")
ap.add_argument("--lpips-vgg", nargs="*", default=None, metavar="PTH", help="BACKBONE.pth LINEAR.pth: torchvision's vgg16 state dict and the lpips package's v0.1 vgg.pth: also LPIPS on the VGG16 backbone; no files: the hash-generated network, with --synthetic only")
ap.add_argument("--fid-weights", default=None, help="pytorch-fid's pt_inception-2015-12-05 state dict: also rFID (InceptionV3 pool3) of every decoder's reconstructions against the originals")
ap.add_argument("--fid", action="store_true", help="with --synthetic and no weight file: rFID on the hash-generated InceptionV3 (the published definition on synthetic weights)")
ap.add_argument("--out", default=None, help="also write the JSON line to this file (rank 0)")
a = ap.parse_args()
if a.lpips_vgg is not None and (len(a.lpips_vgg) not in (0, 2) or (not a.lpips_vgg and not a.synthetic)):
    ap.error("--lpips-vgg takes BACKBONE.pth LINEAR.pth, or nothing together with --synthetic (the published VGG16 and LPIPS weights are not shipped)")
if a.synthetic and a.preprocess != "reference":
    ap.error("--preprocess applies to image files: --synthetic images are generated at data_size")

rank, world, local = D.init_from_env()
torch.cuda.set_device(local)
dev = torch.device("cuda", local)
cfg = parse_args_from_yaml(a.yml_path) if a.yml_path else default_config(512)
K = int(cfg.tokenizer.params.k)
kw = {}
if a.pretrained is None:
    kw = dict(state_dict=W.synthetic_state_dict(W.expected_shapes(K), device=dev), vae_state_dict=W.synthetic_vae_state_dict(device=dev))
pipe = SelftokPipeline(cfg=cfg, ckpt_path=a.pretrained, sd3_path=a.sd3_pretrained, datasize=a.data_size, device=dev, gemm=a.gemm, verbose=False, **kw)
decoders, rpipe = ["diffusion"], None
if a.renderer_pretrained or (a.renderer_yml and a.pretrained is None):
    rcfg = parse_args_from_yaml(a.renderer_yml) if a.renderer_yml else default_config(K, renderer=True)
    rkw = {} if a.renderer_pretrained else dict(state_dict=W.synthetic_state_dict(W.expected_shapes(K, renderer=True), device=dev), vae_state_dict=W.synthetic_vae_state_dict(device=dev))
    rpipe = SelftokPipeline(cfg=rcfg, ckpt_path=a.renderer_pretrained, sd3_path=a.sd3_pretrained, datasize=a.data_size, device=dev, gemm=a.gemm, verbose=False, **rkw)
    decoders.append("renderer")
if a.synthetic:
    n = a.synthetic
    load = lambda lo, hi: synth.synthetic_images(hi - lo, first_index=lo)
    noise = lambda lo, hi: synth.synthetic_noise(hi - lo, first_index=lo)
    src = f"{n} hash-generated images (selftoktokenizer_amd.synth)"
else:
    assert a.images, "--images <dir> or --synthetic N"
    paths = E.list_images(a.images)
    if a.limit:
        paths = paths[:a.limit]
    assert paths, f"no image files under {a.images}"
    n, load, noise, src = len(paths), E.folder_loader(paths, a.data_size, device=dev if a.device_io else None, preprocess=a.preprocess), None, f"{len(paths)} files under {a.images}"
if bool(a.lpips_backbone) != bool(a.lpips_linear):
    ap.error("--lpips-backbone and --lpips-linear go together")
if a.lpips and not a.lpips_backbone and not a.synthetic:
    ap.error("--lpips without --lpips-backbone / --lpips-linear needs --synthetic: the published LPIPS weights are not shipped")
lpips_net = None
if a.lpips_backbone or a.lpips:
    from selftoktokenizer_amd.lpips import LpipsNet
    lpips_net = LpipsNet.from_files(a.lpips_backbone, a.lpips_linear, dev) if a.lpips_backbone else LpipsNet.synthetic(dev)
vgg_net = None
if a.lpips_vgg is not None:
    from selftoktokenizer_amd.lpips import LpipsNet
    vgg_net = LpipsNet.from_files(a.lpips_vgg[0], a.lpips_vgg[1], dev, net="vgg") if a.lpips_vgg else LpipsNet.synthetic(dev, net="vgg")
if a.fid and not a.fid_weights and not a.synthetic:
    ap.error("--fid without --fid-weights needs --synthetic: the published InceptionV3 weights are not shipped")
fid_net = None
if a.fid_weights or a.fid:
    from selftoktokenizer_amd.fid import InceptionNet
    fid_net = InceptionNet.from_files(a.fid_weights, dev) if a.fid_weights else InceptionNet.synthetic(dev)
if a.metrics_u8 and not (a.ssim or a.ssim_skimage or lpips_net or vgg_net or fid_net):
    ap.error("--metrics-u8 needs --ssim, --ssim-skimage, LPIPS or rFID (the device metrics route)")
mkw = dict(metrics=("psnr", "ssim"), metrics_u8=a.metrics_u8) if a.ssim else {}
if lpips_net is not None:
    mkw = dict(metrics=("psnr", "ssim", "lpips") if a.ssim else ("psnr", "lpips"), metrics_u8=a.metrics_u8, lpips=lpips_net)
if vgg_net is not None:                          # a sequence of networks: keys by backbone, `lpips_vgg_*` and, with the AlexNet network, `lpips_alex_*`
    mkw = dict(mkw, metrics=tuple(m for m in mkw.get("metrics", ("psnr",)) if m != "lpips") + ("lpips",), metrics_u8=a.metrics_u8,
               lpips=[lpips_net, vgg_net] if lpips_net is not None else [vgg_net])
if a.ssim_skimage:
    mkw = dict(mkw, metrics=tuple(mkw.get("metrics", ("psnr",))) + ("ssim_skimage",), metrics_u8=a.metrics_u8, ssim_skimage_signed=a.ssim_range == "signed")
if fid_net is not None:
    mkw = dict(mkw, metrics=tuple(mkw.get("metrics", ("psnr",))) + ("rfid",), metrics_u8=a.metrics_u8, fid=fid_net)
res = E.evaluate(pipe, load, n, batch=a.batch, decoders=decoders, noise_fn=noise, seed=a.seed, renderer_pipe=rpipe, verbose=True, **mkw)
D.barrier()
if rank == 0:
    line = {"tool": "eval_psnr", "source": src, "data_size": a.data_size, "preprocess": a.preprocess, "tokens": K, "gemm": pipe.model.model.gemm, "vae": pipe.vae.mode, "vae_decode": pipe.vae.decode_mode, "encoder": pipe.model.encoder.mode,
            "checkpoint": a.pretrained or "synthetic (hash-generated)", "renderer_checkpoint": a.renderer_pretrained, **res,
            "readme_reference_dB": {"tokenizer_512_ckpt": 21.86, "renderer_512_ckpt": 24.14, "tokenizer_1024_ckpt": 23.06, "renderer_1024_ckpt": 26.30,
                                    "note": "README.md:89-94 (256 x 256), needs the published weights"}}
    if a.ssim:                                   # BASELINE.md rows 17-18; the reference's table does not say which decoder produced them
        line["paper_reference_ssim"] = {"512": 0.709, "1024": 0.805,
                                        "note": "assets/results_table.PNG (README.md:61-65): ImageNet-val 50k at 256 x 256, decoder and SSIM variant not stated; needs the published weights"}
    if lpips_net is not None:                    # BASELINE.md rows 17-18; neither the decoder nor the LPIPS variant is stated (alex v0.1 is the package default)
        line["lpips_weights"] = lpips_net.source
        line["paper_reference_lpips"] = {"512": 0.084, "1024": 0.063, "note": "assets/results_table.PNG: needs the published tokenizer, AlexNet and LPIPS weights"}
    if vgg_net is not None:
        line["lpips_vgg_weights"] = vgg_net.source
        line.setdefault("paper_reference_lpips", {"512": 0.084, "1024": 0.063, "note": "assets/results_table.PNG: the LPIPS network is not stated; needs the published tokenizer, backbone and LPIPS weights"})
    if a.ssim_skimage:
        line.setdefault("paper_reference_ssim", {"512": 0.709, "1024": 0.805, "note": "assets/results_table.PNG: ImageNet-val 50k at 256 x 256, decoder and SSIM variant not stated; needs the published weights"})
    if fid_net is not None:                      # the variant the paper used is not stated; rFID depends on N below 2049 images (rfid_rank_deficient)
        line["fid_weights"] = fid_net.source
        line["paper_reference_rfid"] = {"note": "assets/results_table.PNG: ImageNet-val 50k at 256 x 256; needs the published tokenizer and InceptionV3 weights"}
    print(json.dumps(line), flush=True)
    if a.out:
        open(a.out, "w").write(json.dumps(line) + "\n")
D.shutdown()
