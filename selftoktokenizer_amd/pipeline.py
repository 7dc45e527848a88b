"""`SelftokPipeline` -- the drop-in host API of the reference (mimogpt/infer/SelftokPipeline.py:153-322),
re-authored for MI355X: same constructor, `encoding`, `decoding`, `decoding_with_renderer`,
`NormalizeToTensor`, same checkpoint layouts, same dtypes at every hand-off (bf16 VAE <-> fp32 tokenizer),
same RNG source for the decode noise (global CPU torch generator, :264).

Public attributes users touch in the reference are kept: `.model` (with `.encoder`, `.model`, `.diti`),
`.vae`, `.flow`, `.diti`, `.K`, `._steps`, `.cfg_scale`, `.start`.

Nothing here falls back to a CPU path: without libselftok_hip.so / a GPU the constructor raises.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from . import _lib, gemm_tune, ops, weights as W
from .encoder import QformerEncoderGPU, sinusoid_host
from .mmdit import MMDiTGPU
from .modsurface import ModuleSurface
from .schedule import DiTiCont, FlowSchedule, SlotSchedule, StreamFull, context_plan, pattern_groups, request_pattern
from .vae import AutoencoderKLGPU

SD3_SCALE, SD3_SHIFT = 1.5305, 0.0609     # SD3LatentFormat (sd3/sd3_impls.py:136-138)
DEFAULT_GEMM = "fp32"                     # see MMDiTGPU.set_gemm
DEFAULT_VAE_DECODE = "parity"             # decoder arithmetic outside gemm='exact' (see SelftokPipeline.__init__: vae_decode_mode)


class NormalizeToTensor(object):
    """PIL/ndarray HWC uint8 -> float tensor CHW in [-1,1] (reference SelftokPipeline.py:85-97)."""

    def __init__(self, reshape=True):
        self.reshape = reshape

    def __call__(self, image):
        image = np.array(image).astype(np.float32)
        image = (image / 127.5 - 1.0).astype(np.float32)
        if self.reshape:
            image = np.reshape(image, (image.shape[0], image.shape[1], -1))
        return torch.from_numpy(image.transpose((2, 0, 1)))


def norm_ip(img, low=-1, high=1):
    """in-place clamp + rescale to [0,1] (reference :135-137); bf16 device tensors use the HIP kernel."""
    assert (low, high) == (-1, 1)
    return ops.clamp01_(img)


class _Tokenizer(ModuleSurface):
    """`pipe.model` : the ImageTokenizer surface (image_tokenizer.py:58-159) the pipeline and users touch: `.encoder`, `.model`
    (the MMDiT), `.diti`, `.k`, and the read-only Module surface (`state_dict()` has the reference checkpoint's keys)."""

    def __init__(self, encoder, model, diti):
        self.encoder, self.model, self.diti = encoder, model, diti
        self.k = diti.K
        self.device = encoder.device

    def _flat_weights(self):
        d = dict(self.encoder._flat_weights())
        d.update(self.model._flat_weights())
        return d


class _Flow(FlowSchedule):
    """`pipe.flow`: RectifiedFlow(50, start, cut_of_k, val_schedule='uniform', shift=1.0, ...) buffers as numpy,
    plus the device-side sampler (p_sample_loop / sample_one_step / euler_step, sd3/rectified_flow.py:165-309)."""

    def __init__(self, num_steps, start, device, parameterization: str = "velocity"):
        super().__init__(num_steps, start)
        self.device = device
        if parameterization not in ("velocity", "x0"):
            raise ValueError(f"parameterization {parameterization!r}: expected 'velocity' or 'x0'")
        self.parameterization = parameterization                              # euler_step (sd3/rectified_flow.py:301-309)
        # sinusoidal embedding of t*1000 for the scheduled timesteps, evaluated with the reference's CPU arithmetic
        t1000 = torch.from_numpy(self.scheduled_t) * 1000.0
        self.t_freq = sinusoid_host(t1000).to(device)                        # [steps,256]
        # cfg_inference embeds floor(t*1000).int().clamp(0,999) instead (sd3/mmdit.py:1126)
        t_unc = torch.floor(torch.from_numpy(self.scheduled_t) * 1000).int().clamp(0, 999)
        self.t_freq_uncond = sinusoid_host(t_unc).to(device)
        # gemm='exact': the reference's own bits of these two tables (torch.cos / sin = MKL VML there: host dependent, shipped as data for the
        # default schedule -- 50 steps from t = 1; tools/oracle/gen_pos_table.py).  Another schedule falls back to this host's evaluation.
        self.t_freq_exact = self.t_freq_uncond_exact = None
        if num_steps == 50 and float(start) == 1.0:
            import os
            tab = torch.from_numpy(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "flow50_t_sincos.npy")))
            self.t_freq_exact, self.t_freq_uncond_exact = tab[0].to(device).contiguous(), tab[1].to(device).contiguous()

    def plan_context(self, dit: MMDiTGPU, k_table, K: int, prefix_k: Optional[int] = None, super_mask=None, batched: bool = False):
        """-> (schedule.ContextPlan, device index of its `gather`, device words of its `words_rows`; None where the plan has none): `p_sample_loop`'s
        `plan=`.  It reads the mask on the host and uploads, neither of which may happen while a stream is capturing: a caller that captures the
        loop in a hipGraph calls this first and keeps the result for as long as the graph lives."""
        pattern = None if super_mask is None else torch.as_tensor(super_mask).cpu().numpy()
        plan = context_plan(k_table, K, len(k_table), prefix_k, pattern, batched, keep_positions=dit.gemm == "exact")
        index = None if plan.gather is None else torch.tensor(plan.gather, device=self.device)                    # (the plan's arrays are read-only: copy)
        words = None if plan.words_rows is None else dit.pack_key_mask(torch.tensor(plan.words_rows, device=self.device))
        return plan, index, words

    @torch.no_grad()
    def p_sample_loop(self, dit: MMDiTGPU, noise: torch.Tensor, ehs: torch.Tensor, k_table: np.ndarray,
                      context_see_xt: bool = True, uncond_scale: float = 1.0, max_steps: Optional[int] = None,
                      trace: Optional[list] = None, prefix_k: Optional[int] = None, super_mask=None, plan=None) -> torch.Tensor:
        """`prefix_k`: the reference loop's `super_mask` (rectified_flow.py:226-227, mask = mask * super_mask) for the prefix mask
        arange(K) < prefix_k -- only the first prefix_k tokens are ever visible (decode from a partial token sequence).
        `super_mask`: the same hook for ANY visibility pattern over the K tokens ([K] bool / 0-1, the same for every sample).
        Which rows a step sees and by which route (slice / gather / in place under key-mask words) is schedule.context_plan's decision.
        `plan`: the result of `plan_context`, instead of the two -- what a caller that captures this loop in a hipGraph passes, and
        the way to decode a pattern PER SAMPLE as one batch (`batched=True`)."""
        B, K = noise.shape[0], int(ehs.shape[1])
        if plan is not None and (prefix_k is not None or super_mask is not None):
            raise ValueError("plan is exclusive with prefix_k / super_mask")
        plan, index, kwords = plan or self.plan_context(dit, k_table, K, prefix_k, super_mask)
        steps = self.num_timesteps if max_steps is None else min(max_steps, self.num_timesteps)
        if len(plan.n_live) < steps or (plan.words_rows is not None and plan.words_rows.shape not in ((1, K), (B, K))):
            raise ValueError(f"plan: expected {steps} steps and words_rows [1 or B, K] = [1 or {B}, {K}]")
        x = noise.to(self.device).float().contiguous()
        hp, wp = x.shape[-2] // 2, x.shape[-1] // 2
        ctx0, tables = dit.embed_context(ehs), None                           # step independent
        if index is not None:
            ctx0, tables, _ = dit.gather_context(ctx0, index=index)
        cqkv0 = dit.block0_context_qkv(ctx0, tables) if ctx0.shape[1] > 0 else None   # block 0's context QKV is step independent too
        for i in range(steps):
            n_live = int(plan.n_live[i])
            exact = dit.gemm == "exact" and self.t_freq_exact is not None
            tf = (self.t_freq_exact if exact else self.t_freq)[i:i + 1].expand(B, -1).contiguous()
            t_name = float(self.scheduled_t[i])                               # names the embedded timestep (MMDiTGPU._step_modulations)
            # CFG branch (rectified_flow.py:280-289): the conditional call omits context_see_xt (-> False) and the unconditional one
            # (cfg_inference) sees no context token at all
            guided = uncond_scale != 1.0
            y = dit.velocity_tokens(x, tf, ctx0, n_live, context_see_xt and not guided, cqkv0, tables, t_key=("t", t_name), kmask=kwords)
            yu = None
            if guided:
                tfu = (self.t_freq_uncond_exact if exact else self.t_freq_uncond)[i:i + 1].expand(B, -1).contiguous()
                yu = dit.velocity_tokens(x, tfu, ctx0, 0, False, t_key=("floor", t_name))
            if self.parameterization == "x0":
                # the model output is the clean latent: x_prev = v + a_prev (x - v) / a_t  (euler_step, rectified_flow.py:305-307);
                # the CFG mix rides in the unpatchify kernel, the update is the reference's own chain of fp32 element-wise ops
                _, v = ops.unpatchify_cfg_euler(y, None, 0.0, y_uncond=yu, cfg_scale=uncond_scale, C=x.shape[1], hp=hp, wp=wp)
                x = v + float(self.scheduled_t_prev[i]) * (x - v) / float(self.scheduled_t[i])
            else:
                x, _ = ops.unpatchify_cfg_euler(y, x, float(self.dt[i]), y_uncond=yu, cfg_scale=uncond_scale, C=x.shape[1], hp=hp, wp=wp)
            if trace is not None:
                trace.append(x.clone())
        return x


def _on_own_device(fn):
    """run a public entry point with the pipeline's GPU as the current device: every HIP launch goes to the current device's
    stream, and a process may hold several pipelines on different GPUs or change the current device between calls"""
    import functools

    @functools.wraps(fn)
    def wrapped(self, *a, **k):
        with torch.cuda.device(self.device):
            return fn(self, *a, **k)
    return wrapped


class SelftokPipeline():
    def __init__(self, cfg, ckpt_path, sd3_path, datasize=256, start=1.0, cfg_scale=1, model_type='sd3',
                 dtype=torch.bfloat16, ema_decoder=False, device=None, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 vae_state_dict: Optional[Dict[str, torch.Tensor]] = None, verbose: bool = True, gemm: Optional[str] = None,
                 vae_mode: Optional[str] = None, tune_gemm: Optional[bool] = None, encoder_mode: Optional[str] = None,
                 vae_encode_mode: Optional[str] = None, vae_decode_mode: Optional[str] = None, attention: Optional[str] = None,
                 splitk: Optional[str] = None):
        """cfg: parse_args_from_yaml(...) ; ckpt_path: tokenizer .pth ; sd3_path: diffusers SD3 folder (…/vae/…).
        `state_dict` / `vae_state_dict` (extensions) bypass the files, e.g. with weights.synthetic_state_dict().
        `gemm` (extension): arithmetic of the MMDiT block Linears, 'fp32' (hipBLASLt fp32), 'f16x2' (fp32-equivalent
        split GEMM on the f16 matrix cores, csrc/gemm_split.hip), 'exact' (the reference's bits) or 'f16' (LOSSY: fp16-rounded
        operands, fp32 accumulation, csrc/gemm_f16.hip -- for bulk decoding, outside the north star's 1e-3 dB); default DEFAULT_GEMM.
        `attention` (extension, OPT-IN, LOSSY): None / 'split' (default), or 'f16' together with gemm='f16' -- the joint attention of the MMDiT and the renderer
        as one fp16 matrix instruction per product (csrc/attention_f16.hip); ValueError with any other gemm mode.
        `splitk` (extension, OPT-IN, LOSSY): None / 'f16x2' (default: in gemm='f16' one to four images decode on the f16x2 split-K Linears, with f16x2 bits), or
        'f16' together with gemm='f16' -- those row counts on the split-K form of the single-pass fp16 Linear (csrc/gemm_f16_splitk.hip); ValueError with any
        other gemm mode.
        `vae_encode_mode` / `vae_decode_mode` (extensions; `vae_mode` sets both): arithmetic of the two halves of the SD3 VAE (vae.AutoencoderKLGPU).
        'exact': every reduction in the summation ORDER of the reference's torch-CPU run (csrc/vae_exact.hip, fp32 matrix cores) -- encoder: latents and
        token ids from pixels equal the reference's bit for bit; decoder: pixels equal the reference's decode of the same latents, incl. its batch
        dependence (a 3x3 layer whose bf16 activation reaches 2^31 bytes -- 64 images per call at 256 x 256 -- takes oneDNN's order 1: probed at 48 / 64
        images per call, extrapolated above).  'parity': every convolution / GroupNorm through csrc/conv.hip -- fp32 accumulation with the bias inside, one
        rounding, the reference's CPU arithmetic in its own summation order; no MIOpen, bit-stable, batch independent, 5x faster.  'miopen' / 'fast': the
        rounds 1-3 routes through MIOpen (both halves).  Defaults (round 6): encode 'exact' at the probed sizes (128 / 256 / 320 px; token ids need it),
        'parity' elsewhere; decode 'parity' (pixels within the north star's 1e-3 dB of the reference either way), and 'exact' while gemm == 'exact'
        (the mode whose pixels ARE the reference's) unless `vae_decode_mode` / `vae_mode` was given.
        `encoder_mode` (extension): 'exact' (default: the Q-Former encoder in the summation order of every reduction and the polynomial of every
        transcendental torch-CPU executes for the reference, csrc/encoder_exact.hip -- pre-quantizer features and token ids equal those of the
        reference's runs at 8 <= B <= 64 images per call bit for bit, and are the same here for every batching; the reference itself takes other MKL paths at
        B = 1 and for Linears below 16 / 512 rows, which this mode does not follow: DESIGN 15.2, 15.8) or 'fast' (hipBLASLt GEMMs + the fused rounds 1-3 kernels: features within 6e-5, ~2x faster encoder).
        No environment variable is read: every knob is a constructor argument.
        `tune_gemm` (extension, OPT-IN): pick hipBLASLt's kernel for the fp32 block Linears by a ~4 s measurement per batch size
        (gemm_tune.py) -- up front through `pipe.tune_linears(batch)`, or at the first decode of a batch size.  TunableOp is enabled
        (tuning off) only inside this pipeline's own sampler calls and the caller's torch.cuda.tunable flags are restored; on another
        hipBLASLt build than the one the candidate kernels were found with it does nothing, loudly.  Default off."""
        _lib.load()                                                           # fail loudly if the HIP library is missing
        self.tune_gemm = bool(tune_gemm)
        self.gemm_tune_report = None
        if device is None:
            device = "cuda"
        if not torch.cuda.is_available():
            raise _lib.SelftokHipError("SelftokPipeline needs an MI355X (ROCm) device; there is no CPU path")
        if model_type != 'sd3':
            raise ValueError(f"Unsupported MODEL_TYPE: {model_type}. Expected 'sd3'")
        self.cfg, self.datasize, self.model_type, self.dtype = cfg, datasize, model_type, dtype
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SelftokHipError(f"SelftokPipeline needs a GPU device, got {self.device}")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        with torch.cuda.device(self.device):                                  # our launches use the current device's stream
            self._build(cfg, ckpt_path, sd3_path, start, cfg_scale, dtype, ema_decoder, state_dict, vae_state_dict, verbose, gemm, vae_mode, encoder_mode,
                        vae_encode_mode, vae_decode_mode, attention, splitk)

    def _build(self, cfg, ckpt_path, sd3_path, start, cfg_scale, dtype, ema_decoder, state_dict, vae_state_dict, verbose, gemm, vae_mode=None, encoder_mode=None,
               vae_encode_mode=None, vae_decode_mode=None, attention=None, splitk=None):
        if attention == "f16" and (gemm or DEFAULT_GEMM) != "f16" or attention not in (None,) + MMDiTGPU.ATTENTION_MODES:
            raise ValueError(f"attention={attention!r} with gemm={gemm or DEFAULT_GEMM!r}: expected None, 'split', or 'f16' together with gemm='f16'")
        if splitk == "f16" and (gemm or DEFAULT_GEMM) != "f16" or splitk not in (None,) + MMDiTGPU.SPLITK_MODES:
            raise ValueError(f"splitk={splitk!r} with gemm={gemm or DEFAULT_GEMM!r}: expected None, 'f16x2', or 'f16' together with gemm='f16'")
        p = cfg.tokenizer.params
        p.noise_schedule_config.is_eval = cfg.common.is_eval
        # configuration knobs the reference honours but this hot path does not implement: refuse, never ignore silently
        if p.get("diffusion_type", "flow") != "flow":
            raise NotImplementedError("diffusion_type != 'flow' (the Gaussian-diffusion sampler is outside the hot path)")
        nsc = p.noise_schedule_config
        self.parameterization = str(nsc.get("parameterization", "velocity"))
        if self.parameterization not in ("velocity", "x0"):
            raise ValueError(f"noise_schedule_config.parameterization {self.parameterization!r}: expected 'velocity' or 'x0'")
        cut = p.get("cut_of_k", None)
        if cut and float(cut) < 1:
            raise NotImplementedError("cut_of_k < 1 (context padding, rectified_flow.py:216-224) is not implemented; the shipped configs do not set it")
        pre_norm = bool(p.get("encoder_config", {}).get("pre_norm", False))        # models_ours.py:219-220 (round 6; False in the shipped configs)
        K = int(p.k)
        renderer = "Renderer" in str(p.model)
        self.diti = DiTiCont(1000, K, p.stages, p.k_per_stage)
        self.K = K
        self.context_see_xt = bool(p.get("context_see_xt", False))

        vsd = vae_state_dict if vae_state_dict is not None else W.load_vae_checkpoint(sd3_path)
        W.check_vae_state_dict(vsd)
        probed = int(self.datasize) in AutoencoderKLGPU.EXACT_SIZES
        enc_mode = vae_encode_mode or vae_mode or ("exact" if probed else "parity")
        self._vae_decode_explicit = (vae_decode_mode or vae_mode) is not None
        dec_mode = vae_decode_mode or vae_mode or ("exact" if (probed and (gemm or DEFAULT_GEMM) == "exact" and enc_mode in ("exact", "parity")) else
                                                   (enc_mode if enc_mode in ("miopen", "fast") else DEFAULT_VAE_DECODE))
        self.vae = AutoencoderKLGPU(vsd, self.device, dtype, mode=enc_mode, decode_mode=dec_mode)

        self.verbose = verbose
        self._say("Loading all...")
        sd = state_dict if state_dict is not None else W.load_tokenizer_checkpoint(ckpt_path)
        W.check_tokenizer_state_dict(sd, K, renderer=renderer, ema=bool(ema_decoder))   # load_state_dict(strict=False) / strict EMA load
        self.ema_decoder = ema_decoder
        dit_sd = sd
        if ema_decoder:   # reference :193-194: EMA copy of the DiT under 'ema_state_dict' (keys without the 'model.' prefix)
            dit_sd = {"model." + k: v for k, v in sd["ema_state_dict"].items()}       # strict contract checked above: bare MMDiT keys only
        encoder = QformerEncoderGPU(sd, self.device, K, mode=encoder_mode or "exact", pre_norm=pre_norm)
        dit = MMDiTGPU(dit_sd, self.device, K, renderer=renderer)
        dit.set_gemm(gemm or DEFAULT_GEMM, attention=attention, splitk=splitk)
        self.model = _Tokenizer(encoder, dit, self.diti)

        self.count = 0
        self.count_cfg = 0
        self.start = start
        self.cfg_scale = cfg_scale
        self.cut_of_k = p.get("cut_of_k", None) or None
        self._steps = 50
        self.flow = _Flow(self._steps, self.start, self.device, self.parameterization)
        self.k_table = self.diti.to_indices(self.flow.t_long)                # k for each of the 50 steps
        self.cond_vary = True
        self.saved_images = 8
        self._graphs = {}        # (shapes, steps, scale, gemm, attention, splitk, context plan) -> (hipGraph, static noise, static ehs, static output, what the graph reads)

    def _say(self, msg):
        if self.verbose:          # the reference prints these progress lines unconditionally (:192,212,223,230,292,299,320)
            print(msg)

    # ------------------------------------------------------------------------------------------------
    @_on_own_device
    @torch.no_grad()
    def encode_latents(self, images: torch.Tensor) -> torch.Tensor:
        """VAE mean -> SD3LatentFormat.process_in -> fp32 (reference :214-218)"""
        moments = self.vae.encode_moments(images.to(dtype=self.dtype, device=self.device))
        return ops.latent_process_in(moments.contiguous(), moments.shape[1] // 2, SD3_SHIFT, SD3_SCALE)

    @_on_own_device
    @torch.no_grad()
    def encoding(self, images, device=None):
        self._say("Begin encoding.")
        x_0 = self.encode_latents(images)
        _, tokens = self.model.encoder(x_0, d=None)
        self._say('End encoding.')
        return tokens

    @_on_own_device
    @torch.no_grad()
    def encoding_topk(self, images, k: int = 2, device=None):
        """(extension) `encoding` with the runners-up: (ids [B,K,k] int64, scores [B,K,k] fp32), the k <= 8 best codes of every token and
        their exact cosine scores, best first (ties by ascending id).  ids[..., 0] equals encoding(images); tokens.margins(scores) is the
        top-1 / top-2 gap that tells which tokens are near-ties."""
        return self.model.encoder.topk(self.encode_latents(images), k)

    @_on_own_device
    @torch.no_grad()
    def preprocess_u8(self, images, dtype=None, views=None, preprocess: str = "reference") -> torch.Tensor:
        """(extension) uint8 RGB HWC images -- a list of arrays of ANY sizes, or one uint8 tensor [B, H, W, 3] (host or device) -> the
        [B, 3, datasize, datasize] batch `encoding` takes, on the device: Resize(datasize) -> CenterCrop(datasize) -> NormalizeToTensor of
        the reference's user script (test.py:27-31) bit for bit (csrc/image_io.hip).  dtype: this pipeline's bf16 (default) or fp32.
        views = fn(width, height) -> a list of preprocess.View (views_five, views_ten, view_resized_crop, ...): instead [sum of views, 3,
        datasize, datasize], image by image and then view by view, each what torchvision gives on the PIL image (preprocess.apply_view_pil)
        bit for bit (csrc/image_views.hip).  views=None is the centre crop, by the same route as before.
        preprocess: "reference" (the above); "bicubic": Resize(datasize, BICUBIC) -> CenterCrop, the views resampled with BICUBIC likewise
        (apply_view_pil(..., filter="bicubic")); "adm": preprocess.center_crop_adm, the ADM protocol, which takes no views (csrc/image_filters.hip)."""
        dtype = dtype or self.dtype
        if preprocess != "reference":
            from .preprocess import _check_preprocess
            _check_preprocess(preprocess)
            if views is not None and preprocess == "adm":
                raise ValueError('preprocess="adm" takes no views: the ADM protocol is one centre crop per image')
            if torch.is_tensor(images):
                if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
                    raise TypeError(f"expected a uint8 [B, H, W, 3] tensor, got {images.dtype} {tuple(images.shape)}")
                images = list(images.cpu().numpy())                              # the other recipes go through the loader, whatever holds the pixels
            loaders = self.__dict__.setdefault("_u8_loaders", {})
            if (dtype, preprocess) not in loaders:
                from .preprocess import DeviceLoader
                loaders[(dtype, preprocess)] = DeviceLoader(int(self.datasize), self.device, dtype=dtype, preprocess=preprocess)
            return loaders[(dtype, preprocess)].load(images, views=views)
        if torch.is_tensor(images):
            if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
                raise TypeError(f"expected a uint8 [B, H, W, 3] tensor, got {images.dtype} {tuple(images.shape)}")
            if images.is_cuda:
                B, H, W, _ = images.shape
                table = np.array([[b * H * W * 3, W, H] for b in range(B)], dtype=np.int64).reshape(B, 3)
                if views is not None:
                    from .preprocess import view_rows
                    return ops.image_views(images.to(self.device).contiguous().reshape(-1), table, view_rows([views(W, H) for _ in range(B)], int(self.datasize)),
                                           int(self.datasize), dtype=dtype)
                return ops.image_resize_crop_norm(images.to(self.device).contiguous().reshape(-1), table, int(self.datasize), dtype=dtype)
            images = list(images.numpy())
        loaders = self.__dict__.setdefault("_u8_loaders", {})
        if dtype not in loaders:
            from .preprocess import DeviceLoader
            loaders[dtype] = DeviceLoader(int(self.datasize), self.device, dtype=dtype)
        return loaders[dtype].load(images) if views is None else loaders[dtype].load(images, views=views)

    def encoding_u8(self, images, device=None, topk: int = 0, views=None, preprocess: str = "reference"):
        """(extension) `encoding` from 8-bit pixels: equal to encoding(torch.stack([load_image-equivalent of each image])) -- same bf16 tensor
        into the VAE, same token ids -- without the per-image PIL resize, fp32 tensors and pageable copy on the host.  topk = k > 0: the (ids, scores)
        of `encoding_topk(..., k)` instead.  views: see preprocess_u8; one row of ids per view, equal to encoding(torch.stack([apply_view_pil(...)]))."""
        if preprocess != "reference":                                           # see preprocess_u8: load_image(filter="bicubic") / load_image_adm are then the host twins
            x = self.preprocess_u8(images, views=views, preprocess=preprocess)
            return self.encoding_topk(x, k=topk, device=device) if topk else self.encoding(x, device=device)
        x = self.preprocess_u8(images) if views is None else self.preprocess_u8(images, views=views)
        return self.encoding_topk(x, k=topk, device=device) if topk else self.encoding(x, device=device)

    @_on_own_device
    @torch.no_grad()
    def to_uint8(self, recons: torch.Tensor) -> torch.Tensor:
        """(extension) the [0, 1] output of `decoding` / `decoding_with_renderer` -> uint8 [B, H, W, 3] on the device: the bytes
        `preprocess.save_image` writes for each image (torchvision.utils.save_image's arithmetic in the tensor's own dtype)."""
        return ops.image_to_u8(recons.to(self.device))

    @_on_own_device
    @torch.no_grad()
    def _codes(self, idx) -> torch.Tensor:
        if isinstance(idx, np.ndarray):
            if not np.issubdtype(idx.dtype, np.integer):
                raise TypeError(f"token ids must be integers, got {idx.dtype} (the reference indexes the codebook with them)")
            idx = np.ascontiguousarray(idx if idx.dtype in (np.int64, np.int32) else idx.astype(np.int64))   # uint16 / int16 / uint8 wire formats
            token_idx = torch.from_numpy(idx).to(self.device)
        else:
            if idx.is_floating_point() or idx.dtype == torch.bool:
                raise TypeError(f"token ids must be integers, got {idx.dtype}")
            token_idx = idx.to(self.device)
        B = token_idx.shape[0]
        return self.model.encoder.codes_ln(token_idx.reshape(B, -1))          # get_output_from_indices + final_layer_norm3

    @_on_own_device
    @torch.no_grad()
    def _to_pixels(self, pred_x0: torch.Tensor) -> torch.Tensor:
        z = ops.latent_process_out(pred_x0, SD3_SHIFT, SD3_SCALE)             # process_out + .to(bf16) (:285-287)
        recons = self.vae.decode(z)[0].contiguous()
        return norm_ip(recons, -1, 1)

    @_on_own_device
    def tune_linears(self, batch: int, renderer: Optional[bool] = None, guided: bool = False):
        """(extension) measure hipBLASLt's candidate kernels for the fp32 block Linears of a decode at `batch` images now (~4 s, once
        per batch size; gemm_tune.py) and switch `tune_gemm` on, so that this pipeline's sampler calls run under TunableOp with the
        winners.  `guided`: a CFG decode (two MMDiT passes per step, rows of 2 x batch).  Returns the report ({(N, K): (kernel or None,
        ms default, ms chosen)}), or None in f16x2 mode / on another hipBLASLt build."""
        self.tune_gemm = True
        tokens = (self.datasize // 16) ** 2
        renderer = self.model.model.renderer if renderer is None else renderer
        self._tune_linears(int(batch) * (2 if guided else 1), [self.K - 1] if renderer else self.k_table, tokens)
        return self.gemm_tune_report

    @_on_own_device
    def _tune_linears(self, B: int, k_table, image_tokens: int) -> None:
        """fp32 mode: choose hipBLASLt's kernels for this batch size's block Linears once (gemm_tune.py)"""
        if self.tune_gemm and self.model.model.gemm == "fp32":
            rows, reps = gemm_tune.step_row_counts(B, k_table, image_tokens)
            self.gemm_tune_report = gemm_tune.autotune_linears(rows, self.device, reps=reps, verbose=self.verbose)

    def _tunable_scope(self):
        """TunableOp on for the duration of one of OUR sampler calls when kernels were installed; the caller's flags come back after"""
        import contextlib
        return gemm_tune.enabled() if (self.tune_gemm and self.gemm_tune_report and self.model.model.gemm == "fp32") else contextlib.nullcontext()

    def set_gemm(self, mode: str, attention: Optional[str] = None, splitk: Optional[str] = None) -> str:
        """switch the MMDiT between 'fp32', 'f16x2', 'exact' and the lossy 'f16' (see MMDiTGPU.set_gemm); returns the mode in force.  Unless the decoder's arithmetic was
        chosen explicitly (`vae_decode_mode` / `vae_mode`), 'exact' brings the exact-order VAE decoder with it (the mode whose pixels are the reference's
        bit for bit) and the other modes return to the default decoder.  `attention`: None / 'split', or 'f16' together with mode 'f16' (LOSSY single-pass
        fp16 joint attention, MMDiTGPU.set_gemm); a call without it resets it.  `splitk`: None / 'f16x2', or 'f16' together with mode 'f16' (LOSSY: one to four
        images on the split-K single-pass fp16 Linears instead of the f16x2 ones, MMDiTGPU.set_gemm); a call without it resets it."""
        got = self.model.model.set_gemm(mode, attention=attention, splitk=splitk)
        if not self._vae_decode_explicit and self.vae.mode in ("exact", "parity"):
            want = "exact" if (got == "exact" and int(self.datasize) in AutoencoderKLGPU.EXACT_SIZES) else DEFAULT_VAE_DECODE
            if self.vae.decode_mode != want:
                self.vae.set_decode_mode(want)
        return got

    @torch.no_grad()
    def _checked(self, run):
        """run() -> latent.  In the 'f16x2' and 'f16' GEMM modes an activation outside the fp16 range (|a| >= 65504) invalidates the
        result (sticky device flag, one host read per call): redo the call on the fp32 library GEMMs."""
        dit = self.model.model
        out = run()
        mode, attention, splitk = dit.gemm, dit.attention, dit.splitk
        if mode in dit.SPLIT_MODES and int(dit.overflow.item()) != 0:
            print(f"[selftok] {mode} GEMM: activation outside the fp16 range -> recomputing this call with fp32 GEMMs")
            dit.overflow.zero_()
            dit.set_gemm("fp32")
            try:
                out = run()
            finally:
                dit.set_gemm(mode, attention=attention, splitk=splitk)    # the split weights are kept: no re-pack
        return out

    @torch.no_grad()
    def _sample(self, xt, ehs, max_steps, uncond_scale, use_graph, prefix_k=None, super_mask=None, mask_batched=False):
        """the sampler.  A [B, K] `super_mask` with differing rows (the reference's `mask * super_mask` with a [B, K] tensor, rectified_flow.py:226-227)
        is decoded as ONE batch with `mask_batched` (per-sample key bit masks in the joint attention), else in groups of equal rows."""
        B = xt.shape[0]
        pattern = None if super_mask is None else torch.as_tensor(super_mask).cpu().numpy()
        batched = bool(mask_batched) and pattern is not None and pattern.ndim == 2 and pattern.shape[0] == B
        groups = pattern_groups(pattern, B, batched)
        if groups[0][0] is None:
            return self._sample_group(xt, ehs, max_steps, uncond_scale, use_graph, prefix_k, groups[0][1], batched)
        out = torch.empty(xt.shape, dtype=torch.float32, device=self.device)
        for idx, row in groups:
            sel = torch.as_tensor(idx)
            out[sel.to(self.device)] = self._sample_group(xt[sel], ehs[sel.to(ehs.device)], max_steps, uncond_scale, use_graph, prefix_k, row)
        return out

    def _sample_group(self, xt, ehs, max_steps, uncond_scale, use_graph, prefix_k, pattern, batched=False):
        """the 50-step loop, optionally replayed from a hipGraph captured once per (batch, latent size, context plan) -- the loop is
        ~21k kernel launches; at small batch the host cannot issue them as fast as the GPU retires them."""
        dit = self.model.model
        plan = self.flow.plan_context(dit, self.k_table, self.K, prefix_k, pattern, batched)       # host read + uploads: before any capture
        loop = lambda noise, e: self.flow.p_sample_loop(dit, noise, e, self.k_table, context_see_xt=True, uncond_scale=uncond_scale, max_steps=max_steps, plan=plan)
        if not use_graph:
            return loop(xt, ehs)
        key = (tuple(xt.shape), tuple(ehs.shape), max_steps, float(uncond_scale), dit.gemm, dit.attention, dit.splitk, dit.PRESPLIT, dit.SPLITK, plan[0].key)
        if key not in self._graphs:
            s_noise = torch.empty(xt.shape, dtype=torch.float32, device=self.device)
            s_ehs = torch.empty_like(ehs)
            s_noise.copy_(xt); s_ehs.copy_(ehs)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):       # warm-up outside capture (hipBLASLt / allocator warm)
                loop(s_noise, s_ehs)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            dit._capture_refs = [plan]           # what the capture reads: the plan's uploads, remembered modulations (MMDiTGPU._step_modulations); kept alive with the graph
            try:
                with torch.cuda.graph(g):
                    s_out = loop(s_noise, s_ehs)
                refs = dit._capture_refs
            finally:
                dit._capture_refs = None
            self._graphs[key] = (g, s_noise, s_ehs, s_out, refs)
        g, s_noise, s_ehs, s_out = self._graphs[key][:4]
        s_noise.copy_(xt.to(self.device)); s_ehs.copy_(ehs)
        g.replay()
        return s_out.clone()

    @_on_own_device
    @torch.no_grad()
    def decoding(self, idx, device=None, noise: Optional[torch.Tensor] = None, return_latent: bool = False,
                 max_steps: Optional[int] = None, uncond_scale: float = 1.0, use_graph: bool = False,
                 prefix_k: Optional[int] = None, super_mask=None, ar_partial=None, mask_batched: bool = False):
        """idx: np.ndarray int64 [B,K] -> bf16 [B,3,H,W] in [0,1] (reference :227-294).  `noise` (extension) replaces the
        `torch.randn` draw from the global CPU generator (:264); `uncond_scale` exposes the dormant CFG branch
        (p_sample_loop's argument of that name).
        `ar_partial` (extension): THE route for a partial sequence of an AR model.  An AR model emits the tokens in reverse
        (README.md:241): tokenizer index K - 1 first, index 0 last, so its first m tokens are the positions K - m .. K - 1.
        m is an int or one value per sample (0 <= m_b <= K); `tokens.pad_ar_partial` builds idx from what the model emitted.  Sugar for
        super_mask = `tokens.suffix_mask(K, m)`: equal m_b run the uniform route below, differing m_b run ONE batched pass with
        per-sample key masks in the joint attention.  Exclusive with prefix_k / super_mask.
        `prefix_k` (extension): the reference loop's `super_mask` hook (rectified_flow.py:226-227) with the mask arange(K) < prefix_k:
        tokens 0 .. prefix_k - 1, the FINE end of the sequence (`tokens.pad_prefix`).  It is not the AR partial route.
        `super_mask` (extension): the same hook with any visibility pattern over the K tokens ([K] bool / 0-1 array, or [B, K]: one
        pattern per sample, decoded in groups of equal pattern -- or, with `mask_batched=True`, as one batch)."""
        self._say("Begin decoding.")
        super_mask, mask_batched = request_pattern(self.K, int(idx.shape[0]), prefix_k, super_mask, ar_partial, mask_batched)
        outs_q = self._codes(idx)
        B = outs_q.shape[0]
        # t_mapped = timestep_map[0] -> k = K-1 -> enc_mask all true -> encoder_hidden_states = outs_q (:243-252)
        k0 = int(self.diti.to_indices(self.flow.t_long[:1])[0])
        ehs = outs_q if k0 >= self.K - 1 else outs_q * (torch.arange(self.K, device=self.device) <= k0)[None, :, None]
        latent_dim = self.datasize // 8
        xt = noise if noise is not None else torch.randn(B, 16, latent_dim, latent_dim)
        self._tune_linears(B * (2 if uncond_scale != 1.0 else 1), self.k_table, (latent_dim // 2) ** 2)
        with self._tunable_scope():
            pred_x0 = self._checked(lambda: self._sample(xt, ehs, max_steps, uncond_scale, use_graph, prefix_k, super_mask, mask_batched))
        recons = self._to_pixels(pred_x0)
        self._say('End decoding.')
        return (recons, pred_x0) if return_latent else recons

    def decode_stream(self, slots: int, uncond_scale: float = 1.0, max_steps: Optional[int] = None, context: str = "live",
                      return_latent: bool = False) -> "DecodeStream":
        """(extension) in-flight batching of the sampler: a `DecodeStream` of `slots` slots in which every request is at its OWN sampler step --
        `submit` a request whenever a slot is free, `step()` advances all of them by one step and returns the ones that finished.  See DecodeStream."""
        return DecodeStream(self, slots, uncond_scale, max_steps, context, return_latent)

    def decoding_stream(self, requests, slots: int = 8, **stream_kw):
        """(extension) `decoding` over an iterable of (ids [K], kwargs of DecodeStream.submit) through one decode stream that is kept full:
        yields (index of the request, image [3, H, W]) in completion order."""
        stream = self.decode_stream(slots, **stream_kw)
        index, it, pending = {}, iter(enumerate(requests)), True
        while pending or stream.in_flight:
            while pending and stream.free_slots:
                nxt = next(it, None)
                if nxt is None:
                    pending = False
                    break
                i, (ids, kw) = nxt
                index[stream.submit(ids, **(kw or {}))] = i
            for done in stream.step() if stream.in_flight else ():
                yield (index.pop(done[0]),) + tuple(done[1:])

    @_on_own_device
    @torch.no_grad()
    def decoding_with_renderer(self, idx, device=None, return_latent: bool = False):
        """one MMDiT_Renderer pass instead of the 50-step loop (reference :296-322)"""
        self._say("Begin decoding with Renderer.")
        outs_q = self._codes(idx)
        self._tune_linears(outs_q.shape[0], [self.K - 1], (self.datasize // 16) ** 2)
        with self._tunable_scope():
            pred_x0 = self._checked(lambda: self.model.model(y=None, encoder_hidden_states=outs_q)[0])
        recons = self._to_pixels(pred_x0)
        self._say('End decoding with Renderer.')
        return (recons, pred_x0) if return_latent else recons


class DecodeStream:
    """In-flight batching of the 50-step sampler (SelftokPipeline.decode_stream).  `slots` requests share every model
    evaluation, each at its own sampler step: the step state (timestep row of the modulation tables, visibility limit, dt) lives on the device,
    one row per slot (csrc/decode_stream.hip), and the host only mirrors the step counters (schedule.SlotSchedule) to know the context rows
    of the next step and who retires.  A step that retires nobody issues no host synchronisation and no host-to-device copy.
      submit(ids, ...) -> ticket      the only place that copies from the host; StreamFull without a free slot
      step() -> [(ticket, pixels [3, H, W][, latent [16, L, L]])]      the requests that have run their last step, in ticket order
      drain() -> the same, stepping until the stream is empty
    context="live": the model sees the context rows below the largest limit of a request in flight; "full": always all K rows (shape-static;
    in f16x2 a request's bits then do not depend on its slot or its neighbours).  Idle slots are computed and discarded: the row count of
    every Linear is fixed.  gemm='exact' is refused; one CFG scale per stream."""

    def __init__(self, pipe: "SelftokPipeline", slots: int, uncond_scale: float = 1.0, max_steps: Optional[int] = None, context: str = "live",
                 return_latent: bool = False):
        self.pipe, self.dit = pipe, pipe.model.model
        with torch.cuda.device(pipe.device), torch.no_grad():
            self._build(int(slots), float(uncond_scale), max_steps, context, bool(return_latent))

    def _check_mode(self):
        if self.dit.gemm == "exact":
            raise NotImplementedError("gemm='exact' decodes one visibility pattern per sampler call: a decode stream gives every slot its own key mask "
                                      "(run the stream with gemm='fp32' / 'f16x2', or use decoding)")

    def _build(self, slots, uncond_scale, max_steps, context, return_latent):
        pipe, dit, dev = self.pipe, self.dit, self.pipe.device
        self._check_mode()
        if dit.renderer:
            raise NotImplementedError("the renderer is one model pass, not a sampler: there is nothing to stream")
        K, flow = pipe.K, pipe.flow
        limit = np.minimum(np.asarray(pipe.k_table, dtype=np.int64) + 1, K)
        self.sched = SlotSchedule(slots, limit, K, max_steps, context)
        n, self.slots, self.K = self.sched.n_steps, slots, K
        self.uncond_scale, self.guided, self.return_latent = uncond_scale, uncond_scale != 1.0, return_latent
        self.x0_param = flow.parameterization == "x0"
        self.see_xt = not self.guided                                            # p_sample_loop: context_see_xt and not guided (decoding passes True)
        # the modulations of every scheduled timestep, once: [n, R] with R = 24 * 6H + 2H + 2H, and the same for the unconditional branch
        def table(t_freq):
            mx, mc, mf = dit.modulations(dit.time_embed(t_freq[:n].contiguous()), has_ctx=True)
            return torch.cat(list(mx) + [mc, mf], dim=1).contiguous(), [int(t.shape[1]) for t in list(mx) + [mc, mf]]
        with pipe._tunable_scope():
            self.table, widths = table(flow.t_freq)
            self.table_u = table(flow.t_freq_uncond)[0] if self.guided else None
        first = np.concatenate([[0], np.cumsum(widths)[:-1]])
        self.segs = np.ascontiguousarray(np.stack([first, widths], axis=1).astype(np.int32))
        self.R = int(sum(widths))
        self.limit = torch.from_numpy(limit[:n].astype(np.int32)).to(dev)
        self.coef = torch.from_numpy(np.stack([flow.dt[:n], flow.scheduled_t[:n], flow.scheduled_t_prev[:n], np.zeros(n, np.float32)], axis=1)
                                     .astype(np.float32)).contiguous().to(dev)
        L, H, n_words = pipe.datasize // 8, W.DIT_HIDDEN, (K + 31) // 32
        self.L = L
        self.x = torch.zeros(slots, 16, L, L, device=dev)
        self.noise0 = torch.zeros(slots, 16, L, L, device=dev)                   # the request's noise: an overflow restart starts from it again
        self.ctx0 = torch.zeros(slots, K, H, device=dev)
        self.cqkv0 = torch.zeros(slots, K, 3 * H, device=dev)                    # block 0's context QKV: step independent
        self.pattern_words = torch.zeros(slots, n_words, dtype=torch.int32, device=dev)
        self.kwords = torch.zeros(slots, n_words, dtype=torch.int32, device=dev)
        self.step_dev = torch.full((slots,), -1, dtype=torch.int32, device=dev)
        self.coef_rows = torch.zeros(slots, 4, device=dev)
        self._requests = [None] * slots                                          # slot -> (ids, pattern): what a restart needs
        self._fallback = set()                                                   # tickets that run on fp32 GEMMs after an overflow
        self.mods = self._mod_views(torch.zeros(slots * self.R, device=dev))
        self.mods_u = self._mod_views(torch.zeros(slots * self.R, device=dev)) if self.guided else None
        k0 = int(pipe.diti.to_indices(flow.t_long[:1])[0])
        self._ehs_mask = None if k0 >= K - 1 else (torch.arange(K, device=dev) <= k0)[None, :, None]
        pipe._tune_linears(slots * (2 if self.guided else 1), pipe.k_table, (L // 2) ** 2)

    def _mod_views(self, flat):
        """(flat buffer, the `mods` of MMDiTGPU.core as views of it): segment s is the contiguous [slots, width_s] tensor at slots * first_s"""
        views = [flat[self.slots * int(f): self.slots * int(f) + self.slots * int(w)].view(self.slots, int(w)) for f, w in self.segs]
        return flat, (views[:-2], views[-2], views[-1])

    free_slots = property(lambda self: self.sched.free_slots)
    in_flight = property(lambda self: self.sched.in_flight)

    def slot_of(self, ticket: int) -> int:
        return self.sched.ticket.index(ticket)

    # ---- admission -----------------------------------------------------------------------------------
    def submit(self, ids, noise=None, ar_partial=None, super_mask=None, prefix_k=None) -> int:
        """ids: [K] (or [1, K]) integer token ids; noise: [16, L, L] (default: one torch.randn(1, 16, L, L) draw from the global CPU generator);
        ar_partial / super_mask ([K]) / prefix_k: the request's visibility, as `decoding` takes them for one sample.  -> ticket"""
        with torch.cuda.device(self.pipe.device), torch.no_grad():
            return self._submit(ids, noise, ar_partial, super_mask, prefix_k)

    def _submit(self, ids, noise, ar_partial, super_mask, prefix_k):
        self._check_mode()
        K, pipe = self.K, self.pipe
        if self.sched.free_slots == 0:
            raise StreamFull(f"all {self.slots} slots are in flight: step() the stream until a request retires")
        ids = ids.reshape(1, -1)
        if ids.shape[1] != K:
            raise ValueError(f"a request is one row of {K} token ids, got {ids.shape[1]}")
        pattern, _ = request_pattern(K, 1, prefix_k, super_mask, ar_partial, False)
        row = np.ones(K, dtype=bool) if pattern is None else (torch.as_tensor(pattern).cpu().numpy().reshape(-1) != 0)
        if row.size != K:
            raise ValueError(f"super_mask has {row.size} entries, the tokenizer has K = {K} tokens")
        if prefix_k is not None:
            row = row & (np.arange(K) < int(prefix_k))
        xt = torch.randn(1, 16, self.L, self.L) if noise is None else torch.as_tensor(noise).reshape(1, 16, self.L, self.L)
        pos = np.nonzero(row)[0]
        ticket, slot = self.sched.submit(int(pos[0]) if pos.size else None)
        self._requests[slot] = (ids, row)
        self.noise0[slot:slot + 1].copy_(xt.to(self.pipe.device).float())
        self.pattern_words[slot:slot + 1].copy_(ops.pack_key_mask(torch.from_numpy(row[None]).to(pipe.device)))
        self._start(slot)
        return ticket

    def _start(self, slot: int) -> None:
        """(re)start the slot's request at step 0 in the GEMM mode in force: its context, block 0's context QKV, its noise, step = 0"""
        ids, _ = self._requests[slot]
        dit = self.dit
        with self.pipe._tunable_scope():
            ehs = self.pipe._codes(ids)
            if self._ehs_mask is not None:
                ehs = ehs * self._ehs_mask
            ctx0 = dit.embed_context(ehs)
            self.ctx0[slot:slot + 1].copy_(ctx0)
            self.cqkv0[slot:slot + 1].copy_(dit.block0_context_qkv(ctx0))
        self.x[slot:slot + 1].copy_(self.noise0[slot:slot + 1])
        self.step_dev[slot:slot + 1].fill_(0)

    # ---- one sampler step of every slot --------------------------------------------------------------
    def step(self):
        with torch.cuda.device(self.pipe.device), torch.no_grad(), self.pipe._tunable_scope():
            return self._step()

    def _launch(self):
        dit, K = self.dit, self.K
        n_live = self.sched.n_live()
        ops.stream_prepare(self.step_dev, self.limit, self.coef, self.pattern_words, self.table, self.table_u, self.segs, self.kwords, self.coef_rows,
                           self.mods[0], None if self.mods_u is None else self.mods_u[0], K=K)
        ctx = None if n_live == 0 else (self.ctx0 if n_live >= K else self.ctx0[:, :n_live].contiguous())
        y = dit.core(dit.embed_image(self.x), None, ctx, self.see_xt, cqkv0=self.cqkv0 if n_live > 0 else None, mods=self.mods[1],
                     kmask=self.kwords if n_live > 0 else None)
        yu = dit.core(dit.embed_image(self.x), None, None, False, mods=self.mods_u[1]) if self.guided else None
        ops.unpatchify_cfg_euler_rows(y, yu, self.x, self.coef_rows, self.step_dev, cfg_scale=self.uncond_scale, x0_param=self.x0_param)

    def _step(self):
        self._check_mode()
        dit = self.dit
        if self.sched.in_flight == 0:
            return []
        mode = (dit.gemm, dit.attention, dit.splitk)
        if self._fallback and mode[0] in dit.SPLIT_MODES:
            dit.set_gemm("fp32")
            try:
                self._launch()
            finally:
                dit.set_gemm(mode[0], attention=mode[1], splitk=mode[2])
        else:
            self._launch()
        done = self.sched.advance()
        if not done:
            return []
        # a retirement: the host waits here anyway, so this is where the sticky fp16-range flag of the split modes is read (_checked's contract)
        if mode[0] in dit.SPLIT_MODES and int(dit.overflow.item()) != 0:
            print(f"[selftok] {mode[0]} GEMM: activation outside the fp16 range -> restarting the {self.sched.in_flight} requests in flight with fp32 GEMMs")
            dit.overflow.zero_()
            dit.set_gemm("fp32")
            try:
                for slot in self.sched.restart():
                    self._fallback.add(self.sched.ticket[slot])
                    self._start(slot)
            finally:
                dit.set_gemm(mode[0], attention=mode[1], splitk=mode[2])
            return []
        slots = [s for _, s in done]
        latents = self.x[slots[0]:slots[0] + 1].clone() if len(slots) == 1 else torch.cat([self.x[s:s + 1] for s in slots])
        pixels = self.pipe._to_pixels(latents)                                   # the retirements of one step share one VAE call
        out = []
        for j, (ticket, slot) in enumerate(done):
            self.sched.retire(slot)
            self.step_dev[slot:slot + 1].fill_(-1)
            self._requests[slot] = None
            self._fallback.discard(ticket)
            out.append((ticket, pixels[j], latents[j]) if self.return_latent else (ticket, pixels[j]))
        return out

    def drain(self):
        out = []
        while self.in_flight:
            out.extend(self.step())
        return out
