"""Thin torch-tensor front end of the C ABI (include/selftok_hip.h).

Every function takes CUDA(=HIP) tensors, passes `data_ptr()`s and the current torch stream to
libselftok_hip.so, and returns torch tensors.  PyTorch is only the allocator / stream owner here.
"""
from __future__ import annotations

import collections
import functools
from typing import Optional

import numpy as np
import torch

from . import _lib

IDS_I32 = 1
PRENORMED = 2
VQ_F16COARSE = 8     # packed path: f16 coarse pass + exact fp32 re-score (same ids / score bits, ~4x faster than the fp32-MFMA kernel)
VQ_F16COARSE1 = 16   # with VQ_F16COARSE: ONE MFMA per 32 x 32 scores (hi x hi) and a wider exact re-score window (same ids / score bits)
VQ_DEFAULT_COARSE = True
VQ_COARSE_MFMAS = 1  # MFMAs per 32 x 32 coarse scores when `coarse` is True / None: 1 (hi x hi, window 17 x 2^-14; round 4: 0.115 -> 0.079 ms at
                     # N = 32768, profiles/r4_vq_bench_1mfma.txt) or 3 (hi*hi + hi*lo + lo*hi, window 2^-17)


def _coarse_flags(coarse) -> int:
    """coarse: None -> the defaults, False -> fp32-input MFMA kernel, True -> f16 coarse pass with VQ_COARSE_MFMAS, 3 / 1 -> that variant"""
    if coarse is None:
        coarse = VQ_DEFAULT_COARSE
    if coarse is False or coarse == 0:
        return 0
    n = VQ_COARSE_MFMAS if coarse is True else int(coarse)
    if n not in (1, 3):
        raise ValueError(f"coarse = {coarse!r}: expected None, False, True, 1 or 3")
    return VQ_F16COARSE | (VQ_F16COARSE1 if n == 1 else 0)
VQ_EVENTS = None     # bench.py sets this to a list: vq_encode(packed=True) then appends (start, after main kernel, after finalize) HIP events


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _need_cuda(*ts):
    """every op launches on the CURRENT device's current stream: tensors on another GPU are refused (a kernel launched on
    GPU 0's stream against GPU 1 pointers would fault or race) -- SelftokPipeline's entry points select their device themselves
    (`with torch.cuda.device(...)`); direct callers of ops.* must do the same."""
    cur = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise _lib.SelftokHipError("selftok HIP ops need device tensors (there is no CPU fallback)")
        if cur is None:
            cur = torch.cuda.current_device()            # once per op, not once per tensor (host-bound small-batch decode loop)
        if t.device.index != cur:
            raise _lib.SelftokHipError(f"tensor on {t.device} but the current device is cuda:{cur}: "
                                       "call torch.cuda.set_device / use `with torch.cuda.device(...)` first")


def _p(t):
    return None if t is None else t.data_ptr()


class _StreamWorkspace:
    """a pool of byte workspaces: (device index, stream handle) -> tensors, largest last.  Grown on demand (never below `floor` bytes) and reused by the calls of
    THAT stream (they are ordered); two streams never share one (their kernels could overlap); outgrown tensors stay referenced (a captured hipGraph may replay
    on them)."""

    def __init__(self, floor: int):
        self.floor, self.held = floor, {}

    def __call__(self, device, nbytes: int) -> torch.Tensor:
        held = self.held.setdefault((device.index, int(torch.cuda.current_stream(device).cuda_stream)), [])
        if not held or held[-1].numel() < nbytes:
            held.append(torch.empty(max(nbytes, self.floor), dtype=torch.uint8, device=device))
        return held[-1]


def _ws_bytes(entry: str, *args) -> int:
    """the size query `entry` of the library; 0 means refused: raises with the library's message"""
    n = getattr(_lib.load(), entry)(*args)
    if n == 0:
        _lib.check(-1, entry)
    return n


def _out(what: str, out: Optional[torch.Tensor], dtype, shape, device, name: str = "out") -> torch.Tensor:
    """`out` checked to be a contiguous `dtype` tensor of `shape`, or a fresh one when None"""
    shape = tuple(shape)
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != shape or not out.is_contiguous():
        raise _lib.SelftokHipError(f"{what}: `{name}` must be a contiguous {str(dtype).replace('torch.', '')} {list(shape)}, got {out.dtype} {tuple(out.shape)}")
    return out


def _image_pair(what: str, recon: torch.Tensor, original: torch.Tensor):
    """two [B, 3, H, W] tensors of one shape, bf16 or fp32 each -> both contiguous"""
    for name, t in (("recon", recon), ("original", original)):
        if t.dtype not in (torch.bfloat16, torch.float32):
            raise _lib.SelftokHipError(f"{what}: `{name}` dtype {t.dtype}: expected bfloat16 or float32")
    if recon.dim() != 4 or recon.shape[1] != 3 or tuple(original.shape) != tuple(recon.shape):
        raise _lib.SelftokHipError(f"{what}: expected two [B, 3, H, W] tensors of one shape, got {tuple(recon.shape)} and {tuple(original.shape)}")
    return recon.contiguous(), original.contiguous()


def vq_pack_codebook(codebook: torch.Tensor) -> torch.Tensor:
    """[C,16] fp32 -> MFMA-fragment-ordered copy (one-time, the codebook is a constant)."""
    _need_cuda(codebook)
    cb = codebook.contiguous().float()
    C, D = cb.shape
    lib = _lib.load()
    packed = torch.zeros(lib.selftok_vq_packed_bytes(C, D) // 4, dtype=torch.float32, device=cb.device)
    _lib.check(lib.selftok_vq_pack_codebook(_p(cb), _p(packed), C, D, _stream()), "selftok_vq_pack_codebook")
    return packed


def packed_codes(packed: torch.Tensor, D: int = 16) -> int:
    """number of codes in a vq_pack_codebook image: C*D fp32 + 64 metadata floats + C*D fp16 hi/lo pairs (= C*D more floats)"""
    return (packed.numel() - 64) // (2 * D)


def vq_encode(z: torch.Tensor, codebook: torch.Tensor, *, packed: bool = False, return_best: bool = False,
              ids_dtype=torch.int64, prenormed: bool = False, rt: int = 0, split: int = 0, coarse=None):
    """z [...,16] fp32 (pre-norm) , codebook [C,16] (raw, or packed if packed=True) -> ids [...].
    rt / split: launch-shape overrides of the packed path (SELFTOK_VQ_RT / SELFTOK_VQ_SPLIT; 0 = automatic).
    coarse (packed path): True = f16 coarse pass + exact re-score (SELFTOK_VQ_F16COARSE) with VQ_COARSE_MFMAS MFMAs per 32 x 32 scores,
    3 / 1 = that variant explicitly (1 = SELFTOK_VQ_F16COARSE1), False = fp32-input MFMA kernel; None = VQ_DEFAULT_COARSE.  All return
    identical ids and score bits."""
    _need_cuda(z, codebook)
    lib = _lib.load()
    cflags = _coarse_flags(coarse) if packed else 0
    if packed and VQ_EVENTS is not None and not return_best and not prenormed and z.numel() > 0:
        # same two launches as selftok_vq_encode_packed_f32, with HIP events around the argmax kernel on its launch stream
        ids, launch_main, launch_fin = vq_encode_split_launch(z, codebook, ids_dtype, _flags=cflags)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        launch_main()
        e1.record()
        launch_fin()
        e2.record()
        VQ_EVENTS.append((e0, e1, e2))
        return ids
    zz = z.contiguous().float().reshape(-1, z.shape[-1])
    N, D = zz.shape
    C = packed_codes(codebook, D) if packed else codebook.shape[0]
    ids = torch.empty(N, dtype=ids_dtype, device=z.device)
    best = torch.empty(N, dtype=torch.float32, device=z.device) if return_best else None
    ws = torch.empty(lib.selftok_vq_workspace_bytes(N, C), dtype=torch.uint8, device=z.device)
    flags = ((IDS_I32 if ids_dtype == torch.int32 else 0) | (PRENORMED if prenormed else 0) | ((rt & 0xF) << 8) | ((split & 0xFF) << 16)
             | cflags)
    fn = lib.selftok_vq_encode_packed_f32 if packed else lib.selftok_vq_encode_f32
    _lib.check(fn(_p(zz), _p(codebook), _p(ids), _p(best), _p(ws), N, C, D, flags, _stream()),
               "selftok_vq_encode_packed_f32" if packed else "selftok_vq_encode_f32")
    ids = ids.reshape(z.shape[:-1])
    if return_best:
        return ids, best.reshape(z.shape[:-1])
    return ids


def vq_topk(z: torch.Tensor, packed_codebook: torch.Tensor, k: int, ids_dtype=torch.int64, prenormed: bool = False, *, rt: int = 0, split: int = 0):
    """z [...,16] fp32 (pre-norm), packed code book (vq_pack_codebook) -> (ids [...,k], scores [...,k] fp32): the k <= 8 best codes of every
    row and their canonical scores, ordered by score descending, equal scores by ascending index, NaN scores first (the order is defined
    by include/selftok_hip_ext.h, not torch.topk's).  [..., 0] is bit for bit vq_encode(..., return_best=True).  The [N, C] score matrix is
    never materialised.  rt / split: launch-shape overrides (SELFTOK_VQ_RT / SELFTOK_VQ_SPLIT; 0 = automatic), never visible in the result."""
    _need_cuda(z, packed_codebook)
    if ids_dtype not in (torch.int64, torch.int32):
        raise TypeError(f"ids_dtype must be torch.int64 or torch.int32, got {ids_dtype}")
    lib = _lib.load()
    k = int(k)
    zz = z.contiguous().float().reshape(-1, z.shape[-1])
    N, D = zz.shape
    C = packed_codes(packed_codebook, D)
    ids = torch.empty((N, max(k, 0)), dtype=ids_dtype, device=z.device)
    scores = torch.empty((N, max(k, 0)), dtype=torch.float32, device=z.device)
    ws = torch.empty(lib.selftok_vq_topk_workspace_bytes(N, C, k), dtype=torch.uint8, device=z.device)
    flags = (IDS_I32 if ids_dtype == torch.int32 else 0) | (PRENORMED if prenormed else 0) | ((rt & 0xF) << 8) | ((split & 0xFF) << 16)
    _lib.check(lib.selftok_vq_topk_packed_f32(_p(zz), _p(packed_codebook), _p(ids), _p(scores), _p(ws), N, C, D, k, flags, _stream()),
               "selftok_vq_topk_packed_f32")
    return ids.reshape(z.shape[:-1] + (k,)), scores.reshape(z.shape[:-1] + (k,))


def vq_ema_accumulate(z: torch.Tensor, ids: torch.Tensor, C: int, prenormed: bool = False):
    """(bins [C], embed_sum [C,16]) of one batch: bins[c] = #rows with id c, embed_sum[c] = sum of their l2-normalised features
    (the reference's one-hot contractions, vector_quantize_pytorch.py:587-593)."""
    _need_cuda(z, ids)
    zz = z.contiguous().float().reshape(-1, z.shape[-1])
    flat = ids.contiguous().reshape(-1)
    if flat.dtype not in (torch.int32, torch.int64):
        flat = flat.to(torch.int64)
    assert flat.numel() == zz.shape[0]
    bins = torch.zeros(C, dtype=torch.float32, device=z.device)
    esum = torch.zeros(C, zz.shape[1], dtype=torch.float32, device=z.device)
    flags = (IDS_I32 if flat.dtype == torch.int32 else 0) | (PRENORMED if prenormed else 0)
    _lib.check(_lib.load().selftok_vq_ema_accumulate_f32(_p(zz), _p(flat), _p(bins), _p(esum), zz.shape[0], C, zz.shape[1], flags, _stream()),
               "selftok_vq_ema_accumulate_f32")
    return bins, esum


def vq_softmax_stats(z: torch.Tensor, codebook: torch.Tensor, scale: float = 10.0, colmean: bool = True, prenormed: bool = False):
    """The two reductions of p = softmax_c(scale * <l2norm(z[b,k]), codebook[c]>) that the reference's entropy regularisers read from
    its materialised [B, K, C] tensor (calc_entropy / calc_ema_entropy, vector_quantize_pytorch.py:89-118): z [B,K,16] ->
    (rowstats [B*K, 2] = (1 / sum_c exp, H(p[b,k,:])), colmean [K, C] = mean_b p[b,k,:] or None)."""
    _need_cuda(z, codebook)
    assert z.dim() == 3 and codebook.dim() == 2 and z.shape[-1] == codebook.shape[1]
    zz, cb = z.contiguous().float(), codebook.contiguous().float()
    B, K, Dm = zz.shape
    C = cb.shape[0]
    lib = _lib.load()
    rows = torch.empty(B * K, 2, dtype=torch.float32, device=z.device)
    cm = torch.empty(K, C, dtype=torch.float32, device=z.device) if colmean else None
    ws = torch.empty(lib.selftok_vq_softmax_workspace_bytes(B * K), dtype=torch.uint8, device=z.device)
    _lib.check(lib.selftok_vq_softmax_stats_f32(_p(zz), _p(cb), _p(rows), _p(cm), _p(ws), B, K, C, Dm, float(scale), PRENORMED if prenormed else 0, _stream()),
               "selftok_vq_softmax_stats_f32")
    return rows, cm


def vq_softmax_backward(z: torch.Tensor, codebook: torch.Tensor, rowstats: torch.Tensor, g_colmean: torch.Tensor, scale: float = 10.0,
                        prenormed: bool = False) -> torch.Tensor:
    """dF/dz [B,K,16] for a scalar F of vq_softmax_stats' colmean, given g_colmean = dF/d(colmean) [K, C] (code book detached)."""
    _need_cuda(z, codebook, rowstats, g_colmean)
    zz, cb, g = z.contiguous().float(), codebook.contiguous().float(), g_colmean.contiguous().float()
    B, K, Dm = zz.shape
    C = cb.shape[0]
    assert tuple(g.shape) == (K, C) and tuple(rowstats.shape) == (B * K, 2) and rowstats.is_contiguous() and rowstats.dtype == torch.float32
    lib = _lib.load()
    grad = torch.empty_like(zz)
    ws = torch.empty(lib.selftok_vq_softmax_workspace_bytes(B * K), dtype=torch.uint8, device=z.device)
    _lib.check(lib.selftok_vq_softmax_backward_f32(_p(zz), _p(cb), _p(rowstats), _p(g), _p(grad), _p(ws), B, K, C, Dm, float(scale),
                                                   PRENORMED if prenormed else 0, _stream()), "selftok_vq_softmax_backward_f32")
    return grad


def vq_tpc_update_(tpc: torch.Tensor, ids: torch.Tensor, weight: float) -> torch.Tensor:
    """in place: tpc [K,C] <- lerp(tpc, mean over samples of one_hot(ids [B,K]), weight)  (vector_quantize_pytorch.py:568-578)"""
    _need_cuda(tpc, ids)
    assert tpc.is_contiguous() and tpc.dtype == torch.float32 and ids.dim() == 2 and ids.shape[1] == tpc.shape[0]
    flat = ids.contiguous()
    if flat.dtype not in (torch.int32, torch.int64):
        flat = flat.to(torch.int64)
    K, C = tpc.shape
    _lib.check(_lib.load().selftok_vq_tpc_update_f32(_p(tpc), _p(flat), flat.shape[0], K, C, float(weight), IDS_I32 if flat.dtype == torch.int32 else 0,
                                                     _stream()), "selftok_vq_tpc_update_f32")
    return tpc


def code_gather_ln(ids: torch.Tensor, codebook: torch.Tensor, ln_w=None, ln_b=None, eps: float = 1e-6) -> torch.Tensor:
    """ids [...] (int64/int32) -> LayerNorm16(codebook[ids]) [...,16]"""
    _need_cuda(ids, codebook)
    if ids.is_floating_point() or ids.is_complex() or ids.dtype == torch.bool:
        raise TypeError(f"code_gather_ln: ids must be an integer tensor, got {ids.dtype}")
    if ids.dtype not in (torch.int32, torch.int64):
        ids = ids.to(torch.int64)                      # uint16 / int16 / uint8 wire formats: the kernel reads 4- or 8-byte ids only
    flat = ids.contiguous().reshape(-1)
    n = flat.numel()
    C, D = codebook.shape
    out = torch.empty(n, D, dtype=torch.float32, device=ids.device)
    flags = IDS_I32 if flat.dtype == torch.int32 else 0
    _lib.check(_lib.load().selftok_code_gather_ln_f32(_p(flat), _p(codebook), _p(ln_w), _p(ln_b), _p(out), n, C, D,
                                                      eps, flags, _stream()), "selftok_code_gather_ln_f32")
    return out.reshape(*ids.shape, D)


# ----------------------------------------------------------------------------------------------
# fused epilogues (csrc/elementwise.hip)
# ----------------------------------------------------------------------------------------------

def _table_strides(t, per_sample: bool, B: int, T: int, H: int):
    """a modulation / gate table of a [B,T,H] tensor -- a 2-D view [T,H] (per token) or [B,H] (per_sample) with unit inner stride, or
    None -> its (stride_b, stride_t) as the kernels take them"""
    if t is None:
        return 0, 0
    assert t.dim() == 2 and t.stride(1) == 1 and t.shape == ((B, H) if per_sample else (T, H))
    return (t.stride(0), 0) if per_sample else (0, t.stride(0))


def residual_ln_mod(x, *, y=None, gate=None, shift=None, scale=None, per_sample=False, gate_per_sample=None,
                    want_x=True, want_n=True, eps=1e-6, split=False, overflow=None):
    """x' = x + gate*y ; n = LN(x')*(1+scale)+shift.   x,y [B,T,H].  shift/scale/gate are 2-D views
    [T,H] (per token, default) or [B,H] (per_sample=True) -- typically column slices of a [*,6H] table.
    Returns (x', n) (either may be None).  split=True: n comes back as a SplitAct [B,T,H] for linear_f16x2_split; `overflow` bit 0
    is raised if |n| >= 65504."""
    _need_cuda(x)
    B, T, H = x.shape
    assert x.is_contiguous() and x.dtype == torch.float32

    if shift is not None:
        assert scale is not None and shift.stride(0) == scale.stride(0)
    msb, mst = _table_strides(shift, per_sample, B, T, H)
    gsb, gst = _table_strides(gate, per_sample if gate_per_sample is None else gate_per_sample, B, T, H)
    if y is not None:
        assert y.is_contiguous() and y.shape == x.shape
    x_out = torch.empty_like(x) if (y is not None and want_x) else None
    if split and want_n:
        n_s = SplitAct((B, T, H), x.device)
        _lib.check(_lib.load().selftok_residual_ln_mod_split(_p(x), _p(y), _p(gate), _p(shift), _p(scale), _p(x_out), _p(n_s.data),
                                                             _p(overflow), B, T, H, msb, mst, gsb, gst, eps, _stream()), "selftok_residual_ln_mod_split")
        return (x_out if y is not None else x), n_s
    n_out = torch.empty_like(x) if want_n else None
    _lib.check(_lib.load().selftok_residual_ln_mod_f32(_p(x), _p(y), _p(gate), _p(shift), _p(scale), _p(x_out), _p(n_out),
                                                       B, T, H, msb, mst, gsb, gst, eps, _stream()), "selftok_residual_ln_mod_f32")
    return (x_out if y is not None else x), n_out


def bias_gelu_(h, bias=None):
    _need_cuda(h)
    assert h.is_contiguous() and h.dtype == torch.float32
    cols = h.shape[-1]
    _lib.check(_lib.load().selftok_bias_gelu_f32(_p(h), _p(bias), h.numel() // cols, cols, _stream()), "selftok_bias_gelu_f32")
    return h


def linear_gelu(x, weight, bias):
    """gelu_tanh(x @ weight.T + bias) -- Mlp.fc1 + act (sd3/other_impls.py:86-88; timm Mlp modules.py:109,293).
    The bias add and the tanh-GELU ride in hipBLASLt's GEMM epilogue (one pass less over the [rows, 4H] hidden tensor:
    -8 % per MLP GEMM, measured equal to GEMM + selftok_bias_gelu_f32 to 5e-7); `bias_gelu_` remains the stand-alone kernel."""
    _need_cuda(x, weight)
    shp = x.shape
    out = torch._addmm_activation(bias, x.reshape(-1, shp[-1]), weight.t(), use_gelu=True)
    return out.reshape(*shp[:-1], weight.shape[0])


# ----------------------------------------------------------------------------------------------
# fp32-equivalent Linear on the f16 matrix cores (csrc/gemm_split.hip)
# ----------------------------------------------------------------------------------------------
LINEAR_GELU = 1


def linear_f16x2_supported(N: int, K: int) -> bool:
    return N % 128 == 0 and K % 32 == 0


def linear_f16x2_pack(weight: torch.Tensor, overflow: torch.Tensor = None) -> torch.Tensor:
    """nn.Linear weight [N,K] fp32 -> the kernel's split/tiled fp16 image (4*N*K bytes).  One-time, at load.
    `overflow` (int32 [1], device): bit 1 is set if a weight is outside the fp16 range."""
    _need_cuda(weight)
    w = weight.contiguous().float()
    N, K = w.shape
    lib = _lib.load()
    nbytes = lib.selftok_linear_f16x2_packed_bytes(N, K)
    if nbytes == 0:
        raise _lib.SelftokHipError(f"linear_f16x2: weight {N}x{K} needs N % 128 == 0 and K % 32 == 0")
    packed = torch.empty(nbytes // 2, dtype=torch.float16, device=w.device)
    _lib.check(lib.selftok_linear_f16x2_pack_weight(_p(w), _p(packed), N, K, _p(overflow), _stream()), "selftok_linear_f16x2_pack_weight")
    return packed


def _rows16(x: torch.Tensor):
    """x [..., K] fp32 -> ([rows, K] view, row stride) that a kernel can read with 16-byte loads; a copy where the view cannot be"""
    K = x.shape[-1]
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1 or (x2.shape[0] > 1 and (x2.stride(0) % 4 or x2.stride(0) < K)) or x2.data_ptr() % 16:
        x2 = x2.contiguous()
    return x2, (x2.stride(0) if x2.shape[0] > 1 else K)


def linear_f16x2(x: torch.Tensor, packed: torch.Tensor, bias, N: int, gelu: bool = False, overflow: torch.Tensor = None) -> torch.Tensor:
    """act(x @ W.T + bias) with W given as linear_f16x2_pack(W).  x [..., K] fp32 (rows may be strided), out [..., N] fp32."""
    _need_cuda(x, packed)
    K = x.shape[-1]
    assert x.dtype == torch.float32 and packed.numel() * 2 == 4 * N * K, "packed weight does not match (N, K)"
    x2, lda = _rows16(x)
    M = x2.shape[0]
    out = torch.empty(M, N, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().selftok_linear_f16x2_f32(_p(x2), lda, _p(packed), _p(bias), _p(out), N, M, N, K,
                                                    LINEAR_GELU if gelu else 0, _p(overflow), _stream()), "selftok_linear_f16x2_f32")
    return out.reshape(*x.shape[:-1], N)


class SplitAct:
    """A "split activation" (include/selftok_hip.h): the fp32 tensor of logical `shape` [..., K] held as fp16 hi / lo planes in
    1-KiB chunks of 16 rows x 32 k, `data` = fp16 [ceil(rows/16), K/32, 2, 16, 32].  What the fused producers (residual_ln_mod,
    attention, the f16x2 Linear's epilogue) write and linear_f16x2_split consumes; `dtype` is torch.float16 so that callers can
    tell it from an fp32 tensor the way they tell dtypes apart."""
    dtype = torch.float16

    def __init__(self, shape, device, zero: bool = False):
        self.shape = tuple(int(v) for v in shape)
        K = self.shape[-1]
        assert K % 32 == 0, "split activations need K % 32 == 0"
        self.rows = 1
        for v in self.shape[:-1]:
            self.rows *= v
        self.data = (torch.zeros if zero else torch.empty)((self.rows + 15) // 16, K // 32, 2, 16, 32, dtype=torch.float16, device=device)

    @property
    def device(self):
        return self.data.device

    def planes(self) -> torch.Tensor:
        """un-blocked copy fp16 [2, *shape] (hi, lo): tests / debugging"""
        K = self.shape[-1]
        p = self.data.permute(2, 0, 3, 1, 4).reshape(2, -1, K)[:, :self.rows]
        return p.reshape(2, *self.shape)


def split_f16x2(x: torch.Tensor, overflow: torch.Tensor = None) -> SplitAct:
    """fp32 [..., K] -> SplitAct: hi = fp16(x), lo = fp16((x - hi) * 2^11).  The stand-alone producer, for inputs no fused producer
    makes.  `overflow` bit 0 is raised for |x| >= 65504."""
    _need_cuda(x)
    x2, ld = _rows16(x)
    out = SplitAct(x.shape, x.device)
    _lib.check(_lib.load().selftok_split_f16x2_f32(_p(x2), ld, _p(out.data), out.rows, x.shape[-1],
                                                   _p(overflow), _stream()), "selftok_split_f16x2_f32")
    return out


def split_to_f32(xs: SplitAct) -> torch.Tensor:
    """the fp32 value a split activation stands for (tests / debugging)"""
    p = xs.planes()
    return p[0].float() + p[1].float() * (1.0 / 2048.0)


@functools.lru_cache(maxsize=None)
def _cu_count() -> int:
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count) if torch.cuda.is_available() else 256


SPLITK_MAX_ROWS = 1024      # rows up to which the block Linears of the f16x2 mode are worth splitting along K (one .. four images)


@functools.lru_cache(maxsize=4096)
def f16x2_ksplit(M: int, N: int, K: int) -> int:
    """how many work-groups should share an output tile of a [M, K] x [K, N] f16x2 Linear: 1 = the single-pass kernel.  Small M only
    (<= SPLITK_MAX_ROWS): the 256 x 128 tile grid then leaves most of the 256 CUs idle while each work-group walks all of K.  Among
    the divisors s of K / 32 that keep the grid within one work-group per CU (a second round of work-groups costs ~10 us:
    profiles/r4_splitk_sweep.txt) and >= 3 k-tiles per work-group (the DMA pipeline depth), the minimum of a two-term cost fitted to
    that sweep: 0.42 us per k-tile of the longest chain + 1.2 us per million fp32 partials written and re-read, + 4 us for the
    second launch.  NOTE: the split is chosen from M = batch rows, and a split-K sum rounds differently from the single pass -- in f16x2
    mode an image decoded at B <= 4 and at B > 4 differs at fp32 rounding level (1e-7 relative per Linear; the fp32 mode and every encode
    path are batch independent).  The cost constants are one MI355X sweep; the CU count comes from the device."""
    if M <= 0 or M > SPLITK_MAX_ROWS:
        return 1
    tiles = ((M + 255) // 256) * (N // 128)
    kt = K // 32
    cus = _cu_count()
    best, best_cost = 1, 0.42 * kt
    for s in range(2, 65):
        if kt % s or kt // s < 3 or tiles * s > cus:
            continue
        cost = 0.42 * (kt // s) + 1.2e-6 * s * M * N + 4.0
        if cost < best_cost:
            best, best_cost = s, cost
    return best


def _linear_split(xs: SplitAct, packed: torch.Tensor, bias, N: int, *, single_pass: bool, gelu: bool = False, out_split: bool = False, resid=None,
                  gate=None, gate_per_sample: bool = False, ksplit: Optional[int] = None, overflow: torch.Tensor = None):
    """the Linear on a split activation, every form.  Arithmetic: `single_pass` = the fp16 kernels (hi planes only, LOSSY) instead of the f16x2
    kernels.  Route along K, four combinations: f16x2 -> the _k entries of csrc/gemm_split.hip with `ksplit` parts (None = 1, their single
    launch); single_pass with ksplit None -> the plain entries of csrc/gemm_f16.hip; single_pass with a `ksplit` -> the _k entries of
    csrc/gemm_f16_splitk.hip (1 forwards to the plain entry inside the library).  Epilogue = `gelu` / `out_split`, or with `resid` [B,T,N] the
    fused residual update resid + gate * y.  Returns fp32 [..., N], a SplitAct [..., N], or a tensor like resid."""
    _need_cuda(xs.data, packed, resid)
    K = xs.shape[-1]
    assert packed.numel() * 2 == 4 * N * K, "packed weight does not match (N, K)"
    M, lead = xs.rows, xs.shape[:-1]
    lib = _lib.load()
    name = "selftok_linear_f16_split" if single_pass else "selftok_linear_f16x2_split"
    tail = (_p(overflow), _stream())
    k_entry = not single_pass or ksplit is not None       # the _k entries; ksplit == 1 is their single launch
    if k_entry:
        ksplit = 1 if ksplit is None else int(ksplit)
        ws = torch.empty(ksplit * M * N, dtype=torch.float32, device=xs.device) if (ksplit > 1 and M > 0) else None
        tail = (ksplit, _p(ws)) + tail
    if resid is not None:
        assert not gelu and not out_split
        assert resid.dim() == 3 and resid.is_contiguous() and resid.dtype == torch.float32 and resid.shape[-1] == N
        B, T, _ = resid.shape
        assert M == B * T
        gsb, gst = _table_strides(gate, gate_per_sample, B, T, N)
        out = torch.empty_like(resid)
        name += "_residual_k" if k_entry else "_residual"
        _lib.check(getattr(lib, name)(_p(xs.data), _p(packed), _p(bias), _p(resid), N, _p(gate), gsb, gst, T, _p(out), N, M, N, K, *tail), name)
        return out
    out = SplitAct((*lead, N), xs.device) if out_split else torch.empty(M, N, dtype=torch.float32, device=xs.device)
    name += "_k" if k_entry else ""
    _lib.check(getattr(lib, name)(_p(xs.data), _p(packed), _p(bias), None if out_split else _p(out), _p(out.data) if out_split else None, N, M, N, K,
                                  LINEAR_GELU if gelu else 0, *tail), name)
    return out if out_split else out.reshape(*lead, N)


def linear_f16x2_split(xs: SplitAct, packed: torch.Tensor, bias, N: int, gelu: bool = False, overflow: torch.Tensor = None,
                       out_split: bool = False, ksplit: int = 1):
    """linear_f16x2 on a split activation: both operands reach LDS by LDS-DMA.  Returns fp32 [..., N], or with out_split a SplitAct
    [..., N] for the next Linear.  Same results as linear_f16x2 on the fp32 tensor.  ksplit > 1 (small M, `f16x2_ksplit`): that many
    work-groups per output tile + a reduction launch; deterministic, equal to the single-pass result up to fp32 rounding of the
    partial sums (selftok_linear_f16x2_split_k)."""
    return _linear_split(xs, packed, bias, N, single_pass=False, gelu=gelu, out_split=out_split, ksplit=ksplit, overflow=overflow)


def linear_f16x2_split_residual(xs: SplitAct, packed: torch.Tensor, bias, N: int, resid: torch.Tensor, gate=None,
                                gate_per_sample: bool = False, overflow: torch.Tensor = None, ksplit: int = 1) -> torch.Tensor:
    """resid + gate * (xs @ W.T + bias): linear_f16x2_split with the block's residual update fused into the epilogue.
    resid [B,T,N] fp32 contiguous; gate a 2-D view [T,N] (per token) or [B,N] (gate_per_sample) with unit inner stride, or None.
    Bit-identical to residual_ln_mod(resid, y=linear_f16x2_split(...), gate=gate)[0]."""
    return _linear_split(xs, packed, bias, N, single_pass=False, resid=resid, gate=gate, gate_per_sample=gate_per_sample, ksplit=ksplit, overflow=overflow)


# ----------------------------------------------------------------------------------------------
# single-pass fp16 Linear on the same split planes (csrc/gemm_f16.hip): the LOSSY "f16" GEMM mode
# ----------------------------------------------------------------------------------------------
def _as_split(x, overflow) -> SplitAct:
    return x if isinstance(x, SplitAct) else split_f16x2(x, overflow)


def linear_f16_split(xs, packed: torch.Tensor, bias, N: int, gelu: bool = False, overflow: torch.Tensor = None, out_split: bool = False):
    """act(fp16(x) @ fp16(W).T + bias) with fp32 accumulation: linear_f16x2_split with both low planes taken as zero -- fp16-rounded
    operands, one matrix instruction per product instead of three.  LOSSY (11 significand bits per operand), not fp32-equivalent.
    `xs`: a SplitAct, or an fp32 tensor [..., K] (fed through split_f16x2); `packed`: linear_f16x2_pack(W), the same image the
    f16x2 mode holds -- only the hi planes of both are read.  Returns fp32 [..., N], or with out_split a SplitAct with both planes.
    On fp16-representable operands the result equals linear_f16x2_split's.  This entry walks all of K in one work-group per tile: by
    default callers keep row counts <= SPLITK_MAX_ROWS on linear_f16x2_split(..., ksplit=f16x2_ksplit(...)) (MMDiTGPU.lin does); the
    opt-in split-K form in this arithmetic is linear_f16_split_k."""
    return _linear_split(_as_split(xs, overflow), packed, bias, N, single_pass=True, gelu=gelu, out_split=out_split, overflow=overflow)


def linear_f16_split_residual(xs, packed: torch.Tensor, bias, N: int, resid: torch.Tensor, gate=None,
                              gate_per_sample: bool = False, overflow: torch.Tensor = None) -> torch.Tensor:
    """resid + gate * linear_f16_split(xs): the fused residual epilogue of linear_f16x2_split_residual (same operations, same order)
    on the single-pass fp16 product.  Arguments as there; `xs` may be an fp32 tensor."""
    return _linear_split(_as_split(xs, overflow), packed, bias, N, single_pass=True, resid=resid, gate=gate, gate_per_sample=gate_per_sample, overflow=overflow)


# the cost model of f16_ksplit, fitted to profiles/f16_splitk_sweep.txt (tools/sweep_splitk.py --f16): us per k-tile of the longest chain,
# us per fp32 partial written and re-read, us for the second launch, fewest k-tiles per part.  None: no sweep yet -> f16x2_ksplit's choice.
# The fit: over the 16 swept (rows, Linear) cases the choice costs 1.4 us in all over the best swept split, 3 % at worst (qkv at 256 rows);
# a k-tile costs about half of what it costs the f16x2 kernel (0.42 us), so fewer parts pay for their partial planes than there.
F16_SPLITK_COST = (0.23, 1.2e-6, 2.0, 3)


@functools.lru_cache(maxsize=4096)
def f16_ksplit(M: int, N: int, K: int) -> int:
    """how many work-groups should share an output tile of a [M, K] x [K, N] Linear on the single-pass fp16 split-K kernel
    (linear_f16_split_k): the divisor rule of f16x2_ksplit -- a divisor of K / 32 in 1 .. 64 that keeps the grid within one work-group per
    CU, 1 above SPLITK_MAX_ROWS -- with the cost constants of F16_SPLITK_COST.  A pure function of (M, N, K, CU count)."""
    if M <= 0 or M > SPLITK_MAX_ROWS:
        return 1
    if F16_SPLITK_COST is None:
        return f16x2_ksplit(M, N, K)
    per_tile, per_partial, second, min_tiles = F16_SPLITK_COST
    tiles = ((M + 255) // 256) * (N // 128)
    kt = K // 32
    cus = _cu_count()
    best, best_cost = 1, per_tile * kt
    for s in range(2, 65):
        if kt % s or kt // s < min_tiles or tiles * s > cus:
            continue
        cost = per_tile * (kt // s) + per_partial * s * M * N + second
        if cost < best_cost:
            best, best_cost = s, cost
    return best


def linear_f16_split_k(xs, packed: torch.Tensor, bias, N: int, ksplit: int, gelu: bool = False, overflow: torch.Tensor = None, out_split: bool = False):
    """linear_f16_split with `ksplit` work-groups per output tile and a reduction launch (selftok_linear_f16_split_k, csrc/gemm_f16_splitk.hip):
    for row counts <= SPLITK_MAX_ROWS, ksplit = f16_ksplit(M, N, K).  LOSSY like linear_f16_split, deterministic; with r = fp16 rounding
    equal to linear_f16x2_split(r(x), pack(r(W)), ksplit=ksplit) bit for bit.  ksplit must divide K / 32 and be <= 64; 1 is linear_f16_split."""
    return _linear_split(_as_split(xs, overflow), packed, bias, N, single_pass=True, gelu=gelu, out_split=out_split, ksplit=int(ksplit), overflow=overflow)


def linear_f16_split_residual_k(xs, packed: torch.Tensor, bias, N: int, resid: torch.Tensor, ksplit: int, gate=None,
                                gate_per_sample: bool = False, overflow: torch.Tensor = None) -> torch.Tensor:
    """resid + gate * linear_f16_split_k(xs): linear_f16_split_residual with `ksplit` parts along K (selftok_linear_f16_split_residual_k)."""
    return _linear_split(_as_split(xs, overflow), packed, bias, N, single_pass=True, resid=resid, gate=gate, gate_per_sample=gate_per_sample,
                         ksplit=int(ksplit), overflow=overflow)


def silu(x):
    _need_cuda(x)
    x = x.contiguous()
    out = torch.empty_like(x)
    _lib.check(_lib.load().selftok_silu_f32(_p(x), _p(out), x.numel(), _stream()), "selftok_silu_f32")
    return out


def add_rows_(x, table):
    """x[b] += table for every b (in place). x [B,...], table [...] contiguous."""
    _need_cuda(x, table)
    assert x.is_contiguous() and table.is_contiguous() and x[0].numel() == table.numel()
    _lib.check(_lib.load().selftok_add_rows_f32(_p(x), _p(table), _p(x), x.shape[0], table.numel(), _stream()), "selftok_add_rows_f32")
    return x


def timestep_embed(t, freqs, t_scale=1.0):
    _need_cuda(t, freqs)
    t = t.contiguous().float()
    n, half = t.numel(), freqs.numel()
    out = torch.empty(n, 2 * half, dtype=torch.float32, device=t.device)
    _lib.check(_lib.load().selftok_timestep_embed_f32(_p(t), _p(freqs), _p(out), n, 2 * half, float(t_scale), _stream()), "selftok_timestep_embed_f32")
    return out


def patchify(x):
    _need_cuda(x)
    x = x.contiguous().float()
    B, C, H, W = x.shape
    out = torch.empty(B, (H // 2) * (W // 2), 4 * C, dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().selftok_patchify_f32(_p(x), _p(out), B, C, H, W, _stream()), "selftok_patchify_f32")
    return out


def unpatchify_cfg_euler(y_cond, x=None, dt=0.0, y_uncond=None, cfg_scale=1.0, C=16, hp=16, wp=16, want_v=False):
    """returns (x_new or None, v or None)"""
    _need_cuda(y_cond)
    B = y_cond.shape[0]
    assert y_cond.is_contiguous() and y_cond.shape[1] == hp * wp and y_cond.shape[2] == 4 * C
    x_out = torch.empty(B, C, 2 * hp, 2 * wp, dtype=torch.float32, device=y_cond.device) if x is not None else None
    v_out = torch.empty(B, C, 2 * hp, 2 * wp, dtype=torch.float32, device=y_cond.device) if (want_v or x is None) else None
    if x is not None:
        assert x.is_contiguous()
    _lib.check(_lib.load().selftok_unpatchify_cfg_euler_f32(_p(y_cond), _p(y_uncond), _p(x), _p(x_out), _p(v_out), B, C, hp, wp,
                                                            float(dt), float(cfg_scale), _stream()), "selftok_unpatchify_cfg_euler_f32")
    return x_out, v_out


def rmsnorm(x, w=None, eps=1e-6):
    _need_cuda(x)
    x = x.contiguous().float()
    out = torch.empty_like(x)
    dim = x.shape[-1]
    _lib.check(_lib.load().selftok_rmsnorm_f32(_p(x), _p(w), _p(out), x.numel() // dim, dim, eps, _stream()), "selftok_rmsnorm_f32")
    return out


def rotary(t, freqs, start_index: int = 0, scale: float = 1.0):
    """apply_rotary_emb(freqs, t, start_index, scale) (utils/rotary_embedding_torch.py:37-53): t [..., seq, dim], freqs [seq, rot_dim];
    features start_index .. start_index + rot_dim are rotated, the rest passes through."""
    _need_cuda(t, freqs)
    t = t.contiguous().float()
    freqs = freqs.contiguous().float()
    seq, rot = freqs.shape
    dim = t.shape[-1]
    if rot > dim - start_index:
        raise ValueError(f"feature dimension {dim} is not of sufficient size to rotate in all the positions {rot}")
    mid = t if (start_index == 0 and rot == dim) else t[..., start_index:start_index + rot].contiguous()
    out = torch.empty_like(mid)
    _lib.check(_lib.load().selftok_rotary_f32(_p(mid), _p(freqs), _p(out), mid.numel() // rot, seq, rot, float(scale), _stream()), "selftok_rotary_f32")
    if mid is t:
        return out
    return torch.cat((t[..., :start_index], out, t[..., start_index + rot:]), dim=-1)


# ----------------------------------------------------------------------------------------------
# attention (csrc/attention.hip)
# ----------------------------------------------------------------------------------------------

def _seg(q, k, v, o):
    """q/k/v/o: 3-D views [B, L, H*Dh] with unit inner stride (slices of a fused qkv buffer are fine)."""
    s = _lib.AttnSeg()
    if k is None:
        return s
    if isinstance(o, SplitAct):      # split-activation output [B,L,H*Dh]: its pointer goes into the descriptor (attention())
        assert o.shape == (k.shape[0], q.shape[1], q.shape[2])
        o = None
    for name, t in (("q", q), ("k", k), ("v", v), ("o", o)):
        if t is None:
            continue
        assert t.dim() == 3 and t.stride(2) == 1 and t.dtype == torch.float32
        setattr(s, name, t.data_ptr())
        setattr(s, name + "_rs", t.stride(1))
        setattr(s, name + "_bs", t.stride(0))
    s.len = k.shape[1]
    return s


ATTN_F16X2 = 1
ATTN_F16 = 2        # LOSSY single-pass fp16 products (selftok_attn_f16, csrc/attention_f16.hip): the attention of the 'f16' GEMM mode


def pack_key_mask(mask: torch.Tensor) -> torch.Tensor:
    """bool / 0-1 [B, K] -> int32 [B, ceil(K / 32)], the `kmask` words of `attention`: bit j & 31 of word j >> 5 is key j.
    Device ops only (no host synchronisation: legal before and inside a graph capture)."""
    B, K = mask.shape
    W = (K + 31) // 32
    m = torch.zeros(B, W * 32, dtype=torch.int64, device=mask.device)
    m[:, :K] = mask != 0
    words = (m.view(B, W, 32) << torch.arange(32, device=mask.device, dtype=torch.int64)).sum(dim=2)     # 0 .. 2^32 - 1
    return torch.where(words >= (1 << 31), words - (1 << 32), words).to(torch.int32).contiguous()       # the same 32 bits, as int32


def attention(seg0, seg1, heads, head_dim, kvis=None, seg0_sees_seg1=True, scale=None, mode: int = 0, overflow=None,
              kmask=None, kmask_bs=None):
    """seg = (q, k, v, o) tuples of [B,L,heads*head_dim] views (q and o None: keys/values only; seg None: empty).
    Writes into the `o` views.  kvis: int32 [B] or None.  mode = ATTN_F16X2: f16x2-split matrix products (head_dim 64),
    `overflow` (int32 [1] device tensor) gets bit 2 if an operand is outside the fp16 range.  mode = ATTN_F16 (head_dim 64 only, LOSSY):
    one fp16 matrix instruction per product on fp16-rounded q * c, k, v and probabilities (include/selftok_hip_ext.h: selftok_attn_f16); the same flag,
    the same outputs (fp32 views or SplitActs), with or without kmask.
    kmask: int32 / uint32 [B, W] words of a per-sample visibility pattern over the segment-0 keys (`pack_key_mask`; exclusive with
    kvis; bits past the segment's length are ignored), kmask_bs: words per sample (default: kmask's row stride)."""
    lib = _lib.load()
    d = _lib.AttnDesc()
    ref = seg1 if seg1 is not None else seg0
    _need_cuda(ref[1])
    d.seg[0] = _seg(*seg0) if seg0 is not None else _lib.AttnSeg()
    d.seg[1] = _seg(*seg1) if seg1 is not None else _lib.AttnSeg()
    for i, sg in enumerate((seg0, seg1)):               # `o` given as a SplitAct [B,L,H*Dh]; f16x2 and f16 modes only
        if sg is not None and isinstance(sg[3], SplitAct):
            d.o_blk[i] = sg[3].data.data_ptr()
    d.B, d.H, d.head_dim = ref[1].shape[0], heads, head_dim
    if kvis is not None:
        assert kvis.dtype == torch.int32 and kvis.is_cuda and kvis.numel() == d.B
        d.kvis = kvis.data_ptr()
    d.seg0_sees_seg1 = 1 if seg0_sees_seg1 else 0
    d.scale = float(scale if scale is not None else head_dim ** -0.5)
    f16 = int(mode) == ATTN_F16
    d.mode = int(mode) if (head_dim == 64 and not f16) else 0
    d.overflow = _p(overflow)
    import ctypes
    bs = 0
    if kmask is not None:
        assert kmask.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and kmask.is_cuda and kmask.dim() == 2
        assert kmask.shape[0] == d.B and kmask.stride(1) == 1
        bs = int(kmask.stride(0) if kmask_bs is None else kmask_bs)
    if f16:                     # one entry with and without a mask; it refuses head_dim != 64 itself
        _lib.check(lib.selftok_attn_f16(ctypes.byref(d), _p(kmask), bs, _stream()), "selftok_attn_f16")
        return
    if kmask is not None:
        _lib.check(lib.selftok_attn_kmask_f32(ctypes.byref(d), kmask.data_ptr(), bs, _stream()), "selftok_attn_kmask_f32")
        return
    _lib.check(lib.selftok_attn_f32(ctypes.byref(d), _stream()), "selftok_attn_f32")


# ----------------------------------------------------------------------------------------------
# VAE epilogues (csrc/vae.hip)
# ----------------------------------------------------------------------------------------------

def groupnorm_silu(x, weight, bias, groups=32, eps=1e-6, silu_act=True):
    _need_cuda(x)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    _lib.check(_lib.load().selftok_groupnorm_silu_bf16(_p(x), _p(weight), _p(bias), _p(out), B, C, H * W, groups, eps,
                                                       1 if silu_act else 0, _stream()), "selftok_groupnorm_silu_bf16")
    return out


class PackedConv:
    """one convolution's weights in the opaque image selftok_conv2d_nhwc_bf16 reads (csrc/conv.hip) + its bias and geometry"""
    __slots__ = ("packed", "bias", "cout", "cin", "ksize", "bn")

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor]):
        _need_cuda(weight, bias)
        assert weight.dtype == torch.bfloat16 and weight.dim() == 4 and weight.shape[2] == weight.shape[3] and weight.shape[2] in (1, 3)
        w = weight.contiguous()
        self.cout, self.cin, self.ksize = int(w.shape[0]), int(w.shape[1]), int(w.shape[2])
        self.bn = 128 if self.cout >= 64 else 32
        lib = _lib.load()
        self.packed = torch.empty(lib.selftok_conv2d_packed_bytes(self.cout, self.cin, self.ksize, self.bn), dtype=torch.uint8, device=w.device)
        _lib.check(lib.selftok_conv2d_pack_weight_bf16(_p(w), _p(self.packed), self.cout, self.cin, self.ksize, self.bn, _stream()), "selftok_conv2d_pack_weight_bf16")
        self.bias = None if bias is None else bias.to(torch.bfloat16).contiguous()


def conv2d_nhwc(x: torch.Tensor, pc: PackedConv, stride: int = 1, upsample: bool = False, residual: Optional[torch.Tensor] = None,
                cstore: Optional[int] = None) -> torch.Tensor:
    """x [B,H,W,Cin'] bf16 channels-last (Cin' = the layer's Cin rounded up to a multiple of 8, extra channels ignored) ->
    [B,Ho,Wo,cstore] bf16: the convolution with the reference's CPU arithmetic (fp32 accumulate incl. the bias, one rounding).
    stride 2 = Downsample (pad right/bottom + stride-2), upsample = nearest 2x applied to the input on the fly, residual [B,Ho,Wo,cstore]
    is added with its own bf16 rounding (ResnetBlock's `x + h`)."""
    _need_cuda(x, residual)
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and x.dim() == 4
    B, H, W, Cin = x.shape
    assert Cin % 8 == 0 and (Cin + 31) // 32 == (pc.cin + 31) // 32 and Cin >= pc.cin, (Cin, pc.cin)
    cs = (pc.cout + 3) // 4 * 4 if cstore is None else cstore
    # stored zero channels may pad the last channel block of the packed image, never open a block it does not hold (include/selftok_hip.h)
    assert cs % 4 == 0 and cs >= pc.cout and (cs + pc.bn - 1) // pc.bn == (pc.cout + pc.bn - 1) // pc.bn, (cs, pc.cout, pc.bn)
    Hi, Wi = (H * 2, W * 2) if upsample else (H, W)
    Ho, Wo = (Hi // 2, Wi // 2) if stride == 2 else (Hi, Wi)
    out = torch.empty(B, Ho, Wo, cs, dtype=torch.bfloat16, device=x.device)
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == torch.bfloat16
    _lib.check(_lib.load().selftok_conv2d_nhwc_bf16(_p(x), _p(pc.packed), _p(pc.bias), _p(residual), _p(out), B, H, W, Cin, pc.cout, cs, cs, pc.ksize, stride,
                                                    1 if upsample else 0, pc.bn, _stream()), "selftok_conv2d_nhwc_bf16")
    return out


def groupnorm_silu_nhwc(x, weight, bias, groups=32, eps=1e-6, silu_act=True):
    """GroupNorm [+ SiLU] on a channels-last bf16 tensor [B, ..., C]"""
    _need_cuda(x, weight, bias)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    B, C = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C)
    lib = _lib.load()
    out = torch.empty_like(x)
    ws = torch.empty(lib.selftok_groupnorm_nhwc_workspace_bytes(B, HW, C), dtype=torch.uint8, device=x.device)
    _lib.check(lib.selftok_groupnorm_silu_nhwc_bf16(_p(x), _p(weight), _p(bias), _p(out), _p(ws), B, HW, C, groups, eps, 1 if silu_act else 0, _stream()),
               "selftok_groupnorm_silu_nhwc_bf16")
    return out


def latent_process_in(moments, c_keep=16, shift=0.0609, scale=1.5305):
    _need_cuda(moments)
    assert moments.dtype == torch.bfloat16 and moments.is_contiguous()
    B, Cin, H, W = moments.shape
    out = torch.empty(B, c_keep, H, W, dtype=torch.float32, device=moments.device)
    _lib.check(_lib.load().selftok_latent_process_in(_p(moments), _p(out), B, Cin, c_keep, H * W, shift, scale, _stream()), "selftok_latent_process_in")
    return out


def latent_process_out(z, shift=0.0609, scale=1.5305):
    _need_cuda(z)
    z = z.contiguous().float()
    out = torch.empty(z.shape, dtype=torch.bfloat16, device=z.device)
    _lib.check(_lib.load().selftok_latent_process_out(_p(z), _p(out), z.numel(), shift, scale, _stream()), "selftok_latent_process_out")
    return out


def clamp01_(img):
    _need_cuda(img)
    assert img.dtype == torch.bfloat16 and img.is_contiguous()
    _lib.check(_lib.load().selftok_clamp01_bf16(_p(img), img.numel(), _stream()), "selftok_clamp01_bf16")
    return img


def vq_encode_split_launch(z, packed_codebook, ids_dtype=torch.int64, coarse=None, _flags: Optional[int] = None):
    """Same result as vq_encode(packed=True) but returns (ids, launch_main, launch_finalize) closures so a
    benchmark can time the main argmax kernel alone (HIP events around launch_main on the current stream).
    `coarse`: None / False / True / 1 / 3 as in vq_encode; `_flags`: the raw SELFTOK_VQ_* flag word instead (sweeps)."""
    import ctypes
    lib = _lib.load()
    zz = z.contiguous().float().reshape(-1, z.shape[-1])
    N, D = zz.shape
    C = packed_codes(packed_codebook, D)
    ids = torch.empty(N, dtype=ids_dtype, device=z.device)
    ws = torch.empty(lib.selftok_vq_workspace_bytes(N, C), dtype=torch.uint8, device=z.device)
    flags = (IDS_I32 if ids_dtype == torch.int32 else 0) | (int(_flags) if _flags is not None else _coarse_flags(coarse))
    nsplit = ctypes.c_int(0)

    def launch_main():
        _lib.check(lib.selftok_vq_argmax_partial_packed_f32(_p(zz), _p(packed_codebook), _p(ws), ctypes.addressof(nsplit), N, C, D,
                                                            flags, _stream()), "selftok_vq_argmax_partial_packed_f32")

    def launch_finalize():
        _lib.check(lib.selftok_vq_finalize_packed(_p(ws), _p(zz), _p(packed_codebook), _p(ids), None, N, C, D, nsplit.value, flags,
                                                  _stream()), "selftok_vq_finalize_packed")

    return ids.reshape(z.shape[:-1]), launch_main, launch_finalize


# ---- the exact-order SD3-VAE encoder kernels (csrc/vae_exact.hip) -------------------------------------------------------------------
VX_UPSAMPLE2X = 8


def vx_conv2d(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, stride: int = 1, residual: Optional[torch.Tensor] = None, order: int = 0,
              cin: Optional[int] = None, upsample: bool = False) -> torch.Tensor:
    """x [B,H,W,ldx] bf16 channels-last, w [Cout,k,k,Cin] bf16 (the checkpoint's tensor permuted), bias [Cout] bf16 -> [B,Ho,Wo,Cout] bf16 with the
    summation order of the reference's CPU convolution (oneDNN AMX chunks; include/selftok_hip.h).  `order`: 0 / 3 / 1 / 2 (conv_in, cin = 3).
    `upsample`: the convolution reads the nearest-2x upsampled view of x (the decoder's Upsample layer; output [B,2H,2W,Cout])."""
    _need_cuda(x, w, bias, residual)
    assert x.dtype == w.dtype == bias.dtype == torch.bfloat16 and x.is_contiguous() and w.is_contiguous() and x.dim() == 4 and w.dim() == 4
    B, H, W, ldx = x.shape
    Cout, k, k2, Cin = w.shape
    assert k == k2 and (cin is None or cin == Cin)
    if upsample:
        assert stride == 1
        H, W, order = 2 * H, 2 * W, order | VX_UPSAMPLE2X
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    out = torch.empty(B, Ho, Wo, Cout, dtype=torch.bfloat16, device=x.device)
    if residual is not None:
        assert residual.shape == out.shape and residual.is_contiguous() and residual.dtype == torch.bfloat16
    _lib.check(_lib.load().selftok_vx_conv2d_bf16(_p(x), _p(w), _p(bias), _p(residual), _p(out), B, H, W, ldx, Cin, Cout, k, stride, order, _stream()),
               "selftok_vx_conv2d_bf16")
    return out


def vx_silu_table(device) -> torch.Tensor:
    """torch-CPU's bf16 SiLU as a 65536-entry table (int16 view of bf16 bits), built on the device"""
    t = torch.empty(65536, dtype=torch.int16, device=device)
    with torch.cuda.device(t.device):
        _lib.check(_lib.load().selftok_vx_silu_table_bf16(_p(t), _stream()), "selftok_vx_silu_table_bf16")
    return t


def vx_groupnorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, silu_table: Optional[torch.Tensor] = None, groups: int = 32, eps: float = 1e-6,
                 want_stats: bool = False):
    """GroupNorm [+ SiLU via `silu_table`] on [B, ..., C] bf16 channels-last with ATen's CPU statistics order (include/selftok_hip.h)"""
    _need_cuda(x, gamma, beta, silu_table)
    assert x.dtype == torch.bfloat16 and x.is_contiguous()
    B, C = x.shape[0], x.shape[-1]
    if B == 0:
        return (torch.empty_like(x), torch.empty(0, groups, 2, dtype=torch.float32, device=x.device)) if want_stats else torch.empty_like(x)
    HW = x.numel() // (B * C)
    lib = _lib.load()
    nbytes = lib.selftok_vx_groupnorm_workspace_bytes(B, HW, C)
    if nbytes == 0:
        raise _lib.SelftokHipError(f"vx_groupnorm: unsupported shape B={B} HW={HW} C={C}")
    out = torch.empty_like(x)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    stats = torch.empty(B, groups, 2, dtype=torch.float32, device=x.device) if want_stats else None
    _lib.check(lib.selftok_vx_groupnorm_bf16(_p(x), _p(gamma), _p(beta), _p(out), _p(ws), _p(silu_table), _p(stats), B, HW, C, groups, float(eps), _stream()),
               "selftok_vx_groupnorm_bf16")
    return (out, stats) if want_stats else out


def vx_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
    """q, k, v [B,T,C] bf16 -> [B,T,C] bf16: one-head attention as ATen's CPU flash kernel evaluates it (T = 1024)"""
    _need_cuda(q, k, v)
    assert q.dtype == k.dtype == v.dtype == torch.bfloat16 and q.is_contiguous() and k.is_contiguous() and v.is_contiguous() and q.shape == k.shape == v.shape
    B, T, C = q.shape
    lib = _lib.load()
    out = torch.empty_like(q)
    if B == 0:
        return out
    ws = torch.empty(lib.selftok_vx_attention_workspace_bytes(B, T, C), dtype=torch.uint8, device=q.device)
    _lib.check(lib.selftok_vx_attention_bf16(_p(q), _p(k), _p(v), _p(out), _p(ws), B, T, C, _stream()), "selftok_vx_attention_bf16")
    return out


def vx_expf(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty_like(x)
    _lib.check(_lib.load().selftok_vx_expf_f32(_p(x), _p(y), x.numel(), _stream()), "selftok_vx_expf_f32")
    return y


# ----------------------------------------------------------------------------------------------
# the fp32 Q-Former encoder in the reference's exact summation orders (csrc/encoder_exact.hip)
# ----------------------------------------------------------------------------------------------

def _rows2d(t: torch.Tensor):
    """a [..., C] fp32 tensor whose rows are equally strided (contiguous, or a column slice of a contiguous fused projection) -> (rows, row stride)"""
    assert t.dtype == torch.float32 and t.stride(-1) == 1
    ld = t.stride(-2) if t.dim() > 1 else t.shape[-1]
    rows = t.numel() // t.shape[-1]
    for d in range(t.dim() - 2, 0, -1):                              # leading dims must step by whole row blocks
        assert t.shape[d - 1] == 1 or t.stride(d - 1) == t.stride(d) * t.shape[d], "rows are not equally strided"   # (the stride of a size-1 dim is never used)
    return rows, ld


EX_LINEAR_GELU_ON_XE = True     # fc1 + GELU stays on xe_gemm128 with the GELU in its epilogue: in the model 620 / 252 ms per sampler step against 625 - 641 / 255 with
                                # csrc/gemm_fp32.hip + a GELU pass (profiles/r6_exact_mode_ab_v11_fused_ln.txt; the difference is inside the run-to-run noise, the pass is not)
EX_LINEAR_SG_MIN_ROWS = 256     # from this many rows on `ex_linear` runs on the LDS-DMA staged kernel (csrc/gemm_fp32.hip, bit-identical results) where the shape allows


def ex_linear(x: torch.Tensor, weight: torch.Tensor, bias=None, *, gelu: bool = False, res=None, res_mod: int = 0, gate=None, gate_mod: int = 0,
              out: Optional[torch.Tensor] = None, bias_last: bool = False, kernel: str = "auto") -> torch.Tensor:
    """F.linear in MKL sgemm's BLOCKED summation order -- bit-equal to torch-CPU's nn.Linear where MKL takes that path (probed: M >= 512 token rows, >= 16
    conditioning rows; below that MKL switches strategy and this kernel still computes the blocked order: the result for a row is the one it has inside a large
    batch, whatever M is here), optional exact GELU(tanh),
    optional `res + gate * y` epilogue (res / gate rows taken modulo res_mod / gate_mod when positive: per-token tables; divided by
    -mod when negative: per-sample tables).  bias_last: (sum of the K-blocks) + bias, what at::linear computes for a non-contiguous input.
    `kernel`: 'xe' = xe_gemm / xe_gemm128 (csrc/encoder_exact.hip, any shape), 'sg' = the LDS-DMA staged kernel of round 6 (csrc/gemm_fp32.hip: N % 128 == 0,
    K % 32 == 0, K outside (384, 768)), 'auto' = 'sg' from EX_LINEAR_SG_MIN_ROWS rows on where the shape allows.  Same bits either way (tests/test_gemm_fp32_gpu.py)."""
    N, K = weight.shape
    if kernel not in ("auto", "xe", "sg"):
        raise ValueError(f"ex_linear kernel {kernel!r}: expected 'auto', 'xe' or 'sg'")
    sg_ok = not (gelu and (res is not None or gate is not None or (out is not None and not out.is_contiguous())))      # the LDS-DMA kernel's GELU: contiguous out, no res / gate
    if kernel == "sg" or (kernel == "auto" and sg_ok and linear_f32_supported(N, K, mkl_order=True) and x.numel() // max(K, 1) >= EX_LINEAR_SG_MIN_ROWS
                          and not (gelu and EX_LINEAR_GELU_ON_XE)):
        # fc1 + GELU: selftok_linear_f32 runs the GELU as a second launch over `out` (in the GEMM's epilogue four waves per CU worked through ~80 VALU instructions
        # per output while the matrix pipe idled: +0.40 ms on a 2.28 ms Linear; as an element-wise pass +0.2 ms).  Same bits: GELU of the same fp32 value.
        return linear_f32(x, weight, bias, mkl_order=True, gelu=gelu, res=res, res_mod=res_mod, gate=gate, gate_mod=gate_mod, out=out, bias_last=bias_last)
    _need_cuda(x, weight, bias, res, gate)
    assert weight.dtype == torch.float32 and weight.is_contiguous() and x.shape[-1] == K
    M, ldx = _rows2d(x)
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() or out.stride(-1) == 1
    _, ldo = _rows2d(out)
    ldr = _rows2d(res)[1] if res is not None else 0
    ldg = _rows2d(gate)[1] if gate is not None else 0
    _lib.check(_lib.load().selftok_ex_linear_f32(_p(x), ldx, _p(weight), _p(bias), _p(res), ldr, int(res_mod), _p(gate), ldg, int(gate_mod), _p(out), ldo,
                                                 M, N, K, int(bool(gelu)) | (2 if bias_last else 0), _stream()), "selftok_ex_linear_f32")
    return out


LINEAR_BIAS_LAST, LINEAR_MKL_ORDER = 2, 4
_linear_ws = _StreamWorkspace(64 << 20)      # the tail split's workspace


def linear_f32(x: torch.Tensor, weight: torch.Tensor, bias=None, *, mkl_order: bool = False, gelu: bool = False, res=None, res_mod: int = 0, gate=None,
               gate_mod: int = 0, out: Optional[torch.Tensor] = None, bias_last: bool = False, split: int = 0, use_workspace: bool = True, _flags: int = 0) -> torch.Tensor:
    """F.linear on the LDS-DMA staged fp32-MFMA kernel (csrc/gemm_fp32.hip): N % 128 == 0, K % 32 == 0.  mkl_order: MKL sgemm's K-blocking, bit-identical to
    `ex_linear` (gemm='exact'); otherwise one k-ascending chain per output (gemm='fp32').  Epilogue arguments as `ex_linear`.  `split` (tests / tools) forces the
    tail split; `use_workspace=False` runs the tail round unsplit."""
    _need_cuda(x, weight, bias, res, gate)
    N, K = weight.shape
    assert weight.dtype == torch.float32 and weight.is_contiguous() and x.shape[-1] == K
    M, ldx = _rows2d(x)
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), dtype=torch.float32, device=x.device)
    assert out.is_contiguous() or out.stride(-1) == 1
    _, ldo = _rows2d(out)
    ldr = _rows2d(res)[1] if res is not None else 0
    ldg = _rows2d(gate)[1] if gate is not None else 0
    flags = (1 if gelu else 0) | (LINEAR_BIAS_LAST if bias_last else 0) | (LINEAR_MKL_ORDER if mkl_order else 0) | ((int(split) & 0xFF) << 8) | int(_flags)
    lib = _lib.load()
    ws, nws = None, 0
    if use_workspace:
        nws = int(lib.selftok_linear_f32_workspace_bytes(M, N, K, flags))
        ws = _linear_ws(x.device, nws) if nws else None
    _lib.check(lib.selftok_linear_f32(_p(x), ldx, _p(weight), _p(bias), _p(res), ldr, int(res_mod), _p(gate), ldg, int(gate_mod), _p(out), ldo, M, N, K, flags,
                                      _p(ws), (ws.numel() if ws is not None else 0), _stream()), "selftok_linear_f32")
    return out


def linear_f32_supported(N: int, K: int, mkl_order: bool = False) -> bool:
    return N % 128 == 0 and K % 32 == 0 and not (mkl_order and 384 < K < 768)


def ex_layernorm_mod(x: torch.Tensor, shift=None, scale=None, gamma=None, beta=None, eps: float = 1e-6, want_stats: bool = False, per_sample: bool = False):
    """nn.LayerNorm in ATen's arithmetic, then `* (1 + scale[tok]) + shift[tok]` (tok = row % T; shift / scale [T, N] views, equal row stride;
    per_sample: x [B, rows, N] with tables [B, N], tok = the sample)"""
    _need_cuda(x, shift, scale, gamma, beta)
    N = x.shape[-1]
    rows, ldx = _rows2d(x)
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    T, ldt = 0, 0
    if shift is not None:
        assert scale is not None and shift.dim() == 2 and shift.shape == scale.shape and shift.stride(0) == scale.stride(0) and shift.stride(1) == 1 == scale.stride(1)
        T, ldt = shift.shape[0], shift.stride(0)
        if per_sample:
            assert x.dim() == 3 and shift.shape[0] == x.shape[0]
            T = -x.shape[1]
    stats = torch.empty(rows, 2, dtype=torch.float32, device=x.device) if want_stats else None
    _lib.check(_lib.load().selftok_ex_layernorm_mod_f32(_p(x), ldx, _p(out), N, _p(shift), _p(scale), ldt, T, _p(gamma), _p(beta), _p(stats), rows, N, float(eps),
                                                        _stream()), "selftok_ex_layernorm_mod_f32")
    return (out, stats) if want_stats else out


def ex_res_layernorm_mod(x: torch.Tensor, lin: torch.Tensor, *, lin_bias=None, gate=None, gate_mod: int = 0, shift=None, scale=None, eps: float = 1e-6,
                         per_sample: bool = False, x_out: Optional[torch.Tensor] = None):
    """x' = x + gate[row] * (lin + lin_bias); n = LayerNorm(x') * (1 + scale[tok]) + shift[tok]  ->  (x', n).  The residual update of a DismantledBlock
    (sd3/mmdit.py:485-496) fused into the LayerNorm + modulate behind it: the same bits as `ex_linear(..., res=x, gate=gate)` + `ex_layernorm_mod`, with the
    Linear keeping its plain epilogue (round 6).  gate rows: m % gate_mod (> 0: per-token table), m / -gate_mod (< 0: per-sample), m (0).  x_out may be x."""
    _need_cuda(x, lin, lin_bias, gate, shift, scale)
    N = x.shape[-1]
    rows, ldx = _rows2d(x)
    rl, ldl = _rows2d(lin)
    assert rl == rows and lin.shape[-1] == N
    xo = torch.empty(x.shape, dtype=torch.float32, device=x.device) if x_out is None else x_out
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    ldg = _rows2d(gate)[1] if gate is not None else 0
    T, ldt = 0, 0
    if shift is not None:
        assert scale is not None and shift.dim() == 2 and shift.shape == scale.shape and shift.stride(0) == scale.stride(0) and shift.stride(1) == 1 == scale.stride(1)
        T, ldt = shift.shape[0], shift.stride(0)
        if per_sample:
            assert x.dim() == 3 and shift.shape[0] == x.shape[0]
            T = -x.shape[1]
    _lib.check(_lib.load().selftok_ex_res_layernorm_mod_f32(_p(x), ldx, _p(lin), ldl, _p(lin_bias), _p(gate), ldg, int(gate_mod), _p(xo), _rows2d(xo)[1], _p(out), N,
                                                            _p(shift), _p(scale), ldt, T, rows, N, float(eps), _stream()), "selftok_ex_res_layernorm_mod_f32")
    return xo, out


EX_UNARY = {"gelu_tanh": 0, "silu": 1, "sleef_expf": 2, "sleef_tanhf": 3, "exp_u20": 4}


def ex_unary(x: torch.Tensor, kind: str, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """element-wise: y[i] = f(x[i]); `out` may be x itself (in place)"""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    y = torch.empty_like(x) if out is None else out
    assert y.dtype == torch.float32 and y.is_contiguous() and y.numel() == x.numel()
    _lib.check(_lib.load().selftok_ex_unary_f32(_p(x), _p(y), x.numel(), EX_UNARY[kind], _stream()), "selftok_ex_unary_f32")
    return y


EX_ATTENTION_WS_LIMIT = 6 << 30          # bytes of score workspace one call of the unfused exact attention may allocate; larger batches run in slices
EX_ATTENTION_DEFAULT = "auto"     # what kernel='auto' means in ex_attention (tools set 'unfused' for A/B runs)


def ex_attention(q: torch.Tensor, k1, v1, heads: int, k2=None, v2=None, slots1: Optional[int] = None, kernel: str = "auto",
                 kmask: Optional[torch.Tensor] = None, valid1: Optional[int] = None) -> torch.Tensor:
    """F.scaled_dot_product_attention as ATen's fp32 CPU flash kernel evaluates it.  q [B,Tq,H*D], k1 / v1 [B,Tk1,H*D] and an
    optional second key / value segment that follows the first; all may be column slices of fused projections.  -> [B,Tq,H*D].
    `slots1`: the first segment occupies slots1 >= Tk1 key positions of which only the Tk1 given ones are visible (a prefix mask: the
    masked keys keep their place in the kv blocks, see include/selftok_hip.h); k1 = v1 = None with slots1: none of them is visible.
    `kernel`: 'fused' = one kernel, scores never leave the CU (round 6: head_dim 64, slot counts % 64 == 0), 'unfused' = scores GEMM -> row pass -> P V GEMM through a
    workspace (round 5, any shape), 'auto' = fused where it applies.  Same bits (tests/test_encoder_exact_gpu.py).
    `kmask`: int32 [B, W] (or [1, W]: one pattern for the batch) words of `pack_key_mask` over the first segment's slots, W >= ceil(slots / 32): of the Tk1 given
    rows (which stay at their positions 0 .. Tk1 - 1) only those whose bit is set are visible -- any pattern, the reference's `mask * super_mask`; the bits at
    and past Tk1 are ignored.  An invisible row is never read into the arithmetic.  A sample without any visible key gets zeros.
    `valid1` (with kmask): only the first valid1 <= Tk1 given rows can be visible, the bits at and past it are ignored too (the step prefix of `mask * super_mask`
    over a buffer that holds more rows)."""
    if kernel == "auto":
        kernel = EX_ATTENTION_DEFAULT
    if kernel not in ("auto", "fused", "unfused"):
        raise ValueError(f"ex_attention kernel {kernel!r}: expected 'auto', 'fused' or 'unfused'")
    _need_cuda(q, k1, v1, k2, v2)
    B, Tq, HD = q.shape
    D = HD // heads
    _, qs = _rows2d(q)
    rows1, ks1 = 0, 0
    if k1 is not None:
        _, ks1 = _rows2d(k1)
        assert _rows2d(v1)[1] == ks1 and k1.shape == v1.shape
        rows1 = k1.shape[1]
    else:
        assert slots1 is not None and k2 is not None
    Tk1 = rows1 if slots1 is None else int(slots1)
    Tk2, ks2 = 0, 0
    if k2 is not None:
        Tk2, ks2 = k2.shape[1], _rows2d(k2)[1]
        assert _rows2d(v2)[1] == ks2 and k2.shape == v2.shape
    lib = _lib.load()
    km_bs = 0
    nv1 = rows1
    if valid1 is not None:
        assert kmask is not None and 0 <= int(valid1) <= rows1
        nv1 = int(valid1)
    if kmask is not None:
        assert kmask.dtype in (torch.int32, getattr(torch, "uint32", torch.int32)) and kmask.is_cuda and kmask.dim() == 2 and kmask.stride(1) == 1
        assert kmask.shape[0] in (1, B) and kmask.shape[1] * 32 >= Tk1 and Tk1 <= 2048, (tuple(kmask.shape), B, Tk1)
        km_bs = int(kmask.stride(0)) if kmask.shape[0] == B and B > 1 else 0
    # with words a sample may have no visible key at all (no image keys, every context bit clear): its rows stay zero
    out = (torch.zeros if (kmask is not None and Tk2 == 0) else torch.empty)(B, Tq, HD, dtype=torch.float32, device=q.device)
    if B == 0:
        return out
    fused = kernel == "fused" or (kernel == "auto" and lib.selftok_ex_attention_fused_supported(Tk1, Tk2, D))
    if fused and kmask is not None:
        _lib.check(lib.selftok_ex_attention_kmask_fused_f32(_p(q), qs, _p(k1), _p(v1), ks1, Tk1, nv1, rows1, _p(k2), _p(v2), ks2, Tk2, _p(out), B, heads, Tq, D,
                                                            _p(kmask), km_bs, _stream()), "selftok_ex_attention_kmask_fused_f32")
        return out
    if fused:
        _lib.check(lib.selftok_ex_attention_fused_f32(_p(q), qs, _p(k1), _p(v1), ks1, Tk1, rows1, rows1, _p(k2), _p(v2), ks2, Tk2, _p(out), B, heads, Tq, D, _stream()),
                   "selftok_ex_attention_fused_f32")
        return out
    # the unfused route materialises the scores (B * heads * Tq * Tk * 4 bytes + V^T): bounded by running the batch in slices (rows are independent: same bits),
    # which also keeps B * heads inside gridDim.z
    per = int(lib.selftok_ex_attention_workspace_bytes(1, heads, Tq, Tk1 + Tk2, D))
    nb = max(1, min(B, EX_ATTENTION_WS_LIMIT // max(per, 1), 65535 // max(heads, 1)))
    ws = torch.empty(int(lib.selftok_ex_attention_workspace_bytes(nb, heads, Tq, Tk1 + Tk2, D)), dtype=torch.uint8, device=q.device)
    for b0 in range(0, B, nb):
        n = min(nb, B - b0)
        sl = lambda t: None if t is None else t[b0:b0 + n]
        if kmask is not None:
            _lib.check(lib.selftok_ex_attention_kmask_f32(_p(sl(q)), qs, _p(sl(k1)), _p(sl(v1)), ks1, Tk1, nv1, rows1, _p(sl(k2)), _p(sl(v2)), ks2, Tk2, _p(out[b0:b0 + n]), _p(ws),
                                                          n, heads, Tq, D, _p(kmask[b0:b0 + n] if km_bs else kmask), km_bs, _stream()), "selftok_ex_attention_kmask_f32")
            continue
        _lib.check(lib.selftok_ex_attention_f32(_p(sl(q)), qs, _p(sl(k1)), _p(sl(v1)), ks1, Tk1, rows1, rows1, _p(sl(k2)), _p(sl(v2)), ks2, Tk2, _p(out[b0:b0 + n]), _p(ws),
                                                n, heads, Tq, D, _stream()), "selftok_ex_attention_f32")
    return out


# ---- device image I/O (csrc/image_io.hip, csrc/image_views.hip, include/selftok_hip_ext.h) ----
_IMG_LUT = {}


def image_norm_lut(device, dtype=torch.bfloat16) -> torch.Tensor:
    """[256] of `dtype` on `device`: pipeline.NormalizeToTensor evaluated on every uint8 value (its own expression, so the two cannot drift)"""
    import numpy as np
    device = torch.device(device)
    key = (device, dtype)
    if key not in _IMG_LUT:
        from .pipeline import NormalizeToTensor
        lut = NormalizeToTensor()(np.arange(256, dtype=np.uint8).reshape(1, 256, 1)).reshape(256)
        _IMG_LUT[key] = lut.to(dtype).to(device)
    return _IMG_LUT[key]


def _img_table(table):
    import numpy as np
    t = np.ascontiguousarray(np.asarray(table), dtype=np.int64)
    if t.ndim != 2 or t.shape[1] != 3:
        raise _lib.SelftokHipError(f"image table: expected [B, 3] (byte offset, width, height), got {t.shape}")
    return t


IMAGE_FILTERS = {"bilinear": 2, "bicubic": 3, "box": 4}                      # Pillow's own codes (PIL.Image.Resampling)
_UNSERVED_FILTERS = {0: "NEAREST", 1: "LANCZOS", 5: "HAMMING", "nearest": "NEAREST", "lanczos": "LANCZOS", "hamming": "HAMMING"}


def image_filter_code(filter, fn="image filter") -> int:
    """a filter named as Pillow names it ('bilinear' / 'bicubic' / 'box', Image.BILINEAR / BICUBIC / BOX, 2 / 3 / 4) -> its code; LANCZOS,
    HAMMING and NEAREST are refused by name, before the library is asked"""
    key = filter.lower() if isinstance(filter, str) else int(filter)
    if key in _UNSERVED_FILTERS:
        name = _UNSERVED_FILTERS[key]
        why = "Pillow does not resample it through coefficient tables" if name == "NEAREST" else "its weights are libm's sin / cos, whose bits the device does not promise"
        raise _lib.SelftokHipError(f"{fn}: Pillow's {name} filter is not served on the device ({why}); BILINEAR, BICUBIC and BOX are")
    if key in IMAGE_FILTERS:
        return IMAGE_FILTERS[key]
    if key in IMAGE_FILTERS.values():
        return key
    raise _lib.SelftokHipError(f"{fn}: unknown filter {filter!r}: expected one of {sorted(IMAGE_FILTERS)} or Pillow's codes 2, 3, 4")


def _image_resample(fn, entry, layout, dev_name, packed, t, size, dtype, out, t_dev, return_tables, empty_ok=False, filter=None):
    """the body image_resize_crop_norm and image_views share: `t` the host table [N, cols] of the C entry `entry`, `layout` its tap-row query,
    `fn` / `dev_name` the public function and its device-table argument for the messages; `empty_ok`: N = 0 gives an empty tensor; `filter`: the
    code the entry, its query and its layout call take after S (the entries with a filter argument), None for the bilinear entries"""
    import numpy as np
    _need_cuda(packed, out, t_dev)
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise _lib.SelftokHipError(f"{fn}: `packed` must be a contiguous 1-D uint8 tensor, got {packed.dtype} {tuple(packed.shape)}")
    if dtype not in (torch.bfloat16, torch.float32):
        raise _lib.SelftokHipError(f"{fn}: output dtype {dtype}: expected bfloat16 or float32")
    (N, cols), S = t.shape, int(size)
    if out is None:
        out = torch.empty(N, 3, max(S, 0), max(S, 0), dtype=dtype, device=packed.device)
    elif out.dtype != dtype or tuple(out.shape) != (N, 3, S, S) or not out.is_contiguous():
        raise _lib.SelftokHipError(f"{fn}: `out` must be a contiguous {dtype} [{N}, 3, {S}, {S}] tensor")
    if N == 0 and empty_ok:
        return (out, {}) if return_tables else out
    lib = _lib.load()
    fa = () if filter is None else (int(filter),)
    nbytes = _ws_bytes(entry + "_workspace_bytes", t.ctypes.data, N, S, *fa)
    if t_dev is None:
        t_dev = torch.from_numpy(t).to(packed.device)
    elif t_dev.dtype != torch.int64 or t_dev.numel() != cols * N or not t_dev.is_contiguous():
        raise _lib.SelftokHipError(f"{fn}: `{dev_name}` must be the contiguous int64 [{'B' if cols == 3 else 'V'}, {cols}] table")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
    lut = image_norm_lut(packed.device, dtype)
    _lib.check(getattr(lib, entry)(_p(packed), packed.numel(), t.ctypes.data, _p(t_dev), N, S, *fa, _p(out), int(dtype == torch.bfloat16), _p(lut), _p(ws), nbytes, _stream()), entry)
    if not return_tables:
        return out
    lay = np.zeros(4, dtype=np.int64)
    _lib.check(getattr(lib, layout)(t.ctypes.data, N, S, *fa, lay.ctypes.data), layout)
    wi = ws[:(nbytes // 4) * 4].view(torch.int32).cpu().numpy()
    tabs = {}
    for name, base, ks in (("h", int(lay[0]), int(lay[1])), ("v", int(lay[2]), int(lay[3]))):
        rows = wi[base:base + N * S * ks].reshape(N, S, ks)
        tabs[name] = (rows[:, :, 0].copy(), rows[:, :, 1].copy(), rows[:, :, 2:].copy())
    return out, tabs


def image_resize_crop_norm(packed: torch.Tensor, table, size: int, dtype=torch.bfloat16, out: Optional[torch.Tensor] = None,
                           table_dev: Optional[torch.Tensor] = None, return_tables: bool = False):
    """B RGB uint8 HWC images of any sizes, packed in the 1-D uint8 device tensor `packed`; `table` [B, 3] on the host: byte offset, width,
    height of each.  -> [B, 3, size, size] in [-1, 1], bf16 or fp32: NormalizeToTensor(CenterCrop(size)(Resize(size)(PIL image))) bit for bit.
    `table_dev`: the same table already on the device (int64), else it is copied here.  `out`: write into this contiguous tensor.
    return_tables: also the integer tap rows the kernels used, {'h' | 'v': (first [B, size], n [B, size], k [B, size, kmax])} (tests)."""
    return _image_resample("image_resize_crop_norm", "selftok_img_resize_crop_norm_u8", "selftok_img_resize_tables_layout", "table_dev",
                           packed, _img_table(table), size, dtype, out, table_dev, return_tables)


def image_view_rows(sources_table, views):
    """`sources_table` [N, 3] (byte offset, width, height) and `views` [V, 10] (source index, x0, y0, bw, bh, rw, rh, left, top, flip) -> the
    int64 [V, 12] descriptor table of selftok_img_views_u8, one row per output"""
    import numpy as np
    src = _img_table(sources_table)
    v = np.ascontiguousarray(np.asarray(views), dtype=np.int64)
    if v.ndim != 2 or v.shape[1] != 10:
        raise _lib.SelftokHipError(f"image views: expected [V, 10] (source index, x0, y0, bw, bh, rw, rh, left, top, flip), got {v.shape}")
    if v.shape[0] and (v[:, 0].min() < 0 or v[:, 0].max() >= src.shape[0]):
        raise _lib.SelftokHipError(f"image views: a source index outside 0 .. {src.shape[0] - 1}")
    return np.ascontiguousarray(np.concatenate([src[v[:, 0]], v[:, 1:]], axis=1))


def image_views(packed: torch.Tensor, sources_table, views, size: int, dtype=torch.bfloat16, out: Optional[torch.Tensor] = None,
                rows_dev: Optional[torch.Tensor] = None, return_tables: bool = False, rows=None, filter="bilinear"):
    """V views of RGB uint8 HWC sources packed in the 1-D uint8 device tensor `packed` -> [V, 3, size, size] in [-1, 1], bf16 or fp32: per view
    NormalizeToTensor(hflip?(crop(window)(resize(crop(box)(PIL image))))) bit for bit (preprocess.apply_view_pil; csrc/image_views.hip).
    `sources_table` [N, 3] on the host: byte offset, width, height of each source; `views` [V, 10] on the host: source index, x0, y0, bw, bh,
    rw, rh, left, top, flip (preprocess.view_rows).  Several views may name one source.  V = 0 gives an empty tensor.
    `rows`: image_view_rows(sources_table, views) already built on the host (contiguous int64 numpy [V, 12]); it is then the table of record and
    `sources_table` / `views` are not read (pass None).  `rows_dev`: the same rows already on the device (int64 [V, 12]), else they are copied
    here.  `out`: write into this contiguous tensor.  return_tables: also the integer tap rows, {'h' | 'v': (first [V, size], n [V, size], k [V, size, kmax])} (tests).
    `filter`: 'bilinear' (the default: selftok_img_views_u8, as before), 'bicubic' or 'box', or Pillow's Image.BILINEAR / BICUBIC / BOX -- the
    resample of every view then uses that filter (selftok_img_views_filter_u8, csrc/image_filters.hip); LANCZOS / HAMMING / NEAREST are refused."""
    import numpy as np
    code = image_filter_code(filter, "image_views")
    if rows is None:
        rows = image_view_rows(sources_table, views)
    elif not isinstance(rows, np.ndarray) or rows.dtype != np.int64 or rows.ndim != 2 or rows.shape[1] != 12 or not rows.flags["C_CONTIGUOUS"]:
        raise _lib.SelftokHipError("image_views: `rows` must be the contiguous int64 numpy [V, 12] table of image_view_rows")
    if code == IMAGE_FILTERS["bilinear"]:
        return _image_resample("image_views", "selftok_img_views_u8", "selftok_img_views_tables_layout", "rows_dev", packed, rows, size, dtype, out, rows_dev, return_tables,
                               empty_ok=True)
    return _image_resample("image_views", "selftok_img_views_filter_u8", "selftok_img_views_filter_tables_layout", "rows_dev", packed, rows, size, dtype, out, rows_dev,
                           return_tables, empty_ok=True, filter=code)


def image_resize(packed: torch.Tensor, frames, filter, frames_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Pillow's Image.resize((ow, oh), filter) of N whole RGB uint8 HWC frames inside the 1-D uint8 device tensor `packed`, IN PLACE: `frames`
    [N, 6] on the host, per frame the source byte offset, W, H, the destination byte offset, ow, oh -- the result is written at the
    destination, bit for bit Pillow's (csrc/image_filters.hip).  Every region must lie inside `packed` and no destination may overlap a
    source or another destination of the call.  `filter`: 'bilinear' / 'bicubic' / 'box' or Pillow's code.  `frames_dev`: the same table
    already on the device (int64), else it is copied here.  N = 0 does nothing.  -> `packed`."""
    import numpy as np
    code = image_filter_code(filter, "image_resize")
    t = np.ascontiguousarray(np.asarray(frames), dtype=np.int64)
    if t.ndim != 2 or t.shape[1] != 6:
        raise _lib.SelftokHipError(f"image_resize: expected [N, 6] (source offset, W, H, destination offset, ow, oh), got {t.shape}")
    _need_cuda(packed, frames_dev)
    if packed.dtype != torch.uint8 or packed.dim() != 1 or not packed.is_contiguous():
        raise _lib.SelftokHipError(f"image_resize: `packed` must be a contiguous 1-D uint8 tensor, got {packed.dtype} {tuple(packed.shape)}")
    N = t.shape[0]
    if N == 0:
        return packed
    lib = _lib.load()
    nbytes = _ws_bytes("selftok_img_resize_u8_workspace_bytes", t.ctypes.data, N, code)
    if frames_dev is None:
        frames_dev = torch.from_numpy(t).to(packed.device)
    elif frames_dev.dtype != torch.int64 or frames_dev.numel() != 6 * N or not frames_dev.is_contiguous():
        raise _lib.SelftokHipError("image_resize: `frames_dev` must be the contiguous int64 [N, 6] table")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=packed.device)
    _lib.check(lib.selftok_img_resize_u8(_p(packed), packed.numel(), t.ctypes.data, _p(frames_dev), N, code, _p(ws), nbytes, _stream()), "selftok_img_resize_u8")
    return packed


def image_to_u8(img: torch.Tensor) -> torch.Tensor:
    """[B, 3, H, W] in [0, 1], bf16 or fp32 -> uint8 [B, H, W, 3] with torchvision.utils.save_image's arithmetic in the tensor's own dtype
    (x * 255, + 0.5, each rounded to the dtype, clamp to [0, 255], truncate); NaN -> 0"""
    _need_cuda(img)
    if img.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.SelftokHipError(f"image_to_u8: dtype {img.dtype}: expected bfloat16 or float32")
    if img.dim() != 4 or img.shape[1] != 3:
        raise _lib.SelftokHipError(f"image_to_u8: expected [B, 3, H, W], got {tuple(img.shape)}")
    img = img.contiguous()
    B, _, H, W = img.shape
    out = torch.empty(B, H, W, 3, dtype=torch.uint8, device=img.device)
    _lib.check(_lib.load().selftok_img_to_u8(_p(img), int(img.dtype == torch.bfloat16), _p(out), B, H, W, _stream()), "selftok_img_to_u8")
    return out


# ---- device image metrics (csrc/image_metrics.hip, include/selftok_hip_ext.h) ----
_img_metrics_ws = _StreamWorkspace(1 << 20)


def image_metrics(recon: torch.Tensor, original: torch.Tensor, original_signed: bool = True, quantize: bool = False) -> torch.Tensor:
    """recon [B, 3, H, W] in [0, 1] against original [B, 3, H, W] (in [-1, 1] when `original_signed`, else in [0, 1]), bf16 or fp32 each -> float64 [B, 2] on the
    device: {mean SSIM, MSE} per image (11 x 11 Gaussian window of sigma 1.5 = evaluate.ssim_window(), valid windows, population moments, fp64; the MSE with
    evaluate.psnr_each's operations).  `quantize`: on the bytes `image_to_u8` would write for both.  No host synchronisation; H, W >= 11."""
    _need_cuda(recon, original)
    recon, original = _image_pair("image_metrics", recon, original)
    from .evaluate import ssim_window
    win = ssim_window()
    B, _, H, W = recon.shape
    ws = _img_metrics_ws(recon.device, _ws_bytes("selftok_img_metrics_workspace_bytes", B, H, W))
    out = torch.empty(B, 2, dtype=torch.float64, device=recon.device)
    _lib.check(_lib.load().selftok_img_metrics(_p(recon), int(recon.dtype == torch.bfloat16), _p(original), int(original.dtype == torch.bfloat16), int(bool(original_signed)),
                                       int(bool(quantize)), win.ctypes.data, _p(out), _p(ws), ws.numel(), B, H, W, _stream()), "selftok_img_metrics")
    return out


SSIM_PRESETS = ("gaussian", "skimage")


def ssim_preset(name: str):
    """(window, cov_norm) of a named SSIM reading: "gaussian" = evaluate.ssim_window() with population moments (image_metrics' SSIM), "skimage" =
    skimage.metrics.structural_similarity's defaults, the uniform 7 x 7 window with the sample covariance (cov_norm 49 / 48)"""
    from .evaluate import ssim_uniform_window, ssim_window
    if name == "gaussian":
        return ssim_window(), 1.0
    if name == "skimage":
        return ssim_uniform_window(7), 49.0 / 48.0
    raise ValueError(f"SSIM preset {name!r}: expected one of {SSIM_PRESETS}")


def image_ssim(recon: torch.Tensor, original: torch.Tensor, window="skimage", cov_norm: Optional[float] = None, signed_range: bool = True,
               original_signed: bool = True, quantize: bool = False) -> torch.Tensor:
    """recon [B, 3, H, W] in [0, 1] against original [B, 3, H, W] (in [-1, 1] when `original_signed`, else in [0, 1]), bf16 or fp32 each -> float64 [B] on the
    device: the mean SSIM of each image over the valid windows, fp64 (include/selftok_hip_ext.h: selftok_img_ssim).  window: T separable fp64 weights
    (T odd, 3 .. 11) with `cov_norm` (1.0: population moments; T^2 / (T^2 - 1): sample covariance), or a preset name of SSIM_PRESETS, which sets both.
    signed_range: operands on [-1, 1] with data range 2 (the reconstruction becomes 2 r - 1), else on [0, 1] with data range 1.  `quantize`: on the bytes
    `image_to_u8` would write for both.  No host synchronisation; H, W >= T."""
    if isinstance(window, str):
        if cov_norm is not None:
            raise ValueError(f"image_ssim: the preset {window!r} sets cov_norm itself")
        window, cov_norm = ssim_preset(window)
    elif cov_norm is None:
        raise ValueError("image_ssim: a window given as weights needs cov_norm (1.0: population moments)")
    _need_cuda(recon, original)
    recon, original = _image_pair("image_ssim", recon, original)
    import numpy as np
    win = np.ascontiguousarray(window, dtype=np.float64).reshape(-1)
    B, _, H, W = recon.shape
    ws = _img_metrics_ws(recon.device, _ws_bytes("selftok_img_ssim_workspace_bytes", B, H, W, int(win.size)))
    out = torch.empty(B, dtype=torch.float64, device=recon.device)
    _lib.check(_lib.load().selftok_img_ssim(_p(recon), int(recon.dtype == torch.bfloat16), _p(original), int(original.dtype == torch.bfloat16), int(bool(original_signed)),
                                    int(bool(quantize)), win.ctypes.data, int(win.size), float(cov_norm), int(bool(signed_range)), _p(out), _p(ws), ws.numel(), B, H, W,
                                    _stream()), "selftok_img_ssim")
    return out


# ---- LPIPS stages (csrc/lpips.hip, include/selftok_hip_ext.h): channels-last fp32 activations [N, H, W, C] ----
def _lpips_f32(name: str, t: torch.Tensor, dim: int) -> torch.Tensor:
    if t.dtype != torch.float32 or t.dim() != dim:
        raise _lib.SelftokHipError(f"lpips: `{name}` must be a float32 tensor of {dim} dimensions, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def lpips_pack_conv_weight(weight: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, KH, KW] fp32 (any device) -> the [KP, CoutP] image lpips_conv2d reads: row k = (kh * KW + kw) * Cin + ci, K rounded up to 16 and Cout to 64
    with zeros.  A re-layout only (no arithmetic), done once when a network is built."""
    if weight.dim() != 4:
        raise _lib.SelftokHipError(f"lpips_pack_conv_weight: expected [Cout, Cin, KH, KW], got {tuple(weight.shape)}")
    Cout, Cin, KH, KW = weight.shape
    n = _ws_bytes("selftok_lpips_conv2d_packed_floats", Cin, Cout, KH, KW)
    K, CP = KH * KW * Cin, -(-Cout // 64) * 64
    out = torch.zeros(n // CP, CP, dtype=torch.float32, device=weight.device)
    out[:K, :Cout] = weight.detach().float().permute(2, 3, 1, 0).reshape(K, Cout)
    return out


def _conv2d(what: str, entry: str, x, packed, bias, Cout: int, KH: int, KW: int, stride: int, pad_h: int, pad_w: int):
    """what lpips_conv2d and fid_conv2d share: the operand checks -> (x, packed, bias, the C entry `entry`, (N, OH, OW))"""
    x, packed = _lpips_f32("x", x, 4), _lpips_f32("packed", packed, 2)
    bias = None if bias is None else _lpips_f32("bias", bias, 1)
    N, H, W, Cin = x.shape
    lib = _lib.load()
    if packed.numel() != lib.selftok_lpips_conv2d_packed_floats(Cin, Cout, KH, KW) or (bias is not None and bias.numel() != Cout):
        raise _lib.SelftokHipError(f"{what}: packed weight of {packed.numel()} floats / bias do not belong to Cin {Cin}, Cout {Cout}, {KH} x {KW}")
    return x, packed, bias, getattr(lib, entry), (N, (H + 2 * pad_h - KH) // stride + 1, (W + 2 * pad_w - KW) // stride + 1)


def lpips_conv2d(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, KH: int, KW: int, stride: int, pad: int, relu: bool,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, H, W, Cin] fp32 channels-last, `packed` from lpips_pack_conv_weight -> [N, OH, OW, Cout]: per output eight k-ordered fmaf chains on the
    f32-input MFMA (chain j takes the taps with k mod 16 in {2j, 2j + 1}), added as ((c0 + c1) + (c2 + c3)) + ((c4 + c5) + (c6 + c7)), + bias, + ReLU
    (include/selftok_hip_ext.h)."""
    _need_cuda(x, packed, bias, out)
    x, packed, bias, entry, (N, OH, OW) = _conv2d("lpips_conv2d", "selftok_lpips_conv2d_f32", x, packed, bias, Cout, KH, KW, stride, pad, pad)
    out = _out("lpips_conv2d", out, torch.float32, (N, max(OH, 0), max(OW, 0), Cout), x.device)     # no output pixel: the entry refuses
    _lib.check(entry(_p(x), _p(packed), _p(bias), _p(out), *x.shape, Cout, KH, KW, stride, pad, int(bool(relu)), _stream()), "selftok_lpips_conv2d_f32")
    return out


def _lpips_maxpool(what: str, K: int, x: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    _need_cuda(x, out)
    x = _lpips_f32("x", x, 4)
    N, H, W, C = x.shape
    out = _out(what, out, torch.float32, (N, max((H - K) // 2 + 1, 0), max((W - K) // 2 + 1, 0), C), x.device)
    entry = f"selftok_{what}_f32"
    _lib.check(getattr(_lib.load(), entry)(_p(x), _p(out), N, H, W, C, _stream()), entry)
    return out


def lpips_maxpool3s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, H, W, C] fp32 channels-last -> [N, (H - 3) // 2 + 1, (W - 3) // 2 + 1, C]: 3 x 3 windows, stride 2, floor mode, no padding"""
    return _lpips_maxpool("lpips_maxpool3s2", 3, x, out)


def lpips_maxpool2s2(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, H, W, C] fp32 channels-last -> [N, H // 2, W // 2, C]: 2 x 2 windows, stride 2, floor mode, no padding (VGG16's MaxPool2d(2, 2))"""
    return _lpips_maxpool("lpips_maxpool2s2", 2, x, out)


def lpips_input(recon: torch.Tensor, original: torch.Tensor, original_signed: bool = True, quantize: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """recon [B, 3, H, W] in [0, 1] and original [B, 3, H, W] (bf16 or fp32 each) -> the scaling layer's output [2B, H, W, 3] fp32, recon images first"""
    recon, original = _image_pair("lpips_input", recon, original)
    _need_cuda(recon, original, out)
    B, _, H, W = recon.shape
    out = _out("lpips_input", out, torch.float32, (2 * B, H, W, 3), recon.device)
    _lib.check(_lib.load().selftok_lpips_input(_p(recon), int(recon.dtype == torch.bfloat16), _p(original), int(original.dtype == torch.bfloat16),
                                               int(bool(original_signed)), int(bool(quantize)), _p(out), B, H, W, _stream()), "selftok_lpips_input")
    return out


eval_workspace = _StreamWorkspace(1 << 20)   # the evaluation arena: lpips.py and fid.py carve their stage buffers from it, the entries below their workspaces


def _eval_ws(entry: str, args, device, workspace: Optional[torch.Tensor]) -> torch.Tensor:
    """the workspace of an evaluation entry: its size query `entry(*args)` (a refusal raises), then the caller's tensor or the arena"""
    nbytes = _ws_bytes(entry, *args)
    return eval_workspace(device, nbytes) if workspace is None else workspace


def lpips_distance(feat: torch.Tensor, w: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feat [2B, h, w, C] fp32 channels-last (images b and b + B are pair b), w [C] fp32 -> fp64 [B]: the tap's contribution to LPIPS, fp64 from the features on.
    accumulate: added to `out` instead of stored."""
    _need_cuda(feat, w, out, workspace)
    feat, w = _lpips_f32("feat", feat, 4), _lpips_f32("w", w, 1)
    N, h, wd, C = feat.shape
    if N < 2 or N % 2 or w.numel() != C:
        raise _lib.SelftokHipError(f"lpips_distance: expected feat [2B, h, w, C] and w [C], got {tuple(feat.shape)} and {tuple(w.shape)}")
    B = N // 2
    if out is None and accumulate:
        raise _lib.SelftokHipError("lpips_distance: accumulate needs `out`")
    out = _out("lpips_distance", out, torch.float64, (B,), feat.device)
    ws = _eval_ws("selftok_lpips_distance_workspace_bytes", (B, h * wd), feat.device, workspace)
    _lib.check(_lib.load().selftok_lpips_distance(_p(feat), _p(w), _p(out), _p(ws), ws.numel() * ws.element_size(), B, h * wd, C, int(bool(accumulate)), _stream()),
               "selftok_lpips_distance")
    return out


# ---- rFID stages (csrc/fid.hip, include/selftok_hip_ext.h): channels-last fp32 activations; an output may be a channel slice of a wider map ----
FID_POOL_MODES = {"max_s2": 0, "max_s1p1": 1, "avg_s1p1": 2}


def _fid_slice_out(what: str, out: Optional[torch.Tensor], shape, C: int, co_off: int, device):
    """the output map of a slice-writing entry: `out` [N, OH, OW, ldo] (contiguous fp32, ldo >= co_off + C) or a fresh [N, OH, OW, C] when None"""
    N, OH, OW = shape
    if out is None:
        if co_off:
            raise _lib.SelftokHipError(f"{what}: a channel offset needs the `out` map it points into")
        return torch.empty(N, max(OH, 0), max(OW, 0), C, dtype=torch.float32, device=device)
    if out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape[:3]) != (N, OH, OW) or not out.is_contiguous() or co_off < 0 or out.shape[3] < co_off + C:
        raise _lib.SelftokHipError(f"{what}: `out` must be a contiguous float32 [{N}, {OH}, {OW}, ldo >= {co_off} + {C}], got {out.dtype} {tuple(out.shape)}")
    return out


def fid_conv2d(x: torch.Tensor, packed: torch.Tensor, bias: Optional[torch.Tensor], Cout: int, KH: int, KW: int, stride: int, pad_h: int, pad_w: int, relu: bool = True,
               out: Optional[torch.Tensor] = None, co_off: int = 0) -> torch.Tensor:
    """lpips_conv2d's convolution (same kernel body, same packed weight) with a padding per axis, writing channels co_off .. co_off + Cout - 1 of the map
    `out` [N, OH, OW, ldo] and nothing else of it.  Returns the map."""
    _need_cuda(x, packed, bias, out)
    x, packed, bias, entry, (N, OH, OW) = _conv2d("fid_conv2d", "selftok_fid_conv2d_f32", x, packed, bias, Cout, KH, KW, stride, pad_h, pad_w)
    _, H, W, _ = x.shape
    if H + 2 * pad_h < KH or W + 2 * pad_w < KW:                  # decided here: an empty tensor has no pointer to hand to the entry
        raise _lib.SelftokHipError(f"fid_conv2d: {H} x {W} input has no output pixel under a {KH} x {KW} kernel with pad {pad_h}, {pad_w}")
    out = _fid_slice_out("fid_conv2d", out, (N, OH, OW), Cout, co_off, x.device)
    _lib.check(entry(_p(x), _p(packed), _p(bias), _p(out), *x.shape, Cout, KH, KW, stride, pad_h, pad_w, out.shape[3], co_off, int(bool(relu)), _stream()),
               "selftok_fid_conv2d_f32")
    return out


def fid_pool3(x: torch.Tensor, mode: str, out: Optional[torch.Tensor] = None, co_off: int = 0) -> torch.Tensor:
    """3 x 3 pool of x [N, H, W, C]: mode "max_s2" (stride 2, no padding), "max_s1p1" or "avg_s1p1" (stride 1, pad 1; the average divides by the number of
    in-image taps), into channels co_off .. co_off + C - 1 of the map `out`.  Returns the map."""
    _need_cuda(x, out)
    x = _lpips_f32("x", x, 4)
    if mode not in FID_POOL_MODES:
        raise _lib.SelftokHipError(f"fid_pool3: mode {mode!r}: expected one of {sorted(FID_POOL_MODES)}")
    N, H, W, C = x.shape
    if mode == "max_s2" and min(H, W) < 3:
        raise _lib.SelftokHipError(f"fid_pool3: max_s2 needs H, W >= 3 (one window), got {H} x {W}")
    PH, PW = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == "max_s2" else (H, W)
    out = _fid_slice_out("fid_pool3", out, (N, PH, PW), C, co_off, x.device)
    _lib.check(_lib.load().selftok_fid_pool3_f32(_p(x), _p(out), N, H, W, C, FID_POOL_MODES[mode], out.shape[3], co_off, _stream()), "selftok_fid_pool3_f32")
    return out


def fid_input(images: torch.Tensor, signed: bool, quantize: bool = False, tables=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """images [B, 3, H, W] (bf16 or fp32; in [-1, 1] when `signed`, else in [0, 1]) -> [B, OH, OW, 3] fp32 in [-1, 1].  `tables`: (ytab, xtab) int32 device
    tensors [3, OH] and [3, OW] from fid.resize_tables (i0, i1, the bits of the fp32 lambda): the bilinear resize; None: the image as it is."""
    if images.dtype not in (torch.bfloat16, torch.float32):
        raise _lib.SelftokHipError(f"fid_input: dtype {images.dtype}: expected bfloat16 or float32")
    if images.dim() != 4 or images.shape[1] != 3:
        raise _lib.SelftokHipError(f"fid_input: expected a [B, 3, H, W] tensor, got {tuple(images.shape)}")
    _need_cuda(images, out)
    images = images.contiguous()
    B, _, H, W = images.shape
    OH, OW, ytab, xtab = H, W, None, None
    if tables is not None:
        ytab, xtab = tables
        _need_cuda(ytab, xtab)
        for t in (ytab, xtab):
            if t.dtype != torch.int32 or t.dim() != 2 or t.shape[0] != 3 or not t.is_contiguous():
                raise _lib.SelftokHipError(f"fid_input: a tap table must be a contiguous int32 [3, n], got {t.dtype} {tuple(t.shape)}")
        OH, OW = ytab.shape[1], xtab.shape[1]
    out = _out("fid_input", out, torch.float32, (B, OH, OW, 3), images.device)
    _lib.check(_lib.load().selftok_fid_input(_p(images), int(images.dtype == torch.bfloat16), int(bool(signed)), int(bool(quantize)), _p(out), B, H, W, OH, OW,
                                             _p(ytab), _p(xtab), _stream()), "selftok_fid_input")
    return out


def fid_spatial_mean(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [N, h, w, C] fp32 channels-last -> [N, C]: per image and channel the pixels added in index order in fp32, then one division"""
    _need_cuda(x, out)
    x = _lpips_f32("x", x, 4)
    N, h, w, C = x.shape
    out = _out("fid_spatial_mean", out, torch.float32, (N, C), x.device)
    _lib.check(_lib.load().selftok_fid_spatial_mean_f32(_p(x), _p(out), N, h * w, C, _stream()), "selftok_fid_spatial_mean_f32")
    return out


def fid_stats(x: torch.Tensor, mu: Optional[torch.Tensor] = None, sigma: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """x [N, D] fp32 -> (mu [D], sigma [D, D]) fp64 on the device: the mean and the unbiased covariance, two fp64 passes in the fixed order csrc/fid.hip states"""
    _need_cuda(x, mu, sigma, workspace)
    x = _lpips_f32("x", x, 2)
    N, D = x.shape
    ws = _eval_ws("selftok_fid_stats_workspace_bytes", (N, D), x.device, workspace)
    mu = _out("fid_stats", mu, torch.float64, (D,), x.device, "mu")
    sigma = _out("fid_stats", sigma, torch.float64, (D, D), x.device, "sigma")
    _lib.check(_lib.load().selftok_fid_stats(_p(x), _p(mu), _p(sigma), _p(ws), ws.numel() * ws.element_size(), N, D, _stream()), "selftok_fid_stats")
    return mu, sigma


# ---- generative-model metrics (csrc/gen_metrics.hip, include/selftok_hip_ext.h): squared-distance k-NN radii, manifold membership, Inception Score ----
def _gm_rows(name: str, t: torch.Tensor) -> torch.Tensor:
    if t.dim() != 2 or t.dtype != torch.float32:
        raise _lib.SelftokHipError(f"{name}: expected a float32 [rows, D] tensor, got {t.dtype} {tuple(t.shape)}")
    return t.contiguous()


def knn_radius(a: torch.Tensor, k: int = 3, *, split: int = 0, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [N, D] fp32 -> r2 [N] fp32: the k-th smallest SQUARED distance of every row to the other rows (its own index skipped), 1 <= k <= 8, N > k.
    The N x N matrix is never stored.  split: launch-shape override (0 = automatic), never visible in the result."""
    a = _gm_rows("knn_radius", a)
    _need_cuda(a, out, workspace)
    N, D = a.shape
    ws = _eval_ws("selftok_knn_radius_f32_workspace_bytes", (N, D, int(k)), a.device, workspace)
    out = _out("knn_radius", out, torch.float32, (N,), a.device)
    _lib.check(_lib.load().selftok_knn_radius_f32(_p(a), _p(out), _p(ws), ws.numel() * ws.element_size(), N, D, int(k), int(split), _stream()), "selftok_knn_radius_f32")
    return out


def manifold_member(x: torch.Tensor, a: torch.Tensor, r2: torch.Tensor, *, split: int = 0, out: Optional[torch.Tensor] = None,
                    workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [M, D], a [N, D], r2 [N] fp32 -> int32 [M]: 1 where d2(x_i, a_j) <= r2[j] for some j.  M == 0 gives an empty tensor without a launch."""
    x, a = _gm_rows("manifold_member", x), _gm_rows("manifold_member", a)
    _need_cuda(x, a, r2, out, workspace)
    M, D = x.shape
    N = a.shape[0]
    if a.shape[1] != D or r2.dtype != torch.float32 or tuple(r2.shape) != (N,):
        raise _lib.SelftokHipError(f"manifold_member: expected x [M, D], a [N, D] and a float32 r2 [N], got {tuple(x.shape)}, {tuple(a.shape)}, {r2.dtype} {tuple(r2.shape)}")
    r2 = r2.contiguous()
    ws = _eval_ws("selftok_manifold_member_f32_workspace_bytes", (M, N, D), x.device, workspace)
    out = _out("manifold_member", out, torch.int32, (M,), x.device)
    _lib.check(_lib.load().selftok_manifold_member_f32(_p(x) if M else None, _p(a), _p(r2), _p(out) if M else None, _p(ws), ws.numel() * ws.element_size(), M, N, D, int(split),
                                               _stream()), "selftok_manifold_member_f32")
    return out


def _is_logits(name: str, logits: torch.Tensor) -> torch.Tensor:
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise _lib.SelftokHipError(f"{name}: expected float32 logits [N, C], got {logits.dtype} {tuple(logits.shape)}")
    return logits.contiguous()


def is_colmean(logits: torch.Tensor, split_size: int, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """logits [N, C] fp32 -> fp64 [ceil(N / split_size), C]: the column means of softmax(logits) over every consecutive split (the last, partial one included)"""
    _need_cuda(logits, workspace)
    logits = _is_logits("is_colmean", logits)
    N, C = logits.shape
    ws = _eval_ws("selftok_is_colmean_workspace_bytes", (N, C, int(split_size)), logits.device, workspace)
    out = torch.empty(-(-N // int(split_size)), C, dtype=torch.float64, device=logits.device)
    _lib.check(_lib.load().selftok_is_colmean(_p(logits), _p(out), _p(ws), ws.numel() * ws.element_size(), N, C, int(split_size), _stream()), "selftok_is_colmean")
    return out


def is_kl_rows(logits: torch.Tensor, colmean: torch.Tensor, split_size: int, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """kl[n] = sum_y p_ny (log p_ny - log colmean[n // split_size, y]) in fp64, p = softmax(logits[n]) -> fp64 [N]"""
    _need_cuda(logits, colmean, workspace)
    logits = _is_logits("is_kl_rows", logits)
    N, C = logits.shape
    ws = _eval_ws("selftok_is_kl_rows_workspace_bytes", (N, C, int(split_size)), logits.device, workspace)
    if colmean.dtype != torch.float64 or tuple(colmean.shape) != (-(-N // int(split_size)), C) or not colmean.is_contiguous():
        raise _lib.SelftokHipError(f"is_kl_rows: `colmean` must be a contiguous float64 {(-(-N // int(split_size)), C)}, got {colmean.dtype} {tuple(colmean.shape)}")
    out = torch.empty(N, dtype=torch.float64, device=logits.device)
    _lib.check(_lib.load().selftok_is_kl_rows(_p(logits), _p(colmean), _p(out), _p(ws), ws.numel() * ws.element_size(), N, C, int(split_size), _stream()), "selftok_is_kl_rows")
    return out


# ---- density / coverage, nearest neighbours, KID (csrc/gen_metrics_kdc.hip): ball counts and the nearest set row per query, the polynomial-kernel sums ----
def manifold_count_nn(x: torch.Tensor, a: torch.Tensor, r2: Optional[torch.Tensor] = None, *, split: int = 0, out_count: Optional[torch.Tensor] = None,
                      out_d2: Optional[torch.Tensor] = None, out_idx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """x [M, D], a [N, D] fp32, r2 [N] fp32 or None -> (count int32 [M] | None, nn_d2 fp32 [M], nn_idx int32 [M]): count[i] = the number of j with
    d2(x_i, a_j) <= r2[j] (None without radii), nn_d2[i] = the smallest non-NaN d2(x_i, a_j) and nn_idx[i] the lowest j that has it (NaN / -1 when there is none).
    The M x N matrix is never stored; the d2 bits are manifold_member's.  split: launch-shape override, never visible in the result.  M == 0: empty tensors, no launch."""
    x, a = _gm_rows("manifold_count_nn", x), _gm_rows("manifold_count_nn", a)
    _need_cuda(x, a, r2, out_count, out_d2, out_idx, workspace)
    M, D = x.shape
    N = a.shape[0]
    if a.shape[1] != D or (r2 is not None and (r2.dtype != torch.float32 or tuple(r2.shape) != (N,))):
        raise _lib.SelftokHipError(f"manifold_count_nn: expected x [M, D], a [N, D] and a float32 r2 [N] or None, got {tuple(x.shape)}, {tuple(a.shape)}, "
                                   f"{None if r2 is None else (r2.dtype, tuple(r2.shape))}")
    if r2 is None and out_count is not None:
        raise _lib.SelftokHipError("manifold_count_nn: `out_count` without r2 (no radii, no count)")
    r2 = None if r2 is None else r2.contiguous()
    lib = _lib.load()
    ws = _eval_ws("selftok_manifold_count_nn_f32_workspace_bytes", (M, N, D), x.device, workspace)
    outs = []
    for name, t, dtype, want in (("out_count", out_count, torch.int32, r2 is not None), ("out_d2", out_d2, torch.float32, True), ("out_idx", out_idx, torch.int32, True)):
        if not want:
            outs.append(None)
        elif t is None:
            outs.append(torch.empty(M, dtype=dtype, device=x.device))
        elif t.dtype != dtype or tuple(t.shape) != (M,) or not t.is_contiguous():
            raise _lib.SelftokHipError(f"manifold_count_nn: `{name}` must be a contiguous {dtype} [{M}], got {t.dtype} {tuple(t.shape)}")
        else:
            outs.append(t)
    count, d2, idx = outs
    if M:
        _lib.check(lib.selftok_manifold_count_nn_f32(_p(x), _p(a), _p(r2), _p(count), _p(d2), _p(idx), _p(ws), ws.numel() * ws.element_size(), M, N, D, int(split), _stream()),
                   "selftok_manifold_count_nn_f32")
    return count, d2, idx


def kid_sums(xs: torch.Tensor, ys: torch.Tensor, S: int, m: int, *, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """xs, ys [S * m, D] fp32: subset s is rows s * m .. s * m + m - 1 of either -> fp64 [S, 3] = (XX, YY, XY) of k(u, v) = (u.v / D + 1)^3, XX and YY without
    the positions i == j.  A subset's triple depends on its own 2 m rows alone."""
    xs, ys = _gm_rows("kid_sums", xs), _gm_rows("kid_sums", ys)
    _need_cuda(xs, ys, out, workspace)
    S, m = int(S), int(m)
    D = xs.shape[1]
    if tuple(xs.shape) != (S * m, D) or tuple(ys.shape) != (S * m, D) or S < 1:
        raise _lib.SelftokHipError(f"kid_sums: expected xs and ys [S * m, D] = [{S * m}, D], got {tuple(xs.shape)} and {tuple(ys.shape)}")
    ws = _eval_ws("selftok_kid_sums_f32_workspace_bytes", (S, m, D), xs.device, workspace)
    out = _out("kid_sums", out, torch.float64, (S, 3), xs.device)
    _lib.check(_lib.load().selftok_kid_sums_f32(_p(xs), _p(ys), _p(out), _p(ws), ws.numel() * ws.element_size(), S, m, D, _stream()), "selftok_kid_sums_f32")
    return out


# ----------------------------------------------------------------------------------------------
# decode stream: one sampler step per slot (csrc/decode_stream.hip)
# ----------------------------------------------------------------------------------------------

def _stream_check(what: str, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.SelftokHipError(f"{what}: expected a contiguous {dtype} {list(shape)}, got {t.dtype} {list(t.shape)}")


def stream_prepare(step, limit, coef, pattern_words, table, table_uncond, segs, kwords_out, coef_out, mods_out, mods_uncond_out=None, *, K: int):
    """step int32 [B] (a slot is active iff 0 <= step < n_steps), limit int32 [n_steps], coef fp32 [n_steps, 4] = (dt, t, t_prev, 0),
    pattern_words int32 [B, ceil(K / 32)] or None (every key), table / table_uncond fp32 [n_steps, R] (the second or None), segs: a HOST
    numpy int32 [S, 2] of (first column, width) -> writes kwords_out [B, W] (the slot's pattern below its step's limit), coef_out [B, 4] =
    (dt, t, t_prev, active) and the slots' table rows into mods_out / mods_uncond_out [B * R], segment-major: segment s is the
    contiguous [B, width_s] tensor at offset B * first_s.  No host synchronisation, nothing allocated."""
    import numpy as np
    _need_cuda(step, limit, coef, pattern_words, table, table_uncond, kwords_out, coef_out, mods_out, mods_uncond_out)
    if not isinstance(segs, np.ndarray) or segs.dtype != np.int32 or segs.ndim != 2 or segs.shape[1] != 2 or not segs.flags.c_contiguous:
        raise _lib.SelftokHipError("stream_prepare: `segs` must be a C-contiguous host numpy int32 [S, 2]")
    B, W = step.shape[0], (int(K) + 31) // 32
    n_steps, R = table.shape
    _stream_check("stream_prepare: step", step, torch.int32, (B,))
    _stream_check("stream_prepare: limit", limit, torch.int32, (n_steps,))
    _stream_check("stream_prepare: coef", coef, torch.float32, (n_steps, 4))
    _stream_check("stream_prepare: table", table, torch.float32, (n_steps, R))
    _stream_check("stream_prepare: kwords_out", kwords_out, torch.int32, (B, W))
    _stream_check("stream_prepare: coef_out", coef_out, torch.float32, (B, 4))
    _stream_check("stream_prepare: mods_out", mods_out, torch.float32, (B * R,))
    if pattern_words is not None:
        _stream_check("stream_prepare: pattern_words", pattern_words, torch.int32, (B, W))
    if (table_uncond is None) != (mods_uncond_out is None):
        raise _lib.SelftokHipError("stream_prepare: table_uncond and mods_uncond_out come together")
    if table_uncond is not None:
        _stream_check("stream_prepare: table_uncond", table_uncond, torch.float32, (n_steps, R))
        _stream_check("stream_prepare: mods_uncond_out", mods_uncond_out, torch.float32, (B * R,))
    _lib.check(_lib.load().selftok_stream_prepare(_p(step), _p(limit), _p(coef), _p(pattern_words), _p(table), _p(table_uncond), segs.ctypes.data, segs.shape[0],
                                                  _p(kwords_out), _p(coef_out), _p(mods_out), _p(mods_uncond_out), B, int(K), n_steps, R, _stream()),
               "selftok_stream_prepare")


def unpatchify_cfg_euler_rows(y_cond, y_uncond, x, coef_rows, step, *, cfg_scale: float = 1.0, x0_param: bool = False, x_out=None, step_out=None):
    """`unpatchify_cfg_euler` with one dt per slot: coef_rows fp32 [B, 4] = (dt, t, t_prev, active) as `stream_prepare` writes it, step int32 [B].
    An active slot gets the Euler update (x0_param: v + t_prev * (x - v) / t) and step + 1, an idle one keeps x and step byte for byte.
    x_out / step_out None: IN PLACE.  -> (x_out, step_out)"""
    _need_cuda(y_cond, y_uncond, x, coef_rows, step, x_out, step_out)
    B, C, Hh, Ww = x.shape
    hp, wp = Hh // 2, Ww // 2
    x_out = x if x_out is None else x_out
    step_out = step if step_out is None else step_out
    _stream_check("unpatchify_cfg_euler_rows: x", x, torch.float32, (B, C, 2 * hp, 2 * wp))
    _stream_check("unpatchify_cfg_euler_rows: x_out", x_out, torch.float32, (B, C, 2 * hp, 2 * wp))
    _stream_check("unpatchify_cfg_euler_rows: y_cond", y_cond, torch.float32, (B, hp * wp, 4 * C))
    if y_uncond is not None:
        _stream_check("unpatchify_cfg_euler_rows: y_uncond", y_uncond, torch.float32, (B, hp * wp, 4 * C))
    _stream_check("unpatchify_cfg_euler_rows: coef_rows", coef_rows, torch.float32, (B, 4))
    _stream_check("unpatchify_cfg_euler_rows: step", step, torch.int32, (B,))
    _stream_check("unpatchify_cfg_euler_rows: step_out", step_out, torch.int32, (B,))
    _lib.check(_lib.load().selftok_unpatchify_cfg_euler_rows_f32(_p(y_cond), _p(y_uncond), _p(x), _p(x_out), _p(coef_rows), _p(step), _p(step_out), B, C, hp, wp,
                                                                 float(cfg_scale), int(bool(x0_param)), _stream()), "selftok_unpatchify_cfg_euler_rows_f32")
    return x_out, step_out


# ----------------------------------------------------------------------------------------------
# token statistics (csrc/token_stats.hip): code counts, census, agreement, nearest sequence
# ----------------------------------------------------------------------------------------------
_TOKEN_ID_BYTES = {torch.uint16: 2, torch.int32: 4, torch.int64: 8}


def _token_ids(what: str, ids: torch.Tensor):
    """ids [..., K] of dtype uint16 / int32 / int64, any strides -> (tensor, n_rows, K, row_stride, elem_stride) without a copy where the leading
    dimensions collapse into one row stride (a [N, K] view of any strides always does); otherwise one contiguous copy"""
    if ids.dtype not in _TOKEN_ID_BYTES or ids.dim() < 1:
        raise _lib.SelftokHipError(f"{what}: expected uint16, int32 or int64 ids [..., K], got {ids.dtype} {tuple(ids.shape)}")
    K = ids.shape[-1]
    if ids.dim() == 1:
        ids = ids.unsqueeze(0)
    elif ids.dim() > 2:
        lead = ids.shape[:-1]
        n = 1
        for v in lead:
            n *= v
        try:
            ids = ids.view(n, K)                                   # strided views that still collapse stay views
        except RuntimeError:
            ids = ids.reshape(n, K)
    n_rows = ids.shape[0]
    rs, es = (ids.stride(0), ids.stride(1)) if n_rows and K else (K, 1)
    if rs < 0 or es < 0 or (n_rows > 1 and rs == 0):
        ids = ids.contiguous()
        rs, es = K, 1
    return ids, n_rows, K, rs, es


def _token_u32(what: str, name: str, t: torch.Tensor, shape):
    if t.dtype not in (torch.int32, torch.uint32) or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise _lib.SelftokHipError(f"{what}: `{name}` must be a contiguous 32-bit integer tensor {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")


def token_count(ids: torch.Tensor, counts: torch.Tensor, bad: torch.Tensor) -> None:
    """counts[k, id] += 1 for every row and position of ids [..., K] (uint16 / int32 / int64, strided views counted in place: column 0 of an
    `encoding_topk` result needs no copy).  counts: 32-bit [K, C], bad: 32-bit [1], both ACCUMULATING (uint32 arithmetic); an id outside [0, C) only adds 1
    to bad.  No synchronisation."""
    _need_cuda(ids, counts, bad)
    if counts.dim() != 2:
        raise _lib.SelftokHipError(f"token_count: `counts` must be [K, C], got {tuple(counts.shape)}")
    ids, n_rows, K, rs, es = _token_ids("token_count", ids)
    _token_u32("token_count", "counts", counts, (K, counts.shape[1]))
    _token_u32("token_count", "bad", bad, (1,))
    lib = _lib.load()
    _lib.check(lib.selftok_token_count(_p(ids) if n_rows else None, _TOKEN_ID_BYTES[ids.dtype], n_rows, K, counts.shape[1], rs, es, _p(counts), _p(bad), _stream()),
               "selftok_token_count")


def token_census(counts: torch.Tensor, out: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """counts 32-bit [K, C] -> fp64 [K + 1, 5]: (n, used, H, H_ref, max_count) per position, row K for the pooled counts (uint64 column sums).  Entropies in nats,
    fp64 in a fixed order: the same bits every run."""
    _need_cuda(counts, out, workspace)
    if counts.dim() != 2:
        raise _lib.SelftokHipError(f"token_census: `counts` must be [K, C], got {tuple(counts.shape)}")
    K, C = counts.shape
    _token_u32("token_census", "counts", counts, (K, C))
    need = _ws_bytes("selftok_token_census_workspace_bytes", K, C)
    ws = torch.empty(need // 8, dtype=torch.int64, device=counts.device) if workspace is None else workspace
    out = _out("token_census", out, torch.float64, (K + 1, 5), counts.device)
    _lib.check(_lib.load().selftok_token_census(_p(counts), K, C, _p(out), _p(ws), ws.numel() * ws.element_size(), _stream()), "selftok_token_census")
    return out


def token_to_u16(ids: torch.Tensor, bad: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ids [..., K] (uint16 / int32 / int64, any strides) -> dense uint16 [n_rows, K]; an id outside [0, 65535] becomes 0 and adds 1 to bad[0] (32-bit [1],
    accumulating; allocated zeroed when None and then dropped: pass one to see it)."""
    _need_cuda(ids, bad, out)
    ids, n_rows, K, rs, es = _token_ids("token_to_u16", ids)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=ids.device)
    _token_u32("token_to_u16", "bad", bad, (1,))
    out = _out("token_to_u16", out, torch.uint16, (n_rows, K), ids.device)
    lib = _lib.load()
    _lib.check(lib.selftok_token_to_u16(_p(ids) if n_rows else None, _TOKEN_ID_BYTES[ids.dtype], n_rows, K, rs, es, _p(out) if n_rows else None, _p(bad), _stream()),
               "selftok_token_to_u16")
    return out


def _token_dense(what: str, name: str, t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.uint16 or t.dim() != 2 or not t.is_contiguous():
        raise _lib.SelftokHipError(f"{what}: `{name}` must be a dense uint16 [rows, K] tensor (ops.token_to_u16 makes one), got {t.dtype} {tuple(t.shape)}")
    return t


def _token_range(what: str, K: int, k_range):
    k_lo, k_hi = (0, K) if k_range is None else (int(k_range[0]), int(k_range[1]))
    if not 0 <= k_lo <= k_hi <= K:
        raise _lib.SelftokHipError(f"{what}: k_range must satisfy 0 <= k_lo <= k_hi <= K = {K}, got ({k_lo}, {k_hi})")
    return k_lo, k_hi


def token_agree(a: torch.Tensor, b: torch.Tensor, k_range=None, match_pos: Optional[torch.Tensor] = None):
    """a, b dense uint16 [N, K] -> (match_pos 32-bit [K], n_diff, first_diff, last_diff int32 [N]) over the positions k_range = (k_lo, k_hi), default every one:
    match_pos[k] += the rows that agree at k (accumulating when passed in, zeroed when allocated here), first_diff K and last_diff -1 for equal rows."""
    _need_cuda(a, b, match_pos)
    a, b = _token_dense("token_agree", "a", a), _token_dense("token_agree", "b", b)
    if a.shape != b.shape:
        raise _lib.SelftokHipError(f"token_agree: a and b must have one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    N, K = a.shape
    k_lo, k_hi = _token_range("token_agree", K, k_range)
    if match_pos is None:
        match_pos = torch.zeros(K, dtype=torch.int32, device=a.device)
    _token_u32("token_agree", "match_pos", match_pos, (K,))
    n_diff, first, last = (torch.empty(N, dtype=torch.int32, device=a.device) for _ in range(3))
    lib = _lib.load()
    _lib.check(lib.selftok_token_agree(_p(a) if N else None, _p(b) if N else None, N, K, k_lo, k_hi, _p(match_pos), _p(n_diff) if N else None, _p(first) if N else None,
                                       _p(last) if N else None, _stream()), "selftok_token_agree")
    return match_pos, n_diff, first, last


def token_nearest(q: torch.Tensor, ref: torch.Tensor, k_range=None, exclude_self: int = 0, *, split: int = 0, out_match: Optional[torch.Tensor] = None,
                  out_idx: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """q [M, K], ref [N, K] dense uint16 -> (best_match, best_idx) int32 [M]: the largest number of equal positions in k_range over the reference rows and the
    lowest index that attains it; (-1, 0) without a candidate.  exclude_self: 0 = every row is a candidate, 1 + o skips j == i + o (1: the set against itself).
    split: launch-shape override, never visible in the result.  M == 0: empty tensors, no launch."""
    _need_cuda(q, ref, out_match, out_idx, workspace)
    q, ref = _token_dense("token_nearest", "q", q), _token_dense("token_nearest", "ref", ref)
    M, K = q.shape
    N = ref.shape[0]
    if ref.shape[1] != K:
        raise _lib.SelftokHipError(f"token_nearest: q and ref must have one K, got {tuple(q.shape)} and {tuple(ref.shape)}")
    k_lo, k_hi = _token_range("token_nearest", K, k_range)
    need = _ws_bytes("selftok_token_nearest_workspace_bytes", M, N)
    ws = torch.empty(need // 8, dtype=torch.int64, device=q.device) if workspace is None else workspace
    outs = [_out("token_nearest", t, torch.int32, (M,), q.device, name) for name, t in (("out_match", out_match), ("out_idx", out_idx))]
    if M:
        _lib.check(_lib.load().selftok_token_nearest(_p(q), M, _p(ref) if N else None, N, K, k_lo, k_hi, int(exclude_self), int(split), _p(outs[0]), _p(outs[1]), _p(ws),
                                             ws.numel() * ws.element_size(), _stream()), "selftok_token_nearest")
    return outs[0], outs[1]


# ----------------------------------------------------------------------------------------------
# token sampler (csrc/token_sample.hip): AR logits over a window of codes -> one code id per row
# ----------------------------------------------------------------------------------------------
_SAMPLE_DTYPES = {torch.float32: 0, torch.bfloat16: 1}


def token_sample(logits: torch.Tensor, ctr: torch.Tensor, ids_out: torch.Tensor, *, uncond_logits: Optional[torch.Tensor] = None, C: Optional[int] = None,
                 offset: int = 0, cfg_scale: float = 1.0, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, seed: int = 0,
                 pos: Optional[torch.Tensor] = None, col: int = 0, n_kept: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None,
                 logprob: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None):
    """One code id per row of `logits` [B, V] (fp32 or bf16, row stride a multiple of 4 codes) over the window [offset, offset + C) (default: the rest of the
    row): guidance `lu + cfg_scale * (lc - lu)` when `uncond_logits` (same shape, dtype and strides) is given, temperature (0 = greedy), top-k (<= 0 off),
    top-p (outside (0, 1) off) and one Philox4x32-10 draw per row with key `seed` (64 bits) and counter ctr[b] (32-bit [B, 2]) -- include/selftok_hip_ext.h
    states the arithmetic, which numpy reproduces bit for bit.  The id (0-based inside the window) of row b is written to ids_out[b, pos[b]] (`pos` int32 [B]) or
    ids_out[b, col]; ids_out is int32 or int64 [B, K] with unit column stride.  -> (n_kept int32 [B], mass int64 [B, 3] holding the uint64 (Q_total, Q_kept,
    q_id), logprob fp32 [B], bad 32-bit [1], accumulating).  A bad row (NaN / +inf / all -inf, or pos outside [0, K)) gets id -1, n_kept 0, masses 0, logprob
    NaN and adds 1 to bad.  No synchronisation, nothing read back."""
    _need_cuda(logits, uncond_logits, ctr, ids_out, pos, n_kept, mass, logprob, bad)
    what = "token_sample"
    if logits.dtype not in _SAMPLE_DTYPES or logits.dim() != 2:
        raise _lib.SelftokHipError(f"{what}: `logits` must be fp32 or bf16 [B, V], got {logits.dtype} {tuple(logits.shape)}")
    B, V = logits.shape
    if C is None:
        C = V - int(offset)
    C, offset = int(C), int(offset)
    if offset < 0 or C < 1 or offset + C > V:
        raise _lib.SelftokHipError(f"{what}: the window [{offset}, {offset} + {C}) does not lie inside a row of {V} codes")
    if V and logits.stride(1) != 1:
        raise _lib.SelftokHipError(f"{what}: `logits` rows must have unit element stride, got strides {logits.stride()}")
    rs = logits.stride(0) if B > 1 else max(V, logits.stride(0))
    if uncond_logits is not None and (uncond_logits.dtype != logits.dtype or uncond_logits.shape != logits.shape or (B > 1 and uncond_logits.stride() != logits.stride())
                                      or uncond_logits.stride(1) != 1):
        raise _lib.SelftokHipError(f"{what}: `uncond_logits` must have the dtype, shape and strides of `logits`")
    if ctr.dtype not in (torch.int32, torch.uint32) or tuple(ctr.shape) != (B, 2) or not ctr.is_contiguous():
        raise _lib.SelftokHipError(f"{what}: `ctr` must be a contiguous 32-bit integer tensor [{B}, 2], got {ctr.dtype} {tuple(ctr.shape)}")
    if ids_out.dtype not in (torch.int32, torch.int64) or ids_out.dim() != 2 or ids_out.shape[0] != B or ids_out.shape[1] < 1 or ids_out.stride(1) != 1 or \
            (B > 1 and ids_out.stride(0) < ids_out.shape[1]):
        raise _lib.SelftokHipError(f"{what}: `ids_out` must be int32 or int64 [{B}, K] with unit column stride, got {ids_out.dtype} {tuple(ids_out.shape)}")
    K = ids_out.shape[1]
    if pos is not None:
        if pos.dtype != torch.int32 or tuple(pos.shape) != (B,) or not pos.is_contiguous():
            raise _lib.SelftokHipError(f"{what}: `pos` must be a contiguous int32 tensor [{B}], got {pos.dtype} {tuple(pos.shape)}")
    elif not 0 <= int(col) < K:
        raise _lib.SelftokHipError(f"{what}: col {col} outside [0, {K})")
    dev = logits.device
    n_kept = _out(what, n_kept, torch.int32, (B,), dev, "n_kept")
    mass = _out(what, mass, torch.int64, (B, 3), dev, "mass")
    logprob = _out(what, logprob, torch.float32, (B,), dev, "logprob")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    _token_u32(what, "bad", bad, (1,))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids_ptr = _p(ids_out) + (0 if pos is not None else int(col) * ids_out.element_size())
    _lib.check(_lib.load().selftok_sample_token(_p(logits), _p(uncond_logits), _SAMPLE_DTYPES[logits.dtype], B, C, rs, offset, float(cfg_scale), float(temperature),
                                                int(top_k), float(top_p), seed & 0xFFFFFFFF, seed >> 32, _p(ctr), _p(pos), ids_ptr, ids_out.element_size(),
                                                ids_out.stride(0) if B > 1 else K, K if pos is not None else 1, _p(n_kept), _p(mass), _p(logprob), _p(bad), _stream()),
               "selftok_sample_token")
    return n_kept, mass, logprob, bad


# ----------------------------------------------------------------------------------------------
# speculative sampling (csrc/token_verify.hip): S drafted ids per sequence verified against the target's logits, the accepted prefix committed
# ----------------------------------------------------------------------------------------------
VerifyOut = collections.namedtuple("VerifyOut", "accept repl_id n_kept mass logprob_x logprob_repl n_accept n_emit foreign bad")


def _spec_rows(what: str, name: str, t: torch.Tensor, B: int, rows: int):
    """[B, rows, V] logits -> (V, sequence stride, row stride) in elements; a dimension of one element gets the stride a dense tensor would have"""
    if t.dtype not in _SAMPLE_DTYPES or t.dim() != 3 or t.shape[0] != B or t.shape[1] != rows:
        raise _lib.SelftokHipError(f"{what}: `{name}` must be fp32 or bf16 [{B}, {rows}, V], got {t.dtype} {tuple(t.shape)}")
    V = int(t.shape[2])
    if V and t.stride(2) != 1:
        raise _lib.SelftokHipError(f"{what}: `{name}` rows must have unit element stride, got strides {t.stride()}")
    row = int(t.stride(1)) if rows > 1 else V + (-V) % 4
    seq = int(t.stride(0)) if B > 1 else max(rows * row, 0)
    return V, seq, row


def token_verify(target_logits: torch.Tensor, draft_logits: Optional[torch.Tensor], draft_ids: Optional[torch.Tensor], ctr: torch.Tensor, ids: torch.Tensor,
                 logprob: torch.Tensor, n_kept: torch.Tensor, *, target_uncond: Optional[torch.Tensor] = None, draft_uncond: Optional[torch.Tensor] = None,
                 C: Optional[int] = None, offset: int = 0, cfg_scale: float = 1.0, draft_cfg_scale: float = 1.0, temperature: float = 1.0, top_k: int = 0,
                 top_p: float = 1.0, seed: int = 0, n_draft=None, n_draft_dev: Optional[torch.Tensor] = None, accept: Optional[torch.Tensor] = None,
                 repl_id: Optional[torch.Tensor] = None, row_n_kept: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None,
                 logprob_x: Optional[torch.Tensor] = None, logprob_repl: Optional[torch.Tensor] = None, n_accept: Optional[torch.Tensor] = None,
                 n_emit: Optional[torch.Tensor] = None, foreign: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None) -> VerifyOut:
    """One round of speculative sampling: `target_logits` [B, S + 1, V] and `draft_logits` [B, S, V] (fp32 or bf16 each, on their own; None when S = 0) over
    the window [offset, offset + C), `draft_ids` [B, S] (int32 / int64, AR order, 0-based inside the window, unit column stride) -- include/selftok_hip_ext.h
    states the arithmetic.  Each side takes its own unconditional logits (the shape, dtype and strides of its conditional ones) and scale.  `ctr` [B, 2] is
    the sampler's (ticket, step); row (b, s) uses the counter (ticket, step + s).  `n_draft`: None (every sequence drafted S ids) or B HOST integers in
    [0, S] (checked on the host; copied to the device here without a synchronisation, or pass the copy yourself as `n_draft_dev` int32 [B]).
    The verdicts are committed into the sampler's `ids` (int32 / int64), `logprob` (fp32) and `n_kept` (int32) [B, K] matrices at tokenizer positions
    K - 1 - (step + j), and ctr[:, 1] advances by n_emit.  -> VerifyOut: per row [B, S + 1] accept uint8, repl_id int32, n_kept int32, mass int64 [B, S + 1, 4]
    holding the uint64 (P, D, p_x, d_x), logprob_x and logprob_repl fp32; per sequence n_accept and n_emit int32 [B]; foreign and bad 32-bit [1],
    accumulating.  Preallocated outputs are taken as given.  No synchronisation, nothing read back."""
    what = "token_verify"
    _need_cuda(target_logits, draft_logits, draft_ids, ctr, ids, logprob, n_kept, target_uncond, draft_uncond, n_draft_dev, accept, repl_id, row_n_kept, mass,
               logprob_x, logprob_repl, n_accept, n_emit, foreign, bad)
    if target_logits.dim() != 3 or target_logits.shape[1] < 1:
        raise _lib.SelftokHipError(f"{what}: `target_logits` must be [B, S + 1, V], got {tuple(target_logits.shape)}")
    B, S = int(target_logits.shape[0]), int(target_logits.shape[1]) - 1
    V, t_seq, t_row = _spec_rows(what, "target_logits", target_logits, B, S + 1)
    if C is None:
        C = V - int(offset)
    C, offset = int(C), int(offset)
    if offset < 0 or C < 1 or offset + C > V:
        raise _lib.SelftokHipError(f"{what}: the window [{offset}, {offset} + {C}) does not lie inside a target row of {V} codes")
    d_seq = d_row = id_stride = 0
    if S > 0:
        if draft_logits is None or draft_ids is None:
            raise _lib.SelftokHipError(f"{what}: {S + 1} target rows per sequence need draft_logits [B, {S}, V] and draft_ids [B, {S}]")
        Vd, d_seq, d_row = _spec_rows(what, "draft_logits", draft_logits, B, S)
        if offset + C > Vd:
            raise _lib.SelftokHipError(f"{what}: the window [{offset}, {offset} + {C}) does not lie inside a draft row of {Vd} codes")
        if draft_ids.dtype not in (torch.int32, torch.int64) or tuple(draft_ids.shape) != (B, S) or draft_ids.stride(1) != 1:
            raise _lib.SelftokHipError(f"{what}: `draft_ids` must be int32 or int64 [{B}, {S}] with unit column stride, got {draft_ids.dtype} {tuple(draft_ids.shape)}")
        id_stride = int(draft_ids.stride(0)) if B > 1 else S
    else:
        draft_logits = draft_ids = draft_uncond = None
    for un, lg, name in ((target_uncond, target_logits, "target_uncond"), (draft_uncond, draft_logits, "draft_uncond")):
        if un is not None and (un.dtype != lg.dtype or un.shape != lg.shape or                      # the stride of a dimension of one element addresses nothing
                               any(n > 1 and a != b for n, a, b in zip(lg.shape, un.stride(), lg.stride()))):
            raise _lib.SelftokHipError(f"{what}: `{name}` must have the dtype, shape and strides of its conditional logits")
    if ctr.dtype not in (torch.int32, torch.uint32) or tuple(ctr.shape) != (B, 2) or not ctr.is_contiguous():
        raise _lib.SelftokHipError(f"{what}: `ctr` must be a contiguous 32-bit integer tensor [{B}, 2], got {ctr.dtype} {tuple(ctr.shape)}")
    if ids.dtype not in (torch.int32, torch.int64) or ids.dim() != 2 or ids.shape[0] != B or ids.shape[1] < 1 or ids.stride(1) != 1:
        raise _lib.SelftokHipError(f"{what}: `ids` must be int32 or int64 [{B}, K] with unit column stride, got {ids.dtype} {tuple(ids.shape)}")
    K = int(ids.shape[1])
    for t, dt, name in ((logprob, torch.float32, "logprob"), (n_kept, torch.int32, "n_kept")):
        if t.dtype != dt or tuple(t.shape) != (B, K) or t.stride(1) != 1:
            raise _lib.SelftokHipError(f"{what}: `{name}` must be {str(dt).replace('torch.', '')} [{B}, {K}] with unit column stride, got {t.dtype} {tuple(t.shape)}")
    dev = target_logits.device
    nd_host = None
    if n_draft is not None:
        nd_host = np.ascontiguousarray(np.asarray(n_draft, dtype=np.int64).reshape(-1).astype(np.int32))
        if nd_host.shape != (B,):
            raise _lib.SelftokHipError(f"{what}: `n_draft` must hold {B} host integers, got {nd_host.shape}")
        if n_draft_dev is None:
            n_draft_dev = torch.from_numpy(nd_host).to(dev, non_blocking=True)
        if n_draft_dev.dtype != torch.int32 or tuple(n_draft_dev.shape) != (B,) or not n_draft_dev.is_contiguous():
            raise _lib.SelftokHipError(f"{what}: `n_draft_dev` must be a contiguous int32 tensor [{B}]")
    elif n_draft_dev is not None:
        raise _lib.SelftokHipError(f"{what}: `n_draft_dev` goes with the host counts `n_draft` it is a copy of")
    R = (B, S + 1)
    accept = _out(what, accept, torch.uint8, R, dev, "accept")
    repl_id = _out(what, repl_id, torch.int32, R, dev, "repl_id")
    row_n_kept = _out(what, row_n_kept, torch.int32, R, dev, "row_n_kept")
    mass = _out(what, mass, torch.int64, R + (4,), dev, "mass")
    logprob_x = _out(what, logprob_x, torch.float32, R, dev, "logprob_x")
    logprob_repl = _out(what, logprob_repl, torch.float32, R, dev, "logprob_repl")
    n_accept = _out(what, n_accept, torch.int32, (B,), dev, "n_accept")
    n_emit = _out(what, n_emit, torch.int32, (B,), dev, "n_emit")
    if foreign is None:
        foreign = torch.zeros(1, dtype=torch.int32, device=dev)
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    _token_u32(what, "foreign", foreign, (1,))
    _token_u32(what, "bad", bad, (1,))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    rs = lambda t: int(t.stride(0)) if B > 1 else K
    _lib.check(_lib.load().selftok_verify_draft(
        _p(target_logits), _p(target_uncond), _SAMPLE_DTYPES[target_logits.dtype], t_seq, t_row, _p(draft_logits), _p(draft_uncond),
        _SAMPLE_DTYPES[draft_logits.dtype] if S > 0 else 0, d_seq, d_row, _p(draft_ids), draft_ids.element_size() if S > 0 else 8, id_stride,
        None if nd_host is None else nd_host.ctypes.data, _p(n_draft_dev), B, S, C, offset, float(cfg_scale), float(draft_cfg_scale), float(temperature), int(top_k),
        float(top_p), seed & 0xFFFFFFFF, seed >> 32, _p(ctr), _p(accept), _p(repl_id), _p(row_n_kept), _p(mass), _p(logprob_x), _p(logprob_repl), _p(ids),
        ids.element_size(), rs(ids), K, _p(logprob), rs(logprob), _p(n_kept), rs(n_kept), _p(n_accept), _p(n_emit), _p(foreign), _p(bad), _stream()),
        "selftok_verify_draft")
    return VerifyOut(accept, repl_id, row_n_kept, mass, logprob_x, logprob_repl, n_accept, n_emit, foreign, bad)


# ----------------------------------------------------------------------------------------------
# token scorer (csrc/token_score.hip): AR logits and KNOWN ids -> log-probability, rank, first code, entropy per row
# ----------------------------------------------------------------------------------------------
def _logit_rows(what: str, logits: torch.Tensor, C, offset, name: str = "logits"):
    """the row layout of one tensor of logits, [R, V] or [B, S, V] flattened to rows without a copy, and its window -> (rows_shape, R, V, C, offset, row_stride)"""
    if logits.dtype not in _SAMPLE_DTYPES or logits.dim() not in (2, 3):
        raise _lib.SelftokHipError(f"{what}: `{name}` must be fp32 or bf16 [R, V] or [B, S, V], got {logits.dtype} {tuple(logits.shape)}")
    V = logits.shape[-1]
    rows_shape = tuple(logits.shape[:-1])
    R = 1
    for n in rows_shape:
        R *= int(n)
    if R >= 1 << 31:
        raise _lib.SelftokHipError(f"{what}: {R} rows: need fewer than 2^31")
    if C is None:
        C = V - int(offset)
    C, offset = int(C), int(offset)
    if offset < 0 or C < 1 or offset + C > V:
        raise _lib.SelftokHipError(f"{what}: the window [{offset}, {offset} + {C}) does not lie inside a row of {V} codes")
    if V and logits.stride(-1) != 1:
        raise _lib.SelftokHipError(f"{what}: `{name}` rows must have unit element stride, got strides {logits.stride()}")
    if logits.dim() == 3 and R > 1 and logits.shape[0] > 1 and logits.shape[1] > 1 and logits.stride(0) != logits.shape[1] * logits.stride(1):
        raise _lib.SelftokHipError(f"{what}: [B, S, V] `{name}` must flatten to rows without a copy (stride(0) == S * stride(1)), got strides {logits.stride()}")
    if logits.dim() == 2 or logits.shape[1] > 1:
        rs = logits.stride(-2)
    else:
        rs = logits.stride(0)
    if R <= 1:
        rs = max(V, rs)
    return rows_shape, R, V, C, offset, rs


def _token_rows(what: str, logits: torch.Tensor, ids: torch.Tensor, C, offset, rows_per_seq, reverse_steps):
    """the row layout one scorer / loss call hands to its kernel: `logits` [R, V] or [B, S, V] flattened to rows without a copy, the window, and the targets'
    addressing taken from the strides of `ids` -> (rows_shape, R, V, C, offset, row_stride, S, id_seq_stride, id_step_stride, ids_ptr)"""
    rows_shape, R, V, C, offset, rs = _logit_rows(what, logits, C, offset)
    if ids.dtype not in (torch.int32, torch.int64) or ids.dim() not in (1, 2) or ids.numel() != R or (logits.dim() == 3 and ids.dim() == 2 and tuple(ids.shape) != rows_shape):
        raise _lib.SelftokHipError(f"{what}: `ids` must be int32 or int64, [R] or [B, S] with one id per row of `logits` ({R}), got {ids.dtype} {tuple(ids.shape)}")
    if ids.dim() == 2:
        S, seq_stride, step_stride = int(ids.shape[1]), int(ids.stride(0)), int(ids.stride(1))
    else:                                                           # [R] ids: row r scores element r, however the rows are cut into sequences
        S = int(rows_shape[1]) if logits.dim() == 3 else (int(rows_per_seq) if rows_per_seq else max(R, 1))
        step_stride = int(ids.stride(0))
        seq_stride = S * step_stride
    if R and (S < 1 or R % S or (rows_per_seq is not None and int(rows_per_seq) != S)):
        raise _lib.SelftokHipError(f"{what}: rows_per_seq {rows_per_seq} does not go with {R} rows and ids {tuple(ids.shape)}")
    ids_ptr = _p(ids)
    if reverse_steps:
        ids_ptr += (S - 1) * step_stride * ids.element_size()
        step_stride = -step_stride
    return rows_shape, R, V, C, offset, rs, S, seq_stride, step_stride, ids_ptr


def token_score(logits: torch.Tensor, ids: torch.Tensor, *, uncond_logits: Optional[torch.Tensor] = None, C: Optional[int] = None, offset: int = 0,
                cfg_scale: float = 1.0, temperature: float = 1.0, rows_per_seq: Optional[int] = None, reverse_steps: bool = False,
                logprob: Optional[torch.Tensor] = None, mass: Optional[torch.Tensor] = None, rank: Optional[torch.Tensor] = None,
                top_id: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None,
                ignored: Optional[torch.Tensor] = None):
    """Teacher-forced scores of known ids: `logits` [R, V] or [B, S, V] (fp32 or bf16, unit code stride, row stride a multiple of 4 codes; [B, S, V] must
    flatten to rows without a copy) over the window [offset, offset + C) (default: the rest of the row), with the sampler's guidance (`uncond_logits`,
    `cfg_scale`) and `temperature` > 0 -- include/selftok_hip_ext.h states the arithmetic, the sampler's own.  `ids`: int32 or int64, [R] or [B, S] (R = B * S),
    ANY strided view (a column range of a wider [B, K] matrix, every other column, an expanded row): the two id strides are taken from it and nothing is
    copied.  `reverse_steps` reads the steps of a sequence backwards -- row (b, s) scores ids[b, S - 1 - s] -- which is how AR-ordered logits meet
    tokenizer-ordered ids (torch has no negative strides; the kernel has).  `rows_per_seq`, if given, must be the S so derived.  A target is 0-based inside
    the window; a target < 0 is IGNORED (padding), a target >= C makes the row BAD, as does a NaN / +inf / all -inf row.
    -> (logprob fp32, mass int64 [..., 2] holding the uint64 (Q_total, q_t), rank int32, top_id int32, entropy fp32, bad 32-bit [1], ignored 32-bit [1]), the
    row outputs shaped [R] or [B, S]; bad and ignored ACCUMULATE.  Preallocated outputs are taken as given.  No synchronisation, nothing read back."""
    _need_cuda(logits, uncond_logits, ids, logprob, mass, rank, top_id, entropy, bad, ignored)
    what = "token_score"
    rows_shape, R, V, C, offset, rs, S, seq_stride, step_stride, ids_ptr = _token_rows(what, logits, ids, C, offset, rows_per_seq, reverse_steps)
    if uncond_logits is not None and (uncond_logits.dtype != logits.dtype or uncond_logits.shape != logits.shape or (R > 1 and uncond_logits.stride() != logits.stride())
                                      or uncond_logits.stride(-1) != 1):
        raise _lib.SelftokHipError(f"{what}: `uncond_logits` must have the dtype, shape and strides of `logits`")
    dev = logits.device
    logprob = _out(what, logprob, torch.float32, rows_shape, dev, "logprob")
    mass = _out(what, mass, torch.int64, rows_shape + (2,), dev, "mass")
    rank = _out(what, rank, torch.int32, rows_shape, dev, "rank")
    top_id = _out(what, top_id, torch.int32, rows_shape, dev, "top_id")
    entropy = _out(what, entropy, torch.float32, rows_shape, dev, "entropy")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if ignored is None:
        ignored = torch.zeros(1, dtype=torch.int32, device=dev)
    _token_u32(what, "bad", bad, (1,))
    _token_u32(what, "ignored", ignored, (1,))
    if not temperature > 0.0:
        raise _lib.SelftokHipError(f"{what}: need a temperature > 0 (a greedy distribution has no log-probabilities), got {temperature}")
    if R:
        _lib.check(_lib.load().selftok_score_tokens(_p(logits), _p(uncond_logits), _SAMPLE_DTYPES[logits.dtype], R, C, rs, offset, float(cfg_scale), float(temperature),
                                                    ids_ptr, ids.element_size(), S, seq_stride, step_stride, _p(logprob), _p(mass), _p(rank), _p(top_id), _p(entropy),
                                                    _p(bad), _p(ignored), _stream()), "selftok_score_tokens")
    return logprob, mass, rank, top_id, entropy, bad, ignored


# ----------------------------------------------------------------------------------------------
# token loss (csrc/token_xent.hip): AR logits and KNOWN ids -> cross-entropy, log-sum-exp and the gradient row
# ----------------------------------------------------------------------------------------------
def token_xent(logits: torch.Tensor, ids: torch.Tensor, *, C: Optional[int] = None, offset: int = 0, z_coef: float = 0.0, row_scale: Optional[torch.Tensor] = None,
               grad: Optional[torch.Tensor] = None, inplace: bool = False, reverse_steps: bool = False, rows_per_seq: Optional[int] = None,
               nll: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None, ignored: Optional[torch.Tensor] = None):
    """Cross-entropy of known ids and its gradient in one launch: `logits` and `ids` exactly as `token_score` takes them (shapes, strides, window,
    `reverse_steps`), at temperature 1 without guidance -- include/selftok_hip_ext.h states the arithmetic.  Row r gets nll = -log softmax(l)[t], lse = log sum
    exp(l) and the gradient row `a * softmax(l) - g * onehot(t)` of g * (nll + z_coef * lse^2), g = row_scale[r] (fp32, one per row, shaped as the rows; None: 1)
    and a = g * (1 + 2 * z_coef * lse), over all V columns of the row: zero outside the window.  `grad`: a tensor of the logits' shape and dtype with unit code
    stride and rows that flatten as the logits' do (default: a new contiguous one); inplace=True writes the gradient OVER `logits` instead, the same bits, and
    allocates nothing of that size -- the logits are gone afterwards.  An IGNORED row (target < 0) has nll 0 and a zero gradient row; a BAD row (NaN / +inf /
    all -inf, or a target >= C) has nll and lse NaN and a zero gradient row.
    -> (nll fp32, lse fp32, grad, bad 32-bit [1], ignored 32-bit [1]); nll and lse shaped [R] or [B, S]; bad and ignored ACCUMULATE.  No synchronisation,
    nothing read back."""
    _need_cuda(logits, ids, row_scale, grad, nll, lse, bad, ignored)
    what = "token_xent"
    rows_shape, R, V, C, offset, rs, S, seq_stride, step_stride, ids_ptr = _token_rows(what, logits, ids, C, offset, rows_per_seq, reverse_steps)
    z_coef = float(z_coef)
    if not (z_coef >= 0.0 and z_coef != float("inf")):
        raise _lib.SelftokHipError(f"{what}: need a finite z_coef >= 0, got {z_coef}")
    if inplace:
        if grad is not None and grad is not logits:
            raise _lib.SelftokHipError(f"{what}: inplace=True writes the gradient over `logits`: pass no `grad`")
        grad, gs = logits, rs
    else:
        if grad is None:
            grad = torch.empty(tuple(logits.shape), dtype=logits.dtype, device=logits.device)
        if grad.dtype != logits.dtype or grad.shape != logits.shape or (V and grad.stride(-1) != 1) or \
                (grad.dim() == 3 and R > 1 and grad.shape[0] > 1 and grad.shape[1] > 1 and grad.stride(0) != grad.shape[1] * grad.stride(1)):
            raise _lib.SelftokHipError(f"{what}: `grad` must have the dtype and shape of `logits`, unit code stride and rows that flatten without a copy, got "
                                       f"{grad.dtype} {tuple(grad.shape)} strides {grad.stride()}")
        gs = grad.stride(-2) if (grad.dim() == 2 or grad.shape[1] > 1) else grad.stride(0)
        if R <= 1:
            gs = max(V, gs)
    if row_scale is not None and (row_scale.dtype != torch.float32 or row_scale.numel() != R or not row_scale.is_contiguous()):
        raise _lib.SelftokHipError(f"{what}: `row_scale` must be a contiguous fp32 tensor with one element per row ({R}), got {row_scale.dtype} {tuple(row_scale.shape)}")
    dev = logits.device
    nll = _out(what, nll, torch.float32, rows_shape, dev, "nll")
    lse = _out(what, lse, torch.float32, rows_shape, dev, "lse")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if ignored is None:
        ignored = torch.zeros(1, dtype=torch.int32, device=dev)
    _token_u32(what, "bad", bad, (1,))
    _token_u32(what, "ignored", ignored, (1,))
    if R:
        _lib.check(_lib.load().selftok_xent_rows(_p(logits), _SAMPLE_DTYPES[logits.dtype], R, C, rs, offset, ids_ptr, ids.element_size(), S, seq_stride, step_stride, V,
                                                 _p(row_scale), z_coef, _p(nll), _p(lse), _p(grad), gs, _p(bad), _p(ignored), _stream()), "selftok_xent_rows")
    return nll, lse, grad, bad, ignored


# ----------------------------------------------------------------------------------------------
# token policy loss (csrc/token_policy.hip): AR logits, SAMPLED ids, their roll-out log-probabilities and advantages -> PPO / GRPO surrogate and gradient
# ----------------------------------------------------------------------------------------------
PolicyOut = collections.namedtuple("PolicyOut", "logprob lse ratio kl entropy coef flags grad bad ignored")


def _policy_row_operand(what: str, name: str, t, R: int):
    if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.numel() != R or not t.is_contiguous()):
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise _lib.SelftokHipError(f"{what}: `{name}` must be a contiguous fp32 tensor with one element per row ({R}), got {got}")


def token_policy(logits: torch.Tensor, ids: torch.Tensor, old_logprob: torch.Tensor, advantage: torch.Tensor, *, ref_logprob: Optional[torch.Tensor] = None,
                 clip=(0.2, 0.2), kl_coef: float = 0.0, ent_coef: float = 0.0, C: Optional[int] = None, offset: int = 0, row_scale: Optional[torch.Tensor] = None,
                 grad: Optional[torch.Tensor] = None, inplace: bool = False, want_grad: bool = True, reverse_steps: bool = False, rows_per_seq: Optional[int] = None,
                 want_entropy: Optional[bool] = None, logprob: Optional[torch.Tensor] = None, lse: Optional[torch.Tensor] = None, ratio: Optional[torch.Tensor] = None,
                 kl: Optional[torch.Tensor] = None, entropy: Optional[torch.Tensor] = None, coef: Optional[torch.Tensor] = None, flags: Optional[torch.Tensor] = None,
                 bad: Optional[torch.Tensor] = None, ignored: Optional[torch.Tensor] = None):
    """The clipped PPO / GRPO surrogate on SAMPLED ids, the k3 KL estimate to a frozen reference, the entropy and the gradient row of
    g * (-surrogate + kl_coef * kl - ent_coef * entropy) in one launch: `logits` and `ids` exactly as `token_xent` takes them (shapes, strides, window,
    `reverse_steps`), at temperature 1 without guidance -- include/selftok_hip_ext.h states the arithmetic.  `old_logprob`, `advantage` and `ref_logprob`
    (optional): contiguous fp32, one per row IN ROW ORDER.  clip = (lo, hi): the ratio is held to [1 - lo, 1 + hi] on the side the advantage pushes it; a row
    whose ratio left the range that way is CLIPPED (flags bit 0: above, bit 1: below) and its policy gradient is zero.  kl_coef != 0 needs `ref_logprob`.
    `row_scale`, `grad`, inplace=True as in `token_xent`; want_grad=False writes no gradient at all and returns None for it (metrics only).  The entropy is
    computed when ent_coef != 0, when an `entropy` tensor is passed or when want_entropy=True (default: only then; otherwise None is returned for it).
    An IGNORED row (target < 0) has +0 outputs (but its lse) and a zero gradient row; a BAD row (the loss's kinds, or a NaN / infinite advantage, a NaN / +inf
    old or reference log-probability, or -inf against -inf) has NaN outputs and a zero gradient row.
    -> PolicyOut(logprob, lse, ratio, kl, entropy or None, coef -- fp32 -- flags uint8, shaped [R] or [B, S]; grad or None; bad, ignored 32-bit [1],
    ACCUMULATING).  No synchronisation, nothing read back."""
    _need_cuda(logits, ids, old_logprob, advantage, ref_logprob, row_scale, grad, logprob, lse, ratio, kl, entropy, coef, flags, bad, ignored)
    what = "token_policy"
    rows_shape, R, V, C, offset, rs, S, seq_stride, step_stride, ids_ptr = _token_rows(what, logits, ids, C, offset, rows_per_seq, reverse_steps)
    try:
        clip_lo, clip_hi = (float(clip), float(clip)) if isinstance(clip, (int, float)) else (float(clip[0]), float(clip[1]))
    except (TypeError, IndexError, ValueError):
        raise _lib.SelftokHipError(f"{what}: `clip` must be a number or a pair (lo, hi), got {clip!r}")
    kl_coef, ent_coef = float(kl_coef), float(ent_coef)
    inf = float("inf")
    if not (0.0 <= clip_lo < 1.0 and 0.0 <= clip_hi < inf):
        raise _lib.SelftokHipError(f"{what}: need a clip range with 0 <= lo < 1 and a finite hi >= 0, got ({clip_lo}, {clip_hi})")
    if not (0.0 <= kl_coef < inf and 0.0 <= ent_coef < inf):
        raise _lib.SelftokHipError(f"{what}: need a finite kl_coef >= 0 and a finite ent_coef >= 0, got {kl_coef} and {ent_coef}")
    if kl_coef != 0.0 and ref_logprob is None:
        raise _lib.SelftokHipError(f"{what}: kl_coef != 0 needs `ref_logprob`")
    gs = 0
    if not want_grad:
        if inplace or grad is not None:
            raise _lib.SelftokHipError(f"{what}: want_grad=False writes no gradient: pass neither `grad` nor inplace=True")
    elif inplace:
        if grad is not None and grad is not logits:
            raise _lib.SelftokHipError(f"{what}: inplace=True writes the gradient over `logits`: pass no `grad`")
        grad, gs = logits, rs
    else:
        if grad is None:
            grad = torch.empty(tuple(logits.shape), dtype=logits.dtype, device=logits.device)
        if grad.dtype != logits.dtype or grad.shape != logits.shape or (V and grad.stride(-1) != 1) or \
                (grad.dim() == 3 and R > 1 and grad.shape[0] > 1 and grad.shape[1] > 1 and grad.stride(0) != grad.shape[1] * grad.stride(1)):
            raise _lib.SelftokHipError(f"{what}: `grad` must have the dtype and shape of `logits`, unit code stride and rows that flatten without a copy, got "
                                       f"{grad.dtype} {tuple(grad.shape)} strides {grad.stride()}")
        gs = grad.stride(-2) if (grad.dim() == 2 or grad.shape[1] > 1) else grad.stride(0)
        if R <= 1:
            gs = max(V, gs)
    for name, t in (("old_logprob", old_logprob), ("advantage", advantage), ("ref_logprob", ref_logprob), ("row_scale", row_scale)):
        if t is None and name in ("old_logprob", "advantage"):
            raise _lib.SelftokHipError(f"{what}: `{name}` is required")
        _policy_row_operand(what, name, t, R)
    dev = logits.device
    logprob = _out(what, logprob, torch.float32, rows_shape, dev, "logprob")
    lse = _out(what, lse, torch.float32, rows_shape, dev, "lse")
    ratio = _out(what, ratio, torch.float32, rows_shape, dev, "ratio")
    kl = _out(what, kl, torch.float32, rows_shape, dev, "kl")
    coef = _out(what, coef, torch.float32, rows_shape, dev, "coef")
    flags = _out(what, flags, torch.uint8, rows_shape, dev, "flags")
    if entropy is not None or want_entropy or (want_entropy is None and ent_coef != 0.0):
        entropy = _out(what, entropy, torch.float32, rows_shape, dev, "entropy")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if ignored is None:
        ignored = torch.zeros(1, dtype=torch.int32, device=dev)
    _token_u32(what, "bad", bad, (1,))
    _token_u32(what, "ignored", ignored, (1,))
    if R:
        _lib.check(_lib.load().selftok_policy_rows(_p(logits), _SAMPLE_DTYPES[logits.dtype], R, C, rs, offset, ids_ptr, ids.element_size(), S, seq_stride, step_stride, V,
                                                   _p(row_scale), _p(old_logprob), _p(advantage), _p(ref_logprob), clip_lo, clip_hi, kl_coef, ent_coef, _p(logprob),
                                                   _p(lse), _p(ratio), _p(kl), _p(entropy), _p(coef), _p(flags), _p(grad), gs, _p(bad), _p(ignored), _stream()),
                   "selftok_policy_rows")
    return PolicyOut(logprob, lse, ratio, kl, entropy, coef, flags, grad, bad, ignored)


# ----------------------------------------------------------------------------------------------
# token distillation (csrc/token_distill.hip): student and teacher logits -> KL, soft cross-entropy, teacher entropy, student lse and the gradient row
# ----------------------------------------------------------------------------------------------
def _row_stride_of(t: torch.Tensor, R: int, V: int) -> int:
    rs = t.stride(-2) if (t.dim() == 2 or t.shape[1] > 1) else t.stride(0)
    return max(V, rs) if R <= 1 else rs


def token_distill(student: torch.Tensor, teacher: torch.Tensor, *, teacher_uncond: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, C: Optional[int] = None,
                  offset: int = 0, row_scale: Optional[torch.Tensor] = None, row_mask: Optional[torch.Tensor] = None, grad: Optional[torch.Tensor] = None,
                  inplace: bool = False, want_grad: bool = True, kl: Optional[torch.Tensor] = None, ce: Optional[torch.Tensor] = None,
                  h_teacher: Optional[torch.Tensor] = None, lse_student: Optional[torch.Tensor] = None, bad: Optional[torch.Tensor] = None,
                  ignored: Optional[torch.Tensor] = None):
    """KL(teacher || student) per row and its gradient in one launch: `student` exactly as `token_xent` takes its logits ([R, V] or [B, S, V], fp32 or bf16,
    window [offset, offset + C)), `teacher` of the same SHAPE with its own dtype (fp32 or bf16) and its own row stride, at temperature 1 on both sides --
    include/selftok_hip_ext.h states the arithmetic.  `teacher_uncond` (the teacher's shape, dtype and strides) makes the teacher the guided distribution of
    the sampler, `lu + cfg_scale * (lc - lu)` with lc = `teacher`.  Row r gets kl, ce = -sum pA log pB, h_teacher = -sum pA log pA, lse_student, and the
    gradient row g * (softmax(student) - softmax(teacher)), g = row_scale[r] (fp32, one per row; None: 1), over all V columns: zero outside the window.
    `row_mask`: uint8 or bool, one per row; a 0 makes the row IGNORED (nothing of it is read, outputs +0, a zero gradient row).  `grad` / inplace=True as in
    `token_xent` (in place the gradient lands over `student`); want_grad=False writes no gradient at all and returns None for it (metrics only).  A BAD row
    (NaN / +inf in either window or in the guided teacher, or a window with nothing above -inf) has NaN outputs and a zero gradient row; a row whose student
    lies 32768 or more (or at -inf) below its maximum on a code the teacher gives mass has ce = kl = +inf and is not bad.
    -> (kl, ce, h_teacher, lse_student fp32 shaped [R] or [B, S], grad or None, bad 32-bit [1], ignored 32-bit [1]); bad and ignored ACCUMULATE.  No
    synchronisation, nothing read back."""
    what = "token_distill"
    rows_shape, R, V, C, offset, rs = _logit_rows(what, student, C, offset, "student")
    if teacher.dtype not in _SAMPLE_DTYPES or teacher.shape != student.shape:
        raise _lib.SelftokHipError(f"{what}: `teacher` must be fp32 or bf16 of the student's shape {tuple(student.shape)}, got {teacher.dtype} {tuple(teacher.shape)}")
    ts = _logit_rows(what, teacher, C, offset, "teacher")[5]
    if teacher_uncond is not None:
        if teacher_uncond.dtype != teacher.dtype or teacher_uncond.shape != teacher.shape or (R > 1 and teacher_uncond.stride() != teacher.stride()) or \
                (V and teacher_uncond.stride(-1) != 1):
            raise _lib.SelftokHipError(f"{what}: `teacher_uncond` must have the dtype, shape and strides of `teacher` ({teacher.dtype} {tuple(teacher.shape)}), got "
                                       f"{teacher_uncond.dtype} {tuple(teacher_uncond.shape)}")
        cfg_scale = float(cfg_scale)
        if cfg_scale != cfg_scale or cfg_scale in (float("inf"), -float("inf")):
            raise _lib.SelftokHipError(f"{what}: need a finite cfg_scale, got {cfg_scale}")
    _need_cuda(student, teacher, teacher_uncond, row_scale, row_mask, grad, kl, ce, h_teacher, lse_student, bad, ignored)
    gs = 0
    if not want_grad:
        if inplace or grad is not None:
            raise _lib.SelftokHipError(f"{what}: want_grad=False writes no gradient: pass neither `grad` nor inplace=True")
    elif inplace:
        if grad is not None and grad is not student:
            raise _lib.SelftokHipError(f"{what}: inplace=True writes the gradient over `student`: pass no `grad`")
        grad, gs = student, rs
    else:
        if grad is None:
            grad = torch.empty(tuple(student.shape), dtype=student.dtype, device=student.device)
        if grad.dtype != student.dtype or grad.shape != student.shape or (V and grad.stride(-1) != 1) or \
                (grad.dim() == 3 and R > 1 and grad.shape[0] > 1 and grad.shape[1] > 1 and grad.stride(0) != grad.shape[1] * grad.stride(1)):
            raise _lib.SelftokHipError(f"{what}: `grad` must have the dtype and shape of `student`, unit code stride and rows that flatten without a copy, got "
                                       f"{grad.dtype} {tuple(grad.shape)} strides {grad.stride()}")
        gs = _row_stride_of(grad, R, V)
    if row_scale is not None and (row_scale.dtype != torch.float32 or row_scale.numel() != R or not row_scale.is_contiguous()):
        raise _lib.SelftokHipError(f"{what}: `row_scale` must be a contiguous fp32 tensor with one element per row ({R}), got {row_scale.dtype} {tuple(row_scale.shape)}")
    if row_mask is not None and (row_mask.dtype not in (torch.uint8, torch.bool) or row_mask.numel() != R or not row_mask.is_contiguous()):
        raise _lib.SelftokHipError(f"{what}: `row_mask` must be a contiguous uint8 or bool tensor with one element per row ({R}), got {row_mask.dtype} {tuple(row_mask.shape)}")
    dev = student.device
    kl = _out(what, kl, torch.float32, rows_shape, dev, "kl")
    ce = _out(what, ce, torch.float32, rows_shape, dev, "ce")
    h_teacher = _out(what, h_teacher, torch.float32, rows_shape, dev, "h_teacher")
    lse_student = _out(what, lse_student, torch.float32, rows_shape, dev, "lse_student")
    if bad is None:
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
    if ignored is None:
        ignored = torch.zeros(1, dtype=torch.int32, device=dev)
    _token_u32(what, "bad", bad, (1,))
    _token_u32(what, "ignored", ignored, (1,))
    if R:
        _lib.check(_lib.load().selftok_distill_rows(_p(student), _SAMPLE_DTYPES[student.dtype], _p(teacher), _p(teacher_uncond), _SAMPLE_DTYPES[teacher.dtype], R, C, rs,
                                                    ts, offset, float(cfg_scale), V, _p(row_scale), _p(row_mask), _p(kl), _p(ce), _p(h_teacher), _p(lse_student),
                                                    _p(grad), gs, _p(bad), _p(ignored), _stream()), "selftok_distill_rows")
    return kl, ce, h_teacher, lse_student, grad, bad, ignored
