"""Q-Former 'dual' encoder + VQ on MI355X (host orchestration; compute = hipBLASLt GEMMs + our HIP kernels).

Drop-in counterpart of `model.encoder` in the reference (QformerEncoder, mimogpt/models/selftok/
models_ours.py:204-257, 268-353; DualBlock/DualAttention modules.py:165-327; VectorQuantize eval
vector_quantize_pytorch.py:811-1080) over the reference's checkpoint keys (`encoder.*`).

What differs from the reference on purpose (results identical):
  * the per-block adaLN tables depend only on token positions 1000+8k -> computed once at load
    (the reference recomputes them on every call, modules.py:312-318);
  * LayerNorm / modulate / gate / residual are fused HIP passes (ops.residual_ln_mod), attention never
    concatenates [to_query_kv(x), query_kv] (two-segment kernel), the VQ never materialises the [N,C]
    score / one-hot tensors and skips the perplexity logging (vector_quantize_pytorch.py:561,136,957-975).
"""
from __future__ import annotations

import math
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .modsurface import ModuleSurface
from .schedule import DiTiCont
from .weights import ENC_DEPTH, ENC_HEADS, ENC_HIDDEN, ENC_QDIM, ENC_QHEADS, FREQ_DIM


def sinusoid_host(t: torch.Tensor, dim: int = FREQ_DIM) -> torch.Tensor:
    """timestep_embedding on the HOST with torch-CPU ops, i.e. the reference's own arithmetic
    (models.py:56-74).  Used for input-independent tables (positions, the 50 scheduled timesteps)."""
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    return torch.cat([torch.cos(args), torch.sin(args)], dim=-1)


_POS_TABLE = None


def encoder_pos_embedding(K: int) -> torch.Tensor:
    """sinusoidal embedding of the token positions 1000 + 8 k, k < K, with the bits the REFERENCE produces on an AVX-512 Intel host
    (`timestep_embedding`, models.py:56-74: torch.exp / cos / sin = MKL VML there -- closed source, vendor-dispatched, NOT the correctly
    rounded values: the same call returns other bits on this box's host CPU).  Input- and weight-independent, so it ships as data
    (selftoktokenizer_amd/data/encoder_pos_sincos.npy, tools/oracle/gen_pos_table.py); K > 1024 falls back to the host evaluation."""
    global _POS_TABLE
    if _POS_TABLE is None:
        import os
        _POS_TABLE = torch.from_numpy(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "encoder_pos_sincos.npy")))
    if K > _POS_TABLE.shape[0]:
        print(f"[selftok] encoder_pos_embedding: K = {K} exceeds the shipped table ({_POS_TABLE.shape[0]} positions): evaluated on this host's "
              "CPU instead -- token ids may differ from the reference's at near-ties")
        return sinusoid_host(torch.from_numpy(DiTiCont.get_position(np.arange(K))).to(torch.int64))
    return _POS_TABLE[:K].clone()


class _Quantizer:
    """`model.encoder.quantizer` surface used by the pipeline: get_output_from_indices."""

    def __init__(self, enc: "QformerEncoderGPU"):
        self._enc = enc

    @property
    def codebook(self):
        return self._enc.codebook

    def get_output_from_indices(self, indices: torch.Tensor) -> torch.Tensor:
        return ops.code_gather_ln(indices, self._enc.codebook)   # project_out is Identity (dim 16 == 16)


class QformerEncoderGPU(ModuleSurface):
    _sd_prefix = "encoder."
    def __init__(self, sd: Dict[str, torch.Tensor], device, K: int, mode: str = "exact", pre_norm: bool = False):
        """`mode`: 'exact' (default) -- every reduction / transcendental in the summation order torch-CPU executes for the reference
        (csrc/encoder_exact.hip): the pre-quantizer features, and with them the token ids, are those of the reference's runs at 8 <= B <= 64
        images per call bit for bit, and do not depend on the batch size HERE (every kernel is row independent; the reference's own B = 1 run
        takes another MKL path, which this mode does not follow: DESIGN 15.2); 'fast' -- hipBLASLt GEMMs + the rounds 1-3 fused kernels (features within 6e-5, ids equal except
        at reference near-ties, ~2x faster encoder).  `pre_norm`: encoder_config.pre_norm (models_ours.py:219-220): final_layer_norm on the query tokens
        before the quantizer (ATen's LayerNorm arithmetic in both modes)."""
        self.pre_norm = bool(pre_norm)
        g = lambda k: sd[k].to(device=device, dtype=torch.float32).contiguous()
        if mode not in ("exact", "fast"):
            raise ValueError(f"encoder mode {mode!r}: expected 'exact' or 'fast'")
        self.device, self.K, self.mode = device, K, mode
        self.post_norm = True
        self.w = {k: g(k) for k in sd if k.startswith("encoder.") and "_codebook" not in k and "quantizer.c" not in k and "quantizer.s" not in k}
        self.codebook = g("encoder.quantizer._codebook.embed")[0].contiguous()
        self.codebook_packed = ops.vq_pack_codebook(self.codebook)
        # patch embed as a GEMM: weight [64,16,2,2] -> [64(in: c*4+p*2+q), 64(out)]
        self.pe_w = self.w["encoder.x_embedder.proj.weight"].reshape(ENC_HIDDEN, -1).t().contiguous()
        self._pos_cache = {}
        # input-independent adaLN tables: Linear(SiLU(t_embedder(1000+8k)))  [K, 6*512] per block
        if mode == "exact":
            pos_emb = encoder_pos_embedding(K).to(device)
        else:
            pos_emb = sinusoid_host(torch.from_numpy(DiTiCont.get_position(np.arange(K))).to(torch.int64)).to(device)
        self.tables = []
        lin = ops.ex_linear if mode == "exact" else F.linear
        silu = (lambda t: ops.ex_unary(t.contiguous(), "silu")) if mode == "exact" else ops.silu
        for i in range(ENC_DEPTH):
            p = f"encoder.blocks.{i}"
            h = lin(pos_emb, self.w[p + ".t_embedder.mlp.0.weight"], self.w[p + ".t_embedder.mlp.0.bias"])
            h = lin(silu(h), self.w[p + ".t_embedder.mlp.2.weight"], self.w[p + ".t_embedder.mlp.2.bias"])
            self.tables.append(lin(silu(h), self.w[p + ".adaLN_modulation.1.weight"], self.w[p + ".adaLN_modulation.1.bias"]).contiguous())
        # exact mode: the PatchEmbed convolution as ONE 64-tap chain in (kh, kw, ic) order = a Linear over the re-ordered patch
        # (oracle/encoder_exact.c); ops.patchify emits (ic, kh, kw)
        self.pe_w_exact = self.w["encoder.x_embedder.proj.weight"].permute(0, 2, 3, 1).reshape(ENC_HIDDEN, -1).contiguous()
        self._pe_perm = torch.arange(64, device=device).reshape(16, 2, 2).permute(1, 2, 0).reshape(-1)
        self.quantizer = _Quantizer(self)

    def _flat_weights(self):
        d = dict(self.w)
        d["encoder.quantizer._codebook.embed"] = self.codebook[None]
        return d

    # ---- helpers -------------------------------------------------------------------------------
    def _pos_bias(self, h: int, w: int) -> torch.Tensor:
        """centre-cropped sin-cos table (cropped_pos_embed, models_ours.py:183-202) + conv bias -> [h*w, 64]"""
        key = (h, w)
        if key not in self._pos_cache:
            pe = self.w["encoder.pos_embed"]
            grid = int(round(math.sqrt(pe.shape[1])))
            top, left = (grid - h) // 2, (grid - w) // 2
            crop = pe.reshape(grid, grid, -1)[top:top + h, left:left + w].reshape(h * w, -1)
            self._pos_cache[key] = (crop + self.w["encoder.x_embedder.proj.bias"]).contiguous()
        return self._pos_cache[key]

    def lin(self, name, x):
        return F.linear(x, self.w[name + ".weight"], self.w[name + ".bias"])

    def final_layer_norm3(self, codes: torch.Tensor) -> torch.Tensor:
        return F.layer_norm(codes, (16,), self.w["encoder.final_layer_norm3.weight"], self.w["encoder.final_layer_norm3.bias"], 1e-6)

    def codes_ln(self, ids: torch.Tensor) -> torch.Tensor:
        """fused codebook[ids] -> final_layer_norm3 (SelftokPipeline.py:236-240).  exact mode: the gather is a copy, the LayerNorm(16) runs in ATen's
        arithmetic (csrc/encoder_exact.hip) -- the fused kernel's own LayerNorm is within 7e-7 of it, which is the decoder's conditioning"""
        if self.mode == "exact":
            flat = ids.reshape(-1).long()
            if flat.numel() and (int(flat.min()) < 0 or int(flat.max()) >= self.codebook.shape[0]):     # the fused kernel path refuses them too
                raise ValueError(f"token ids must lie in [0, {self.codebook.shape[0]}): got [{int(flat.min())}, {int(flat.max())}]")
            codes = self.codebook[flat].reshape(*ids.shape, -1).contiguous()
            return ops.ex_layernorm_mod(codes, gamma=self.w["encoder.final_layer_norm3.weight"], beta=self.w["encoder.final_layer_norm3.bias"])
        return ops.code_gather_ln(ids, self.codebook, self.w["encoder.final_layer_norm3.weight"], self.w["encoder.final_layer_norm3.bias"])

    def get_encoder_mask(self, x, d, single_token=False):
        """arange(K) <= d (models_ours.py:345-353)"""
        ar = torch.arange(self.K, device=d.device)[None, :].expand(x.shape[0], self.K)
        return (ar == d.unsqueeze(1)) if single_token else (ar <= d.unsqueeze(1))

    # ---- forward -------------------------------------------------------------------------------
    def _pos_only(self, h: int, w: int) -> torch.Tensor:
        """centre-cropped sin-cos table WITHOUT the conv bias (exact mode adds the bias inside the Linear, then the table: two roundings) -> [h*w, 64]"""
        key = ("pos", h, w)
        if key not in self._pos_cache:
            pe = self.w["encoder.pos_embed"]
            grid = int(round(math.sqrt(pe.shape[1])))
            top, left = (grid - h) // 2, (grid - w) // 2
            self._pos_cache[key] = pe.reshape(grid, grid, -1)[top:top + h, left:left + w].reshape(h * w, -1).contiguous()
        return self._pos_cache[key]

    def _pre_norm(self, q: torch.Tensor) -> torch.Tensor:
        """`outs = self.final_layer_norm(outs)` (models_ours.py:219-220) when encoder_config.pre_norm"""
        if not self.pre_norm:
            return q
        return ops.ex_layernorm_mod(q, gamma=self.w["encoder.final_layer_norm.weight"], beta=self.w["encoder.final_layer_norm.bias"])

    @torch.no_grad()
    def features_exact(self, x0: torch.Tensor) -> torch.Tensor:
        """`features` with every operation in the order / polynomial torch-CPU executes for the reference (models_ours.py:204-257,
        modules.py:216-327): z equals the reference's pre-quantizer features bit for bit (tests/golden/encode_b64.npz, pipeline_b16.npz)."""
        B, _, Hh, Ww = x0.shape
        H, Q, K = ENC_HIDDEN, ENC_QDIM, self.K
        w = self.w
        lin = lambda name, t, **kw: ops.ex_linear(t, w[name + ".weight"], w[name + ".bias"], **kw)
        patch = ops.patchify(x0)[..., self._pe_perm].contiguous()            # [B, N, 64] in (kh, kw, ic) order
        N = patch.shape[1]
        x = ops.ex_linear(patch, self.pe_w_exact, w["encoder.x_embedder.proj.bias"], res=self._pos_only(Hh // 2, Ww // 2), res_mod=N)
        q = w["encoder.query_tokens"].expand(B, -1, -1).contiguous()
        for i in range(ENC_DEPTH):
            p = f"encoder.blocks.{i}"
            t = self.tables[i]
            xn = ops.ex_layernorm_mod(x)
            qn = ops.ex_layernorm_mod(q, shift=t[:, 0:Q], scale=t[:, Q:2 * Q])
            qkv = lin(p + ".attn.qkv", xn)                          # [B,N,3*64]
            kvx = lin(p + ".attn.to_query_kv", xn)                  # [B,N,2*512]
            qq = lin(p + ".attn.query_linear", qn)                  # [B,K,3*512]
            xa = ops.ex_attention(qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], ENC_HEADS)
            qa = ops.ex_attention(qq[..., :Q], kvx[..., :Q], kvx[..., Q:], ENC_QHEADS, qq[..., Q:2 * Q], qq[..., 2 * Q:])
            x = lin(p + ".attn.proj", xa, res=x)                                            # x + proj(attn)
            h = lin(p + ".mlp.fc1", ops.ex_layernorm_mod(x), gelu=True)
            x = lin(p + ".mlp.fc2", h, res=x)                                               # x + mlp(LN(x))
            q = lin(p + ".attn.query_proj", qa, res=q, gate=t[:, 2 * Q:3 * Q], gate_mod=K)   # q + g1 * proj(attn_q)
            h = lin(p + ".q_mlp.fc1", ops.ex_layernorm_mod(q, shift=t[:, 3 * Q:4 * Q], scale=t[:, 4 * Q:5 * Q]), gelu=True)
            q = lin(p + ".q_mlp.fc2", h, res=q, gate=t[:, 5 * Q:6 * Q], gate_mod=K)          # q + g2 * mlp_q(mod(LN(q)))
        return lin("encoder.quantizer.project_in", self._pre_norm(q))

    @torch.no_grad()
    def features(self, x0: torch.Tensor) -> torch.Tensor:
        """x0 [B,16,h,w] fp32 -> pre-quantizer features z [B,K,16] (incl. quantizer.project_in)"""
        if self.mode == "exact":
            return self.features_exact(x0)
        B, _, Hh, Ww = x0.shape
        H, Q, K = ENC_HIDDEN, ENC_QDIM, self.K
        x = torch.matmul(ops.patchify(x0), self.pe_w)
        ops.add_rows_(x, self._pos_bias(Hh // 2, Ww // 2))
        N = x.shape[1]
        q = self.w["encoder.query_tokens"].expand(B, -1, -1).contiguous()
        tab = self.tables
        _, xn = ops.residual_ln_mod(x)
        _, qn = ops.residual_ln_mod(q, shift=tab[0][:, 0:Q], scale=tab[0][:, Q:2 * Q])
        for i in range(ENC_DEPTH):
            p = f"encoder.blocks.{i}"
            t = tab[i]
            qkv = self.lin(p + ".attn.qkv", xn)                    # [B,N,3*64]  (q|k|v, each 4 heads x 16)
            kvx = self.lin(p + ".attn.to_query_kv", xn)            # [B,N,2*512]
            qq = self.lin(p + ".attn.query_linear", qn)            # [B,K,3*512]
            xa = torch.empty(B, N, H, device=x.device)
            qa = torch.empty(B, K, Q, device=x.device)
            ops.attention(None, (qkv[..., :H], qkv[..., H:2 * H], qkv[..., 2 * H:], xa), ENC_HEADS, H // ENC_HEADS)
            ops.attention((None, kvx[..., :Q], kvx[..., Q:], None), (qq[..., :Q], qq[..., Q:2 * Q], qq[..., 2 * Q:], qa),
                          ENC_QHEADS, Q // ENC_QHEADS)
            # latent stream: x += proj(attn); x += mlp(LN(x))
            x, xn2 = ops.residual_ln_mod(x, y=self.lin(p + ".attn.proj", xa))
            h = ops.linear_gelu(xn2, self.w[p + ".mlp.fc1.weight"], self.w[p + ".mlp.fc1.bias"])
            last = i == ENC_DEPTH - 1
            x, xn = ops.residual_ln_mod(x, y=self.lin(p + ".mlp.fc2", h), want_n=not last)
            # query stream: q += g1*proj(attn); q += g2*mlp(mod(LN(q)))
            q, qn2 = ops.residual_ln_mod(q, y=self.lin(p + ".attn.query_proj", qa), gate=t[:, 2 * Q:3 * Q],
                                         shift=t[:, 3 * Q:4 * Q], scale=t[:, 4 * Q:5 * Q])
            h = ops.linear_gelu(qn2, self.w[p + ".q_mlp.fc1.weight"], self.w[p + ".q_mlp.fc1.bias"])
            m = self.lin(p + ".q_mlp.fc2", h)
            if last:
                q, _ = ops.residual_ln_mod(q, y=m, gate=t[:, 5 * Q:6 * Q], want_n=False)
            else:
                tn = tab[i + 1]
                q, qn = ops.residual_ln_mod(q, y=m, gate=t[:, 5 * Q:6 * Q], shift=tn[:, 0:Q], scale=tn[:, Q:2 * Q])
        return self.lin("encoder.quantizer.project_in", self._pre_norm(q))

    @torch.no_grad()
    def topk(self, x: torch.Tensor, k: int = 2):
        """(extension) x0 -> (ids [B,K,k] int64, scores [B,K,k] fp32): the k best codes of every token and their canonical scores
        (ops.vq_topk) from the same pre-quantizer features `__call__` quantizes; ids[..., 0] are its token ids."""
        return ops.vq_topk(self.features(x), self.codebook_packed, k)

    @torch.no_grad()
    def __call__(self, x=None, hidden_states=None, d=None, kwargs=None):
        """`outs_q, indices = encoder(x_0, d=None)` (models_ours.py:204-251).  With d given, returns the
        7-tuple of the reference (only `attn_mask` is ever consumed, rectified_flow.py:215)."""
        z = self.features(x)
        ids = ops.vq_encode(z, self.codebook_packed, packed=True)          # int64 [B,K]
        outs_q = self.codes_ln(ids)
        if d is None:
            return outs_q, ids
        mask = self.get_encoder_mask(x, d)
        return outs_q * mask[..., None], z, outs_q, mask, 0.0, {}, ids
