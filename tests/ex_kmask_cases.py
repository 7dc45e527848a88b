"""Case tables of tests/test_ex_attention_kmask_gpu.py and tests/test_exact_masks_gpu.py (the exact-order attention with a per-sample
key bit mask), shared with the golden generator (tools/oracle/gen_golden.py, stage `exact_masks`).  tests/test_exact_masks_cpu.py
checks, without a GPU, that these tables hold the patterns they claim and that every case would see one flipped mask bit.

Every input is a function of a name (synth.hash_normalish with a crc32 seed) or of a literal seed, so it regenerates on any host.
The fp64 reference is plain torch: softmax(q k^T scale) v in float64 over the visible key set.  No project code is a reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from selftoktokenizer_amd import synth

DH = 64
SCALE = DH ** -0.5        # 0.125: exact
HASH_SEED = 0x5A5A


# ---------------------------------------------------------------------------------------------------------------------------------
# patterns over K context slots (bool [K])
# ---------------------------------------------------------------------------------------------------------------------------------
def hash_pattern(K: int, seed: int = HASH_SEED, mod: int = 3) -> np.ndarray:
    """two thirds of the positions, scattered: hash_u32(seed, K) % mod != 0"""
    return (synth.hash_u32(seed, K).numpy() % mod) != 0


def suffix(K: int, m: int) -> np.ndarray:
    """the m positions K - m .. K - 1: what an AR model has emitted after m tokens (tokens.suffix_mask)"""
    return np.arange(K) >= K - m


def prefix(K: int, n: int) -> np.ndarray:
    return np.arange(K) < n


def single(K: int, j: int) -> np.ndarray:
    return np.arange(K) == j


def alternating(K: int) -> np.ndarray:
    return (np.arange(K) & 1) == 1


def empty_word(K: int, word: int) -> np.ndarray:
    """everything visible but the 32 positions of one word: an empty word inside a live 64-key tile"""
    return (np.arange(K) >> 5) != word


def model_rows(K: int = 512) -> np.ndarray:
    """the per-sample [16, K] mask of golden (c): row 0 full, 1 the suffix m = 301, 2 the hash pattern, 3 a single visible key (position 100),
    4 first visible key above 256 (positions 300 ..), 5 .. 15 other suffixes / prefixes / hash patterns.  Every row keeps a key <= 375 (the
    step mask of schedule index 30), so no sample of the reference's run is without a visible context key."""
    rows = [prefix(K, K), suffix(K, 301), hash_pattern(K), single(K, 100), suffix(K, K - 300), suffix(K, 140), ~hash_pattern(K), np.roll(hash_pattern(K), 7),
            prefix(K, 100), alternating(K), empty_word(K, 5), single(K, 0)]
    for r in range(12, 16):
        rows.append(hash_pattern(K, HASH_SEED + r, 2 + r % 3))
    return np.stack(rows)


def pack(rows: np.ndarray, words: int = 0) -> np.ndarray:
    """bool [B, K] -> int32 [B, max(ceil(K / 32), words)]: key j = bit j & 31 of word j >> 5 (numpy twin of ops.pack_key_mask)"""
    B, K = rows.shape
    W = max((K + 31) // 32, words)
    out = np.zeros((B, W), dtype=np.uint32)
    for b in range(B):
        for j in np.nonzero(rows[b])[0]:
            out[b, j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    return out.view(np.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# kernel-level cases: ops.ex_attention(q, k1, v1, H, k2, v2, slots1=Tk1, kmask=)
# ---------------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    Tk1: int                      # context slots
    Tk2: int                      # image keys (always visible)
    Tq: int
    rows: Tuple[str, ...]         # one pattern name per sample
    H: int = 2
    shared: bool = False          # pass ONE word row ([1, W], kmask_bs = 0); every sample has rows[0]

    @property
    def B(self):
        return len(self.rows)


def pattern(name: str, K: int) -> np.ndarray:
    kind, _, arg = name.partition(":")
    if kind == "full":
        return prefix(K, K)
    if kind == "none":
        return prefix(K, 0)
    if kind == "hash":
        return hash_pattern(K, HASH_SEED + int(arg or 0))
    if kind == "nothash":
        return ~hash_pattern(K)
    if kind == "suffix":
        return suffix(K, int(arg))
    if kind == "prefix":
        return prefix(K, int(arg))
    if kind == "single":
        return single(K, int(arg))
    if kind == "alt":
        return alternating(K)
    if kind == "noword":
        return empty_word(K, int(arg))
    if kind == "from":                       # positions arg .. K - 1
        return np.arange(K) >= int(arg)
    raise ValueError(name)


def case_mask(c: Case) -> np.ndarray:
    return np.stack([pattern(r, c.Tk1) for r in c.rows])


# valid counts around the 32 / 64 / 256 / 512 edges: the ten visibility cases of tests/test_encoder_exact_gpu.py (slots, valid, Tk2, Tq) plus valid = 0 at K = 1024
PREFIX_CASES = [(512, 512, 256, 512), (512, 358, 256, 358), (512, 358, 256, 256), (512, 100, 256, 100), (512, 20, 256, 256), (512, 0, 256, 256),
                (512, 300, 0, 300), (1024, 750, 256, 750), (1024, 300, 256, 256), (1024, 1024, 256, 200), (1024, 0, 256, 256),
                (512, 31, 256, 128), (512, 32, 256, 128), (512, 33, 256, 128), (512, 63, 256, 128), (512, 64, 256, 128), (512, 65, 256, 128),
                (512, 255, 256, 128), (512, 256, 256, 128), (512, 257, 256, 128), (512, 511, 256, 128), (1024, 512, 256, 128), (1024, 513, 256, 128)]
# shapes of the unfused-only route: the 320 px key count (400 image keys: a last kv block of 400) and a ragged slot count
PREFIX_CASES_UNFUSED = [(512, 358, 400, 400), (512, 33, 400, 130), (512, 0, 400, 130), (496, 300, 64, 64)]

MASK_CASES = [
    Case("suffixes", 512, 256, 200, ("suffix:301", "suffix:37", "suffix:1", "suffix:512")),
    Case("single_key", 512, 256, 130, ("single:0", "single:100", "single:511", "single:31")),
    Case("alternating", 512, 256, 130, ("alt", "hash", "nothash")),
    Case("empty_word_in_live_tile", 512, 256, 130, ("noword:5", "noword:0", "noword:15", "noword:8")),
    Case("empty_first_block_k1024", 1024, 256, 200, ("suffix:300", "from:512", "single:900")),
    Case("no_context_key", 512, 256, 130, ("none", "full", "none")),
    Case("rows_differ", 512, 256, 256, ("full", "suffix:301", "hash", "single:100", "from:300")),
    Case("shared_row", 512, 256, 130, ("hash", "hash", "hash"), shared=True),
    Case("context_only", 512, 0, 300, ("hash", "suffix:301", "single:100", "full")),          # Tk2 = 0: the CFG conditional pass of the context rows
    Case("context_only_dead_sample", 512, 0, 130, ("hash", "none", "suffix:37")),             # ... with a sample that sees nothing: zeros
    Case("k1024_mixed", 1024, 256, 130, ("hash", "suffix:300", "alt", "full")),
]
# the same on the unfused-only shapes
MASK_CASES_UNFUSED = [
    Case("px320_rows_differ", 512, 400, 400, ("full", "suffix:301", "hash", "single:100", "from:300")),
    Case("px320_shared", 512, 400, 130, ("suffix:37", "suffix:37"), shared=True),
]
# kernel-level goldens (e): F.scaled_dot_product_attention(q, k, v, attn_mask=bool) of torch-CPU; 2 samples x 2 heads x 128 queries x head_dim 64
SDPA_CASES = [
    Case("sdpa512_full_suffix301", 512, 256, 128, ("full", "suffix:301")),
    Case("sdpa512_hash_single", 512, 256, 128, ("hash", "single:100")),
    Case("sdpa512_from300_hash", 512, 256, 128, ("from:300", "hash")),
    Case("sdpa1024_suffix300", 1024, 256, 128, ("suffix:300", "suffix:300")),
    Case("sdpa1024_hash_suffix300", 1024, 256, 128, ("hash", "suffix:300")),
]


def inputs(c: Case, device="cpu"):
    """q [B, Tq, 3 H 64] (its first third is the query), ctx [B, Tk1, 3 H 64] and img [B, Tk2, 3 H 64] fused q | k | v projections"""
    HD = c.H * DH
    q = synth.hash_normalish(synth.name_seed(f"exk/{c.name}/q"), (c.B, c.Tq, 3 * HD)).float() * 1.3
    ctx = synth.hash_normalish(synth.name_seed(f"exk/{c.name}/ctx"), (c.B, c.Tk1, 3 * HD)).float() * 1.3
    img = synth.hash_normalish(synth.name_seed(f"exk/{c.name}/img"), (c.B, max(c.Tk2, 1), 3 * HD)).float() * 1.3
    return q.to(device).contiguous(), ctx.to(device).contiguous(), img.to(device).contiguous()


def _heads(t, H, part):
    HD = H * DH
    return t[..., part * HD:(part + 1) * HD].reshape(t.shape[0], t.shape[1], H, DH).transpose(1, 2)       # [B, H, T, 64]


def reference(c: Case, q, ctx, img, mask: np.ndarray, dtype=torch.float64):
    """masked softmax attention in plain torch, [B, Tq, H 64]; a sample without a visible key gives zeros.
    dtype float64: the reference; float32: the comparator of the gate (torch's own fp32 matmul / softmax)."""
    q, ctx, img = q.cpu(), ctx.cpu(), img.cpu()
    out = torch.zeros(c.B, c.Tq, c.H * DH, dtype=dtype)
    for b in range(c.B):
        vis = torch.from_numpy(np.nonzero(mask[b])[0])
        qq = _heads(q[b:b + 1], c.H, 0).to(dtype)
        k = _heads(ctx[b:b + 1, vis], c.H, 1).to(dtype)
        v = _heads(ctx[b:b + 1, vis], c.H, 2).to(dtype)
        if c.Tk2:
            k = torch.cat([k, _heads(img[b:b + 1, :c.Tk2], c.H, 1).to(dtype)], 2)
            v = torch.cat([v, _heads(img[b:b + 1, :c.Tk2], c.H, 2).to(dtype)], 2)
        if k.shape[2] == 0:
            continue
        s = torch.matmul(qq, k.transpose(-1, -2)) * SCALE
        p = torch.exp(s - s.amax(-1, keepdim=True))
        o = torch.matmul(p, v) / p.sum(-1, keepdim=True)
        out[b] = o.transpose(1, 2).reshape(c.Tq, c.H * DH)
    return out


def sdpa_aten(c: Case, q, ctx, img, mask: np.ndarray):
    """what the generator stores for SDPA_CASES: torch-CPU's F.scaled_dot_product_attention with the reference's materialised bool mask
    [B, 1, Tq, Tk] (sd3/mmdit.py:1081-1084, sd3/other_impls.py:37-45) -> [B, Tq, H 64]"""
    import torch.nn.functional as F
    qq = _heads(q, c.H, 0)
    k = torch.cat([_heads(ctx, c.H, 1), _heads(img[:, :c.Tk2], c.H, 1)], 2)
    v = torch.cat([_heads(ctx, c.H, 2), _heads(img[:, :c.Tk2], c.H, 2)], 2)
    m = torch.cat([torch.from_numpy(mask), torch.ones(c.B, c.Tk2, dtype=torch.bool)], 1)
    m = m.bool().unsqueeze(1).unsqueeze(2).repeat(1, 1, c.Tq, 1)
    o = F.scaled_dot_product_attention(qq, k, v, attn_mask=m, dropout_p=0.0, is_causal=False)
    return o.transpose(1, 2).reshape(c.B, c.Tq, c.H * DH)
