"""Case table and fp64 reference of tests/test_attention_kmask_gpu.py: the joint attention with a per-sample key bit mask
(selftok_attn_kmask_f32, include/selftok_hip_ext.h).  tests/test_ar_partial_cpu.py checks without a GPU that the table holds the
patterns it claims and that every case would see ONE wrong bit.

Inputs are functions of the case name (synth.hash_uniform), so they regenerate on any host; buffers, padding and the accuracy gate
follow tests/edge_cases.py.  The reference is plain torch: softmax(q k^T scale) v in float64 over the visible key set, the
materialised-mask semantics of sd3/mmdit.py:1059-1094 (a context key is visible to every row iff its bit is set; a context ROW
whose bit is clear is dead).  No project code is used as a reference.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

import edge_cases as E
from selftoktokenizer_amd import synth

DH, SCALE = E.DH, E.SCALE


@dataclass(frozen=True)
class KCase:
    name: str
    H: int
    Kc: int                                  # segment-0 `len` of the launch
    nx: int
    patterns: Tuple[Tuple[str, bytes], ...]  # per sample: (label, packed bool mask over Kw keys) -- see `mask`
    see: bool
    Kw: int                                  # keys the mask words cover (>= Kc; bits at Kc .. Kw - 1 must be ignored)
    pre_only: bool = False

    @property
    def B(self):
        return len(self.patterns)

    @property
    def D(self):
        return self.H * DH

    @property
    def W(self):
        return 3 * self.D + E.COL_PAD

    def mask(self, b: int) -> np.ndarray:
        """bool [Kw] as given to the kernel (bits past Kc possibly set)"""
        return np.unpackbits(np.frombuffer(self.patterns[b][1], dtype=np.uint8), bitorder="little")[:self.Kw].astype(bool)

    def visible(self, b: int) -> np.ndarray:
        """sorted visible key indices < Kc"""
        return np.nonzero(self.mask(b)[:self.Kc])[0]

    def masks(self) -> np.ndarray:
        return np.stack([self.mask(b) for b in range(self.B)])


def pack_words(mask: np.ndarray) -> np.ndarray:
    """numpy statement of the kernel's bit layout: bool [B, K] -> uint32 [B, ceil(K/32)], key j = bit j & 31 of word j >> 5"""
    B, K = mask.shape
    W = (K + 31) // 32
    m = np.zeros((B, W * 32), dtype=np.uint64)
    m[:, :K] = mask
    return (m.reshape(B, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def _pat(label, m):
    return label, np.packbits(np.asarray(m, dtype=bool), bitorder="little").tobytes()


def hash_pattern(K: int) -> np.ndarray:
    """the visibility pattern of tests/golden/sampler_options_b1.npz (~2/3 of the tokens visible, no structure)"""
    return (synth.hash_u32(0x5A5A, K) % 3 != 0).numpy().astype(bool)


def suffix(K: int, lo: int) -> np.ndarray:
    return np.arange(K) >= lo


def pattern_set(K: int):
    """one sample per pattern: suffix windows with the lower edge at -1 / 0 / +1 around multiples of 32 and 128, single keys, empty, full,
    every other key, every other tile, the last tile only, the hash pattern"""
    pats = []
    for e in (32, 64, 128, 256, 384, K - 128, K - 32):
        for d in (-1, 0, 1):
            pats.append(_pat(f"suffix_lo{e + d}", suffix(K, e + d)))
    for j in (0, 31, 32, K - 1):
        pats.append(_pat(f"single{j}", np.arange(K) == j))
    a = np.arange(K)
    pats += [_pat("empty", a < 0), _pat("full", a >= 0), _pat("odd_keys", a % 2 == 1), _pat("even_tiles", (a // 32) % 2 == 0),
             _pat("last_tile", a >= K - 32), _pat("hash", hash_pattern(K))]
    return tuple(pats)


def _b5(K):
    a = np.arange(K)
    return (_pat("suffix_lo301", suffix(K, 301)), _pat("hash", hash_pattern(K)), _pat("empty", a < 0),
            _pat("odd_tiles", (a // 32) % 2 == 1), _pat("single_last", a == K - 1))


def _trunc(K, n):
    """masks over K = 512 keys for a launch truncated to n rows: bits at and past n set on purpose"""
    a = np.arange(K)
    return (_pat("full_beyond", a >= 0), _pat("suffix_lo_n-1", a >= n - 1), _pat("hash", hash_pattern(K)), _pat("only_beyond", a >= n),
            _pat("odd_keys", a % 2 == 1))


def _product():
    """B = 64, H = 24, 512 + 256 rows: 64 different suffix lengths spread over 1 .. 512"""
    K = 512
    ms = [1 + (b * 511) // 63 for b in range(64)]
    assert len(set(ms)) == 64 and ms[0] == 1 and ms[-1] == 512
    return KCase("product_b64_h24_suffix", 24, K, 256, tuple(_pat(f"suffix_m{m}", suffix(K, K - m)) for m in ms), True, K)


PATTERN_CASES = [
    KCase("pat512_see1", 2, 512, 256, pattern_set(512), True, 512),
    KCase("pat512_see0", 2, 512, 256, pattern_set(512), False, 512),
    KCase("pat1024_see1", 2, 1024, 256, pattern_set(1024), True, 1024),
    KCase("pat1024_see0", 2, 1024, 256, pattern_set(1024), False, 1024),
    KCase("preonly_pat512", 2, 512, 256, pattern_set(512), True, 512, pre_only=True),
    KCase("preonly_pat1024", 2, 1024, 256, pattern_set(1024), True, 1024, pre_only=True),
    KCase("b5_mixed_512", 3, 512, 45, _b5(512), True, 512),
]
TRUNC_CASES = [KCase(f"trunc_n{n}_see{int(see)}", 2, n, 256, _trunc(512, n), see, 512) for n, see in ((358, True), (33, False), (1, True))]
PRODUCT_CASE = _product()
CASES = PATTERN_CASES + TRUNC_CASES + [PRODUCT_CASE]


def sample(case: KCase, b: int, device="cpu", poison: bool = False):
    """sample b's segment-0 / segment-1 buffers [rows, W] = q | k | v | padding columns (rows past `len` included).
    poison: every invisible context key (and every row past `len`) gets k = NaN / +Inf and v = NaN / POISON_V alternating, and
    every dead context row's q is NaN -- contents the kernel must never let into its arithmetic."""
    D = case.D
    c = synth.hash_uniform(synth.name_seed(f"kmask/{case.name}/ctx/{b}"), (case.Kw + E.CTX_PAD, case.W), -1.5, 1.5, device)
    x = synth.hash_uniform(synth.name_seed(f"kmask/{case.name}/img/{b}"), (case.nx + E.IMG_PAD, case.W), -1.5, 1.5, device)
    if poison:
        dead = torch.ones(c.shape[0], dtype=torch.bool)
        dead[torch.from_numpy(case.visible(b))] = False
        dead = dead.to(device)
        alt = (torch.arange(c.shape[0], device=device) % 2 == 0)
        c[dead & alt, D:2 * D] = float("nan")
        c[dead & ~alt, D:2 * D] = float("inf")
        c[dead & alt, 2 * D:3 * D] = E.POISON_V
        c[dead & ~alt, 2 * D:3 * D] = float("nan")
        c[dead, 0:D] = float("nan")
    return c, x


def buffers(case: KCase, device="cpu", poison: bool = False):
    cs, xs = zip(*(sample(case, b, device, poison) for b in range(case.B)))
    return torch.stack(cs), torch.stack(xs)


def reference(case: KCase, b: int, c: torch.Tensor, x: torch.Tensor, fp64: bool = True, heads=None, vis: Optional[np.ndarray] = None):
    """(context rows [h, n_visible, 64] in the order of `vis`, or None; image rows [h, nx, 64]) over the visible key set"""
    heads = tuple(range(case.H)) if heads is None else tuple(heads)
    vis = case.visible(b) if vis is None else vis
    c, x = c.cpu(), x.cpu()
    qc, kc, vc = E._heads(c[torch.from_numpy(vis)], case.H, heads)
    qx, kx, vx = E._heads(x[:case.nx], case.H, heads)
    k_all, v_all = torch.cat([kc, kx], 1), torch.cat([vc, vx], 1)
    o_x = E._attend(qx, k_all, v_all, fp64)
    o_c = None
    if not case.pre_only and len(vis) > 0:
        o_c = E._attend(qc, k_all, v_all, fp64) if case.see else E._attend(qc, kc, vc, fp64)
    return o_c, o_x


def flip_one_bit(case: KCase, b: int):
    """(new visible set, key flipped): the lowest visible key hidden, or key 0 shown when nothing is visible"""
    vis = case.visible(b)
    if len(vis) == 0:
        return np.array([0]), 0
    return vis[1:], int(vis[0])
