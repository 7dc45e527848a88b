"""Token file / wire formats either side of the hot path.

The reference hands tokens around as `np.save` of an int64 `[B,K]` array (test.py:38-39) -- 8 bytes per 15-bit id.
Ids are < 32768 = 2^15, so they also fit uint16 (4x smaller) or a dense 15-bit stream (4.27x smaller); both are
lossless and round-trip to the reference's int64 layout.  `reverse_for_ar` implements the README's note for AR
training ("decode the sequence reversely", README.md:241).  The sampler's step mask is `arange(K) <= k(t)` with k falling
from K - 1 (models_ours.py:345-353): index 0 is visible at EVERY step, index K - 1 only at the first ones (large t).  An AR
model emits index K - 1 first and index 0 last, so the first m tokens it has emitted are the tokenizer positions K - m .. K - 1,
a SUFFIX: `pad_ar_partial` / `suffix_mask` place them, `SelftokPipeline.decoding(ar_partial=m)` decodes from them.
`pad_prefix` / `prefix_mask` serve the reference's other hook, `arange(K) < k` (decoding(prefix_k=)): NOT the AR partial route.
"""
from __future__ import annotations

import numpy as np

CODEBOOK_BITS = 15


def save_reference_npy(path: str, tokens) -> None:
    """exactly what the reference script writes: int64 [B,K] .npy"""
    np.save(path, np.asarray(tokens, dtype=np.int64))


def load_reference_npy(path: str) -> np.ndarray:
    t = np.load(path)
    if t.dtype != np.int64:
        t = t.astype(np.int64)
    return t


def to_uint16(tokens) -> np.ndarray:
    t = np.asarray(tokens)
    if t.size and (t.min() < 0 or t.max() >= (1 << 16)):
        raise ValueError("token id out of uint16 range")
    return t.astype(np.uint16)


def pack15(tokens) -> bytes:
    """dense little-endian bit stream, 15 bits per id, row-major; header-less (shape travels separately)."""
    t = np.asarray(tokens, dtype=np.int64).reshape(-1)
    if t.size and (t.min() < 0 or t.max() >= (1 << CODEBOOK_BITS)):
        raise ValueError("token id does not fit 15 bits")
    bits = ((t[:, None] >> np.arange(CODEBOOK_BITS)) & 1).astype(np.uint8).reshape(-1)
    return np.packbits(bits, bitorder="little").tobytes()


def unpack15(buf: bytes, shape) -> np.ndarray:
    n = int(np.prod(shape))
    bits = np.unpackbits(np.frombuffer(buf, dtype=np.uint8), bitorder="little")[: n * CODEBOOK_BITS]
    vals = (bits.reshape(n, CODEBOOK_BITS).astype(np.int64) << np.arange(CODEBOOK_BITS)).sum(axis=1)
    return vals.reshape(shape)


def reverse_for_ar(tokens) -> np.ndarray:
    """[B,K] -> [B,K] with the token axis reversed (coarse-to-fine order for AR models)."""
    return np.ascontiguousarray(np.asarray(tokens)[:, ::-1])


def to_ar_order(tokens) -> np.ndarray:
    """tokenizer order -> the order an AR model is trained on / emits (README.md:241: reversed)"""
    return reverse_for_ar(tokens)


def from_ar_order(tokens) -> np.ndarray:
    """what an AR model emitted (coarse -> fine) -> tokenizer order, ready for `SelftokPipeline.decoding`"""
    return reverse_for_ar(tokens)


def pad_prefix(prefix, K: int, fill: int = 0):
    """[B,k] tokenizer-order prefix (k <= K) -> (int64 [B,K] padded with `fill`, k): the arguments of
    `SelftokPipeline.decoding(idx, prefix_k=k)`.  The padding ids are never visible (mask * super_mask)."""
    t = np.asarray(prefix)
    if t.ndim != 2 or t.shape[1] > K:
        raise ValueError(f"prefix must be [B,k] with k <= {K}")
    out = np.full((t.shape[0], K), fill, dtype=np.int64)
    out[:, : t.shape[1]] = t
    return out, int(t.shape[1])


def pad_ar_partial(ar_tokens, K: int, fill: int = 0):
    """what an AR model has emitted so far, in the order it emitted it (coarse first) -> (int64 [B,K] ids in tokenizer order, int64 [B] m).
    `ar_tokens`: [B,m], or a list of B 1-D sequences of different lengths m_b <= K.  Token i of sample b lands at tokenizer position
    K - 1 - i; every other position holds `fill` (never read: `suffix_mask(K, m)` hides it).  The arguments of
    `SelftokPipeline.decoding(idx, ar_partial=m)`."""
    if isinstance(ar_tokens, np.ndarray) and ar_tokens.ndim == 2:
        rows = list(ar_tokens)
    else:
        rows = [np.asarray(r) for r in ar_tokens]
    out = np.full((len(rows), K), fill, dtype=np.int64)
    m = np.zeros(len(rows), dtype=np.int64)
    for b, r in enumerate(rows):
        r = np.asarray(r)
        if r.ndim != 1 or r.shape[0] > K:
            raise ValueError(f"sample {b}: expected a 1-D sequence of at most K = {K} tokens, got shape {r.shape}")
        if r.size and not np.issubdtype(r.dtype, np.integer):
            raise TypeError(f"token ids must be integers, got {r.dtype}")
        m[b] = r.shape[0]
        out[b, K - r.shape[0]:] = r[::-1]
    return out, m


def suffix_mask(K: int, m) -> np.ndarray:
    """bool [B,K]: arange(K) >= K - m[b], the positions the first m[b] tokens of an AR model occupy (`pad_ar_partial`)"""
    m = np.asarray(m, dtype=np.int64).reshape(-1, 1)
    if m.size and (m.min() < 0 or m.max() > K):
        raise ValueError(f"m must be in [0, {K}]")
    return np.arange(K)[None, :] >= K - m


def prefix_mask(K: int, k) -> np.ndarray:
    """visibility mask of a partial decode that uses only tokens 0..k (reference get_encoder_mask, models_ours.py:345-353)"""
    k = np.asarray(k).reshape(-1, 1)
    return np.arange(K)[None, :] <= k


def margins(scores):
    """scores [..., k >= 2] of `SelftokPipeline.encoding_topk` / `ops.vq_topk` -> scores[..., 0] - scores[..., 1], the amount by which every
    token's id won over the runner-up.  A small margin marks a near-tie: a token that another VAE mode, batch size or GPU may move.
    numpy in, numpy out; a torch tensor gives a torch tensor."""
    if scores.shape[-1] < 2:
        raise ValueError("margins need the two best scores of every token (k >= 2)")
    return scores[..., 0] - scores[..., 1]
