"""Statistics of token-id matrices, computed on the device (csrc/token_stats.hip through ops.token_*): what a [N, K] matrix of code ids says about the
tokenizer that made it.

  TokenCensus          running code counts per position -> code-book usage, perplexity (exp of the Shannon entropy of the POOLED counts, and the reference's
                       `get_group_perplexity` form with its 1e-10 inside the logarithm), per-position figures, dead codes; counts merge and save as .npz, so
                       ranks and shards combine offline.
  token_agreement      two tokenisations of the same rows: match rate overall and per position, equal rows, and per row the number of differing positions with
                       the lowest and the highest differing index.  Both ends matter: the sampler sees index 0 at every step, an autoregressive model that
                       emits in the reference's reverse order emits index K - 1 first (tokens.py), so ITS first wrong token is `last_diff`.
  nearest_sequences    for every query sequence the reference sequence with the most equal positions (ties: the lowest index) -- whether a generated sequence
                       is a near-copy of a training sequence, or (exclude_self) of another row of its own set.

Ids are integers of any dtype, device tensors or numpy arrays, [..., K], strided views included.  There is no CPU fallback: the arithmetic of record in numpy is
tests/token_stats_cases.py, and it is a test's, not the product's.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import _lib, ops

ROW_LIMIT = (1 << 32) - 1          # a uint32 counter holds at most this many rows
NEAREST_WS_BYTES = 64 << 20        # nearest_sequences chunks its queries so that one call's workspace stays below this
_NATIVE = (torch.uint16, torch.int32, torch.int64)


def _device_ids(ids, device, what: str) -> torch.Tensor:
    """integer ids of any dtype, numpy or torch, host or device -> a device tensor of a dtype the kernels read (uint16, int32, int64); a device tensor of
    such a dtype comes back as it is, strides and all"""
    if isinstance(ids, np.ndarray):
        if not np.issubdtype(ids.dtype, np.integer):
            raise TypeError(f"{what}: token ids must be integers, got {ids.dtype}")
        if ids.dtype == np.uint64:
            ids = np.where(ids > np.uint64(np.iinfo(np.int64).max), np.int64(-1), ids.astype(np.int64))       # past int64: a bad id either way
        elif ids.dtype not in (np.uint16, np.int32, np.int64):
            ids = ids.astype(np.int64)
        ids = torch.from_numpy(np.ascontiguousarray(ids))
    if not isinstance(ids, torch.Tensor):
        raise TypeError(f"{what}: expected a torch tensor or a numpy array of token ids, got {type(ids).__name__}")
    if ids.dtype.is_floating_point or ids.dtype.is_complex or ids.dtype == torch.bool:
        raise TypeError(f"{what}: token ids must be integers, got {ids.dtype}")
    if ids.dim() < 1:
        raise ValueError(f"{what}: expected ids [..., K], got a scalar")
    if not ids.is_cuda:
        ids = ids.to(device)
    if ids.dtype not in _NATIVE:
        ids = ids.to(torch.int64)
    return ids


def _u32(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint32)


class TokenCensus:
    """Running counts of code ids per position.  `update` launches one kernel and reads nothing back; `result` does one host read."""

    def __init__(self, K: int, C: int = 32768, device="cuda"):
        K, C = int(K), int(C)
        if K < 1 or C < 1 or K * C >= 1 << 31:
            raise ValueError(f"TokenCensus: need K >= 1, C >= 1 and K * C below 2^31, got K {K}, C {C}")
        self.K, self.C, self.device = K, C, torch.device(device)
        self.rows = 0                                              # rows counted, host side: the limit is decided without the device
        self._dev = None                                           # int32 [K, C] (uint32 arithmetic) and int32 [1] on the device, allocated by the first update
        self._bad = None
        self._host = None                                          # uint32 [K, C] counts that arrived through merge / load and are not on the device yet
        self._host_bad = 0

    def _reserve(self, n_rows: int) -> None:
        if self.rows + n_rows > ROW_LIMIT:
            raise ValueError(f"TokenCensus: {self.rows} + {n_rows} rows pass the limit of {ROW_LIMIT} rows a uint32 counter holds; start a second census and merge offline in a wider type")

    def _ensure(self) -> None:
        if self._dev is None:
            self._dev = torch.zeros(self.K, self.C, dtype=torch.int32, device=self.device)
            self._bad = torch.zeros(1, dtype=torch.int32, device=self.device)

    def update(self, ids) -> "TokenCensus":
        if not isinstance(ids, (np.ndarray, torch.Tensor)):
            raise TypeError(f"TokenCensus.update: expected a torch tensor or a numpy array, got {type(ids).__name__}")
        if ids.ndim < 1 or ids.shape[-1] != self.K:
            raise ValueError(f"TokenCensus.update: expected ids [..., {self.K}], got {tuple(ids.shape)}")
        n_rows = int(np.prod(ids.shape[:-1])) if ids.ndim > 1 else 1
        self._reserve(n_rows)                                      # before anything touches the device
        ids = _device_ids(ids, self.device, "TokenCensus.update")
        with torch.cuda.device(self.device):
            self._ensure()
            ops.token_count(ids, self._dev, self._bad)
        self.rows += n_rows
        return self

    def _flush(self) -> None:
        """counts that arrived on the host join the device's"""
        if self._host is not None:
            self._ensure()
            self._dev += torch.from_numpy(self._host.view(np.int32)).to(self.device)       # two's complement: the uint32 sum
            self._bad += int(self._host_bad)
            self._host, self._host_bad = None, 0

    def counts(self) -> np.ndarray:
        """uint32 [K, C]"""
        out = np.zeros((self.K, self.C), np.uint32) if self._dev is None else _u32(self._dev)
        return out if self._host is None else out + self._host

    def bad_ids(self) -> int:
        return (0 if self._bad is None else int(_u32(self._bad)[0])) + int(self._host_bad)

    def dead_codes(self) -> np.ndarray:
        """the codes no position ever used, ascending (int64)"""
        return np.flatnonzero(self.counts().astype(np.uint64).sum(0) == 0)

    def result(self) -> dict:
        with torch.cuda.device(self.device):
            self._flush()
            self._ensure()
            census = ops.token_census(self._dev)
            host = torch.cat([census.reshape(-1), (self._bad.to(torch.int64) & 0xFFFFFFFF).to(torch.float64)]).cpu().numpy()     # the one host read
        t, bad = host[:-1].reshape(self.K + 1, 5), int(host[-1])
        n, used, H, H_ref, mx = t[self.K]
        return {"rows": self.rows, "bad_ids": bad, "K": self.K, "C": self.C, "tokens": int(n),
                "usage": float(used) / self.C, "used": int(used),
                "perplexity": math.exp(H), "perplexity_ref": math.exp(H_ref), "entropy_bits": H / math.log(2.0),
                "max_code_share": float(mx) / float(n) if n > 0 else 0.0,
                "used_pos": t[:self.K, 1].astype(np.int64), "perplexity_pos": np.exp(t[:self.K, 2]), "perplexity_ref_pos": np.exp(t[:self.K, 3])}

    def summary(self) -> dict:
        """`result()` as plain JSON types, the per-position arrays reduced to their minimum, mean and maximum"""
        r = self.result()
        out = {k: v for k, v in r.items() if not isinstance(v, np.ndarray)}
        for k in ("used_pos", "perplexity_pos", "perplexity_ref_pos"):
            out[k] = {"min": float(r[k].min()), "mean": float(r[k].mean()), "max": float(r[k].max())}
        return out

    def merge(self, other: "TokenCensus") -> "TokenCensus":
        if (other.K, other.C) != (self.K, self.C):
            raise ValueError(f"TokenCensus.merge: [K, C] differ: {(self.K, self.C)} and {(other.K, other.C)}")
        self._reserve(other.rows)
        add = other.counts()
        self._host = add if self._host is None else self._host + add
        self._host_bad += other.bad_ids()
        self.rows += other.rows
        return self

    def save(self, path: str) -> None:
        np.savez_compressed(path, counts=self.counts(), bad_ids=np.int64(self.bad_ids()), rows=np.int64(self.rows))

    @classmethod
    def load(cls, path: str, device="cuda") -> "TokenCensus":
        with np.load(path) as z:
            counts, bad, rows = z["counts"], int(z["bad_ids"]), int(z["rows"])
        if counts.ndim != 2 or counts.dtype != np.uint32:
            raise ValueError(f"TokenCensus.load: {path} holds no uint32 [K, C] counts")
        c = cls(counts.shape[0], counts.shape[1], device)
        c._reserve(rows)
        c._host, c._host_bad, c.rows = counts.copy(), bad, rows
        return c


def _dense_u16(ids, device, what: str) -> torch.Tensor:
    ids = _device_ids(ids, device, what)
    if ids.dim() != 2:
        raise ValueError(f"{what}: expected ids [N, K], got {tuple(ids.shape)}")
    if ids.dtype == torch.uint16 and ids.is_contiguous():
        return ids
    bad = torch.zeros(1, dtype=torch.int32, device=ids.device)
    out = ops.token_to_u16(ids, bad)
    if int(bad.item()):
        raise ValueError(f"{what}: {int(bad.item())} ids outside [0, 65535]")
    return out


def _device_of(*xs):
    for x in xs:
        if isinstance(x, torch.Tensor) and x.is_cuda:
            return x.device
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cuda")


def token_agreement(a, b, k_range=None) -> dict:
    """a, b [N, K] ids of the same rows -> match_rate (over N * positions), match_rate_pos (float64 [k_hi - k_lo]), rows_equal, and per row n_diff, first_diff
    (K when the rows agree) and last_diff (-1 when they agree) as int32 numpy arrays."""
    dev = _device_of(a, b)
    with torch.cuda.device(dev):
        a, b = _dense_u16(a, dev, "token_agreement"), _dense_u16(b, dev, "token_agreement")
        if a.shape != b.shape:
            raise ValueError(f"token_agreement: shapes differ: {tuple(a.shape)} and {tuple(b.shape)}")
        N, K = a.shape
        k_lo, k_hi = (0, K) if k_range is None else (int(k_range[0]), int(k_range[1]))
        match_pos, n_diff, first, last = ops.token_agree(a, b, (k_lo, k_hi))
        host = torch.cat([match_pos, n_diff, first, last]).cpu().numpy()
    match_pos, n_diff, first, last = host[:K].view(np.uint32)[k_lo:k_hi], host[K:K + N], host[K + N:K + 2 * N], host[K + 2 * N:]
    span = k_hi - k_lo
    return {"rows": N, "positions": span, "match_rate": float(match_pos.sum()) / (N * span) if N * span else 1.0,
            "match_rate_pos": match_pos.astype(np.float64) / N if N else np.ones(span), "rows_equal": int((n_diff == 0).sum()),
            "n_diff": n_diff.copy(), "first_diff": first.copy(), "last_diff": last.copy()}


def nearest_chunk(N: int, chunk: Optional[int] = None) -> int:
    """queries per call: the workspace is one 64-bit key per reference split (at most min(64, ceil(N / 64))) and query"""
    if chunk is not None:
        if int(chunk) < 1:
            raise ValueError("nearest_sequences: chunk must be >= 1")
        return int(chunk)
    parts = max(1, min(64, -(-N // 64)))
    return max(64, NEAREST_WS_BYTES // (8 * parts) // 64 * 64)


def nearest_sequences(q, ref, k_range=None, exclude_self: bool = False, chunk: Optional[int] = None):
    """q [M, K], ref [N, K] ids -> (best_match, best_idx), int32 device tensors [M]: the largest number of equal positions (within k_range) over the reference rows
    and the lowest reference index that attains it; (-1, 0) where there is no candidate.  exclude_self: row i is not its own candidate (q is ref: dedup).
    The queries go through in chunks that bound the workspace; the result is the same for every chunk size."""
    dev = _device_of(q, ref)
    with torch.cuda.device(dev):
        qd = _dense_u16(q, dev, "nearest_sequences")
        rd = qd if ref is q else _dense_u16(ref, dev, "nearest_sequences")
        M, N = qd.shape[0], rd.shape[0]
        if qd.shape[1] != rd.shape[1]:
            raise ValueError(f"nearest_sequences: K differs: {tuple(qd.shape)} and {tuple(rd.shape)}")
        step = nearest_chunk(N, chunk)
        best = torch.empty(M, dtype=torch.int32, device=dev)
        idx = torch.empty(M, dtype=torch.int32, device=dev)
        for i0 in range(0, M, step):
            i1 = min(M, i0 + step)
            ops.token_nearest(qd[i0:i1], rd, k_range, 1 + i0 if exclude_self else 0, out_match=best[i0:i1], out_idx=idx[i0:i1])
    return best, idx
