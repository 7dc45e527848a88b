"""Host-side schedule of the rectified-flow decode (product code; numpy fp32, no torch kernels involved).

Reproduces bit-for-bit what the reference computes with torch-CPU:
  RectifiedFlow.make_schedule('uniform')  sd3/rectified_flow.py:66-80   (torch.linspace fp32 on CPU)
  timestep_map[i] -> .long()              sd3/rectified_flow.py:203 ; SelftokPipeline.py:243
  DiTi_cont.to_indices / get_position     diti_utils.py:73-110
  encoder mask  arange(K) <= k            models_ours.py:345-353   (here: just the visible count k+1)
The fragile part is float: linspace(1,0,51)*1000 truncates to 459, 399, ... not 460, 400;
tests/test_schedule.py pins this module to tests/golden/schedule.npz (captured from the reference).

`context_plan`: which context rows each sampler step hands to the model, and by which route (tests/test_context_plan_cpu.py).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np

from . import tokens

f32 = np.float32


def _fma32(a, b, c):
    # a*b is exact in float64 for fp32 inputs and the sum below fits 53 bits for the magnitudes used here,
    # so one rounding to fp32 == fmaf(a, b, c)
    return f32(np.float64(a) * np.float64(b) + np.float64(c))


def linspace32(start: float, end: float, steps: int) -> np.ndarray:
    """ATen CPU linspace for fp32: step=(end-start)/(steps-1); i < steps/2 counts up with an fma,
    the rest counts down from `end`."""
    start, end = f32(start), f32(end)
    step = f32((end - start) / f32(steps - 1))
    out = np.empty(steps, dtype=np.float32)
    half = steps // 2
    for i in range(steps):
        if i < half:
            out[i] = _fma32(step, f32(i), start)
        else:
            out[i] = f32(end - f32(step * f32(steps - 1 - i)))
    return out


class FlowSchedule:
    """RectifiedFlow(num_steps, start=1.0, val_schedule='uniform', shift=1.0) buffers."""

    def __init__(self, num_steps: int = 50, start: float = 1.0):
        base = linspace32(start, 0.0, num_steps + 1)
        self.num_timesteps = num_steps
        self.scheduled_t = base[:-1].copy()
        self.scheduled_t_prev = base[1:].copy()
        self.timestep_map = (self.scheduled_t * f32(1000.0)).astype(np.float32)
        self.one_minus_scheduled_t = (f32(1.0) - self.scheduled_t).astype(np.float32)
        self.t_long = self.timestep_map.astype(np.int64)          # .long(): truncation toward zero
        self.dt = (self.scheduled_t - self.scheduled_t_prev).astype(np.float32)   # a_t - a_prev in fp32


class DiTiCont:
    """DiTi_cont: piecewise-linear timestep -> index of the last visible token."""

    def __init__(self, n_timesteps: int, K: int, stages: str, k_per_stage: str):
        assert stages and k_per_stage
        self.K = K
        self.k_per_stage = [int(k) for k in k_per_stage.split(",")]
        self.stages = [0] + [int(s) for s in stages.split(",")]
        self.segments = []
        acc = 0
        for i, kp in enumerate(self.k_per_stage):
            slope = float(kp) / (self.stages[i + 1] - self.stages[i])
            self.segments.append((self.stages[i], slope, acc))
            acc += kp

    def to_indices(self, t_long) -> np.ndarray:
        """t_long: integer timesteps.  int64 tensor * python float -> fp32 product, truncated."""
        t = np.asarray(t_long, dtype=np.int64)
        ind = np.zeros_like(t)
        for low, slope, base in self.segments:
            xp = t - low
            val = (xp.astype(np.float32) * f32(slope)).astype(np.int64) + base
            ind = np.where(xp >= 0, val, ind)
        return np.clip(ind, 0, self.K - 1)

    @staticmethod
    def get_position(k):
        return 1000 + k * 8


def decode_plan(num_steps: int, diti: DiTiCont):
    """-> (FlowSchedule, k[num_steps]) : everything the decode loop needs from the host."""
    flow = FlowSchedule(num_steps)
    return flow, diti.to_indices(flow.t_long)


# ---- which context tokens a sampler step may see: mask = (arange(K) <= k) * super_mask  (models_ours.py:353, rectified_flow.py:226-227) ----
def rows_uniform(rows: np.ndarray) -> bool:
    return bool((rows == rows[:1]).all())


def prefix_lengths(rows: np.ndarray) -> Optional[np.ndarray]:
    """bool [B, K] -> the visible count of every row if each row is a prefix (arange(K) < count), else None"""
    cnt = rows.sum(axis=1)
    return cnt if bool((rows == (np.arange(rows.shape[1])[None] < cnt[:, None])).all()) else None


def last_visible(rows: np.ndarray) -> int:
    """bool [B, K] -> the last position any row sees, + 1 (0: nobody sees anything)"""
    pos = np.nonzero(rows.any(axis=0))[0]
    return int(pos[-1]) + 1 if pos.size else 0


class ContextPlan(NamedTuple):
    n_live: np.ndarray                  # int64 [steps]: the context rows handed to the model at each step
    gather: Optional[np.ndarray]        # sorted positions to gather once (MMDiTGPU.gather_context), or None
    words_rows: Optional[np.ndarray]    # bool [1, K] / [B, K] to pack into key-mask words (ops.pack_key_mask), or None
    key: tuple                          # identifies the plan's launches (hipGraph cache)


def context_plan(k_table, K: int, steps: int, prefix_k: Optional[int] = None, pattern=None, batched: bool = False,
                 keep_positions: bool = False) -> ContextPlan:
    """The visibility of every sampler step, resolved once on the host.  Step i may see token j iff j < limit[i] = min(k_table[i] + 1,
    prefix_k) and pattern[j]; `pattern`: None, [K], or [B, K] (bool / 0-1).  Routes (arrays of the result are read-only):
      slice     no pattern: the first n_live = limit rows.
      gather    one pattern for the batch: its visible rows are gathered once, a step takes the n_live of them below its limit.
      in place  one NON-prefix pattern with `keep_positions` (gemm='exact' keeps every key at its position in the reference's key
                sequence -- kv blocks of 512, MKL's K-blocks -- and a gather would move them): rows 0 .. n_live - 1 stay, n_live =
                the last visible position below the limit, + 1, and the attention takes one shared row of words.
      batched   differing rows, `batched`: rows stay, n_live = limit (0 when no sample sees a key below it), per-sample words.
                Without `batched` differing rows are refused: `pattern_groups` splits such a batch first."""
    limit = np.minimum(np.asarray(k_table[:steps], dtype=np.int64) + 1, K if prefix_k is None else int(prefix_k))
    n_live, gather, words = limit, None, None
    rows = None if pattern is None else np.asarray(pattern)
    if rows is not None and rows.ndim == 2 and not rows_uniform(rows):
        if not batched:
            raise NotImplementedError("p_sample_loop takes ONE visibility pattern per call (decode the samples in groups of equal pattern)")
        if keep_positions:
            raise NotImplementedError("gemm='exact' decodes one visibility pattern per sampler call: pass super_mask=tokens.suffix_mask(K, m) without "
                                      "mask_batched (groups of equal pattern), or decode the batch in one pass with gemm='fp32' / 'f16x2'")
        if prefix_k is not None:
            raise ValueError("mask_batched is exclusive with prefix_k")
        if rows.shape[1] != K:
            raise ValueError(f"super_mask has {rows.shape[1]} entries per sample, the tokenizer has K = {K} tokens")
        words = rows != 0
        any_below = np.concatenate([[False], np.cumsum(words.any(axis=0)) > 0])         # any_below[n]: some sample has a visible key < n
        n_live = np.where(any_below[limit], limit, 0)
    elif rows is not None:
        row = (rows[0] if rows.ndim == 2 else rows).reshape(-1) != 0
        if row.size != K:
            raise ValueError(f"super_mask has {row.size} entries, the tokenizer has K = {K} tokens")
        pos = np.nonzero(row)[0].astype(np.int64)
        below = np.searchsorted(pos, limit, side="left")                                # visible positions below each step's limit
        if keep_positions and prefix_lengths(row[None]) is None:
            words, n_live = row[None], np.where(below > 0, pos[np.maximum(below, 1) - 1] + 1, 0)
        else:
            gather, n_live = pos, below
    n_live = n_live.astype(np.int64)
    for a in (n_live, gather, words):
        if a is not None:
            a.setflags(write=False)
    return ContextPlan(n_live, gather, words, (n_live.tobytes(), gather is not None and gather.tobytes(), words is not None and (words.shape, words.tobytes())))


def pattern_groups(pattern, B: int, batched: bool = False):
    """-> [(sample indices, or None: the whole batch; pattern for `context_plan`)].  A [B, K] pattern with differing rows that is not decoded
    as one batch becomes one group per distinct row (samples are independent; a group's context is gathered once)."""
    rows = None if pattern is None else np.asarray(pattern)
    if rows is None or batched or rows.ndim != 2 or rows.shape[0] != B or rows_uniform(rows):
        return [(None, rows)]
    rows, seen = rows.reshape(B, -1) != 0, {}
    for b in range(B):
        seen.setdefault(rows[b].tobytes(), []).append(b)
    return [(idx, rows[idx[0]]) for idx in seen.values()]


def request_pattern(K: int, B: int, prefix_k=None, super_mask=None, ar_partial=None, mask_batched: bool = False):
    """the visibility arguments of `SelftokPipeline.decoding`, checked -> (pattern, mask_batched).  `ar_partial` (an int, or one value per
    sample) is the pattern tokens.suffix_mask(K, m): one [K] row when every m is the same, else [B, K] decoded as one batch."""
    if prefix_k is not None and not (0 <= int(prefix_k) <= K):
        raise ValueError(f"prefix_k must be in [0, {K}]")
    if ar_partial is None:
        return super_mask, mask_batched
    if prefix_k is not None or super_mask is not None:
        raise ValueError("ar_partial is exclusive with prefix_k / super_mask")
    m = np.asarray(ar_partial, dtype=np.int64).reshape(-1)
    m = np.repeat(m, B) if m.size == 1 else m
    if m.size != B:
        raise ValueError(f"ar_partial: expected an int or {B} values, got {m.size}")
    if m.min() < 0 or m.max() > K:
        raise ValueError(f"ar_partial must be in [0, {K}]")
    sm = tokens.suffix_mask(K, m)
    return (sm[0], mask_batched) if bool((m == m[0]).all()) else (sm, True)


# ---- decode stream: which slot is at which sampler step (pipeline.DecodeStream; tests/test_decode_stream_cpu.py) ----
class StreamFull(RuntimeError):
    """`submit` on a stream without a free slot: step the stream (a retirement frees a slot) and submit again"""


class SlotSchedule:
    """The host's mirror of a decode stream: `slots` slots, each idle (step -1) or at sampler step 0 .. n_steps - 1 of its own request.
    Pure host logic.  `limit[i]` = min(k_table[i] + 1, K): the keys a request at step i may see; a request runs n_steps = min(max_steps,
    len(limit)) steps.  Tickets count up from 0 in submit order; a request takes the LOWEST free slot."""
    CONTEXTS = ("live", "full")

    def __init__(self, slots: int, limit, K: int, max_steps: Optional[int] = None, context: str = "live"):
        if int(slots) < 1:
            raise ValueError(f"slots = {slots}: expected at least 1")
        if context not in self.CONTEXTS:
            raise ValueError(f"context {context!r}: expected one of {self.CONTEXTS}")
        self.limit = np.asarray(limit, dtype=np.int64).copy()
        if self.limit.ndim != 1 or self.limit.size < 1 or self.limit.min() < 0 or self.limit.max() > K:
            raise ValueError(f"limit: expected one value in [0, {K}] per step")
        if max_steps is not None and int(max_steps) < 1:
            raise ValueError(f"max_steps = {max_steps}: expected None or at least 1")
        self.slots, self.K, self.context = int(slots), int(K), context
        self.n_steps = self.limit.size if max_steps is None else min(int(max_steps), self.limit.size)
        self.step = [-1] * self.slots            # the device's `step`, mirrored
        self.ticket = [None] * self.slots
        self.first_visible = [None] * self.slots  # lowest position the slot's pattern shows (None: none at all)
        self._next = 0

    @property
    def free_slots(self) -> int:
        return sum(t is None for t in self.ticket)

    @property
    def in_flight(self) -> int:
        return self.slots - self.free_slots

    def active(self):
        """the occupied slots in ticket (= submit) order"""
        return sorted((s for s in range(self.slots) if self.ticket[s] is not None), key=lambda s: self.ticket[s])

    def submit(self, first_visible: Optional[int] = 0):
        """-> (ticket, slot).  `first_visible`: the lowest position of the request's visibility pattern (0 without a pattern; None for an
        empty pattern)"""
        for s in range(self.slots):
            if self.ticket[s] is None:
                self.ticket[s], self.step[s], self.first_visible[s] = self._next, 0, first_visible
                self._next += 1
                return self.ticket[s], s
        raise StreamFull(f"all {self.slots} slots are in flight: step() the stream until a request retires")

    def n_live(self) -> int:
        """context rows of the NEXT step: the largest limit[step] of an occupied slot ('full': K), 0 when no occupied slot sees a key"""
        occ = [s for s in range(self.slots) if self.ticket[s] is not None]
        if not occ:
            return 0
        if self.context == "full":
            return self.K
        sees = any(self.first_visible[s] is not None and self.first_visible[s] < self.limit[self.step[s]] for s in occ)
        return int(max(self.limit[self.step[s]] for s in occ)) if sees else 0

    def advance(self):
        """one stream step has been launched: every occupied slot moves on; -> [(ticket, slot)] of the requests that have now run their
        n_steps steps, in ticket order.  They keep their slots until `retire`."""
        done = []
        for s in self.active():
            self.step[s] += 1
            if self.step[s] >= self.n_steps:
                done.append((self.ticket[s], s))
        return done

    def retire(self, slot: int) -> None:
        self.ticket[slot], self.step[slot], self.first_visible[slot] = None, -1, None

    def restart(self):
        """every occupied slot back to step 0 (the overflow fallback of the split GEMM modes) -> the slots, in ticket order"""
        occ = self.active()
        for s in occ:
            self.step[s] = 0
        return occ
