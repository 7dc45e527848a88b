"""The step that produces the ids: AR logits -> code ids on the device, bit-reproducible (csrc/token_sample.hip, `ops.token_sample`).

An AR image model emits one row of logits per sample and step; `TokenSampler` turns them into the `[B, K]` id matrix that
`SelftokPipeline.decoding(ids, ar_partial=m)` and `DecodeStream.submit(ids, ar_partial=m)` take.  AR step s of a sample lands at tokenizer
position K - 1 - s (tokens.py: the model emits position K - 1 first).  The draw of a sample at a step is a function of (seed, ticket, step)
and that sample's logits alone: the same request gives the same ids alone or in any batch, in any row, run to run, and after a
`state()` / `load_state()` round trip.  Nothing is read back and nothing synchronises: the counters live and advance on the device.

    sampler = TokenSampler(K=512, temperature=1.0, top_k=50, top_p=0.9, cfg_scale=3.0, seed=1234)
    sampler.begin(B)                                   # tickets 0 .. B - 1; pass `tickets=` to name requests yourself
    for s in range(K):
        sampler.step(cond_logits, uncond_logits)       # [B, V] fp32 or bf16, the codes at [offset, offset + C)
        if s % 64 == 63:
            ids, m = sampler.partial()
            preview = pipe.decoding(ids, ar_partial=m)

The teacher-forced side (csrc/token_score.hip, `ops.token_score`): `score_tokens(logits[B, S, V], ids[B, K])` gives a `TokenScore` -- the log-probability,
rank and entropy of every known id under the same arithmetic, and NLL / perplexity / top-k accuracy / per-position NLL over them.

Speculative sampling (csrc/token_verify.hip, `ops.token_verify`): a small model drafts S tokens through a `fork()` of the sampler, the large model scores
S + 1 positions in one forward, `verify()` keeps a prefix of the draft and replaces the first rejected token -- distributed as if the large model had
sampled alone, and with draft logits equal to target logits bit for bit the ids of the plain `step` loop.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import ops as _ops


SpecRound = namedtuple("SpecRound", "n_accept n_emit foreign bad")
SpecRound.__doc__ = """One `TokenSampler.verify` round: n_accept int32 [B] on the device (drafted tokens kept per sequence), n_emit a HOST int64 array [B] (tokens
committed per sequence: the kept drafts plus the replacement or bonus token, capped at K), foreign and bad the sampler's accumulating device counters."""


class TokenSampler:
    """K: tokens per image.  C / offset: the window of image codes inside a logits row.  temperature 0 is greedy; top_k <= 0 and top_p outside (0, 1) are
    off; cfg_scale None means no guidance (`step` then refuses unconditional logits, and demands them otherwise).  seed: 64 bits, the Philox key."""

    def __init__(self, K: int, C: int = 32768, offset: int = 0, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0, cfg_scale: Optional[float] = None,
                 seed: int = 0, *, id_dtype=torch.int64, ops=None):
        if K < 1 or not 1 <= C <= 65536 or offset < 0 or offset % 4:
            raise ValueError(f"need K >= 1, 1 <= C <= 65536 and an offset >= 0 that is a multiple of 4, got K {K}, C {C}, offset {offset}")
        if not (temperature >= 0.0) or temperature == float("inf") or top_p != top_p:
            raise ValueError(f"need a finite temperature >= 0 and a top_p that is a number, got {temperature}, {top_p}")
        if id_dtype not in (torch.int32, torch.int64):
            raise ValueError("id_dtype must be torch.int32 or torch.int64")
        self.K, self.C, self.offset = int(K), int(C), int(offset)
        self.temperature, self.top_k, self.top_p = float(temperature), int(top_k), float(top_p)
        self.cfg_scale = None if cfg_scale is None else float(cfg_scale)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.id_dtype = id_dtype
        self._ops = _ops if ops is None else ops
        self.B = None

    # ---- a batch of requests ----
    def begin(self, B: int, tickets=None, steps=None, device="cuda"):
        """allocate ids / logprob / n_kept [B, K] (ids and n_kept zeroed, logprob NaN) and the counters (ticket, step) [B, 2].  tickets: one 32-bit number per
        row, default 0 .. B - 1 -- the identity of a request: its draws do not depend on the row it sits in.  steps: the AR step each row starts at, default 0;
        rows at different steps share every call through a per-row write position."""
        B = int(B)
        tickets = np.arange(B, dtype=np.int64) if tickets is None else np.asarray(tickets, dtype=np.int64).reshape(-1)
        steps = np.zeros(B, dtype=np.int64) if steps is None else np.asarray(steps, dtype=np.int64).reshape(-1)
        if tickets.shape != (B,) or steps.shape != (B,) or (B and (tickets.min() < 0 or tickets.max() > 0xFFFFFFFF or steps.min() < 0 or steps.max() > self.K)):
            raise ValueError(f"need {B} tickets in [0, 2^32) and {B} steps in [0, K]")
        self.B = B
        self._steps = steps.copy()                                  # host mirror: the device never has to be asked
        self._ticket_host, self._fork_steps = tickets.copy(), None
        ctr = np.stack([tickets, steps], axis=1).astype(np.uint32).view(np.int32)
        self.ctr = torch.from_numpy(ctr.copy()).to(device)
        self.ids = torch.zeros(B, self.K, dtype=self.id_dtype, device=device)
        self.logprob = torch.full((B, self.K), float("nan"), dtype=torch.float32, device=device)
        self.n_kept = torch.zeros(B, self.K, dtype=torch.int32, device=device)
        self.bad = torch.zeros(1, dtype=torch.int32, device=device)
        self.foreign = torch.zeros(1, dtype=torch.int32, device=device)   # drafted ids the draft distribution could not have drawn (verify)
        self._row_lp = torch.empty(B, dtype=torch.float32, device=device)
        self._row_nk = torch.empty(B, dtype=torch.int32, device=device)
        self._row_mass = torch.empty(B, 3, dtype=torch.int64, device=device)
        return self

    def _uniform(self) -> bool:
        return self.B == 0 or bool((self._steps == self._steps[0]).all())

    def step(self, logits: torch.Tensor, uncond_logits: Optional[torch.Tensor] = None):
        """sample the next AR step of every row: row b's id goes to tokenizer position K - 1 - step_b, its log-probability and kept count beside it, and the
        counters advance on the device.  Reads nothing back."""
        if self.B is None:
            raise RuntimeError("TokenSampler.step before begin")
        if (uncond_logits is None) != (self.cfg_scale is None):
            raise ValueError("unconditional logits go with a cfg_scale: pass both or neither")
        if self.B and int(self._steps.max()) >= self.K:
            raise RuntimeError(f"a row already holds its K = {self.K} tokens")
        kw = dict(uncond_logits=uncond_logits, C=self.C, offset=self.offset, cfg_scale=1.0 if self.cfg_scale is None else self.cfg_scale,
                  temperature=self.temperature, top_k=self.top_k, top_p=self.top_p, seed=self.seed, n_kept=self._row_nk, mass=self._row_mass,
                  logprob=self._row_lp, bad=self.bad)
        if self._uniform():
            col = self.K - 1 - int(self._steps[0]) if self.B else 0
            self._ops.token_sample(logits, self.ctr, self.ids, col=col, **kw)
            self.logprob[:, col].copy_(self._row_lp)
            self.n_kept[:, col].copy_(self._row_nk)
        else:
            pos = (self.K - 1) - self.ctr[:, 1]                     # int32, on the device
            self._ops.token_sample(logits, self.ctr, self.ids, pos=pos, **kw)
            p64 = pos.to(torch.int64).unsqueeze(1)
            self.logprob.scatter_(1, p64, self._row_lp.unsqueeze(1))
            self.n_kept.scatter_(1, p64, self._row_nk.unsqueeze(1))
        self.ctr[:, 1] += 1
        self._steps += 1
        return self

    def partial(self):
        """(ids [B, K], m): the arguments of `SelftokPipeline.decoding(ids, ar_partial=m)` and `DecodeStream.submit(ids[b], ar_partial=m_b)`; m is an int when
        every row is at the same step, else one value per row"""
        if self.B is None:
            raise RuntimeError("TokenSampler.partial before begin")
        return self.ids, (int(self._steps[0]) if self.B and self._uniform() else self._steps.copy())

    # ---- speculative sampling: draft through a fork, verify here ----
    def fork(self, cfg_scale="same") -> "TokenSampler":
        """a DRAFT sampler: the same parameters, seed and tickets, the device counters copied as they stand, its own [B, K] matrices.  The drafter runs
        ordinary `step` calls on it; `drafted()` then hands over what it drew.  cfg_scale: the draft side's own guidance rule (None: an unguided student,
        the usual product of distilling the guided distribution); by default this sampler's.  Reads nothing back: the host mirror of the steps is copied
        from this sampler's."""
        if self.B is None:
            raise RuntimeError("TokenSampler.fork before begin")
        d = TokenSampler(self.K, self.C, self.offset, self.temperature, self.top_k, self.top_p, self.cfg_scale if cfg_scale == "same" else cfg_scale, self.seed,
                         id_dtype=self.id_dtype, ops=self._ops)
        d.begin(self.B, tickets=self._ticket_host, steps=self._steps, device=self.ctr.device)
        d.ctr.copy_(self.ctr)
        d._fork_steps = self._steps.copy()
        return d

    def drafted(self):
        """on a fork: (draft_ids [B, S] in AR order, n_draft host int64 [B]) -- the ids drawn since the fork, S the largest count, -1 past a row's own"""
        if getattr(self, "_fork_steps", None) is None:
            raise RuntimeError("TokenSampler.drafted: not a fork")
        n = self._steps - self._fork_steps
        S = int(n.max()) if self.B else 0
        if S == 0:
            return torch.empty(self.B, 0, dtype=self.id_dtype, device=self.ids.device), n
        pos = (self.K - 1) - (torch.from_numpy(self._fork_steps).to(self.ids.device, non_blocking=True).unsqueeze(1) + torch.arange(S, device=self.ids.device))
        live = torch.from_numpy(n).to(self.ids.device, non_blocking=True).unsqueeze(1) > torch.arange(S, device=self.ids.device)
        x = torch.gather(self.ids, 1, pos.clamp_(0, self.K - 1))
        return torch.where(live, x, torch.full_like(x, -1)), n

    def _read_back(self, t: torch.Tensor) -> np.ndarray:
        return t.cpu().numpy()

    def verify(self, draft_ids: torch.Tensor, draft_logits: Optional[torch.Tensor], target_logits: torch.Tensor, *, draft_uncond: Optional[torch.Tensor] = None,
               target_uncond: Optional[torch.Tensor] = None, draft_cfg_scale: Optional[float] = None, n_draft=None) -> SpecRound:
        """One round of speculative sampling.  draft_ids [B, S] (AR order: what a `fork()` drew, see `drafted`), draft_logits [B, S, V] the logits they were
        drawn from, target_logits [B, S + 1, V] this model's logits at the same S positions and one more; S = 0 (draft_logits None) is one plain step.
        target_uncond goes with this sampler's cfg_scale, draft_uncond with draft_cfg_scale, both or neither on each side.  n_draft: host counts <= S for
        rows that drafted fewer.  Per sequence the longest accepted prefix, then the replacement of the first rejected token (or, when every draft was
        kept, one more token from the last target row) are written into ids / logprob / n_kept at their tokenizer positions, and the device counters
        advance by the number emitted, which stops at K.

        THE ONE READ-BACK: after the two launches `n_emit` (B int32 values) is copied to the host, once, the only device -> host copy of a round; the
        caller needs these counts anyway to crop its KV caches.  It refreshes the host mirror of the steps, so `step`, `partial`, `state` and
        `load_state` keep working afterwards -- rows are then at different steps, which every one of them supports."""
        if self.B is None:
            raise RuntimeError("TokenSampler.verify before begin")
        if (target_uncond is None) != (self.cfg_scale is None):
            raise ValueError("unconditional target logits go with a cfg_scale: pass both or neither")
        if (draft_uncond is None) != (draft_cfg_scale is None):
            raise ValueError("unconditional draft logits go with a draft_cfg_scale: pass both or neither")
        out = self._ops.token_verify(target_logits, draft_logits, draft_ids, self.ctr, self.ids, self.logprob, self.n_kept, target_uncond=target_uncond,
                                     draft_uncond=draft_uncond, C=self.C, offset=self.offset, cfg_scale=1.0 if self.cfg_scale is None else self.cfg_scale,
                                     draft_cfg_scale=1.0 if draft_cfg_scale is None else float(draft_cfg_scale), temperature=self.temperature,
                                     top_k=self.top_k, top_p=self.top_p, seed=self.seed, n_draft=n_draft, foreign=self.foreign, bad=self.bad)
        n_emit = self._read_back(out.n_emit).astype(np.int64)
        self._steps = self._steps + n_emit
        return SpecRound(out.n_accept, n_emit, self.foreign, self.bad)

    # ---- resumable requests ----
    def state(self) -> dict:
        """everything a later `load_state` needs to continue bit for bit (one device -> host copy: not for the inner loop)"""
        if self.B is None:
            raise RuntimeError("TokenSampler.state before begin")
        return {"K": self.K, "C": self.C, "offset": self.offset, "temperature": self.temperature, "top_k": self.top_k, "top_p": self.top_p,
                "cfg_scale": self.cfg_scale, "seed": self.seed, "id_dtype": str(self.id_dtype).replace("torch.", ""),
                "ctr": self.ctr.cpu().numpy().view(np.uint32).copy(), "steps": self._steps.copy(), "ids": self.ids.cpu().numpy().copy(),
                "logprob": self.logprob.cpu().numpy().copy(), "n_kept": self.n_kept.cpu().numpy().copy(), "bad": int(self.bad.cpu()[0])}

    def load_state(self, st: dict, device="cuda"):
        for name in ("K", "C", "offset", "temperature", "top_k", "top_p", "cfg_scale", "seed"):
            if st[name] != getattr(self, name):
                raise ValueError(f"state was saved with {name} = {st[name]!r}, this sampler has {getattr(self, name)!r}")
        ctr = np.asarray(st["ctr"], dtype=np.uint32)
        self.begin(ctr.shape[0], tickets=ctr[:, 0], steps=np.asarray(st["steps"]), device=device)
        if not np.array_equal(ctr[:, 1].astype(np.int64), self._steps):
            raise ValueError("state: the counters' step words and `steps` differ")
        self.ids.copy_(torch.from_numpy(np.asarray(st["ids"])).to(self.id_dtype))
        self.logprob.copy_(torch.from_numpy(np.asarray(st["logprob"], dtype=np.float32)))
        self.n_kept.copy_(torch.from_numpy(np.asarray(st["n_kept"], dtype=np.int32)))
        self.bad.fill_(int(st["bad"]))
        return self


# ---- the teacher-forced side: what did the model give ids that are already known? (csrc/token_score.hip, `ops.token_score`) ----
class TokenScore:
    """The device tensors of one `score_tokens` call, [B, S] each (mass [B, S, 2] holds the uint64 (Q_total, q_t) in int64), the two counters, and
    `positions` [S]: the tokenizer position column s was scored against.  The reductions below are torch fp64 on the device and return 0-d / 1-d fp64
    tensors; they leave out ignored rows (rank -1) and REFUSE to summarise while bad > 0 (one read-back) unless allow_bad=True, which leaves bad rows
    out as well."""

    def __init__(self, logprob, mass, rank, top_id, entropy, bad, ignored, positions, K):
        self.logprob, self.mass, self.rank, self.top_id, self.entropy, self.bad, self.ignored = logprob, mass, rank, top_id, entropy, bad, ignored
        self.positions, self.K = np.asarray(positions, dtype=np.int64), int(K)

    def _scored(self, allow_bad: bool) -> torch.Tensor:
        n_bad = int(self.bad.reshape(-1)[0])
        if n_bad > 0 and not allow_bad:
            raise ValueError(f"{n_bad} bad rows (NaN / +inf / all -inf logits, or a target outside the window): pass allow_bad=True to summarise the rest")
        return self.rank >= 0                                        # ignored and bad rows both carry rank -1

    def _lp(self, ok):
        return torch.where(ok, self.logprob.double(), torch.zeros((), dtype=torch.float64, device=self.logprob.device))

    def sequence_logprob(self, allow_bad: bool = False) -> torch.Tensor:
        """[B]: the sum of the scored rows' log-probabilities per sequence"""
        return self._lp(self._scored(allow_bad)).sum(dim=1)

    def nll(self, allow_bad: bool = False) -> torch.Tensor:
        """the mean negative log-probability per scored token (NaN when none was scored)"""
        ok = self._scored(allow_bad)
        return -self._lp(ok).sum() / ok.sum().double()

    def perplexity(self, allow_bad: bool = False) -> torch.Tensor:
        return torch.exp(self.nll(allow_bad))

    def per_position_nll(self, allow_bad: bool = False) -> torch.Tensor:
        """[K], indexed by TOKENIZER position; NaN where no row was scored"""
        ok = self._scored(allow_bad)
        col = -self._lp(ok).sum(dim=0) / ok.sum(dim=0).double()
        out = torch.full((self.K,), float("nan"), dtype=torch.float64, device=col.device)
        out[torch.from_numpy(self.positions).to(col.device)] = col
        return out

    def topk_accuracy(self, k: int = 1, allow_bad: bool = False) -> torch.Tensor:
        """the share of scored rows whose target sits at rank < k"""
        ok = self._scored(allow_bad)
        return (ok & (self.rank < int(k))).sum().double() / ok.sum().double()

    def mean_rank(self, allow_bad: bool = False) -> torch.Tensor:
        ok = self._scored(allow_bad)
        return torch.where(ok, self.rank, torch.zeros_like(self.rank)).double().sum() / ok.sum().double()

    def mean_entropy(self, allow_bad: bool = False) -> torch.Tensor:
        ok = self._scored(allow_bad)
        return torch.where(ok, self.entropy.double(), torch.zeros((), dtype=torch.float64, device=self.entropy.device)).sum() / ok.sum().double()


def target_view(ids: torch.Tensor, S: int, ar_order: bool, steps):
    """How S rows of logits meet ids [B, K] in tokenizer order (shared by `score_tokens` and `losses.token_cross_entropy`) -> (view [B, S], reverse, positions
    [S]).  ar_order=True: row s is AR step s and meets tokenizer position K - 1 - s; the view is the last S columns, in tokenizer order, to be walked backwards
    (reverse=True) -- nothing is flipped or copied.  ar_order=False: row s meets position s.  steps (an int or one count per sequence): rows at or past a
    sequence's count get the target -1; this builds one [B, S] tensor in row order (reverse=False)."""
    B, K = ids.shape
    positions = (K - 1 - np.arange(S)) if ar_order else np.arange(S)
    view = ids[:, K - S:] if ar_order else ids[:, :S]               # [B, S] in tokenizer order; reverse_steps walks it backwards
    reverse = bool(ar_order)
    if steps is not None:
        st = torch.as_tensor(np.broadcast_to(np.asarray(steps, dtype=np.int64).reshape(-1), (B,)).copy(), device=ids.device)
        tgt = view.flip(1) if reverse else view                     # row order
        live = torch.arange(S, device=ids.device).unsqueeze(0) < st.unsqueeze(1)
        view, reverse = torch.where(live, tgt, torch.full_like(tgt, -1)), False
    return view, reverse, positions


def score_tokens(logits: torch.Tensor, ids: torch.Tensor, *, ar_order: bool = True, steps=None, uncond_logits: Optional[torch.Tensor] = None,
                 C: Optional[int] = None, offset: int = 0, cfg_scale: Optional[float] = None, temperature: float = 1.0, ops=None) -> TokenScore:
    """logits [B, S, V] (fp32 or bf16) the model produced for the KNOWN ids [B, K] (int32 / int64, tokenizer order, any column stride), S <= K.
    ar_order=True: logits row s is AR step s and scores tokenizer position K - 1 - s, so the S steps are positions K - S .. K - 1 -- the ids and step count
    of `TokenSampler.partial()` go in as they are, and nothing is flipped or copied.  ar_order=False: row s scores position s.  steps: an int or one count
    per sequence, as partial()'s m: rows at or past a sequence's count are IGNORED (this builds one [B, S] id tensor; ids that are negative already are
    ignored without it).  cfg_scale goes with uncond_logits, both or neither.  Reads nothing back."""
    o = _ops if ops is None else ops
    if logits.dim() != 3 or ids.dim() != 2 or ids.shape[0] != logits.shape[0] or logits.shape[1] > ids.shape[1]:
        raise ValueError(f"need logits [B, S, V] and ids [B, K] with S <= K, got {tuple(logits.shape)} and {tuple(ids.shape)}")
    if (uncond_logits is None) != (cfg_scale is None):
        raise ValueError("unconditional logits go with a cfg_scale: pass both or neither")
    K = ids.shape[1]
    view, reverse, positions = target_view(ids, logits.shape[1], ar_order, steps)
    out = o.token_score(logits, view, uncond_logits=uncond_logits, C=C, offset=offset, cfg_scale=1.0 if cfg_scale is None else float(cfg_scale),
                        temperature=float(temperature), reverse_steps=reverse)
    return TokenScore(*out, positions=positions, K=K)


# ---- how far apart are two next-token distributions? (csrc/token_distill.hip without its gradient, `ops.token_distill(want_grad=False)`) ----
class TokenKL(namedtuple("TokenKL", "kl ce entropy_p bad ignored")):
    """The device tensors of one `token_kl` call: kl = KL(p || q), ce = -sum p log q and entropy_p = -sum p log p, fp32 [B, S] each, and the two counters.
    `live` ([B, S] bool or None) and `positions` ([S]: the tokenizer position column s stands for) ride along as attributes.  The reductions are torch fp64
    on the device; they leave out ignored rows and REFUSE to summarise while bad > 0 (one read-back) unless allow_bad=True, which leaves bad rows out too."""

    def _ok(self, allow_bad: bool) -> torch.Tensor:
        n_bad = int(self.bad.reshape(-1)[0])
        if n_bad > 0 and not allow_bad:
            raise ValueError(f"{n_bad} bad rows (NaN / +inf / all -inf logits): pass allow_bad=True to summarise the rest")
        ok = ~torch.isnan(self.kl)
        return ok if self.live is None else ok & self.live

    def mean(self, field: str = "kl", allow_bad: bool = False) -> torch.Tensor:
        """the mean of `field` over the live rows, 0-d fp64"""
        ok = self._ok(allow_bad)
        return torch.where(ok, getattr(self, field).double(), torch.zeros((), dtype=torch.float64, device=self.kl.device)).sum() / ok.sum().double()

    def per_position(self, field: str = "kl", allow_bad: bool = False) -> torch.Tensor:
        """[S] fp64, indexed by TOKENIZER position; NaN where no row was live"""
        ok = self._ok(allow_bad)
        col = torch.where(ok, getattr(self, field).double(), torch.zeros((), dtype=torch.float64, device=self.kl.device)).sum(dim=0) / ok.sum(dim=0).double()
        out = torch.full((len(self.positions),), float("nan"), dtype=torch.float64, device=col.device)
        out[torch.from_numpy(np.asarray(self.positions, dtype=np.int64)).to(col.device)] = col
        return out


def token_kl(logits_p: torch.Tensor, logits_q: torch.Tensor, *, uncond_p: Optional[torch.Tensor] = None, cfg_scale: float = 1.0, ar_order: bool = True, steps=None,
             C: Optional[int] = None, offset: int = 0, ops=None) -> TokenKL:
    """KL(p || q) per row between two next-token distributions given as logits [B, S, V] (fp32 or bf16 each, on their own), over the window
    [offset, offset + C): how far guidance (`uncond_p` with `cfg_scale`: p is the guided `lu + s (lc - lu)`), a fine-tune or a quantised model moves the
    distribution.  ar_order and steps as in `score_tokens`: rows at or past a sequence's step count are ignored.  No gradient is written and nothing is read
    back."""
    o = _ops if ops is None else ops
    if logits_p.dim() != 3 or logits_q.shape != logits_p.shape:
        raise ValueError(f"need two logits tensors of one shape [B, S, V], got {tuple(logits_p.shape)} and {tuple(logits_q.shape)}")
    if uncond_p is None and float(cfg_scale) != 1.0:
        raise ValueError("a cfg_scale goes with uncond_p")
    B, S, _ = logits_p.shape
    positions = (S - 1 - np.arange(S)) if ar_order else np.arange(S)
    live = None
    if steps is not None:
        view, reverse, _ = target_view(torch.zeros((B, S), dtype=torch.int32, device=logits_p.device), S, ar_order, steps)
        live = (view.flip(1) if reverse else view) >= 0
    kl, ce, h, _, _, bad, ignored = o.token_distill(logits_q, logits_p, teacher_uncond=uncond_p, cfg_scale=float(cfg_scale), C=C, offset=offset,
                                                    row_mask=None if live is None else live.to(torch.uint8).contiguous(), want_grad=False)
    out = TokenKL(kl, ce, h, bad, ignored)
    out.live, out.positions = live, positions
    return out
