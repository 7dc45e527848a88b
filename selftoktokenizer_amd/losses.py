"""The training losses over image tokens.  Supervised: cross-entropy of known ids under AR logits, with its gradient, in ONE launch of csrc/token_xent.hip
(`ops.token_xent`; include/selftok_hip_ext.h states the arithmetic).  The forward pass writes `softmax - onehot`, already scaled by each row's share of
the reduction, so the backward pass is one multiplication by the upstream gradient; with inplace=True that gradient is written over the logits and the loss
costs one read and one write of them and no buffer of their size.  `token_distillation` (csrc/token_distill.hip) and, for reinforcement learning on sampled
ids, `token_policy_loss` with `group_advantages` (csrc/token_policy.hip: the clipped PPO / GRPO surrogate, a k3 KL penalty, an entropy bonus) work the same way."""
from collections import namedtuple
from typing import Optional

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import ops as _ops
from .sampling import target_view

XentStats = namedtuple("XentStats", "nll lse bad ignored")
REDUCTIONS = ("mean", "sum", "none")


class _TokenXent(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, view, reverse, w, C, offset, z, reduction, inplace, o):
        B, S = logits.shape[0], logits.shape[1]
        dev = logits.device
        tgt = view.flip(1) if reverse else view                     # [B, S] in row order: which rows are scored (B * S ids, not B * S * V logits)
        scored = tgt >= 0
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        wd = None if w is None else w.double()
        if reduction == "mean":                                     # the weight of the scored rows, counted on the device: nothing is read back
            denom = scored.sum().double() if wd is None else torch.where(scored, wd, zero).sum()
            scale = ((1.0 / denom) if wd is None else (wd / denom)).float().expand(B, S).contiguous()
        else:
            denom = None
            scale = None if w is None else w.float().expand(B, S).contiguous()
        nll, lse, grad, bad, ignored = o.token_xent(logits, view, C=C, offset=offset, z_coef=z, row_scale=scale, inplace=inplace, reverse_steps=reverse)
        rows = nll.double() + z * lse.double() * lse.double() if z else nll.double()
        rows = torch.where(scored, rows if wd is None else rows * wd, zero)        # an ignored row has nll 0 but an lse; a bad row keeps its NaN
        if reduction == "none":
            loss = rows.float()
        elif reduction == "sum":
            loss = rows.sum().float()
        else:
            loss = (rows.sum() / denom).float()
        ctx.buf, ctx.per_row = grad, reduction == "none"
        if inplace and hasattr(torch.autograd.graph, "increment_version"):
            torch.autograd.graph.increment_version(logits)         # whoever saved the logits for its own backward must hear that they are gone
        ctx.mark_non_differentiable(nll, lse, bad, ignored)
        return loss, nll, lse, bad, ignored

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, *_):
        buf = ctx.buf
        if buf is None:
            raise RuntimeError("token_cross_entropy: backward a second time: the gradient buffer was scaled by the first upstream gradient and handed over "
                               "(run the forward pass again)")
        ctx.buf = None
        buf.mul_(g_loss.unsqueeze(-1) if ctx.per_row else g_loss)
        return (buf,) + (None,) * 9


def token_cross_entropy(logits: torch.Tensor, ids: torch.Tensor, *, ar_order: bool = True, steps=None, C: Optional[int] = None, offset: int = 0,
                        z_loss: float = 0.0, weights: Optional[torch.Tensor] = None, reduction: str = "mean", inplace: bool = False,
                        return_stats: bool = False, ops=None):
    """Cross-entropy of the KNOWN ids [B, K] (int32 / int64, tokenizer order) under logits [B, S, V] (fp32 or bf16, S <= K) over the window
    [offset, offset + C) of each row (default: the rest of the row), plus z_loss * logsumexp^2 per row, differentiable with respect to `logits`.
    ar_order and steps mean what they mean in `sampling.score_tokens`: ar_order=True lets row s be AR step s and meet tokenizer position K - 1 - s without a
    flipped copy; rows at or past a sequence's step count, and ids that are negative already, are IGNORED: no loss, a zero gradient row.
    weights: [K], indexed by TOKENIZER position, or [B, S], one per row of `logits`.  reduction: "mean" (sum of w * loss over sum of w, over the scored
    rows), "sum" or "none" ([B, S], 0 on ignored rows).  The gradient is computed IN THE FORWARD LAUNCH, scaled per row on the device (the count of scored
    rows included: nothing is read back); `loss.backward()` multiplies that buffer by the upstream gradient and hands it to `logits.grad`.  One backward per
    forward; double backward is refused.  inplace=True writes the gradient OVER `logits` and allocates nothing of their size: THE LOGITS ARE GONE AFTERWARDS,
    so whatever else needs their values (another loss, a metric, an operation that saved them for its own backward) must come first or do without.
    A row with a NaN / +inf / all -inf window or an id >= C is BAD: its loss is NaN -- so "mean" and "sum" are NaN -- and its gradient row is zero.
    The scalar is formed from nll and lse in fp64 on the device and returned as fp32.  return_stats=True: -> (loss, XentStats(nll [B, S], lse [B, S], bad [1],
    ignored [1])), device tensors."""
    o = _ops if ops is None else ops
    if logits.dim() != 3 or ids.dim() != 2 or ids.shape[0] != logits.shape[0] or logits.shape[1] > ids.shape[1]:
        raise ValueError(f"need logits [B, S, V] and ids [B, K] with S <= K, got {tuple(logits.shape)} and {tuple(ids.shape)}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    z = float(z_loss)
    if not (z >= 0.0 and z != float("inf")):
        raise ValueError(f"need a finite z_loss >= 0, got {z_loss}")
    B, S, _ = logits.shape
    K = ids.shape[1]
    view, reverse, positions = target_view(ids, S, ar_order, steps)
    w = None
    if weights is not None:
        if tuple(weights.shape) == (K,):
            w = weights.index_select(0, torch.as_tensor(positions, device=weights.device)).unsqueeze(0)      # [1, S]: the weight of the position row s meets
        elif tuple(weights.shape) == (B, S):
            w = weights
        else:
            raise ValueError(f"weights must be [K] = [{K}] by tokenizer position or [B, S] = [{B}, {S}] by row, got {tuple(weights.shape)}")
        w = w.detach()
    loss, nll, lse, bad, ignored = _TokenXent.apply(logits, view, reverse, w, C, int(offset), z, reduction, bool(inplace), o)
    return (loss, XentStats(nll, lse, bad, ignored)) if return_stats else loss


# ---- distillation: KL(teacher || student) over the whole window, csrc/token_distill.hip through `ops.token_distill` ----
DistillStats = namedtuple("DistillStats", "kl ce h_teacher lse bad ignored")


class _TokenDistill(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, uncond, s, live, w, C, offset, reduction, inplace, o):
        B, S = student.shape[0], student.shape[1]
        dev = student.device
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        wd = None if w is None else w.double()
        mask = None if live is None else live.to(torch.uint8).contiguous()
        if reduction == "mean":                                     # the weight of the live rows, counted on the device: nothing is read back
            if live is None:
                denom = torch.full((), float(B * S), dtype=torch.float64, device=dev) if wd is None else wd.expand(B, S).sum()
            else:
                denom = live.sum().double() if wd is None else torch.where(live, wd, zero).sum()
            scale = ((1.0 / denom) if wd is None else (wd / denom)).float().expand(B, S).contiguous()
        else:
            denom = None
            scale = None if w is None else w.float().expand(B, S).contiguous()
        kl, ce, h, lse, grad, bad, ignored = o.token_distill(student, teacher, teacher_uncond=uncond, cfg_scale=s, C=C, offset=offset, row_scale=scale, row_mask=mask,
                                                             inplace=inplace)
        rows = kl.double() if wd is None else kl.double() * wd      # an ignored row has kl 0; a bad row keeps its NaN
        if live is not None:
            rows = torch.where(live, rows, zero)
        if reduction == "none":
            loss = rows.float()
        elif reduction == "sum":
            loss = rows.sum().float()
        else:
            loss = (rows.sum() / denom).float()
        ctx.buf, ctx.per_row = grad, reduction == "none"
        if inplace and hasattr(torch.autograd.graph, "increment_version"):
            torch.autograd.graph.increment_version(student)        # whoever saved the logits for its own backward must hear that they are gone
        ctx.mark_non_differentiable(kl, ce, h, lse, bad, ignored)
        return loss, kl, ce, h, lse, bad, ignored

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, *_):
        buf = ctx.buf
        if buf is None:
            raise RuntimeError("token_distillation: backward a second time: the gradient buffer was scaled by the first upstream gradient and handed over "
                               "(run the forward pass again)")
        ctx.buf = None
        buf.mul_(g_loss.unsqueeze(-1) if ctx.per_row else g_loss)
        return (buf,) + (None,) * 10


def token_distillation(student_logits: torch.Tensor, teacher_logits: torch.Tensor, *, teacher_uncond: Optional[torch.Tensor] = None, cfg_scale: float = 1.0,
                       steps=None, ar_order: bool = True, weights: Optional[torch.Tensor] = None, reduction: str = "mean", C: Optional[int] = None, offset: int = 0,
                       inplace: bool = False, return_stats: bool = False, ops=None):
    """KL(teacher || student) between two full next-token distributions over the window [offset, offset + C) of each row, differentiable with respect to
    `student_logits` [B, S, V] (fp32 or bf16).  `teacher_logits` has the same shape and its own dtype; with `teacher_uncond` the teacher is the guided
    distribution `lu + cfg_scale * (lc - lu)` the sampler draws from, never materialised.  The teacher receives no gradient.  steps and ar_order mean what
    they mean in `token_cross_entropy`: rows at or past a sequence's step count are IGNORED (no loss, a zero gradient row, none of their logits read).
    weights: [S] by TOKENIZER position (row s meets position S - 1 - s when ar_order) or [B, S] by row.  reduction: "mean" (sum of w * kl over sum of w, over
    the live rows), "sum" or "none" ([B, S], 0 on ignored rows).  The gradient is computed IN THE FORWARD LAUNCH, scaled per row on the device; `loss.backward()`
    multiplies that buffer by the upstream gradient.  One backward per forward; double backward is refused.  inplace=True writes the gradient OVER
    `student_logits`: THE LOGITS ARE GONE AFTERWARDS.  A bad row makes "mean" and "sum" NaN and has a zero gradient row.  return_stats=True: -> (loss,
    DistillStats(kl, ce, h_teacher, lse [B, S] each, bad [1], ignored [1])), device tensors."""
    o = _ops if ops is None else ops
    if student_logits.dim() != 3 or teacher_logits.shape != student_logits.shape:
        raise ValueError(f"need student and teacher logits of one shape [B, S, V], got {tuple(student_logits.shape)} and {tuple(teacher_logits.shape)}")
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    if teacher_uncond is None and float(cfg_scale) != 1.0:
        raise ValueError("a cfg_scale goes with teacher_uncond")
    B, S, _ = student_logits.shape
    live = None
    positions = (S - 1 - torch.arange(S)) if ar_order else torch.arange(S)
    if steps is not None:                                           # the scorer's rule for partial sequences, on placeholder ids: target -1 = ignored
        view, reverse, _ = target_view(torch.zeros((B, S), dtype=torch.int32, device=student_logits.device), S, ar_order, steps)
        live = (view.flip(1) if reverse else view) >= 0
    w = None
    if weights is not None:
        if tuple(weights.shape) == (S,):
            w = weights.index_select(0, positions.to(weights.device)).unsqueeze(0)
        elif tuple(weights.shape) == (B, S):
            w = weights
        else:
            raise ValueError(f"weights must be [S] = [{S}] by tokenizer position or [B, S] = [{B}, {S}] by row, got {tuple(weights.shape)}")
        w = w.detach()
    unc = None if teacher_uncond is None else teacher_uncond.detach()
    loss, kl, ce, h, lse, bad, ignored = _TokenDistill.apply(student_logits, teacher_logits.detach(), unc, float(cfg_scale), live, w, C, int(offset), reduction,
                                                             bool(inplace), o)
    return (loss, DistillStats(kl, ce, h, lse, bad, ignored)) if return_stats else loss


# ---- reinforcement learning: the clipped PPO / GRPO surrogate on sampled ids, csrc/token_policy.hip through `ops.token_policy` ----
PolicyStats = namedtuple("PolicyStats", "logprob ratio kl entropy coef flags clip_frac bad ignored")
POLICY_REDUCTIONS = ("mean", "seq_mean", "sum", "none")


class _TokenPolicy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, view, reverse, old, adv, ref, w, clip, kl_coef, ent_coef, C, offset, reduction, inplace, want_entropy, o):
        B, S = logits.shape[0], logits.shape[1]
        dev = logits.device
        tgt = view.flip(1) if reverse else view                     # [B, S] in row order: which rows are scored
        scored = tgt >= 0
        zero = torch.zeros((), dtype=torch.float64, device=dev)
        wd = torch.ones((), dtype=torch.float64, device=dev).expand(B, S) if w is None else w.double().expand(B, S)
        live_w = torch.where(scored, wd, zero)                      # the weight of the scored rows, counted on the device: nothing is read back
        nonzero = lambda x: torch.where(x != 0, x, torch.ones_like(x))      # a batch (a sequence) without a scored row: its rows are all ignored, the loss is 0
        if reduction == "mean":
            share = wd / nonzero(live_w.sum())
        elif reduction == "seq_mean":                               # the mean over each sequence's scored rows, then over the sequences that have any
            share = wd / (nonzero(live_w.sum(1, keepdim=True)) * nonzero((scored.any(1)).sum().double()))
        else:
            share = wd
        scale = None if (w is None and reduction in ("sum", "none")) else share.float().contiguous()
        out = o.token_policy(logits, view, old, adv, ref_logprob=ref, clip=clip, kl_coef=kl_coef, ent_coef=ent_coef, C=C, offset=offset, row_scale=scale,
                             inplace=inplace, reverse_steps=reverse, want_entropy=want_entropy)
        lo, hi = float(np.float32(1.0) - np.float32(clip[0])), float(np.float32(1.0) + np.float32(clip[1]))       # the kernel's fp32 bounds
        a64, r64 = adv.reshape(B, S).double(), out.ratio.double()
        surrogate = torch.where((out.flags & 1) != 0, hi * a64, torch.where((out.flags & 2) != 0, lo * a64, torch.where(a64 == 0, zero, r64 * a64)))
        rows = -surrogate
        if kl_coef:
            rows = rows + kl_coef * out.kl.double()
        if ent_coef:
            rows = rows - ent_coef * out.entropy.double()
        rows = torch.where(scored, rows * share, zero)              # an ignored row has +0 outputs; a bad row keeps its NaN
        loss = rows.float() if reduction == "none" else rows.sum().float()
        n_scored = scored.sum().double()
        clip_frac = (((out.flags != 0) & scored).sum().double() / torch.where(n_scored != 0, n_scored, torch.ones_like(n_scored))).float().reshape(1)
        ctx.buf, ctx.per_row = out.grad, reduction == "none"
        if inplace and hasattr(torch.autograd.graph, "increment_version"):
            torch.autograd.graph.increment_version(logits)         # whoever saved the logits for its own backward must hear that they are gone
        entropy = out.entropy if out.entropy is not None else torch.zeros((), device=dev)
        ctx.mark_non_differentiable(out.logprob, out.ratio, out.kl, entropy, out.coef, out.flags, clip_frac, out.bad, out.ignored)
        ctx.has_entropy = out.entropy is not None
        return loss, out.logprob, out.ratio, out.kl, entropy, out.coef, out.flags, clip_frac, out.bad, out.ignored

    @staticmethod
    @once_differentiable
    def backward(ctx, g_loss, *_):
        buf = ctx.buf
        if buf is None:
            raise RuntimeError("token_policy_loss: backward a second time: the gradient buffer was scaled by the first upstream gradient and handed over "
                               "(run the forward pass again)")
        ctx.buf = None
        buf.mul_(g_loss.unsqueeze(-1) if ctx.per_row else g_loss)
        return (buf,) + (None,) * 15


def _rows_of_logprob(name, t, B, S, K, positions, layout):
    """a roll-out's log-probabilities as contiguous fp32 [B, S] in row order: [B, S] already so, or [B, K] by tokenizer position (`TokenSampler.logprob`)"""
    if t is None:
        return None
    same_order = S == K and bool((positions == np.arange(S)).all())
    if layout is None:
        if tuple(t.shape) == (B, K) and (S != K or same_order):
            layout = "tokens"
        elif tuple(t.shape) == (B, S) and S != K:
            layout = "rows"
        elif tuple(t.shape) == (B, S):
            raise ValueError(f"{name} {tuple(t.shape)} is both [B, S] and [B, K] and the two orders differ: pass logprob_layout='rows' or 'tokens'")
    if layout == "tokens" and tuple(t.shape) == (B, K):
        t = t.index_select(1, torch.as_tensor(positions.copy(), device=t.device))
    elif not (layout == "rows" and tuple(t.shape) == (B, S)):
        raise ValueError(f"{name} must be [B, S] = [{B}, {S}] in row order or [B, K] = [{B}, {K}] in tokenizer order, got {tuple(t.shape)} (layout {layout!r})")
    return t.detach().float().contiguous()


def token_policy_loss(logits: torch.Tensor, ids: torch.Tensor, old_logprob: torch.Tensor, advantages: torch.Tensor, *, ref_logprob: Optional[torch.Tensor] = None,
                      clip=0.2, kl_coef: float = 0.0, ent_coef: float = 0.0, ar_order: bool = True, steps=None, weights: Optional[torch.Tensor] = None,
                      reduction: str = "mean", C: Optional[int] = None, offset: int = 0, inplace: bool = False, return_stats: bool = False,
                      logprob_layout: Optional[str] = None, ops=None):
    """The PPO / GRPO policy loss of the SAMPLED ids [B, K] (int32 / int64, tokenizer order) under logits [B, S, V] (fp32 or bf16, S <= K), differentiable with
    respect to `logits`: per row  -min(ratio A, clamp(ratio, 1 - lo, 1 + hi) A) + kl_coef * k3(ref || policy) - ent_coef * entropy,  ratio = exp(logprob -
    old_logprob), in ONE launch of csrc/token_policy.hip (include/selftok_hip_ext.h states the arithmetic).  ar_order, steps, C, offset, weights, inplace and
    the one-backward rule mean what they mean in `token_cross_entropy`.  `advantages`: [B] (one per sequence, as GRPO has it) or [B, S] in row order.
    `old_logprob` / `ref_logprob`: [B, S] in row order (what `score_tokens` returns) or [B, K] by tokenizer position (`TokenSampler.logprob`); where the
    two shapes coincide and the orders differ, say which with logprob_layout = "rows" | "tokens".  A roll-out scored by this project's kernels at temperature
    1 has ratio exactly 1.  clip: one number or (lo, hi).  reduction: "mean" (over the scored rows, weighted), "seq_mean" (the mean over each sequence's scored
    rows, then over the sequences that have any), "sum" or "none" ([B, S], 0 on ignored rows); every count is taken on the device; a batch without a single
    scored row has loss 0 and a zero gradient under every reduction.  A bad row (see
    `ops.token_policy`) makes the reduced loss NaN and has a zero gradient row.  return_stats=True: -> (loss, PolicyStats(logprob, ratio, kl, entropy, coef,
    flags [B, S], clip_frac [1], bad [1], ignored [1])), device tensors; the entropy is computed only then or with ent_coef != 0."""
    o = _ops if ops is None else ops
    if logits.dim() != 3 or ids.dim() != 2 or ids.shape[0] != logits.shape[0] or logits.shape[1] > ids.shape[1]:
        raise ValueError(f"need logits [B, S, V] and ids [B, K] with S <= K, got {tuple(logits.shape)} and {tuple(ids.shape)}")
    if reduction not in POLICY_REDUCTIONS:
        raise ValueError(f"reduction must be one of {POLICY_REDUCTIONS}, got {reduction!r}")
    clip = (float(clip), float(clip)) if isinstance(clip, (int, float)) else (float(clip[0]), float(clip[1]))
    kl_coef, ent_coef = float(kl_coef), float(ent_coef)
    inf = float("inf")
    if not (0.0 <= clip[0] < 1.0 and 0.0 <= clip[1] < inf and 0.0 <= kl_coef < inf and 0.0 <= ent_coef < inf):
        raise ValueError(f"need 0 <= clip lo < 1, a finite clip hi >= 0 and finite kl_coef, ent_coef >= 0, got {clip}, {kl_coef}, {ent_coef}")
    if kl_coef != 0.0 and ref_logprob is None:
        raise ValueError("kl_coef != 0 needs ref_logprob")
    if logprob_layout not in (None, "rows", "tokens"):
        raise ValueError(f"logprob_layout must be None, 'rows' or 'tokens', got {logprob_layout!r}")
    B, S, _ = logits.shape
    K = ids.shape[1]
    view, reverse, positions = target_view(ids, S, ar_order, steps)
    old = _rows_of_logprob("old_logprob", old_logprob, B, S, K, positions, logprob_layout)
    ref = _rows_of_logprob("ref_logprob", ref_logprob, B, S, K, positions, logprob_layout)
    if tuple(advantages.shape) == (B,):
        adv = advantages.detach().float().unsqueeze(1).expand(B, S).contiguous()
    elif tuple(advantages.shape) == (B, S):
        adv = advantages.detach().float().contiguous()
    else:
        raise ValueError(f"advantages must be [B] = [{B}] or [B, S] = [{B}, {S}], got {tuple(advantages.shape)}")
    w = None
    if weights is not None:
        if tuple(weights.shape) == (K,):
            w = weights.index_select(0, torch.as_tensor(positions.copy(), device=weights.device)).unsqueeze(0)
        elif tuple(weights.shape) == (B, S):
            w = weights
        else:
            raise ValueError(f"weights must be [K] = [{K}] by tokenizer position or [B, S] = [{B}, {S}] by row, got {tuple(weights.shape)}")
        w = w.detach()
    want_entropy = bool(return_stats) or ent_coef != 0.0
    loss, logprob, ratio, kl, entropy, coef, flags, clip_frac, bad, ignored = _TokenPolicy.apply(
        logits, view, reverse, old, adv, ref, w, clip, kl_coef, ent_coef, C, int(offset), reduction, bool(inplace), want_entropy, o)
    return (loss, PolicyStats(logprob, ratio, kl, entropy if want_entropy else None, coef, flags, clip_frac, bad, ignored)) if return_stats else loss


def group_advantages(rewards: torch.Tensor, group_size: int, eps: float = 1e-6, normalize_std: bool = True) -> torch.Tensor:
    """GRPO's advantages: rewards [G * n], consecutive runs of n = group_size samples of one prompt -> (r - mean of its group) / (std of its group + eps), fp32
    [G * n], computed in fp64 on the rewards' device; the std is the population one (divisor n: a group of one gets advantage 0, not NaN).
    normalize_std=False leaves out the division.  A length that is not a multiple of group_size is refused."""
    n = int(group_size)
    if rewards.dim() != 1 or n < 1 or rewards.numel() % n:
        raise ValueError(f"need rewards [G * group_size] with group_size >= 1, got {tuple(rewards.shape)} and group_size {group_size}")
    r = rewards.detach().double().reshape(-1, n)
    centred = r - r.mean(1, keepdim=True)
    if normalize_std:
        centred = centred / (centred.pow(2).mean(1, keepdim=True).sqrt() + float(eps))
    return centred.reshape(-1).float()
