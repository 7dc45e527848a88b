"""-m gpu: the exact-order attention with a per-sample key bit mask (selftok_ex_attention_kmask_f32 / _kmask_fused_f32,
csrc/encoder_exact.hip) -- `ops.ex_attention(..., kmask=)`.  Cases: tests/ex_kmask_cases.py.

 1. prefix bits are the `valid1` route bit for bit (the route tests/test_encoder_exact_gpu.py pins to ATen through the CPU twin);
 2. fused = unfused bit for bit on every non-prefix pattern;
 3. a sample alone = the sample inside its batch;
 4. NaN / Inf in K and V at every invisible slot change no output bit;
 5. the stored outputs of torch-CPU's F.scaled_dot_product_attention with the bool mask (tests/golden/ex_kmask_sdpa.npz): 0 differing bits;
 6. a float64 masked softmax in plain torch, under the project's gate (tests/edge_cases.py: <= 2x rms / 4x max of torch fp32's own error).
"""
import os

import numpy as np
import pytest
import torch

import edge_cases as EC
import ex_kmask_cases as XK
from selftoktokenizer_amd import ops

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
HD = lambda c: c.H * XK.DH


def _same(a: torch.Tensor, b: torch.Tensor, what: str):
    x, y = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    assert x.shape == y.shape, (x.shape, y.shape)
    bad = x.view(np.uint32) != y.view(np.uint32)
    bad &= ~((x == 0) & (y == 0))                          # +0 / -0 are equal values
    n = int(bad.sum())
    if n:
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {n} of {x.size} fp32 elements differ; first at {i}: {x[i]!r} vs {y[i]!r}")


def _words(mask: np.ndarray, shared: bool = False) -> torch.Tensor:
    return torch.from_numpy(XK.pack(mask[:1] if shared else mask)).cuda()


def _run(c, q, ctx, img, mask, kernel, rows1=None, valid1=None):
    """rows1: how many context rows are handed over (default: up to the last visible position of any sample; the slots stay c.Tk1);
    valid1: the step prefix inside those rows (default: all of them)"""
    h = HD(c)
    any_vis = np.nonzero(mask.any(axis=0))[0]
    n = (int(any_vis[-1]) + 1 if any_vis.size else 0) if rows1 is None else rows1
    cx = ctx[:, :n].contiguous()
    im = img[:, :c.Tk2].contiguous()
    k1, v1 = (cx[..., h:2 * h], cx[..., 2 * h:]) if n else (None, None)
    k2, v2 = (im[..., h:2 * h], im[..., 2 * h:]) if c.Tk2 else (None, None)
    if k1 is None and k2 is None:
        return torch.zeros(c.B, c.Tq, h, device=q.device)
    return ops.ex_attention(q[..., :h], k1, v1, c.H, k2, v2, slots1=c.Tk1, kernel=kernel, kmask=_words(mask, c.shared), valid1=valid1)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,slots,valid,Tk2,Tq", [("fused",) + t for t in XK.PREFIX_CASES] + [("unfused",) + t for t in XK.PREFIX_CASES + XK.PREFIX_CASES_UNFUSED])
def test_prefix_bits_are_the_valid1_route(kernel, slots, valid, Tk2, Tq):
    """the words of `arange(slots) < valid` against the entry without a mask that is handed `valid` rows; then the same words over ALL the rows (valid1 = slots:
    the mask alone hides the rest, whose K / V are live data)"""
    c = XK.Case(f"prefix_{slots}_{valid}_{Tk2}_{Tq}", slots, Tk2, Tq, ("full", "full"), H=3)
    q, ctx, img = XK.inputs(c, "cuda")
    h = HD(c)
    cx, im = ctx[:, :valid].contiguous(), img[:, :Tk2].contiguous()
    k1, v1 = (cx[..., h:2 * h], cx[..., 2 * h:]) if valid else (None, None)
    k2, v2 = (im[..., h:2 * h], im[..., 2 * h:]) if Tk2 else (None, None)
    want = ops.ex_attention(q[..., :h], k1, v1, c.H, k2, v2, slots1=slots, kernel=kernel)
    mask = np.stack([XK.prefix(slots, valid)] * 2)
    got = _run(c, q, ctx, img, mask, kernel)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all())
    _same(got, want, f"{kernel}: prefix bits, {valid} of {slots} + {Tk2}")
    _same(_run(c, q, ctx, img, mask, kernel, rows1=slots), want, f"{kernel}: prefix bits over all {slots} rows")
    _same(_run(XK.Case(c.name, slots, Tk2, Tq, c.rows, H=3, shared=True), q, ctx, img, mask, kernel), want, f"{kernel}: one shared word row")


# ---- 2, 3 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XK.MASK_CASES, ids=lambda c: c.name)
def test_fused_equals_unfused(c):
    q, ctx, img = XK.inputs(c, "cuda")
    mask = XK.case_mask(c)
    f = _run(c, q, ctx, img, mask, "fused")
    u = _run(c, q, ctx, img, mask, "unfused")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(f).all()) and bool(torch.isfinite(u).all())
    _same(f, u, f"{c.name}: fused vs unfused")
    _same(_run(c, q, ctx, img, mask, "fused", rows1=c.Tk1), f, f"{c.name}: all rows handed over vs rows up to the last visible one")
    for b in range(c.B):
        if not mask[b].any() and not c.Tk2:
            assert float(f[b].abs().max()) == 0.0 and float(u[b].abs().max()) == 0.0, "a sample without a visible key: zeros"
    if c.shared:
        rep = XK.Case(c.name, c.Tk1, c.Tk2, c.Tq, c.rows, c.H, shared=False)
        _same(_run(rep, q, ctx, img, mask, "fused"), f, f"{c.name}: kmask_bs = 0 vs the same row repeated")
        _same(_run(rep, q, ctx, img, mask, "unfused"), f, f"{c.name}: kmask_bs = 0 vs the same row repeated (unfused)")


@pytest.mark.parametrize("c", XK.MASK_CASES + XK.MASK_CASES_UNFUSED, ids=lambda c: c.name)
def test_sample_alone_equals_sample_in_batch(c):
    kernel = "auto" if c in XK.MASK_CASES else "unfused"
    q, ctx, img = XK.inputs(c, "cuda")
    mask = XK.case_mask(c)
    whole = _run(c, q, ctx, img, mask, kernel)
    for b in range(c.B):
        one = XK.Case(c.name, c.Tk1, c.Tk2, c.Tq, c.rows[b:b + 1], c.H)
        alone = _run(one, q[b:b + 1], ctx[b:b + 1], img[b:b + 1], mask[b:b + 1], kernel, rows1=c.Tk1)
        _same(alone, _run(c, q, ctx, img, mask, kernel, rows1=c.Tk1)[b:b + 1], f"{c.name}: sample {b} alone vs in the batch")
        _same(alone, whole[b:b + 1], f"{c.name}: sample {b} alone vs in the batch (rows up to the last visible one)")


def test_unfused_batch_slices_take_their_words(monkeypatch):
    c = XK.MASK_CASES_UNFUSED[0]
    q, ctx, img = XK.inputs(c, "cuda")
    mask = XK.case_mask(c)
    whole = _run(c, q, ctx, img, mask, "unfused")
    per = int(ops._lib.load().selftok_ex_attention_workspace_bytes(1, c.H, c.Tq, c.Tk1 + c.Tk2, XK.DH))
    monkeypatch.setattr(ops, "EX_ATTENTION_WS_LIMIT", 2 * per)                   # slices of 2, 2, 1 samples
    _same(_run(c, q, ctx, img, mask, "unfused"), whole, "unfused, batch in slices of two")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,kernel", [(c, k) for c in XK.MASK_CASES for k in ("fused", "unfused")] + [(c, "unfused") for c in XK.MASK_CASES_UNFUSED],
                         ids=lambda v: v if isinstance(v, str) else v.name)
def test_invisible_keys_are_never_read_into_the_arithmetic(c, kernel):
    q, ctx, img = XK.inputs(c, "cuda")
    mask = XK.case_mask(c)
    h = HD(c)
    clean = _run(c, q, ctx, img, mask, kernel, rows1=c.Tk1)
    bad = ctx.clone()
    inv = torch.from_numpy(~mask).cuda()                                          # [B, Tk1]
    poison = torch.tensor([float("nan"), float("inf"), -float("inf")], device="cuda")[torch.arange(c.Tk1, device="cuda") % 3]
    bad[..., h:] = torch.where(inv[..., None], poison[None, :, None], bad[..., h:])
    _same(_run(c, q, bad, img, mask, kernel, rows1=c.Tk1), clean, f"{c.name} [{kernel}]: NaN / Inf at every invisible slot")
    # rows >= valid1: a step prefix that ends before the last visible position; every row at and past it is poisoned, whatever its bit says
    any_vis = np.nonzero(mask.any(axis=0))[0]
    v1 = int(any_vis[len(any_vis) // 2]) + 1 if any_vis.size else 0
    cut = mask & (np.arange(c.Tk1)[None] < v1)
    want = _run(c, q, ctx, img, cut, kernel, rows1=c.Tk1)
    bad[:, v1:, h:] = float("nan")
    _same(_run(c, q, bad, img, mask, kernel, rows1=c.Tk1, valid1=v1), want, f"{c.name} [{kernel}]: valid1 = {v1} cuts the pattern; poisoned rows at and past it")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["fused", "unfused"])
@pytest.mark.parametrize("c", XK.SDPA_CASES, ids=lambda c: c.name)
def test_equals_aten_sdpa_with_a_bool_mask(c, kernel):
    """0 differing bits against torch-CPU's F.scaled_dot_product_attention(q, k, v, attn_mask=bool) as stored by tools/oracle/gen_golden.py (stage exact_masks)."""
    gold = np.load(os.path.join(GOLD, "ex_kmask_sdpa.npz"))
    q, ctx, img = XK.inputs(c, "cuda")
    got = _run(c, q, ctx, img, XK.case_mask(c), kernel)
    _same(got, torch.from_numpy(gold[c.name]), f"{c.name} [{kernel}] vs ATen")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", XK.MASK_CASES + XK.MASK_CASES_UNFUSED + XK.SDPA_CASES, ids=lambda c: c.name)
def test_against_fp64_masked_softmax(c):
    q, ctx, img = XK.inputs(c, "cuda")
    mask = XK.case_mask(c)
    ref = XK.reference(c, q, ctx, img, mask, torch.float64)
    t32 = XK.reference(c, q, ctx, img, mask, torch.float32)
    et, eg = EC.ErrAcc(), EC.ErrAcc()
    et.add(t32, ref)
    got = _run(c, q, ctx, img, mask, "unfused" if c in XK.MASK_CASES_UNFUSED else "auto")
    eg.add(got.cpu(), ref)
    rms_b, max_b = EC.gate(et.rms, et.mx)
    print(f"[ex_kmask] {c.name}: rms {eg.rms:.3e} (torch fp32 {et.rms:.3e}, bound {rms_b:.3e}), max {eg.mx:.3e} (torch fp32 {et.mx:.3e}, bound {max_b:.3e})")
    assert eg.rms <= rms_b and eg.mx <= max_b
