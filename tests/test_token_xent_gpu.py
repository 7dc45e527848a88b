"""-m gpu: the token loss (csrc/token_xent.hip through ops.token_xent and losses.token_cross_entropy) against the numpy arithmetic of record of
tests/token_xent_cases.py: every gradient element (fp32 and bf16) and both counters equal on every case inside guard bands and sentinel pad columns, nll and
lse within 1 fp32 ulp (the device's fp64 log may differ from numpy's in the last place before the one rounding to fp32; a row with z_coef != 0 may then
carry the factor of `a` one ulp off, and is held to the emulation with exactly that factor), the invariances bit for bit -- in place above all -- the scorer
kernel held to this one by equality, and the public function against fp64 autograd through a Linear head."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_xent_cases as XC
from selftoktokenizer_amd import losses, ops

pytestmark = pytest.mark.gpu
GUARD = 64                                                          # guard elements either side of the logits and of the gradient (a multiple of four codes)
f32, u32 = np.float32, np.uint32
ALLOWANCE = {"rows": 0, "factor_rows": 0, "ulp_rows": 0}            # how often the one-ulp allowances were needed (printed by the last test)


def _torch_dtype(c):
    return torch.bfloat16 if c.dtype == "bf16" else torch.float32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _banded(host_bits, c, fill):
    """host [R, row] (fp32, or bf16 bits) or None -> (a [R, row] device view inside a flat buffer with guard bands of `fill`, the flat buffer)"""
    R = XC.rows_of(c)
    flat = torch.full((GUARD + R * c.row + GUARD,), fill, dtype=_torch_dtype(c), device="cuda")
    if host_bits is not None:
        t = torch.from_numpy(host_bits.view(np.int16) if c.dtype == "bf16" else host_bits)
        flat[GUARD:GUARD + t.numel()] = (t.view(torch.bfloat16) if c.dtype == "bf16" else t).reshape(-1).cuda()
    return flat[GUARD:GUARD + R * c.row].view(R, c.row), flat


def _dev_ids(c, host):
    """the id buffer on the device and the [B, S] view the case describes (torch strides are positive: a negative step stride is `reverse_steps`)"""
    _, base, seq, step = XC.id_geometry(c)
    buf = torch.from_numpy(host).cuda()
    lo = base if step > 0 else base + (c.S - 1) * step
    return torch.as_strided(buf, (c.B, c.S), (seq, abs(step)), lo), step < 0, buf


def _launch(c, logits_rows, ids, *, reverse=False, scale=None, inplace=False, shape3=False, **kw):
    """one call over the [R, row] view `logits_rows` (its first V columns are the tensor handed over) with sentinel-filled, guard-banded outputs -> dict of
    host arrays; out of place the whole [R, row] gradient buffer comes back as bits, in place the logits buffer does"""
    R = logits_rows.shape[0]
    nll = torch.full((R + 2,), 123.0, device="cuda")
    lse = torch.full((R + 2,), 123.0, device="cuda")
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    shape = (c.B, c.S) if shape3 else (R,)
    cut = lambda rows: rows.view(c.B, c.S, c.row)[:, :, :c.V] if shape3 else rows[:, :c.V]
    grows, gflat = (logits_rows, None) if inplace else _banded(None, c, float(XC.SENT))
    ops.token_xent(cut(logits_rows), ids, C=c.C, offset=c.offset, z_coef=float(c.z), row_scale=scale, reverse_steps=reverse, inplace=inplace,
                   grad=None if inplace else cut(grows), nll=nll[1:R + 1].view(shape), lse=lse[1:R + 1].view(shape), bad=bad, ignored=ign, **kw)
    torch.cuda.synchronize()
    h_nll, h_lse = nll.cpu().numpy(), lse.cpu().numpy()
    assert (h_nll[[0, -1]] == 123.0).all() and (h_lse[[0, -1]] == 123.0).all(), "an output guard row was written"
    if gflat is not None:
        assert bool((gflat[:GUARD] == float(XC.SENT)).all()) and bool((gflat[-GUARD:] == float(XC.SENT)).all()), "a gradient guard band was written"
    g = _bits(grows).cpu().numpy()
    return dict(nll=h_nll[1:-1], lse=h_lse[1:-1], grad=g.view(np.uint16) if c.dtype == "bf16" else g.view(u32), bad=int(bad.cpu()[0]), ignored=int(ign.cpu()[0]))


_RUNS = {}


def run_case(name):
    """the case on the device, once, out of place: (result, the device inputs)"""
    if name not in _RUNS:
        c, d = XC.BY_NAME[name], XC.make(name)
        logits, lflat = _banded(d["logits"], c, float("nan"))
        ids, reverse, buf = _dev_ids(c, d["ids"])
        scale = None if d["scale"] is None else torch.from_numpy(d["scale"]).cuda()
        before, ids_before = _bits(lflat).clone(), buf.clone()
        out = _launch(c, logits, ids, reverse=reverse, scale=scale)
        assert torch.equal(_bits(lflat), before) and torch.equal(buf, ids_before)              # out of place the inputs are only read
        _RUNS[name] = (out, dict(logits=logits, lflat=lflat, ids=ids, reverse=reverse, scale=scale))
    return _RUNS[name]


def _ulp_apart(a, b):
    ia, ib = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _same_bits(a, b, keys=("nll", "lse", "grad")):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and a["bad"] == b["bad"] and a["ignored"] == b["ignored"]


def _ref_bits(c, ref):
    return ref.grad.view(np.uint16 if c.dtype == "bf16" else u32)


def _check(name, out):
    c, ref = XC.BY_NAME[name], XC.reference(name)
    good = ~ref.bad
    assert out["bad"] == int(ref.bad.sum()) and out["ignored"] == int(ref.ignored.sum()), (name, out["bad"], out["ignored"])
    assert np.isnan(out["nll"][~good]).all() and np.isnan(out["lse"][~good]).all()
    assert (_ulp_apart(out["nll"][good], ref.nll[good]) <= 1).all(), (name, "nll", out["nll"][good][:4], ref.nll[good][:4])
    assert (_ulp_apart(out["lse"][good], ref.lse[good]) <= 1).all(), (name, "lse", out["lse"][good][:4], ref.lse[good][:4])
    assert (out["nll"][ref.ignored].view(u32) == 0).all()                                        # +0.0 exactly
    ALLOWANCE["rows"] += int(good.sum())
    ALLOWANCE["ulp_rows"] += int(((out["nll"][good].view(u32) != ref.nll[good].view(u32)) | (out["lse"][good].view(u32) != ref.lse[good].view(u32))).sum())
    want = _ref_bits(c, ref)
    off = np.flatnonzero((out["grad"] != want).any(1))
    if off.size and c.z != 0:                                       # the factor of `a` one ulp either way: the whole row must be the emulation's with that factor
        lo, hi = _ref_bits(c, XC.reference(name, factor_ulps=-1)), _ref_bits(c, XC.reference(name, factor_ulps=1))
        still = [r for r in off if not (np.array_equal(out["grad"][r], lo[r]) or np.array_equal(out["grad"][r], hi[r]))]
        ALLOWANCE["factor_rows"] += off.size - len(still)
        off = np.asarray(still)
    assert off.size == 0, (name, "gradient rows", off[:5], [int(np.flatnonzero(out["grad"][r] != want[r])[0]) for r in off[:5]])


@pytest.mark.parametrize("name", [c.name for c in XC.CASES])
def test_token_xent_equals_the_emulation(name):
    """every gradient element equal, nll and lse within 1 fp32 ulp, nothing written outside what is stated: the pad columns [V, row) keep their sentinel (they are
    part of the comparison), the guard bands and guard rows theirs; bad and ignored rows are written as zeros and counted once each"""
    out, _ = run_case(name)
    _check(name, out)


@pytest.mark.parametrize("name", [c.name for c in XC.CASES if XC.rows_of(c) <= 64])
def test_in_place_equals_out_of_place(name):
    """grad == logits: columns [0, V) of every row are the out-of-place bits, nll, lse and the counters too; the pad columns [V, row) and the guard bands keep
    the logits buffer's NaN"""
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    lflat = dev["lflat"].clone()
    rows = lflat[GUARD:GUARD + XC.rows_of(c) * c.row].view(-1, c.row)
    got = _launch(c, rows, dev["ids"], reverse=dev["reverse"], scale=dev["scale"], inplace=True)
    assert _same_bits(out, got, keys=("nll", "lse")) and np.array_equal(got["grad"][:, :c.V], out["grad"][:, :c.V]), name
    keep = torch.ones(c.row, dtype=torch.bool, device="cuda")
    keep[:c.V] = False
    assert torch.equal(_bits(rows)[:, keep], _bits(dev["logits"])[:, keep]) and torch.equal(_bits(lflat)[:GUARD], _bits(dev["lflat"])[:GUARD])
    assert torch.equal(_bits(lflat)[-GUARD:], _bits(dev["lflat"])[-GUARD:])


@pytest.mark.parametrize("name", ["c4096_R64", "c32768_bf16_g8", "c65536_g8", "four_bf16_z", "bad_rows_z", "ignored_z", "bad_rows_stream"])
def test_run_to_run_alone_and_in_any_row_order(name):
    """the same bits again; a row alone gives what it gave in the batch; the rows reversed give the reversed outputs -- a bad or ignored row beside it or not"""
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    assert _same_bits(out, _launch(c, dev["logits"], dev["ids"], reverse=dev["reverse"], scale=dev["scale"]))
    R = XC.rows_of(c)
    t = torch.from_numpy(XC.make(name)["targets"]).cuda()
    for r in sorted({0, 1, R // 2, R - 1}):
        one = c._replace(B=1, S=1)
        got = _launch(one, dev["logits"][r:r + 1], t[r:r + 1], scale=None if dev["scale"] is None else dev["scale"][r:r + 1])
        assert all(got[k][0].tobytes() == out[k][r].tobytes() for k in ("nll", "lse", "grad")), (name, r)
    perm = torch.arange(R - 1, -1, -1, device="cuda")
    flat = c._replace(B=R, S=1)
    rev = _launch(flat, dev["logits"][perm].contiguous(), t[perm].contiguous(), scale=None if dev["scale"] is None else dev["scale"][perm].contiguous())
    p = perm.cpu().numpy()
    assert all(rev[k].tobytes() == out[k][p].tobytes() for k in ("nll", "lse", "grad")) and rev["bad"] == out["bad"] and rev["ignored"] == out["ignored"]


@pytest.mark.parametrize("name", ["c257_bf16_zbig", "c2048_bf16", "c4097_bf16_S40_wide_rev", "c32768_bf16_g8", "c32769_bf16_z", "c65536_bf16_z"])
def test_bf16_equals_the_same_values_widened_to_fp32(name):
    """nll and lse bit for bit (the gradient is rounded to the logits' dtype, so it is not compared)"""
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    wide = _launch(c._replace(dtype="f32"), dev["logits"].float(), dev["ids"], reverse=dev["reverse"], scale=dev["scale"])
    assert _same_bits(out, wide, keys=("nll", "lse"))


@pytest.mark.parametrize("name", ["c5_S3_rev_zbig", "c4096_S40_rev_z", "c2050_int32_wide", "c1000_bf16_vlm_wide_rev_zbig", "c32768_vlm_z", "c32770_vlm",
                                  "ignored_int32_rev_bf16"])
def test_three_dimensional_logits_and_reversed_steps_equal_the_flat_call(name):
    """[B, S, V] logits and gradient give what their [B * S, V] rows give; ids walked backwards in place (step stride -1 or -2) give what a materialised flip gives"""
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    assert _same_bits(out, _launch(c, dev["logits"], dev["ids"], reverse=dev["reverse"], scale=dev["scale"], shape3=True))
    dense = (dev["ids"].flip(1) if dev["reverse"] else dev["ids"]).contiguous()
    assert _same_bits(out, _launch(c, dev["logits"], dense, scale=dev["scale"], shape3=True))
    assert _same_bits(out, _launch(c, dev["logits"], dense.reshape(-1), scale=dev["scale"]))
    assert _same_bits(out, _launch(c, dev["logits"], dense.reshape(-1), scale=dev["scale"], rows_per_seq=c.S))


@pytest.mark.parametrize("name", ["c4095_stride_z", "c32767_g8_z", "c32768_vlm_z", "c65536_bf16_z", "target_neginf", "dominant_zbig", "ignored_z", "bad_rows_bf16",
                                  "zeros_pair", "four"])
def test_nll_is_the_scorer_kernels_logprob_with_the_sign_turned(name):
    """kernel against kernel: ops.token_score at temperature 1 without guidance on the same buffers"""
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    lp = ops.token_score(dev["logits"][:, :c.V], dev["ids"], C=c.C, offset=c.offset, temperature=1.0, reverse_steps=dev["reverse"])[0].reshape(-1).cpu().numpy()
    ref = XC.reference(name)
    sc = ~ref.bad & ~ref.ignored
    assert np.array_equal(out["nll"][sc].view(u32), lp[sc].view(u32) ^ u32(0x80000000)) and np.isnan(lp[ref.bad]).all() and (lp[ref.ignored] == 0).all()


def test_graph_replay_equals_eager():
    name = "c32768_vlm_z"
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    lg3 = dev["logits"].view(c.B, c.S, c.row)[:, :, :c.V]
    grad = torch.zeros(c.B, c.S, c.row, device="cuda")
    nll, lse = torch.zeros(c.B, c.S, device="cuda"), torch.zeros(c.B, c.S, device="cuda")
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda: ops.token_xent(lg3, dev["ids"], C=c.C, offset=c.offset, z_coef=float(c.z), row_scale=dev["scale"], reverse_steps=dev["reverse"], grad=grad[:, :, :c.V],
                                  nll=nll, lse=lse, bad=bad, ignored=ign)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in (grad, nll, lse):
        t.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    R = XC.rows_of(c)
    assert nll.cpu().numpy().reshape(R).tobytes() == out["nll"].tobytes() and lse.cpu().numpy().reshape(R).tobytes() == out["lse"].tobytes()
    assert np.array_equal(grad.view(R, c.row)[:, :c.V].cpu().numpy().view(u32), out["grad"][:, :c.V]) and bool((grad.view(R, c.row)[:, c.V:] == 7.0).all())


def test_no_rows_accumulating_counters_and_refusals():
    lg = torch.zeros(0, 128, device="cuda")
    nll, lse, grad, bad, ign = ops.token_xent(lg, torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert nll.shape == (0,) and lse.shape == (0,) and grad.shape == (0, 128) and int(bad.cpu()[0]) == 0 and int(ign.cpu()[0]) == 0
    name = "bad_rows_z"
    c = XC.BY_NAME[name]
    out, dev = run_case(name)
    bad, ign = torch.full((1,), 10, dtype=torch.int32, device="cuda"), torch.full((1,), 20, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(XC.make(name)["targets"]).cuda()
    t[0] = -5
    lg = dev["logits"][:, :c.V]
    for _ in range(2):
        ops.token_xent(lg, t, C=c.C, offset=c.offset, bad=bad, ignored=ign)
    assert int(bad.cpu()[0]) == 10 + 2 * out["bad"] and int(ign.cpu()[0]) == 20 + 2
    before = _bits(dev["lflat"]).clone()
    for kw in (dict(z_coef=-1.0), dict(z_coef=float("nan")), dict(C=c.C + 1), dict(rows_per_seq=2), dict(grad=torch.as_strided(dev["lflat"], (9, c.V), (c.row, 1), GUARD + 4)),
               dict(grad=torch.zeros(9, c.V, device="cuda"), inplace=True), dict(row_scale=torch.ones(8, device="cuda")), dict(grad=torch.zeros(9, c.V, dtype=torch.bfloat16, device="cuda"))):
        with pytest.raises(Exception):
            ops.token_xent(lg, t, **dict(dict(C=c.C, offset=c.offset), **kw))
    torch.cuda.synchronize()
    assert torch.equal(_bits(dev["lflat"]), before)                  # a refused call leaves its buffers untouched


# ---- the public function ------------------------------------------------------------------------------------------------------------------------------
def _head_reference(logits, x, ids, *, ar_order, steps, weights, z, reduction):
    """the same graph under F.cross_entropy in fp64 on the fp32 logits the head produced -> (loss, dloss/dW, their bounds): the per-element bounds of
    tests/token_xent_cases.py carried through the reduction and the matmul dW = dlogits^T x, plus the fp32 rounding of the row scales (2^-24 each) and of the
    backward matmul itself ((R + 2) 2^-24 of the sum of absolute products)"""
    B, S, V = logits.shape
    K = ids.shape[1]
    tgt = (ids[:, K - S:].flip(1) if ar_order else ids[:, :S]).clone()
    if steps is not None:
        tgt[torch.arange(S).unsqueeze(0) >= torch.as_tensor(steps).reshape(-1, 1)] = -1
    pos = (K - 1 - torch.arange(S)) if ar_order else torch.arange(S)
    w = torch.ones(B, S, dtype=torch.float64) if weights is None else (weights[pos].expand(B, S) if weights.dim() == 1 else weights).double()
    lg = logits.detach().double().cpu().requires_grad_(True)
    scored = tgt >= 0
    L = torch.logsumexp(lg, -1)
    ce = F.cross_entropy(lg.reshape(-1, V), tgt.reshape(-1).clamp(min=0), reduction="none").reshape(B, S)
    rows = torch.where(scored, w * (ce + z * L * L), torch.zeros((), dtype=torch.float64))
    denom = torch.where(scored, w, torch.zeros((), dtype=torch.float64)).sum()
    loss = rows if reduction == "none" else rows.sum() if reduction == "sum" else rows.sum() / denom
    up = torch.arange(1.0, B * S + 1, dtype=torch.float64).reshape(B, S) / (B * S) if reduction == "none" else torch.ones((), dtype=torch.float64)
    (loss * up).sum().backward()
    g_rows = (w * up / (denom if reduction == "mean" else 1.0)) * scored                           # the scale of each row, as the kernel gets it (times upstream)
    x64 = x.detach().double().cpu().reshape(B * S, -1)
    dW = lg.grad.reshape(B * S, V).t() @ x64
    p = torch.softmax(lg.detach(), -1).numpy()
    Ln = L.detach().numpy()
    bg = np.zeros((B * S, V))
    for r in range(B * S):
        b, s = divmod(r, S)
        if scored[b, s]:
            g = float(g_rows[b, s])
            onehot = np.zeros(V)
            onehot[int(tgt[b, s])] = 1.0
            bg[r] = XC.bound_grad(V, p[b, s], g * (1 + 2 * z * Ln[b, s]), g, z, Ln[b, s], onehot) + 2.0 ** -23 * np.abs(lg.grad[b, s].numpy())
    ax = np.abs(x64.numpy())
    b_dW = bg.T @ ax + (B * S + 2) * 2.0 ** -24 * (np.abs(lg.grad.reshape(B * S, V).numpy()).T @ ax)
    b_rows = np.where(scored.numpy(), w.numpy() * (XC.bound_row_scalar(V, 1.0) + np.abs(ce.detach().numpy()) * 2.0 ** -24 +
                                                  z * (2 * np.abs(Ln) + 1) * (XC.bound_row_scalar(V, 1.0) + np.abs(Ln) * 2.0 ** -24)), 0.0)
    if reduction == "none":
        b_loss = b_rows + np.abs(rows.detach().numpy()) * 2.0 ** -24
    else:
        b_loss = b_rows.sum() / (float(denom) if reduction == "mean" else 1.0) + abs(float(loss.detach())) * 2.0 ** -23
    return loss.detach().numpy(), dW.numpy(), b_loss, b_dW


HEAD_CASES = [dict(reduction="mean"), dict(reduction="sum"), dict(reduction="none"), dict(reduction="mean", weights="K", z=1e-4), dict(reduction="sum", weights="BS", steps=[6, 3, 0, 5]),
              dict(reduction="none", weights="K", z=1e-4, steps=[6, 3, 0, 5]), dict(reduction="mean", ar_order=False, steps=[1, 2, 3, 4], z=0.5), dict(reduction="mean", inplace=True, z=1e-4)]


@pytest.mark.parametrize("kw", HEAD_CASES, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_token_cross_entropy_through_a_linear_head(kw):
    """loss and head.weight.grad within the derived bound, carried through the matmul, of F.cross_entropy + z logsumexp^2 in fp64 on the same logits; the loss
    times 3 before backward() triples every gradient"""
    B, S, K, D, V = 4, 6, 8, 32, 300
    g = torch.Generator().manual_seed(11)
    head = torch.nn.Linear(D, V).cuda()
    x = torch.randn(B, S, D, generator=g).cuda()
    ids = torch.randint(0, V, (B, K), generator=g)
    ids[1, 5] = -1
    weights = {"K": torch.rand(K, generator=g) + 0.5, "BS": torch.rand(B, S, generator=g) + 0.5, None: None}[kw.get("weights")]
    z, red, steps, ar = kw.get("z", 0.0), kw["reduction"], kw.get("steps"), kw.get("ar_order", True)
    call = lambda lg: losses.token_cross_entropy(lg, ids.cuda(), ar_order=ar, steps=steps, z_loss=z, weights=None if weights is None else weights.cuda(), reduction=red,
                                                 inplace=kw.get("inplace", False))
    up = (torch.arange(1.0, B * S + 1).reshape(B, S) / (B * S)).cuda() if red == "none" else None
    grads = []
    for times in (1.0, 3.0):
        head.zero_grad()
        logits = head(x)
        kept = logits.detach().clone()
        loss = call(logits)
        ((loss * up).sum() * times if up is not None else loss * times).backward()
        grads.append(head.weight.grad.clone())
    want_loss, want_dW, b_loss, b_dW = _head_reference(kept, x, ids, ar_order=ar, steps=steps, weights=weights, z=z, reduction=red)
    e_loss, e_dW = np.abs(loss.detach().double().cpu().numpy() - want_loss), np.abs(grads[0].double().cpu().numpy() - want_dW)
    share = lambda e, b: float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), 0.0)))
    print(f"\nloss share of the bound {share(e_loss, b_loss):.3f}, weight gradient share {share(e_dW, b_dW):.3f}")
    assert (e_loss <= b_loss).all() and (e_dW <= b_dW).all() and float(np.abs(want_dW).max()) > 1e-3
    # tripled: both runs round the scaled gradient rows (2^-24 each) and the backward matmul ((R + 2) 2^-24 of the absolute products, which b_dW holds once)
    # on their own, the second at three times the size: 3 (2 (R + 2) + 3) 2^-24 of the absolute products in all, under 8 b_dW
    assert (np.abs(grads[1].double().cpu().numpy() - 3.0 * grads[0].double().cpu().numpy()) <= 8.0 * b_dW).all()
    if kw.get("inplace"):
        assert not torch.equal(logits.detach(), kept)               # the logits are gone


def test_token_cross_entropy_memory_synchronisation_and_second_backward():
    R, V = 256, 32768
    ids = torch.randint(0, V, (4, 64), device="cuda")
    size = R * V * 4
    for inplace in (True, False):
        logits = torch.randn(4, 64, V, device="cuda").requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")                     # a forward call synchronises nothing and reads nothing back
        try:
            loss, st = losses.token_cross_entropy(logits, ids, z_loss=1e-4, inplace=inplace, return_stats=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert (peak < 1 << 20) if inplace else (size <= peak < size + (1 << 20)), (inplace, peak)
        assert st.nll.shape == (4, 64) and int(st.bad.cpu()[0]) == 0 and math.isfinite(float(loss.detach()))
    loss.backward(retain_graph=True)
    assert logits.grad is not None and abs(float(logits.grad.double().sum())) < 1.0
    with pytest.raises(RuntimeError):
        loss.backward()
    logits = torch.randn(2, 3, 64, device="cuda").requires_grad_(True)
    loss = losses.token_cross_entropy(logits, ids[:2, :8])
    (gr,) = torch.autograd.grad(loss, logits, create_graph=True)
    if gr.requires_grad:                                            # once_differentiable: differentiating a second time is an error
        with pytest.raises(RuntimeError):
            gr.sum().backward()


def test_zz_report_the_allowances_used():
    """not a check of the kernel: prints how many rows needed the one-ulp allowance on nll / lse and how many the one-ulp allowance on the factor of `a`"""
    print(f"\n{ALLOWANCE['rows']} good rows compared: {ALLOWANCE['ulp_rows']} with nll or lse one ulp from numpy's, {ALLOWANCE['factor_rows']} gradient rows with the factor one ulp off")
