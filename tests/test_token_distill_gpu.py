"""-m gpu: the token distillation (csrc/token_distill.hip through ops.token_distill, losses.token_distillation and sampling.token_kl) against the numpy
arithmetic of record of tests/token_distill_cases.py: every gradient element (fp32 and bf16) and both counters equal on every case inside guard bands and
sentinel pad columns, the four row outputs within 1 fp32 ulp (the device's fp64 log may differ from numpy's in the last place before the one rounding to
fp32), the invariances bit for bit -- in place and metrics-only above all -- the scorer and the loss kernels held to this one by equality, and the public
function against torch fp64 through a Linear head."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import token_distill_cases as DC
from selftoktokenizer_amd import losses, ops, sampling

pytestmark = pytest.mark.gpu
GUARD = 64                                                          # guard elements either side of every logits buffer and of the gradient (a multiple of four codes)
f32, u32 = np.float32, np.uint32
OUTPUTS = ("kl", "ce", "h", "lse")
ALLOWANCE = {"rows": 0, "ulp_rows": 0}                              # how often the one-ulp allowance was needed (printed by the last test)


def _tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _banded(host_bits, R, rowlen, dtype, fill):
    """host [R, rowlen] (fp32, or bf16 bits) or None -> (a [R, rowlen] device view inside a flat buffer with guard bands of `fill`, the flat buffer)"""
    flat = torch.full((GUARD + R * rowlen + GUARD,), fill, dtype=_tdt(dtype), device="cuda")
    if host_bits is not None:
        t = torch.from_numpy(host_bits.view(np.int16) if dtype == "bf16" else host_bits)
        flat[GUARD:GUARD + t.numel()] = (t.view(torch.bfloat16) if dtype == "bf16" else t).reshape(-1).cuda()
    return flat[GUARD:GUARD + R * rowlen].view(R, rowlen), flat


def _launch(c, srows, trows, urows, *, scale=None, mask=None, inplace=False, want_grad=True, shape3=None):
    """one call over the [R, row] views (their first V / offset + C columns are the tensors handed over) with sentinel-filled, guard-banded outputs -> dict of
    host arrays; out of place the whole [R, row] gradient buffer comes back as bits, in place the student buffer does"""
    R = srows.shape[0]
    outs = {k: torch.full((R + 2,), 123.0, device="cuda") for k in OUTPUTS}
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    shape = shape3 if shape3 else (R,)
    cut = lambda rows, n: None if rows is None else (rows.view(shape3 + (rows.shape[1],))[:, :, :n] if shape3 else rows[:, :n])
    grows, gflat = (srows, None) if inplace or not want_grad else _banded(None, R, c.row, c.sd, float(DC.SENT))
    ops.token_distill(cut(srows, c.V), _as_width(cut(trows, min(c.V, c.trow)), c.V), teacher_uncond=_as_width(cut(urows, min(c.V, c.trow)), c.V), cfg_scale=1.0 if c.s is None else float(c.s),
                      C=c.C, offset=c.offset, row_scale=scale, row_mask=mask, inplace=inplace, want_grad=want_grad, grad=cut(grows, c.V) if want_grad and not inplace else None,
                      kl=outs["kl"][1:R + 1].view(shape), ce=outs["ce"][1:R + 1].view(shape), h_teacher=outs["h"][1:R + 1].view(shape),
                      lse_student=outs["lse"][1:R + 1].view(shape), bad=bad, ignored=ign)
    torch.cuda.synchronize()
    res = dict(bad=int(bad.cpu()[0]), ignored=int(ign.cpu()[0]))
    for k in OUTPUTS:
        hst = outs[k].cpu().numpy()
        assert (hst[[0, -1]] == 123.0).all(), "an output guard row was written"
        res[k] = hst[1:-1]
    if gflat is not None:
        assert bool((gflat[:GUARD] == float(DC.SENT)).all()) and bool((gflat[-GUARD:] == float(DC.SENT)).all()), "a gradient guard band was written"
    if want_grad:
        g = _bits(grows).cpu().numpy()
        res["grad"] = g.view(np.uint16) if c.sd == "bf16" else g.view(u32)
    return res


def _as_width(t, V):
    """a teacher view whose last dimension is made V wide WITHOUT touching memory: the teacher's rows of the table are shorter than the student's V where the
    student has pad columns inside V; the kernel reads the window alone, so the view may claim columns the next row owns"""
    if t is None or t.shape[-1] == V:
        return t
    return torch.as_strided(t, tuple(t.shape[:-1]) + (V,), t.stride(), t.storage_offset())


_RUNS = {}


def run_case(name):
    """the case on the device, once, out of place: (result, the device inputs)"""
    if name not in _RUNS:
        c, d = DC.BY_NAME[name], DC.make(name)
        srows, sflat = _banded(d["student"], c.R, c.row, c.sd, float("nan"))
        trows, tflat = _banded(d["teacher"], c.R, c.trow, c.td, float("nan"))
        urows, uflat = (None, None) if d["uncond"] is None else _banded(d["uncond"], c.R, c.trow, c.td, float("nan"))
        scale = None if d["scale"] is None else torch.from_numpy(d["scale"]).cuda()
        mask = None if d["mask"] is None else torch.from_numpy(d["mask"]).cuda()
        before = [_bits(f).clone() for f in (sflat, tflat, uflat) if f is not None]
        out = _launch(c, srows, trows, urows, scale=scale, mask=mask)
        assert all(torch.equal(_bits(f), b) for f, b in zip([f for f in (sflat, tflat, uflat) if f is not None], before))      # out of place the inputs are only read
        _RUNS[name] = (out, dict(s=srows, t=trows, u=urows, sflat=sflat, scale=scale, mask=mask))
    return _RUNS[name]


def _ulp_apart(a, b):
    ia, ib = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _same_bits(a, b, keys=OUTPUTS + ("grad",)):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and a["bad"] == b["bad"] and a["ignored"] == b["ignored"]


def _check(name, out):
    c, ref = DC.BY_NAME[name], DC.reference(name)
    good = ~ref.bad & ~ref.ignored
    assert out["bad"] == int(ref.bad.sum()) and out["ignored"] == int(ref.ignored.sum()), (name, out["bad"], out["ignored"])
    used = np.zeros(c.R, bool)
    for k in OUTPUTS:
        got, want = out[k], getattr(ref, k)
        assert np.isnan(got[ref.bad]).all() and (got[ref.ignored].view(u32) == 0).all(), (name, k)      # NaN on bad rows, +0.0 exactly on ignored ones
        fin = good & np.isfinite(want)
        assert np.array_equal(got[good & ~fin].view(u32), want[good & ~fin].view(u32)), (name, k, "infinite rows")
        assert (_ulp_apart(got[fin], want[fin]) <= 1).all(), (name, k, got[fin][:4], want[fin][:4])
        used |= good & (got.view(u32) != want.view(u32))
    ALLOWANCE["rows"] += int(good.sum())
    ALLOWANCE["ulp_rows"] += int(used.sum())
    want = ref.grad.view(np.uint16 if c.sd == "bf16" else u32)
    off = np.flatnonzero((out["grad"] != want).any(1))
    assert off.size == 0, (name, "gradient rows", off[:5], [int(np.flatnonzero(out["grad"][r] != want[r])[0]) for r in off[:5]])


@pytest.mark.parametrize("name", [c.name for c in DC.CASES])
def test_token_distill_equals_the_emulation(name):
    """every gradient element equal, the four outputs within 1 fp32 ulp, nothing written outside what is stated: the pad columns [V, row) keep their sentinel
    (they are part of the comparison), the guard bands and guard rows theirs; bad and ignored rows are written as zeros and counted once each"""
    out, _ = run_case(name)
    _check(name, out)


@pytest.mark.parametrize("name", [c.name for c in DC.CASES if c.R <= 64])
def test_in_place_and_metrics_only_equal_out_of_place(name):
    """grad == student: columns [0, V) of every row are the out-of-place bits, the outputs and the counters too; the pad columns [V, row) and the guard bands
    keep the student buffer's NaN.  want_grad=False: the same outputs and counters, and nothing else written"""
    c = DC.BY_NAME[name]
    out, dev = run_case(name)
    only = _launch(c, dev["s"], dev["t"], dev["u"], scale=dev["scale"], mask=dev["mask"], want_grad=False)
    assert _same_bits(out, only, keys=OUTPUTS), name
    sflat = dev["sflat"].clone()
    rows = sflat[GUARD:GUARD + c.R * c.row].view(-1, c.row)
    got = _launch(c, rows, dev["t"], dev["u"], scale=dev["scale"], mask=dev["mask"], inplace=True)
    assert _same_bits(out, got, keys=OUTPUTS) and np.array_equal(got["grad"][:, :c.V], out["grad"][:, :c.V]), name
    keep = torch.ones(c.row, dtype=torch.bool, device="cuda")
    keep[:c.V] = False
    assert torch.equal(_bits(rows)[:, keep], _bits(dev["s"])[:, keep]) and torch.equal(_bits(sflat)[:GUARD], _bits(dev["sflat"])[:GUARD])
    assert torch.equal(_bits(sflat)[-GUARD:], _bits(dev["sflat"])[-GUARD:])


@pytest.mark.parametrize("name", ["c4096_R64", "c8192_f32_bf16", "c65536_g8", "four_bf16_reg", "bad_rows_reg_s1", "masked_bf16", "bad_rows_stream_s3", "c1000_vlm_mixed_s3"])
def test_run_to_run_alone_in_any_row_order_and_three_dimensional(name):
    """the same bits again; a row alone gives what it gave in the batch; the rows reversed give the reversed outputs -- a bad or ignored row beside it or not;
    [B, S, V] tensors give what their flattened rows give"""
    c = DC.BY_NAME[name]
    out, dev = run_case(name)
    assert _same_bits(out, _launch(c, dev["s"], dev["t"], dev["u"], scale=dev["scale"], mask=dev["mask"]))
    pick = lambda t, idx: None if t is None else t[idx].contiguous()
    for r in sorted({0, 1, c.R // 2, c.R - 1}):
        got = _launch(c._replace(R=1), dev["s"][r:r + 1], dev["t"][r:r + 1], None if dev["u"] is None else dev["u"][r:r + 1], scale=pick(dev["scale"], slice(r, r + 1)),
                      mask=pick(dev["mask"], slice(r, r + 1)))
        assert all(got[k][0].tobytes() == out[k][r].tobytes() for k in OUTPUTS + ("grad",)), (name, r)
    perm = torch.arange(c.R - 1, -1, -1, device="cuda")
    rev = _launch(c, pick(dev["s"], perm), pick(dev["t"], perm), pick(dev["u"], perm), scale=pick(dev["scale"], perm), mask=pick(dev["mask"], perm))
    p = perm.cpu().numpy()
    assert all(rev[k].tobytes() == out[k][p].tobytes() for k in OUTPUTS + ("grad",)) and rev["bad"] == out["bad"] and rev["ignored"] == out["ignored"]
    if c.R % 3 == 0:
        assert _same_bits(out, _launch(c, dev["s"], dev["t"], dev["u"], scale=dev["scale"], mask=dev["mask"], shape3=(c.R // 3, 3)))


@pytest.mark.parametrize("name", ["c2050_pads", "c4097_bf16_both_s3", "c8192_f32_bf16", "c65536_bf16_both_s1", "bad_rows_small_s3", "onehot", "four"])
def test_teacher_entropy_is_the_scorer_kernels_entropy(name):
    """kernel against kernel: ops.token_score at temperature 1 on the teacher's buffers, guided or not"""
    c = DC.BY_NAME[name]
    out, dev = run_case(name)
    w = c.offset + c.C
    ent = ops.token_score(dev["t"][:, :w], torch.zeros(c.R, dtype=torch.int64, device="cuda"), uncond_logits=None if dev["u"] is None else dev["u"][:, :w], C=c.C,
                          offset=c.offset, cfg_scale=1.0 if c.s is None else float(c.s), temperature=1.0)[4].cpu().numpy()
    ref = DC.reference(name)
    good = ~ref.bad & ~ref.ignored
    assert good.any() and np.array_equal(out["h"][good].view(u32), ent[good].view(u32)), name


@pytest.mark.parametrize("name", ["onehot", "onehot_reg_bf16"])
def test_one_hot_teacher_gradient_is_the_loss_kernels(name):
    """kernel against kernel: ops.token_xent on the student's buffer with the teacher's one finite code as the target, no row scale"""
    c = DC.BY_NAME[name]
    _, dev = run_case(name)
    mine = _launch(c, dev["s"], dev["t"], None)
    t = torch.from_numpy(np.argmax(DC.windows(name)[0], axis=1).astype(np.int64)).cuda()
    buf = torch.zeros(c.R, c.row, dtype=_tdt(c.sd), device="cuda")  # rows a multiple of four codes apart, as the student's are
    nll, lse, grad, _, _ = ops.token_xent(dev["s"][:, :c.V], t, C=c.C, offset=c.offset, grad=buf[:, :c.V])
    g = _bits(grad).cpu().numpy()
    assert np.array_equal(mine["grad"][:, :c.V], g.view(np.uint16) if c.sd == "bf16" else g.view(u32)) and mine["lse"].tobytes() == lse.cpu().numpy().tobytes()
    assert (_ulp_apart(mine["ce"], nll.cpu().numpy()) <= 1).all()


def test_graph_replay_equals_eager():
    name = "c8192_vlm"
    c = DC.BY_NAME[name]
    out, dev = run_case(name)
    grad = torch.zeros(c.R, c.row, device="cuda")
    o = {k: torch.zeros(c.R, device="cuda") for k in OUTPUTS}
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda: ops.token_distill(dev["s"][:, :c.V], dev["t"][:, :c.V], C=c.C, offset=c.offset, row_scale=dev["scale"], row_mask=dev["mask"], grad=grad[:, :c.V],
                                     kl=o["kl"], ce=o["ce"], h_teacher=o["h"], lse_student=o["lse"], bad=bad, ignored=ign)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in [grad] + list(o.values()):
        t.fill_(7.0)
    g.replay()
    torch.cuda.synchronize()
    assert all(o[k].cpu().numpy().tobytes() == out[k].tobytes() for k in OUTPUTS)
    assert np.array_equal(grad[:, :c.V].cpu().numpy().view(u32), out["grad"][:, :c.V]) and bool((grad[:, c.V:] == 7.0).all())


def test_no_rows_accumulating_counters_and_refusals():
    st = torch.zeros(0, 128, device="cuda")
    kl, ce, h, lse, grad, bad, ign = ops.token_distill(st, st.clone())
    assert kl.shape == (0,) and grad.shape == (0, 128) and int(bad.cpu()[0]) == 0 and int(ign.cpu()[0]) == 0
    name = "bad_rows_small"
    c = DC.BY_NAME[name]
    out, dev = run_case(name)
    bad, ign = torch.full((1,), 10, dtype=torch.int32, device="cuda"), torch.full((1,), 20, dtype=torch.int32, device="cuda")
    mask = torch.ones(c.R, dtype=torch.bool, device="cuda")
    mask[0] = False
    s, t = dev["s"][:, :c.V], dev["t"][:, :c.V]
    for _ in range(2):
        ops.token_distill(s, t, C=c.C, offset=c.offset, row_mask=mask, bad=bad, ignored=ign, want_grad=False)
    assert int(bad.cpu()[0]) == 10 + 2 * out["bad"] and int(ign.cpu()[0]) == 20 + 2
    before = _bits(dev["sflat"]).clone()
    for kw in (dict(cfg_scale=float("nan"), teacher_uncond=t), dict(C=c.C + 1), dict(grad=torch.as_strided(dev["sflat"], (c.R, c.V), (c.row, 1), GUARD + 4)), dict(grad=t),
               dict(grad=torch.zeros(c.R, c.V, device="cuda"), inplace=True), dict(grad=torch.zeros(c.R, c.V, device="cuda"), want_grad=False), dict(inplace=True, want_grad=False),
               dict(row_scale=torch.ones(c.R - 1, device="cuda")), dict(row_mask=torch.ones(c.R, dtype=torch.int32, device="cuda")),
               dict(grad=torch.zeros(c.R, c.V, dtype=torch.bfloat16, device="cuda")), dict(teacher_uncond=t.bfloat16())):
        with pytest.raises(Exception):
            ops.token_distill(s, t, **dict(dict(C=c.C, offset=c.offset), **kw))
    with pytest.raises(Exception):
        ops.token_distill(s, s, C=c.C, offset=c.offset, inplace=True)          # the teacher may not be the buffer the gradient lands in
    torch.cuda.synchronize()
    assert torch.equal(_bits(dev["sflat"]), before)                  # a refused call leaves its buffers untouched


# ---- the public functions -----------------------------------------------------------------------------------------------------------------------------
def _head_reference(logits, x, teacher, uncond, s, *, ar_order, steps, weights, reduction):
    """the same graph under F.kl_div in fp64 on the fp32 logits the head produced and the fp32 guided teacher -> (loss, dloss/dW, their bounds): the per-element
    bounds of tests/token_distill_cases.py carried through the reduction and the matmul dW = dlogits^T x, plus the fp32 rounding of the row scales (2^-24 each)
    and of the backward matmul itself ((R + 2) 2^-24 of the sum of absolute products)"""
    B, S, V = logits.shape
    live = torch.ones(B, S, dtype=torch.bool)
    if steps is not None:
        live = torch.arange(S).unsqueeze(0) < torch.as_tensor(steps).reshape(-1, 1)
    pos = (S - 1 - torch.arange(S)) if ar_order else torch.arange(S)
    w = torch.ones(B, S, dtype=torch.float64) if weights is None else (weights[pos].expand(B, S) if weights.dim() == 1 else weights).double()
    a = torch.from_numpy(DC.guided(teacher.numpy(), None if uncond is None else uncond.numpy(), s)).double()
    lg = logits.detach().double().cpu().requires_grad_(True)
    kl = F.kl_div(torch.log_softmax(lg, -1), torch.softmax(a, -1), reduction="none").sum(-1)
    zero = torch.zeros((), dtype=torch.float64)
    rows = torch.where(live, w * kl, zero)
    denom = torch.where(live, w, zero).sum()
    loss = rows if reduction == "none" else rows.sum() if reduction == "sum" else rows.sum() / denom
    up = torch.arange(1.0, B * S + 1, dtype=torch.float64).reshape(B, S) / (B * S) if reduction == "none" else torch.ones((), dtype=torch.float64)
    (loss * up).sum().backward()
    g_rows = (w * up / (denom if reduction == "mean" else 1.0)) * live
    x64 = x.detach().double().cpu().reshape(B * S, -1)
    dW = lg.grad.reshape(B * S, V).t() @ x64
    p, q = torch.softmax(a, -1).numpy(), torch.softmax(lg.detach(), -1).numpy()
    x_i, y_i = (lg.detach().max(-1, keepdim=True)[0] - lg.detach()).numpy(), (a.max(-1, keepdim=True)[0] - a).numpy()
    bg, b_rows = np.zeros((B * S, V)), np.zeros((B, S))
    for r in range(B * S):
        b, st = divmod(r, S)
        if live[b, st]:
            bg[r] = DC.bound_grad(V, p[b, st], q[b, st], float(g_rows[b, st])) + 2.0 ** -23 * np.abs(lg.grad[b, st].numpy())
            far = y_i[b, st] > 22.0
            ex, ea = float((p[b, st] * x_i[b, st])[~far].sum()), float((p[b, st] * y_i[b, st]).sum())
            b_rows[b, st] = float(w[b, st]) * DC.bound_kl(V, float(kl[b, st]), ex, ea, float((p[b, st] * x_i[b, st])[far].sum()), float((p[b, st] * y_i[b, st])[far].sum()))
    ax = np.abs(x64.numpy())
    b_dW = bg.T @ ax + (B * S + 2) * 2.0 ** -24 * (np.abs(lg.grad.reshape(B * S, V).numpy()).T @ ax)
    if reduction == "none":
        b_loss = b_rows + np.abs(rows.detach().numpy()) * 2.0 ** -24
    else:
        b_loss = b_rows.sum() / (float(denom) if reduction == "mean" else 1.0) + abs(float(loss.detach())) * 2.0 ** -23
    return loss.detach().numpy(), dW.numpy(), b_loss, b_dW


HEAD_CASES = [dict(reduction="mean"), dict(reduction="sum"), dict(reduction="none"), dict(reduction="mean", weights="S", guided=3.0), dict(reduction="sum", weights="BS", steps=[6, 3, 0, 5]),
              dict(reduction="none", weights="S", steps=[6, 3, 0, 5], guided=1.0), dict(reduction="mean", ar_order=False, steps=[1, 2, 3, 4], tdtype="bf16"),
              dict(reduction="mean", inplace=True, guided=3.0)]


@pytest.mark.parametrize("kw", HEAD_CASES, ids=lambda k: "-".join(f"{a}={b}" for a, b in k.items()))
def test_token_distillation_through_a_linear_head(kw):
    """loss and head.weight.grad within the derived bound, carried through the matmul, of F.kl_div in fp64 on the same logits; the loss times 3 before
    backward() triples every gradient; the teacher gets no gradient"""
    B, S, D, V = 4, 6, 32, 300
    g = torch.Generator().manual_seed(12)
    head = torch.nn.Linear(D, V).cuda()
    x = torch.randn(B, S, D, generator=g).cuda()
    tdt = torch.bfloat16 if kw.get("tdtype") == "bf16" else torch.float32
    teacher = torch.randn(B, S, V, generator=g).to(tdt)
    s = kw.get("guided")
    uncond = None if s is None else (teacher.float() - 0.5 * torch.randn(B, S, V, generator=g)).to(tdt)
    weights = {"S": torch.rand(S, generator=g) + 0.5, "BS": torch.rand(B, S, generator=g) + 0.5, None: None}[kw.get("weights")]
    red, steps, ar = kw["reduction"], kw.get("steps"), kw.get("ar_order", True)
    t_dev = teacher.cuda().requires_grad_(True)
    call = lambda lg: losses.token_distillation(lg, t_dev, teacher_uncond=None if uncond is None else uncond.cuda(), cfg_scale=1.0 if s is None else s, ar_order=ar, steps=steps,
                                                weights=None if weights is None else weights.cuda(), reduction=red, inplace=kw.get("inplace", False))
    up = (torch.arange(1.0, B * S + 1).reshape(B, S) / (B * S)).cuda() if red == "none" else None
    grads = []
    for times in (1.0, 3.0):
        head.zero_grad()
        logits = head(x)
        kept = logits.detach().clone()
        loss = call(logits)
        ((loss * up).sum() * times if up is not None else loss * times).backward()
        grads.append(head.weight.grad.clone())
    assert t_dev.grad is None
    want_loss, want_dW, b_loss, b_dW = _head_reference(kept, x, teacher.float(), None if uncond is None else uncond.float(), s, ar_order=ar, steps=steps, weights=weights, reduction=red)
    e_loss, e_dW = np.abs(loss.detach().double().cpu().numpy() - want_loss), np.abs(grads[0].double().cpu().numpy() - want_dW)
    share = lambda e, b: float(np.max(np.where(b > 0, e / np.where(b > 0, b, 1.0), 0.0)))
    print(f"\nloss share of the bound {share(e_loss, b_loss):.3f}, weight gradient share {share(e_dW, b_dW):.3f}")
    assert (e_loss <= b_loss).all() and (e_dW <= b_dW).all() and float(np.abs(want_dW).max()) > 1e-3
    # tripled: both runs round the scaled gradient rows (2^-24 each) and the backward matmul ((R + 2) 2^-24 of the absolute products, which b_dW holds once)
    # on their own, the second at three times the size: 3 (2 (R + 2) + 3) 2^-24 of the absolute products in all, under 8 b_dW
    assert (np.abs(grads[1].double().cpu().numpy() - 3.0 * grads[0].double().cpu().numpy()) <= 8.0 * b_dW).all()
    if kw.get("inplace"):
        assert not torch.equal(logits.detach(), kept)               # the logits are gone


def test_token_distillation_memory_synchronisation_second_backward_and_token_kl():
    R, V = 256, 32768
    teacher = torch.randn(4, 64, V, device="cuda")
    size = R * V * 4
    for inplace in (True, False):
        logits = torch.randn(4, 64, V, device="cuda").requires_grad_(True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        torch.cuda.set_sync_debug_mode("error")                     # a forward call synchronises nothing and reads nothing back
        try:
            loss, st = losses.token_distillation(logits, teacher, inplace=inplace, return_stats=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert (peak < 1 << 20) if inplace else (size <= peak < size + (1 << 20)), (inplace, peak)
        assert st.kl.shape == (4, 64) and int(st.bad.cpu()[0]) == 0 and math.isfinite(float(loss.detach()))
    loss.backward(retain_graph=True)
    assert logits.grad is not None and abs(float(logits.grad.double().sum())) < 1.0
    with pytest.raises(RuntimeError):
        loss.backward()
    small = torch.randn(2, 3, 64, device="cuda").requires_grad_(True)
    loss = losses.token_distillation(small, teacher[:2, :3, :64].contiguous())
    (gr,) = torch.autograd.grad(loss, small, create_graph=True)
    if gr.requires_grad:                                            # once_differentiable: differentiating a second time is an error
        with pytest.raises(RuntimeError):
            gr.sum().backward()
    # token_kl: the same kl the loss reports, no gradient buffer, a reduction per tokenizer position
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = sampling.token_kl(teacher, logits.detach(), steps=[64, 64, 10, 0])
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < 1 << 20
    assert torch.equal(out.kl[:2], st.kl[:2]) and int(out.ignored.cpu()[0]) == 54 + 64 and bool((out.kl[3] == 0).all())
    pp = out.per_position().cpu().numpy()
    assert pp.shape == (64,) and np.isfinite(pp).all() and pp[63] == pytest.approx(float(out.kl[:3, 0].double().mean())) and pp[0] == pytest.approx(float(out.kl[:2, 63].double().mean()))
    assert float(out.mean()) == pytest.approx(float(out.kl.double().sum()) / (64 + 64 + 10))


def test_zz_report_the_allowance_used():
    """not a check of the kernel: prints how many rows needed the one-ulp allowance on an output"""
    print(f"\n{ALLOWANCE['rows']} good rows compared: {ALLOWANCE['ulp_rows']} with kl, ce, h_teacher or lse_student one ulp from numpy's")
