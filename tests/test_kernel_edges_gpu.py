"""-m gpu: the joint attention (csrc/attention.hip) and the residual + LayerNorm + adaLN pass (csrc/elementwise.hip) at their tile
and walk edges, against plain fp64 references (tests/edge_cases.py).

Accuracy gate per case: the kernel's rms / max error against fp64 is at most 2x / 4x that of torch's fp32 implementation of the
same operation (+ 1e-8 / 1e-7).  Every case prints its measured ratios (kernel error / torch fp32 error).
Exact properties are checked bit for bit: batch slices, kvis versus truncation, split outputs, untouched dead rows."""
import time

import pytest
import torch

import edge_cases as E
from selftoktokenizer_amd import ops

pytestmark = pytest.mark.gpu

MODES = [0, ops.ATTN_F16X2]
MODE_NAME = {0: "fp32", ops.ATTN_F16X2: "f16x2"}
SENT32 = 0x7FC0DEAD          # NaN sentinel of the fp32 output buffers (int32 bit pattern)
SENT16 = 0x7E5A              # NaN sentinel of the fp16 split planes (int16 bit pattern)
_T0 = time.time()


@pytest.fixture(scope="module", autouse=True)
def _wall_time():
    yield
    print(f"\n[edge] wall time of tests/test_kernel_edges_gpu.py: {time.time() - _T0:.1f} s")


def _report(tag, acc_k, acc_t):
    rb, mb = E.gate(acc_t.rms, acc_t.mx)
    print(f"[edge] {tag}: rms {acc_k.rms:.3e} / torch {acc_t.rms:.3e} = {acc_k.rms / max(acc_t.rms, 1e-300):.2f}x (gate {rb:.3e}); "
          f"max {acc_k.mx:.3e} / torch {acc_t.mx:.3e} = {acc_k.mx / max(acc_t.mx, 1e-300):.2f}x (gate {mb:.3e})")
    assert acc_k.n == acc_t.n and acc_k.n > 0
    assert acc_k.rms <= rb, f"{tag}: rms error {acc_k.rms:.3e} > {rb:.3e}"
    assert acc_k.mx <= mb, f"{tag}: max error {acc_k.mx:.3e} > {mb:.3e}"


# ---------------------------------------------------------------------------------------------------------------------------------
# joint attention
# ---------------------------------------------------------------------------------------------------------------------------------
def _out_buf(B, rows, D):
    """sentinel-filled [B, rows + pad, D + 128] buffer and its [B, rows, D] column-slice view"""
    buf = torch.full((B, rows + E.OUT_ROW_PAD, D + 128), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[:, :rows, E.OUT_COL_OFF:E.OUT_COL_OFF + D]


def _split_buf(B, rows, D):
    s = ops.SplitAct((B, rows, D), "cuda")
    s.data.view(torch.int16).fill_(SENT16)
    return s


def _launch(case, cb, xb, kvis, mode, Kc=None, split=False, flag=None):
    """one ops.attention call on views: segment 0 = cb[:, :Kc] (batch stride != Kc * row stride), segment 1 = xb[:, :nx];
    outputs are column slices of sentinel-filled buffers (or sentinel-filled SplitActs).  Returns (ctx out, img out)."""
    Kc = case.Kc if Kc is None else Kc
    B, D, nx = cb.shape[0], case.D, case.nx
    c, x = cb[:, :Kc], xb[:, :nx]
    if split:
        oc = None if case.pre_only else _split_buf(B, Kc, D)
        ox = _split_buf(B, nx, D)
        oc_v, ox_v = oc, ox
    else:
        oc, oc_v = (None, None) if case.pre_only else _out_buf(B, Kc, D)
        ox, ox_v = _out_buf(B, nx, D)
    seg0 = (None if case.pre_only else c[..., :D], c[..., D:2 * D], c[..., 2 * D:3 * D], oc_v)
    seg1 = (x[..., :D], x[..., D:2 * D], x[..., 2 * D:3 * D], ox_v)
    ops.attention(seg0, seg1, case.H, 64, kvis=kvis, seg0_sees_seg1=case.see, mode=mode, overflow=flag)
    return oc, ox


def _live_mask(B, rows, D, n_live):
    """True where a kernel may write: rows [0, n_live[b]) and this launch's head columns"""
    m = torch.zeros(B, rows + E.OUT_ROW_PAD, D + 128, dtype=torch.bool, device="cuda")
    for b in range(B):
        m[b, :n_live[b], E.OUT_COL_OFF:E.OUT_COL_OFF + D] = True
    return m


def _check_sentinel(tag, buf, live):
    bits = buf.view(torch.int32)
    assert bool((bits[~live] == SENT32).all()), f"{tag}: an element outside the live rows / head columns was written"
    assert bool(torch.isfinite(buf[live]).all()), f"{tag}: a live output element was not written (or is not finite)"


def _check_split_sentinel(tag, s, n_live):
    p = s.planes().view(torch.int16)                       # [2, B, rows, D]
    for b in range(p.shape[1]):
        assert bool((p[:, b, n_live[b]:] == SENT16).all()), f"{tag}: split plane rows past the live ones were written (b={b})"


_REF = {}


def _references(case, cb, xb):
    """{(b, h): (fp64 ctx, fp64 img, torch-fp32 ctx, torch-fp32 img)} for the case's checked pairs (cached across modes)"""
    if case.name not in _REF:
        out = {}
        by_b = {}
        for b, h in case.checked_pairs():
            by_b.setdefault(b, []).append(h)
        for b, hs in by_b.items():
            c64, x64 = E.attn_reference(case, b, cb[b], xb[b], True, hs)
            c32, x32 = E.attn_reference(case, b, cb[b], xb[b], False, hs)
            for i, h in enumerate(hs):
                out[(b, h)] = (None if c64 is None else c64[i], x64[i], None if c32 is None else c32[i], x32[i])
        _REF[case.name] = out
    return _REF[case.name]


def _accuracy(tag, case, cb, xb, oc, ox):
    refs = _references(case, cb, xb)
    acc_k, acc_t = E.ErrAcc(), E.ErrAcc()
    oc_c = None if oc is None else oc[:, :case.Kc, E.OUT_COL_OFF:E.OUT_COL_OFF + case.D].cpu()
    ox_c = ox[:, :case.nx, E.OUT_COL_OFF:E.OUT_COL_OFF + case.D].cpu()
    for (b, h), (c64, x64, c32, x32) in refs.items():
        acc_k.add(ox_c[b, :, h * 64:(h + 1) * 64], x64)
        acc_t.add(x32, x64)
        if c64 is not None:
            n0 = case.n0(b)
            acc_k.add(oc_c[b, :n0, h * 64:(h + 1) * 64], c64)
            acc_t.add(c32, c64)
    _report(tag, acc_k, acc_t)


def _n_live_ctx(case):
    return [0 if case.pre_only else case.n0(b) for b in range(case.B)]


def _full_check(case, mode, cb, xb, kvis):
    """main launch: sentinels, accuracy against fp64, split outputs and the overflow flag; returns the fp32 outputs"""
    tag = f"{case.name} {MODE_NAME[mode]}"
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    oc, ox = _launch(case, cb, xb, kvis, mode, flag=flag)
    torch.cuda.synchronize()
    if oc is not None:
        _check_sentinel(tag + " ctx", oc, _live_mask(case.B, case.Kc, case.D, _n_live_ctx(case)))
    _check_sentinel(tag + " img", ox, _live_mask(case.B, case.nx, case.D, [case.nx] * case.B))
    _accuracy(tag, case, cb, xb, oc, ox)
    if mode == ops.ATTN_F16X2:
        sc, sx = _launch(case, cb, xb, kvis, mode, split=True, flag=flag)
        v = lambda o, rows: o[:, :rows, E.OUT_COL_OFF:E.OUT_COL_OFF + case.D]
        assert torch.equal(sx.planes(), ops.split_f16x2(v(ox, case.nx)).planes()), f"{tag}: image split planes != split_f16x2(fp32 outputs)"
        _check_split_sentinel(tag + " img split", sx, [case.nx] * case.B)
        if sc is not None:
            ref_planes, got = ops.split_f16x2(v(oc, case.Kc)).planes(), sc.planes()
            for b, n in enumerate(_n_live_ctx(case)):
                assert torch.equal(got[:, b, :n], ref_planes[:, b, :n]), f"{tag}: context split planes != split_f16x2 (b={b})"
            _check_split_sentinel(tag + " ctx split", sc, _n_live_ctx(case))
    assert int(flag.item()) == 0, f"{tag}: overflow flag raised on in-range inputs"
    return oc, ox


def _kvis_t(case):
    return None if case.kvis is None else torch.tensor(case.kvis, dtype=torch.int32, device="cuda")


@pytest.mark.parametrize("mode", MODES, ids=lambda m: MODE_NAME[m])
@pytest.mark.parametrize("case", E.ATTN_KVIS_CASES, ids=lambda c: c.name)
def test_attention_kvis_sweep(case, mode):
    """one launch, one sample per kvis value (-1 .. Kc - 1 around the 32-key and 128-row tile edges); poisoned invisible keys;
    then bit for bit: every sample alone, and kvis = k against the context truncated to k + 1 keys with kvis = None"""
    cb, xb = E.attn_buffers(case, "cuda")
    kvis = _kvis_t(case)
    oc, ox = _full_check(case, mode, cb, xb, kvis)
    for b in range(case.B):
        oc1, ox1 = _launch(case, cb[b:b + 1], xb[b:b + 1], kvis[b:b + 1], mode)
        assert torch.equal(ox1.view(torch.int32)[0], ox.view(torch.int32)[b]), f"sample {b} alone: image rows differ"
        if oc is not None:
            assert torch.equal(oc1.view(torch.int32)[0], oc.view(torch.int32)[b]), f"sample {b} alone: context rows differ"
        n = case.n0(b)
        oct, oxt = _launch(case, cb[b:b + 1], xb[b:b + 1], None, mode, Kc=n)
        assert torch.equal(oxt.view(torch.int32)[0], ox.view(torch.int32)[b]), f"kvis={case.kvis[b]}: image rows != truncated context"
        if oc is not None and n > 0:
            cols = slice(E.OUT_COL_OFF, E.OUT_COL_OFF + case.D)
            assert torch.equal(oct.view(torch.int32)[0, :n, cols], oc.view(torch.int32)[b, :n, cols]), \
                f"kvis={case.kvis[b]}: live context rows != truncated context"


@pytest.mark.parametrize("mode", MODES, ids=lambda m: MODE_NAME[m])
@pytest.mark.parametrize("case", E.ATTN_LEN_CASES, ids=lambda c: c.name)
def test_attention_truncated_lengths(case, mode):
    """the decode's truncated context lengths (kvis = None) x the image grids, rows past `len` poisoned"""
    cb, xb = E.attn_buffers(case, "cuda")
    _full_check(case, mode, cb, xb, None)


@pytest.mark.parametrize("mode", MODES, ids=lambda m: MODE_NAME[m])
def test_attention_product_shape(mode):
    """B = 64, H = 24, n = 358, nx = 256, per-sample kvis: the whole output's sentinels, fp64 on a seeded sample of (b, h)"""
    case = E.ATTN_PRODUCT_CASE
    cb, xb = E.attn_buffers(case, "cuda")
    _full_check(case, mode, cb, xb, _kvis_t(case))


@pytest.mark.parametrize("L", E.HD16_L)
def test_attention_head_dim16(L):
    """attn16_kernel (one workgroup per (sample, head), K / V of the head in dynamic LDS) up to the dispatcher's 1024 rows"""
    buf = E.hd16_buffer(L, "cuda")
    D = E.HD16_H * 16
    t = buf[:, :L]
    ob, ov = _out_buf(E.HD16_B, L, D)
    ops.attention(None, (t[..., :D], t[..., D:2 * D], t[..., 2 * D:3 * D], ov), E.HD16_H, 16)
    torch.cuda.synchronize()
    _check_sentinel(f"hd16 L={L}", ob, _live_mask(E.HD16_B, L, D, [L] * E.HD16_B))
    r64, r32 = E.hd16_reference(buf, L, True), E.hd16_reference(buf, L, False)
    acc_k, acc_t = E.ErrAcc(), E.ErrAcc()
    acc_k.add(ov.cpu(), r64)
    acc_t.add(r32, r64)
    _report(f"hd16 L={L}", acc_k, acc_t)


# ---------------------------------------------------------------------------------------------------------------------------------
# residual_ln_mod
# ---------------------------------------------------------------------------------------------------------------------------------
def _ln_call(case, x, y, mt, gt, split=None, overflow=None):
    H = case.H
    kw = {}
    if mt is not None:
        kw.update(shift=mt[:, 0:H], scale=mt[:, H:2 * H], per_sample=case.mod == "sample")
    if gt is not None and y is not None:
        kw.update(gate=gt[:, 2 * H:3 * H], gate_per_sample=case.gate == "sample")
    return ops.residual_ln_mod(x, y=y, want_x=case.want_x, want_n=case.want_n, split=case.split if split is None else split,
                               overflow=overflow, **kw)


def _slice_table(t, lay, b):
    return None if t is None else (t[b:b + 1] if lay == "sample" else t)


@pytest.mark.parametrize("case", E.LN_CASES, ids=lambda c: c.name)
def test_residual_ln_mod_walk(case):
    plan = case.plan()
    print(f"[edge] {case.name}: plan (walk_tokens, R, tail, HM, HG) = {plan}")
    x, y, mt, gt = E.ln_inputs(case, "cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    xo, n = _ln_call(case, x, y, mt, gt, overflow=flag)
    xp64, n64 = E.ln_reference(case, x, y, mt, gt, torch.float64)
    xp32, n32 = E.ln_reference(case, x, y, mt, gt, torch.float32)
    if y is not None and case.want_x:
        if gt is None:
            assert torch.equal(xo, x + y), "x' = x + y is not bit-equal to torch"
        else:   # torch's two roundings or one correctly rounded FMA: neither is further from the exact value
            bound = (xp32.double() - xp64).abs() + 2.0 ** -50 * xp64.abs()
            assert bool(((xo.double() - xp64).abs() <= bound).all()), "x' = x + g y further from fp64 than torch fp32"
    else:
        assert xo is None or xo is x
    if case.want_n:
        n_f = n
        if case.split:
            assert int(flag.item()) == 0
            plain = E.LnCase(**{**case.__dict__, "split": False})
            _, n_f = _ln_call(plain, x, y, mt, gt, split=False)
            assert torch.equal(n.planes(), ops.split_f16x2(n_f).planes()), "split output != split_f16x2 of the fp32 output"
        acc_k, acc_t = E.ErrAcc(), E.ErrAcc()
        acc_k.add(n_f, n64)
        acc_t.add(n32, n64)
        _report(case.name, acc_k, acc_t)
    else:
        assert n is None
    # batch invariance: every row equals the same row computed by a one-sample call, which runs at R = 1 (elementwise.hip:130)
    for b in range(case.B):
        p1 = E.ln_walk_plan(1, case.T, case.H, case.mod, case.gate, case.y)
        assert p1 is None or p1[1] == 1
        yb = None if y is None else y[b:b + 1].contiguous()
        xo1, n1 = _ln_call(case, x[b:b + 1].contiguous(), yb, _slice_table(mt, case.mod, b), _slice_table(gt, case.gate, b))
        if y is not None and case.want_x:
            assert torch.equal(xo1[0], xo[b]), f"x' of sample {b} differs from its one-sample call"
        if case.want_n:
            got = n.planes()[:, b] if case.split else n[b]
            one = n1.planes()[:, 0] if case.split else n1[0]
            assert torch.equal(got, one), f"n of sample {b} differs from its one-sample call"


def test_residual_ln_mod_split_overflow_flag():
    """split mode: one token's scale row = 2000 and one spike in x in the last row of a ragged walk -> flag bit 0; without the
    spike the flag stays 0.  fp64 on the CPU confirms that only that row's output exceeds 65504."""
    case, t, b = E.LN_OVF_CASE, E.LN_OVF_TOKEN, E.LN_OVF_SAMPLE
    walk_tokens, R, tail, _, _ = case.plan()
    assert walk_tokens == 0 and tail > 1 and b == case.B - 1          # b is the last row of the ragged walk over samples
    x, y, mt, gt = E.ln_inputs(case, "cpu")
    mt[t, case.H:2 * case.H] = E.LN_OVF_SCALE
    for spike in (False, True):
        xs = x.clone()
        if spike:
            xs[b, t, E.LN_OVF_COL] = E.LN_OVF_SPIKE
        _, n64 = E.ln_reference(case, xs, y, mt, gt, torch.float64)
        over = (n64.abs() >= 65504).any(-1)
        expect = torch.zeros_like(over)
        if spike:
            expect[b, t] = True
        assert torch.equal(over, expect), f"fp64: rows over the fp16 range {over.nonzero().tolist()}"
        flag = torch.zeros(1, dtype=torch.int32, device="cuda")
        _ln_call(case, xs.cuda(), y.cuda(), mt.cuda(), gt.cuda(), overflow=flag)
        assert (int(flag.item()) & 1) == int(spike), f"spike={spike}: flag {int(flag.item())}"
