"""-m gpu: the joint attention with a per-sample key bit mask (selftok_attn_kmask_f32) against plain fp64 references
(tests/kmask_cases.py), in both arithmetics and on every route of the dispatcher (LDS-DMA staged, register staged, f16x2 with and
without split-plane outputs).

Accuracy gate per case: pooled rms / max error against fp64 at most 2x / 4x that of torch's fp32 attention on the same visible key
set (+ 1e-8 / 1e-7), edge_cases.gate.  Every (b, h) pair and every live row of every case is compared.
Exact properties are bit for bit: prefix masks versus kvis, each sample alone, the full mask versus no mask, poisoned invisible
contents; dead rows, rows past `len`, neighbouring columns and dead rows' split planes keep their NaN sentinels."""
import numpy as np
import pytest
import torch

import edge_cases as E
import kmask_cases as KM
from selftoktokenizer_amd import _lib, ops

pytestmark = pytest.mark.gpu

MODE_NAME = {0: "fp32", ops.ATTN_F16X2: "f16x2"}
SENT32 = 0x7FC0DEAD
SENT16 = 0x7E5A
# every route the dispatcher can take: mode 0 LDS-DMA staged, mode 0 register staged (K / V rows off a 16-byte boundary), f16x2
ROUTES = [(0, False), (0, True), (ops.ATTN_F16X2, False)]
ROUTE_ID = lambda r: MODE_NAME[r[0]] + ("_register_staged" if r[1] else "")
# the product shape runs once per arithmetic
CASE_ROUTES = [(c, r) for c in KM.CASES for r in ROUTES if not (c is KM.PRODUCT_CASE and r[1])]


def _words(masks: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(KM.pack_words(masks).view(np.int32)).cuda()


def _out_buf(B, rows, D):
    buf = torch.full((B, rows + E.OUT_ROW_PAD, D + 128), SENT32, dtype=torch.int32, device="cuda").view(torch.float32)
    return buf, buf[:, :rows, E.OUT_COL_OFF:E.OUT_COL_OFF + D]


def _split_buf(B, rows, D):
    s = ops.SplitAct((B, rows, D), "cuda")
    s.data.view(torch.int16).fill_(SENT16)
    return s


def _launch(case, cb, xb, mode, kmask=None, kvis=None, split=False, flag=None, unaligned=False, Kc=None):
    """one ops.attention call on strided views (segment 0 = cb[:, :Kc] of a longer, wider buffer); outputs are column slices of
    sentinel-filled buffers or sentinel-filled SplitActs.  unaligned: K / V views start 4 bytes off a 16-byte boundary, which sends
    mode 0 to the register-staged kernel."""
    Kc = case.Kc if Kc is None else Kc
    B, D, nx = cb.shape[0], case.D, case.nx
    if unaligned:
        def shift(t):
            w = torch.empty(t.shape[0], t.shape[1], t.shape[2] + 4, device="cuda")
            w[..., 1:1 + t.shape[2]] = t
            return w[..., 1:1 + t.shape[2]]
        # row strides must stay multiples of 4 floats: the view starts 1 float into a buffer 4 floats wider
        cb, xb = shift(cb), shift(xb)
        assert cb.data_ptr() % 16 == 4
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
    ops.attention(seg0, seg1, case.H, 64, kvis=kvis, seg0_sees_seg1=case.see, mode=mode, overflow=flag, kmask=kmask)
    return oc, ox


def _live(case, rows, D, row_masks):
    m = torch.zeros(len(row_masks), rows + E.OUT_ROW_PAD, D + 128, dtype=torch.bool, device="cuda")
    for b, rm in enumerate(row_masks):
        m[b, :rows, E.OUT_COL_OFF:E.OUT_COL_OFF + D] = torch.from_numpy(np.asarray(rm, dtype=bool)).cuda()[:, None]
    return m


def _ctx_row_masks(case):
    return [np.zeros(case.Kc, bool) if case.pre_only else case.mask(b)[:case.Kc] for b in range(case.B)]


def _check_sentinel(tag, buf, live):
    bits = buf.view(torch.int32)
    assert bool((bits[~live] == SENT32).all()), f"{tag}: an element outside the live rows / head columns was written"
    assert bool(torch.isfinite(buf[live]).all()), f"{tag}: a live output element was not written (or is not finite)"


def _check_split_sentinel(tag, s, row_masks):
    p = s.planes().view(torch.int16)                       # [2, B, rows, D]
    for b, rm in enumerate(row_masks):
        dead = torch.from_numpy(~np.asarray(rm, dtype=bool)).cuda()
        assert bool((p[:, b, dead] == SENT16).all()), f"{tag}: split planes of dead rows were written (b={b})"


def _accuracy(tag, case, cb, xb, oc, ox):
    acc_k, acc_t = E.ErrAcc(), E.ErrAcc()
    v = lambda o, rows: o[:, :rows, E.OUT_COL_OFF:E.OUT_COL_OFF + case.D].cpu()
    oc_c, ox_c = (None if oc is None else v(oc, case.Kc)), v(ox, case.nx)
    cbc, xbc = cb.cpu(), xb.cpu()
    for b in range(case.B):                                 # every (b, h) pair, every live row
        vis = case.visible(b)
        c64, x64 = KM.reference(case, b, cbc[b], xbc[b], True)
        c32, x32 = KM.reference(case, b, cbc[b], xbc[b], False)
        got_x = ox_c[b].reshape(case.nx, case.H, 64).transpose(0, 1)
        acc_k.add(got_x, x64); acc_t.add(x32, x64)
        if c64 is not None:
            got_c = oc_c[b][torch.from_numpy(vis)].reshape(len(vis), case.H, 64).transpose(0, 1)
            acc_k.add(got_c, c64); acc_t.add(c32, c64)
    rb, mb = E.gate(acc_t.rms, acc_t.mx)
    print(f"[kmask] {tag}: rms {acc_k.rms:.3e} / torch {acc_t.rms:.3e} (gate {rb:.3e}); max {acc_k.mx:.3e} / torch {acc_t.mx:.3e} (gate {mb:.3e}); "
          f"{acc_k.n} elements")
    assert acc_k.n == acc_t.n and acc_k.n > 0
    assert acc_k.rms <= rb, f"{tag}: rms error {acc_k.rms:.3e} > {rb:.3e}"
    assert acc_k.mx <= mb, f"{tag}: max error {acc_k.mx:.3e} > {mb:.3e}"


def _bits(t):
    return t.view(torch.int32)


def _eq_live(tag, a, b, live):
    """bit for bit on every live element"""
    assert torch.equal(_bits(a)[live], _bits(b)[live]), f"{tag}: live rows differ"


@pytest.mark.parametrize("case,route", CASE_ROUTES, ids=lambda v: v.name if isinstance(v, KM.KCase) else ROUTE_ID(v))
def test_kmask_accuracy_sentinels_and_exact_properties(case, route):
    """accuracy vs fp64 on every pair; sentinels; split planes; each sample alone; poisoned invisible contents: bit for bit"""
    mode, unaligned = route
    tag = f"{case.name} {ROUTE_ID(route)}"
    cb, xb = KM.buffers(case, "cuda")
    km = _words(case.masks())
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    oc, ox = _launch(case, cb, xb, mode, kmask=km, flag=flag, unaligned=unaligned)
    torch.cuda.synchronize()
    rows_c = _ctx_row_masks(case)
    live_c = _live(case, case.Kc, case.D, rows_c)
    live_x = _live(case, case.nx, case.D, [np.ones(case.nx, bool)] * case.B)
    if oc is not None:
        _check_sentinel(tag + " ctx", oc, live_c)
    _check_sentinel(tag + " img", ox, live_x)
    _accuracy(tag, case, cb, xb, oc, ox)
    v = lambda o, rows: o[:, :rows, E.OUT_COL_OFF:E.OUT_COL_OFF + case.D]
    if mode == ops.ATTN_F16X2:
        sc, sx = _launch(case, cb, xb, mode, kmask=km, split=True, flag=flag)
        assert torch.equal(sx.planes(), ops.split_f16x2(v(ox, case.nx)).planes()), f"{tag}: image split planes != split_f16x2(fp32 outputs)"
        if sc is not None:
            ref_planes, got = ops.split_f16x2(torch.nan_to_num(v(oc, case.Kc))).planes(), sc.planes()
            for b, rm in enumerate(rows_c):
                r = torch.from_numpy(rm).cuda()
                assert torch.equal(got[:, b, r], ref_planes[:, b, r]), f"{tag}: context split planes != split_f16x2 (b={b})"
            _check_split_sentinel(tag + " ctx split", sc, rows_c)
    # (d) poisoned invisible keys (NaN / Inf k, NaN / POISON_V v) and dead rows' q (NaN): no bit of a live row moves, no overflow flag
    pcb, pxb = KM.buffers(case, "cuda", poison=True)
    poc, pox = _launch(case, pcb, pxb, mode, kmask=km, flag=flag, unaligned=unaligned)
    _eq_live(tag + " poisoned img", pox, ox, live_x)
    if oc is not None:
        _eq_live(tag + " poisoned ctx", poc, oc, live_c)
        _check_sentinel(tag + " poisoned ctx", poc, live_c)
    assert int(flag.item()) == 0, f"{tag}: overflow flag raised by in-range visible inputs (invisible keys are poisoned)"
    # (b) each sample alone equals the sample inside the batch
    if case is not KM.PRODUCT_CASE:
        for b in range(case.B):
            oc1, ox1 = _launch(case, cb[b:b + 1], xb[b:b + 1], mode, kmask=km[b:b + 1], unaligned=unaligned)
            assert torch.equal(_bits(ox1)[0], _bits(ox)[b]), f"{tag}: sample {b} ({case.patterns[b][0]}) alone: image rows differ"
            if oc is not None:
                assert torch.equal(_bits(oc1)[0], _bits(oc)[b]), f"{tag}: sample {b} ({case.patterns[b][0]}) alone: context rows differ"


@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_ID)
@pytest.mark.parametrize("see,pre_only", [(True, False), (False, False), (True, True)])
def test_prefix_mask_equals_kvis_and_full_mask_equals_no_mask(see, pre_only, route):
    """(a) bits 0..k == selftok_attn_f32 with kvis = k for every k of edge_cases.KVIS_512, split planes included; (c) full mask == kvis NULL"""
    mode, unaligned = route
    K = 512
    a = np.arange(K)
    case = KM.KCase(f"prefix_vs_kvis_see{int(see)}_pre{int(pre_only)}", 2, K, 256, tuple(KM._pat(f"k{k}", a <= k) for k in E.KVIS_512), see, K, pre_only)
    cb, xb = KM.buffers(case, "cuda")
    km = _words(case.masks())
    kvis = torch.tensor(E.KVIS_512, dtype=torch.int32, device="cuda")
    live_c = _live(case, K, case.D, _ctx_row_masks(case))
    for split in ([False, True] if mode == ops.ATTN_F16X2 else [False]):
        oc_m, ox_m = _launch(case, cb, xb, mode, kmask=km, split=split, unaligned=unaligned)
        oc_k, ox_k = _launch(case, cb, xb, mode, kvis=kvis, split=split, unaligned=unaligned)
        if split:
            assert torch.equal(ox_m.planes(), ox_k.planes())
            if oc_m is not None:
                assert torch.equal(oc_m.planes().view(torch.int16), oc_k.planes().view(torch.int16)), "context split planes (sentinels included) differ"
        else:
            assert torch.equal(_bits(ox_m), _bits(ox_k)), "prefix mask: image rows differ from kvis"
            if oc_m is not None:
                assert torch.equal(_bits(oc_m), _bits(oc_k)), "prefix mask: context buffer (sentinels included) differs from kvis"
                _check_sentinel("prefix ctx", oc_m, live_c)
    full = KM.KCase("full_vs_none", 2, K, 256, tuple(KM._pat("full", a >= 0) for _ in range(3)), see, K, pre_only)
    cb, xb = KM.buffers(full, "cuda")
    oc_m, ox_m = _launch(full, cb, xb, mode, kmask=_words(full.masks()), unaligned=unaligned)
    oc_n, ox_n = _launch(full, cb, xb, mode, unaligned=unaligned)
    assert torch.equal(_bits(ox_m), _bits(ox_n)) and (oc_m is None or torch.equal(_bits(oc_m), _bits(oc_n))), "full mask differs from kvis = NULL"


def test_kmask_refusals():
    case = KM.KCase("refuse", 2, 512, 64, (KM._pat("full", np.ones(512, bool)),) * 2, True, 512)
    cb, xb = KM.buffers(case, "cuda")
    km = _words(case.masks())
    with pytest.raises(_lib.SelftokHipError, match="exclusive"):
        _launch(case, cb, xb, 0, kmask=km, kvis=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="kmask_bs"):
        _launch(case, cb, xb, 0, kmask=km[:, :15].contiguous())
    q = torch.zeros(2, 64, 64, device="cuda")
    with pytest.raises(_lib.SelftokHipError, match="head_dim 64"):
        ops.attention(None, (q, q, q, torch.empty_like(q)), 4, 16, kmask=km)
