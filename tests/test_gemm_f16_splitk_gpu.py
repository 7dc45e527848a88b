"""-m gpu: the split-K form of the single-pass fp16 Linear (csrc/gemm_f16_splitk.hip; MMDiTGPU.set_gemm("f16", splitk="f16")) held to the f16x2
split-K route BY EQUALITY, as its parent kernel is held to the f16x2 single-pass kernel (tests/test_gemm_f16_gpu.py).  With r(t) = t.half().float()
the low planes of r(x) and r(W) are exactly zero, the f16x2 partial kernel's low MFMAs add exact zeros, and both routes run the same reduction
launch, so for every legal split s
    linear_f16_split_k(x, W, s) == linear_f16x2_split_k(r(x), r(W), s)          (torch.equal) for arbitrary fp32 x, W.
A part of K / 32 / s k-tiles walks a ring of three stages of TWO k-tiles each, filled two iterations ahead: parts of 1, 2, 3 (odd; as many as the ring
has stages) and 4 tiles are covered, plus the model's K = 1536 and 6144 (parts of 3, 12 and 24).  Then the routes, the model's accuracy and the pipeline."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from selftoktokenizer_amd import _lib, ops, synth, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MS = (1, 15, 16, 17, 255, 256, 257, 513, 1024)
NS = (128, 384)
KT_S = ((2, 2), (4, 2), (6, 2), (9, 3), (8, 2), (12, 4), (48, 16), (48, 4), (192, 64), (192, 8))
EINVAL = -1


def r(t):
    return t.half().float()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _acts(M, K):
    g = torch.Generator(device="cuda").manual_seed(7919 * M + K)
    return torch.randn(M, K, device="cuda", generator=g) * (1.0 + 3.0 * torch.rand(1, K, device="cuda", generator=g))


def _weights(N, K):
    g = torch.Generator(device="cuda").manual_seed(31 * N + K)
    return (torch.rand(N, K, device="cuda", generator=g) * 2 - 1) * (3.0 / K) ** 0.5, torch.randn(N, device="cuda", generator=g) * 0.1


def _bt(M):
    B = 3 if M % 3 == 0 else 2 if M % 2 == 0 else 1
    return B, M // B


def _raw_k(name, xs, packed, bias, out, out_blk, ldo, M, N, K, ksplit, ws, flags=0, overflow=None):
    """selftok_linear_f16_split_k / selftok_linear_f16x2_split_k: one argument list"""
    return getattr(_lib.load(), name)(_p(xs), _p(packed), _p(bias), _p(out), _p(out_blk), ldo, M, N, K, flags, ksplit, _p(ws), _p(overflow), _stream())


def _raw_res_k(name, xs, packed, bias, resid, ldr, T, out, M, N, K, ksplit, ws, overflow=None):
    return getattr(_lib.load(), name)(_p(xs), _p(packed), _p(bias), _p(resid), ldr, None, 0, 0, T, _p(out), N, M, N, K, ksplit, _p(ws), _p(overflow), _stream())


@pytest.mark.parametrize("kt,s", KT_S)
def test_equals_the_f16x2_split_k_route_on_fp16_operands_every_epilogue(kt, s):
    """every M x N of the table at this (K, ksplit): bias / none, GELU, split output (both planes), the three residual forms and the in-place
    residual, each EQUAL to the f16x2 split-K entries with the same ksplit on the fp16-rounded operands; run to run bit for bit"""
    K = 32 * kt
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for N in NS:
        w, b = _weights(N, K)
        wp, wr = ops.linear_f16x2_pack(w, flag), ops.linear_f16x2_pack(r(w), flag)         # what the mode holds; the same rounded: zero low planes
        assert not bool(wr.view(N // 128, kt, 2, -1)[:, :, 1].any())
        for M in MS:
            a = _acts(M, K)
            xs, xr = ops.split_f16x2(a, flag), ops.split_f16x2(r(a), flag)
            assert not bool(xr.planes()[1].any()) and torch.equal(xr.planes()[0], xs.planes()[0])
            tag = f"M={M} N={N} K={K} ksplit={s}"
            ref = ops.linear_f16x2_split(xr, wr, b, N, overflow=flag, ksplit=s)
            got = ops.linear_f16_split_k(xs, wp, b, N, s, overflow=flag)
            assert torch.equal(got, ref), tag + ": arbitrary fp32 operands"
            assert torch.equal(ops.linear_f16_split_k(xr, wr, b, N, s, overflow=flag), ref), tag + ": rounded operands"
            assert torch.equal(ops.linear_f16_split_k(xs, wp, b, N, s, overflow=flag), got), tag + ": run to run"
            assert torch.equal(ops.linear_f16_split_k(a, wp, b, N, s, overflow=flag), got), tag + ": fp32 input through split_f16x2"
            assert torch.equal(ops.linear_f16_split_k(xs, wp, None, N, s, overflow=flag), ops.linear_f16x2_split(xr, wr, None, N, overflow=flag, ksplit=s)), tag + ": no bias"
            ref_g = ops.linear_f16x2_split(xr, wr, b, N, gelu=True, overflow=flag, ksplit=s)
            assert torch.equal(ops.linear_f16_split_k(xs, wp, b, N, s, gelu=True, overflow=flag), ref_g), tag + ": GELU"
            for gelu, y in ((False, ref), (True, ref_g)):
                os_ = ops.linear_f16_split_k(xs, wp, b, N, s, gelu=gelu, overflow=flag, out_split=True)
                assert os_.shape == (M, N) and torch.equal(os_.planes(), ops.split_f16x2(y).planes()), tag + f": split output (gelu={gelu}), both planes"
                assert torch.equal(os_.planes(), ops.linear_f16x2_split(xr, wr, b, N, gelu=gelu, overflow=flag, out_split=True, ksplit=s).planes())
            B, T = _bt(M)
            g = torch.Generator(device="cuda").manual_seed(M + N)
            resid = torch.randn(B, T, N, device="cuda", generator=g)
            tab_t, tab_b = torch.randn(T, 3 * N, device="cuda", generator=g), torch.randn(B, 3 * N, device="cuda", generator=g)
            xs3, xr3 = ops.split_f16x2(a.reshape(B, T, K)), ops.split_f16x2(r(a).reshape(B, T, K))
            for gate, ps in ((tab_t[:, N:2 * N], False), (tab_b[:, 2 * N:], True), (None, False)):
                want = ops.linear_f16x2_split_residual(xr3, wr, b, N, resid, gate=gate, gate_per_sample=ps, overflow=flag, ksplit=s)
                have = ops.linear_f16_split_residual_k(xs3, wp, b, N, resid, s, gate=gate, gate_per_sample=ps, overflow=flag)
                assert torch.equal(have, want), tag + f": residual, gate {'none' if gate is None else 'per sample' if ps else 'per token'}"
            # in place: out == resid (the reduction reads a residual element before the same thread writes it)
            inplace = resid.clone()
            ws = torch.empty(s * M * N, device="cuda")
            assert _raw_res_k("selftok_linear_f16_split_residual_k", xs3.data, wp, b, inplace, N, T, inplace, M, N, K, s, ws, flag) == 0
            assert torch.equal(inplace, want), tag + ": residual in place"
    assert int(flag.item()) == 0


@pytest.mark.parametrize("M,N,kt,s", [(17, 128, 2, 2), (257, 384, 9, 3), (513, 128, 48, 16), (1, 384, 6, 2), (1024, 128, 12, 4)])
def test_guard_bands_poisoned_lo_planes_and_the_workspace_beyond_the_partials(M, N, kt, s):
    """NaN in EVERY lo plane of the activations and of a copy of the packed weights changes nothing; NaN guard bands around the inputs, a strided `out`,
    the split output and the workspace are neither read into a result nor written: the workspace beyond ksplit * M * N floats stays as it was, and
    its first ksplit * M * N floats are the partial planes -- finite, and adding up (ascending) to the result without its bias"""
    K = 32 * kt
    a = _acts(M, K)
    w, b = _weights(N, K)
    xs, wp = ops.split_f16x2(a), ops.linear_f16x2_pack(w)
    xr, wr = ops.split_f16x2(r(a)), ops.linear_f16x2_pack(r(w))
    ref = ops.linear_f16x2_split(xr, wr, b, N, ksplit=s)
    nan = float("nan")
    G = 4096

    def guarded(t):
        buf = torch.full((t.numel() + 2 * G,), nan, dtype=t.dtype, device="cuda")
        buf[G:G + t.numel()] = t.reshape(-1)
        return buf, buf[G:G + t.numel()].view(t.shape)

    def bands_intact(buf, n):
        return bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())

    xbuf, xdata = guarded(xs.data)
    xdata[:, :, 1] = nan
    wbuf, wdata = guarded(wp)
    wdata.view(N // 128, kt, 2, -1)[:, :, 1] = nan
    bbuf, bdata = guarded(b)
    ldo = N + 8
    obuf = torch.full((M * ldo + 2 * G,), nan, device="cuda")
    out = obuf[G:G + M * ldo].view(M, ldo)
    wsbuf = torch.full((s * M * N + 2 * G,), nan, device="cuda")
    ws = wsbuf[G:G + s * M * N]
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw_k("selftok_linear_f16_split_k", xdata, wdata, bdata, out, None, ldo, M, N, K, s, ws, 0, flag) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, :N], ref), "strided out / guarded, poisoned inputs: result moved"
    assert bool(torch.isnan(out[:, N:]).all()) and bands_intact(obuf, M * ldo), "wrote outside out[:, :N]"
    assert bands_intact(wsbuf, s * M * N), "wrote outside the ksplit * M * N partials of the workspace"
    planes = ws.view(s, M, N)
    assert bool(torch.isfinite(planes).all()), "a partial plane was left unwritten"
    acc = planes[0].clone()
    for i in range(1, s):
        acc += planes[i]
    assert torch.equal(acc + b, ref), "the planes are not the partial sums the reduction adds in ascending order"
    assert int(flag.item()) == 0, "a poisoned lo plane or a guard band reached the range check"
    # the split output (guard bands around both planes) and the residual form on the same guarded, poisoned inputs
    want = ops.split_f16x2(ref)
    sbuf, sdata = guarded(want.data)
    sdata.fill_(nan)
    wsbuf[G:G + s * M * N] = nan
    assert _raw_k("selftok_linear_f16_split_k", xdata, wdata, bdata, None, sdata, N, M, N, K, s, ws, 0, flag) == 0
    torch.cuda.synchronize()
    got = ops.SplitAct((M, N), "cuda")
    got.data = sdata
    assert torch.equal(got.planes(), want.planes()) and bands_intact(sbuf, want.data.numel()) and bands_intact(wsbuf, s * M * N)
    B, T = _bt(M)
    resid = torch.randn(B, T, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    xs3 = ops.SplitAct((B, T, K), "cuda")
    xs3.data = xdata
    assert torch.equal(ops.linear_f16_split_residual_k(xs3, wdata, bdata, N, resid, s, overflow=flag), resid + ref.reshape(B, T, N))
    assert int(flag.item()) == 0
    for buf, n in ((xbuf, xs.data.numel()), (wbuf, wp.numel()), (bbuf, b.numel())):
        assert bands_intact(buf, n)


def test_one_part_is_the_single_pass_entry_and_empty_input():
    for M, N, kt in ((257, 384, 9), (16, 128, 1), (1024, 128, 48)):
        K = 32 * kt
        a = _acts(M, K)
        w, b = _weights(N, K)
        xs, wp = ops.split_f16x2(a), ops.linear_f16x2_pack(w)
        assert torch.equal(ops.linear_f16_split_k(xs, wp, b, N, 1), ops.linear_f16_split(xs, wp, b, N))
        assert torch.equal(ops.linear_f16_split_k(xs, wp, b, N, 1, gelu=True, out_split=True).planes(), ops.linear_f16_split(xs, wp, b, N, gelu=True, out_split=True).planes())
        B, T = _bt(M)
        resid = torch.randn(B, T, N, device="cuda")
        xs3 = ops.split_f16x2(a.reshape(B, T, K))
        assert torch.equal(ops.linear_f16_split_residual_k(xs3, wp, b, N, resid, 1), ops.linear_f16_split_residual(xs3, wp, b, N, resid))
        out = torch.empty(M, N, device="cuda")
        assert _raw_k("selftok_linear_f16_split_k", xs.data, wp, b, out, None, N, M, N, K, 1, None) == 0, "ksplit = 1 needs no workspace"
        assert torch.equal(out, ops.linear_f16_split(xs, wp, b, N))
    # M = 0: success without a launch, workspace or not
    a = _acts(300, 64)
    w, b = _weights(128, 64)
    packed = ops.linear_f16x2_pack(w)
    assert ops.linear_f16_split_k(ops.split_f16x2(a[:0]), packed, b, 128, 2).shape == (0, 128)
    assert ops.linear_f16_split_residual_k(ops.split_f16x2(a[:0].reshape(0, 5, 64)), packed, b, 128, torch.zeros(0, 5, 128, device="cuda"), 2).shape == (0, 5, 128)
    assert _raw_k("selftok_linear_f16_split_k", None, None, None, None, None, 128, 0, 128, 64, 2, None) == 0


def test_range_flag():
    a = _acts(300, 192)
    w, b = _weights(128, 192)
    packed = ops.linear_f16x2_pack(w)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.linear_f16_split_k(ops.split_f16x2(a), packed, b, 128, 3, overflow=flag)
    assert int(flag.item()) == 0
    big = a.clone()
    big[17, 5] = 7.0e4                                                      # an activation beyond the fp16 range: hi = inf -> a non-finite partial and output
    out = ops.linear_f16_split_k(ops.split_f16x2(big), packed, b, 128, 3, overflow=flag)
    assert int(flag.item()) & 1 and not bool(torch.isfinite(out[17]).all()) and bool(torch.isfinite(out[:17]).all()) and bool(torch.isfinite(out[18:]).all())
    flag.zero_()
    xs = ops.split_f16x2(a * 3.0e3)                                         # inputs in range, outputs beyond the fp16 range: the split output is not finite
    ops.linear_f16_split_k(xs, ops.linear_f16x2_pack(w * 50.0), None, 128, 2, overflow=flag, out_split=True)
    assert int(flag.item()) & 1
    flag.zero_()
    ops.linear_f16_split_residual_k(ops.split_f16x2(big.reshape(1, 300, 192)), packed, b, 128, torch.zeros(1, 300, 128, device="cuda"), 6, overflow=flag)
    assert int(flag.item()) & 1


def test_refusals_are_those_of_the_f16x2_split_k_entries():
    lib = _lib.load()
    a = _acts(300, 192)                                                      # K / 32 = 6 k-tiles
    w, b = _weights(128, 192)
    xs, packed = ops.split_f16x2(a), ops.linear_f16x2_pack(w)
    out, res = torch.empty(300, 128, device="cuda"), torch.zeros(300, 128, device="cuda")
    oblk = ops.SplitAct((300, 128), "cuda").data
    ws = torch.empty(6 * 300 * 128 + 4, device="cuda")
    plain = lambda name, ks, w_: _raw_k(name, xs.data, packed, b, out, None, 128, 300, 128, 192, ks, w_)
    resid = lambda name, ks, w_: _raw_res_k(name, xs.data, packed, b, res, 128, 300, out, 300, 128, 192, ks, w_)
    for what, ks, w_ in (("ksplit = 4 does not divide K / 32 = 6", 4, ws), ("ksplit = 65", 65, ws), ("ksplit = 0", 0, ws), ("ksplit = -2", -2, ws),
                         ("no workspace", 2, None), ("workspace 4 bytes off", 2, ws[1:])):
        assert plain("selftok_linear_f16x2_split_k", ks, w_) == EINVAL, what + ": the f16x2 entry"
        assert plain("selftok_linear_f16_split_k", ks, w_) == EINVAL, what
        assert b"linear_f16_split_k" in lib.selftok_last_error()
        assert resid("selftok_linear_f16x2_split_residual_k", ks, w_) == EINVAL, what + ": the f16x2 residual entry"
        assert resid("selftok_linear_f16_split_residual_k", ks, w_) == EINVAL, what + " (residual)"
        assert b"linear_f16_split_residual_k" in lib.selftok_last_error()
    # the plain contract, with a valid split and workspace
    for what, args in (("N % 128", (xs.data, packed, b, out, None, 100, 300, 100, 192)), ("K % 32", (xs.data, packed, b, out, None, 128, 300, 128, 48)),
                       ("no activations", (None, packed, b, out, None, 128, 300, 128, 192)), ("no weights", (xs.data, None, b, out, None, 128, 300, 128, 192)),
                       ("no output", (xs.data, packed, b, None, None, 128, 300, 128, 192)), ("both outputs", (xs.data, packed, b, out, oblk, 128, 300, 128, 192)),
                       ("ldo < N", (xs.data, packed, b, out, None, 64, 300, 128, 192)), ("ldo % 4", (xs.data, packed, b, out, None, 130, 300, 128, 192)),
                       ("M < 0", (xs.data, packed, b, out, None, 128, -1, 128, 192)), ("unaligned bias", (xs.data, packed, b[1:], out, None, 128, 300, 128, 192))):
        codes = [_raw_k(n, *args, 2, ws) for n in ("selftok_linear_f16x2_split_k", "selftok_linear_f16_split_k")]
        assert codes == [EINVAL, EINVAL], (what, codes)
    for what, (x_, w_, r_, ldr, T, M_, N_, K_) in (("N % 128", (xs.data, packed, res, 128, 300, 300, 100, 192)), ("no residual", (xs.data, packed, None, 128, 300, 300, 128, 192)),
                                                   ("ldr < N", (xs.data, packed, res, 64, 300, 300, 128, 192)), ("T = 0", (xs.data, packed, res, 128, 0, 300, 128, 192))):
        codes = [_raw_res_k(n, x_, w_, b, r_, ldr, T, out, M_, N_, K_, 2, ws) for n in ("selftok_linear_f16x2_split_residual_k", "selftok_linear_f16_split_residual_k")]
        assert codes == [EINVAL, EINVAL], (what, codes)
    for ks in (2, 3, 6):
        assert plain("selftok_linear_f16_split_k", ks, ws) == 0 and resid("selftok_linear_f16_split_residual_k", ks, ws) == 0, f"ksplit = {ks} with its workspace is legal"
    torch.cuda.synchronize()


# ---- model level -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return W.synthetic_state_dict(W.expected_shapes(512), device="cuda")


def test_block_linear_routes_with_and_without_the_switch(sd, monkeypatch):
    """which ops entry MMDiTGPU.lin and ._res_ln reach, and with which ksplit (recorders that call through, as in tests/test_gemm_f16_gpu.py).  With
    splitk="f16": 16 and 1024 rows reach the new entries with ops.f16_ksplit, 1040 rows the single-pass entries.  Without it: exactly today's calls."""
    from selftoktokenizer_amd import mmdit
    H = 1536
    dev = torch.device("cuda", torch.cuda.current_device())
    d = mmdit.MMDiTGPU(sd, dev, 512)
    calls = []
    for fn in ("linear_f16x2", "linear_f16x2_split", "linear_f16x2_split_residual", "linear_f16_split", "linear_f16_split_residual",
               "linear_f16_split_k", "linear_f16_split_residual_k"):
        def recorder(*a, _fn=fn, _real=getattr(ops, fn), **kw):
            calls.append((_fn, kw.get("ksplit")))
            return _real(*a, **kw)
        monkeypatch.setattr(mmdit.ops, fn, recorder)
    blk = "model.joint_blocks.3.x_block."
    g = torch.Generator(device="cuda").manual_seed(11)
    assert d.SPLITK and ops.SPLITK_MAX_ROWS == 1024

    def reached(run):
        del calls[:]
        out = run()
        torch.cuda.synchronize()
        return list(calls), out

    for mode, splitk in (("f16", "f16"), ("f16", None), ("f16", "f16x2"), ("f16x2", None)):
        assert d.set_gemm(mode, splitk=splitk) == mode and d.splitk == (splitk or "f16x2")
        for rows in (16, 1024, 1040):
            B, T = 2, rows // 2
            x = torch.randn(B, T, H, device="cuda", generator=g)
            tab = torch.randn(B, 3 * H, device="cuda", generator=g)
            single = mode == "f16" and rows > ops.SPLITK_MAX_ROWS
            new = mode == "f16" and splitk == "f16" and not single
            shape = lambda name: d.w[blk + name + ".weight"].shape
            ks = lambda name: (ops.f16_ksplit if new else ops.f16x2_ksplit)(rows, *shape(name))
            plain = lambda name: ("linear_f16_split", None) if single else ("linear_f16_split_k", ks(name)) if new else ("linear_f16x2_split", ks(name))
            tag = f"{mode}, splitk={splitk}, {rows} rows"
            got, y = reached(lambda: d.lin(blk + "attn.qkv", ops.split_f16x2(x)))
            assert got == [plain("attn.qkv")] and tuple(y.shape) == (B, T, 3 * H), tag + ": lin, split input"
            got, y = reached(lambda: d.lin(blk + "attn.qkv", x))
            assert got == [plain("attn.qkv") if (single or new) else ("linear_f16x2", None)], tag + ": lin, fp32 input (split here for the fp16 kernels)"
            got, y = reached(lambda: d.lin(blk + "mlp.fc1", ops.split_f16x2(x), gelu=True, out_split=True))
            assert got == [plain("mlp.fc1")] and isinstance(y, ops.SplitAct) and y.shape == (B, T, 4 * H), tag + ": lin(gelu, out_split) on mlp.fc1"
            got, (x2, n) = reached(lambda: d._res_ln(blk + "mlp.fc1", x, blk + "attn.proj", ops.split_f16x2(x), gate=tab[:, 2 * H:], gate_per_sample=True,
                                                     shift=tab[:, :H], scale=tab[:, H:2 * H], per_sample=True))
            want = ("linear_f16_split_residual", None) if single else ("linear_f16_split_residual_k", ks("attn.proj")) if new else ("linear_f16x2_split_residual", ks("attn.proj"))
            assert got == [want] and tuple(x2.shape) == (B, T, H) and isinstance(n, ops.SplitAct), tag + ": _res_ln on attn.proj"
    # a call without the argument resets it; the other modes never carry it
    d.set_gemm("f16", splitk="f16")
    assert d.set_gemm("f16") == "f16" and d.splitk == "f16x2"
    d.set_gemm("f16", splitk="f16")
    assert d.set_gemm("fp32") == "fp32" and d.splitk == "f16x2"
    with pytest.raises(ValueError):
        d.set_gemm("f16x2", splitk="f16")
    assert int(d.overflow.item()) == 0


def test_velocity_error_at_one_image_is_that_of_fp16_rounded_operands(sd):
    """MMDiT.forward at B = 1 (256 image rows, k + 1 context rows: every block Linear on the split-K fp16 kernel), case "a" of tests/golden/dit_forward_b1.npz
    (the reference's velocity).  Comparator and ratio of tests/test_gemm_f16_gpu.py: the fp32 mode with `lin()` overridden for exactly the packed names to
    F.linear(r(x), r(w), b) -- fp16-rounded operands on the fp32 library, same B = 1 -- and rms error <= 1.25 x that route's.  The figures are printed and
    written to profiles/f16_splitk_accuracy.txt."""
    from selftoktokenizer_amd.encoder import QformerEncoderGPU
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    dev = torch.device("cuda", torch.cuda.current_device())
    enc = QformerEncoderGPU(sd, dev, 512)
    d = MMDiTGPU(sd, dev, 512)
    g = np.load(os.path.join(GOLD, "dit_forward_b1.npz"))
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(1)).cuda())
    x = synth.synthetic_noise(1, device="cuda")
    t = torch.full((1,), float(g["t_a"]), device="cuda")
    k = int(g["k_a"])
    mask = torch.arange(512, device="cuda")[None] <= k
    ref = torch.from_numpy(g["v_a"]).double()
    assert 256 <= ops.SPLITK_MAX_ROWS and k + 1 <= ops.SPLITK_MAX_ROWS

    def errors():
        v, _ = d(x, t, encoder_hidden_states=ehs, mask=mask, context_see_xt=True)
        e = v.cpu().double() - ref
        return float(e.pow(2).mean().sqrt()), float(e.abs().max())

    err = {}
    for name, mode, kw in (("fp32", "fp32", {}), ("f16x2", "f16x2", {}), ("f16 (rows <= 1024 on f16x2 split-K)", "f16", {}), ("f16, splitk='f16'", "f16", {"splitk": "f16"})):
        assert d.set_gemm(mode, **kw) == mode
        err[name] = errors()
        assert int(d.overflow.item()) == 0
    assert err["f16 (rows <= 1024 on f16x2 split-K)"] == err["f16x2"], "without the switch one image decodes with f16x2 bits"
    packed_names = set(d._packed)
    d.set_gemm("fp32")
    plain = d.lin

    def rounded_lin(name, t_, gelu=False, out_split=False):
        if name not in packed_names:
            return plain(name, t_, gelu=gelu, out_split=out_split)
        y = F.linear(r(t_), r(d.w[name + ".weight"]), d.w[name + ".bias"])
        return F.gelu(y, approximate="tanh") if gelu else y

    d.lin = rounded_lin
    try:
        err["fp32 on fp16-rounded operands"] = errors()
    finally:
        del d.lin
    route, mine = err["fp32 on fp16-rounded operands"], err["f16, splitk='f16'"]
    lines = [f"velocity vs the reference (dit_forward_b1.npz case a, k = {k}, B = 1), |v| up to {float(ref.abs().max()):.2f}: rms / max abs error"]
    lines += [f"  {name:38s} rms {e[0]:.3e}  max {e[1]:.3e}" for name, e in err.items()]
    lines += [f"  rms ratio splitk='f16' / fp32 on fp16-rounded operands: {mine[0] / route[0]:.4f} (bound 1.25)"]
    print("\n" + "\n".join(lines))
    try:
        with open(os.path.join(ROOT, "profiles", "f16_splitk_accuracy.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass
    assert mine[0] <= 1.25 * route[0], (mine, route)
    assert mine != err["f16x2"], "the switch left the f16x2 arithmetic in place"


# ---- pipeline level ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipes(sd):
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    vsd = W.synthetic_vae_state_dict(device="cuda")
    mk = lambda **kw: SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd, vae_state_dict=vsd, verbose=False, **kw)
    with pytest.raises(ValueError, match="splitk"):
        mk(gemm="f16x2", splitk="f16")
    return mk(gemm="f16", splitk="f16"), mk(gemm="f16x2")


def _lat(pipe, ids, noise, **kw):
    return pipe.decoding(ids, noise=noise, max_steps=2, return_latent=True, **kw)[1]


@pytest.mark.parametrize("B", [1, 2])
def test_pipeline_with_the_switch(pipes, B):
    """SelftokPipeline(gemm="f16", splitk="f16") at 1 and 2 images: ids independent of the switch; gemm="f16" without it is the f16x2 pipeline bit for
    bit (the parent's route); with it: another, finite result, bit-stable, hipGraph == eager, no graph shared across the switch, CFG (doubles the rows),
    ar_partial, pixels, and both lossy switches together."""
    ps, px2 = pipes
    dit = ps.model.model
    assert (dit.gemm, dit.splitk, dit.attention) == ("f16", "f16", "split") and px2.model.model.splitk == "f16x2"
    imgs = synth.synthetic_images(B, device="cuda")
    ids_t = ps.encoding(imgs)
    assert torch.equal(ids_t, px2.encoding(imgs)), "token ids depend on the switch"
    ids, n = ids_t.cpu().numpy(), synth.synthetic_noise(B)
    lx = _lat(px2, ids, n)
    ls = _lat(ps, ids, n)
    assert bool(torch.isfinite(ls).all()) and torch.equal(ls, _lat(ps, ids, n)), "not bit-stable run to run"
    assert not torch.equal(ls, lx), "the switch left the f16x2 arithmetic in place"
    print(f"\n{B} image(s), 2 steps: splitk='f16' vs f16x2 latents max abs diff {float((ls - lx).abs().max()):.3e} (|latent| up to {float(lx.abs().max()):.2f})")
    try:
        assert ps.set_gemm("f16") == "f16" and dit.splitk == "f16x2"
        assert torch.equal(_lat(ps, ids, n), lx), "gemm='f16' without the switch must keep the f16x2 split-K route"
        n_graphs = len(ps._graphs)
        assert torch.equal(_lat(ps, ids, n, use_graph=True), lx) and len(ps._graphs) == n_graphs + 1
        assert ps.set_gemm("f16", splitk="f16") == "f16" and dit.splitk == "f16"
        assert torch.equal(_lat(ps, ids, n, use_graph=True), ls), "hipGraph capture + replay differs from eager"
        assert len(ps._graphs) == n_graphs + 2, "a graph captured without the switch was replayed with it"
        assert torch.equal(_lat(ps, ids, n, use_graph=True), ls) and len(ps._graphs) == n_graphs + 2, "hipGraph replay differs from eager"
        lc = _lat(ps, ids, n, uncond_scale=2.0)
        assert bool(torch.isfinite(lc).all()) and not torch.equal(lc, ls) and not torch.equal(lc, _lat(px2, ids, n, uncond_scale=2.0))
        la = _lat(ps, ids, n, ar_partial=np.array([300, 37][:B]))
        assert bool(torch.isfinite(la).all()) and not torch.equal(la, ls)
        rec = ps.decoding(ids, noise=n, max_steps=2)
        assert tuple(rec.shape) == (B, 3, 256, 256) and float(rec.min()) >= 0 and float(rec.max()) <= 1
        assert ps.set_gemm("f16", attention="f16", splitk="f16") == "f16" and (dit.attention, dit.splitk) == ("f16", "f16")
        lb = _lat(ps, ids, n)
        assert bool(torch.isfinite(lb).all()) and not torch.equal(lb, ls) and torch.equal(lb, _lat(ps, ids, n))
        assert torch.equal(_lat(ps, ids, n, use_graph=True), lb)
        assert ps.set_gemm("f16", attention="f16") == "f16" and (dit.attention, dit.splitk) == ("f16", "f16x2")
        assert not torch.equal(_lat(ps, ids, n), lb)
    finally:
        ps.set_gemm("f16", splitk="f16")
    assert int(dit.overflow.item()) == 0 and torch.equal(_lat(ps, ids, n), ls)


def test_forced_overflow_recomputes_on_fp32_and_returns_with_the_switch(pipes):
    ps, _ = pipes
    dit = ps.model.model
    ids, n = synth.synthetic_token_ids(2), synth.synthetic_noise(2)
    ls = _lat(ps, ids, n)
    packed_before = {k: v.data_ptr() for k, v in dit._packed.items()}
    dit.overflow.fill_(1)
    forced = _lat(ps, ids, n)
    assert (dit.gemm, dit.splitk) == ("f16", "f16") and int(dit.overflow.item()) == 0
    assert {k: v.data_ptr() for k, v in dit._packed.items()} == packed_before
    assert ps.set_gemm("fp32") == "fp32" and dit.splitk == "f16x2"
    try:
        l32 = _lat(ps, ids, n)
    finally:
        assert ps.set_gemm("f16", splitk="f16") == "f16"
    assert torch.equal(forced, l32) and not torch.equal(forced, ls)
    assert torch.equal(_lat(ps, ids, n), ls)


def test_set_gemm_round_trips_among_the_modes(pipes):
    ps, px2 = pipes
    ids, n = synth.synthetic_token_ids(2), synth.synthetic_noise(2)
    before = _lat(px2, ids, n)
    seen = {}
    try:
        for mode, kw in (("f16", {"splitk": "f16"}), ("exact", {}), ("fp32", {}), ("f16", {}), ("f16", {"splitk": "f16"}), ("f16x2", {}), ("f16", {"splitk": "f16x2"}),
                         ("fp32", {}), ("f16x2", {}), ("exact", {}), ("f16", {"splitk": "f16"}), ("f16x2", {})):
            assert ps.set_gemm(mode, **kw) == mode and ps.model.model.splitk == (kw.get("splitk") or "f16x2")
            if mode in ("f16", "f16x2"):
                key = "f16+splitk" if kw.get("splitk") == "f16" else "f16x2"        # gemm='f16' without the switch IS the f16x2 route at 2 images
                lat = _lat(ps, ids, n)
                assert torch.equal(seen.setdefault(key, lat), lat), f"{mode} {kw}: the result depends on the modes visited before"
        with pytest.raises(ValueError):
            ps.set_gemm("fp32", splitk="f16")
    finally:
        ps.set_gemm("f16", splitk="f16")
    assert torch.equal(seen["f16x2"], before) and not torch.equal(seen["f16+splitk"], before)


def test_renderer_runs_with_the_switch():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512, renderer=True), device="cuda")
    rp = SelftokPipeline(default_config(512, renderer=True), None, None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"),
                         verbose=False, gemm="f16", splitk="f16")
    assert (rp.model.model.gemm, rp.model.model.splitk) == ("f16", "f16")
    ids = synth.synthetic_token_ids(2)                                      # 512 image rows: the split-K regime
    rec, lat = rp.decoding_with_renderer(ids, return_latent=True)
    assert tuple(rec.shape) == (2, 3, 256, 256) and float(rec.min()) >= 0 and float(rec.max()) <= 1 and bool(torch.isfinite(lat).all())
    assert torch.equal(rp.decoding_with_renderer(ids, return_latent=True)[1], lat)
    assert rp.set_gemm("f16") == "f16"
    lx = rp.decoding_with_renderer(ids, return_latent=True)[1]
    assert rp.set_gemm("f16x2") == "f16x2"
    assert torch.equal(rp.decoding_with_renderer(ids, return_latent=True)[1], lx), "without the switch the renderer keeps the f16x2 route at 2 images"
    print(f"\nrenderer, 2 images: splitk='f16' vs f16x2 latents max abs diff {float((lat - lx).abs().max()):.3e}")
    assert not torch.equal(lat, lx) and int(rp.model.model.overflow.item()) == 0
