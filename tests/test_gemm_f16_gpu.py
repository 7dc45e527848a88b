"""-m gpu: the single-pass fp16 Linear (csrc/gemm_f16.hip, gemm="f16") held to the f16x2 kernel BY EQUALITY, then the mode at model and
pipeline level.  With r(t) = t.half().float(): the hi plane of every split operand is fp16(x), and on operands with x = r(x) the low planes
are exactly zero, so the f16x2 kernel's two low MFMAs add exact zeros and its result is the single-pass fp16 product -- the new kernel must
return the same numbers (torch.equal: +-0 alike), for every epilogue, at every tile / ring / tail edge:
    linear_f16_split(x, W) == linear_f16x2_split(r(x), r(W))        for arbitrary fp32 x, W.
The kernel stages TWO 32-deep k-tiles per ring stage, three stages, two iterations ahead: K / 32 = 1 .. 8 covers fewer, as many and more
iterations than the ring depth (3) and than the prefetch distance (2), each with an odd and an even tile count; K = 1536 is the model's."""
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
MS = (1, 15, 16, 17, 255, 256, 257, 513)
NS = (128, 384)
KS = (32, 64, 96, 128, 160, 192, 224, 256, 1536)


def r(t):
    return t.half().float()


def _data(M, N, K):
    g = torch.Generator(device="cuda").manual_seed(7919 * M + 31 * N + K)
    a = torch.randn(M, K, device="cuda", generator=g) * (1.0 + 3.0 * torch.rand(1, K, device="cuda", generator=g))
    w = (torch.rand(N, K, device="cuda", generator=g) * 2 - 1) * (3.0 / K) ** 0.5
    b = torch.randn(N, device="cuda", generator=g) * 0.1
    return a, w, b


def _bt(M):
    B = 3 if M % 3 == 0 else 2 if M % 2 == 0 else 1
    return B, M // B


def _raw(fn_name, xs, packed, bias, out, out_blk, ldo, M, N, K, flags=0, overflow=None):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return getattr(_lib.load(), fn_name)(p(xs), p(packed), p(bias), p(out), p(out_blk), ldo, M, N, K, flags, p(overflow), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


def _raw_k(xs, packed, bias, out, out_blk, ldo, M, N, K, ksplit, ws, flags=0):
    """selftok_linear_f16x2_split_k: the plain entry's arguments + (ksplit, workspace)"""
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    return _lib.load().selftok_linear_f16x2_split_k(p(xs), p(packed), p(bias), p(out), p(out_blk), ldo, M, N, K, flags, ksplit, p(ws), None,
                                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize("K", KS)
def test_equals_the_f16x2_kernel_on_fp16_operands_every_epilogue(K):
    """every M x N of the table at this K: plain / no bias / GELU / split output / the three residual forms, each EQUAL to the f16x2 single-pass
    kernel on the fp16-rounded operands; the rounded operands' low planes are checked to be zero, and both entries see the same inputs there"""
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    for N in NS:
        for M in MS:
            a, w, b = _data(M, N, K)
            xs, wp = ops.split_f16x2(a, flag), ops.linear_f16x2_pack(w, flag)                 # what the f16 mode holds: arbitrary fp32 operands, split
            xr, wr = ops.split_f16x2(r(a), flag), ops.linear_f16x2_pack(r(w), flag)           # the same operands rounded: zero low planes
            assert not bool(xr.planes()[1].any()) and not bool(wr.view(N // 128, K // 32, 2, -1)[:, :, 1].any())
            assert torch.equal(xr.planes()[0], xs.planes()[0]) and torch.equal(wr.view(N // 128, K // 32, 2, -1)[:, :, 0], wp.view(N // 128, K // 32, 2, -1)[:, :, 0])
            tag = f"M={M} N={N} K={K}"
            ref = ops.linear_f16x2_split(xr, wr, b, N, overflow=flag)
            assert torch.equal(ops.linear_f16_split(xr, wr, b, N, overflow=flag), ref), tag + ": rounded operands"
            got = ops.linear_f16_split(xs, wp, b, N, overflow=flag)
            assert torch.equal(got, ref), tag + ": arbitrary fp32 operands"
            assert torch.equal(ops.linear_f16_split(xs, wp, b, N, overflow=flag), got), tag + ": run to run"
            assert torch.equal(ops.linear_f16_split(a, wp, b, N, overflow=flag), got), tag + ": fp32 input through split_f16x2"
            assert torch.equal(ops.linear_f16_split(xs, wp, None, N, overflow=flag), ops.linear_f16x2_split(xr, wr, None, N, overflow=flag)), tag + ": no bias"
            ref_g = ops.linear_f16x2_split(xr, wr, b, N, gelu=True, overflow=flag)
            assert torch.equal(ops.linear_f16_split(xs, wp, b, N, gelu=True, overflow=flag), ref_g), tag + ": GELU"
            for gelu, y in ((False, ref), (True, ref_g)):
                os_ = ops.linear_f16_split(xs, wp, b, N, gelu=gelu, overflow=flag, out_split=True)
                assert os_.shape == (M, N) and torch.equal(os_.planes(), ops.split_f16x2(y).planes()), tag + f": split output (gelu={gelu}), both planes"
                assert torch.equal(os_.planes(), ops.linear_f16x2_split(xr, wr, b, N, gelu=gelu, overflow=flag, out_split=True).planes())
            B, T = _bt(M)
            g = torch.Generator(device="cuda").manual_seed(M + N)
            resid = torch.randn(B, T, N, device="cuda", generator=g)
            tab_t, tab_b = torch.randn(T, 3 * N, device="cuda", generator=g), torch.randn(B, 3 * N, device="cuda", generator=g)
            xs3, xr3 = ops.split_f16x2(a.reshape(B, T, K)), ops.split_f16x2(r(a).reshape(B, T, K))
            for gate, ps in ((tab_t[:, N:2 * N], False), (tab_b[:, 2 * N:], True), (None, False)):
                want = ops.linear_f16x2_split_residual(xr3, wr, b, N, resid, gate=gate, gate_per_sample=ps, overflow=flag)
                have = ops.linear_f16_split_residual(xs3, wp, b, N, resid, gate=gate, gate_per_sample=ps, overflow=flag)
                assert torch.equal(have, want), tag + f": residual, gate {'none' if gate is None else 'per sample' if ps else 'per token'}"
    assert int(flag.item()) == 0


@pytest.mark.parametrize("M,N,K", [(17, 128, 96), (257, 384, 160), (513, 128, 1536), (1, 384, 32)])
def test_strided_out_guard_bands_and_poisoned_lo_planes(M, N, K):
    """a strided `out` (ldo > N) keeps the columns between the rows; NaN guard bands around the activation planes, the packed weights, the bias
    and the output are neither read into a result nor written; NaN in EVERY lo plane of the activations and of a copy of the packed weights
    changes nothing (the kernel fetches the hi planes alone)."""
    a, w, b = _data(M, N, K)
    xs, wp = ops.split_f16x2(a), ops.linear_f16x2_pack(w)
    ref = ops.linear_f16x2_split(ops.split_f16x2(r(a)), ops.linear_f16x2_pack(r(w)), b, N)
    nan = float("nan")
    G = 4096                                                                # guard elements on either side (16-byte multiples)

    def guarded(t):
        buf = torch.full((t.numel() + 2 * G,), nan, dtype=t.dtype, device="cuda")
        buf[G:G + t.numel()] = t.reshape(-1)
        return buf, buf[G:G + t.numel()].view(t.shape)

    xbuf, xdata = guarded(xs.data)
    xdata[:, :, 1] = nan                                                    # every lo plane of the activations ...
    wbuf, wdata = guarded(wp)
    wdata.view(N // 128, K // 32, 2, -1)[:, :, 1] = nan                     # ... and of (a copy of) the packed weights
    bbuf, bdata = guarded(b)
    ldo = N + 8
    obuf = torch.full((M * ldo + 2 * G,), nan, device="cuda")
    out = obuf[G:G + M * ldo].view(M, ldo)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert _raw("selftok_linear_f16_split", xdata, wdata, bdata, out, None, ldo, M, N, K, 0, flag) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:, :N], ref), "strided out / guarded, poisoned inputs: result moved"
    assert bool(torch.isnan(out[:, N:]).all()) and bool(torch.isnan(obuf[:G]).all()) and bool(torch.isnan(obuf[G + M * ldo:]).all()), "wrote outside out[:, :N]"
    assert int(flag.item()) == 0, "a poisoned lo plane or a guard band reached the range check"
    # the split output and the residual form on the same guarded, poisoned inputs
    xs2 = ops.SplitAct((M, K), "cuda")
    xs2.data = xdata
    os_ = ops.linear_f16_split(xs2, wdata, bdata, N, overflow=flag, out_split=True)
    assert torch.equal(os_.planes(), ops.split_f16x2(ref).planes())
    B, T = _bt(M)
    resid = torch.randn(B, T, N, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    xs3 = ops.SplitAct((B, T, K), "cuda")
    xs3.data = xdata
    assert torch.equal(ops.linear_f16_split_residual(xs3, wdata, bdata, N, resid, overflow=flag), resid + ref.reshape(B, T, N))
    assert int(flag.item()) == 0
    for buf, n in ((xbuf, xs.data.numel()), (wbuf, wp.numel()), (bbuf, b.numel())):
        assert bool(torch.isnan(buf[:G]).all()) and bool(torch.isnan(buf[G + n:]).all())


def test_range_flag_empty_input_and_refusals():
    a, w, b = _data(300, 128, 64)
    packed = ops.linear_f16x2_pack(w)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.linear_f16_split(ops.split_f16x2(a), packed, b, 128, overflow=flag)
    assert int(flag.item()) == 0
    big = a.clone()
    big[17, 5] = 7.0e4                                                      # an activation beyond the fp16 range: hi = inf -> a non-finite output
    out = ops.linear_f16_split(ops.split_f16x2(big), packed, b, 128, overflow=flag)
    assert int(flag.item()) & 1 and not bool(torch.isfinite(out[17]).all()) and bool(torch.isfinite(out[:17]).all())
    flag.zero_()
    xs = ops.split_f16x2(a * 3.0e3)                                         # inputs in range, outputs of the Linear beyond the fp16 range: the split output is not finite
    ops.linear_f16_split(xs, ops.linear_f16x2_pack(w * 50.0), None, 128, overflow=flag, out_split=True)
    assert int(flag.item()) & 1
    flag.zero_()
    resid = torch.zeros(1, 300, 128, device="cuda")
    ops.linear_f16_split_residual(ops.split_f16x2(big.reshape(1, 300, 64)), packed, b, 128, resid, overflow=flag)
    assert int(flag.item()) & 1
    # M = 0: success without a launch
    assert ops.linear_f16_split(ops.split_f16x2(a[:0]), packed, b, 128).shape == (0, 128)
    assert ops.linear_f16_split_residual(ops.split_f16x2(a[:0].reshape(0, 5, 64)), packed, b, 128, torch.zeros(0, 5, 128, device="cuda")).shape == (0, 5, 128)
    # the refusals of the f16x2 entries
    xs = ops.split_f16x2(a)
    out = torch.empty(300, 128, device="cuda")
    oblk = ops.SplitAct((300, 128), "cuda").data
    EINVAL = -1
    ws = torch.empty(2 * 300 * 128, device="cuda")                          # a valid workspace for ksplit = 2: the split-K entries refuse these rows for the plain contract
    for what, args in (("N % 128", (xs.data, packed, b, out, None, 100, 300, 100, 64)), ("K % 32", (xs.data, packed, b, out, None, 128, 300, 128, 48)),
                       ("no activations", (None, packed, b, out, None, 128, 300, 128, 64)), ("no weights", (xs.data, None, b, out, None, 128, 300, 128, 64)),
                       ("no output", (xs.data, packed, b, None, None, 128, 300, 128, 64)), ("both outputs", (xs.data, packed, b, out, oblk, 128, 300, 128, 64)),
                       ("ldo < N", (xs.data, packed, b, out, None, 64, 300, 128, 64)), ("ldo % 4", (xs.data, packed, b, out, None, 130, 300, 128, 64)),
                       ("M < 0", (xs.data, packed, b, out, None, 128, -1, 128, 64)), ("unaligned bias", (xs.data, packed, b[1:], out, None, 128, 300, 128, 64))):
        assert _raw("selftok_linear_f16_split", *args) == EINVAL, what
        assert _raw("selftok_linear_f16x2_split", *args) == EINVAL, what + " (the f16x2 entry refuses it too)"
        assert _raw_k(*args, 2, ws) == EINVAL, what + " (and the f16x2 split-K entry)"
        assert b"linear_f16" in _lib.load().selftok_last_error()
    lib, p = _lib.load(), lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    res = torch.zeros(300, 128, device="cuda")
    for what, (x_, w_, r_, ldr, T, M_, N_, K_) in (("N % 128", (xs.data, packed, res, 128, 300, 300, 100, 64)), ("K % 32", (xs.data, packed, res, 128, 300, 300, 128, 48)),
                                                   ("no residual", (xs.data, packed, None, 128, 300, 300, 128, 64)), ("ldr < N", (xs.data, packed, res, 64, 300, 300, 128, 64)),
                                                   ("T = 0", (xs.data, packed, res, 128, 0, 300, 128, 64)), ("no activations", (None, packed, res, 128, 300, 300, 128, 64))):
        for name, sk in (("selftok_linear_f16_split_residual", ()), ("selftok_linear_f16x2_split_residual", ()), ("selftok_linear_f16x2_split_residual_k", (2, p(ws)))):
            assert getattr(lib, name)(p(x_), p(w_), p(b), p(r_), ldr, None, 0, 0, T, p(out), 128, M_, N_, K_, *sk, None, None) == EINVAL, (what, name)
    # what the split-K entries refuse on top: K / 32 = 6 k-tiles, so 4 is no divisor; more than 64 parts; no workspace; one that is not 16-byte aligned
    a6, w6, b6 = _data(300, 128, 192)
    xs6, packed6 = ops.split_f16x2(a6), ops.linear_f16x2_pack(w6)
    ws6 = torch.empty(4 * 300 * 128 + 4, device="cuda")
    plain_k = lambda ks, w_: _raw_k(xs6.data, packed6, b6, out, None, 128, 300, 128, 192, ks, w_)
    resid_k = lambda ks, w_: lib.selftok_linear_f16x2_split_residual_k(p(xs6.data), p(packed6), p(b6), p(res), 128, None, 0, 0, 300, p(out), 128, 300, 128, 192, ks, p(w_), None, None)
    for what, ks, w_ in (("ksplit = 4 does not divide K / 32 = 6", 4, ws6), ("ksplit = 65", 65, ws6), ("no workspace", 2, None), ("workspace 4 bytes off", 2, ws6[1:])):
        assert plain_k(ks, w_) == EINVAL, what
        assert b"linear_f16x2_split_k" in lib.selftok_last_error()
        assert resid_k(ks, w_) == EINVAL, what + " (residual)"
        assert b"linear_f16x2_split_residual_k" in lib.selftok_last_error()
    assert plain_k(2, ws6) == 0 and resid_k(2, ws6) == 0, "ksplit = 2 with its workspace is the legal call the rows above depart from"
    torch.cuda.synchronize()


# ---- model level -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sd():
    return W.synthetic_state_dict(W.expected_shapes(512), device="cuda")


def test_velocity_error_against_the_reference_is_that_of_fp16_rounded_operands(sd):
    """MMDiT.forward at B = 16 (4096 image rows, 16 (k + 1) context rows: every block Linear on the single-pass kernel), one scheduled timestep of
    tests/golden/dit_forward_b16.npz (the reference's velocity, sub-sampled).  Comparison route, built here: the fp32 mode with `lin()` overridden for
    exactly the packed names to F.linear(r(x), r(w), b) -- fp16-rounded operands on the fp32 library.  The f16 mode's error (rms and max) must not
    exceed 1.25 x that route's: the margin DESIGN.md section 9 applies to f16x2 against fp32; the two routes differ in accumulation order and in the
    attention kernel only.  The three figures (with the f16x2 mode's) are printed and written to profiles/f16_mode_accuracy.txt."""
    from selftoktokenizer_amd.encoder import QformerEncoderGPU
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    from selftoktokenizer_amd.pipeline import _Flow
    dev = torch.device("cuda", torch.cuda.current_device())
    enc = QformerEncoderGPU(sd, dev, 512)
    d = MMDiTGPU(sd, dev, 512)
    g = np.load(os.path.join(GOLD, "dit_forward_b16.npz"))
    B, j = 16, 0
    i, k = int(g["steps"][j]), int(g[f"k_{j}"])
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(B)).cuda())
    x = synth.synthetic_noise(B, device="cuda")
    flow = _Flow(50, 1.0, dev)
    tf = flow.t_freq[i:i + 1].expand(B, -1).contiguous()
    ref = torch.from_numpy(g[f"vsub_{j}"]).double()
    assert B * 256 > ops.SPLITK_MAX_ROWS and B * (k + 1) > ops.SPLITK_MAX_ROWS

    def errors():
        y = d.velocity_tokens(x, tf, d.embed_context(ehs), k + 1, True)
        _, v = ops.unpatchify_cfg_euler(y, None, 0.0, C=16, hp=16, wp=16)
        e = v[:, :, ::4, ::4].contiguous().cpu().double() - ref
        return float(e.pow(2).mean().sqrt()), float(e.abs().max())

    err = {}
    for mode in ("fp32", "f16x2", "f16"):
        assert d.set_gemm(mode) == mode
        err[mode] = errors()
        assert int(d.overflow.item()) == 0
    packed_names = set(d._packed)
    assert len(packed_names) >= 24 * 4 and all(".joint_blocks." in n for n in packed_names)     # qkv / proj / fc1 / fc2 of the joint blocks
    d.set_gemm("fp32")
    plain = d.lin

    def rounded_lin(name, t, gelu=False, out_split=False):
        if name not in packed_names:
            return plain(name, t, gelu=gelu, out_split=out_split)
        y = F.linear(r(t), r(d.w[name + ".weight"]), d.w[name + ".bias"])
        return F.gelu(y, approximate="tanh") if gelu else y

    d.lin = rounded_lin
    try:
        err["fp32 on fp16-rounded operands"] = errors()
    finally:
        del d.lin
    lines = [f"velocity vs the reference (dit_forward_b16.npz step {i}, k = {k}, sub-sampled), |v| up to {float(ref.abs().max()):.2f}: rms / max abs error"]
    lines += [f"  {name:32s} rms {e[0]:.3e}  max {e[1]:.3e}" for name, e in err.items()]
    print("\n" + "\n".join(lines))
    try:
        with open(os.path.join(ROOT, "profiles", "f16_mode_accuracy.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass
    route = err["fp32 on fp16-rounded operands"]
    assert err["f16"][0] <= 1.25 * route[0] and err["f16"][1] <= 1.25 * route[1], (err["f16"], route)


def test_block_linear_routes_by_mode_and_row_count(sd, monkeypatch):
    """which ops entry MMDiTGPU.lin and ._res_ln reach, and with which ksplit: the five Linear entries, as mmdit sees them, are replaced by recorders that
    call through.  16 rows (one chunk) and 1040 (the first chunk count above SPLITK_MAX_ROWS) of the model's width 1536; split input to `lin` plain,
    `lin(gelu, out_split)` on mlp.fc1 and `_res_ln` with a per-sample gate on attn.proj, and fp32 input to `lin` (the PRESPLIT = False reference form).
    Rows <= SPLITK_MAX_ROWS land on the f16x2 entries in both modes with ksplit = f16x2_ksplit(rows, N, K); above, on the single-pass fp16 entries in
    "f16" only."""
    from selftoktokenizer_amd import mmdit
    H = 1536
    dev = torch.device("cuda", torch.cuda.current_device())
    d = mmdit.MMDiTGPU(sd, dev, 512)
    calls = []
    for fn in ("linear_f16x2", "linear_f16x2_split", "linear_f16x2_split_residual", "linear_f16_split", "linear_f16_split_residual"):
        def recorder(*a, _fn=fn, _real=getattr(ops, fn), **kw):
            calls.append((_fn, kw.get("ksplit")))
            return _real(*a, **kw)
        monkeypatch.setattr(mmdit.ops, fn, recorder)
    blk = "model.joint_blocks.3.x_block."
    g = torch.Generator(device="cuda").manual_seed(11)
    assert d.SPLITK and ops.SPLITK_MAX_ROWS == 1024
    for mode in ("f16x2", "f16"):
        assert d.set_gemm(mode) == mode
        for rows in (16, 1040):
            B, T = 2, rows // 2
            x = torch.randn(B, T, H, device="cuda", generator=g)
            tab = torch.randn(B, 3 * H, device="cuda", generator=g)
            single = mode == "f16" and rows > ops.SPLITK_MAX_ROWS
            ks = lambda name: ops.f16x2_ksplit(rows, *d.w[blk + name + ".weight"].shape)
            tag = f"{mode}, {rows} rows"

            def reached(run):
                del calls[:]
                out = run()
                torch.cuda.synchronize()
                return list(calls), out

            got, y = reached(lambda: d.lin(blk + "attn.qkv", ops.split_f16x2(x)))
            assert got == [("linear_f16_split", None) if single else ("linear_f16x2_split", ks("attn.qkv"))], tag + ": lin, split input"
            assert tuple(y.shape) == (B, T, 3 * H)
            got, y = reached(lambda: d.lin(blk + "attn.qkv", x))
            assert got == [("linear_f16_split", None) if single else ("linear_f16x2", None)], tag + ": lin, fp32 input"
            assert tuple(y.shape) == (B, T, 3 * H)
            got, y = reached(lambda: d.lin(blk + "mlp.fc1", ops.split_f16x2(x), gelu=True, out_split=True))
            assert got == [("linear_f16_split", None) if single else ("linear_f16x2_split", ks("mlp.fc1"))], tag + ": lin(gelu, out_split) on mlp.fc1"
            assert isinstance(y, ops.SplitAct) and y.shape == (B, T, 4 * H)
            got, (x2, n) = reached(lambda: d._res_ln(blk + "mlp.fc1", x, blk + "attn.proj", ops.split_f16x2(x), gate=tab[:, 2 * H:], gate_per_sample=True,
                                                     shift=tab[:, :H], scale=tab[:, H:2 * H], per_sample=True))
            assert got == [("linear_f16_split_residual", None) if single else ("linear_f16x2_split_residual", ks("attn.proj"))], tag + ": _res_ln on attn.proj"
            assert tuple(x2.shape) == (B, T, H) and isinstance(n, ops.SplitAct)
            if rows <= ops.SPLITK_MAX_ROWS:
                assert ks("attn.qkv") > 1, "16 rows are the split-K regime"
    assert int(d.overflow.item()) == 0


# ---- pipeline level ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipes(sd):
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    vsd = W.synthetic_vae_state_dict(device="cuda")
    mk = lambda gemm: SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd, vae_state_dict=vsd, verbose=False, gemm=gemm)
    return mk("f16"), mk("f16x2")


def _lat(pipe, ids, noise, **kw):
    return pipe.decoding(ids, noise=noise, max_steps=2, return_latent=True, **kw)[1]


def test_pipeline_f16_mode(pipes):
    """SelftokPipeline(gemm="f16"): the encoder does not depend on the mode; 2 images (512 rows <= SPLITK_MAX_ROWS) stay on the f16x2 split-K
    route, bit for bit; 5 images (1280 image rows) run the single-pass kernel: finite, run to run bit-stable, hipGraph replay == eager,
    ar_partial and CFG run."""
    p16, px2 = pipes
    dit = p16.model.model
    assert dit.gemm == "f16" and px2.model.model.gemm == "f16x2"
    imgs = synth.synthetic_images(2, device="cuda")
    ids = p16.encoding(imgs)
    assert torch.equal(ids, px2.encoding(imgs)), "token ids depend on the GEMM mode"
    ids2, n2 = ids.cpu().numpy(), synth.synthetic_noise(2)
    l2 = _lat(p16, ids2, n2)
    assert bool(torch.isfinite(l2).all()) and torch.equal(l2, _lat(p16, ids2, n2))
    assert torch.equal(l2, _lat(px2, ids2, n2)), "rows <= SPLITK_MAX_ROWS must keep the f16x2 split-K route"
    assert torch.equal(l2, _lat(p16, ids2, n2, use_graph=True)), "hipGraph replay differs from eager (2 images)"
    ids5, n5 = synth.synthetic_token_ids(5), synth.synthetic_noise(5)
    assert 5 * 256 > ops.SPLITK_MAX_ROWS
    l5 = _lat(p16, ids5, n5)
    assert bool(torch.isfinite(l5).all()) and torch.equal(l5, _lat(p16, ids5, n5)), "not bit-stable run to run"
    lx = _lat(px2, ids5, n5)
    assert not torch.equal(l5, lx), "5 images: the f16 mode ran the f16x2 arithmetic"
    print(f"\n5 images, 2 steps: f16 vs f16x2 latents max abs diff {float((l5 - lx).abs().max()):.3e} (|latent| up to {float(lx.abs().max()):.2f})")
    assert torch.equal(l5, _lat(p16, ids5, n5, use_graph=True)), "hipGraph capture + replay differs from eager"
    assert torch.equal(l5, _lat(p16, ids5, n5, use_graph=True)), "hipGraph replay differs from eager"
    la = _lat(p16, ids5, n5, ar_partial=np.array([512, 300, 37, 1, 130]))
    assert bool(torch.isfinite(la).all()) and not torch.equal(la, l5)
    lc = _lat(p16, ids5, n5, uncond_scale=2.0)
    assert bool(torch.isfinite(lc).all()) and not torch.equal(lc, l5)
    rec = p16.decoding(ids5, noise=n5, max_steps=2)
    assert tuple(rec.shape) == (5, 3, 256, 256) and float(rec.min()) >= 0 and float(rec.max()) <= 1
    assert int(dit.overflow.item()) == 0 and dit.gemm == "f16"


def test_forced_activation_overflow_recomputes_on_fp32_and_returns_to_f16(pipes):
    """the sticky range flag is what the kernels raise (test_range_flag_... above); raised here before the call, as an activation beyond the fp16
    range inside the first step would leave it: the pipeline must discard the f16 result, run the call again on the fp32 GEMMs -- the same bits
    as a call in fp32 mode -- clear the flag and be back in "f16" with the packed weights kept."""
    p16, _ = pipes
    dit = p16.model.model
    ids5, n5 = synth.synthetic_token_ids(5), synth.synthetic_noise(5)
    l16 = _lat(p16, ids5, n5)
    packed_before = {k: v.data_ptr() for k, v in dit._packed.items()}
    dit.overflow.fill_(1)
    forced = _lat(p16, ids5, n5)
    assert dit.gemm == "f16" and int(dit.overflow.item()) == 0
    assert {k: v.data_ptr() for k, v in dit._packed.items()} == packed_before
    assert p16.set_gemm("fp32") == "fp32"
    try:
        l32 = _lat(p16, ids5, n5)
    finally:
        assert p16.set_gemm("f16") == "f16"
    assert torch.equal(forced, l32) and not torch.equal(forced, l16)
    assert torch.equal(_lat(p16, ids5, n5), l16)


def test_set_gemm_round_trips_leave_f16x2_results_as_they_were(pipes):
    _, p = pipes
    ids5, n5 = synth.synthetic_token_ids(5), synth.synthetic_noise(5)
    before = _lat(p, ids5, n5)
    seen = {}
    try:
        for mode in ("f16", "exact", "fp32", "f16", "f16x2", "fp32", "f16x2", "exact", "f16", "f16x2"):
            assert p.set_gemm(mode) == mode
            if mode in ("f16", "f16x2"):
                lat = _lat(p, ids5, n5)
                assert torch.equal(seen.setdefault(mode, lat), lat), f"{mode}: the result depends on the modes visited before"
        with pytest.raises(ValueError):
            p.set_gemm("fp16")
    finally:
        p.set_gemm("f16x2")
    assert torch.equal(seen["f16x2"], before) and not torch.equal(seen["f16"], before)


def test_renderer_runs_in_f16_mode():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512, renderer=True), device="cuda")
    rp = SelftokPipeline(default_config(512, renderer=True), None, None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"),
                         verbose=False, gemm="f16")
    assert rp.model.model.gemm == "f16"
    ids = synth.synthetic_token_ids(6)                                      # 1536 image rows: the single-pass kernel
    rec, lat = rp.decoding_with_renderer(ids, return_latent=True)
    assert tuple(rec.shape) == (6, 3, 256, 256) and float(rec.min()) >= 0 and float(rec.max()) <= 1 and bool(torch.isfinite(lat).all())
    assert torch.equal(rp.decoding_with_renderer(ids, return_latent=True)[1], lat)
    assert rp.set_gemm("f16x2") == "f16x2"
    lx = rp.decoding_with_renderer(ids, return_latent=True)[1]
    print(f"\nrenderer, 6 images: f16 vs f16x2 latents max abs diff {float((lat - lx).abs().max()):.3e}")
    assert not torch.equal(lat, lx) and int(rp.model.model.overflow.item()) == 0
