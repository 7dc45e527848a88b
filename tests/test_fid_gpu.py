"""-m gpu: rFID on the device (csrc/fid.hip, ops.fid_*, fid.InceptionNet, evaluate(metrics=(..., "rfid"))) against the emulation of tests/fid_cases.py --
the convolution entry alone under the project's standing fp32 gate at every kernel shape of the network, writing channel slices of NaN-filled maps; the pools
and the spatial mean by equality against a numpy fp32 restatement of their stated order; the input stage; the whole network against the staged calls (bit for
bit) and the fp64 emulation; bit for bit against itself (run to run, alone against a batch, any order, across the internal chunking, next to a NaN image,
replayed from a hipGraph); the fp64 statistics under a derived tolerance; and through the evaluation harness.

Every measured figure is printed before it is asserted."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_cases as EC
import fid_cases as FC
from selftoktokenizer_amd import _lib, evaluate as E, fid as FD, ops, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def net():
    return FD.InceptionNet.synthetic("cuda")


def dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """equal bits, NaN payloads aside"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.nan_to_num(a, nan=0.0).view(np.uint32 if a.dtype == np.float32 else np.uint64),
                                                                                             np.nan_to_num(b, nan=0.0).view(np.uint32 if b.dtype == np.float32 else np.uint64))


def guarded(t, guard=4096):
    """`t` as a view inside a larger NaN-filled allocation (16-byte aligned): a read that strays turns outputs into NaN, a write is seen in the band"""
    buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=t.dtype, device="cuda")
    buf[guard:guard + t.numel()] = t.reshape(-1)
    return buf, buf[guard:guard + t.numel()].view(t.shape)


def band_intact(buf, n, guard=4096):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def run(net, case, x=None):
    x = FC.make(case) if x is None else x
    return net.pool3(dev(x, case.bf16), case.signed, case.quantize, case.resize).cpu().numpy()


# ---- the convolution entry alone: one unit per kernel shape of the table ----
CONV_UNITS = {"1x1": "Mixed_5b.branch1x1", "3x3_s2": "Mixed_6a.branch3x3", "3x3_p1": "Mixed_5b.branch3x3dbl_2", "5x5_p2": "Mixed_5b.branch5x5_2",
              "1x7": "Mixed_6b.branch7x7_2", "7x1": "Mixed_6b.branch7x7_3", "1x3": "Mixed_7b.branch3x3_2a", "3x1": "Mixed_7b.branch3x3_2b", "stem_cin3": "Conv2d_1a_3x3",
              "pool_224_of_256": "Mixed_5b.branch_pool", "pool_1856_of_2048": "Mixed_7b.branch_pool"}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("side", [7, 3, 1])
@pytest.mark.parametrize("shape", list(CONV_UNITS))
def test_convolution_into_a_slice_against_fp64_under_the_standing_gate(net, shape, side, B):
    name = CONV_UNITS[shape]
    ci, co, kh, kw, s, ph, pw = FD.UNITS[name]
    H = W = side
    if (H + 2 * ph - kh) < 0 or (W + 2 * pw - kw) < 0:
        with pytest.raises(_lib.SelftokHipError, match="no output pixel"):                   # a 1 x 1 map under an unpadded 3 x 3 kernel: refused, nothing launched
            ops.fid_conv2d(torch.zeros(B, H, W, ci, device="cuda"), net.packed[name], net.bias[name], co, kh, kw, s, ph, pw)
        return
    sd = FD.InceptionNet.synthetic_tensors()
    w, b = FD.fold_bn(sd[name + ".conv.weight"], {leaf: sd[f"{name}.bn.{leaf}"] for leaf in FD.BN_LEAVES})
    x = synth.hash_uniform(synth.name_seed(f"fid_conv_{shape}_{side}_{B}"), (B, ci, H, W), -1.0, 1.0)
    if ci != 3:
        x = x.clamp_min(0.0)                                       # what a ReLU hands on
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=(ph, pw)))
    cmp_acc = EC.ErrAcc(); cmp_acc.add(F.relu(F.conv2d(x, w, b, stride=s, padding=(ph, pw))), ref)
    rms_gate, max_gate = EC.gate(cmp_acc.rms, cmp_acc.mx)
    OH, OW = ref.shape[2:]
    xin_buf, xin = guarded(nhwc(x).cuda())
    first = None
    for co_off, ldo in ((0, co), (0, co + 32), (224, max(256, 224 + co)), (1856, max(2048, 1856 + co))):
        out_buf, out = guarded(torch.full((B, OH, OW, ldo), float("nan"), device="cuda"))
        got = ops.fid_conv2d(xin, net.packed[name], net.bias[name], co, kh, kw, s, ph, pw, True, out=out, co_off=co_off)
        assert got.data_ptr() == out.data_ptr() and band_intact(out_buf, out.numel()) and band_intact(xin_buf, xin.numel())
        outside = torch.cat([got[..., :co_off], got[..., co_off + co:]], dim=3)
        assert bool(torch.isnan(outside).all()), f"bytes outside the slice {co_off}..{co_off + co} of {ldo} were written"
        val = got[..., co_off:co_off + co].permute(0, 3, 1, 2).cpu()
        assert torch.isfinite(val).all(), "an output depends on something outside its image or the tensors"
        if first is None:
            first = val
            acc = EC.ErrAcc(); acc.add(val, ref)
            print(f"\nconv {name} {kh}x{kw} in {H}x{W} B{B}: device rms {acc.rms:.3e} max {acc.mx:.3e} | torch-CPU fp32 rms {cmp_acc.rms:.3e} max {cmp_acc.mx:.3e} (gate 2 x rms, 4 x max)")
            assert acc.rms <= rms_gate and acc.mx <= max_gate
            if ph == pw:                                           # ldo = Cout, co_off = 0, pad_h = pad_w: the LPIPS entry, bit for bit
                assert torch.equal(ops.lpips_conv2d(xin, net.packed[name], net.bias[name], co, kh, kw, s, ph, True).permute(0, 3, 1, 2).cpu(), val)
        else:
            assert torch.equal(val, first), f"the slice at {co_off} of {ldo} differs from the tight output"
    for i in range(B):                                             # each image alone inside NaN: the bits it has in the batch
        one_buf, one = guarded(xin[i:i + 1])
        alone = ops.fid_conv2d(one, net.packed[name], net.bias[name], co, kh, kw, s, ph, pw).permute(0, 3, 1, 2).cpu()
        assert torch.isfinite(alone).all() and torch.equal(alone, first[i:i + 1]), f"image {i}"


# ---- pools and the spatial mean: equality against the stated order in numpy fp32 ----
def pool_np(x, mode):
    """x [N, C, H, W] fp32 -> the pool in the order csrc/fid.hip states"""
    f32 = np.float32
    N, C, H, W = x.shape
    s, p = (2, 0) if mode == "max_s2" else (1, 1)
    PH, PW = ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == "max_s2" else (H, W)
    acc, cnt = np.zeros((N, C, PH, PW), f32), np.zeros((PH, PW), np.int32)
    ys, xs = np.arange(PH) * s - p, np.arange(PW) * s - p
    for dy in range(3):
        for dx in range(3):
            iy, ix = ys + dy, xs + dx
            ok = ((iy >= 0) & (iy < H))[:, None] & ((ix >= 0) & (ix < W))[None, :]
            v = x[:, :, np.clip(iy, 0, H - 1)][..., np.clip(ix, 0, W - 1)]
            with np.errstate(invalid="ignore"):
                if mode == "avg_s1p1":
                    acc = np.where(ok, (acc + v).astype(f32), acc)
                else:
                    acc = np.where(ok & ((cnt == 0) | (v > acc) | np.isnan(v)), v, acc)
            cnt = cnt + ok
    with np.errstate(invalid="ignore"):
        return (acc / cnt.astype(f32)).astype(f32) if mode == "avg_s1p1" else acc


POOL_CASES = [pytest.param(mode, shape, id=f"{shape}-{mode}") for mode in ("max_s2", "max_s1p1", "avg_s1p1")
              for shape in [(1, 64, 7, 7), (3, 32, 3, 3), (2, 16, 1, 1), (2, 24, 1, 2), (1, 8, 9, 11), (3, 192, 4, 5)]]
POOL_CASES.append(pytest.param("lpips_maxpool3s2", [(1, 3, 3, 1), (2, 7, 8, 5), (1, 9, 11, 24)], id="lpips_maxpool3s2-is-max_s2"))      # [N, H, W, C]


@pytest.mark.parametrize("mode,shape", POOL_CASES)
def test_pools_equal_the_stated_order(mode, shape):
    if mode == "lpips_maxpool3s2":                                 # the LPIPS 3 x 3 / 2 pool and mode max_s2 are one body (csrc/pool_shared.h): the same bits
        for s in shape:
            x = synth.hash_uniform(synth.name_seed(f"pool_eq_{s}"), s, -1.0, -0.01).numpy()       # negative, so the planted -0.0 is the largest value of its windows
            x[0, s[1] // 2, s[2] // 2, 0] = np.nan
            x[-1, 0, 0, -1] = -0.0
            a, b = ops.lpips_maxpool3s2(dev(x)).cpu().numpy(), ops.fid_pool3(dev(x), "max_s2").cpu().numpy()
            assert a.shape == (s[0], (s[1] - 3) // 2 + 1, (s[2] - 3) // 2 + 1, s[3]) and same(a, b), s
            assert np.isnan(a).sum() >= 1 and ((bits(a) == 0x80000000).sum() >= 1 or a.size == 1), s      # both plants are seen (3 x 3 x 1: the NaN owns the one output)
        return
    N, C, H, W = shape
    if mode == "max_s2" and min(H, W) < 3:
        with pytest.raises(_lib.SelftokHipError, match="H, W >= 3"):
            ops.fid_pool3(torch.zeros(N, H, W, C, device="cuda"), mode)
        return
    x = synth.hash_uniform(synth.name_seed(f"fid_pool_{shape}"), shape, -1.0, 1.0).numpy()
    x[0, 0, H // 2, W // 2] = np.nan
    x[-1, -1, -1, -1] = np.inf
    x[-1, 1, 0, 0] = -np.inf
    want = pool_np(x, mode)
    t = torch.from_numpy(x)
    ref = F.max_pool2d(t, 3, 2) if mode == "max_s2" else (F.max_pool2d(t, 3, 1, 1) if mode == "max_s1p1" else F.avg_pool2d(t, 3, 1, 1, count_include_pad=False))
    assert want.shape == tuple(ref.shape) and np.array_equal(np.isnan(want), torch.isnan(ref).numpy())          # the restatement is torch's pool, NaN windows included
    assert same(want, ref.numpy()) if mode != "avg_s1p1" else np.allclose(np.nan_to_num(want, posinf=9, neginf=-9), np.nan_to_num(ref.numpy(), posinf=9, neginf=-9), rtol=1e-6, atol=1e-7)
    assert np.isnan(want).sum() >= 1 and np.isnan(want[1:]).sum() == 0 and np.isnan(want[0, 1:]).sum() == 0     # the NaN wins its windows and no other
    xin_buf, xin = guarded(nhwc(t).cuda())
    tight = ops.fid_pool3(xin, mode).permute(0, 3, 1, 2).cpu().numpy()
    assert same(tight, want)
    out_buf, out = guarded(torch.full((N,) + want.shape[2:] + (C + 40,), float("nan"), device="cuda"))
    got = ops.fid_pool3(xin, mode, out=out, co_off=8)
    assert band_intact(out_buf, out.numel()) and bool(torch.isnan(got[..., :8]).all()) and bool(torch.isnan(got[..., 8 + C:]).all())
    assert same(got[..., 8:8 + C].permute(0, 3, 1, 2).cpu().numpy(), want)


@pytest.mark.parametrize("shape", [(3, 1, 1, 2048), (2, 1, 2, 2048), (1, 8, 8, 256), (2, 7, 7, 100), (1, 35, 35, 16)], ids=str)
def test_spatial_mean_equals_the_stated_order(shape):
    N, h, w, C = shape
    x = synth.hash_uniform(synth.name_seed(f"fid_mean_{shape}"), shape, 0.0, 1.0).numpy()
    x[N - 1, h - 1, w - 1, 3] = np.nan
    s = np.zeros((N, C), np.float32)
    flat = x.reshape(N, h * w, C)
    with np.errstate(invalid="ignore"):
        for p in range(h * w):
            s = (s + flat[:, p]).astype(np.float32)
        want = (s / np.float32(h * w)).astype(np.float32)
    xin_buf, xin = guarded(torch.from_numpy(x).cuda())
    out_buf, out = guarded(torch.full((N, C), float("nan"), device="cuda"))
    got = ops.fid_spatial_mean(xin, out=out).cpu().numpy()
    assert band_intact(out_buf, out.numel()) and same(got, want) and np.isnan(got).sum() == 1 and np.isnan(got[N - 1, 3])


# ---- the input stage ----
@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("quantize", [False, True], ids=["float", "u8"])
def test_input_stage_equals_the_host_expression_on_every_bf16_pattern(signed, quantize):
    pat = np.arange(0x0000, 0x3F81, dtype=np.uint16)
    vals = (pat.astype(np.uint32) << 16).view(np.float32)                                 # every bf16 pattern in [0, 1]
    extra = (np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32)
    H = W = 75
    for bf16, v in ((True, vals), (False, np.concatenate([vals, extra]))):
        B = -(-v.size // (H * W))
        unit = np.repeat(np.resize(v, (B, 1, H, W)), 3, axis=1).astype(np.float32)
        x = (unit * np.float32(2) - np.float32(1)).astype(np.float32) if signed else unit
        x = FC._bf16(x) if bf16 else x
        want = FC.to_signed(x, bf16, signed, quantize)
        got = ops.fid_input(dev(x, bf16), signed, quantize)
        assert got.shape == (B, H, W, 3) and np.array_equal(bits(got.permute(0, 3, 1, 2).cpu().numpy()), bits(want)), (bf16, signed, quantize)


def test_input_stage_resize(net):
    for n_in in (64, 200, 320):
        ytab, _ = FD.resize_tables(n_in, n_in, "cuda")
        i0, i1, lam = FC.taps(n_in, FD.SIDE)
        assert np.array_equal(ytab.cpu().numpy(), np.stack([i0, i1, lam.view(np.int32)]))  # the tables the device reads are the emulation's
    for name in ("64x64_b3_noise_bux_resize", "320x200_b1_smooth_bux_resize", "256x256_b1_noise_fsq_resize"):
        case = FC.BY_NAME[name]
        x = FC.make(case)
        s = FC.to_signed(x, case.bf16, case.signed, case.quantize)
        got = ops.fid_input(dev(x, case.bf16), case.signed, case.quantize, FD.resize_tables(case.H, case.W, "cuda")).permute(0, 3, 1, 2).cpu().numpy()
        err = np.abs(got.astype(np.float64) - FC.resize_tables_f64(s)).max()
        print(f"\nresize {name}: |device - fp64 blend| {err:.3e} (tolerance 24 u = {FC.RESIZE_TOL:.3e}); against torch's fp64 interpolate {np.abs(got - FC.resize(s).numpy()).max():.3e}")
        assert got.shape == (case.B, 3, 299, 299) and err <= FC.RESIZE_TOL and np.abs(got - FC.resize(s).numpy()).max() <= FC.RESIZE_TOL + 4 * FC.U32
    case = FC.BY_NAME["299x299_b1_smooth_fsx_resize"]                                     # identity at 299 x 299: bit for bit, -0.0 included
    x = FC.make(case)
    x[0, 0, 0, :4] = [-0.0, 0.0, -1.0, 1.0]
    st = net.stages(dev(x), True, False, True)
    assert np.array_equal(bits(st["input"].cpu().numpy()), bits(x))
    y = ops.fid_input(dev(x), True, False, FD.resize_tables(299, 299, "cuda")).permute(0, 3, 1, 2).cpu().numpy()      # through the blend itself: lambda = 0 everywhere
    assert np.array_equal(y, x)


# ---- the network ----
class DeviceOps:
    """fid_cases.network's operations on the device entries with tight outputs and torch.cat: the staged calls"""
    mut = None

    def __init__(self, net):
        self.net = net
        self.cat = lambda ts: torch.cat(ts, 1)

    def unit(self, name, x):
        _, co, kh, kw, s, ph, pw = FD.UNITS[name]
        return ops.fid_conv2d(nhwc(x), self.net.packed[name], self.net.bias[name], co, kh, kw, s, ph, pw).permute(0, 3, 1, 2)

    def avg(self, x):
        return ops.fid_pool3(nhwc(x), "avg_s1p1").permute(0, 3, 1, 2)

    def max_s1(self, x):
        return ops.fid_pool3(nhwc(x), "max_s1p1").permute(0, 3, 1, 2)

    def max_s2(self, x):
        return ops.fid_pool3(nhwc(x), "max_s2").permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", FC.CASES, ids=lambda c: c.name)
def test_pool3_equals_the_staged_calls_and_the_emulation(net, case):
    x = dev(FC.make(case), case.bf16)
    got = net.pool3(x, case.signed, case.quantize, case.resize)
    st = net.stages(x, case.signed, case.quantize, case.resize)
    assert got.dtype == torch.float32 and tuple(got.shape) == (case.B, 2048) and torch.equal(st["pool3"], got)
    keep = {}
    last = FC.network(st["input"], DeviceOps(net), keep)
    for k, v in keep.items():
        assert torch.equal(v, st[k]), f"{k}: the slice-writing path differs from the staged calls"
    assert torch.equal(ops.fid_spatial_mean(nhwc(last)), got)
    want = FC.case_features(case.name)
    rel32 = FC.fp32_relative_error()
    rel = FC.rel_err(got.cpu().numpy(), want)
    print(f"\npool3 {case.name}: device relative error {rel.max():.3e} against the fp64 emulation (gate 4 x {rel32:.3e} = {4 * rel32:.3e}, torch-CPU fp32's largest over the table)")
    assert np.isfinite(got.cpu().numpy()).all() and (rel <= 4.0 * rel32).all()


BATCH5 = FC.Case("76x75_b5_noise_fux", 76, 75, 5, "noise", False, False, False, False)


def test_bit_for_bit_run_to_run_alone_any_order_and_chunked(net):
    x = FC.make(BATCH5)
    a, b = run(net, BATCH5, x), run(net, BATCH5, x)
    assert np.array_equal(bits(a), bits(b)) and len({a[i].tobytes() for i in range(5)}) == 5
    for i in range(BATCH5.B):
        assert np.array_equal(bits(run(net, BATCH5, x[i:i + 1])), bits(a[i:i + 1])), f"image {i} alone differs from the same image inside B = 5"
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(bits(run(net, BATCH5, x[perm])), bits(a[perm]))
    try:
        for chunk in (1, 2, 3, 4):                                 # the internal chunking: ragged last chunk included
            net.chunk_images = chunk
            assert np.array_equal(bits(run(net, BATCH5, x)), bits(a)), f"chunks of {chunk} images change the value"
    finally:
        net.chunk_images = None


def test_a_nan_image_poisons_only_its_own_row(net):
    x = FC.make(BATCH5)
    clean = run(net, BATCH5, x)
    for where in ((2, 1, 20, 17), (4, 2, 74, 74), (0, 0, 0, 0)):          # row 75 of a 76-row image is never read: the stride-2 stem stops at row 74
        bad = x.copy()
        bad[where] = np.nan
        got = run(net, BATCH5, bad)
        keep = [i for i in range(BATCH5.B) if i != where[0]]
        assert np.isnan(got[where[0]]).any() and np.array_equal(bits(got[keep]), bits(clean[keep])), where


def test_hipgraph_replay_equals_eager(net):
    case = FC.BY_NAME["64x64_b3_noise_bux_resize"]
    x = dev(FC.make(case), case.bf16)
    call = lambda: net.pool3(x, case.signed, case.quantize, case.resize)
    eager = call().cpu().numpy()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = call()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(eager))
    x.copy_(dev(FC.make(case, seed=1), case.bf16))
    g.replay()
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert np.array_equal(bits(again), bits(call().cpu().numpy())) and not np.array_equal(bits(again), bits(eager))


# ---- the statistics ----
@pytest.mark.parametrize("N,D", [(n, d) for d in (16, 64, 2048) for n in (2, 3, 17, 300)] + [(1100, 16)], ids=lambda v: str(v))
def test_statistics_against_numpy_fp64(N, D):
    X = FC.stats_matrix(N, D)
    mu_w, sg_w = FC.statistics(X)
    tol_mu, tol_sg = FC.stats_tolerance(X)
    x_buf, x = guarded(dev(X))
    lib = _lib.load()
    nbytes = lib.selftok_fid_stats_workspace_bytes(N, D)
    assert nbytes == -(-N // 256) * D * 8
    mu_buf, mu = guarded(torch.full((D,), float("nan"), dtype=torch.float64, device="cuda"))
    sg_buf, sg = guarded(torch.full((D, D), float("nan"), dtype=torch.float64, device="cuda"))
    ws_buf, ws = guarded(torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda"))
    got_mu, got_sg = ops.fid_stats(x, mu=mu, sigma=sg, workspace=ws)
    assert band_intact(mu_buf, D) and band_intact(sg_buf, D * D) and band_intact(ws_buf, nbytes // 8) and band_intact(x_buf, N * D)
    m, s = got_mu.cpu().numpy(), got_sg.cpu().numpy()
    ratio_mu = float((np.abs(m - mu_w) / np.maximum(tol_mu, 1e-300)).max())
    ratio_sg = float((np.abs(s - sg_w) / np.maximum(tol_sg, 1e-300)).max())
    print(f"\nstats N {N} D {D}: |mu - numpy| / tolerance {ratio_mu:.3f}, |sigma - numpy| / tolerance {ratio_sg:.3f} (c = {FC.STATS_C}, k = {FC.STATS_K})")
    assert np.isfinite(m).all() and np.isfinite(s).all()
    assert (np.abs(m - mu_w) <= tol_mu).all() and (np.abs(s - sg_w) <= tol_sg).all()
    assert np.array_equal(s.view(np.uint64), s.T.copy().view(np.uint64)), "sigma is not exactly symmetric"
    m2, s2 = ops.fid_stats(x)                                      # run to run, fresh outputs and the shared workspace
    assert np.array_equal(m2.cpu().numpy().view(np.uint64), m.view(np.uint64)) and np.array_equal(s2.cpu().numpy().view(np.uint64), s.view(np.uint64))
    assert (np.linalg.eigvalsh(s) >= -1e-12 * np.trace(s)).all() if D <= 64 else True
    a, b = FD.statistics(x)
    assert torch.equal(a, m2) and torch.equal(b, s2)


# ---- the harness ----
class _SetPipe:
    """a stand-in tokenizer (evaluate only needs .device, .encoding, .decoding*): image i of the originals decodes to image i of the reconstruction set"""
    device = torch.device("cuda")

    def __init__(self):
        self.orig = dev(FC.set_images("smooth"))
        self.recon = dev(FC.set_images("noise"), bf16=True)
        self.range = None

    def load(self, lo, hi):
        self.range = (lo, hi)
        return self.orig[lo:hi]

    def encoding(self, imgs, device=None):
        lo, hi = self.range
        return torch.arange(lo, hi)[:, None].repeat(1, 8)

    def decoding(self, ids, device=None, noise=None):
        return self.recon[torch.from_numpy(np.asarray(ids)[:, 0]).cuda()]

    def decoding_with_renderer(self, ids, device=None):
        return self.decoding(ids).float() * 0.75 + 0.125


@pytest.fixture
def straight(net):
    """the network feeding 75 x 75 images straight in, as the emulation of the two sets does"""
    net.resize = False
    yield net
    net.resize = True


def test_harness_rfid_option(straight):
    net, pipe = straight, _SetPipe()
    n, dec = FC.SET_N, ("diffusion", "renderer")
    both = E.evaluate(pipe, pipe.load, n, batch=n, decoders=dec, metrics=("psnr", "ssim"))
    full = E.evaluate(pipe, pipe.load, n, batch=n, decoders=dec, metrics=("psnr", "ssim", "rfid"), fid=net)
    assert list(full) == list(both) and list(full["diffusion"]) == ["psnr_mean_dB", "psnr_each_dB", "ssim_mean", "ssim_each", "rfid", "rfid_n", "rfid_rank_deficient"]
    assert full["metric_definition"]["rfid"] == dict(FD.FID_DEFINITION, weights="synthetic", resized=False)
    assert {k: v for k, v in full["metric_definition"].items() if k != "rfid"} == both["metric_definition"]
    ids = np.arange(n)[:, None]
    mu0, s0 = FD.statistics(net.pool3(pipe.orig, True))
    for d, rec in (("diffusion", pipe.decoding(ids)), ("renderer", pipe.decoding_with_renderer(ids))):
        assert {k: v for k, v in full[d].items() if not k.startswith("rfid")} == both[d]            # every other entry identical to a run without "rfid"
        direct = FD.frechet_distance(*FD.statistics(net.pool3(rec, False)), mu0, s0)
        assert full[d]["rfid"] == direct and full[d]["rfid_n"] == n and full[d]["rfid_rank_deficient"] is True and direct > 0
    want, want32 = FC.set_distance(), FC.set_distance(torch.float32)
    got = full["diffusion"]["rfid"]
    print(f"\nrfid of the two sets: device {got:.9f}, fp64 emulation {want:.9f}: |difference| {abs(got - want):.3e}; torch-CPU fp32 features through the fp64 tail "
          f"deviate by {abs(want32 - want):.3e} (gate 4 x that)")
    assert want > 1.0                                                                               # well away from 0
    assert abs(got - want) <= 4.0 * abs(want32 - want)
    ragged = E.evaluate(pipe, pipe.load, n, batch=7, decoders=dec, metrics=("psnr", "ssim", "rfid"), fid=net)
    assert ragged["batch"] == 7 and {k: v for k, v in ragged.items() if k != "batch"} == {k: v for k, v in full.items() if k != "batch"}
    only = E.evaluate(pipe, pipe.load, n, batch=n, metrics=("rfid",), fid=net)
    assert only["diffusion"]["rfid"] == got

    u8 = E.evaluate(pipe, pipe.load, n, batch=n, metrics=("ssim", "rfid"), metrics_u8=True, fid=net)
    assert u8["metric_definition"]["on"] == "u8"
    direct = FD.frechet_distance(*FD.statistics(net.pool3(pipe.recon, False, quantize=True)), *FD.statistics(net.pool3(pipe.orig, True, quantize=True)))
    want_q, want32_q = FC.set_distance(quantize=True), FC.set_distance(torch.float32, quantize=True)
    print(f"on the bytes: device {direct:.9f}, fp64 emulation {want_q:.9f}: |difference| {abs(direct - want_q):.3e}; fp32 comparator {abs(want32_q - want_q):.3e}")
    assert u8["diffusion"]["rfid"] == direct and direct != got and abs(direct - want_q) <= 4.0 * abs(want32_q - want_q)
    with pytest.raises(ValueError, match="rfid"):
        E.evaluate(pipe, pipe.load, n, metrics=("rfid",))
    with pytest.raises(ValueError, match="rfid"):
        E.evaluate(pipe, pipe.load, n, metrics=("psnr", "rfid"), fid=None)
    with pytest.raises(ValueError, match="2 images"):
        E.evaluate(pipe, pipe.load, 1, metrics=("rfid",), fid=net)


def test_refusals(net):
    f = torch.zeros(2, 3, 80, 80, device="cuda")
    for x, kw in ((f.double(), {}), (f.half(), {}), (f[0], {}), (f[:, :2], {}), (f[..., :74], {"resize": False}), (f[..., :74, :], {"resize": False}), (f.cpu(), {})):
        with pytest.raises(_lib.SelftokHipError):
            net.pool3(x, True, **kw)
    assert tuple(net.pool3(f[..., :74], True).shape) == (2, 2048)                                   # with the resize a small image is fine
    x = torch.zeros(1, 8, 8, 4, device="cuda")
    pk = ops.lpips_pack_conv_weight(torch.zeros(64, 4, 1, 7)).cuda()
    wide = torch.zeros(1, 8, 8, 96, device="cuda")
    for args, kw in (((x, pk, None, 64, 1, 7, 1, 1, 3), {}), ((x, pk, None, 64, 1, 7, 1, 0, 7), {}), ((x, pk, None, 64, 7, 1, 1, 0, 3), {}),
                     ((x, pk, None, 64, 1, 7, 1, 0, 3), {"out": wide, "co_off": 36}), ((x, pk, None, 64, 1, 7, 1, 0, 3), {"co_off": 4}),
                     ((x, pk, None, 64, 1, 7, 1, 0, 3), {"out": wide[:, :4]}), ((x.double(), pk, None, 64, 1, 7, 1, 0, 3), {}),
                     ((x, pk, torch.zeros(63, device="cuda"), 64, 1, 7, 1, 0, 3), {})):
        with pytest.raises(_lib.SelftokHipError):
            ops.fid_conv2d(*args, **kw)
    assert not ops.fid_conv2d(x, pk, None, 64, 1, 7, 1, 0, 3, out=wide, co_off=32)[..., :32].any()
    with pytest.raises(_lib.SelftokHipError):
        ops.fid_pool3(x[:, :2], "max_s2")
    with pytest.raises(_lib.SelftokHipError):
        ops.fid_stats(torch.zeros(1, 16, device="cuda"))
    with pytest.raises(_lib.SelftokHipError):
        ops.fid_stats(torch.zeros(4, 24, device="cuda"))
    with pytest.raises(_lib.SelftokHipError):
        ops.fid_stats(torch.zeros(4, 16, device="cuda"), workspace=torch.empty(64, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SelftokHipError):
        ops.fid_input(f, True, tables=(torch.zeros(3, 299, device="cuda"), torch.zeros(3, 299, device="cuda")))      # float tables
