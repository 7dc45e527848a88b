"""-m gpu: LPIPS on the VGG16 backbone (csrc/lpips_vgg.hip, ops.lpips_maxpool2s2, lpips.LpipsNet(net="vgg")) against the emulation of
tests/lpips_vgg_cases.py -- the 2 x 2 pool by equality, the convolution at the 13 VGG geometries under the project's standing fp32 gate, the whole
network against the staged calls (bit for bit) and the fp64 emulation, bit for bit against itself (run to run, alone against a batch, any order,
across the internal chunking, symmetric, next to a NaN image, replayed from a hipGraph), and the AlexNet network against its own staged calls.

Every measured ratio is printed, and written to the file SELFTOK_LPIPS_VGG_PROFILE names when it is set (a run replaces the file)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_cases as EC
import lpips_cases as L
import lpips_vgg_cases as V
from selftoktokenizer_amd import _lib, lpips as LP, ops, synth

pytestmark = pytest.mark.gpu

_PROFILE_OPENED = []


def _record(line):
    print("\n" + line)
    if os.environ.get("SELFTOK_LPIPS_VGG_PROFILE"):
        with open(os.environ["SELFTOK_LPIPS_VGG_PROFILE"], "a" if _PROFILE_OPENED else "w") as f:
            f.write(line + "\n")
        _PROFILE_OPENED.append(True)


@pytest.fixture(scope="module")
def net():
    return LP.LpipsNet.synthetic("cuda", net="vgg")


@pytest.fixture(scope="module")
def alex():
    return LP.LpipsNet.synthetic("cuda")


def dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(net, case, recon=None, orig=None):
    if recon is None:
        recon, orig = V.make(case)
    return net(dev(recon, case.recon_bf16), dev(orig, case.orig_bf16), original_signed=case.signed, quantize=case.quantize).cpu().numpy()


def guarded(t, guard=4096):
    """`t` as a view inside a larger NaN-filled allocation (16-byte aligned): a read that strays turns outputs into NaN, a write is seen in the band"""
    buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=t.dtype, device="cuda")
    buf[guard:guard + t.numel()] = t.reshape(-1)
    return buf, buf[guard:guard + t.numel()].view(t.shape)


def band_intact(buf, n, guard=4096):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


# ---- the 2 x 2 pool: equality ----
@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (31, 31), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("C", [64, 512])
@pytest.mark.parametrize("N", [1, 3])
def test_pool_equals_torch(hw, C, N):
    shape = (N, C) + hw
    x = synth.hash_uniform(synth.name_seed(f"lpips_pool2_{shape}"), shape, -1.0, 1.0)
    x[0, 0, 1, 1] = float("nan")                                    # inside window (0, 0) of every map
    x[-1, -1, 0, 0] = float("inf")
    want = F.max_pool2d(x, 2, 2)
    assert want.shape[2:] == (hw[0] // 2, hw[1] // 2)
    buf, xin = guarded(x.permute(0, 2, 3, 1).contiguous().cuda())
    out_buf, out = guarded(torch.full((N,) + tuple(want.shape[2:]) + (C,), float("nan"), device="cuda"))
    got = ops.lpips_maxpool2s2(xin, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.permute(0, 3, 1, 2).cpu()
    assert band_intact(out_buf, out.numel()) and band_intact(buf, xin.numel())
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    assert int(torch.isnan(want).sum()) == 1 and bool(torch.isnan(got[0, 0, 0, 0]))     # the NaN wins its one window (torch's rule) and no other
    assert torch.equal(ops.lpips_maxpool2s2(xin).permute(0, 3, 1, 2).cpu().nan_to_num(), want.nan_to_num())


# ---- the convolution at the VGG geometries ----
# maps: one pixel, a ragged one, and 63 / 65 pixels: one short of and one past the kernel's 64-row pixel tile (with B = 3: 189 and 195 rows)
CONV_MAPS = [(1, 1), (3, 5), (7, 9), (5, 13)]


@pytest.mark.parametrize("layer", range(13), ids=[l[0] for l in LP.VGG_LAYERS])
@pytest.mark.parametrize("hw", CONV_MAPS, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("B", [1, 3])
def test_convolution_at_the_vgg_geometries_under_the_standing_gate(layer, hw, B):
    name, key, co, ci, _, _ = LP.VGG_LAYERS[layer]
    H, W = hw
    sd, _ = LP.LpipsNet.synthetic_tensors("vgg")
    w, b = sd[key + ".weight"], sd[key + ".bias"]
    x = synth.hash_uniform(synth.name_seed(f"lpips_vgg_conv_{name}_{H}x{W}_{B}"), (B, ci, H, W), -1.0, 1.0)
    if layer:
        x = x.clamp_min(0.0)                                       # what a ReLU hands on
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=1))
    t32 = F.relu(F.conv2d(x, w, b, padding=1))
    cmp_acc = EC.ErrAcc(); cmp_acc.add(t32, ref)
    rms_gate, max_gate = EC.gate(cmp_acc.rms, cmp_acc.mx)
    xin_buf, xin = guarded(x.permute(0, 2, 3, 1).contiguous().cuda())
    packed_buf, packed = guarded(ops.lpips_pack_conv_weight(w).cuda())
    bias_buf, bias = guarded(b.cuda())
    out_buf, out = guarded(torch.full((B, H, W, co), float("nan"), device="cuda"))
    got = ops.lpips_conv2d(xin, packed, bias, co, 3, 3, 1, 1, True, out=out).permute(0, 3, 1, 2).cpu()
    assert band_intact(out_buf, out.numel()) and band_intact(xin_buf, xin.numel()) and band_intact(packed_buf, packed.numel()) and band_intact(bias_buf, bias.numel())
    assert torch.isfinite(got).all(), "an output depends on something outside its image or the tensors"
    acc = EC.ErrAcc(); acc.add(got, ref)
    _record(f"conv {name} ({ci} -> {co}) in {H}x{W} B{B}: device rms {acc.rms:.3e} max {acc.mx:.3e} | torch-CPU fp32 rms {cmp_acc.rms:.3e} max {cmp_acc.mx:.3e} | "
            f"ratio rms {acc.rms / max(cmp_acc.rms, 1e-30):.2f} max {acc.mx / max(cmp_acc.mx, 1e-30):.2f} (gate 2 x rms + 1e-8, 4 x max + 1e-7)")
    assert acc.rms <= rms_gate and acc.mx <= max_gate
    for i in range(B):                                             # an image alone inside NaN neighbours: the bits it has inside the batch
        one_buf, one = guarded(xin[i:i + 1])
        alone = ops.lpips_conv2d(one, packed, bias, co, 3, 3, 1, 1, True).permute(0, 3, 1, 2).cpu()
        assert torch.isfinite(alone).all() and torch.equal(alone, got[i:i + 1]), f"image {i}"


# ---- end to end ----
@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_network_equals_the_staged_calls_and_the_emulation(net, case):
    recon, orig = V.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    got = net(x, y, original_signed=case.signed, quantize=case.quantize).cpu().numpy()
    t = ops.lpips_input(x, y, case.signed, case.quantize)
    staged, tap = None, 0
    feats = net.features(x, y, case.signed, case.quantize)
    assert [tuple(f.shape[2:]) for f in feats] == LP.tap_sizes(case.H, case.W, "vgg")
    for (_, _, co, _, is_tap, pool), packed, bias in zip(LP.VGG_LAYERS, net.packed, net.bias):
        t = ops.lpips_conv2d(t, packed, bias, co, 3, 3, 1, 1, True)
        if is_tap:
            assert torch.equal(t.permute(0, 3, 1, 2), feats[tap])
            d = ops.lpips_distance(t, net.lin[tap])
            staged = d if staged is None else staged + d
            tap += 1
        if pool:
            t = ops.lpips_maxpool2s2(t)
    assert tap == 5 and got.dtype == np.float64 and got.shape == (case.B,)
    assert np.array_equal(bits(got), bits(staged.cpu().numpy()))
    want = V.case_value(case.name)
    if case.content == "identical":
        assert (got == 0.0).all()
    assert np.isfinite(got).all() and (got >= 0).all()
    m = V.gated_pairs(case.name)
    assert m.all() or case not in V.GATED
    if m.any():
        gate = V.relative_gate(case.name)
        rel = float((np.abs(got[m] - want[m]) / want[m]).max())
        _record(f"lpips-vgg {case.name}: {int(m.sum())} of {case.B} pairs gated, device relative error {rel:.3e} against the fp64 emulation (gate {gate:.3e} = 4 x the largest "
                f"relative error of torch-CPU fp32 features over the {'const' if case.content == 'const' else 'noise and smooth'} pairs), d {want[m].min():.4f} .. {want[m].max():.4f}")
        assert rel <= gate
    if not m.all():
        _record(f"lpips-vgg {case.name}: {int((~m).sum())} of {case.B} pairs below d = {V.D_GATED}, device |d - emulation| {np.abs(got[~m] - want[~m]).max():.3e} "
                f"at d {want[~m].min():.3e} .. {want[~m].max():.3e} (not gated)")


BATCH5 = V.Case("vgg_47x34_b5_noise", 47, 34, 5, "noise", False, True, True, False)


def test_bit_for_bit_run_to_run_alone_any_order_chunked_and_symmetric(net):
    recon, orig = V.make(BATCH5)
    a, b = run(net, BATCH5, recon, orig), run(net, BATCH5, recon, orig)
    assert np.array_equal(bits(a), bits(b)) and (a > 0.05).all()
    for i in range(BATCH5.B):
        assert np.array_equal(bits(run(net, BATCH5, recon[i:i + 1], orig[i:i + 1])), bits(a[i:i + 1])), f"pair {i} alone differs from the same pair inside B = 5"
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(bits(run(net, BATCH5, recon[perm], orig[perm])), bits(a[perm]))
    try:
        for chunk in (1, 2):                                       # the internal chunking: ragged last chunk included
            net.chunk_pairs = chunk
            assert np.array_equal(bits(run(net, BATCH5, recon, orig)), bits(a)), f"chunks of {chunk} pairs change the value"
    finally:
        net.chunk_pairs = None
    u = ((orig + np.float32(1)) / np.float32(2)).astype(np.float32)
    fwd = net(dev(recon), dev(u), original_signed=False).cpu().numpy()
    rev = net(dev(u), dev(recon), original_signed=False).cpu().numpy()
    assert np.array_equal(bits(fwd), bits(rev)) and (net(dev(u), dev(u), original_signed=False).cpu().numpy() == 0.0).all()


def test_a_nan_image_poisons_only_its_own_value(net):
    recon, orig = V.make(BATCH5)
    clean = run(net, BATCH5, recon, orig)
    for where in ((2, 1, 20, 17), (4, 2, 46, 33), (0, 0, 0, 0)):
        bad = recon.copy()
        bad[where] = np.nan
        got = run(net, BATCH5, bad, orig)
        keep = [i for i in range(BATCH5.B) if i != where[0]]
        assert np.isnan(got[where[0]]) and np.array_equal(bits(got[keep]), bits(clean[keep])), where
    bad = orig.copy()
    bad[1] = np.nan
    got = run(net, BATCH5, recon, bad)
    assert np.isnan(got[1]) and np.array_equal(bits(got[[0, 2, 3, 4]]), bits(clean[[0, 2, 3, 4]]))


def test_hipgraph_replay_equals_eager(net):
    case = V.BY_NAME["vgg_47x34_b3_recon_noise_bfsx"]
    recon, orig = V.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    call = lambda: net(x, y, original_signed=case.signed, quantize=case.quantize)
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
    recon2, orig2 = V.make(case, seed=1)
    x.copy_(dev(recon2, case.recon_bf16)); y.copy_(dev(orig2, case.orig_bf16))
    g.replay()
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert np.array_equal(bits(again), bits(call().cpu().numpy())) and not np.array_equal(bits(again), bits(eager))


def test_the_alexnet_network_still_makes_its_own_staged_calls(alex):
    """net="alex" is the default everywhere and its route is the one spelled out here, call for call: the same bits, and the emulation's value"""
    assert alex.net == "alex" and alex.definition is LP.LPIPS_DEFINITION
    for case in [c for c in L.CASES if c.H < 256][::3]:
        recon, orig = L.make(case)
        x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
        got = alex(x, y, original_signed=case.signed, quantize=case.quantize).cpu().numpy()
        t = ops.lpips_input(x, y, case.signed, case.quantize)
        staged = None
        for (_, _, co, _, k, s, p, pool), packed, bias, lin in zip(LP.LAYERS, alex.packed, alex.bias, alex.lin):
            t = ops.lpips_conv2d(t, packed, bias, co, k, k, s, p, True)
            d = ops.lpips_distance(t, lin)
            staged = d if staged is None else staged + d
            if pool:
                t = ops.lpips_maxpool3s2(t)
        assert np.array_equal(bits(got), bits(staged.cpu().numpy())), case.name
        m = L.gated_pairs(case.name)
        want = L.case_value(case.name)
        assert (np.abs(got[m] - want[m]) <= 4.0 * L.fp32_relative_error() * want[m]).all(), case.name


def test_refusals(net):
    f = torch.zeros(2, 3, 32, 32, device="cuda")
    for recon, orig in ((f.double(), f), (f, f.half()), (f, f[:1]), (f[0], f[0]), (f[:, :2], f[:, :2]), (f[..., :30], f[..., :30]), (f[..., :30, :], f[..., :30, :]),
                        (f.cpu(), f), (f, f.cpu())):
        with pytest.raises(_lib.SelftokHipError):
            net(recon, orig)
    x = torch.zeros(1, 8, 8, 4, device="cuda")
    for bad in (x[:, :1], x[:, :, :1], x.double()):
        with pytest.raises(_lib.SelftokHipError):
            ops.lpips_maxpool2s2(bad)
    with pytest.raises(_lib.SelftokHipError):
        ops.lpips_maxpool2s2(x, out=torch.zeros(1, 4, 4, 5, device="cuda"))
    assert (net(f, f, original_signed=False).cpu().numpy() == 0.0).all()
