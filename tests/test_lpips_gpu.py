"""-m gpu: LPIPS on the device (csrc/lpips.hip, ops.lpips_*, lpips.LpipsNet, evaluate(metrics=(..., "lpips"))) against the emulation of
tests/lpips_cases.py -- the convolution alone under the project's standing fp32 gate, the pool and the input stage by equality, the distance
stage under a derived fp64 tolerance, the whole network against the fp64 emulation, bit for bit against itself (run to run, alone against a
batch, any order, across the internal chunking, symmetric, next to a NaN image, replayed from a hipGraph), and through the evaluation harness.

Every measured ratio and the fp32 comparator's end-to-end error is printed, and written to the file SELFTOK_LPIPS_PROFILE names when it is set (a run
replaces the file): profiles/lpips_vs_fp64.txt is one such run."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import edge_cases as EC
import image_io_cases as IO
import lpips_cases as L
from selftoktokenizer_amd import _lib, evaluate as E, lpips as LP, ops, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


_PROFILE_OPENED = []


def _record(line):
    print("\n" + line)
    if os.environ.get("SELFTOK_LPIPS_PROFILE"):
        with open(os.environ["SELFTOK_LPIPS_PROFILE"], "a" if _PROFILE_OPENED else "w") as f:       # a run replaces the file, it does not add to an earlier one
            f.write(line + "\n")
        _PROFILE_OPENED.append(True)


@pytest.fixture(scope="module")
def net():
    return LP.LpipsNet.synthetic("cuda")


def dev(a, bf16=False):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.to(torch.bfloat16) if bf16 else t


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def run(net, case, recon=None, orig=None):
    if recon is None:
        recon, orig = L.make(case)
    return net(dev(recon, case.recon_bf16), dev(orig, case.orig_bf16), original_signed=case.signed, quantize=case.quantize).cpu().numpy()


def guarded(t, guard=4096):
    """`t` as a view inside a larger NaN-filled allocation (16-byte aligned): a read that strays turns outputs into NaN, a write is seen in the band"""
    buf = torch.full((t.numel() + 2 * guard,), float("nan"), dtype=t.dtype, device="cuda")
    buf[guard:guard + t.numel()] = t.reshape(-1)
    return buf, buf[guard:guard + t.numel()].view(t.shape)


def band_intact(buf, n, guard=4096):
    return bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())


# ---- the convolution alone ----
# (layer index, H, W of the layer's INPUT): the smallest input each layer sees (a 31 x 31 image) and a ragged one (35 x 47 / 67 x 95 images)
CONV_GEOMS = [(0, 31, 31), (0, 35, 47), (1, 3, 3), (1, 7, 11), (2, 1, 1), (2, 3, 5), (3, 1, 1), (3, 3, 5), (4, 1, 1), (4, 7, 11)]


@pytest.mark.parametrize("layer,H,W", CONV_GEOMS, ids=[f"{LP.LAYERS[l][0]}_{h}x{w}" for l, h, w in CONV_GEOMS])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("relu", [True, False], ids=["relu", "linear"])
def test_convolution_against_fp64_under_the_standing_gate(layer, H, W, B, relu):
    name, key, co, ci, k, s, p, _ = LP.LAYERS[layer]
    sd, _ = LP.LpipsNet.synthetic_tensors()
    w, b = sd[key + ".weight"], sd[key + ".bias"]
    seed = synth.name_seed(f"lpips_conv_{name}_{H}x{W}_{B}")
    x = synth.hash_uniform(seed, (B, ci, H, W), -1.0, 1.0)
    if layer:
        x = x.clamp_min(0.0)                                       # what a ReLU hands on
    act = (lambda t: F.relu(t)) if relu else (lambda t: t)
    ref = act(F.conv2d(x.double(), w.double(), b.double(), stride=s, padding=p))
    t32 = act(F.conv2d(x, w, b, stride=s, padding=p))
    cmp_acc = EC.ErrAcc(); cmp_acc.add(t32, ref)
    rms_gate, max_gate = EC.gate(cmp_acc.rms, cmp_acc.mx)

    # NaN bands around input, weights, bias and output: the batch is one contiguous tensor with NaN before its first and after its last element only, so a
    # tap that strays off either END of the batch turns an output into NaN and a stray write shows in a band; what isolates the images from each other is the
    # loop at the end of this test
    OH, OW = ref.shape[2:]
    xin_buf, xin = guarded(x.permute(0, 2, 3, 1).contiguous().cuda())
    packed_buf, packed = guarded(ops.lpips_pack_conv_weight(w).cuda())
    bias_buf, bias = guarded(b.cuda())
    out_buf, out = guarded(torch.full((B, OH, OW, co), float("nan"), device="cuda"))
    got = ops.lpips_conv2d(xin, packed, bias, co, k, k, s, p, relu, out=out)
    assert got.data_ptr() == out.data_ptr()
    got = got.permute(0, 3, 1, 2).cpu()
    assert band_intact(out_buf, out.numel()) and band_intact(xin_buf, xin.numel()) and band_intact(packed_buf, packed.numel()) and band_intact(bias_buf, bias.numel())
    assert torch.isfinite(got).all(), "an output depends on something outside its image or the tensors"
    acc = EC.ErrAcc(); acc.add(got, ref)
    _record(f"conv {name} in {H}x{W} B{B} {'relu' if relu else 'linear'}: device rms {acc.rms:.3e} max {acc.mx:.3e} | torch-CPU fp32 rms {cmp_acc.rms:.3e} max {cmp_acc.mx:.3e} | "
            f"ratio rms {acc.rms / max(cmp_acc.rms, 1e-30):.2f} max {acc.mx / max(cmp_acc.mx, 1e-30):.2f} (gate 2 x rms + 1e-8, 4 x max + 1e-7)")
    assert acc.rms <= rms_gate and acc.mx <= max_gate
    # the padding is zero: every image alone, with NaN before and after it, stays finite and gives the bits it has inside the batch -- a top or bottom padding
    # tap that read memory instead of a zero would see a NaN here and a neighbour's pixel there.  A left or right padding tap that wrapped would land on the
    # same image's neighbouring row in both runs: that mistake is caught by the fp64 gate above, not here
    for i in range(B):
        one_buf, one = guarded(xin[i:i + 1])
        alone = ops.lpips_conv2d(one, packed, bias, co, k, k, s, p, relu).permute(0, 3, 1, 2).cpu()
        assert torch.isfinite(alone).all() and torch.equal(alone, got[i:i + 1]), f"image {i}"


def test_convolution_is_generic_in_its_geometry():
    """a layer the network does not have (Cin 5, Cout 70, 3 x 2 kernel, stride 2, pad 1; 3 x 31 x 29 -> 1392 rows, 70 columns: ragged against every tile)"""
    g = torch.Generator().manual_seed(5)
    x, w, b = torch.randn(3, 5, 31, 29, generator=g), torch.randn(70, 5, 3, 2, generator=g) * 0.2, torch.randn(70, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), stride=2, padding=1)
    t32 = F.conv2d(x, w, b, stride=2, padding=1)
    got = ops.lpips_conv2d(x.permute(0, 2, 3, 1).contiguous().cuda(), ops.lpips_pack_conv_weight(w).cuda(), b.cuda(), 70, 3, 2, 2, 1, False).permute(0, 3, 1, 2).cpu()
    cmp_acc = EC.ErrAcc(); cmp_acc.add(t32, ref)
    acc = EC.ErrAcc(); acc.add(got, ref)
    rms_gate, max_gate = EC.gate(cmp_acc.rms, cmp_acc.mx)
    assert got.shape == ref.shape and acc.rms <= rms_gate and acc.mx <= max_gate, (acc.rms, acc.mx, cmp_acc.rms, cmp_acc.mx)
    nobias = ops.lpips_conv2d(x.permute(0, 2, 3, 1).contiguous().cuda(), ops.lpips_pack_conv_weight(w).cuda(), None, 70, 3, 2, 2, 1, False).permute(0, 3, 1, 2).cpu()
    assert torch.equal((nobias + b.view(1, -1, 1, 1)), got)        # the bias is one fp32 addition after the chains


# ---- pool and input stage: equality ----
@pytest.mark.parametrize("shape", [(1, 64, 7, 7), (3, 64, 8, 11), (5, 192, 3, 3), (2, 192, 16, 23), (1, 7, 4, 63)], ids=str)
def test_pool_equals_torch(shape):
    x = synth.hash_uniform(synth.name_seed(f"lpips_pool_{shape}"), shape, -1.0, 1.0)
    x[0, 0, 1, 1] = float("nan")
    x[-1, -1, -1, -1] = float("inf")
    want = F.max_pool2d(x, 3, 2)
    buf, xin = guarded(x.permute(0, 2, 3, 1).contiguous().cuda())
    out_buf, out = guarded(torch.full((shape[0],) + tuple(want.shape[2:]) + (shape[1],), float("nan"), device="cuda"))
    got = ops.lpips_maxpool3s2(xin, out=out).permute(0, 3, 1, 2).cpu()
    assert band_intact(out_buf, out.numel())
    assert got.shape == want.shape and torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got), torch.nan_to_num(want))
    assert int(torch.isnan(want).sum()) == 1                       # the NaN wins its one window (torch's rule) and no other


@pytest.mark.parametrize("signed", [True, False], ids=["signed", "unsigned"])
@pytest.mark.parametrize("quantize", [False, True], ids=["float", "u8"])
def test_input_stage_equals_the_host_expression_on_every_bf16_pattern_and_byte(signed, quantize):
    """every bf16 pattern in [0, 1] (16257 of them), every k / 255, every NormalizeToTensor output, the to_u8 sample sweep -- as recon and as original"""
    pat = np.arange(0x0000, 0x3F81, dtype=np.uint16)
    vals = (pat.astype(np.uint32) << 16).view(np.float32)
    assert vals[0] == 0.0 and vals[-1] == 1.0
    extra = np.concatenate([(np.arange(256, dtype=np.float32) / np.float32(255)).astype(np.float32), ((IO.normalize_lut() + np.float32(1)) / np.float32(2)).astype(np.float32),
                            IO.f32_samples()[np.isfinite(IO.f32_samples())].clip(0, 1)])
    H = W = 31
    for bf16, v in ((True, vals), (False, np.concatenate([vals, extra]))):
        B = -(-v.size // (H * W))
        unit = np.repeat(np.resize(v, (B, 1, H, W)), 3, axis=1).astype(np.float32)      # every value meets every channel's constants
        orig = (unit * np.float32(2) - np.float32(1)).astype(np.float32) if signed else unit
        orig = L._bf16(orig) if bf16 else orig
        want = L.input_stage(unit, orig, bf16, signed, quantize)
        got = ops.lpips_input(dev(unit, bf16), dev(orig, bf16), original_signed=signed, quantize=quantize)
        assert got.shape == (2 * B, H, W, 3)
        assert np.array_equal(got.permute(0, 3, 1, 2).cpu().numpy().view(np.uint32), want.view(np.uint32)), (bf16, signed, quantize)


# ---- the distance stage alone ----
@pytest.mark.parametrize("fc", L.FEAT_CASES, ids=lambda f: f.name)
def test_distance_stage_against_the_fp64_emulation(fc):
    """tolerance: lpips_cases.distance_tolerance (derived from the fp64 operation counts, no tuned factor)"""
    feat, w = L.make_features(fc)
    want = L.tap_distance(feat[:fc.B], feat[fc.B:], w)
    tol = L.distance_tolerance(want, fc.C, fc.h * fc.w, float(w.max()))
    buf, f = guarded(dev(feat).permute(0, 2, 3, 1).contiguous())
    got = ops.lpips_distance(f, dev(w))
    again = ops.lpips_distance(f, dev(w), out=got.clone(), accumulate=True).cpu().numpy()
    got = got.cpu().numpy()
    _record(f"distance {fc.name}: |device - emulation| {np.abs(got - want).max():.3e} (tolerance {tol.min():.3e} .. {tol.max():.3e}), value {want.min():.3e} .. {want.max():.3e}")
    assert got.dtype == np.float64 and got.shape == (fc.B,) and (np.abs(got - want) <= tol).all()
    assert np.array_equal(bits(again), bits(got + got))            # accumulate: out[b] += the same contribution
    swapped = ops.lpips_distance(torch.cat([f[fc.B:], f[:fc.B]]), dev(w)).cpu().numpy()
    assert np.array_equal(bits(swapped), bits(got))                # (a - b)^2 == (b - a)^2
    for i in range(fc.B):                                          # a pair alone
        one = ops.lpips_distance(torch.stack([f[i], f[fc.B + i]]), dev(w)).cpu().numpy()
        assert np.array_equal(bits(one), bits(got[i:i + 1]))


# ---- end to end ----
@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_network_equals_the_staged_calls_and_the_emulation(net, case):
    recon, orig = L.make(case)
    x, y = dev(recon, case.recon_bf16), dev(orig, case.orig_bf16)
    got = net(x, y, original_signed=case.signed, quantize=case.quantize).cpu().numpy()
    # the staged calls composed here, each from ops
    t = ops.lpips_input(x, y, case.signed, case.quantize)
    want_in = L.input_stage(recon, orig, case.recon_bf16, case.signed, case.quantize)
    assert np.array_equal(t.permute(0, 3, 1, 2).cpu().numpy().view(np.uint32), want_in.view(np.uint32))
    staged = None
    feats = net.features(x, y, case.signed, case.quantize)
    for i, ((_, _, co, _, k, s, p, pool), packed, bias, lin) in enumerate(zip(LP.LAYERS, net.packed, net.bias, net.lin)):
        t = ops.lpips_conv2d(t, packed, bias, co, k, k, s, p, True)
        assert torch.equal(t.permute(0, 3, 1, 2), feats[i]) and tuple(t.shape[1:3]) == LP.tap_sizes(case.H, case.W)[i]
        d = ops.lpips_distance(t, lin)
        staged = d if staged is None else staged + d
        if pool:
            t = ops.lpips_maxpool3s2(t)
    assert got.dtype == np.float64 and got.shape == (case.B,)
    assert np.array_equal(bits(got), bits(staged.cpu().numpy()))
    want = L.case_value(case.name)
    if case.content == "identical":
        assert (got == 0.0).all()
    assert np.isfinite(got).all() and (got >= 0).all()
    m = L.gated_pairs(case.name)                                   # per pair: d >= 0.05 under the emulation, whatever the content (const and recon_noise pairs too)
    assert m.all() or case not in L.GATED
    if m.any():
        rel32 = L.fp32_relative_error()
        rel = float((np.abs(got[m] - want[m]) / want[m]).max())
        _record(f"lpips {case.name}: {int(m.sum())} of {case.B} pairs gated, device relative error {rel:.3e} against the fp64 emulation (gate 4 x {rel32:.3e} = {4 * rel32:.3e}, "
                f"the largest relative error of torch-CPU fp32 features over the {len(L.GATED)} noise and smooth cases), d {want[m].min():.4f} .. {want[m].max():.4f}")
        assert rel <= 4.0 * rel32
    if not m.all():                                                # no end-to-end gate under cancellation: the two stage gates cover these pairs; the figure is recorded
        _record(f"lpips {case.name}: {int((~m).sum())} of {case.B} pairs below d = {L.D_GATED}, device |d - emulation| {np.abs(got[~m] - want[~m]).max():.3e} "
                f"at d {want[~m].min():.3e} .. {want[~m].max():.3e} (not gated)")


BATCH5 = L.BY_NAME["35x47_b5_noise_fbsq"]._replace(quantize=False)


def test_bit_for_bit_run_to_run_alone_any_order_chunked_and_symmetric(net):
    recon, orig = L.make(BATCH5)
    a, b = run(net, BATCH5, recon, orig), run(net, BATCH5, recon, orig)
    assert np.array_equal(bits(a), bits(b)) and (a > 0.05).all()
    for i in range(BATCH5.B):
        assert np.array_equal(bits(run(net, BATCH5, recon[i:i + 1], orig[i:i + 1])), bits(a[i:i + 1])), f"pair {i} alone differs from the same pair inside B = 5"
    perm = [3, 0, 4, 2, 1]
    assert np.array_equal(bits(run(net, BATCH5, recon[perm], orig[perm])), bits(a[perm]))
    try:
        for chunk in (1, 2, 3, 4):                                 # the internal chunking: ragged last chunk included
            net.chunk_pairs = chunk
            assert np.array_equal(bits(run(net, BATCH5, recon, orig)), bits(a)), f"chunks of {chunk} pairs change the value"
    finally:
        net.chunk_pairs = None
    # d(x, y) == d(y, x), d(x, x) == 0: both images in [0, 1], fp32, unsigned
    u = ((orig + np.float32(1)) / np.float32(2)).astype(np.float32)
    fwd = net(dev(recon), dev(u), original_signed=False).cpu().numpy()
    rev = net(dev(u), dev(recon), original_signed=False).cpu().numpy()
    assert np.array_equal(bits(fwd), bits(rev)) and (net(dev(u), dev(u), original_signed=False).cpu().numpy() == 0.0).all()


def test_a_nan_image_poisons_only_its_own_value(net):
    recon, orig = L.make(BATCH5)
    clean = run(net, BATCH5, recon, orig)
    for where in ((2, 1, 20, 17), (4, 2, 34, 46), (0, 0, 0, 0)):
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
    case = L.BY_NAME["67x95_b3_recon_noise_bfsx"]
    recon, orig = L.make(case)
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
    recon2, orig2 = L.make(case, seed=1)
    x.copy_(dev(recon2, case.recon_bf16)); y.copy_(dev(orig2, case.orig_bf16))
    g.replay()
    torch.cuda.synchronize()
    again = out.cpu().numpy()
    assert np.array_equal(bits(again), bits(call().cpu().numpy())) and not np.array_equal(bits(again), bits(eager))


# ---- the harness ----
class _PoolingPipe:
    """a stand-in tokenizer (evaluate only needs .device, .encoding, .decoding*): 8 x 8 mean pooling to 16 levels and nearest-neighbour decoding, every image on
    its own, so a batch's composition cannot change a value"""
    device = torch.device("cuda")

    def encoding(self, imgs, device=None):
        p = F.avg_pool2d(imgs.float(), 8)
        self.shape = tuple(p.shape[1:])
        return p.mul(7.5).add(7.5).round().clamp(0, 15).to(torch.int64).flatten(1)

    def decoding(self, ids, device=None, noise=None):
        t = torch.from_numpy(np.asarray(ids)).to(self.device).float().view(-1, *self.shape) / 15.0
        return F.interpolate(t, scale_factor=8, mode="nearest").to(torch.bfloat16)

    def decoding_with_renderer(self, ids, device=None):
        return self.decoding(ids).float() * 0.75 + 0.125


def _smooth_images(lo, hi):
    a = F.avg_pool2d(synth.synthetic_images(hi - lo, size=128, first_index=lo), 8)
    return F.interpolate(a, scale_factor=4, mode="bilinear").mul(3.0).clamp(-1, 1)                   # 64 x 64


def test_harness_lpips_option(net):
    pipe = _PoolingPipe()
    dec = ("diffusion", "renderer")
    both = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec, metrics=("psnr", "ssim"))
    full = E.evaluate(pipe, _smooth_images, 3, batch=3, decoders=dec, metrics=("psnr", "ssim", "lpips"), lpips=net)
    assert list(full) == list(both) and list(full["diffusion"]) == ["psnr_mean_dB", "psnr_each_dB", "ssim_mean", "ssim_each", "lpips_mean", "lpips_each"]
    assert full["metric_definition"]["lpips"] == dict(LP.LPIPS_DEFINITION, weights="synthetic")
    assert {k: v for k, v in full["metric_definition"].items() if k != "lpips"} == both["metric_definition"]
    imgs = _smooth_images(0, 3).cuda()
    ids = pipe.encoding(imgs).cpu().numpy()
    for d, rec in (("diffusion", pipe.decoding(ids)), ("renderer", pipe.decoding_with_renderer(ids))):
        assert {k: v for k, v in full[d].items() if not k.startswith("lpips")} == both[d]          # PSNR / SSIM entries identical to a run without "lpips"
        direct = net(rec, imgs).cpu().numpy()
        assert full[d]["lpips_each"] == [round(float(v), 9) for v in direct] and full[d]["lpips_mean"] == float(direct.mean()) and direct.min() > 0
        want = L.emulate(rec.float().cpu().numpy(), imgs.cpu().numpy(), rec.dtype == torch.bfloat16, True, False)
        assert (np.abs(direct - want) <= 4.0 * L.fp32_relative_error() * want).all() and want.min() >= 0.05, (direct, want)
    ragged = E.evaluate(pipe, _smooth_images, 3, batch=2, decoders=dec, metrics=("psnr", "ssim", "lpips"), lpips=net)
    assert ragged["batch"] == 2 and {k: v for k, v in ragged.items() if k != "batch"} == {k: v for k, v in full.items() if k != "batch"}
    only = E.evaluate(pipe, _smooth_images, 3, batch=3, metrics=("lpips",), lpips=net)
    assert only["diffusion"]["lpips_each"] == full["diffusion"]["lpips_each"]

    u8 = E.evaluate(pipe, _smooth_images, 3, batch=3, metrics=("ssim", "lpips"), metrics_u8=True, lpips=net)
    assert u8["metric_definition"]["on"] == "u8"
    direct = net(pipe.decoding(ids), imgs, quantize=True).cpu().numpy()
    assert u8["diffusion"]["lpips_each"] == [round(float(v), 9) for v in direct] and u8["diffusion"]["lpips_each"] != full["diffusion"]["lpips_each"]
    want = L.emulate(pipe.decoding(ids).float().cpu().numpy(), imgs.cpu().numpy(), True, True, True)
    assert (np.abs(direct - want) <= 4.0 * L.fp32_relative_error() * want).all()
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics=("lpips",))
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics=("psnr", "lpips"), lpips=None)
    with pytest.raises(ValueError):
        E.evaluate(pipe, _smooth_images, 3, metrics=("psnr", "fid"), lpips=net)


def test_refusals(net):
    f = torch.zeros(2, 3, 32, 32, device="cuda")
    for recon, orig in ((f.double(), f), (f, f.half()), (f, f[:1]), (f[0], f[0]), (f[:, :2], f[:, :2]), (f[..., :30], f[..., :30]), (f[..., :30, :], f[..., :30, :]),
                        (f.cpu(), f), (f, f.cpu())):
        with pytest.raises(_lib.SelftokHipError):
            net(recon, orig)
    x = torch.zeros(1, 8, 8, 4, device="cuda")
    pk = ops.lpips_pack_conv_weight(torch.zeros(64, 4, 3, 3)).cuda()
    for args in ((x, pk, None, 64, 3, 3, 1, 3, True), (x, pk, None, 64, 5, 5, 1, 1, True), (x.double(), pk, None, 64, 3, 3, 1, 1, True), (x[:, :2, :2], pk, None, 64, 3, 3, 1, 0, True),
                 (x, pk, torch.zeros(63, device="cuda"), 64, 3, 3, 1, 1, True)):
        with pytest.raises(_lib.SelftokHipError):
            ops.lpips_conv2d(*args)
    with pytest.raises(_lib.SelftokHipError):
        ops.lpips_maxpool3s2(x[:, :2])
    with pytest.raises(_lib.SelftokHipError):
        ops.lpips_distance(x[:1], torch.ones(4, device="cuda"))     # an odd number of images is no set of pairs
    with pytest.raises(_lib.SelftokHipError):
        ops.lpips_distance(torch.cat([x, x]), torch.ones(4, device="cuda"), workspace=torch.empty(7, dtype=torch.uint8, device="cuda"))
    assert (net(f, f, original_signed=False).cpu().numpy() == 0.0).all()
