"""not gpu: the rFID arithmetic of record (tests/fid_cases.py) pinned on the host -- the emulation against an independent formulation (folded weights,
im2col + einsum), the shapes of the maps, the condition on the synthetic weights, the planted mistakes the case table must be able to see, the Frechet
distance against closed forms and scipy, the new C entries against the ctypes table, the kernels' scratch / LDS budget, the weight-file loader and the
host-side refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fid_cases as FC
from selftoktokenizer_amd import _lib, evaluate as E, fid as FD, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_fid_conv2d_f32", "selftok_fid_pool3_f32", "selftok_fid_input", "selftok_fid_spatial_mean_f32", "selftok_fid_stats_workspace_bytes",
               "selftok_fid_stats"}


def test_case_table_and_map_shapes():
    assert {(c.H, c.W) for c in FC.CASES if not c.resize} == {(75, 75), (76, 75), (91, 107)}
    assert {(c.H, c.W) for c in FC.CASES if c.resize} == {(64, 64), (256, 256), (299, 299), (320, 200)}
    assert {c.B for c in FC.CASES} == {1, 3} and {c.content for c in FC.CASES} == set(FC.CONTENTS) and len({c.name for c in FC.CASES}) == len(FC.CASES)
    assert len({(c.bf16, c.signed, c.quantize) for c in FC.CASES}) == 8
    assert FD.map_sizes(299, 299) == [(35, 35), (17, 17), (8, 8)] and FD.map_sizes(75, 75) == [(7, 7), (3, 3), (1, 1)]
    assert FD.map_sizes(91, 107) == [(9, 11), (4, 5), (1, 2)] and FD.map_sizes(76, 75) == [(7, 7), (3, 3), (1, 1)]
    assert len(FD.UNITS) == 94 and len(FD.state_shapes()) == 94 * 5
    keep = {}
    case = FC.BY_NAME["91x107_b1_const_fsx"]
    f = FC.pool3(FC.make(case), case.bf16, case.signed, case.quantize, False, keep=keep)
    want = {"stem": 192, "Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768, "Mixed_6e": 768,
            "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}
    assert {k: v.shape[1] for k, v in keep.items() if k != "input"} == want and f.shape == (1, 2048) and tuple(keep["Mixed_7c"].shape[2:]) == (1, 2)
    for c in FC.CASES:
        x = FC.make(c)
        assert x.dtype == np.float32 and x.shape == (c.B, 3, c.H, c.W) and (not c.bf16 or not (x.view(np.uint32) & 0xFFFF).any())
        assert (-1 if c.signed else 0) <= x.min() and x.max() <= 1


def test_definition_of_record():
    d = FD.FID_DEFINITION
    assert (d["features"], d["dim"], d["bn_eps"], d["min_side"]) == ("pool3", 2048, 1e-3, 75) and "pytorch-fid" in d["net"] and "count_include_pad=False" in d["pools"]
    assert d["units"]["Mixed_6b.branch7x7_2"] == [128, 128, 1, 7, 1, 0, 3] and d["units"]["Mixed_7c.branch3x3_2b"] == [384, 384, 3, 1, 1, 1, 0]
    assert d["units"]["Conv2d_1a_3x3"] == [3, 32, 3, 3, 2, 0, 0] and d["units"]["Mixed_5b.branch5x5_2"] == [48, 64, 5, 5, 1, 2, 2]
    assert "unpinned against the package" in FD.__doc__


@pytest.mark.parametrize("name", ["75x75_b1_noise_fux", "91x107_b1_const_fsx"])
def test_emulation_equals_the_independent_formulation(name):
    """torch conv2d + unfolded batch_norm + torch pools in fp64 == folded weights, explicit im2col + einsum, window pools in numpy fp64: the stem and every block
    (each of the five block types several times), to 1e-12 of the map's largest value"""
    case = FC.BY_NAME[name]
    keep, keep2 = {}, {}
    f = FC.pool3(FC.make(case), case.bf16, case.signed, case.quantize, False, keep=keep)
    m = FC.network(keep["input"].numpy(), FC.NumpyOps(), keep2)
    assert set(keep2) == set(keep) - {"input"} and len(keep2) == 12
    for k, v in keep2.items():
        assert np.abs(v - keep[k].numpy()).max() <= 1e-12 * np.abs(v).max(), k
    assert np.abs(m.mean((2, 3)) - f).max() <= 1e-12 * np.abs(f).max() and np.array_equal(f, FC.case_features(name))


def test_resize_tables_and_their_blend():
    for n_in in (64, 200, 256, 299, 320, 1, 600):
        for got, want in zip(FD.resize_taps(n_in, 299), FC.taps(n_in, 299)):
            assert got.dtype == want.dtype and np.array_equal(got, want), n_in
    i0, i1, lam = FD.resize_taps(299, 299)
    assert np.array_equal(i0, np.arange(299)) and not lam.any()                         # identity: every lambda is zero
    i0, i1, lam = FD.resize_taps(64, 299)
    assert i0[0] == 0 and lam[0] == 0 and i1[-1] == 63 and i0.max() == 63 and (lam >= 0).all() and (lam < 1).all()
    x = FC.to_signed(FC.make(FC.BY_NAME["320x200_b1_smooth_bux_resize"]), True, False, False)
    a, b = FC.resize(x).numpy(), FC.resize_tables_f64(x)
    assert a.shape == (1, 3, 299, 299) and np.abs(a - b).max() <= 4 * FC.U32       # the fp32 lambda of the table against torch's fp64 one: 2u per axis
    assert FC.resize(np.zeros((1, 3, 299, 299), np.float32)).shape == (1, 3, 299, 299)


def test_synthetic_weights_keep_different_images_apart():
    """a condition on the table: every pair of different-content images has pool3 features >= 1e-2 apart (relative), and the rms is in [1e-3, 1e2]"""
    rows = [(c.name, i, c.content, f) for c in FC.CASES for i, f in enumerate(FC.case_features(c.name))]
    for _, _, _, f in rows:
        assert 1e-3 <= np.sqrt((f * f).mean()) <= 1e2
    worst = 9.0
    for a in range(len(rows)):
        for b in range(a):
            fa, fb = rows[a][3], rows[b][3]
            worst = min(worst, np.linalg.norm(fa - fb) / max(np.linalg.norm(fa), np.linalg.norm(fb)))
    print(f"\nclosest pair of images of the table: {worst:.3e} relative")
    assert worst >= 1e-2
    rel = FC.fp32_relative_error()
    print(f"torch-CPU fp32 against the fp64 emulation, largest per-image relative error over the table: {rel:.3e} (the pool3 gate is 4 x this)")
    assert 0 < rel < 1e-5


def _visible(mut, case):
    if mut == "avg_in_7c":                      # on a 1 x 1 map the 3 x 3 / pad 1 maximum and the in-image average are the same value
        return case.resize or (case.H, case.W) == (91, 107)
    if mut == "align_corners":                  # (in - 1) / (out - 1) against in / out: a smooth image hardly moves (1e-3 at 200 -> 299), and at 256 -> 299 the
        return case.resize and case.content == "noise" and not (0.8 < min(case.H, case.W) / FD.SIDE < 1.25)      # two differ by 0.07 pixel at most (noise: 3e-3)
    return True


@pytest.mark.parametrize("mut", FC.MUTS)
def test_every_case_that_can_see_a_planted_mistake_sees_it(mut):
    """each mistake moves every image of every case that can see it by >= 1000 x the GPU gate (4 x torch fp32's relative error)"""
    gate = 4.0 * FC.fp32_relative_error()
    seen = 0
    for case in [c for c in FC.CASES if _visible(mut, c)]:
        moved = FC.rel_err(FC.case_features(case.name, torch.float64, mut), FC.case_features(case.name))
        assert (moved >= 1000 * gate).all(), f"{case.name}: {mut} moves pool3 by only {moved.min():.2e} (1000 x gate = {1000 * gate:.2e})"
        seen += 1
    assert seen >= {"avg_in_7c": 10, "align_corners": 1}.get(mut, len(FC.CASES)), seen


def test_tail_mistakes_move_the_end_to_end_distance():
    d = FC.set_distance()
    d32 = FC.set_distance(torch.float32)
    gate = 4.0 * abs(d32 - d)
    print(f"\nend to end: d^2 {d:.6f}; torch-CPU fp32 features through the fp64 tail deviate by {abs(d32 - d):.3e} ({abs(d32 - d) / d:.3e} relative)")
    assert d > 1.0 and 0 < gate < 1e-3 * d                                              # d^2 well away from 0
    for mut in FC.TAIL_MUTS:
        assert abs(FC.set_distance(mut=mut) - d) >= 1000 * gate, mut
    for which in ("smooth", "noise"):                                                   # the premise of stats_tolerance's second-order term
        X = FC.set_features(which, torch.float32).astype(np.float64)
        live = X.std(0) > 0
        assert (np.abs(X).mean(0)[live] <= 1e3 * X.std(0)[live]).all()


def _spd(D, seed, lo=0.5, hi=2.0):
    g = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(g.standard_normal((D, D)))
    return Q, g.uniform(lo, hi, D)


def test_frechet_distance_against_closed_forms_and_scipy():
    D = 64
    Q, a = _spd(D, 1)
    _, b = _spd(D, 2)
    g = np.random.default_rng(3)
    m1, m2 = g.standard_normal(D), g.standard_normal(D)
    s1 = (Q * a) @ Q.T
    s1 = (s1 + s1.T) / 2
    assert abs(FD.frechet_distance(m1, s1, m1, s1)) <= 1e-9 * np.trace(s1)
    # diagonal covariances
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((m1 - m2) ** 2).sum()
    assert abs(FD.frechet_distance(m1, np.diag(a), m2, np.diag(b)) - want) <= 1e-10 * want
    # commuting covariances: one eigenbasis
    s2 = (Q * b) @ Q.T
    s2 = (s2 + s2.T) / 2
    assert abs(FD.frechet_distance(m1, s1, m2, s2) - want) <= 1e-10 * want
    assert abs(FC.frechet(m1, s1, m2, s2) - want) <= 1e-10 * want
    # torch tensors are taken too
    assert FD.frechet_distance(torch.from_numpy(m1), torch.from_numpy(s1), torch.from_numpy(m2), torch.from_numpy(s2)) == FD.frechet_distance(m1, s1, m2, s2)
    # rank-deficient: N = 8 samples at D = 64; against the non-zero eigenvalues of the 8 x 8 dual problem: tr (s1 s2)^(1/2) = sum of the singular values of
    # A1 A2^T / (N - 1) with A the centred sample matrices
    X1, X2 = g.standard_normal((8, D)), g.standard_normal((8, D)) + 0.5
    (mu1, c1), (mu2, c2) = FC.statistics(X1), FC.statistics(X2)
    sv = np.linalg.svd((X1 - mu1) @ (X2 - mu2).T / 7.0, compute_uv=False)
    want = ((mu1 - mu2) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2.0 * sv.sum()
    got = FD.frechet_distance(mu1, c1, mu2, c2)
    assert np.linalg.matrix_rank(c1) == 7 and np.isfinite(got) and abs(got - want) <= 1e-7 * want, (got, want)      # sqrt of eigenvalues near 0: ~sqrt(u) each
    assert abs(FC.frechet(mu1, c1, mu2, c2) - got) <= 1e-7 * want
    # scipy's sqrtm on well-conditioned matrices (test-only: the product does not import scipy)
    from scipy import linalg as SL
    Q2, b2 = _spd(D, 4)
    s3 = (Q2 * b2) @ Q2.T
    s3 = (s3 + s3.T) / 2
    want = ((m1 - m2) ** 2).sum() + np.trace(s1) + np.trace(s3) - 2.0 * np.trace(SL.sqrtm(s1 @ s3)).real
    assert abs(FD.frechet_distance(m1, s1, m2, s3) - want) <= 1e-9 * want
    src = open(os.path.join(ROOT, "selftoktokenizer_amd", "fid.py")).read()
    assert "import scipy" not in src and "from scipy" not in src
    with pytest.raises(ValueError):
        FD.frechet_distance(m1, s1, m2[:3], s2)


def test_stats_files_round_trip(tmp_path):
    g = np.random.default_rng(0)
    mu, sigma = g.standard_normal(16), g.standard_normal((16, 16))
    p = str(tmp_path / "ref.npz")
    FD.save_stats(p, torch.from_numpy(mu), sigma)
    with np.load(p) as z:
        assert sorted(z.files) == ["mu", "sigma"]
    m, s = FD.load_stats(p)
    assert np.array_equal(m, mu) and np.array_equal(s, sigma) and m.dtype == np.float64
    np.savez(p, mu=mu)
    with pytest.raises(KeyError, match="sigma"):
        FD.load_stats(p)
    np.savez(p, mu=mu, sigma=sigma[:8])
    with pytest.raises(ValueError):
        FD.load_stats(p)


def test_ext_header_declares_the_fid_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and names == set(_lib.EXT_SIGNATURES) and not (names & set(_lib.SIGNATURES))
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    for n in NEW_ENTRIES:
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want, (n, args)
        assert res == ctype_of[m.group(1)]
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_fid_compiles_for_gfx950_without_scratch_and_shares_the_convolution(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "fid.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(kernels) == 11 and len(scratch) == len(lds) == len(occ) == 11, kernels     # conv x 2, pool x 3, input x 2, mean, column sums, mu, covariance
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    conv = [i for i, k in enumerate(kernels) if "fid_conv_kernel" in k]
    assert len(conv) == 2 and all(lds[i] == 8704 for i in conv) and all(occ[i] == 3 for i in conv)       # the LPIPS kernel's budget: it is the same body
    src = open(os.path.join(G.CSRC, "fid.hip")).read()
    lp = open(os.path.join(G.CSRC, "lpips.hip")).read()
    assert "asm" not in src and "atomic" not in src.replace("No atomics", "") and "mfma" not in src.split("#include", 1)[1]
    assert "conv_f32::conv_tile<VEC>(a)" in src and "conv_f32::conv_tile<VEC>(a)" in lp                 # one body, in csrc/conv_f32_shared.h


def _state_equal(a, b):
    return all(torch.equal(a.packed[k], b.packed[k]) and torch.equal(a.bias[k], b.bias[k]) for k in FD.UNITS)


def test_from_files_round_trips_and_refuses(tmp_path):
    sd = FD.InceptionNet.synthetic_tensors()
    mem = FD.InceptionNet(sd, "cpu", "synthetic")
    assert mem.source == "synthetic" and tuple(mem.packed["Conv2d_1a_3x3"].shape) == (32, 64) and tuple(mem.packed["Mixed_6b.branch7x7_2"].shape) == (896, 128)
    name = "Mixed_7c.branch3x3_2b"
    scale = sd[name + ".bn.weight"].double() / torch.sqrt(sd[name + ".bn.running_var"].double() + 1e-3)
    w = (sd[name + ".conv.weight"].double() * scale.view(-1, 1, 1, 1)).float()
    assert torch.equal(mem.packed[name][:1152].reshape(3, 1, 384, 384), w.permute(2, 3, 1, 0))                  # k = (kh, kw, ci), folded in fp64, rounded once
    assert torch.equal(mem.bias[name], (sd[name + ".bn.bias"].double() - sd[name + ".bn.running_mean"].double() * scale).float())
    full = dict(sd, **{"fc.weight": torch.zeros(3, 3), "AuxLogits.conv0.conv.weight": torch.zeros(2), "Conv2d_1a_3x3.bn.num_batches_tracked": torch.zeros(())})
    p = str(tmp_path / "pt_inception-2015-12-05.pth")
    torch.save(full, p)
    net = FD.InceptionNet.from_files(p, "cpu")
    assert _state_equal(net, mem) and net.source == "pt_inception-2015-12-05.pth"
    torch.save({k: v for k, v in full.items() if k != "Mixed_6e.branch7x7dbl_4.bn.running_var"}, p)
    with pytest.raises(KeyError, match="Mixed_6e.branch7x7dbl_4.bn.running_var"):
        FD.InceptionNet.from_files(p, "cpu")
    torch.save(dict(full, **{"Mixed_6b.branch7x7_2.conv.weight": torch.zeros(128, 128, 7, 1)}), p)
    with pytest.raises(ValueError, match="Mixed_6b.branch7x7_2.conv.weight"):
        FD.InceptionNet.from_files(p, "cpu")


class _NoPipe:
    device = torch.device("cpu")


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.zeros(4096, np.float32)
    d = np.zeros(4096)
    p, dp = x.ctypes.data, d.ctypes.data
    conv = lambda i, w, o, N, H, W, Cin, Cout, KH, KW, s, ph, pw, ldo, off: lib.selftok_fid_conv2d_f32(i, w, None, o, N, H, W, Cin, Cout, KH, KW, s, ph, pw, ldo, off, 1, None)
    ok = (1, 8, 8, 4, 64, 1, 7, 1, 0, 3, 64, 0)
    for args, word in (((None, p, p) + ok, "null"), ((p, None, p) + ok, "null"), ((p, p, None) + ok, "null"),
                       ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 1, 1, 3, 64, 0), "pad_h"), ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 1, 0, 7, 64, 0), "pad_w"),
                       ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 1, 0, -1, 64, 0), "pad_w"), ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 0, 0, 3, 64, 0), "stride"),
                       ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 1, 0, 3, 63, 0), "ldo"), ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 1, 0, 3, 96, 36), "ldo"),
                       ((p, p, p, 1, 8, 8, 4, 64, 1, 7, 1, 0, 3, 96, -4), "co_off"), ((p, p, p, 1, 8, 2, 4, 64, 1, 7, 1, 0, 0, 64, 0), "no output pixel"),
                       ((p, p, p, 32768, 256, 256, 4, 64, 3, 3, 1, 1, 1, 64, 0), "2^31"), ((p, p, p, 4, 64, 64, 4, 64, 3, 3, 1, 1, 1, 1 << 20, 0), "2^31"),
                       ((p + 4, p, p) + ok, "aligned")):
        assert conv(*args) == -1 and word in err(), (args[3:], word, err())
    pool = lambda i, o, N, H, W, C, mode, ldo, off: lib.selftok_fid_pool3_f32(i, o, N, H, W, C, mode, ldo, off, None)
    for args, word in (((None, p, 1, 7, 7, 64, 0, 64, 0), "null"), ((p, None, 1, 7, 7, 64, 0, 64, 0), "null"), ((p, p, 1, 2, 7, 64, 0, 64, 0), "H, W >= 3"),
                       ((p, p, 1, 7, 7, 64, 3, 64, 0), "mode"), ((p, p, 1, 7, 7, 64, -1, 64, 0), "mode"), ((p, p, 1, 7, 7, 64, 2, 63, 0), "ldo"),
                       ((p, p, 1, 7, 7, 64, 1, 96, 33), "ldo"), ((p, p, 65536, 256, 256, 64, 1, 64, 0), "2^31"), ((p, p, 0, 7, 7, 64, 1, 64, 0), "N")):
        assert pool(*args) == -1 and word in err(), (args[2:], word, err())
    inp = lambda s, o, B, H, W, OH, OW, yt, xt: lib.selftok_fid_input(s, 0, 1, 0, o, B, H, W, OH, OW, yt, xt, None)
    for args, word in (((None, p, 1, 75, 75, 75, 75, None, None), "null"), ((p, None, 1, 75, 75, 75, 75, None, None), "null"), ((p, p, 1, 64, 64, 299, 299, None, None), "tap tables"),
                       ((p, p, 1, 64, 64, 299, 299, p, None), "go together"), ((p, p, 0, 75, 75, 75, 75, None, None), "B"), ((p, p, 4096, 512, 512, 512, 512, None, None), "2^31"),
                       ((p, p, 8192, 64, 64, 299, 299, p, p), "2^31")):
        assert inp(*args) == -1 and word in err(), (args[2:], word, err())
    assert lib.selftok_fid_spatial_mean_f32(None, p, 1, 1, 16, None) == -1 and "null" in err()
    assert lib.selftok_fid_spatial_mean_f32(p, p, 1, 0, 16, None) == -1 and "npix" in err()
    assert lib.selftok_fid_spatial_mean_f32(p, p, 1 << 20, 64, 2048, None) == -1 and "2^31" in err()
    ws = lib.selftok_fid_stats_workspace_bytes
    assert ws(2, 16) == 16 * 8 and ws(256, 2048) == 2048 * 8 and ws(257, 2048) == 2 * 2048 * 8 and ws(50000, 2048) == 196 * 2048 * 8
    for N, D in ((1, 16), (0, 16), (2, 8), (2, 24), (2, 0), (1 << 24, 16), (1 << 20, 2048)):
        assert ws(N, D) == 0 and "fid_stats" in err(), (N, D)
    stats = lambda xx, mu, sg, w, wb, N, D: lib.selftok_fid_stats(xx, mu, sg, w, wb, N, D, None)
    for args, word in (((None, dp, dp, dp, 1 << 20, 2, 16), "null"), ((p, None, dp, dp, 1 << 20, 2, 16), "null"), ((p, dp, None, dp, 1 << 20, 2, 16), "null"),
                       ((p, dp, dp, None, 1 << 20, 2, 16), "null"), ((p, dp, dp, dp, 127, 2, 16), "workspace"), ((p, dp, dp, dp, 1 << 20, 1, 16), "N"),
                       ((p, dp, dp, dp, 1 << 20, 2, 20), "multiple of 16"), ((p, dp, dp + 4, dp, 1 << 20, 2, 16), "aligned")):
        assert stats(*args) == -1 and word in err(), (args[4:], word, err())
    t = torch.zeros(1, 3, 80, 80)
    net = FD.InceptionNet(FD.InceptionNet.synthetic_tensors(), "cpu", "synthetic")
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        net.pool3(t, True)
    with pytest.raises(_lib.SelftokHipError, match="H, W >= 75"):
        net.pool3(t[..., :74, :], True, resize=False)
    with pytest.raises(_lib.SelftokHipError, match=r"\[B, 3, H, W\]"):
        net.pool3(t[:, :2], True)
    with pytest.raises(_lib.SelftokHipError, match="dtype"):
        net.pool3(t.double(), True)
    with pytest.raises(_lib.SelftokHipError):
        ops.fid_pool3(torch.zeros(1, 4, 4, 8), "median")
    with pytest.raises(ValueError, match="rfid"):
        E.evaluate(_NoPipe(), lambda lo, hi: t, 2, metrics=("psnr", "rfid"))               # "rfid" without fid=: the weights are not shipped
    with pytest.raises(ValueError):
        E.evaluate(_NoPipe(), lambda lo, hi: t, 2, metrics=("rfid",))
