"""not gpu: the LPIPS arithmetic of record (tests/lpips_cases.py) pinned on the host -- the emulation against an independent im2col + einsum
formulation, its exact properties (d(x, x) = 0, symmetry), the planted mistakes the case tables must be able to see, the d >= 0.05 condition
of the end-to-end gate, the new C entries against the ctypes table, the kernels' scratch / LDS / occupancy budget, the weight-file loader,
and the host-side refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lpips_cases as L
from selftoktokenizer_amd import _lib, evaluate as E, lpips as LP, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_lpips_conv2d_packed_floats", "selftok_lpips_conv2d_f32", "selftok_lpips_maxpool3s2_f32", "selftok_lpips_input",
               "selftok_lpips_distance_workspace_bytes", "selftok_lpips_distance"}


def test_case_table_covers_what_it_claims():
    assert {(c.H, c.W) for c in L.CASES} == {(31, 31), (35, 47), (67, 95), (64, 64), (256, 256)}
    assert {c.B for c in L.CASES if c.H < 256} == {1, 3, 5} and max(c.B for c in L.CASES if c.H == 256) <= 2
    assert {c.content for c in L.CASES} == set(L.CONTENTS) and len({c.name for c in L.CASES}) == len(L.CASES)
    assert len({(c.recon_bf16, c.orig_bf16, c.signed, c.quantize) for c in L.CASES}) == 16
    assert LP.tap_sizes(31, 31) == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)] and LP.tap_sizes(256, 256) == [(63, 63), (31, 31), (15, 15), (15, 15), (15, 15)]
    for c in L.CASES:
        recon, orig = L.make(c)
        assert recon.dtype == np.float32 and orig.dtype == np.float32 and recon.shape == (c.B, 3, c.H, c.W) == orig.shape
        assert not c.recon_bf16 or not (recon.view(np.uint32) & 0xFFFF).any()
        assert not c.orig_bf16 or not (orig.view(np.uint32) & 0xFFFF).any()
        assert 0 <= recon.min() and recon.max() <= 1 and (-1 if c.signed else 0) <= orig.min() and orig.max() <= 1


def test_definition_is_the_published_one():
    d = LP.LPIPS_DEFINITION
    assert (d["net"], d["version"], d["eps"], d["min_side"]) == ("alex", "0.1", 1e-10, 31)
    assert d["shift"] == [-0.030, -0.088, -0.188] and d["scale"] == [0.458, 0.448, 0.450]
    assert [(l["kernel"], l["stride"], l["pad"], l["channels"]) for l in d["layers"]] == [(11, 4, 2, [3, 64]), (5, 1, 2, [64, 192]), (3, 1, 1, [192, 384]),
                                                                                       (3, 1, 1, [384, 256]), (3, 1, 1, [256, 256])]
    assert np.array_equal(L.SHIFT, np.array(d["shift"], np.float32)) and np.array_equal(L.SCALE, np.array(d["scale"], np.float32))


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.name)
def test_emulation_equals_the_independent_formulation(case):
    """torch conv2d / max_pool2d in fp64 == explicit im2col + einsum in numpy fp64 (1e-25: the second formulation's two halves of an identical pair need not
    be the same bits, the emulation of record's are)"""
    recon, orig = L.make(case)
    v, v2 = L.case_value(case.name), L.emulate_im2col(recon, orig, case.recon_bf16, case.signed, case.quantize)
    assert v.shape == (case.B,) and np.isfinite(v).all()
    assert (np.abs(v2 - v) <= 1e-12 * v + 1e-25).all(), (v, v2)


def test_identical_pairs_are_zero_and_the_distance_is_symmetric():
    seen = 0
    for case in L.CASES:
        if case.content == "identical":
            assert (L.case_value(case.name) == 0.0).all(), case.name
            seen += 1
    assert seen >= 8
    for case in [c for c in L.CASES if c.content in ("noise", "recon_noise") and c.H < 256 and not c.quantize]:
        recon, orig = L.make(case)
        x0, x1 = L.to_signed(recon, orig, case.recon_bf16, case.signed, False)
        fwd = L.distance(L.features(L.scaling_layer(np.concatenate([x0, x1]))))
        rev = L.distance(L.features(L.scaling_layer(np.concatenate([x1, x0]))))
        assert np.array_equal(fwd.view(np.uint64), rev.view(np.uint64)), case.name
        assert np.array_equal(fwd.view(np.uint64), L.case_value(case.name).view(np.uint64))


def test_gated_cases_are_far_from_cancellation():
    """the end-to-end relative gate is only meaningful where d is not a difference of near-equal features: every gated case has d >= 0.05"""
    assert len(L.GATED) >= 16 and any(c.H == 256 for c in L.GATED)
    for case in L.GATED:
        assert L.case_value(case.name).min() >= 0.05, (case.name, L.case_value(case.name))
    # the gate is per pair: every pair of the table at d >= 0.05 is gated, whatever its content -- most const pairs are, the small-noise reconstructions are not
    pairs = {content: sum(int(L.gated_pairs(c.name).sum()) for c in L.CASES if c.content == content) for content in L.CONTENTS}
    total = {content: sum(c.B for c in L.CASES if c.content == content) for content in L.CONTENTS}
    print(f"\npairs with d >= {L.D_GATED} of all pairs, by content: " + ", ".join(f"{k} {pairs[k]} / {total[k]}" for k in L.CONTENTS))
    assert pairs["noise"] == total["noise"] and pairs["smooth"] == total["smooth"] and pairs["identical"] == 0 and 2 * pairs["const"] >= total["const"]
    rel = L.fp32_relative_error()
    print(f"torch-CPU fp32 features against the fp64 emulation, largest relative error over the {len(L.GATED)} noise and smooth cases: {rel:.3e} "
          f"(the gate, 4 x this, is applied to all {sum(pairs.values())} pairs at d >= {L.D_GATED})")
    assert 0 < rel < 1e-5


def _visible(mut, case):
    if case.content == "identical":
        return False
    if mut == "ceil_pool":                      # only where a pooled side is even: floor and ceil then differ
        return any(s % 2 == 0 for s in LP.tap_sizes(case.H, case.W)[0] + LP.tap_sizes(case.H, case.W)[1])
    if mut == "conv1_pad0":                     # at 31 x 31 the unpadded network has no pixel left at tap 3: the mistake is an error there, not a value
        return min(case.H, case.W) >= 35
    return mut != "eps_inside"                  # sqrt(s + eps) against sqrt(s) + eps differ by 5e-11 relative at ordinary norms: only the crafted features see it


@pytest.mark.parametrize("mut", [m for m in L.MUTS if m != "eps_inside"])
def test_every_case_that_can_see_a_planted_mistake_sees_it(mut):
    """each mistake moves every pair of every case that can see it by >= 1000 x that case's GPU gate (4 x torch fp32's relative error x d)"""
    rel_gate = 4.0 * L.fp32_relative_error()
    seen = 0
    for case in [c for c in L.CASES if _visible(mut, c)]:
        v = L.case_value(case.name)
        moved = np.abs(L.case_value(case.name, torch.float64, mut) - v)
        assert (moved >= 1000 * rel_gate * v).all(), f"{case.name}: {mut} moves d by only {moved.min():.2e} ({v})"
        seen += 1
    assert seen >= {"ceil_pool": 10, "conv1_pad0": 20}.get(mut, 30), seen


def test_crafted_features_see_the_eps_inside_the_root():
    seen = 0
    for fc in L.FEAT_CASES:
        feat, w = L.make_features(fc)
        v = L.tap_distance(feat[:fc.B], feat[fc.B:], w)
        assert np.isfinite(v).all() and v.shape == (fc.B,)
        if fc.content != "tiny":
            continue
        moved = np.abs(L.tap_distance(feat[:fc.B], feat[fc.B:], w, "eps_inside") - v)
        tol = L.distance_tolerance(v, fc.C, fc.h * fc.w, float(w.max()))
        assert (moved >= 1000 * tol).all(), (fc.name, moved, tol)
        seen += 1
    assert seen >= 2
    z = np.zeros((2, 8, 2, 2), np.float32)
    assert (L.tap_distance(z[:1], z[1:], np.ones(8, np.float32)) == 0.0).all()          # 0 / eps = 0: the eps keeps an all-zero pixel finite


def test_ext_header_declares_the_lpips_entries():
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


def test_lpips_compiles_for_gfx950_within_its_budget(tmp_path):
    """0 scratch everywhere; the convolution kernel's LDS and occupancy are what DESIGN.md section 24 states"""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "lpips.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(kernels) == 9 and len(scratch) == len(lds) == len(occ) == 9, kernels      # conv x 2, pool, input x 4 dtype pairs, distance, finish
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    conv = [i for i, k in enumerate(kernels) if "lpips_conv_kernel" in k]
    assert len(conv) == 2 and all(lds[i] == 2 * 16 * 68 * 4 == 8704 for i in conv) and all(occ[i] == 3 for i in conv), [(kernels[i], lds[i], occ[i]) for i in conv]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "8704 bytes" in design and "3 waves per SIMD" in design
    src = open(os.path.join(G.CSRC, "lpips.hip")).read()
    assert "asm" not in src and "atomic" not in src.replace("No atomics", "") and "mfma_f32_32x32x2f32" in src


def _packed_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.packed + a.bias + a.lin, b.packed + b.bias + b.lin))


def test_from_files_round_trips_and_refuses(tmp_path):
    sd, lin = LP.LpipsNet.synthetic_tensors()
    mem = LP.LpipsNet(sd, lin, "cpu", "synthetic")
    assert mem.source == "synthetic" and all((w >= 0).all() for w in mem.lin) and [tuple(p.shape) for p in mem.packed] == [(368, 64), (1600, 192), (1728, 384), (3456, 256), (2304, 256)]
    w1 = sd["features.0.weight"]
    assert torch.equal(mem.packed[0][:363].reshape(11, 11, 3, 64), w1.permute(2, 3, 1, 0)) and not mem.packed[0][363:].any()      # k = (kh, kw, ci); zero K tail
    full = dict(sd, **{"classifier.1.weight": torch.zeros(3, 3), "features.0.num_batches_tracked": torch.zeros(())})     # extra keys are ignored
    lins = {f"lin{i}.model.1.weight": w for i, w in enumerate(lin)}
    lins["version"] = torch.tensor(0.1)
    bp, lp = str(tmp_path / "alexnet-owt.pth"), str(tmp_path / "alex.pth")
    torch.save(full, bp); torch.save(lins, lp)
    net = LP.LpipsNet.from_files(bp, lp, "cpu")
    assert _packed_equal(net, mem) and net.source == ["alexnet-owt.pth", "alex.pth"]
    missing = {k: v for k, v in full.items() if k != "features.8.bias"}
    torch.save(missing, bp)
    with pytest.raises(KeyError, match="features.8.bias"):
        LP.LpipsNet.from_files(bp, lp, "cpu")
    torch.save(dict(full, **{"features.3.weight": torch.zeros(192, 64, 3, 3)}), bp)
    with pytest.raises(ValueError, match="features.3.weight"):
        LP.LpipsNet.from_files(bp, lp, "cpu")
    torch.save(full, bp)
    torch.save({k: v for k, v in lins.items() if k != "lin4.model.1.weight"}, lp)
    with pytest.raises(KeyError, match="lin4"):
        LP.LpipsNet.from_files(bp, lp, "cpu")
    torch.save(dict(lins, **{"lin2.model.1.weight": torch.zeros(1, 256, 1, 1)}), lp)
    with pytest.raises(ValueError, match="lin2"):
        LP.LpipsNet.from_files(bp, lp, "cpu")


class _NoPipe:
    device = torch.device("cpu")


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    assert lib.selftok_lpips_conv2d_packed_floats(3, 64, 11, 11) == 368 * 64 and lib.selftok_lpips_conv2d_packed_floats(384, 256, 3, 3) == 3456 * 256
    assert lib.selftok_lpips_conv2d_packed_floats(3, 65, 1, 1) == 16 * 128 and lib.selftok_lpips_conv2d_packed_floats(0, 64, 3, 3) == 0
    assert lib.selftok_lpips_distance_workspace_bytes(1, 1) == 8 and lib.selftok_lpips_distance_workspace_bytes(3, 65) == 48
    assert lib.selftok_lpips_distance_workspace_bytes(64, 63 * 63) == 64 * 63 * 8
    assert lib.selftok_lpips_distance_workspace_bytes(0, 4) == 0 and "B" in err() and lib.selftok_lpips_distance_workspace_bytes(1, 0) == 0
    x = np.zeros(4096, np.float32)
    d = np.zeros(64)
    p = x.ctypes.data
    inp = lambda recon, orig, out, B, H, W: lib.selftok_lpips_input(recon, 0, orig, 0, 1, 0, out, B, H, W, None)
    for args, word in (((None, p, p, 1, 31, 31), "null"), ((p, None, p, 1, 31, 31), "null"), ((p, p, None, 1, 31, 31), "null"), ((p, p, p, 1, 30, 31), "H, W >= 31"),
                       ((p, p, p, 1, 31, 30), "H, W >= 31"), ((p, p, p, 0, 31, 31), "B >= 1"), ((p, p, p, 1366, 512, 512), "2^31"), ((p, p, p, 1, 18919, 18919), "2^31")):
        assert inp(*args) == -1 and word in err(), (args[3:], word, err())
    conv = lambda i, w, o, N, H, W, Cin, Cout, KH, KW, s, pd: lib.selftok_lpips_conv2d_f32(i, w, None, o, N, H, W, Cin, Cout, KH, KW, s, pd, 1, None)
    for args, word in (((None, p, p, 1, 8, 8, 4, 64, 3, 3, 1, 1), "null"), ((p, None, p, 1, 8, 8, 4, 64, 3, 3, 1, 1), "null"), ((p, p, None, 1, 8, 8, 4, 64, 3, 3, 1, 1), "null"),
                       ((p, p, p, 1, 2, 8, 4, 64, 5, 5, 1, 0), "no output pixel"), ((p, p, p, 1, 8, 8, 4, 64, 3, 3, 1, 3), "pad"), ((p, p, p, 1, 8, 8, 4, 64, 3, 3, 0, 1), "stride"),
                       ((p, p, p, 32768, 256, 256, 4, 64, 3, 3, 1, 1), "2^31"), ((p + 4, p, p, 1, 8, 8, 4, 64, 3, 3, 1, 1), "aligned")):
        assert conv(*args) == -1 and word in err(), (args[3:], word, err())
    assert lib.selftok_lpips_maxpool3s2_f32(p, None, 1, 7, 7, 64, None) == -1 and "null" in err()
    assert lib.selftok_lpips_maxpool3s2_f32(p, p, 1, 2, 7, 64, None) == -1 and "H, W >= 3" in err()
    assert lib.selftok_lpips_maxpool3s2_f32(p, p, 65536, 256, 256, 64, None) == -1 and "2^31" in err()
    dist = lambda f, w, o, ws, wb, B, npix, C: lib.selftok_lpips_distance(f, w, o, ws, wb, B, npix, C, 0, None)
    dp = d.ctypes.data
    for args, word in (((None, p, dp, dp, 64, 1, 49, 64), "null"), ((p, None, dp, dp, 64, 1, 49, 64), "null"), ((p, p, None, dp, 64, 1, 49, 64), "null"),
                       ((p, p, dp, None, 64, 1, 49, 64), "null"), ((p, p, dp, dp, 7, 1, 49, 64), "workspace"), ((p, p, dp, dp, 15, 1, 65, 64), "workspace"),
                       ((p, p, dp, dp, 1 << 40, 4096, 4096, 256), "2^31"), ((p, p, dp, dp, 64, 0, 49, 64), "B")):
        assert dist(*args) == -1 and word in err(), (args[4:], word, err())
    t = torch.zeros(1, 3, 32, 32)
    net = LP.LpipsNet(*LP.LpipsNet.synthetic_tensors(), "cpu", "synthetic")
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        net(t, t)                                                                           # CPU tensors: there is no CPU fallback
    with pytest.raises(_lib.SelftokHipError, match="H, W >= 31"):
        net(t[..., :30, :], t[..., :30, :])
    with pytest.raises(_lib.SelftokHipError, match="one shape"):
        net(t, t[..., :31])
    with pytest.raises(_lib.SelftokHipError, match="one shape"):
        ops.lpips_input(t, torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="lpips"):
        E.evaluate(_NoPipe(), lambda lo, hi: t, 1, metrics=("psnr", "lpips"))              # "lpips" without lpips=: the weights are not shipped
    with pytest.raises(ValueError):
        E.evaluate(_NoPipe(), lambda lo, hi: t, 1, metrics=("lpips",))
