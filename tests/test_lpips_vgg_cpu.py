"""not gpu: the LPIPS-VGG16 arithmetic of record (tests/lpips_vgg_cases.py) pinned on the host -- the emulation against an independent im2col +
einsum formulation, its exact properties (d(x, x) = 0, symmetry), tap_sizes against the emulation's shapes, the d >= 0.05 condition of the
end-to-end gate on the synthetic weights, the planted mistakes the case table must be able to see, the new pool entry against the ctypes table and
its scratch budget, the weight-file loader, the activation plan, and the host-side refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lpips_cases as L
import lpips_vgg_cases as V
from selftoktokenizer_amd import _lib, evaluate as E, lpips as LP, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_lpips_maxpool2s2_f32"}


def test_case_table_and_definition():
    assert {(c.H, c.W) for c in V.CASES} == {(31, 31), (32, 33), (47, 34), (64, 64), (96, 96)} and sum(c.H == 96 for c in V.CASES) == 1
    assert {c.B for c in V.CASES if c.H < 96} == {1, 3} and {c.content for c in V.CASES} == set(L.CONTENTS) and len({c.name for c in V.CASES}) == len(V.CASES)
    assert len({(c.recon_bf16, c.orig_bf16, c.signed, c.quantize) for c in V.CASES}) == 16
    d = LP.LPIPS_VGG_DEFINITION
    assert (d["net"], d["version"], d["eps"], d["min_side"], d["pools"]) == ("vgg", "0.1", 1e-10, 31, [4, 9, 16, 23]) and LP.VGG_ARCH_MIN_SIDE == 16
    assert d["shift"] == LP.LPIPS_DEFINITION["shift"] and d["scale"] == LP.LPIPS_DEFINITION["scale"] and d["normalize"] == LP.LPIPS_DEFINITION["normalize"]
    assert [int(l["key"].split(".")[1]) for l in d["layers"]] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [l["name"] for l in d["layers"] if l["tap"]] == ["conv1_2", "conv2_2", "conv3_3", "conv4_3", "conv5_3"]
    assert [l["channels"][1] for l in d["layers"] if l["tap"]] == [64, 128, 256, 512, 512]
    assert [l["channels"] for l in d["layers"]] == [[3, 64], [64, 64], [64, 128], [128, 128], [128, 256], [256, 256], [256, 256], [256, 512], [512, 512], [512, 512],
                                                    [512, 512], [512, 512], [512, 512]]
    assert LP.DEFINITIONS["alex"] is LP.LPIPS_DEFINITION and LP.LPIPS_DEFINITION["net"] == "alex"
    with pytest.raises(ValueError, match="squeeze"):
        LP.tap_sizes(64, 64, "squeeze")


def test_tap_sizes_are_the_emulations_shapes():
    assert LP.tap_sizes(31, 31, "vgg") == [(31, 31), (15, 15), (7, 7), (3, 3), (1, 1)] and LP.tap_sizes(16, 16, "vgg")[-1] == (1, 1)
    assert LP.tap_sizes(256, 256, "vgg") == [(256, 256), (128, 128), (64, 64), (32, 32), (16, 16)]
    assert LP.tap_sizes(31, 31) == LP.tap_sizes(31, 31, "alex") == [(7, 7), (3, 3), (1, 1), (1, 1), (1, 1)]
    for H, W in ((31, 31), (32, 33), (47, 34), (33, 62), (64, 64)):
        taps = V.features(np.zeros((1, 3, H, W), np.float32))
        assert [t.shape[2:] for t in taps] == LP.tap_sizes(H, W, "vgg") and [t.shape[1] for t in taps] == [64, 128, 256, 512, 512], (H, W)


@pytest.mark.parametrize("case", V.CASES, ids=lambda c: c.name)
def test_emulation_equals_the_independent_formulation(case):
    """torch conv2d / max_pool2d in fp64 == explicit im2col + einsum in numpy fp64, <= 1e-12 relative (1e-25: the second formulation's two halves of an
    identical pair need not be the same bits, the emulation of record's are)"""
    recon, orig = V.make(case)
    v, v2 = V.case_value(case.name), V.emulate_im2col(recon, orig, case.recon_bf16, case.signed, case.quantize)
    assert v.shape == (case.B,) and np.isfinite(v).all()
    assert (np.abs(v2 - v) <= 1e-12 * v + 1e-25).all(), (v, v2)


def test_identical_pairs_are_zero_and_the_distance_is_symmetric():
    seen = 0
    for case in V.CASES:
        if case.content == "identical":
            assert (V.case_value(case.name) == 0.0).all(), case.name
            seen += 1
    assert seen >= 8
    seen = 0
    for case in [c for c in V.CASES if c.content in ("noise", "recon_noise") and not c.quantize]:
        recon, orig = V.make(case)
        x0, x1 = L.to_signed(recon, orig, case.recon_bf16, case.signed, False)
        fwd = V.distance(V.features(L.scaling_layer(np.concatenate([x0, x1]))))
        rev = V.distance(V.features(L.scaling_layer(np.concatenate([x1, x0]))))
        assert np.array_equal(fwd.view(np.uint64), rev.view(np.uint64)), case.name
        assert np.array_equal(fwd.view(np.uint64), V.case_value(case.name).view(np.uint64))
        seen += 1
    assert seen >= 6


def test_gated_cases_are_far_from_cancellation_on_the_synthetic_weights():
    """a condition on the reference alone: every pair of every noise and smooth case has d >= 0.05 under the hash-generated VGG16 weights"""
    assert len(V.GATED) >= 16 and any(c.H == 96 for c in V.GATED)
    for case in V.GATED:
        assert V.case_value(case.name).min() >= 0.05, (case.name, V.case_value(case.name))
    pairs = {content: sum(int(V.gated_pairs(c.name).sum()) for c in V.CASES if c.content == content) for content in L.CONTENTS}
    total = {content: sum(c.B for c in V.CASES if c.content == content) for content in L.CONTENTS}
    rel, rel_const = V.fp32_relative_error(), V.fp32_relative_error(const=True)
    assert rel < rel_const < 1e-5 and V.relative_gate(V.GATED[0].name) == 4 * rel and V.relative_gate(next(c.name for c in V.CASES if c.content == "const")) == 4 * rel_const
    print(f"\ntorch-CPU fp32 features on the const pairs at d >= {V.D_GATED}: {rel_const:.3e}")
    print(f"\npairs with d >= {V.D_GATED} of all pairs, by content: " + ", ".join(f"{k} {pairs[k]} / {total[k]}" for k in L.CONTENTS)
          + f"; torch-CPU fp32 features against the fp64 emulation, largest relative error over the {len(V.GATED)} noise and smooth cases: {rel:.3e}")
    assert pairs["noise"] == total["noise"] and pairs["smooth"] == total["smooth"] and pairs["identical"] == 0
    assert 0 < rel < 1e-5


def _pooled_sides(case):
    return [s for hw in LP.tap_sizes(case.H, case.W, "vgg")[:4] for s in hw]


def _visible(mut, case):
    if case.content == "identical":
        return False
    if mut in ("ceil_pool", "alex_pool") and case.content == "const":
        return False                            # the maximum of equal values does not say which window it was taken over: only the padded border differs
    if mut == "ceil_pool":                      # only where a pooled side is odd: floor drops its last row / column, ceil keeps it
        return any(s % 2 for s in _pooled_sides(case))
    return True


@pytest.mark.parametrize("mut", V.MUTS)
def test_every_case_that_can_see_a_planted_mistake_sees_it(mut):
    """each mistake moves every pair of every case that can see it by >= 1000 x that case's GPU gate (4 x torch fp32's relative error x d).  A const pair below
    d = 0.05 has no GPU gate (lpips_vgg_cases.relative_gate is the figure of the const pairs AT d >= 0.05), so nothing is asked of it; the pairs of the other
    contents are all held to the noise-and-smooth figure, gated or not, as in tests/test_lpips_cpu.py"""
    seen = 0
    for case in [c for c in V.CASES if _visible(mut, c)]:
        v = V.case_value(case.name)
        moved = np.abs(V.case_value(case.name, torch.float64, mut) - v)
        m = V.gated_pairs(case.name) if case.content == "const" else np.ones(case.B, bool)
        assert m.any() and (moved[m] >= 1000 * V.relative_gate(case.name) * v[m]).all(), f"{case.name}: {mut} moves d by only {moved[m].min():.2e} ({v})"
        seen += 1
    assert seen >= {"ceil_pool": 18, "alex_pool": 25}.get(mut, 30), seen


def test_ext_header_declares_the_pool_entry():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and names == set(_lib.EXT_SIGNATURES)
    m = re.search(r"(\w+)\s+selftok_lpips_maxpool2s2_f32\s*\(([^)]*)\)\s*;", hdr)
    args = [a.strip() for a in m.group(2).split(",")]
    C = ctypes
    ctype_of = {"int": C.c_int, "hipStream_t": C.c_void_p}
    assert _lib.EXT_SIGNATURES["selftok_lpips_maxpool2s2_f32"] == (C.c_int, [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]) and m.group(1) == "int"
    assert _lib.EXT_SIGNATURES["selftok_lpips_maxpool2s2_f32"] == _lib.EXT_SIGNATURES["selftok_lpips_maxpool3s2_f32"]
    assert hasattr(C.CDLL(_lib.LIB_PATH), "selftok_lpips_maxpool2s2_f32")


def test_the_pool_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "lpips_vgg.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    assert len(kernels) == 1 and "lpips_pool2_kernel" in kernels[0] and scratch == [0] and lds == [0], (kernels, scratch, lds)
    src = open(os.path.join(G.CSRC, "lpips_vgg.hip")).read()
    assert "asm" not in src and "atomic" not in src


def _packed_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a.packed + a.bias + a.lin, b.packed + b.bias + b.lin))


def test_from_files_round_trips_the_vgg_key_layout_and_refuses(tmp_path):
    sd, lin = LP.LpipsNet.synthetic_tensors("vgg")
    assert sorted(sd, key=lambda k: (int(k.split(".")[1]), k)) == [f"features.{i}.{leaf}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28) for leaf in ("bias", "weight")]
    mem = LP.LpipsNet(sd, lin, "cpu", "synthetic", net="vgg")
    assert mem.net == "vgg" and mem.definition is LP.LPIPS_VGG_DEFINITION and mem.source == "synthetic" and all((w >= 0).all() for w in mem.lin)
    assert [tuple(p.shape) for p in mem.packed][:3] == [(32, 64), (576, 64), (576, 128)] and tuple(mem.packed[-1].shape) == (4608, 512) and len(mem.packed) == 13
    assert [w.numel() for w in mem.lin] == [64, 128, 256, 512, 512]
    alex = LP.LpipsNet(*LP.LpipsNet.synthetic_tensors(), "cpu", "synthetic")
    assert alex.net == "alex" and alex.definition is LP.LPIPS_DEFINITION and len(alex.packed) == 5
    full = dict(sd, **{"classifier.0.weight": torch.zeros(3, 3), "classifier.6.bias": torch.zeros(1000)})      # the classifier's keys are ignored
    lins = {f"lin{i}.model.1.weight": w for i, w in enumerate(lin)}
    bp, lp = str(tmp_path / "vgg16-397923af.pth"), str(tmp_path / "vgg.pth")
    torch.save(full, bp); torch.save(lins, lp)
    net = LP.LpipsNet.from_files(bp, lp, "cpu", net="vgg")
    assert _packed_equal(net, mem) and net.source == ["vgg16-397923af.pth", "vgg.pth"] and net.net == "vgg"
    with pytest.raises(ValueError, match="lin1"):                                           # vgg.pth is no alex.pth (128 against 192 weights) ...
        LP.LpipsNet.from_files(bp, lp, "cpu")
    with pytest.raises(ValueError, match="features.0.weight"):                              # ... and a VGG16 state dict is no AlexNet one (3 x 3 against 11 x 11)
        LP.LpipsNet(full, LP.LpipsNet.synthetic_tensors()[1], "cpu", "files")
    with pytest.raises(ValueError, match="squeeze"):
        LP.LpipsNet.from_files(bp, lp, "cpu", net="squeeze")
    torch.save({k: v for k, v in full.items() if k != "features.26.bias"}, bp)
    with pytest.raises(KeyError, match="features.26.bias"):
        LP.LpipsNet.from_files(bp, lp, "cpu", net="vgg")
    torch.save(dict(full, **{"features.5.weight": torch.zeros(128, 64, 5, 5)}), bp)
    with pytest.raises(ValueError, match="features.5.weight"):
        LP.LpipsNet.from_files(bp, lp, "cpu", net="vgg")
    torch.save(full, bp)
    torch.save({k: v for k, v in lins.items() if k != "lin3.model.1.weight"}, lp)
    with pytest.raises(KeyError, match="lin3"):
        LP.LpipsNet.from_files(bp, lp, "cpu", net="vgg")
    torch.save(dict(lins, **{"lin1.model.1.weight": torch.zeros(1, 192, 1, 1)}), lp)          # AlexNet's second weighting
    with pytest.raises(ValueError, match="lin1"):
        LP.LpipsNet.from_files(bp, lp, "cpu", net="vgg")


def test_the_vgg_plan_keeps_five_taps_and_two_ping_pong_buffers():
    """every step reads a buffer that holds what it needs, writes another one, never overwrites a tap, and fits its destination"""
    net = LP.LpipsNet(*LP.LpipsNet.synthetic_tensors("vgg"), "cpu", "synthetic", net="vgg")
    for H, W in ((31, 31), (47, 34), (256, 256)):
        shapes, steps = LP._vgg_steps(H, W)
        taps = LP.tap_sizes(H, W, "vgg")
        assert len(shapes) == 8 and shapes[0] == (H, W, 3) and shapes[1:6] == [(h, w, c) for (h, w), c in zip(taps, (64, 128, 256, 512, 512))]
        assert [k for k, *_ in steps].count("conv") == 13 and [k for k, *_ in steps].count("pool") == 4
        holds = {0: (H, W, 3)}
        for kind, layer, src, dst, shape in steps:
            assert src in holds and src != dst and (dst >= 6 or dst not in holds)
            assert shape[0] * shape[1] * shape[2] <= shapes[dst][0] * shapes[dst][1] * shapes[dst][2]
            if kind == "conv":
                assert holds[src][2] == LP.VGG_LAYERS[layer][3] and shape == holds[src][:2] + (LP.VGG_LAYERS[layer][2],)
            else:
                assert 1 <= src <= 5 and shape == (holds[src][0] // 2, holds[src][1] // 2, holds[src][2])
            holds[dst] = shape
        assert [holds[i] for i in range(1, 6)] == shapes[1:6]
        assert net._plan(2, H, W) == [(2,) + s for s in shapes]
    kept = sum(h * w * c for h, w, c in LP._vgg_steps(256, 256)[0])
    every = 256 * 256 * 3 + sum(shape[0] * shape[1] * shape[2] for *_, shape in LP._vgg_steps(256, 256)[1])
    assert kept < 0.75 * every and every > 19e6                                            # about 20 M activations per image if every intermediate were kept


class _NoPipe:
    device = torch.device("cpu")


def test_host_side_refusals_without_a_gpu():
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.zeros(4096, np.float32)
    p = x.ctypes.data
    assert lib.selftok_lpips_maxpool2s2_f32(None, p, 1, 4, 4, 64, None) == -1 and "null" in err()
    assert lib.selftok_lpips_maxpool2s2_f32(p, None, 1, 4, 4, 64, None) == -1 and "null" in err()
    assert lib.selftok_lpips_maxpool2s2_f32(p, p, 1, 1, 4, 64, None) == -1 and "H, W >= 2" in err()
    assert lib.selftok_lpips_maxpool2s2_f32(p, p, 1, 4, 1, 64, None) == -1 and "H, W >= 2" in err()
    assert lib.selftok_lpips_maxpool2s2_f32(p, p, 0, 4, 4, 64, None) == -1 and "N, C >= 1" in err()
    assert lib.selftok_lpips_maxpool2s2_f32(p, p, 65536, 256, 256, 64, None) == -1 and "2^31" in err()
    t = torch.zeros(1, 3, 32, 32)
    net = LP.LpipsNet(*LP.LpipsNet.synthetic_tensors("vgg"), "cpu", "synthetic", net="vgg")
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        net(t, t)
    with pytest.raises(_lib.SelftokHipError, match="H, W >= 31"):                           # 16 would do for the architecture; the shared input stage keeps 31
        net(t[..., :30, :], t[..., :30, :])
    with pytest.raises(_lib.SelftokHipError, match="one shape"):
        net(t, t[..., :31])
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.lpips_maxpool2s2(torch.zeros(1, 4, 4, 8))
    with pytest.raises(ValueError, match="squeeze"):
        LP.LpipsNet.synthetic("cpu", net="squeeze")
    alex = LP.LpipsNet(*LP.LpipsNet.synthetic_tensors(), "cpu", "synthetic")
    load = lambda lo, hi: t
    for nets in ([alex, net], (net,), [net, alex]):                                        # accepted: the call gets as far as the stand-in pipe's missing `encoding`
        with pytest.raises(AttributeError, match="encoding"):
            E.evaluate(_NoPipe(), load, 1, metrics=("psnr", "ssim", "ssim_skimage", "lpips"), lpips=nets)
    with pytest.raises(ValueError, match="different backbones"):
        E.evaluate(_NoPipe(), load, 1, metrics=("lpips",), lpips=[alex, alex])
    with pytest.raises(ValueError, match="sequence"):
        E.evaluate(_NoPipe(), load, 1, metrics=("lpips",), lpips=[])
    with pytest.raises(ValueError, match="sequence"):
        E.evaluate(_NoPipe(), load, 1, metrics=("lpips",), lpips=[alex, "vgg"])
    with pytest.raises(ValueError, match="lpips"):
        E.evaluate(_NoPipe(), load, 1, metrics=("psnr", "lpips_vgg"), lpips=[alex, net])
