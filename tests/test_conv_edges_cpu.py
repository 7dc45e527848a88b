"""not gpu: the tables and references of tests/conv_edge_cases.py hold what they claim (tile edges, parities, tails, pixel-range counts,
exact sums, enough roundings and ties), the CPU twin (oracle/libselftok_cpu.so) gives the reference's bits on every convolution case and is
inside the GroupNorm gate on every case, the packed image is the documented index formula, both libraries' new refusals are there, every
planted mistake is seen by exactly the cases `applies` names, and csrc/conv.hip / csrc/vae.hip compile for gfx950 without scratch."""
import os
import re
import subprocess

import numpy as np
import pytest

import abi_cases as A
import conv_edge_cases as CE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def twin():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return A.bind(os.path.join(ROOT, "oracle", "libselftok_cpu.so"))


def by_launch(shape, cases=CE.CONV_EXACT):
    return [c for c in cases if c.launch == shape]


# ---- the table holds what it claims ---------------------------------------------------------------------------------------------------
def test_conv_table_reaches_every_edge():
    assert len({c.name for c in CE.CONV_CASES}) == len(CE.CONV_CASES)
    for shape in CE.LAUNCH_SHAPES:
        cs, th = by_launch(shape), CE.TILE_H[shape]
        assert len(cs) >= 3 and len(by_launch(shape, CE.CONV_GAUSS)) >= 1, shape
        assert any(c.rounding for c in cs), shape
        wo, ho = {c.Wo for c in cs}, {c.Ho for c in cs}
        # the tile edge and one beyond it in both axes; a single pixel
        assert 32 in wo and 33 in wo | {w - 32 for w in wo} and any(w % 32 == 31 or w == 1 for w in wo), (shape, wo)
        assert any(h % th == 0 for h in ho) and any(h % th == 1 for h in ho), (shape, ho)
        assert any(c.B > 1 for c in cs), shape
        # Cin tails (a last 32-block of 8, 16 or 24 channels) and whole blocks; one and several blocks: both weight buffer parities
        assert any(c.Cin % 32 for c in cs) and any(c.Cin % 32 == 0 for c in by_launch(shape, CE.CONV_CASES)), shape
        assert any(c.ncb == 1 for c in cs) and any(c.ncb >= 2 for c in cs), shape
    rows, s2, n3, p1 = by_launch(CE.ROWS), by_launch(CE.S2), by_launch(CE.N3), by_launch(CE.P1)
    assert {31, 32, 33} <= {c.Wo for c in rows} | {c.Wo - 32 for c in rows} and {3, 4, 5} <= {c.Ho for c in rows}
    assert {7, 8, 9} <= {c.Ho for c in n3} and {31, 32, 33} <= {c.Wo for c in n3}
    assert any(c.ncb % 2 == 0 and c.ncb >= 2 for c in rows) and any(c.ncb % 2 == 1 and c.ncb >= 3 for c in rows)         # halo / weight group parities
    assert {1, 2, 3} <= {c.ncb for c in p1}
    # stride 2: odd sizes lose the last row / column, even ones read the padded one; Cin 24 and 72; B = 3
    assert {(c.H, c.W) for c in s2} == {(2, 2), (5, 67), (8, 64), (9, 65)} and {c.Cin for c in s2} == {24, 72} and any(c.B == 3 for c in s2)
    # channel-block tails: a second block 4 wide, zero channels inside a block, a pitch wider than the store, 3 channels stored as 4
    assert any(c.cs % c.bn == 4 and c.channel_blocks == 2 for c in rows) and any(c.cs % c.bn == 4 and c.channel_blocks == 2 for c in n3)
    assert any(c.cs - c.Cout >= 28 and c.ld > c.cs for c in rows) and any(c.Cout == 3 and c.cs == 4 for c in n3)
    assert any(c.channel_blocks == 4 and c.ncb == 16 for c in rows) and any(c.cin_s == 8 and c.Cin == 3 for c in rows)
    assert any(not c.bias for c in rows) and any(c.resid for c in rows)
    up = [c for c in CE.CONV_EXACT if c.up]
    assert any(c.H == c.W == 1 for c in up) and any(c.Wo == 34 for c in up) and any(c.Wo == c.Ho == 32 for c in up) and any(c.resid for c in up)
    # no case reaches past the packed image: the stored channels open no block the image does not hold (include/selftok_hip.h)
    for c in CE.CONV_CASES:
        assert c.channel_blocks == (c.Cout + c.bn - 1) // c.bn and c.cs % 4 == 0 and c.ld % 4 == 0 and c.cs <= c.ld, c.name
        assert c.cin_s % 8 == 0 and (c.cin_s + 31) // 32 == c.ncb and c.Ho > 0 and c.Wo > 0, c.name
        assert c.Cin <= 512 and c.B * c.Ho * c.Wo * c.cs <= 1 << 20, c.name


def test_groupnorm_table_reaches_every_route():
    assert len({c.name for c in CE.GN_CASES}) == len(CE.GN_CASES)
    nhwc = [c for c in CE.GN_CASES if c.layout == "nhwc"]
    nchw = [c for c in CE.GN_CASES if c.layout == "nchw"]
    assert {1, 255, 511, 512, 513, 769, 1600, 8192, 8193} <= {c.HW for c in nhwc}
    assert {1, 2, 3, 4, 6, 32} <= {c.nblk for c in nhwc}                                      # pixel ranges per sample
    per = lambda c: -(-c.HW // c.nblk)
    assert any(c.HW % c.nblk == 0 and c.nblk > 1 for c in nhwc) and any(per(c) * c.nblk > c.HW for c in nhwc)      # even and ragged ranges
    assert any(c.HW == 769 and (per(c), c.HW - 2 * per(c)) == (257, 255) for c in nhwc) and any(c.HW == 1600 and per(c) == 267 for c in nhwc)
    assert {(8, 1), (32, 8), (128, 32), (512, 32), (1024, 32), (2048, 32), (256, 64)} <= {(c.C, c.groups) for c in nhwc}
    for c in nhwc:                                                                           # the entry's own argument rules
        assert c.C % c.groups == 0 and (c.C // c.groups) % 4 == 0 and c.C % 8 == 0 and 256 % (c.C // 8) == 0 and c.groups <= 64, c.name
    big = [c for c in nhwc if c.B == 64]
    assert big and all((c.HW * (c.C // 8) + 255) // 256 > (256 * 16 + c.B - 1) // c.B == 64 for c in big)      # more chunk blocks than the workgroup cap
    for lay in (nhwc, nchw):
        assert {"const", "offset"} <= {c.content for c in lay} and any(c.B == 3 for c in lay)
    assert any(c.HW == 8 and c.C == c.groups for c in nchw) and {2, 16} <= {c.C // c.groups for c in nchw if c.HW == 64}
    assert {520, 4104} <= {c.HW for c in nchw} and all(c.HW % 8 == 0 for c in nchw)
    assert all((c.C // c.groups * c.HW // 8) % 512 for c in nchw if c.HW in (520, 4104))
    assert max(c.n for c in CE.GN_CASES) <= 10 << 20


@pytest.mark.parametrize("case", CE.CONV_EXACT, ids=lambda c: c.name)
def test_exact_cases_are_exact_and_round(case):
    bound = CE.conv_abs_bound(case)
    assert bound < 2 ** 24, bound
    d = CE.conv_inputs(case)
    assert np.abs(d["x"]).max() <= 8 and np.abs(d["w"]).max() <= 8 and (d["bias"] is None or np.abs(d["bias"]).max() <= 64)
    assert d["res"] is None or (np.abs(d["res"]).max() <= 512 and np.array_equal(d["res"], np.rint(d["res"])))
    share, ties = CE.rounding_stats(case)
    print(f"{case.name}: bound {bound:.0f}, {100 * share:.1f} % of the sums are not bf16 values, {ties} ties")
    if case.rounding:
        assert share >= 0.20 and ties >= 16, (share, ties)


def test_rounding_helpers():
    f = np.array([256.0, 257.0, 258.0, 259.0, -257.0, -259.0, 1.0, 513.0, 514.0, 515.0], np.float32)
    val = lambda how: CE.bf16_bits_to_f32(CE.f32_to_bf16_bits(f, how)).tolist()
    assert val(CE.RNE) == [256, 256, 258, 260, -256, -260, 1, 512, 512, 516]
    assert val(CE.TRUNC) == [256, 256, 258, 258, -256, -258, 1, 512, 512, 512]
    assert val(CE.TIES_AWAY) == [256, 258, 258, 260, -258, -260, 1, 512, 516, 516]
    assert np.array_equal(CE.f64_to_bf16_bits(f.astype(np.float64)), CE.f32_to_bf16_bits(f))
    x = np.random.default_rng(1).standard_normal(4096) * np.exp(np.random.default_rng(2).uniform(-20, 20, 4096))
    assert np.array_equal(CE.f64_to_bf16_bits(x.astype(np.float32).astype(np.float64)), A.to_bf16(x.astype(np.float32)))       # torch's conversion
    # one rounding, not two: 1 + 2^-8 + 2^-30 is above the tie, its fp32 rounding is the tie
    assert CE.f64_to_bf16_bits(np.array([1 + 2.0 ** -8 + 2.0 ** -30]))[0] == 0x3F81 and CE.f32_to_bf16_bits(np.float32(1 + 2.0 ** -8 + 2.0 ** -30)) == 0x3F80
    o = CE.bf16_ord(np.array([0x0000, 0x8000, 0x0001, 0x8001, 0x3F80, 0x3F81], np.uint16))
    assert o.tolist() == [0, 0, 1, -1, 0x3F80, 0x3F81]


# ---- the CPU twin against the references ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CE.CONV_CASES, ids=lambda c: c.name)
def test_twin_convolution(twin, case):
    rc, out, _ = CE.conv_call(twin, case, CE.Host)
    assert rc == 0, twin.selftok_last_error()
    got, ref = out.numpy(), CE.conv_expected(case)
    assert (got[..., case.cs:] == CE.SENTINEL).all()                           # [Cstore, ldo) left alone
    got = got[..., :case.cs]
    if case.gauss:
        ok, share = CE.gauss_gate(got, ref)
        assert ok, share
    else:
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:4]
    tail = got[..., case.Cout:]                                                # [Cout, Cstore): zero, or bf16(res)
    assert np.array_equal(tail, CE.f32_to_bf16_bits(CE.conv_inputs(case)["res"][..., case.Cout:case.cs]) if case.resid else np.zeros_like(tail))


_twin_gn = {}


def twin_gn(twin, case, silu):
    if (case.name, silu) not in _twin_gn:
        rc, out = CE.gn_call(twin, case, CE.Host, silu)
        assert rc == 0, twin.selftok_last_error()
        _twin_gn[case.name, silu] = out.numpy()
    return _twin_gn[case.name, silu]


@pytest.mark.parametrize("case", CE.GN_CASES, ids=lambda c: c.name)
def test_twin_groupnorm_counts(twin, case):
    """the number of elements that differ from the reference is inside the cap; a constant group gives bf16(bias) [SiLU] exactly"""
    for silu in (0, 1):
        got = twin_gn(twin, case, silu)
        _, diff, cap = CE.gn_gate(case, got, silu)
        print(f"{case.name} silu {silu}: twin {diff / case.n:.2e}, torch bf16 {CE.gn_torch_counts(case)[silu] / case.n:.2e} of {case.n}")
        assert diff <= cap, (silu, diff, cap)
        if case.content == "const":
            cpg, g = case.C // case.groups, CE.CONST_GROUP % case.groups
            o = got if case.layout == "nhwc" else got.transpose(0, 2, 1)
            assert (o[:, :, g * cpg:(g + 1) * cpg] == CE.gn_const_expected(case, silu)).all()


@pytest.mark.parametrize("case", CE.GN_CASES, ids=lambda c: c.name)
def test_twin_groupnorm_bracket(twin, case):
    """every element is the reference's value or an adjacent bf16 value (with SiLU: within one output ulp of SiLU of those three).

    This is what rules out an fp32 evaluation of (x - mean) * rstd * w + b: where the product and the bias cancel to ~1e-7 (with the mean at 300:
    to below 1e-3) its rounding is several bf16 ulps of the result.  torch-CPU's own bf16 F.group_norm leaves the bracket there (1, 1, 5 and 533
    elements of nhwc_hw513_c256_g64, nhwc_b3_hw600_c256, nhwc_b64_hw1100_c128 and nhwc_offset300_hw769_c128), and so did the channels-last
    entry (1, 1, 7, 533) until it evaluated the normalisation in fp64 with one rounding."""
    what = {silu: CE.gn_outside(case, twin_gn(twin, case, silu), silu) for silu in (0, 1)}
    print(f"{case.name}: {what}")
    assert all(CE.gn_gate(case, twin_gn(twin, case, silu), silu)[0] for silu in (0, 1)), what


def test_groupnorm_gate_rejects_wrong_results():
    """the gate is not vacuous: statistics without the last pixel, a missing SiLU, a biased mean and a 2-ulp error all fail it"""
    case = CE.GN_BY_NAME["nhwc_hw513_c32_g8"]
    g_ref, y_ref = CE.gn_reference(case)
    for silu, ref in ((0, g_ref), (1, y_ref)):
        inside, diff, cap = CE.gn_gate(case, ref, silu)
        assert inside and diff == 0
        o = CE.bf16_ord(ref)
        two = np.where(o + 2 < 0, (-(o + 2)) | 0x8000, o + 2).astype(np.uint16)
        assert not CE.gn_gate(case, two, silu)[0] or silu                      # two ulps: outside the plain bracket
        bumped = ref.copy(); bumped[:, ::3] = np.where(o + 1 < 0, (-(o + 1)) | 0x8000, o + 1).astype(np.uint16)[:, ::3]
        inside, diff, cap = CE.gn_gate(case, bumped, silu)
        assert diff > cap                                                      # a third of the elements one ulp off: inside every bracket, over the cap
    assert not CE.gn_gate(case, g_ref, 1)[0] and not CE.gn_gate(case, y_ref, 0)[0]      # SiLU missing / applied where none was asked
    xb, wb, bb = CE.gn_inputs(case)
    x = CE.bf16_bits_to_f32(xb).astype(np.float64).reshape(case.B, case.HW, case.groups, -1)
    m = x[:, :-1].mean((1, 3), keepdims=True)                                  # statistics that miss the last pixel
    v = ((x[:, :-1] - m) ** 2).mean((1, 3), keepdims=True)
    y = ((x - m) / np.sqrt(v + CE.EPS)).reshape(case.B, case.HW, case.C) * CE.bf16_bits_to_f32(wb) + CE.bf16_bits_to_f32(bb)
    inside, diff, cap = CE.gn_gate(case, CE.f64_to_bf16_bits(y), 0)
    assert diff > cap


# ---- the packed image ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", CE.PACK_CASES, ids=str)
def test_twin_pack_is_the_index_formula(twin, shape):
    Cout, Cin, ks, bn = shape
    w = np.random.default_rng(CE.seed_of(f"pack{shape}")).integers(1, 0x7F80, (Cout, Cin, ks, ks)).astype(np.uint16)      # no zero: padding is told from data
    n = twin.selftok_conv2d_packed_bytes(Cout, Cin, ks, bn)
    assert n == (Cout + bn - 1) // bn * ((Cin + 31) // 32) * ks * ks * bn * 32 * 2
    packed = np.full(n // 2 + 64, CE.NAN_BF16, np.uint16)
    assert twin.selftok_conv2d_pack_weight_bf16(w.ctypes.data, packed.ctypes.data, Cout, Cin, ks, bn, None) == 0
    want = CE.pack_expected(w, Cout, Cin, ks, bn)
    assert np.array_equal(packed[:n // 2], want) and (packed[n // 2:] == CE.NAN_BF16).all()
    assert int((want != 0).sum()) == w.size and int((packed[:n // 2] == 0).sum()) == n // 2 - w.size                    # the padding is all zero


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", CE.NEW_REFUSALS + CE.OLD_REFUSALS, ids=lambda r: r[0])
def test_twin_refusals(twin, r):
    rc, out = CE.refused_call(twin, CE.Host, r)
    assert rc == CE.EINVAL and (out == CE.SENTINEL).all()
    msg = twin.selftok_last_error()
    assert msg.startswith(b"conv2d_nhwc_bf16:")
    assert any(m in msg for m in CE.NEW_MESSAGES) == (r in CE.NEW_REFUSALS), msg


def test_both_libraries_state_the_new_refusals_alike():
    """one message and one code in csrc/conv.hip and oracle/selftok_cpu.c, before any launch; the header states them and the two preconditions"""
    hip = open(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "conv.hip")).read()
    cpu = open(os.path.join(ROOT, "oracle", "selftok_cpu.c")).read()
    hdr = re.sub(r"\s*\*?\s+", " ", open(os.path.join(ROOT, "include", "selftok_hip.h")).read())
    for m in CE.NEW_MESSAGES:
        full = re.findall(r'"(conv2d_nhwc_bf16: ' + re.escape(m.decode()) + r'[^"]*)"', hip)
        assert len(full) == 1 and cpu.count('"' + full[0] + '"') == 1, m
    entry = hip[hip.index("int selftok_conv2d_nhwc_bf16("):]
    assert entry.index("empty stride-2 output") < entry.index("if (B == 0) return SELFTOK_OK") < entry.index("hipLaunchKernelGGL")
    for words in ("ceil(Cstore / bn) == ceil(Cout / bn)", "empty", "SELFTOK_EINVAL", "(Cin + 31) / 32", "finite"):
        assert words in hdr[hdr.index("SD3-VAE convolutions and GroupNorm, channels-last"):hdr.index("size_t selftok_conv2d_packed_bytes")], words


def test_host_wrapper_asserts_cstore():
    src = open(os.path.join(ROOT, "selftoktokenizer_amd", "ops.py")).read()
    body = src[src.index("def conv2d_nhwc("):src.index("def groupnorm_silu_nhwc(")]
    assert "(cs + pc.bn - 1) // pc.bn == (pc.cout + pc.bn - 1) // pc.bn" in body and body.index("(cs + pc.bn - 1) // pc.bn") < body.index("torch.empty(")


# ---- planted mistakes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mut", CE.CONV_MISTAKES)
def test_planted_mistake_is_seen_by_exactly_its_cases(mut):
    """each mistake, applied to the reference, changes every case `applies` names and no case it rules out (None: the drawn data decides)"""
    seen = 0
    for c in CE.CONV_EXACT:
        touched = CE.applies(c, mut)
        d = int((CE.conv_expected(c, mut) != CE.conv_expected(c)).sum())
        if touched is not None:
            assert (d >= 1) == touched, f"{c.name}: {mut} changes {d} elements, applies() says {touched}"
        seen += bool(touched)
    assert seen >= 2, (mut, seen)
    for shape in CE.LAUNCH_SHAPES:                  # every launch shape has a case that sees each mistake its geometry can make
        if mut in (CE.MUT_TRUNC, CE.MUT_TIES_AWAY, CE.MUT_BIAS_AFTER, CE.MUT_CIN_TAIL, CE.MUT_PARTIAL_TILE):
            assert any(CE.applies(c, mut) for c in by_launch(shape)), (mut, shape)


# ---- the kernels still build ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,least", [("conv", 9), ("vae", 4)])
def test_unit_compiles_for_gfx950_without_scratch(tmp_path, unit, least):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == unit + ".o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) >= least and len(scratch) == len(kernels), (kernels, scratch)
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
