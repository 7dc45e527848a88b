"""-m gpu: the bf16 convolution of csrc/conv.hip in its five launch shapes, the weight packer and GroupNorm [+ SiLU] in both layouts on
the cases of tests/conv_edge_cases.py.  Exact convolution cases must equal the float64 reference in every bit, the gaussian ones and
GroupNorm are held to the gates stated there.  Every device operand is a view inside its own allocation with bf16-NaN guard bands of
max(64 KiB, one packed weight block) on both sides: a read past an operand shows as a NaN in the output, a write as a damaged band.
No call here passes a Cstore that opens a channel block the packed image does not hold; that shape appears only as a refusal, which
launches nothing.  tests/test_conv_edges_cpu.py checks the tables, the references and the CPU twin without a GPU."""
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_cases as A
import conv_edge_cases as CE
from selftoktokenizer_amd import _lib, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAND = 64 << 10


@pytest.fixture(scope="module")
def libs():
    path = os.path.join(ROOT, "oracle", "libselftok_cpu.so")
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return _lib.load(), A.bind(path)


class Guarded:
    """a device operand inside its own allocation: [band of 0x7FC0][the array][band of 0x7FC0]"""

    def __init__(self, a, name, band):
        a = np.ascontiguousarray(a)
        raw = a.reshape(-1).view(np.uint8)
        assert raw.size % 2 == 0 and band % 256 == 0
        self.name, self.shape, self.dtype, self.n, self.band = name, a.shape, a.dtype, raw.size, band
        self.buf = torch.full(((2 * band + (raw.size + 15) // 16 * 16) // 2,), CE.NAN_BF16, dtype=torch.int16, device="cuda")
        self.buf.view(torch.uint8)[band:band + raw.size] = torch.from_numpy(raw.copy()).cuda()
        self.ptr = self.buf.data_ptr() + band
        assert self.ptr % 256 == 0

    def numpy(self):
        return self.buf.view(torch.uint8)[self.band:self.band + self.n].cpu().numpy().view(self.dtype).reshape(self.shape)

    def intact(self):
        return bool((self.buf[:self.band // 2] == CE.NAN_BF16).all()) and bool((self.buf[(self.band + self.n) // 2:] == CE.NAN_BF16).all())


def guarded(band=BAND):
    """(alloc, check): alloc for CE.conv_call / CE.gn_call, check() synchronises and asserts every band of every operand intact"""
    band = (max(band, BAND) + 255) // 256 * 256
    made = []

    def alloc(a, name=""):
        made.append(Guarded(a, name, band))
        return made[-1]

    def check():
        torch.cuda.synchronize()
        for m in made:
            assert m.intact(), f"guard band of {m.name} written"
        return len(made)
    return alloc, check


RECORD = {"conv": {}, "gn": {}}


# ---- convolution ------------------------------------------------------------------------------------------------------------------------
def run_conv(lib, case, samples=None):
    alloc, check = guarded(case.block_bytes)
    rc, out, packed = CE.conv_call(lib, case, alloc, samples)
    assert rc == 0, lib.selftok_last_error()
    assert check() == 4 + case.bias + case.resid                   # x, w, packed weights, out [, bias] [, residual]: every band intact
    return out.numpy(), packed.numpy()


@pytest.mark.parametrize("case", CE.CONV_CASES, ids=lambda c: c.name)
def test_convolution_case(libs, case):
    gpu, twin = libs
    full, image = run_conv(gpu, case)
    got, ref = full[..., :case.cs], CE.conv_expected(case)
    assert (full[..., case.cs:] == CE.SENTINEL).all()                           # [Cstore, ldo) keeps its sentinel
    if case.gauss:
        ok, share = CE.gauss_gate(got, ref)
        print(f"{case.name}: {100 * share:.3f} % of the outputs differ from fp64-accumulate-round-once")
        RECORD["conv"][case.name] = share
        assert ok, share
    else:
        differ = int((got != ref).sum())
        print(f"{case.name}: {differ} of {got.size} elements differ from the exact reference")
        assert differ == 0, (differ, np.argwhere(got != ref)[:4], got[got != ref][:4], ref[got != ref][:4])
    tail = got[..., case.Cout:]                                                 # [Cout, Cstore): zero, or bf16(res)
    assert np.array_equal(tail, CE.f32_to_bf16_bits(CE.conv_inputs(case)["res"][..., case.Cout:case.cs]) if case.resid else np.zeros_like(tail))
    # bit for bit: run to run, each sample alone, the CPU twin (packed image: padding included)
    again, image2 = run_conv(gpu, case)
    assert np.array_equal(again, full) and np.array_equal(image2, image)
    for b in sorted({0, case.B - 1}) if case.B > 1 else ():
        alone, _ = run_conv(gpu, case, slice(b, b + 1))
        assert np.array_equal(alone[0], full[b]), b
    rc, tout, timage = CE.conv_call(twin, case, CE.Host)
    assert rc == 0 and np.array_equal(image, timage.numpy())
    if not case.gauss:
        assert np.array_equal(full, tout.numpy())


@pytest.mark.parametrize("case", [c for c in CE.CONV_EXACT if c.launch == CE.ROWS], ids=lambda c: c.name)
def test_rows_kernel_through_ops_equals_the_raw_entry(libs, case):
    gpu, _ = libs
    raw, _ = run_conv(gpu, case)
    d = CE.conv_inputs(case)
    bf = lambda a: torch.from_numpy(CE.f32_to_bf16_bits(a).view(np.int16)).cuda().view(torch.bfloat16)
    pc = ops.PackedConv(bf(d["w"]), bf(d["bias"]) if case.bias else None)
    assert pc.bn == case.bn
    res = bf(np.ascontiguousarray(d["res"][..., :case.cs])) if case.resid else None
    out = ops.conv2d_nhwc(bf(d["x"]), pc, stride=case.stride, upsample=bool(case.up), residual=res, cstore=case.cs)
    torch.cuda.synchronize()
    assert np.array_equal(out.view(torch.int16).cpu().numpy().view(np.uint16), raw[..., :case.cs])


def test_ops_refuses_a_cstore_past_the_packed_image():
    pc = ops.PackedConv(torch.zeros(128, 32, 3, 3, dtype=torch.bfloat16, device="cuda"), None)
    with pytest.raises(AssertionError):
        ops.conv2d_nhwc(torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16, device="cuda"), pc, cstore=132)


@pytest.mark.parametrize("shape", CE.PACK_CASES, ids=str)
def test_pack_equals_the_twin_and_the_formula(libs, shape):
    gpu, twin = libs
    Cout, Cin, ks, bn = shape
    w = np.random.default_rng(CE.seed_of(f"pack{shape}")).integers(1, 0x7F80, (Cout, Cin, ks, ks)).astype(np.uint16)
    n = gpu.selftok_conv2d_packed_bytes(Cout, Cin, ks, bn)
    assert n == twin.selftok_conv2d_packed_bytes(Cout, Cin, ks, bn)
    alloc, check = guarded()
    image = alloc(np.full(n // 2, CE.SENTINEL, np.uint16), "packed")
    assert gpu.selftok_conv2d_pack_weight_bf16(alloc(w, "w").ptr, image.ptr, Cout, Cin, ks, bn, None) == 0
    check()
    timage = np.full(n // 2, CE.SENTINEL, np.uint16)
    assert twin.selftok_conv2d_pack_weight_bf16(w.ctypes.data, timage.ctypes.data, Cout, Cin, ks, bn, None) == 0
    assert np.array_equal(image.numpy(), timage) and np.array_equal(timage, CE.pack_expected(w, Cout, Cin, ks, bn))


# ---- GroupNorm ------------------------------------------------------------------------------------------------------------------------------
_gpu_gn = {}


def run_gn(lib, case, silu, samples=None):
    alloc, check = guarded()
    rc, out = CE.gn_call(lib, case, alloc, silu, samples)
    assert rc == 0, lib.selftok_last_error()
    assert check() == (5 if case.layout == "nhwc" else 4)          # the workspace is not written beyond the size the library states
    return out.numpy()


def gpu_gn(lib, case, silu):
    if (case.name, silu) not in _gpu_gn:
        _gpu_gn[case.name, silu] = run_gn(lib, case, silu)
    return _gpu_gn[case.name, silu]


@pytest.mark.parametrize("case", CE.GN_CASES, ids=lambda c: c.name)
def test_groupnorm_case(libs, case):
    """inside the count cap, a constant group exact, run to run and a sample alone bit for bit, every guard band intact"""
    gpu, _ = libs
    for silu in (0, 1):
        got = gpu_gn(gpu, case, silu)
        _, diff, cap = CE.gn_gate(case, got, silu)
        torch_n = CE.gn_torch_counts(case)[silu]
        RECORD["gn"][case.name, silu] = (diff / case.n, torch_n / case.n, cap / case.n, CE.gn_outside(case, got, silu))
        print(f"{case.name} silu {silu}: {diff} of {case.n} differ from the fp64 reference (torch-CPU bf16: {torch_n}, cap {cap})")
        assert diff <= cap, (silu, diff, cap)
        if case.content == "const":
            cpg, g = case.C // case.groups, CE.CONST_GROUP % case.groups
            o = got if case.layout == "nhwc" else got.transpose(0, 2, 1)
            assert (o[:, :, g * cpg:(g + 1) * cpg] == CE.gn_const_expected(case, silu)).all()
        assert np.array_equal(run_gn(gpu, case, silu), got)
        for b in sorted({0, case.B - 1}) if case.B > 1 else ():
            assert np.array_equal(run_gn(gpu, case, silu, slice(b, b + 1))[0], got[b]), b


@pytest.mark.parametrize("case", CE.GN_CASES, ids=lambda c: c.name)
def test_groupnorm_bracket(libs, case):
    """every element is the reference's value or an adjacent bf16 value (with SiLU: within one output ulp of SiLU of those three), also where
    (x - mean) * rstd * w and the bias cancel to ~1e-7: the channels-last entry evaluates the normalisation in fp64 and rounds once
    (test_conv_edges_cpu.py::test_twin_groupnorm_bracket has what an fp32 evaluation, torch-CPU's included, does there)."""
    gpu, _ = libs
    what = {silu: CE.gn_outside(case, gpu_gn(gpu, case, silu), silu) for silu in (0, 1)}
    print(f"{case.name}: {what}")
    assert all(CE.gn_gate(case, gpu_gn(gpu, case, silu), silu)[0] for silu in (0, 1)), what


# ---- refusals, empty batch ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r", CE.NEW_REFUSALS + CE.OLD_REFUSALS, ids=lambda r: r[0])
def test_refusals_return_the_twins_code_and_write_nothing(libs, r):
    gpu, twin = libs
    alloc, check = guarded()
    rc, out = CE.refused_call(gpu, alloc, r)
    check()
    trc, _ = CE.refused_call(twin, CE.Host, r)
    assert rc == trc == CE.EINVAL and (out == CE.SENTINEL).all()
    assert gpu.selftok_last_error() == twin.selftok_last_error()
    assert any(m in gpu.selftok_last_error() for m in CE.NEW_MESSAGES) == (r in CE.NEW_REFUSALS)


def test_empty_batch_is_ok_and_untouched(libs):
    gpu, twin = libs
    for lib, (alloc, check) in ((gpu, guarded()), (twin, (CE.Host, lambda: None))):
        rc, out = CE.refused_call(lib, alloc, ("empty", 0, 4, 4, 32, 128, 128, 128, 3, 1, 0, 128))
        assert rc == 0 and (out == CE.SENTINEL).all()
        x, p, o = (alloc(np.full(4096, CE.SENTINEL, np.uint16), n) for n in ("x", "p", "out"))
        ws = alloc(np.full(4096, 0xC0, np.uint8), "workspace")
        assert lib.selftok_groupnorm_silu_nhwc_bf16(x.ptr, p.ptr, p.ptr, o.ptr, ws.ptr, 0, 16, 128, 32, CE.EPS, 1, None) == 0
        assert lib.selftok_groupnorm_silu_bf16(x.ptr, p.ptr, p.ptr, o.ptr, 0, 128, 16, 32, CE.EPS, 1, None) == 0
        check()
        assert (o.numpy() == CE.SENTINEL).all() and (ws.numpy() == 0xC0).all()


# ---- the record (profiles/conv_edges_vs_fp64.txt) -----------------------------------------------------------------------------------------------
def test_record(libs):
    """prints what the tests above measured: share of elements that differ from the fp64 reference, GPU | torch-CPU bf16 | cap"""
    gpu, _ = libs
    for case in CE.GN_CASES:
        for silu in (0, 1):
            if (case.name, silu) not in RECORD["gn"]:
                got = gpu_gn(gpu, case, silu)
                RECORD["gn"][case.name, silu] = (CE.gn_gate(case, got, silu)[1] / case.n, CE.gn_torch_counts(case)[silu] / case.n, CE.gn_cap(case, silu) / case.n,
                                                 CE.gn_outside(case, got, silu))
    print("\n[conv_edges] GroupNorm: share of elements that differ from the fp64 reference (gfx950 | torch-CPU bf16 | cap); elements outside the bracket")
    for (name, silu), (g, t, cap, outside) in RECORD["gn"].items():
        print(f"[conv_edges] {name:32s} {'silu ' if silu else 'plain'} {g:.2e} | {t:.2e} | {cap:.2e}; {outside}")
    for case in CE.CONV_GAUSS:
        if case.name not in RECORD["conv"]:
            RECORD["conv"][case.name] = CE.gauss_gate(run_conv(gpu, case)[0][..., :case.cs], CE.conv_expected(case))[1]
    print("[conv_edges] gaussian convolutions: share of outputs that differ from fp64-accumulate-round-once (gate: adjacent values, < 1 %)")
    for name, share in RECORD["conv"].items():
        print(f"[conv_edges] {name:32s} {share:.2e}")
    print(f"[conv_edges] worst gaussian convolution share {max(RECORD['conv'].values()):.2e}; exact convolution cases: {len(CE.CONV_EXACT)}, 0 elements differ in each")
    assert max(RECORD["conv"].values()) < 0.01
