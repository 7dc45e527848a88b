"""not gpu: the split-K form of the single-pass fp16 Linear (csrc/gemm_f16_splitk.hip; set_gemm("f16", splitk="f16")) pinned without a GPU -- the
two C entries against the ctypes table, their f16x2 `_k` counterparts and the built library; the kernel file's resources as built; the switch on
the host side (signatures, refusal, graph key); ops.f16_ksplit as a function; and the numpy STATEMENT of tests/test_gemm_f16_cpu.py extended to
"ksplit ascending partial chains, then an ascending sum of the planes", held to the f16x2 split-K emulation with zero low parts and shown to
move under the two mistakes such a kernel pair can make."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import test_f16x2_arith_cpu as X2
import test_gemm_f16_cpu as F16
from selftoktokenizer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_linear_f16_split_k": "selftok_linear_f16x2_split_k", "selftok_linear_f16_split_residual_k": "selftok_linear_f16x2_split_residual_k"}
H = 1536
MODEL_SHAPES = ((3 * H, H), (H, H), (4 * H, H), (H, 4 * H))          # (N, K) of qkv, proj, fc1, fc2
MS = (1, 17, 257)
NS = (128, 384)
# (K / 32, ksplit): 1, 2, 3 (odd; as many as the ring has stages) and 4 k-tiles per part, and the model's K = 1536 and 6144 (parts of 3, 12 and 24)
KT_S = ((2, 2), (4, 2), (6, 2), (9, 3), (8, 2), (12, 4), (48, 16), (48, 4), (192, 64), (192, 8))


def test_ext_header_declares_the_split_k_entries_with_the_f16x2_k_argument_lists():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    assert "There is no split-K variant" not in hdr
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    lib = C.CDLL(_lib.LIB_PATH)
    for n, twin in NEW_ENTRIES.items():
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, f"{n} is not declared in selftok_hip_ext.h"
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
        assert n in _lib.EXT_SIGNATURES and n not in _lib.SIGNATURES, n
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want and res == ctype_of[m.group(1)], (n, args)
        assert (res, got) == _lib.SIGNATURES[twin], f"{n}: not the argument list of {twin}"
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"
        assert getattr(_lib.load(), n).argtypes == got


def test_gemm_f16_splitk_compiles_for_gfx950_with_the_resources_of_the_single_pass_kernel(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "gemm_f16_splitk.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    assert len(kernels) == 1 and "linear_f16_splitk_partial_kernel" in kernels[0], kernels       # the partial kernel; the reduction is gemm_split.hip's
    assert scratch == [0] and lds == [3 * 2 * (16384 + 8192)] and occ == [2], (scratch, lds, occ)  # no more LDS than linear_f16_pre_kernel; ping-pong kept


def test_the_switch_exists_on_the_host_side_and_is_refused_outside_the_f16_mode():
    from selftoktokenizer_amd import ops
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    from selftoktokenizer_amd.pipeline import SelftokPipeline
    assert MMDiTGPU.SPLITK_MODES == ("f16x2", "f16")
    for fn in (MMDiTGPU.set_gemm, SelftokPipeline.__init__, SelftokPipeline.set_gemm):
        p = inspect.signature(fn).parameters
        assert "splitk" in p and p["splitk"].default is None, fn
    assert callable(ops.linear_f16_split_k) and callable(ops.linear_f16_split_residual_k) and callable(ops.f16_ksplit)
    assert "ksplit" not in inspect.signature(ops.linear_f16_split).parameters, "the default route calls linear_f16_split without a ksplit"
    dit = MMDiTGPU.__new__(MMDiTGPU)                  # no device: the refusal comes before anything is touched
    for mode in ("f16x2", "fp32", "exact"):
        with pytest.raises(ValueError, match="splitk"):
            dit.set_gemm(mode, splitk="f16")
    with pytest.raises(ValueError, match="splitk"):
        dit.set_gemm("f16", splitk="fp16")
    pipe = SelftokPipeline.__new__(SelftokPipeline)
    pipe.model = types.SimpleNamespace(model=dit)
    with pytest.raises(ValueError, match="splitk"):
        pipe.set_gemm("f16x2", splitk="f16")
    doc = MMDiTGPU.set_gemm.__doc__
    assert "LOSSY" in doc and "splitk" in doc and "SPLITK_MAX_ROWS" in doc and "SPLITK_MAX_ROWS" in ops.linear_f16_split.__doc__
    src = inspect.getsource(SelftokPipeline._sample_group)
    key_line = src.split("key = ")[1].split("\n")[0]
    assert "dit.splitk" in key_line and "dit.attention" in key_line, "the split-K setting must be part of the hipGraph cache key, next to the attention setting"
    chk = inspect.getsource(SelftokPipeline._checked)
    assert "splitk=splitk" in chk, "the overflow -> fp32 -> back path must restore the setting"


def test_f16_ksplit_is_a_legal_split_for_every_small_row_count_of_the_model():
    from selftoktokenizer_amd import ops
    for N, K in MODEL_SHAPES:
        kt = K // 32
        for M in range(1, ops.SPLITK_MAX_ROWS + 1):
            s = ops.f16_ksplit(M, N, K)
            assert isinstance(s, int) and 1 <= s <= 64 and kt % s == 0, (M, N, K, s)
            assert s == ops.f16_ksplit(M, N, K)
        for M in (ops.SPLITK_MAX_ROWS + 1, 1040, 4096, 22912):
            assert ops.f16_ksplit(M, N, K) == 1, (M, N, K)
        assert ops.f16_ksplit(0, N, K) == 1
    # one image: the long chains (fc2: 192 k-tiles, proj: 48 on 12 tiles) are split; where the sweep found the single pass best (fc1) 1 is legal
    assert ops.f16_ksplit(256, H, 4 * H) > 1 and ops.f16_ksplit(256, H, H) > 1


# ---- the arithmetic, in numpy ------------------------------------------------------------------------------------------------------
def f16_splitk_matmul(a, w, s, descending=False, drop_last_tile=False):
    """THE STATEMENT, extended.  Part p = 0 .. s - 1 is the statement of tests/test_gemm_f16_cpu.py over columns [p K / s, (p + 1) K / s): the fp32
    chain over ascending 16-deep steps of exact fp16 x fp16 products, started at zero.  The s planes are then added in ascending order, plane 0
    first, one fp32 rounding per addition.  Planted mistakes: `descending` adds the planes last to first; `drop_last_tile` never multiplies the
    last 32-deep k-tile of every part (nothing then remains of a one-tile part)."""
    K = a.shape[1]
    assert K % (32 * s) == 0
    kp = K // s
    planes = []
    for p in range(s):
        ap, wp = a[:, p * kp:(p + 1) * kp], w[:, p * kp:(p + 1) * kp]
        if drop_last_tile and kp == 32:
            planes.append(np.zeros((a.shape[0], w.shape[0]), np.float32))
        else:
            planes.append(F16.f16_matmul(ap, wp, drop_last_tile=drop_last_tile))
    order = planes[::-1] if descending else planes
    acc = order[0]
    for pl in order[1:]:
        acc = acc + pl
    return acc


def f16x2_splitk_emulation(a, w, s):
    """the f16x2 split-K route in the arithmetic of tests/test_f16x2_arith_cpu.py: split_matmul per part, planes added in ascending order"""
    kp = a.shape[1] // s
    acc = X2.split_matmul(a[:, :kp], w[:, :kp])
    for p in range(1, s):
        acc = acc + X2.split_matmul(a[:, p * kp:(p + 1) * kp], w[:, p * kp:(p + 1) * kp])
    return acc


@pytest.mark.parametrize("kt,s", KT_S)
def test_statement_equals_the_f16x2_split_k_emulation_with_zero_low_parts(kt, s):
    """on operands whose every partial sum is exact (tests/test_gemm_f16_cpu.py: operands(exact_sums=True), up to 1536 products; K = 6144 sums four
    times as many, still below 2^17 in multiples of 2^-8 -> 25 bits: NOT exact in general, so that K takes magnitudes a quarter as large) the order
    of no fp32 sum can matter: bit-equal to the f16x2 split-K emulation, to the single-pass statement, and to the exact product.  s = 1 IS the
    single-pass statement on any operands."""
    K = 32 * kt
    for M in MS:
        for N in NS:
            a, w = F16.operands(M, N, K, exact_sums=True)
            if K > 1536:
                a = (np.round(a * 4.0) / 4.0).astype(np.float32) * np.float32(0.5)     # multiples of 2^-3 below 2: products multiples of 2^-6 below 8, 6144 of them < 2^16 -> 22 bits
                w = (np.round(w * 4.0) / 4.0).astype(np.float32) * np.float32(0.5)
            assert not X2.split(a)[1].any() and not X2.split(w)[1].any()
            got = f16_splitk_matmul(a, w, s)
            assert np.array_equal(got.view(np.uint32), f16x2_splitk_emulation(a, w, s).view(np.uint32)), (M, N, K, s)
            assert np.array_equal(got.astype(np.float64), a.astype(np.float64) @ w.astype(np.float64).T)
            assert np.array_equal(got, F16.f16_matmul(a, w))
            a, w = F16.operands(M, N, K)
            assert np.array_equal(f16_splitk_matmul(a, w, 1).view(np.uint32), F16.f16_matmul(a, w).view(np.uint32))
            # general operands: two summation orders of the same exact products, each within (n - 1) 2^-24 sum |a0 w0| of the exact sum
            a, w = F16.r16(a), F16.r16(w)
            bound = 2.0 * K * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T)
            assert (np.abs(f16_splitk_matmul(a, w, s).astype(np.float64) - f16x2_splitk_emulation(a, w, s).astype(np.float64)) <= bound).all(), (M, N, K, s)


@pytest.mark.parametrize("kt,s", KT_S)
def test_planted_mistakes_change_the_result_on_every_shape(kt, s):
    K = 32 * kt
    for M in MS:
        for N in NS:
            a, w = F16.operands(M, N, K)
            good = f16_splitk_matmul(a, w, s)
            bad = f16_splitk_matmul(a, w, s, drop_last_tile=True)
            assert (np.abs(good - bad).max(axis=1) > 0).all(), ("a part's last k-tile dropped", M, N, K, s)
            if s > 2:           # two planes: a + b == b + a in fp32; from three planes on the order of the roundings shows
                assert not np.array_equal(good, f16_splitk_matmul(a, w, s, descending=True)), ("planes added in descending order", M, N, K, s)
