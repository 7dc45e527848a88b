"""not gpu: the single-pass fp16 Linear mode (gemm="f16", csrc/gemm_f16.hip) pinned without a GPU -- the two C entries against the ctypes table
and the built library, the kernel file's scratch budget, the mode's presence on the host side, and a numpy STATEMENT of its arithmetic:
fp16-rounded operands, exact fp16 x fp16 products, fp32 accumulation in ascending 16-deep k-steps (the chain of the f16x2 kernel's high
accumulator).  The statement is held to the f16x2 emulation of tests/test_f16x2_arith_cpu.py run with zero low parts, its error against fp64
is printed (the figure DESIGN.md section 22 quotes), and the two mistakes a kernel of this kind can make -- the lo plane instead of the hi one,
a dropped last k-tile -- must change it on every shape."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import test_f16x2_arith_cpu as X2
from selftoktokenizer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_linear_f16_split", "selftok_linear_f16_split_residual"}
MS = (1, 15, 16, 17, 255, 256, 257, 513)
NS = (128, 384)
KS = (32, 64, 96, 128, 160, 192, 224, 256, 1536)       # 1 .. 8 k-tiles of 32: below, at and above the kernel's ring (3 stages of 2 k-tiles), and the model's K


def test_ext_header_declares_the_f16_entries_with_the_f16x2_argument_lists():
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
        assert (res, got) == _lib.SIGNATURES[n.replace("_f16_", "_f16x2_")], f"{n}: not the argument list of its f16x2 counterpart"
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_linear_f16_split.argtypes == _lib.EXT_SIGNATURES["selftok_linear_f16_split"][1]


def test_gemm_f16_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "gemm_f16.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    occ = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)]
    # ACT x OSPLIT without the residual form, + the residual form
    assert len(kernels) == 5 and all("linear_f16_pre_kernel" in k for k in kernels) and len(scratch) == len(lds) == len(occ) == 5, kernels
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert all(v == 3 * 2 * (16384 + 8192) for v in lds), lds           # three ring stages of two hi-plane k-tiles (activation 16 KiB + weight 8 KiB)
    assert all(o == 2 for o in occ), occ                                # the ping-pong schedule needs both waves of a SIMD resident


def test_the_mode_exists_on_the_host_side():
    from selftoktokenizer_amd import ops
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    assert "f16" in MMDiTGPU.GEMM_MODES and set(MMDiTGPU.SPLIT_MODES) == {"f16x2", "f16"}
    assert MMDiTGPU.GEMM_MODES[:3] == ("fp32", "f16x2", "exact")        # the three existing modes, unchanged
    assert callable(ops.linear_f16_split) and callable(ops.linear_f16_split_residual)
    for fn in (ops.linear_f16_split, MMDiTGPU.set_gemm):
        assert "SPLITK_MAX_ROWS" in fn.__doc__, "the docstring must say that small row counts stay on the f16x2 split-K route"


# ---- the arithmetic, in numpy ------------------------------------------------------------------------------------------------------
def r16(x):
    return x.astype(np.float16).astype(np.float32)


def f16_matmul(a, w, plane=0, drop_last_tile=False):
    """THE STATEMENT.  out[m, n] = the fp32 chain over ascending 16-deep k-steps of sum_k fp16(a[m, k]) fp16(w[n, k]): every product is exact in
    fp32 (11 x 11 significand bits); a 16-deep step is added to the running fp32 sum as one term.  `plane` = 1 and `drop_last_tile` are the planted
    mistakes: the lo plane of the split instead of the hi one; the last 32-deep k-tile never multiplied."""
    a0, w0 = (X2.split(a)[plane], X2.split(w)[plane])
    K = a.shape[1] - (32 if drop_last_tile else 0)
    acc = np.zeros((a.shape[0], w.shape[0]), np.float32)
    for s in range(0, K, 16):
        acc = acc + (a0[:, s:s + 16].astype(np.float64) @ w0[:, s:s + 16].astype(np.float64).T).astype(np.float32)   # the step's 16 exact products, one rounding
    return acc


def operands(M, N, K, exact_sums=False):
    rng = np.random.default_rng(1000003 * M + 1009 * N + K)
    if exact_sums:
        # multiples of 2^-4 below 4: products are multiples of 2^-8 below 16, every partial sum of up to 1536 of them is below 2^15 -> 23 bits, exact in fp32
        return (rng.integers(-63, 64, (M, K)) / 16.0).astype(np.float32), (rng.integers(-63, 64, (N, K)) / 16.0).astype(np.float32)
    a = (rng.standard_normal((M, K)) * (1.0 + 3.0 * rng.random((1, K)))).astype(np.float32)
    w = ((rng.random((N, K)) * 2 - 1) * np.sqrt(3.0 / K)).astype(np.float32)
    return a, w


@pytest.mark.parametrize("K", KS)
def test_statement_equals_the_f16x2_emulation_with_zero_low_parts(K):
    """`split_matmul` of tests/test_f16x2_arith_cpu.py on fp16-representable operands has zero low parts: it is hi + 0 with hi = a0 @ w0.T.
    Bit-equal wherever the order of an fp32 sum cannot matter -- operands whose every partial sum is exact (the emulation sums in the order of
    numpy's GEMM, the statement in 16-deep steps; on such operands both ARE the exact sum).  On general operands two fp32 summation orders of the
    same exact products differ by accumulation rounding only: each chain is within (n - 1) 2^-24 sum_k |a0 w0| of the exact sum (the textbook
    bound, n <= K additions in any order), so |difference| <= 2 K 2^-24 sum_k |a0 w0|."""
    for M in MS:
        for N in NS:
            a, w = operands(M, N, K, exact_sums=True)
            assert np.array_equal(X2.split(a)[1], np.zeros_like(a)) and np.array_equal(X2.split(w)[1], np.zeros_like(w))
            got, emu = f16_matmul(a, w), X2.split_matmul(a, w)
            assert np.array_equal(got.view(np.uint32), emu.view(np.uint32)), (M, N, K)
            assert np.array_equal(got.astype(np.float64), a.astype(np.float64) @ w.astype(np.float64).T)      # and both are the exact product
            a, w = operands(M, N, K)
            a, w = r16(a), r16(w)
            got, emu = f16_matmul(a, w), X2.split_matmul(a, w)
            bound = 2.0 * K * 2.0 ** -24 * (np.abs(a).astype(np.float64) @ np.abs(w).astype(np.float64).T)
            assert (np.abs(got.astype(np.float64) - emu.astype(np.float64)) <= bound).all(), (M, N, K)


@pytest.mark.parametrize("K", KS)
def test_planted_mistakes_change_the_result_on_every_shape(K):
    for M in MS:
        for N in NS:
            a, w = operands(M, N, K)
            good = f16_matmul(a, w)
            assert not np.array_equal(good, f16_matmul(a, w, plane=1)), ("lo plane instead of hi", M, N, K)
            assert not np.array_equal(good, f16_matmul(a, w, drop_last_tile=True)), ("last k-tile dropped", M, N, K)
            # every output row and column sees either mistake
            assert (np.abs(good - f16_matmul(a, w, drop_last_tile=True)).max(axis=1) > 0).all() and (np.abs(good - f16_matmul(a, w, plane=1)).max(axis=0) > 0).all()


def test_error_against_fp64_is_that_of_fp16_operands(capsys):
    """the figure the documents quote: rms error of the statement against the fp64 product of the fp32 operands, relative to the rms output, next to
    the f16x2 emulation's and numpy's fp32 GEMM.  Asserted: the operand rounding dominates -- two independent relative errors of at most 2^-11
    (uniform rounding error: rms 2^-11 / sqrt(3) each for values spread over a binade) per product, so the relative rms error of a sum of
    products stays below sqrt(2) 2^-11 -- and the mode is far outside the f16x2 arithmetic (it is a LOSSY mode, and the test says so)."""
    lines = []
    for K in KS:
        for M, N in ((257, 128), (513, 384)):
            a, w = operands(M, N, K)
            ref = a.astype(np.float64) @ w.astype(np.float64).T
            scale = np.sqrt(np.mean(ref ** 2))
            e16 = np.sqrt(np.mean((f16_matmul(a, w).astype(np.float64) - ref) ** 2)) / scale
            ex2 = np.sqrt(np.mean((X2.split_matmul(a, w).astype(np.float64) - ref) ** 2)) / scale
            e32 = np.sqrt(np.mean(((a @ w.T).astype(np.float64) - ref) ** 2)) / scale
            lines.append(f"M={M} N={N} K={K}: relative rms error vs fp64: f16 {e16:.3e}  f16x2 {ex2:.3e}  fp32 GEMM {e32:.3e}")
            assert e16 <= np.sqrt(2.0) * 2.0 ** -11, lines[-1]
            assert e16 > 100 * ex2, lines[-1]
    with capsys.disabled():
        print("\n" + "\n".join(lines))
