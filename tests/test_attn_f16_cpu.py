"""not gpu: the single-pass fp16 joint attention (selftok_attn_f16, csrc/attention_f16.hip) pinned without a GPU -- the C entry against
the ctypes table and the built library, the switch on the host side, the kernel file's resources, and the numpy statement of its
arithmetic (tests/attn_f16_cases.py) against the fp64 reference of record and its per-element gate on every case of both tables.

Resources measured with -Rpass-analysis=kernel-resource-usage (hipcc of ROCm 7, gfx950), as DESIGN.md section 23 states them:
    attn64_f16_kernel<false>: 122 VGPRs, 0 AGPRs, 0 scratch, 16640 B LDS, 4 waves / SIMD
    attn64_f16_kernel<true> : 130 VGPRs, 0 AGPRs, 0 scratch, 16640 B LDS, 3 waves / SIMD

What the gate can and cannot see (figures of this file's own run, emulation error / gate, max over a case's rows):
    the statement itself          0.03 .. 0.33   (inside, with room; 32- and 64-key tiles)
    row sum of the last tile lost  1.6 .. 919 on every case (each has a row set with more than one tile) -> leaves the gate everywhere
    last visible key dropped / first invisible key admitted: the REFERENCE moves by >= 21 x the gate (asserted: >= 10) on every planted case
    q rounded before the multiply by c, p truncated instead of rounded: 0.04 .. 0.44 and 0.03 .. 0.52 of THAT gate on the tables' random data:
    it bounds any perturbation of the weights of relative size 2^-10 and cannot tell which fp16 value a weight was rounded to.
    These two roundings are pinned by the crafted two-key rows of attn_f16_cases.closed_form_rows instead, held to the closed form
    o = (1 - p~) / (1 + p~) with an fp32-sized tolerance (2^-22): the statement stays within 3e-8 of it; q rounded first (165 of 512 rows), q~ from
    the exact product as a fused multiply-convert gives it (91 of the 128 rows searched for double rounding) and p truncated (257 of 512) each
    leave it by up to 4e-4 .. 5e-4, asserted here; the same rows run on the kernel in tests/test_attn_f16_gpu.py."""
import ctypes
import inspect
import os
import re
import subprocess
import types

import numpy as np
import pytest

import attn_f16_cases as F
import edge_cases as E
import kmask_cases as KM
from selftoktokenizer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = F.ATTN_CASES + F.KMASK_CASES
MAX_SAMPLES = 8          # samples per case whose heads are emulated (spread over the case's samples, first and last included)
ROW_PICKS = (0, 1, 30, 31, 32, 33, 63, 64, 65, 126, 127, 128, 129, 255)


# ---- C ABI and host side -----------------------------------------------------------------------------------------------------------
def test_ext_header_declares_selftok_attn_f16():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert "selftok_attn_f16" in names and names == set(_lib.EXT_SIGNATURES) and not (names & set(_lib.SIGNATURES))
    m = re.search(r"(\w+)\s+selftok_attn_f16\s*\(([^)]*)\)\s*;", hdr)
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "hipStream_t": C.c_void_p}
    want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in (a.strip() for a in m.group(2).split(","))]
    res, got = _lib.EXT_SIGNATURES["selftok_attn_f16"]
    assert got == want and res == C.c_int
    assert (res, got) == _lib.EXT_SIGNATURES["selftok_attn_kmask_f32"], "the argument list of the masked entry: descriptor, words, words per sample, stream"
    assert hasattr(C.CDLL(_lib.LIB_PATH), "selftok_attn_f16"), "declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_attn_f16.argtypes == got


def test_the_switch_exists_on_the_host_side_and_is_refused_outside_the_f16_mode():
    from selftoktokenizer_amd import ops
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    from selftoktokenizer_amd.pipeline import SelftokPipeline
    assert ops.ATTN_F16 == 2 and ops.ATTN_F16X2 == 1
    assert MMDiTGPU.ATTENTION_MODES == ("split", "f16")
    for fn in (MMDiTGPU.set_gemm, SelftokPipeline.set_gemm, SelftokPipeline.__init__):
        p = inspect.signature(fn).parameters
        assert "attention" in p and p["attention"].default is None, fn
    dit = MMDiTGPU.__new__(MMDiTGPU)                  # no device: the refusal comes before anything is touched
    for mode in ("f16x2", "fp32", "exact"):
        with pytest.raises(ValueError, match="attention"):
            dit.set_gemm(mode, attention="f16")
    with pytest.raises(ValueError, match="attention"):
        dit.set_gemm("f16", attention="fp16")
    pipe = SelftokPipeline.__new__(SelftokPipeline)
    pipe.model = types.SimpleNamespace(model=dit)
    with pytest.raises(ValueError, match="attention"):
        pipe.set_gemm("f16x2", attention="f16")
    assert "LOSSY" in MMDiTGPU.set_gemm.__doc__ and "attention" in MMDiTGPU.set_gemm.__doc__
    src = inspect.getsource(SelftokPipeline._sample_group)
    assert "dit.attention" in src.split("key = ")[1].split("\n")[0], "the attention setting must be part of the hipGraph cache key"


def test_attention_f16_compiles_for_gfx950_with_the_stated_resources(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "attention_f16.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda name: [int(v) for v in re.findall(name + r": (\d+)", r.stderr)]
    vgpr, agpr, scratch = field(r" VGPRs"), field(r"AGPRs"), field(r"ScratchSize \[bytes/lane\]")
    lds, occ = field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == 2 and all("attn64_f16_kernel" in k for k in kernels), kernels
    print(dict(zip(kernels, zip(vgpr, agpr, scratch, lds, occ))))
    assert scratch == [0, 0] and agpr == [0, 0]
    assert lds == [16640, 16640]                      # two buffers of one K image (4224 B) + one V^T image (4096 B)
    by = {("ILb1E" in k): (v, o) for k, v, o in zip(kernels, vgpr, occ)}
    assert by[False][1] == 4 and by[False][0] <= 128, by            # 122 VGPRs measured
    assert by[True][1] == 3 and by[True][0] <= 168, by              # 130 VGPRs measured
    assert min(occ) >= 2
    hdr = open(os.path.join(G.CSRC, "attention.hip")).read()
    for moved in ("struct AttnParams", "struct KMaskWalk", "ragged_word(int key0, int nkeys) {"):
        assert moved not in hdr and moved in open(os.path.join(G.CSRC, "attention_shared.h")).read(), f"{moved}: one definition, in the shared header"


# ---- the arithmetic ----------------------------------------------------------------------------------------------------------------
def test_fp16_helpers():
    x = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -10 - 2.0 ** -20, -(1.0 + 2.0 ** -10 - 2.0 ** -20), 2.0 ** -26], dtype=np.float32)
    assert np.array_equal(F.f16_round(x), np.array([1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 2.0 ** -24 * 0], dtype=np.float32))
    assert np.array_equal(F.f16_trunc(x), np.array([1.0, 1.0 + 2.0 ** -10, 1.0, -1.0, 0.0], dtype=np.float32))
    assert float(F.C_F32) == float(np.float32(0.125) * np.float32(1.4426950408889634))


_CACHE = {}


def _case_data(case, planted):
    key = (case.name, planted)
    if key not in _CACHE:
        cb, xb = F.buffers(case, planted=planted)
        B = case.B
        bs = sorted(set(np.linspace(0, B - 1, min(B, MAX_SAMPLES)).round().astype(int).tolist()))
        pairs = [(b, b % case.H) for b in bs]
        e = F.e32(case, cb, xb, pairs=pairs)
        _CACHE[key] = (cb, xb, pairs, e)
    return _CACHE[key]


def _pick(q):
    idx = sorted({i for i in ROW_PICKS if i < len(q)} | {len(q) - 1})
    return q[idx]


def _ratios(case, planted, mistake=None, tiles=(F.KEY_TILE,)):
    """max over the case's picked rows of |emulation - R| / gate, and whether any (row set) has more than one tile"""
    cb, xb, pairs, e = _case_data(case, planted)
    worst, multi = 0.0, False
    for b, h in pairs:
        for tag, q, k, v in F.head_rows(case, F.head_operands(case, b, h, cb, xb)):
            q = _pick(q)
            R, A = F.reference(q, k, v)
            g = F.gate(A, len(k), float(np.abs(v).max()), e)
            for tile in tiles:
                if mistake == "drop_last_sum" and len(k) <= tile:
                    continue
                multi = multi or len(k) > tile
                worst = max(worst, float((np.abs(F.emulate(q, k, v, tile=tile, mistake=mistake).astype(np.float64) - R) / g).max()))
    return worst, multi


@pytest.mark.parametrize("planted", [False, True], ids=["plain", "planted"])
@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_statement_is_inside_the_gate_and_the_lost_row_sum_is_not(case, planted):
    """the emulation with the kernel's 32-key tiles and with 64-key tiles against the reference of record; the planted mistakes"""
    good, _ = _ratios(case, planted, tiles=(32, 64))
    lost, multi = _ratios(case, planted, "drop_last_sum")
    qr, _ = _ratios(case, planted, "q_round_first")
    pt, _ = _ratios(case, planted, "p_trunc")
    print(f"[attn_f16] {case.name} {'planted' if planted else 'plain'}: emulation / gate {good:.3f}; row sum of the last tile lost {lost:.1f}; "
          f"q rounded first {qr:.3f}; p truncated {pt:.3f}")
    assert good <= 1.0, f"{case.name}: the statement of the arithmetic leaves its own gate ({good:.3f})"
    assert multi, f"{case.name}: no row set with more than one tile"
    assert lost > 1.0, f"{case.name}: a lost row sum stays inside the gate ({lost:.3f})"


def test_bound_holds_from_1_to_1281_keys_for_gaussian_and_scaled_q():
    """the gate against the tiled emulation at 1 .. 1281 keys, gaussian and 4 x scaled q (E32 = 0: the bound's own two terms + the fp32
    accumulation allowance of n 2^-24 max|v| that the second term already grants)"""
    rng = np.random.default_rng(20)
    worst = 0.0
    for n in (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 614, 1281):
        for qs in (1.0, 4.0):
            q = (rng.standard_normal((48, 64)) * qs).astype(np.float32)
            k = F.f16_round(rng.standard_normal((n, 64)).astype(np.float32))
            v = F.f16_round(rng.standard_normal((n, 64)).astype(np.float32))
            R, A = F.reference(q, k, v)
            g = F.gate(A, n, float(np.abs(v).max()), 1e-7)
            for tile in (32, 64):
                r = float((np.abs(F.emulate(q, k, v, tile=tile).astype(np.float64) - R) / g).max())
                worst = max(worst, r)
                assert r <= 1.0, (n, qs, tile, r)
    print(f"[attn_f16] largest emulation error / gate over 1 .. 1281 keys: {worst:.3f}")


def test_closed_form_rows_pin_the_two_roundings_and_fail_each_planted_rounding_mistake():
    """the crafted two-key rows of attn_f16_cases.closed_form_rows: the statement equals o = (1 - p~) / (1 + p~) within CLOSED_TOL (four fp32
    roundings, no tuned factor) on every row and dimension, with 32- and 64-key tiles; q rounded before the multiply by c, q~ taken from the exact
    product (a fused multiply-convert) and p truncated each LEAVE that tolerance -- by three orders of magnitude -- on the rows that can see them"""
    q, (k0, v0), (k1, v1), o, _ = F.closed_form_rows()
    k, v = np.concatenate([k0, k1]), np.concatenate([v0, v1])
    n1 = F.CLOSED_ROWS
    err = lambda **kw: np.abs(F.emulate(q, k, v, **kw).astype(np.float64) - o[:, None]).max(axis=1)
    for tile in (32, 64):
        e = err(tile=tile)
        assert e.max() <= F.CLOSED_TOL, (tile, e.max())
    bad = {m: err(mistake=m) > F.CLOSED_TOL for m in ("q_round_first", "q_fused", "p_trunc")}
    worst = {m: float(err(mistake=m).max()) for m in bad}
    print(f"[attn_f16] closed form: statement {err().max():.2e} (tolerance {F.CLOSED_TOL:.2e}); rows beyond it / largest error: "
          + "; ".join(f"{m} {int(b[:n1].sum())} of {n1} + {int(b[n1:].sum())} of {len(b) - n1}, {worst[m]:.2e}" for m, b in bad.items()))
    assert bad["p_trunc"][:n1].sum() >= n1 // 4, "truncation differs from rounding wherever p rounds up: about half of the rows"
    assert bad["q_round_first"].any() and worst["q_round_first"] > 100 * F.CLOSED_TOL
    # evenly spread x rarely sit on a double-rounding tie; the searched rows all do: one rounding instead of two moves q~ by an fp16 ulp there
    assert bad["q_fused"][n1:].sum() >= (len(o) - n1) // 4
    assert not (err(mistake="drop_last_sum") > F.CLOSED_TOL).any()   # (the keys past the first tile carry exact zeros: this mistake belongs to the gate above)


def _moved(case, b, h, cb, xb, e, vis=None, nx=None):
    """max norm of (reference over a changed visible set - reference) and of the gate, over every row of head h of sample b (a handful of rows can miss the planted key's weight)"""
    move = gmax = 0.0
    base = F.head_rows(case, F.head_operands(case, b, h, cb, xb))
    pert = F.head_rows(case, F.head_operands(case, b, h, cb, xb, vis=vis, nx=nx))
    for (tag, q, k, v), (_, _, k2, v2) in zip(base, pert):
        if len(k2) == 0 or (k2.shape == k.shape and np.array_equal(v2, v)):
            continue                                   # rows left without a key (they would be dead), rows that do not see the changed segment
        R, A = F.reference(q, k, v)
        R2, _ = F.reference(q, k2, v2)
        move = max(move, float(np.abs(R2 - R).max()))
        gmax = max(gmax, float(F.gate(A, len(k), float(np.abs(v).max()), e).max()))
    return move, gmax


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c.name)
def test_one_key_off_moves_the_reference_by_ten_gates_on_every_planted_case(case):
    cb, xb, pairs, e = _case_data(case, True)
    least = np.inf
    for b, h in pairs:
        vis = F.visible_ctx(case, b)
        probes = [dict(nx=case.nx - 1), dict(nx=case.nx + 1)]                          # image segment: last key dropped, first row past `len` admitted
        if len(vis):
            probes.append(dict(vis=vis[:-1]))                                           # last visible context key dropped
        hidden = np.setdiff1d(np.arange(case.Kc + 1), vis)                              # index Kc: the first row past `len`
        probes.append(dict(vis=np.sort(np.append(vis, hidden[0]))))                     # first invisible context key admitted
        for p in probes:
            move, gmax = _moved(case, b, h, cb, xb, e, **p)
            assert gmax > 0 and move >= 10.0 * gmax, f"{case.name} b={b} {list(p)}: reference moves by {move:.3e} = {move / gmax:.1f} gates"
            least = min(least, move / gmax)
    print(f"[attn_f16] {case.name}: one key off moves the reference by >= {least:.0f} gates")
