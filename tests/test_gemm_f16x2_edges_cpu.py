"""not gpu: tests/gemm_f16x2_cases.py checked on the host -- the case tables reach the ring, tile-map, ragged and split-K edges they claim; the
exact-data conditions hold (asserted from numpy float16, not from the plan); the restated tile map is a bijection; the CPU twin
(oracle/libselftok_cpu.so) equals the reference bit for bit through all five f16x2 entries, and its packed image and split planes equal
pack_image / planes; every planted mistake changes every case `applies` names and none it calls blind; csrc/gemm_split.hip still compiles for
gfx950 without scratch.  tests/test_gemm_f16x2_edges_gpu.py then holds the gfx950 kernels to the same reference."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import abi_cases as A
import gemm_f16x2_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K6144 = G.Case("cpu/kt192/M33/N128", "ring", 33, 128, 6144)
TWIN_MAX_FMAS = 1e7             # the twin is a scalar loop: of a larger case it computes the first and the last TWIN_HEAVY_ROWS rows (every output row is
TWIN_HEAVY_ROWS = 48            # a function of its own input row alone, so these are the case's own numbers; its weights are packed and compared whole)


@pytest.fixture(scope="module")
def twin():
    path = os.path.join(ROOT, "oracle", "libselftok_cpu.so")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return A.bind(path)


def same(a, b):
    """equal as numbers (signed zeros alike), no NaN on either side"""
    return a.shape == b.shape and bool((a == b).all())


# ---- the tables reach what they claim ----------------------------------------------------------------------------------------------------
def test_ring_table_reaches_both_kernels_rings_and_prefetch_distances_odd_and_even():
    kts = sorted({c.K // 32 for c in G.RING})
    assert kts == sorted(G.RING_KT) and {(c.M, c.N) for c in G.RING} == {(m, n) for m in G.RING_M for n in G.RING_N}
    assert len(G.RING) == len(G.RING_KT) * len(G.RING_M) * len(G.RING_N)
    for depth in (G.RING_A1, G.RING_W1, G.AHEAD_W1, G.RING_A2, G.RING_W2, G.AHEAD_A2, G.AHEAD_W2):
        for kt in (depth - 1, depth, depth + 1, 2 * depth, 2 * depth + 1):      # fewer, as many, one more (the first reuse), a whole second lap and past it
            assert kt in kts or kt == 0, (depth, kt)
    for parity in (0, 1):
        assert sum(kt % 2 == parity for kt in kts) >= 5
    assert 1 in kts and 2 in kts and 3 in kts            # the prologue alone, with every clamped prefetch: tiles 1, 2 (and 3) past the end
    assert 48 in kts                                     # the model's K = 1536
    assert any(not c.bias for c in G.RING) and sum(c.bias for c in G.RING) > len(G.RING) // 2


def test_m_table_stands_on_every_16_64_256_edge():
    ms = set(G.RING_M)
    for edge in (16, 256):
        assert {edge - 1, edge, edge + 1} <= ms, edge
    assert {255, 256, 257} <= ms and 272 in ms and 513 in ms and 1 in ms
    # the 64-row wave slice: a ragged end inside the first, the second (272 = 256 + 16: one chunk into it) and a full slice; more than one, two row blocks
    assert any(0 < m % 256 < 64 for m in ms) and any(m % 256 > 192 for m in ms) and any(m > 512 for m in ms)
    assert any(m % 16 == 0 and m % 256 for m in ms) and any(m % 16 == 1 for m in ms) and any(m % 16 == 15 for m in ms)


def test_tile_map_table_reaches_every_residue_and_group_shape():
    grids = [(-(-c.M // 256), c.N // 128) for c in G.TILEMAP]
    assert grids == list(G.TILE_GRIDS)
    assert {(mb * nb) % 8 for mb, nb in grids} == set(range(8))
    assert {mb % 4 for mb, _ in grids} == set(range(4))
    assert {nb for _, nb in grids} == {1, 2, 3, 5, 8}
    assert {(1, 1), (2, 1), (3, 1), (5, 1), (4, 2), (5, 2), (7, 3), (6, 3), (9, 5), (8, 8), (3, 5)} <= set(grids)
    assert all(c.M % 256 and c.K == 32 for c in G.TILEMAP)                      # the last row block ragged
    assert any(G.applies("tilemap_r8", c) for c in G.TILEMAP) and any(G.applies("tilemap_gsz", c) for c in G.TILEMAP)
    assert any(mb > 8 and mb % 4 for mb, _ in grids), "a short last group after two full ones"


def test_split_k_table_reaches_every_tiles_per_part():
    per = {(c.K // 32) // c.ksplit for c in G.SPLITK if c.ksplit > 1}
    assert {1, 2, 3, 4} <= per
    assert {(c.K, c.ksplit) for c in G.SPLITK} >= {(2048, 64), (2048, 32)}
    assert {c.M for c in G.SPLITK} == {1, 16, 257, 1024} and any(c.ksplit == 1 for c in G.SPLITK)
    assert all((c.K // 32) % c.ksplit == 0 and 1 <= c.ksplit <= 64 for c in G.SPLITK + G.RESID)
    assert {(c.B, c.T) for c in G.RESID} >= {(3, 77), (2, 129), (5, 51), (1, 257)} and {c.gate for c in G.RESID} == {"token", "sample", None}
    inside_tile = [c for c in G.RESID if c.B > 1 and c.T % 256]
    assert any(c.T % 64 for c in inside_tile) and any(c.T % 256 == 0 for c in G.RESID if c.B > 1)
    assert sorted(c.K // 32 for c in G.GAUSS) == [1, 4, 5, 6, 48]
    names = [c.name for c in G.EXACT + G.GAUSS]
    assert len(set(names)) == len(names)


# ---- the exact-data conditions, from numpy float16 ---------------------------------------------------------------------------------------
def _check_exact(case):
    d = G.exact_data(case)
    for x, h, l, s in ((d["a"], d["ah"], d["al"], d["sa"]), (d["w"], d["wh"], d["wl"], d["sw"])):
        assert 0 <= s <= 12
        hi, lo = G.planes(x)
        assert np.array_equal(hi.astype(np.float64) * 2.0 ** s, h.astype(np.float64)), case.name + ": a hi plane element is not the planned integer"
        assert np.array_equal(lo.astype(np.float64) * 2.0 ** s, l.astype(np.float64)), case.name + ": a lo plane element is not the planned integer"
        assert ((np.abs(h) >= 5) & (np.abs(h) <= 7) | ((h == 0) & (l == 0))).all() and (np.abs(l) <= 3).all()
        if x.size >= 4096:
            assert (l != 0).mean() >= G.LO_NONZERO_SHARE, (case.name, float((l != 0).mean()))
    share, top = G.rounded_share(case)
    assert top < 2 ** 24, case.name
    return share


def test_exact_data_conditions_hold_on_every_case():
    """every hi and lo plane element is the planned integer; the largest sum |a0||w0| stays below 2^24; the stated share of the low parts is
    non-zero; data differs in every tile, k-tile and plane (no two 32-deep tiles of a tensor are equal in either plane)"""
    for case in G.EXACT:
        _check_exact(case)
        d = G.exact_data(case)
        if case.M >= 16:
            for t, width in ((d["ah"], 32), (d["al"], 32), (d["wh"], 32), (d["wl"], 32)):
                tiles = t.reshape(t.shape[0], -1, width).transpose(1, 0, 2).reshape(t.shape[1] // width, -1)
                assert len({tl.tobytes() for tl in tiles}) == len(tiles), case.name
    for case in G.EXACT:
        if case.family == "resid":
            d = G.exact_data(case)
            assert np.array_equal(d["resid"], np.round(d["resid"]))
            if case.gate:
                m, e = np.frexp(d["table"])
                assert (np.abs(m) == 0.5).all() and d["table"].shape[1] == 3 * case.N


def test_stated_shares_of_rounded_outputs():
    big = next(c for c in G.RING if c.K == 1536 and c.M == 257 and c.N == 384)
    s1536 = _check_exact(big)
    s6144 = _check_exact(K6144)
    print(f"\noutputs that need the final rounding: K = 1536 {s1536:.3f}, K = 6144 {s6144:.3f}")
    assert s1536 >= G.ROUNDED_SHARE_K1536 and s6144 >= G.ROUNDED_SHARE_K6144
    assert 49 * 6144 < 2 ** 24 and 42 * 6144 < 2 ** 24


# ---- the tile map ------------------------------------------------------------------------------------------------------------------------
def test_tile_of_workgroup_is_a_bijection_onto_the_grid():
    for mblocks in range(1, 13):
        for nblocks in range(1, 13):
            T = mblocks * nblocks
            tiles = [G.tile_of_workgroup(T, o, mblocks, nblocks) for o in range(T)]
            assert sorted(tiles) == [(m, n) for m in range(mblocks) for n in range(nblocks)], (mblocks, nblocks)
            own = G.owner_of_tiles(mblocks, nblocks)
            assert all(len(v) == 1 for v in own.values()) and len(own) == T
            case = G.Case("x", "tilemap", 256 * mblocks - 37, 128 * nblocks, 32)
            for mistake in ("tilemap_r8", "tilemap_gsz"):      # `applies` == "some tile is left without a work-group"
                assert (len(G.owner_of_tiles(mblocks, nblocks, mistake)) < T) == G.applies(mistake, case), (mistake, mblocks, nblocks)


# ---- the CPU twin ------------------------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def _twin_all_entries(twin, case, rows=None):
    """the reference of `case` against the twin's five f16x2 entries (those the case's shape allows); `rows`: a subset of rows (each output row
    is a function of its own input row: the subset is the case's own numbers)"""
    d = G.exact_data(case)
    ref = G.reference(case)
    M, N, K, s = case.M, case.N, case.K, case.ksplit
    a, bias = d["a"], d["bias"]
    sel = np.arange(M) if rows is None else rows
    ov = np.zeros(1, np.int32)
    packed = np.zeros(N * K * 2, np.uint16)
    assert twin.selftok_linear_f16x2_pack_weight(_p(d["w"]), _p(packed), N, K, _p(ov), None) == 0
    assert np.array_equal(packed, G.pack_image(d["w"])), case.name + ": packed image"
    a_sel = np.ascontiguousarray(a[sel])
    m = len(sel)
    blk = np.zeros(((m + 15) // 16, K // 32, 2, 16, 32), np.uint16)
    assert twin.selftok_split_f16x2_f32(_p(a_sel), K, _p(blk), m, K, _p(ov), None) == 0
    assert np.array_equal(blk, G.split_image(a_sel)), case.name + ": split planes"
    hi, lo = G.planes(a_sel)
    assert np.array_equal(G.image_planes(blk, m), np.stack([hi, lo]))
    out = np.full((m, N), np.nan, np.float32)
    ws = np.zeros(max(s, 2) * m * N, np.float32)
    tag = case.name
    if case.family == "resid":
        # rows keep their sample and token index only for the whole case
        assert rows is None
        gate = d["table"][:, N:2 * N] if case.gate else None
        gsb, gst = (0, 3 * N) if case.gate == "token" else (3 * N, 0)
        args = (_p(blk), _p(packed), _p(bias), _p(d["resid"]), N, _p(gate), gsb, gst, case.T, _p(out), N, M, N, K)
        if s == 1:
            assert twin.selftok_linear_f16x2_split_residual(*args, _p(ov), None) == 0
            assert same(out, ref), tag + ": _split_residual"
            out[:] = np.nan
        assert twin.selftok_linear_f16x2_split_residual_k(*args, s, _p(ws), _p(ov), None) == 0
        assert same(out, ref), tag + ": _split_residual_k"
    else:
        if s == 1:
            assert twin.selftok_linear_f16x2_f32(_p(a_sel), K, _p(packed), _p(bias), _p(out), N, m, N, K, 0, _p(ov), None) == 0
            assert same(out, ref[sel]), tag + ": _f32"
            out[:] = np.nan
            assert twin.selftok_linear_f16x2_split(_p(blk), _p(packed), _p(bias), _p(out), None, N, m, N, K, 0, _p(ov), None) == 0
            assert same(out, ref[sel]), tag + ": _split"
        else:
            assert twin.selftok_linear_f16x2_split_k(_p(blk), _p(packed), _p(bias), _p(out), None, N, m, N, K, 0, s, _p(ws), _p(ov), None) == 0
            assert same(out, ref[sel]), tag + ": _split_k"
        oblk = np.zeros(((m + 15) // 16, N // 32, 2, 16, 32), np.uint16)      # the split output, through _split_k (ksplit = 1 forwards)
        assert twin.selftok_linear_f16x2_split_k(_p(blk), _p(packed), _p(bias), None, _p(oblk), N, m, N, K, 0, s, _p(ws), _p(ov), None) == 0
        rh, rl = G.planes(ref[sel])
        assert same(G.image_planes(oblk, m).astype(np.float32), np.stack([rh, rl]).astype(np.float32)), tag + ": split output"
    assert int(ov[0]) == 0
    return ref.size if rows is None else m * N


def _rows_for_twin(case):
    if case.family == "resid" or case.M <= 2 * TWIN_HEAVY_ROWS or case.M * case.N * case.K <= TWIN_MAX_FMAS:
        return None
    return np.concatenate([np.arange(TWIN_HEAVY_ROWS), np.arange(case.M - TWIN_HEAVY_ROWS, case.M)])


@pytest.mark.parametrize("family", ["ring", "tilemap", "splitk", "resid"])
def test_cpu_twin_equals_the_reference_bit_for_bit(twin, family):
    table = {"ring": G.RING, "tilemap": G.TILEMAP, "splitk": G.SPLITK, "resid": G.RESID}[family]
    n = 0
    for case in table:
        assert case.K <= G.TWIN_MAX_K
        n += _twin_all_entries(twin, case, _rows_for_twin(case))
    print(f"\n{family}: {len(table)} cases, {n} elements per entry, 0 differing")


def test_cpu_twin_at_its_largest_k(twin):
    _twin_all_entries(twin, K6144)
    _twin_all_entries(twin, K6144._replace(name="cpu/kt192/s8", ksplit=8, family="splitk"))


# ---- planted mistakes --------------------------------------------------------------------------------------------------------------------
def _differs(a, b):
    return not bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def test_every_planted_mistake_shows_where_applies_says_and_nowhere_it_calls_blind():
    """per exact case and kernel: the reference with the mistake planted differs from the reference iff `applies` says so (None = not asserted:
    "descending" where the running sum of the planes is rounded).  A mistake of the other kernel is no mistake of this one; a mistake both
    kernels can make is modelled once (the model does not depend on the kernel) and `applies` must give the first kernel the same verdict."""
    seen = dict.fromkeys(G.MISTAKES, 0)
    blind = dict.fromkeys(G.MISTAKES, 0)
    for case in G.EXACT:
        base = G.reference(case)
        first_route = case.ksplit == 1 and case.family != "resid"
        for mistake, (who, _) in G.MISTAKES.items():
            want = G.applies(mistake, case, "second" if who != "first" else "first")
            other = G.applies(mistake, case, "first" if who != "first" else "second")
            if who == "first":
                assert other is False
                if not first_route:
                    assert want is False
                    continue
            elif who == "second" or not first_route:
                assert other is False
            else:
                assert other == want
            if want is None:
                continue
            changed = _differs(G.reference(case, mistake, "first" if who == "first" else "second"), base)
            assert changed == want, (mistake, case.name, "changed" if changed else "unchanged")
            seen[mistake] += want
            blind[mistake] += not want
    print("\n" + "\n".join(f"{m:16s} seen by {seen[m]:3d} cases, blind in {blind[m]:3d}" for m in G.MISTAKES))
    assert all(seen[m] > 0 for m in G.MISTAKES if m != "descending")
    # "descending": blind on exact data wherever every prefix sum is exact or two planes commute, not asserted elsewhere; three gaussian planes see it
    assert seen["descending"] == 0 and all(G.applies("descending", c) is False for c in G.EXACT if c.ksplit <= 2 or c.K <= 128)
    rng = np.random.default_rng(5)
    parts = [rng.standard_normal((17, 128)).astype(np.float32) for _ in range(3)]
    assert _differs((parts[0] + parts[1]) + parts[2], (parts[2] + parts[1]) + parts[0])


# ---- the kernel file as built --------------------------------------------------------------------------------------------------------------
def test_gemm_split_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as B
    objs, _ = B.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "gemm_split.o")
    r = subprocess.run(cmd, cwd=B.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == len(scratch) and sum("linear_f16x2_pre_kernel" in k for k in kernels) >= 6 and sum("linear_f16x2_kernel" in k for k in kernels) >= 2, kernels
    assert sum("splitk_finish_kernel" in k for k in kernels) >= 5
    assert scratch and all(v == 0 for v in scratch), dict(zip(kernels, scratch))
