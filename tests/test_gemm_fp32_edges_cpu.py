"""not gpu: tests/gemm_fp32_cases.py checked on the host -- the restated launch plan of csrc/gemm_fp32.hip computes every (tile, chunk)
exactly once for any shape and workspace, the case table reaches the edges it claims, and the MKL-order reference (the oracle + a numpy
epilogue) reproduces the CPU twin's `selftok_linear_f32` bit for bit while five planted mistakes do not.
tests/test_gemm_fp32_edges_gpu.py then holds the gfx950 kernel to the same reference."""
import os
import subprocess

import numpy as np
import pytest
import torch

import abi_cases as A
import gemm_fp32_cases as G
from selftoktokenizer_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MKL_ORDER, BIAS_LAST, GELU_FLAG = 4, 2, 1
SENT32 = 0x7FC0DEAD
TWIN_MAX_FMAS = 4e8              # a case the twin computes whole in about a second


@pytest.fixture(scope="module")
def twin():
    path = os.path.join(ROOT, "oracle", "libselftok_cpu.so")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    return A.bind(path)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(a, b):
    """signed zeros alike, as `_bits_equal` of tests/test_gemm_fp32_gpu.py"""
    return bool(((bits(a) == bits(b)) | ((a == 0) & (b == 0))).all())


def test_inputs_are_synth_hash_normalish():
    for seed, shape in ((0, (7,)), (0x51, (33, 65)), (G.name_seed("gemm_fp32_edges/257x256x800/w"), (256, 800))):
        assert np.array_equal(bits(G.hash_normalish(seed, shape)), bits(synth.hash_normalish(seed, shape).numpy()))
    assert G.name_seed("a/b") == synth.name_seed("a/b")


# ---- exact cover -----------------------------------------------------------------------------------------------------------------
def _check_plan(M, N, K, mkl, ws_avail, force=0, seen=None):
    """`seen`: the plans of this (M, N, K, order) already walked -- another workspace size that leads to the same plan is only held to its bytes"""
    p = G.plan(M, N, K, mkl, ws_avail, force)
    tag = f"M={M} N={N} K={K} mkl={mkl} ws={ws_avail} force={force}"
    assert p.ws_bytes <= ws_avail, f"{tag}: a plan of {p.ws_bytes} bytes was taken"
    assert p.ws_bytes <= G.workspace_bytes(M, N, K, mkl), tag
    assert p.grid == 8 * (p.full_pos + p.tail_cnt * p.split), tag
    if seen is not None:
        if p in seen:
            return p
        seen.add(p)
    us = G.units(p)
    assert len(us) == p.grid
    assert sorted({G.tile_of(s, p.mt, p.nt) for s in range(p.tiles)}) == [(a, b) for a in range(p.mt) for b in range(p.nt)], f"{tag}: the tile list is no permutation"
    cover = np.zeros((p.tiles, p.nchunks), np.int32)
    slots, by_tile = set(), {}
    for u in us:
        if u is None:
            continue
        assert (u.tm, u.tn) == G.tile_of(u.sidx, p.mt, p.nt) and u.tm < p.mt and u.tn < p.nt
        cover[u.sidx, u.c0:u.c1] += 1
        if u.slot is None:
            assert u.c0 == 0 and u.c1 == p.nchunks, f"{tag}: a tile that goes straight to out is not whole"
        else:
            assert u.slot not in slots, f"{tag}: plane {u.slot} written twice"
            assert (u.slot + 1) * G.PLANE * 4 <= p.ws_bytes, f"{tag}: plane {u.slot} lies past the {p.ws_bytes} bytes stated"
            slots.add(u.slot)
            by_tile.setdefault(u.sidx, []).append((u.c0, u.slot))
            if mkl:
                assert u.c0 % 12 == 0 and u.c1 - u.c0 == min(12, p.nchunks - u.c0), f"{tag}: an MKL unit is no K-block"
    assert (cover == 1).all(), f"{tag}: {int((cover != 1).sum())} (tile, chunk) pairs not computed exactly once"
    fin = dict(G.finish_reads(p))
    assert set(fin) == set(by_tile), f"{tag}: the finish kernel and the units disagree on the tail tiles"
    for sidx, order in fin.items():
        assert order == [s for _, s in sorted(by_tile[sidx])], f"{tag}: planes of tile {sidx} are not added in K order"
    return p


def test_plan_computes_every_tile_and_chunk_exactly_once():
    Ms = sorted({m for q in range(1, 10) for m in (256 * q - 1, 256 * q, 256 * q + 1)} | {1, 2400} | {1 + int(v) % 2400 for v in G._hash_u32(0xC0FE, 12)})
    walked = refused = distinct = 0
    for M in Ms:
        h = G._hash_u32(M, 2 * 12)
        shapes = {(1, 1), (48, 64), (48, 1), (1, 64), (29, 25), (29, 2)} | {(1 + int(h[2 * i]) % 48, 1 + int(h[2 * i + 1]) % 64) for i in range(12)}
        for nt, kc in sorted(shapes):
            N, K = 128 * nt, 32 * kc
            for mkl in (True, False):
                if mkl and 384 < K < 768:
                    with pytest.raises(G.Refused):
                        G.plan(M, N, K, True, 1 << 40)
                    refused += 1
                    continue
                top = G.workspace_bytes(M, N, K, mkl)
                best = G.plan(M, N, K, mkl, top)
                sizes = {0, top, top // 2, max(best.ws_bytes - 1, 0), best.ws_bytes, 1 << 40}
                seen = set()
                for ws in sorted(sizes):
                    p = _check_plan(M, N, K, mkl, ws, seen=seen)
                    if ws >= best.ws_bytes:
                        assert p == best, "a larger workspace changes the plan"
                    walked += 1
                if not mkl:
                    for S in (2, 3, 4, 6, 8):
                        if kc % S == 0:
                            _check_plan(M, N, K, False, top, force=S, seen=seen)
                            walked += 1
                distinct += len(seen)
    print(f"\n[gemm_fp32 edges] cover sweep: {walked} (M, N, K, order, workspace) plans walked ({distinct} distinct launch geometries), {refused} MKL-order shapes with 384 < K < 768 refused")
    assert walked > 4000


def test_forced_split_refusals_of_the_restatement():
    top = G.workspace_bytes(257, 256, 800, False)
    for force in (2, 3, 4, 6, 8):
        with pytest.raises(G.Refused):
            G.plan(257, 256, 800, False, top, force)            # 25 chunks: only 5 divides
    with pytest.raises(G.Refused):
        G.plan(257, 256, 800, True, top, 2)                      # 3 K-blocks
    need = G.plan(257, 256, 800, True, top, 3).ws_bytes
    with pytest.raises(G.Refused):
        G.plan(257, 256, 800, True, need - 1, 3)
    assert G.plan(2048, 4096, 800, True, 0, 7).split == 1        # 256 tiles = one full round, no tail round: nothing to force


# ---- the table's claims --------------------------------------------------------------------------------------------------------------
def _e(name, mkl, **kw):
    c = G.BY_NAME[name]
    return G.edges(c.M, c.N, c.K, mkl, **kw)


def test_case_table_reaches_the_edges_it_claims():
    e = _e("1x128x32", True)
    assert (e.tiles, e.unit_chunks, e.live_last_rows, e.grid, e.split) == (1, (1,), 1, 8, 1) and sorted(e.short_xcds) == list(range(1, 8))
    assert _e("1x128x32", False).split == 1
    for name, n in (("255x128x64", 2), ("256x128x96", 3), ("257x128x128", 4)):
        e = _e(name, True)
        assert (e.split, e.unit_chunks) == (1, (n,)), name                      # MKL order: one whole tile of n chunks
        f = _e(name, False)
        assert (f.tail_cnt, f.split, f.unit_chunks) == (1, n, (1,)), name       # free order: n units of ONE chunk
    assert _e("255x128x64", True).live_last_rows == 255 and _e("256x128x96", True).live_last_rows == 256 and _e("257x128x128", True).live_last_rows == 1

    e, f = _e("257x256x800", True), _e("257x256x800", False)
    assert (e.tiles, e.per, e.tail_cnt, e.split, e.unit_chunks) == (4, 1, 1, 3, (1, 12)) and (f.split, f.unit_chunks) == (5, (5,))
    assert e.tail_absent == {x: (0,) for x in (4, 5, 6, 7)} == f.tail_absent
    assert e.ws_bytes == 8 * 1 * 3 * G.PLANE * 4 and f.ws_bytes == 8 * 1 * 5 * G.PLANE * 4

    e, f = _e("513x128x384", True), _e("513x128x384", False)
    assert (e.mt_rem, e.tiles, e.split, e.unit_chunks, e.ws_bytes) == (3, 3, 1, (12,), 0) and G.n_blocks(384) == 1
    assert (f.split, f.unit_chunks) == (6, (2,))

    e = _e("768x384x1184", True)
    assert (e.mt_rem, e.tiles, e.per, e.full_rounds, e.tail_cnt, e.split, e.unit_chunks) == (3, 9, 2, 0, 2, 4, (1, 12)) and 1184 == 3 * 384 + 32
    assert e.short_xcds == {4: 1, 5: 0, 6: 0, 7: 0} and e.tail_absent == {4: (1,), 5: (0, 1), 6: (0, 1), 7: (0, 1)}
    assert e.ws_bytes == 8 * 2 * 4 * G.PLANE * 4

    e = _e("1793x128x1536", True)
    assert (e.mt_rem, e.tiles, e.per, e.live_last_rows, e.split, e.unit_chunks) == (0, 8, 1, 1, 4, (12,)) and not e.short_xcds

    e = _e("2049x128x2048", True)
    assert (e.mt_rem, e.tiles, e.per, e.tail_cnt, e.split, e.unit_chunks, e.live_last_rows) == (1, 9, 2, 2, 6, (4, 12), 1)

    for mkl, split in ((True, 3), (False, 5)):
        e = _e("2301x3712x800", mkl)
        assert (e.mt_rem, e.tiles, e.per, e.full_rounds, e.tail_cnt, e.split, e.live_last_rows) == (1, 261, 33, 1, 1, split, 253)
        assert e.short_xcds == {7: 30} and e.tail_absent == {7: (0,)}       # XCD 7: entries 30 and 31 of the full round and the tail entry are absent
        assert e.grid == 8 * (32 + split)

    e, f = _e("2304x3712x64", True), _e("2304x3712x64", False)
    assert (e.tiles, e.per, e.full_rounds, e.tail_cnt, e.split, e.unit_chunks, e.grid, e.live_last_rows) == (261, 33, 1, 0, 1, (2,), 8 * 33, 256)
    assert (f.tail_cnt, f.split, f.unit_chunks, f.grid) == (1, 2, (1, 2), 8 * 34) and f.short_xcds == {7: 30}

    assert (_e("1153x256x32", True).mt_rem, _e("1700x384x32", True).mt_rem, _e("4700x256x32", True).mt_rem) == (5, 7, 3)
    assert _e("1700x384x32", True).short_xcds == {7: 0} and G.plan(4700, 256, 32, True, 0).mt == 19

    f = _e("300x128x512", False)
    assert not G.BY_NAME["300x128x512"].mkl_ok and (f.split, f.unit_chunks) == (8, (2,)) and G.BY_NAME["300x128x512"].free_splits() == [2, 4, 8]

    # over the whole table: every remainder band 0, 1, 3, 5, 7; 1, 2, 3, 4 chunks per unit; a short XCD list inside a full round
    rems = {_e(c.name, False).mt_rem for c in G.CASES}
    assert {0, 1, 3, 5, 7} <= rems
    assert {1, 2, 3, 4} <= {n for c in G.CASES for mkl in (False, True) if mkl <= c.mkl_ok for n in _e(c.name, mkl).unit_chunks}
    for c in G.CASES:                                            # the no-workspace variant is the unsplit plan
        assert _e(c.name, False, ws_avail=0).split == 1
        assert 256 * (c.m_half // 256) == c.m_half != c.M or c.M == 256


def test_evaluated_tiles_hold_what_the_issue_asks():
    for c in G.CASES:
        ev = set(G.evaluated_tiles(c))
        for mkl in (False, True):
            if mkl and not c.mkl_ok:
                continue
            p = G.plan(c.M, c.N, c.K, mkl, G.workspace_bytes(c.M, c.N, c.K, mkl))
            assert {G.tile_of(s, p.mt, p.nt) for s, _ in G.finish_reads(p)} <= ev, c.name
            for x in range(8):
                n = G.list_len(p, x)
                if n:
                    assert {G.tile_of(x * p.per, p.mt, p.nt), G.tile_of(x * p.per + n - 1, p.mt, p.nt)} <= ev, c.name
            if c.M % 256:
                assert {(p.mt - 1, tn) for tn in range(p.nt)} <= ev, c.name
        assert len(ev) <= 64


# ---- the reference against the CPU twin --------------------------------------------------------------------------------------------------
def _twin_run(twin, case, epi, x_wide, w, b, gate, res):
    """the twin's selftok_linear_f32 in MKL order on the GPU test's buffer layout: x a column slice (ldx = 2 K + 32), out a column slice
    at offset 32 of a sentinel buffer [M + 3, N + 128] (contiguous for GELU), gate / res column slices of their tables"""
    M, N, K = case.M, case.N, case.K
    x = G.x_of(case, x_wide)
    if epi.gelu:
        buf = np.full((M + 3, N), SENT32, np.uint32).view(np.float32)
        out = buf[:M]
    else:
        buf = np.full((M + 3, N + 128), SENT32, np.uint32).view(np.float32)
        out = buf[:M, 32:32 + N]
    if epi.res == "alias":
        out[:] = res
        res = out
    ld = lambda a: a.strides[0] // 4
    flags = MKL_ORDER | (BIAS_LAST if epi.bias_last else 0) | (GELU_FLAG if epi.gelu else 0)
    rc = twin.selftok_linear_f32(x.ctypes.data, ld(x), w.ctypes.data, b.ctypes.data if epi.bias else None, res.ctypes.data if res is not None else None,
                                 ld(res) if res is not None else 0, epi.res_mod, gate.ctypes.data if gate is not None else None, ld(gate) if gate is not None else 0,
                                 epi.gate_mod, out.ctypes.data, ld(out), M, N, K, flags, None, 0, None)
    assert rc == 0, twin.selftok_last_error()
    live = np.zeros(buf.shape, bool)
    live[:M, (0 if epi.gelu else 32):(0 if epi.gelu else 32) + N] = True
    assert (buf.view(np.uint32)[~live] == SENT32).all()
    return out.copy()


def _all_tiles(case):
    return [(a, b) for a in range(-(-case.M // 256)) for b in range(case.N // 128)]


def _reference_whole(case, epi, x_wide, w, b, gate, res, mistake=None):
    x = G.x_of(case, x_wide)[:case.M]
    out = np.empty((case.M, case.N), np.float32)
    for (tm, tn), v in G.reference_tiles(case, x, w, b, epi, gate, res, _all_tiles(case), mistake).items():
        rs, cs = G.tile_slices(case, tm, tn)
        out[rs, cs] = v
    return out


@pytest.mark.parametrize("case", [c for c in G.CASES if c.mkl_ok and c.M * c.N * c.K <= TWIN_MAX_FMAS], ids=lambda c: c.name)
def test_reference_equals_the_twin_plain(twin, case):
    xw, w, b = G.inputs(case)
    assert same_bits(_reference_whole(case, G.PLAIN, xw, w, b, None, None), _twin_run(twin, case, G.PLAIN, xw, w, b, None, None))


@pytest.mark.parametrize("epi", G.EPILOGUES + [G.GELU], ids=lambda e: e.name)
@pytest.mark.parametrize("case", G.EPILOGUE_CASES[:2], ids=lambda c: c.name)
def test_reference_equals_the_twin_with_every_epilogue(twin, case, epi):
    xw, w, b = G.inputs(case)
    gate, res = G.epilogue_tables(case, epi)
    assert same_bits(_reference_whole(case, epi, xw, w, b, gate, res), _twin_run(twin, case, epi, xw, w, b, gate, res))


def test_spelled_out_k_blocks_equal_the_oracle():
    for name in ("257x256x800", "768x384x1184", "513x128x384"):
        case = G.BY_NAME[name]
        xw, w, b = G.inputs(case)
        x = np.ascontiguousarray(G.x_of(case, xw)[:case.M])
        assert np.array_equal(bits(G.mkl_product(x, w, b, restated=True)), bits(G.mkl_product(x, w, b)))


MISTAKE_EPI = {      # an epilogue in which the mistake is visible: two or more K-blocks behind a bias, a per-token gate, gate and res together
    "bias_first_despite_bias_last": "bias_last_gate_token_res_row",
    "div_for_mod": "bias_last_gate_token_res_row",
    "gate_after_res": "bias_last_gate_token_res_row",
    "kblock_352": "bias_first_res_row",
    "blocks_descending": "bias_first_res_row",
}


@pytest.mark.parametrize("mistake", G.MISTAKES)
def test_planted_mistake_breaks_the_equality(twin, mistake):
    case = G.BY_NAME["257x256x800"]
    epi = {e.name: e for e in G.EPILOGUES}[MISTAKE_EPI[mistake]]
    xw, w, b = G.inputs(case)
    gate, res = G.epilogue_tables(case, epi)
    got = _twin_run(twin, case, epi, xw, w, b, gate, res)
    assert same_bits(_reference_whole(case, epi, xw, w, b, gate, res), got)
    wrong = _reference_whole(case, epi, xw, w, b, gate, res, mistake)
    n = int((bits(wrong) != bits(got)).sum())
    print(f"\n[gemm_fp32 edges] planted {mistake}: {n} of {got.size} elements differ from the twin")
    assert n > got.size // 100, f"{mistake} went unnoticed"


def test_free_order_reference_is_fp64_of_the_same_operation(twin):
    """the twin's free order (one chain over K) against the fp64 reference: within fp32 accumulation noise, epilogue included"""
    case = G.BY_NAME["257x256x800"]
    epi = {e.name: e for e in G.EPILOGUES}["bias_last_gate_token_res_row"]
    xw, w, b = G.inputs(case)
    gate, res = G.epilogue_tables(case, epi)
    x = G.x_of(case, xw)
    out = np.zeros((case.M, case.N), np.float32)
    rc = twin.selftok_linear_f32(x.ctypes.data, x.strides[0] // 4, w.ctypes.data, b.ctypes.data, res.ctypes.data, res.strides[0] // 4, epi.res_mod, gate.ctypes.data,
                                 gate.strides[0] // 4, epi.gate_mod, out.ctypes.data, case.N, case.M, case.N, case.K, BIAS_LAST, None, 0, None)
    assert rc == 0
    r64 = G.reference_f64(x[:case.M], w, b, epi, gate, res)
    t32 = (torch.from_numpy(res.copy())[G.table_row(np.arange(case.M), epi.res_mod)]
           + torch.from_numpy(gate.copy())[G.table_row(np.arange(case.M), epi.gate_mod)] * torch.nn.functional.linear(torch.from_numpy(x[:case.M].copy()), torch.from_numpy(w), torch.from_numpy(b))).numpy()
    e_twin, e_torch = np.sqrt(np.mean((out - r64) ** 2)), np.sqrt(np.mean((t32 - r64) ** 2))
    assert e_twin <= 2 * e_torch + 1e-8, (e_twin, e_torch)
