"""not gpu: the token statistics pinned on the host -- the numpy emulations of tests/token_stats_cases.py against a second formulation each, what the case tables
claim to hold, the planted mistakes in both directions, the C entries against the ctypes table, the kernels' resource budget, the host-side refusals and the
host half of TokenCensus (row limit, merge, save, load)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import token_stats_cases as TC
from selftoktokenizer_amd import _lib, ops, tokenstats as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"selftok_token_count", "selftok_token_census_workspace_bytes", "selftok_token_census", "selftok_token_to_u16", "selftok_token_agree",
           "selftok_token_nearest_workspace_bytes", "selftok_token_nearest"}


def _census_close(a, b):
    return np.array_equal(a[:, [0, 1, 4]], b[:, [0, 1, 4]]) and (np.abs(a[:, 2:4] - b[:, 2:4]) <= TC.H_TOL).all()


@pytest.mark.parametrize("name", [c.name for c in TC.COUNT_CASES])
def test_count_and_census_emulations_equal_their_second_formulation(name):
    c = TC.COUNT_BY_NAME[name]
    base, view = TC.make_ids(name)
    assert view.shape == (c.N, c.K) and view.dtype == TC._NP[c.dtype] and (c.N == 0 or view.strides == ((c.K * c.es + c.rpad) * view.itemsize, c.es * view.itemsize))
    counts, bad = TC.count(view, c.C)
    bc, bb = TC.count_brute(view, c.C)
    assert np.array_equal(counts, bc) and bad == bb and int(counts.astype(np.uint64).sum()) + bad == c.N * c.K
    cen = TC.census(counts)
    assert _census_close(cen, TC.census_brute(counts)) and not np.signbit(cen[:, [0, 1, 2, 4]]).any()          # H_ref of a single code is -ln(1 + 1e-10) < 0, as the reference's
    packed, pbad = TC.to_u16(view)
    v = view.astype(np.int64)
    assert pbad == int(((v < 0) | (v > 65535)).sum()) and np.array_equal(packed[(v >= 0) & (v <= 65535)], v[(v >= 0) & (v <= 65535)])


def test_the_count_table_holds_what_it_claims():
    cs = TC.COUNT_CASES
    assert {0, 1, 63, 64, 65} <= {c.N for c in cs} and {c.K for c in cs} == {1, 3, 40, 512, 1024} and {5, 64, 32768} <= {c.C for c in cs}
    assert {c.N * c.K for c in cs} >= {255, 256, 257, 240, 280} and TC.ROW_TILE == 256                       # the flat tile of 256 ids +- 1, in rows and in ids
    assert {c.dtype for c in cs} == {"uint16", "int32", "int64"} and {c.es for c in cs} == {1, 2, 8} and any(c.rpad for c in cs)
    for c in cs:
        base, view = TC.make_ids(c.name)
        counts, bad = TC.count(view, c.C)
        cen = TC.census(counts)
        v = view.astype(np.int64)
        if c.kind == "equal":
            assert c.N == 4096 and counts[0, 7] == 4096 and counts.sum() == 4096
        if c.kind == "ends":
            assert counts[:, 0].all() and counts[:, c.C - 1].all() and counts[:, 1:c.C - 1].sum() == 0 and bad == 0
        if c.kind == "bad":
            want = {"uint16": {c.C, 65535}, "int32": {-1, c.C}, "int64": {-1, c.C, 1 << 40, TC.INT64_MIN}}[c.dtype]
            assert want <= set(v[(v < 0) | (v >= c.C)].tolist()) and bad >= len(want)
        if c.kind == "uniform":                                     # every code once (or N / C times) per position: perplexity == C to the last bit but a few
            assert (cen[:, 1] == c.C).all() and np.abs(np.exp(cen[:, 2]) - c.C).max() <= 1e-9 * c.C and (counts == counts[0, 0]).all()
        if c.kind in ("one_code", "equal"):
            assert (cen[:, 2] == 0.0).all() and (cen[:, 1] == 1).all() and (cen[:, 4] == cen[:, 0]).all()
        if c.kind == "dead_pos":
            assert (cen[0] == 0).all() and cen[1, 0] == c.N and bad == c.N
        if c.kind == "skewed":
            n_k = cen[:c.K, 0]
            assert len(set(n_k.tolist())) > 1 and TC.census_applies("pooled_mean", counts)[0][c.K]
        if c.kind == "high":
            assert c.C == 65536 and (v >= 32768).all() and bad == 0
    assert {c.kind for c in cs} == {"random", "equal", "ends", "bad", "uniform", "one_code", "dead_pos", "skewed", "high"}


@pytest.mark.parametrize("mut", TC.COUNT_MUTS)
def test_every_count_case_that_can_see_a_planted_mistake_sees_it(mut):
    seen = 0
    for c in TC.COUNT_CASES:
        base, view = TC.make_ids(c.name)
        good = TC.count(view, c.C)
        bad = TC.count(view, c.C, mut, base=base, es=c.es)
        moved = not (np.array_equal(good[0], bad[0]) and good[1] == bad[1])
        if mut == "u16_signed":                                     # the packing entry reads the same ids: it sees the mistake wherever a uint16 id has its top bit set
            moved_pack = not np.array_equal(TC.to_u16(view)[0], TC.to_u16(view, mut)[0])
            assert moved_pack == (c.dtype == "uint16" and bool((view.astype(np.int64) >= 32768).any())), c.name
        assert moved == TC.count_applies(mut, c, view), (mut, c.name)
        seen += moved
    assert seen >= {"u16_signed": 1, "no_elem_stride": 4, "clamp": 6}.get(mut, 10), (mut, seen)


@pytest.mark.parametrize("mut", TC.CENSUS_MUTS)
def test_every_census_case_that_can_see_a_planted_mistake_sees_it(mut):
    seen = 0
    for c in TC.COUNT_CASES:
        base, view = TC.make_ids(c.name)
        counts, _ = TC.count(view, c.C)
        good, bad = TC.census(counts), TC.census(counts, mut)
        rows, cols = TC.census_applies(mut, counts)
        others = [j for j in range(5) if j not in cols]
        assert np.array_equal(good[:, others], bad[:, others]), (mut, c.name)                                # exactly the columns it names
        delta = np.abs(good - bad)[:, list(cols)]
        assert (delta[rows] >= TC.MOVE).any(axis=1).all(), (mut, c.name, delta[rows].min() if rows.any() else None)
        if mut in ("used_gt1", "pooled_mean", "log2"):              # ... and the rows it does not name stay as they are (the 1e-10 mistakes fade with `used`, they do not stop)
            assert (delta[~rows] <= 10 * TC.MOVE).all(), (mut, c.name)
        if mut == "pooled_mean":
            assert np.array_equal(good[:c.K], bad[:c.K])
        seen += int(rows.any())
    assert seen >= {"pooled_mean": 3}.get(mut, 8), (mut, seen)


@pytest.mark.parametrize("name", [c.name for c in TC.AGREE_CASES])
def test_agreement_emulation_equals_the_matrix_formulation_and_sees_the_planted_mistakes(name):
    c = TC.AGREE_BY_NAME[name]
    a, b = TC.make_agree(name)
    good = TC.agree(a, b, c.k_lo, c.k_hi)
    for x, y in zip(good, TC.agree_brute(a, b, c.k_lo, c.k_hi)):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    match_pos, n_diff, first, last = good
    assert (match_pos[:c.k_lo] == 0).all() and (match_pos[c.k_hi:] == 0).all()
    if c.N:
        assert int(match_pos.sum()) + int(n_diff.sum()) == c.N * (c.k_hi - c.k_lo)
        assert ((n_diff == 0) == (first == c.K)).all() and ((n_diff == 0) == (last == -1)).all() and (first[n_diff > 0] <= last[n_diff > 0]).all()
    touched = np.arange(c.N) % 3 != 1
    if c.kind == "equal":
        assert (n_diff == 0).all() and (match_pos[c.k_lo:c.k_hi] == c.N).all()
    if c.kind == "flip0":
        assert (first[touched] == 0).all() and (last[touched] == 0).all() and (n_diff[touched] == 1).all() and (n_diff[~touched] == 0).all()
    if c.kind == "flipend":
        assert (first[touched] == c.K - 1).all() and (last[touched] == c.K - 1).all()
    if c.kind == "flipboth":                                        # either end of the range cuts its flip off
        want_first = 0 if c.k_lo == 0 else (c.K - 1 if c.k_hi == c.K else c.K)
        want_last = c.K - 1 if c.k_hi == c.K else (0 if c.k_lo == 0 else -1)
        assert (first[touched] == want_first).all() and (last[touched] == want_last).all() and (n_diff[touched] == (c.k_lo == 0) + (c.k_hi == c.K)).all()
    for mut in TC.AGREE_MUTS:
        bad = TC.agree(a, b, c.k_lo, c.k_hi, mut)
        moved = not all(np.array_equal(x, y) for x, y in zip(good, bad))
        assert moved == TC.agree_applies(mut, c, a, b), (mut, name)


def test_the_agreement_table_holds_what_it_claims():
    kinds = {(c.kind, c.k_lo > 0, c.k_hi < c.K) for c in TC.AGREE_CASES}
    assert {("equal", False, False), ("flip0", False, False), ("flipend", False, False), ("flipboth", False, False), ("flipboth", True, False),
            ("flipboth", False, True), ("flipboth", True, True)} <= kinds and {c.N for c in TC.AGREE_CASES} >= {0, 257} and {c.K for c in TC.AGREE_CASES} >= {1, 40, 41, 512, 1024}
    for mut in TC.AGREE_MUTS:
        assert sum(TC.agree_applies(mut, c, *TC.make_agree(c.name)) for c in TC.AGREE_CASES) >= 4


@pytest.mark.parametrize("name", [c.name for c in TC.NEAR_CASES])
def test_nearest_emulation_equals_the_matrix_formulation_and_sees_the_planted_mistakes(name):
    c = TC.NEAR_BY_NAME[name]
    q, ref = TC.make_near(name)
    assert q.shape == (c.M, c.K) and ref.shape == (c.N, c.K) and q.dtype == ref.dtype == np.uint16 and (c.self == (q is ref))
    best, idx = TC.nearest(q, ref, c.k_lo, c.k_hi, c.self)
    bb, bi = TC.nearest_brute(q, ref, c.k_lo, c.k_hi, c.self)
    assert np.array_equal(best, bb) and np.array_equal(idx, bi) and best.dtype == idx.dtype == np.int32
    for parts in (1, 3):                                            # the emulation's own partition is invisible
        assert all(np.array_equal(x, y) for x, y in zip((best, idx), TC.nearest(q, ref, c.k_lo, c.k_hi, c.self, parts=parts)))
    span = c.k_hi - c.k_lo
    if c.N == 0 or (c.self and c.N == 1):
        assert (best == -1).all() and (idx == 0).all()
    elif c.kind in ("c4", "planted", "dups") and span >= 30 and c.M:
        t = TC.tied(q, ref, c.k_lo, c.k_hi, c.self)
        if c.M >= 30:
            assert t.mean() >= 0.10, (name, t.mean())               # ties are common: the index rule decides
        copies = best == span
        if c.kind == "planted":
            assert copies[0] and idx[0] == TC.PLANT[0] and copies.sum() == 1 and (ref[TC.PLANT[1]] == q[0]).all()
        elif c.kind == "dups":                                      # rows 3, 10 and N - 1 are one row, 20 and 21 another: each finds its lowest other copy
            assert set(np.flatnonzero(copies)) == {3, 10, c.N - 1, 20, 21} and idx[3] == 10 and idx[10] == 3 and idx[c.N - 1] == 3 and idx[20] == 21 and idx[21] == 20
        else:
            assert not copies.any()
        assert (best > 0).all() and (best[~copies] < span).all()   # strictly inside (0, K) but for the planted rows
    for mut in TC.NEAR_MUTS:
        bad = TC.nearest(q, ref, c.k_lo, c.k_hi, c.self, mut)
        moved = not (np.array_equal(best, bad[0]) and np.array_equal(idx, bad[1]))
        assert moved == TC.near_applies(mut, c, q, ref), (mut, name)
        if mut == "highest_index":
            assert np.array_equal(best, bad[0])                     # the index alone moves


def test_the_nearest_table_holds_what_it_claims():
    cs = TC.NEAR_CASES
    assert {63, 64, 65, 0, 1} <= {c.M for c in cs} and {0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513} <= {c.N for c in cs} and {1, 40, 512, 1024} <= {c.K for c in cs}
    assert {c.kind for c in cs} == {"c4", "k1", "planted", "dups"} and sum(c.self for c in cs) >= 4 and sum((c.k_lo, c.k_hi) != (0, c.K) for c in cs) >= 5
    assert any(c.K % 2 for c in cs if c.K > 1) and any(c.k_lo % 2 and c.K % 2 == 0 for c in cs) and any(c.k_lo == c.k_hi for c in cs)
    for mut in TC.NEAR_MUTS:
        assert sum(TC.near_applies(mut, c, *TC.make_near(c.name)) for c in cs) >= 3, mut
    assert TC.TILE == 64 and TC.SPLITS == (1, 2, 3, 5, 64)


def test_ext_header_declares_the_entries_of_the_ctypes_table():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    assert set(re.findall(r"\b(selftok_token_\w+)\s*\(", hdr)) == ENTRIES == {n for n in _lib.EXT_SIGNATURES if n.startswith("selftok_token_")}
    lib = C.CDLL(_lib.LIB_PATH)
    for n in ENTRIES:
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want and res == ctype_of[m.group(1)], (n, args)
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_token_stats_compiles_for_gfx950_without_scratch(tmp_path):
    """recorded at this revision: 9 kernels.  tok_nearest_kernel (both paths) 159 VGPRs, 20480 bytes of LDS (two 64 x 36-word tiles and 2 KiB of keys), 3 waves per
    SIMD -- three workgroups per compute unit; its inner loop is 512 each of v_pk_sub, v_pk_min_u16 and v_pk_add_u16 per 64 ds_read_b128, three vector
    instructions per two id comparisons.  tok_census_kernel 60 VGPRs (the fp64 log), 160 bytes; count, pack, pool, agreement and finalize 8 - 17 VGPRs, no LDS, 8 waves."""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "token_stats.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 9, kernels
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert sum("tok_nearest_kernel" in k for k in kernels) == 2
    for k, v, l, o in zip(kernels, vgprs, lds, occ):
        if "tok_nearest_kernel" in k:
            assert o >= 3 and v <= 168 and l <= 20480, (k, v, l, o)
        elif "tok_census_kernel" in k:
            assert v <= 64 and l <= 256 and o == 8, (k, v, l, o)
        else:
            assert v <= 24 and l == 0 and o == 8, (k, v, l, o)
    src = open(os.path.join(G.CSRC, "token_stats.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "asm" not in code and "mfma" not in code and code.count("atomicAdd(") == 4          # count, its bad ids, the packer's bad ids, match_pos: nothing else


def test_host_side_refusals_and_workspace_sizes_without_a_gpu():
    """every refusal is decided on the host before anything is launched: these calls pass HOST pointers and would fault in a kernel"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.full(4096, 0x5A5A5A5A, np.uint32)
    p = x.ctypes.data
    count = lambda ib, n, K, Cc, rs=1, es=1, ids=p, cnt=p, bad=p: lib.selftok_token_count(ids, ib, n, K, Cc, rs, es, cnt, bad, None)
    for ib in (0, 1, 3, 16, -2):
        assert count(ib, 1, 4, 5) == -1 and "id_bytes" in err(), ib
        assert lib.selftok_token_to_u16(p, ib, 1, 4, 4, 1, p, p, None) == -1 and "id_bytes" in err(), ib
    for K, Cc in ((0, 5), (-1, 5), (4, 0), (4, -3), (1 << 16, 1 << 15)):
        assert count(4, 1, K, Cc) == -1 and ("K" in err()), (K, Cc)
        assert lib.selftok_token_census_workspace_bytes(K, Cc) == 0 and "token_census" in err()
        assert lib.selftok_token_census(p, K, Cc, p, p, 1 << 14, None) == -1
    assert count(4, -1, 4, 5) == -1 and count(4, 1 << 30, 4, 5) == -1 and count(4, 1, 4, 5, rs=-1) == -1 and count(4, 1, 4, 5, es=-1) == -1
    assert count(4, 1, 4, 5, cnt=None) == -1 and "null" in err() and count(4, 1, 4, 5, bad=None) == -1 and count(4, 1, 4, 5, ids=None) == -1 and count(8, 1, 4, 5, ids=p + 4) == -1
    assert count(4, 0, 4, 5, ids=None) == 0                          # no rows: nothing to do, nothing launched
    assert lib.selftok_token_census_workspace_bytes(512, 32768) == 32768 * 8 and lib.selftok_token_census_workspace_bytes(1, 5) == 40
    assert lib.selftok_token_census(p, 4, 5, p, p, 39, None) == -1 and "workspace" in err()
    assert lib.selftok_token_census(p, 4, 5, p + 4, p, 40, None) == -1 and "aligned" in err() and lib.selftok_token_census(None, 4, 5, p, p, 40, None) == -1
    agree = lambda n, K, lo, hi, a=p, mp=p: lib.selftok_token_agree(a, p, n, K, lo, hi, mp, p, p, p, None)
    for K, lo, hi in ((40, 5, 4), (40, -1, 4), (40, 0, 41), (0, 0, 0), (65536, 0, 1)):
        assert agree(1, K, lo, hi) == -1 and "k_lo <= k_hi" in err(), (K, lo, hi)
        assert lib.selftok_token_nearest(p, 1, p, 1, K, lo, hi, 0, 0, p, p, p, 1 << 14, None) == -1 and "k_lo <= k_hi" in err()
    assert agree(-1, 40, 0, 40) == -1 and agree(1, 40, 0, 40, a=None) == -1 and agree(1, 40, 0, 40, mp=None) == -1 and agree(0, 40, 0, 40, a=None) == 0
    wn = lib.selftok_token_nearest_workspace_bytes
    # one 64-bit key per query and reference split, at most min(64, tiles of 64 rows); it does not grow with M * N
    assert wn(10, 0) == 80 and wn(0, 5) == 8 and wn(100, 64) == 800 and wn(100, 65) == 1600 and wn(10000, 100000) == 64 * 10000 * 8 and wn(-1, 5) == 0 and wn(5, -1) == 0
    near = lambda M, N, K=40, lo=0, hi=40, ex=0, split=0, q=p, ws=p, wb=1 << 14, out=p: lib.selftok_token_nearest(q, M, p, N, K, lo, hi, ex, split, out, p, ws, wb, None)
    assert near(100, 65, wb=1599) == -1 and "workspace" in err() and near(5, 5, ex=-1) == -1 and near(5, 5, split=-1) == -1 and "split" in err()
    assert near(5, 5, q=None) == -1 and "null" in err() and near(5, 5, out=None) == -1 and near(5, 5, ws=None) == -1 and near(5, 5, ws=p + 4) == -1 and "aligned" in err()
    assert near(0, 5, q=None, ws=None, out=None) == 0                # no query: nothing to do
    assert (x == 0x5A5A5A5A).all()                                   # a refused call leaves its outputs untouched
    t = torch.zeros(8, 40, dtype=torch.int64)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_count(t, torch.zeros(40, 5, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_census(torch.zeros(40, 5, dtype=torch.int32))
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_to_u16(t)
    u = torch.zeros(8, 40, dtype=torch.uint16)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_agree(u, u)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        ops.token_nearest(u, u)
    assert "oracle" not in open(os.path.join(ROOT, "selftoktokenizer_amd", "tokenstats.py")).read().replace("the arithmetic of record", "")


def test_token_census_row_limit_merge_save_load(tmp_path):
    c = TS.TokenCensus(4, 5)
    c.rows = TS.ROW_LIMIT - 2
    with pytest.raises(ValueError, match="limit"):                   # decided on the host, before the device is touched: a counter can never wrap
        c.update(np.zeros((3, 4), np.int64))
    with pytest.raises(ValueError, match=r"\[\.\.\., 4\]"):
        c.update(np.zeros((3, 5), np.int64))
    with pytest.raises(TypeError):
        c.update([[0, 1, 2, 3]])
    for K, Cc in ((0, 5), (4, 0), (1 << 16, 1 << 15)):
        with pytest.raises(ValueError, match="K >= 1"):
            TS.TokenCensus(K, Cc)
    assert TS.ROW_LIMIT == 2 ** 32 - 1 and TS.TokenCensus(512).C == 32768
    rng = np.random.default_rng(5)
    a, b = TS.TokenCensus(4, 5), TS.TokenCensus(4, 5)
    ca, cb = rng.integers(0, 1000, size=(4, 5)).astype(np.uint32), rng.integers(0, 1000, size=(4, 5)).astype(np.uint32)
    ca[:, 2] = cb[:, 2] = 0
    a._host, a.rows, a._host_bad = ca.copy(), 1000, 3
    b._host, b.rows, b._host_bad = cb.copy(), 999, 4
    a.save(str(tmp_path / "a.npz"))
    a2 = TS.TokenCensus.load(str(tmp_path / "a.npz"))
    assert np.array_equal(a2.counts(), ca) and a2.counts().dtype == np.uint32 and (a2.rows, a2.bad_ids(), a2.K, a2.C) == (1000, 3, 4, 5)
    a2.merge(b)
    assert np.array_equal(a2.counts(), ca + cb) and (a2.rows, a2.bad_ids()) == (1999, 7) and np.array_equal(b.counts(), cb)
    assert np.array_equal(a2.dead_codes(), [2])
    a2.save(str(tmp_path / "ab.npz"))
    assert np.array_equal(TS.TokenCensus.load(str(tmp_path / "ab.npz")).counts(), ca + cb)
    with pytest.raises(ValueError, match="differ"):
        a2.merge(TS.TokenCensus(4, 6))
    big = TS.TokenCensus(4, 5)
    big.rows = TS.ROW_LIMIT - 999
    with pytest.raises(ValueError, match="limit"):
        big.merge(a)
    assert TS.nearest_chunk(100000) == TS.NEAREST_WS_BYTES // (8 * 64) and TS.nearest_chunk(10) == TS.NEAREST_WS_BYTES // 8 and TS.nearest_chunk(10, 7) == 7
