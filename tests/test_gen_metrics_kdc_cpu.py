"""not gpu: the definitions of record of density / coverage, the nearest-neighbour entry and KID (tests/gen_metrics_kdc_cases.py) pinned on the host -- the fp64
emulations against brute-force double loops, what the case tables claim to hold, the caps on the inputs (bracket width, unclear neighbours, undecided coverage
rows) on the reference alone, the planted mistakes in both directions, the four C entries against the ctypes table, the kernels' resource budget and the
host-side refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gen_metrics_cases as GC
import gen_metrics_kdc_cases as KC
from selftoktokenizer_amd import _lib, evaluate as E, fid as FD, genmetrics as GM, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_manifold_count_nn_f32_workspace_bytes", "selftok_manifold_count_nn_f32", "selftok_kid_sums_f32_workspace_bytes", "selftok_kid_sums_f32"}


def _close(a, b, tol):
    return np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(np.nan_to_num(a) - np.nan_to_num(b)) <= tol).all()


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_count_and_nearest_emulations_equal_the_brute_force_double_loop(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    r2 = KC.r2_f32(name)
    if c.M == 0:
        assert KC.counts(X, A, r2).shape == (0,) and KC.nearest(X, A)[0].shape == (0,) and KC.count_brackets(X, A, r2)[0].shape == (0,)
        return
    tol = 64 * 2.0 ** -53 * c.D * max((np.nan_to_num(A.astype(np.float64)) ** 2).sum(1).max(), (np.nan_to_num(X.astype(np.float64)) ** 2).sum(1).max()) * 4
    lo, hi = KC.count_brackets(X, A, r2)
    got, brute = KC.counts(X, A, r2), KC.counts_brute(X, A, r2)
    assert (lo <= got).all() and (got <= hi).all() and (lo <= brute).all() and (brute <= hi).all()
    assert np.array_equal(got[lo == hi], brute[lo == hi])           # a pair closer than the fp32 bound to its radius is nobody's to decide
    nd, ni = KC.nearest(X, A)
    bd, bi = KC.nearest_brute(X, A)
    clear, _ = KC.nearest_clear(X, A)
    assert _close(nd, bd, tol) and np.array_equal(ni[clear], bi[clear]) and np.array_equal(ni < 0, np.isnan(nd))
    den, dc = KC.density(A, X, r2, c.k)
    cov, cc = KC.coverage(A, X, r2, c.k)
    assert dc == int(got.sum()) and den == dc / (c.k * c.M) and cov == cc / c.N
    settled = KC.coverage_settled(A, X, r2)
    cd, _ = KC.nearest_brute(A, X)
    with np.errstate(invalid="ignore"):
        assert np.array_equal((cd <= r2)[settled], (KC.nearest(A, X)[0] <= r2)[settled])
    assert settled[KC.coverage_decided(A, X, r2)].all()             # decided by the row's largest E implies settled pair by pair


def test_the_count_table_holds_what_it_claims():
    """the parent's table: the 128-row / 128-candidate tile +-1, the split edge, N = k + 1, M = 0 and 1, every D, and the planted kinds"""
    assert {127, 128, 129, 639, 640, 641} <= {c.N for c in GC.CASES} and {0, 1} <= {c.M for c in GC.CASES} and {c.D for c in GC.CASES} == {16, 64, 2048}
    assert {(c.N, c.k) for c in GC.CASES} >= {(2, 1), (4, 3), (9, 8)} and {129, 130, 257} <= {c.M for c in GC.CASES}
    assert {c.kind for c in GC.CASES} == {"random", "dups", "tie", "clusters_p1r0", "clusters_p0r1", "nan"}
    for c in GC.CASES:
        A, X = GC.make(c.name)
        r2 = KC.r2_f32(c.name)
        if c.kind == "dups":                                       # bit-copied candidates at distances of equal bits: the index rule decides, and the lowest wins
            nd, ni = KC.nearest(X, A)
            d = GC.d2_matrix(X, A)
            shared = np.array([(d[i] == nd[i]).sum() > 1 for i in range(c.M)])
            assert shared.sum() >= 10 and all(ni[i] == np.flatnonzero(d[i] == nd[i])[0] for i in range(c.M))
            assert (nd[::2] == 0.0).all()                          # queries that are bit-copies of rows
        if c.kind == "tie":                                        # the query on row 0's radius: counted by <=, not by <, in that ball alone
            exact = GC.radii(A, c.k)[:1]
            assert KC.counts(X[:1], A[:1], exact)[0] == 1 and KC.counts(X[:1], A[:1], exact, "lt")[0] == 0
        if c.kind.startswith("clusters"):                          # decided outright: brackets of width 0, every coverage row settled, the integers derived
            lo, hi = KC.count_brackets(X, A, r2)
            assert np.array_equal(lo, hi) and KC.coverage_settled(A, X, r2).all()
            (den, dc), (cov, cc) = KC.density(A, X, r2, c.k), KC.coverage(A, X, r2, c.k)
            if c.kind == "clusters_p1r0":                          # wide reference, tight generated: every tight row sits in many wide balls
                near = np.arange(c.N) < c.N // 2
                owns = np.array([(GC.d2_matrix(A[j:j + 1], X)[0] <= r2[j]).any() for j in range(c.N)])
                assert den > 1.0 and dc == int(KC.counts(X, A, r2).sum()) and cc == int(owns[near].sum()) > 0 and not owns[~near].any() and cov == cc / c.N
            else:                                                  # the reverse: no wide row inside a tight ball, no tight ball that reaches a wide row
                assert (den, dc, cov, cc) == (0.0, 0, 0.0, 0)
        if c.kind == "nan":
            qbad, bad = np.isnan(X).any(1), np.isnan(A).any(1)
            nd, ni = KC.nearest(X, A)
            assert qbad.any() and np.array_equal(np.isnan(nd), qbad) and np.array_equal(ni < 0, qbad) and not np.isin(ni, np.flatnonzero(bad)).any()
            assert not KC.counts(X, A, r2)[qbad].any()


def test_the_caps_hold_on_the_reference_alone():
    """conditions on the inputs, checked in fp64 only: on every random case the brackets are at most 1 % wide, at most 1 % of the queries have an unclear nearest
    neighbour and at most 1 % of the reference rows an undecided coverage"""
    seen, worst = 0, [0.0, 0.0, 0.0]
    for c in GC.CASES:
        if not (c.margin and c.M):
            continue
        A, X = GC.make(c.name)
        r2 = KC.r2_f32(c.name)
        lo, hi = KC.count_brackets(X, A, r2)
        width = (hi - lo).sum() / max(hi.sum(), 1)
        unclear = 1.0 - KC.nearest_clear(X, A)[0].mean()
        undecided = 1.0 - KC.coverage_decided(A, X, r2).mean()
        assert width <= KC.CAP, (c.name, width)
        if c.name in KC.NN_CAP_EXEMPT:
            assert (round(unclear * c.M), round(undecided * c.N)) == (1, 1)        # the stated exception: one query of 40, one row of 40
        else:
            assert unclear <= KC.CAP and undecided <= KC.CAP, (c.name, unclear, undecided)
            worst = [max(worst[0], width), max(worst[1], unclear), max(worst[2], undecided)]
        seen += 1
    print(f"\ncaps: worst bracket width {100 * worst[0]:.2f} %, unclear neighbours {100 * worst[1]:.2f} %, undecided coverage rows {100 * worst[2]:.2f} % over {seen} random cases")
    assert seen >= 20 and all(c.margin for c in GC.CASES if c.kind == "random") and KC.NN_CAP_EXEMPT == ("wide_n40_d2048_k3",)


@pytest.mark.parametrize("mut", KC.DC_MUTS)
def test_every_count_case_that_can_see_a_planted_mistake_sees_it(mut):
    seen = 0
    for c in GC.CASES:
        A, X = GC.make(c.name)
        r2 = KC.r2_f32(c.name)
        if not KC.dc_applies(mut, c):
            if c.M and c.kind != "nan" and mut in ("div_m", "highest_index"):      # ... and the other direction: blind by construction
                if mut == "div_m" and c.k == 1:
                    assert KC.density(A, X, r2, c.k, mut) == KC.density(A, X, r2, c.k)
                if mut == "highest_index" and c.kind == "random":
                    assert np.array_equal(KC.nearest(X, A, mut)[1], KC.nearest(X, A)[1])
            continue
        if mut == "lt":
            exact = GC.radii(A, c.k)[:1]
            assert KC.counts(X[:1], A[:1], exact)[0] == 1 and KC.counts(X[:1], A[:1], exact, mut)[0] == 0
        elif mut == "highest_index":
            moved = (KC.nearest(X, A, mut)[1] != KC.nearest(X, A)[1]).sum()
            assert moved >= 10, (c.name, moved)
        elif mut == "candidate_radius":
            gate = (~KC.coverage_settled(A, X, r2)).sum() / c.N
            move = abs(KC.coverage(A, X, r2, c.k, mut)[0] - KC.coverage(A, X, r2, c.k)[0])
            assert move > 0 and move >= KC.MOVE * gate, (c.name, move, gate)
        else:
            lo, hi = KC.count_brackets(X, A, r2)
            gate = (hi - lo).sum() / (c.k * c.M)
            move = abs(KC.density(A, X, r2, c.k, mut)[0] - KC.density(A, X, r2, c.k)[0])
            assert move > 0 and move >= KC.MOVE * gate, (c.name, move, gate)
        seen += 1
    assert seen >= {"lt": 2, "candidate_radius": 2, "highest_index": 2}.get(mut, 15), seen


@pytest.mark.parametrize("name", [c.name for c in KC.KID_CASES])
def test_kid_emulation_bound_and_planted_mistakes(name):
    c = KC.KID_BY_NAME[name]
    xs, ys = KC.kid_make(name)
    assert xs.shape == ys.shape == (c.S * c.m, c.D) and xs.dtype == ys.dtype == np.float32
    sums, T = KC.kid_sums64(xs, ys, c.S, c.m), KC.kid_sum_bounds(xs, ys, c.S, c.m)
    brute = KC.kid_sums_brute(xs, ys, c.S, c.m)
    live = ~np.isnan(sums)
    assert np.array_equal(np.isnan(brute), ~live) and (np.abs(brute - sums)[live] <= 1e-3 * T[live]).all()      # two fp64 orders: far inside the fp32 bound
    if c.kind == "nan":                                            # the NaN row poisons the sums it enters, XX and XY of its subset, and nothing else
        assert np.array_equal(~live, np.array([[s == KC.NAN_SUBSET, False, s == KC.NAN_SUBSET] for s in range(c.S)]))
        return
    assert live.all() and (T > 0).all() and (T <= 1e-3 * np.abs(sums)).all()
    if c.kind == "copies":                                         # bit-copied rows at two positions count: only the POSITION i = j is excluded
        k_self = (float(np.dot(xs[3].astype(np.float64), xs[3].astype(np.float64))) / c.D + 1.0) ** 3
        without = np.delete(np.arange(c.m), [7, c.m - 1])
        assert (xs[7] == xs[3]).all() and (xs[c.m - 1] == xs[3]).all() and sums[0, 0] > KC.kid_sums64(xs[without], ys[without], 1, c.m - 2)[0, 0] + 5 * k_self
    gate, good = KC.mmd2_gate(T, c.m), KC.mmd2_of(sums, c.m)
    for mut in KC.KID_SUM_MUTS:
        bad = KC.kid_sums64(xs, ys, c.S, c.m, mut)
        if not KC.kid_applies(mut, c):
            if c.m % 128 == 0:
                assert np.array_equal(bad, sums), mut              # padded by value at a subset that fills its tiles: invisible, as applies() says
            continue
        if mut in ("diag_included", "padded_by_value"):            # on every sum the mistake touches, against that sum's T
            touched = [0, 1] if mut == "diag_included" else [0, 1, 2]
            assert (np.abs(bad - sums)[:, touched] >= KC.MOVE * T[:, touched]).all(), (mut, (np.abs(bad - sums) / T).min())
            if mut == "diag_included":
                assert np.array_equal(bad[:, 2], sums[:, 2])
        else:
            assert (np.abs(KC.mmd2_of(bad, c.m, mut) - good) >= KC.MOVE * gate).all(), (mut, (np.abs(KC.mmd2_of(bad, c.m, mut) - good) / gate).min())


def test_the_kid_table_holds_what_it_claims():
    assert {c.m for c in KC.KID_CASES} == {2, 5, 127, 128, 129, 130, 257} and {c.D for c in KC.KID_CASES} == {16, 64, 2048} and {c.S for c in KC.KID_CASES} == {1, 3}
    assert {c.kind for c in KC.KID_CASES} == {"random", "copies", "nan"} and sum(c.scale == 8.0 for c in KC.KID_CASES) == 1
    assert sum(KC.kid_applies(m, c) for m in KC.KID_SUM_MUTS for c in KC.KID_CASES) >= 60
    ref, gen = KC.sets(400, 400, 64)
    assert np.linalg.matrix_rank(np.concatenate([ref, gen]).astype(np.float64), tol=1e-4) == 8              # one 8-dimensional subspace for both sets
    n_ref, n_gen = (ref.astype(np.float64) ** 2).sum(1).mean(), (gen.astype(np.float64) ** 2).sum(1).mean()
    assert abs(n_ref - 8.0) < 1.0 and abs(n_gen - 8.0 * (1.5 ** 2 + 1.0)) < 3.0                            # unit scale: N(0, I) and 1.5 N(0, I) + 1 in the basis


@pytest.mark.parametrize("case", KC.KID_SET_CASES)
def test_kid_figure_and_the_mistakes_of_its_tail(case):
    n_ref, n_gen, D, subsets, m = case
    ref, gen = KC.sets(n_ref, n_gen, D)
    good = KC.kid64(ref, gen, subsets, m, 2020)
    gi, ri = GM.kid_subsets(n_gen, n_ref, subsets, m, 2020)
    wi = KC.kid_draw(n_gen, n_ref, subsets, m, 2020)
    assert np.array_equal(gi, wi[0]) and np.array_equal(ri, wi[1])                                          # the product's draw is the emulation's
    mean, std, mmd2 = GM.kid_of_sums(KC.kid_sums64(gen[gi.reshape(-1)], ref[ri.reshape(-1)], subsets, m), m)
    assert (mean, std) == (good["kid"], good["kid_std"]) and np.array_equal(mmd2, good["mmd2"]) and std == float(np.std(good["mmd2"]))
    for mut in KC.KID_FIGURE_MUTS:
        bad = KC.kid64(ref, gen, subsets, m, 2020, mut)
        if not KC.kid_figure_applies(mut, case):
            continue
        if mut == "sample_std":                                    # np.std is 1-Lipschitz in the largest perturbation of its arguments
            assert bad["kid"] == good["kid"] and abs(bad["kid_std"] - good["kid_std"]) >= KC.MOVE * good["gate"].max()
        else:
            assert abs(bad["kid"] - good["kid"]) >= KC.MOVE * good["gate"].mean() and abs(bad["kid_std"] - good["kid_std"]) >= KC.MOVE * good["gate"].max()
    assert sum(KC.kid_figure_applies(mut, cs) for mut in KC.KID_FIGURE_MUTS for cs in KC.KID_SET_CASES) >= 4


def test_kid_subsets_is_deterministic_and_draws_in_the_stated_order():
    gi, ri = GM.kid_subsets(50, 40, 3, 7, 2020)
    assert gi.shape == ri.shape == (3, 7) and gi.dtype == ri.dtype == np.int64
    again = GM.kid_subsets(50, 40, 3, 7, 2020)
    assert np.array_equal(gi, again[0]) and np.array_equal(ri, again[1])
    rng = np.random.RandomState(2020)
    for s in range(3):                                             # per subset in order: the generated rows first, then the reference rows
        assert np.array_equal(gi[s], rng.choice(50, 7, replace=False)) and np.array_equal(ri[s], rng.choice(40, 7, replace=False))
    assert all(len(set(row)) == 7 for row in gi) and gi.max() < 50 and ri.max() < 40
    assert not np.array_equal(GM.kid_subsets(50, 40, 3, 7, 2021)[0], gi)
    more = GM.kid_subsets(50, 40, 5, 7, 2020)                     # a prefix: more subsets never change the earlier ones
    assert np.array_equal(more[0][:3], gi) and np.array_equal(more[1][:3], ri)
    for n_gen, n_ref, S, m in ((50, 40, 3, 1), (50, 40, 3, 41), (40, 50, 3, 41), (50, 40, 0, 7)):
        with pytest.raises(ValueError, match="subset_size"):
            GM.kid_subsets(n_gen, n_ref, S, m)
    assert GM.kid_chunk(1000, 2048) == 16 and 2 * 16 * 1000 * 2048 * 4 <= GM.KID_CHUNK_BYTES < 2 * 17 * 1000 * 2048 * 4 and GM.kid_chunk(1 << 20, 2048) == 1
    assert (GM.KID_SUBSETS, GM.KID_SUBSET_SIZE, GM.KID_SEED) == (100, 1000, 2020)


def test_definition_of_record():
    d = GM.GEN_METRICS_DEFINITION
    assert d["k"] == 3 == GM.K_DEFAULT and (d["kid_subsets"], d["kid_subset_size"], d["kid_seed"]) == (100, 1000, 2020)
    assert "<=" in d["count"] and "prdc compares with <" in d["count"] and "false against NaN" in d["count"]
    assert "lowest j" in d["nearest"] and "<< 32" in d["nearest"] and "-1" in d["nearest"]
    assert "k * M" in d["density"] and "REFERENCE row's own radius" in d["coverage"] and "once per compare_sets call" in d["radii"]
    assert "(u.v / D + 1)^3" in d["kid"] and "excluded by position" in d["kid"] and "m (m - 1)" in d["kid"] and "ddof 0" in d["kid"] and "RandomState" in d["kid"]
    assert "unpinned" in d["pinned_kdc"] and "unpinned against either package" in GM.__doc__
    assert E.COMPARE_METRICS == ("fid", "is", "precision", "recall") and E.COMPARE_METRICS_EXTRA == ("kid", "density", "coverage")


def test_ext_header_declares_the_four_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2]] for a in args]
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want and res == ctype_of[m.group(1)], (n, args)
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_kdc_compiles_for_gfx950_without_scratch_and_takes_its_arithmetic_from_the_shared_header(tmp_path):
    """recorded at this revision: 6 kernels; gm_count_nn_kernel<count> 167 VGPRs, 17920 bytes of LDS, 3 waves per SIMD (the 64-bit key and the count cost 29
    registers over the keys-only form's 138 and no wave of occupancy: gm_pairs_kernel runs at 3 too); <no count> 138 VGPRs, 17408 bytes, 3 waves; kid_tile_kernel
    118 VGPRs, 16928 bytes, 4 waves (its fp64 epilogue runs after the accumulators' last use as fp32: no wave lost); the norm and finalize kernels 8 - 14 VGPRs"""
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "gen_metrics_kdc.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    field = lambda what: [int(v) for v in re.findall(what + r": (\d+)", r.stderr)]
    scratch, vgprs, lds, occ = field(r"ScratchSize \[bytes/lane\]"), field(r" VGPRs"), field(r"LDS Size \[bytes/block\]"), field(r"Occupancy \[waves/SIMD\]")
    assert len(kernels) == len(scratch) == len(vgprs) == len(lds) == len(occ) == 6, kernels      # norms, count / nearest x (with, without radii), its finalize, KID tiles, KID finalize
    print("\n" + "\n".join(f"{k}: {v} VGPRs, {l} bytes LDS, {o} waves/SIMD" for k, v, l, o in zip(kernels, vgprs, lds, occ)))
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert sum("gm_count_nn_kernel" in k for k in kernels) == 2 and sum("kid_tile_kernel" in k for k in kernels) == 1
    for k, v, l, o in zip(kernels, vgprs, lds, occ):
        if "gm_count_nn_kernel" in k or "kid_tile_kernel" in k:
            assert o >= 3 and v <= 170 and l <= 18432, (k, v, l, o)      # three waves per SIMD, as gm_pairs_kernel
    src = open(os.path.join(G.CSRC, "gen_metrics_kdc.hip")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "asm" not in code and "atomic" not in code and "mfma" not in code and "fmaf" not in code        # the arithmetic lives in the shared header alone
    assert code.count("gm::pair_d2(") == 1 and code.count("gm::tile_dots(") == 2 and code.count("gm::row_norm(") == 1
    assert '#include "gen_metrics_shared.h"' in code and "fp contract(off)" in code


def test_host_side_refusals_and_workspace_sizes_without_a_gpu():
    """every refusal is decided on the host before anything is launched"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.zeros(1 << 16, np.float32)
    d = np.zeros(4096)
    p, dp = x.ctypes.data, d.ctypes.data
    wc, wk = lib.selftok_manifold_count_nn_f32_workspace_bytes, lib.selftok_kid_sums_f32_workspace_bytes
    # both norm arrays (rounded up to 256 bytes) + 2 parts per column split (at most min(64, tiles)) x M x (one 64-bit key + one count); it does not grow with M * N
    assert wc(300, 1100, 64) == 1280 + 4608 + 2 * 9 * 300 * 12 and wc(0, 5, 16) == 256 + 256 + 2 * 1 * 1 * 12 and wc(50000, 10000, 2048) == 200192 + 40192 + 2 * 64 * 50000 * 12
    # one fp64 per (subset, sum, 128 x 128 tile)
    assert wk(1, 2, 16) == 24 and wk(3, 129, 64) == 3 * 3 * 4 * 8 and wk(100, 1000, 2048) == 100 * 3 * 64 * 8
    for M, N, D in ((-1, 5, 16), (5, 0, 16), (5, 5, 20), (5, 5, 0), (5, 5, 4096), (1 << 27, 5, 16), (5, 1 << 27, 16)):
        assert wc(M, N, D) == 0 and "manifold_count_nn" in err(), (M, N, D)
    for S, m, D in ((0, 5, 16), (1, 1, 16), (1, 0, 16), (70000, 5, 16), (1, 5, 24), (1, 5, 4096), (1, (1 << 22) + 1, 16), (1 << 10, 1 << 17, 16)):
        assert wk(S, m, D) == 0 and "kid_sums" in err(), (S, m, D)
    cnt = lambda xx, a, r, c, nd, ni, w, wb, M, N, D, s: lib.selftok_manifold_count_nn_f32(xx, a, r, c, nd, ni, w, wb, M, N, D, s, None)
    for args, word in (((None, p, p, p, p, p, p, 1 << 16, 5, 5, 16, 0), "null"), ((p, None, p, p, p, p, p, 1 << 16, 5, 5, 16, 0), "null"),
                       ((p, p, p, p, None, p, p, 1 << 16, 5, 5, 16, 0), "null"), ((p, p, p, p, p, None, p, 1 << 16, 5, 5, 16, 0), "null"),
                       ((p, p, p, p, p, p, None, 1 << 16, 5, 5, 16, 0), "null"), ((p, p, p, None, p, p, p, 1 << 16, 5, 5, 16, 0), "exactly when r2"),
                       ((p, p, None, p, p, p, p, 1 << 16, 5, 5, 16, 0), "exactly when r2"), ((p, p, p, p, p, p, p, 64, 5, 5, 16, 0), "workspace"),
                       ((p, p, p, p, p, p, p, 1 << 16, 5, 5, 56, 0), "multiple of 16"), ((p, p, p, p, p, p, p, 1 << 16, 5, 0, 16, 0), "N >= 1"),
                       ((p, p, p, p, p, p, p, 1 << 16, 5, 5, 16, -2), "split"), ((p, p + 8, p, p, p, p, p, 1 << 16, 5, 5, 16, 0), "aligned"),
                       ((p, p, p, p, p, p, p + 8, 1 << 16, 5, 5, 16, 0), "aligned")):
        assert cnt(*args) == -1 and word in err(), (args[7:], word, err())
    assert cnt(None, p, None, None, None, None, p, 1 << 16, 0, 5, 16, 0) == 0                               # no query: nothing to do, nothing launched
    kid = lambda xs, ys, s, w, wb, S, m, D: lib.selftok_kid_sums_f32(xs, ys, s, w, wb, S, m, D, None)
    for args, word in (((None, p, dp, dp, 4096, 1, 5, 16), "null"), ((p, None, dp, dp, 4096, 1, 5, 16), "null"), ((p, p, None, dp, 4096, 1, 5, 16), "null"),
                       ((p, p, dp, None, 4096, 1, 5, 16), "null"), ((p, p, dp, dp, 16, 1, 5, 16), "workspace"), ((p, p, dp, dp, 4096, 1, 1, 16), "m <="),
                       ((p, p, dp, dp, 4096, 0, 5, 16), "S <="), ((p, p, dp, dp, 4096, 1, 5, 40), "multiple of 16"), ((p + 4, p, dp, dp, 4096, 1, 5, 16), "aligned"),
                       ((p, p, dp + 4, dp, 4096, 1, 5, 16), "aligned")):
        assert kid(*args) == -1 and word in err(), (args[4:], word, err())
    t = torch.zeros(8, 16)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        GM.nearest_neighbours(t, t)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        GM.density_coverage(t, t)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        GM.kid(t, t, 2, 4)
    with pytest.raises(_lib.SelftokHipError, match=r"\[rows, D\]"):
        ops.manifold_count_nn(t.double(), t)
    with pytest.raises(_lib.SelftokHipError, match="density_coverage"):
        GM.density_coverage(t, torch.zeros(8, 32))
    with pytest.raises(ValueError, match="subset_size"):
        GM.kid(t, t, 2, 9)
    with pytest.raises(ValueError, match="chunk"):
        GM.kid(t, t, 2, 4, chunk=0)


def test_compare_sets_accepts_and_refuses_the_right_names():
    load = lambda lo, hi: torch.zeros(hi - lo, 3, 80, 80)
    net = FD.InceptionNet(FD.InceptionNet.synthetic_tensors(), "cpu", "synthetic")
    assert E.COMPARE_METRICS == ("fid", "is", "precision", "recall") and E.COMPARE_METRICS_EXTRA == ("kid", "density", "coverage")
    for bad in (("fid", "sfid"), ("sfid",), ("kid", "mmd"), ()):
        with pytest.raises(ValueError, match="subset"):
            E.compare_sets(load, 8, load, 8, fid=net, metrics=bad)
    with pytest.raises(ValueError, match="kid_subset_size"):
        E.compare_sets(load, 8, load, 8, fid=net, metrics=("kid",))                                        # the default 1000 rows from 8 images
    with pytest.raises(ValueError, match="kid_subset_size"):
        E.compare_sets(load, 8, load, 8, fid=net, metrics=("kid",), kid_subset_size=1)
    with pytest.raises(ValueError, match="kid_subset_size"):
        E.compare_sets(load, 8, load, 6, fid=net, metrics=("kid",), kid_subset_size=7)
    with pytest.raises(ValueError, match="kid_subsets"):
        E.compare_sets(load, 8, load, 8, fid=net, metrics=("kid",), kid_subset_size=4, kid_subsets=0)
    with pytest.raises(ValueError, match="more than k reference"):
        E.compare_sets(load, 3, load, 8, fid=net, metrics=("density",))
    with pytest.raises(ValueError, match="more than k reference"):
        E.compare_sets(load, 8, load, 8, fid=net, metrics=("coverage",), k=9)
    with pytest.raises(ValueError, match="more than k"):
        E.compare_sets(load, 8, load, 3, fid=net, metrics=("precision", "density"))
    # accepted names get past the checks: the walk then needs device tensors
    for good in (("kid",), ("density", "coverage"), ("fid", "kid", "density", "coverage", "precision", "recall")):
        with pytest.raises(_lib.SelftokHipError, match="no CPU fallback|device"):
            E.compare_sets(load, 8, load, 8, fid=net, metrics=good, kid_subset_size=4, kid_subsets=2)
    src = open(os.path.join(ROOT, "tools", "eval_generated.py")).read()
    assert all(opt in src for opt in ("--kid-subsets", "--kid-subset-size", "--kid-seed", "--nn-out")) and 'default=",".join(E.COMPARE_METRICS)' in src
