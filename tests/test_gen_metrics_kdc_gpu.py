"""gpu: the count / nearest entry and the KID sums (csrc/gen_metrics_kdc.hip) against the fp64 restatement of tests/gen_metrics_kdc_cases.py under the derived
brackets and bounds, their bit-for-bit properties (run to run, every column split, a query or a subset alone against in the batch, permutations, the lowest
index on equal bits, NaN rows, guard bands, hipGraph replay), the same d2 bits as the membership and radius entries, and the harness (genmetrics.kid /
density_coverage, compare_sets, tools/eval_generated.py).  The lines printed with -s are profiles/gen_metrics_kdc_bound.txt.

Measured on an MI355X: nn_d2 reaches 0.0009 - 0.146 of the bound E = (D + 5) 2^-24 (|u|^2 + |v|^2) (0.007 - 0.146 at D = 16, 0.0009 - 0.010 at D = 2048), every count is inside its
bracket and every clear nearest neighbour is the fp64 argmin; a KID sum reaches at most 0.029 of its T (m = 2; at most 0.001 from m = 127 on), mmd2 at most 0.0046 of its gate."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import fid_cases as FC
import gen_metrics_cases as GC
import gen_metrics_kdc_cases as KC
from selftoktokenizer_amd import _lib, evaluate as E, fid as FD, genmetrics as GM, ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLITS = (1, 2, 3, 5, 64)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(a, b):
    """equal bits, NaN payloads aside"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind != "f":
        return a.shape == b.shape and np.array_equal(a, b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(np.nan_to_num(a, nan=0.0)), bits(np.nan_to_num(b, nan=0.0)))


def guarded(t, guard=4096, fill=float("nan")):
    """`t` as a view inside a larger filled allocation (16-byte aligned): a read that strays turns outputs into NaN, a write is seen in the band"""
    buf = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device="cuda")
    buf[guard:guard + t.numel()] = t.reshape(-1)
    return buf, buf[guard:guard + t.numel()].view(t.shape)


def band_intact(buf, n, guard=4096, fill=None):
    ok = torch.isnan if fill is None else (lambda v: v == fill)
    return bool(ok(buf[:guard]).all()) and bool(ok(buf[guard + n:]).all())


def count_nn(X, A, r2=None, **kw):
    """(count | None, nn_d2, nn_idx) as numpy"""
    t = lambda v: v if v is None or isinstance(v, torch.Tensor) else dev(v)
    return tuple(None if o is None else o.cpu().numpy() for o in ops.manifold_count_nn(t(X), t(A), t(r2), **kw))


def same3(a, b):
    return all((x is None and y is None) or same(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_count_and_nearest_inside_the_brackets_and_bit_for_bit(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    r2 = KC.r2_f32(name)                                           # the same fp32 array on both sides: only d2 carries error
    nbytes = _lib.load().selftok_manifold_count_nn_f32_workspace_bytes(c.M, c.N, c.D)
    assert nbytes > 0
    x_buf, x = guarded(dev(X))
    a_buf, a = guarded(dev(A))
    r_buf, r = guarded(dev(r2))
    c_buf, oc = guarded(torch.full((c.M,), -7, dtype=torch.int32, device="cuda"), fill=-7)
    d_buf, od = guarded(torch.full((c.M,), 7.5, device="cuda"), fill=7.5)
    i_buf, oi = guarded(torch.full((c.M,), -7, dtype=torch.int32, device="cuda"), fill=-7)
    ws_buf, ws = guarded(torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda"), fill=0x5A)      # exactly the stated size: nothing beyond is touched
    got = tuple(o.cpu().numpy() for o in ops.manifold_count_nn(x, a, r, out_count=oc, out_d2=od, out_idx=oi, workspace=ws))
    assert band_intact(x_buf, X.size) and band_intact(a_buf, A.size) and band_intact(r_buf, c.N) and band_intact(ws_buf, nbytes, fill=0x5A)
    assert band_intact(c_buf, c.M, fill=-7) and band_intact(d_buf, c.M, fill=7.5) and band_intact(i_buf, c.M, fill=-7)
    cnt, nd, ni = got
    assert cnt.shape == nd.shape == ni.shape == (c.M,) and cnt.dtype == np.int32 and nd.dtype == np.float32 and ni.dtype == np.int32
    if c.M == 0:
        return
    lo, hi = KC.count_brackets(X, A, r2)
    want_d, want_i = KC.nearest(X, A)
    clear, e_row = KC.nearest_clear(X, A)
    assert (lo <= cnt).all() and (cnt <= hi).all(), "count outside its bracket"
    assert np.array_equal(np.isnan(nd), np.isnan(want_d)) and np.array_equal(ni < 0, np.isnan(want_d))
    ok = ~np.isnan(want_d)
    share = float((np.abs(nd[ok] - want_d[ok]) / e_row[ok]).max()) if ok.any() else 0.0
    print(f"\ncount / nearest {name}: M {c.M} N {c.N} D {c.D}: sum count {int(cnt.sum())} in [{int(lo.sum())}, {int(hi.sum())}], largest |nn_d2 - fp64| / E = {share:.4f}, "
          f"{int((~clear).sum())} unclear neighbours, {int((ni[clear] == want_i[clear]).sum())} of {int(clear.sum())} clear ones equal")
    assert share <= 1.0 and (nd[ok] >= 0).all() and ((ni[ok] >= 0) & (ni[ok] < c.N)).all()
    assert np.array_equal(ni[clear], want_i[clear]), "a clear nearest neighbour is the fp64 argmin"
    if c.margin:
        assert (hi - lo).sum() <= KC.CAP * max(hi.sum(), 1)        # conditions on the inputs (the CPU test holds them on the reference alone)
    if c.kind.startswith("clusters"):                              # decided outright: the integers
        assert np.array_equal(cnt, KC.counts(X, A, r2)) and int(cnt.sum()) == KC.density(A, X, r2, c.k)[1]
    assert np.array_equal(cnt > 0, ops.manifold_member(x, a, r).cpu().numpy() != 0), "count > 0 is the membership entry bit for bit"
    none = count_nn(x, a)
    assert none[0] is None and same(none[1], nd) and same(none[2], ni), "without radii the nearest neighbours are unchanged"
    assert same3(count_nn(x, a, r), got), "run to run"
    for s in SPLITS:                                               # every launch shape: the bits never depend on the column split
        assert same3(count_nn(x, a, r, split=s), got), f"split {s}"
        assert same3(count_nn(x, a, split=s), none), f"split {s}, no radii"
    for i in sorted({0, c.M // 2, c.M - 1}):                       # a query alone is the query in the batch
        one_buf, one = guarded(x[i:i + 1])
        alone = count_nn(one, a, r)
        assert alone[0][0] == cnt[i] and same(alone[1], nd[i:i + 1]) and alone[2][0] == ni[i], i
    if c.kind == "dups":                                           # bit-copied candidates give equal bits: the lowest index wins
        copies = 0
        for i in range(c.M):
            twins = np.flatnonzero((A == A[ni[i]]).all(1))
            assert ni[i] == twins[0], (i, ni[i], twins)
            copies += len(twins) > 1
        assert copies >= 10


@pytest.mark.parametrize("name", ["clusters_p1r0_d64", "clusters_p0r1_d2048", "scaled_n300_d64_k3", "wide_n300_d2048_k3", "edge_n641_d16_k3", "m1_n129_d64_k3"])
def test_density_and_coverage_end_to_end(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    r2 = KC.r2_f32(name)
    a, x, r = dev(A), dev(X), dev(r2)
    got = GM.density_coverage(a, x, c.k, r2_ref=r)
    assert set(got) == {"density", "coverage", "density_count", "coverage_count", "n_ref", "n_gen", "k"} and (got["n_ref"], got["n_gen"], got["k"]) == (c.N, c.M, c.k)
    assert got["density"] == got["density_count"] / (c.k * c.M) and got["coverage"] == got["coverage_count"] / c.N
    lo, hi = KC.count_brackets(X, A, r2)
    (_, dc), (_, cc) = KC.density(A, X, r2, c.k), KC.coverage(A, X, r2, c.k)
    settled = KC.coverage_settled(A, X, r2)
    decided = KC.coverage_decided(A, X, r2)
    print(f"\ndensity / coverage {name}: device counts {got['density_count']} / {got['coverage_count']}, fp64 {dc} in [{int(lo.sum())}, {int(hi.sum())}] / {cc} "
          f"({int((~decided).sum())} of {c.N} rows undecided, {int((~settled).sum())} unsettled)")
    assert lo.sum() <= got["density_count"] <= hi.sum() and abs(got["coverage_count"] - cc) <= (~settled).sum()
    nd = ops.manifold_count_nn(a, x)[1]                           # the rows themselves: every settled row as the fp64 reference has it, in fp32 <= on device values
    with np.errstate(invalid="ignore"):
        assert np.array_equal((nd <= r).cpu().numpy()[settled], (KC.nearest(A, X)[0] <= r2)[settled]) and int((nd <= r).sum().item()) == got["coverage_count"]
    if c.kind == "clusters_p1r0":                                  # wide reference, tight generated
        assert (got["density_count"], got["coverage_count"]) == (dc, cc) and got["density"] > 1.0 and 0 < cc < c.N // 2
    if c.kind == "clusters_p0r1":                                  # the reverse
        assert (got["density"], got["coverage"], got["density_count"], got["coverage_count"]) == (0.0, 0.0, 0, 0)
    if c.margin and name not in KC.NN_CAP_EXEMPT:
        assert (~decided).mean() <= KC.CAP
    own = GM.density_coverage(a, x, c.k)                           # with the device's own radii: each carries E, a pair within 2 E of its radius may fall either way
    with np.errstate(invalid="ignore"):
        slack = int((np.abs(GC.d2_matrix(X, A) - GC.radii(A, c.k)[None, :]) <= 2 * GC.bound(X, A)).sum())
    assert abs(own["density_count"] - dc) <= slack
    twin = GM.density_coverage(a, a, c.k)                          # identical sets: every row is inside its own ball and at least k others reach it or it them
    assert twin["coverage"] == 1.0 and twin["density"] >= 1.0


@pytest.mark.parametrize("name", ["wide_n300_d2048_k3", "edge_n1100_d16_k3", "dups_n130_d2048_k1"])
def test_candidates_and_queries_in_any_order(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    r2 = KC.r2_f32(name)
    cnt, nd, ni = count_nn(X, A, r2)
    clear, _ = KC.nearest_clear(X, A)
    g = np.random.default_rng(5)
    for _ in range(2):
        perm = g.permutation(c.N)
        pc, pd, pi = count_nn(X, A[perm], r2[perm])
        assert np.array_equal(pc, cnt) and same(pd, nd)
        back = perm[pi]
        assert np.array_equal(back[clear], ni[clear])              # where the minimum's bits are unique the index follows the permutation ...
        for i in np.flatnonzero(back != ni):                       # ... and where they are not, both answers are bit-copies of one row
            assert (A[back[i]] == A[ni[i]]).all(), i
    qperm = g.permutation(c.M)
    assert same3(count_nn(X[qperm], A, r2), (cnt[qperm], nd[qperm], ni[qperm]))


@pytest.mark.parametrize("name", ["edge_n257_d16_k3", "wide_n300_d2048_k3", "dups_n130_d16_k3", "k1_n300_d64"])
def test_nearest_of_a_row_without_itself_is_its_radius_for_k_1(name):
    """the same bits through both entries: nn_d2 of row j against the set without row j is selftok_knn_radius_f32(k = 1)[j]"""
    c = GC.BY_NAME[name]
    A, _ = GC.make(name)
    r1 = ops.knn_radius(dev(A), 1).cpu().numpy()
    for j in (0, 1, 2, 127, 128, c.N // 2, c.N - 1):
        rest = np.delete(A, j, axis=0)
        _, nd, ni = count_nn(A[j:j + 1], rest)
        assert same(nd, r1[j:j + 1]), j
        whole = count_nn(A[j:j + 1], A)                            # with itself in the set: one more candidate, the same bits for the others
        assert whole[1][0] <= nd[0] and whole[1][0] <= GC.bound(A[j:j + 1], A[j:j + 1])[0, 0]


def test_nan_rows_poison_only_themselves():
    c = GC.BY_NAME["nan_n200_d64_k3"]
    A, X = GC.make(c.name)
    r2 = KC.r2_f32(c.name)
    bad, qbad = np.isnan(A).any(1), np.isnan(X).any(1)
    cnt, nd, ni = count_nn(X, A, r2)
    assert np.array_equal(np.isnan(nd), qbad) and np.array_equal(ni == -1, qbad) and not cnt[qbad].any() and np.isnan(r2[bad]).all()
    keep = np.flatnonzero(~bad)
    cc, cd, ci = count_nn(X[~qbad], A[~bad], r2[~bad])             # the other queries: what they have against the set without the NaN rows
    assert np.array_equal(cnt[~qbad], cc) and same(nd[~qbad], cd) and np.array_equal(ni[~qbad], keep[ci])
    every = np.full(c.N, np.nan, np.float32)                       # every radius NaN: no comparison is true, the neighbours unchanged
    ec, ed, ei = count_nn(X, A, every)
    assert not ec.any() and same(ed, nd) and np.array_equal(ei, ni)
    only = count_nn(X, A[bad], r2[bad])                            # a set of NaN rows alone: no distance at all
    assert not only[0].any() and np.isnan(only[1]).all() and (only[2] == -1).all()


def _graph_equals_eager(call, refill):
    eager = [t.cpu().numpy() for t in call()]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = call()
    g.replay()
    torch.cuda.synchronize()
    assert all(same(o.cpu().numpy(), e) for o, e in zip(outs, eager))
    want = refill()                                                # the graph reads the tensors of its capture: new contents, new results
    g.replay()
    torch.cuda.synchronize()
    assert all(same(o.cpu().numpy(), e) for o, e in zip(outs, want))


def test_hipgraph_replay_equals_eager():
    c = GC.BY_NAME["edge_n641_d16_k3"]
    A, X = GC.make(c.name)
    a, x, r = dev(A), dev(X), dev(KC.r2_f32(c.name))

    def refill():
        want = count_nn(X[::-1].copy(), A, KC.r2_f32(c.name))
        x.copy_(dev(X[::-1].copy()))
        return want
    _graph_equals_eager(lambda: ops.manifold_count_nn(x, a, r), refill)
    k = KC.KID_BY_NAME["kid_m129_d16_s3"]
    xs_np, ys_np = KC.kid_make(k.name)
    xs, ys = dev(xs_np), dev(ys_np)

    def refill_kid():
        want = [ops.kid_sums(dev(ys_np), dev(xs_np), k.S, k.m).cpu().numpy()]
        xs.copy_(dev(ys_np)); ys.copy_(dev(xs_np))
        return want
    _graph_equals_eager(lambda: [ops.kid_sums(xs, ys, k.S, k.m)], refill_kid)


# ---- KID ----
@pytest.mark.parametrize("name", [c.name for c in KC.KID_CASES])
def test_kid_sums_under_the_derived_bound_and_bit_for_bit(name):
    c = KC.KID_BY_NAME[name]
    xs_np, ys_np = KC.kid_make(name)
    want, T = KC.kid_sums64(xs_np, ys_np, c.S, c.m), KC.kid_sum_bounds(xs_np, ys_np, c.S, c.m)
    nbytes = _lib.load().selftok_kid_sums_f32_workspace_bytes(c.S, c.m, c.D)
    assert nbytes == c.S * 3 * (-(-c.m // 128)) ** 2 * 8
    x_buf, xs = guarded(dev(xs_np))
    y_buf, ys = guarded(dev(ys_np))
    o_buf, out = guarded(torch.full((c.S, 3), float("nan"), dtype=torch.float64, device="cuda"))
    ws_buf, ws = guarded(torch.full((nbytes // 8,), float("nan"), dtype=torch.float64, device="cuda"))
    got = ops.kid_sums(xs, ys, c.S, c.m, out=out, workspace=ws).cpu().numpy()
    assert band_intact(x_buf, xs_np.size) and band_intact(y_buf, ys_np.size) and band_intact(o_buf, c.S * 3) and band_intact(ws_buf, nbytes // 8)
    assert got.shape == (c.S, 3) and got.dtype == np.float64
    live = ~np.isnan(want)
    assert np.array_equal(np.isnan(got), ~live), "a NaN row poisons the sums it enters and no other"
    share = float((np.abs(got - want)[live] / T[live]).max())
    rows = [s for s in range(c.S) if live[s].all()]
    gate = KC.mmd2_gate(T[rows], c.m)
    diff = np.abs(KC.mmd2_of(got[rows], c.m) - KC.mmd2_of(want[rows], c.m))
    print(f"\nkid {name}: S {c.S} m {c.m} D {c.D}: largest |sum - fp64| / T = {share:.4f} (T / |sum| up to {float((T[live] / np.abs(want[live])).max()):.2e}), "
          f"largest |mmd2 - fp64| / gate = {float((diff / gate).max()):.4f}")
    assert share <= 1.0 and (diff <= gate).all()
    if c.kind == "nan":
        assert np.array_equal(~live, np.array([[s == KC.NAN_SUBSET, False, s == KC.NAN_SUBSET] for s in range(c.S)]))
    assert same(ops.kid_sums(xs, ys, c.S, c.m).cpu().numpy(), got), "run to run"
    m = c.m
    for s in range(c.S):                                           # a subset alone is the subset among the others
        one_buf, one_x = guarded(xs[s * m:(s + 1) * m])
        assert same(ops.kid_sums(one_x, ys[s * m:(s + 1) * m].contiguous(), 1, m).cpu().numpy(), got[s:s + 1]), s
    if c.S > 1:                                                    # ... in any subset order
        order = [2, 0, 1]
        pick = torch.cat([torch.arange(s * m, (s + 1) * m) for s in order]).cuda()
        assert same(ops.kid_sums(xs[pick], ys[pick], c.S, m).cpu().numpy(), got[order])
    sym = ops.kid_sums(ys, xs, c.S, c.m).cpu().numpy()             # the two sets exchanged: XX and YY change places, XY is a sum over the same pairs in another order
    assert same(sym[:, 0], got[:, 1]) and same(sym[:, 1], got[:, 0])
    assert (np.abs(sym[:, 2] - got[:, 2])[live[:, 2]] <= 2 * T[:, 2][live[:, 2]]).all()


@pytest.mark.parametrize("case", KC.KID_SET_CASES)
def test_kid_figure_is_the_same_for_every_chunk(case):
    n_ref, n_gen, D, subsets, m = case
    ref_np, gen_np = KC.sets(n_ref, n_gen, D)
    want = KC.kid64(ref_np, gen_np, subsets, m, 2020)
    ref, gen = dev(ref_np), dev(gen_np)
    got = GM.kid(ref, gen, subsets, m, 2020)
    print(f"\nkid figure {case}: device {got['kid']:.12g} +- {got['kid_std']:.6g}, fp64 {want['kid']:.12g} +- {want['kid_std']:.6g}, "
          f"|difference| / gate {abs(got['kid'] - want['kid']) / want['gate'].mean():.4f}")
    assert set(got) == {"kid", "kid_std", "kid_subsets", "kid_subset_size", "kid_seed"} and (got["kid_subsets"], got["kid_subset_size"], got["kid_seed"]) == (subsets, m, 2020)
    assert abs(got["kid"] - want["kid"]) <= want["gate"].mean() and abs(got["kid_std"] - want["kid_std"]) <= want["gate"].max()
    for chunk in (1, 2, 3, subsets, 100):
        assert GM.kid(ref, gen, subsets, m, 2020, chunk=chunk) == got, chunk
    other = GM.kid(ref, gen, subsets, m, 2021)
    assert (other["kid"] != got["kid"] or m == min(n_ref, n_gen)) and other["kid_seed"] == 2021
    gi, ri = GM.kid_subsets(n_gen, n_ref, subsets, m, 2020)        # ... and is the direct call on the gathered rows
    sums = ops.kid_sums(gen[torch.from_numpy(gi.reshape(-1)).cuda()], ref[torch.from_numpy(ri.reshape(-1)).cuda()], subsets, m).cpu().numpy()
    assert GM.kid_of_sums(sums, m)[:2] == (got["kid"], got["kid_std"])


# ---- the harness ----
@pytest.fixture(scope="module")
def net():
    n = FD.InceptionNet.synthetic("cuda", logits=True)
    n.resize = False                                               # 75 x 75 images straight in
    return n


def _sets():
    ref = dev(FC.set_images("smooth"))
    gen = dev(FC.set_images("noise")).float() * 2.0 - 1.0
    return ref, gen


def test_compare_sets_equals_the_direct_calls_and_keeps_every_existing_key(net):
    ref, gen = _sets()
    n = FC.SET_N
    assert n == 24 and tuple(ref.shape[1:]) == (3, 75, 75)
    lr, lg = (lambda lo, hi: ref[lo:hi]), (lambda lo, hi: gen[lo:hi])
    base = E.compare_sets(lr, n, lg, n, fid=net, batch=n, split_size=10)
    full = E.compare_sets(lr, n, lg, n, fid=net, batch=7, split_size=10, metrics=E.COMPARE_METRICS + E.COMPARE_METRICS_EXTRA, kid_subset_size=8, kid_subsets=5)
    new = {"kid", "kid_std", "kid_subsets", "kid_subset_size", "kid_seed", "density", "coverage", "density_count", "coverage_count"}
    assert set(full) - set(base) == new and {k: v for k, v in full.items() if k not in new | {"batch"}} == {k: v for k, v in base.items() if k != "batch"}
    fr, fg = net.pool3(ref, True), net.pool3(gen, True)
    r2 = GM.knn_radii(fr, 3)
    dc = GM.density_coverage(fr, fg, 3)
    assert all(full[k] == dc[k] for k in ("density", "coverage", "density_count", "coverage_count")) and dc == GM.density_coverage(fr, fg, 3, r2_ref=r2)
    assert {k: full[k] for k in ("kid", "kid_std", "kid_subsets", "kid_subset_size", "kid_seed")} == GM.kid(fr, fg, 5, 8, GM.KID_SEED) and full["kid_seed"] == 2020
    count = ops.manifold_count_nn(fg, fr, r2)[0]                   # precision taken as count > 0 is the membership entry's figure
    assert full["precision_count"] == int((count > 0).sum()) == int(GM.manifold_members(fg, fr, r2).sum()) == base["precision_count"]
    assert full["metric_definition"]["gen_metrics"] == GM.GEN_METRICS_DEFINITION
    some = E.compare_sets(lr, n, lg, n - 5, fid=net, metrics=("kid", "coverage"), batch=5, k=2, kid_subset_size=19, kid_subsets=2, kid_seed=7)
    assert "fid" not in some and "density" not in some and "precision" not in some and some["k"] == 2 and (some["kid_subsets"], some["kid_subset_size"], some["kid_seed"]) == (2, 19, 7)
    assert some["coverage_count"] == GM.density_coverage(fr, fg[:n - 5], 2)["coverage_count"] and some["kid"] == GM.kid(fr, fg[:n - 5], 2, 19, 7)["kid"]
    only_p = E.compare_sets(lr, n, lg, n, fid=net, metrics=("precision", "coverage"), batch=n)
    assert only_p["precision_count"] == base["precision_count"] and "recall" not in only_p and only_p["coverage_count"] == full["coverage_count"]
    twin = E.compare_sets(lr, n, lr, n, fid=net, batch=7, metrics=("density", "coverage", "kid"), kid_subset_size=n, kid_subsets=2)
    assert twin["density"] >= 1.0 and twin["coverage"] == 1.0 and twin["coverage_count"] == n and twin["kid"] < full["kid"]


def test_nearest_returns_the_planted_copies(net):
    ref, gen = _sets()
    n = FC.SET_N
    gen = gen.clone()
    planted = {3: 17, 11: 0, 20: 23}                               # generated image -> the reference image it is a bit-copy of
    for gi, ri in planted.items():
        gen[gi] = ref[ri]
    out = E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: gen[lo:hi], n, fid=net, metrics=("fid",), batch=7, nearest=True)
    idx, d2 = out["nearest"]["index"], out["nearest"]["d2"]
    assert len(idx) == len(d2) == n and all(isinstance(v, int) for v in idx) and all(0 <= v < n for v in idx)
    fr, fg = net.pool3(ref, True), net.pool3(gen, True)
    ni, nd = GM.nearest_neighbours(fg, fr)
    assert idx == ni.cpu().tolist() and d2 == [float(v) for v in nd.cpu().numpy()]
    e = GC.bound(fg.cpu().numpy(), fr.cpu().numpy())
    for gi, ri in planted.items():
        assert idx[gi] == ri and d2[gi] <= e[gi, ri], (gi, idx[gi], d2[gi])
    with_density = E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: gen[lo:hi], n, fid=net, metrics=("density",), batch=n, nearest=True)
    assert with_density["nearest"] == out["nearest"] and "nearest" not in E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: gen[lo:hi], n, fid=net, metrics=("fid",), batch=n)


def test_eval_generated_tool_with_the_new_metrics(tmp_path):
    g = np.random.default_rng(11)
    smooth = np.clip(np.cumsum(g.integers(-6, 7, (9, 75, 75, 3)), axis=2) + 128, 0, 255).astype(np.uint8)
    noisy = g.integers(0, 256, (8, 75, 75, 3), dtype=np.uint8)
    noisy[5] = smooth[2]
    pa, pb, out, nn = str(tmp_path / "ref.npz"), str(tmp_path / "gen.npz"), str(tmp_path / "out.json"), str(tmp_path / "nn.npz")
    np.savez(pa, smooth); np.savez(pb, noisy)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_generated.py"), "--ref", pa, "--samples", pb, "--synthetic", "--no-resize", "--k", "2", "--batch", "4",
                        "--metrics", "fid,kid,density,coverage", "--kid-subsets", "3", "--kid-subset-size", "6", "--kid-seed", "5", "--nn-out", nn, "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line == json.load(open(out)) and line["tool"] == "eval_generated" and "nearest" not in line and line["nn_out"] == nn
    assert (line["n_ref"], line["n_gen"], line["k"], line["kid_subsets"], line["kid_subset_size"], line["kid_seed"]) == (9, 8, 2, 3, 6, 5)
    assert line["fid"] > 0 and line["kid_std"] >= 0 and 0 <= line["coverage"] <= 1 and line["density"] >= 0 and "is" not in line and "precision" not in line
    assert line["density_count"] == round(line["density"] * 2 * 8) and line["coverage_count"] == round(line["coverage"] * 9)
    with np.load(nn) as z:
        assert z["index"].shape == z["d2"].shape == (8,) and z["index"].dtype == np.int32 and z["d2"].dtype == np.float32 and z["index"][5] == 2 and z["d2"][5] == z["d2"].min()


def test_refusals_on_the_device():
    a = torch.zeros(8, 16, device="cuda")
    with pytest.raises(_lib.SelftokHipError, match="r2"):
        ops.manifold_count_nn(a, a, torch.zeros(7, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="multiple of 16"):
        ops.manifold_count_nn(torch.zeros(8, 24, device="cuda"), torch.zeros(8, 24, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="workspace"):
        ops.manifold_count_nn(a, a, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="out_count"):
        ops.manifold_count_nn(a, a, out_count=torch.zeros(8, dtype=torch.int32, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="out_idx"):
        ops.manifold_count_nn(a, a, out_idx=torch.zeros(8, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match=r"S \* m"):
        ops.kid_sums(a, a, 3, 4)
    with pytest.raises(_lib.SelftokHipError, match="m <="):
        ops.kid_sums(a, a, 8, 1)
    with pytest.raises(_lib.SelftokHipError, match="workspace"):
        ops.kid_sums(a, a, 2, 4, workspace=torch.zeros(8, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="subset_size"):
        GM.kid(a, a, 2, 9)
    empty = ops.manifold_count_nn(a[:0], a, torch.ones(8, device="cuda"))
    assert all(t.shape == (0,) for t in empty) and ops.manifold_count_nn(a[:0], a)[0] is None
    zeros = ops.manifold_count_nn(a, a, torch.zeros(8, device="cuda"))      # eight bit-copies at distance +0 with radius 0: every ball holds every query, the lowest index is nearest
    assert (zeros[0] == 8).all() and (zeros[1] == 0).all() and (zeros[2] == 0).all()
