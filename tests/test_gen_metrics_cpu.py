"""not gpu: the generative-metric definitions of record (tests/gen_metrics_cases.py) pinned on the host -- the fp64 emulation against a brute-force double loop,
what the case table claims to hold, the planted mistakes it must be able to see, the margin condition of the membership cases on the reference alone, the new
C entries against the ctypes table, the kernels' scratch budget, the host-side refusals and the fc head of the weight-file loader."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import gen_metrics_cases as GC
from selftoktokenizer_amd import _lib, evaluate as E, fid as FD, genmetrics as GM, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_knn_radius_f32", "selftok_manifold_member_f32", "selftok_is_colmean", "selftok_is_kl_rows", "selftok_knn_radius_f32_workspace_bytes",
               "selftok_manifold_member_f32_workspace_bytes", "selftok_is_colmean_workspace_bytes", "selftok_is_kl_rows_workspace_bytes"}


def _same_with_nan(a, b, tol):
    return np.array_equal(np.isnan(a), np.isnan(b)) and (np.abs(np.nan_to_num(a) - np.nan_to_num(b)) <= tol).all()


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_emulation_equals_the_brute_force_double_loop(name):
    """|u|^2 + |v|^2 - 2 u.v in fp64 against sum_k (u_k - v_k)^2 pair by pair; radii and memberships from a per-row python sort / loop"""
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    tol = 64 * 2.0 ** -53 * c.D * max((np.nan_to_num(A.astype(np.float64)) ** 2).sum(1).max(), (np.nan_to_num(X.astype(np.float64)) ** 2).sum(1).max(initial=0.0)) * 4
    daa = GC.d2_brute(A, A)
    assert _same_with_nan(GC.d2_matrix(A, A), daa, tol)
    want = np.empty(c.N)
    for j in range(c.N):
        others = sorted(v for i, v in enumerate(daa[j]) if i != j and v == v)
        want[j] = others[c.k - 1] if len(others) >= c.k else np.nan
    r2 = GC.radii(A, c.k)
    assert _same_with_nan(r2, want, tol)
    with_self = np.sort(np.where(np.isnan(daa), np.inf, daa), axis=1)[:, c.k] if c.kind != "nan" else None      # "entry k of the sorted row with self included"
    if with_self is not None and c.kind != "dups":               # (with duplicates self is not necessarily entry 0: the index rule is the definition)
        assert _same_with_nan(r2, with_self, tol)
    if c.M:
        dxa = GC.d2_brute(X, A)
        want_m = np.array([any(dxa[i, j] <= r2[j] for j in range(c.N)) for i in range(c.M)])
        dec = GC.decided(X, A, r2)
        assert np.array_equal(GC.members(X, A, r2)[dec], want_m[dec])           # a pair closer than the fp32 bound to its radius is nobody's to decide
    else:
        assert GC.members(X, A, r2).shape == (0,)


def test_the_case_table_holds_what_it_claims():
    names = [c.name for c in GC.CASES]
    assert len(set(names)) == len(names)
    assert {127, 128, 129, 255, 256, 257, 639, 640, 641} <= {c.N for c in GC.CASES}                  # the 128-row / 128-candidate tile and the split edge, +-1
    assert {(c.N, c.k) for c in GC.CASES} >= {(2, 1), (4, 3), (9, 8)}                                # N = k + 1
    assert {c.k for c in GC.CASES} == {1, 3, 8} and {c.D for c in GC.CASES} == {16, 64, 2048}
    assert {0, 1} <= {c.M for c in GC.CASES}
    assert {c.kind for c in GC.CASES} == {"random", "dups", "tie", "clusters_p1r0", "clusters_p0r1", "nan"}
    assert all(c.N > c.k and c.N <= 1100 and c.M <= 1100 for c in GC.CASES)
    for c in GC.CASES:
        A, X = GC.make(c.name)
        assert A.dtype == X.dtype == np.float32 and A.shape == (c.N, c.D) and X.shape == (c.M, c.D)
        r2 = GC.radii(A, c.k)
        if c.kind == "dups":                                     # zero distances and tied radii
            assert (A[2::3] == A[1:-1:3][: len(A[2::3])]).all() and (GC.d2_matrix(A, A)[2, 1] == 0.0)
            assert (r2 == 0.0).sum() >= (2 * ((c.N - 1) // 3) if c.k == 1 else 0) and len(np.unique(r2)) < c.N
        if c.kind == "tie":                                      # the query is a bit-copy of the row that defines a_0's radius: exactly on it, a member of that ball alone
            d0 = GC.d2_matrix(X[:1], A[:1])[0, 0]
            assert d0 == r2[0] and d0 > 0 and GC.members(X[:1], A[:1], r2[:1]).all() and not GC.members(X[:1], A[:1], r2[:1], "lt").any()
            assert any((X[0] == A[i]).all() for i in range(1, c.N)) and not GC.members(X[1:], A, r2).any()
            nb, clear = GC.kth_neighbour(A, 0, c.k)              # ... and no other row is within 2 E of being that neighbour: the device must select the same one
            assert clear and (X[0] == A[nb]).all()
        if c.kind.startswith("clusters"):
            pr = GC.precision_recall(A, X, c.k)
            assert (pr["precision"], pr["recall"]) == ((1.0, 0.0) if c.kind == "clusters_p1r0" else (0.0, 1.0))
            assert GC.decided(X, A, r2).all() and GC.decided(A, X, GC.radii(X, c.k)).all()      # decided outright: the device must give the same counts
        if c.kind == "nan":
            bad = np.isnan(A).any(1)
            assert bad.sum() == 2 and np.array_equal(np.isnan(r2), bad) and np.isnan(X).any()
            keep = ~bad                                          # a NaN row changes no other row's radius: the radii of the set without them
            assert np.array_equal(r2[keep], GC.radii(A[keep], c.k)) and not GC.members(X[np.isnan(X).any(1)], A, r2).any()


def test_margin_condition_holds_on_the_reference_alone():
    """every random membership case leaves at most 1 % of its queries closer than the fp32 bound to a radius -- a property of the inputs, checked in fp64 only"""
    seen = 0
    for c in GC.CASES:
        if not (c.margin and c.M):
            continue
        A, X = GC.make(c.name)
        for S, Q, kk in ((A, X, c.k),) + (((X, A, c.k),) if c.M > c.k else ()):            # both directions precision / recall walk
            share = 1.0 - GC.decided(Q, S, GC.radii(S, kk)).mean()
            assert share <= GC.UNDECIDED_MAX, (c.name, share)
            seen += 1
    assert seen >= 40 and all(c.margin for c in GC.CASES if c.kind == "random")
    assert GC.C_ERR == 5 and GC.bound(np.ones((1, 16), np.float32), np.ones((1, 16), np.float32))[0, 0] == pytest.approx(21 * 2.0 ** -24 * 32)


@pytest.mark.parametrize("mut", GC.MUTS)
def test_every_case_that_can_see_a_planted_mistake_sees_it(mut):
    seen = 0
    for c in GC.CASES:
        if not GC.mut_visible(mut, c):
            continue
        A, X = GC.make(c.name)
        r2 = GC.radii(A, c.k)
        if mut in ("self_included", "k_plus_1"):                 # most radii (the tied ones cannot) move by more than ten times the bound
            moved = GC.radii(A, c.k, mut)
            if c.N == c.k + 1 and mut == "k_plus_1":
                assert np.isnan(moved).all()                     # there is no (k + 1)-th neighbour
            else:
                far = np.abs(moved - r2) > 10 * GC.bound(A, A).max(1)          # the device test holds every radius to 1 x the bound
                assert far.mean() >= 0.3, (c.name, far.mean())
        elif mut == "lt":
            assert GC.members(X[:1], A[:1], r2[:1]).all() and not GC.members(X[:1], A[:1], r2[:1], mut).any()
        else:
            good, bad = GC.precision_recall(A, X, c.k), GC.precision_recall(A, X, c.k, mut)
            assert abs(good["precision_count"] - bad["precision_count"]) + abs(good["recall_count"] - bad["recall_count"]) >= 0.2 * min(c.N, c.M), (c.name, good, bad)
        seen += 1
    assert seen >= {"lt": 2, "swapped": 2, "query_radius": 2, "sqrt_radius": 2}.get(mut, 20), seen


@pytest.mark.parametrize("N,split,C", GC.IS_CASES)
def test_inception_score_emulation_and_its_planted_mistakes(N, split, C):
    x = GC.make_logits(N, C)
    want = GC.inception_score(x, split)
    assert 1.0 < want < C and N % split != 0                     # a partial split everywhere
    if N * C <= 20000:
        assert abs(GC.inception_score_brute(x, split) - want) <= 1e-12 * want
    tol = GC.is_tolerance(x, split)
    assert 0 < tol < 1e-9 * want
    for mut in GC.IS_MUTS:
        if GC.is_mut_visible(mut, N, split):
            assert abs(GC.inception_score(x, split, mut) - want) >= 1000 * tol, mut
        else:
            assert GC.inception_score(x, split, mut) == want
    assert GC.inception_score(np.zeros((7, C), np.float32), 3) == pytest.approx(1.0, abs=1e-12)
    assert sum(GC.is_mut_visible(m, n, s) for m in GC.IS_MUTS for n, s, _ in GC.IS_CASES) >= 12


def test_definition_of_record():
    d = GM.GEN_METRICS_DEFINITION
    assert d["k"] == 3 and d["k_max"] == 8 and d["split_size"] == 5000 and d["classes"] == 1008 == FD.CLASSES
    assert "never square-rooted" in d["distance"] and "by index" in d["radius"] and "<=" in d["membership"] and "last partial split included" in d["inception_score"]
    assert "not offered" in d["sfid"] and "unpinned" in d["pinned"] and "unpinned against the evaluator" in GM.__doc__
    assert E.COMPARE_METRICS == ("fid", "is", "precision", "recall")


def test_ext_header_declares_the_new_entries():
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
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_gen_metrics_compiles_for_gfx950_without_scratch_and_shares_the_pair_arithmetic(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "gen_metrics.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == len(scratch) == 15, kernels           # norms, pairs x (4 radius + 1 member), radius finalize x 4, member finalize, 4 Inception Score kernels
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert sum("gm_pairs_kernel" in k for k in kernels) == 5
    src = open(os.path.join(G.CSRC, "gen_metrics.hip")).read()
    shared = open(os.path.join(G.CSRC, "gen_metrics_shared.h")).read()
    code = "\n".join(l.split("//")[0] for l in src.splitlines())
    assert "asm" not in code and "atomic" not in code and "mfma" not in code and "fmaf" not in code        # the arithmetic lives in the shared header alone
    assert code.count("gm::pair_d2(") == 1 and code.count("gm::tile_dots(") == 1 and code.count("gm::row_norm(") == 1
    assert "mfma_f32_32x32x2f32" in shared and "pair_d2" in shared


def test_host_side_refusals_without_a_gpu():
    """every refusal is decided on the host before anything is launched"""
    lib = _lib.load()
    err = lambda: lib.selftok_last_error().decode()
    x = np.zeros(1 << 16, np.float32)
    d = np.zeros(4096)
    p, dp = x.ctypes.data, d.ctypes.data
    wr, wm = lib.selftok_knn_radius_f32_workspace_bytes, lib.selftok_manifold_member_f32_workspace_bytes
    # norms (rounded up to 256 bytes) + 2 parts per column split (at most min(64, tiles)) x N x k rounded up to 1, 2, 4, 8 x 4 bytes; it does not grow with N * N
    assert wr(4, 16, 3) == 256 + 2 * 1 * 4 * 4 * 4 and wr(300, 2048, 8) == 1280 + 2 * 3 * 300 * 8 * 4 and wr(50000, 2048, 3) == 200192 + 2 * 64 * 50000 * 4 * 4
    assert wm(0, 5, 16) > 0 and wm(300, 1100, 64) == 1280 + 4608 + 2 * 9 * 300 * 4
    for N, D, k in ((3, 16, 3), (4, 16, 0), (100, 16, 9), (100, 8, 3), (100, 24, 3), (100, 4096, 3), (1 << 27, 16, 3), (0, 16, 1)):
        assert wr(N, D, k) == 0 and "knn_radius" in err(), (N, D, k)
    for M, N, D in ((-1, 5, 16), (5, 0, 16), (5, 5, 20), (5, 5, 0), (1 << 27, 5, 16)):
        assert wm(M, N, D) == 0 and "manifold_member" in err(), (M, N, D)
    rad = lambda a, r, w, wb, N, D, k, s: lib.selftok_knn_radius_f32(a, r, w, wb, N, D, k, s, None)
    for args, word in (((None, p, p, 1 << 16, 100, 16, 3, 0), "null"), ((p, None, p, 1 << 16, 100, 16, 3, 0), "null"), ((p, p, None, 1 << 16, 100, 16, 3, 0), "null"),
                       ((p, p, p, 100, 100, 16, 3, 0), "workspace"), ((p, p, p, 1 << 16, 3, 16, 3, 0), "N > k"), ((p, p, p, 1 << 16, 100, 16, 9, 0), "k <= 8"),
                       ((p, p, p, 1 << 16, 100, 40, 3, 0), "multiple of 16"), ((p, p, p, 1 << 16, 100, 16, 3, -1), "split"), ((p + 4, p, p, 1 << 16, 100, 16, 3, 0), "aligned")):
        assert rad(*args) == -1 and word in err(), (args[3:], word, err())
    mem = lambda xx, a, r, m, w, wb, M, N, D, s: lib.selftok_manifold_member_f32(xx, a, r, m, w, wb, M, N, D, s, None)
    for args, word in (((None, p, p, p, p, 1 << 16, 5, 5, 16, 0), "null"), ((p, p, None, p, p, 1 << 16, 5, 5, 16, 0), "null"), ((p, p, p, None, p, 1 << 16, 5, 5, 16, 0), "null"),
                       ((p, p, p, p, p, 64, 5, 5, 16, 0), "workspace"), ((p, p, p, p, p, 1 << 16, 5, 5, 48 + 8, 0), "multiple of 16"), ((p, p, p, p, p, 1 << 16, 5, 0, 16, 0), "N >= 1"),
                       ((p, p, p, p, p, 1 << 16, 5, 5, 16, -2), "split"), ((p, p + 8, p, p, p, 1 << 16, 5, 5, 16, 0), "aligned")):
        assert mem(*args) == -1 and word in err(), (args[5:], word, err())
    assert mem(None, p, p, None, p, 1 << 16, 0, 5, 16, 0) == 0   # no query: nothing to do, nothing launched
    wc, wk = lib.selftok_is_colmean_workspace_bytes, lib.selftok_is_kl_rows_workspace_bytes
    assert wc(17, 1008, 5) == 17 * 16 + 4 * 1 * 1008 * 8 and wc(1100, 1008, 700) == 1100 * 16 + 2 * 3 * 1008 * 8 and wk(300, 1008, 128) == 300 * 16
    for N, C, s in ((0, 1008, 5), (5, 0, 5), (5, 1008, 0), (1 << 22, 1008, 5000), (70000, 16, 1)):
        assert wc(N, C, s) == 0 and "is_colmean" in err() and wk(N, C, s) == 0 and "is_kl_rows" in err(), (N, C, s)
    assert lib.selftok_is_colmean(None, dp, dp, 1 << 20, 5, 16, 5, None) == -1 and "null" in err()
    assert lib.selftok_is_colmean(p, dp, dp, 16, 5, 16, 5, None) == -1 and "workspace" in err()
    assert lib.selftok_is_colmean(p, dp + 4, dp, 1 << 20, 5, 16, 5, None) == -1 and "aligned" in err()
    assert lib.selftok_is_kl_rows(p, None, dp, dp, 1 << 20, 5, 16, 5, None) == -1 and "null" in err()
    assert lib.selftok_is_kl_rows(p, dp, dp, dp, 8, 5, 16, 5, None) == -1 and "workspace" in err()
    t = torch.zeros(8, 16)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        GM.knn_radii(t)
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        GM.manifold_members(t, t, torch.zeros(8))
    with pytest.raises(_lib.SelftokHipError, match="no CPU fallback"):
        GM.inception_score(t)
    with pytest.raises(_lib.SelftokHipError, match=r"\[rows, D\]"):
        ops.knn_radius(t.double())
    with pytest.raises(_lib.SelftokHipError, match="precision_recall"):
        GM.precision_recall(t, torch.zeros(8, 32))
    load = lambda lo, hi: torch.zeros(hi - lo, 3, 80, 80)
    net = FD.InceptionNet(FD.InceptionNet.synthetic_tensors(), "cpu", "synthetic")
    with pytest.raises(ValueError, match="precision_recall"):
        E.evaluate(type("P", (), {"device": torch.device("cpu")})(), load, 8, metrics=("psnr", "precision_recall"))          # without fid=: no default network
    with pytest.raises(ValueError, match="more than k"):
        E.evaluate(type("P", (), {"device": torch.device("cpu")})(), load, 3, metrics=("precision_recall",), fid=net)
    with pytest.raises(ValueError, match="fid="):
        E.compare_sets(load, 8, load, 8)
    with pytest.raises(ValueError, match="subset"):
        E.compare_sets(load, 8, load, 8, fid=net, metrics=("fid", "sfid"))
    with pytest.raises(ValueError, match="logits=True"):
        E.compare_sets(load, 8, load, 8, fid=net)
    with pytest.raises(ValueError, match="more than k"):
        E.compare_sets(load, 8, load, 3, fid=net, metrics=("precision",))
    with pytest.raises(ValueError, match="2 images"):
        E.compare_sets(load, 8, load, 1, fid=net, metrics=("fid",))
    with pytest.raises(_lib.SelftokHipError, match="logits=True"):
        net.logits(torch.zeros(2, 2048))


def test_from_files_reads_the_fc_head_and_refuses(tmp_path):
    sd = dict(FD.InceptionNet.synthetic_tensors(), **FD.InceptionNet.synthetic_fc_tensors())
    assert FD.fc_shapes() == {"fc.weight": (1008, 2048), "fc.bias": (1008,)} and not (set(FD.fc_shapes()) & set(FD.state_shapes())) and len(FD.state_shapes()) == 470
    mem = FD.InceptionNet(sd, "cpu", "synthetic", logits=True)
    assert tuple(mem.fc_packed.shape) == (2048, 1024) and torch.equal(mem.fc_packed[:, :1008], sd["fc.weight"].t()) and not mem.fc_packed[:, 1008:].any()
    assert torch.equal(mem.fc_bias, sd["fc.bias"]) and FD.InceptionNet(sd, "cpu", "synthetic").fc_packed is None
    p = str(tmp_path / "pt_inception-2015-12-05.pth")
    torch.save(dict(sd, **{"AuxLogits.fc.weight": torch.zeros(2)}), p)
    net = FD.InceptionNet.from_files(p, "cpu", logits=True)
    assert torch.equal(net.fc_packed, mem.fc_packed) and torch.equal(net.fc_bias, mem.fc_bias) and net.source == "pt_inception-2015-12-05.pth"
    assert FD.InceptionNet.from_files(p, "cpu").fc_packed is None                                   # the default still ignores fc.*
    torch.save({k: v for k, v in sd.items() if k != "fc.bias"}, p)
    assert FD.InceptionNet.from_files(p, "cpu").fc_packed is None
    with pytest.raises(KeyError, match="fc.bias"):
        FD.InceptionNet.from_files(p, "cpu", logits=True)
    torch.save(dict(sd, **{"fc.weight": torch.zeros(1000, 2048)}), p)
    assert FD.InceptionNet.from_files(p, "cpu").fc_packed is None
    with pytest.raises(ValueError, match="fc.weight"):
        FD.InceptionNet.from_files(p, "cpu", logits=True)


def test_index_noise_depends_on_the_index_alone():
    noise = E.index_noise(7, 4)
    whole = noise(0, 6)
    assert whole.shape == (6, 16, 4, 4) and noise(3, 3).shape == (0, 16, 4, 4)
    assert torch.equal(noise(2, 5), whole[2:5]) and torch.equal(torch.cat([noise(0, 1), noise(1, 6)]), whole)      # any batching, any shard boundary
    assert not torch.equal(whole[0], whole[1]) and torch.equal(E.index_noise(8, 4)(0, 1), whole[1:2]) and abs(float(whole.mean())) < 0.2
    src = open(os.path.join(ROOT, "tools", "eval_generated.py")).read()
    assert "E.index_noise(a.seed" in src and "manual_seed" not in src                             # the tool's --tokens route draws its noise this way


def test_npz_loader(tmp_path):
    arr = np.random.default_rng(0).integers(0, 256, (5, 8, 6, 3), dtype=np.uint8)
    p = str(tmp_path / "samples.npz")
    np.savez(p, arr)
    load, n = E.npz_loader(p)
    got = load(1, 4)
    assert n == 5 and got.shape == (3, 3, 8, 6) and got.dtype == torch.float32
    assert torch.equal(got, torch.from_numpy(arr[1:4]).permute(0, 3, 1, 2).float() / 127.5 - 1.0) and -1 <= got.min() and got.max() <= 1
    np.savez(p, arr.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        E.npz_loader(p)
    np.savez(p, other=arr)
    with pytest.raises(KeyError, match="arr_0"):
        E.npz_loader(p)
