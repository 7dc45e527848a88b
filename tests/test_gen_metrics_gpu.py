"""gpu: k-NN radii, manifold membership and the Inception Score reductions (csrc/gen_metrics.hip) against the fp64 restatement of tests/gen_metrics_cases.py
under the derived bound, their bit-for-bit properties (run to run, every launch-shape override, permutations, alone against in the batch, the exact tie through
both entries, NaN rows, guard bands, hipGraph replay), the fc logits under the standing gate, and the harness (compare_sets, evaluate's "precision_recall",
tools/eval_generated.py).

Measured on an MI355X (profiles/gen_metrics_bound.txt): the radii reach 0.003 - 0.12 of the bound E = (D + 5) 2^-24 (|u|^2 + |v|^2) (0.02 - 0.12 at D = 16, 0.003 - 0.010 at
D = 2048), every random membership case is inside the margin condition (1 undecided query of 129 on one D = 2048 case, 0 elsewhere), the Inception Score equals numpy fp64 to 15 digits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import edge_cases as EC
import fid_cases as FC
import gen_metrics_cases as GC
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
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(np.nan_to_num(a, nan=0.0)), bits(np.nan_to_num(b, nan=0.0)))


def guarded(t, guard=4096, fill=float("nan")):
    """`t` as a view inside a larger filled allocation (16-byte aligned): a read that strays turns outputs into NaN, a write is seen in the band"""
    buf = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device="cuda")
    buf[guard:guard + t.numel()] = t.reshape(-1)
    return buf, buf[guard:guard + t.numel()].view(t.shape)


def band_intact(buf, n, guard=4096, fill=None):
    ok = torch.isnan if fill is None else (lambda v: v == fill)
    return bool(ok(buf[:guard]).all()) and bool(ok(buf[guard + n:]).all())


def radii_dev(A, k, **kw):
    return ops.knn_radius(A if isinstance(A, torch.Tensor) else dev(A), k, **kw).cpu().numpy()


def members_dev(X, A, r2, **kw):
    t = lambda v: v if isinstance(v, torch.Tensor) else dev(v)
    return ops.manifold_member(t(X), t(A), t(r2), **kw).cpu().numpy()


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_radii_against_the_fp64_emulation_under_the_derived_bound(name):
    c = GC.BY_NAME[name]
    A, _ = GC.make(name)
    want = GC.radii(A, c.k)
    with np.errstate(invalid="ignore"):
        E_row = np.nanmax(GC.bound(A, A), axis=1)                  # the k-th order statistic moves by at most the largest perturbation of the row's distances
    nbytes = _lib.load().selftok_knn_radius_f32_workspace_bytes(c.N, c.D, c.k)
    a_buf, a = guarded(dev(A))
    out_buf, out = guarded(torch.full((c.N,), float("nan"), device="cuda"))
    ws_buf, ws = guarded(torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda"), fill=0x5A)      # exactly the stated size: nothing beyond is touched
    got = ops.knn_radius(a, c.k, out=out, workspace=ws).cpu().numpy()
    assert band_intact(a_buf, A.size) and band_intact(out_buf, c.N) and band_intact(ws_buf, nbytes, fill=0x5A)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN radii exactly on the rows that hold a NaN"
    ok = ~np.isnan(want)
    frac = float((np.abs(got[ok] - want[ok]) / E_row[ok]).max())
    print(f"\nradii {name}: N {c.N} D {c.D} k {c.k}: largest |device - fp64| / E = {frac:.4f} (E = (D + {GC.C_ERR}) 2^-24 (|u|^2 + |v|^2))")
    assert (got[ok] >= 0).all() and frac <= 1.0
    assert same(radii_dev(a, c.k), got), "run to run"
    for s in SPLITS:                                               # every launch shape: the bits never depend on the column split
        assert same(radii_dev(a, c.k, split=s), got), f"split {s}"
    if c.k < 8 and c.N > c.k + 1:                                  # the k-th and the (k + 1)-th are ordered, and k pads to the next list size without a trace
        assert (radii_dev(a, c.k + 1)[ok] >= got[ok]).all()


@pytest.mark.parametrize("name", [c.name for c in GC.CASES])
def test_membership_against_the_fp64_emulation_on_every_decided_query(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    r64 = GC.radii(A, c.k)
    r2 = r64.astype(np.float32)                                    # the reference's radii, rounded once (2^-24 r2, far inside E): the entry is tested on its own
    want, dec = GC.members(X, A, r2), GC.decided(X, A, r2)
    nbytes = _lib.load().selftok_manifold_member_f32_workspace_bytes(c.M, c.N, c.D)
    assert nbytes > 0
    x_buf, x = guarded(dev(X))
    a_buf, a = guarded(dev(A))
    r_buf, r = guarded(dev(r2))
    out_buf, out = guarded(torch.full((c.M,), -7, dtype=torch.int32, device="cuda"), fill=-7)
    ws_buf, ws = guarded(torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda"), fill=0x5A)
    got = ops.manifold_member(x, a, r, out=out, workspace=ws).cpu().numpy()
    assert band_intact(x_buf, X.size) and band_intact(a_buf, A.size) and band_intact(r_buf, c.N) and band_intact(out_buf, c.M, fill=-7) and band_intact(ws_buf, nbytes, fill=0x5A)
    assert got.shape == (c.M,) and set(np.unique(got)) <= {0, 1}
    undecided = 1.0 - dec.mean() if c.M else 0.0
    print(f"\nmembership {name}: {int(got.sum())} of {c.M} inside (fp64: {int(want.sum())}), {int((~dec).sum())} undecided ({100 * undecided:.2f} %)")
    if c.margin:
        assert undecided <= GC.UNDECIDED_MAX                       # a condition on the inputs (the CPU test holds it on the reference alone)
    assert np.array_equal(got[dec] != 0, want[dec])
    if c.kind.startswith("clusters"):
        assert dec.all() and int(got.sum()) == (c.M if c.kind == "clusters_p1r0" else 0)
    assert np.array_equal(members_dev(x, a, r), got), "run to run"
    for s in SPLITS:
        assert np.array_equal(members_dev(x, a, r, split=s), got), f"split {s}"
    for i in sorted({0, c.M // 2, c.M - 1} - {-1}) if c.M else ():  # a query alone is the query in the batch
        one_buf, one = guarded(x[i:i + 1])
        assert members_dev(one, a, r)[0] == got[i], i
    assert bool((GM.manifold_members(x, a, r).cpu().numpy() == (got != 0)).all())


@pytest.mark.parametrize("name", ["clusters_p1r0_d64", "clusters_p0r1_d2048", "scaled_n300_d64_k3"])
def test_precision_recall_end_to_end(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    want = GC.precision_recall(A, X, c.k)
    got = GM.precision_recall(dev(A), dev(X), c.k)
    print(f"\nprecision / recall {name}: device {got['precision_count']} / {got['recall_count']}, fp64 {want['precision_count']} / {want['recall_count']}")
    assert set(got) == {"precision", "recall", "precision_count", "recall_count", "n_ref", "n_gen", "k"} and (got["n_ref"], got["n_gen"], got["k"]) == (c.N, c.M, c.k)
    assert got["precision"] == got["precision_count"] / c.M and got["recall"] == got["recall_count"] / c.N
    if c.kind.startswith("clusters"):                              # decided outright: the counts are equal
        assert (got["precision_count"], got["recall_count"]) == (want["precision_count"], want["recall_count"]) == ((c.M, 0) if c.kind == "clusters_p1r0" else (0, c.N))
    else:                                                          # radii and distances both carry E: a query within 2 E of a radius may fall either way
        r_ref, r_gen = GC.radii(A, c.k), GC.radii(X, c.k)
        with np.errstate(invalid="ignore"):
            slack_p = int((np.abs(GC.d2_matrix(X, A) - r_ref[None, :]) <= 2 * GC.bound(X, A)).any(1).sum())
            slack_r = int((np.abs(GC.d2_matrix(A, X) - r_gen[None, :]) <= 2 * GC.bound(A, X)).any(1).sum())
        assert abs(got["precision_count"] - want["precision_count"]) <= slack_p and abs(got["recall_count"] - want["recall_count"]) <= slack_r
    same_set = GM.precision_recall(dev(A), dev(A), c.k)           # identical sets: every row sits at distance d2(u, u) <= its own ball
    assert same_set["precision"] == same_set["recall"] == 1.0


@pytest.mark.parametrize("name", ["wide_n300_d2048_k3", "edge_n1100_d16_k3", "dups_n130_d2048_k1"])
def test_a_rows_radius_inside_any_permutation(name):
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    base = radii_dev(A, c.k)
    g = np.random.default_rng(5)
    for _ in range(2):
        perm = g.permutation(c.N)
        assert same(radii_dev(A[perm], c.k), base[perm])
    r = dev(base)
    got = members_dev(X, A, r)
    perm = g.permutation(c.N)
    assert np.array_equal(members_dev(X, A[perm], dev(base[perm])), got)
    qperm = g.permutation(c.M)
    assert np.array_equal(members_dev(X[qperm], A, r), got[qperm])


@pytest.mark.parametrize("name", ["tie_n257_d64_k3", "tie_n129_d2048_k8"])
def test_the_exact_tie_query_through_both_entries(name):
    """query 0 is a bit-copy of the row that defines row 0's radius: the membership entry computes the very bits the radius entry selected, so d2 <= r2 holds
    with equality -- against row 0's ball ALONE the query is inside, and one ulp less radius puts it outside"""
    c = GC.BY_NAME[name]
    A, X = GC.make(name)
    r2 = radii_dev(A, c.k)
    a0, x0 = dev(A[:1]), dev(X[:1])
    assert GC.kth_neighbour(A, 0, c.k)[1] and r2[0] > 0 and members_dev(x0, a0, dev(r2[:1]))[0] == 1
    assert members_dev(x0, a0, dev(np.nextafter(r2[:1], np.float32(0))))[0] == 0
    whole = members_dev(X, A, dev(r2))
    assert whole[0] == 1 and not whole[1:].any()
    seen = 0
    for j in range(1, c.N, 7):                                     # the same through other rows: the query that copies ITS k-th neighbour
        nb, clear = GC.kth_neighbour(A, j, c.k)
        if not clear:
            continue                                               # the fp64 order of two neighbours closer than 2 E is not the device's to reproduce
        assert members_dev(A[nb:nb + 1], A[j:j + 1], dev(r2[j:j + 1]))[0] == 1, j
        assert members_dev(A[nb:nb + 1], A[j:j + 1], dev(np.nextafter(r2[j:j + 1], np.float32(0))))[0] == 0, j
        seen += 1
    assert seen >= 5


def test_nan_rows_poison_only_themselves():
    c = GC.BY_NAME["nan_n200_d64_k3"]
    A, X = GC.make(c.name)
    bad, qbad = np.isnan(A).any(1), np.isnan(X).any(1)
    r2 = radii_dev(A, c.k)
    assert np.array_equal(np.isnan(r2), bad)
    assert same(r2[~bad], radii_dev(A[~bad], c.k)), "the other rows' radii are those of the set without the NaN rows"
    got = members_dev(X, A, dev(r2))
    assert not got[qbad].any()
    assert np.array_equal(got[~qbad], members_dev(X[~qbad], A[~bad], dev(r2[~bad])))
    rr = r2.copy(); rr[~bad] = np.nan                              # every radius NaN: no comparison is true
    assert not members_dev(X, A, dev(rr)).any()


def test_hipgraph_replay_equals_eager():
    c = GC.BY_NAME["edge_n257_d16_k3"]
    A, X = GC.make(c.name)
    a, x = dev(A), dev(X)
    logits = dev(GC.make_logits(300, GC.CLASSES))

    def call():
        r = ops.knn_radius(a, c.k)
        q = ops.is_colmean(logits, 128)
        return r, ops.manifold_member(x, a, r), ops.is_kl_rows(logits, q, 128)
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
    assert all(same(o.cpu().numpy(), e) if e.dtype.kind == "f" else np.array_equal(o.cpu().numpy(), e) for o, e in zip(outs, eager))
    a.copy_(dev(A[::-1].copy()))
    g.replay()
    torch.cuda.synchronize()
    assert same(outs[0].cpu().numpy(), eager[0][::-1])             # the graph reads the tensors of its capture: new contents, new results


# ---- Inception Score ----
@pytest.mark.parametrize("N,split,C", GC.IS_CASES)
def test_inception_score_against_numpy_fp64(N, split, C):
    x = GC.make_logits(N, C)
    want, tol = GC.inception_score(x, split), GC.is_tolerance(x, split)
    lib = _lib.load()
    S = -(-N // split)
    nb_q, nb_k = lib.selftok_is_colmean_workspace_bytes(N, C, split), lib.selftok_is_kl_rows_workspace_bytes(N, C, split)
    x_buf, xd = guarded(dev(x))
    wq_buf, wq = guarded(torch.full((nb_q // 8,), float("nan"), dtype=torch.float64, device="cuda"))
    wk_buf, wk = guarded(torch.full((nb_k // 8,), float("nan"), dtype=torch.float64, device="cuda"))
    q = ops.is_colmean(xd, split, workspace=wq)
    kl = ops.is_kl_rows(xd, q, split, workspace=wk)
    assert band_intact(x_buf, x.size) and band_intact(wq_buf, nb_q // 8) and band_intact(wk_buf, nb_k // 8)
    p = GC.softmax64(x)
    qn, kln = q.cpu().numpy(), kl.cpu().numpy()
    rel = (C + min(split, N) + 8) * 2.0 ** -52                     # is_tolerance's per-element term, both sides
    for s in range(S):
        rows = slice(s * split, min((s + 1) * split, N))
        assert np.abs(qn[s] - p[rows].mean(0)).max() <= rel * p[rows].mean(0).max() and abs(qn[s].sum() - 1.0) <= rel
        assert np.abs(kln[rows] - GC.kl_rows(p[rows], p[rows].mean(0))).max() <= tol / want
    got = GM.inception_score(xd, split)
    print(f"\ninception score N {N} split {split} C {C}: device {got:.15f}, numpy fp64 {want:.15f}, |difference| / tolerance {abs(got - want) / tol:.4f}")
    assert abs(got - want) <= tol
    assert got == GM.inception_score(xd, split) and same(ops.is_kl_rows(xd, ops.is_colmean(xd, split), split).cpu().numpy(), kln)      # run to run
    if N > 17:                                                     # a row's KL depends on its split alone: the first split on its own
        first = dev(x[:split])
        assert same(ops.is_colmean(first, split).cpu().numpy(), qn[:1]) and same(ops.is_kl_rows(first, q[:1].contiguous(), split).cpu().numpy(), kln[:split])


def test_uniform_logits_give_exactly_one():
    for N, split in ((2, 5000), (17, 1), (300, 1), (4, 2)):       # every split's column sums are exact there (one row, or p + p): q = p bit for bit, every term log p - log q = 0
        for v in (0.0, -3.25, 11.0):
            x = torch.full((N, GC.CLASSES), v, device="cuda")
            assert GM.inception_score(x, split) == 1.0, (N, split, v)
    x = torch.full((300, GC.CLASSES), 0.5, device="cuda")         # any other shape: 1 up to the rounding of the column sums
    assert abs(GM.inception_score(x, 128) - 1.0) <= 300 * 2.0 ** -52


@pytest.fixture(scope="module")
def net():
    n = FD.InceptionNet.synthetic("cuda", logits=True)
    n.resize = False                                               # 75 x 75 images straight in, as the emulation of the two sets does
    return n


def test_logits_against_fp64_under_the_standing_gate(net):
    sd = FD.InceptionNet.synthetic_fc_tensors()
    w, b = sd["fc.weight"], sd["fc.bias"]
    f = torch.from_numpy(np.abs(np.random.default_rng(3).standard_normal((37, FD.FEATURES))).astype(np.float32))      # what a spatial mean of ReLU maps hands on
    ref = f.double() @ w.double().t() + b.double()
    cmp_acc = EC.ErrAcc(); cmp_acc.add(f @ w.t() + b, ref)
    rms_gate, max_gate = EC.gate(cmp_acc.rms, cmp_acc.mx)
    f_buf, fd = guarded(f.cuda())
    got = net.logits(fd)
    acc = EC.ErrAcc(); acc.add(got.cpu(), ref)
    print(f"\nfc logits: device rms {acc.rms:.3e} max {acc.mx:.3e} | torch-CPU fp32 rms {cmp_acc.rms:.3e} max {cmp_acc.mx:.3e} (gate 2 x rms, 4 x max)")
    assert got.shape == (37, FD.CLASSES) and band_intact(f_buf, f.numel()) and acc.rms <= rms_gate and acc.mx <= max_gate
    for i in (0, 36):                                              # a row alone: the bits it has in the batch
        assert torch.equal(net.logits(fd[i:i + 1]), got[i:i + 1])
    assert net.logits(fd[:0]).shape == (0, FD.CLASSES)
    with pytest.raises(_lib.SelftokHipError, match="logits=True"):
        FD.InceptionNet.synthetic("cuda").logits(fd)


# ---- the harness ----
def _sets():
    ref = dev(FC.set_images("smooth"))
    gen = dev(FC.set_images("noise")) * 2.0 - 1.0
    return ref, gen


def test_compare_sets_equals_the_direct_calls(net):
    ref, gen = _sets()
    n = FC.SET_N
    full = E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: gen[lo:hi].cpu(), n, fid=net, batch=n, split_size=10)
    fr, fg = net.pool3(ref, True), net.pool3(gen, True)
    pf, lg = net.features(gen, True)
    assert torch.equal(pf, fg) and torch.equal(lg, net.logits(fg))
    pr = GM.precision_recall(fr, fg, 3)
    assert full["fid"] == FD.frechet_distance(*FD.statistics(fg), *FD.statistics(fr)) and full["fid_rank_deficient"] is True
    assert full["is"] == GM.inception_score(lg, 10) and full["split_size"] == 10 and full["is"] > 1.0
    assert all(full[k] == pr[k] for k in ("precision", "recall", "precision_count", "recall_count", "k")) and (full["n_ref"], full["n_gen"]) == (n, n)
    assert full["metric_definition"]["gen_metrics"] == GM.GEN_METRICS_DEFINITION and full["metric_definition"]["fid"] == FD.FID_DEFINITION
    assert full["metric_definition"]["weights"] == "synthetic" and full["metric_definition"]["resized"] is False
    ragged = E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: gen[lo:hi], n, fid=net, batch=7, split_size=10)       # 7 + 7 + 7 + 3
    assert {k: v for k, v in ragged.items() if k != "batch"} == {k: v for k, v in full.items() if k != "batch"}
    some = E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: gen[lo:hi], n - 5, fid=net, metrics=("precision", "is"), batch=5, k=2)
    assert "fid" not in some and "recall" not in some and some["k"] == 2 and some["n_gen"] == n - 5
    assert some["precision_count"] == GM.precision_recall(fr, fg[:n - 5], 2)["precision_count"] and some["is"] == GM.inception_score(lg[:n - 5], GM.SPLIT_SIZE)
    twin = E.compare_sets(lambda lo, hi: ref[lo:hi], n, lambda lo, hi: ref[lo:hi], n, fid=net, batch=7)
    assert abs(twin["fid"]) <= 1e-3 * float(FD.statistics(fr)[1].diagonal().sum()) and twin["precision"] == twin["recall"] == 1.0


class _SetPipe:
    """a stand-in tokenizer (evaluate only needs .device, .encoding, .decoding*): image i of the originals decodes to image i of the reconstruction set"""
    device = torch.device("cuda")

    def __init__(self):
        self.orig = dev(FC.set_images("smooth"))
        self.recon = dev(FC.set_images("noise")).to(torch.bfloat16)
        self.range = None

    def load(self, lo, hi):
        self.range = (lo, hi)
        return self.orig[lo:hi]

    def encoding(self, imgs, device=None):
        lo, hi = self.range
        return torch.arange(lo, hi)[:, None].repeat(1, 8)

    def decoding(self, ids, device=None, noise=None):
        return self.recon[torch.from_numpy(np.asarray(ids)[:, 0]).cuda()]


def test_evaluate_precision_recall_leaves_every_existing_key_unchanged(net):
    pipe, n = _SetPipe(), FC.SET_N
    base = E.evaluate(pipe, pipe.load, n, batch=n, metrics=("psnr", "ssim", "rfid"), fid=net)
    full = E.evaluate(pipe, pipe.load, n, batch=7, metrics=("psnr", "ssim", "rfid", "precision_recall"), fid=net)
    new = {"precision", "recall", "precision_count", "recall_count"}
    assert list(full) == list(base) and set(full["diffusion"]) - set(base["diffusion"]) == new
    assert {k: v for k, v in full["diffusion"].items() if k not in new} == base["diffusion"]
    assert {k: v for k, v in full["metric_definition"].items() if k != "precision_recall"} == base["metric_definition"]
    assert full["metric_definition"]["precision_recall"] == dict(GM.GEN_METRICS_DEFINITION, weights="synthetic", resized=False, n=n)
    pr = GM.precision_recall(net.pool3(pipe.orig, True), net.pool3(pipe.recon, False), 3)
    assert all(full["diffusion"][k] == pr[k] for k in new)
    only = E.evaluate(pipe, pipe.load, n, batch=n, metrics=("precision_recall",), fid=net)
    assert all(only["diffusion"][k] == pr[k] for k in new) and "rfid" not in only["diffusion"] and "rfid" not in only["metric_definition"]


def test_eval_generated_tool_on_a_tiny_npz_pair(tmp_path):
    g = np.random.default_rng(11)
    smooth = np.clip(np.cumsum(g.integers(-6, 7, (6, 75, 75, 3)), axis=2) + 128, 0, 255).astype(np.uint8)
    noisy = g.integers(0, 256, (5, 75, 75, 3), dtype=np.uint8)
    pa, pb, out = str(tmp_path / "ref.npz"), str(tmp_path / "gen.npz"), str(tmp_path / "out.json")
    np.savez(pa, smooth); np.savez(pb, noisy)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_generated.py"), "--ref", pa, "--samples", pb, "--synthetic", "--no-resize", "--k", "2",
                        "--split-size", "3", "--batch", "4", "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line == json.load(open(out)) and line["tool"] == "eval_generated" and line["fid_weights"] == "synthetic" and "unpinned" in line["pinned"]
    assert (line["n_ref"], line["n_gen"], line["k"], line["split_size"], line["batch"]) == (6, 5, 2, 3, 4)
    assert line["fid"] > 0 and line["is"] >= 1.0 and 0 <= line["precision"] <= 1 and 0 <= line["recall"] <= 1 and line["precision_count"] == round(line["precision"] * 5)


def test_refusals_on_the_device():
    a = torch.zeros(8, 16, device="cuda")
    with pytest.raises(_lib.SelftokHipError, match="N > k"):
        ops.knn_radius(a[:3], 3)
    with pytest.raises(_lib.SelftokHipError, match="k <= 8"):
        ops.knn_radius(a, 9)
    with pytest.raises(_lib.SelftokHipError, match="multiple of 16"):
        ops.knn_radius(torch.zeros(8, 24, device="cuda"), 3)
    with pytest.raises(_lib.SelftokHipError, match="r2"):
        ops.manifold_member(a, a, torch.zeros(7, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="workspace"):
        ops.knn_radius(a, 3, workspace=torch.zeros(16, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.SelftokHipError, match="colmean"):
        ops.is_kl_rows(a, torch.zeros(1, 16, device="cuda"), 8)
    assert ops.manifold_member(a[:0], a, torch.ones(8, device="cuda")).shape == (0,)
