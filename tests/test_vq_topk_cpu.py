"""not gpu: the VQ top-k lookup pinned on the host -- the extension header against the ctypes table, the kernel file's scratch budget, the case
table's claims, the emulation of tests/vq_topk_cases.py against the argmax oracle, the planted mistakes every case that can see them must
show, the reference's own top-1 / top-2 goldens, and the host-side surface (tokens.margins, refusals decided before any launch)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import vq_topk_cases as T
from oracle import clib
from selftoktokenizer_amd import _lib, ops, tokens, weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW_ENTRIES = {"selftok_vq_topk_workspace_bytes", "selftok_vq_topk_packed_f32"}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_ext_header_declares_the_topk_entries():
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


def test_vq_topk_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "vq_topk.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", r.stderr)]
    # main kernel: RT in {1, 2, 4} x K in {1, 2, 4, 8}; finalize: two id types x four K
    assert len(kernels) == 12 + 8 and len(scratch) == len(kernels) == len(lds), (kernels, scratch, lds)
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    assert max(lds) == 2 * 8 * 2048, dict(zip(kernels, lds))               # the double-buffered chunk of 8 code tiles


def test_case_table_holds_the_edges_it_claims():
    assert {c.C for c in T.CASES} == {32, 64, 8192, 32768} and {c.N for c in T.CASES} >= {1, 31, 32, 33, 127, 128, 129, 513}
    assert T.KS == (1, 2, 3, 8) and len({c.name for c in T.CASES}) == len(T.CASES)
    for C in (32, 64, 8192, 32768):
        assert {c.name.rsplit("_N", 1)[0] for c in T.CASES if c.C == C} >= {"random", "dups", "one_stream", "ulp_ties"}
    half, tile = lambda c: (c >> 2) & 1, lambda c: c >> 5
    seen = set()
    for case in T.CASES:
        z, cb, plan = T.make(case)
        ids, sc = T.case_ref(case, 8)
        kind = case.name.rsplit("_N", 1)[0]
        seen.add(kind)
        if kind == "dups":
            for r, g in plan["dups"].items():
                assert ids[r, :min(len(g), 8)].tolist() == g[:8] and len(set(bits(sc[r, :min(len(g), 8)]).tolist())) == 1, (case.name, r)
            groups = sorted(plan["dups"].values(), key=len)
            nine = groups[-1]
            assert len(nine) == 9 and (case.C < 2048 or {c * 8 // case.C for c in nine} == set(range(8)))        # one in each of 8 code splits
            assert {half(c) for c in nine} == {0, 1} and tile(nine[0]) == 0 and tile(nine[-1]) == (case.C >> 5) - 1
            if case.N > 1:
                a, b = groups[0], groups[1]
                assert tile(a[0]) == tile(a[1]) and half(a[0]) == half(a[1])                                        # inside one lane's 16 codes
                assert tile(b[0]) == tile(b[1]) and half(b[0]) != half(b[1])                                        # across the wave halves
                if case.C >= 64:
                    c_, d = groups[2], groups[3]
                    assert tile(c_[0]) != tile(c_[1]) and half(c_[0]) == half(c_[1]) and c_[1] - c_[0] == 32        # two tiles of one stream
                    assert tile(d[0]) == 0 and tile(d[1]) == (case.C >> 5) - 1                                      # first and last split
        if kind == "one_stream":
            last = (case.C >> 5) - 1
            assert sorted(ids[0, :8].tolist()) == [0, 1, 2, 3, 8, 9, 10, 11] and len(set(bits(sc[0]).tolist())) == 8
            nine = T.topk_ref(z[:2], cb, 9)[0]
            assert case.C == 32 or (tile(nine[0, 8]) == last and half(nine[0, 8]) == 1)                             # the 9th best: another stream, the last split
            if case.N > 1:
                assert {(tile(c), half(c)) for c in ids[1, :8].tolist()} == {(last, 1)} and (case.C == 32 or tile(nine[1, 8]) == last - 1)
        if kind == "zero_row":
            r = plan["zero_row"]
            assert ids[r].tolist() == list(range(8)) and (bits(sc[r]) == 0).all()
        if kind == "nan_row":
            r = plan["nan_row"]
            assert ids[r].tolist() == list(range(8)) and (bits(sc[r]) == T.QNAN).all()
            assert case.N == 1 or not np.isnan(sc[np.arange(case.N) != r]).any()
        if kind == "nonfinite_codes":
            C = case.C
            assert ids[0, :4].tolist() == [6, C // 2 + 1, C // 2 + 9, C - 3] and (bits(sc[0, :4]) == T.QNAN).all() and np.isfinite(sc[0, 4:]).all()
            if case.N > 2:
                assert ids[1, :2].tolist() == [6, C - 3] and np.isinf(sc[1, 2]) and sc[1, 2] > 0 and ids[1, 2] in (C // 2 + 1, C // 2 + 9)
                assert (bits(sc[case.N - 1]) == T.QNAN).all() and ids[case.N - 1].tolist() == list(range(8))
            raw = T.scores_of(z, cb)
            assert case.N == 1 or (np.isneginf(raw).any() and np.isposinf(raw).any())
        if kind == "signed_zeros":
            raw = bits(T.scores_of(z[:1], cb)[0])
            want = plan["signed_zeros"]
            assert raw[want[0]] == 0x80000000 == raw[want[2]] and raw[want[1]] == 0
            assert ids[0, :3].tolist() == want and (bits(sc[0, :3]) == 0).all() and (sc[0, 3:] < 0).all()
        if kind == "ulp_ties":
            for r, codes in plan["ulp"].items():
                assert sorted(ids[r].tolist() + [int(T.topk_ref(z[r:r + 1], cb, 9)[0][0, 8])]) == codes
                step = np.diff(bits(sc[r]).astype(np.int64))
                assert set(step.tolist()) == {0, -1} and (step == 0).sum() == 2                                   # single ulps and two exact ties
                assert all(ids[r, i] < ids[r, i + 1] for i in np.flatnonzero(step == 0))
            codes = plan["ulp"][0]
            assert {half(c) for c in codes} == {0, 1} and len({tile(c) for c in codes}) == (1 if case.C == 32 else 2 if case.C == 64 else 9)
    assert seen == {"random", "dups", "one_stream", "zero_row", "nan_row", "nonfinite_codes", "signed_zeros", "ulp_ties"}


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_column_0_of_the_emulation_is_the_argmax_oracle(case):
    """ids as they are; score bits as they are except the two rewrites the device's `best` output makes as well: -0.0 -> +0.0, NaN -> 0x7FC00000"""
    z, cb, _ = T.make(case)
    ids, sc = T.case_ref(case, 1)
    ids0, best = clib.vq_encode(z, cb)
    want = bits(best + np.float32(0)).copy()
    want[np.isnan(best)] = T.QNAN
    assert np.array_equal(ids[:, 0], ids0) and np.array_equal(bits(sc[:, 0]), want)
    for k in T.KS[1:]:                                                       # the order is total: smaller k is a prefix
        a, b = T.topk_ref(z[:2], cb, k)
        assert np.array_equal(a, T.case_ref(case, 8)[0][:2, :k]) and np.array_equal(bits(b), bits(T.case_ref(case, 8)[1][:2, :k]))


def test_the_kernels_list_algorithm_restated_on_the_oracle_scores_equals_the_order_of_record():
    """per-stream sorted lists with a strict compare, half merge, split merge (tests/vq_topk_cases.py: kernel_walk_row) == topk_ref on the planted rows and
    the edge rows of every case with C <= 8192, on the path (fast / exact) the kernel would take, for k and split counts that change the stream structure"""
    seen = 0
    for case in T.CASES:
        if case.C > 8192:
            continue
        z, cb, plan = T.make(case)
        x, sc = clib.l2norm16(z), T.scores_of(z, cb)
        ids, ss = T.case_ref(case, 8)
        book_bad = not (np.abs(cb) < 1e18).all()
        rows = {0, case.N - 1} | {r for v in plan.values() if isinstance(v, dict) for r in v} | {v for v in plan.values() if isinstance(v, int)}
        for r in sorted(rows)[:5]:
            exact = book_bad or not (np.abs(x[r]) < 1e18).all()
            for K, split in ((8, 1), (2, 3), (4, 64)) if case.C <= 64 or r in (0, 1) else ((8, 8),):
                got_ids, got_bits = T.kernel_walk_row(sc[r], K, split, exact)
                assert got_ids == ids[r, :K].tolist() and got_bits == bits(ss[r, :K]).tolist(), (case.name, r, K, split)
                seen += 1
    assert seen >= 60


MUTS = {T.MUT_TIES_DESC: "ties", T.MUT_NAN_LAST: "nan", T.MUT_UNSTABLE: "ties"}


@pytest.mark.parametrize("mut", list(MUTS), ids=list(MUTS))
def test_every_case_that_can_see_a_planted_mistake_shows_it(mut):
    seen = 0
    for case in T.CASES:
        z, cb, _ = T.make(case)
        ids, sc = T.case_ref(case, 8)
        bad_ids, bad_sc = T.topk_ref(z, cb, 8, mut=mut)
        changed = not (np.array_equal(ids, bad_ids) and np.array_equal(bits(sc), bits(bad_sc)))
        if MUTS[mut] in case.tags:
            assert changed, f"{case.name} does not see {mut}"
            seen += 1
        elif not case.tags:
            assert not changed, f"{case.name} has no ties and no NaN scores, yet {mut} changes it"
    assert seen >= 3


@pytest.mark.parametrize("name", ["pipeline_b16", "encode_b64"])
def test_emulation_against_the_references_top2_goldens(name):
    """the reference's (normalize(z) @ codebook.T).topk(2): `tokens`, runner-up `id2`, `gap`.  Its scores come from a library GEMM in another summation
    order: each score of unit vectors in 16 dimensions errs by at most 16 x 2^-24, a gap differences two of them on each side -> 4 x 16 x 2^-24.
    id2 may differ only where the emulated second-to-third gap is below that bound, and at most 1 % of the tokens may be excused so."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    cb = W._synth_tensor("encoder.quantizer._codebook.embed", (1, 32768, 16), "cpu")[0].contiguous().numpy()
    ids, sc = T.topk_ref(g["z"].reshape(-1, 16), cb, 3)
    bound = 4 * 16 * 2.0 ** -24
    tok, id2, gap = (g[k].reshape(-1) for k in ("tokens", "id2", "gap"))
    assert np.array_equal(ids[:, 0], tok.astype(np.int64))
    margin = tokens.margins(sc)
    err = np.abs(margin.astype(np.float64) - gap.astype(np.float64))
    differ = ids[:, 1] != id2.astype(np.int64)
    gap23 = sc[:, 1].astype(np.float64) - sc[:, 2].astype(np.float64)
    print(f"\n{name}: {tok.size} tokens, max |margin - gap| {err.max():.3e} (bound {bound:.3e}), runner-up differs at {int(differ.sum())} tokens, "
          f"their 2nd-to-3rd gaps {np.sort(gap23[differ])[:8]}, smallest margin {margin.min():.3e}")
    assert err.max() <= bound
    assert (gap23[differ] < bound).all()
    assert differ.sum() <= 0.01 * tok.size


def test_margins_and_host_side_refusals_without_a_gpu():
    s = np.array([[[0.9, 0.5, 0.1], [0.25, 0.25, -1.0]]], np.float32)
    assert np.array_equal(tokens.margins(s), s[..., 0] - s[..., 1]) and tokens.margins(s).shape == (1, 2)
    assert torch.equal(tokens.margins(torch.from_numpy(s)), torch.from_numpy(s[..., 0] - s[..., 1]))
    with pytest.raises(ValueError):
        tokens.margins(s[..., :1])
    lib = _lib.load()
    assert lib.selftok_vq_topk_workspace_bytes(32768, 32768, 2) == 64 * 32768 * 2 * 8
    assert lib.selftok_vq_topk_workspace_bytes(513, 8192, 3) == 64 * 513 * 4 * 8 and lib.selftok_vq_topk_workspace_bytes(0, 64, 8) == 2 * 1 * 8 * 8
    assert lib.selftok_vq_topk_workspace_bytes(7, 32, 1) == 7 * 8 and lib.selftok_vq_topk_workspace_bytes(7, 32, 5) == 7 * 8 * 8
    for N, C, k in ((7, 32, 0), (7, 32, 9), (7, 48, 2), (7, 0, 2), (-1, 32, 2)):
        assert lib.selftok_vq_topk_workspace_bytes(N, C, k) == 0 and "vq_topk_workspace_bytes" in lib.selftok_last_error().decode()
    x = np.zeros(16 * 4, np.float32)
    p = x.ctypes.data
    for (N, C, D, k), word in (((4, 32, 16, 0), "k must be in 1..8"), ((4, 32, 16, 9), "k must be in 1..8"), ((4, 32, 8, 2), "D == 16"), ((4, 40, 16, 2), "C % 32 == 0"),
                               ((-1, 32, 16, 2), "N < 0")):
        assert lib.selftok_vq_topk_packed_f32(p, p, p, p, p, N, C, D, k, 0, None) == -1
        assert word in lib.selftok_last_error().decode(), (word, lib.selftok_last_error().decode())
    assert lib.selftok_vq_topk_packed_f32(None, p, p, p, p, 4, 32, 16, 2, 0, None) == -1 and "null" in lib.selftok_last_error().decode()
    assert lib.selftok_vq_topk_packed_f32(None, None, None, None, None, 0, 32, 16, 2, 0, None) == 0         # empty batch: nothing to do
    t = torch.zeros(4, 16)
    with pytest.raises(_lib.SelftokHipError):
        ops.vq_topk(t, t, 2)                                                                                 # CPU tensors: there is no CPU fallback
