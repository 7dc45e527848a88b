"""-m gpu: the token statistics (csrc/token_stats.hip, ops.token_*, selftoktokenizer_amd/tokenstats.py, tools/token_stats.py, tools/tokenize_folder.py --stats)
against the numpy emulations of tests/token_stats_cases.py.  Every check is an equality, except the two fp64 entropies: within TC.H_TOL = 1e-10 nats (derived in
the case file, not tuned), perplexity within 1e-10 relative.  Every output sits between guard bands of a sentinel pattern that must survive."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import token_stats_cases as TC
from selftoktokenizer_amd import _lib, evaluate as E, ops, synth, tokenstats as TS, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 64
SENT32, SENT16, SENT64 = 0x5A5A5A5A, 0xA5A5, 0x5A5A5A5A5A5A5A5A
WORST = {"H": 0.0, "ppl_rel": 0.0}


def guarded(n, np_dtype, sentinel):
    """(whole buffer, the n inner elements as a contiguous view) with PAD sentinel elements either side"""
    full = torch.from_numpy(np.full(n + 2 * PAD, sentinel, dtype=np_dtype)).cuda()
    return full, full[PAD:PAD + n]


def intact(full, n, sentinel):
    h = full.cpu().numpy()
    return bool((h[:PAD] == sentinel).all() and (h[PAD + n:] == sentinel).all())


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def device_view(c, base):
    tb = torch.from_numpy(base).cuda()
    return tb, tb[:, :c.K * c.es:c.es]


@pytest.mark.parametrize("name", [c.name for c in TC.COUNT_CASES])
def test_count_census_and_packing_equal_the_emulation(name):
    c = TC.COUNT_BY_NAME[name]
    base, view = TC.make_ids(name)
    tb, tv = device_view(c, base)
    assert tuple(tv.shape) == (c.N, c.K) and (c.N == 0 or tv.stride() == (c.K * c.es + c.rpad, c.es))
    want, want_bad = TC.count(view, c.C)
    n = c.K * c.C
    full, inner = guarded(n, np.int32, SENT32)
    fb, bad = guarded(1, np.int32, SENT32)
    inner.zero_(); bad.zero_()
    counts = inner.view(c.K, c.C)
    h = c.N // 2                                                    # two calls equal one call on the concatenation; the strided view is counted in place
    ops.token_count(tv[:h], counts, bad)
    ops.token_count(tv[h:], counts, bad)
    assert np.array_equal(u32(counts), want) and int(u32(bad)[0]) == want_bad and intact(full, n, SENT32) and intact(fb, 1, SENT32)
    assert torch.equal(tb.cpu(), torch.from_numpy(base))            # bad ids change nothing but `bad`
    # census: guard bands around the output and around a workspace of exactly the stated size
    lib = _lib.load()
    need = lib.selftok_token_census_workspace_bytes(c.K, c.C)
    assert need == c.C * 8
    fo, out = guarded((c.K + 1) * 5, np.float64, -7.25)
    fw, ws = guarded(need // 8, np.int64, SENT64)
    got = ops.token_census(counts, out.view(c.K + 1, 5), ws).cpu().numpy()
    ref = TC.census(want)
    assert np.array_equal(got[:, [0, 1, 4]], ref[:, [0, 1, 4]])
    dH = np.abs(got[:, 2:4] - ref[:, 2:4]).max()
    rel = np.abs(np.exp(got[:, 2:4]) / np.exp(ref[:, 2:4]) - 1.0).max()
    WORST["H"], WORST["ppl_rel"] = max(WORST["H"], float(dH)), max(WORST["ppl_rel"], float(rel))
    print(f"\n{name}: max |H - emulation| {dH:.3e} nats, perplexity {rel:.3e} relative")
    assert dH <= TC.H_TOL and rel <= TC.PPL_RTOL
    assert intact(fo, (c.K + 1) * 5, -7.25) and intact(fw, need // 8, SENT64) and np.array_equal(u32(counts), want)
    again = ops.token_census(counts)
    assert np.array_equal(again.cpu().numpy().view(np.uint64), got.view(np.uint64))          # the same bits run to run
    if c.kind in ("one_code", "equal"):
        assert (got[:, 2] == 0.0).all() and not np.signbit(got[:, 2]).any()
    if c.kind == "uniform":
        assert (got[:, 1] == c.C).all()
    if c.kind == "dead_pos":
        assert (got[0] == 0.0).all()
    # packing
    pw, pbad = TC.to_u16(view)
    fp, po = guarded(c.N * c.K, np.uint16, SENT16)
    bad.zero_()
    packed = ops.token_to_u16(tv, bad, po.view(c.N, c.K))
    assert np.array_equal(packed.cpu().numpy(), pw) and int(u32(bad)[0]) == pbad and intact(fp, c.N * c.K, SENT16) and intact(fb, 1, SENT32)


def test_a_replayed_graph_adds_exactly_twice():
    c = TC.COUNT_BY_NAME["n65_k40_c64_int64_es2"]
    base, view = TC.make_ids(c.name)
    tb, tv = device_view(c, base)
    want, _ = TC.count(view, c.C)
    counts, bad = torch.zeros(c.K, c.C, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.token_count(tv, counts, bad)                            # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    counts.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.token_count(tv, counts, bad)
    counts.zero_()
    g.replay(); g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(u32(counts), 2 * want)


@pytest.mark.parametrize("name", [c.name for c in TC.AGREE_CASES])
def test_agreement_equals_the_emulation(name):
    c = TC.AGREE_BY_NAME[name]
    a, b = TC.make_agree(name)
    ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    want = TC.agree(a, b, c.k_lo, c.k_hi)
    fm, mp = guarded(c.K, np.int32, SENT32)
    mp.zero_()
    rows = [guarded(c.N, np.int32, SENT32) for _ in range(3)]
    lib = _lib.load()
    p = lambda t: t.data_ptr() if t.numel() else None
    for rep in (1, 2):                                              # match_pos accumulates, the per-row outputs are written
        _lib.check(lib.selftok_token_agree(p(ta), p(tb), c.N, c.K, c.k_lo, c.k_hi, mp.data_ptr(), p(rows[0][1]), p(rows[1][1]), p(rows[2][1]),
                                           torch.cuda.current_stream().cuda_stream), "selftok_token_agree")
        assert np.array_equal(u32(mp), rep * want[0])
        for (full, inner), w in zip(rows, want[1:]):
            assert np.array_equal(inner.cpu().numpy(), w) and intact(full, c.N, SENT32)
    assert intact(fm, c.K, SENT32)
    r = TS.token_agreement(ta, torch.from_numpy(b.astype(np.int64)).cuda(), (c.k_lo, c.k_hi))              # the host side, ids of another width
    assert np.array_equal(r["n_diff"], want[1]) and np.array_equal(r["first_diff"], want[2]) and np.array_equal(r["last_diff"], want[3])
    assert r["rows_equal"] == int((want[1] == 0).sum()) and r["rows"] == c.N and r["positions"] == c.k_hi - c.k_lo
    if c.N and c.k_hi > c.k_lo:
        assert np.array_equal(r["match_rate_pos"], want[0][c.k_lo:c.k_hi] / c.N) and r["match_rate"] == float(want[0].sum()) / (c.N * (c.k_hi - c.k_lo))


@pytest.mark.parametrize("name", [c.name for c in TC.NEAR_CASES])
def test_nearest_equals_the_emulation_for_every_split_chunk_and_order(name):
    c = TC.NEAR_BY_NAME[name]
    q, ref = TC.make_near(name)
    tq = torch.from_numpy(q).cuda()
    tr = tq if c.self else torch.from_numpy(ref).cuda()
    want = TC.nearest(q, ref, c.k_lo, c.k_hi, c.self)
    kr = (c.k_lo, c.k_hi)
    lib = _lib.load()
    need = lib.selftok_token_nearest_workspace_bytes(c.M, c.N)
    assert need == max(1, min(64, -(-c.N // TC.TILE))) * max(c.M, 1) * 8
    fw, ws = guarded(need // 8, np.int64, SENT64)
    (fa, oa), (fi, oi) = guarded(c.M, np.int32, SENT32), guarded(c.M, np.int32, SENT32)
    for split in (0,) + TC.SPLITS + (0,):                           # the automatic split, every override, and once more: the same bits
        oa.fill_(-77); oi.fill_(-77)
        best, idx = ops.token_nearest(tq, tr, kr, 1 if c.self else 0, split=split, out_match=oa, out_idx=oi, workspace=ws)
        assert np.array_equal(best.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1]), split
        assert intact(fw, need // 8, SENT64) and intact(fa, c.M, SENT32) and intact(fi, c.M, SENT32)
    for chunk in (None, 1 if c.M <= 70 else 37, 64, 65):             # the host side: every chunk size, exclude_self by the chunk's first row
        best, idx = TS.nearest_sequences(tq, tr, kr, exclude_self=c.self, chunk=chunk)
        assert np.array_equal(best.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1]), chunk
    if c.M and not c.self:
        for i in (0, c.M - 1):                                      # a query alone answers as in the batch
            best, idx = ops.token_nearest(tq[i:i + 1], tr, kr)
            assert (int(best[0]), int(idx[0])) == (int(want[0][i]), int(want[1][i]))
        perm = np.random.default_rng(3).permutation(c.M)            # a permutation of the queries permutes the answers
        best, idx = ops.token_nearest(torch.from_numpy(np.ascontiguousarray(q[perm])).cuda(), tr, kr)
        assert np.array_equal(best.cpu().numpy(), want[0][perm]) and np.array_equal(idx.cpu().numpy(), want[1][perm])
    if c.M and c.K == 40 and not c.self:                            # ids of another width and a numpy array go through the packer
        best, idx = TS.nearest_sequences(q.astype(np.int64), torch.from_numpy(ref.astype(np.int32)).cuda(), kr)
        assert np.array_equal(best.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1])


def test_token_census_takes_any_integer_ids_views_and_merges():
    rng = np.random.default_rng(11)
    K, C = 40, 64
    topk = rng.integers(0, C, size=(3, 7, K, 4))                    # [..., K, k]: column 0 of a top-k result, counted without a copy
    want, _ = TC.count(topk[..., 0].reshape(-1, K), C)
    for arr in (topk.astype(np.int64), topk.astype(np.int16), topk.astype(np.uint8), topk.astype(np.uint16), topk.astype(np.uint64)):
        cen = TS.TokenCensus(K, C)
        cen.update(torch.from_numpy(arr).cuda()[..., 0] if arr.dtype in (np.int64, np.int16, np.uint8) else np.ascontiguousarray(arr[..., 0]))
        assert np.array_equal(cen.counts(), want) and cen.rows == 21 and cen.bad_ids() == 0, arr.dtype
    a, b = TS.TokenCensus(K, C), TS.TokenCensus(K, C)
    a.update(topk[:2, ..., 0]); b.update(topk[2:, ..., 0]); b.update(np.full((2, K), -5))
    a.merge(b)
    r, ref = a.result(), TC.census(want)
    assert np.array_equal(a.counts(), want) and (r["rows"], r["bad_ids"], r["tokens"]) == (23, 2 * K, 21 * K) and r["used"] == int(ref[K, 1]) and r["usage"] == ref[K, 1] / C
    assert abs(r["perplexity"] / np.exp(ref[K, 2]) - 1) <= TC.PPL_RTOL and abs(r["perplexity_ref"] / np.exp(ref[K, 3]) - 1) <= TC.PPL_RTOL
    assert abs(r["entropy_bits"] - ref[K, 2] / np.log(2)) <= 2 * TC.H_TOL and r["max_code_share"] == ref[K, 4] / ref[K, 0]
    assert np.array_equal(r["used_pos"], ref[:K, 1]) and np.abs(r["perplexity_pos"] / np.exp(ref[:K, 2]) - 1).max() <= TC.PPL_RTOL
    assert np.array_equal(a.dead_codes(), np.flatnonzero(want.sum(0) == 0)) and json.dumps(a.summary())
    with pytest.raises(ValueError, match="outside"):
        TS.token_agreement(np.full((2, K), 70000), np.zeros((2, K), np.int64))


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    return SelftokPipeline(default_config(512), None, None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False)


def test_pipeline_census_agreement_and_evaluate(pipe):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pipeline_b16.npz"))
    gold = g["tokens"].astype(np.int64)
    ids = pipe.encoding(synth.synthetic_images(16).to(pipe.device), device=pipe.device)
    cen = TS.TokenCensus(512, 32768).update(ids)
    want, bad = TC.count(gold, 32768)
    assert np.array_equal(cen.counts(), want) and bad == 0
    r, ref = cen.result(), TC.census(want)
    assert r["used"] == int(ref[512, 1]) and abs(r["perplexity"] / np.exp(ref[512, 2]) - 1) <= TC.PPL_RTOL and r["rows"] == 16 and r["bad_ids"] == 0
    ag = TS.token_agreement(ids, pipe.encoding(synth.synthetic_images(16).to(pipe.device), device=pipe.device))
    assert ag["rows_equal"] == 16 and ag["match_rate"] == 1.0 and (ag["first_diff"] == 512).all() and (ag["last_diff"] == -1).all() and (ag["match_rate_pos"] == 1.0).all()
    ag = TS.token_agreement(ids, gold)
    assert ag["rows_equal"] == 16
    load, noise = (lambda lo, hi: synth.synthetic_images(hi - lo, first_index=lo)), (lambda lo, hi: synth.synthetic_noise(hi - lo, first_index=lo))
    plain = E.evaluate(pipe, load, 2, batch=2, noise_fn=noise, metrics=("psnr",))
    withtok = E.evaluate(pipe, load, 2, batch=2, noise_fn=noise, metrics=("psnr", "tokens"))
    assert "token_census" not in plain and {k: v for k, v in withtok.items() if k != "token_census"} == plain
    want2, _ = TC.count(gold[:2], 32768)
    tc = withtok["token_census"]
    assert tc["rows"] == 2 and tc["used"] == int((want2.sum(0) > 0).sum()) and tc["dead_codes"] == 32768 - tc["used"] and json.dumps(tc)


def test_the_tools_run_in_a_child_process(tmp_path):
    tool = os.path.join(ROOT, "tools", "tokenize_folder.py")
    r = subprocess.run([sys.executable, tool, "--synthetic", "4", "--crops", "five", "--stats", "--batch", "4", "--out", str(tmp_path / "five")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    ids = np.load(tmp_path / "five.rank0.npy")
    assert ids.shape == (4, 5, 512) and ids.dtype == np.int64
    want, _ = TC.count(ids.reshape(-1, 512), 32768)
    tc, va = line["rank0_token_census"], line["rank0_view_agreement"]
    assert tc["rows"] == 20 and tc["bad_ids"] == 0 and tc["used"] == int((want.sum(0) > 0).sum()) and tc["dead_codes"] == 32768 - tc["used"]
    assert abs(tc["perplexity"] / np.exp(TC.census(want)[512, 2]) - 1) <= TC.PPL_RTOL
    same = ids[:, 1:] == ids[:, :1]
    assert va["rows"] == 16 and va["match_rate"] == float(same.mean()) and va["mean_n_diff"] == float((~same).sum()) / 16
    assert np.array_equal(TS.TokenCensus.load(str(tmp_path / "five.rank0.census.npz")).counts(), want)
    # tools/token_stats.py on a tiny set with a planted duplicate, the reference's int64 and the uint16 form
    rng = np.random.default_rng(2)
    small = rng.integers(0, 4, size=(70, 40))
    small[66] = small[5]
    np.save(tmp_path / "a.npy", small.astype(np.int64))
    other = small.copy()
    other[:, 0] ^= 1
    np.save(tmp_path / "b.npy", other.astype(np.uint16))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "token_stats.py"), "--ids", str(tmp_path / "a.npy"), "--against", str(tmp_path / "b.npy"), "--nearest-in",
                        str(tmp_path / "b.npy"), "--dedup", "--codes", "4"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    best, idx = TC.nearest(small.astype(np.uint16), small.astype(np.uint16), 0, 40, True)
    d = line["dedup"]
    assert d["exact_copies"] == 2 and d["best_match_max"] == 40 and d["closest"][0] == {"row": 5, "nearest": 66, "equal_positions": 40} and d["closest"][1]["row"] == 66
    assert d["best_match_mean"] == float(best.mean()) and line["census"]["used"] == 4 and line["census"]["rows"] == 70
    assert line["agreement"]["rows_equal"] == 0 and line["agreement"]["n_diff_max"] == 1 and line["agreement"]["first_diff_mean"] == 0.0 and line["agreement"]["worst_position"] == 0
    assert line["nearest"]["best_match_max"] == 39 and line["nearest"]["exact_copies"] == 0


def test_the_largest_entropy_deviation_stays_inside_the_derived_bound():
    """runs last in this file: what the census cases above measured against the fp64 emulation"""
    print(f"\nlargest |H - emulation| over the case table: {WORST['H']:.3e} nats (bound {TC.H_TOL:.0e}); perplexity {WORST['ppl_rel']:.3e} relative (bound {TC.PPL_RTOL:.0e})")
    assert WORST["H"] <= TC.H_TOL and WORST["ppl_rel"] <= TC.PPL_RTOL
