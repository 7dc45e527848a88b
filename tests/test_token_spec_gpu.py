"""-m gpu: speculative token sampling (csrc/token_verify.hip through ops.token_verify and sampling.TokenSampler.fork / verify) against the arithmetic of
record of tests/token_spec_cases.py: every output equal on every case inside guard bands, the log-probabilities within 1 fp32 ulp (the device's fp64 log may
differ from numpy's in the last place before the one rounding to fp32), the invariances bit for bit, a row without a draft against the sampler's own kernel,
and the end-to-end property: with draft logits equal to target logits the draft / verify loop emits the ids of the plain step loop."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import token_spec_cases as SC
from selftoktokenizer_amd import ops, sampling, synth, tokens, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 64, SC.SENT                                           # guard elements either side of every logits buffer (a multiple of four codes)
f32 = np.float32
ROW_KEYS = ("accept", "repl_id", "n_kept", "mass", "n_accept", "n_emit", "ids", "nk_mat", "ctr")


def _dev_logits(host, dt):
    """host [B, R, row] (fp32, or bf16 bits) -> (a [B, R, row] device view inside a flat buffer with NaN guard bands, the flat buffer)"""
    if host is None:
        return None, None
    t = torch.from_numpy(host.view(np.int16) if dt == "bf16" else host)
    t = t.view(torch.bfloat16) if dt == "bf16" else t
    flat = torch.full((GUARD + t.numel() + GUARD,), float("nan"), dtype=t.dtype, device="cuda")
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1).cuda()
    return flat[GUARD:GUARD + t.numel()].view(t.shape), flat


def _launch(c, dev, *, n_draft="case", **over):
    """one call with sentinel-filled, guard-banded outputs and a fresh copy of the counters -> dict of host arrays (guards checked here)"""
    tl = dev["target"]
    B, S = tl.shape[0], tl.shape[1] - 1
    idt = torch.int32 if c.ids == "int32" else torch.int64
    full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device="cuda")
    ids, lpm, nkm = full((B + 2, c.K), SENT, idt), full((B + 2, c.K), 123.0, torch.float32), full((B + 2, c.K), SENT, torch.int32)
    acc, repl, nk = full((B + 2, S + 1), 99, torch.uint8), full((B + 2, S + 1), SENT, torch.int32), full((B + 2, S + 1), SENT, torch.int32)
    mass, lpx, lpr = full((B + 2, S + 1, 4), SENT, torch.int64), full((B + 2, S + 1), 123.0, torch.float32), full((B + 2, S + 1), 123.0, torch.float32)
    na, ne = full((B + 2,), SENT, torch.int32), full((B + 2,), SENT, torch.int32)
    ctr = full((B + 2, 2), SENT, torch.int32)
    ctr[1:B + 1] = dev["ctr"]
    foreign, bad = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(target_uncond=dev["target_uncond"], draft_uncond=dev["draft_uncond"], C=c.C, offset=c.offset, cfg_scale=c.st, draft_cfg_scale=c.sd, temperature=c.T,
              top_k=c.k, top_p=c.P, seed=c.seed, n_draft=dev["n_draft"] if n_draft == "case" else n_draft, accept=acc[1:B + 1], repl_id=repl[1:B + 1],
              row_n_kept=nk[1:B + 1], mass=mass[1:B + 1], logprob_x=lpx[1:B + 1], logprob_repl=lpr[1:B + 1], n_accept=na[1:B + 1], n_emit=ne[1:B + 1], foreign=foreign,
              bad=bad)
    kw.update(over)
    ops.token_verify(tl, dev["draft"], dev["x"], ctr[1:B + 1], ids[1:B + 1], lpm[1:B + 1], nkm[1:B + 1], **kw)
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    for g, v in ((ids, SENT), (nkm, SENT), (repl, SENT), (nk, SENT), (mass, SENT), (na, SENT), (ne, SENT), (ctr, SENT), (acc, 99), (lpm, 123.0), (lpx, 123.0), (lpr, 123.0)):
        assert (h(g)[[0, -1]] == v).all(), "an output guard row was written"
    return dict(accept=h(acc)[1:-1], repl_id=h(repl)[1:-1], n_kept=h(nk)[1:-1], mass=h(mass)[1:-1].view(np.uint64), lp_x=h(lpx)[1:-1], lp_repl=h(lpr)[1:-1],
                n_accept=h(na)[1:-1], n_emit=h(ne)[1:-1], ids=h(ids)[1:-1], lp_mat=h(lpm)[1:-1], nk_mat=h(nkm)[1:-1], ctr=h(ctr)[1:-1].view(np.uint32),
                foreign=int(foreign.cpu()[0]), bad=int(bad.cpu()[0]))


_RUNS = {}


def run_case(name):
    """the case on the device, once: (result, the device inputs)"""
    if name not in _RUNS:
        c, d = SC.BY_NAME[name], SC.make(name)
        dev, flats = {}, []
        for key, dt in (("target", c.tdt), ("target_uncond", c.tdt), ("draft", c.ddt), ("draft_uncond", c.ddt)):
            dev[key], flat = _dev_logits(d[key] if d[key] is None or d[key].shape[1] else None, dt)
            if flat is not None:
                flats.append((flat, flat.clone()))
        dev["x"] = None if c.S == 0 else torch.from_numpy(d["x"].astype(np.int32 if c.xids == "int32" else np.int64)).cuda()
        dev["ctr"] = torch.from_numpy(d["ctr"].view(np.int32)).cuda()
        dev["n_draft"] = d["n_draft"]
        out = _launch(c, dev)
        as_int = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
        assert all(torch.equal(as_int(a), as_int(b)) for a, b in flats), "the logits are only read"
        _RUNS[name] = (out, dev)
    return _RUNS[name]


def _ulp_apart(a, b):
    ia, ib = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _lp_close(got, want):
    got, want = np.asarray(got, f32).reshape(-1), np.asarray(want, f32).reshape(-1)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and (_ulp_apart(got[~nan], want[~nan]) <= 1).all()


def _check(c, out, ref, ctr0):
    rows = ref.rows
    grid = lambda f, dt=np.int64: np.array([[f(r) for r in rb] for rb in rows], dtype=dt)
    assert np.array_equal(out["accept"], grid(lambda r: r.accept)), (c.name, "accept", out["accept"].tolist())
    assert np.array_equal(out["repl_id"], grid(lambda r: r.repl_id)), (c.name, "repl_id", out["repl_id"].tolist(), grid(lambda r: r.repl_id).tolist())
    assert np.array_equal(out["n_kept"], grid(lambda r: r.n_kept)), (c.name, "n_kept")
    want_mass = np.array([[[r.P, r.D, r.p_x, r.d_x] for r in rb] for rb in rows], dtype=np.uint64)
    assert np.array_equal(out["mass"], want_mass), (c.name, "mass")
    assert _lp_close(out["lp_x"], grid(lambda r: r.lp_x, f32)) and _lp_close(out["lp_repl"], grid(lambda r: r.lp_repl, f32)), (c.name, "logprob")
    assert out["n_accept"].tolist() == ref.n_accept and out["n_emit"].tolist() == ref.n_emit, (c.name, out["n_accept"], ref.n_accept, out["n_emit"], ref.n_emit)
    assert np.array_equal(out["ids"].astype(np.int64), ref.ids) and out["ids"].dtype == (np.int32 if c.ids == "int32" else np.int64), (c.name, "ids")
    assert np.array_equal(out["nk_mat"].astype(np.int64), ref.n_kept), (c.name, "n_kept matrix")
    written = ref.ids != SENT
    assert (out["lp_mat"][~written] == 123.0).all() and _lp_close(out["lp_mat"][written], ref.logprob[written]), (c.name, "logprob matrix")
    assert np.array_equal(out["ctr"][:, 0], ctr0[:, 0]) and out["ctr"][:, 1].tolist() == ref.step_after, (c.name, "ctr")
    assert (out["foreign"], out["bad"]) == (ref.foreign, ref.bad), (c.name, out["foreign"], out["bad"])


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_token_verify_equals_the_emulation(name):
    """accept, repl_id, n_kept, the four masses, n_accept, n_emit, the committed ids and kept counts and the counters equal, every log-probability within 1 fp32
    ulp, nothing written outside what is stated (sentinels and guard rows): a bad row writes accept 0, id -1, n_kept 0, zero masses, NaN and counts once; a
    foreign row is rejected and counts once; positions the commit does not own keep their sentinel; the logits are only read"""
    c = SC.BY_NAME[name]
    out, _ = run_case(name)
    _check(c, out, SC.reference(name), SC.make(name)["ctr"])


def _same_bits(a, b, keys=ROW_KEYS, rows=slice(None)):
    return all(np.array_equal(a[k][rows], b[k]) for k in keys) and all(a[k][rows].tobytes() == b[k].tobytes() for k in ("lp_x", "lp_repl", "lp_mat"))


@pytest.mark.parametrize("name", ["c5_s3_k2_p50_ragged", "c1000_bf16_bf16_cfg_t_vlm", "c32768_cfg_both_vlm", "c65536_k50_p90", "four_bf16_T07", "bad_rows",
                                  "foreign_p_eq_d"])
def test_run_to_run_alone_and_in_any_sequence_order(name):
    """the same bits again; each sequence alone gives what it gave in the batch; the sequences reversed, counters, draft ids and draft counts carried along, give
    the reversed outputs"""
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    again = _launch(c, dev)
    assert _same_bits(out, again) and (out["foreign"], out["bad"]) == (again["foreign"], again["bad"])
    cut = lambda t, sl: None if t is None else t[sl].contiguous()
    for b in sorted({0, c.B // 2, c.B - 1}):
        one = {k: cut(dev[k], slice(b, b + 1)) for k in ("target", "target_uncond", "draft", "draft_uncond", "x", "ctr")}
        one["n_draft"] = None if dev["n_draft"] is None else dev["n_draft"][b:b + 1]
        assert _same_bits(out, _launch(c, one), rows=slice(b, b + 1)), (name, b)
    perm = torch.arange(c.B - 1, -1, -1, device="cuda")
    rev = {k: cut(dev[k], perm) for k in ("target", "target_uncond", "draft", "draft_uncond", "x", "ctr")}
    rev["n_draft"] = None if dev["n_draft"] is None else dev["n_draft"][::-1]
    assert _same_bits(out, _launch(c, rev), rows=perm.cpu().numpy()), name


@pytest.mark.parametrize("name", ["c256_bf16_f32_p50", "c1000_bf16_bf16_cfg_t_vlm", "c4095_f32_bf16_cfg_d_T4", "four_bf16_T07", "bad_rows_bf16_cfg"])
def test_bf16_equals_the_same_values_widened_to_fp32(name):
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    wide = dict(dev, **{k: None if dev[k] is None else dev[k].float() for k in ("target", "target_uncond", "draft", "draft_uncond")})
    got = _launch(c, wide)
    assert _same_bits(out, got) and (out["foreign"], out["bad"]) == (got["foreign"], got["bad"])


@pytest.mark.parametrize("name", ["c255_k50_p90", "c4096_equal", "four_k300_p50"])
def test_no_guidance_equals_guidance_of_scale_one_on_equal_logits(name):
    """s = 1 with lu = lc: lc - lu is exactly +0 for every finite logit, 1 * 0 = 0 and lu + 0 = lc (a -0.0 becomes +0.0, which the key counts as equal): the guided
    path is exact on finite logits, on either side and on both"""
    c = SC.BY_NAME[name]
    assert not c.tg and not c.dg and all(np.isfinite(w).all() for w in SC.windows(name) if w is not None)
    out, dev = run_case(name)
    for t_on, d_on in ((True, False), (False, True), (True, True)):
        got = _launch(c, dict(dev, target_uncond=dev["target"].clone() if t_on else None, draft_uncond=dev["draft"].clone() if d_on else None), cfg_scale=1.0,
                      draft_cfg_scale=1.0)
        assert _same_bits(out, got), (name, t_on, d_on)


def test_graph_replay_equals_eager():
    name = "c32768_cfg_both_vlm"
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    B, S = c.B, c.S
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    ids, lpm, nkm, ctr = z((B, c.K), torch.int64), z((B, c.K), torch.float32), z((B, c.K), torch.int32), dev["ctr"].clone()
    pre = dict(accept=z((B, S + 1), torch.uint8), repl_id=z((B, S + 1), torch.int32), row_n_kept=z((B, S + 1), torch.int32), mass=z((B, S + 1, 4), torch.int64),
               logprob_x=z((B, S + 1), torch.float32), logprob_repl=z((B, S + 1), torch.float32), n_accept=z((B,), torch.int32), n_emit=z((B,), torch.int32),
               foreign=z((1,), torch.int32), bad=z((1,), torch.int32))
    nd_dev = torch.tensor(dev["n_draft"], dtype=torch.int32, device="cuda")
    call = lambda: ops.token_verify(dev["target"], dev["draft"], dev["x"], ctr, ids, lpm, nkm, target_uncond=dev["target_uncond"], draft_uncond=dev["draft_uncond"],
                                    C=c.C, offset=c.offset, cfg_scale=c.st, draft_cfg_scale=c.sd, temperature=c.T, top_k=c.k, top_p=c.P, seed=c.seed,
                                    n_draft=dev["n_draft"], n_draft_dev=nd_dev, **pre)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in [ids, lpm, nkm] + list(pre.values()):
        t.zero_()
    ctr.copy_(dev["ctr"])
    g.replay()
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy()
    assert np.array_equal(h(pre["accept"]), out["accept"]) and np.array_equal(h(pre["repl_id"]), out["repl_id"]) and np.array_equal(h(pre["row_n_kept"]), out["n_kept"])
    assert np.array_equal(h(pre["mass"]).view(np.uint64), out["mass"]) and h(pre["logprob_x"]).tobytes() == out["lp_x"].tobytes()
    assert h(pre["logprob_repl"]).tobytes() == out["lp_repl"].tobytes() and h(pre["n_emit"]).tolist() == out["n_emit"].tolist()
    written = out["ids"] != SENT
    assert np.array_equal(h(ids)[written], out["ids"][written]) and (h(ids)[~written] == 0).all() and np.array_equal(h(ctr).view(np.uint32), out["ctr"])
    assert (int(pre["foreign"].cpu()[0]), int(pre["bad"].cpu()[0])) == (out["foreign"], out["bad"])


@pytest.mark.parametrize("name", ["c2_s0", "c5_s3_k2_p50_ragged", "c1000_bf16_bf16_cfg_t_vlm", "c32768_cfg_both_vlm", "c65536_k50_p90", "greedy_agree", "no_draft_marks"])
def test_a_row_without_a_draft_equals_the_sampler_kernel(name):
    """kernel against kernel: every row without a draft gives the id, n_kept, Q_kept, the id's mass and the logprob bits of ops.token_sample on that row"""
    c, d = SC.BY_NAME[name], SC.make(name)
    out, dev = run_case(name)
    nd = SC.n_draft_of(name)
    n = 0
    for s in range(c.S + 1):
        bs = [b for b in range(c.B) if not (s < nd[b] and d["x"][b, s] >= 0)]
        if not bs:
            continue
        ctr = dev["ctr"].clone()
        ctr[:, 1] += s
        ids = torch.full((c.B, 1), SENT, dtype=torch.int64, device="cuda")
        nk, mass, lp, _ = ops.token_sample(dev["target"][:, s], ctr, ids, uncond_logits=None if dev["target_uncond"] is None else dev["target_uncond"][:, s], C=c.C,
                                           offset=c.offset, cfg_scale=c.st, temperature=c.T, top_k=c.k, top_p=c.P, seed=c.seed)
        torch.cuda.synchronize()
        ids, nk, mass, lp = ids.cpu().numpy()[:, 0], nk.cpu().numpy(), mass.cpu().numpy().view(np.uint64), lp.cpu().numpy()
        for b in bs:
            assert (out["accept"][b, s], out["repl_id"][b, s], out["n_kept"][b, s]) == (0, ids[b], nk[b]), (name, b, s)
            assert out["mass"][b, s].tolist() == [int(mass[b, 1]), 0, int(mass[b, 2]), 0] and out["lp_repl"][b, s].tobytes() == lp[b].tobytes(), (name, b, s)
            n += 1
    assert n >= 1


def _hash_rows(tickets, steps, V, salt):
    """deterministic pseudo-logits in [-4, 4), a function of (ticket, step, code) alone: tickets [B], steps [B, R] -> [B, R, V] fp32"""
    t, s = np.asarray(tickets, dtype=np.uint64)[:, None, None], np.asarray(steps, dtype=np.uint64)[:, :, None]
    i = ((t * np.uint64(1000003) + s * np.uint64(7919) + np.uint64(salt)) * np.uint64(2654435761) + np.arange(V, dtype=np.uint64)[None, None, :]) & np.uint64(0xFFFFFFFF)
    i = (i ^ (i >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    i = (i ^ (i >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
    i = i ^ (i >> np.uint64(15))
    return ((i >> np.uint64(8)).astype(np.float64) / 2.0 ** 24 * 8.0 - 4.0).astype(f32)


def _steps_of(s):
    m = s.partial()[1]
    return np.full(s.B, m, np.int64) if isinstance(m, int) else np.asarray(m, np.int64)


def _count_read_backs(monkeypatch):
    reads, real = [], sampling.TokenSampler._read_back
    monkeypatch.setattr(sampling.TokenSampler, "_read_back", lambda self, t: (reads.append(tuple(t.shape)), real(self, t))[1])
    return reads


def test_draft_equal_to_target_emits_the_ids_of_the_plain_step_loop(monkeypatch):
    """THE END-TO-END PROPERTY.  K = 40, B = 3, C = 300, top-k 50, top-p 0.9, logits a hash of (ticket, step): a draft / verify loop with S = 4 and draft logits
    == target logits fills ids in K / (S + 1) = 8 rounds with one read-back each, and equals 40 plain TokenSampler.step calls: ids, logprob bits, n_kept"""
    K, B, C, S = 40, 3, 300, 4
    tickets = [7, 1 << 31, 12345]
    kw = dict(C=C, temperature=1.0, top_k=50, top_p=0.9, seed=(0xABCD << 32) | 0x1234)
    plain = sampling.TokenSampler(K, **kw).begin(B, tickets=tickets)
    for t in range(K):
        plain.step(torch.from_numpy(_hash_rows(tickets, np.full((B, 1), t), C, 1)[:, 0]).cuda())
    reads = _count_read_backs(monkeypatch)
    spec = sampling.TokenSampler(K, **kw).begin(B, tickets=tickets)
    rounds = 0
    while _steps_of(spec).min() < K:
        m = spec.partial()[1]
        assert isinstance(m, int)                                    # every draft is kept, so the rows stay in step
        tl = torch.from_numpy(_hash_rows(tickets, m + np.tile(np.arange(S + 1), (B, 1)), C, 1)).cuda()
        dr = spec.fork()
        for s in range(S):
            dr.step(tl[:, s])
        x, n = dr.drafted()
        r = spec.verify(x, tl[:, :S], tl, n_draft=n)
        assert r.n_emit.tolist() == [S + 1] * B and r.n_accept.cpu().tolist() == [S] * B
        rounds += 1
    assert rounds == K // (S + 1) and reads == [(B,)] * rounds
    assert torch.equal(spec.ids, plain.ids) and torch.equal(spec.n_kept, plain.n_kept) and torch.equal(spec.ctr, plain.ctr)
    assert spec.logprob.cpu().numpy().tobytes() == plain.logprob.cpu().numpy().tobytes()
    assert int(spec.bad.cpu()[0]) == 0 and int(spec.foreign.cpu()[0]) == 0 and len(set(plain.ids.cpu().numpy().reshape(-1).tolist())) > 30


def test_a_noisy_draft_finishes_every_row_and_equals_the_emulated_loop(monkeypatch):
    """draft != target: rows fall out of step, the loop still ends with every row at K (a finished row emits nothing while the others go on, the last rounds
    draft fewer tokens), one read-back per round, and every committed id, kept count and counter is the emulation's, stepped on the host"""
    K, B, C, S = 24, 3, 300, 4
    tickets = [3, 99, 1 << 30]
    seed = 0x51EC
    kw = dict(C=C, temperature=1.0, top_k=50, top_p=0.9, seed=seed)
    reads = _count_read_backs(monkeypatch)
    spec = sampling.TokenSampler(K, **kw).begin(B, tickets=tickets)
    steps, rounds = np.zeros(B, np.int64), 0
    want = np.zeros((B, K), np.int64)
    while steps.min() < K:
        S_r = int(min(S, K - steps.max()))
        st = steps[:, None] + np.arange(S_r + 1)[None, :]
        tl_h = _hash_rows(tickets, st, C, 1)
        dl_h = (tl_h[:, :S_r] + f32(0.35) * _hash_rows(tickets, st[:, :S_r], C, 2)).astype(f32)
        tl, dl = torch.from_numpy(tl_h).cuda(), torch.from_numpy(dl_h).cuda() if S_r else None
        dr = spec.fork()
        for s in range(S_r):
            dr.step(dl[:, s])
        x, n = dr.drafted()
        r = spec.verify(x, dl, tl, n_draft=n)
        x_h = x.cpu().numpy()
        for b in range(B):                                           # the emulation of this round
            ts = [SC.side(tl_h[b, s], None, 1.0, 1.0, 50, 0.9) for s in range(S_r + 1)]
            ds = [SC.side(dl_h[b, s], None, 1.0, 1.0, 50, 0.9) for s in range(S_r)]
            xs = [int(v) for v in x_h[b]] + [-1]
            rows = [SC.verify_row(ts[s], ds[s] if s < S_r else None, xs[s], C, seed, tickets[b], int(steps[b]) + s) for s in range(S_r + 1)]
            na, ne, writes = SC.commit(rows, xs, S_r, int(steps[b]), K)
            for pos, i, _, _ in writes:
                want[b, pos] = i
            assert (int(r.n_accept[b]), int(r.n_emit[b])) == (na, ne), (rounds, b)
            steps[b] += ne
        assert _steps_of(spec).tolist() == steps.tolist()
        rounds += 1
        assert rounds <= K                                           # every round emits at least one token for every unfinished row
    assert reads == [(B,)] * rounds and K // (S + 1) < rounds <= K and spec.ctr.cpu()[:, 1].tolist() == [K] * B
    assert np.array_equal(spec.ids.cpu().numpy(), want) and int(spec.bad.cpu()[0]) == 0 and int(spec.foreign.cpu()[0]) == 0
    assert not torch.isnan(spec.logprob).any() and int(spec.n_kept.min()) >= 1
    with pytest.raises(RuntimeError, match="already holds"):
        spec.step(torch.zeros(B, C, device="cuda"))


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    p = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"))
    p.verbose = False
    return p


def test_partial_after_verify_goes_through_decoding(pipe):
    """six rounds of K = 512 over the 32768 codes with a noisy draft: the rows stand at different steps, partial() feeds decoding(ar_partial=m) directly and gives
    the pixels of the same ids placed by pad_ar_partial"""
    K, B, C, S = 512, 2, 32768, 4
    tickets = [11, 22]
    spec = sampling.TokenSampler(K, temperature=1.0, top_k=50, top_p=0.9, seed=99).begin(B, tickets=tickets)
    for _ in range(6):
        st = _steps_of(spec)[:, None] + np.arange(S + 1)[None, :]
        tl_h = _hash_rows(tickets, st, C, 3)
        tl = torch.from_numpy(tl_h).cuda()
        dl = torch.from_numpy((tl_h[:, :S] + f32(0.3) * _hash_rows(tickets, st[:, :S], C, 4)).astype(f32)).cuda()
        dr = spec.fork()
        for s in range(S):
            dr.step(dl[:, s])
        x, n = dr.drafted()
        spec.verify(x, dl, tl, n_draft=n)
    ids, m = spec.partial()
    m = _steps_of(spec)
    assert int(spec.bad.cpu()[0]) == 0 and (m >= 6).all() and (m <= 6 * (S + 1)).all()
    ids_h = ids.cpu().numpy()
    emitted = [ids_h[b, K - m[b]:][::-1] for b in range(B)]            # in the order the model emitted them
    placed, m2 = tokens.pad_ar_partial(emitted, K)
    assert np.array_equal(placed, ids_h) and m2.tolist() == m.tolist()
    noise = synth.synthetic_noise(B, first_index=40)
    a = pipe.decoding(ids, noise=noise, max_steps=2, ar_partial=m)
    b = pipe.decoding(placed, noise=noise, max_steps=2, ar_partial=m2)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_bench_tool_runs_at_a_tiny_size(tmp_path):
    out = tmp_path / "spec.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_token_speculative.py"), "--synthetic", "--quick", "--C", "1024", "--S", "2", "--out", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(out.read_text())
    assert res["C"] == 1024 and res["S"] == 2 and len(res["rows"]) == 2 * 2 * 2 * 3
    for row in res["rows"]:
        assert row["verify"]["median_ms"] > 0 and row["torch"]["median_ms"] > 0 and row["sample_floor"]["median_ms"] > 0
        assert 0.0 <= row["acceptance_rate"] <= 1.0 and 1.0 <= row["tokens_per_round"] <= 3.0 and row["foreign"] == 0
    assert any(r["acceptance_rate"] > 0.5 for r in res["rows"]) and subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_token_speculative.py")],
                                                                                   capture_output=True).returncode != 0
