"""-m gpu: the token sampler (csrc/token_sample.hip through ops.token_sample and sampling.TokenSampler) against the numpy arithmetic of record of
tests/token_sample_cases.py: every output equal on every case inside guard bands, logprob within 1 fp32 ulp (the device's fp64 log may differ from numpy's in
the last place before the one rounding to fp32), and the invariances the reproducibility claim rests on, bit for bit."""
import numpy as np
import pytest
import torch

import token_sample_cases as TC
from selftoktokenizer_amd import ops, sampling, synth, tokens, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
GUARD, SENT = 64, -777                                              # guard elements either side of every buffer (a multiple of four codes); the id sentinel
f32 = np.float32


def _dev_logits(c, host, guard_value=float("nan")):
    """host [B, row] (fp32, or bf16 bits) -> a [B, row] device view inside a flat buffer with NaN guard bands"""
    if host is None:
        return None, None
    t = torch.from_numpy(host.view(np.int16) if c.dtype == "bf16" else host)
    t = t.view(torch.bfloat16) if c.dtype == "bf16" else t
    flat = torch.full((GUARD + t.numel() + GUARD,), guard_value, dtype=t.dtype, device="cuda")
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1).cuda()
    return flat[GUARD:GUARD + t.numel()].view(c.B, c.row), flat


def _launch(c, logits, uncond, ctr, pos, *, rows=None, **over):
    """one call with sentinel-filled, guard-banded outputs -> dict of host arrays (guards checked here)"""
    B = logits.shape[0]
    idt = torch.int32 if c.ids == "int32" else torch.int64
    ids = torch.full((B + 2, c.K), SENT, dtype=idt, device="cuda")
    nk = torch.full((B + 2,), SENT, dtype=torch.int32, device="cuda")
    mass = torch.full((B + 2, 3), SENT, dtype=torch.int64, device="cuda")
    lp = torch.full((B + 2,), 123.0, dtype=torch.float32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    kw = dict(uncond_logits=uncond, C=c.C, offset=c.offset, cfg_scale=c.s, temperature=c.T, top_k=c.k, top_p=c.P, seed=c.seed, pos=pos, col=c.K - 1 if pos is None else 0,
              n_kept=nk[1:B + 1], mass=mass[1:B + 1], logprob=lp[1:B + 1], bad=bad)
    kw.update(over)
    ops.token_sample(logits, ctr, ids[1:B + 1], **kw)
    torch.cuda.synchronize()
    ids_h, nk_h, mass_h, lp_h = ids.cpu().numpy(), nk.cpu().numpy(), mass.cpu().numpy(), lp.cpu().numpy()
    for g in (ids_h[[0, -1]], nk_h[[0, -1]], mass_h[[0, -1]]):
        assert (g == SENT).all(), "an output guard row was written"
    assert (lp_h[[0, -1]] == 123.0).all()
    return dict(ids=ids_h[1:-1], n_kept=nk_h[1:-1], mass=mass_h[1:-1].view(np.uint64), logprob=lp_h[1:-1], bad=int(bad.cpu()[0]))


_RUNS = {}


def run_case(name):
    """the case on the device, once: (result, the device inputs)"""
    if name not in _RUNS:
        c, d = TC.BY_NAME[name], TC.make(name)
        logits, lflat = _dev_logits(c, d["logits"])
        uncond, uflat = _dev_logits(c, d["uncond"])
        ctr = torch.from_numpy(d["ctr"].view(np.int32)).cuda()
        pos = None if d["pos"] is None else torch.from_numpy(d["pos"]).cuda()
        before = lflat.clone()
        out = _launch(c, logits, uncond, ctr, pos)
        assert torch.equal(lflat.view(torch.int16 if c.dtype == "bf16" else torch.int32), before.view(torch.int16 if c.dtype == "bf16" else torch.int32))
        _RUNS[name] = (out, dict(logits=logits, uncond=uncond, ctr=ctr, pos=pos))
    return _RUNS[name]


def _ulp_apart(a, b):
    ia, ib = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _check(c, out, rows, pos):
    B = len(rows)
    col = [c.K - 1] * B if pos is None else [int(p) for p in pos]
    want_ids = np.full((B, c.K), SENT, np.int64)
    for b, r in enumerate(rows):
        want_ids[b, col[b]] = r.id
    assert np.array_equal(out["ids"].astype(np.int64), want_ids), (c.name, "ids", [(b, int(out["ids"][b, col[b]]), r.id) for b, r in enumerate(rows) if out["ids"][b, col[b]] != r.id][:4])
    assert out["ids"].dtype == (np.int32 if c.ids == "int32" else np.int64)
    assert out["n_kept"].tolist() == [r.n_kept for r in rows], (c.name, "n_kept")
    assert [tuple(int(v) for v in m) for m in out["mass"]] == [(r.q_total, r.q_kept, r.q_id) for r in rows], (c.name, "mass")
    good = np.array([not r.bad for r in rows])
    want_lp = np.array([r.logprob for r in rows], f32)
    assert np.isnan(out["logprob"][~good]).all() and (_ulp_apart(out["logprob"][good], want_lp[good]) <= 1).all(), (c.name, out["logprob"], want_lp)
    assert out["bad"] == int((~good).sum())


@pytest.mark.parametrize("name", [c.name for c in TC.CASES])
def test_token_sample_equals_the_emulation(name):
    """id, n_kept and the three masses equal, logprob within 1 fp32 ulp, nothing written outside what is stated (sentinels and guard rows), bad rows write id -1,
    n_kept 0, zero masses, NaN and count once each; the logits are only read"""
    c = TC.BY_NAME[name]
    out, dev = run_case(name)
    _check(c, out, TC.reference(name), TC.make(name)["pos"])


@pytest.mark.parametrize("name", ["c4096_B64", "c32768_cfg_vlm_pos", "c65536_k50_p90", "four_bf16_T07", "bad_rows"])
def test_run_to_run_alone_and_in_any_row_order(name):
    """the same bits again; each row alone gives what it gave in the batch; the rows reversed, counters and positions carried along, give the reversed outputs"""
    c = TC.BY_NAME[name]
    out, dev = run_case(name)
    again = _launch(c, dev["logits"], dev["uncond"], dev["ctr"], dev["pos"])
    for k in ("ids", "n_kept", "mass"):
        assert np.array_equal(out[k], again[k]), (name, k)
    assert out["logprob"].tobytes() == again["logprob"].tobytes() and out["bad"] == again["bad"]
    col = lambda o, b, p: o["ids"][b, c.K - 1 if p is None else int(p[b])]
    pos_h = TC.make(name)["pos"]
    for b in sorted({0, c.B // 2, c.B - 1}):
        one = _launch(c, dev["logits"][b:b + 1], None if dev["uncond"] is None else dev["uncond"][b:b + 1], dev["ctr"][b:b + 1].contiguous(),
                      None if dev["pos"] is None else dev["pos"][b:b + 1].contiguous())
        assert col(one, 0, None if pos_h is None else pos_h[b:b + 1]) == col(out, b, pos_h) and one["n_kept"][0] == out["n_kept"][b]
        assert np.array_equal(one["mass"][0], out["mass"][b]) and one["logprob"][:1].tobytes() == out["logprob"][b:b + 1].tobytes()
    perm = torch.arange(c.B - 1, -1, -1, device="cuda")
    lg = dev["logits"][perm].contiguous()
    un = None if dev["uncond"] is None else dev["uncond"][perm].contiguous()
    rev = _launch(c._replace(row=c.row), lg, un, dev["ctr"][perm].contiguous(), None if dev["pos"] is None else dev["pos"][perm].contiguous())
    p = perm.cpu().numpy()
    assert np.array_equal(rev["ids"], out["ids"][p]) and np.array_equal(rev["n_kept"], out["n_kept"][p]) and np.array_equal(rev["mass"], out["mass"][p])
    assert rev["logprob"].tobytes() == out["logprob"][p].tobytes()


@pytest.mark.parametrize("name", ["c256_bf16_p50", "c1000_bf16_cfg_vlm", "c32768_bf16_T4_p999", "c65536_bf16_cfg_p50"])
def test_bf16_equals_the_same_values_widened_to_fp32(name):
    c = TC.BY_NAME[name]
    out, dev = run_case(name)
    wide = _launch(c._replace(dtype="f32"), dev["logits"].float(), None if dev["uncond"] is None else dev["uncond"].float(), dev["ctr"], dev["pos"])
    for k in ("ids", "n_kept", "mass"):
        assert np.array_equal(out[k], wide[k]), (name, k)
    assert out["logprob"].tobytes() == wide["logprob"].tobytes()


@pytest.mark.parametrize("name", ["c255_k50_p90", "c32767_kC_p50", "four_k300_p50"])
def test_no_guidance_equals_guidance_of_scale_one_on_equal_logits_and_k_equal_C_equals_off(name):
    """s = 1 with lu = lc: lc - lu is exactly +0 for every finite logit, 1 * 0 = 0 and lu + 0 = lu = lc (a -0.0 becomes +0.0, which the key counts as equal
    anyway): the guided path is EXACT on finite logits, so the two calls agree bit for bit.  (-inf would differ: inf - inf is NaN; none of these cases has one.)
    top_k = C, C + 1 and 2^31 - 1 are the launch of top-k off."""
    c = TC.BY_NAME[name]
    assert not c.guided and np.isfinite(TC.windows(name)[0]).all()
    out, dev = run_case(name)
    same = _launch(c, dev["logits"], dev["logits"].clone(), dev["ctr"], dev["pos"], cfg_scale=1.0)
    for k in ("ids", "n_kept", "mass"):
        assert np.array_equal(out[k], same[k]), (name, k)
    assert out["logprob"].tobytes() == same["logprob"].tobytes()
    off = _launch(c, dev["logits"], None, dev["ctr"], dev["pos"], top_k=0)
    for kk in (c.C, c.C + 1, 2 ** 31 - 1):
        full = _launch(c, dev["logits"], None, dev["ctr"], dev["pos"], top_k=kk)
        assert all(np.array_equal(off[k], full[k]) for k in ("ids", "n_kept", "mass")) and off["logprob"].tobytes() == full["logprob"].tobytes()


def test_graph_replay_equals_eager():
    name = "c32768_cfg_vlm_pos"
    c = TC.BY_NAME[name]
    out, dev = run_case(name)
    idt = torch.int64
    ids = torch.full((c.B, c.K), SENT, dtype=idt, device="cuda")
    nk, mass = torch.zeros(c.B, dtype=torch.int32, device="cuda"), torch.zeros(c.B, 3, dtype=torch.int64, device="cuda")
    lp, bad = torch.zeros(c.B, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda: ops.token_sample(dev["logits"], dev["ctr"], ids, uncond_logits=dev["uncond"], C=c.C, offset=c.offset, cfg_scale=c.s, temperature=c.T, top_k=c.k,
                                    top_p=c.P, seed=c.seed, pos=dev["pos"], n_kept=nk, mass=mass, logprob=lp, bad=bad)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in (ids, nk, mass, lp):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    pos_h = TC.make(name)["pos"]
    assert [int(ids[b, pos_h[b]]) for b in range(c.B)] == [int(out["ids"][b, pos_h[b]]) for b in range(c.B)]
    assert np.array_equal(nk.cpu().numpy(), out["n_kept"]) and np.array_equal(mass.cpu().numpy().view(np.uint64), out["mass"])
    assert lp.cpu().numpy().tobytes() == out["logprob"].tobytes()


def _hash_logits(B, V, step, salt):
    """deterministic pseudo-logits in [-4, 4), a function of (row, code, step) alone"""
    i = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(1000003) + np.arange(V, dtype=np.uint64)[None, :]) * np.uint64(2654435761) + np.uint64(step * 97 + salt)
    i = (i ^ (i >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    i = (i ^ (i >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
    return ((i >> np.uint64(8)).astype(np.float64) / 2.0 ** 24 * 8.0 - 4.0).astype(f32)


def test_token_sampler_equals_the_emulation_stepped_on_the_host():
    """K = 40 steps at B = 3, guidance, temperature, top-k and top-p on: AR step s lands at tokenizer position K - 1 - s; no synchronisation inside step();
    a state round trip after 25 steps continues bit for bit"""
    K, B, C, off, V = 40, 3, 1000, 8, 1024
    kw = dict(C=C, offset=off, temperature=0.7, top_k=50, top_p=0.9, cfg_scale=2.0, seed=(0xABCD << 32) | 0x1234)
    s = sampling.TokenSampler(K, **kw).begin(B, tickets=[7, 1 << 31, 12345])
    lc = [torch.from_numpy(_hash_logits(B, V, t, 1)).cuda() for t in range(K)]
    lu = [torch.from_numpy(_hash_logits(B, V, t, 2)).cuda() for t in range(K)]
    torch.cuda.synchronize()
    resumed = None
    for t in range(K):
        if t == 25:
            resumed = sampling.TokenSampler(K, **kw).load_state(s.state())
        torch.cuda.set_sync_debug_mode("error")
        try:
            s.step(lc[t], lu[t])
        finally:
            torch.cuda.set_sync_debug_mode("default")
        if resumed is not None:
            resumed.step(lc[t], lu[t])
    ids, m = s.partial()
    assert m == K and ids.shape == (B, K) and ids.dtype == torch.int64
    want = np.zeros((B, K), np.int64)
    want_nk, want_lp = np.zeros((B, K), np.int32), np.zeros((B, K), f32)
    for t in range(K):
        a, u = lc[t].cpu().numpy()[:, off:off + C], lu[t].cpu().numpy()[:, off:off + C]
        for b, ticket in enumerate((7, 1 << 31, 12345)):
            r = TC.sample_row(a[b], u[b], s=2.0, temperature=0.7, top_k=50, top_p=0.9, seed=kw["seed"], ctr=(ticket, t))
            want[b, K - 1 - t], want_nk[b, K - 1 - t], want_lp[b, K - 1 - t] = r.id, r.n_kept, r.logprob
    assert np.array_equal(ids.cpu().numpy(), want) and np.array_equal(s.n_kept.cpu().numpy(), want_nk) and int(s.bad.cpu()[0]) == 0
    assert (_ulp_apart(s.logprob.cpu().numpy(), want_lp) <= 1).all() and len(set(want.reshape(-1).tolist())) > 30
    assert torch.equal(resumed.ids, ids) and torch.equal(resumed.ctr, s.ctr) and resumed.logprob.cpu().numpy().tobytes() == s.logprob.cpu().numpy().tobytes()
    assert s.ctr.cpu().tolist() == [[7, K], [-(1 << 31), K], [12345, K]]
    # rows at different AR steps share a call: each gives what it gave in step with the others
    r = sampling.TokenSampler(K, **kw).begin(B, tickets=[7, 1 << 31, 12345], steps=[0, 5, 39])
    mixed = torch.stack([lc[0][0], lc[5][1], lc[39][2]]), torch.stack([lu[0][0], lu[5][1], lu[39][2]])
    r.step(*mixed)
    got, mm = r.partial()
    assert list(mm) == [1, 6, 40] and [int(got[0, K - 1]), int(got[1, K - 6]), int(got[2, 0])] == [want[0, K - 1], want[1, K - 6], want[2, 0]]


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    p = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"))
    p.verbose = False
    return p


def test_partial_goes_through_decoding(pipe):
    """37 steps of K = 512 over the 32768 codes: partial() feeds decoding(ar_partial=m) directly and gives the pixels of the same ids placed by pad_ar_partial"""
    K, B, steps = 512, 2, 37
    s = sampling.TokenSampler(K, temperature=1.0, top_k=50, top_p=0.9, seed=99).begin(B)
    for t in range(steps):
        s.step(torch.from_numpy(_hash_logits(B, 32768, t, 3)).cuda())
    ids, m = s.partial()
    assert m == steps and int(s.bad.cpu()[0]) == 0
    emitted = ids.cpu().numpy()[:, K - steps:][:, ::-1]                # in the order the model emitted them
    placed, m2 = tokens.pad_ar_partial(np.ascontiguousarray(emitted), K)
    assert np.array_equal(placed, ids.cpu().numpy()) and m2.tolist() == [steps] * B and len(set(emitted.reshape(-1).tolist())) > steps
    noise = synth.synthetic_noise(B, first_index=40)
    a = pipe.decoding(ids, noise=noise, max_steps=2, ar_partial=m)
    b = pipe.decoding(placed, noise=noise, max_steps=2, ar_partial=m2)
    assert torch.isfinite(a.float()).all() and torch.equal(a, b)
