"""-m gpu: the token scorer (csrc/token_score.hip through ops.token_score and sampling.score_tokens) against the numpy arithmetic of record of
tests/token_score_cases.py: rank, first code, both masses and the bad / ignored counts equal on every case inside guard bands, logprob and entropy within 1
fp32 ulp (the device's fp64 log may differ from numpy's in the last place before the one rounding to fp32; S_h itself is not an output, the entropy is its
only image), the invariances bit for bit, and the existing sampler kernel held to this one by equality."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import token_score_cases as SC
from selftoktokenizer_amd import ops, sampling

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENT = 64, -777                                              # guard elements either side of the logits (a multiple of four codes); the output sentinel
f32 = np.float32


def _dev_logits(c, host):
    """host [R, row] (fp32, or bf16 bits) -> a [R, row] device view inside a flat buffer with NaN guard bands"""
    if host is None:
        return None, None
    t = torch.from_numpy(host.view(np.int16) if c.dtype == "bf16" else host)
    t = t.view(torch.bfloat16) if c.dtype == "bf16" else t
    flat = torch.full((GUARD + t.numel() + GUARD,), float("nan"), dtype=t.dtype, device="cuda")
    flat[GUARD:GUARD + t.numel()] = t.reshape(-1).cuda()
    return flat[GUARD:GUARD + t.numel()].view(host.shape[0], c.row), flat


def _dev_ids(c, host):
    """the id buffer on the device and the [B, S] view the case describes (torch strides are positive: a negative step stride is `reverse_steps`)"""
    _, base, seq, step = SC.id_geometry(c)
    buf = torch.from_numpy(host).cuda()
    lo = base if step > 0 else base + (c.S - 1) * step
    return torch.as_strided(buf, (c.B, c.S), (seq, abs(step)), lo), step < 0, buf


def _launch(logits, ids, *, reverse=False, **kw):
    """one call with sentinel-filled, guard-banded outputs -> dict of host arrays over the R rows (guards checked here)"""
    R = logits.shape[0] if logits.dim() == 2 else logits.shape[0] * logits.shape[1]
    lp = torch.full((R + 2,), 123.0, dtype=torch.float32, device="cuda")
    ent = torch.full((R + 2,), 123.0, dtype=torch.float32, device="cuda")
    mass = torch.full((R + 2, 2), SENT, dtype=torch.int64, device="cuda")
    rank = torch.full((R + 2,), SENT, dtype=torch.int32, device="cuda")
    top = torch.full((R + 2,), SENT, dtype=torch.int32, device="cuda")
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    shape = tuple(logits.shape[:-1])
    ops.token_score(logits, ids, reverse_steps=reverse, logprob=lp[1:R + 1].view(shape), mass=mass[1:R + 1].view(shape + (2,)), rank=rank[1:R + 1].view(shape),
                    top_id=top[1:R + 1].view(shape), entropy=ent[1:R + 1].view(shape), bad=bad, ignored=ign, **kw)
    torch.cuda.synchronize()
    h = [t.cpu().numpy() for t in (lp, ent, mass, rank, top)]
    assert (h[0][[0, -1]] == 123.0).all() and (h[1][[0, -1]] == 123.0).all(), "an output guard row was written"
    for g in h[2:]:
        assert (g[[0, -1]] == SENT).all(), "an output guard row was written"
    return dict(logprob=h[0][1:-1], entropy=h[1][1:-1], mass=h[2][1:-1].view(np.uint64), rank=h[3][1:-1], top_id=h[4][1:-1], bad=int(bad.cpu()[0]), ignored=int(ign.cpu()[0]))


def _kw(c, uncond):
    return dict(uncond_logits=uncond, C=c.C, offset=c.offset, cfg_scale=c.s, temperature=c.T)


_RUNS = {}


def run_case(name):
    """the case on the device, once: (result, the device inputs)"""
    if name not in _RUNS:
        c, d = SC.BY_NAME[name], SC.make(name)
        logits, lflat = _dev_logits(c, d["logits"])
        uncond, _ = _dev_logits(c, d["uncond"])
        ids, reverse, buf = _dev_ids(c, d["ids"])
        bits = torch.int16 if c.dtype == "bf16" else torch.int32
        before, ids_before = lflat.view(bits).clone(), buf.clone()
        out = _launch(logits, ids, reverse=reverse, **_kw(c, uncond))
        assert torch.equal(lflat.view(bits), before) and torch.equal(buf, ids_before)          # the inputs are only read
        _RUNS[name] = (out, dict(logits=logits, uncond=uncond, ids=ids, reverse=reverse))
    return _RUNS[name]


def _ulp_apart(a, b):
    ia, ib = np.asarray(a, f32).view(np.int32).astype(np.int64), np.asarray(b, f32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def _same_bits(a, b, keys=("logprob", "entropy", "mass", "rank", "top_id")):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys) and a["bad"] == b["bad"] and a["ignored"] == b["ignored"]


def _check(name, out, ref):
    good = ~ref.bad
    assert out["rank"].tolist() == ref.rank.tolist(), (name, "rank")
    assert out["top_id"].tolist() == ref.top_id.tolist(), (name, "top_id")
    assert np.array_equal(out["mass"][:, 0], ref.q_total) and np.array_equal(out["mass"][:, 1], ref.q_t), (name, "mass")
    assert out["bad"] == int(ref.bad.sum()) and out["ignored"] == int(ref.ignored.sum()), (name, out["bad"], out["ignored"])
    assert np.isnan(out["logprob"][~good]).all() and np.isnan(out["entropy"][~good]).all()
    assert (_ulp_apart(out["logprob"][good], ref.logprob[good]) <= 1).all(), (name, "logprob", out["logprob"][good][:4], ref.logprob[good][:4])
    assert (_ulp_apart(out["entropy"][good], ref.entropy[good]) <= 1).all(), (name, "entropy", out["entropy"][good][:4], ref.entropy[good][:4])
    assert (out["logprob"][ref.ignored].view(np.uint32) == 0).all()                               # +0.0 exactly


@pytest.mark.parametrize("name", [c.name for c in SC.CASES])
def test_token_score_equals_the_emulation(name):
    """rank, top_id and both masses equal, logprob and entropy within 1 fp32 ulp, nothing written outside what is stated (sentinels and guard rows); bad rows
    write NaN, -1, -1, zero masses, NaN and count once each, ignored rows 0.0, -1, q_t 0 beside their Q_total, top_id and entropy; the inputs are only read"""
    out, _ = run_case(name)
    _check(name, out, SC.reference(name))


@pytest.mark.parametrize("name", ["c4096_R64", "c32768_bf16_T4", "c65536", "four_bf16_T07", "bad_rows", "ignored"])
def test_run_to_run_alone_and_in_any_row_order(name):
    """the same bits again; a row alone gives what it gave in the batch; the rows reversed give the reversed outputs -- a bad or ignored row beside it or not"""
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    kw = _kw(c, dev["uncond"])
    assert _same_bits(out, _launch(dev["logits"], dev["ids"], reverse=dev["reverse"], **kw))
    R = SC.rows_of(c)
    t = torch.from_numpy(SC.make(name)["targets"]).cuda()
    keys = ("logprob", "entropy", "mass", "rank", "top_id")
    for r in sorted({0, 1, R // 2, R - 1}):
        one = _launch(dev["logits"][r:r + 1], t[r:r + 1], **dict(kw, uncond_logits=None if dev["uncond"] is None else dev["uncond"][r:r + 1]))
        assert all(one[k][0].tobytes() == out[k][r].tobytes() for k in keys), (name, r)
    perm = torch.arange(R - 1, -1, -1, device="cuda")
    rev = _launch(dev["logits"][perm].contiguous(), t[perm].contiguous(), **dict(kw, uncond_logits=None if dev["uncond"] is None else dev["uncond"][perm].contiguous()))
    p = perm.cpu().numpy()
    assert all(rev[k].tobytes() == out[k][p].tobytes() for k in keys) and rev["bad"] == out["bad"] and rev["ignored"] == out["ignored"]


@pytest.mark.parametrize("name", ["c256_bf16", "c2048_bf16_cfg", "c4097_bf16_S40", "c32768_bf16_T4", "c32769_bf16_cfg", "c65536_bf16_cfg"])
def test_bf16_equals_the_same_values_widened_to_fp32(name):
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    wide = _launch(dev["logits"].float(), dev["ids"], reverse=dev["reverse"], **_kw(c, None if dev["uncond"] is None else dev["uncond"].float()))
    assert _same_bits(out, wide)


@pytest.mark.parametrize("name", ["c255_T07", "c2049_T4", "c32767_T4", "c32769", "four"])
def test_no_guidance_equals_guidance_of_scale_one_on_equal_logits(name):
    """s = 1 with lu = lc: lc - lu is exactly +0 for every finite logit, 1 * 0 = 0 and lu + 0 = lc: the guided kernels are EXACT here"""
    c = SC.BY_NAME[name]
    assert not c.guided and np.isfinite(SC.windows(name)[0]).all()
    out, dev = run_case(name)
    assert _same_bits(out, _launch(dev["logits"], dev["ids"], reverse=dev["reverse"], **dict(_kw(c, dev["logits"].clone()), cfg_scale=1.0)))


@pytest.mark.parametrize("name", ["c5_S3_rev", "c4096_S40_rev", "c2050_int32_wide", "c1000_bf16_cfg_vlm_wide_rev", "c32768_cfg_vlm", "ignored_int32_rev"])
def test_three_dimensional_logits_and_reversed_steps_equal_the_flat_call(name):
    """[B, S, V] logits give what their [B * S, V] rows give; ids walked backwards in place (step stride -1 or -2) give what a materialised flip gives"""
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    lg3 = dev["logits"].view(c.B, c.S, c.row)
    un3 = None if dev["uncond"] is None else dev["uncond"].view(c.B, c.S, c.row)
    assert _same_bits(out, _launch(lg3, dev["ids"], reverse=dev["reverse"], **_kw(c, un3)))
    dense = (dev["ids"].flip(1) if dev["reverse"] else dev["ids"]).contiguous()
    assert _same_bits(out, _launch(lg3, dense, **_kw(c, un3)))
    assert _same_bits(out, _launch(dev["logits"], dense.reshape(-1), **_kw(c, dev["uncond"])))
    assert _same_bits(out, _launch(dev["logits"], dense.reshape(-1), rows_per_seq=c.S, **_kw(c, dev["uncond"])))


def test_graph_replay_equals_eager():
    name = "c32768_cfg_vlm"
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    R = SC.rows_of(c)
    lp, ent = torch.zeros(c.B, c.S, device="cuda"), torch.zeros(c.B, c.S, device="cuda")
    mass, rank, top = torch.zeros(c.B, c.S, 2, dtype=torch.int64, device="cuda"), torch.zeros(c.B, c.S, dtype=torch.int32, device="cuda"), torch.zeros(c.B, c.S, dtype=torch.int32, device="cuda")
    bad, ign = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    lg3, un3 = dev["logits"].view(c.B, c.S, c.row), dev["uncond"].view(c.B, c.S, c.row)
    call = lambda: ops.token_score(lg3, dev["ids"], reverse_steps=dev["reverse"], logprob=lp, mass=mass, rank=rank, top_id=top, entropy=ent, bad=bad, ignored=ign, **_kw(c, un3))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    for t in (lp, ent, mass, rank, top):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    got = dict(logprob=lp.cpu().numpy().reshape(R), entropy=ent.cpu().numpy().reshape(R), mass=mass.cpu().numpy().view(np.uint64).reshape(R, 2),
               rank=rank.cpu().numpy().reshape(R), top_id=top.cpu().numpy().reshape(R), bad=out["bad"], ignored=out["ignored"])
    assert _same_bits(out, got)


def test_no_rows_and_accumulating_counters():
    lg = torch.zeros(0, 128, device="cuda")
    lp, mass, rank, top, ent, bad, ign = ops.token_score(lg, torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert lp.shape == (0,) and mass.shape == (0, 2) and rank.shape == (0,) and int(bad.cpu()[0]) == 0 and int(ign.cpu()[0]) == 0
    name = "bad_rows"
    c = SC.BY_NAME[name]
    out, dev = run_case(name)
    bad, ign = torch.full((1,), 10, dtype=torch.int32, device="cuda"), torch.full((1,), 20, dtype=torch.int32, device="cuda")
    t = torch.from_numpy(SC.make(name)["targets"]).cuda()
    t[0] = -5
    for _ in range(2):
        ops.token_score(dev["logits"], t, bad=bad, ignored=ign, **_kw(c, dev["uncond"]))
    assert int(bad.cpu()[0]) == 10 + 2 * out["bad"] and int(ign.cpu()[0]) == 20 + 2
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(C=c.C + 1, offset=c.row - c.C), dict(rows_per_seq=2)):
        with pytest.raises(Exception):
            ops.token_score(dev["logits"], t, **dict(_kw(c, dev["uncond"]), **kw))


def _hash_logits(B, V, step, salt):
    """deterministic pseudo-logits in [-4, 4), a function of (row, code, step) alone"""
    i = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(1000003) + np.arange(V, dtype=np.uint64)[None, :]) * np.uint64(2654435761) + np.uint64(step * 97 + salt)
    i = (i ^ (i >> np.uint64(15))) * np.uint64(0x2C1B3C6D) & np.uint64(0xFFFFFFFF)
    i = (i ^ (i >> np.uint64(12))) * np.uint64(0x297A2D39) & np.uint64(0xFFFFFFFF)
    return ((i >> np.uint64(8)).astype(np.float64) / 2.0 ** 24 * 8.0 - 4.0).astype(f32)


def test_the_sampler_kernel_and_the_scorer_kernel_share_one_arithmetic():
    """TokenSampler for 40 steps at B = 3 with guidance, temperature, top-k and top-p, the logits of every step kept; score_tokens of those logits against
    partial()'s ids returns the sampler's logprob, Q_total and q_id bit for bit and rank < n_kept on every row; a greedy run's ids are top_id"""
    K, B, C, off, V = 40, 3, 1000, 8, 1024
    kw = dict(C=C, offset=off, temperature=0.7, top_k=50, top_p=0.9, cfg_scale=2.0, seed=(0xABCD << 32) | 0x1234)
    lc = torch.stack([torch.from_numpy(_hash_logits(B, V, t, 1)) for t in range(K)], dim=1).cuda()         # [B, K, V], AR order
    lu = torch.stack([torch.from_numpy(_hash_logits(B, V, t, 2)) for t in range(K)], dim=1).cuda()
    s = sampling.TokenSampler(K, **kw).begin(B)
    g = sampling.TokenSampler(K, **dict(kw, temperature=0.0)).begin(B)
    masses = []
    for t in range(K):
        s.step(lc[:, t], lu[:, t])
        masses.append(s._row_mass.clone())
        g.step(lc[:, t], lu[:, t])
    ids, m = s.partial()
    assert m == K and int(s.bad.cpu()[0]) == 0
    sc = sampling.score_tokens(lc, ids, uncond_logits=lu, cfg_scale=2.0, temperature=0.7, C=C, offset=off)
    assert int(sc.bad.cpu()[0]) == 0 and int(sc.ignored.cpu()[0]) == 0 and sc.positions.tolist() == list(range(K - 1, -1, -1))
    ar = lambda x: x.flip(1)                                        # [B, K] by tokenizer position -> by AR step
    assert sc.logprob.cpu().numpy().tobytes() == ar(s.logprob).contiguous().cpu().numpy().tobytes()
    mm = torch.stack(masses, dim=1)                                 # [B, K, 3] by AR step: (Q_total, Q_kept, q_id)
    assert torch.equal(sc.mass[..., 0], mm[..., 0]) and torch.equal(sc.mass[..., 1], mm[..., 2])
    assert bool((sc.rank >= 0).all()) and bool((sc.rank < ar(s.n_kept)).all())
    top1 = sampling.score_tokens(lc, ids, uncond_logits=lu, cfg_scale=2.0, temperature=1.0, C=C, offset=off).top_id
    assert torch.equal(top1.to(torch.int64), ar(g.partial()[0]))
    assert float(sc.nll()) == pytest.approx(-float(s.logprob.double().mean()), rel=1e-12) and sc.per_position_nll().shape == (K,)
    # the first 25 AR steps alone are positions K - 25 .. K - 1, as partial() after 25 steps has them
    part = sampling.score_tokens(lc[:, :25].contiguous(), ids, uncond_logits=lu[:, :25].contiguous(), cfg_scale=2.0, temperature=0.7, C=C, offset=off)
    assert part.logprob.cpu().numpy().tobytes() == sc.logprob[:, :25].contiguous().cpu().numpy().tobytes() and part.positions.tolist() == list(range(K - 1, K - 26, -1))
    masked = sampling.score_tokens(lc, ids, steps=[40, 25, 0], uncond_logits=lu, cfg_scale=2.0, temperature=0.7, C=C, offset=off)
    assert int(masked.ignored.cpu()[0]) == 15 + 40 and masked.sequence_logprob().cpu().tolist()[0] == sc.sequence_logprob().cpu().tolist()[0]
    assert torch.equal(masked.top_id, sc.top_id) and masked.entropy.cpu().numpy().tobytes() == sc.entropy.cpu().numpy().tobytes()


def test_score_tokens_tool_runs_on_synthetic_data():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "score_tokens.py"), "--synthetic", "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "perplexity" in r.stdout and "top-5" in r.stdout and "position" in r.stdout, r.stdout
