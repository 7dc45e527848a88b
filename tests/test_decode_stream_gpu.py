"""-m gpu: the decode stream (SelftokPipeline.decode_stream / decoding_stream, csrc/decode_stream.hip): the two kernels against the emulation of
tests/decode_stream_cases.py and against the existing Euler entry, and the stream on the real MMDiT against the reference's own sampler
(tests/golden/ar_partial_b4.npz), against `decoding`, and against itself (slot and neighbour independence, restart after an overflow)."""
import os

import numpy as np
import pytest
import torch

import decode_stream_cases as DS
from selftoktokenizer_amd import ops, synth, tokens, weights as W
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.pipeline import DecodeStream, StreamFull

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
K = 512


def _dev(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a))
    return t.cuda() if dtype is None else t.to(dtype).cuda()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


# ---- the kernels -----------------------------------------------------------------------------------------
def _guarded(n, dtype, guard=64):
    """a buffer of n elements between two NaN (or -1) guard bands -> (whole, the n elements)"""
    whole = torch.full((n + 2 * guard,), float("nan") if dtype == torch.float32 else -1, dtype=dtype, device="cuda")
    return whole, whole[guard:guard + n]


def _guards_intact(whole, n, guard=64):
    g = torch.cat([whole[:guard], whole[guard + n:]])
    return bool(torch.isnan(g).all()) if whole.dtype == torch.float32 else bool((g == -1).all())


@pytest.mark.parametrize("case", DS.CASES, ids=lambda c: c.name)
def test_prepare_and_rows_euler_equal_the_emulation(case):
    d, want = DS.inputs(case), DS.outcome(case)
    B, Wd, R = case.B, case.W, case.R
    kw_all, kw = _guarded(B * Wd, torch.int32)
    cf_all, cf = _guarded(B * 4, torch.float32)
    m_all, m = _guarded(B * R, torch.float32)
    mu_all, mu = _guarded(B * R, torch.float32) if case.guided else (None, None)
    step = _dev(d["step"])
    ops.stream_prepare(step, _dev(d["limit"]), _dev(d["coef"]), _dev(d["pattern_words"]), _dev(d["table"]), _dev(d["table_u"]), d["segs"],
                       kw.view(B, Wd), cf.view(B, 4), m, mu, K=case.K)
    assert np.array_equal(_bits(kw).reshape(B, Wd), want["kwords"]) and np.array_equal(_bits(cf).reshape(B, 4), want["coef_rows"].view(np.uint32))
    assert np.array_equal(_bits(m), want["mods"].view(np.uint32))
    assert _guards_intact(kw_all, B * Wd) and _guards_intact(cf_all, B * 4) and _guards_intact(m_all, B * R)
    if case.guided:
        assert np.array_equal(_bits(mu), want["mods_u"].view(np.uint32)) and _guards_intact(mu_all, B * R)
    n = d["x"].size
    x_all, x_out = _guarded(n, torch.float32)
    s_all, s_out = _guarded(B, torch.int32)
    x = _dev(d["x"])
    ops.unpatchify_cfg_euler_rows(_dev(d["y"]), _dev(d["yu"]), x, cf.view(B, 4), step, cfg_scale=d["cfg_scale"], x0_param=case.x0,
                                  x_out=x_out.view(x.shape), step_out=s_out)
    assert np.array_equal(_bits(x_out).reshape(d["x"].shape), want["x"].view(np.uint32)) and np.array_equal(s_out.cpu().numpy(), want["step"])
    assert _guards_intact(x_all, n) and _guards_intact(s_all, B)
    assert np.array_equal(_bits(x), d["x"].view(np.uint32)) and np.array_equal(step.cpu().numpy(), d["step"])      # out of place: the inputs stay
    ops.unpatchify_cfg_euler_rows(_dev(d["y"]), _dev(d["yu"]), x, cf.view(B, 4), step, cfg_scale=d["cfg_scale"], x0_param=case.x0)   # in place: the same
    assert torch.equal(x, x_out.view(x.shape)) and torch.equal(step, s_out)


@pytest.mark.parametrize("hw", [2, 16])
@pytest.mark.parametrize("guided", [False, True], ids=["cond", "cfg"])
def test_rows_euler_equals_the_existing_entry_and_torch(hw, guided):
    """per active slot the bits of selftok_unpatchify_cfg_euler_f32 with that slot's dt; in x0 mode the torch expression of p_sample_loop; idle
    slots byte for byte, NaN payloads included, with y NaN there too"""
    B, C = 5, 16
    g = torch.Generator(device="cuda").manual_seed(7 + hw)
    y = torch.randn(B, hw * hw, 4 * C, device="cuda", generator=g)
    yu = torch.randn(B, hw * hw, 4 * C, device="cuda", generator=g) if guided else None
    x = torch.randn(B, C, 2 * hw, 2 * hw, device="cuda", generator=g)
    active = [True, False, True, True, False]
    sched = np.array([[0.019999981, 0.98, 0.96, 0], [0.5, 0.5, 0.5, 0], [0.020000011, 0.3, 0.28, 0], [0.02, 0.02, 0.0, 0], [0.1, 0.2, 0.3, 0]], np.float32)
    coef = torch.from_numpy(sched).cuda()
    coef[:, 3] = torch.tensor(active, device="cuda").float()
    step = torch.tensor([0, -1, 17, 49, 50], dtype=torch.int32, device="cuda")
    idle = [b for b in range(B) if not active[b]]
    x.view(torch.int32)[idle] = 0x7FC12345
    y[idle] = float("nan")
    if guided:
        yu[idle] = float("nan")
    scale = 2.0 if guided else 1.0
    for x0 in (False, True):
        xo, so = torch.zeros_like(x), torch.zeros_like(step)
        ops.unpatchify_cfg_euler_rows(y, yu, x, coef, step, cfg_scale=scale, x0_param=x0, x_out=xo, step_out=so)
        assert so.tolist() == [1, -1, 18, 50, 50]
        for b in range(B):
            sl = slice(b, b + 1)
            if not active[b]:
                assert torch.equal(xo[sl].view(torch.int32), x[sl].view(torch.int32))
            elif x0:
                _, v = ops.unpatchify_cfg_euler(y[sl].contiguous(), None, 0.0, y_uncond=None if yu is None else yu[sl].contiguous(), cfg_scale=scale, C=C, hp=hw, wp=hw)
                want = v + float(sched[b, 2]) * (x[sl] - v) / float(sched[b, 1])
                assert torch.equal(xo[sl], want), (b, float((xo[sl] - want).abs().max()))
            else:
                want, _ = ops.unpatchify_cfg_euler(y[sl].contiguous(), x[sl].contiguous(), float(sched[b, 0]), y_uncond=None if yu is None else yu[sl].contiguous(),
                                                   cfg_scale=scale, C=C, hp=hw, wp=hw)
                assert torch.equal(xo[sl], want), b
        xi, si = x.clone(), step.clone()
        ops.unpatchify_cfg_euler_rows(y, yu, xi, coef, si, cfg_scale=scale, x0_param=x0)
        assert torch.equal(xi.view(torch.int32), xo.view(torch.int32)) and torch.equal(si, so)


# ---- the stream on the real MMDiT ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    p = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd,
                        vae_state_dict=W.synthetic_vae_state_dict(device="cuda"))
    p.verbose = False
    return p


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "ar_partial_b4.npz"))


@pytest.fixture(scope="module")
def noise():
    return synth.synthetic_noise(5, first_index=40)


@pytest.fixture(scope="module")
def ids5(gold):
    return np.concatenate([gold["ids"], synth.synthetic_token_ids(1, first_index=9)])


M5 = (512, 301, 37, 1, 200)


@pytest.fixture(scope="module")
def baseline(pipe, gold, noise):
    """`decoding` before any stream existed (fp32 and f16x2): test_decoding_keeps_its_bits compares at the end of the module"""
    out = {}
    for gemm in ("fp32", "f16x2"):
        assert pipe.set_gemm(gemm) == gemm
        out[gemm] = pipe.decoding(gold["ids"][:2], noise=noise[:2], max_steps=2, return_latent=True, ar_partial=[301, 37])
    pipe.set_gemm("fp32")
    return out


class _mode:
    def __init__(self, pipe, gemm, param="velocity"):
        self.pipe, self.gemm, self.param = pipe, gemm, param

    def __enter__(self):
        assert self.pipe.set_gemm(self.gemm) == self.gemm
        self.pipe.flow.parameterization = self.param

    def __exit__(self, *a):
        self.pipe.flow.parameterization = "velocity"
        self.pipe.set_gemm("fp32")


def _run(stream, plan, ids, noise, m=None):
    """plan: {stream step: [request indices admitted before it]} -> {request: latent}, stepping until empty"""
    out, owner, i = {}, {}, 0
    while i <= max(plan) or stream.in_flight:
        for r in plan.get(i, ()):
            owner[stream.submit(ids[r], noise=noise[r], ar_partial=None if m is None else int(m[r]))] = r
        for ticket, pixels, latent in stream.step():
            out[owner[ticket]] = (pixels, latent)
        i += 1
    return out


@pytest.mark.parametrize("gemm", ["fp32", "f16x2"])
def test_stream_vs_reference(pipe, gold, baseline, gemm):
    """the four requests of ar_partial_b4.npz admitted at stream steps 0, 1, 1 and 3 into 3 slots, each with its own ar_partial: every request's latent
    after ITS steps 1 and 2 against the reference's sampler, max abs error < 2e-5 (the standing gate of the same sampler reached by another route)"""
    noise = synth.synthetic_noise(4, first_index=40)
    admit = {0: [0], 1: [1, 2], 3: [3]}
    with _mode(pipe, gemm):
        stream = pipe.decode_stream(3, max_steps=2, return_latent=True)
        owner, seen, errs = {}, {r: [] for r in range(4)}, []
        for i in range(5):
            for r in admit.get(i, ()):
                owner[stream.submit(gold["ids"][r], noise=noise[r], ar_partial=int(gold["m"][r]))] = r
            mid = {owner[t]: s for s, t in enumerate(stream.sched.ticket) if t is not None and stream.sched.step[s] == 0}
            done = stream.step()
            for r, s in mid.items():
                seen[r].append(stream.x[s].clone())                            # after its step 1 (it is still in its slot)
            for ticket, _, latent in done:
                seen[owner[ticket]].append(latent)                             # after its step 2
        assert stream.in_flight == 0 and all(len(v) == 2 for v in seen.values())
        for r in range(4):
            for n in (1, 2):
                err = float((seen[r][n - 1].cpu() - torch.from_numpy(gold[f"after_{n}"][r])).abs().max())
                print(f"[decode_stream] [{gemm}] request {r} (m = {int(gold['m'][r])}) after its step {n} vs the reference: max abs err {err:.3e}")
                errs.append(err)
        assert max(errs) < 2e-5


@pytest.mark.parametrize("gemm,context,scale,param", [("fp32", "live", 1.0, "velocity"), ("fp32", "full", 1.0, "velocity"), ("f16x2", "live", 1.0, "velocity"),
                                                      ("f16x2", "full", 1.0, "velocity"), ("fp32", "live", 2.0, "velocity"), ("f16x2", "live", 2.0, "x0")])
def test_stream_vs_decoding(pipe, ids5, noise, baseline, gemm, context, scale, param):
    """a request against decoding(ids[i:i+1], noise=n_i, max_steps=4): atol 2e-5 (not equality: the split-K Linears choose their partition from M);
    the pixels are _to_pixels of the returned latent"""
    with _mode(pipe, gemm, param):
        stream = pipe.decode_stream(2, uncond_scale=scale, max_steps=4, context=context, return_latent=True)
        got = _run(stream, {0: [4], 1: [1]}, ids5, noise, M5)
        for r in (4, 1):
            px, lat = got[r]
            _, want = pipe.decoding(ids5[r:r + 1], noise=noise[r:r + 1], max_steps=4, return_latent=True, uncond_scale=scale, ar_partial=M5[r])
            err = float((lat - want[0]).abs().max())
            print(f"[decode_stream] [{gemm} {context} scale {scale} {param}] request {r} vs decoding: max abs diff {err:.3e}")
            assert err <= 2e-5
            assert torch.equal(px, pipe._to_pixels(lat[None].clone())[0])
        assert stream.step_dev.cpu().tolist() == stream.sched.step == [-1, -1]


def test_f16x2_full_context_bits_do_not_depend_on_slot_or_neighbours(pipe, ids5, noise, baseline):
    """f16x2, context='full': five requests staggered into 3 slots equal, bit for bit, the same requests run lock-step (three, then two), whatever
    slot they land in; and a second staggered run equals the first"""
    with _mode(pipe, "f16x2"):
        stag = {0: [0], 1: [1, 2], 4: [3], 5: [4]}                             # request 3 takes the slot request 0 left, request 4 the one request 1 left
        a = _run(pipe.decode_stream(3, max_steps=4, context="full", return_latent=True), stag, ids5, noise, M5)
        b = _run(pipe.decode_stream(3, max_steps=4, context="full", return_latent=True), stag, ids5, noise, M5)
        lock = _run(pipe.decode_stream(3, max_steps=4, context="full", return_latent=True), {0: [2, 1, 0], 4: [4, 3]}, ids5, noise, M5)
        for r in range(5):
            assert torch.equal(a[r][1], b[r][1]) and torch.equal(a[r][0], b[r][0]), f"request {r}: run to run"
            assert torch.equal(a[r][1], lock[r][1]), f"request {r}: staggered vs lock-step, max abs diff {float((a[r][1] - lock[r][1]).abs().max()):.3e}"


def test_idle_slots_and_invisible_ids_change_nothing(pipe, ids5, noise, baseline):
    with _mode(pipe, "fp32"):
        def run(poison=False, ids=ids5):
            stream = pipe.decode_stream(3, max_steps=3, return_latent=True)
            t = stream.submit(ids[1], noise=noise[1], ar_partial=M5[1])
            stream.step()
            t2 = stream.submit(ids[2], noise=noise[2], ar_partial=M5[2])
            idle = [s for s in range(3) if stream.sched.ticket[s] is None]
            assert len(idle) == 1
            if poison:
                for buf in (stream.x, stream.ctx0, stream.cqkv0):
                    buf[idle] = float("nan")
            out = dict((tk, lat) for tk, _, lat in stream.drain())
            if poison:
                assert bool(torch.isnan(stream.x[idle]).all())                  # the idle slot was computed, discarded and left as it was
            assert stream.step_dev.cpu().tolist() == stream.sched.step == [-1] * 3
            return out[t], out[t2]
        clean = run()
        dirty = run(poison=True)
        assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])
        ids2 = ids5.copy()
        hidden = ~tokens.suffix_mask(K, np.array(M5))
        ids2[hidden] = (ids2[hidden] + 12345) % 32768
        other = run(ids=ids2)
        assert torch.equal(clean[0], other[0]) and torch.equal(clean[1], other[1])


def test_a_step_that_retires_nobody_does_not_synchronise(pipe, ids5, noise, baseline):
    with _mode(pipe, "fp32"):
        stream = pipe.decode_stream(2, max_steps=4)
        stream.submit(ids5[0], noise=noise[0])
        assert stream.step() == []                                             # warm: library handles, allocator
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            assert stream.step() == [] and stream.step() == []
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert [t for t, _ in stream.step()] == [0]


def test_one_full_request_in_two_slots(pipe, ids5, noise, baseline):
    """all 50 steps.  Against decoding's 50 steps at atol 1e-3: each step of the two routes agrees within the standing 2e-5, and 50 such steps add up to
    at most 50 x 2e-5 when the update does not expand differences (it contracts them: dt / t of the distance to the prediction)"""
    with _mode(pipe, "fp32"):
        stream = pipe.decode_stream(2, return_latent=True)
        t = stream.submit(ids5[4], noise=noise[4], ar_partial=M5[4])
        for i in range(49):
            assert stream.step() == [] and stream.sched.step[0] == i + 1
        assert stream.step_dev.cpu().tolist() == [49, -1]
        (ticket, px, lat), = stream.step()
        assert ticket == t and stream.in_flight == 0 and bool(torch.isfinite(lat).all())
        _, want = pipe.decoding(ids5[4:5], noise=noise[4:5], return_latent=True, ar_partial=M5[4])
        err = float((lat - want[0]).abs().max())
        print(f"[decode_stream] 50 steps in a 2-slot stream vs decoding: max abs diff {err:.3e}")
        assert err <= 1e-3


def test_forced_overflow_restarts_on_fp32_and_returns_to_the_mode(pipe, ids5, noise, baseline, capsys):
    dit = pipe.model.model
    with _mode(pipe, "fp32"):
        want = _run(pipe.decode_stream(2, max_steps=3, return_latent=True), {0: [0, 1]}, ids5, noise, M5)
    with _mode(pipe, "f16x2"):
        fresh = _run(pipe.decode_stream(2, max_steps=3, return_latent=True), {0: [2]}, ids5, noise, M5)
        stream = pipe.decode_stream(2, max_steps=3, return_latent=True)
        t0 = stream.submit(ids5[0], noise=noise[0], ar_partial=M5[0])
        stream.step()
        t1 = stream.submit(ids5[1], noise=noise[1], ar_partial=M5[1])
        stream.step()
        dit.overflow.fill_(1)                                                  # as an activation outside the fp16 range leaves it
        assert stream.step() == [] and stream.in_flight == 2 and stream.sched.step == [0, 0]      # nobody leaves with an invalid image
        assert int(dit.overflow.item()) == 0 and dit.gemm == "f16x2" and stream._fallback == {t0, t1}
        assert "restarting the 2 requests" in capsys.readouterr().out
        got = dict((tk, lat) for tk, _, lat in stream.drain())
        assert torch.equal(got[t0], want[0][1]) and torch.equal(got[t1], want[1][1])              # the fp32 stream's bits
        assert dit.gemm == "f16x2" and not stream._fallback and int(dit.overflow.item()) == 0
        t2 = stream.submit(ids5[2], noise=noise[2], ar_partial=M5[2])
        (tk, _, lat), = stream.drain()
        assert tk == t2 and torch.equal(lat, fresh[2][1])                      # back on the configured mode


def test_decoding_stream_refusals_and_stream_full(pipe, ids5, noise, baseline):
    with _mode(pipe, "fp32"):
        torch.manual_seed(5)
        reqs = [(ids5[i % 5], dict(ar_partial=M5[i % 5]) if i % 2 else None) for i in range(7)]
        got = list(pipe.decoding_stream(reqs, slots=3, max_steps=2))
        assert sorted(i for i, _ in got) == list(range(7))
        assert all(img.shape == (3, pipe.datasize, pipe.datasize) and img.dtype == pipe.dtype and bool(torch.isfinite(img.float()).all()) for _, img in got)
        assert [i for i, _ in got[:3]] == [0, 1, 2]                            # equal length: first in, first out
        stream = pipe.decode_stream(2, max_steps=2)
        assert isinstance(stream, DecodeStream) and (stream.free_slots, stream.in_flight) == (2, 0) and stream.step() == []
        torch.manual_seed(11)
        stream.submit(ids5[0])
        torch.manual_seed(11)
        assert torch.equal(stream.x[0:1].cpu(), torch.randn(1, 16, 32, 32))    # the default noise: one draw from the global CPU generator
        stream.submit(ids5[1][None], noise=noise[1])
        with pytest.raises(StreamFull):
            stream.submit(ids5[2], noise=noise[2])
        assert (stream.free_slots, stream.in_flight) == (0, 2)
        assert len(stream.drain()) == 2
        for kw in (dict(ar_partial=3, prefix_k=3), dict(ar_partial=K + 1), dict(super_mask=np.ones(K - 1, bool)), dict(prefix_k=K + 1)):
            with pytest.raises(ValueError):
                stream.submit(ids5[2], **kw)
        with pytest.raises(ValueError):
            stream.submit(ids5[2][:100])
        assert stream.free_slots == 2
        with pytest.raises(ValueError):
            pipe.decode_stream(0)
        with pytest.raises(ValueError):
            pipe.decode_stream(2, context="dead")
    assert pipe.set_gemm("exact") == "exact"
    try:
        with pytest.raises(NotImplementedError):
            pipe.decode_stream(2)
    finally:
        pipe.set_gemm("fp32")


def test_decoding_keeps_its_bits(pipe, gold, noise, baseline):
    """after streams have been created, run and dropped, `decoding` computes what it computed before any existed"""
    for gemm in ("fp32", "f16x2"):
        with _mode(pipe, gemm):
            px, lat = pipe.decoding(gold["ids"][:2], noise=noise[:2], max_steps=2, return_latent=True, ar_partial=[301, 37])
        assert torch.equal(lat, baseline[gemm][1]) and torch.equal(px, baseline[gemm][0]), gemm
