"""-m gpu: decoding partial AR sequences with a different progress per sample (SelftokPipeline.decoding(ar_partial=),
mask_batched=, MMDiTGPU.__call__(mask=)), against the reference's own sampler on the real MMDiT (tests/golden/ar_partial_b4.npz:
B = 4, m = (512, 301, 37, 1), two steps) and against the existing one-pattern-per-call routes."""
import os

import numpy as np
import pytest
import torch

from selftoktokenizer_amd import ops, synth, tokens, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
K = 512


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


def _latent(pipe, ids, noise, **kw):
    return pipe.decoding(ids, noise=noise, max_steps=2, return_latent=True, **kw)[1]


@pytest.mark.parametrize("gemm", ["fp32", "f16x2"])
def test_ar_partial_vs_reference(pipe, gold, gemm):
    """latent after steps 1 and 2 of decoding(ar_partial=m) against the reference's RectifiedFlow.sample_one_step with
    mask = get_encoder_mask(x, k) * suffix_mask: max abs error < 2e-5 (the gate of the uniform non-prefix pattern,
    test_pipeline_gpu.py::test_sampler_options_vs_reference).  At step 1 (k = 510) the m = 1 sample has NO visible token."""
    assert gold["k"].tolist() == [K - 1, K - 2] and gold["visible"][1].tolist() == [511, 300, 36, 0]
    noise = synth.synthetic_noise(4, first_index=40)
    assert pipe.set_gemm(gemm) == gemm
    real = pipe.flow.p_sample_loop
    try:
        trace = []
        pipe.flow.p_sample_loop = lambda *a, **k: real(*a, trace=trace, **k)
        pipe.decoding(gold["ids"], noise=noise, max_steps=2, ar_partial=gold["m"])
        assert len(trace) == 2, "differing m must run ONE batched pass"
        errs = []
        for n in (1, 2):
            d = (trace[n - 1].cpu() - torch.from_numpy(gold[f"after_{n}"])).abs()
            errs.append(float(d.max()))
            print(f"[ar_partial] [{gemm}] latent after {n} steps vs the reference: max abs err {errs[-1]:.3e} (per sample {[f'{float(v):.2e}' for v in d.amax(dim=(1, 2, 3))]})")
        assert max(errs) < 2e-5
    finally:
        pipe.flow.p_sample_loop = real
        pipe.set_gemm("fp32")


@pytest.mark.parametrize("gemm", ["fp32", "f16x2"])
def test_batched_equals_grouped_and_invisible_ids_are_never_read(pipe, gold, gemm):
    noise = synth.synthetic_noise(4, first_index=40)
    ids, m = gold["ids"], gold["m"]
    suf = tokens.suffix_mask(K, m)
    assert pipe.set_gemm(gemm) == gemm
    try:
        lb = _latent(pipe, ids, noise, ar_partial=m)
        lg = _latent(pipe, ids, noise, super_mask=suf)                       # mask_batched=False: today's grouping, one call per pattern
        print(f"[ar_partial] [{gemm}] batched vs grouped: max abs diff {float((lb - lg).abs().max()):.3e}")
        torch.testing.assert_close(lb, lg, rtol=0, atol=2e-5)
        assert torch.equal(_latent(pipe, ids, noise, super_mask=suf, mask_batched=True), lb)
        # ids at invisible positions are never read
        ids2 = ids.copy()
        ids2[~suf] = (ids2[~suf] + 12345) % 32768
        assert torch.equal(_latent(pipe, ids2, noise, ar_partial=m), lb)
        # the AR round trip: what the model emitted, padded -> the same bits as the full ids under the suffix mask ...
        ar = tokens.to_ar_order(ids)
        idx, m2 = tokens.pad_ar_partial([ar[b, :m[b]] for b in range(4)], K)
        assert np.array_equal(m2, m)
        assert torch.equal(_latent(pipe, idx, noise, ar_partial=m2), lb)
        # ... and NOT the recipe documented before (from_ar_order -> pad_prefix -> prefix_k), which put the tokens at positions 0 .. m - 1
        old_ids, k = tokens.pad_prefix(tokens.from_ar_order(ar[1:2, :m[1]]), K)
        l_old = _latent(pipe, old_ids, noise[1:2], prefix_k=k)
        assert float((l_old - lb[1:2]).abs().max()) > 1e-3, "the pad_prefix recipe decodes something else"
        # graph capture, then replay with another id set: the eager bits
        lc = _latent(pipe, ids, noise, ar_partial=m, use_graph=True)
        assert torch.equal(lc, lb)
        assert torch.equal(_latent(pipe, ids2, noise, ar_partial=m, use_graph=True), lb)
        # equal m: the existing uniform route, bit for bit
        assert torch.equal(_latent(pipe, ids, noise, ar_partial=37), _latent(pipe, ids, noise, super_mask=tokens.suffix_mask(K, [37])[0]))
        assert torch.equal(_latent(pipe, ids, noise, ar_partial=[37] * 4), _latent(pipe, ids, noise, ar_partial=37))
    finally:
        pipe.set_gemm("fp32")


def test_refusals(pipe, gold):
    noise = synth.synthetic_noise(4, first_index=40)
    for kw in (dict(ar_partial=3, prefix_k=3), dict(ar_partial=3, super_mask=np.ones(K, bool)), dict(ar_partial=[1, 2, 3]), dict(ar_partial=K + 1),
               dict(ar_partial=[-1, 0, 0, 0])):
        with pytest.raises(ValueError):
            pipe.decoding(gold["ids"], noise=noise, max_steps=1, **kw)
    assert pipe.set_gemm("exact") == "exact"
    try:
        with pytest.raises(NotImplementedError):
            pipe.decoding(gold["ids"], noise=noise, max_steps=1, ar_partial=gold["m"])
    finally:
        pipe.set_gemm("fp32")


@pytest.mark.parametrize("gemm", ["fp32", "f16x2"])
def test_mmdit_call_with_per_sample_masks(pipe, gold, gemm, monkeypatch):
    """MMDiTGPU.__call__(mask=): a non-prefix [B, K] mask runs through the key bit mask and agrees with the gather route per sample;
    a prefix mask still makes the kvis call it made before (no kmask)"""
    import kmask_cases as KM
    dit = pipe.model.model
    assert pipe.set_gemm(gemm) == gemm
    try:
        B = 3
        ehs = pipe._codes(gold["ids"][:B])
        x = synth.synthetic_noise(B, first_index=40).cuda()
        t = torch.full((B,), 0.7)
        h = KM.hash_pattern(K)
        masks = np.stack([h, ~h, np.roll(h, 7)])
        v, _ = dit(x, t, encoder_hidden_states=ehs, mask=torch.from_numpy(masks), context_see_xt=True)
        tf = ops.timestep_embed(t[:1].cuda().float(), dit.freqs, 1000.0)
        for b in range(B):
            ctx = dit.embed_context(ehs[b:b + 1])
            cg, tabs, _ = dit.gather_context(ctx, visible=torch.from_numpy(masks[b]))
            out = dit.core(dit.embed_image(x[b:b + 1]), dit.time_embed(tf), cg, True, tables=tabs)
            _, vg = ops.unpatchify_cfg_euler(out, C=16, hp=x.shape[-2] // 2, wp=x.shape[-1] // 2)
            err = float((v[b:b + 1] - vg).abs().max())
            print(f"[ar_partial] [{gemm}] __call__(mask=pattern {b}) vs the gather route: max abs diff {err:.3e}")
            assert err < 2e-5
        calls = []
        real = ops.attention
        monkeypatch.setattr(ops, "attention", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
        pre = torch.arange(K)[None] < torch.tensor([100, 512, 1])[:, None]
        dit(x, t, encoder_hidden_states=ehs, mask=pre, context_see_xt=True)
        assert len(calls) == 24 and all(c.get("kmask") is None and c["kvis"].tolist() == [99, 511, 0] for c in calls)
    finally:
        pipe.set_gemm("fp32")
