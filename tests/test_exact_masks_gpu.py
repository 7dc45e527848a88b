"""-m gpu: gemm='exact' with visibility patterns that are no prefix (the reference's `mask * super_mask`, rectified_flow.py:226-231): the context
rows keep their positions and the exact-order attention takes the pattern as key bit words.  Against the REFERENCE's own runs at B = 16
(tests/golden/exact_masks_b16.npz, exact_masks_k1024_b16.npz; tools/oracle/gen_golden.py stage exact_masks): crc32 of the whole tensor and a sub-sample.
The generator's host check passed (tests/golden/PINNING_exact_masks.json: it reproduced the committed cfg_b16.npz bit for bit), so every comparison
with a golden here is BIT-EXACT.  Then the routes against each other: graph replay, ar_partial, per-sample rows through the grouping, a full pattern,
and the unfused route of the 128 / 320 px grids against fp32."""
import os
import zlib

import numpy as np
import pytest
import torch

import ex_kmask_cases as XK
from selftoktokenizer_amd import ops, synth, tokens, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
K = 512


def _crc(t):
    return zlib.crc32(t.contiguous().cpu().numpy().tobytes())


def _bits_equal(a, b, what):
    x, y = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    n = int((x.view(np.uint32) != y.view(np.uint32)).sum())
    assert n == 0, f"{what}: {n} of {x.size} fp32 elements differ (max abs diff {np.abs(x - y).max():.3e})"


@pytest.fixture(scope="module")
def models():
    from selftoktokenizer_amd.encoder import QformerEncoderGPU
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    from selftoktokenizer_amd.pipeline import _Flow
    from selftoktokenizer_amd.schedule import DiTiCont
    sd = W.synthetic_state_dict(W.expected_shapes(K), device="cuda")
    dev = torch.device("cuda", torch.cuda.current_device())
    enc = QformerEncoderGPU(sd, dev, K, mode="exact")
    dit = MMDiTGPU(sd, dev, K, gemm="exact")
    flow = _Flow(50, 1.0, dev)
    cfgp = default_config(K).tokenizer.params
    ktab = DiTiCont(1000, K, cfgp.stages, cfgp.k_per_stage).to_indices(flow.t_long)
    return sd, enc, dit, flow, ktab


@pytest.fixture(scope="module")
def pipe(models):
    from selftoktokenizer_amd.pipeline import SelftokPipeline
    return SelftokPipeline(default_config(K), None, None, device="cuda", state_dict=models[0], vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False,
                           gemm="exact")


@pytest.mark.parametrize("tag", ["hash", "suffix301"])
def test_sampler_steps_with_a_pattern_equal_the_reference(models, tag):
    """two sample_one_step steps of the reference at B = 16, context_see_xt=True, mask = (arange(K) <= k) * pattern"""
    sd, enc, dit, flow, ktab = models
    g = np.load(os.path.join(GOLD, "exact_masks_b16.npz"))
    pat = XK.hash_pattern(K) if tag == "hash" else XK.suffix(K, 301)
    B = 16
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(B, first_index=11)).cuda())
    noise = synth.synthetic_noise(B, first_index=11)
    for steps in (1, 2):
        lat = flow.p_sample_loop(dit, noise, ehs, ktab, context_see_xt=True, max_steps=steps, super_mask=pat)
        sub = lat[:, :, ::4, ::4].contiguous().cpu().numpy()
        print(f"\n[{tag}] after {steps} step(s): sub-sample max abs diff vs the reference {np.abs(sub - g[f'{tag}_sub_{steps}']).max():.3e}")
        assert np.array_equal(sub.view(np.uint32), g[f"{tag}_sub_{steps}"].view(np.uint32))
        assert _crc(lat) == int(g[f"{tag}_crc_{steps}"]), f"latents after {steps} step(s) with the {tag} pattern differ from the reference's"


def test_call_with_a_mask_per_sample_equals_the_reference(models):
    """MMDiT.forward at schedule index 30 (k = 375) with a different [K] pattern per sample (full, suffix, hash, single key, first key above 256, ...)"""
    sd, enc, dit, flow, ktab = models
    g = np.load(os.path.join(GOLD, "exact_masks_b16.npz"))
    B, i = 16, int(g["fwd_index"])
    assert int(ktab[i]) == int(g["fwd_k"])
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(B, first_index=11)).cuda())
    x = synth.synthetic_noise(B, first_index=11)
    mask = (np.arange(K)[None] <= int(ktab[i])) & XK.model_rows(K)
    v, _ = dit(x, torch.tensor([flow.scheduled_t[i]] * B), encoder_hidden_states=ehs, mask=torch.from_numpy(mask), context_see_xt=True)
    sub = v[:, :, ::4, ::4].contiguous().cpu().numpy()
    print(f"\nper-sample masks: sub-sample max abs diff vs the reference {np.abs(sub - g['fwd_sub']).max():.3e}")
    assert np.array_equal(sub.view(np.uint32), g["fwd_sub"].view(np.uint32))
    assert _crc(v) == int(g["fwd_crc"])
    # per-sample PREFIXES take the same route: each sample equals its own uniform-prefix call (the route pinned to the reference before)
    cnt = [376, 100, 1, 333]
    pm = np.arange(K)[None] < np.asarray(cnt)[:, None]
    t4 = torch.tensor([flow.scheduled_t[i]] * 4)
    v4, _ = dit(x[:4], t4, encoder_hidden_states=ehs[:4], mask=torch.from_numpy(pm), context_see_xt=True)
    for b in range(4):
        v1, _ = dit(x[b:b + 1], t4[:1], encoder_hidden_states=ehs[b:b + 1], mask=torch.from_numpy(pm[b:b + 1]), context_see_xt=True)
        _bits_equal(v4[b:b + 1], v1, f"per-sample prefix {cnt[b]} vs the uniform prefix route")


def test_k1024_first_kv_block_masked_equals_the_reference():
    """K = 1024 with the suffix m = 300: the whole first kv block of 512 keys is masked (ATen's "every key so far masked" branch)"""
    from selftoktokenizer_amd.encoder import QformerEncoderGPU
    from selftoktokenizer_amd.mmdit import MMDiTGPU
    from selftoktokenizer_amd.pipeline import _Flow
    g = np.load(os.path.join(GOLD, "exact_masks_k1024_b16.npz"))
    sd = W.synthetic_state_dict(W.expected_shapes(1024), device="cuda")
    dev = torch.device("cuda", torch.cuda.current_device())
    enc = QformerEncoderGPU(sd, dev, 1024, mode="exact")
    B = 16
    outs_q, ids = enc(synth.synthetic_latents(B, first_index=5).to(torch.bfloat16).float().cuda())
    assert np.array_equal(ids.cpu().numpy(), g["ids"].astype(np.int64))
    dit = MMDiTGPU(sd, dev, 1024, gemm="exact")
    flow = _Flow(50, 1.0, dev)
    i, k = int(g["step"]), int(g["k"])
    mask = (np.arange(1024) <= k) & XK.suffix(1024, 300)
    assert int(mask.sum()) == int(g["visible"]) and not mask[:512].any()
    x = synth.synthetic_noise(B, first_index=5)
    v, _ = dit(x, torch.tensor([flow.scheduled_t[i]] * B), encoder_hidden_states=outs_q, mask=torch.from_numpy(np.repeat(mask[None], B, 0)), context_see_xt=True)
    print(f"\nK = 1024, suffix 300 at k = {k}: sub-sample max abs diff vs the reference {np.abs(v[:, :, ::4, ::4].cpu().numpy() - g['vsub']).max():.3e}")
    assert _crc(v) == int(g["vcrc"])


def test_graph_replay_ar_partial_and_grouped_rows(pipe):
    B = 3
    ids = synth.synthetic_token_ids(B, first_index=40)
    noise = synth.synthetic_noise(B, first_index=40)
    sm = tokens.suffix_mask(K, [37])[0]
    _, eager = pipe.decoding(ids, noise=noise, max_steps=3, super_mask=sm, return_latent=True)
    assert bool(torch.isfinite(eager).all())
    _, graph = pipe.decoding(ids, noise=noise, max_steps=3, super_mask=sm, return_latent=True, use_graph=True)
    _bits_equal(graph, eager, "use_graph=True replay vs eager")
    _, again = pipe.decoding(ids, noise=noise, max_steps=3, super_mask=sm, return_latent=True, use_graph=True)
    _bits_equal(again, eager, "second replay vs eager")
    _, ar = pipe.decoding(ids, noise=noise, max_steps=3, ar_partial=37, return_latent=True)
    _bits_equal(ar, eager, "ar_partial=37 vs super_mask=suffix_mask(K, [37])")
    # [B, K] with three different rows: the grouping decodes each pattern on its own -- and equals each sample alone
    rows = np.stack([XK.suffix(K, 301), XK.hash_pattern(K), XK.single(K, 100)])
    _, l3 = pipe.decoding(ids, noise=noise, max_steps=2, super_mask=rows, return_latent=True)
    for b in range(B):
        _, l1 = pipe.decoding(ids[b:b + 1], noise=noise[b:b + 1], max_steps=2, super_mask=rows[b], return_latent=True)
        _bits_equal(l3[b:b + 1], l1, f"sample {b} of a [B, K] super_mask vs the sample alone")
    # the one-batch per-sample route stays refused in this mode
    with pytest.raises(NotImplementedError, match="suffix_mask"):
        pipe.decoding(ids, noise=noise, max_steps=1, super_mask=rows, mask_batched=True)


def test_full_pattern_is_no_pattern_and_prefix_words_are_the_prefix_route(models, monkeypatch):
    sd, enc, dit, flow, ktab = models
    B = 2
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(B, first_index=11)).cuda())
    noise = synth.synthetic_noise(B, first_index=11)
    plain = flow.p_sample_loop(dit, noise, ehs, ktab, context_see_xt=True, max_steps=3)
    _bits_equal(flow.p_sample_loop(dit, noise, ehs, ktab, context_see_xt=True, max_steps=3, super_mask=np.ones(K, bool)), plain, "full-ones pattern vs no pattern, 3 steps")
    # per-sample prefixes run through the words and give each sample the bits of its own uniform-prefix call
    seen = []
    real = ops.ex_attention
    monkeypatch.setattr(ops, "ex_attention", lambda *a, **k: (seen.append(k.get("kmask") is not None), real(*a, **k))[1])
    x = synth.synthetic_noise(B, first_index=11)
    t = torch.tensor([flow.scheduled_t[30]] * B)
    k = int(ktab[30])
    pre = np.arange(K)[None] <= np.asarray([k, k - 1])[:, None]                                      # differing prefixes: the word route
    v, _ = dit(x, t, encoder_hidden_states=ehs, mask=torch.from_numpy(pre), context_see_xt=True)
    assert seen and all(seen), "per-sample prefixes in exact mode run through the key bit words"
    seen.clear()
    for b in range(B):
        v0, _ = dit(x[b:b + 1], t[:1], encoder_hidden_states=ehs[b:b + 1], mask=torch.from_numpy(pre[b:b + 1]), context_see_xt=True)
        _bits_equal(v[b:b + 1], v0, "words of a prefix vs the prefix route")
    assert seen and not any(seen), "a uniform prefix keeps the route without words"


def test_guided_steps_with_a_pattern_and_no_visible_key(models):
    """CFG: the conditional pass runs with context_see_xt=False (context rows see context keys only, Tk2 = 0 in their attention).  A pattern whose lowest
    position is above a step's k leaves that step without a visible key: the n_live = 0 route for the whole batch, whatever k is"""
    sd, enc, dit, flow, ktab = models
    B = 2
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(B, first_index=11)).cuda())
    noise = synth.synthetic_noise(B, first_index=11)
    pat = XK.hash_pattern(K)
    a = flow.p_sample_loop(dit, noise, ehs, ktab, context_see_xt=True, uncond_scale=2.0, max_steps=2, super_mask=pat)
    assert bool(torch.isfinite(a).all())
    try:
        fp = flow.p_sample_loop(_other(dit, "fp32"), noise, ehs, ktab, context_see_xt=True, uncond_scale=2.0, max_steps=2, super_mask=pat)
    finally:
        dit.set_gemm("exact")
    err = float((a - fp).abs().max())
    print(f"\nguided steps with the hash pattern: exact vs fp32 max abs diff {err:.3e}")
    assert err < 2e-5
    # position K - 1 only: visible at step 0 (k = K - 1), and steps 1 and 2 see nothing -- so their k does not matter
    top = XK.single(K, K - 1)
    b = flow.p_sample_loop(dit, noise, ehs, np.asarray([K - 1, 300, 200]), context_see_xt=True, uncond_scale=2.0, max_steps=3, super_mask=top)
    c = flow.p_sample_loop(dit, noise, ehs, np.asarray([K - 1, 510, 0]), context_see_xt=True, uncond_scale=2.0, max_steps=3, super_mask=top)
    assert bool(torch.isfinite(b).all())
    _bits_equal(b, c, "steps without a visible key do not depend on k")
    none = flow.p_sample_loop(dit, noise, ehs, np.asarray([K - 1, 300, 200]), context_see_xt=True, uncond_scale=2.0, max_steps=3, prefix_k=0)
    assert not torch.equal(b, none), "step 0 sees position K - 1"


def _other(dit, mode):
    dit.set_gemm(mode)
    return dit


@pytest.mark.parametrize("R", [128, 320])
def test_other_resolutions_run_the_unfused_route_and_agree_with_fp32(models, R, monkeypatch):
    sd, enc, dit, flow, ktab = models
    B = 2
    ehs = enc.codes_ln(torch.from_numpy(synth.synthetic_token_ids(B, first_index=11)).cuda())
    noise = synth.hash_normalish(synth.name_seed(f"exact_masks/noise/{R}"), (B, 16, R // 8, R // 8)).float()
    pat = XK.hash_pattern(K)
    lib = ops._lib.load()
    nx = (R // 16) ** 2
    assert bool(lib.selftok_ex_attention_fused_supported(K, nx, 64)) == (R == 128)
    kernel = "unfused"
    real = ops.ex_attention
    monkeypatch.setattr(ops, "ex_attention", lambda *a, **k: real(*a, **{**k, "kernel": kernel}))
    ex = flow.p_sample_loop(dit, noise, ehs, ktab, context_see_xt=True, max_steps=2, super_mask=pat)
    try:
        fp = flow.p_sample_loop(_other(dit, "fp32"), noise, ehs, ktab, context_see_xt=True, max_steps=2, super_mask=pat)
    finally:
        dit.set_gemm("exact")
    err = float((ex - fp).abs().max())
    print(f"\n{R} px, hash pattern, unfused exact attention vs fp32: max abs diff {err:.3e}")
    assert bool(torch.isfinite(ex).all()) and err < 2e-5
