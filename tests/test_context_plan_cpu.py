"""not gpu: schedule.context_plan -- which context rows every sampler step hands to the model and by which route -- against the brute-force
visible set V = { j : j <= k_table[i] and j < prefix_k and pattern[b, j] } of EVERY step and sample, on the real step tables (K = 512 with the stage
strings of test_ar_partial_cpu.py, K = 1024 with those of its config); the refusals; the graph key; the grouping of differing rows."""
import numpy as np
import pytest

import kmask_cases as KM
from selftoktokenizer_amd import tokens
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.schedule import (ContextPlan, DiTiCont, FlowSchedule, context_plan, last_visible, pattern_groups, prefix_lengths,
                                           request_pattern, rows_uniform)

STEPS = 50
TABLES = {512: ("200,400,600,800,1000", "144,112,96,96,64"),
          1024: (default_config(1024).tokenizer.params.stages, default_config(1024).tokenizer.params.k_per_stage)}


def k_table(K):
    return DiTiCont(1000, K, *TABLES[K]).to_indices(FlowSchedule(STEPS, 1.0).t_long)


def patterns(K):
    """name -> [K] bool"""
    ar = np.arange(K)
    p = {"ones": np.ones(K, bool), "zeros": np.zeros(K, bool), "bit0": ar == 0, f"bit{K - 1}": ar == K - 1,
         "hash": KM.hash_pattern(K), "hash_rolled": np.roll(KM.hash_pattern(K), 7), "not_hash": ~KM.hash_pattern(K)}
    for m in (1, 37, 301, K):
        p[f"prefix{m}"] = ar < m
        p[f"suffix{m}"] = tokens.suffix_mask(K, [m])[0]
    return p


def row_sets(K):
    """name -> [B, K] bool with differing rows"""
    h = KM.hash_pattern(K)
    return {"suffix_m": tokens.suffix_mask(K, [0, 37, K, 1, 301, 37]),
            "suffix_0_and_K": tokens.suffix_mask(K, [0, K]),
            "hash_rows": np.stack([h, ~h, np.roll(h, 7), np.roll(h, 100) & (np.arange(K) > 300)]),
            "zeros_and_top": np.stack([np.zeros(K, bool), np.arange(K) == K - 1]),
            "mixed": np.stack([np.ones(K, bool), np.arange(K) < 37, h, np.zeros(K, bool), np.arange(K) == 0])}


PREFIX_KS = lambda K: (None, 0, 20, 376, K)


def brute(kt, K, prefix_k, rows):
    """bool [steps, B, K]: V as an indicator"""
    ar = np.arange(K)
    lim = (ar[None] <= np.asarray(kt)[:, None]) & (ar[None] < (K if prefix_k is None else prefix_k))
    return lim[:, None, :] & np.asarray(rows, bool).reshape(-1, K)[None]


def check_plan(plan, V, route, name):
    """the issue's per-route conditions, for every step and every sample of V [steps, B, K]"""
    steps, B, K = V.shape
    assert isinstance(plan, ContextPlan) and isinstance(plan, tuple) and plan.n_live.shape == (steps,)
    for a in (plan.n_live, plan.gather, plan.words_rows):
        assert a is None or not a.flags.writeable
    assert {"slice": (True, True), "gather": (False, True), "in place": (True, False), "batched": (True, False)}[route] == (plan.gather is None, plan.words_rows is None), name
    hash(plan.key)
    bits = None
    if plan.words_rows is not None:
        assert plan.words_rows.dtype == bool and plan.words_rows.shape == ((1, K) if route == "in place" else (B, K))
        w = KM.pack_words(plan.words_rows)                                  # the words the kernel reads: key j = bit j & 31 of word j >> 5
        bits = ((w[:, np.arange(K) >> 5] >> (np.arange(K) & 31).astype(np.uint32)) & 1).astype(bool)
    for i in range(steps):
        n = int(plan.n_live[i])
        assert 0 <= n <= K
        for b in range(B):
            v = V[i, b]
            where = f"{name}, step {i}, sample {b}"
            if route == "slice":
                assert np.array_equal(v, np.arange(K) < n), where
            elif route == "gather":
                assert np.array_equal(plan.gather[:n], np.nonzero(v)[0]), where
            elif route == "in place":
                assert n == (int(np.nonzero(v)[0][-1]) + 1 if v.any() else 0), where
                assert np.array_equal(bits[0, :n], v[:n]), where
            else:
                assert (n == 0) == (not V[i].any()), where
                if n:
                    assert np.array_equal(v, bits[b] & (np.arange(K) < n)), where


@pytest.mark.parametrize("K", [512, 1024])
def test_every_step_of_every_route_is_the_brute_force_set(K):
    kt = k_table(K)
    assert len(kt) == STEPS and int(kt[0]) == K - 1
    plans, checked = [], 0
    for pk in PREFIX_KS(K):
        plan = context_plan(kt, K, STEPS, prefix_k=pk)
        check_plan(plan, brute(kt, K, pk, np.ones(K, bool)), "slice", f"no pattern, prefix_k={pk}")
        assert np.array_equal(plan.n_live, np.minimum(kt + 1, K if pk is None else pk))
        plans.append(plan)
        for name, pat in patterns(K).items():
            V = brute(kt, K, pk, pat)
            is_prefix = np.array_equal(pat, np.arange(K) < pat.sum())
            for keep in (False, True):
                # a prefix-shaped pattern still gathers when positions are kept: the route test_pipeline_gpu compares with prefix_k
                route = "in place" if keep and not is_prefix else "gather"
                for given in (pat, pat.astype(np.int64), np.repeat(pat[None], 3, 0)):     # bool, 0-1, batch-uniform [B, K]
                    plan = context_plan(kt, K, STEPS, prefix_k=pk, pattern=given, batched=given.ndim == 2, keep_positions=keep)
                    check_plan(plan, V, route, f"{name}, prefix_k={pk}, keep_positions={keep}")
                    plans.append(plan)
                    checked += 1
    for name, rows in row_sets(K).items():
        plan = context_plan(kt, K, STEPS, pattern=rows, batched=True)
        check_plan(plan, brute(kt, K, None, rows), "batched", name)
        plans.append(plan)
        # without mask_batched: one group per distinct row, each a plan of its own
        groups = pattern_groups(rows, rows.shape[0])
        assert sorted(b for idx, _ in groups for b in idx) == list(range(rows.shape[0]))
        assert len(groups) == len({r.tobytes() for r in rows})
        for idx, row in groups:
            assert all(np.array_equal(rows[b], row) for b in idx)
            for keep in (False, True):
                for pk in PREFIX_KS(K):
                    route = "in place" if keep and not np.array_equal(row, np.arange(K) < row.sum()) else "gather"
                    plan = context_plan(kt, K, STEPS, prefix_k=pk, pattern=row, keep_positions=keep)
                    check_plan(plan, brute(kt, K, pk, row), route, f"{name} group {idx}, prefix_k={pk}, keep_positions={keep}")
                    plans.append(plan)
    assert checked == len(PREFIX_KS(K)) * len(patterns(K)) * 2 * 3 and len(patterns(K)) == 15
    # fewer steps: the head of the table
    short = context_plan(kt, K, 3, pattern=KM.hash_pattern(K), keep_positions=True)
    check_plan(short, brute(kt[:3], K, None, KM.hash_pattern(K)), "in place", "3 steps")
    plans.append(short)
    # the key: equal for equal launches, different as soon as n_live, gather or words_rows differ
    sig = lambda p: (p.n_live.tolist(), None if p.gather is None else p.gather.tolist(), None if p.words_rows is None else p.words_rows.tolist())
    by_key, by_sig = {}, {}
    for p in plans:
        s = repr(sig(p))
        assert by_key.setdefault(p.key, s) == s, "two plans with different launches share a key"
        assert by_sig.setdefault(s, p.key) == p.key, "two plans with the same launches have different keys"
    again = context_plan(kt, K, STEPS, prefix_k=376, pattern=KM.hash_pattern(K), keep_positions=True)
    assert again.key == context_plan(list(kt), K, STEPS, prefix_k=376, pattern=KM.hash_pattern(K).astype(np.float32), keep_positions=True).key
    assert again.key != context_plan(kt, K, STEPS, prefix_k=376, pattern=KM.hash_pattern(K)).key
    assert context_plan(kt, K, STEPS, pattern=np.arange(K) < 100).key != context_plan(kt, K, STEPS, prefix_k=100).key     # two routes: gather / slice


def test_pattern_groups_leaves_one_batch_alone():
    K = 512
    h = KM.hash_pattern(K)
    rows = np.stack([h, ~h, h])
    assert pattern_groups(None, 3) == [(None, None)]
    for given, B, batched in ((h, 3, False), (np.repeat(h[None], 3, 0), 3, False), (rows, 3, True), (rows, 2, False)):
        (idx, pat), = pattern_groups(given, B, batched)
        assert idx is None and pat is not None and np.array_equal(pat, given)
    groups = pattern_groups(rows.astype(np.int64), 3)
    assert [idx for idx, _ in groups] == [[0, 2], [1]] and np.array_equal(groups[0][1], h) and np.array_equal(groups[1][1], ~h)


def test_refusals():
    K = 512
    kt = k_table(K)
    h = KM.hash_pattern(K)
    rows = np.stack([h, ~h])
    for bad in (np.ones(100, bool), np.ones(K + 1, bool), np.ones((2, K - 1), bool)):
        with pytest.raises(ValueError, match=r"super_mask has \d+ entries, the tokenizer has K = 512 tokens"):
            context_plan(kt, K, STEPS, pattern=bad)
    with pytest.raises(ValueError, match=r"super_mask has 511 entries per sample"):
        context_plan(kt, K, STEPS, pattern=rows[:, :K - 1], batched=True)
    for keep in (False, True):
        with pytest.raises(NotImplementedError, match="ONE visibility pattern per call"):
            context_plan(kt, K, STEPS, pattern=rows, keep_positions=keep)
    with pytest.raises(NotImplementedError, match=r"gemm='exact' decodes one visibility pattern per sampler call: pass super_mask=tokens.suffix_mask\(K, m\)"):
        context_plan(kt, K, STEPS, pattern=rows, batched=True, keep_positions=True)
    with pytest.raises(ValueError, match="mask_batched is exclusive with prefix_k"):
        context_plan(kt, K, STEPS, prefix_k=100, pattern=rows, batched=True)
    # the arguments of decoding()
    for pk in (-1, K + 1):
        with pytest.raises(ValueError, match=r"prefix_k must be in \[0, 512\]"):
            request_pattern(K, 4, prefix_k=pk)
    for kw in (dict(prefix_k=3), dict(super_mask=np.ones(K, bool))):
        with pytest.raises(ValueError, match="ar_partial is exclusive with prefix_k / super_mask"):
            request_pattern(K, 4, ar_partial=3, **kw)
    with pytest.raises(ValueError, match="ar_partial: expected an int or 4 values, got 3"):
        request_pattern(K, 4, ar_partial=[1, 2, 3])
    for m in (K + 1, [-1, 0, 0, 0]):
        with pytest.raises(ValueError, match=r"ar_partial must be in \[0, 512\]"):
            request_pattern(K, 4, ar_partial=m)
    assert request_pattern(K, 4, prefix_k=K, super_mask=h, mask_batched=True) == (h, True) and request_pattern(K, 4) == (None, False)
    for m in (37, [37] * 4):                                                 # equal m: ONE [K] row, the uniform route
        pat, batched = request_pattern(K, 4, ar_partial=m)
        assert batched is False and np.array_equal(pat, tokens.suffix_mask(K, [37])[0])
    pat, batched = request_pattern(K, 4, ar_partial=[0, 37, K, 37])            # differing m: one batch
    assert batched is True and np.array_equal(pat, tokens.suffix_mask(K, [0, 37, K, 37]))


def test_sampler_refuses_a_plan_together_with_the_arguments_it_replaces():
    import torch
    from selftoktokenizer_amd.pipeline import _Flow
    K = 512
    kt = k_table(K)
    flow = _Flow(STEPS, 1.0, torch.device("cpu"))
    noise, ehs = torch.zeros(2, 16, 32, 32), torch.zeros(2, K, 16)
    plan = (context_plan(kt, K, STEPS), None, None)
    for kw in (dict(prefix_k=3), dict(super_mask=np.ones(K, bool))):
        with pytest.raises(ValueError, match="plan is exclusive with prefix_k / super_mask"):
            flow.p_sample_loop(None, noise, ehs, kt, plan=plan, **kw)
    with pytest.raises(ValueError, match="plan: expected 50 steps"):
        flow.p_sample_loop(None, noise, ehs, kt, plan=(context_plan(kt, K, 3), None, None))
    with pytest.raises(ValueError, match="words_rows"):
        flow.p_sample_loop(None, noise, ehs, kt, plan=(context_plan(kt, K, STEPS, pattern=np.ones((3, K), bool) & (np.arange(3)[:, None] < 2), batched=True), None, None))


def test_mask_predicates():
    K = 64
    ar = np.arange(K)
    pre = ar[None] < np.asarray([[5], [0], [K]])
    assert prefix_lengths(pre).tolist() == [5, 0, K] and not rows_uniform(pre) and last_visible(pre) == K
    assert prefix_lengths(np.stack([ar < 5, ar == 7])) is None and prefix_lengths((ar >= 3)[None]) is None
    assert rows_uniform(np.repeat((ar < 9)[None], 4, 0)) and last_visible(np.repeat((ar < 9)[None], 4, 0)) == 9
    assert last_visible(np.zeros((2, K), bool)) == 0 and last_visible(np.stack([ar == 3, ar == 40])) == 41
    assert prefix_lengths(np.zeros((2, K), bool)).tolist() == [0, 0]
