"""not gpu: the host side of partial AR decoding -- tokens.pad_ar_partial / suffix_mask against the sampler's own step masks, the
extension header and its ctypes table, the bit layout of the key-mask words, and the case table of tests/test_attention_kmask_gpu.py
(tests/kmask_cases.py): it holds the patterns it claims and every case would see ONE wrong mask bit."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import edge_cases as E
import kmask_cases as KM
from selftoktokenizer_amd import _lib, ops, tokens
from selftoktokenizer_amd.schedule import DiTiCont, FlowSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 512


# ---- tokens ----
def test_pad_ar_partial_positions_dtype_and_edges():
    ar = np.array([[10, 11, 12], [20, 21, 22]], dtype=np.int32)             # coarse first
    idx, m = tokens.pad_ar_partial(ar, K, fill=7)
    assert idx.dtype == np.int64 and m.dtype == np.int64 and idx.shape == (2, K) and m.tolist() == [3, 3]
    for i in range(3):                                                      # token i -> position K - 1 - i
        assert idx[0, K - 1 - i] == 10 + i and idx[1, K - 1 - i] == 20 + i
    assert (idx[:, :K - 3] == 7).all()
    ragged = [np.arange(5), np.arange(0), np.arange(K)]                     # m = 5, 0, K
    idx, m = tokens.pad_ar_partial(ragged, K)
    assert m.tolist() == [5, 0, K] and idx.dtype == np.int64
    assert (idx[1] == 0).all() and np.array_equal(idx[2], np.arange(K)[::-1]) and np.array_equal(idx[0, K - 5:], np.arange(5)[::-1])
    with pytest.raises(ValueError):
        tokens.pad_ar_partial([np.arange(K + 1)], K)
    with pytest.raises(ValueError):
        tokens.suffix_mask(K, [K + 1])
    sm = tokens.suffix_mask(K, [0, 1, K])
    assert sm.dtype == bool and sm.shape == (3, K) and sm.sum(axis=1).tolist() == [0, 1, K] and sm[1, K - 1]


def test_ar_round_trip_and_suffix_mask_marks_the_surviving_ids():
    rng = np.random.RandomState(3)
    ids = rng.randint(1, 32768, size=(3, K)).astype(np.int64)               # no id equals the fill value 0
    ar = tokens.to_ar_order(ids)
    assert np.array_equal(tokens.pad_ar_partial(ar, K)[0], ids)             # a complete sequence comes back
    for mm in (1, 37, 301):
        idx, m = tokens.pad_ar_partial(ar[:, :mm], K)
        sm = tokens.suffix_mask(K, m)
        assert np.array_equal(sm, idx == ids) and np.array_equal(sm, idx != 0)
        # the recipe this replaces put the same tokens at positions 0 .. m - 1
        old, k = tokens.pad_prefix(tokens.from_ar_order(ar[:, :mm]), K)
        assert k == mm and not np.array_equal(old, idx)


def test_suffix_is_what_the_sampler_reveals_first():
    """the step masks are arange(K) <= k_table[i] with k falling from K - 1: position K - 1 is visible at step 0 only while k = K - 1,
    position 0 at every step -- so the tokens an AR model emits first (coarse) are the top of the index range"""
    flow = FlowSchedule(50, 1.0)
    k_table = DiTiCont(1000, K, "200,400,600,800,1000", "144,112,96,96,64").to_indices(flow.t_long)
    assert int(k_table[0]) == K - 1
    assert all(int(k_table[i]) >= int(k_table[i + 1]) for i in range(len(k_table) - 1))
    steps = np.arange(K)[None, :] <= np.asarray(k_table)[:, None]            # [steps, K]
    assert steps[:, 0].all() and steps[0, K - 1]
    n_steps_visible = steps.sum(axis=0)                                      # falls with the position: high positions leave first
    assert (np.diff(n_steps_visible) <= 0).all() and n_steps_visible[K - 1] < n_steps_visible[0]
    for m in (1, 37, 301, K):
        sm = tokens.suffix_mask(K, [m])[0]
        # among all sets of m positions, the suffix is the one made of the m positions that are visible for the FEWEST steps
        order = np.argsort(n_steps_visible, kind="stable")
        assert n_steps_visible[sm].max() <= n_steps_visible[~sm].min() if m < K else sm.all()
        assert set(np.nonzero(sm)[0]) == set(range(K - m, K)) and n_steps_visible[order[:m]].sum() == n_steps_visible[sm].sum()


# ---- the extension header ----
def test_ext_header_is_c99_and_matches_the_ctypes_table(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert names == set(_lib.EXT_SIGNATURES) and not (names & set(_lib.SIGNATURES))
    base = open(os.path.join(ROOT, "include", "selftok_hip.h")).read()
    assert not any(n in base for n in names)
    src = tmp_path / "t.c"
    src.write_text('#include "selftok_hip_ext.h"\nint main(void) { return selftok_attn_kmask_f32 == 0; }\n')
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-Wno-address", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
    import ctypes
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"
    assert _lib.load().selftok_attn_kmask_f32.argtypes == _lib.EXT_SIGNATURES["selftok_attn_kmask_f32"][1]


# ---- mask packing ----
@pytest.mark.parametrize("Kk", [1, 31, 32, 33, 358, 512, 1000, 1024])
def test_pack_key_mask_bit_layout(Kk):
    rng = np.random.RandomState(Kk)
    mask = rng.rand(5, Kk) < 0.5
    mask[0] = True; mask[1] = False
    want = np.zeros((5, (Kk + 31) // 32), dtype=np.uint32)
    for b in range(5):
        for j in np.nonzero(mask[b])[0]:
            want[b, j >> 5] |= np.uint32(1) << np.uint32(j & 31)
    assert np.array_equal(KM.pack_words(mask), want)
    got = ops.pack_key_mask(torch.from_numpy(mask))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy().view(np.uint32), want)


# ---- the GPU case table ----
def test_case_table_holds_the_patterns_it_claims():
    for Kk in (512, 1024):
        c = next(c for c in KM.PATTERN_CASES if c.Kc == Kk and c.see and not c.pre_only and c.B > 5)
        lab = {p[0]: c.mask(b) for b, p in enumerate(c.patterns)}
        los = {int(np.nonzero(v)[0][0]) for n, v in lab.items() if n.startswith("suffix_lo")}
        for e in (32, 128, 256, Kk - 128, Kk - 32):
            assert {e - 1, e, e + 1} <= los
        for n, v in lab.items():
            if n.startswith("suffix_lo"):
                assert v[int(n[9:]):].all() and not v[:int(n[9:])].any()
        assert {int(np.nonzero(lab[f"single{j}"])[0][0]) for j in (0, 31, 32, Kk - 1)} == {0, 31, 32, Kk - 1}
        assert not lab["empty"].any() and lab["full"].all() and lab["odd_keys"].sum() == Kk // 2
        tiles = lab["even_tiles"].reshape(-1, 32)
        assert tiles[0::2].all() and not tiles[1::2].any()
        assert np.array_equal(np.nonzero(lab["last_tile"])[0], np.arange(Kk - 32, Kk))
        gold = np.load(os.path.join(ROOT, "tests", "golden", "sampler_options_b1.npz"))["super_mask"].astype(bool)
        assert np.array_equal(KM.hash_pattern(512), gold) and np.array_equal(lab["hash"], KM.hash_pattern(Kk))
    assert {(c.see, c.pre_only) for c in KM.PATTERN_CASES} >= {(True, False), (False, False), (True, True)}
    b5 = next(c for c in KM.CASES if c.name.startswith("b5"))
    assert b5.B == 5 and len({p[1] for p in b5.patterns}) == 5
    assert {c.Kc for c in KM.TRUNC_CASES} == {358, 33, 1}
    for c in KM.TRUNC_CASES:
        assert c.Kw == 512 and any(c.mask(b)[c.Kc:].any() for b in range(c.B)) and any(len(c.visible(b)) == 0 for b in range(c.B))
    p = KM.PRODUCT_CASE
    assert (p.B, p.H, p.Kc, p.nx) == (64, 24, 512, 256) and len({len(p.visible(b)) for b in range(64)}) == 64


def _sens_samples(case):
    """the product shape: 6 samples x 2 heads here (the GPU test compares all 64 x 24); every other case in full"""
    if case is KM.PRODUCT_CASE:
        return [(b, (0, 23)) for b in (0, 1, 17, 40, 62, 63)]
    return [(b, None) for b in range(case.B)]


def _cat(o_c, o_x):
    return torch.cat([t.reshape(-1) for t in ([o_x] if o_c is None else [o_x, o_c])])


@pytest.mark.parametrize("case", KM.CASES, ids=lambda c: c.name)
def test_every_case_sees_one_wrong_mask_bit(case):
    """flip one bit of one sample (hide its lowest visible key; show key 0 where nothing is visible): that sample's fp64 reference moves
    by >= 1000 x the max-error gate the GPU test applies to the case, so a tolerance test cannot pass with a wrong mask"""
    acc_t = E.ErrAcc()
    moves = []
    for b, heads in _sens_samples(case):
        c, x = KM.sample(case, b)
        vis = case.visible(b)
        c64, x64 = KM.reference(case, b, c, x, True, heads)
        c32, x32 = KM.reference(case, b, c, x, False, heads)
        acc_t.add(_cat(c32, x32), _cat(c64, x64))
        vis2, j = KM.flip_one_bit(case, b)
        c64f, x64f = KM.reference(case, b, c, x, True, heads, vis=vis2)
        d = float((x64f - x64).abs().max())                                  # the image rows are live under both masks
        if c64 is not None and c64f is not None and len(vis2) < len(vis):    # context rows that are live under both masks
            d = max(d, float((c64f - c64[:, 1:]).abs().max()))
        moves.append((d, b, j))
    _, max_gate = E.gate(acc_t.rms, acc_t.mx)
    worst = min(moves)
    print(f"[kmask] {case.name}: torch fp32 max err {acc_t.mx:.3e}, max gate {max_gate:.3e}, smallest one-bit move {worst[0]:.3e} (b={worst[1]}, key {worst[2]})")
    assert worst[0] >= 1000 * max_gate, f"{case.name}: flipping key {worst[2]} of sample {worst[1]} moves the output by only {worst[0]:.3e}"
