"""not gpu: the tables and goldens of the exact-mode key-mask tests (tests/ex_kmask_cases.py, tests/test_ex_attention_kmask_gpu.py,
tests/test_exact_masks_gpu.py) hold what they claim, and the two new entry points are declared the way the loader binds them."""
import json
import os
import re

import numpy as np
import pytest
import torch

import edge_cases as EC
import ex_kmask_cases as XK
from selftoktokenizer_amd import _lib, ops, tokens
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.schedule import DiTiCont, FlowSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NEW = ("selftok_ex_attention_kmask_f32", "selftok_ex_attention_kmask_fused_f32")


def test_header_and_ctypes_table_agree():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert set(NEW) <= names and names == set(_lib.EXT_SIGNATURES)
    for n, base in zip(NEW, ("selftok_ex_attention_f32", "selftok_ex_attention_fused_f32")):
        res, args = _lib.EXT_SIGNATURES[n]
        bres, bargs = _lib.SIGNATURES[base]
        assert res is bres and args == bargs[:-1] + [_lib._vp, _lib._l, _lib._vp], "the base entry's arguments, then kmask, kmask_bs, stream"
        decl = re.search(n + r"\s*\(([^;]*)\)\s*;", hdr).group(1)
        assert len(decl.split(",")) == len(args) and decl.rstrip().endswith("const unsigned* kmask, long kmask_bs, hipStream_t stream")
    src = open(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "encoder_exact.hip")).read()
    for n in NEW:
        assert re.search(r"^int " + n + r"\(", src, re.M), f"{n} is not defined in csrc/encoder_exact.hip"
    if os.path.exists(_lib.LIB_PATH):
        lib = _lib.load()
        for n in NEW:
            assert getattr(lib, n).argtypes == _lib.EXT_SIGNATURES[n][1]


def test_patterns_are_what_their_names_say():
    K = 512
    h = XK.hash_pattern(K)
    assert 0.6 < h.mean() < 0.73 and not np.array_equal(h, XK.prefix(K, int(h.sum())))
    assert np.array_equal(XK.suffix(K, 301), tokens.suffix_mask(K, [301])[0])
    assert XK.single(K, 100).sum() == 1 and XK.alternating(K).sum() == K // 2
    e = XK.empty_word(K, 5)
    assert not e[160:192].any() and e[128:160].all() and e[192:].all()            # word 5 empty inside the live tile 128 .. 191
    rows = XK.model_rows(K)
    assert rows.shape == (16, K) and rows[0].all() and np.array_equal(rows[1], XK.suffix(K, 301)) and np.array_equal(rows[2], h) and rows[3].sum() == 1
    assert int(np.nonzero(rows[4])[0][0]) > 256
    assert all(rows[b][:376].any() for b in range(16)), "every sample keeps a key at k = 375"
    assert len({r.tobytes() for r in rows}) == 16
    # the packing twin
    m = np.stack([h, XK.suffix(K, 37)])
    assert np.array_equal(XK.pack(m), ops.pack_key_mask(torch.from_numpy(m)).numpy())


def test_case_table_reaches_the_edges_it_claims():
    valid = {(s, v) for s, v, _, _ in XK.PREFIX_CASES}
    for v in (0, 20, 31, 32, 33, 63, 64, 65, 255, 256, 257, 511, 512):
        assert (512, v) in valid
    assert {(1024, 0), (1024, 300), (1024, 512), (1024, 513), (1024, 1024)} <= valid
    lib_ok = lambda a, b: a % 64 == 0 and b % 64 == 0 and ((a + b) % 512 == 0 or (a + b) % 512 <= 384)       # selftok_ex_attention_fused_supported at head_dim 64
    assert all(lib_ok(s, t2) for s, _, t2, _ in XK.PREFIX_CASES) and not any(lib_ok(s, t2) for s, _, t2, _ in XK.PREFIX_CASES_UNFUSED)
    assert all(lib_ok(c.Tk1, c.Tk2) for c in XK.MASK_CASES + XK.SDPA_CASES) and not any(lib_ok(c.Tk1, c.Tk2) for c in XK.MASK_CASES_UNFUSED)
    by = {c.name: XK.case_mask(c) for c in XK.MASK_CASES}
    assert not by["empty_first_block_k1024"][:, :512].any() and by["empty_first_block_k1024"].any(axis=1).all()
    assert not by["no_context_key"][0].any() and by["no_context_key"][1].all()
    assert (by["single_key"].sum(axis=1) == 1).all()
    w = XK.pack(by["empty_word_in_live_tile"])
    for b, word in enumerate((5, 0, 15, 8)):
        assert w[b, word] == 0 and w[b, word ^ 1] == -1                          # the other half of the same 64-key tile is full
    assert len({r.tobytes() for r in by["rows_differ"]}) == 5
    dead = [c for c in XK.MASK_CASES if c.Tk2 == 0 and not XK.case_mask(c).any(axis=1).all()]
    assert dead, "a sample without any visible key"
    assert any(c.shared for c in XK.MASK_CASES) and any(c.shared for c in XK.MASK_CASES_UNFUSED)
    for c in XK.MASK_CASES + XK.MASK_CASES_UNFUSED + XK.SDPA_CASES:
        assert c.Tk1 <= 2048 and c.Tk1 % 16 == 0 and XK.case_mask(c).shape == (c.B, c.Tk1)
        if c.shared:
            assert len(set(c.rows)) == 1


@pytest.mark.parametrize("c", XK.MASK_CASES + XK.SDPA_CASES, ids=lambda c: c.name)
def test_one_flipped_mask_bit_moves_the_reference_far_beyond_the_gate(c):
    """a kernel that got one bit of the pattern wrong cannot pass test 6: flipping one mask bit of one sample moves the fp64 output of that sample by >= 1000x the
    gate's max bound (taken from torch fp32's own error on the case).  Checked on the first sample's rows to keep the CPU time small."""
    small = XK.Case(c.name, c.Tk1, c.Tk2, min(c.Tq, 32), c.rows[:1], c.H)
    q, ctx, img = XK.inputs(c)
    q, ctx, img = q[:1, :small.Tq], ctx[:1], img[:1]
    mask = XK.case_mask(c)[:1]
    ref = XK.reference(small, q, ctx, img, mask, torch.float64)
    t32 = XK.reference(small, q, ctx, img, mask, torch.float32)
    acc = EC.ErrAcc()
    acc.add(t32, ref)
    _, max_b = EC.gate(acc.rms, acc.mx)
    vis, inv = np.nonzero(mask[0])[0], np.nonzero(~mask[0])[0]
    flips = [int(p[len(p) // 2]) for p in (vis, inv) if p.size] + [int(p[0]) for p in (vis, inv) if p.size]
    for j in flips:
        m2 = mask.copy()
        m2[0, j] = ~m2[0, j]
        if not m2.any() and not c.Tk2:
            continue
        moved = float((XK.reference(small, q, ctx, img, m2, torch.float64) - ref).abs().max())
        assert moved >= 1000 * max_b, f"{c.name}: flipping bit {j} moves the reference by {moved:.3e}, gate {max_b:.3e}"


def test_goldens_load_and_match_the_schedule():
    K = 512
    pin = json.load(open(os.path.join(GOLD, "PINNING_exact_masks.json")))
    assert pin["host_check"]["same_bits"] is True and pin["host_check"]["cfg16_crc"] == pin["host_check"]["committed"]
    old = np.load(os.path.join(GOLD, "cfg_b16.npz"))
    assert pin["host_check"]["committed"] == [int(old["crc_1"]), int(old["crc_2"])]
    g = np.load(os.path.join(GOLD, "exact_masks_b16.npz"))
    assert bool(g["host_check_same_bits"])
    fs = FlowSchedule(50, 1.0)
    p = default_config(K).tokenizer.params
    ktab = DiTiCont(1000, K, p.stages, p.k_per_stage).to_indices(fs.t_long)
    for tag, pat in (("hash", XK.hash_pattern(K)), ("suffix301", XK.suffix(K, 301))):
        assert [int(k) for k in g[f"{tag}_k"]] == [int(ktab[0]), int(ktab[1])]
        assert [int(n) for n in g[f"{tag}_visible"]] == [int((pat & (np.arange(K) <= ktab[i])).sum()) for i in (0, 1)]
        for s in (1, 2):
            assert g[f"{tag}_sub_{s}"].shape == (16, 16, 8, 8) and np.isfinite(g[f"{tag}_sub_{s}"]).all()
    i = int(g["fwd_index"])
    assert i == 30 and int(g["fwd_k"]) == int(ktab[i]) == 375
    assert np.array_equal(g["fwd_visible"], (XK.model_rows(K) & (np.arange(K)[None] <= 375)).sum(axis=1))
    assert g["fwd_sub"].shape == (16, 16, 8, 8) and np.isfinite(g["fwd_sub"]).all()
    g2 = np.load(os.path.join(GOLD, "exact_masks_k1024_b16.npz"))
    kt = DiTiCont(1000, 1024, p.stages, "384,368,144,96,32").to_indices(fs.t_long)
    assert int(g2["k"]) == int(kt[int(g2["step"])]) and int(g2["visible"]) == int((XK.suffix(1024, 300) & (np.arange(1024) <= int(g2["k"]))).sum())
    assert int(g2["k"]) >= 724 and g2["vsub"].shape == (16, 16, 8, 8)
    sd = np.load(os.path.join(GOLD, "ex_kmask_sdpa.npz"))
    assert set(sd.files) == {c.name for c in XK.SDPA_CASES}
    for c in XK.SDPA_CASES:
        assert sd[c.name].shape == (2, 128, 128) and sd[c.name].dtype == np.float32 and np.isfinite(sd[c.name]).all()
    for f in ("ex_kmask_sdpa.npz", "exact_masks_b16.npz", "exact_masks_k1024_b16.npz"):
        assert os.path.getsize(os.path.join(GOLD, f)) < (1 << 20)
