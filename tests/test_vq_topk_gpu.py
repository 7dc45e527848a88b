"""-m gpu: the VQ top-k lookup (csrc/vq_topk.hip, ops.vq_topk, SelftokPipeline.encoding_topk, tools/tokenize_folder.py --topk) against the
host emulation of tests/vq_topk_cases.py.  Every check is an equality: ids, and scores bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import vq_topk_cases as T
from oracle import clib
from selftoktokenizer_amd import _lib, ops, synth, tokens, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
_packed = {}


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if torch.is_tensor(a) else a, np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.array(a, np.float32)).cuda()          # a copy: the cases' arrays are read-only


def packed_of(case):
    if case.name not in _packed:
        _packed[case.name] = ops.vq_pack_codebook(dev(T.make(case)[1]))
    return _packed[case.name]


def same(got, want, what):
    ids, sc = got
    assert tuple(ids.shape) == want[0].shape == tuple(sc.shape), what
    assert np.array_equal(ids.cpu().numpy().astype(np.int64), want[0]), f"{what}: ids differ"
    assert np.array_equal(bits(sc), bits(want[1])), f"{what}: score bits differ"


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_every_case_equals_the_emulation(case):
    """k = 1, 2, 3, 8; int64 and int32 ids; normalised in the kernel and SELFTOK_PRENORMED on the oracle's own unit rows"""
    z, cb, _ = T.make(case)
    pk, zc, xc = packed_of(case), dev(z), dev(clib.l2norm16(z))
    for k in T.KS:
        want = T.case_ref(case, k)
        for dt in (torch.int64, torch.int32):
            got = ops.vq_topk(zc, pk, k, ids_dtype=dt)
            assert got[0].dtype == dt and got[1].dtype == torch.float32
            same(got, want, f"{case.name} k={k} {dt}")
            same(ops.vq_topk(xc, pk, k, ids_dtype=dt, prenormed=True), want, f"{case.name} k={k} {dt} prenormed")


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_column_0_is_the_argmax_entry(case):
    z, _, _ = T.make(case)
    pk, zc = packed_of(case), dev(z)
    for coarse in (None, False):                 # the default argmax route (f16 coarse pass + exact re-score) and the fp32-input MFMA kernel
        ids1, best = ops.vq_encode(zc, pk, packed=True, return_best=True, coarse=coarse)
        for k in (1, 8):
            ids, sc = ops.vq_topk(zc, pk, k)
            assert torch.equal(ids[:, 0], ids1), f"coarse={coarse} k={k}"
            assert torch.equal(sc[:, 0].contiguous().view(torch.int32), best.view(torch.int32)), f"coarse={coarse} k={k}"


@pytest.mark.parametrize("case", [c for c in T.CASES if c.C >= 64 and (c.tags or c.name.startswith("one_stream"))], ids=lambda c: c.name)
def test_launch_shape_overrides_give_the_same_bytes(case):
    z, _, _ = T.make(case)
    pk, zc = packed_of(case), dev(z)
    for k in (2, 8):
        want = T.case_ref(case, k)
        for rt in (1, 2, 4):
            for split in (1, 2, 3, 8, 64):
                same(ops.vq_topk(zc, pk, k, rt=rt, split=split), want, f"{case.name} k={k} rt={rt} split={split}")


def test_a_row_alone_equals_the_row_inside_the_batch():
    case = next(c for c in T.CASES if c.name.startswith("dups_N129"))
    z, _, plan = T.make(case)
    pk = packed_of(case)
    ids, sc = T.case_ref(case, 8)
    for r in sorted(set(plan["dups"]) | {7, 128}):
        same(ops.vq_topk(dev(z[r:r + 1]), pk, 8), (ids[r:r + 1], sc[r:r + 1]), f"row {r} alone")


def _raw_call(z, pk, ids, scores, ws, N, C, D, k, flags=0):
    p = lambda t: None if t is None else t.data_ptr()
    return _lib.load().selftok_vq_topk_packed_f32(p(z), p(pk), p(ids), p(scores), p(ws), N, C, D, k, flags, torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("k", [1, 3, 8])
def test_guard_bands_stay_intact(k):
    """ids, scores and the workspace sit inside 0xFF / NaN-filled buffers; only ids [N, k], scores [N, k] and the queried workspace bytes may change"""
    case = next(c for c in T.CASES if c.name.startswith("random_N129_C32"))
    z, _, _ = T.make(case)
    N, C, G = case.N, case.C, 4096
    pk, zc = packed_of(case), dev(z)
    wsb = _lib.load().selftok_vq_topk_workspace_bytes(N, C, k)
    assert wsb == min(64, C // 32) * N * {1: 1, 3: 4, 8: 8}[k] * 8
    for i32 in (False, True):
        isz = 4 if i32 else 8
        ids = torch.full((G + N * k * isz + G,), 0xFF, dtype=torch.uint8, device="cuda")
        sc = torch.full((G + N * k * 4 + G,), 0xFF, dtype=torch.uint8, device="cuda")
        ws = torch.full((G + wsb + G,), 0xFF, dtype=torch.uint8, device="cuda")
        assert _raw_call(zc, pk, ids[G:], sc[G:], ws[G:], N, C, 16, k, 1 if i32 else 0) == 0
        torch.cuda.synchronize()
        for buf, n in ((ids, N * k * isz), (sc, N * k * 4), (ws, wsb)):
            assert bool((buf[:G] == 0xFF).all()) and bool((buf[G + n:] == 0xFF).all())
        got_ids = ids[G:G + N * k * isz].view(torch.int32 if i32 else torch.int64).reshape(N, k)
        same((got_ids, sc[G:G + N * k * 4].view(torch.float32).reshape(N, k)), T.case_ref(case, k), f"guarded k={k} i32={i32}")


def test_empty_batch_and_refusals_write_nothing():
    case = next(c for c in T.CASES if c.name.startswith("random_N31_C64"))
    z, cb, _ = T.make(case)
    pk, zc = packed_of(case), dev(z)
    lib = _lib.load()
    ids = torch.full((31 * 8,), -7, dtype=torch.int64, device="cuda")
    sc = torch.full((31 * 8,), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.full((lib.selftok_vq_topk_workspace_bytes(31, 64, 8),), 0xFF, dtype=torch.uint8, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return bool((ids == -7).all()) and bool(torch.isnan(sc).all()) and bool((ws == 0xFF).all())

    assert _raw_call(zc, pk, ids, sc, ws, 0, 64, 16, 2) == 0 and untouched()
    assert _raw_call(None, pk, None, None, None, 0, 64, 16, 2) == 0
    e_ids, e_sc = ops.vq_topk(zc[:0], pk, 2)
    assert tuple(e_ids.shape) == (0, 2) == tuple(e_sc.shape)
    for (N, C, D, k), word in (((31, 64, 16, 0), "k must be in 1..8"), ((31, 64, 16, 9), "k must be in 1..8"), ((31, 64, 16, -1), "k must be in 1..8"),
                               ((31, 64, 8, 2), "D == 16"), ((31, 48, 16, 2), "C % 32 == 0"), ((31, 0, 16, 2), "C % 32 == 0"), ((-1, 64, 16, 2), "N < 0")):
        assert _raw_call(zc, pk, ids, sc, ws, N, C, D, k) == -1, (N, C, D, k)
        assert word in lib.selftok_last_error().decode(), (word, lib.selftok_last_error().decode())
        assert untouched(), (N, C, D, k)
    assert _raw_call(zc, pk, None, sc, ws, 31, 64, 16, 2) == -1 and "null" in lib.selftok_last_error().decode() and untouched()
    assert lib.selftok_vq_topk_workspace_bytes(31, 64, 9) == 0 and lib.selftok_vq_topk_workspace_bytes(31, 48, 2) == 0
    with pytest.raises(_lib.SelftokHipError):
        ops.vq_topk(zc, pk, 9)


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    p = SelftokPipeline(default_config(512), ckpt_path=None, sd3_path=None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"))
    p.verbose = False
    return p


def test_encoding_topk_on_the_golden_images(pipe):
    """default (exact) encoder mode: column 0 is `encoding` and the reference's tokens, the whole result is the emulation on the reference's own
    pre-quantizer features, and one image alone gives the bits it gives inside the batch of 16"""
    assert pipe.model.encoder.mode == "exact"
    g = np.load(os.path.join(GOLD, "pipeline_b16.npz"))
    images = synth.synthetic_images(16)
    ids, sc = pipe.encoding_topk(images, k=2, device="cuda")
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and tuple(ids.shape) == (16, 512, 2) == tuple(sc.shape)
    assert torch.equal(ids[..., 0], pipe.encoding(images, device="cuda"))
    assert np.array_equal(ids[..., 0].cpu().numpy(), g["tokens"].astype(np.int64))
    cb = W._synth_tensor("encoder.quantizer._codebook.embed", (1, 32768, 16), "cpu")[0].contiguous().numpy()
    want = T.topk_ref(g["z"].reshape(-1, 16), cb, 2)
    same((ids.reshape(-1, 2), sc.reshape(-1, 2)), want, "encoding_topk vs the emulation on the golden z")
    m = tokens.margins(sc)
    assert torch.equal(m, sc[..., 0] - sc[..., 1]) and bool((m >= 0).all())
    ids1, sc1 = pipe.encoding_topk(images[:1], k=2, device="cuda")
    assert torch.equal(ids1, ids[:1]) and torch.equal(sc1.view(torch.int32), sc[:1].contiguous().view(torch.int32))


def test_encoding_u8_topk_is_encoding_topk_of_the_preprocessed_images(pipe):
    imgs = synth.synthetic_u8_images(3)
    ids, sc = pipe.encoding_u8(imgs, topk=2)
    ids2, sc2 = pipe.encoding_topk(pipe.preprocess_u8(imgs), 2)
    assert torch.equal(ids, ids2) and torch.equal(sc.view(torch.int32), sc2.view(torch.int32))
    assert torch.equal(ids[..., 0], pipe.encoding_u8(imgs))


def test_tokenize_folder_topk_in_a_child_process(tmp_path):
    """--topk leaves the id file as it is and adds <out>.rank0.topk.npz, whose column 0 is that id file"""
    tool = os.path.join(ROOT, "tools", "tokenize_folder.py")
    lines = {}
    for name, extra in (("plain", []), ("topk", ["--topk", "2"])):
        r = subprocess.run([sys.executable, tool, "--synthetic", "8", "--batch", "8", "--out", str(tmp_path / name)] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines[name] = json.loads(r.stdout.strip().splitlines()[-1])
    plain, ids = np.load(tmp_path / "plain.rank0.npy"), np.load(tmp_path / "topk.rank0.npy")
    assert plain.dtype == np.int64 and plain.shape == (8, 512) and np.array_equal(plain, ids)
    assert not os.path.exists(tmp_path / "plain.rank0.topk.npz")
    tk = np.load(tmp_path / "topk.rank0.topk.npz")
    assert tk["ids"].dtype == np.uint16 and tk["ids"].shape == (8, 512, 2) and tk["scores"].dtype == np.float32 and tk["scores"].shape == (8, 512, 2)
    assert np.array_equal(tk["ids"][..., 0].astype(np.int64), plain)
    m = tokens.margins(tk["scores"])
    assert (m >= 0).all() and (tk["ids"][..., 0] != tk["ids"][..., 1]).all()
    assert set(lines["topk"]) - set(lines["plain"]) == {"topk", "rank0_margin_below_1e-5", "rank0_margin_below_1e-4", "rank0_min_margin"}
    assert lines["topk"]["rank0_min_margin"] == float(m.min()) and lines["topk"]["rank0_margin_below_1e-4"] == int((m < 1e-4).sum())
    assert lines["topk"]["rank0_margin_below_1e-5"] == int((m < 1e-5).sum())
