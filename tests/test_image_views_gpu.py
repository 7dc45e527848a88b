"""-m gpu: the device image views (csrc/image_views.hip) against the arithmetic of record.  Every comparison is an equality and no view is
left out of any: the entry against the emulation of tests/image_views_cases.py and against live Pillow on every view, its integer tap rows,
the centre view against the existing entry, batching / ordering, sentinels and guard bands, a device table that disagrees with the host's,
`encoding_u8(views=...)` against `encoding(stack(apply_view_pil))`, and tools/tokenize_folder.py --crops ten in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import image_io_cases as IO
import image_views_cases as VC
from selftoktokenizer_amd import _lib, ops, preprocess as P, synth, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = {}
for _c in VC.CASES:
    BATCHES.setdefault((_c.w, _c.h, _c.R, _c.view.size), []).append(_c)


def pack(cases):
    """every distinct source once, at odd offsets -> (uint8 device tensor, sources [N, 3], views [V, 10])"""
    at, chunks, where, sources = 0, [], {}, []
    for c in cases:
        key = (c.w, c.h, c.content)
        if key not in where:
            where[key] = len(sources)
            sources.append((at, c.w, c.h))
            chunks += [VC.image(c).reshape(-1), np.full(5, 0xA5, np.uint8)]
            at += c.w * c.h * 3 + 5
    views = np.array([[where[(c.w, c.h, c.content)]] + list(c.view[:9]) for c in cases], dtype=np.int64)
    return torch.from_numpy(np.concatenate(chunks)).to(DEV), np.array(sources, dtype=np.int64), views


def bits(t):
    t = t.detach().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy().view(np.uint32)


def want_bits(case, bf16):
    t = VC.to_tensor(VC.expected(case), bf16)
    return t if bf16 else t.view(np.uint32)


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    return SelftokPipeline(default_config(512), None, None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False,
                           encoder_mode="exact", vae_mode="exact")


@pytest.mark.parametrize("key", list(BATCHES), ids=lambda k: f"{k[0]}x{k[1]}_R{k[2]}_S{k[3]}")
def test_views_equal_the_emulation_and_live_pillow(key):
    cases = BATCHES[key]
    S = key[3]
    buf, sources, views = pack(cases)
    out16 = ops.image_views(buf, sources, views, S, dtype=torch.bfloat16)
    out32 = ops.image_views(buf, sources, views, S, dtype=torch.float32)
    assert out16.dtype == torch.bfloat16 and out32.dtype == torch.float32 and tuple(out16.shape) == tuple(out32.shape) == (len(cases), 3, S, S)
    b16, b32 = bits(out16), bits(out32)
    for v, c in enumerate(cases):
        assert np.array_equal(b16[v], want_bits(c, True)), f"{c.name}: bf16 output differs from the emulation"
        assert np.array_equal(b32[v], want_bits(c, False)), f"{c.name}: fp32 output differs from the emulation"
        live = P.apply_view_pil(VC.image(c), c.view)
        assert np.array_equal(b32[v], bits(live)) and np.array_equal(b16[v], bits(live.to(torch.bfloat16))), f"{c.name}: differs from live Pillow"


_tap_rows = {}


def tap_rows(insz, outsz, first, S):
    """IO.tables of one axis of one view (box coordinates), computed once per distinct geometry"""
    key = (insz, outsz, first, S)
    if key not in _tap_rows:
        _tap_rows[key] = IO.tables(insz, outsz, first, S)
    return _tap_rows[key]


def check_tap_rows(cases, S):
    """the integer tap rows the kernels left in the workspace == `tables`, both axes of every view of the call: first index, tap count and every
    live coefficient (a row's entries past its own count are not part of the table)"""
    buf, sources, views = pack(cases)
    _, tabs = ops.image_views(buf, sources, views, S, return_tables=True)
    for b, c in enumerate(cases):
        v = c.view
        for axis, insz, outsz, first in (("h", v.bw, v.rw, v.left), ("v", v.bh, v.rh, v.top)):
            xmin, n, k = tap_rows(insz, outsz, first, S)
            gx, gn, gk = (t[b] for t in tabs[axis])
            assert gx.shape == gn.shape == (S,) and gk.shape[0] == S and gk.shape[1] >= k.shape[1], (c.name, axis)
            assert np.array_equal(gx, xmin) and np.array_equal(gn, n), (c.name, axis)
            live = np.arange(k.shape[1])[None, :] < n[:, None]
            assert np.array_equal(gk[:, :k.shape[1]][live], k[live]), (c.name, axis)


@pytest.mark.parametrize("key", list(BATCHES), ids=lambda k: f"{k[0]}x{k[1]}_R{k[2]}_S{k[3]}")
def test_tap_rows_equal_the_emulation(key):
    check_tap_rows(BATCHES[key], key[3])                                      # every view of every case, each geometry in a call of its own


@pytest.mark.parametrize("S", sorted({c.view.size for c in VC.CASES}))
def test_tap_rows_equal_the_emulation_in_the_mixed_batch(S):
    check_tap_rows([c for c in VC.MIXED if c.view.size == S], S)              # group c: rows of different widths share one table pitch


def test_view_center_equals_the_existing_entry_on_its_mixed_batch():
    cases = IO.MIXED
    arrays = [IO.image(c) for c in cases]
    table = np.zeros((len(arrays), 3), dtype=np.int64)
    at = 0
    for i, a in enumerate(arrays):
        table[i] = (at, a.shape[1], a.shape[0])
        at += a.size
    buf = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrays])).to(DEV)
    views = P.view_rows([[P.view_center(c.w, c.h, 256)] for c in cases], 256)
    for dtype in (torch.bfloat16, torch.float32):
        old = ops.image_resize_crop_norm(buf, table, 256, dtype=dtype)
        new = ops.image_views(buf, table, views, 256, dtype=dtype)
        assert np.array_equal(bits(new), bits(old))


def test_batching_and_order_do_not_matter():
    c0 = next(c for c in VC.CASES if c.name == "a_375x500_R281_S256_00")
    ten = P.views_ten(c0.w, c0.h, 281, 256)
    a = VC.image(c0)
    buf = torch.from_numpy(a.reshape(-1).copy()).to(DEV)
    src = np.array([[0, c0.w, c0.h]], dtype=np.int64)
    rows = P.view_rows([ten], 256)
    one = ops.image_views(buf, src, rows, 256)
    for i in range(10):                                                       # ten views in one call == ten calls
        assert torch.equal(ops.image_views(buf, src, rows[i:i + 1], 256)[0], one[i]), i
    cases = [c for c in VC.MIXED if c.view.size == 16]
    buf, sources, views = pack(cases)
    ref = ops.image_views(buf, sources, views, 16)
    rows16 = ops.image_view_rows(sources, views)                              # the [V, 12] rows built by the caller are taken as they are
    assert torch.equal(ops.image_views(buf, None, None, 16, rows=rows16), ref)
    with pytest.raises(_lib.SelftokHipError, match=r"\[V, 12\]"):
        ops.image_views(buf, None, None, 16, rows=views)
    order = [(i * 11 + 3) % len(cases) for i in range(len(cases))]
    assert sorted(order) == list(range(len(cases)))
    assert torch.equal(ops.image_views(buf, sources, views[order], 16), ref[order])
    rep = [i % len(cases) for i in range(256)]                                # V = 256
    got = ops.image_views(buf, sources, views[rep], 16)
    assert tuple(got.shape) == (256, 3, 16, 16) and torch.equal(got, ref[rep])
    for S in sorted({c.view.size for c in VC.MIXED}):                         # group c: the mixed batch of every size (one call has one S), reversed, sources shared
        mixed = [c for c in VC.MIXED if c.view.size == S]
        b = bits(ops.image_views(*pack(mixed), S))
        for i, c in enumerate(mixed):
            assert np.array_equal(b[i], want_bits(c, True)), c.name
    empty = ops.image_views(buf, sources, views[:0], 16, dtype=torch.float32)  # V = 0: an empty tensor, no error
    assert tuple(empty.shape) == (0, 3, 16, 16) and empty.dtype == torch.float32 and empty.is_cuda


def test_sentinels_guard_bands_and_a_device_table_that_disagrees():
    cases = [c for c in VC.MIXED if c.view.size == 16][:40]
    V = len(cases)
    buf, sources, views = pack(cases)
    ref = ops.image_views(buf, sources, views, 16)
    for dtype in (torch.bfloat16, torch.float32):                             # planes outside the batch stay untouched
        big = torch.full((V + 2, 3, 16, 16), -7.0, dtype=dtype, device=DEV)
        ops.image_views(buf, sources, views, 16, dtype=dtype, out=big[1:V + 1])
        assert torch.equal(big[1:V + 1].to(torch.bfloat16), ref) and bool((big[0] == -7.0).all()) and bool((big[V + 1] == -7.0).all())
    # the workspace inside a larger buffer of 0xC3 bytes: nothing outside the queried size is written
    lib = _lib.load()
    rows = ops.image_view_rows(sources, views)
    n = lib.selftok_img_views_u8_workspace_bytes(rows.ctypes.data, V, 16)
    assert n > 0
    guard = 4096
    wsbuf = torch.full((guard + n + guard,), 0xC3, dtype=torch.uint8, device=DEV)
    out = torch.full((V, 3, 16, 16), -7.0, dtype=torch.bfloat16, device=DEV)
    rows_dev = torch.from_numpy(rows).to(DEV)
    lut = ops.image_norm_lut(DEV, torch.bfloat16)
    assert wsbuf.data_ptr() % 16 == 0
    rc = lib.selftok_img_views_u8(buf.data_ptr(), buf.numel(), rows.ctypes.data, rows_dev.data_ptr(), V, 16, out.data_ptr(), 1, lut.data_ptr(), wsbuf.data_ptr() + guard, n,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.selftok_last_error()
    assert torch.equal(out, ref) and bool((wsbuf[:guard] == 0xC3).all()) and bool((wsbuf[guard + n:] == 0xC3).all())
    # device rows that disagree with the host copy: each such view is skipped, the others stay correct, the call returns 0
    bad = rows.copy()
    bad[1, 11] = 2                                                            # a flip that is no flip
    bad[4, 0] = buf.numel()                                                   # a source past the packed buffer
    bad[7, 5:7] = (bad[7, 1] + 1, 1)                                          # a box wider than its source
    bad[9, 9] = bad[9, 7] - 16 + 1                                            # a window outside the resized box
    wide = int(np.argmax(rows[:, 1] == 100))                                  # a legal view of its own (180 rows -> 16) that needs more vertical taps than the host sized
    bad[12] = rows[wide]; bad[12, 7:9] = (16, 16); bad[12, 9:11] = 0
    skipped = [1, 4, 7, 9, 12]
    lay, lay12 = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    alone = np.ascontiguousarray(bad[12:13])
    assert lib.selftok_img_views_tables_layout(rows.ctypes.data, V, 16, lay.ctypes.data) == 0 and lib.selftok_img_views_tables_layout(alone.ctypes.data, 1, 16, lay12.ctypes.data) == 0
    assert lay12[3] > lay[3]
    out = ops.image_views(buf, sources, views, 16, out=torch.full((V, 3, 16, 16), -7.0, dtype=torch.bfloat16, device=DEV), rows_dev=torch.from_numpy(bad).to(DEV))
    for v in range(V):
        if v in skipped:
            assert bool((out[v] == -7.0).all()), v
        else:
            assert torch.equal(out[v], ref[v]), v
    err = _lib.SelftokHipError                                                # the host copy is what refuses
    for col, val, word in ((11, 2, "flip that is neither"), (5, 1000, "box that is empty"), (9, 10 ** 6, "window outside"), (7, 15, "below S")):
        t = views.copy()
        t[3, col - 2] = val
        with pytest.raises(err, match=word):
            ops.image_views(buf, sources, t, 16)
    with pytest.raises(err, match="rows_dev"):
        ops.image_views(buf, sources, views, 16, rows_dev=rows_dev[:-1])
    with pytest.raises(err, match=r"\[V, 10\]"):
        ops.image_views(buf, sources, rows, 16)


def test_encoding_u8_through_views_equals_encoding_of_the_host_route(pipe, monkeypatch):
    arrays = synth.synthetic_u8_images(1, first_index=1) + [VC.image(next(c for c in VC.CASES if c.w == 500))]      # 375 x 500 and 500 x 375
    S = int(pipe.datasize)
    fn = lambda w, h: P.views_ten(w, h, 281, S) if (w, h) != (500, 375) else [P.view_resized_crop(w, h, (17, 23, 200, 150), S, flip=True), P.view_center(w, h, S)]
    host = torch.stack([P.apply_view_pil(a, v) for a in arrays for v in fn(a.shape[1], a.shape[0])])
    assert host.shape[0] == 12
    x = pipe.preprocess_u8(arrays, views=fn)
    assert x.dtype == torch.bfloat16 and np.array_equal(bits(x), bits(host.to(torch.bfloat16)))        # what the VAE is fed
    assert np.array_equal(bits(pipe.preprocess_u8(arrays, dtype=torch.float32, views=fn)), bits(host))
    ids_ref = pipe.encoding(host, device=DEV)
    ids = pipe.encoding_u8(arrays, views=fn)
    assert ids.dtype == ids_ref.dtype and tuple(ids.shape) == (12, 512) and torch.equal(ids, ids_ref)
    tk_ids, tk_scores = pipe.encoding_u8(arrays, views=fn, topk=2)
    assert tuple(tk_ids.shape) == (12, 512, 2) and torch.equal(tk_ids[..., 0], ids_ref) and bool((tk_scores[..., 0] >= tk_scores[..., 1]).all())
    # a uint8 CUDA tensor [B, H, W, 3] gives what the host arrays give
    same = [arrays[1], arrays[1][::-1].copy()]
    t = torch.from_numpy(np.stack(same))
    ten = lambda w, h: P.views_ten(w, h, 281, S)
    a = pipe.preprocess_u8(same, views=ten)
    assert tuple(a.shape) == (20, 3, S, S) and torch.equal(pipe.preprocess_u8(t.to(DEV), views=ten), a) and torch.equal(pipe.preprocess_u8(t, views=ten), a)
    one = lambda w, h: [P.view_resized_crop(w, h, (17, 23, 200, 150), S, flip=True)]
    assert torch.equal(pipe.encoding_u8(t.to(DEV), views=one), pipe.encoding_u8(same, views=one))
    # views=None is the route of before: the existing entry is the one called, the new one is not
    calls = []
    old, new = ops.image_resize_crop_norm, ops.image_views
    monkeypatch.setattr(ops, "image_resize_crop_norm", lambda *a, **k: (calls.append("center"), old(*a, **k))[1])
    monkeypatch.setattr(ops, "image_views", lambda *a, **k: (calls.append("views"), new(*a, **k))[1])
    plain = pipe.preprocess_u8(arrays)
    want = torch.stack([P.apply_view_pil(a, P.view_center(a.shape[1], a.shape[0], S)) for a in arrays]).to(torch.bfloat16)
    assert calls == ["center"] and np.array_equal(bits(plain), bits(want))
    assert torch.equal(pipe.preprocess_u8(arrays, views=lambda w, h: [P.view_center(w, h, S)]), plain) and calls == ["center", "views"]
    assert torch.equal(pipe.preprocess_u8(t.to(DEV)), pipe.preprocess_u8(same)) and calls == ["center", "views", "center", "center"]


def test_loader_batches_with_views_equal_the_host_route():
    arrays = synth.synthetic_u8_images(7, first_index=11)
    fn = lambda w, h: P.mirrored(P.views_five(w, h, 70, 64))[1:8]              # seven views per image, flipped ones among them
    loader = P.DeviceLoader(64, DEV, dtype=torch.float32, workers=2)
    got = list(loader.batches(arrays, 3, views=fn))
    assert [g.shape[0] for g in got] == [21, 21, 7]
    want = torch.stack([P.apply_view_pil(a, v) for a in arrays for v in fn(a.shape[1], a.shape[0])])
    assert np.array_equal(bits(torch.cat(got)), bits(want))
    assert np.array_equal(bits(loader.load(arrays[:2], views=fn)), bits(want[:14]))
    plain = loader.load(arrays[:2])                                           # and without views the loader is the centre crop
    assert np.array_equal(bits(plain), bits(torch.stack([P.apply_view_pil(a, P.view_center(a.shape[1], a.shape[0], 64)) for a in arrays[:2]])))
    loader.close()


def test_tokenize_folder_ten_crop_in_a_child_process(pipe, tmp_path):
    tool = os.path.join(ROOT, "tools", "tokenize_folder.py")
    r = subprocess.run([sys.executable, tool, "--synthetic", "3", "--crops", "ten", "--resize", "281", "--batch", "2", "--encoder-mode", "exact", "--vae-mode", "exact",
                        "--out", str(tmp_path / "ten")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["crops"] == "ten" and line["resize"] == 281 and line["views_per_image"] == 10 and line["views"] == 30 and "TenCrop(256)" in line["recipe"]
    ids = np.load(tmp_path / "ten.rank0.npy")
    assert ids.dtype == np.int64 and ids.shape == (3, 10, 512)
    arrays, ten = synth.synthetic_u8_images(3), lambda w, h: P.views_ten(w, h, 281, 256)
    here = torch.cat([pipe.encoding_u8(arrays[:2], views=ten), pipe.encoding_u8(arrays[2:], views=ten)])       # the tool's batches: two images, then one
    assert np.array_equal(ids.reshape(30, 512), here.cpu().numpy())
    r = subprocess.run([sys.executable, tool, "--synthetic", "3", "--resize", "200"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--resize" in r.stderr
