"""-m gpu: the device image input with a chosen Pillow filter (csrc/image_filters.hip) against the arithmetic of record, all by equality: the
views entry with BICUBIC / BOX and the whole-frame resize against the emulation of tests/image_filters_cases.py and against live Pillow on every
case, the integer tap rows, filter = 2 against the bilinear entry bit for bit, the ADM chain (mixed depths in one batch == each alone),
sentinels and guard bands around the outputs, the workspace and every destination region, device tables that disagree with the host's, N = 0,
`encoding_u8(preprocess=...)`, DeviceLoader, evaluate() by both loader routes, the two tools in child processes, and the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import image_io_cases as IO
import image_filters_cases as FC
import image_views_cases as VC
from selftoktokenizer_amd import _lib, evaluate as E, ops, preprocess as P, synth, weights as W
from selftoktokenizer_amd.config import default_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = FC.FILTER_NAMES


def bits(t):
    t = t.detach().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy().view(np.uint32)


def want_bits(case, bf16):
    t = IO.to_tensor(FC.expected(case), bf16)
    return t if bf16 else t.view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    return SelftokPipeline(default_config(512), None, None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False,
                           encoder_mode="exact", vae_mode="exact")


def big_arrays():
    """uint8 sources for a 256-pixel pipeline: 0, 1 and 2 halvings, an upscale; the largest is 1 Mpixel"""
    t = synth.synthetic_u8_images(2, first_index=3)
    tile = lambda a, h, w: np.ascontiguousarray(np.tile(a, (h // a.shape[0] + 1, w // a.shape[1] + 1, 1))[:h, :w])
    return [t[0], tile(t[1], 520, 601), tile(t[0], 1024, 1024), FC.image(FC.AdmCase("up", 100, 180, 256, "binary")), tile(t[1], 511, 1300)]


@pytest.mark.parametrize("filt", [FC.BICUBIC, FC.BOX], ids=["bicubic", "box"])
def test_views_with_a_filter_equal_the_emulation_live_pillow_and_its_tap_rows(filt):
    for S in sorted({c.view.size for c in FC.VIEW_CASES}):
        cases = [c for c in FC.VIEW_CASES if c.filter == filt and c.view.size == S][::-1]
        buf, rows = FC.pack_views(cases)
        out16 = ops.image_views(dev(buf), None, None, S, dtype=torch.bfloat16, rows=rows, filter=NAME[filt])
        out32, tabs = ops.image_views(dev(buf), None, None, S, dtype=torch.float32, rows=rows, filter=filt, return_tables=True)
        b16, b32 = bits(out16), bits(out32)
        for v, c in enumerate(cases):
            assert np.array_equal(b16[v], want_bits(c, True)) and np.array_equal(b32[v], want_bits(c, False)), f"{c.name}: differs from the emulation"
            live = P.apply_view_pil(FC.image(c), c.view, filter=filt)
            assert np.array_equal(b32[v], bits(live)) and np.array_equal(b16[v], bits(live.to(torch.bfloat16))), f"{c.name}: differs from live Pillow"
            for axis, insz, outsz, first in (("h", c.view.bw, c.view.rw, c.view.left), ("v", c.view.bh, c.view.rh, c.view.top)):
                xmin, n, k = FC.tables(insz, outsz, first, S, filt)
                gx, gn, gk = (t[v] for t in tabs[axis])
                assert gk.shape[1] >= FC.ksize(insz, outsz, filt) and np.array_equal(gx, xmin) and np.array_equal(gn, n), (c.name, axis)
                live_k = np.arange(k.shape[1])[None, :] < n[:, None]
                assert np.array_equal(gk[:, :k.shape[1]][live_k], k[live_k]), (c.name, axis)
        assert tabs["h"][2].shape[2] == max(FC.ksize(c.view.bw, c.view.rw, filt) for c in cases)          # the pitch: the widest row of the call


def run_views_entry(lib, name, buf, rows, S, filt, bf16, rows_dev=None, guard=4096):
    """one C entry called directly, its workspace inside a larger buffer of 0xC3 bytes -> (out, the int32 workspace); filt None: the bilinear entry"""
    V = len(rows)
    fa = () if filt is None else (filt,)
    n = getattr(lib, name + "_workspace_bytes")(rows.ctypes.data, V, S, *fa)
    assert n > 0, lib.selftok_last_error()
    wsbuf = torch.full((guard + n + guard,), 0xC3, dtype=torch.uint8, device=DEV)
    out = torch.full((V + 2, 3, S, S), -7.0, dtype=torch.bfloat16 if bf16 else torch.float32, device=DEV)
    rows_dev = dev(rows) if rows_dev is None else rows_dev
    lut = ops.image_norm_lut(DEV, out.dtype)
    assert wsbuf.data_ptr() % 16 == 0
    rc = getattr(lib, name)(buf.data_ptr(), buf.numel(), rows.ctypes.data, rows_dev.data_ptr(), V, S, *fa, out[1:].data_ptr(), int(bf16), lut.data_ptr(), wsbuf.data_ptr() + guard, n,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.selftok_last_error()
    torch.cuda.synchronize()
    assert bool((wsbuf[:guard] == 0xC3).all()) and bool((wsbuf[guard + n:] == 0xC3).all())               # nothing outside the queried size
    assert bool((out[0] == -7.0).all()) and bool((out[V + 1] == -7.0).all())                            # nor outside the V planes
    return out[1:V + 1], wsbuf[guard:guard + n // 4 * 4].view(torch.int32).cpu().numpy()


@pytest.mark.parametrize("S", sorted({c.view.size for c in VC.MIXED}))
def test_filter_2_is_the_bilinear_entry_bit_for_bit(S):
    """outputs AND the whole workspace (headers, both tap-row blocks, the rows between the passes), on the bilinear entry's own mixed batch of this size"""
    lib = _lib.load()
    cases = [c for c in VC.MIXED if c.view.size == S]
    at, chunks, where = 0, [], {}
    for c in cases:
        if (c.w, c.h, c.content) not in where:
            where[(c.w, c.h, c.content)] = at
            chunks.append(VC.image(c).reshape(-1))
            at += chunks[-1].size
    rows = np.array([[where[(c.w, c.h, c.content)], c.w, c.h] + list(c.view[:9]) for c in cases], dtype=np.int64)
    buf = dev(np.concatenate(chunks))
    lay, lay2 = np.zeros(4, np.int64), np.zeros(4, np.int64)
    assert lib.selftok_img_views_tables_layout(rows.ctypes.data, len(rows), S, lay.ctypes.data) == 0
    assert lib.selftok_img_views_filter_tables_layout(rows.ctypes.data, len(rows), S, 2, lay2.ctypes.data) == 0 and lay.tolist() == lay2.tolist()
    tables_end = int(lay[2] + len(rows) * S * lay[3])
    for bf16 in (True, False):
        old, ws_old = run_views_entry(lib, "selftok_img_views_u8", buf, rows, S, None, bf16)
        new, ws_new = run_views_entry(lib, "selftok_img_views_filter_u8", buf, rows, S, 2, bf16)
        assert np.array_equal(bits(old), bits(new)) and not bool((new == -7.0).all(dim=(1, 2, 3)).any())
        assert (ws_old[:lay[0]].reshape(-1, 20)[:, 0] == 1).all() and tables_end * 4 < ws_old.size * 4
        assert np.array_equal(ws_old, ws_new)                                  # headers, both tap-row blocks, the rows between the passes; what neither writes is 0xC3 in both


@pytest.mark.parametrize("filt", [FC.BOX, FC.BILINEAR, FC.BICUBIC], ids=["box", "bilinear", "bicubic"])
def test_whole_frame_resize_equals_the_emulation_and_live_pillow(filt):
    cases = [c for c in FC.RESIZE_CASES if c.filter == filt]
    for batch in [[c] for c in cases[:3]] + [cases[::-1]]:
        host, frames = FC.pack_resize(batch)
        buf = dev(host)
        assert ops.image_resize(buf, frames, NAME[filt]) is buf
        got = buf.cpu().numpy()
        regions = []
        for c, r in zip(batch, frames):
            out = got[r[3]:r[3] + c.ow * c.oh * 3].reshape(c.oh, c.ow, 3)
            assert np.array_equal(out, FC.expected(c)), f"{c.name}: differs from the emulation"
            assert np.array_equal(out, np.asarray(Image.fromarray(FC.image(c)).resize((c.ow, c.oh), filt))), f"{c.name}: differs from live Pillow"
            regions.append((int(r[3]), c.ow * c.oh * 3))
        for off, n in regions:                                                 # sources, gaps and guard bytes are as they were
            host[off:off + n] = got[off:off + n]
        assert np.array_equal(host, got)


def adm_on_device(cases, S, dtype, depth_dev=None, rows_dev=None):
    buf, depth, rows = FC.pack_adm(cases)
    t = dev(buf)
    for d, frames in enumerate(depth):
        ops.image_resize(t, frames, "box", frames_dev=None if depth_dev is None else depth_dev[d])
    return ops.image_views(t, None, None, S, dtype=dtype, rows=rows, filter="bicubic", rows_dev=rows_dev), t.cpu().numpy(), buf, depth, rows


@pytest.mark.parametrize("S", [16, 24])
def test_adm_chain_equals_the_emulation_and_the_published_function(S):
    cases = [c for c in FC.ADM_CASES if c.S == S][::-1]
    for dtype in (torch.bfloat16, torch.float32):
        out, got, before, depth, rows = adm_on_device(cases, S, dtype)
        b = bits(out)
        for i, c in enumerate(cases):
            assert np.array_equal(b[i], want_bits(c, dtype == torch.bfloat16)), f"{c.name}: differs from the emulation"
            live = P.NormalizeToTensor()(P.center_crop_adm(Image.fromarray(FC.image(c)), S))
            assert np.array_equal(b[i], bits(live.to(dtype))), f"{c.name}: differs from center_crop_arr on live Pillow"
    for frames in depth:                                                       # every halved frame is Pillow's; nothing else in the buffer changed
        for r in frames:
            n = int(r[4] * r[5] * 3)
            src = got[r[0]:r[0] + r[1] * r[2] * 3].reshape(r[2], r[1], 3)
            assert np.array_equal(got[r[3]:r[3] + n].reshape(r[5], r[4], 3), np.asarray(Image.fromarray(src).resize((int(r[4]), int(r[5])), Image.BOX)))
            before[r[3]:r[3] + n] = got[r[3]:r[3] + n]
    assert np.array_equal(before, got)


def test_one_adm_batch_of_mixed_depths_equals_each_alone():
    pick = {}
    for c in FC.ADM_CASES:
        if c.S == 16:
            pick.setdefault((len(FC.adm_numbers(c.w, c.h, 16)[0]) - 1, c.content), c)
    assert {k[0] for k in pick} == {0, 1, 2, 3, 4}
    cases = [pick[k] for k in sorted(pick, key=lambda k: (k[1], -k[0]))]      # depths in no order
    arrays = [FC.image(c) for c in cases]
    with P.DeviceLoader(16, DEV, dtype=torch.float32, workers=2, preprocess="adm") as loader:
        mixed = loader.load(arrays)
        for i, (c, a) in enumerate(zip(cases, arrays)):
            assert np.array_equal(bits(mixed[i]), want_bits(c, False)), c.name
            assert torch.equal(loader.load([a])[0], mixed[i]), c.name
        order = [(i * 7 + 2) % len(arrays) for i in range(len(arrays))]
        assert sorted(order) == list(range(len(arrays))) and torch.equal(loader.load([arrays[i] for i in order]), mixed[order])
        assert loader.last_times["bytes"] < 64 + len(arrays) * (12 + 6 * 4) * 8 + 64 + sum((a.size + 15) // 16 * 16 for a in arrays)      # the halved frames do not cross


def test_device_tables_that_disagree_with_the_hosts():
    lib = _lib.load()
    # the views entry with a filter: skipped views stay untouched, the others are correct, return 0
    cases = [c for c in FC.VIEW_CASES if c.filter == FC.BICUBIC and c.view.size == 16][:24]
    host, rows = FC.pack_views(cases)
    buf = dev(host)
    ref = ops.image_views(buf, None, None, 16, rows=rows, filter="bicubic")
    bad = rows.copy()
    bad[1, 11] = 2                                                            # a flip that is no flip
    bad[4, 0] = buf.numel()                                                   # a source past the packed buffer
    bad[7, 5:7] = (bad[7, 1] + 1, 1)                                          # a box wider than its source
    bad[9, 9] = bad[9, 7] - 16 + 1                                            # a window outside the resized box
    wide = int(np.argmax(rows[:, 1] == 100))                                  # a legal view (180 rows -> 16) that needs more vertical taps than the host sized
    bad[12] = rows[wide]; bad[12, 7:9] = (16, 16); bad[12, 9:11] = 0
    out, _ = run_views_entry(lib, "selftok_img_views_filter_u8", buf, rows, 16, 3, True, rows_dev=dev(bad))
    for v in range(len(cases)):
        assert bool((out[v] == -7.0).all()) if v in (1, 4, 7, 9, 12) else torch.equal(out[v], ref[v]), v
    # the whole-frame entry: a skipped frame's destination stays GUARD, the others are correct
    rc = [c for c in FC.RESIZE_CASES if c.filter == FC.BICUBIC]
    host, frames = FC.pack_resize(rc)
    bad = frames.copy()
    bad[0, 1] = 0                                                             # a side of 0
    bad[2, 0] = host.size                                                     # a source past the buffer
    bad[3, 3] = host.size - 5                                                 # a destination past the buffer
    bad[5, 3] = bad[6, 3] + 3                                                 # a destination on another destination: both are skipped
    bad[8, 3] = bad[9, 0]                                                     # a destination on a source
    assert tuple(frames[11, 4:6]) == (16, 20) and frames[:, 4:6].max() == 300
    bad[11, 4:6] = (320, 1)                                                   # a legal frame of the same bytes that needs a wider launch than the host sized
    skipped = {0, 2, 3, 5, 6, 8, 11}
    n = lib.selftok_img_resize_u8_workspace_bytes(frames.ctypes.data, len(frames), 3)
    guard = 4096
    wsbuf = torch.full((guard + n + guard,), 0xC3, dtype=torch.uint8, device=DEV)
    buf, bad_dev = dev(host), dev(bad)
    assert lib.selftok_img_resize_u8(buf.data_ptr(), buf.numel(), frames.ctypes.data, bad_dev.data_ptr(), len(frames), 3, wsbuf.data_ptr() + guard, n, torch.cuda.current_stream().cuda_stream) == 0
    got = buf.cpu().numpy()
    assert bool((wsbuf[:guard] == 0xC3).all()) and bool((wsbuf[guard + n:] == 0xC3).all())
    for i, (c, r) in enumerate(zip(rc, frames)):
        region = got[r[3]:r[3] + c.ow * c.oh * 3]
        assert (region == FC.GUARD).all() if i in skipped else np.array_equal(region.reshape(c.oh, c.ow, 3), FC.expected(c)), (i, c.name)
        host[r[3]:r[3] + c.ow * c.oh * 3] = region
    assert np.array_equal(host, got)                                           # and nothing was written anywhere else
    with pytest.raises(_lib.SelftokHipError, match="frames_dev"):
        ops.image_resize(buf, frames, "bicubic", frames_dev=bad_dev[:-1])


def test_empty_calls_and_refusals():
    buf = dev(np.full(4096, FC.GUARD, np.uint8))
    assert ops.image_resize(buf, np.zeros((0, 6), np.int64), "box") is buf and bool((buf == FC.GUARD).all())          # N = 0
    empty = ops.image_views(buf, None, None, 16, dtype=torch.float32, rows=np.zeros((0, 12), np.int64), filter="bicubic")
    assert tuple(empty.shape) == (0, 3, 16, 16) and empty.dtype == torch.float32 and empty.is_cuda
    err = _lib.SelftokHipError
    good = np.array([[0, 8, 6, 200, 4, 3]], dtype=np.int64)
    for filt, word in (("lanczos", "LANCZOS"), (Image.HAMMING, "HAMMING"), ("nearest", "NEAREST"), (7, "unknown filter")):
        with pytest.raises(err, match=word):
            ops.image_resize(buf, good, filt)
        with pytest.raises(err, match=word):
            ops.image_views(buf, np.array([[0, 8, 6]]), np.array([[0, 0, 0, 8, 6, 16, 16, 0, 0, 0]]), 16, filter=filt)
    for rows, word in (([[0, 8, 6, 143, 4, 3]], "overlaps"), ([[0, 8, 6, 200, 4, 3], [300, 8, 6, 235, 4, 3]], "overlaps"), ([[0, 8, 6, 4090, 4, 3]], "destination that reaches past"),
                       ([[4000, 8, 6, 200, 4, 3]], "source that reaches past"), ([[0, 8, 0, 200, 4, 3]], "1 .. 65536")):
        with pytest.raises(err, match=word):
            ops.image_resize(buf, np.array(rows, dtype=np.int64), "box")
    assert bool((buf == FC.GUARD).all())                                       # nothing was launched
    with pytest.raises(err, match="1-D uint8"):
        ops.image_resize(buf.view(torch.int8), good, "box")
    with P.DeviceLoader(16, DEV, preprocess="adm") as loader:
        with pytest.raises(ValueError, match="takes no views"):
            loader.load([np.zeros((20, 20, 3), np.uint8)], views=lambda w, h: P.views_five(w, h, 16, 16))


def test_encoding_u8_with_a_preprocess_equals_encoding_of_the_host_route(pipe, tmp_path):
    arrays = big_arrays()
    S = int(pipe.datasize)
    assert [len(P.adm_plan(a.shape[1], a.shape[0], S).frames) - 1 for a in arrays] == [0, 1, 2, 0, 0] and max(a.shape[0] * a.shape[1] for a in arrays) <= 1 << 20
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / f"{i}.png"))
        Image.fromarray(a).save(paths[-1])
    host = torch.stack([P.load_image_adm(p, S) for p in paths])
    x = pipe.preprocess_u8(arrays, preprocess="adm")
    assert x.dtype == torch.bfloat16 and np.array_equal(bits(x), bits(host.to(torch.bfloat16)))        # what the VAE is fed
    assert np.array_equal(bits(pipe.preprocess_u8(arrays, dtype=torch.float32, preprocess="adm")), bits(host))
    ids_ref = pipe.encoding(host, device=DEV)
    ids = pipe.encoding_u8(arrays, preprocess="adm")
    assert ids.dtype == ids_ref.dtype and tuple(ids.shape) == (5, 512) and torch.equal(ids, ids_ref)
    assert not torch.equal(ids, pipe.encoding_u8(arrays))                      # and the recipes do differ
    same = torch.from_numpy(np.stack([arrays[1], arrays[1][::-1].copy()]))     # the tensor forms, host and device
    assert torch.equal(pipe.preprocess_u8(same.to(DEV), preprocess="adm"), pipe.preprocess_u8(list(same.numpy()), preprocess="adm"))
    # "bicubic": Resize(S, BICUBIC) -> CenterCrop, and the ten-crop of Resize(281, BICUBIC)
    small = arrays[:2] + arrays[3:4]
    host = torch.stack([P.load_image(p, S, filter="bicubic") for p in paths[:2] + paths[3:4]])
    assert np.array_equal(bits(pipe.preprocess_u8(small, dtype=torch.float32, preprocess="bicubic")), bits(host))
    assert torch.equal(pipe.encoding_u8(small, preprocess="bicubic"), pipe.encoding(host, device=DEV))
    ten = lambda w, h: P.views_ten(w, h, 281, S)
    host = torch.stack([P.apply_view_pil(a, v, filter="bicubic") for a in small[:2] for v in ten(a.shape[1], a.shape[0])])
    assert np.array_equal(bits(pipe.preprocess_u8(small[:2], dtype=torch.float32, views=ten, preprocess="bicubic")), bits(host))
    ids = pipe.encoding_u8(small[:2], views=ten, preprocess="bicubic")
    assert tuple(ids.shape) == (20, 512) and torch.equal(ids, pipe.encoding(host, device=DEV))
    with pytest.raises(ValueError, match="takes no views"):
        pipe.encoding_u8(small, views=ten, preprocess="adm")
    with pytest.raises(ValueError, match="expected one of"):
        pipe.preprocess_u8(small, preprocess="lanczos")


@pytest.mark.parametrize("mode", ["adm", "bicubic"])
def test_loader_batches_with_a_preprocess_equal_the_host_route(mode):
    arrays = [FC.image(c) for c in FC.ADM_CASES if c.S == 24 and c.content != "stripes"][:11]
    host = (lambda a: P.center_crop_adm(Image.fromarray(a), 24)) if mode == "adm" else (lambda a: P.center_crop(P.resize_shorter_side(Image.fromarray(a), 24, "bicubic"), 24))
    want = torch.stack([P.NormalizeToTensor()(host(a)) for a in arrays])
    with P.DeviceLoader(24, DEV, dtype=torch.float32, workers=2, preprocess=mode) as loader:
        got = list(loader.batches(arrays, 4))
        assert [g.shape[0] for g in got] == [4, 4, 3] and np.array_equal(bits(torch.cat(got)), bits(want))
        if mode == "bicubic":
            fn = lambda w, h: P.mirrored(P.views_five(w, h, 30, 24))[2:7]
            v = torch.cat(list(loader.batches(arrays, 4, views=fn)))
            assert np.array_equal(bits(v), bits(torch.stack([P.apply_view_pil(a, x, filter="bicubic") for a in arrays for x in fn(a.shape[1], a.shape[0])])))
    with P.DeviceLoader(24, DEV, dtype=torch.float32, workers=2) as plain:      # the default is the reference's recipe, untouched
        ref = torch.stack([P.NormalizeToTensor()(P.center_crop(P.resize_shorter_side(Image.fromarray(a), 24), 24)) for a in arrays])
        assert plain.preprocess == "reference" and np.array_equal(bits(plain.load(arrays)), bits(ref))


def test_evaluate_by_both_routes_with_the_adm_protocol(pipe, tmp_path):
    arrays = big_arrays()[:3]
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / f"{i:02d}.png"))
        Image.fromarray(a).save(paths[-1])
    host, device = E.folder_loader(paths, 256, preprocess="adm"), E.folder_loader(paths, 256, device=pipe.device, preprocess="adm")
    h, d = host(0, 3), device(0, 3)
    assert d.is_cuda and d.dtype == torch.float32 and np.array_equal(bits(d), bits(h))
    assert np.array_equal(bits(E.folder_loader(paths, 256, device=pipe.device, preprocess="bicubic")(0, 3)), bits(E.folder_loader(paths, 256, preprocess="bicubic")(0, 3)))
    assert not np.array_equal(bits(h), bits(E.folder_loader(paths, 256)(0, 3)))
    noise = lambda lo, hi: synth.synthetic_noise(hi - lo, first_index=lo)
    r1 = E.evaluate(pipe, host, 3, batch=3, noise_fn=noise)
    r2 = E.evaluate(pipe, device, 3, batch=3, noise_fn=noise)
    assert r1["diffusion"]["psnr_each_dB"] == r2["diffusion"]["psnr_each_dB"] and r1["token_ids_first_image"] == r2["token_ids_first_image"]
    with pytest.raises(ValueError, match="expected one of"):
        E.folder_loader(paths, 256, preprocess="lanczos")


def test_the_tools_with_preprocess_adm_in_child_processes(pipe, tmp_path):
    arrays = big_arrays()[:3]
    folder = tmp_path / "images"
    folder.mkdir()
    for i, a in enumerate(arrays):
        Image.fromarray(a).save(str(folder / f"{i:02d}.png"))
    paths = E.list_images(str(folder))
    tool = os.path.join(ROOT, "tools", "tokenize_folder.py")
    r = subprocess.run([sys.executable, tool, "--images", str(folder), "--preprocess", "adm", "--batch", "2", "--encoder-mode", "exact", "--vae-mode", "exact",
                        "--out", str(tmp_path / "adm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["preprocess"] == "adm" and line["images"] == 3
    ids = np.load(tmp_path / "adm.rank0.npy")
    want = pipe.encoding(torch.stack([P.load_image_adm(p, 256) for p in paths]), device=DEV)
    assert ids.shape == (3, 512) and np.array_equal(ids, want.cpu().numpy())
    r = subprocess.run([sys.executable, tool, "--synthetic", "2", "--preprocess", "adm", "--crops", "ten"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--preprocess adm" in r.stderr
    tool = os.path.join(ROOT, "tools", "eval_psnr.py")
    r = subprocess.run([sys.executable, tool, "--images", str(folder), "--preprocess", "adm", "--device-io", "--batch", "3", "--out", str(tmp_path / "psnr.json")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(open(tmp_path / "psnr.json").read())
    assert line["preprocess"] == "adm" and len(line["diffusion"]["psnr_each_dB"]) == 3 and all(np.isfinite(v) for v in line["diffusion"]["psnr_each_dB"])
    r = subprocess.run([sys.executable, tool, "--synthetic", "2", "--preprocess", "adm"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--preprocess" in r.stderr
