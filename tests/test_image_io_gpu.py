"""-m gpu: the device image I/O (csrc/image_io.hip) against the arithmetic of record.  Every comparison is equality: the resize / crop /
normalise entry against the golden crc32s (and live Pillow when it is the recorded version) on every case of tests/image_io_cases.py,
its integer tap tables against the emulation's, batching / ordering / sentinels, `encoding_u8` against `encoding(stack(load_image))`,
the uint8 output entry on every bf16 pattern, the refusals and the double-buffered loader."""
import os

import numpy as np
import pytest
import torch

import image_io_cases as IO
from selftoktokenizer_amd import _lib, evaluate as E, ops, preprocess, synth, weights as W
from selftoktokenizer_amd.config import default_config
from selftoktokenizer_amd.pipeline import NormalizeToTensor

pytestmark = pytest.mark.gpu
DEV = "cuda"


def pack(arrays, order=None, gap=0):
    """-> (uint8 device tensor, [B, 3] table); `order`: the order the pixels lie in the buffer; `gap`: unused bytes between images"""
    order = list(range(len(arrays))) if order is None else list(order)
    table = np.zeros((len(arrays), 3), dtype=np.int64)
    chunks, at = [], 0
    for i in order:
        a = arrays[i]
        table[i] = (at, a.shape[1], a.shape[0])
        chunks += [a.reshape(-1), np.full(gap, 0xA5, np.uint8)]
        at += a.size + gap
    return torch.from_numpy(np.concatenate(chunks)).to(DEV), table


def bits(t):
    t = t.detach().cpu()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy().view(np.uint32)


def host_chain(a, S):
    from PIL import Image
    return NormalizeToTensor()(preprocess.center_crop(preprocess.resize_shorter_side(Image.fromarray(a), S), S))


@pytest.fixture(scope="module")
def golden():
    return np.load(IO.GOLDEN)


@pytest.fixture(scope="module")
def pipe():
    from mimogpt.infer.SelftokPipeline import SelftokPipeline
    sd = W.synthetic_state_dict(W.expected_shapes(512), device="cuda")
    return SelftokPipeline(default_config(512), None, None, device="cuda", state_dict=sd, vae_state_dict=W.synthetic_vae_state_dict(device="cuda"), verbose=False,
                           encoder_mode="exact", vae_mode="exact")


@pytest.mark.parametrize("case", IO.CASES, ids=lambda c: c.name)
def test_resize_crop_norm_equals_golden_and_pillow(case, golden):
    import PIL
    a = IO.image(case)
    buf, table = pack([a])
    i = list(golden["names"]).index(case.name)
    lut = IO.normalize_lut()
    out16 = ops.image_resize_crop_norm(buf, table, case.S, dtype=torch.bfloat16)
    out32 = ops.image_resize_crop_norm(buf, table, case.S, dtype=torch.float32)
    assert out16.dtype == torch.bfloat16 and out32.dtype == torch.float32 and tuple(out16.shape) == tuple(out32.shape) == (1, 3, case.S, case.S)
    assert IO.crc(bits(out16)[0]) == int(golden["crc_bf16"][i]), "bf16 output differs from the recorded tensor"
    u8 = np.searchsorted(lut, out32[0].cpu().numpy()).astype(np.uint8)                       # the table is strictly increasing: invert it
    assert np.array_equal(lut[u8].view(np.uint32), bits(out32)[0]), "fp32 output holds a value outside the 256-entry table"
    assert IO.crc(u8.transpose(1, 2, 0)) == int(golden["crc_u8"][i]), "fp32 output differs from the recorded uint8 crop"
    if PIL.__version__ == str(golden["pillow_version"]):
        want = host_chain(a, case.S)
        assert np.array_equal(bits(out32)[0], bits(want)) and np.array_equal(bits(out16)[0], bits(want.to(torch.bfloat16)))
    else:
        print(f"Pillow {PIL.__version__} is not the recorded {golden['pillow_version']}: golden comparison only")


def test_tap_tables_equal_the_emulation(golden):
    names = ["g500x375", "g375x500", "g255x255", "g77x1031", "one_wide", "one_high", "crop_43p5_up", "side_is_S_h700", "taps49_6000"]
    cases = [IO.BY_NAME[n] for n in names]
    arrays = [IO.image(c) for c in cases]
    buf, table = pack(arrays)
    _, tabs = ops.image_resize_crop_norm(buf, table, 256, return_tables=True)
    for b, c in enumerate(cases):
        ow, oh = IO.target_size(c.w, c.h, 256)
        for axis, insz, outsz in (("h", c.w, ow), ("v", c.h, oh)):
            xmin, n, k = IO.tables(insz, outsz, IO.crop_offset(outsz, 256), 256)
            gx, gn, gk = (t[b] for t in tabs[axis])
            assert np.array_equal(gx, xmin) and np.array_equal(gn, n), (c.name, axis)
            for i in range(256):
                assert np.array_equal(gk[i, :n[i]], k[i, :n[i]]), (c.name, axis, i)
    def written(t, b, width):                                                                # taps at x >= n are never written: compare them as 0
        gx, gn, gk = (a[b] for a in t)
        return gx, gn, np.where(np.arange(gk.shape[1])[None, :] < gn[:, None], gk, 0)[:, :width]
    # ... and the recorded full-width tables: (500 -> 341) is g500x375's horizontal pass, columns 42 .. 298
    rk = golden["tab_500_341_k"]
    gx, gn, gk = written(tabs["h"], 0, rk.shape[1])
    assert np.array_equal(gx, golden["tab_500_341_xmin"][42:298]) and np.array_equal(gn, golden["tab_500_341_n"][42:298]) and np.array_equal(gk, rk[42:298])
    rk = golden["tab_6000_256_k"]                                                            # 6000 -> 256: every column, 49 taps
    gx, gn, gk = written(tabs["h"], 8, rk.shape[1])
    assert np.array_equal(gx, golden["tab_6000_256_xmin"]) and np.array_equal(gn, golden["tab_6000_256_n"]) and gn.max() >= 47 and np.array_equal(gk, rk)


def test_mixed_batch_order_and_sentinels(golden):
    cases = IO.MIXED
    arrays = [IO.image(c) for c in cases]
    B = len(cases)
    want = [int(golden["crc_bf16"][list(golden["names"]).index(c.name)]) for c in cases]
    buf, table = pack(arrays)
    mixed = ops.image_resize_crop_norm(buf, table, 256)
    assert [IO.crc(bits(mixed)[b]) for b in range(B)] == want                                # the batch == each image alone (the per-case test)
    order = [(b * 7 + 3) % B for b in range(B)]
    assert sorted(order) == list(range(B))
    buf2, table2 = pack(arrays, order=order, gap=13)                                         # pixels in another order, odd offsets, gaps
    assert torch.equal(ops.image_resize_crop_norm(buf2, table2, 256), mixed)
    big = torch.full((B + 2, 3, 256, 256), -7.0, dtype=torch.bfloat16, device=DEV)           # planes outside the batch stay untouched
    ops.image_resize_crop_norm(buf, table, 256, out=big[1:B + 1])
    assert torch.equal(big[1:B + 1], mixed) and bool((big[0] == -7.0).all()) and bool((big[B + 1] == -7.0).all())
    bigf = torch.full((B + 2, 3, 256, 256), -7.0, dtype=torch.float32, device=DEV)
    ops.image_resize_crop_norm(buf, table, 256, dtype=torch.float32, out=bigf[1:B + 1])
    assert torch.equal(bigf[1:B + 1].to(torch.bfloat16), mixed) and bool((bigf[0] == -7.0).all()) and bool((bigf[B + 1] == -7.0).all())


TINY = [IO.Case("tiny_wide", 40, 24, 16, "noise"), IO.Case("tiny_high", 24, 40, 16, "noise"), IO.Case("tiny_identity", 16, 16, 16, "noise"),
        IO.Case("tiny_taps", 37, 180, 16, "noise")]                                         # wider, higher, identity taps on both axes, many vertical taps


@pytest.fixture(scope="module")
def tiny():
    """the four tiny sources packed, their [4, 3] table, and the emulation's tensors {dtype: device [4, 3, 16, 16]}, computed once"""
    buf, table = pack([IO.image(c) for c in TINY])
    u8 = [IO.resize_crop(IO.image(c), 16) for c in TINY]
    want = {torch.bfloat16: torch.from_numpy(np.stack([IO.to_tensor(u, True) for u in u8]).view(np.int16)).view(torch.bfloat16).to(DEV),
            torch.float32: torch.from_numpy(np.stack([IO.to_tensor(u, False) for u in u8])).to(DEV)}
    return buf, table, want


def test_tiny_batch_guard_bands_and_sentinels(tiny):
    """the workspace inside a larger buffer of 0xC3 bytes, the output between two sentinel planes: nothing outside the queried size and
    outside the batch is written, and the batch equals the emulation"""
    buf, table, want = tiny
    B, guard = len(TINY), 4096
    lib = _lib.load()
    n = lib.selftok_img_resize_crop_norm_u8_workspace_bytes(table.ctypes.data, B, 16)
    assert n > 0
    table_dev = torch.from_numpy(table).to(DEV)
    for dtype in (torch.bfloat16, torch.float32):
        wsbuf = torch.full((guard + n + guard,), 0xC3, dtype=torch.uint8, device=DEV)
        big = torch.full((B + 2, 3, 16, 16), -7.0, dtype=dtype, device=DEV)
        lut = ops.image_norm_lut(DEV, dtype)
        assert wsbuf.data_ptr() % 16 == 0
        rc = lib.selftok_img_resize_crop_norm_u8(buf.data_ptr(), buf.numel(), table.ctypes.data, table_dev.data_ptr(), B, 16, big[1:].data_ptr(), int(dtype == torch.bfloat16),
                                                 lut.data_ptr(), wsbuf.data_ptr() + guard, n, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, lib.selftok_last_error()
        assert np.array_equal(bits(big[1:B + 1]), bits(want[dtype])) and bool((big[0] == -7.0).all()) and bool((big[B + 1] == -7.0).all())
        assert bool((wsbuf[:guard] == 0xC3).all()) and bool((wsbuf[guard + n:] == 0xC3).all())
        assert np.array_equal(bits(ops.image_resize_crop_norm(buf, table, 16, dtype=dtype)), bits(want[dtype]))


def test_tiny_batch_with_a_device_table_that_disagrees(tiny):
    """device rows that disagree with the host copy are skipped, the others stay correct, the call returns 0"""
    buf, table, want = tiny
    bad = table.copy()
    bad[0] = (0, 64, 64)                                                                     # inside the buffer, but 64 rows -> 16 needs more vertical taps than the host sized
    bad[1, 0] = buf.numel()                                                                  # an offset past the packed buffer
    assert 3 * 64 * 64 <= buf.numel()
    lib = _lib.load()
    lay, lay0 = np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.int64)
    alone = np.ascontiguousarray(bad[0:1])
    assert lib.selftok_img_resize_tables_layout(table.ctypes.data, 4, 16, lay.ctypes.data) == 0 and lib.selftok_img_resize_tables_layout(alone.ctypes.data, 1, 16, lay0.ctypes.data) == 0
    assert lay0[3] > lay[3]
    for dtype in (torch.bfloat16, torch.float32):
        out = ops.image_resize_crop_norm(buf, table, 16, dtype=dtype, out=torch.full((4, 3, 16, 16), -7.0, dtype=dtype, device=DEV), table_dev=torch.from_numpy(bad).to(DEV))
        assert bool((out[:2] == -7.0).all()) and np.array_equal(bits(out[2:]), bits(want[dtype][2:]))


def test_batch_of_256(golden):
    small = [c for c in IO.MIXED if c.w * c.h <= 1 << 20]
    cases = [small[b % len(small)] for b in range(256)]
    imgs = {c.name: IO.image(c) for c in small}
    buf, table = pack([imgs[c.name] for c in cases])
    out = ops.image_resize_crop_norm(buf, table, 256)
    crcs = {c.name: int(golden["crc_bf16"][list(golden["names"]).index(c.name)]) for c in small}
    ob = bits(out)
    assert [IO.crc(ob[b]) for b in range(256)] == [crcs[c.name] for c in cases]


def test_encoding_u8_equals_encoding_of_load_image(pipe):
    arrays = synth.synthetic_u8_images(16)
    assert len({a.shape for a in arrays}) >= 6
    ref = torch.stack([host_chain(a, 256) for a in arrays])
    x = pipe.preprocess_u8(arrays)
    assert x.dtype == torch.bfloat16 and np.array_equal(bits(x), bits(ref.to(DEV).to(torch.bfloat16)))    # what the VAE is fed
    assert np.array_equal(bits(pipe.preprocess_u8(arrays, dtype=torch.float32)), bits(ref))
    ids_ref = pipe.encoding(ref, device=DEV)
    ids = pipe.encoding_u8(arrays)
    assert ids.dtype == ids_ref.dtype and torch.equal(ids, ids_ref)
    same = [a for a in arrays if a.shape == arrays[0].shape]
    t = torch.from_numpy(np.stack(same))                                                     # the [B, H, W, 3] tensor forms, host and device
    want = torch.stack([host_chain(a, 256) for a in same]).to(torch.bfloat16)
    assert np.array_equal(bits(pipe.preprocess_u8(t)), bits(want)) and np.array_equal(bits(pipe.preprocess_u8(t.to(DEV))), bits(want))


def test_evaluate_by_both_routes(pipe, tmp_path):
    from PIL import Image
    arrays = synth.synthetic_u8_images(16)
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / f"{i:02d}.png"))
        Image.fromarray(a).save(paths[-1])
    host, dev = E.folder_loader(paths, 256), E.folder_loader(paths, 256, device=pipe.device)
    h, d = host(0, 16), dev(0, 16)
    assert d.is_cuda and d.dtype == torch.float32 and np.array_equal(bits(d), bits(h))
    noise = lambda lo, hi: synth.synthetic_noise(hi - lo, first_index=lo)
    r1 = E.evaluate(pipe, host, 16, batch=16, noise_fn=noise)
    r2 = E.evaluate(pipe, dev, 16, batch=16, noise_fn=noise)
    assert r1["diffusion"]["psnr_each_dB"] == r2["diffusion"]["psnr_each_dB"] and r1["token_ids_first_image"] == r2["token_ids_first_image"]


def test_to_u8_every_bf16_pattern_and_fp32_sample():
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = torch.from_numpy(pat.view(np.int16).copy()).view(torch.bfloat16)
    ok = ~torch.isnan(x)
    want = np.zeros(65536, np.uint8)                                                         # NaN -> 0: this project's choice
    want[ok.numpy()] = x.clone().mul_(255).add_(0.5).clamp_(0, 255)[ok].to(torch.uint8).numpy()
    img = x.reshape(1, 1, 128, 512).expand(2, 3, 128, 512).clone()
    img[1] = img[1].flip(-1)
    img[:, 1] = img[:, 1].roll(7, -1)
    got = ops.image_to_u8(img.to(DEV)).cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 128, 512, 3)
    idx = torch.from_numpy(np.arange(65536, dtype=np.int64)).reshape(1, 1, 128, 512).expand(2, 3, 128, 512).clone()
    idx[1] = idx[1].flip(-1)
    idx[:, 1] = idx[:, 1].roll(7, -1)
    assert np.array_equal(got.numpy(), want[idx.permute(0, 2, 3, 1).numpy()])
    assert np.array_equal(want, IO.to_u8_bf16(pat))
    f = IO.f32_samples()
    f = np.concatenate([f, np.zeros((-len(f)) % 96, np.float32), np.array([np.nan] * 96, np.float32)])
    t = torch.from_numpy(f).reshape(1, 3, -1, 32)
    wantf = t.clone().mul_(255).add_(0.5).clamp_(0, 255)
    wantf = torch.where(torch.isnan(wantf), torch.zeros_like(wantf), wantf).to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(ops.image_to_u8(t.to(DEV)).cpu(), wantf)
    assert ops.image_to_u8(torch.tensor([float("inf"), float("-inf"), float("nan")], device=DEV).reshape(1, 3, 1, 1)).cpu().reshape(-1).tolist() == [255, 0, 0]


def test_to_uint8_of_a_decode_is_what_save_image_writes(pipe, tmp_path):
    from PIL import Image
    ids = synth.synthetic_token_ids(3, 512)
    rec = pipe.decoding(ids, device=DEV, noise=synth.synthetic_noise(3))
    u8 = pipe.to_uint8(rec)
    assert u8.is_cuda and u8.dtype == torch.uint8 and tuple(u8.shape) == (3, 256, 256, 3)
    paths = [str(tmp_path / f"new{i}.png") for i in range(3)]
    preprocess.save_images(rec, paths)
    for i in range(3):
        preprocess.save_image(rec[i], str(tmp_path / f"old{i}.png"))
        old = np.asarray(Image.open(tmp_path / f"old{i}.png"))
        assert np.array_equal(old, u8[i].cpu().numpy()) and np.array_equal(old, np.asarray(Image.open(paths[i])))
    assert len(np.unique(u8.cpu().numpy())) > 16


def test_refusals():
    a = IO.image(IO.BY_NAME["g300x300"])
    buf, table = pack([a])
    err = _lib.SelftokHipError
    with pytest.raises(err, match="device tensors"):
        ops.image_resize_crop_norm(buf.cpu(), table, 256)
    with pytest.raises(err, match="uint8"):
        ops.image_resize_crop_norm(buf.float(), table, 256)
    with pytest.raises(err, match="1-D"):
        ops.image_resize_crop_norm(buf.reshape(300, 900), table, 256)
    with pytest.raises(err, match="dtype"):
        ops.image_resize_crop_norm(buf, table, 256, dtype=torch.float16)
    with pytest.raises(err, match=r"\[B, 3\]"):
        ops.image_resize_crop_norm(buf, table.reshape(-1), 256)
    for S in (0, -3, 4097):
        with pytest.raises(err, match="1 <= S <= 4096"):
            ops.image_resize_crop_norm(buf, table, S)
    for bad, word in (([0, 0, 300], "zero side"), ([0, 300, 0], "zero side"), ([1, 300, 300], "past the packed buffer"), ([-1, 300, 300], "past the packed buffer"),
                      ([0, 300, 301], "past the packed buffer"), ([0, 70000, 1], "limits")):
        with pytest.raises(err, match=word):
            ops.image_resize_crop_norm(buf, np.array([bad], dtype=np.int64), 256)
    with pytest.raises(err, match="out"):
        ops.image_resize_crop_norm(buf, table, 256, out=torch.empty(1, 3, 256, 255, dtype=torch.bfloat16, device=DEV))
    with pytest.raises(err, match="device tensors"):
        ops.image_to_u8(torch.zeros(1, 3, 4, 4))
    with pytest.raises(err, match="dtype"):
        ops.image_to_u8(torch.zeros(1, 3, 4, 4, dtype=torch.float16, device=DEV))
    with pytest.raises(err, match=r"\[B, 3, H, W\]"):
        ops.image_to_u8(torch.zeros(3, 4, 4, device=DEV))
    if torch.cuda.device_count() > 1:
        with pytest.raises(err, match="current device"):
            ops.image_resize_crop_norm(buf.to("cuda:1"), table, 256)
    with pytest.raises(ValueError):
        preprocess.DeviceLoader(256, "cpu")
    with pytest.raises(ValueError, match="uint8"):
        preprocess.DeviceLoader(256, DEV).load([np.zeros((4, 4, 3), np.float32)])
    assert preprocess.DeviceLoader(256, DEV, workers=1000).workers == 16


def test_double_buffered_loader_equals_the_synchronous_route(tmp_path):
    from PIL import Image
    arrays = synth.synthetic_u8_images(22, first_index=40)
    items = list(arrays)
    for i in (1, 8, 15):                                                                     # paths and arrays mixed: files are decoded on the pool
        p = str(tmp_path / f"{i}.png")
        Image.fromarray(arrays[i]).save(p)
        items[i] = p
    for dtype in (torch.float32, torch.bfloat16):
        loader = preprocess.DeviceLoader(256, DEV, dtype=dtype, workers=4)
        got = list(loader.batches(items, 8))                                                 # 8 + 8 + 6: three consecutive batches, two slots
        assert [g.shape[0] for g in got] == [8, 8, 6]
        sync = preprocess.DeviceLoader(256, DEV, dtype=dtype, workers=1)
        for j, g in enumerate(got):
            want = torch.stack([host_chain(a, 256) for a in arrays[8 * j:8 * j + 8]]).to(dtype)
            assert np.array_equal(bits(g), bits(want)) and np.array_equal(bits(sync.load(arrays[8 * j:8 * j + 8])), bits(want))
        again = list(loader.batches(items, 8))                                               # the staging slots are reused
        assert all(torch.equal(x, y) for x, y in zip(got, again))
        loader.close(); sync.close()
