"""not gpu: csrc/image_io.hip itself, compiled for the HOST (tests/host_standin/common.h turns a launch into loops over the grid) and
run on every case of tests/image_io_cases.py: the kernels' own source gives the golden checksums (bf16 and fp32 output, mixed batch in
reversed pixel order) and torch's bytes on every bf16 pattern.  It shows that the C++ text computes the arithmetic of record; what only
the GPU can show (the device compiler's fp64 code, memory ordering) is left to tests/test_image_io_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_io_cases as IO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("standin")
    shutil.copy(os.path.join(ROOT, "tests", "host_standin", "common.h"), d / "common.h")
    shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "image_io.hip"), d / "image_io.inc")
    for h in ("image_resample_shared.h", "u8_shared.h"):                    # the headers the file includes, beside it
        shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", h), d / h)
    (d / "selftok_hip_ext.h").write_text("#pragma once\n")
    (d / "unit.cpp").write_text('#include "common.h"\nextern "C" {\n'
                                "size_t selftok_img_resize_crop_norm_u8_workspace_bytes(const long*, int, int);\n"
                                "int selftok_img_resize_tables_layout(const long*, int, int, long*);\n"
                                "int selftok_img_resize_crop_norm_u8(const unsigned char*, size_t, const long*, const long*, int, int, void*, int, const void*, void*, size_t, hipStream_t);\n"
                                "int selftok_img_to_u8(const void*, int, unsigned char*, int, int, int, hipStream_t);\n}\n"
                                '#include "image_io.inc"\n')
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I", str(d), str(d / "unit.cpp"), "-o", str(d / "libstandin.so")])
    lib = C.CDLL(str(d / "libstandin.so"))
    lib.selftok_img_resize_crop_norm_u8_workspace_bytes.restype = C.c_size_t
    lib.selftok_img_resize_crop_norm_u8_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.selftok_img_resize_crop_norm_u8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.selftok_img_to_u8.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.selftok_last_error.restype = C.c_char_p
    return lib


def run(lib, arrays, S, bf16, order=None):
    order = list(range(len(arrays))) if order is None else order
    table = np.zeros((len(arrays), 3), np.int64)
    chunks, at = [], 0
    for i in order:
        table[i] = (at, arrays[i].shape[1], arrays[i].shape[0])
        chunks.append(arrays[i].reshape(-1))
        at += arrays[i].size
    buf = np.concatenate(chunks)
    n = lib.selftok_img_resize_crop_norm_u8_workspace_bytes(table.ctypes.data, len(arrays), S)
    assert n, lib.selftok_last_error()
    ws = np.zeros(n, np.uint8)
    out = np.full((len(arrays), 3, S, S), 7, np.uint16 if bf16 else np.float32)
    lut = IO.bf16_bits(IO.normalize_lut()) if bf16 else IO.normalize_lut()
    rc = lib.selftok_img_resize_crop_norm_u8(buf.ctypes.data, buf.size, table.ctypes.data, table.ctypes.data, len(arrays), S, out.ctypes.data, int(bf16), lut.ctypes.data,
                                             ws.ctypes.data, n, None)
    assert rc == 0, lib.selftok_last_error()
    return out


SMALL = [c for c in IO.CASES if c.w * c.h <= 1 << 22]       # one thread after the other: the three multi-megapixel cases are left to the GPU


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_kernel_source_on_the_host_gives_the_golden_checksums(lib, case):
    g = np.load(IO.GOLDEN)
    i = list(g["names"]).index(case.name)
    a = IO.image(case)
    assert IO.crc(run(lib, [a], case.S, True)[0]) == int(g["crc_bf16"][i])
    lut = IO.normalize_lut()
    o32 = run(lib, [a], case.S, False)[0]
    u8 = np.searchsorted(lut, o32).astype(np.uint8)
    assert np.array_equal(lut[u8].view(np.uint32), o32.view(np.uint32)) and IO.crc(u8.transpose(1, 2, 0)) == int(g["crc_u8"][i])


def test_mixed_batch_in_reversed_pixel_order(lib):
    g = np.load(IO.GOLDEN)
    cs = [c for c in SMALL if c.S == 256]
    out = run(lib, [IO.image(c) for c in cs], 256, True, order=list(range(len(cs)))[::-1])
    assert [IO.crc(out[b]) for b in range(len(cs))] == [int(g["crc_bf16"][list(g["names"]).index(c.name)]) for c in cs]


def test_to_u8_source_on_the_host(lib):
    import torch
    pat = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    img = np.stack([pat.reshape(128, 512), pat[::-1].reshape(128, 512), np.roll(pat, 7).reshape(128, 512)])[None].copy()
    out = np.zeros((1, 128, 512, 3), np.uint8)
    assert lib.selftok_img_to_u8(img.ctypes.data, 1, out.ctypes.data, 1, 128, 512, None) == 0
    x = torch.from_numpy(pat.view(np.int16).copy()).view(torch.bfloat16)
    ok = ~torch.isnan(x)
    want = np.zeros(65536, np.uint8)
    want[ok.numpy()] = x.clone().mul_(255).add_(0.5).clamp_(0, 255)[ok].to(torch.uint8).numpy()
    assert np.array_equal(out[0, :, :, 0].reshape(-1), want) and np.array_equal(out[0, :, :, 1].reshape(-1), want[::-1])
    assert np.array_equal(out[0, :, :, 2].reshape(-1), np.roll(want, 7))
    f = IO.f32_samples()
    f = np.concatenate([f, np.zeros((-len(f)) % 3, np.float32)])
    img = f.reshape(1, 3, 1, -1).copy()
    out = np.zeros((1, 1, img.shape[3], 3), np.uint8)
    assert lib.selftok_img_to_u8(img.ctypes.data, 0, out.ctypes.data, 1, 1, img.shape[3], None) == 0
    assert np.array_equal(out[0, 0].T.reshape(-1), IO.to_u8_f32(f))
