"""not gpu: csrc/image_views.hip itself, compiled for the HOST (tests/host_standin/common.h turns a launch into loops over the grid) and run on
every case of tests/image_views_cases.py, each alone and all in one reversed batch, in bf16 and fp32: the kernels' own source gives the
emulation's bytes.  What only the GPU can show (the device compiler's fp64 code, memory ordering) is left to tests/test_image_views_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_io_cases as IO
import image_views_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("standin_views")
    shutil.copy(os.path.join(ROOT, "tests", "host_standin", "common.h"), d / "common.h")
    shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "image_views.hip"), d / "image_views.inc")
    (d / "selftok_hip_ext.h").write_text("#pragma once\n")
    (d / "unit.cpp").write_text('#include "common.h"\nextern "C" {\n'
                                "size_t selftok_img_views_u8_workspace_bytes(const long*, int, int);\n"
                                "int selftok_img_views_tables_layout(const long*, int, int, long*);\n"
                                "int selftok_img_views_u8(const unsigned char*, size_t, const long*, const long*, int, int, void*, int, const void*, void*, size_t, hipStream_t);\n}\n"
                                '#include "image_views.inc"\n')
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I", str(d), str(d / "unit.cpp"), "-o", str(d / "libstandin.so")])
    lib = C.CDLL(str(d / "libstandin.so"))
    lib.selftok_img_views_u8_workspace_bytes.restype = C.c_size_t
    lib.selftok_img_views_u8_workspace_bytes.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.selftok_img_views_u8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.selftok_last_error.restype = C.c_char_p
    return lib


def pack(cases):
    """every distinct source once -> (uint8 buffer, int64 [V, 12] descriptor rows)"""
    at, chunks, where = 0, [], {}
    for c in cases:
        if (c.w, c.h, c.content) not in where:
            where[(c.w, c.h, c.content)] = at
            chunks.append(VC.image(c).reshape(-1))
            at += chunks[-1].size + 5                                         # odd offsets
            chunks.append(np.full(5, 0xA5, np.uint8))
    rows = np.array([[where[(c.w, c.h, c.content)], c.w, c.h] + list(c.view[:9]) for c in cases], dtype=np.int64)
    return np.concatenate(chunks), rows


def run(lib, cases, S, bf16):
    buf, rows = pack(cases)
    V = len(cases)
    n = lib.selftok_img_views_u8_workspace_bytes(rows.ctypes.data, V, S)
    assert n, lib.selftok_last_error()
    ws = np.zeros(n, np.uint8)
    out = np.full((V, 3, S, S), 7, np.uint16 if bf16 else np.float32)
    lut = IO.bf16_bits(IO.normalize_lut()) if bf16 else IO.normalize_lut()
    rc = lib.selftok_img_views_u8(buf.ctypes.data, buf.size, rows.ctypes.data, rows.ctypes.data, V, S, out.ctypes.data, int(bf16), lut.ctypes.data, ws.ctypes.data, n, None)
    assert rc == 0, lib.selftok_last_error()
    return out


def same(out, want, bf16):
    return np.array_equal(out, want) if bf16 else np.array_equal(out.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("S", sorted({c.view.size for c in VC.CASES}))
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_kernel_source_on_the_host_equals_the_emulation(lib, S, bf16):
    cases = [c for c in VC.CASES if c.view.size == S]
    for c in cases:                                                           # every view alone ...
        assert same(run(lib, [c], S, bf16)[0], VC.to_tensor(VC.expected(c), bf16), bf16), c.name
    mixed = [c for c in VC.MIXED if c.view.size == S]                         # ... and the mixed batch of this size, reversed, sources shared
    out = run(lib, mixed, S, bf16)
    for v, c in enumerate(mixed):
        assert same(out[v], VC.to_tensor(VC.expected(c), bf16), bf16), c.name
