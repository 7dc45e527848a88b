"""not gpu: csrc/image_views.hip itself, compiled for the HOST (tests/host_standin/common.h turns a launch into loops over the grid) and run on
every case of tests/image_views_cases.py, each alone and all in one reversed batch, in bf16 and fp32: the kernels' own source gives the
emulation's bytes.  csrc/image_io.hip, built the same way, gives the views entry's bits and tap rows on its own mixed batch.  What only the GPU can show (the device compiler's fp64 code, memory ordering) is left to tests/test_image_views_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_io_cases as IO
import image_views_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = ("selftok_img_views_u8_workspace_bytes", "selftok_img_views_tables_layout", "selftok_img_views_u8")
CENTER = ("selftok_img_resize_crop_norm_u8_workspace_bytes", "selftok_img_resize_tables_layout", "selftok_img_resize_crop_norm_u8")


def standin(d, unit, names, extra=""):
    """csrc/<unit>.hip and the shared headers it includes, copied beside the stand-in common.h and built for the host -> the ctypes library"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    query, layout, entry = names
    shutil.copy(os.path.join(ROOT, "tests", "host_standin", "common.h"), d / "common.h")
    shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", unit + ".hip"), d / (unit + ".inc"))
    for h in ("image_resample_shared.h", "u8_shared.h"):
        shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", h), d / h)
    (d / "selftok_hip_ext.h").write_text("#pragma once\n")
    (d / "unit.cpp").write_text('#include "common.h"\nextern "C" {\n'
                                f"size_t {query}(const long*, int, int);\n"
                                f"int {layout}(const long*, int, int, long*);\n"
                                f"int {entry}(const unsigned char*, size_t, const long*, const long*, int, int, void*, int, const void*, void*, size_t, hipStream_t);\n{extra}}}\n"
                                f'#include "{unit}.inc"\n')
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I", str(d), str(d / "unit.cpp"), "-o", str(d / "libstandin.so")])
    lib = C.CDLL(str(d / "libstandin.so"))
    getattr(lib, query).restype = C.c_size_t
    getattr(lib, query).argtypes = [C.c_void_p, C.c_int, C.c_int]
    getattr(lib, layout).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    getattr(lib, entry).argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lib.selftok_last_error.restype = C.c_char_p
    return lib


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    return standin(tmp_path_factory.mktemp("standin_views"), "image_views", VIEWS)


@pytest.fixture(scope="module")
def lib_center(tmp_path_factory):
    return standin(tmp_path_factory.mktemp("standin_center"), "image_io", CENTER, extra="int selftok_img_to_u8(const void*, int, unsigned char*, int, int, int, hipStream_t);\n")


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


def call(lib, names, buf, rows, S, bf16):
    """one entry on one host table -> (output, {'h' | 'v': its [N, S, ks] tap rows, read out of the workspace through the entry's own layout call})"""
    N = len(rows)
    query, layout, entry = (getattr(lib, n) for n in names)
    n = query(rows.ctypes.data, N, S)
    assert n, lib.selftok_last_error()
    ws = np.zeros(n, np.uint8)
    out = np.full((N, 3, S, S), 7, np.uint16 if bf16 else np.float32)
    lut = IO.bf16_bits(IO.normalize_lut()) if bf16 else IO.normalize_lut()
    assert entry(buf.ctypes.data, buf.size, rows.ctypes.data, rows.ctypes.data, N, S, out.ctypes.data, int(bf16), lut.ctypes.data, ws.ctypes.data, n, None) == 0, lib.selftok_last_error()
    lay = np.zeros(4, np.int64)
    assert layout(rows.ctypes.data, N, S, lay.ctypes.data) == 0, lib.selftok_last_error()
    wi = ws[:n // 4 * 4].view(np.int32)
    return out, {"h": wi[lay[0]:lay[0] + N * S * lay[1]].reshape(N, S, lay[1]), "v": wi[lay[2]:lay[2] + N * S * lay[3]].reshape(N, S, lay[3])}


def run(lib, cases, S, bf16):
    buf, rows = pack(cases)
    return call(lib, VIEWS, buf, rows, S, bf16)[0]


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_centre_entry_equals_the_views_entry_on_view_center_rows(lib, lib_center, bf16):
    """the [B, 3] rows of the centre-crop entry and the `preprocess.view_center` rows of the same sources through the views entry: the same
    output bits and the same tap rows, on every IO.MIXED case the host loop can afford"""
    from selftoktokenizer_amd import preprocess as P
    cases = [c for c in IO.MIXED if c.w * c.h <= 1 << 22]
    assert len(cases) >= 10
    for S in sorted({c.S for c in cases}):
        cs = [c for c in cases if c.S == S]
        arrays = [IO.image(c) for c in cs]
        table = np.zeros((len(cs), 3), np.int64)
        at = 0
        for i, a in enumerate(arrays):
            table[i] = (at, a.shape[1], a.shape[0])
            at += a.size
        buf = np.concatenate([a.reshape(-1) for a in arrays])
        views = P.view_rows([[P.view_center(c.w, c.h, S)] for c in cs], S)
        rows = np.ascontiguousarray(np.concatenate([table[views[:, 0]], views[:, 1:]], axis=1))
        old, old_taps = call(lib_center, CENTER, buf, table, S, bf16)
        new, new_taps = call(lib, VIEWS, buf, rows, S, bf16)
        assert old.dtype == new.dtype and np.array_equal(old.view(np.uint8), new.view(np.uint8))
        assert not (old == 7).all(axis=(1, 2, 3)).any()                       # every image was written
        for axis in "hv":
            assert old_taps[axis].shape == new_taps[axis].shape and np.array_equal(old_taps[axis], new_taps[axis]), axis


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
