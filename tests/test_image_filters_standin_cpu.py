"""not gpu: csrc/image_filters.hip itself, compiled for the HOST through tests/host_standin/common.h as it is (a launch becomes loops over the
grid) and run on every case of tests/image_filters_cases.py: the views entry with BICUBIC and BOX, the whole-frame resize with the three filters,
and the ADM chain (one resize call per depth, then the BICUBIC views call), each case alone and all of a size in one reversed batch, bf16 and
fp32.  The kernels' own source gives the emulation's bytes; what only the GPU can show is left to tests/test_image_filters_gpu.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import image_io_cases as IO
import image_filters_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECLS = """
size_t selftok_img_views_filter_u8_workspace_bytes(const long*, int, int, int);
int selftok_img_views_filter_tables_layout(const long*, int, int, int, long*);
int selftok_img_views_filter_u8(const unsigned char*, size_t, const long*, const long*, int, int, int, void*, int, const void*, void*, size_t, hipStream_t);
size_t selftok_img_resize_u8_workspace_bytes(const long*, int, int);
int selftok_img_resize_u8(unsigned char*, size_t, const long*, const long*, int, int, void*, size_t, hipStream_t);
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("standin_filters")
    shutil.copy(os.path.join(ROOT, "tests", "host_standin", "common.h"), d / "common.h")
    shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "image_filters.hip"), d / "image_filters.inc")
    shutil.copy(os.path.join(ROOT, "selftoktokenizer_amd", "csrc", "image_resample_shared.h"), d / "image_resample_shared.h")
    (d / "selftok_hip_ext.h").write_text("#pragma once\n")
    (d / "unit.cpp").write_text('#include "common.h"\nextern "C" {' + DECLS + '}\n#include "image_filters.inc"\n')
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-I", str(d), str(d / "unit.cpp"), "-o", str(d / "libstandin.so")])
    lib = C.CDLL(str(d / "libstandin.so"))
    vp, i, sz = C.c_void_p, C.c_int, C.c_size_t
    lib.selftok_img_views_filter_u8_workspace_bytes.restype, lib.selftok_img_views_filter_u8_workspace_bytes.argtypes = sz, [vp, i, i, i]
    lib.selftok_img_views_filter_tables_layout.argtypes = [vp, i, i, i, vp]
    lib.selftok_img_views_filter_u8.argtypes = [vp, sz, vp, vp, i, i, i, vp, i, vp, vp, sz, vp]
    lib.selftok_img_resize_u8_workspace_bytes.restype, lib.selftok_img_resize_u8_workspace_bytes.argtypes = sz, [vp, i, i]
    lib.selftok_img_resize_u8.argtypes = [vp, sz, vp, vp, i, i, vp, sz, vp]
    lib.selftok_last_error.restype = C.c_char_p
    return lib


def views(lib, buf, rows, S, filt, bf16):
    """the views entry on one host table -> (output, {'h' | 'v': [V, S, ks] tap rows out of the workspace})"""
    V = len(rows)
    n = lib.selftok_img_views_filter_u8_workspace_bytes(rows.ctypes.data, V, S, filt)
    assert n, lib.selftok_last_error()
    ws = np.zeros(n, np.uint8)
    out = np.full((V, 3, S, S), 7, np.uint16 if bf16 else np.float32)
    lut = IO.bf16_bits(IO.normalize_lut()) if bf16 else IO.normalize_lut()
    rc = lib.selftok_img_views_filter_u8(buf.ctypes.data, buf.size, rows.ctypes.data, rows.ctypes.data, V, S, filt, out.ctypes.data, int(bf16), lut.ctypes.data, ws.ctypes.data, n, None)
    assert rc == 0, lib.selftok_last_error()
    lay = np.zeros(4, np.int64)
    assert lib.selftok_img_views_filter_tables_layout(rows.ctypes.data, V, S, filt, lay.ctypes.data) == 0, lib.selftok_last_error()
    wi = ws[:n // 4 * 4].view(np.int32)
    return out, {"h": wi[lay[0]:lay[0] + V * S * lay[1]].reshape(V, S, lay[1]), "v": wi[lay[2]:lay[2] + V * S * lay[3]].reshape(V, S, lay[3])}


def resize(lib, buf, frames, filt):
    N = len(frames)
    n = lib.selftok_img_resize_u8_workspace_bytes(frames.ctypes.data, N, filt)
    assert n, lib.selftok_last_error()
    ws = np.zeros(n, np.uint8)
    assert lib.selftok_img_resize_u8(buf.ctypes.data, buf.size, frames.ctypes.data, frames.ctypes.data, N, filt, ws.ctypes.data, n, None) == 0, lib.selftok_last_error()


def same(out, want, bf16):
    return np.array_equal(out, want) if bf16 else np.array_equal(out.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("filt", [FC.BICUBIC, FC.BOX], ids=["bicubic", "box"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_views_entry_on_the_host_equals_the_emulation(lib, filt, bf16):
    for S in sorted({c.view.size for c in FC.VIEW_CASES}):
        cases = [c for c in FC.VIEW_CASES if c.filter == filt and c.view.size == S]
        assert len(cases) >= 8
        for c in cases:                                                       # every view alone, its tap rows too ...
            out, taps = views(lib, *FC.pack_views([c]), S, filt, bf16)
            assert same(out[0], IO.to_tensor(FC.expected(c), bf16), bf16), c.name
            v = c.view
            for axis, (insz, outsz, first) in (("h", (v.bw, v.rw, v.left)), ("v", (v.bh, v.rh, v.top))):
                xmin, n, k = FC.tables(insz, outsz, first, S, filt)
                assert taps[axis].shape[2] == 2 + FC.ksize(insz, outsz, filt), (c.name, axis)
                assert np.array_equal(taps[axis][0, :, 0], xmin) and np.array_equal(taps[axis][0, :, 1], n), (c.name, axis)
                for i in range(S):
                    assert np.array_equal(taps[axis][0, i, 2:2 + n[i]], k[i, :n[i]]), (c.name, axis, i)
        mixed = cases[::-1]                                                   # ... and the batch of this size, reversed, sources shared
        out, _ = views(lib, *FC.pack_views(mixed), S, filt, bf16)
        for i, c in enumerate(mixed):
            assert same(out[i], IO.to_tensor(FC.expected(c), bf16), bf16), c.name


def test_bilinear_through_the_filter_entry_is_the_bilinear_arithmetic(lib):
    """filter = 2: the emulation of the existing entry, image_views_cases' group of resized crops"""
    import image_views_cases as VC
    cases = [c for c in VC.GROUP_B if c.view.size == 16][::-1]
    at, chunks, where = 0, [], {}
    for c in cases:
        if (c.w, c.h) not in where:
            where[(c.w, c.h)] = at
            chunks.append(VC.image(c).reshape(-1))
            at += chunks[-1].size
    rows = np.array([[where[(c.w, c.h)], c.w, c.h] + list(c.view[:9]) for c in cases], dtype=np.int64)
    out, _ = views(lib, np.concatenate(chunks), rows, 16, FC.BILINEAR, True)
    for i, c in enumerate(cases):
        assert same(out[i], VC.to_tensor(VC.expected(c), True), True), c.name


@pytest.mark.parametrize("filt", [FC.BOX, FC.BILINEAR, FC.BICUBIC], ids=["box", "bilinear", "bicubic"])
def test_resize_entry_on_the_host_equals_the_emulation(lib, filt):
    cases = [c for c in FC.RESIZE_CASES if c.filter == filt]
    for batch in [[c] for c in cases] + [cases[::-1]]:
        buf, frames = FC.pack_resize(batch)
        before = buf.copy()
        resize(lib, buf, frames, filt)
        regions = []
        for c, r in zip(batch, frames):
            got = buf[r[3]:r[3] + c.ow * c.oh * 3].reshape(c.oh, c.ow, 3)
            assert np.array_equal(got, FC.expected(c)), c.name
            regions.append((int(r[3]), c.ow * c.oh * 3))
        for off, n in regions:
            before[off:off + n] = buf[off:off + n]
        assert np.array_equal(before, buf)                                     # nothing but the destinations was written


@pytest.mark.parametrize("S", [16, 24])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_adm_chain_on_the_host_equals_the_emulation(lib, S, bf16):
    cases = [c for c in FC.ADM_CASES if c.S == S]
    assert {len(FC.adm_numbers(c.w, c.h, S)[0]) - 1 for c in cases} >= ({0, 1, 2, 3, 4} if S == 16 else {0, 1, 2})
    for batch in [[c] for c in cases] + [cases[::-1]]:
        buf, depth, rows = FC.pack_adm(batch)
        for frames in depth:
            resize(lib, buf, frames, FC.BOX)
        out, _ = views(lib, buf, rows, S, FC.BICUBIC, bf16)
        for i, c in enumerate(batch):
            assert same(out[i], IO.to_tensor(FC.expected(c), bf16), bf16), c.name
