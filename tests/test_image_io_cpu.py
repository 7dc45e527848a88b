"""not gpu: the arithmetic of record of the device image I/O (csrc/image_io.hip) pinned on the host -- the numpy emulation of
tests/image_io_cases.py against Pillow, against the golden file, through the whole `load_image` chain; save_image's uint8 conversion
on every bf16 pattern; the extension header against the ctypes table; the kernels' register budget; and the planted mistakes every
case must be able to see."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import image_io_cases as IO
from selftoktokenizer_amd import _lib, preprocess
from selftoktokenizer_amd.pipeline import NormalizeToTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_img_resize_crop_norm_u8_workspace_bytes", "selftok_img_resize_tables_layout", "selftok_img_resize_crop_norm_u8", "selftok_img_to_u8"}

_cache = {}


def emulated(case):
    if case.name not in _cache:
        _cache[case.name] = IO.resize_crop(IO.image(case), case.S)
    return _cache[case.name]


@pytest.fixture(scope="module")
def golden():
    return np.load(IO.GOLDEN)


def test_case_table_covers_what_it_claims():
    geoms = {(c.w, c.h) for c in IO.CASES if c.S == 256}
    assert geoms >= {(500, 375), (375, 500), (257, 256), (256, 999), (1024, 768), (300, 300), (255, 255), (100, 180), (640, 427), (3000, 2000), (256, 256),
                     (511, 513), (77, 1031)}
    assert {c.S for c in IO.CASES} >= {128, 256, 320}
    assert {c.content for c in IO.CASES} >= {"noise", "ramp", "stripes1", "stripes2", "stripes3"}
    halves = {(o * 2 < s - 256) for c in IO.CASES if c.S == 256 for s in IO.target_size(c.w, c.h, 256) if (s - 256) % 2 for o in [IO.crop_offset(s, 256)]}
    assert halves == {True, False}                                          # x.5 -> the even integer below AND above
    assert IO.crop_offset(256 + 85, 256) == 42 and IO.crop_offset(256 + 87, 256) == 44
    assert any(IO.target_size(c.w, c.h, c.S) == (c.w, c.h) and max(c.w, c.h) > c.S for c in IO.CASES)      # a side is S already, the other longer
    assert any(c.w == 1 for c in IO.CASES) and any(c.h == 1 for c in IO.CASES) and any(max(c.w, c.h) >= 6000 for c in IO.CASES)
    assert max(IO.tables(6000, 256, 0, 256)[1]) >= 47                       # the many-tap route
    assert len(IO.MIXED) >= 20


@pytest.mark.parametrize("case", IO.CASES, ids=lambda c: c.name)
def test_emulation_equals_pillow_and_golden(case, golden):
    got = emulated(case)
    i = list(golden["names"]).index(case.name)
    assert IO.crc(got) == int(golden["crc_u8"][i]), "uint8 crop differs from the recorded one"
    assert IO.crc(IO.to_tensor(got, True)) == int(golden["crc_bf16"][i]), "bf16 tensor differs from the recorded one"
    from PIL import Image
    ref = np.asarray(preprocess.center_crop(preprocess.resize_shorter_side(Image.fromarray(IO.image(case)), case.S), case.S))
    assert ref.shape == got.shape and int((ref != got).sum()) == 0, f"{int((ref != got).sum())} bytes differ from Pillow"


def test_golden_coefficient_tables(golden):
    assert len(golden["names"]) == len(IO.CASES) and list(golden["names"]) == [c.name for c in IO.CASES]
    for insz, outsz in IO.TABLE_GEOMS:
        xmin, n, k = IO.tables(insz, outsz, 0, outsz)
        assert np.array_equal(xmin, golden[f"tab_{insz}_{outsz}_xmin"]) and np.array_equal(n, golden[f"tab_{insz}_{outsz}_n"])
        assert np.array_equal(k, golden[f"tab_{insz}_{outsz}_k"])
        assert abs(int(k.sum(axis=1).min()) - (1 << IO.PB)) <= k.shape[1] and (k >= 0).all()             # the negative-weight branch never fires
    assert os.path.getsize(IO.GOLDEN) < 256 * 1024


@pytest.mark.parametrize("case", IO.CASES, ids=lambda c: c.name)
def test_full_host_chain_bit_for_bit(case):
    """emulation -> 256-entry table == NormalizeToTensor()(center_crop(resize_shorter_side(...))): fp32, and after .to(bf16)"""
    from PIL import Image
    want = NormalizeToTensor()(preprocess.center_crop(preprocess.resize_shorter_side(Image.fromarray(IO.image(case)), case.S), case.S))
    got = IO.to_tensor(emulated(case), False)
    assert want.dtype == torch.float32 and tuple(want.shape) == (3, case.S, case.S)
    assert np.array_equal(got.view(np.uint32), want.numpy().view(np.uint32))
    assert np.array_equal(IO.to_tensor(emulated(case), True), want.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_lut_is_the_normalize_expression():
    lut = IO.normalize_lut()
    v = np.arange(256, dtype=np.float32)
    assert np.array_equal(lut.view(np.uint32), (v / 127.5 - 1.0).astype(np.float32).view(np.uint32)) and lut[0] == -1.0 and lut[255] == 1.0
    assert np.array_equal(IO.bf16_bits(lut), torch.from_numpy(lut).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16))


def test_to_u8_emulation_on_every_bf16_pattern():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x = torch.from_numpy(bits.view(np.int16)).view(torch.bfloat16)
    ok = ~torch.isnan(x).numpy()
    want = x.clone().mul_(255).add_(0.5).clamp_(0, 255)[torch.from_numpy(ok)].to(torch.uint8).numpy()
    got = IO.to_u8_bf16(bits)
    assert int(ok.sum()) == 65536 - 2 * 127 and np.array_equal(got[ok], want)
    assert (got[~ok] == 0).all()                                            # NaN -> 0: this project's choice
    inf = np.array([0x7F80, 0xFF80], np.uint16)
    assert IO.to_u8_bf16(inf).tolist() == [255, 0]
    f = IO.f32_samples()
    ok = ~np.isnan(f)
    want = torch.from_numpy(f[ok]).clone().mul_(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()
    assert np.array_equal(IO.to_u8_f32(f)[ok], want) and len(set(want.tolist())) == 256


def test_ext_header_declares_the_image_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and names == set(_lib.EXT_SIGNATURES) and not (names & set(_lib.SIGNATURES))
    assert not any(n in open(os.path.join(ROOT, "include", "selftok_hip.h")).read() for n in NEW_ENTRIES)
    C = ctypes
    ctype_of = {"int": C.c_int, "long": C.c_long, "size_t": C.c_size_t, "hipStream_t": C.c_void_p}
    for n in NEW_ENTRIES:
        m = re.search(r"(\w+)\s+" + n + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m, n
        args = [a.strip() for a in m.group(2).split(",")]
        want = [C.c_void_p if "*" in a else ctype_of[a.split()[-2] if len(a.split()) > 1 else a] for a in args]
        res, got = _lib.EXT_SIGNATURES[n]
        assert got == want, (n, args)
        assert res == ctype_of[m.group(1)]
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NEW_ENTRIES:
        assert hasattr(lib, n), f"{n} declared in selftok_hip_ext.h but not exported"


def test_host_planner_refuses_and_sizes_without_a_gpu():
    """the workspace query and the layout call are host code: they validate the table and need no device"""
    lib = _lib.load()
    t = np.array([[0, 500, 375], [562500, 1, 5]], dtype=np.int64)
    n = lib.selftok_img_resize_crop_norm_u8_workspace_bytes(t.ctypes.data, 2, 256)
    lay = np.zeros(4, dtype=np.int64)
    assert lib.selftok_img_resize_tables_layout(t.ctypes.data, 2, 256, lay.ctypes.data) == 0
    assert lay[0] == 2 * 20 and lay[1] == 2 + 5 and lay[3] == 2 + 5 and n > 4 * (lay[2] + 2 * 256 * lay[3]) + 256 * 256 * 3
    for bad, word in (([[0, 0, 375]], "zero side"), ([[0, 10, 0]], "zero side"), ([[0, 70000, 10]], "limits"), ([[-1, 10, 10]], "past")):
        t = np.array(bad, dtype=np.int64)
        assert lib.selftok_img_resize_crop_norm_u8_workspace_bytes(t.ctypes.data, 1, 256) == 0
        assert word in lib.selftok_last_error().decode()
    t = np.array([[0, 10, 10]], dtype=np.int64)
    for S in (0, -1, 4097):
        assert lib.selftok_img_resize_crop_norm_u8_workspace_bytes(t.ctypes.data, 1, S) == 0 and "S" in lib.selftok_last_error().decode()


def test_image_io_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "image_io.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) >= 6 and len(scratch) == len(kernels), (kernels, scratch)
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    src = open(os.path.join(G.CSRC, "image_io.hip")).read() + open(os.path.join(G.CSRC, "image_resample_shared.h")).read()
    assert "asm" not in src.replace("namespace", "")                        # plain C++: no inline assembly in this unit or in the resample it includes


MUTS = {"xmin_off_by_one": IO.MUT_XMIN, "truncate_before_shift": IO.MUT_TRUNC, "no_u8_between_passes": IO.MUT_NO_U8, "crop_round_half_up": IO.MUT_HALF_UP}


@pytest.mark.parametrize("mut", list(MUTS), ids=list(MUTS))
def test_every_case_sees_the_planted_mistake(mut):
    """each mistake changes at least one output byte in EVERY case whose arithmetic it touches, the 49-tap case included"""
    seen = 0
    for case in IO.CASES:
        if not IO.applies(case, MUTS[mut]):
            continue
        d = int((IO.resize_crop(IO.image(case), case.S, MUTS[mut]) != emulated(case)).sum())
        assert d >= 1, f"{case.name}: {mut} changes no byte"
        seen += 1
    assert seen >= {"crop_round_half_up": 5}.get(mut, 10), seen
