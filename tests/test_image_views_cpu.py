"""not gpu: the arithmetic of record of the device image views (csrc/image_views.hip) pinned on the host -- the numpy emulation of
tests/image_views_cases.py against live Pillow on every view, the centre view against the existing emulation and its golden file, the order
of the ten-crop, the planted mistakes every case must be able to see, the new declarations, the kernels' scratch and the host-side refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import image_io_cases as IO
import image_views_cases as VC
from selftoktokenizer_amd import _lib, ops, preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_img_views_u8_workspace_bytes", "selftok_img_views_tables_layout", "selftok_img_views_u8"}

BATCHES = {}
for _c in VC.CASES:
    BATCHES.setdefault((_c.w, _c.h, _c.R, _c.view.size), []).append(_c)


def test_case_table_covers_what_it_claims():
    a = {(c.w, c.h, c.R, c.view.size) for c in VC.GROUP_A}
    assert a == {(w, h, R, 16) for w, h in ((37, 29), (29, 37), (64, 64), (100, 180)) for R in (16, 18, 23)} | {(23, 41, 11, 8), (500, 375, 281, 256), (375, 500, 281, 256)}
    for key in a:                                                             # every window of group a both flipped and unflipped
        vs = [c.view for c in BATCHES[key]]
        assert len(vs) == 20 and {v._replace(flip=0) for v in vs if v.flip} == {v for v in vs if not v.flip}
    five = P.views_five(37, 29, 16, 16)
    assert len({(v.top) for v in five}) == 1 and five[0].rh == 16              # R = S: the windows coincide on the short axis
    assert P.views_five(37, 29, 18, 16)[4].top == 1                           # R = 18: the centre offset is 1.0
    v23 = P.views_five(37, 29, 23, 16)[4]
    assert (v23.rw - 16) % 2 == 1 and v23.left == 6                           # 6.5 -> 6: half to even decides
    b = VC.GROUP_B
    assert {c.view.size for c in b} == {8, 16, 64} and any(c.view.rw > c.view.bw for c in b) and any(c.view.rw < c.view.bw for c in b)      # up and down
    assert any(c.view.bw == 1 and c.view.x0 == c.w - 1 for c in b) and any(c.view.bw == c.w and c.view.y0 + c.view.bh == c.h and c.view.bh == 7 for c in b)
    assert any((c.view.bw, c.view.bh) == (c.w, c.h) for c in b) and any((c.w, c.view.x0, c.view.y0, c.view.bw, c.view.bh) == (500, 17, 23, 200, 150) for c in b)
    assert any(c.view.bw * c.view.rh != c.view.bh * c.view.rw for c in b)     # anisotropic
    assert VC.MIXED == VC.CASES[::-1] and len({(c.w, c.h) for c in VC.MIXED}) >= 7


@pytest.mark.parametrize("key", list(BATCHES), ids=lambda k: f"{k[0]}x{k[1]}_R{k[2]}_S{k[3]}")
def test_emulation_equals_live_pillow(key):
    for c in BATCHES[key]:
        ref = np.asarray(P.apply_view_pil(VC.image(c), c.view, to_tensor=False))
        got = VC.expected(c)
        assert ref.shape == got.shape == (c.view.size, c.view.size, 3) and int((ref != got).sum()) == 0, f"{c.name}: {int((ref != got).sum())} bytes differ from Pillow"
        t = P.apply_view_pil(VC.image(c), c.view)
        assert np.array_equal(VC.to_tensor(got, False).view(np.uint32), t.numpy().view(np.uint32)), c.name


@pytest.mark.parametrize("case", IO.CASES, ids=lambda c: c.name)
def test_view_center_is_the_existing_geometry(case):
    g = np.load(IO.GOLDEN)
    i = list(g["names"]).index(case.name)
    v = P.view_center(case.w, case.h, case.S)
    assert (v.rw, v.rh) == IO.target_size(case.w, case.h, case.S) and (v.left, v.top) == (IO.crop_offset(v.rw, case.S), IO.crop_offset(v.rh, case.S))
    got = VC.emulate(IO.image(case), v)
    assert IO.crc(got) == int(g["crc_u8"][i]) and IO.crc(IO.to_tensor(got, True)) == int(g["crc_bf16"][i])
    assert np.array_equal(got, IO.resize_crop(IO.image(case), case.S))


@pytest.mark.parametrize("w,h,R,S", [(37, 29, 18, 16), (37, 29, 23, 16), (29, 37, 23, 16), (100, 180, 23, 16), (23, 41, 11, 8), (64, 64, 16, 16), (500, 375, 281, 256)])
def test_ten_crop_order_is_torchvisions(w, h, R, S):
    """TenCrop = five crops (tl, tr, bl, br, centre), then the five crops of the MIRRORED resized image: done here with Pillow as torchvision does it"""
    a = IO.image(IO.Case("src", w, h, 0, "noise"))
    resized = P.resize_shorter_side(Image.fromarray(a), R)
    rw, rh = resized.size
    def five(im):
        at = [(0, 0), (rw - S, 0), (0, rh - S), (rw - S, rh - S)]
        return [im.crop((l, t, l + S, t + S)) for l, t in at] + [P.center_crop(im, S)]
    want = five(resized) + five(resized.transpose(Image.FLIP_LEFT_RIGHT))
    ten = P.views_ten(w, h, R, S)
    assert len(ten) == 10 and ten[:5] == P.views_five(w, h, R, S)
    for i, v in enumerate(ten):
        assert np.array_equal(np.asarray(P.apply_view_pil(a, v, to_tensor=False)), np.asarray(want[i])), i
        assert np.array_equal(VC.emulate(a, v), np.asarray(want[i])), i
    # view 5 + i is the mirror image of a window of the unmirrored image: tl <-> tr, bl <-> br, the centre stays the centre (of the mirrored side)
    f = ten[:5]
    for i, j in ((0, 1), (1, 0), (2, 3), (3, 2)):
        assert ten[5 + i] == f[j]._replace(flip=1)
    assert ten[9] == f[4]._replace(left=rw - S - f[4].left, flip=1) and abs(ten[9].left - f[4].left) == (rw - S) % 2
    assert P.mirrored(ten) == VC.recipe(w, h, R, S)                              # the case table's own restatement of the geometry
    assert P.view_resized_crop(w, h, (1, 2, 5, 7), S, flip=True) == P.View(1, 2, 5, 7, S, S, 0, 0, 1, S)
    with pytest.raises(ValueError):
        P.view_resized_crop(w, h, (w - 4, 0, 5, 7), S)
    with pytest.raises(ValueError):
        P.views_five(w, h, S - 1, S)


MUTS = {"resize_box_semantics": VC.MUT_BOX, "offset_in_source_coordinates": VC.MUT_SRC_OFFSET, "corner_off_by_one": VC.MUT_CORNER,
        "centre_round_half_up": VC.MUT_HALF_UP, "flip_of_the_same_named_window": VC.MUT_SAME_NAME}


@pytest.mark.parametrize("mut", list(MUTS), ids=list(MUTS))
def test_every_case_sees_the_planted_mistake(mut):
    """each mistake changes at least one output byte in EVERY case it can touch, and none in a case it cannot"""
    seen = 0
    for c in VC.CASES:
        touched = VC.applies(c, MUTS[mut])
        d = int((VC.mutated(c, MUTS[mut]) != VC.expected(c)).sum())
        assert (d >= 1) == touched, f"{c.name}: {mut} changes {d} bytes, applies() says {touched}"
        seen += touched
    assert seen >= {"resize_box_semantics": 20, "offset_in_source_coordinates": 100, "corner_off_by_one": 100, "centre_round_half_up": 16,
                    "flip_of_the_same_named_window": 50}[mut], seen


def test_ext_header_declares_the_view_entries():
    hdr = open(os.path.join(ROOT, "include", "selftok_hip_ext.h")).read()
    names = set(re.findall(r"\b(selftok_\w+)\s*\(", hdr))
    assert NEW_ENTRIES <= names and NEW_ENTRIES <= set(_lib.EXT_SIGNATURES) and not (NEW_ENTRIES & set(_lib.SIGNATURES))
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


def test_image_views_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "image_views.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == 5 and len(scratch) == len(kernels), (kernels, scratch)                # plan, tables, horizontal, vertical x {bf16, fp32}
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    src, shared = (open(os.path.join(G.CSRC, f)).read() for f in ("image_views.hip", "image_resample_shared.h"))
    assert "asm" not in (src + shared).replace("namespace", "")               # plain C++, in the unit and in the resample it includes,
    assert "#pragma clang fp contract(off)" in src and "#pragma clang fp contract(off)" in shared   # every fp64 operation rounded on its own
    assert "-ffp-contract=off" in cmd


GOOD = [0, 37, 29, 9, 14, 20, 9, 16, 16, 0, 0, 1]                           # offset, W, H, x0, y0, bw, bh, Rw, Rh, left, top, flip


def _row(**kw):
    names = ["off", "W", "H", "x0", "y0", "bw", "bh", "rw", "rh", "left", "top", "flip"]
    r = list(GOOD)
    for k, v in kw.items():
        r[names.index(k)] = v
    return np.array([GOOD, r], dtype=np.int64)


REFUSED = [("box that is empty", dict(x0=18)), ("box that is empty", dict(y0=21)), ("box that is empty", dict(x0=-1)), ("box that is empty", dict(bw=0)), ("box that is empty", dict(bh=38)),
           ("window outside", dict(left=1)), ("window outside", dict(rw=20, left=5)), ("window outside", dict(top=-1)), ("below S", dict(rw=15)), ("below S", dict(rh=15)),
           ("below S", dict(rh=1 << 30)), ("flip that is neither", dict(flip=2)), ("flip that is neither", dict(flip=-1)), ("1 .. 65536", dict(W=0)), ("1 .. 65536", dict(H=65537)),
           ("past the packed buffer", dict(off=-1))]


def test_host_side_refusals_launch_nothing():
    """the query and the entry validate the host table first: SELFTOK_EINVAL with a message, and the entry returns before it touches a pointer"""
    lib = _lib.load()
    good = np.array([GOOD], dtype=np.int64)
    n = lib.selftok_img_views_u8_workspace_bytes(good.ctypes.data, 1, 16)
    lay = np.zeros(4, dtype=np.int64)
    assert n > 0 and lib.selftok_img_views_tables_layout(good.ctypes.data, 1, 16, lay.ctypes.data) == 0
    assert lay[0] == 20 and lay[1] == 2 + 5 and lay[2] == 20 + 16 * 7 and lay[3] == 2 + 3      # 20 -> 16: 2 * ceil(1.25) + 1 taps; 9 -> 16 up: 3
    dummy = np.zeros(64, np.uint8)                                            # never read: every call below is refused by the host table
    for word, kw in REFUSED:
        t = _row(**kw)
        assert lib.selftok_img_views_u8_workspace_bytes(t.ctypes.data, 2, 16) == 0, kw
        msg = lib.selftok_last_error().decode()
        assert word in msg and "view 1" in msg, (kw, msg)
        rc = lib.selftok_img_views_u8(dummy.ctypes.data, 37 * 29 * 3, t.ctypes.data, dummy.ctypes.data, 2, 16, dummy.ctypes.data, 1, dummy.ctypes.data, dummy.ctypes.data, 1 << 30, None)
        assert rc == -1 and word in lib.selftok_last_error().decode(), kw
    rc = lib.selftok_img_views_u8(dummy.ctypes.data, 37 * 29 * 3 - 1, good.ctypes.data, dummy.ctypes.data, 1, 16, dummy.ctypes.data, 1, dummy.ctypes.data, dummy.ctypes.data, 1 << 30, None)
    assert rc == -1 and "past the packed buffer" in lib.selftok_last_error().decode()
    rc = lib.selftok_img_views_u8(dummy.ctypes.data, 37 * 29 * 3, good.ctypes.data, dummy.ctypes.data, 1, 16, dummy.ctypes.data, 1, dummy.ctypes.data, dummy.ctypes.data, n - 1, None)
    assert rc == -1 and "workspace" in lib.selftok_last_error().decode()
    for V, S in ((0, 16), (65536, 16), (1, 0), (1, 4097)):
        assert lib.selftok_img_views_u8_workspace_bytes(good.ctypes.data, V, S) == 0 and "1 <= S <= 4096" in lib.selftok_last_error().decode()
    # the Python layer: no views is an empty table, not an error; a source index outside the table is refused before the library is asked
    assert P.view_rows([[], []], 16).shape == (0, 10) and ops.image_view_rows(np.array([[0, 37, 29]]), P.view_rows([[]], 16)).shape == (0, 12)
    rows = ops.image_view_rows(np.array([[0, 37, 29], [3219, 5, 4]]), P.view_rows([[], P.views_five(5, 4, 4, 2)], 2))
    assert rows.shape == (5, 12) and rows[0].tolist()[:3] == [3219, 5, 4]
    with pytest.raises(_lib.SelftokHipError, match="source index"):
        ops.image_view_rows(np.array([[0, 37, 29]]), np.array([[1] + GOOD[3:]]))
    with pytest.raises(ValueError, match="size"):
        P.view_rows([[P.view_center(37, 29, 16)]], 8)
