"""not gpu: the arithmetic of record of csrc/image_filters.hip pinned on the host -- the numpy emulation of tests/image_filters_cases.py
against live Pillow on every case (the ADM cases against the published center_crop_arr run with Pillow), against its golden file, its bilinear
filter against the existing emulation and golden file, the planted mistakes every table must be able to see, the integer plan of the ADM chain,
the new declarations, the kernels' scratch and the host-side refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import image_io_cases as IO
import image_filters_cases as FC
from selftoktokenizer_amd import _lib, ops, preprocess as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"selftok_img_views_filter_u8_workspace_bytes", "selftok_img_views_filter_tables_layout", "selftok_img_views_filter_u8",
               "selftok_img_resize_u8_workspace_bytes", "selftok_img_resize_u8"}


def center_crop_arr(pil_image, image_size):
    """the published function (guided-diffusion's image_datasets.py, copied by the DiT / LlamaGen / VAR / MAR evaluation scripts), as it stands"""
    while min(*pil_image.size) >= 2 * image_size:
        pil_image = pil_image.resize(tuple(x // 2 for x in pil_image.size), resample=Image.BOX)
    scale = image_size / min(*pil_image.size)
    pil_image = pil_image.resize(tuple(round(x * scale) for x in pil_image.size), resample=Image.BICUBIC)
    arr = np.array(pil_image)
    crop_y = (arr.shape[0] - image_size) // 2
    crop_x = (arr.shape[1] - image_size) // 2
    return Image.fromarray(arr[crop_y: crop_y + image_size, crop_x: crop_x + image_size])


def halvings(c):
    return len(FC.adm_numbers(c.w, c.h, c.S)[0]) - 1


def test_case_tables_cover_what_they_claim():
    for S in (16, 24):
        short = {min(c.w, c.h) for c in FC.ADM_CASES if c.S == S}
        assert {2 * S - 1, 2 * S, 2 * S + 1, 4 * S - 1, 4 * S, 4 * S + 1} <= short, (S, short)
        geoms = {(c.w, c.h) for c in FC.ADM_CASES if c.S == S}
        assert all({x.content for x in FC.ADM_CASES if (x.w, x.h, x.S) == (w, h, S)} == set(FC.CONTENTS) for w, h in geoms)     # every geometry with every content
    g16 = {(c.w, c.h) for c in FC.ADM_CASES if c.S == 16}
    assert {(16, 300), (300, 16), (7, 9), (1, 3), (511, 300)} <= g16 and any(w % 2 != h % 2 for w, h in g16)
    assert FC.adm_numbers(16, 300, 16)[:3] == ([(16, 300)], 16, 300) and FC.adm_numbers(511, 300, 16)[0] == [(511, 300), (255, 150), (127, 75), (63, 37), (31, 18)]
    assert FC.adm_numbers(34, 32, 24)[1] == 26 and FC.adm_numbers(38, 32, 24)[1] == 28                 # 25.5 -> 26, 28.5 -> 28: Python's round
    assert {halvings(c) for c in FC.ADM_CASES} == {0, 1, 2, 3, 4}
    r = {(c.filter, c.w, c.h, c.ow, c.oh) for c in FC.RESIZE_CASES}
    for f in (FC.BOX, FC.BILINEAR, FC.BICUBIC):
        assert (f, 65, 33, 32, 16) in r and (f, 20, 20, 21, 300) in r
        assert any(x[0] == f and x[3] > x[1] for x in r) and any(x[0] == f and x[3] < x[1] for x in r)
    assert any(c.w == c.ow and c.h != c.oh for c in FC.RESIZE_CASES) and any(c.h == c.oh and c.w != c.ow for c in FC.RESIZE_CASES)
    assert max(c.w * c.h for c in FC.ADM_CASES + FC.RESIZE_CASES + FC.VIEW_CASES) <= 1 << 20
    a = FC.image(FC.ADM_CASES[2])
    assert FC.ADM_CASES[2].content == "binary" and set(np.unique(a)) == {0, 255}
    s = FC.image(FC.ADM_CASES[1])
    assert FC.ADM_CASES[1].content == "stripes" and (s == s[:1]).all() and len(np.unique(s[0, :, 0])) > 4
    sharp = [c for c in FC.ADM_CASES if c.content == "binary" and halvings(c) == 0 and c.w > 1 and FC.applies(c, FC.MUT_A075)]
    assert len(sharp) >= 5
    for c in sharp:                                                            # BICUBIC on unsmoothed {0, 255}: the unclipped sums leave 0 .. 255 on both sides
        rw = FC.adm_numbers(c.w, c.h, c.S)[1]
        raw = IO._pass(FC.image(c), FC.tables(c.w, rw, 0, rw, FC.BICUBIC), IO.MUT_NONE, keep_float=True)
        assert raw.min() < -1 and raw.max() > 256, (c.name, raw.min(), raw.max())


@pytest.mark.parametrize("S", [16, 24])
def test_adm_emulation_equals_the_published_function_on_live_pillow(S):
    for c in (c for c in FC.ADM_CASES if c.S == S):
        im = Image.fromarray(FC.image(c))
        ref = np.asarray(center_crop_arr(im, S))
        got = FC.expected(c)
        assert ref.shape == got.shape == (S, S, 3) and int((ref != got).sum()) == 0, f"{c.name}: {int((ref != got).sum())} bytes differ from Pillow"
        assert np.array_equal(np.asarray(P.center_crop_adm(im, S)), ref), c.name                        # the package's restatement, the route of record
        plan = P.adm_plan(c.w, c.h, S)                                         # the integers the device route is built from
        assert (list(plan.frames), plan.rw, plan.rh, plan.left, plan.top) == FC.adm_numbers(c.w, c.h, S), c.name
        assert tuple(P.view_adm(plan, S)) == FC.adm_view(c.w, c.h, S)
        chain = FC.image(c)                                                    # frame by frame, then the view: what the device route does
        for fw, fh in plan.frames[1:]:
            chain = FC.resize(chain, fw, fh, FC.BOX)
        assert np.array_equal(FC.view(chain, FC.adm_view(c.w, c.h, S), FC.BICUBIC), got), c.name


def test_resize_and_view_emulation_equal_live_pillow():
    for c in FC.RESIZE_CASES:
        ref = np.asarray(Image.fromarray(FC.image(c)).resize((c.ow, c.oh), c.filter))
        assert int((ref != FC.expected(c)).sum()) == 0, c.name
    for c in FC.VIEW_CASES:
        ref = np.asarray(P.apply_view_pil(FC.image(c), c.view, to_tensor=False, filter=c.filter))
        assert int((ref != FC.expected(c)).sum()) == 0, c.name
        t = P.apply_view_pil(FC.image(c), c.view, filter=FC.FILTER_NAMES[c.filter])
        assert np.array_equal(IO.to_tensor(FC.expected(c), False).view(np.uint32), t.numpy().view(np.uint32)), c.name
    a = FC.image(FC.RESIZE_CASES[0])                                           # the host helpers take the filter by name or by Pillow's code
    assert np.array_equal(np.asarray(P.resize_shorter_side(Image.fromarray(a), 16, "bicubic")), np.asarray(P.resize_shorter_side(Image.fromarray(a), 16, Image.BICUBIC)))
    assert np.array_equal(np.asarray(P.resize_shorter_side(Image.fromarray(a), 16)), np.asarray(P.resize_shorter_side(Image.fromarray(a), 16, "bilinear")))
    with pytest.raises(ValueError, match="unknown filter"):
        P.resize_shorter_side(Image.fromarray(a), 16, "cubic")


def test_emulation_equals_the_golden_file():
    g = np.load(FC.GOLDEN)
    cases = FC.ADM_CASES + FC.RESIZE_CASES + FC.VIEW_CASES
    assert list(g["names"]) == [c.name for c in cases]
    for i, c in enumerate(cases):
        assert FC.crc(FC.expected(c)) == int(g["crc_u8"][i]), c.name
        if not isinstance(c, FC.ResizeCase):
            assert FC.crc(IO.to_tensor(FC.expected(c), True)) == int(g["crc_bf16"][i]), c.name
    for filt, insz, outsz in ((FC.BICUBIC, 37, 16), (FC.BICUBIC, 16, 37), (FC.BOX, 65, 32), (FC.BOX, 20, 300)):
        xmin, n, k = FC.tables(insz, outsz, 0, outsz, filt)
        key = f"tab_{filt}_{insz}_{outsz}_"
        assert np.array_equal(g[key + "xmin"], xmin) and np.array_equal(g[key + "n"], n) and np.array_equal(g[key + "k"], k), key
        assert k.shape[1] <= FC.ksize(insz, outsz, filt) and np.abs(k.sum(axis=1) - (1 << FC.PB)).max() <= k.shape[1]
    assert (FC.tables(37, 16, 0, 16, FC.BICUBIC)[2] < 0).any()                # the lobes: negative coefficients, the sign-aware rounding is in use


@pytest.mark.parametrize("case", IO.CASES, ids=lambda c: c.name)
def test_bilinear_through_the_new_emulation_is_the_existing_one(case):
    g = np.load(IO.GOLDEN)
    i = list(g["names"]).index(case.name)
    got = FC.view(IO.image(case), tuple(P.view_center(case.w, case.h, case.S)), FC.BILINEAR)
    assert np.array_equal(got, IO.resize_crop(IO.image(case), case.S))
    assert IO.crc(got) == int(g["crc_u8"][i]) and IO.crc(IO.to_tensor(got, True)) == int(g["crc_bf16"][i])
    for insz, outsz in IO.TABLE_GEOMS[:2]:
        for a, b in zip(FC.tables(insz, outsz, 3, 40, FC.BILINEAR), IO.tables(insz, outsz, 3, 40)):
            assert np.array_equal(a, b)


MUTS = {"bicubic_a_minus_0p75": FC.MUT_A075, "box_closed_on_the_other_side": FC.MUT_BOX_CLOSED, "mean_of_2x2_for_the_box_taps": FC.MUT_MEAN2X2,
        "one_bicubic_pass_without_the_chain": FC.MUT_NO_CHAIN, "crop_offset_half_to_even": FC.MUT_CROP_HALF_EVEN, "target_size_half_up": FC.MUT_SIZE_HALF_UP,
        "no_uint8_between_chain_stages": FC.MUT_NO_U8_CHAIN, "vertical_pass_first": FC.MUT_VFIRST}


@pytest.mark.parametrize("mut", list(MUTS), ids=list(MUTS))
def test_the_tables_see_the_planted_mistake(mut):
    """each mistake changes at least one byte in exactly the cases `applies` names, and at least two cases see it.  Where `applies` gives None
    (a rounding-order mistake on lattice content: its docstring) the case is asked nothing."""
    seen = 0
    for c in FC.ADM_CASES + FC.RESIZE_CASES:
        touched = FC.applies(c, MUTS[mut])
        got = FC.mutated(c, MUTS[mut])
        d = int((got != FC.expected(c)).sum()) if got.shape == FC.expected(c).shape else -1
        if touched is None:
            continue
        assert (d != 0) == touched, f"{c.name}: {mut} changes {d} bytes, applies() says {touched}"
        seen += touched
    assert seen >= 2, seen
    noise = [c for c in FC.ADM_CASES + FC.RESIZE_CASES if c.content == "noise"]
    assert all(FC.applies(c, MUTS[mut]) is not None for c in noise)            # hash noise decides every mistake


def test_adm_plan_limits():
    assert P.adm_plan(1, 3, 16) == P.AdmPlan(((1, 3),), 16, 48, 0, 16)
    assert len(P.adm_plan(65536, 65536, 256).frames) == 9                      # eight halvings, down to 256 x 256
    with pytest.raises(ValueError, match="halvings"):
        P.adm_plan(65536, 65536, 128)
    with pytest.raises(ValueError):
        P.adm_plan(0, 3, 16)
    assert P.center_crop(Image.new("RGB", (19, 16)), 16).size == (16, 16) and P._centre(19, 16) == 2 and P.adm_plan(19, 16, 16).left == 1      # 1.5: half to even against floor


def test_ext_header_declares_the_filter_entries():
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
    for old in ("selftok_img_resize_crop_norm_u8", "selftok_img_views_u8"):    # the bilinear entries keep their signatures
        assert len(_lib.EXT_SIGNATURES[old][1]) == 12


def test_image_filters_compiles_for_gfx950_without_scratch(tmp_path):
    import __graft_entry__ as G
    objs, _ = G.compile_commands(objdir=str(tmp_path), extra=("-Rpass-analysis=kernel-resource-usage",))
    cmd = next(c for o, _, c in objs if os.path.basename(o) == "image_filters.o")
    r = subprocess.run(cmd, cwd=G.CSRC, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = re.findall(r"Function Name: (\S+)", r.stderr)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(kernels) == 10 and len(scratch) == len(kernels), (kernels, scratch)               # the shared five, and check, layout, tables, horizontal, vertical of the frames
    assert all(s == 0 for s in scratch), dict(zip(kernels, scratch))
    src, shared = (open(os.path.join(G.CSRC, f)).read() for f in ("image_filters.hip", "image_resample_shared.h"))
    assert "asm" not in (src + shared).replace("namespace", "")
    assert "#pragma clang fp contract(off)" in src and "#pragma clang fp contract(off)" in shared and "-ffp-contract=off" in cmd
    for libm in ("sin(", "cos(", "pow(", "exp(", "math.h", "cmath"):
        assert libm not in src + shared, libm                                  # polynomials and comparisons only


GOOD_VIEW = [0, 37, 29, 9, 14, 20, 9, 16, 16, 0, 0, 1]
GOOD_FRAME = [0, 8, 6, 200, 4, 3]                                             # 144 source bytes at 0, 36 destination bytes at 200


def test_host_side_refusals_launch_nothing():
    """filters, tables and regions are refused on the host table, before a pointer is touched (every device pointer below is a host dummy)"""
    lib = _lib.load()
    dummy = np.zeros(64, np.uint8)
    view, frame = np.array([GOOD_VIEW], dtype=np.int64), np.array([GOOD_FRAME], dtype=np.int64)
    lay = np.zeros(4, dtype=np.int64)
    for filt, ksh, ksv in ((FC.BILINEAR, 5, 3), (FC.BICUBIC, 7, 5), (FC.BOX, 3, 3)):           # 20 -> 16 down, 9 -> 16 up
        assert lib.selftok_img_views_filter_u8_workspace_bytes(view.ctypes.data, 1, 16, filt) > 0
        assert lib.selftok_img_views_filter_tables_layout(view.ctypes.data, 1, 16, filt, lay.ctypes.data) == 0
        assert lay.tolist() == [20, 2 + ksh, 20 + 16 * (2 + ksh), 2 + ksv], (filt, lay)
        assert (ksh, ksv) == (FC.ksize(20, 16, filt), FC.ksize(9, 16, filt))
        assert lib.selftok_img_resize_u8_workspace_bytes(frame.ctypes.data, 1, filt) > 0
    old = np.zeros(4, dtype=np.int64)
    assert lib.selftok_img_views_tables_layout(view.ctypes.data, 1, 16, old.ctypes.data) == 0 and old.tolist() == [20, 7, 20 + 16 * 7, 5]
    assert lib.selftok_img_views_filter_u8_workspace_bytes(view.ctypes.data, 1, 16, 2) == lib.selftok_img_views_u8_workspace_bytes(view.ctypes.data, 1, 16)
    for code, name in ((1, "LANCZOS"), (5, "HAMMING"), (0, "NEAREST"), (6, "unknown"), (-1, "unknown")):
        assert lib.selftok_img_views_filter_u8_workspace_bytes(view.ctypes.data, 1, 16, code) == 0 and name in lib.selftok_last_error().decode()
        assert lib.selftok_img_views_filter_tables_layout(view.ctypes.data, 1, 16, code, lay.ctypes.data) == -1
        rc = lib.selftok_img_views_filter_u8(dummy.ctypes.data, 37 * 29 * 3, view.ctypes.data, dummy.ctypes.data, 1, 16, code, dummy.ctypes.data, 1, dummy.ctypes.data, dummy.ctypes.data, 1 << 30, None)
        msg = lib.selftok_last_error().decode()
        assert rc == -1 and name in msg and "BICUBIC" in msg, msg
        assert ("sin / cos" in msg) == (name in ("LANCZOS", "HAMMING")), msg
        assert lib.selftok_img_resize_u8_workspace_bytes(frame.ctypes.data, 1, code) == 0 and name in lib.selftok_last_error().decode()
        rc = lib.selftok_img_resize_u8(dummy.ctypes.data, 1 << 20, frame.ctypes.data, dummy.ctypes.data, 1, code, dummy.ctypes.data, 1 << 30, None)
        assert rc == -1 and name in lib.selftok_last_error().decode()
    for name in ("lanczos", "HAMMING", "nearest", Image.LANCZOS, Image.HAMMING, Image.NEAREST):
        with pytest.raises(_lib.SelftokHipError, match="(?i)" + (name if isinstance(name, str) else "not served")):
            ops.image_filter_code(name)
    assert [ops.image_filter_code(f) for f in ("bilinear", "BICUBIC", "box", Image.BILINEAR, Image.BICUBIC, Image.BOX)] == [2, 3, 4, 2, 3, 4]
    with pytest.raises(_lib.SelftokHipError, match="unknown filter"):
        ops.image_filter_code("cubic")
    # a bad view row is refused as by the bilinear entry
    bad = np.array([GOOD_VIEW, GOOD_VIEW[:9] + [1, 0, 1]], dtype=np.int64)
    assert lib.selftok_img_views_filter_u8_workspace_bytes(bad.ctypes.data, 2, 16, 3) == 0 and "view 1" in lib.selftok_last_error().decode() and "window outside" in lib.selftok_last_error().decode()
    # frames: limits, regions inside the buffer, no destination on a source or a destination
    def frames(*rows):
        return np.array(rows, dtype=np.int64).reshape(len(rows), 6)
    refused = [("1 .. 65536", frames([0, 0, 6, 200, 4, 3]), 1 << 20), ("1 .. 65536", frames([0, 8, 6, 200, 65537, 3]), 1 << 40), ("source that reaches past", frames(GOOD_FRAME), 143 + 0),
               ("source that reaches past", frames([-1, 8, 6, 200, 4, 3]), 1 << 20), ("destination that reaches past", frames(GOOD_FRAME), 235),
               ("overlaps", frames([0, 8, 6, 143, 4, 3]), 1 << 20),                                  # its own source's last byte
               ("overlaps", frames(GOOD_FRAME, [300, 8, 6, 235, 4, 3]), 1 << 20),                    # the last byte of the other destination
               ("overlaps", frames(GOOD_FRAME, [210, 2, 2, 500, 1, 1]), 1 << 20),                    # a source inside the other row's destination
               ("overlaps", frames(GOOD_FRAME, [300, 8, 6, 200, 4, 3]), 1 << 20)]                    # the same destination twice
    for word, t, nbytes in refused:
        rc = lib.selftok_img_resize_u8(dummy.ctypes.data, nbytes, t.ctypes.data, dummy.ctypes.data, len(t), 4, dummy.ctypes.data, 1 << 30, None)
        assert rc == -1 and word in lib.selftok_last_error().decode(), (word, t.tolist(), lib.selftok_last_error().decode())
    ok = frames(GOOD_FRAME, [0, 8, 6, 236, 4, 3], [144, 2, 2, 272, 1, 1])      # one source twice, regions that touch: accepted by the host
    n = lib.selftok_img_resize_u8_workspace_bytes(ok.ctypes.data, 3, 4)
    assert n > 0
    assert lib.selftok_img_resize_u8(dummy.ctypes.data, 275, ok.ctypes.data, dummy.ctypes.data, 3, 4, dummy.ctypes.data, n - 1, None) == -1 and "workspace" in lib.selftok_last_error().decode()
    for N in (0, 65536):
        assert lib.selftok_img_resize_u8_workspace_bytes(ok.ctypes.data, N, 4) == 0 and "1 <= N <= 65535" in lib.selftok_last_error().decode()
    with pytest.raises(_lib.SelftokHipError, match=r"\[N, 6\]"):
        ops.image_resize(None, np.zeros((1, 5), np.int64), "box")
    with pytest.raises(_lib.SelftokHipError, match="LANCZOS"):
        ops.image_resize(None, ok, Image.LANCZOS)
    with pytest.raises(_lib.SelftokHipError, match="HAMMING"):
        ops.image_views(None, None, None, 16, filter="hamming")
    # the loader: views with the ADM protocol, an unknown recipe
    with pytest.raises(ValueError, match="expected one of"):
        P.DeviceLoader(16, "cuda", preprocess="lanczos")
    loader = P.DeviceLoader(16, "cuda", preprocess="adm")
    try:
        with pytest.raises(ValueError, match="takes no views"):
            loader._stage([np.zeros((20, 20, 3), np.uint8)], 0, views=lambda w, h: P.views_five(w, h, 16, 16))
    finally:
        loader.close()
