"""The case table of tests/test_image_views_*.py and a numpy restatement of the arithmetic of record of a *view* (csrc/image_views.hip):

    im = source.crop(box) -> im.resize((rw, rh), BILINEAR) unless that is the box's size -> im.crop(window) -> FLIP_LEFT_RIGHT if flip

which is what torchvision's FiveCrop / TenCrop / resized_crop / hflip do to a PIL image.  The resample is image_io_cases' (`tables`, `_pass`:
Pillow's 8-bit ImagingResample), only the window's S rows and columns are computed.  The geometry of the recipes is restated here
(`recipe`), apart from selftoktokenizer_amd.preprocess, with `MUT_*` switches that plant the mistakes the table must be able to see.

Sizes are the smallest at which each edge exists; the two 256-pixel cases are the recipe in use (Resize(281) -> TenCrop(256))."""
from collections import namedtuple

import numpy as np

import image_io_cases as IO
from image_io_cases import PB, _pass, tables
from selftoktokenizer_amd.preprocess import View

MUT_NONE, MUT_BOX, MUT_SRC_OFFSET, MUT_CORNER, MUT_HALF_UP, MUT_SAME_NAME = range(6)

# name: sources are images of image_io_cases (a function of the pixel index); view: a preprocess.View; R / index: the recipe the view came from
# (group a), None for the resized crops of group b
Case = namedtuple("Case", "name w h content view R index")


def recipe(w, h, R, S, mut=MUT_NONE):
    """Resize(R) -> TenCrop(S), then the mirror image of each of the ten: 20 views, every window both flipped and unflipped"""
    rw, rh = IO.target_size(w, h, R)
    far = 1 if mut == MUT_CORNER else 0                                      # the planted off-by-one of the right / bottom corner
    cx, cy = (IO.crop_offset(s, S, mut == MUT_HALF_UP) for s in (rw, rh))
    right, bottom = max(rw - S - far, 0), max(rh - S - far, 0)
    five = [(0, 0), (right, 0), (0, bottom), (right, bottom), (cx, cy)]
    ten = [View(0, 0, w, h, rw, rh, l, t, 0, S) for l, t in five]
    ten += [v._replace(flip=1) if mut == MUT_SAME_NAME else v._replace(left=rw - S - v.left, flip=1) for v in ten]
    return ten + [v._replace(flip=1 - v.flip) for v in ten]


def _group_a():
    out = []
    geoms = [(37, 29, "noise", 16, R) for R in (16, 18, 23)] + [(29, 37, "noise", 16, R) for R in (16, 18, 23)]
    geoms += [(64, 64, "noise", 16, R) for R in (16, 18, 23)] + [(100, 180, "ramp", 16, R) for R in (16, 18, 23)]
    geoms += [(23, 41, "noise", 8, 11), (500, 375, "noise", 256, 281), (375, 500, "noise", 256, 281)]
    for w, h, content, S, R in geoms:
        for i, v in enumerate(recipe(w, h, R, S)):
            out.append(Case(f"a_{w}x{h}_R{R}_S{S}_{i:02d}", w, h, content, v, R, i))
    return out


def _group_b():
    out = []
    boxes = [(37, 29, (9, 14, 20, 9)), (37, 29, (25, 3, 11, 13)), (37, 29, (36, 0, 1, 29)), (37, 29, (0, 22, 37, 7)), (37, 29, (0, 0, 37, 29)),
             (500, 375, (17, 23, 200, 150))]
    for w, h, (x0, y0, bw, bh) in boxes:
        for S in (8, 16, 64):
            for flip in (0, 1):
                out.append(Case(f"b_{w}x{h}_box{x0}_{y0}_{bw}x{bh}_S{S}_f{flip}", w, h, "noise", View(x0, y0, bw, bh, S, S, 0, 0, flip, S), None, None))
    return out


GROUP_A, GROUP_B = _group_a(), _group_b()
CASES = GROUP_A + GROUP_B
MIXED = CASES[::-1]                                                          # group c: everything in one call, reversed, several views per source

_images = {}


def image(case):
    key = (case.w, case.h, case.content)
    if key not in _images:
        _images[key] = IO.image(IO.Case("src", case.w, case.h, 0, case.content))
        _images[key].setflags(write=False)
    return _images[key]


def _tables_box(insz, in0, in1, outsz, first, count):
    """Pillow's resize(box=): precompute_coeffs with the box INSIDE a larger image, so that the taps of the edge outputs reach pixels outside
    the box (absolute coordinates).  Not the arithmetic of record -- the planted mistake MUT_BOX."""
    scale = (in1 - in0) / outsz
    fs = max(scale, 1.0)
    support, ss = 1.0 * fs, 1.0 / fs
    center = in0 + (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    n = np.minimum((center + support + 0.5).astype(np.int64), insz) - xmin
    kmax = int(n.max())
    w, ww = np.zeros((count, kmax)), np.zeros(count)
    for x in range(kmax):
        a = np.abs(((x + xmin) - center + 0.5) * ss)
        w[:, x] = np.where((a < 1.0) & (x < n), 1.0 - a, 0.0)
        ww = ww + w[:, x]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = (0.5 + w * (1 << PB)).astype(np.int64)
    k[np.arange(kmax)[None, :] >= n[:, None]] = 0
    return xmin, n, k


def _axis(full, lo, box, resized, first, S, mut):
    """tap rows of one axis in ABSOLUTE source coordinates"""
    if mut == MUT_BOX and box != resized:
        return _tables_box(full, lo, lo + box, resized, first, S)
    if mut == MUT_SRC_OFFSET and box != resized:
        xmin, n, k = tables(box, resized, 0, S)
        xmin = np.minimum(xmin + first, box - 1)
        return xmin + lo, np.minimum(n, box - xmin), k
    xmin, n, k = tables(box, resized, first, S)
    return xmin + lo, n, k


def emulate(a, view, mut=MUT_NONE):
    """uint8 [h, w, 3] source -> uint8 [S, S, 3]: the view, the window only.  `mut`: MUT_BOX / MUT_SRC_OFFSET plant an arithmetic mistake here; the
    geometry mistakes are planted in `recipe`."""
    v = View(*view)
    h, w, _ = a.shape
    th = _axis(w, v.x0, v.bw, v.rw, v.left, v.size, mut)
    tv = _axis(h, v.y0, v.bh, v.rh, v.top, v.size, mut)
    r0, r1 = int(tv[0].min()), int((tv[0] + tv[1]).max())
    mid = _pass(a[r0:r1], th, IO.MUT_NONE)
    out = _pass(mid.transpose(1, 0, 2), (tv[0] - r0, tv[1], tv[2]), IO.MUT_NONE).transpose(1, 0, 2)
    return np.ascontiguousarray(out[:, ::-1] if v.flip else out)


_expected = {}


def expected(case):
    """the view's uint8 [S, S, 3], computed once and shared (read-only)"""
    if case.name not in _expected:
        _expected[case.name] = emulate(image(case), case.view)
        _expected[case.name].setflags(write=False)
    return _expected[case.name]


def mutated(case, mut):
    """the case's output under a planted mistake; a mistake of the five / ten-crop recipe leaves a resized crop (no recipe) as it is"""
    if mut in (MUT_BOX, MUT_SRC_OFFSET):
        return emulate(image(case), case.view, mut)
    if case.R is None:
        return expected(case)
    return emulate(image(case), recipe(case.w, case.h, case.R, case.view.size, mut)[case.index])


def applies(case, mut):
    """can the planted mistake change the arithmetic of this case at all?"""
    v = case.view
    S = v.size
    if mut == MUT_BOX:                          # an axis that is resampled from a box with source pixels beyond one of its ends
        return (v.bw != v.rw and (v.x0 > 0 or v.x0 + v.bw < case.w)) or (v.bh != v.rh and (v.y0 > 0 or v.y0 + v.bh < case.h))
    if mut == MUT_SRC_OFFSET:                   # a resampled axis whose window does not start at 0: left * scale != left
        return (v.bw != v.rw and v.left > 0) or (v.bh != v.rh and v.top > 0)
    if case.R is None:                          # the geometry mistakes live in the five / ten-crop recipe
        return False
    i = case.index % 10                         # the mirror images (10 ..) are the same windows
    dx, dy = v.rw - S, v.rh - S
    win = i % 5                                 # tl, tr, bl, br, centre; 5 .. 9 of the mirrored image
    if mut == MUT_CORNER:                       # the right / bottom windows, of the image and of its mirror image alike
        return (win in (1, 3) and dx > 0) or (win in (2, 3) and dy > 0)
    if mut == MUT_HALF_UP:                      # x.5 with an even integer part: half-even goes down, half-up goes up
        return win == 4 and any(d % 2 == 1 and (d // 2) % 2 == 0 for d in (dx, dy))
    if mut == MUT_SAME_NAME:                    # the window of the mirrored image is another window unless it is its own mirror image
        return i >= 5 and (dx > 0 if win < 4 else dx % 2 == 1)
    return False


def to_tensor(u8, bf16):
    return IO.to_tensor(u8, bf16)
