"""The case tables of tests/test_image_filters_*.py and a numpy restatement of the arithmetic of record of csrc/image_filters.hip:

    Image.resize((ow, oh), filter) for Pillow's BILINEAR, BICUBIC and BOX (8-bit ImagingResample: fp64 weights in Pillow's order, 22-bit
    coefficients, horizontal pass first, uint8 between the passes, an unchanged axis not resampled), a *view* resampled with such a filter,
    and the ADM protocol `center_crop_arr`: BOX halvings while the shorter side is >= 2 S, one BICUBIC resize to Python's round(side * (S / min)),
    the centre crop at (side - S) // 2.

The filters are evaluated in fp64 exactly as Pillow's C writes them (`weight`).  `MUT_*` switches plant the mistakes the tables must be able to see;
`applies` says, from the geometry and the tap arguments alone, which cases each mistake can reach.

Sources are tiny (S = 16 and S = 24) and arithmetic: hash noise, one-pixel vertical stripes (a hashed level each), and {0, 255} hash noise whose
bicubic overshoot hits the clip.

    python tests/image_filters_cases.py --write-golden      # re-records tests/golden/image_filters.npz
"""
import os
import sys
from collections import namedtuple

import numpy as np

if __name__ == "__main__":                                                    # run as a script: the package lies beside tests/
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import image_io_cases as IO
from image_io_cases import PB, _pass

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_filters.npz")
BILINEAR, BICUBIC, BOX = 2, 3, 4                                              # Pillow's codes
SUPPORT = {BILINEAR: 1.0, BICUBIC: 2.0, BOX: 0.5}
FILTER_NAMES = {BILINEAR: "bilinear", BICUBIC: "bicubic", BOX: "box"}

(MUT_NONE, MUT_A075, MUT_BOX_CLOSED, MUT_MEAN2X2, MUT_NO_CHAIN, MUT_CROP_HALF_EVEN, MUT_SIZE_HALF_UP, MUT_NO_U8_CHAIN, MUT_VFIRST) = range(9)


# ---- the arithmetic of record ----
def weight(filt, x, mut=MUT_NONE):
    """Pillow's bilinear_filter / bicubic_filter / box_filter on an fp64 array, operation by operation"""
    x = np.asarray(x, np.float64)
    if filt == BOX:
        inside = (x >= -0.5) & (x < 0.5) if mut == MUT_BOX_CLOSED else (x > -0.5) & (x <= 0.5)
        return np.where(inside, 1.0, 0.0)
    x = np.abs(x)
    if filt == BICUBIC:
        a = -0.75 if mut == MUT_A075 else -0.5
        near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        far = (((x - 5) * x + 8) * x - 4) * a
        return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))
    return np.where(x < 1.0, 1.0 - x, 0.0)


def tap_args(insz, outsz, first, count, filt):
    """precompute_coeffs' bounds: (xmin [count], n [count], the filter's argument of every tap [count, kmax], its validity mask)"""
    scale = insz / outsz
    fs = max(scale, 1.0)
    support, ss = SUPPORT[filt] * fs, 1.0 / fs
    center = (np.arange(first, first + count, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)            # astype truncates toward zero, as (int)
    n = np.minimum((center + support + 0.5).astype(np.int64), insz) - xmin
    kmax = int(n.max())
    x = np.arange(kmax)[None, :]
    return xmin, n, ((x + xmin[:, None]) - center[:, None] + 0.5) * ss, x < n[:, None]


def ksize(insz, outsz, filt):
    """Pillow's ksize, the width of the kernels' tap rows: 2 * ceil(support) + 1; 1 for an axis that is not resampled"""
    return 1 if insz == outsz else 2 * int(np.ceil(SUPPORT[filt] * max(insz / outsz, 1.0))) + 1


def tables(insz, outsz, first, count, filt, mut=MUT_NONE):
    """tap rows of output indices first .. first + count: (xmin, n, k [count, kmax] int64); the identity when the axis keeps its length"""
    if insz == outsz:
        return np.arange(first, first + count), np.ones(count, np.int64), np.full((count, 1), 1 << PB, np.int64)
    xmin, n, arg, valid = tap_args(insz, outsz, first, count, filt)
    w = np.where(valid, weight(filt, arg, mut), 0.0)
    ww = np.zeros(count)
    for x in range(w.shape[1]):                                              # left to right, as the C loop accumulates ww
        ww = ww + w[:, x]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    k = np.where(w < 0, (-0.5 + w * (1 << PB)).astype(np.int64), (0.5 + w * (1 << PB)).astype(np.int64))
    k[~valid] = 0
    return xmin, n, k


def resize(a, ow, oh, filt, mut=MUT_NONE, keep_float=False, from_float=False):
    """Image.resize((ow, oh), filt) of a [h, w, 3] frame.  keep_float / from_float: the frame leaves / arrives unrounded (MUT_NO_U8_CHAIN)"""
    h, w, _ = a.shape
    th, tv = tables(w, ow, 0, ow, filt, mut), tables(h, oh, 0, oh, filt, mut)
    if mut == MUT_VFIRST:
        mid = _pass(a.transpose(1, 0, 2), tv, IO.MUT_NONE, from_float=from_float).transpose(1, 0, 2) if h != oh else a
        ff = from_float and h == oh
        return _pass(mid, th, IO.MUT_NONE, keep_float=keep_float, from_float=ff) if w != ow else (mid if not ff or keep_float else _round(mid))
    if w != ow:
        mid, ff = _pass(a, th, IO.MUT_NONE, keep_float=keep_float and h == oh, from_float=from_float), False
    else:
        mid, ff = a, from_float
    if h != oh:
        return np.ascontiguousarray(_pass(mid.transpose(1, 0, 2), tv, IO.MUT_NONE, keep_float=keep_float, from_float=ff).transpose(1, 0, 2))
    return mid if not ff or keep_float else _round(mid)


def _round(f):
    return np.clip(np.floor(f + 0.5), 0, 255).astype(np.uint8)


def adm_numbers(w, h, S, mut=MUT_NONE):
    """center_crop_arr as integers, restated here apart from selftoktokenizer_amd.preprocess.adm_plan: (frames, rw, rh, left, top)"""
    frames = [(w, h)]
    while min(w, h) >= 2 * S and mut != MUT_NO_CHAIN:
        w, h = w // 2, h // 2
        frames.append((w, h))
    scale = S / min(w, h)
    rnd = (lambda v: int(np.floor(v + 0.5))) if mut == MUT_SIZE_HALF_UP else round
    rw, rh = rnd(w * scale), rnd(h * scale)
    off = (lambda side: IO.crop_offset(side, S)) if mut == MUT_CROP_HALF_EVEN else (lambda side: (side - S) // 2)
    return frames, rw, rh, off(rw), off(rh)


def _mean2x2(a):
    h, w, _ = a.shape
    b = a[:h // 2 * 2, :w // 2 * 2].astype(np.int64)
    return ((b[0::2, 0::2] + b[0::2, 1::2] + b[1::2, 0::2] + b[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def adm(a, S, mut=MUT_NONE):
    """uint8 [h, w, 3] -> uint8 [S, S, 3]: center_crop_arr, every frame of the chain resized whole"""
    h, w, _ = a.shape
    frames, rw, rh, left, top = adm_numbers(w, h, S, mut)
    loose = mut == MUT_NO_U8_CHAIN
    for i, (fw, fh) in enumerate(frames[1:]):
        a = _mean2x2(a) if mut == MUT_MEAN2X2 else resize(a, fw, fh, BOX, mut, keep_float=loose, from_float=loose and i > 0)
    a = resize(a, rw, rh, BICUBIC, mut, from_float=loose and len(frames) > 1)
    if a.dtype != np.uint8:                                                   # a chain that ends unrounded (no bicubic pass after the halvings)
        a = _round(a)
    return np.ascontiguousarray(a[top:top + S, left:left + S])


def view(a, v, filt):
    """a preprocess.View of a uint8 [h, w, 3] source resampled with `filt`, the window only (image_views_cases.emulate with a filter)"""
    x0, y0, bw, bh, rw, rh, left, top, flip, S = (int(t) for t in v)
    th, tv = tables(bw, rw, left, S, filt), tables(bh, rh, top, S, filt)
    r0, r1 = int(tv[0].min()), int((tv[0] + tv[1]).max())
    mid = _pass(a[y0 + r0:y0 + r1, x0:x0 + bw], th, IO.MUT_NONE)
    out = _pass(mid.transpose(1, 0, 2), (tv[0] - r0, tv[1], tv[2]), IO.MUT_NONE).transpose(1, 0, 2)
    return np.ascontiguousarray(out[:, ::-1] if flip else out)


def adm_view(w, h, S):
    """the last frame's size and the view (x0 .. size) that turns it into the ADM output"""
    frames, rw, rh, left, top = adm_numbers(w, h, S)
    fw, fh = frames[-1]
    return (0, 0, fw, fh, rw, rh, left, top, 0, S)


# ---- the cases ----
AdmCase = namedtuple("AdmCase", "name w h S content")
ResizeCase = namedtuple("ResizeCase", "name w h ow oh filter content")
CONTENTS = ("noise", "stripes", "binary")

_ADM16 = [(16, 19), (19, 16), (32, 38), (31, 40), (32, 45), (33, 50), (63, 70), (64, 81), (65, 90), (40, 31), (45, 32), (90, 65), (70, 64), (16, 300), (300, 16), (7, 9), (1, 3), (511, 300), (37, 130), (130, 200)]
_ADM24 = [(48, 62), (47, 50), (48, 61), (49, 52), (95, 96), (96, 101), (97, 120), (34, 32), (38, 32), (32, 38), (32, 34), (130, 49)]
ADM_CASES = [AdmCase(f"adm_{w}x{h}_S{S}_{c}", w, h, S, c) for S, geoms in ((16, _ADM16), (24, _ADM24)) for w, h in geoms for c in CONTENTS]

_RESIZE = [(65, 33, 32, 16), (20, 20, 21, 300), (37, 29, 16, 16), (16, 16, 37, 29), (33, 16, 16, 16), (16, 40, 16, 20), (64, 48, 32, 24), (25, 27, 10, 12), (41, 23, 7, 50)]
RESIZE_CASES = [ResizeCase(f"rs_{FILTER_NAMES[f]}_{w}x{h}_to_{ow}x{oh}_{c}", w, h, ow, oh, f, c)
                for f in (BOX, BILINEAR, BICUBIC) for (w, h, ow, oh) in _RESIZE for c in (("noise", "binary") if f == BICUBIC else ("noise",))]

# views with a filter: the ten-crop of Resize(R) and resized crops (up, down, anisotropic, a one-pixel box), as in image_views_cases' small groups
ViewCase = namedtuple("ViewCase", "name w h content view filter")


def _view_cases():
    from selftoktokenizer_amd.preprocess import View, views_ten
    out = []
    for w, h, R, S, content in [(37, 29, 18, 16, "noise"), (29, 37, 23, 16, "binary"), (100, 180, 23, 16, "noise"), (23, 41, 11, 8, "binary"), (64, 64, 16, 16, "noise")]:
        for f in (BICUBIC, BOX):
            out += [ViewCase(f"v_{FILTER_NAMES[f]}_{w}x{h}_R{R}_S{S}_{i}", w, h, content, v, f) for i, v in enumerate(views_ten(w, h, R, S))]
    for w, h, box in [(37, 29, (9, 14, 20, 9)), (37, 29, (36, 0, 1, 29)), (37, 29, (0, 22, 37, 7)), (100, 180, (17, 23, 60, 150))]:
        for S in (8, 16):
            for f in (BICUBIC, BOX):
                out.append(ViewCase(f"v_{FILTER_NAMES[f]}_{w}x{h}_box{'_'.join(map(str, box))}_S{S}", w, h, "binary" if S == 8 else "noise", View(*box, S, S, 0, 0, S == 8, S), f))
    return out


VIEW_CASES = _view_cases()

_images = {}


def image(case):
    """uint8 [h, w, 3], a function of the pixel index alone"""
    key = (case.w, case.h, case.content)
    if key not in _images:
        if case.content == "binary":                                           # {0, 255} hash noise
            a = ((IO.image(IO.Case("src", case.w, case.h, 1, "noise")) >> 7) * 255).astype(np.uint8)
        elif case.content == "stripes":                                        # one-pixel vertical stripes, each with a level of its own (hashed), constant along y
            a = np.ascontiguousarray(np.broadcast_to(IO.image(IO.Case("src", case.w, 1, 2, "noise")), (case.h, case.w, 3)))
        else:
            a = IO.image(IO.Case("src", case.w, case.h, 0, case.content))
        a.setflags(write=False)
        _images[key] = a
    return _images[key]


_expected = {}


def expected(case):
    """the case's uint8 result, computed once and shared (read-only)"""
    if case.name not in _expected:
        a = image(case)
        r = adm(a, case.S) if isinstance(case, AdmCase) else view(a, case.view, case.filter) if isinstance(case, ViewCase) else resize(a, case.ow, case.oh, case.filter)
        r.setflags(write=False)
        _expected[case.name] = r
    return _expected[case.name]


def mutated(case, mut):
    a = image(case)
    if isinstance(case, AdmCase):
        return adm(a, case.S, mut)
    if mut in (MUT_A075, MUT_BOX_CLOSED, MUT_VFIRST):
        return resize(a, case.ow, case.oh, case.filter, mut)
    return expected(case)


def _on_the_edge(insz, outsz):
    """does a BOX tap of this axis sit exactly on the interval's edge (argument +-0.5 in fp64)?  Only then does the closed side matter"""
    if insz == outsz:
        return False
    scale = insz / outsz
    fs = max(scale, 1.0)
    center = (np.arange(outsz, dtype=np.float64) + 0.5) * scale
    lo = (center - 0.5 * fs + 0.5).astype(np.int64)
    x = np.arange(-1, int(np.ceil(fs)) + 2)[None, :] + lo[:, None]             # one input index beyond the taps on either side: the mistake may add a tap
    ok = (x >= 0) & (x < insz)
    arg = (x - center[:, None] + 0.5) * (1.0 / fs)
    return bool((ok & (np.abs(arg) == 0.5)).any())


def applies(case, mut):
    """can the planted mistake change the arithmetic of this case at all?  True / False from the geometry and the fp64 tap arguments, never from
    pixel values.  The contents enter only through what they are by construction:
      * "stripes" is constant along y, so a vertical pass returns its input (the coefficients sum to 2^22 within a few units) and a vertical
        offset moves nothing: only what a mistake does along x can show, and the order of the passes cannot;
      * an axis of one pixel is replicated by any filter.
    None: the mistake reaches the case but only through WHERE sums are rounded (MUT_NO_U8_CHAIN, MUT_VFIRST) and the content sits on a coarse
    lattice ("stripes" through a vertical pass, the two-level "binary"): whether a sum then crosses a rounding boundary is not decided by
    geometry, and the test asks nothing of such a case.  Hash noise decides every mistake."""
    stripes = case.content == "stripes"
    if isinstance(case, ResizeCase):                                           # all of them hash noise or two-level noise
        px, py = case.w != case.ow and case.w > 1, case.h != case.oh and case.h > 1
        if mut == MUT_A075:
            return case.filter == BICUBIC and (px or py)
        if mut == MUT_BOX_CLOSED:
            return case.filter == BOX and (_on_the_edge(case.w, case.ow) or _on_the_edge(case.h, case.oh))
        if mut == MUT_VFIRST:                                                  # BOX on an axis that grows is a selection (one tap of weight 1): nothing is rounded there
            grows = case.filter == BOX and (case.ow > case.w or case.oh > case.h)
            return (px and py and not grows) and (None if case.content == "binary" else True)
        return False
    frames, rw, rh, left, top = adm_numbers(case.w, case.h, case.S)
    halvings, (fw, fh) = len(frames) - 1, frames[-1]
    cx, cy = rw != fw and fw > 1, rh != fh and fh > 1 and not stripes          # the BICUBIC stage resamples this axis, visibly
    if mut == MUT_A075:
        return cx or cy
    if mut == MUT_BOX_CLOSED:
        return any(_on_the_edge(w0, w1) or (not stripes and _on_the_edge(h0, h1)) for (w0, h0), (w1, h1) in zip(frames, frames[1:]))
    if mut == MUT_MEAN2X2:                                                     # constant along y, an even width: (2a + 2b + 2) >> 2 is the BOX pair (a + b + 1) >> 1
        return any(w % 2 == 1 for w, _ in frames[:-1]) if stripes else halvings >= 1
    if mut == MUT_NO_CHAIN:
        return halvings >= 1
    wrong = adm_numbers(case.w, case.h, case.S, mut)
    if mut in (MUT_CROP_HALF_EVEN, MUT_SIZE_HALF_UP):                          # other numbers: a resized side, an offset
        return (wrong[1], wrong[3]) != (rw, left) or (not stripes and (wrong[2], wrong[4]) != (rh, top))
    if mut == MUT_NO_U8_CHAIN:                                                 # a stage must consume an unrounded frame
        reach = halvings >= 2 or (halvings == 1 and (rw, rh) != (fw, fh))
        return reach and (None if case.content != "noise" else True)
    if mut == MUT_VFIRST:                                                      # a stage with both passes: every halving, or the BICUBIC resize of both axes
        reach = not stripes and (halvings >= 1 or (cx and cy))
        return reach and (None if case.content == "binary" else True)
    return False


def crc(a):
    return IO.crc(a)


# ---- packing: what the stand-in and the GPU tests hand to the entries ----
GUARD = 0xA5


def pack_sources(cases, gap=5):
    """every distinct source once, odd gaps of GUARD between them -> (uint8 buffer, {(w, h, content): byte offset})"""
    at, chunks, where = 0, [], {}
    for c in cases:
        key = (c.w, c.h, c.content)
        if key not in where:
            where[key] = at
            chunks += [image(c).reshape(-1), np.full(gap, GUARD, np.uint8)]
            at += image(c).size + gap
    return np.concatenate(chunks), where


def pack_views(cases):
    """ViewCases -> (buffer, int64 [V, 12] descriptor rows)"""
    buf, where = pack_sources(cases)
    rows = np.array([[where[(c.w, c.h, c.content)], c.w, c.h] + [int(t) for t in c.view[:9]] for c in cases], dtype=np.int64).reshape(len(cases), 12)
    return buf, rows


def pack_resize(cases, gap=7):
    """ResizeCases -> (buffer of sources and GUARD-filled destinations with GUARD gaps, int64 [N, 6] frame rows)"""
    buf, where = pack_sources(cases)
    at, rows = buf.size, []
    for c in cases:
        rows.append([where[(c.w, c.h, c.content)], c.w, c.h, at, c.ow, c.oh])
        at += c.ow * c.oh * 3 + gap
    return np.concatenate([buf, np.full(at - buf.size, GUARD, np.uint8)]), np.array(rows, dtype=np.int64).reshape(len(cases), 6)


def pack_adm(cases, gap=3):
    """AdmCases, laid out as preprocess.DeviceLoader lays a batch out (the sources, then each source's halved frames) but with GUARD gaps ->
    (buffer, [the [n, 6] frame rows of each chain depth], int64 [B, 12] BICUBIC view rows that name each source's last frame)"""
    at, chunks, src = 0, [], []
    for c in cases:                                                           # a source per case, shared or not: the chain writes behind all of them
        src.append((at, c.w, c.h))
        chunks += [image(c).reshape(-1), np.full(gap, GUARD, np.uint8)]
        at += image(c).size + gap
    depth, rows = [], []
    for c, s in zip(cases, src):
        frames = adm_numbers(c.w, c.h, c.S)[0]
        for d, (fw, fh) in enumerate(frames[1:]):
            if d == len(depth):
                depth.append([])
            depth[d].append(list(s) + [at, fw, fh])
            s = (at, fw, fh)
            at += fw * fh * 3 + gap
        rows.append(list(s) + list(adm_view(c.w, c.h, c.S)[:9]))
    buf = np.concatenate(chunks + [np.full(at - sum(ch.size for ch in chunks), GUARD, np.uint8)])
    return buf, [np.array(d, dtype=np.int64).reshape(len(d), 6) for d in depth], np.array(rows, dtype=np.int64).reshape(len(cases), 12)


def untouched(buf, regions):
    """is every byte of `buf` outside the (offset, length) regions still GUARD?"""
    mask = np.ones(buf.size, bool)
    for off, n in regions:
        mask[off:off + n] = False
    return bool((buf[mask] == GUARD).all())


def make_golden():
    import PIL
    cases = ADM_CASES + RESIZE_CASES + VIEW_CASES
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([c.name for c in cases]),
           "crc_u8": np.array([crc(expected(c)) for c in cases], np.uint32)}
    out["crc_bf16"] = np.array([0 if isinstance(c, ResizeCase) else crc(IO.to_tensor(expected(c), True)) for c in cases], np.uint32)
    for filt, insz, outsz in ((BICUBIC, 37, 16), (BICUBIC, 16, 37), (BOX, 65, 32), (BOX, 20, 300)):
        xmin, n, k = tables(insz, outsz, 0, outsz, filt)
        out[f"tab_{filt}_{insz}_{outsz}_xmin"], out[f"tab_{filt}_{insz}_{outsz}_n"], out[f"tab_{filt}_{insz}_{outsz}_k"] = xmin.astype(np.int32), n.astype(np.int32), k.astype(np.int32)
    return out


if __name__ == "__main__":
    if "--write-golden" in sys.argv:
        np.savez_compressed(GOLDEN, **make_golden())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
