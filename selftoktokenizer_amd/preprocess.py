"""Image pre/post-processing of the reference's user script without torchvision (reference test.py:27-31, 42-43):
Resize(size) [shorter side, bilinear + antialias on PIL images] -> CenterCrop(size) -> NormalizeToTensor, and
`save_image` for the [0,1] outputs of `decoding`; the augmented recipes (FiveCrop / TenCrop / resized_crop / hflip on a PIL image) as
*views* -- pure integer geometry (`views_five`, `views_ten`, `view_resized_crop`), their PIL route (`apply_view_pil`) and, through
`DeviceLoader(..., views=fn)`, the same tensors computed on the GPU (csrc/image_views.hip).  Besides the reference's bilinear recipe two others,
chosen per call or per loader (`filter=`, `preprocess=`), never per view: Resize(S, BICUBIC) -> CenterCrop(S), the timm / torchvision evaluation
default, and the ADM protocol `center_crop_adm` (BOX halvings, one BICUBIC resize, floor-divided centre crop) that published ImageNet rFID / PSNR
tables are taken on; on the GPU through csrc/image_filters.hip."""
from __future__ import annotations

import time
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, NamedTuple, Sequence

import numpy as np
import torch
from PIL import Image

from .pipeline import NormalizeToTensor


PREPROCESS = ("reference", "bicubic", "adm")                                # the recipes of DeviceLoader / preprocess_u8 / the tools
_PIL_FILTERS = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "box": Image.BOX}


def _pil_filter(filter):
    """'bilinear' / 'bicubic' / 'box' or a Pillow code -> the Pillow code (the host route hands it to Image.resize as it is)"""
    if isinstance(filter, str):
        if filter.lower() not in _PIL_FILTERS:
            raise ValueError(f"unknown filter {filter!r}: expected one of {sorted(_PIL_FILTERS)} or a Pillow code")
        return _PIL_FILTERS[filter.lower()]
    return int(filter)


def _check_preprocess(preprocess: str) -> str:
    if preprocess not in PREPROCESS:
        raise ValueError(f"preprocess={preprocess!r}: expected one of {PREPROCESS}")
    return preprocess


def resize_shorter_side(img: Image.Image, size: int, filter="bilinear") -> Image.Image:
    """torchvision.transforms.Resize(int, interpolation) on a PIL image: shorter side -> size, aspect kept; bilinear unless `filter` says otherwise."""
    w, h = img.size
    if (w <= h and w == size) or (h <= w and h == size):
        return img
    if w < h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    return img.resize((ow, oh), _pil_filter(filter))


def center_crop(img: Image.Image, size: int) -> Image.Image:
    w, h = img.size
    left, top = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def load_image(path: str, size: int = 256, filter="bilinear") -> torch.Tensor:
    """-> float tensor [3,size,size] in [-1,1] (what `SelftokPipeline.encoding` takes, stacked along dim 0).  filter: Resize's interpolation."""
    img = Image.open(path).convert("RGB")
    return NormalizeToTensor()(center_crop(resize_shorter_side(img, size, filter), size))


# ---- the ADM protocol (guided-diffusion's center_crop_arr; the evaluation scripts of DiT, LlamaGen, VAR, MAR use it) ----
MAX_ADM_HALVINGS = 8


def center_crop_adm(img: Image.Image, S: int) -> Image.Image:
    """the published `center_crop_arr` on PIL, the route of record: halve with BOX while the shorter side is >= 2 S, one BICUBIC resize by
    S / shorter side (Python's round), centre crop at (side - S) // 2"""
    while min(*img.size) >= 2 * S:
        img = img.resize(tuple(x // 2 for x in img.size), resample=Image.BOX)
    scale = S / min(*img.size)
    img = img.resize(tuple(round(x * scale) for x in img.size), resample=Image.BICUBIC)
    a = np.array(img)
    top, left = (a.shape[0] - S) // 2, (a.shape[1] - S) // 2
    return Image.fromarray(a[top:top + S, left:left + S])


def load_image_adm(path: str, S: int = 256) -> torch.Tensor:
    """`load_image` with the ADM protocol in place of Resize -> CenterCrop"""
    return NormalizeToTensor()(center_crop_adm(Image.open(path).convert("RGB"), S))


class AdmPlan(NamedTuple):
    """`center_crop_adm` as numbers: frames = [(w, h), (w // 2, h // 2), ...], the source and each BOX halving; (rw, rh) what the last frame is
    resized to with BICUBIC; (left, top) the crop's origin, by floor division (`center_crop` rounds half to even instead)"""
    frames: tuple
    rw: int
    rh: int
    left: int
    top: int


def adm_plan(w: int, h: int, S: int) -> AdmPlan:
    w, h, S = int(w), int(h), int(S)
    if w < 1 or h < 1 or S < 1:
        raise ValueError(f"adm_plan: a {w} x {h} image and S = {S}: every one must be at least 1")
    frames = [(w, h)]
    while min(w, h) >= 2 * S:
        w, h = w // 2, h // 2
        frames.append((w, h))
    if len(frames) - 1 > MAX_ADM_HALVINGS:
        raise ValueError(f"adm_plan: a {frames[0][0]} x {frames[0][1]} image takes {len(frames) - 1} halvings to reach S = {S}; at most {MAX_ADM_HALVINGS} are served")
    scale = S / min(w, h)
    rw, rh = round(w * scale), round(h * scale)
    return AdmPlan(tuple(frames), rw, rh, (rw - S) // 2, (rh - S) // 2)


def view_adm(plan: AdmPlan, S: int) -> View:
    """the last frame of an ADM chain -> its S x S output, as a view (to be resampled with BICUBIC)"""
    w, h = plan.frames[-1]
    return View(0, 0, w, h, plan.rw, plan.rh, plan.left, plan.top, 0, S)


# ---- views: torchvision's five / ten-crop, resized_crop and hflip on a PIL image, as numbers (csrc/image_views.hip) ----
class View(NamedTuple):
    """one size x size output of one w x h source: source.crop((x0, y0, x0 + bw, y0 + bh)) -> resize to (rw, rh) unless that is (bw, bh) ->
    crop((left, top, left + size, top + size)) -> FLIP_LEFT_RIGHT if flip.  Pure integers: nothing here draws a random number."""
    x0: int
    y0: int
    bw: int
    bh: int
    rw: int
    rh: int
    left: int
    top: int
    flip: int
    size: int


def _resized_size(w: int, h: int, size: int):
    """the size `resize_shorter_side` gives"""
    if (w <= h and w == size) or (h <= w and h == size):
        return w, h
    return (size, int(size * h / w)) if w < h else (int(size * w / h), size)


def _centre(side: int, size: int) -> int:
    return int(round((side - size) / 2.0))                                    # `center_crop`: Python's round, half to even


def view_center(w: int, h: int, S: int) -> View:
    """`load_image`'s geometry: Resize(S) -> CenterCrop(S)"""
    rw, rh = _resized_size(w, h, S)
    return View(0, 0, w, h, rw, rh, _centre(rw, S), _centre(rh, S), 0, S)


def views_five(w: int, h: int, R: int, S: int) -> list:
    """Resize(R) -> FiveCrop(S) in torchvision's order: top left, top right, bottom left, bottom right, centre"""
    rw, rh = _resized_size(w, h, R)
    if rw < S or rh < S:
        raise ValueError(f"five-crop of {S} from a {w} x {h} image resized to {rw} x {rh}: the crop is larger than the image")
    at = [(0, 0), (rw - S, 0), (0, rh - S), (rw - S, rh - S), (_centre(rw, S), _centre(rh, S))]
    return [View(0, 0, w, h, rw, rh, left, top, 0, S) for left, top in at]


def views_ten(w: int, h: int, R: int, S: int) -> list:
    """Resize(R) -> TenCrop(S): the five crops, then the five crops of the MIRRORED resized image.  A window at `left` of the mirrored image
    is the mirror image of the window at rw - S - left: view 5 is the mirrored top-right window, and so on."""
    five = views_five(w, h, R, S)
    return five + [v._replace(left=v.rw - S - v.left, flip=1) for v in five]


def view_resized_crop(w: int, h: int, box, S: int, flip: bool = False) -> View:
    """torchvision's resized_crop (what RandomResizedCrop applies once it has drawn `box` = (x0, y0, bw, bh)): the box becomes S x S,
    each axis by its own ratio; `flip`: followed by hflip"""
    x0, y0, bw, bh = (int(v) for v in box)
    if bw < 1 or bh < 1 or x0 < 0 or y0 < 0 or x0 + bw > w or y0 + bh > h:
        raise ValueError(f"box {tuple(box)} is empty or outside the {w} x {h} image")
    return View(x0, y0, bw, bh, S, S, 0, 0, int(bool(flip)), S)


def mirrored(views) -> list:
    """the views and then the mirror image of each"""
    views = list(views)
    return views + [v._replace(flip=1 - v.flip) for v in views]


def apply_view_pil(img, view, to_tensor: bool = True, filter="bilinear"):
    """the host route of one view with live Pillow; `img`: a PIL image or a uint8 [H, W, 3] array.  -> NormalizeToTensor's [3, size, size]
    fp32 tensor, or with to_tensor=False the PIL image itself.  filter: the resample's ('bilinear', 'bicubic', 'box' or a Pillow code)"""
    v = View(*view)
    S = v.size
    im = img if isinstance(img, Image.Image) else Image.fromarray(np.asarray(img))
    im = im.crop((v.x0, v.y0, v.x0 + v.bw, v.y0 + v.bh))
    if (v.rw, v.rh) != (v.bw, v.bh):
        im = im.resize((v.rw, v.rh), _pil_filter(filter))
    im = im.crop((v.left, v.top, v.left + S, v.top + S))
    if v.flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return NormalizeToTensor()(im) if to_tensor else im


def view_rows(views_per_source, size: int) -> np.ndarray:
    """one list of views per source -> the int64 [sum of views, 10] table of ops.image_views (source index, x0, y0, bw, bh, rw, rh, left, top,
    flip), in source order and then view order; every view must be a `size` one"""
    rows = []
    for n, vs in enumerate(views_per_source):
        for v in vs:
            v = View(*v)
            if v.size != size:
                raise ValueError(f"a view of size {v.size} in a batch of size {size}")
            rows.append((n,) + tuple(int(x) for x in v[:9]))
    return np.array(rows, dtype=np.int64).reshape(len(rows), 10)


def save_image(img: torch.Tensor, path: str) -> None:
    """[3,H,W] in [0,1] (any float dtype/device) -> 8-bit file with torchvision.utils.save_image's arithmetic:
    `mul(255).add_(0.5).clamp_(0, 255)` evaluated IN THE TENSOR'S OWN DTYPE (the reference passes the bf16 output of `decoding`
    straight to torchvision, test.py:42-43, so the x*255+0.5 rounding happens in bf16), then truncation to uint8."""
    a = img.detach().cpu().clone().mul_(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(torch.uint8).numpy()
    Image.fromarray(a).save(path)


def save_images(recons: torch.Tensor, paths: Sequence[str]) -> None:
    """[B,3,H,W] in [0,1] on the GPU -> one 8-bit file per image, the bytes `save_image` writes: the conversion runs on the device
    (ops.image_to_u8) and the batch comes to the host in ONE copy."""
    from . import ops
    if len(paths) != recons.shape[0]:
        raise ValueError(f"{recons.shape[0]} images but {len(paths)} paths")
    with torch.cuda.device(recons.device):
        a = ops.image_to_u8(recons.detach()).cpu().numpy()
    for img, p in zip(a, paths):
        Image.fromarray(img).save(p)


MAX_DECODE_WORKERS = 16


def _decode(item) -> np.ndarray:
    """a path -> RGB uint8 HWC (the host part of `load_image`); an array is checked and passed on"""
    if isinstance(item, (str, bytes)) or hasattr(item, "__fspath__"):
        return np.asarray(Image.open(item).convert("RGB"))
    a = np.asarray(item)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"expected a uint8 [H, W, 3] array, got {a.dtype} {a.shape}")
    return a


class _Staged:
    __slots__ = ("slot", "table", "rows", "chain", "nbytes", "copied", "t_decode", "t_pack")


class DeviceLoader:
    """`load_image` for a whole batch on the GPU: paths or uint8 HWC arrays of any sizes -> [B, 3, size, size] in [-1, 1] on `device`
    (fp32: the values `load_image` returns; bf16: those rounded as `encoding` rounds them), bit for bit.  File decoding stays on the
    host, on at most MAX_DECODE_WORKERS threads; the pixels are packed into a reused pinned staging buffer together with their
    (offset, width, height) table, cross in one asynchronous copy, and one call of ops.image_resize_crop_norm does the rest.
    `batches()` keeps two staging slots so that the host work of batch i + 1 overlaps the copy and the kernels of batch i.
    `views=fn` (load and batches): fn(width, height) -> a list of `View`s of this loader's size (views_five, views_ten, view_resized_crop, ...);
    the output is then [sum of views, 3, size, size], in item order and then view order, through ops.image_views -- every source still crosses
    once.  views=None is the centre crop through ops.image_resize_crop_norm.
    `preprocess`: "reference" (the above, untouched); "bicubic": Resize(size, BICUBIC) -> CenterCrop(size), and with views=fn the views resampled
    with BICUBIC (ops.image_views(filter="bicubic")); "adm": `center_crop_adm` -- behind the sources the device buffer has room for each source's BOX
    halvings (at most a third more bytes; made on the device, so the copy does not carry them), one ops.image_resize call per chain depth over the sources
    that still need a halving, then one ops.image_views(filter="bicubic") call whose rows name each source's last frame.  views= with "adm" is
    refused: the protocol is a single centre crop.
    `load()` stages into slot 0: do not call it while a `batches()` iteration of the SAME loader is under way (it would overwrite a
    staged batch).  Owns two thread pools: `close()` it, use it as a context manager, or let the finaliser do it."""

    def __init__(self, size: int, device, dtype=torch.float32, workers: int = 8, preprocess: str = "reference"):
        self.size, self.device, self.dtype = int(size), torch.device(device), dtype
        self.preprocess = _check_preprocess(preprocess)
        if self.device.type != "cuda":
            raise ValueError(f"DeviceLoader needs a GPU device, got {self.device}")
        self.workers = max(1, min(int(workers), MAX_DECODE_WORKERS))
        self._pool = ThreadPoolExecutor(max_workers=self.workers)
        self._stager = ThreadPoolExecutor(max_workers=1)
        self._pinned = [None, None]          # host staging, one per slot
        self._dev = [None, None]             # its device twin
        self._copied = [None, None]          # event: the slot's last host -> device copy has completed
        self.timing = False                  # True: `last_events` = HIP events (before the copy, after it, after the kernels) of the last batch
        self.last_times, self.last_events = {}, None

    def close(self):
        self._pool.shutdown(wait=True)
        self._stager.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self._pool.shutdown(wait=False)
            self._stager.shutdown(wait=False)
        except Exception:                                                       # interpreter shutdown / half-built object
            pass

    def _stage(self, items, slot: int, views=None) -> _Staged:
        if views is not None and self.preprocess == "adm":
            raise ValueError('DeviceLoader(preprocess="adm") takes no views: the ADM protocol is one centre crop per image')
        t0 = time.perf_counter()
        arrays = list(self._pool.map(_decode, items)) if self.workers > 1 and len(items) > 1 else [_decode(i) for i in items]
        t1 = time.perf_counter()
        B = len(arrays)
        table = np.empty((B, 3), dtype=np.int64)
        plans = [adm_plan(a.shape[1], a.shape[0], self.size) for a in arrays] if self.preprocess == "adm" else None
        last = np.empty((B, 3), dtype=np.int64)                                 # "adm": the last frame of each source's chain
        depth = [[] for _ in range(MAX_ADM_HALVINGS)]                           # "adm": the [n, 6] frame rows of each chain depth
        at = 0
        for b, a in enumerate(arrays):
            table[b] = (at, a.shape[1], a.shape[0])
            at += (a.size + 15) // 16 * 16
        copied = at                                                             # what crosses to the device: the tables and the sources
        for b in range(B if plans is not None else 0):                          # room for the halved frames behind the sources, source by source
            src = tuple(int(v) for v in table[b])
            for d, (fw, fh) in enumerate(plans[b].frames[1:]):
                depth[d].append(src + (at, fw, fh))
                src = (at, fw, fh)
                at += (fw * fh * 3 + 15) // 16 * 16
            last[b] = src
        rows, chain = None, []
        if views is not None or self.preprocess != "reference":
            from . import ops
            if plans is not None:
                rows = ops.image_view_rows(last, view_rows([[view_adm(p, self.size)] for p in plans], self.size))
                chain = [np.array(d, dtype=np.int64).reshape(len(d), 6) for d in depth if d]
            else:
                per = views if views is not None else (lambda w, h: [view_center(w, h, self.size)])
                rows = ops.image_view_rows(table, view_rows([per(a.shape[1], a.shape[0]) for a in arrays], self.size))   # built once; _launch hands them on
        front = table if rows is None else rows                                 # the tables the kernels read travel in front of the pixels
        if chain:
            front = np.concatenate([rows.reshape(-1)] + [c.reshape(-1) for c in chain])
        head = (front.size * 8 + 63) // 64 * 64
        need = head + at
        if self._pinned[slot] is None or self._pinned[slot].numel() < need:
            cap = max(need, 1 << 20) * 5 // 4
            self._pinned[slot] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._dev[slot] = None
        elif self._copied[slot] is not None:
            self._copied[slot].synchronize()                                   # the copy that last read this slot
        host = self._pinned[slot].numpy()
        host[:front.size * 8] = front.reshape(-1).view(np.uint8)
        for b, a in enumerate(arrays):
            o = head + int(table[b, 0])
            host[o:o + a.size] = a.reshape(-1)
        st = _Staged()
        st.slot, st.table, st.rows, st.chain, st.nbytes, st.copied, st.t_decode, st.t_pack = slot, table, rows, chain, need, head + copied, t1 - t0, time.perf_counter() - t1
        return st

    def _launch(self, st: _Staged) -> torch.Tensor:
        from . import ops
        s = st.slot
        front = st.table if st.rows is None else st.rows
        longs = front.size + sum(c.size for c in st.chain)
        head = (longs * 8 + 63) // 64 * 64
        with torch.cuda.device(self.device):
            if self._dev[s] is None or self._dev[s].numel() < self._pinned[s].numel():
                self._dev[s] = torch.empty(self._pinned[s].numel(), dtype=torch.uint8, device=self.device)
            if self.timing:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            self._dev[s][:st.copied].copy_(self._pinned[s][:st.copied], non_blocking=True)
            ev = torch.cuda.Event(enable_timing=self.timing)
            ev.record()
            self._copied[s] = ev
            front_dev = self._dev[s][:front.size * 8].view(torch.int64)
            if st.rows is None:
                out = ops.image_resize_crop_norm(self._dev[s][head:st.nbytes], st.table, self.size, dtype=self.dtype, table_dev=front_dev)
            else:
                lo = front.size
                for c in st.chain:                                              # depth by depth: frame d of every source that has one, from its frame d - 1
                    ops.image_resize(self._dev[s][head:st.nbytes], c, "box", frames_dev=self._dev[s][lo * 8:(lo + c.size) * 8].view(torch.int64))
                    lo += c.size
                out = ops.image_views(self._dev[s][head:st.nbytes], None, None, self.size, dtype=self.dtype, rows=st.rows, rows_dev=front_dev,
                                      filter="bilinear" if self.preprocess == "reference" else "bicubic")
            if self.timing:
                e2 = torch.cuda.Event(enable_timing=True)
                e2.record()
                self.last_events = (e0, ev, e2)
        self.last_times = {"decode_s": st.t_decode, "pack_s": st.t_pack, "bytes": int(st.copied)}
        return out

    def load(self, items, views=None) -> torch.Tensor:
        """one batch, synchronous on the host side (the GPU work is queued on the current stream)"""
        return self._launch(self._stage(list(items), 0, views))

    def batches(self, items: Sequence, batch: int, views=None) -> Iterator[torch.Tensor]:
        """consecutive batches of `batch` items; while the caller works on batch i, batch i + 1 is decoded and packed into the other slot"""
        items = list(items)
        chunks = [items[i:i + batch] for i in range(0, len(items), batch)]
        fut = self._stager.submit(self._stage, chunks[0], 0, views) if chunks else None
        for i in range(len(chunks)):
            st = fut.result()
            if i + 1 < len(chunks):
                fut = self._stager.submit(self._stage, chunks[i + 1], (i + 1) & 1, views)
            yield self._launch(st)
