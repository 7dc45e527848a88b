"""Image pre/post-processing of the reference's user script without torchvision (reference test.py:27-31, 42-43):
Resize(size) [shorter side, bilinear + antialias on PIL images] -> CenterCrop(size) -> NormalizeToTensor, and
`save_image` for the [0,1] outputs of `decoding`."""
from __future__ import annotations

import time
from concurrent.futures import ThreadPoolExecutor
from typing import Iterator, Sequence

import numpy as np
import torch
from PIL import Image

from .pipeline import NormalizeToTensor


def resize_shorter_side(img: Image.Image, size: int) -> Image.Image:
    """torchvision.transforms.Resize(int) on a PIL image: shorter side -> size, aspect kept, bilinear."""
    w, h = img.size
    if (w <= h and w == size) or (h <= w and h == size):
        return img
    if w < h:
        ow, oh = size, int(size * h / w)
    else:
        oh, ow = size, int(size * w / h)
    return img.resize((ow, oh), Image.BILINEAR)


def center_crop(img: Image.Image, size: int) -> Image.Image:
    w, h = img.size
    left, top = int(round((w - size) / 2.0)), int(round((h - size) / 2.0))
    return img.crop((left, top, left + size, top + size))


def load_image(path: str, size: int = 256) -> torch.Tensor:
    """-> float tensor [3,size,size] in [-1,1] (what `SelftokPipeline.encoding` takes, stacked along dim 0)."""
    img = Image.open(path).convert("RGB")
    return NormalizeToTensor()(center_crop(resize_shorter_side(img, size), size))


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
    __slots__ = ("slot", "table", "nbytes", "t_decode", "t_pack")


class DeviceLoader:
    """`load_image` for a whole batch on the GPU: paths or uint8 HWC arrays of any sizes -> [B, 3, size, size] in [-1, 1] on `device`
    (fp32: the values `load_image` returns; bf16: those rounded as `encoding` rounds them), bit for bit.  File decoding stays on the
    host, on at most MAX_DECODE_WORKERS threads; the pixels are packed into a reused pinned staging buffer together with their
    (offset, width, height) table, cross in one asynchronous copy, and one call of ops.image_resize_crop_norm does the rest.
    `batches()` keeps two staging slots so that the host work of batch i + 1 overlaps the copy and the kernels of batch i.
    `load()` stages into slot 0: do not call it while a `batches()` iteration of the SAME loader is under way (it would overwrite a
    staged batch).  Owns two thread pools: `close()` it, use it as a context manager, or let the finaliser do it."""

    def __init__(self, size: int, device, dtype=torch.float32, workers: int = 8):
        self.size, self.device, self.dtype = int(size), torch.device(device), dtype
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

    def _stage(self, items, slot: int) -> _Staged:
        t0 = time.perf_counter()
        arrays = list(self._pool.map(_decode, items)) if self.workers > 1 and len(items) > 1 else [_decode(i) for i in items]
        t1 = time.perf_counter()
        B = len(arrays)
        head = (B * 24 + 63) // 64 * 64                                        # the table travels in front of the pixels
        table = np.empty((B, 3), dtype=np.int64)
        at = 0
        for b, a in enumerate(arrays):
            table[b] = (at, a.shape[1], a.shape[0])
            at += (a.size + 15) // 16 * 16
        need = head + at
        if self._pinned[slot] is None or self._pinned[slot].numel() < need:
            cap = max(need, 1 << 20) * 5 // 4
            self._pinned[slot] = torch.empty(cap, dtype=torch.uint8).pin_memory()
            self._dev[slot] = None
        elif self._copied[slot] is not None:
            self._copied[slot].synchronize()                                   # the copy that last read this slot
        host = self._pinned[slot].numpy()
        host[:B * 24] = table.reshape(-1).view(np.uint8)
        for b, a in enumerate(arrays):
            o = head + int(table[b, 0])
            host[o:o + a.size] = a.reshape(-1)
        st = _Staged()
        st.slot, st.table, st.nbytes, st.t_decode, st.t_pack = slot, table, need, t1 - t0, time.perf_counter() - t1
        return st

    def _launch(self, st: _Staged) -> torch.Tensor:
        from . import ops
        s = st.slot
        B = st.table.shape[0]
        head = (B * 24 + 63) // 64 * 64
        with torch.cuda.device(self.device):
            if self._dev[s] is None or self._dev[s].numel() < self._pinned[s].numel():
                self._dev[s] = torch.empty(self._pinned[s].numel(), dtype=torch.uint8, device=self.device)
            if self.timing:
                e0 = torch.cuda.Event(enable_timing=True)
                e0.record()
            self._dev[s][:st.nbytes].copy_(self._pinned[s][:st.nbytes], non_blocking=True)
            ev = torch.cuda.Event(enable_timing=self.timing)
            ev.record()
            self._copied[s] = ev
            out = ops.image_resize_crop_norm(self._dev[s][head:st.nbytes], st.table, self.size, dtype=self.dtype,
                                             table_dev=self._dev[s][:B * 24].view(torch.int64))
            if self.timing:
                e2 = torch.cuda.Event(enable_timing=True)
                e2.record()
                self.last_events = (e0, ev, e2)
        self.last_times = {"decode_s": st.t_decode, "pack_s": st.t_pack, "bytes": int(st.nbytes)}
        return out

    def load(self, items) -> torch.Tensor:
        """one batch, synchronous on the host side (the GPU work is queued on the current stream)"""
        return self._launch(self._stage(list(items), 0))

    def batches(self, items: Sequence, batch: int) -> Iterator[torch.Tensor]:
        """consecutive batches of `batch` items; while the caller works on batch i, batch i + 1 is decoded and packed into the other slot"""
        items = list(items)
        chunks = [items[i:i + batch] for i in range(0, len(items), batch)]
        fut = self._stager.submit(self._stage, chunks[0], 0) if chunks else None
        for i in range(len(chunks)):
            st = fut.result()
            if i + 1 < len(chunks):
                fut = self._stager.submit(self._stage, chunks[i + 1], (i + 1) & 1)
            yield self._launch(st)
