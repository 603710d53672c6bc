"""Baseline JPEG decoding on the device: the reference's `Image.open(path)` / `cv2.imread(path)` (drone/yolo.py,
get_map*.py, ufpmp_det_eval.py:93), bit for bit what Pillow gives for the same bytes.

The serial part -- markers and Huffman -- runs on the host inside libglsdet_hip (glsdet_jpeg_parse,
glsdet_jpeg_entropy_decode: no HIP call, they work without a GPU); dequantisation, the 8x8 inverse DCT, chroma
upsampling and YCbCr -> RGB run in two HIP kernels (glsdet_jpeg_reconstruct) and leave the uint8 HWC picture that
DronePreprocessor and the UFP first-stage preprocessor take as a device tensor.  What the library refuses (progressive,
CMYK, other sampling factors, ...: include/glsdet_hip.h) goes to Pillow on the host with fallback="pillow", or raises.
EXIF orientation is not applied: Pillow's Image.open does not apply it either."""
from __future__ import annotations

import ctypes as C
import io
import os
from typing import List, Sequence

import numpy as np

from . import _lib
from ._lib import JpegDesc

ORDERS = {"rgb": 0, "bgr": 1}
_SUBSAMPLING = {(1, 1): "4:4:4", (2, 1): "4:2:2", (2, 2): "4:2:0"}


class JpegRefused(ValueError):
    """glsdet_jpeg_parse refused the stream; the text is the library's message."""


def _read(src) -> bytes:
    if isinstance(src, (bytes, bytearray, memoryview)):
        return bytes(src)
    if isinstance(src, (str, os.PathLike)):
        with open(src, "rb") as f:
            return f.read()
    if hasattr(src, "read"):
        return src.read()
    raise TypeError("a JPEG source is bytes, a path or an open binary file, not %s" % type(src).__name__)


def parse(data: bytes) -> JpegDesc:
    """glsdet_jpeg_parse (host only) -> the descriptor; JpegRefused with the library's message for a refused stream."""
    lib = _lib.load()
    d = JpegDesc()
    if lib.glsdet_jpeg_parse(data, len(data), C.byref(d)) < 0:
        raise JpegRefused(lib.glsdet_last_error().decode(errors="replace"))
    return d


def entropy_decode(data: bytes, desc: JpegDesc = None):
    """glsdet_jpeg_entropy_decode (host only) -> (coef int16 [n_blocks, 64] natural order, not dequantised;
    qtab uint16 [3, 64]).  ValueError with the library's message where the entropy-coded data is bad."""
    lib = _lib.load()
    desc = desc or parse(data)
    coef = np.empty((desc.n_blocks, 64), np.int16)
    qtab = np.empty((3, 64), np.uint16)
    if lib.glsdet_jpeg_entropy_decode(data, len(data), C.byref(desc), coef.ctypes.data, qtab.ctypes.data) < 0:
        raise ValueError(lib.glsdet_last_error().decode(errors="replace"))
    return coef, qtab


def geometry(desc: JpegDesc) -> List[int]:
    """The int list torch.ops.glsdet.jpeg_reconstruct takes: width, height, ncomp, hs[3], vs[3]."""
    return [desc.width, desc.height, desc.ncomp] + list(desc.hs) + list(desc.vs)


def desc_from_geometry(geom: Sequence[int]) -> JpegDesc:
    """The descriptor of a geometry list, derived fields filled as glsdet_jpeg_parse fills them (the library checks
    them again and refuses a layout it does not take)."""
    if len(geom) != 9:
        raise ValueError("jpeg geometry is [width, height, ncomp, hs0, hs1, hs2, vs0, vs1, vs2], got %d values" % len(geom))
    d = JpegDesc()
    d.width, d.height, d.ncomp = (int(v) for v in geom[:3])
    for c in range(3):
        d.hs[c], d.vs[c] = int(geom[3 + c]), int(geom[6 + c])
    if d.ncomp in (1, 3) and d.hs[0] >= 1 and d.vs[0] >= 1:
        d.mcus_x = -(-d.width // (8 * d.hs[0]))
        d.mcus_y = -(-d.height // (8 * d.vs[0]))
        for c in range(d.ncomp):
            d.blocks_x[c], d.blocks_y[c] = d.mcus_x * d.hs[c], d.mcus_y * d.vs[c]
        d.n_blocks = sum(d.blocks_x[c] * d.blocks_y[c] for c in range(3))
    return d


class JpegDecoder:
    """JPEG bytes / paths / open files -> uint8 [H, W, 3] tensors on the device.

    fallback="pillow": a stream glsdet_jpeg_parse refuses (progressive, CMYK, a file that is no JPEG, ...) is decoded by
    Pillow on the host and uploaded, so a directory of mixed files works; fallback="raise": the refusal surfaces as
    ValueError with the library's message.  A stream that parses but is bad in its entropy-coded data raises in both
    modes (Pillow fails on such a stream too)."""

    def __init__(self, device: str = "cuda:0", fallback: str = "pillow"):
        if fallback not in ("pillow", "raise"):
            raise ValueError("fallback is 'pillow' or 'raise', got %r" % (fallback,))
        self.lib = _lib.load()
        self.device = device
        self.fallback = fallback
        self._stage = [None, None]          # two pinned int16 buffers: decode picture i+1 while picture i uploads
        self._event = [None, None]
        self._slot = 0

    # ------------------------------------------------------------------ host only
    def probe(self, src) -> dict:
        """size, mode and subsampling of a stream the library takes, read from its markers alone (no GPU needed);
        refused streams: ValueError with the library's message, whatever the fallback."""
        d = parse(_read(src))
        return {"width": d.width, "height": d.height, "size": (d.width, d.height),
                "mode": "L" if d.ncomp == 1 else "RGB",
                "subsampling": None if d.ncomp == 1 else _SUBSAMPLING[(d.hs[0], d.vs[0])],
                "restart_interval": d.restart_interval}

    # ------------------------------------------------------------------ device
    def _device(self):
        import torch
        if not torch.cuda.is_available():
            raise _lib.GlsdetLibraryError("glsdet_amd needs an MI355X visible to PyTorch-ROCm (no CPU fallback)")
        return torch.device(self.device)

    def _staging(self, n: int):
        import torch
        s = self._slot
        self._slot ^= 1
        if self._event[s] is not None:
            self._event[s].synchronize()      # the upload that last read this buffer is done
        if self._stage[s] is None or self._stage[s].numel() < n:
            self._stage[s] = torch.empty(max(n, 1 << 16), dtype=torch.int16, pin_memory=True)
        return s, self._stage[s]

    def _check_out(self, out, h: int, w: int, dev):
        import torch
        if out is None:
            return torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
        if out.dtype != torch.uint8 or tuple(out.shape) != (h, w, 3) or out.device != dev or out.stride(2) != 1 or \
                out.stride(1) != 3 or (h > 1 and out.stride(0) < 3 * w):
            raise ValueError("out must be a uint8 [%d, %d, 3] window on %s whose pixels are contiguous within a row" % (h, w, dev))
        return out

    def _pillow(self, data: bytes, order: str, out, dev):
        import torch
        from PIL import Image
        arr = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
        if order == "bgr":
            arr = arr[:, :, ::-1]
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(dev)
        if out is None:
            return t
        self._check_out(out, arr.shape[0], arr.shape[1], dev).copy_(t)
        return out

    def decode(self, src, order: str = "rgb", out=None):
        """One picture -> uint8 [H, W, 3] on the device, asynchronous on the current stream.  `out` may be a window of a
        larger device buffer ([H, W, 3] view with contiguous pixels): its row stride is honoured and nothing outside the
        window is written."""
        import torch
        if order not in ORDERS:
            raise ValueError("order is 'rgb' or 'bgr', got %r" % (order,))
        data = _read(src)
        try:
            d = parse(data)
        except JpegRefused:
            if self.fallback == "raise":
                raise
            return self._pillow(data, order, out, self._device())
        dev = self._device()
        out = self._check_out(out, d.height, d.width, dev)
        n = d.n_blocks * 64
        slot, stage = self._staging(n + 192)
        if self.lib.glsdet_jpeg_entropy_decode(data, len(data), C.byref(d), stage.data_ptr(), stage.data_ptr() + 2 * n) < 0:
            raise ValueError(self.lib.glsdet_last_error().decode(errors="replace"))
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            buf = torch.empty(n + 192, dtype=torch.int16, device=dev)          # coefficients, then the three tables
            buf.copy_(stage[:n + 192], non_blocking=True)
            self._event[slot] = torch.cuda.Event()
            self._event[slot].record(stream)
            nws = self.lib.glsdet_jpeg_workspace_bytes(C.byref(d))
            ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=dev)
            _lib.check(self.lib.glsdet_jpeg_reconstruct(C.byref(d), buf.data_ptr(), buf.data_ptr() + 2 * n, ws.data_ptr(), nws,
                                                        out.data_ptr(), out.stride(0) if d.height > 1 else 3 * d.width,
                                                        ORDERS[order], stream.cuda_stream), "jpeg_reconstruct")
        return out

    def decode_batch(self, sources: Sequence, order: str = "rgb") -> list:
        """A list of pictures (any sizes): each is entropy-decoded on the host into reused pinned staging, then one
        asynchronous upload and one reconstruct per picture go on the current stream; nothing synchronises except the
        reuse of a staging buffer two pictures later."""
        return [self.decode(s, order) for s in sources]
