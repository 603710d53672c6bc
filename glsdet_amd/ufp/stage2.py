"""Device side of the UFPMP-Det second stage and the two-stage driver (ufp/ufpmp_det_eval.py:253-300):

    coarse detector -> unified foreground packing (host, packing.py, or glsdet_ufp_pack on the device) -> mosaic of
    magnified crops (glsdet_ufp_mosaic) -> mmdet test pipeline (glsdet_resize_normalize_pad) -> fine detector ->
    back-mapping + per-class merge NMS (glsdet_ufp_backmap_merge).

Only the chip list (a few hundred floats) and the final detections cross the PCIe bus; the source
image, the mosaic and both network inputs stay in HBM.  With packing="device" the coarse detections and the chip list
stay there too: 32 bytes (box count, chip count, canvas extents) come back between the two stages."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .. import _lib
from .packing import unified_foreground_packing

MEAN_RGB = (123.675, 116.28, 103.53)            # img_norm_cfg of configs/UFPMP-Det/*.py
STD_RGB = (58.395, 57.12, 57.375)


class DevicePacking:
    """Result of UfpSecondStage.pack: the chip list in HBM.  chips_floor fp32 [max_det,7] is what mosaic / merge read
    (n_chips rows are valid); n_boxes, n_chips, canvas_w, canvas_h come from the one header readback; .chips reads the
    exact float64 list back on first use."""

    def __init__(self, chips_exact: torch.Tensor, chips_floor: torch.Tensor, header: Sequence[float]):
        self._exact, self.chips_floor = chips_exact, chips_floor
        self.n_boxes, self.n_chips = int(header[0]), int(header[1])
        self.canvas_w, self.canvas_h = float(header[2]), float(header[3])
        self._chips = None

    def __len__(self):
        return self.n_chips

    @property
    def chips(self) -> List[List[float]]:
        if self._chips is None:
            self._chips = self._exact[: self.n_chips].cpu().numpy().tolist()
        return self._chips


def _check_packing_mode(packing: str) -> str:
    if packing not in ("host", "device"):
        raise ValueError("packing must be 'host' or 'device', not %r" % (packing,))
    return packing


def rescale_size(old_wh: Tuple[int, int], scale: Tuple[int, int]) -> Tuple[int, int]:
    """mmcv.rescale_size for a (long edge, short edge) tuple: keep the aspect ratio."""
    w, h = old_wh
    f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(f) + 0.5), int(h * float(f) + 0.5)


class UfpSecondStage:
    def __init__(self, device: str = "cuda:0", img_scale: Tuple[int, int] = (1333, 800), size_divisor: int = 32,
                 mean_rgb: Sequence[float] = MEAN_RGB, std_rgb: Sequence[float] = STD_RGB):
        self.lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GlsdetLibraryError("glsdet_amd needs an MI355X visible to PyTorch-ROCm (no CPU fallback)")
        self.device = torch.device(device)
        self.img_scale, self.div = tuple(img_scale), size_divisor
        self._mean = (C.c_double * 3)(*mean_rgb)
        self._std = (C.c_double * 3)(*std_rgb)

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    # ---- UnifiedForegroundPacking on the coarse detector's buffers, unified_foreground_packing.py:6-197
    def pack(self, dets: torch.Tensor, count: torch.Tensor, image_wh: Sequence[int], expand: float = 1.5) -> DevicePacking:
        """dets fp32 [max_det,7] / count int32 on the device (the coarse detector's buffers for ONE image), image_wh =
        (width, height) of the source image -> DevicePacking.  One kernel on the current stream, then the 32-byte header
        readback (the only device-to-host copy)."""
        if dets.dtype != torch.float32 or dets.dim() != 2 or dets.shape[1] != 7 or not dets.is_contiguous():
            raise ValueError("pack: dets must be a contiguous fp32 [max_det, 7] tensor")
        if count.dtype != torch.int32 or not count.is_contiguous() or count.numel() < 1:
            raise ValueError("pack: count must be a contiguous int32 tensor")
        max_det = int(dets.shape[0])
        exact = torch.empty(max_det, 7, dtype=torch.float64, device=self.device)
        floor = torch.empty(max_det, 7, dtype=torch.float32, device=self.device)
        header = torch.empty(4, dtype=torch.float64, device=self.device)
        status = torch.empty(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.glsdet_ufp_pack(dets.data_ptr(), count.data_ptr(), 1, max_det, float(expand), int(image_wh[0]),
                                            int(image_wh[1]), exact.data_ptr(), floor.data_ptr(), header.data_ptr(),
                                            status.data_ptr(), self._stream()), "ufp_pack")
        host = header.cpu().tolist()
        if not 0 <= host[0] <= max_det:          # status bit 0: the header then carries the count as it was read
            raise RuntimeError("pack: the detection count %d lies outside [0, max_det=%d]" % (int(host[0]), max_det))
        return DevicePacking(exact, floor, host)

    def _chips_on_device(self, chips):
        """-> (tensor that keeps the chips alive or None, device pointer or None, n_chips)"""
        if isinstance(chips, DevicePacking):
            return chips.chips_floor, (chips.chips_floor.data_ptr() if chips.n_chips else None), chips.n_chips
        n = len(chips)
        # the reference floors every chip field with math.floor on Python floats (ufpmp_det_eval.py:283): floor in
        # float64 on the host, so a value just below an integer cannot round up on its way to float32
        cdev = torch.tensor(np.floor(np.asarray(chips, np.float64)).astype(np.float32).reshape(-1, 7), device=self.device) if n else None
        return cdev, (cdev.data_ptr() if n else None), n

    # ---- display_merge_result, ufpmp_det_eval.py:182-193
    def mosaic(self, img_bgr: torch.Tensor, chips, width: float, height: float) -> torch.Tensor:
        """img_bgr: uint8 [H,W,3] on the device; chips: a host chip list or a DevicePacking (no upload)
        -> fp32 canvas [ceil(height), ceil(width), 3]."""
        assert img_bgr.dtype == torch.uint8 and img_bgr.dim() == 3 and img_bgr.shape[2] == 3 and img_bgr.is_contiguous()
        ch, cw = max(1, math.ceil(height)), max(1, math.ceil(width))
        canvas = torch.empty(ch, cw, 3, dtype=torch.float32, device=self.device)
        cdev, cptr, n = self._chips_on_device(chips)
        _lib.check(self.lib.glsdet_ufp_mosaic(img_bgr.data_ptr(), img_bgr.shape[0], img_bgr.shape[1],
                                              cptr, n, canvas.data_ptr(), ch, cw, self._stream()),
                   "ufp_mosaic")
        torch.cuda.current_stream().synchronize()
        return canvas

    # ---- Resize(keep_ratio) -> Normalize(to_rgb) -> Pad -> ImageToTensor
    FLIP_CODES = {None: 0, "horizontal": 1, "vertical": 2, "diagonal": 3}      # mmcv.imflip's directions

    def pipeline_input(self, img_bgr: torch.Tensor, img_scale=None, flip=None):
        """HWC BGR image on the device -> (fp32 [1,3,ph,pw], meta dict as mmdet's img_metas).
        uint8 (a decoded frame, the first stage): cv2's uint8 fixed-point resize, rounded to uint8 before
        Normalize; float32 (the mosaic, a float array in the reference): float bilinear.
        img_scale: another (long edge, short edge) than the stage's; flip: None / False, or 'horizontal' / 'vertical' /
        'diagonal' -- RandomFlip mirrors the resized picture before Normalize and Pad (transforms.py:457-461), so the
        padding stays at the right and the bottom and scale_factor / img_shape are those of the unflipped call."""
        assert img_bgr.dtype in (torch.float32, torch.uint8) and img_bgr.is_contiguous() and img_bgr.dim() == 3
        flip = flip or None
        if flip not in self.FLIP_CODES:
            raise ValueError("flip must be None, 'horizontal', 'vertical' or 'diagonal', not %r" % (flip,))
        h, w = int(img_bgr.shape[0]), int(img_bgr.shape[1])
        nw, nh = rescale_size((w, h), self.img_scale if img_scale is None else tuple(img_scale))
        ph, pw = int(math.ceil(nh / self.div)) * self.div, int(math.ceil(nw / self.div)) * self.div
        out = torch.empty(1, 3, ph, pw, dtype=torch.float32, device=self.device)
        fn = self.lib.glsdet_resize_normalize_pad_ex if img_bgr.dtype == torch.float32 else self.lib.glsdet_resize_normalize_pad_u8_ex
        _lib.check(fn(img_bgr.data_ptr(), h, w, nh, nw, out.data_ptr(), ph, pw, self._mean, self._std, self.FLIP_CODES[flip],
                      self._stream()), "resize_normalize_pad")
        torch.cuda.current_stream().synchronize()
        sf = np.array([nw / w, nh / h, nw / w, nh / h], dtype=np.float32)
        return out, dict(img_shape=(nh, nw, 3), pad_shape=(ph, pw, 3), ori_shape=(h, w, 3), scale_factor=sf,
                         flip=flip is not None, flip_direction=flip)

    # ---- back-mapping + merge NMS, ufpmp_det_eval.py:282-300
    def merge(self, dets: torch.Tensor, count: torch.Tensor, chips, num_classes: int,
              iof_thr: float = 0.9, nms_thr: float = 0.6, max_cand: int = 4096) -> List[np.ndarray]:
        """dets [max_det,7] fp32 / count int32 on the device (the fine detector's buffers for ONE image); chips: a host
        chip list or a DevicePacking (no upload)
        -> per class ndarray (k,5) x1,y1,x2,y2,score in source-image coordinates, NMS order."""
        max_det = int(dets.shape[0])
        cdev, cptr, n = self._chips_on_device(chips)
        ws = torch.zeros(int(self.lib.glsdet_ufp_merge_workspace_bytes(max_cand)) + 256, dtype=torch.uint8, device=self.device)
        off = (-ws.data_ptr()) % 256
        out = torch.zeros(max_cand, 7, dtype=torch.float32, device=self.device)
        cnt = torch.zeros(2, dtype=torch.int32, device=self.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.glsdet_ufp_backmap_merge(dets.data_ptr(), count.data_ptr(), max_det, cptr, n,
                                                     iof_thr, nms_thr, max_cand, max_cand, out.data_ptr(), cnt.data_ptr(),
                                                     status.data_ptr(), ws.data_ptr() + off, ws.numel() - off, self._stream()),
                   "ufp_backmap_merge")
        k = int(cnt[0].item())
        if int(status.item()) & 1:
            raise RuntimeError("more than max_cand=%d (chip, detection) matches" % max_cand)
        rows = out[:k].cpu().numpy()
        labels = rows[:, 6].astype(np.int64)
        return [rows[labels == c][:, :5].astype(np.float64) for c in range(num_classes)]


def _coarse_on_device(coarse, x1, m1, cfg: dict, use_graph: bool, instance: int = 0):
    """HipGflDetector.detect without its collect: the same plan (same cache key) is run and its buffers stay in HBM."""
    post = dict(score_thr=cfg.get("score_thr", 0.05), iou_thr=cfg.get("iou_thr", 0.6), nms_pre=cfg.get("nms_pre", 1000),
                max_per_img=cfg.get("max_per_img", 100), rescale=True)
    c = coarse.compile(1, x1.shape[2], x1.shape[3], post, use_graph=use_graph, instance=instance)
    dev = c.img.device
    coarse.run(c, x1.to(dev, torch.float32), torch.tensor([[m1["img_shape"][0], m1["img_shape"][1]]], dtype=torch.float32).to(dev),
               torch.tensor(np.asarray(m1["scale_factor"], np.float32).reshape(1, 4)).to(dev))
    return c


def _pack_on_device(stage, c, image_wh, expand):
    pk = stage.pack(c.nb["dets"][0], c.nb["count"], image_wh, expand)
    # the stream is idle after the header readback: the capacity word of the coarse plan costs no second wait
    if int(c.nb["status"].item()) & 1:
        raise RuntimeError("GFL candidate capacity exceeded on a level (raise max_cand)")
    return pk


def two_stage_detect(coarse, fine, img_bgr_u8, stage: UfpSecondStage, coarse_cfg: dict, fine_cfg: dict,
                     expand: float = 1.5, use_graph: bool = False, packing: str = "host"):
    """One image through coarse -> UFP -> mosaic -> fine -> merge (ufpmp_det_eval.py:253-300).
    coarse / fine: glsdet_amd.resdet.HipGflDetector; *_cfg: dict(score_thr, iou_thr, nms_pre, max_per_img).
    packing: "host" (packing.py on the collected detections) or "device" (glsdet_ufp_pack on the coarse plan's buffers;
    the intermediates then hold `packing`, a DevicePacking, and `coarse_compiled` in place of `first`).
    -> (per class ndarray (k,5) in source-image coordinates, intermediates dict)."""
    _check_packing_mode(packing)
    img = torch.as_tensor(np.ascontiguousarray(img_bgr_u8)).to(stage.device)
    H, W = int(img.shape[0]), int(img.shape[1])
    x1, m1 = stage.pipeline_input(img)                                # uint8 frame: cv2 uint8 resize
    if packing == "device":
        c1 = _coarse_on_device(coarse, x1, m1, coarse_cfg, use_graph)
        pk = _pack_on_device(stage, c1, (W, H), expand)
        if pk.n_boxes == 0:
            return [np.zeros((0, 5)) for _ in range(fine.num_classes)], dict(chips=[], packing=pk, coarse_compiled=c1)
        canvas = stage.mosaic(img, pk, pk.canvas_w, pk.canvas_h)
        merged, c, m2 = _fine_and_merge(fine, stage, canvas, pk, fine_cfg, use_graph)
        return merged, dict(packing=pk, canvas=canvas, coarse_compiled=c1, fine_compiled=c, meta2=m2,
                            canvas_wh=(pk.canvas_w, pk.canvas_h))
    first = coarse.detect(x1, img_shapes=[m1["img_shape"]], scale_factors=[m1["scale_factor"]], use_graph=use_graph, **coarse_cfg)[0]
    order = np.argsort(first[1], kind="stable")                     # np.concatenate(first_results): class-major
    boxes = first[0][order][:, :4]
    if len(boxes) == 0:
        return [np.zeros((0, 5)) for _ in range(fine.num_classes)], dict(chips=[], first=first)
    chips, cw, ch = unified_foreground_packing(boxes.copy(), expand, [W, H])
    canvas = stage.mosaic(img, chips, cw, ch)
    merged, c, m2 = _fine_and_merge(fine, stage, canvas, chips, fine_cfg, use_graph)
    return merged, dict(chips=chips, canvas=canvas, first=first, fine_compiled=c, meta2=m2, canvas_wh=(cw, ch))


def _fine_and_merge(fine, stage, canvas, chips, fine_cfg, use_graph, instance: int = 0):
    """mosaic -> test pipeline -> fine detector -> back-mapping + merge NMS; chips: host list or DevicePacking"""
    x2, m2 = stage.pipeline_input(canvas)
    post = dict(score_thr=fine_cfg["score_thr"], iou_thr=fine_cfg["iou_thr"], nms_pre=fine_cfg.get("nms_pre", 1000),
                max_per_img=fine_cfg.get("max_per_img", 500), rescale=True)
    c = fine.compile(1, x2.shape[2], x2.shape[3], post, use_graph=use_graph, instance=instance)
    fine.run(c, x2, torch.tensor([[m2["img_shape"][0], m2["img_shape"][1]]], dtype=torch.float32, device=stage.device),
             torch.tensor(m2["scale_factor"].reshape(1, 4), device=stage.device))
    return stage.merge(c.nb["dets"][0], c.nb["count"], chips, fine.num_classes), c, m2


class TwoStagePipeline:
    """BASELINE config 5: coarse and fine detector pipelined on separate HIP streams.  `workers` lanes,
    each a pair of host threads with their own streams and their own plan instances (private activation
    buffers): one thread runs preprocessing + coarse detector + packing for its next frame while the other
    runs mosaic + fine detector + merge for its previous one (the host waits of a stage release the GIL,
    the recorded plans are per thread).  Frame i goes to lane i % workers; results come back in order.
    At batch 1 neither detector fills the chip, so several frames in flight is where the throughput is
    (tools/two_stage_bench.py)."""

    def __init__(self, coarse, fine, stage: UfpSecondStage, coarse_cfg: dict, fine_cfg: dict, expand: float = 1.5,
                 depth: int = 2, use_graph: bool = False, workers: int = 1, packing: str = "host"):
        self.coarse, self.fine, self.stage = coarse, fine, stage
        # "device": glsdet_ufp_pack on the lane's coarse buffers; the producer hands a DevicePacking to the consumer
        self.packing = _check_packing_mode(packing)
        self.coarse_cfg, self.fine_cfg, self.expand, self.depth = coarse_cfg, fine_cfg, expand, depth
        # use_graph: one captured plan per input shape.  Measured (tools/two_stage_bench.py, 540x1024 frames): at batch 1
        # the stages are GPU bound, graph replay gains nothing sequentially (180 frames/s either way) and LOSES the
        # overlap of the two threads (185 vs 280 frames/s with eager plans), so it is off by default.
        self.use_graph = use_graph
        self.workers = max(1, int(workers))

    def _first(self, img_bgr_u8, lane: int = 0):
        st = self.stage
        img = torch.as_tensor(np.ascontiguousarray(img_bgr_u8)).to(st.device)
        H, W = int(img.shape[0]), int(img.shape[1])
        x1, m1 = st.pipeline_input(img)
        if self.packing == "device":
            pk = _pack_on_device(st, _coarse_on_device(self.coarse, x1, m1, self.coarse_cfg, self.use_graph, lane), (W, H), self.expand)
            return img, (None if pk.n_boxes == 0 else (pk, pk.canvas_w, pk.canvas_h))
        first = self.coarse.detect(x1, img_shapes=[m1["img_shape"]], scale_factors=[m1["scale_factor"]], use_graph=self.use_graph,
                                   instance=lane, **self.coarse_cfg)[0]
        order = np.argsort(first[1], kind="stable")
        boxes = first[0][order][:, :4]
        if len(boxes) == 0:
            return img, None
        return img, unified_foreground_packing(boxes.copy(), self.expand, [W, H])

    def _second(self, img, packed, lane: int = 0):
        st, fine = self.stage, self.fine
        if packed is None:
            return [np.zeros((0, 5)) for _ in range(fine.num_classes)]
        chips, cw, ch = packed                      # chips: a host list, or the producer's DevicePacking
        return _fine_and_merge(fine, st, st.mosaic(img, chips, cw, ch), chips, self.fine_cfg, self.use_graph, lane)[0]

    def run(self, images: Sequence) -> List[List[np.ndarray]]:
        import queue
        import threading
        results: List = [None] * len(images)
        errors: List[BaseException] = []
        dev = self.stage.device

        def producer(lane, q):
            try:
                with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                    for i in range(lane, len(images), self.workers):
                        item = self._first(images[i], lane)
                        torch.cuda.current_stream().synchronize()
                        q.put((i,) + item)
            except BaseException as e:          # noqa: BLE001 - re-raised in the caller's thread
                errors.append(e)
            finally:
                q.put(None)

        def consumer(lane, q):
            try:
                with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                    while True:
                        item = q.get()
                        if item is None:
                            return
                        i, img, packed = item
                        results[i] = self._second(img, packed, lane)
            except BaseException as e:          # noqa: BLE001
                errors.append(e)
                while q.get() is not None:      # drain so that the producer can finish
                    pass

        ts = []
        for lane in range(self.workers):
            q: "queue.Queue" = queue.Queue(maxsize=self.depth)
            ts += [threading.Thread(target=producer, args=(lane, q)), threading.Thread(target=consumer, args=(lane, q))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errors:
            raise errors[0]
        return results
