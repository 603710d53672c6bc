"""Shape-specialised, plan-backed detector: weights resident in HBM, one recorded plan
(optionally one hipGraph) per input shape, no Python in the per-layer loop."""
from __future__ import annotations

from typing import List, Optional

import numpy as np
import torch

from .engine import DECODE_MODES, Engine
from .nets import build_forward
from .plans import PlanBacked


class _Compiled:
    __slots__ = ("img", "plan", "levels", "stems", "decoded", "nmsb", "eng", "post", "graph_stream", "scale")


class HipDetector(PlanBacked):
    """kind: 'base' (YOLOX) | 'gl' (YOLOX + GL-fusion neck) | 'cross' (cross-scale head, new/yolox6.py) | 'cross10' (the
    same behind residual Patch_Conv_NonLocal_new blocks on dark3 / 4 / 5, new/yolox10.py) | 'cfp' (YOLOX with the EVCBlock
    on the upsampled P5 lateral, cfp/yolox_cfp.py).  state_dict uses the
    reference's key names (drone flavour).  dtype 'f16' (fp16 storage / fp32 accumulate,
    the benchmarked mode) or 'f32' (exact-f32 MFMA, the strict-parity mode)."""

    def __init__(self, kind: str, state_dict, dtype: str = "f16", device: str = "cuda:0", autotune: bool = False):
        self.kind, self.dtype, self.device, self.autotune = kind, dtype, device, autotune
        self.sd = {k: v.detach().cpu() for k, v in state_dict.items()}
        super().__init__()                        # the plan cache: self._plans, its dict self._compiled
        self.num_classes = None

    # ------------------------------------------------------------------ compile
    def compile(self, n: int, H: int, W: int, post: Optional[dict] = None, use_graph: bool = False,
                instance: int = 0) -> _Compiled:
        """post: None (raw logits only) or dict(conf_thres, nms_thres, max_cand, max_det, mode, sigmoid, exchange_cap);
        max_cand = NMS candidates kept per image, default min(4096, A) (A = anchors of the input shape); more passing
        anchors than that make collect() raise.  max_cand = A can never overflow and costs an A * ceil(A / 64) * 8 byte
        suppression mask per image (9 MB at A = 8400, 61 MB at A = 22050) in the plan's workspace; at most 32768.
        max_det = rows of the result per image, default 1000.
        sigmoid = the decode's sigmoid mask (bit 0 objectness, bit 1 classes; default 3 = both, see DECODE_MODES);
        exchange_cap = K appends the multi-GPU exchange record ([n, K+1, 7], Engine.pack_detections) to the plan.
        `instance` > 0 builds an independent copy (own buffers, own stream) of the same plan, so
        consecutive batches can be in flight concurrently (see run_async)."""
        key = (n, H, W, tuple(sorted(post.items())) if post else None, use_graph, instance)
        return self._plans.get(key, lambda: self._build(n, H, W, post, use_graph))

    def _build(self, n: int, H: int, W: int, post: Optional[dict], use_graph: bool) -> _Compiled:
        if H % 32 or W % 32:
            raise ValueError("input H and W must be multiples of 32 (got %dx%d)" % (H, W))
        eng = Engine(self.dtype, self.device, autotune=self.autotune)
        c = _Compiled()
        c.eng = eng
        c.img = torch.zeros(n, 3, H, W, dtype=torch.float32, device=eng.device)
        c.plan = eng.new_plan()
        c.post = post
        c.decoded = c.nmsb = c.scale = None
        if post is not None and post.get("rescale"):
            c.scale = torch.ones(n, 4, dtype=torch.float32, device=eng.device)   # per-image divisors (mmdet rescale)
        with c.plan:
            c.levels, self.num_classes, c.stems = build_forward(self.kind, eng, self.sd, c.img)
            if post is not None:
                A = sum(l.h * l.w for l in c.levels)
                c.decoded = eng.decode(c.levels, self.num_classes, H, W, mode=post.get("mode", 0),
                                       strides=[8, 16, 32] if post.get("mode", 0) == 1 else None,
                                       scale_factors=c.scale, sigmoid=post.get("sigmoid", 3))
                # candidate capacity per image: 4096 unless the caller asks for more (the class-segmented NMS kernels take up to
                # 4096 candidates per image; beyond that the three-kernel path of rounds 1-2 runs as well).  More candidates
                # than the capacity raise the status flag -> HipDetector.collect says "raise max_cand".
                c.nmsb = eng.nms_buffers(n, A, min(post.get("max_cand", 4096), A), post.get("max_det", 1000))
                eng.nms(c.decoded, self.num_classes, post.get("mode", 0), post["conf_thres"], post["nms_thres"], c.nmsb)
                if post.get("exchange_cap"):
                    eng.pack_detections(c.nmsb, int(post["exchange_cap"]))
        return self._finish(c, use_graph)

    # ------------------------------------------------------------------ run
    def run(self, c: _Compiled, img: Optional[torch.Tensor] = None, stream=None, scale: Optional[torch.Tensor] = None):
        """One forward (+ post-processing if compiled in), see PlanBacked._replay."""
        self._replay(c, stream, img=img, scale=scale)

    def forward_raw(self, img: torch.Tensor) -> List[torch.Tensor]:
        """Reference-shaped output: list of [B, 5+nc, H_l, W_l] fp32 logits (NCHW)."""
        n, _, H, W = img.shape
        c = self.compile(n, H, W)
        self.run(c, img.to(c.img.device, torch.float32))
        return [l.to_nchw(5 + self.num_classes) for l in c.levels]

    @staticmethod
    def num_anchors(H: int, W: int) -> int:
        """anchors of an H x W input: one per cell of the stride 8, 16 and 32 levels"""
        return sum((H // s) * (W // s) for s in (8, 16, 32))

    def detect(self, img: torch.Tensor, conf_thres: float, nms_thres: float, max_det: Optional[int] = None, mode: int = 0,
               decode_mode: str = "default", max_cand: Optional[int] = None):
        """-> (decoded [B,A,5+nc] device tensor, list per image of ndarray(k,7) [x1,y1,x2,y2,obj,cls_conf,cls])
        max_cand / max_det: NMS candidates / result rows per image; None = all A anchors, so no confidence threshold
        can overflow them (the reference is scored at 0.01 and 0.0001, where nearly every anchor is a candidate).  That
        costs an A * ceil(A / 64) * 8 byte mask per image in the plan's workspace (about 61 MB at A = 22050); where the
        scenes are known to be sparse pass a smaller max_cand, e.g. max_cand=4096 keeps the whole NMS in the
        class-segmented kernels with a 2 MB mask.  More candidates than max_cand, or more detections than max_det, raise.
        decode_mode: the reference harness's name (drone/yolo.py:75-82) for the score channels that get a sigmoid --
        'default' | 'obj_sigmoid' | 'no_sigmoid' | 'cls_sigmoid'; the others reach the NMS as raw logits."""
        if decode_mode not in DECODE_MODES:
            raise ValueError("decode_mode must be one of %s (got %r)" % (sorted(DECODE_MODES), decode_mode))
        n, _, H, W = img.shape
        A = self.num_anchors(H, W)
        if A > 32768 and max_cand is None:
            raise ValueError("a %dx%d input has %d anchors; the NMS takes at most 32768 candidates per image: pass max_cand" % (H, W, A))
        post = dict(conf_thres=conf_thres, nms_thres=nms_thres, max_det=A if max_det is None else max_det, mode=mode,
                    max_cand=A if max_cand is None else max_cand)
        if DECODE_MODES[decode_mode] != 3:          # the default keeps the plan-cache key it always had
            post["sigmoid"] = DECODE_MODES[decode_mode]
        c = self.compile(n, H, W, post)
        self.run(c, img.to(c.img.device, torch.float32))
        return c.decoded, self.collect(c)

    @staticmethod
    def collect(c: _Compiled):
        count = c.nmsb["count"].cpu().numpy()            # the one host sync of the path
        if int(c.nmsb["status"].item()) & 1:
            raise RuntimeError("NMS candidate capacity exceeded (raise max_cand)")
        dets = c.nmsb["dets"].cpu().numpy()
        n = c.nmsb["n"]
        if (count[n:] > c.nmsb["max_det"]).any():
            raise RuntimeError("more detections than max_det=%d (raise max_det)" % c.nmsb["max_det"])
        return [dets[i, : count[i]].copy() for i in range(n)]
