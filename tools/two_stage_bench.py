#!/usr/bin/env python3
"""Latency of the two-stage UFPMP-Det path for ONE 540x1024 frame (synthetic weights): coarse GFL at
1333x800 -> host packing -> device mosaic -> fine MPDet -> device back-mapping + merge NMS; then the throughput of the
pipelined forms, and a same-process A/B of packing="host" against packing="device" (glsdet_ufp_pack) at one, two and
three lanes with the pack kernel's own time from HIP events.  --packing-only skips the middle part."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from glsdet_amd.resdet import HipGflDetector
from glsdet_amd.synth import synth_input, synth_resdet_state_dict
from glsdet_amd.ufp import TwoStagePipeline, UfpSecondStage, two_stage_detect
from glsdet_amd.ufp.packing import unified_foreground_packing
from tests.test_preprocess import synth_image

img = synth_image((540, 1024), 2)[:, :, ::-1].copy()
calib = synth_input((1, 3, 128, 160), 100)
coarse = HipGflDetector("gfl", synth_resdet_state_dict("gfl", 0, calib), dtype="f16", autotune=True)
fine = HipGflDetector("mpdet", synth_resdet_state_dict("mpdet", 1, calib), dtype="f16", autotune=True)
stage = UfpSecondStage()


def thr_for(det, x, keep):
    cls, _ = det.forward_raw(x)
    p = torch.sigmoid(torch.cat([c.flatten() for c in cls]))
    return float(torch.topk(p, keep).values[-1])


x1, _ = stage.pipeline_input(torch.from_numpy(img).cuda().contiguous())
c1 = dict(score_thr=thr_for(coarse, x1, 80), iou_thr=0.6, nms_pre=1000, max_per_img=100)
_, mid = two_stage_detect(coarse, fine, img, stage, c1, dict(score_thr=0.9999, iou_thr=0.6))
x2, _ = stage.pipeline_input(mid["canvas"])
c2 = dict(score_thr=thr_for(fine, x2, 600), iou_thr=0.6, nms_pre=1000, max_per_img=500)
for _ in range(3):
    merged, mid = two_stage_detect(coarse, fine, img, stage, c1, c2)
torch.cuda.synchronize()
t0 = time.perf_counter()
n = 20
for _ in range(n):
    merged, mid = two_stage_detect(coarse, fine, img, stage, c1, c2)
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / n
boxes = mid["first"][0][:, :4]
t0 = time.perf_counter()
for _ in range(20):
    unified_foreground_packing(boxes.copy(), 1.5, [1024, 540])
tp = (time.perf_counter() - t0) / 20
print("two-stage, one 540x1024 frame: %.2f ms end to end (%.1f frames/s); host packing of %d boxes %.2f ms; "
      "%d chips, mosaic %dx%d, fine input %s, %d merged detections"
      % (dt * 1e3, 1 / dt, len(boxes), tp * 1e3, len(mid["chips"]), mid["canvas"].shape[1], mid["canvas"].shape[0],
         tuple(x2.shape), sum(len(m) for m in merged)))

frames = [synth_image((540, 1024), 100 + i)[:, :, ::-1].copy() for i in range(8)] * 4


def packing_ab():
    """frames/s of both packing modes, interleaved in one process; results must be identical"""
    pl = {(w, m): TwoStagePipeline(coarse, fine, stage, c1, c2, workers=w, packing=m) for w in (1, 2, 3) for m in ("host", "device")}
    for (w, m), p in pl.items():
        p.run(frames[:8] * w)                # every lane sees every shape once
    torch.cuda.synchronize()
    ref = None
    for rep in range(3):
        line = []
        for (w, m), p in pl.items():
            t0 = time.perf_counter()
            out = p.run(frames)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ref = out if ref is None else ref
            same = all(all(np.array_equal(a, b) for a, b in zip(x, y)) for x, y in zip(ref, out))
            line.append("%d lane%s %s %.1f%s" % (w, "s" if w > 1 else "", m, len(frames) / dt, "" if same else " (RESULTS DIFFER)"))
        print("packing A/B, 32 frames, frames/s: " + "; ".join(line))
    for m in ("host", "device"):
        for _ in range(3):
            two_stage_detect(coarse, fine, img, stage, c1, c2, packing=m)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            two_stage_detect(coarse, fine, img, stage, c1, c2, packing=m)
        torch.cuda.synchronize()
        print("sequential two_stage_detect, packing=%s: %.2f ms per frame" % (m, (time.perf_counter() - t0) / 20 * 1e3))


def pack_kernel_time():
    """glsdet_ufp_pack alone, HIP events around 20 launches: the bench frame's coarse buffers, then max_det at the limit"""
    from glsdet_amd import _lib
    lib = _lib.load()
    _, dmid = two_stage_detect(coarse, fine, img, stage, c1, c2, packing="device")
    nb = dmid["coarse_compiled"].nb
    limit = int(lib.glsdet_ufp_pack_max_boxes())
    rng = np.random.default_rng(0)
    cases = [("bench frame", nb["dets"][0].clone(), nb["count"][:1].clone(), 1024, 540)]
    for name, lo, hi in (("limit, overlapping boxes of 6..220 px", 6, 220), ("limit, sparse boxes of 4..40 px", 4, 40)):
        c = rng.uniform(0, 1, (limit, 2)) * [1920, 1080]
        wh = np.exp(rng.uniform(np.log(lo), np.log(hi), (limit, 2)))
        d = np.zeros((limit, 7), np.float32)
        d[:, :4] = np.clip(np.concatenate([c - wh / 2, c + wh / 2], 1), 0, [1919, 1079, 1919, 1079])
        d[:, 6] = rng.integers(0, 10, limit)
        cases.append((name, torch.from_numpy(d).cuda(), torch.tensor([limit], dtype=torch.int32).cuda(), 1920, 1080))
    for name, dets, count, W, H in cases:
        n = int(dets.shape[0])
        exact = torch.empty(n, 7, dtype=torch.float64, device="cuda")
        floor = torch.empty(n, 7, dtype=torch.float32, device="cuda")
        header = torch.empty(4, dtype=torch.float64, device="cuda")
        status = torch.empty(1, dtype=torch.int32, device="cuda")

        def launch():
            _lib.check(lib.glsdet_ufp_pack(dets.data_ptr(), count.data_ptr(), 1, n, 1.5, W, H, exact.data_ptr(), floor.data_ptr(),
                                           header.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream), "ufp_pack")
        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            launch()
        e1.record()
        e1.synchronize()
        h = header.cpu().tolist()
        print("glsdet_ufp_pack, %s: %d boxes -> %d chips, canvas %g x %g, %.1f us per launch (max_det %d)"
              % (name, h[0], h[1], h[2], h[3], e0.elapsed_time(e1) / 20 * 1e3, n))


if "--packing-only" in sys.argv:
    packing_ab()
    pack_kernel_time()
    sys.exit(0)
pipes = {g: TwoStagePipeline(coarse, fine, stage, c1, c2, use_graph=g) for g in (False, True)}
for g in (False, True):                     # warm: plans (and graphs) for the mosaic shapes of these frames
    for f in frames[:8]:
        two_stage_detect(coarse, fine, f, stage, c1, c2, use_graph=g)
    pipes[g].run(frames[:8])
lanes = {w: TwoStagePipeline(coarse, fine, stage, c1, c2, workers=w) for w in (2, 3, 4)}
for w, pl in lanes.items():
    pl.run(frames[:8] * w)                  # every lane sees every shape once
torch.cuda.synchronize()
ref = None
for rep in range(2):
    line = []
    for name, fn in (("sequential eager", lambda: [two_stage_detect(coarse, fine, f, stage, c1, c2)[0] for f in frames]),
                     ("sequential graph replay", lambda: [two_stage_detect(coarse, fine, f, stage, c1, c2, use_graph=True)[0] for f in frames]),
                     ("two-stream pipeline eager", lambda: pipes[False].run(frames)),
                     ("two-stream pipeline graph replay", lambda: pipes[True].run(frames)),
                     ("2 lanes", lambda: lanes[2].run(frames)), ("3 lanes", lambda: lanes[3].run(frames)),
                     ("4 lanes", lambda: lanes[4].run(frames))):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ref = out if ref is None else ref
        same = all(all(np.array_equal(a, b) for a, b in zip(x, y)) for x, y in zip(ref, out))
        line.append("%s %.1f%s" % (name, len(frames) / dt, "" if same else " (RESULTS DIFFER)"))
    print("32 frames, frames/s: " + "; ".join(line))
packing_ab()
pack_kernel_time()
