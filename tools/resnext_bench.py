#!/usr/bin/env python3
"""End-to-end img/s of MPDet on the ResNeXt-101 backbones (configs/UFPMP-Det/mp_det_x101_32x4d.py, mp_det_x101_64x4d.py) at
8 x 800 x 1344, f16, autotuned, one captured hipGraph per plan -- with conv2 on the grouped kernel (where the tuner keeps
it) and, GLSDET_NO_GROUPED_CONV=1, as the block-diagonal dense conv; both plans are built in this process and timed in
alternating windows.  Synthetic weights (BN calibrated on a small input), forward + GFL post-processing.

    python tools/resnext_bench.py [--n 8 --height 800 --width 1344 --windows 5 --steps 10]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

from glsdet_amd.resdet import HipGflDetector
from glsdet_amd.synth import synth_resdet_state_dict
from oracle.glsdet_oracle import synth_input


def build(sd, groups, n, H, W, expand):
    if expand:
        os.environ["GLSDET_NO_GROUPED_CONV"] = "1"
    else:
        os.environ.pop("GLSDET_NO_GROUPED_CONV", None)
    det = HipGflDetector("mpdet", sd, dtype="f16", autotune=True, depth=101, groups=groups, base_width=4)
    c = det.compile(n, H, W, dict(score_thr=0.3, iou_thr=0.6, nms_pre=1000, max_per_img=100), use_graph=True)
    os.environ.pop("GLSDET_NO_GROUPED_CONV", None)
    names = [o["name"] for o in c.plan.ops()]
    return det, c, sum(nm.startswith("conv_grouped") for nm in names)


def window(det, c, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(c.graph_stream)
    for _ in range(steps):
        c.plan.launch(c.graph_stream)
    e1.record(c.graph_stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1344)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    cal = synth_input((1, 3, 128, 160), 100)
    for groups in (32, 64):
        sd = synth_resdet_state_dict("mpdet", 0, cal, depth=101, groups=groups, base_width=4)
        plans = {"grouped": build(sd, groups, a.n, a.height, a.width, False), "expanded": build(sd, groups, a.n, a.height, a.width, True)}
        img = synth_input((a.n, 3, a.height, a.width), 7).cuda()
        for det, c, _ in plans.values():
            c.img.copy_(img)
            window(det, c, 3)                                # warm-up
        ms = {k: [] for k in plans}
        for _ in range(a.windows):                           # alternating windows
            for k, (det, c, _) in plans.items():
                ms[k].append(window(det, c, a.steps))
        for k, (det, c, n_grouped) in plans.items():
            v = sorted(ms[k])
            med = v[len(v) // 2]
            print("x101_%dx4d %-8s: %d conv_grouped ops of %d, median %.2f ms per batch of %d = %.1f img/s (min %.2f max %.2f ms)" %
                  (groups, k, n_grouped, c.plan.num_ops, med, a.n, a.n * 1e3 / med, v[0], v[-1]), flush=True)
        del plans, det, c
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
