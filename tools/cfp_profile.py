"""Per-op times of HipDetector("cfp") beside HipDetector("base"): phi `s`, 8 x 3 x 640 x 640, f16,
synthetic weights, kernel selection without autotuning, `Plan.run_timed` (one pair of device events per op, eager replay).

    python tools/cfp_profile.py [--out FILE.json] [--reps 20] [--no-graph]

Prints the table of the EVC block's launches with their share of the cfp forward, the time per batch of both kinds as
captured hipGraphs (alternating windows after a settle period, device events, median and range), and one JSON line.
For kernel-level times run it under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/cfp_profile.py --no-graph
--reps 5`, in a run of its own."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glsdet_amd.arch import state_dict_shapes            # noqa: E402
from glsdet_amd.detector import HipDetector              # noqa: E402
from glsdet_amd.synth import synth_input, synth_state_dict   # noqa: E402


def per_op(kind, phi, shape, reps):
    det = HipDetector(kind, synth_state_dict(state_dict_shapes(kind, phi, 10), 0), dtype="f16")
    c = det.compile(shape[0], shape[2], shape[3])
    det.run(c, synth_input(shape, 1).cuda())
    for _ in range(3):
        c.plan.run_timed()
    ms = c.plan.run_timed(reps=reps)
    torch.cuda.synchronize()
    return [dict(o, ms=float(t)) for o, t in zip(c.plan.ops(), ms)]


def graph_ms(kinds, phi, shape, windows=7, replays=50):
    """ms per batch of each kind as one captured hipGraph: `windows` alternating windows of `replays` replays each,
    timed with device events after a settle period -> {kind: (median, min, max)}"""
    import time
    plans = {}
    for kind in kinds:
        det = HipDetector(kind, synth_state_dict(state_dict_shapes(kind, phi, 10), 0), dtype="f16")
        c = det.compile(shape[0], shape[2], shape[3], None, use_graph=True)
        det.run(c, synth_input(shape, 1).cuda())
        plans[kind] = (det, c)
    t0 = time.time()
    while time.time() - t0 < 1.5:                       # settle: clocks up, both graphs resident
        for det, c in plans.values():
            det.run(c)
        torch.cuda.synchronize()
    out = {k: [] for k in kinds}
    for _ in range(windows):
        for kind, (det, c) in plans.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(replays):
                det.run(c)
            b.record()
            torch.cuda.synchronize()
            out[kind].append(a.elapsed_time(b) / replays)
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--phi", default="s")
    ap.add_argument("--shape", default="8,3,640,640")
    ap.add_argument("--no-graph", action="store_true")
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.shape.split(","))
    base, cfp = per_op("base", a.phi, shape, a.reps), per_op("cfp", a.phi, shape, a.reps)
    # the EVC block's ops: what the cfp plan has between the upsample of the P5 lateral (the plan's first upsample_nearest) and
    # C3_p4; the block ends with GroupNorm, fc1, fc2 and cnv1 behind its last channel_fuse (NetBuilder.evc)
    names = [o["name"] for o in cfp]
    first = next(i for i, nm in enumerate(names) if nm.startswith("upsample_nearest")) + 1
    last = max(i for i, nm in enumerate(names) if nm.startswith("channel_fuse")) + 4        # GroupNorm, fc1, fc2, cnv1 follow
    tot_b, tot_c = sum(o["ms"] for o in base), sum(o["ms"] for o in cfp)
    print("base: %d ops, %.3f ms per batch; cfp: %d ops, %.3f ms per batch (sum of per-op events)" % (len(base), tot_b, len(cfp), tot_c))
    print("| # | op | GFLOP | ms | share of the cfp forward |")
    print("|---|---|---|---|---|")
    for i in range(first, min(last + 1, len(cfp))):
        o = cfp[i]
        print("| %d | %s | %.2f | %.4f | %.1f %% |" % (i - first, o["name"], o["flops"] / 1e9, o["ms"], 100 * o["ms"] / tot_c))
    evc = sum(o["ms"] for o in cfp[first:last + 1])
    print("EVC block: %.3f ms = %.1f %% of the cfp forward; cfp - base = %.3f ms" % (evc, 100 * evc / tot_c, tot_c - tot_b))
    graphs = None
    if not a.no_graph:
        graphs = graph_ms(("base", "cfp"), a.phi, shape)
        for k, (med, lo, hi) in graphs.items():
            print("captured graph, %s: %.3f ms per batch (%.3f - %.3f over 7 windows of 50 replays)" % (k, med, lo, hi))
    res = {"shape": shape, "graph_ms": graphs, "phi": a.phi, "base_ms": tot_b, "cfp_ms": tot_c, "evc_ms": evc,
           "evc_ops": [{"name": o["name"], "ms": o["ms"], "gflop": o["flops"] / 1e9} for o in cfp[first:last + 1]]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
