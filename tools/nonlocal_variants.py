"""Times glsdet_nonlocal_multi (scalar kernels) against glsdet_nonlocal_mfma (matrix cores) on the non-local blocks of a
`cross10` detector, with HIP events: the four quadrants of dark3 / dark4 / dark5 of YOLOX-s at 8x800x1344 and 8x640x640,
both engine dtypes.

    python tools/nonlocal_variants.py [--reps 7] [--iters 20] [--json out.json]

Per shape and path: WARM untimed calls, then REPS windows of ITERS back-to-back calls between two events; reported are the
median window, the spread (max - min) / median of the windows and the achieved TFLOP/s on the algorithmic count of the three
launches (Gram 2 N C^2, fold 2 C^3, apply 2 N C^2 per image and quadrant).  The MFMA path counts as faster for a geometry
only where its median lies below the scalar path's by more than the scalar path's own spread.  The operands are random and
the same for both paths; outputs go to a separate buffer.  The windows of the two paths are interleaved.  Then the per-op
times of a whole cross10-s forward at 8x800x1344 (Plan.run_timed) with either kernel family give the share of the three
non-local ops.  The state of the box is printed before and after as far as this process can see it without changing
anything (time, devices, free memory, load average): read the spread before trusting a ratio."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glsdet_amd._lib import View                                 # noqa: E402
from glsdet_amd.engine import Engine, _stream_ptr                # noqa: E402

WARM = 5
LEVELS = {"800x1344": [(128, 100, 168), (256, 50, 84), (512, 25, 42)], "640x640": [(128, 80, 80), (256, 40, 40), (512, 20, 20)]}


SWEEP_C = (64, 96, 128, 192, 256, 320, 384, 512, 640, 1024, 1280)
SWEEP_MAPS = ((4, 6), (10, 14), (20, 28), (40, 56), (100, 168))     # quadrants of 6, 35, 140, 560, 4200 pixels


def flops(n, C_, wins):
    return sum(n * (4.0 * (h * w) * C_ * C_ + 2.0 * C_ ** 3) for h, w in wins)


def time_pair(old, new, reps, iters):
    """windows of the two paths INTERLEAVED (old, new, old, new, ...), so that drift of the box hits both alike
    -> ((median ms, spread) of old, of new)"""
    for fn in (old, new):
        for _ in range(WARM):
            fn()
    torch.cuda.synchronize()
    ms = {0: [], 1: []}
    for _ in range(reps):
        for k, fn in enumerate((old, new)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b) / iters)
    stat = lambda v: (float(np.median(v)), float((np.max(v) - np.min(v)) / np.median(v)))
    return stat(ms[0]), stat(ms[1])


def box_state():
    """what this process can see of the box without changing it"""
    free, total = torch.cuda.mem_get_info()
    return dict(time=time.strftime("%Y-%m-%d %H:%M:%S"), device=torch.cuda.get_device_name(0), devices=torch.cuda.device_count(),
                mem_free_gb=round(free / 2 ** 30, 1), mem_total_gb=round(total / 2 ** 30, 1), loadavg=os.getloadavg())


def forward_share(dtype, batch, H, W, reps):
    """per-op times of a whole cross10-s forward with the scalar and with the matrix-core non-local kernels
    -> {policy: (ms of the three non-local ops, ms of the forward)}"""
    from glsdet_amd.arch import state_dict_shapes
    from glsdet_amd.detector import HipDetector
    from glsdet_amd.synth import synth_state_dict
    sd = synth_state_dict(state_dict_shapes("cross10", "s", 10), 0)
    x = torch.randn(batch, 3, H, W, device="cuda")
    out = {}
    for policy in ("0", "1"):
        os.environ["GLSDET_NONLOCAL_MFMA"] = policy
        det = HipDetector("cross10", sd, dtype=dtype)
        c = det.compile(batch, H, W)
        for _ in range(3):
            det.run(c, x)
        torch.cuda.synchronize()
        ms = c.plan.run_timed(reps=reps)
        names = [o["name"] for o in c.plan.ops()]
        nl = [m for m, nm in zip(ms, names) if nm.startswith("nonlocal")]
        assert len(nl) == 3 and all(("mfma" in nm) == (policy == "1") for nm in names if nm.startswith("nonlocal")), names
        out[policy] = (float(sum(nl)), float(ms.sum()), [float(v) for v in nl])
        del det, c
    os.environ.pop("GLSDET_NONLOCAL_MFMA")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default="")
    ap.add_argument("--sweep", action="store_true", help="the width x map grid behind Engine.NONLOCAL_MFMA_FROM instead of the cross10-s levels")
    ap.add_argument("--no-forward", action="store_true", help="skip the whole-forward share (kernel-trace runs)")
    args = ap.parse_args()
    state = box_state()
    print("box:", state, flush=True)
    rows = []
    for dtype in ("f16", "f32"):
        eng = Engine(dtype)
        tt = torch.float16 if dtype == "f16" else torch.float32
        grid = {"%dx%d" % m: [(c, m[0], m[1]) for c in SWEEP_C] for m in SWEEP_MAPS} if args.sweep else LEVELS
        for size, levels in grid.items():
            for C_, H, W in levels:
                n = args.batch
                mark = len(eng._keep)
                x, t, o = eng.tensor(n, H, W, C_), eng.tensor(n, H, W, 3 * C_), eng.tensor(n, H, W, C_)
                x.buf.view(tt)[:] = torch.randn(x.buf.numel() // x.buf.view(tt).element_size(), device="cuda").to(tt)
                t.buf.view(tt)[:] = torch.rand(t.buf.numel() // t.buf.view(tt).element_size(), device="cuda").to(tt)
                q = [(0, H // 2, 0, W // 2), (H // 2, H, 0, W // 2), (0, H // 2, W // 2, W), (H // 2, H, W // 2, W)]
                xs, ts, os_ = [x.window(*w) for w in q], [t.window(*w) for w in q], [o.window(*w) for w in q]
                assert eng.nonlocal_mfma_takes(xs, ts, C_, os_)
                wouts = [eng.upload(torch.randn(C_, C_) * (4.0 / C_)) for _ in q]
                bouts = [eng.upload(torch.randn(C_)) for _ in q]
                xa, ta, oa = (View * 4)(*[v.as_c() for v in xs]), (View * 4)(*[v.as_c() for v in ts]), (View * 4)(*[v.as_c() for v in os_])
                wa, ba = (C.c_void_p * 4)(*[w.data_ptr() for w in wouts]), (C.c_void_p * 4)(*[b.data_ptr() for b in bouts])
                nbytes = eng.lib.glsdet_nonlocal_mfma_workspace_bytes(n, 4, C_, C_)
                ws = eng.raw(nbytes)
                st = _stream_ptr(None)
                old = lambda: eng.lib.glsdet_nonlocal_multi(xa, ta, 4, C_, wa, ba, ws.data_ptr(), oa, st)
                new = lambda: eng.lib.glsdet_nonlocal_mfma(xa, ta, 4, C_, wa, ba, ws.data_ptr(), nbytes, oa, st)
                assert old() == 0 and new() == 0, eng.lib.glsdet_last_error().decode()
                fl = flops(n, C_, [(w[1] - w[0], w[3] - w[2]) for w in q])
                (mo, so), (mn, sn) = time_pair(old, new, args.reps, args.iters)
                row = dict(dtype=dtype, size=size, C=C_, H=H, W=W, gflop=fl / 1e9, scalar_ms=mo, scalar_spread=so, mfma_ms=mn,
                           mfma_spread=sn, scalar_tf=fl / mo / 1e9, mfma_tf=fl / mn / 1e9, mfma_faster=bool(mn < mo * (1.0 - so)))
                rows.append(row)
                print("%s %-9s C=%-4d %3dx%-3d %6.2f GFLOP | scalar %8.3f ms (+-%4.1f %%) %6.1f TF | mfma %8.3f ms (+-%4.1f %%) %6.1f TF | %s" % (
                    dtype, size, C_, H, W, row["gflop"], mo, 100 * so, row["scalar_tf"], mn, 100 * sn, row["mfma_tf"],
                    "mfma faster" if row["mfma_faster"] else "NOT faster"), flush=True)
                torch.cuda.synchronize()
                del eng._keep[mark:]
        del eng
    if args.sweep:
        # per dtype and width: the smallest measured quadrant from which the matrix-core path is faster at every larger one
        table = {}
        for r in rows:
            table.setdefault(r["dtype"], {}).setdefault(r["C"], []).append(((r["H"] // 2) * (r["W"] // 2), r["mfma_faster"]))
        for dt, per in table.items():
            out = {}
            for c, pts in sorted(per.items()):
                pts.sort()
                need = None
                for N, ok in reversed(pts):
                    if not ok:
                        break
                    need = N
                if need is not None:
                    out[c] = need
            print("NONLOCAL_MFMA_FROM[%s] = %r" % (dt, out))
    shares = {}
    for dtype in (() if args.no_forward or args.sweep else ("f16", "f32")):
        shares[dtype] = forward_share(dtype, args.batch, 800, 1344, 1)
        for policy, (nl, total, each) in shares[dtype].items():
            print("cross10-s %s 8x800x1344, non-local kernels %s: %.3f ms of %.3f ms per forward (%.1f %%), levels %s" % (
                dtype, "mfma" if policy == "1" else "scalar", nl, total, 100 * nl / total, ["%.3f" % v for v in each]), flush=True)
    print("box:", box_state())
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(box=state, rows=rows, forward=shares), f, indent=1)


if __name__ == "__main__":
    main()
