"""What decoding JPEG on the device is worth: wall time per picture of

  pillow : Image.open(bytes).convert("RGB") -> torch.as_tensor -> .to(device)        (what a harness did before)
  device : JpegDecoder.decode = host parse + Huffman -> one upload -> glsdet_jpeg_reconstruct

each ending in a device synchronise, on two photo-like synthetic frames (1360x765 and 2000x1500, 4:2:0, quality 90).  The
two paths alternate inside one process; every figure is a median with its 10th / 90th percentile over --reps timed calls
after --warmup untimed ones.  The device path is also split into its host part (parse + entropy decode, host clock) and
its device part (upload + the two kernels, device events).  The results of the two paths are compared before anything is
timed.  One JSON line per frame.

    python tools/jpeg_bench.py [--reps 60] [--warmup 10]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frame(w, h, seed):
    """photo-like: smooth coloured regions (a coarse random field, bicubically enlarged), a few hard edges, mild grain"""
    from PIL import Image
    rng = np.random.RandomState(seed)
    coarse = Image.fromarray(rng.randint(0, 256, (h // 40 + 2, w // 40 + 2, 3)).astype(np.uint8))
    img = np.asarray(coarse.resize((w, h), Image.BICUBIC)).astype(np.float64)
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(12):                                               # rectangles: roofs, roads, vehicles
        x0, y0, bw, bh = rng.randint(0, w), rng.randint(0, h), rng.randint(20, w // 4), rng.randint(20, h // 4)
        m = (xx >= x0) & (xx < x0 + bw) & (yy >= y0) & (yy < y0 + bh)
        img[m] = img[m] * 0.4 + rng.randint(0, 256, 3) * 0.6
    img += rng.normal(0, 4.0, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def stats(ms):
    a = np.asarray(ms)
    return {"median_ms": round(float(np.median(a)), 4), "p10_ms": round(float(np.percentile(a, 10)), 4),
            "p90_ms": round(float(np.percentile(a, 90)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    import torch
    from PIL import Image
    from glsdet_amd import _lib
    from glsdet_amd import jpeg as J
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs an MI355X: a CPU run measures nothing")
    lib = _lib.load()
    dev = torch.device("cuda:0")
    dec = J.JpegDecoder("cuda:0", fallback="raise")

    def pillow_path(data):
        t = torch.as_tensor(np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))).to(dev)
        torch.cuda.synchronize()
        return t

    def device_path(data):
        t = dec.decode(data)
        torch.cuda.synchronize()
        return t

    for (w, h) in ((1360, 765), (2000, 1500)):
        b = io.BytesIO()
        Image.fromarray(frame(w, h, w)).save(b, "JPEG", subsampling=2, quality=90)
        data = b.getvalue()
        assert torch.equal(pillow_path(data), device_path(data)), "the two paths disagree"
        d = J.parse(data)
        n = d.n_blocks * 64
        stage = torch.empty(n + 192, dtype=torch.int16, pin_memory=True)
        buf = torch.empty(n + 192, dtype=torch.int16, device=dev)
        ws = torch.empty(lib.glsdet_jpeg_workspace_bytes(C.byref(d)), dtype=torch.uint8, device=dev)
        out = torch.empty(h, w, 3, dtype=torch.uint8, device=dev)
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        t_pil, t_dev, t_host, t_up, t_kern = [], [], [], [], []
        for i in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            pillow_path(data)
            t1 = time.perf_counter()
            device_path(data)
            t2 = time.perf_counter()
            # the split of the device path
            dd = J.parse(data)
            _lib.check(lib.glsdet_jpeg_entropy_decode(data, len(data), C.byref(dd), stage.data_ptr(), stage.data_ptr() + 2 * n))
            t3 = time.perf_counter()
            st = torch.cuda.current_stream()
            e0.record(st)
            buf.copy_(stage, non_blocking=True)
            e1.record(st)
            _lib.check(lib.glsdet_jpeg_reconstruct(C.byref(dd), buf.data_ptr(), buf.data_ptr() + 2 * n, ws.data_ptr(), ws.numel(),
                                                   out.data_ptr(), 3 * w, 0, st.cuda_stream))
            e2.record(st)
            torch.cuda.synchronize()
            if i >= args.warmup:
                t_pil.append((t1 - t0) * 1e3)
                t_dev.append((t2 - t1) * 1e3)
                t_host.append((t3 - t2) * 1e3)
                t_up.append(e0.elapsed_time(e1))
                t_kern.append(e1.elapsed_time(e2))
        print(json.dumps({"frame": "%dx%d" % (w, h), "jpeg_bytes": len(data), "coef_bytes": 2 * n, "rgb_bytes": 3 * w * h,
                          "reps": args.reps, "pillow_path": stats(t_pil), "device_path": stats(t_dev),
                          "device_path_host_entropy": stats(t_host), "device_path_upload": stats(t_up),
                          "device_path_kernels": stats(t_kern),
                          "speedup_median": round(float(np.median(t_pil) / np.median(t_dev)), 3)}), flush=True)


if __name__ == "__main__":
    main()
