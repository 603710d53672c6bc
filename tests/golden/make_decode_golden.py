#!/usr/bin/env python3
"""Generator of tests/golden/decode_modes_golden.npz -- runs ONLY where the reference checkout is mounted
(/root/reference).  It imports the reference's own `models/core/utils_bbox.py` at run time (torchvision, which that
module imports for its NMS only, is stubbed) and records, for one small synthetic head output, what its five decode
functions return in float32 on the CPU:

    decode_outputs, decode_outputs_cls_sigmoid, decode_outputs_no_sigmoid, decode_outputs_no_sigmoid_all,
    decode_outputs_xyxy                                                   (utils_bbox.py:36-306)

Input: batch 2, 10 classes, three levels of a 96 x 160 input whose grids are NOT in_w / w wide (the stride of both
axes is in_h / h in the reference), size logits over +-20, saturated and tiny score logits.  Data only.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_decode_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference/yolox-drone/models/core/utils_bbox.py"
sys.dont_write_bytecode = True

NAMES = ("decode_outputs", "decode_outputs_cls_sigmoid", "decode_outputs_no_sigmoid", "decode_outputs_no_sigmoid_all",
         "decode_outputs_xyxy")
INPUT_SHAPE = (96, 160)
SIZES = ((12, 16), (6, 8), (3, 4))
NC, BATCH = 10, 2


def reference_module():
    tv, ops = types.ModuleType("torchvision"), types.ModuleType("torchvision.ops")
    ops.boxes = types.ModuleType("torchvision.ops.boxes")
    tv.ops = ops
    saved = {k: sys.modules.get(k) for k in ("torchvision", "torchvision.ops", "torchvision.ops.boxes")}
    sys.modules.update({"torchvision": tv, "torchvision.ops": ops, "torchvision.ops.boxes": ops.boxes})
    try:
        spec = importlib.util.spec_from_file_location("ref_utils_bbox", REF)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def synth_levels():
    g = torch.Generator().manual_seed(20240)
    xs = []
    for h, w in SIZES:
        x = torch.randn(BATCH, 5 + NC, h, w, generator=g) * 3.0
        x[:, 2:4] = torch.rand(BATCH, 2, h, w, generator=g) * 40.0 - 20.0          # exp over the whole +-20 range
        x[0, 2, 0, 0], x[0, 3, 0, 0] = 20.0, -20.0
        x[0, 4, 0, 0], x[0, 5, 0, 0], x[1, 4, 0, 0], x[1, 5, 0, 0] = 20.0, -20.0, 40.0, -40.0      # saturated sigmoid
        x[1, 6, 0, 0], x[1, 7, 0, 0] = 1e-40, -1e-40                                # denormal logits
        xs.append(x)
    return xs


def main():
    ref = reference_module()
    xs = synth_levels()
    out = {"input_shape": np.asarray(INPUT_SHAPE, np.int64), "num_classes": np.asarray(NC, np.int64)}
    for l, x in enumerate(xs):
        out["level%d" % l] = x.numpy().copy()
    with torch.no_grad():
        for name in NAMES:
            got = getattr(ref, name)([x.clone() for x in xs], list(INPUT_SHAPE))
            assert got.dtype == torch.float32 and got.shape == (BATCH, sum(h * w for h, w in SIZES), 5 + NC)
            out["ref/" + name] = got.contiguous().numpy().copy()
    for l, x in enumerate(xs):
        assert np.array_equal(out["level%d" % l], x.numpy())                       # the reference left its inputs alone
    path = os.path.join(HERE, "decode_modes_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
