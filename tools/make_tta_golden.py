"""Records tests/golden/tta_golden.npz: the outputs of the reference's own bbox_flip / bbox_mapping_back
(mmdet/core/bbox/transforms.py:22-72, imported by file path -- the file needs only numpy and torch) for random float32
boxes x {none, horizontal, vertical, diagonal} x a few scale-factor rows, dyadic and not.

    python tools/make_tta_golden.py <reference checkout>/mmdet/core/bbox/transforms.py

The tests read only the .npz (tests/test_tta_reference.py pins tests/tta_reference.map_back to it bit for bit,
tests/test_tta_fuzz.py the kernel)."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTIONS = (None, "horizontal", "vertical", "diagonal")        # index = the flip code of the C ABI
N = 12


def _rescale(w, h, scale):
    """Resize(keep_ratio=True): mmcv.rescale_size + the float32 scale_factor row mmdet stores"""
    f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    nw, nh = int(w * float(f) + 0.5), int(h * float(f) + 0.5)
    return (nh, nw), np.array([nw / w, nh / h, nw / w, nh / h], np.float32)


def cases():
    """(img_shape (h, w), scale_factor row [4] float32)"""
    out = [((608, 800), np.full(4, 1.0, np.float32)), ((300, 417), np.full(4, 0.5, np.float32)),
           ((1216, 1601), np.full(4, 2.0, np.float32))]
    for (w, h), scale in (((1920, 1080), (1333, 800)), ((1360, 765), (1333, 800)), ((2000, 1500), (2000, 1200)),
                          ((1916, 1078), (1000, 600)), ((640, 481), (1333, 800))):
        out.append(_rescale(w, h, scale))
    return out


def main(path):
    spec = importlib.util.spec_from_file_location("ref_bbox_transforms", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    rng = np.random.default_rng(20240)
    data = {}
    cs = cases()
    data["img_shape"] = np.asarray([c[0] for c in cs], np.int64)
    data["scale_factor"] = np.stack([c[1] for c in cs])
    for ci, ((h, w), sf) in enumerate(cs):
        p = rng.uniform(0, 1, (N, 4)).astype(np.float32)
        x = np.sort(p[:, :2] * np.float32(w), axis=1)
        y = np.sort(p[:, 2:] * np.float32(h), axis=1)
        boxes = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1).astype(np.float32)
        boxes[0] = [0, 0, w, h]                                     # the clamp limits of get_bboxes
        boxes[1] = [0, 0, 0, 0]
        data["boxes/%d" % ci] = boxes
        t = torch.from_numpy(boxes)
        for code, d in enumerate(DIRECTIONS):
            if d is not None:
                data["flip/%d/%d" % (ci, code)] = ref.bbox_flip(t, (h, w, 3), d).numpy()
            back = ref.bbox_mapping_back(t, (h, w, 3), sf, d is not None, d if d is not None else "horizontal")
            assert back.dtype == torch.float32
            data["back/%d/%d" % (ci, code)] = back.numpy()
    out = os.path.join(ROOT, "tests", "golden", "tta_golden.npz")
    np.savez_compressed(out, **data)
    print("wrote %s: %d bytes" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main(sys.argv[1])
