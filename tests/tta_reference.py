"""A deliberately naive reference of the cross-augmentation step of test-time augmentation (glsdet_aug_merge_nms):
map every augmentation's candidates back in numpy float32, concatenate, then tests/post_reference.greedy_nms.
TEST INFRASTRUCTURE ONLY; imports nothing from `oracle` or the package.

The map-back restates bbox_flip / bbox_mapping_back (mmdet/core/bbox/transforms.py:22-72) and is pinned bit for bit
to the reference's own outputs in tests/golden/tta_golden.npz (tools/make_tta_golden.py) by tests/test_tta_reference.py.

Order contract: score descending, then concatenation index ascending -- of two bit-equal scores the
row of the earlier augmentation is visited first; suppression only inside a class; IoU > thr suppresses; areas
without +1.

Flip codes are those of the C ABI: 0 none, 1 horizontal, 2 vertical, 3 diagonal.  The order of the augmentations is
MultiScaleFlipAug's (mmdet/datasets/pipelines/test_time_aug.py:96-108): scale-major; per scale the unflipped picture
first, then the directions as listed."""
import os

import numpy as np

from tests import post_reference as R

F32 = np.float32
DIRECTIONS = (None, "horizontal", "vertical", "diagonal")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tta_golden.npz")


def aug_order(scales, flip, directions):
    """test_time_aug.py:96-108 restated -> [(scale, flip, direction)]"""
    directions = list(directions) if isinstance(directions, (list, tuple)) else [directions]
    out = []
    for s in scales:
        out.append((s, False, None))
        if flip:
            out += [(s, True, d) for d in directions]
    return out


def flip_boxes(boxes, img_shape, code, mutate=None):
    """bbox_flip in float32, one subtraction per coordinate.  mutate (the mutation check only): 'swap' mirrors x1 from x1
    and x2 from x2; ('padded', pw, ph) mirrors inside the padded extent instead of img_shape."""
    b = np.asarray(boxes, F32).reshape(-1, 4)
    h, w = F32(img_shape[0]), F32(img_shape[1])
    if isinstance(mutate, tuple) and mutate[0] == "padded":
        w, h = F32(mutate[1]), F32(mutate[2])
    out = b.copy()
    lo, hi = (0, 2) if mutate == "swap" else (2, 0)
    if code & 1:
        out[:, 0] = w - b[:, lo]
        out[:, 2] = w - b[:, hi]
    if code & 2:
        out[:, 1] = h - b[:, lo + 1]
        out[:, 3] = h - b[:, hi + 1]
    return out


def map_back(boxes, img_shape, scale_factor, code, mutate=None):
    """bbox_mapping_back: mirror inside img_shape when flipped, then ONE float32 division per coordinate.
    mutate='reciprocal' multiplies by the float32 reciprocal instead."""
    out = flip_boxes(boxes, img_shape, code, mutate)
    sf = np.asarray(scale_factor, F32).reshape(4)
    if mutate == "reciprocal":
        return (out * (F32(1) / sf)).astype(F32)
    return (out / sf).astype(F32)


def merge(aug_rows, metas, iou_thr, max_det, out_scale=None):
    """aug_rows[k]: float32 [m_k, 6] = x1,y1,x2,y2,score,label of ONE image in augmentation k (already cut to its count);
    metas[k] = (img_h, img_w, scale_factor[4], flip code).  -> (dets float32 [min(kept, max_det), 7] = x1,y1,x2,y2,score,
    score,label as glsdet_gfl_detect writes them, kept before the cut, index of each det in the concatenation)."""
    boxes, scores, labels = [], [], []
    for rows, (h, w, sf, code) in zip(aug_rows, metas):
        rows = np.asarray(rows, F32).reshape(-1, 6)
        boxes.append(map_back(rows[:, :4], (h, w), sf, int(code)))
        scores.append(rows[:, 4])
        labels.append(rows[:, 5])
    boxes, scores, labels = np.concatenate(boxes), np.concatenate(scores), np.concatenate(labels)
    keep = R.greedy_nms(boxes, scores, labels.astype(np.int64), np.arange(len(scores)), iou_thr)
    total = len(keep)
    keep = keep[:max_det]
    b = boxes[keep]
    if out_scale is not None:
        b = (b * np.asarray(out_scale, F32).reshape(1, 4)).astype(F32)
    dets = np.concatenate([b, scores[keep, None], scores[keep, None], labels[keep, None]], 1).astype(F32)
    return dets.reshape(-1, 7), total, keep
