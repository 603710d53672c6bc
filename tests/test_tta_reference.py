"""CPU: the naive test-time-augmentation reference (tests/tta_reference.py) against the reference's own recorded
bbox_flip / bbox_mapping_back outputs (tests/golden/tta_golden.npz, tools/make_tta_golden.py), and the augmentation
order of the `Compose` shim against MultiScaleFlipAug's (test_time_aug.py:96-108)."""
import os
import sys

import numpy as np
import pytest

from tests import tta_reference as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "glsdet_amd", "compat")
SHIMMED = ("mmdet", "mmcv", "pycocotools", "cv2")


@pytest.fixture(scope="module")
def golden():
    return np.load(T.GOLDEN)


def _cases(g):
    for ci in range(len(g["img_shape"])):
        yield ci, g["boxes/%d" % ci], tuple(int(v) for v in g["img_shape"][ci]), g["scale_factor"][ci]


def test_golden_covers_dyadic_and_non_dyadic_scale_factors(golden):
    sf = golden["scale_factor"]
    assert sf.dtype == np.float32 and sf.shape[1] == 4
    for v in (1.0, 0.5, 2.0):
        assert (sf == v).all(1).any()
    mant = np.frexp(sf.astype(np.float64))[0]
    assert ((mant != 0.5).any(1)).sum() >= 4                       # rows that are no power of two
    assert (sf[:, 0] != sf[:, 1]).any()                            # x and y factors differ somewhere


def test_map_back_equals_the_recorded_reference_bit_for_bit(golden):
    rows = 0
    for ci, boxes, shape, sf in _cases(golden):
        for code in range(4):
            np.testing.assert_array_equal(T.map_back(boxes, shape, sf, code), golden["back/%d/%d" % (ci, code)])
            if code:
                np.testing.assert_array_equal(T.flip_boxes(boxes, shape, code), golden["flip/%d/%d" % (ci, code)])
            rows += len(boxes)
    assert rows >= 4 * 8 * 12


@pytest.mark.parametrize("mutation", ["swap", "padded", "reciprocal"])
def test_a_wrong_map_back_changes_some_golden_row(golden, mutation):
    """x1 / x2 swapped in the mirror, the padded width instead of img_shape's, a multiplication by the reciprocal:
    each must be visible in the golden, or the golden would not pin what it is there to pin."""
    changed = 0
    for ci, boxes, shape, sf in _cases(golden):
        mut = ("padded", -(-shape[1] // 32) * 32, -(-shape[0] // 32) * 32) if mutation == "padded" else mutation
        for code in range(4):
            changed += int((T.map_back(boxes, shape, sf, code, mutate=mut) != golden["back/%d/%d" % (ci, code)]).any(1).sum())
    assert changed > 0


def test_merge_keeps_the_earlier_augmentation_of_a_tie_and_cuts():
    a = np.float32([[8, 8, 24, 24, 0.75, 2], [40, 8, 56, 24, 0.5, 2]])
    twin = np.float32([[64 - 24, 8, 64 - 8, 24, 0.75, 2]])                    # the first box, mirrored in a 64-wide picture
    metas = [(64, 64, [1, 1, 1, 1], 0), (64, 64, [1, 1, 1, 1], 1)]
    dets, total, keep = T.merge([a, twin], metas, 0.5, 10)
    assert total == 2 and keep.tolist() == [0, 1]
    np.testing.assert_array_equal(dets[0], np.float32([8, 8, 24, 24, 0.75, 0.75, 2]))
    dets, total, keep = T.merge([a, twin], metas, 0.5, 1, out_scale=[2, 2, 2, 2])
    assert total == 2 and len(dets) == 1
    np.testing.assert_array_equal(dets[0, :4], np.float32([16, 16, 48, 48]))
    dets, total, _ = T.merge([np.zeros((0, 6), np.float32)] * 2, metas, 0.5, 5)
    assert dets.shape == (0, 7) and total == 0


# ------------------------------------------------------------------------------------------------ Compose (no GPU: construction only)
@pytest.fixture()
def shim_path():
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in SHIMMED}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, SHIM)
    yield
    sys.path.remove(SHIM)
    for k in [k for k in sys.modules if k.split(".")[0] in SHIMMED]:
        del sys.modules[k]
    sys.modules.update(saved)


INNER = [dict(type="Resize", keep_ratio=True), dict(type="RandomFlip"),
         dict(type="Normalize", mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True),
         dict(type="Pad", size_divisor=32), dict(type="ImageToTensor", keys=["img"]), dict(type="Collect", keys=["img"])]
SCALES = [(1333, 800), (1000, 600), (1666, 1000)]


@pytest.mark.parametrize("nscales", [1, 2, 3])
@pytest.mark.parametrize("flip", [None, "horizontal", ["horizontal", "vertical", "diagonal"]], ids=["off", "h", "hvd"])
def test_compose_orders_the_augmentations_like_multiscaleflipaug(shim_path, nscales, flip):
    from mmdet.datasets.pipelines import Compose
    scales = SCALES[:nscales]
    msfa = dict(type="MultiScaleFlipAug", img_scale=scales if nscales > 1 else scales[0], flip=flip is not None, transforms=INNER)
    if flip is not None:
        msfa["flip_direction"] = flip
    c = Compose([msfa])
    want = T.aug_order(scales, flip is not None, flip if flip is not None else "horizontal")
    assert c.augs == want
    assert len(c.augs) == nscales * (1 + (0 if flip is None else (len(flip) if isinstance(flip, list) else 1)))
    assert c.augs[0] == (scales[0], False, None) and c.args["img_scale"] == scales[0]


def test_compose_flip_without_randomflip_flips_nothing_and_list_of_one_scale(shim_path):
    from mmdet.datasets.pipelines import Compose
    inner = [s for s in INNER if s["type"] != "RandomFlip"]
    c = Compose([dict(type="MultiScaleFlipAug", img_scale=[(1333, 800)], flip=True, transforms=inner)])
    assert c.augs == [((1333, 800), False, None)]


def test_compose_still_refuses_scale_factor_and_a_pipeline_without_keep_ratio_resize(shim_path):
    from mmdet.datasets.pipelines import Compose
    with pytest.raises(NotImplementedError):
        Compose([dict(type="MultiScaleFlipAug", scale_factor=[0.5, 1.0], flip=True, transforms=INNER)])
    with pytest.raises(NotImplementedError):
        Compose([dict(type="MultiScaleFlipAug", img_scale=SCALES, flip=True,
                      transforms=[dict(type="Resize", keep_ratio=False)] + INNER[1:])])
    with pytest.raises(NotImplementedError):
        Compose([dict(type="MultiScaleFlipAug", img_scale=SCALES, flip=True, transforms=INNER[1:])])
    with pytest.raises(NotImplementedError):                                   # tests/test_compat_shim.py's case
        Compose([dict(type="MultiScaleFlipAug", img_scale=(1333, 800), flip=True, transforms=[])])


# ------------------------------------------------------------------------------------------------ host-side argument checks
def test_new_entry_points_refuse_bad_arguments_before_anything_is_launched():
    """No GPU: the pointers are never dereferenced.  33 769 > 32 768 candidates, K outside 1..12 and a flip code outside
    0..3 are GLSDET_E_ARG with a message that says why."""
    import ctypes as C
    from glsdet_amd import _lib
    lib = _lib.load()
    err = lambda: lib.glsdet_last_error().decode()
    pa, pc = (C.c_void_p * 2)(0x10000, 0x20000), (C.c_void_p * 2)(0x30000, 0x30100)
    call = lambda caps, K: lib.glsdet_aug_merge_nms(pa, pc, (C.c_int32 * 2)(*caps), K, 1, 0x40000, 0.5, 10, None, 0x50000,
                                                    0x60000, 0x70000, 0x100000, 1 << 40, None)
    assert call((16384, 16385), 2) == -1 and "32768" in err()
    assert call((8, 8), 0) == -1 and call((8, 8), 13) == -1 and "GLSDET_MAX_AUGS" in err()
    assert lib.glsdet_aug_merge_workspace_bytes(1, (C.c_int32 * 2)(16384, 16385), 2) == 0
    assert lib.glsdet_aug_merge_workspace_bytes(1, (C.c_int32 * 2)(16384, 16384), 2) > 32768 * 512 * 8
    m = (C.c_double * 3)(1, 1, 1)
    for fn in (lib.glsdet_resize_normalize_pad_ex, lib.glsdet_resize_normalize_pad_u8_ex):
        assert fn(0x1000, 4, 4, 4, 4, 0x2000, 4, 4, m, m, 4, None) == -1 and "flip" in err()
    assert lib.glsdet_gfl_candidates_workspace_bytes(1, 9, 100) == 0 and lib.glsdet_gfl_candidates_workspace_bytes(2, 5, 4096) > 0
