"""GPU: test-time augmentation (ABI 16) -- mirrored preprocessing, the candidate exit of the GFL post-processing, the
map-back / merge / NMS launch, and the whole path through Compose and the mmdet surface.

Bit equality is demanded where the arithmetic allows it: the mirrored preprocessing is the unflipped one indexed
differently; glsdet_aug_merge_nms is fed candidates in the dyadic regime of tests/post_reference.py (corners multiples
of 1/64, integer img_w / img_h, scale factors 0.5 / 1 / 2: the map-back is exact and so is every IoU decision) and
compared with tests/tta_reference.merge on all seven columns; on non-dyadic scale factors the mapped coordinates are
compared with the reference's own recorded bbox_mapping_back rows (tests/golden/tta_golden.npz)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import glsdet_oracle as O
from oracle import mpdet_oracle as M
from tests import post_reference as R
from tests import tta_reference as T
from tests.helpers import calibrated_resdet_sd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.5
MEAN = (123.675, 116.28, 103.53)
STD = (58.395, 57.12, 57.375)


@pytest.fixture(scope="module")
def eng():
    from glsdet_amd.engine import Engine
    return Engine("f32")


# ------------------------------------------------------------------------------------------------ mirrored preprocessing
def _pre(src, nh, nw, ph, pw, flip):
    """flip None: the old entry point; else the _ex one.  -> [3, ph, pw] on the device, written into a sentinel-filled buffer"""
    from glsdet_amd import _lib
    lib = _lib.load()
    u8 = src.dtype == torch.uint8
    dst = torch.full((3, ph, pw), SENT, dtype=torch.float32, device="cuda")
    mean, std = (C.c_double * 3)(*MEAN), (C.c_double * 3)(*STD)
    st = torch.cuda.current_stream().cuda_stream
    h, w = src.shape[:2]
    if flip is None:
        fn = lib.glsdet_resize_normalize_pad_u8 if u8 else lib.glsdet_resize_normalize_pad
        _lib.check(fn(src.data_ptr(), h, w, nh, nw, dst.data_ptr(), ph, pw, mean, std, st), "resize_normalize_pad")
    else:
        fn = lib.glsdet_resize_normalize_pad_u8_ex if u8 else lib.glsdet_resize_normalize_pad_ex
        _lib.check(fn(src.data_ptr(), h, w, nh, nw, dst.data_ptr(), ph, pw, mean, std, flip, st), "resize_normalize_pad_ex")
    torch.cuda.synchronize()
    return dst


def _source(h, w, u8, seed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8)
    return (t if u8 else t.float() + torch.rand(h, w, 3, generator=g)).contiguous().cuda()


def _check_flips(src, nh, nw, ph, pw, flips=(1, 2, 3)):
    base = _pre(src, nh, nw, ph, pw, 0)
    assert torch.equal(base, _pre(src, nh, nw, ph, pw, None))              # flip 0 is the old entry point
    pad = torch.ones(ph, pw, dtype=torch.bool, device="cuda")
    pad[:nh, :nw] = False
    assert not bool((base[:, :nh, :nw] == SENT).any()) and bool((base[:, pad] == 0).all())
    for f in flips:
        want = base.clone()
        dims = [d for d, bit in ((2, 1), (1, 2)) if f & bit]
        want[:, :nh, :nw] = torch.flip(base[:, :nh, :nw], dims)
        got = _pre(src, nh, nw, ph, pw, f)
        assert torch.equal(got, want), "flip %d: %d elements differ" % (f, int((got != want).sum()))
    if nh > 1 and nw > 1:
        assert not torch.equal(base, _pre(src, nh, nw, ph, pw, 1))          # the mirror really changes the picture


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("shape", [(37, 53, 45, 61, 64, 64), (37, 53, 37, 53, 64, 64), (37, 53, 1, 1, 3, 5), (37, 53, 45, 61, 45, 61)],
                         ids=["resize_pad", "same_size", "one_pixel", "no_pad"])
def test_mirrored_preprocessing_equals_the_flipped_window_of_the_unflipped_call(u8, shape):
    h, w, nh, nw, ph, pw = shape
    _check_flips(_source(h, w, u8, 7 + h + nh), nh, nw, ph, pw)


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
def test_mirrored_preprocessing_beyond_the_grid_stride_cap(u8):
    nh, nw, ph, pw = 4100, 4093, 4128, 4096
    assert ph * pw > 65535 * 256
    _check_flips(_source(64, 64, u8, 3), nh, nw, ph, pw, flips=(3,))


def test_preprocessing_refuses_an_unknown_flip_code():
    from glsdet_amd import _lib
    lib = _lib.load()
    m = (C.c_double * 3)(1, 1, 1)
    for fn in (lib.glsdet_resize_normalize_pad_ex, lib.glsdet_resize_normalize_pad_u8_ex):
        for flip in (-1, 4):
            assert fn(0x1000, 4, 4, 4, 4, 0x2000, 4, 4, m, m, flip, None) == -1 and "flip" in lib.glsdet_last_error().decode()


# ------------------------------------------------------------------------------------------------ gfl_candidates
import tests.test_post_fuzz as PF  # noqa: E402  (its GFL inputs, level sizes and cases; nothing is copied)


@pytest.mark.parametrize("case", PF.GFL_CASES, ids=[c["id"] for c in PF.GFL_CASES])
def test_gfl_candidates_vs_oracle_pre_nms(eng, case):
    """glsdet_gfl_candidates against oracle.mpdet_oracle.gfl_pre_nms (get_bboxes with rescale=False, with_nms=False):
    counts, labels and order equal; scores to 1e-6; boxes to max(1e-3, 2 x the float32 oracle's distance from the
    float64 one) -- the bound of tests/test_post_fuzz.py's gfl_detect test; rows beyond the count keep the sentinel."""
    from tests.test_resdet import _fp32_view
    n, nc = 2, case["nc"]
    cls, reg = PF._gfl_inputs(case, n)
    _, _, ncut = PF._gfl_seed_conditions(case, cls, reg)                    # asserted, never skipped
    assert ncut > 0 or "cut" not in case["id"]
    pre = {dt: M.gfl_pre_nms([c.to(dt) for c in cls], [r.to(dt) for r in reg], PF.GFL_STRIDES, PF.GFL_SHAPES, case["thr"],
                             case["nms_pre"], None, case["reg_max"]) for dt in (torch.float32, torch.float64)}
    cap = eng.gfl_candidate_cap(PF.GFL_SIZES, nc, case["nms_pre"])
    assert cap == sum(min(case["nms_pre"], h * w * nc) for h, w in PF.GFL_SIZES)
    cb = eng.gfl_candidate_buffers(n, 5, 2 * PF.MAX_CAND, case["nms_pre"], cap)
    cb["cand"].fill_(SENT)
    hw = torch.tensor([[s[0], s[1]] for s in PF.GFL_SHAPES], dtype=torch.float32).cuda()
    cand, count, status = eng.gfl_candidates([_fp32_view(eng, c) for c in cls], [_fp32_view(eng, r) for r in reg],
                                             PF.GFL_STRIDES, nc, case["reg_max"], PF.GFL_IN[0], PF.GFL_IN[1], case["thr"],
                                             cb, img_hw=hw)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    cand, count = cand.cpu().numpy(), count.cpu().numpy()
    err_k = err_o = 0.0
    for i in range(n):
        b32, s32, l32 = (t.numpy() for t in pre[torch.float32][i])
        b64, _, l64 = (t.numpy() for t in pre[torch.float64][i])
        assert np.array_equal(l32, l64), "float32 / float64 oracles select different candidates: pick another seed"
        assert count[i] == len(s32) and 0 < count[i] <= cap
        got = cand[i, : count[i]]
        np.testing.assert_array_equal(got[:, 5].astype(np.int64), l32)
        np.testing.assert_allclose(got[:, 4], s32, atol=1e-6, rtol=0)
        assert (got[:, 6:] == 0).all()
        assert (cand[i, count[i]:] == np.float32(SENT)).all()
        assert (got[:, 4] == 1.0).sum() >= 2                                 # the saturated positions: tied scores, index order
        err_k = max(err_k, float(np.abs(got[:, :4].astype(np.float64) - b64).max()))
        err_o = max(err_o, float(np.abs(b32.astype(np.float64) - b64).max()))
    print("gfl_candidates %s: kernel vs float64 %.3e, float32 oracle vs float64 %.3e, counts %s of cap %d"
          % (case["id"], err_k, err_o, count, cap))
    assert err_k <= max(1e-3, 2 * err_o), (err_k, err_o)


def test_gfl_candidates_refuses_too_small_a_row_capacity(eng):
    from glsdet_amd._lib import GlsdetError
    from tests.test_resdet import _fp32_view
    case = PF.GFL_CASES[0]
    cls, reg = PF._gfl_inputs(case, 1)
    cap = eng.gfl_candidate_cap(PF.GFL_SIZES, case["nc"], case["nms_pre"])
    cb = eng.gfl_candidate_buffers(1, 5, PF.MAX_CAND, case["nms_pre"], cap - 1)
    with pytest.raises(GlsdetError, match="cap"):
        eng.gfl_candidates([_fp32_view(eng, c) for c in cls], [_fp32_view(eng, r) for r in reg], PF.GFL_STRIDES, case["nc"],
                           case["reg_max"], PF.GFL_IN[0], PF.GFL_IN[1], case["thr"], cb)


# ------------------------------------------------------------------------------------------------ aug_merge_nms
SFS = (1.0, 0.5, 2.0)


def _to_aug(boxes, sf, code):
    """original-image boxes (multiples of 1/64 in [0, 64)) -> the augmentation's frame: scaled by sf (0.5 / 1 / 2: exact),
    mirrored inside the integer extent 64 * sf (exact).  -> (rows [m,4], img_h, img_w)"""
    ext = int(64 * sf)
    b = (np.asarray(boxes, np.float32) * np.float32(sf)).astype(np.float32)
    return T.flip_boxes(b, (ext, ext), code), ext, ext


def _aug_inputs(seed, counts, codes, sfs, nc=6, struct="clusters", scores="distinct"):
    """counts[k][b] rows of image b in augmentation k; codes[k][b] / sfs[k][b] its flip code and scale factor.
    -> (rows[k][b] float32 [m,6], metas[k][b] = (img_h, img_w, sf[4], code))"""
    K, n = len(counts), len(counts[0])
    rng = np.random.default_rng([seed, K, n])
    rows = [[None] * n for _ in range(K)]
    metas = [[None] * n for _ in range(K)]
    for b in range(n):
        m = sum(counts[k][b] for k in range(K))
        boxes = R.build_boxes(struct, m, 0.5, rng) if m else np.zeros((0, 4), np.float32)
        obj, conf = R.build_scores(scores, m, rng) if m else (np.zeros(0, np.float32),) * 2
        sc = (obj * conf).astype(np.float32)
        lab = R.build_labels("balanced", m, nc, rng) if m else np.zeros(0, np.int64)
        if m:                                        # bit-equal scores across augmentations, in ONE class only
            tie = np.flatnonzero(lab == 0)
            sc[tie] = np.float32(rng.choice(R.TIE_TABLE, len(tie)) / 256.0)
        perm = rng.permutation(m)
        start = 0
        for k in range(K):
            idx = perm[start:start + counts[k][b]]
            start += counts[k][b]
            sf, code = sfs[k][b], codes[k][b]
            bx, h, w = _to_aug(boxes[idx], sf, code)
            rows[k][b] = np.concatenate([bx, sc[idx, None], lab[idx, None].astype(np.float32)], 1).astype(np.float32).reshape(-1, 6)
            metas[k][b] = (h, w, [sf] * 4, code)
    return rows, metas


def _run_merge(eng, rows, metas, thr, max_det, out_scale=None, slack=3):
    """-> (dets [n, max_det, 7], count [2n]) from glsdet_aug_merge_nms; every buffer is sentinel-filled beyond its count"""
    K, n = len(rows), len(rows[0])
    caps = [max(max(len(rows[k][b]) for b in range(n)) + slack, 1) for k in range(K)]
    mb = eng.aug_merge_buffers(n, caps, max_det)
    cands, counts = [], []
    meta = np.zeros((K, n, 8), np.float32)
    for k in range(K):
        c = np.full((n, caps[k], 8), np.nan, np.float32)                   # rows beyond the count are never read
        for b in range(n):
            c[b, : len(rows[k][b]), :6] = rows[k][b]
            c[b, : len(rows[k][b]), 6:] = 0
            h, w, sf, code = metas[k][b]
            meta[k, b] = [h, w] + list(sf) + [code, 0]
        cands.append(torch.from_numpy(c).cuda())
        counts.append(torch.tensor([len(rows[k][b]) for b in range(n)], dtype=torch.int32).cuda())
    mb["meta"].copy_(torch.from_numpy(meta))
    if out_scale is not None:
        mb["out_scale"].copy_(torch.from_numpy(np.asarray(out_scale, np.float32).reshape(n, 4)))
    mb["dets"].fill_(SENT)
    dets, count, status = eng.aug_merge_nms(cands, counts, thr, mb, use_out_scale=out_scale is not None)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    return dets.cpu().numpy(), count.cpu().numpy()


def _check_merge(eng, rows, metas, thr, max_det, out_scale=None, slack=3):
    K, n = len(rows), len(rows[0])
    dets, count = _run_merge(eng, rows, metas, thr, max_det, out_scale, slack)
    totals = []
    for b in range(n):
        want, total, keep = T.merge([rows[k][b] for k in range(K)], [metas[k][b] for k in range(K)], thr, max_det,
                                    None if out_scale is None else out_scale[b])
        assert count[b] == len(want) and count[n + b] == total, (b, count.tolist(), len(want), total)
        np.testing.assert_array_equal(dets[b, : len(want)], want)
        assert (dets[b, len(want):] == np.float32(SENT)).all()
        totals.append((total, sum(len(rows[k][b]) for k in range(K)), keep))
    return totals


@pytest.mark.parametrize("scale", [False, True], ids=["no_out_scale", "out_scale"])
@pytest.mark.parametrize("K", [1, 2, 3, 6, 12])
def test_aug_merge_nms_equals_the_naive_reference(eng, K, scale):
    """n = 2 with different metas per image; every flip code and scale factor occurs (K >= 3); suppression across
    augmentations happens (the boxes of one cluster are dealt to different augmentations)."""
    counts = [[150 + 17 * k, 90 + 5 * k] for k in range(K)]
    codes = [[k % 4, (k + 1 + k // 4) % 4] for k in range(K)]
    sfs = [[SFS[k % 3], SFS[(k + 2) % 3]] for k in range(K)]
    rows, metas = _aug_inputs(11 + K, counts, codes, sfs)
    out_scale = [[2.0, 0.5, 2.0, 0.5], [0.5, 1.0, 0.5, 1.0]] if scale else None
    totals = _check_merge(eng, rows, metas, 0.5, 2000, out_scale)
    for total, m, _ in totals:
        assert 0 < total < m                                                 # something is kept, something suppressed


def test_aug_merge_nms_max_det_cuts(eng):
    rows, metas = _aug_inputs(5, [[200], [180], [160]], [[0], [1], [3]], [[1.0], [2.0], [0.5]])
    (total, _, _), = _check_merge(eng, rows, metas, 0.5, 7, [[2.0, 2.0, 2.0, 2.0]])
    assert total > 7


@pytest.mark.parametrize("counts", [[[120, 0], [0, 0], [75, 40]], [[0, 0], [0, 0], [0, 0]]], ids=["empty_in_the_middle", "all_empty"])
def test_aug_merge_nms_empty_augmentations(eng, counts):
    rows, metas = _aug_inputs(9, counts, [[0, 1], [2, 3], [1, 0]], [[1.0, 2.0], [0.5, 0.5], [2.0, 1.0]])
    totals = _check_merge(eng, rows, metas, 0.5, 50)
    if not any(sum(c) for c in counts):
        assert all(t[0] == 0 for t in totals)                                # count 0 and (checked above) no row written


def test_aug_merge_nms_tie_keeps_the_row_of_the_earlier_augmentation(eng):
    """The same box unflipped in augmentation 0 and mirrored in augmentation 1, bit-equal score, same class: the row of
    augmentation 0 is kept, its twin suppressed (IoU 1 > thr).  A second pair with the classes apart keeps both."""
    box = np.float32([[8.25, 9.5, 24.0, 30.75], [40.0, 8.0, 56.5, 24.0]])
    a0 = np.concatenate([box, np.float32([[0.75, 2], [0.5, 1]])], 1)
    a1 = np.concatenate([T.flip_boxes(box, (64, 64), 1), np.float32([[0.75, 2], [0.5, 3]])], 1)
    metas = [[(64, 64, [1.0] * 4, 0)], [(64, 64, [1.0] * 4, 1)]]
    (total, _, keep), = _check_merge(eng, [[a0], [a1]], metas, 0.5, 10)
    assert total == 3 and keep.tolist() == [0, 1, 3]


@pytest.mark.parametrize("total", [4096, 4097])
def test_aug_merge_nms_around_4096_merged_candidates(eng, total):
    rows, metas = _aug_inputs(total, [[2048], [total - 2048]], [[0], [1]], [[1.0], [2.0]])
    (kept, m, _), = _check_merge(eng, rows, metas, 0.5, 5000)
    assert m == total and 0 < kept < total


def test_aug_merge_nms_full_lists_at_the_capacity_limit(eng):
    """The capacities sum to exactly GLS_NMS_MAXW * 64 = 32768 and every list is full to its last row (no slack): the
    rank sort, the 512-word mask rows and the scan's shared arrays at their upper limit.  Three augmentations with three
    scale factors and flips; 40 classes keep the naive reference at some 10^7 pairs."""
    counts = [[16384], [8192], [8192]]
    rows, metas = _aug_inputs(32768, counts, [[0], [1], [3]], [[1.0], [2.0], [0.5]], nc=40)
    (kept, m, _), = _check_merge(eng, rows, metas, 0.5, 32768, slack=0)
    assert m == 32768 and 4096 < kept < m


def test_aug_merge_nms_capacity_limit(eng):
    """The capacities may sum to GLS_NMS_MAXW * 64 = 32768: accepted (and run, on empty lists); 32769 is refused with
    GLSDET_E_ARG and a message that names the limit -- an argument check, nothing is launched."""
    from glsdet_amd._lib import GlsdetError
    lib = eng.lib
    mb = eng.aug_merge_buffers(1, [16384, 16384], 10)
    cands = [torch.zeros(1, 16384, 8, device="cuda") for _ in range(2)]
    counts = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    _, count, _ = eng.aug_merge_nms(cands, counts, 0.5, mb)
    torch.cuda.synchronize()
    assert count.cpu().tolist() == [0, 0]
    with pytest.raises(GlsdetError):
        eng.aug_merge_buffers(1, [16384, 16385], 10)
    pa = (C.c_void_p * 2)(cands[0].data_ptr(), cands[1].data_ptr())
    pc = (C.c_void_p * 2)(counts[0].data_ptr(), counts[1].data_ptr())
    rc = lib.glsdet_aug_merge_nms(pa, pc, (C.c_int32 * 2)(16384, 16385), 2, 1, mb["meta"].data_ptr(), 0.5, 10, None,
                                  mb["dets"].data_ptr(), mb["count"].data_ptr(), mb["status"].data_ptr(), mb["ws"].data_ptr(),
                                  mb["ws"].numel(), None)
    assert rc == -1 and "32768" in lib.glsdet_last_error().decode()
    for K in (0, 13):
        rc = lib.glsdet_aug_merge_nms(pa, pc, (C.c_int32 * 2)(8, 8), K, 1, mb["meta"].data_ptr(), 0.5, 10, None,
                                      mb["dets"].data_ptr(), mb["count"].data_ptr(), mb["status"].data_ptr(),
                                      mb["ws"].data_ptr(), mb["ws"].numel(), None)
        assert rc == -1 and "GLSDET_MAX_AUGS" in lib.glsdet_last_error().decode()


def test_aug_merge_nms_map_back_on_non_dyadic_scale_factors_equals_the_recorded_reference(eng):
    """iou_thr = 1.0 suppresses nothing, so every candidate comes out, in score order: image i is golden case i, its
    boxes once per flip code (K = 4); the coordinates equal the reference's bbox_mapping_back rows bit for bit."""
    g = np.load(T.GOLDEN)
    n = len(g["img_shape"])
    N = len(g["boxes/0"])
    rng = np.random.default_rng(4)
    rows, metas, want = [[None] * n for _ in range(4)], [[None] * n for _ in range(4)], []
    for i in range(n):
        sc = ((1 + rng.permutation(4 * N)) / np.float32(4 * N + 1)).astype(np.float32).reshape(4, N)      # distinct
        lab = rng.integers(0, 3, (4, N)).astype(np.float32)
        h, w = (int(v) for v in g["img_shape"][i])
        for code in range(4):
            rows[code][i] = np.concatenate([g["boxes/%d" % i], sc[code][:, None], lab[code][:, None]], 1).astype(np.float32)
            metas[code][i] = (h, w, g["scale_factor"][i], code)
        back = np.concatenate([g["back/%d/%d" % (i, code)] for code in range(4)])
        order = np.argsort(-sc.reshape(-1), kind="stable")
        want.append(np.concatenate([back, sc.reshape(-1, 1), sc.reshape(-1, 1), lab.reshape(-1, 1)], 1)[order].astype(np.float32))
    dets, count = _run_merge(eng, rows, metas, 1.0, 4 * N + 5)
    for i in range(n):
        assert count[i] == count[n + i] == 4 * N
        np.testing.assert_array_equal(dets[i, : 4 * N], want[i])


# ------------------------------------------------------------------------------------------------ end to end
def _tta_pipeline(cfg, scales, flip, directions="horizontal"):
    msfa = dict(cfg.data.test.pipeline[1])
    assert msfa["type"] == "MultiScaleFlipAug"
    msfa.update(img_scale=scales, flip=flip, flip_direction=directions)
    return [msfa]


def _expect(det, data, thr, iou, nms_pre, max_per_img, dtype):
    """The expectation from the kernel's OWN logits (the network is chaotic at 2e-4): per augmentation forward_raw ->
    oracle gfl_pre_nms (rescale=False) -> the reference map-back -> oracle batched_nms over the union -> max_per_img.
    -> (boxes, scores, labels, keep, augmentation of each candidate, kept by the NMS of its own augmentation alone)"""
    boxes, scores, labels, aug, alone = [], [], [], [], []
    for k, (img, meta) in enumerate(zip(data["img"], data["img_metas"])):
        cls, reg = det.forward_raw(img[None])
        cls, reg = [c.cpu().to(dtype) for c in cls], [r.cpu().to(dtype) for r in reg]
        (b, s, l), = M.gfl_pre_nms(cls, reg, det.cfg["strides"][:len(cls)], [meta["img_shape"]], thr, nms_pre, None, det.cfg["reg_max"])
        code = T.DIRECTIONS.index(meta["flip_direction"] if meta["flip"] else None)
        if dtype == torch.float32:
            b = T.map_back(b.numpy(), meta["img_shape"], meta["scale_factor"], code)
        else:
            b = _flip64(b.numpy(), meta["img_shape"], code) / np.asarray(meta["scale_factor"], np.float64).reshape(1, 4)
        s, l = s.numpy(), l.numpy()
        own = np.zeros(len(s), bool)
        if len(s):
            own[O.batched_nms(b, s, l.astype(np.float32), iou)] = True
        boxes.append(b), scores.append(s), labels.append(l), aug.append(np.full(len(s), k)), alone.append(own)
    boxes, scores, labels = np.concatenate(boxes), np.concatenate(scores), np.concatenate(labels)
    keep = O.batched_nms(boxes, scores, labels.astype(np.float32), iou)
    return boxes, scores, labels, keep[:max_per_img], np.concatenate(aug), np.concatenate(alone)


def _flip64(b, img_shape, code):
    out = b.astype(np.float64).copy()
    h, w = float(img_shape[0]), float(img_shape[1])
    if code & 1:
        out[:, 0], out[:, 2] = w - b[:, 2], w - b[:, 0]
    if code & 2:
        out[:, 1], out[:, 3] = h - b[:, 3], h - b[:, 1]
    return out


@pytest.fixture()
def shim_path():
    import sys
    shim, names = os.path.join(ROOT, "glsdet_amd", "compat"), ("mmdet", "mmcv", "pycocotools", "cv2")
    saved = {k: v for k, v in sys.modules.items() if k.split(".")[0] in names}
    for k in saved:
        del sys.modules[k]
    sys.path.insert(0, shim)
    yield
    sys.path.remove(shim)
    for k in [k for k in sys.modules if k.split(".")[0] in names]:
        del sys.modules[k]
    sys.modules.update(saved)


@pytest.mark.parametrize("cfg", ["coarse_det.py", "mp_det_res50.py"])
def test_multi_scale_flip_through_compose_and_the_surface(shim_path, cfg):
    """A synthetic uint8 frame -> Compose(two scales with different padded shapes x horizontal flip, K = 4) ->
    model(return_loss=False, rescale=True, **data), f32 engine, against the expectation built from the kernel's own
    logits; per class rtol 1e-4 / atol 1e-3 (tests/test_mmdet_surface.py's bound).
    The logits of the synthetic net differ from process to process at 1e-6 (kernel selection), so every run draws new
    candidates: the float32 / float64 condition is on the kept SET, and the threshold keeps max_per_img from cutting --
    with a cut, which of two float32-equal scores falls behind it differs between the two expectations (seen once on an
    MI355X with 150 passing pairs and max_per_img = 100 binding)."""
    from mmdet.datasets.pipelines import Compose
    from glsdet_amd.mmdet_surface import init_detector
    from tests.golden.make_golden import synth_image
    kind = "mpdet" if cfg.startswith("mp_") else "gfl"
    model = init_detector(os.path.join(ROOT, "configs/UFPMP-Det", cfg))
    model.hip_dtype = "f32"
    model.load_state_dict(calibrated_resdet_sd(kind, 3, O.synth_input((2, 3, 128, 160), 11)))
    frame = np.ascontiguousarray(synth_image((100, 150), 5)[:, :, ::-1])                   # BGR uint8
    data = Compose(_tta_pipeline(model.cfg, [(160, 128), (224, 160)], True))(dict(img=frame))
    assert len(data["img"]) == 4 and [m["flip"] for m in data["img_metas"]] == [False, True, False, True]
    assert data["img"][0].shape != data["img"][2].shape and data["img"][0].shape == data["img"][1].shape
    w0 = data["img_metas"][0]["img_shape"][1]
    assert torch.equal(data["img"][1][:, :, :w0], torch.flip(data["img"][0][:, :, :w0], [2]))
    det = model._detector()
    # random heads fire everywhere: a threshold that 100 (position, class) pairs of augmentation 0 pass -- few enough that
    # max_per_img does not cut (asserted below): which of two nearly equal scores falls behind a cut is not what is tested
    p = torch.sigmoid(torch.cat([c.flatten() for c in det.forward_raw(data["img"][0][None])[0]])).cpu()
    top = torch.topk(p, 101).values.double()
    thr = float(np.float32((top[-1] + top[-2]) / 2))                          # between two scores: no borderline pair
    tc = model.bbox_head.test_cfg
    tc["score_thr"] = thr
    iou, nms_pre, max_per_img = float(tc["nms"]["iou_threshold"]), int(tc.get("nms_pre", 1000)), int(tc.get("max_per_img", 100))
    wrapped = dict(img=[t[None] for t in data["img"]], img_metas=[[m] for m in data["img_metas"]])
    with torch.no_grad():
        res = model(return_loss=False, rescale=True, **wrapped)
    assert len(res) == 1 and len(res[0]) == 10
    b32, s32, l32, k32, aug, alone = _expect(det, data, thr, iou, nms_pre, max_per_img, torch.float32)
    _, _, l64, k64, _, _ = _expect(det, data, thr, iou, nms_pre, max_per_img, torch.float64)
    assert len(k32) < max_per_img and len(k64) < max_per_img, "max_per_img cuts: lower the number of passing pairs"
    assert np.array_equal(l32, l64) and set(k32.tolist()) == set(k64.tolist()), \
        "float32 / float64 expectations keep different sets: pick another seed"
    n_det = 0
    for c in range(10):
        kc = k32[l32[k32] == c]
        want = np.concatenate([b32[kc], s32[kc, None]], 1).astype(np.float32)
        assert res[0][c].dtype == np.float32 and res[0][c].shape == want.shape, (c, res[0][c].shape, want.shape)
        np.testing.assert_allclose(res[0][c], want, rtol=1e-4, atol=1e-3)
        n_det += len(want)
    assert n_det > 0
    print("tta %s: thr %.4f, candidates per augmentation %s, kept per augmentation %s, kept alone but not merged %d"
          % (cfg, thr, np.bincount(aug, minlength=4), np.bincount(aug[k32], minlength=4), int((alone & ~np.isin(np.arange(len(aug)), k32)).sum())))
    assert (np.bincount(aug[k32], minlength=4) > 0).all()                      # every augmentation contributes a kept box
    full = O.batched_nms(b32, s32, l32.astype(np.float32), iou)
    assert (alone & ~np.isin(np.arange(len(aug)), full)).any()                 # a box its own augmentation keeps falls to another's
    # rescale=False: the boxes at augmentation 0's input scale
    with torch.no_grad():
        res0 = model(return_loss=False, rescale=False, **wrapped)
    sf0 = np.asarray(data["img_metas"][0]["scale_factor"], np.float32)
    for c in range(10):
        np.testing.assert_array_equal(res0[0][c][:, :4], (res[0][c][:, :4] * sf0).astype(np.float32))
        np.testing.assert_array_equal(res0[0][c][:, 4], res[0][c][:, 4])
    # K = 1 is simple_test, bit for bit
    one = Compose(_tta_pipeline(model.cfg, (160, 128), False))(dict(img=frame))
    assert len(one["img"]) == 1 and torch.equal(one["img"][0], data["img"][0])
    with torch.no_grad():
        r1 = model(return_loss=False, rescale=True, img=[one["img"][0][None]], img_metas=[[one["img_metas"][0]]])
        r2 = model.simple_test(one["img"][0][None], [one["img_metas"][0]], rescale=True)
    for a, b in zip(r1[0], r2[0]):
        np.testing.assert_array_equal(a, b)
    with pytest.raises(AssertionError):                                         # detectors/base.py:149
        model(return_loss=False, img=[torch.zeros(2, 3, 32, 32)] * 2, img_metas=[[{}, {}]] * 2)


def test_the_yolox_surface_still_refuses_test_time_augmentation():
    from glsdet_amd.mmdet_surface import init_detector
    model = init_detector(os.path.join(ROOT, "configs/yolox/yolox_s_visdrone.py"))
    x = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="dense_test_mixins.py:68"):
        model(return_loss=False, img=[x, x], img_metas=[[{}], [{}]])
