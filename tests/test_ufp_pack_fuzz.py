"""GPU: glsdet_ufp_pack against the scalar restatement (tests/ufp_pack_reference.py, pinned to the reference on the CPU by
tests/test_ufp_pack_reference.py).  All four output buffers are sentinel-filled and compared whole; chips and header bit
for bit.  Then the surface: torch.ops.glsdet.ufp_pack, one graph capture, mosaic / merge on a DevicePacking, and the
two-stage drivers in packing="device" against packing="host"."""
import os

import numpy as np
import pytest

from tests import ufp_pack_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT_D, SENT_F, SENT_I = -7.25e9, -3.5e7, 0x5A5A5A5A
_want = {}


def golden_scenes():
    g = np.load(os.path.join(ROOT, "tests", "golden", "ufp_pack_golden.npz"))
    out = {}
    for name in g["names"].tolist():
        expand, W, H = g[name + "/params"]
        out[name] = (g[name + "/boxes"], g[name + "/labels"], float(expand), int(W), int(H))
    return out


def fixed_scene(seed, n, wh=(1360, 765), size=(6, 220)):
    """as R.random_scene with the image size given: scenes of one call share expand and the image"""
    rng = np.random.default_rng([seed, 0x0FC])
    W, H = wh
    c = rng.uniform(0, 1, (n, 2)) * [W, H]
    s = np.exp(rng.uniform(np.log(size[0]), np.log(size[1]), (n, 2)))
    b = np.concatenate([c - s / 2, c + s / 2], 1)
    b[:, 0::2] = np.clip(b[:, 0::2], 0, W - 1)
    b[:, 1::2] = np.clip(b[:, 1::2], 0, H - 1)
    return b.astype(np.float32), rng.integers(0, 10, n).astype(np.int64), 1.5, W, H


def want_of(key, scene):
    """the restatement's answer, computed once per scene"""
    if key not in _want:
        _want[key] = R.ufp_pack(*scene)
    return _want[key]


def dets_of(scenes, max_det, counts=None, seed=0):
    """fp32 [n_img, max_det, 7] rows x1,y1,x2,y2,score,score,label; rows beyond the count are dirty (large, NaN, inf)"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(-1e6, 1e6, (len(scenes), max_det, 7)).astype(np.float32)
    d[:, ::3, 0] = np.nan
    d[:, 1::3, 3] = np.inf
    cnt = np.zeros(len(scenes), np.int32)
    for i, (boxes, labels, _, _, _) in enumerate(scenes):
        n = len(boxes)
        cnt[i] = n
        d[i, :n, :4] = boxes
        d[i, :n, 4] = d[i, :n, 5] = np.linspace(0.9, 0.1, n) if n else 0
        d[i, :n, 6] = labels
    if counts is not None:
        cnt[:] = counts
    return d, cnt


def run_kernel(scenes, max_det, counts=None):
    """one C-ABI call on sentinel-filled buffers -> (chips, chips_floor, header, status) as numpy"""
    import torch
    from glsdet_amd import _lib
    lib = _lib.load()
    d, cnt = dets_of(scenes, max_det, counts)
    n_img = len(scenes)
    dets, count = torch.from_numpy(d).cuda(), torch.from_numpy(cnt).cuda()
    chips = torch.full((n_img, max_det, 7), SENT_D, dtype=torch.float64, device="cuda")
    floor = torch.full((n_img, max_det, 7), SENT_F, dtype=torch.float32, device="cuda")
    header = torch.full((n_img, 4), SENT_D, dtype=torch.float64, device="cuda")
    status = torch.full((n_img,), SENT_I, dtype=torch.int32, device="cuda")
    _, _, expand, W, H = scenes[0]
    assert all(s[2:] == scenes[0][2:] for s in scenes)
    _lib.check(lib.glsdet_ufp_pack(dets.data_ptr(), count.data_ptr(), n_img, max_det, expand, W, H, chips.data_ptr(), floor.data_ptr(),
                                   header.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream), "ufp_pack")
    torch.cuda.synchronize()
    return chips.cpu().numpy(), floor.cpu().numpy(), header.cpu().numpy(), status.cpu().numpy()


def expected(wants, max_det, bad=()):
    """the four buffers as they must be, sentinels where nothing is written; bad: {image: count as read}"""
    n_img = len(wants)
    chips = np.full((n_img, max_det, 7), SENT_D, np.float64)
    floor = np.full((n_img, max_det, 7), SENT_F, np.float32)
    header = np.zeros((n_img, 4), np.float64)
    status = np.zeros(n_img, np.int32)
    for i, (n_boxes, (c, cw, ch)) in enumerate(wants):
        if i in dict(bad):
            header[i, 0], status[i] = dict(bad)[i], 1
            continue
        c = np.asarray(c, np.float64).reshape(-1, 7)
        chips[i, : len(c)] = c
        floor[i, : len(c)] = np.floor(c).astype(np.float32)
        header[i] = [n_boxes, len(c), cw, ch]
    return chips, floor, header, status


def assert_whole(got, want, what):
    for g, w, name in zip(got, want, ("chips", "chips_floor", "header", "status")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        gi, wi = (g.view(np.int64), w.view(np.int64)) if g.dtype == np.float64 else (g.view(np.int32), w.view(np.int32))
        assert np.array_equal(gi, wi), (what, name, np.argwhere(gi != wi)[:4].tolist())


def check_scenes(keys_scenes, max_det, what):
    scenes = [s for _, s in keys_scenes]
    wants = [(len(s[0]), want_of(k, s)) for k, s in keys_scenes]
    assert_whole(run_kernel(scenes, max_det), expected(wants, max_det), what)


# ---------------------------------------------------------------------------------- kernel against restatement
def test_every_committed_scene():
    for name, sc in golden_scenes().items():
        check_scenes([(name, sc)], len(sc[0]) + 3, name)


@pytest.mark.parametrize("block", range(4))
def test_random_scenes(block):
    for seed in range(50 * block, 50 * block + 50):                    # 200 scenes of 1..120 boxes, every fifth integer-valued
        sc = R.random_scene(seed, integer=seed % 5 == 0)
        check_scenes([(("random", seed), sc)], len(sc[0]) + (seed % 4), ("random", seed))


def test_three_images_ragged_with_an_empty_one_in_the_middle():
    ks = [(("fixed", 1, 70), fixed_scene(1, 70)), (("fixed", 2, 0), fixed_scene(2, 0)), (("fixed", 3, 23), fixed_scene(3, 23))]
    check_scenes(ks, 75, "ragged")


def test_max_det_at_the_limit_fully_populated():
    """1575 boxes over one frame: every loop runs its 25 chunks; the boxes overlap into a few regions (which also keeps
    the restatement quick)"""
    from glsdet_amd import _lib
    limit = _lib.load().glsdet_ufp_pack_max_boxes()
    check_scenes([(("fixed", 4, limit), fixed_scene(4, limit, wh=(1920, 1080)))], limit, "limit")


def test_many_regions():
    """300 small boxes that never merge: more than 64 rectangles in every fill scan, sort and claim"""
    rng = np.random.default_rng(5)
    b = []
    for i in range(300):
        x0, y0 = 20.0 + 196.0 * (i % 20), 20.0 + 196.0 * (i // 20)
        w, h = float(rng.integers(8, 25)) * 2, float(rng.integers(8, 25)) * 2          # few distinct sizes: equal-size claims
        b.append([x0, y0, x0 + w, y0 + h])
    order = rng.permutation(300)
    sc = (np.asarray(b, np.float32)[order], rng.integers(0, 10, 300).astype(np.int64), 1.5, 4000, 3000)
    want = want_of("many", sc)
    assert len(want[0]) == 300
    check_scenes([("many", sc)], 300, "many")


def test_count_out_of_range_sets_the_status_bit_and_leaves_the_others_alone():
    a, b = fixed_scene(6, 40), fixed_scene(7, 17)
    for bad_count in (51, -1):
        got = run_kernel([a, b, a], 50, counts=[40, bad_count, 40])
        wants = [(40, want_of(("fixed", 6, 40), a)), (0, ([], 0.0, 0.0)), (40, want_of(("fixed", 6, 40), a))]
        assert_whole(got, expected(wants, 50, bad=[(1, bad_count)]), bad_count)


# ---------------------------------------------------------------------------------- surface and wiring
def test_torch_op_and_one_graph_capture():
    import torch
    import glsdet_amd.torch_ops  # noqa: F401
    a, b = fixed_scene(8, 60), fixed_scene(9, 35)
    d, cnt = dets_of([a], 64)
    dets, count = torch.from_numpy(d).cuda(), torch.from_numpy(cnt).cuda()
    out = torch.ops.glsdet.ufp_pack(dets, count, 1.5, 1360, 765)
    torch.cuda.synchronize()
    wa, wb = want_of(("fixed", 8, 60), a), want_of(("fixed", 9, 35), b)

    def check(out, scene, want):
        chips, floor, header, status = (o.cpu().numpy() for o in out)
        k = len(want[0])
        assert header.tolist() == [[len(scene[0]), k, want[1], want[2]]] and status.tolist() == [0]
        assert np.array_equal(chips[0, :k].view(np.int64), np.asarray(want[0], np.float64).view(np.int64))
        assert np.array_equal(floor[0, :k], np.floor(np.asarray(want[0])).astype(np.float32))
    check(out, a, wa)
    # a single kernel node; the replay reads the buffers as they are then
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = torch.ops.glsdet.ufp_pack(dets, count, 1.5, 1360, 765)
    d2, cnt2 = dets_of([b], 64, seed=1)
    dets.copy_(torch.from_numpy(d2))
    count.copy_(torch.from_numpy(cnt2))
    g.replay()
    torch.cuda.synchronize()
    check(out, b, wb)


def _image(H, W, seed):
    from tests.test_preprocess import synth_image
    return synth_image((H, W), seed)[:, :, ::-1].copy()


def test_mosaic_and_merge_take_a_device_packing():
    import torch
    from glsdet_amd.ufp import DevicePacking, UfpSecondStage
    W, H = 420, 300
    sc = fixed_scene(10, 14, wh=(W, H), size=(6, 60))
    d, cnt = dets_of([sc], 20)
    stage = UfpSecondStage()
    pk = stage.pack(torch.from_numpy(d[0]).cuda(), torch.from_numpy(cnt).cuda(), (W, H), 1.5)
    want = want_of(("fixed", 10, 14, W), sc)
    assert isinstance(pk, DevicePacking) and (pk.n_boxes, pk.n_chips, pk.canvas_w, pk.canvas_h) == (14, len(want[0]), want[1], want[2])
    assert np.array_equal(np.asarray(pk.chips).view(np.int64), np.asarray(want[0], np.float64).view(np.int64))
    img = torch.from_numpy(_image(H, W, 5)).cuda()
    on_dev = stage.mosaic(img, pk, pk.canvas_w, pk.canvas_h).cpu().numpy()
    on_host = stage.mosaic(img, pk.chips, pk.canvas_w, pk.canvas_h).cpu().numpy()
    assert np.array_equal(on_dev, on_host) and on_host.max() > 0
    rng = np.random.default_rng(3)
    rows = []
    for chip in pk.chips:                                # detections inside every chip, clustered so that the NMS bites
        ox, oy, w, h, nx, ny, s = [np.floor(v) for v in chip]
        for _ in range(4):
            bw, bh = rng.uniform(4, max(5, w * s / 3)), rng.uniform(4, max(5, h * s / 3))
            x, y = nx + rng.uniform(0, max(1, w * s - bw)), ny + rng.uniform(0, max(1, h * s - bh))
            for jit in range(2):
                rows.append([x + jit, y + jit, x + bw + jit, y + bh + jit, rng.uniform(0.05, 1), 0, rng.integers(0, 3)])
    rows = np.asarray(rows, np.float32)
    rows[:, 5] = rows[:, 4]
    rows = rows[np.argsort(-rows[:, 4], kind="stable")]
    fine = torch.from_numpy(rows).cuda()
    k = torch.tensor([len(rows), len(rows)], dtype=torch.int32).cuda()
    a, b = stage.merge(fine, k, pk, 3), stage.merge(fine, k, pk.chips, 3)
    assert sum(len(x) for x in b) > 10 and all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(RuntimeError, match="outside"):
        stage.pack(torch.from_numpy(d[0]).cuda(), torch.tensor([21], dtype=torch.int32).cuda(), (W, H), 1.5)


def test_two_stage_device_packing_equals_host_packing():
    """the scene of tests/test_ufp.py::test_two_stage_pipeline_runs_end_to_end (the only test here that compiles detectors)"""
    import torch
    from glsdet_amd.resdet import HipGflDetector
    from glsdet_amd.synth import synth_input, synth_resdet_state_dict
    from glsdet_amd.ufp import TwoStagePipeline, UfpSecondStage, two_stage_detect
    img = _image(270, 480, 2)
    calib = synth_input((1, 3, 128, 160), 100)
    coarse = HipGflDetector("gfl", synth_resdet_state_dict("gfl", 0, calib), dtype="f16")
    fine = HipGflDetector("mpdet", synth_resdet_state_dict("mpdet", 1, calib), dtype="f16")
    stage = UfpSecondStage()

    def thr_for(det, x, keep):
        cls, _ = det.forward_raw(x)
        p = torch.sigmoid(torch.cat([c.flatten() for c in cls]))
        return float(torch.topk(p, keep).values[-1])
    x1, _ = stage.pipeline_input(torch.from_numpy(img).cuda().contiguous())
    c1 = dict(score_thr=thr_for(coarse, x1, 60), iou_thr=0.6, nms_pre=1000, max_per_img=40)
    _, mid = two_stage_detect(coarse, fine, img, stage, c1, dict(score_thr=0.999, iou_thr=0.6, nms_pre=1000, max_per_img=300))
    x2, _ = stage.pipeline_input(mid["canvas"])
    c2 = dict(score_thr=thr_for(fine, x2, 400), iou_thr=0.6, nms_pre=1000, max_per_img=300)
    host, hmid = two_stage_detect(coarse, fine, img, stage, c1, c2, packing="host")
    dev, dmid = two_stage_detect(coarse, fine, img, stage, c1, c2, packing="device")
    pk = dmid["packing"]
    assert len(hmid["chips"]) >= 1 and pk.n_boxes == len(hmid["first"][0])
    assert np.array_equal(np.asarray(pk.chips).view(np.int64), np.asarray(hmid["chips"], np.float64).reshape(-1, 7).view(np.int64))
    assert dmid["canvas_wh"] == tuple(float(v) for v in hmid["canvas_wh"])
    assert np.array_equal(dmid["canvas"].cpu().numpy(), hmid["canvas"].cpu().numpy())
    assert sum(len(m) for m in host) > 0 and all(np.array_equal(a, b) for a, b in zip(host, dev))
    frames = [img, _image(270, 480, 3), img, _image(270, 480, 4)]
    want = TwoStagePipeline(coarse, fine, stage, c1, c2, workers=2, packing="host").run(frames)
    got = TwoStagePipeline(coarse, fine, stage, c1, c2, workers=2, packing="device").run(frames)
    for a, b in zip(want, got):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # no coarse detection at all: what the host path returns for no boxes
    none = dict(c1, score_thr=1.0)
    e_host, _ = two_stage_detect(coarse, fine, img, stage, none, c2, packing="host")
    e_dev, e_mid = two_stage_detect(coarse, fine, img, stage, none, c2, packing="device")
    assert e_mid["packing"].n_boxes == 0 and len(e_dev) == len(e_host) and all(x.shape == y.shape == (0, 5) for x, y in zip(e_dev, e_host))
