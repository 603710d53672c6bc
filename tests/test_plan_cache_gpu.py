"""The plan cache under the detectors themselves: an evicted plan is rebuilt on demand and computes what the first one did
(HipDetector eagerly, HipGflDetector through the hipGraph capture), and two instances of one shape replay on their own
streams (run_async)."""
import numpy as np
import pytest
import torch

from oracle import glsdet_oracle as O
from tests.helpers import calibrated_resdet_sd, model_case

pytestmark = pytest.mark.gpu

SHAPES = [(64, 64), (64, 96), (96, 64), (64, 64)]         # the fourth asks for the first again, after two others evicted it


def _image(H, W, big):
    """the fixed random image, cut to H x W"""
    return big[:, :, :H, :W].contiguous().cuda()


def _plan_of(det, H, W):
    hits = [c for k, c in det._compiled.items() if k[:3] == (1, H, W)]
    assert len(hits) == 1
    return hits[0]


@pytest.fixture(scope="module")
def nano(golden, shapes):
    from glsdet_amd.detector import HipDetector
    meta, sd, _, _, _ = model_case(golden, shapes, "base_nano_seed0")
    return HipDetector(meta["model"], sd, dtype="f16", autotune=False)


def test_yolox_rebuilds_an_evicted_plan_with_the_same_result(nano, monkeypatch):
    monkeypatch.setenv("GLSDET_MAX_PLANS", "2")
    big = O.synth_input((1, 3, 96, 96), 41)
    runs, plans = [], []
    for H, W in SHAPES:
        dec, dets = nano.detect(_image(H, W, big), 0.05, 0.5)
        runs.append((dec.cpu().numpy(), dets))
        plans.append(_plan_of(nano, H, W))
    (dec0, dets0), (dec3, dets3) = runs[0], runs[3]
    print("detections per image, first / fourth call:", [len(d) for d in dets0], [len(d) for d in dets3])
    assert dec0.shape == (1, 84, dec0.shape[2]) and len(dets0) == len(dets3) == 1
    assert len(dets0[0]) > 0                       # (equal empty arrays would show nothing)
    assert np.array_equal(dec0, dec3)
    for a, b in zip(dets0, dets3):
        assert np.array_equal(a, b)
    assert len(nano._compiled) == 2
    assert [k[:3] for k in nano._compiled] == [(1, 96, 64), (1, 64, 64)]      # least recently used first
    assert plans[3] is not plans[0]


def test_gfl_rebuilds_an_evicted_captured_plan_with_the_same_result(monkeypatch):
    from glsdet_amd.resdet import HipGflDetector
    monkeypatch.setenv("GLSDET_MAX_PLANS", "2")
    big = O.synth_input((1, 3, 96, 96), 42)
    det = HipGflDetector("gfl", calibrated_resdet_sd("gfl", 0, big), dtype="f16", autotune=False)
    runs, plans = [], []
    for H, W in SHAPES:
        runs.append(det.detect(_image(H, W, big), use_graph=True))
        plans.append(_plan_of(det, H, W))
        assert plans[-1].plan.captured and plans[-1].graph_stream is not None
    print("detections per image, first / fourth call:", [len(l) for _, l in runs[0]], [len(l) for _, l in runs[3]])
    assert len(runs[0]) == len(runs[3]) == 1 and len(runs[0][0][1]) > 0
    for (a, la), (b, lb) in zip(runs[0], runs[3]):
        assert np.array_equal(a, b) and np.array_equal(la, lb)
    assert len(det._compiled) == 2
    assert [k[:3] for k in det._compiled] == [(1, 96, 64), (1, 64, 64)]
    assert plans[3] is not plans[0]


def test_run_async_of_two_instances_equals_the_eager_result(nano):
    x = _image(64, 64, O.synth_input((1, 3, 96, 96), 43))
    dec, want = nano.detect(x, 0.05, 0.5)
    dec = dec.cpu().numpy()
    assert len(want[0]) > 0
    A = nano.num_anchors(64, 64)
    post = dict(conf_thres=0.05, nms_thres=0.5, max_det=A, mode=0, max_cand=A)
    inst = [nano.compile(1, 64, 64, post, use_graph=True, instance=i) for i in (0, 1)]
    assert inst[0] is not inst[1] and inst[0].graph_stream is not inst[1].graph_stream
    for c in inst:
        c.img.copy_(x)
    torch.cuda.synchronize()
    for _ in range(2):
        for c in inst:
            nano.run_async(c)
    for c in inst:
        c.graph_stream.synchronize()
    for c in inst:
        got = nano.collect(c)
        assert np.array_equal(c.decoded.cpu().numpy(), dec)
        assert len(got) == len(want) == 1 and np.array_equal(got[0], want[0])
