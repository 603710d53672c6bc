"""CPU: the arithmetic contract of glsdet_ufp_pack (unified foreground packing on float32 detections).

tests/ufp_pack_reference.py, the scalar restatement with every dtype written out, is pinned here to
glsdet_amd/ufp/packing.py and to records of the reference's own UnifiedForegroundPacking on hand-built edge scenes
(tests/golden/ufp_pack_golden.npz, tools/make_ufp_pack_golden.py); every planted mistake of the restatement must show on
a committed scene.  The surface tests (exports, host refusals, the packing= keyword) need the library, not a GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import ufp_pack_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "ufp_pack_golden.npz"))


def scene_of(golden, name):
    expand, W, H = golden[name + "/params"]
    return golden[name + "/boxes"], golden[name + "/labels"], float(expand), int(W), int(H)


def bits(chips):
    return np.asarray(chips, np.float64).reshape(-1, 7).view(np.int64)


def same(a, b):
    return bits(a[0]).shape == bits(b[0]).shape and np.array_equal(bits(a[0]), bits(b[0])) and \
        float(a[1]) == float(b[1]) and float(a[2]) == float(b[2])


def test_scene_list_is_complete(golden):
    names = set(golden["names"].tolist())
    want = {"n0", "n1", "n2", "edge_share_dyadic", "edge_share_contraction", "chain_after_growth", "before_first_hit",
            "swallow_earlier", "area_1024", "area_1024_minus_ulp", "area_9216", "area_9216_minus_ulp", "three_box_region",
            "clipped_borders", "equal_heights", "equal_sizes_2_3", "wider_than_2666", "interleaved_labels",
            "last_probe_infeasible"}
    want |= {"fill_rank%s" % k for k in ("1", "2", "3", "4a", "4b", "4c", "4d")} | {"boxes_%d" % n for n in (63, 64, 65, 127, 128, 129)}
    assert want <= names, want - names
    for n in (63, 64, 65, 127, 128, 129):
        assert len(golden["boxes_%d/boxes" % n]) == n
    assert all(golden[n + "/boxes"].dtype == np.float32 for n in names)
    assert str(golden["numpy_version"]).split(".")[0] == "2"          # the records were made under NEP 50 promotion


def test_restatement_equals_the_recorded_reference_and_packing_py(golden):
    from glsdet_amd.ufp.packing import unified_foreground_packing
    for name in golden["names"].tolist():
        boxes, labels, expand, W, H = scene_of(golden, name)
        got = R.ufp_pack(boxes, labels, expand, W, H)
        assert same(got, (golden[name + "/chips"], *golden[name + "/canvas"])), name
        if len(boxes):
            order = np.argsort(labels, kind="stable")
            assert same(got, unified_foreground_packing(boxes[order].copy(), expand, [W, H])), name


def test_scenes_have_the_properties_they_are_named_for(golden):
    def run(name, trace=None):
        return R.ufp_pack(*scene_of(golden, name), trace=trace)
    assert run("n0") == ([], 0.0, 0.0) and len(run("n1")[0]) == 1
    assert len(run("edge_share_dyadic")[0]) == 2                       # union == sum: no merge
    assert len(run("chain_after_growth")[0]) == 2 and len(run("before_first_hit")[0]) == 1
    assert [c[6] for c in run("area_1024")[0]] == [2.0] and [c[6] for c in run("area_1024_minus_ulp")[0]] == [4.0]
    assert [c[6] for c in run("area_9216")[0]] == [1.0] and [c[6] for c in run("area_9216_minus_ulp")[0]] == [2.0]
    assert len(run("three_box_region")[0]) == 1
    b, (W, H) = np.asarray(run("clipped_borders")[0]), (640, 480)
    assert b[:, 0].min() == 0 and b[:, 1].min() == 0 and (b[:, 0] + b[:, 2]).max() == W - 1 and (b[:, 1] + b[:, 3]).max() == H - 1
    eq = np.asarray(run("equal_sizes_2_3")[0])
    pos = {}
    for c in eq:
        pos.setdefault((c[2] * c[6], c[3] * c[6]), set()).add((c[4], c[5]))
    assert sorted(sum(1 for c in eq if (c[2] * c[6], c[3] * c[6]) == k) for k in pos) == [1, 2, 3]
    assert all(len(v) == 1 for v in pos.values())                      # equal-sized regions share one canvas position
    assert max(c[2] * c[6] for c in run("wider_than_2666")[0]) > 2666
    assert len(set(golden["interleaved_labels/labels"].tolist())) < 10 and golden["interleaved_labels/labels"].max() == 9
    for k in ("1", "2", "3", "4a", "4b", "4c", "4d"):
        tr = {}
        run("fill_rank" + k, tr)
        assert tr.get("rank" + k, 0) > 0 and tr["probes"] == 11, (k, tr)
    tr = {}
    run("last_probe_infeasible", tr)
    assert tr["last_infeasible"]


@pytest.mark.parametrize("block", range(4))
def test_restatement_equals_packing_py_on_random_float32_scenes(block):
    from glsdet_amd.ufp.packing import unified_foreground_packing
    for seed in range(60 * block, 60 * block + 60):                    # 240 scenes of 1..48 boxes, every fifth integer-valued
        boxes, labels, expand, W, H = R.random_scene(seed, max_n=48, integer=seed % 5 == 0)
        order = np.argsort(labels, kind="stable")
        want = unified_foreground_packing(boxes[order].copy(), expand, [W, H])
        assert same(R.ufp_pack(boxes, labels, expand, W, H), want), seed


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_planted_mistake_shows_on_a_committed_scene(golden, mistake):
    shown = [n for n in golden["names"].tolist() if len(golden[n + "/boxes"]) <= 12 and
             not same(R.ufp_pack(*scene_of(golden, n), mistakes=(mistake,)), (golden[n + "/chips"], *golden[n + "/canvas"]))]
    assert shown, mistake


# ---------------------------------------------------------------------------------- surface, no GPU
def test_exports_and_limit():
    from glsdet_amd import _lib
    assert "glsdet_ufp_pack" in _lib.EXPORTS and "glsdet_ufp_pack_max_boxes" in _lib.EXPORTS
    lib = _lib.load()
    # per box: region 16 + size and position 32 + stack slot 32 + area sum and count 8 + four int32 maps 16; one more slot
    assert lib.glsdet_ufp_pack_max_boxes() == (160 * 1024 - 32) // 104 == 1575 >= 1000


def test_host_refusals():
    """every malformed call is refused with a negative code naming ufp_pack before anything is launched: the pointers
    are never dereferenced"""
    from glsdet_amd import _lib
    lib = _lib.load()
    limit = lib.glsdet_ufp_pack_max_boxes()
    good = dict(dets=0x10000, count=0x20000, n_img=2, max_det=100, expand=1.5, img_w=640, img_h=480, chips=0x30000,
                chips_floor=0x40000, header=0x50000, status=0x60000)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.glsdet_ufp_pack(a["dets"], a["count"], a["n_img"], a["max_det"], a["expand"], a["img_w"], a["img_h"], a["chips"],
                                 a["chips_floor"], a["header"], a["status"], None)
        return rc, lib.glsdet_last_error().decode()
    bad = [dict(dets=None), dict(count=None), dict(chips=None), dict(chips_floor=None), dict(header=None), dict(status=None),
           dict(dets=0x10002), dict(count=0x20001), dict(chips=0x30004), dict(chips_floor=0x40002), dict(header=0x50004),
           dict(status=0x60003), dict(n_img=0), dict(n_img=-1), dict(max_det=0), dict(max_det=limit + 1),
           dict(expand=0.0), dict(expand=-1.5), dict(expand=float("inf")), dict(expand=float("nan")),
           dict(img_w=0), dict(img_h=0), dict(img_w=-5)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc < 0 and "ufp_pack" in msg, (kw, rc, msg)
    assert call(chips=0x30004)[0] == -3 and call(max_det=limit + 1)[0] == -1


def test_packing_keyword_and_its_default():
    from glsdet_amd.ufp import DevicePacking, TwoStagePipeline, UfpSecondStage, two_stage_detect
    assert inspect.signature(two_stage_detect).parameters["packing"].default == "host"
    assert inspect.signature(TwoStagePipeline.__init__).parameters["packing"].default == "host"
    sig = inspect.signature(UfpSecondStage.pack)
    assert list(sig.parameters)[1:] == ["dets", "count", "image_wh", "expand"] and sig.parameters["expand"].default == 1.5
    with pytest.raises(ValueError):
        TwoStagePipeline(None, None, None, {}, {}, packing="gpu")
    p = DevicePacking(None, None, [3.0, 2.0, 640.5, 300.0])
    assert (p.n_boxes, p.n_chips, p.canvas_w, p.canvas_h, len(p)) == (3, 2, 640.5, 300.0, 2)


def test_torch_op_is_registered_and_refuses_cpu_tensors():
    import torch
    import glsdet_amd.torch_ops  # noqa: F401
    dets, counts = torch.zeros(1, 8, 7), torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.glsdet.ufp_pack(dets, counts, 1.5, 640, 480)
    out = torch.ops.glsdet.ufp_pack(dets.to("meta"), counts.to("meta"), 1.5, 640, 480)
    assert [tuple(o.shape) for o in out] == [(1, 8, 7), (1, 8, 7), (1, 4), (1,)]
    assert [o.dtype for o in out] == [torch.float64, torch.float32, torch.float64, torch.int32]
