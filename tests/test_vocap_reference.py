"""CPU: the arithmetic contract of glsdet_voc_ap (VOC-style mAP, get_map of drone/models/core/utils_map.py:294-813).

tests/voc_reference.py, the scalar restatement, is pinned here to records of the reference's own get_map on the committed
scenes (tests/golden/vocap_golden.npz, tools/make_vocap_golden.py) at the overlaps 0.5 and 0.75: rec, prec, ap, mrec,
mpre, mr, fppi bit for bit and results.txt as text.  lamr holds within 1e-12 relative: the nine picked miss rates are
exact, then nine `log`, one mean and one `exp` are each good to a few ulp (2^-52 = 2.2e-16 each; a dozen of them stay
far below 1e-12).  Every planted mistake of the restatement must show on a committed scene.  The surface tests (exports,
host refusals, signature, layout check) need the library, not a GPU."""
import inspect
import os

import numpy as np
import pytest

from tests import voc_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("rec", "prec", "mrec", "mpre", "mr", "fppi")


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def bits(x):
    return np.asarray(x, np.float64).reshape(-1).view(np.int64)


def record(g, name, thr):
    p = "%s/%g/" % (name, thr)
    return {k: g[p + k] for k in EXACT + ("ap", "lamr", "n_det", "results", "printed")}


def differences(rec, ev):
    """the names of what differs between a record of the reference and an evaluation of the restatement"""
    cls = [ev["per_class"][c] for c in ev["classes"]]
    bad = []
    if rec["n_det"].tolist() != [c["n_det"] for c in cls]:
        bad.append("n_det")
    for k in EXACT:
        if not np.array_equal(bits(rec[k]), bits([x for c in cls for x in c[k]])):
            bad.append(k)
    if not np.array_equal(bits(rec["ap"]), bits([c["ap"] for c in cls])):
        bad.append("ap")
    lamr = np.array([float(c["lamr"]) for c in cls])
    if lamr.shape != rec["lamr"].shape or (np.abs(lamr - rec["lamr"]) > 1e-12 * np.abs(rec["lamr"])).any():
        bad.append("lamr")
    text, printed = R.results_text(ev)
    if text != rec["results"].tobytes().decode():
        bad.append("results")
    if printed != rec["printed"].tolist():
        bad.append("printed")
    return bad


def test_restatement_equals_the_recorded_reference(golden):
    g, scenes = golden
    assert g["thresholds"].tolist() == [0.5, 0.75] and len(scenes) >= 18
    for name, (gt, dr) in scenes.items():
        for thr in (0.5, 0.75):
            assert differences(record(g, name, thr), R.evaluate(gt, dr, thr)) == [], (name, thr)


def test_committed_scenes_hold_the_edge_cases(golden):
    g, scenes = golden
    ev = {n: R.evaluate(*scenes[n], 0.5) for n in scenes}
    pc = lambda n, c: ev[n]["per_class"][c]
    assert any(t == "" for n in scenes for t in scenes[n][1].values())                          # an empty detection file
    assert pc("empty_and_missing", "person")["n_det"] == 0 and pc("empty_and_missing", "person")["ap"] == 0.0
    assert "dog" in ev["empty_and_missing"]["det_counter"] and "dog" not in ev["empty_and_missing"]["classes"]
    assert ev["difficult"]["classes"] == ["car"] and "bus" in ev["difficult"]["det_counter"]    # difficult-only: no class
    c = pc("difficult", "car")                                   # two matches on a difficult ground truth: neither tp nor fp
    assert c["tp"] == [0, 0, 1, 1] and c["fp"] == [0, 0, 0, 1] and c["score05_idx"] == 3          # all scores above 0.5
    c = pc("on_threshold_and_repeat", "car")                    # 0 0 9 9 against 0 0 9 4 is exactly 0.5; then a repeat
    assert R.overlap([0, 0, 9, 4], [0, 0, 9, 9]) == 0.5 and c["tp"] == [1, 1, 1] and c["fp"] == [0, 1, 2]
    assert c["rec"][0] == 1.0 and c["n_det"] == 3                                               # recall 1.0 before the end
    bb = R.parse_dr_line(scenes["one_ulp_below"][1]["a"].strip())[2]
    assert R.overlap(bb, [0.0, 0.0, 9.0, 9.0]) == np.nextafter(0.5, 0.0) and pc("one_ulp_below", "car")["tp"] == [0]
    assert pc("tie_first_wins", "car")["tp"] == [1, 1] and pc("tie_first_wins", "car")["fp"] == [0, 1]
    assert R.overlap([0, 0, 10, 9], [10, 0, 19, 9]) is not None and R.overlap([0, 0, 10, 9], [11, 0, 20, 9]) is None
    assert "car 0.9 0 0 10 9" in scenes["plus_one_rule"][1]["a"] and "car 11 0 20 9" in scenes["plus_one_rule"][0]["b"]
    c = pc("equal_scores", "car")                               # equal scores across files keep the file order
    assert c["score"] == [0.5, 0.5] and c["tp"] == [0, 1] and c["score05_idx"] == 0              # no score above 0.5
    assert set(pc("equal_scores", "van")["rec"]) == {0.0}                                       # recall never changes
    assert "traffic light" in ev["blank_in_name"]["classes"] and ev["blank_in_name"]["det_counter"]["traffic"] == 3
    assert "20.25" in scenes["blank_in_name"][1]["a"]                                           # non-integer coordinates
    assert pc("n_img_of_class", "person")["n_images"] == 1 and len(scenes["n_img_of_class"][0]) == 3


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_every_planted_mistake_shows_on_a_committed_scene(golden, mistake):
    g, scenes = golden
    shown = [(n, thr) for n, (gt, dr) in scenes.items() for thr in (0.5, 0.75)
             if differences(record(g, n, thr), R.evaluate(gt, dr, thr, mistakes=(mistake,)))]
    assert shown, mistake


def test_missing_partner_file_raises():
    with pytest.raises(FileNotFoundError):
        R.evaluate({"a": "car 0 0 9 9\n"}, {}, 0.5)
    with pytest.raises(FileNotFoundError):
        R.evaluate({"a": "car 0 0 9 9\n"}, {"a": "", "b": ""}, 0.5)


# ---------------------------------------------------------------------------------- surface, no GPU
def test_exports_header_and_table():
    from glsdet_amd import _lib
    assert "glsdet_voc_ap" in _lib.EXPORTS and "glsdet_voc_ap_workspace_bytes" in _lib.EXPORTS
    src = open(os.path.join(ROOT, "include", "glsdet_hip.h")).read()
    assert "int glsdet_voc_ap(" in src and "int64_t glsdet_voc_ap_workspace_bytes(" in src and "utils_map.py:294-813" in src
    lib = _lib.load()
    assert lib.glsdet_abi_version() == 17
    assert lib.glsdet_voc_ap_workspace_bytes(0, 1) == 256 and lib.glsdet_voc_ap_workspace_bytes(1000, 3) == 3072
    assert lib.glsdet_voc_ap_workspace_bytes(2 ** 31 - 1, 3) == (3 * (2 ** 31 - 1) + 255) // 256 * 256      # 64-bit
    assert lib.glsdet_voc_ap_workspace_bytes(-1, 1) == 0 and lib.glsdet_voc_ap_workspace_bytes(10, 0) == 0


def test_host_refusals():
    """every malformed call is refused with a negative code naming voc_ap before anything is launched: the pointers are
    never dereferenced"""
    from glsdet_amd import _lib
    lib = _lib.load()
    names = ("dt_box", "score", "cls_off", "n_dt", "n_cls", "pair_off", "pair_det", "gt_off", "n_pairs", "gt_box", "gt_difficult",
             "n_gt_boxes", "n_gt", "n_img", "min_overlap", "n_thr", "fppi_ref", "tp", "fp", "rec", "prec", "mpre", "cls_out", "ws",
             "ws_bytes")
    good = {n: 0x10000 * (k + 1) for k, n in enumerate(names)}
    good.update(n_dt=100, n_cls=3, n_pairs=20, n_gt_boxes=50, n_thr=2, ws_bytes=256)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.glsdet_voc_ap(*[a[n] for n in names], None)
        return rc, lib.glsdet_last_error().decode()
    pointers = [n for n in names if not n.startswith("n_") or n in ("n_gt", "n_img")]
    pointers.remove("ws_bytes")
    bad = [{n: None} for n in pointers]
    bad += [{n: good[n] + 4} for n in ("dt_box", "score", "gt_box", "min_overlap", "fppi_ref", "rec", "prec", "mpre", "cls_out")]
    bad += [{n: good[n] + 2} for n in ("cls_off", "pair_off", "pair_det", "gt_off", "n_gt", "n_img", "tp", "fp")]
    bad += [dict(n_dt=-1), dict(n_cls=-1), dict(n_pairs=-1), dict(n_gt_boxes=-1), dict(n_thr=0), dict(n_thr=-2),
            dict(n_pairs=101), dict(ws_bytes=255), dict(ws_bytes=0), dict(n_gt_boxes=200, ws_bytes=256)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc < 0 and "voc_ap" in msg, (kw, rc, msg)
    assert call(n_thr=0)[0] == -1 and call(dt_box=good["dt_box"] + 4)[0] == -3
    # no detections / no ground truths: their arrays may be null (nothing is launched here: zero classes)
    assert call(n_cls=0, n_dt=0, n_pairs=0, dt_box=None, score=None, pair_det=None, tp=None, fp=None, rec=None, prec=None,
                mpre=None, n_gt_boxes=0, gt_box=None, gt_difficult=None)[0] == 0


def test_layout_check_refuses_what_the_library_cannot_see():
    from glsdet_amd.eval.voc import check_layout
    ok = dict(cls_off=[0, 2, 5], pair_off=[0, 1, 3, 5], pair_det=[0, 2, 1, 4, 3], gt_off=[0, 0, 2, 3], n_dt=5, n_gt_boxes=3)
    check_layout(**ok)
    for kw in (dict(cls_off=[0, 3, 2]), dict(cls_off=[1, 2, 5]), dict(cls_off=[0, 2, 4]), dict(pair_off=[0, 3, 1, 5]),
               dict(pair_off=[0, 1, 1, 5]), dict(gt_off=[0, 2, 1, 3]), dict(gt_off=[0, 0, 2, 4]), dict(gt_off=[0, 3]),
               dict(pair_det=[0, 2, 1, 4, 4]), dict(pair_det=[0, 2, 1, 4, 5]), dict(pair_det=[0, 2, 1, 4])):
        with pytest.raises(ValueError, match="voc_ap"):
            check_layout(**dict(ok, **kw))


def test_get_map_has_the_reference_signature():
    from glsdet_amd.eval import VocEval, get_map
    sig = inspect.signature(get_map)
    assert list(sig.parameters) == ["MINOVERLAP", "draw_plot", "path"] and sig.parameters["path"].default == './map_out'
    assert sig.parameters["MINOVERLAP"].default is inspect.Parameter.empty
    sig = inspect.signature(VocEval.__init__)
    assert list(sig.parameters) == ["self", "classes", "device"] and sig.parameters["device"].default == "cuda:0"
    assert inspect.signature(VocEval.evaluate).parameters["min_overlap"].default == 0.5
    for name in ("add_ground_truth", "add_detections", "load_dirs"):
        assert callable(getattr(VocEval, name))


def test_host_preparation_builds_the_documented_arrays(golden):
    """the CSR arrays of a committed scene: class-major rank order, pairs in (class, image) order, ground truths in file order"""
    from glsdet_amd.eval.voc import VocEval, check_layout
    _, scenes = golden
    gt, dr = scenes["n_img_of_class"]
    E = VocEval()
    for i in gt:
        E.add_ground_truth(i, [(n, *b, d) for n, b, d in map(R.parse_gt_line, R.lines_of(gt[i]))])
        E.add_detections(i, [(n, s, *b) for n, s, b in map(R.parse_dr_line, R.lines_of(dr[i]))])
    h = E._prepare()
    assert h["classes"] == ["car", "person"] and h["n_gt"].tolist() == [3, 1] and h["n_img"].tolist() == [3, 1]
    assert h["cls_off"].tolist() == [0, 3, 5] and h["score"].tolist() == [0.95, 0.9, 0.2, 0.9, 0.8]
    assert h["pair_off"].tolist() == [0, 1, 3, 5] and h["pair_det"].tolist() == [1, 0, 2, 3, 4]
    assert h["gt_off"].tolist() == [0, 1, 2, 3] and h["gt_box"].tolist() == [[0, 0, 9, 9], [5, 5, 20, 20], [0, 0, 9, 9]]
    check_layout(h["cls_off"], h["pair_off"], h["pair_det"], h["gt_off"], h["ND"], len(h["gt_difficult"]))
    with pytest.raises(FileNotFoundError):
        VocEval()._prepare()
    E.add_ground_truth("lonely", [("car", 0, 0, 1, 1)])
    with pytest.raises(FileNotFoundError):
        E._prepare()


def test_torch_op_is_registered_and_refuses_cpu_tensors():
    import torch
    import glsdet_amd.torch_ops  # noqa: F401
    f64, i32 = (lambda *s: torch.zeros(*s, dtype=torch.float64)), (lambda *s: torch.zeros(*s, dtype=torch.int32))
    args = [f64(5, 4), f64(5), i32(3), i32(4), i32(5), i32(4), f64(3, 4), torch.zeros(3, dtype=torch.uint8), i32(2), i32(2),
            f64(2), f64(9)]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        torch.ops.glsdet.voc_ap(*args)
    out = torch.ops.glsdet.voc_ap(*[a.to("meta") for a in args])
    assert [tuple(o.shape) for o in out] == [(2, 5)] * 5 + [(2, 2, 16)]
    assert [o.dtype for o in out] == [torch.int32] * 2 + [torch.float64] * 4
