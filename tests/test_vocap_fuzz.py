"""GPU: glsdet_voc_ap against the scalar restatement (tests/voc_reference.py, pinned to the reference's own get_map on the
CPU by tests/test_vocap_reference.py).  Every output buffer is sentinel-filled and compared whole, bit for bit; the
workspace is dirty.  Then the surface: torch.ops.glsdet.voc_ap, VocEval.load_dirs and get_map against the recorded
results.txt bytes."""
import os

import numpy as np
import pytest

from tests import voc_reference as R

pytestmark = pytest.mark.gpu
SENT_D, SENT_I = -7.25e9, 0x5A5A5A5A


def prepare(gt, dr):
    """a scene's texts through VocEval's host preparation -> its arrays"""
    from glsdet_amd.eval.voc import VocEval, check_layout
    E = VocEval()
    for i in gt:
        E.add_ground_truth(i, [(n, *b, d) for n, b, d in map(R.parse_gt_line, R.lines_of(gt[i]))])
        E.add_detections(i, [(n, s, *b) for n, s, b in map(R.parse_dr_line, R.lines_of(dr[i]))])
    h = E._prepare()
    check_layout(h["cls_off"], h["pair_off"], h["pair_det"], h["gt_off"], h["ND"], len(h["gt_difficult"]))
    return h


def run_device(h, thr, dirt=0xA5):
    """one glsdet_voc_ap call into sentinel-filled outputs with a dirty workspace -> host arrays"""
    import torch
    from glsdet_amd import _lib
    lib = _lib.load()
    thr = np.asarray(thr, np.float64)
    T, ND, C, NG, P = len(thr), h["ND"], len(h["classes"]), len(h["gt_difficult"]), len(h["pair_off"]) - 1
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dev = {k: up(h[k]) for k in ("dt_box", "score", "cls_off", "pair_off", "pair_det", "gt_off", "gt_box", "gt_difficult", "n_gt",
                                 "n_img")}
    d_thr, d_ref = up(thr), up(np.logspace(-2.0, 0.0, num=9))
    ws = torch.full((int(lib.glsdet_voc_ap_workspace_bytes(NG, T)),), dirt, dtype=torch.uint8, device="cuda")
    tp, fp = (torch.full((T, ND), SENT_I, dtype=torch.int32, device="cuda") for _ in range(2))
    rec, prec, mpre = (torch.full((T, ND), SENT_D, dtype=torch.float64, device="cuda") for _ in range(3))
    cls_out = torch.full((T, C, 16), SENT_D, dtype=torch.float64, device="cuda")
    ptr = lambda t: t.data_ptr() if t.numel() else None
    _lib.check(lib.glsdet_voc_ap(ptr(dev["dt_box"]), ptr(dev["score"]), dev["cls_off"].data_ptr(), ND, C, dev["pair_off"].data_ptr(),
                                 ptr(dev["pair_det"]), dev["gt_off"].data_ptr(), P, ptr(dev["gt_box"]), ptr(dev["gt_difficult"]), NG,
                                 dev["n_gt"].data_ptr(), dev["n_img"].data_ptr(), d_thr.data_ptr(), T, d_ref.data_ptr(), ptr(tp),
                                 ptr(fp), ptr(rec), ptr(prec), ptr(mpre), cls_out.data_ptr(), ws.data_ptr(), ws.numel(),
                                 torch.cuda.current_stream().cuda_stream), "voc_ap")
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in (tp, fp, rec, prec, mpre, cls_out))


def expected(gt, dr, thr, h):
    """the restatement's answer in the layout of the kernel's buffers"""
    T, ND, C = len(thr), h["ND"], len(h["classes"])
    tp, fp = np.zeros((T, ND), np.int32), np.zeros((T, ND), np.int32)
    rec, prec, mpre = np.zeros((T, ND)), np.zeros((T, ND)), np.zeros((T, ND))
    cls_out = np.zeros((T, C, 16))
    for t, v in enumerate(thr):
        ev = R.evaluate(gt, dr, float(v))
        assert ev["classes"] == h["classes"]
        for k, name in enumerate(ev["classes"]):
            c = ev["per_class"][name]
            d0, d1 = h["cls_off"][k], h["cls_off"][k + 1]
            assert d1 - d0 == c["n_det"] and h["score"][d0:d1].tolist() == c["score"]
            tp[t, d0:d1], fp[t, d0:d1], rec[t, d0:d1], prec[t, d0:d1] = c["tp"], c["fp"], c["rec"], c["prec"]
            mpre[t, d0:d1] = c["mpre"][1:-1]
            s = c["score05_idx"]
            at = [c["f1"][s], c["rec"][s], c["prec"][s]] if c["n_det"] else [0.0, 0.0, 0.0]
            cls_out[t, k] = [c["ap"], c["n_tp"], s] + at + c["mr9"] + [c["fp"][-1] if c["n_det"] else 0]
    return tp, fp, rec, prec, mpre, cls_out


def check_scene(gt, dr, thr, what, dirt=0xA5):
    h = prepare(gt, dr)
    got = run_device(h, thr, dirt)
    want = expected(gt, dr, thr, h)
    for name, a, b in zip(("tp", "fp", "rec", "prec", "mpre", "cls_out"), got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        same = a.view(np.int32 if a.dtype == np.int32 else np.int64) == b.view(np.int32 if b.dtype == np.int32 else np.int64)
        assert same.all(), (what, name, int((~same).sum()), np.argwhere(~same)[:4].tolist())
    return h, got


def test_committed_scenes_two_thresholds_in_one_launch():
    _, scenes = R.load_golden()
    for name, (gt, dr) in scenes.items():
        check_scene(gt, dr, [0.5, 0.75], name)


def test_hundred_seeded_scenes_one_and_three_thresholds():
    for seed in range(100):
        gt, dr = R.random_scene(5000 + seed)
        check_scene(gt, dr, [0.5] if seed % 2 else [0.3, 0.5, 0.75], seed)


def row_scene(n_gt, n_det, seed, n_img=1):
    """tiny 4-pixel boxes in a row, 6 pixels apart, so a detection overlaps one ground truth or two neighbours at most;
    every eighth ground truth is difficult; detections sit on, half a box beside or between the ground truths"""
    rng = np.random.default_rng(seed)
    gt, dr = {}, {}
    for i in range(n_img):
        g = ["car %d 0 %d 3%s" % (6 * k, 6 * k + 3, " difficult" if k % 8 == 5 else "") for k in range(n_gt)]
        if i == 0:
            g.append("car 0 100 3 103")                     # the class exists even when the row is empty
        d = []
        for k in range(n_det // n_img + (1 if i < n_det % n_img else 0)):
            x = 6 * int(rng.integers(0, max(n_gt, 1) + 2)) + int(rng.integers(0, 3))
            d.append("car %s %d 0 %d %d" % (repr(round(float(rng.integers(1, 1000)) / 1000, 3)), x, x + 3, 3 - int(rng.integers(0, 2))))
        gt["r%05d" % i], dr["r%05d" % i] = "\n".join(g) + "\n", "\n".join(d) + ("\n" if d else "")
    return gt, dr


@pytest.mark.parametrize("n_gt", [0, 1, 63, 64, 65, 129])
def test_lane_tails_of_the_matching(n_gt):
    """ground truths per pair around the wave size: lanes beyond the last one, one, two and three rounds per lane"""
    gt, dr = row_scene(n_gt - 1 if n_gt else 0, 3 * n_gt + 5, n_gt)
    if n_gt == 0:
        gt = {"r00000": "car 0 100 3 103\n", "r00001": ""}    # the detections' pair has no ground truth at all
        dr = {"r00000": "", "r00001": dr["r00000"]}
    h, _ = check_scene(gt, dr, [0.5, 0.2], n_gt)
    assert np.diff(h["gt_off"]).max() == n_gt


@pytest.mark.parametrize("n_det", [1, 255, 256, 257, 1023, 1024, 1025, 70001])
def test_chunk_edges_and_carry_of_the_scans(n_det):
    """detections per class around the 256-wide chunk, and 70 001: the carry crosses 273 chunk edges in all three passes"""
    big = n_det == 70001                  # 64 images of 12 ground truths keep the restatement under a second
    gt, dr = row_scene(12 if big else 40, n_det, n_det, n_img=64 if big else 1)
    h, got = check_scene(gt, dr, [0.5], n_det)
    assert h["ND"] == n_det and (not big or 100 < got[5][0, 0, 1] <= 12 * 64 + 1)


def test_more_pairs_than_the_match_grid_and_more_curves_than_the_curve_grid():
    """16 384 waves and 512 workgroups are the grid caps (vocap.hip): 16 600 pairs and 200 classes x 3 thresholds stride"""
    gt, dr = row_scene(1, 16600, 7, n_img=16600)
    h, _ = check_scene(gt, dr, [0.5], "pairs")
    assert len(h["pair_off"]) - 1 == 16600 > 16384
    gt = {"a": "".join("c%03d %d 0 %d 3\n" % (k, 6 * k, 6 * k + 3) for k in range(200))}
    dr = {"a": "".join("c%03d 0.%d %d 0 %d %d\n" % (k, 1 + k % 9, 6 * k, 6 * k + 3, 3 - k % 2) for k in range(200))}
    h, _ = check_scene(gt, dr, [0.4, 0.5, 0.75], "classes")
    assert len(h["classes"]) * 3 == 600 > 512


def test_workspace_contents_do_not_matter():
    gt, dr = R.random_scene(77)
    for dirt in (0x00, 0x01, 0xFF):
        check_scene(gt, dr, [0.5, 0.75], dirt, dirt)


def test_torch_op_eager():
    import torch
    import glsdet_amd.torch_ops  # noqa: F401
    gt, dr = R.random_scene(78)
    h = prepare(gt, dr)
    thr = [0.5, 0.75]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [up(h[k]) for k in ("dt_box", "score", "cls_off", "pair_off", "pair_det", "gt_off", "gt_box", "gt_difficult", "n_gt", "n_img")]
    args += [up(np.array(thr)), up(np.logspace(-2.0, 0.0, num=9))]
    got = [o.cpu().numpy() for o in torch.ops.glsdet.voc_ap(*args, True)]
    for a, b in zip(got, expected(gt, dr, thr, h)):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    bad = list(args)
    bad[4] = torch.zeros_like(args[4])                                # pair_det: no permutation
    with pytest.raises(RuntimeError, match="pair_det"):
        torch.ops.glsdet.voc_ap(*bad, True)
    bad = list(args)
    bad[2] = torch.flip(args[2], [0])                                 # cls_off: falls
    with pytest.raises(RuntimeError, match="cls_off"):
        torch.ops.glsdet.voc_ap(*bad, True)
    with pytest.raises(RuntimeError, match="score"):
        torch.ops.glsdet.voc_ap(args[0], args[1].float(), *args[2:])


def test_load_dirs_and_get_map_write_the_recorded_results(tmp_path, capsys):
    from glsdet_amd.eval.voc import VocEval, get_map
    g, scenes = R.load_golden()
    for name, (gt, dr) in scenes.items():
        root = tmp_path / name
        for sub, texts in (("ground-truth", gt), ("detection-results", dr)):
            os.makedirs(root / sub)
            for fid, text in texts.items():
                (root / sub / (fid + ".txt")).write_text(text)
        for thr in (0.5, 0.75):
            capsys.readouterr()
            ev = get_map(thr, False, path=str(root))
            printed = capsys.readouterr().out.splitlines()
            p = "%s/%g/" % (name, thr)
            assert (root / "results" / "results.txt").read_bytes() == g[p + "results"].tobytes(), (name, thr)
            assert printed == g[p + "printed"].tolist(), (name, thr)
            want = R.evaluate(gt, dr, thr)
            assert ev["mAP"] == want["mAP"] and ev["classes"] == want["classes"]
            for c in ev["classes"]:
                a, b = ev["per_class"][c], want["per_class"][c]
                assert abs(float(a["lamr"]) - float(b["lamr"])) <= 1e-12 * abs(float(b["lamr"]))
                assert (a["n_gt"], a["n_images"], a["n_det"], a["n_tp"]) == (b["n_gt"], b["n_images"], b["n_det"], b["n_tp"])
    gt, dr = scenes["difficult"]
    two = VocEval().load_dirs(str(tmp_path / "difficult" / "ground-truth"), str(tmp_path / "difficult" / "detection-results")) \
        .evaluate([0.5, 0.75])
    assert [e["min_overlap"] for e in two] == [0.5, 0.75] and two[0]["mAP"] == R.evaluate(gt, dr, 0.5)["mAP"]
    with pytest.warns(UserWarning, match="plots are not drawn"):
        get_map(0.5, True, path=str(tmp_path / "difficult"))
    os.remove(tmp_path / "difficult" / "detection-results" / "a.txt")
    with pytest.raises(FileNotFoundError):
        get_map(0.5, False, path=str(tmp_path / "difficult"))
