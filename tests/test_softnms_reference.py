"""CPU-only: tests/softnms_reference.py (the naive restatement the GPU tests compare glsdet_soft_nms with) equals the
reference's own recorded outputs bit for bit -- tests/golden/softnms_golden.npz, written by tools/make_softnms_golden.py
from py_cpu_softnms / batched_soft_nms (drone/merge_results.py:41-130) -- and the recorded data is sharp enough to see
each of seven planted mistakes.  Also what of the new surface can be checked without a GPU: the margin condition of the
gaussian fuzz seeds, ResultMerger's argument validation, the ctypes table and the host refusals."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import softnms_reference as S

MUTANTS = ("swap_le", "last_max", "rotate", "area_no_plus1", "fp64_scores", "nt_ge", "thresh_ge")


@pytest.fixture(scope="module")
def gold():
    return S.load_golden()


def _param_sets(g):
    for ci in range(int(g["n_cases"])):
        for pi in range(int(g["c%d/n_params" % ci])):
            method, nt, sigma, thresh = g["c%d/p%d/params" % (ci, pi)].tolist()
            yield ci, pi, int(method), nt, sigma, thresh


def _restated(g, ci, method, nt, sigma, thresh, mutant=None):
    """-> (scores by position, keep, nkeep) concatenated over the classes present in ascending order, and the batched order"""
    boxes, scores, labels = g["c%d/boxes" % ci], g["c%d/scores" % ci], g["c%d/labels" % ci]
    sc, keep, nkeep = [np.zeros(0, np.float32)], [np.zeros(0, np.int64)], []
    for c in sorted(set(labels.tolist())):
        rows = np.where(labels == c)[0]
        seg = S.segment(boxes[rows], scores[rows], method, nt, sigma, thresh, mutant)
        sc.append(seg["scores"])
        keep.append(seg["keep"])
        nkeep.append(len(seg["keep"]))
    order = S.batched(boxes, scores, labels, method, nt, sigma, thresh, mutant=mutant)["order"]
    return np.concatenate(sc), np.concatenate(keep), np.asarray(nkeep, np.int64), order


def _canonical(g, ci, order):
    """The recorded order is the reference's `scores[keep].sort(descending=True)`: descending in the original score,
    and among EQUAL scores whatever torch.sort happened to do (unspecified; it is not by index).  Where the kept scores
    are all distinct the recorded order is returned verbatim.  Otherwise -- the project's contract sends ties to the
    lower original index -- the recorded order is checked to be descending and its runs of equal scores are put in index
    order before the comparison.  -> (order to compare with, whether it is the recorded one verbatim)"""
    sc = g["c%d/scores" % ci]
    order = [int(v) for v in order]
    if len({float(sc[r]) for r in order}) == len(order):
        return order, True
    assert all(sc[a] >= sc[b] for a, b in zip(order, order[1:]))
    return sorted(order, key=lambda r: (-float(sc[r]), r)), False


def test_golden_covers_what_it_claims(gold):
    sets = list(_param_sets(gold))
    assert int(gold["n_cases"]) >= 40 and {s[2] for s in sets} == {1, 2, 3}
    ns = [len(gold["c%d/scores" % ci]) for ci in range(int(gold["n_cases"]))]
    assert min(ns) == 0 and max(ns) == 80
    ncls = {len(set(gold["c%d/labels" % ci].tolist())) for ci in range(int(gold["n_cases"]))}
    assert 1 in ncls and max(ncls) >= 9
    frac = [bool((gold["c%d/boxes" % ci] % 1 != 0).any()) for ci in range(int(gold["n_cases"]))]
    assert any(frac) and not all(frac)
    assert len({s[3:] for s in sets}) >= 4                                   # the reference's Nt / sigma / thresh and others


def test_restatement_equals_every_recorded_array_bit_for_bit(gold):
    n = verbatim = 0
    for ci, pi, method, nt, sigma, thresh in _param_sets(gold):
        sc, keep, nkeep, order = _restated(gold, ci, method, nt, sigma, thresh)
        key = "c%d/p%d/" % (ci, pi)
        want = gold[key + "scores"]
        assert sc.dtype == want.dtype == np.float32
        assert sc.view(np.uint32).tolist() == want.view(np.uint32).tolist(), key
        assert keep.tolist() == gold[key + "keep"].tolist() and nkeep.tolist() == gold[key + "nkeep"].tolist(), key
        want_order, as_recorded = _canonical(gold, ci, gold[key + "order"])
        assert order.tolist() == want_order, key
        verbatim += as_recorded and len(want_order) > 1
        n += 1
    assert n >= 150 and verbatim >= 60                                        # most orders are compared exactly as recorded


@pytest.mark.parametrize("mutant", MUTANTS)
def test_the_recorded_data_sees_the_mistake(gold, mutant):
    differing = 0
    for ci, pi, method, nt, sigma, thresh in _param_sets(gold):
        sc, keep, nkeep, order = _restated(gold, ci, method, nt, sigma, thresh, mutant)
        key = "c%d/p%d/" % (ci, pi)
        same = (sc.view(np.uint32).tolist() == gold[key + "scores"].view(np.uint32).tolist()
                and keep.tolist() == gold[key + "keep"].tolist()
                and order.tolist() == _canonical(gold, ci, gold[key + "order"])[0])
        differing += not same
    assert differing >= 1, "no recorded case distinguishes the mutant " + mutant


def test_merged_files_equal_the_recorded_lines(gold, tmp_path):
    from glsdet_amd.eval.results import VISDRONE_CLASSES, parse_detection_results
    index = {c: i for i, c in enumerate(VISDRONE_CLASSES)}
    assert int(gold["n_scenes"]) == 3
    dropped = []
    for si in range(3):
        rows = []
        for k in "ab":
            p = tmp_path / ("%d%s.txt" % (si, k))
            p.write_text(gold["s%d/%s" % (si, k)])
            rows += parse_detection_results(str(p), index)
        lines = S.merged_lines(np.asarray(rows, np.float32).reshape(-1, 6), VISDRONE_CLASSES)
        assert "".join(lines) == gold["s%d/out" % si]
        assert 0 < len(lines) <= len(rows)
        dropped.append(len(rows) - len(lines))
    assert dropped[0] > 0 and dropped[1] > 0                                 # the crowded scenes lose rows, see the generator


def test_gaussian_fuzz_seeds_meet_the_margin_condition():
    """The GPU test compares keep sets and orders of the gaussian cases although the decayed scores may differ by
    u * 2^-23 relative: that is sound only when no selection and no threshold decision sits inside that band.  Every
    seed's two recorded gaps must exceed N * 2^-23 (N >= every update count) by a factor of 4."""
    from tests.softnms_cases import GAUSSIAN_CASES, gaussian_rows
    assert len(GAUSSIAN_CASES) >= 6
    for case in GAUSSIAN_CASES:
        rows = gaussian_rows(case)
        N = max(len(r) for r in rows)
        for r in rows:
            res = S.batched(r[:, :4], r[:, 4], r[:, 5].astype(np.int64), 2, case["nt"], case["sigma"], case["thresh"])
            bound = 4 * N * 2.0 ** -23
            assert res["sel_gap"] > bound and res["thr_gap"] > bound, (case, res["sel_gap"], res["thr_gap"], bound)
            assert int(res["updates"].max(initial=0)) <= N


# ------------------------------------------------------------------------------------------------ surface, no GPU
def test_lib_declares_the_three_symbols():
    from glsdet_amd import _lib
    for name in ("glsdet_soft_nms_workspace_bytes", "glsdet_soft_nms_segment_limit", "glsdet_soft_nms"):
        assert name in _lib.EXPORTS
    assert _lib.ABI_VERSION == 17
    assert _lib._SIGS["glsdet_soft_nms"][1][6:9] == [C.c_double, C.c_double, C.c_float]     # Nt and sigma stay fp64


def test_segment_limit_is_what_the_lds_layout_holds():
    from glsdet_amd import _lib
    lib = _lib.load()
    limit = lib.glsdet_soft_nms_segment_limit()
    assert limit == (160 * 1024 - 1024) // 24 == 6784                       # box 16 + score 4 + index 4 bytes, 1 KiB of slots
    assert lib.glsdet_soft_nms_workspace_bytes(2, 100) == 1024 and lib.glsdet_soft_nms_workspace_bytes(1, 32768) == 131072
    assert lib.glsdet_soft_nms_workspace_bytes(0, 100) == 0 and lib.glsdet_soft_nms_workspace_bytes(1, 32769) == 0


def test_host_refusals_launch_nothing():
    """Every malformed call is refused with a negative code and a message before anything is launched: the pointers are
    never dereferenced, so this runs without a GPU."""
    from glsdet_amd import _lib
    lib = _lib.load()
    good = dict(cand=0x10000, cnt=0x20000, n=1, cap=64, nc=10, method=2, nt=0.3, sigma=0.5, thr=1e-4, rescore=0, max_det=64,
                dets=0x30000, count=0x40000, status=0x50000, ws=0x60000, ws_bytes=1 << 20)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.glsdet_soft_nms(a["cand"], a["cnt"], a["n"], a["cap"], a["nc"], a["method"], a["nt"], a["sigma"], a["thr"],
                                 a["rescore"], a["max_det"], a["dets"], a["count"], a["status"], a["ws"], a["ws_bytes"], None)
        return rc, lib.glsdet_last_error().decode()

    for kw, code, text in ((dict(n=0), -1, "bad sizes"), (dict(cap=32769), -1, "32768"), (dict(cap=0), -1, "bad sizes"),
                           (dict(max_det=0), -1, "bad sizes"), (dict(nc=0), -1, "num_classes"),
                           (dict(method=0), -1, "method"), (dict(method=4), -1, "method"),
                           (dict(sigma=0.0), -1, "sigma"), (dict(sigma=-1.0), -1, "sigma"), (dict(sigma=float("nan")), -1, "sigma"),
                           (dict(nt=float("nan")), -1, "NaN"), (dict(thr=-1e-4), -1, "min_score"),
                           (dict(thr=float("nan")), -1, "min_score"), (dict(thr=float("inf")), -1, "min_score"), (dict(cand=None), -1, "null"), (dict(ws=None), -1, "null"),
                           (dict(cand=0x10008), -3, "aligned"), (dict(dets=0x30002), -3, "aligned"),
                           (dict(ws=0x60080), -3, "256-byte"), (dict(ws_bytes=255), -5, "workspace")):
        rc, msg = call(**kw)
        assert rc == code and "soft_nms" in msg and text in msg, (kw, rc, msg)
    # sigma is only read by the gaussian decay
    # (a well-formed call is not made here: it would launch)


def test_result_merger_argument_validation_needs_no_gpu():
    from glsdet_amd.eval.results import ResultMerger
    for kw in (dict(method="gauss"), dict(method="soft", soft_method="quadratic"), dict(method="soft", sigma=0.0),
               dict(method="soft", sigma=-0.5), dict(method="soft", iou_thr=float("nan")), dict(method="soft", min_score=-0.1),
               dict(method="soft", min_score=float("nan")),
               dict(method="soft", capacity=32769), dict(method="soft", capacity=0), dict(rescore=True)):
        with pytest.raises(ValueError):
            ResultMerger(device="cpu", **kw)
    import inspect
    sig = inspect.signature(ResultMerger.__init__).parameters
    assert [sig[k].default for k in ("method", "soft_method", "sigma", "iou_thr", "min_score", "rescore")] == \
        ["hard", "gaussian", 0.5, 0.3, 1e-4, False]
    assert sig["nms_thres"].default == 0.65 and sig["capacity"].default == 8192


def test_header_cites_the_reference_and_states_the_contract():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "glsdet_hip.h")).read()
    for text in ("drone/merge_results.py:41-130", ":159-163", "glsdet_soft_nms_segment_limit() = 6784", "FIRST position",
                 "one rounding to fp32 per update", "#define GLSDET_ABI_VERSION 17"):
        assert text in src, text
