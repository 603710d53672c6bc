"""GPU: glsdet_soft_nms (ABI 17; py_cpu_softnms / batched_soft_nms, drone/merge_results.py:41-130) against the naive
restatement tests/softnms_reference.py, which tests/test_softnms_reference.py pins bit for bit to the reference's own
recorded outputs.

Linear and hard decay: every fp64 step is an IEEE operation on both sides, so all seven columns, both counts and the
status must come out bit for bit, on dyadic and on free fp32 inputs alike.  Gaussian decay: the weight is an fp64 `exp`
on either side (each good to an ulp or so); after the rounding to fp32 two updates of one score differ by at most one
fp32 ulp, so a decayed score may be off by u * 2^-23 relative after u updates -- that bound is asserted per row, the kept
rows and their order must be equal (the seeds keep every decision clear of the band, asserted on the CPU).  Largest
gaussian difference observed on an MI355X: see DESIGN section 4.

`dets` is filled with a sentinel before every launch and compared WHOLE: rows at and beyond the count stay untouched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import softnms_reference as S
from tests.softnms_cases import GAUSSIAN_CASES, dyadic_rows, gaussian_rows, random_rows

pytestmark = pytest.mark.gpu
SENT = -12345.5
M = S.METHODS


@pytest.fixture(scope="module")
def eng():
    from glsdet_amd.engine import Engine
    return Engine("f32")


def _launch(eng, images, nc, method, nt=0.3, sigma=0.5, thresh=1e-4, rescore=False, max_det=None, cap=None, counts=None,
            pad=0.0):
    """images: per image fp32 [n_b, 6] rows -> (dets [n, max_det, 7] with the sentinel where nothing was written,
    count [2n], status).  counts overrides the device counts; pad fills what the kernel must not read (columns 6, 7 and
    the rows beyond the count)."""
    n = len(images)
    cap = cap or max(max(len(r) for r in images) + 3, 1)
    max_det = max_det or cap
    host = np.full((n, cap, 8), pad, np.float32)
    for b, r in enumerate(images):
        host[b, : len(r), :6] = np.asarray(r, np.float32).reshape(-1, 6)
    sb = eng.soft_nms_buffers(n, cap, max_det)
    sb["dets"].fill_(SENT)
    cnt = torch.tensor([len(r) for r in images] if counts is None else counts, dtype=torch.int32).cuda()
    name = {v: k for k, v in M.items()}[method]
    dets, count, status = eng.soft_nms(torch.from_numpy(host).cuda(), cnt, nc, sb, name, nt, sigma, thresh, rescore)
    torch.cuda.synchronize()
    return dets.cpu().numpy(), count.cpu().numpy(), int(status.item())


def _want(images, method, nt, sigma, thresh, rescore, max_det):
    """-> (dets [n, max_det, 7] sentinel-filled, count [2n], the per-image `batched` dicts)"""
    n = len(images)
    dets = np.full((n, max_det, 7), SENT, np.float32)
    count = np.zeros(2 * n, np.int32)
    infos = []
    for b, r in enumerate(images):
        d, K, info = S.detections(np.asarray(r, np.float32).reshape(-1, 6), method, nt, sigma, thresh, rescore, max_det)
        dets[b, : len(d)] = d
        count[b], count[n + b] = len(d), K
        infos.append(info)
    return dets, count, infos


def _exact(eng, images, nc, method, nt=0.3, sigma=0.5, thresh=1e-4, rescore=False, max_det=None, cap=None, pad=0.0):
    cap = cap or max(max(len(r) for r in images) + 3, 1)
    max_det = max_det or cap
    dets, count, status = _launch(eng, images, nc, method, nt, sigma, thresh, rescore, max_det, cap, pad=pad)
    want, wcount, infos = _want(images, method, nt, sigma, thresh, rescore, max_det)
    assert status == 0
    assert count.tolist() == wcount.tolist()
    assert dets.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    return wcount, infos


# ------------------------------------------------------------------------------------------------ linear / hard: bit for bit
@pytest.mark.parametrize("method", ["linear", "hard"])
@pytest.mark.parametrize("kind", ["dyadic", "free", "integer"])
def test_linear_and_hard_equal_the_restatement_bit_for_bit(eng, method, kind):
    make = {"dyadic": lambda s, n: dyadic_rows(s, n, 3), "free": lambda s, n: random_rows(s, n, 3),
            "integer": lambda s, n: random_rows(s, n, 3, integer=True)}[kind]
    images = [make(11, 150), make(12, 0), make(13, 97)]
    wcount, _ = _exact(eng, images, 3, M[method])
    assert 0 < wcount[3] <= 150 and wcount[4] == 0
    if method == "hard":
        assert wcount[3] < 150 and wcount[5] < 97                            # something is suppressed


@pytest.mark.parametrize("method", ["linear", "hard"])
def test_other_thresholds(eng, method):
    images = [dyadic_rows(21, 120, 2), random_rows(22, 90, 2)]
    _exact(eng, images, 2, M[method], nt=0.5, thresh=0.25)
    _exact(eng, images, 2, M[method], nt=0.125, thresh=0.001)


# ------------------------------------------------------------------------------------------------ gaussian: bounded
@pytest.mark.parametrize("ci", range(len(GAUSSIAN_CASES)))
def test_gaussian_keeps_the_same_rows_in_the_same_order_and_scores_within_one_ulp_per_update(eng, ci):
    case = GAUSSIAN_CASES[ci]
    images = gaussian_rows(case)
    cap = max(case["counts"]) + 3
    dets, count, status = _launch(eng, images, case["nc"], 2, case["nt"], case["sigma"], case["thresh"], cap=cap)
    want, wcount, infos = _want(images, 2, case["nt"], case["sigma"], case["thresh"], False, cap)
    assert status == 0 and count.tolist() == wcount.tolist()
    exact = [0, 1, 2, 3, 4, 6]
    assert dets[:, :, exact].view(np.uint32).tolist() == want[:, :, exact].view(np.uint32).tolist()     # rows, order, sentinel
    worst = 0.0
    for b, info in enumerate(infos):
        k = int(wcount[b])
        u = info["updates"][info["order"][:k]]
        got, ref = dets[b, :k, 5].astype(np.float64), want[b, :k, 5].astype(np.float64)
        rel = np.abs(got - ref) / ref
        worst = max(worst, float(rel.max(initial=0.0)))
        assert (rel <= u * 2.0 ** -23).all(), (b, rel.max(), u)
    assert (dets[:, :, 5][want[:, :, 5] == np.float32(SENT)] == np.float32(SENT)).all()
    print("gaussian case %d: largest relative difference of a decayed score %.3e" % (ci, worst))


def test_gaussian_without_any_overlap_is_exact(eng):
    """disjoint boxes: every ovr is 0, every weight exp(-0) = 1, every fp64 step exact"""
    rng = np.random.default_rng(5)
    n = 70
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0] = 8 * (np.arange(n) % 10)
    rows[:, 1] = 8 * (np.arange(n) // 10)
    rows[:, 2:4] = rows[:, :2] + 4
    rows[:, 4] = rng.integers(1, 9, n) / 8.0
    rows[:, 5] = rng.integers(0, 2, n)
    wcount, _ = _exact(eng, [rows], 2, 2)
    assert wcount[0] == n


# ------------------------------------------------------------------------------------------------ exact edges
@pytest.mark.parametrize("method", ["linear", "hard"])
def test_counts_and_segments(eng, method):
    m = M[method]
    _exact(eng, [np.zeros((0, 6), np.float32)], 4, m)                        # an empty image
    _exact(eng, [dyadic_rows(1, 1, 1)], 1, m)                                # one row
    _exact(eng, [dyadic_rows(2, 80, 1)], 1, m)                               # one class only
    rows = dyadic_rows(3, 80, 1)
    rows[:, 5] = 7
    _exact(eng, [rows], 10, m)                                               # ten classes, nine of them empty
    _exact(eng, [dyadic_rows(4, 70, 4), np.zeros((0, 6), np.float32), dyadic_rows(5, 33, 4)], 4, m, cap=75)   # ragged


@pytest.mark.parametrize("method", ["linear", "hard"])
def test_ties(eng, method):
    twin = np.float32([[2, 2, 9, 9, 0.5, 0], [2, 2, 9, 9, 0.5, 0], [2, 2, 9, 9, 0.5, 0], [30, 30, 34, 34, 0.5, 0]])
    wcount, infos = _exact(eng, [twin], 1, M[method])
    if method == "hard":
        assert infos[0]["order"].tolist() == [0, 3]                          # the first twin stays, by position
    # equal scores all over: which of them is selected depends on the swaps made so far
    _exact(eng, [dyadic_rows(31, 200, 2, span=24, score_grid=4), dyadic_rows(32, 64, 1, span=16, score_grid=2)], 2, M[method])


def test_thresholds_are_strict(eng):
    # ovr = 2 / 4 = 0.5 exactly: `ovr > Nt` is false at Nt = 0.5, true just below
    pair = np.float32([[0, 0, 2, 0, 0.75, 0], [1, 0, 3, 0, 0.5, 0]])
    for m in (1, 3):
        _, infos = _exact(eng, [pair], 1, m, nt=0.5)
        assert infos[0]["decayed"].tolist() == [0.75, 0.5]
    _, infos = _exact(eng, [pair], 1, 3, nt=0.4375)
    assert infos[0]["order"].tolist() == [0]
    # linear: 0.5 * (1 - 0.5) = 0.25 = min_score exactly: dropped (strict `>`), kept just below
    wcount, infos = _exact(eng, [pair], 1, 1, nt=0.25, thresh=0.25)
    assert infos[0]["decayed"].tolist() == [0.75, 0.25] and wcount[0] == 1
    wcount, _ = _exact(eng, [pair], 1, 1, nt=0.25, thresh=0.2499)
    assert wcount[0] == 2
    # an undecayed score that IS fp32(1e-4)
    wcount, _ = _exact(eng, [np.float32([[0, 0, 4, 4, np.float32(1e-4), 0], [20, 20, 24, 24, 0.5, 0]])], 1, 1)
    assert wcount[0] == 1


@pytest.mark.parametrize("method", ["linear", "hard"])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025])
def test_wave_and_block_edges(eng, n, method):
    """one class of n rows: 64 is a wave, 1024 the block"""
    wcount, _ = _exact(eng, [dyadic_rows(40 + n, n, 1, span=16 if n < 100 else 96)], 1, M[method])
    assert 0 < wcount[1] <= n


def _limit_rows(n, twins):
    """n rows of one class on a grid of disjoint 3 x 3 boxes, scores a permutation of distinct dyadic values; the last
    `twins` rows repeat the boxes of the first `twins` rows: of each such pair the lower score meets ovr = 1."""
    rng = np.random.default_rng(n)
    j = np.arange(n)
    j[n - twins:] = np.arange(twins)
    rows = np.zeros((n, 6), np.float32)
    rows[:, 0], rows[:, 1] = 4 * (j % 128), 4 * (j // 128)
    rows[:, 2:4] = rows[:, :2] + 2
    rows[:, 4] = (1 + rng.permutation(n)) / 8192.0
    return rows


def test_segment_limit(eng):
    """The limit itself runs; the expectation is worked out by hand, the restatement's O(N^2) loop in Python would take
    a minute: hard decay, so of each twin pair the lower score is zeroed and everything else keeps its score; the output
    is the survivors by descending (distinct) score."""
    limit = eng.lib.glsdet_soft_nms_segment_limit()
    twins = 50
    rows = _limit_rows(limit, twins)
    dets, count, status = _launch(eng, [rows], 1, 3, cap=limit)
    lose = [a if rows[a, 4] < rows[b, 4] else b for a, b in zip(range(twins), range(limit - twins, limit))]
    keep = np.setdiff1d(np.arange(limit), lose)
    keep = keep[np.argsort(-rows[keep, 4], kind="stable")]
    want = np.full((limit, 7), SENT, np.float32)
    want[: len(keep)] = np.concatenate([rows[keep, :5], rows[keep, 4:5], rows[keep, 5:6]], 1)
    assert status == 0 and count.tolist() == [limit - twins] * 2
    assert dets[0].view(np.uint32).tolist() == want.view(np.uint32).tolist()


def test_segment_over_the_limit_sets_status_bit_1(eng):
    """limit + 1 rows of one class: refused by status, every loop clamped; the second image's class 1 is fine but the
    call's results are invalid as a whole for the first"""
    limit = eng.lib.glsdet_soft_nms_segment_limit()
    rows = _limit_rows(limit + 1, 0)
    dets, count, status = _launch(eng, [rows], 2, 3, cap=limit + 1)
    assert status == 2
    assert count.tolist() == [0, 0] and (dets == np.float32(SENT)).all()     # the over-long segment is dropped whole
    rows[5, 5] = 1                                                           # one row fewer in class 0: exactly the limit
    _, count, status = _launch(eng, [rows], 2, 3, cap=limit + 1)
    assert status == 0 and count.tolist() == [limit + 1] * 2


def test_invalid_input_sets_the_status_bits(eng):
    rows = dyadic_rows(50, 40, 3)
    dets, count, status = _launch(eng, [rows], 3, 1, cap=40, counts=[45])    # a count above cap: clamped to cap, bit 0
    want, wcount, _ = _want([rows], 1, 0.3, 0.5, 1e-4, False, 40)            # ... and the 40 rows treated as 40 rows
    assert status == 1 and count.tolist() == wcount.tolist()
    assert dets.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    for bad in (3.0, -1.0, float("nan"), 1e9):
        r = rows.copy()
        r[7, 5] = bad
        dets, count, status = _launch(eng, [r], 3, 1)
        assert status == 2
        # the row with the bad label is dropped, the others are treated as if it were absent
        want, wcount, _ = _want([np.delete(r, 7, axis=0)], 1, 0.3, 0.5, 1e-4, False, 43)
        assert count.tolist() == wcount.tolist() and dets.view(np.uint32).tolist() == want.view(np.uint32).tolist()
    _, _, status = _launch(eng, [rows], 3, 1, counts=[-5])                   # a negative count reads nothing
    assert status == 0


@pytest.mark.parametrize("rescore", [False, True])
def test_max_det_and_rescore(eng, rescore):
    images = [dyadic_rows(60, 140, 2, span=24), dyadic_rows(61, 9, 2)]
    wcount, infos = _exact(eng, images, 2, 1, rescore=rescore, max_det=25, cap=150)
    assert wcount.tolist()[0] == 25 and wcount[2] > 25 and wcount[1] == wcount[3] <= 9      # clamped, then unclamped
    full, _ = _exact(eng, images, 2, 1, rescore=rescore)
    if rescore:
        other = S.batched(images[0][:, :4], images[0][:, 4], images[0][:, 5].astype(np.int64), 1)["order"]
        assert infos[0]["order"].tolist() != other.tolist()                  # the two orders really differ on this data


def test_candidate_buffer_layout_with_dirty_padding(eng):
    """rows as Engine.gfl_candidates leaves them in a reused buffer: columns 6 and 7 and the rows beyond the count hold
    anything (NaN here); nothing of it is read"""
    images = [dyadic_rows(70, 100, 3), dyadic_rows(71, 55, 3)]
    for m in (1, 3):
        _exact(eng, images, 3, m, cap=128, pad=float("nan"))


def test_host_refusals(eng):
    from glsdet_amd._lib import GlsdetError
    lib = eng.lib
    sb = eng.soft_nms_buffers(1, 64, 64)
    cand = torch.zeros(1, 64, 8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    sb["dets"].fill_(SENT)

    def call(n=1, cap=64, nc=3, method=2, nt=0.3, sigma=0.5, thr=1e-4, max_det=64, cand_p=None, ws=None, ws_bytes=None):
        return lib.glsdet_soft_nms(cand.data_ptr() if cand_p is None else cand_p, cnt.data_ptr(), n, cap, nc, method, nt, sigma,
                                   thr, 0, max_det, sb["dets"].data_ptr(), sb["count"].data_ptr(), sb["status"].data_ptr(),
                                   sb["ws"].data_ptr() if ws is None else ws, sb["ws"].numel() if ws_bytes is None else ws_bytes,
                                   None)

    for kw, code in ((dict(n=0), -1), (dict(cap=32769), -1), (dict(sigma=0.0), -1), (dict(sigma=-1.0), -1), (dict(method=5), -1),
                     (dict(max_det=0), -1), (dict(nc=0), -1), (dict(thr=-1e-4), -1), (dict(thr=float("inf")), -1), (dict(cand_p=cand.data_ptr() + 4), -3),
                     (dict(ws=sb["ws"].data_ptr() + 16), -3), (dict(ws_bytes=128), -5)):
        assert call(**kw) == code and "soft_nms" in lib.glsdet_last_error().decode(), kw
    assert call(method=1, sigma=0.0) == 0                                    # sigma belongs to the gaussian decay only
    torch.cuda.synchronize()
    assert (sb["dets"] == SENT).all() and sb["count"].cpu().tolist() == [0, 0]
    with pytest.raises(GlsdetError):
        eng.soft_nms_buffers(1, 32769, 10)
    with pytest.raises(ValueError):
        eng.soft_nms(cand, cnt, 3, sb, method="quadratic")


def test_recorded_in_a_plan_and_captured(eng):
    """like the other ops: recorded once, replayed eagerly (the warm-up every caller of capture makes, detector.py) and
    from a captured graph, reading the buffers of the moment"""
    a, b = dyadic_rows(80, 90, 3), dyadic_rows(81, 60, 3)
    cap = 3000                                # more than 64 KiB of LDS: the launch that raises the kernel's dynamic LDS limit
    sb = eng.soft_nms_buffers(1, cap, cap)
    cand = torch.zeros(1, cap, 8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    plan = eng.new_plan()
    with plan:
        eng.soft_nms(cand, cnt, 3, sb, "linear")
    assert plan.num_ops == 1

    def load(rows):
        cand.zero_()
        cand[0, : len(rows), :6] = torch.from_numpy(rows).cuda()
        cnt.fill_(len(rows))
        sb["dets"].fill_(SENT)
        torch.cuda.synchronize()

    def check(rows):
        want, wcount, _ = _want([rows], 1, 0.3, 0.5, 1e-4, False, cap)
        assert sb["count"].cpu().tolist() == wcount.tolist() and int(sb["status"].item()) == 0
        assert sb["dets"].cpu().numpy().view(np.uint32).tolist() == want.view(np.uint32).tolist()

    load(a)
    plan.run()
    torch.cuda.synchronize()
    check(a)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        plan.capture(st)
    st.synchronize()
    load(b)
    with torch.cuda.stream(st):
        plan.launch(st)
    st.synchronize()
    check(b)


# ------------------------------------------------------------------------------------------------ torch op, public surface
def test_torch_op(eng):
    import glsdet_amd.torch_ops  # noqa: F401
    images = [dyadic_rows(90, 75, 3), dyadic_rows(91, 20, 3)]
    cap = 80
    host = np.zeros((2, cap, 8), np.float32)
    for b, r in enumerate(images):
        host[b, : len(r), :6] = r
    cand, cnt = torch.from_numpy(host).cuda(), torch.tensor([75, 20], dtype=torch.int32).cuda()
    dets, count, status = torch.ops.glsdet.soft_nms(cand, cnt, 3, 1, 0.3, 0.5, 1e-4, False, cap)
    torch.cuda.synchronize()
    want, wcount, _ = _want(images, 1, 0.3, 0.5, 1e-4, False, cap)
    assert int(status.item()) == 0 and count.cpu().tolist() == wcount.tolist()
    for b in range(2):
        k = int(wcount[b])
        assert dets[b, :k].cpu().numpy().view(np.uint32).tolist() == want[b, :k].view(np.uint32).tolist()
        assert (dets[b, k:] == 0).all()                                      # the op hands out zeroed buffers
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.soft_nms(cand.cpu(), cnt.cpu(), 3, 1, 0.3, 0.5, 1e-4, False, cap)
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.soft_nms(cand[:, :, :7], cnt, 3, 1, 0.3, 0.5, 1e-4, False, cap)
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.soft_nms(cand, cnt.long(), 3, 1, 0.3, 0.5, 1e-4, False, cap)


def test_result_merger_soft_merge_dirs_equals_the_recorded_files(tmp_path):
    """the three recorded scenes: two result directories in, the merged files' TEXT equal to what the reference's own
    functions gave (gaussian, Nt 0.3, sigma 0.5, thresh 1e-4; distinct scores, so the order is fully specified)"""
    from glsdet_amd.eval.results import ResultMerger
    g = S.load_golden()
    da, db, out = tmp_path / "a", tmp_path / "b", tmp_path / "out"
    da.mkdir()
    db.mkdir()
    for si in range(int(g["n_scenes"])):
        (da / ("%d.txt" % si)).write_text(g["s%d/a" % si])
        (db / ("%d.txt" % si)).write_text(g["s%d/b" % si])
    merger = ResultMerger(method="soft", capacity=256)
    total = merger.merge_dirs([str(da), str(db)], str(out))
    for si in range(int(g["n_scenes"])):
        assert (out / ("%d.txt" % si)).read_text() == g["s%d/out" % si]
    assert total == sum(g["s%d/out" % si].count("\n") for si in range(int(g["n_scenes"])))
    # rescore (this project's addition): the decayed score is written and decides the order
    rows = merger.merge_rows(dyadic_rows(95, 60, 3))
    rs = ResultMerger(method="soft", soft_method="linear", capacity=256, rescore=True).merge_rows(dyadic_rows(95, 60, 3))
    want, _, _ = S.detections(dyadic_rows(95, 60, 3), 1, rescore=True)
    assert rs[:, 4].tolist() == want[:, 5].tolist() and (np.diff(rs[:, 4]) <= 0).all() and (np.diff(rows[:, 4]) <= 0).all()
    with pytest.raises(RuntimeError):
        merger.merge_rows(np.float32([[0, 0, 4, 4, 0.5, 10]]))               # class index outside the class list
    with pytest.raises(RuntimeError):
        merger.merge_rows(np.zeros((257, 6), np.float32))                    # more rows than the capacity
