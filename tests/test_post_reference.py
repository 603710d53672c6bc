"""CPU checks of the naive post-processing reference (tests/post_reference.py) that tests/test_post_fuzz.py holds the
HIP kernels to: it agrees with the oracle where both are defined alike, its float32 suppress decisions equal the
exact-arithmetic ones on every case of the GPU matrix (the condition that lets the GPU tests demand bit equality),
and hand-computed known answers."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import glsdet_oracle as O
from tests import post_reference as R

NMS_CASES = R.nms_cases()


def _ref_and_oracle(pred_i, nc, mode, thr):
    c = R.candidates(pred_i, nc, mode)
    mine = R.greedy_nms(c["boxes"], c["scores"], c["labels"], c["anchors"], thr)
    theirs = O.batched_nms(c["boxes"], c["scores"], c["labels"].astype(np.float32), thr)
    return c, mine, theirs


@pytest.mark.parametrize("m,struct,thr", [(500, "clusters", 0.5), (1300, "clusters", 0.65), (450, "chain", 0.5),
                                          (300, "exact", 0.65), (300, "exact", 0.5), (200, "degenerate", 0.5),
                                          (64, "identical", 0.5), (400, "disjoint", 0.0)])
def test_greedy_nms_equals_the_oracle_on_tie_free_inputs(m, struct, thr):
    """distinct scores: the two independent implementations return the same indices in the same order"""
    sc = "desc" if struct == "chain" else "distinct"
    im = R.build_image(2000, 7, m, struct=struct, scores=sc, thr=thr, seed=m)
    for mode in (0, 1):
        c, mine, theirs = _ref_and_oracle(R.to_pred([im], 7, mode)[0], 7, mode, thr)
        assert len(c["scores"]) == m and len(np.unique(c["scores"])) == m
        np.testing.assert_array_equal(mine, theirs)
        assert 0 < len(mine) <= m


def test_cross_class_ties_differ_from_the_oracle_in_order_only():
    """Equal scores in different classes: the kernels' contract (and greedy_nms) is anchor ascending; the oracle
    concatenates its per-class results before a stable sort, so it orders such ties class first.  Same set, and inside
    every class the same order; the overall order really differs on this input (so the difference stays documented)."""
    im = R.build_image(1500, 6, 600, struct="clusters", scores="few", seed=5)
    c, mine, theirs = _ref_and_oracle(R.to_pred([im], 6, 1)[0], 6, 1, 0.5)
    assert sorted(mine.tolist()) == sorted(theirs.tolist())
    assert not np.array_equal(mine, theirs)
    for k in range(6):
        np.testing.assert_array_equal(mine[c["labels"][mine] == k], theirs[c["labels"][theirs] == k])
    np.testing.assert_array_equal(c["scores"][mine], c["scores"][theirs])
    s, a = c["scores"][mine], c["anchors"][mine]
    assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (a[:-1] < a[1:])))
    # the oracle's order: score desc, then class asc, then anchor asc
    s, l, a = c["scores"][theirs], c["labels"][theirs], c["anchors"][theirs]
    assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & ((l[:-1] < l[1:]) | ((l[:-1] == l[1:]) & (a[:-1] < a[1:])))))


def _pairwise_agreement(boxes, labels, thr):
    """every same-class pair: float32 formula == exact arithmetic.  -> (pairs checked, pairs that suppress)"""
    npairs = nsup = 0
    for k in np.unique(labels):
        b = boxes[labels == k]
        u = R.to_units(b)
        for r0 in range(0, len(b), 256):
            rows = np.arange(r0, min(len(b), r0 + 256))
            want = R.exact_suppress_matrix(u[r0:], rows - r0, thr)           # columns r0 ...: the upper triangle
            got = np.stack([R.suppresses_row(b[r], b[r0:], thr) for r in rows])
            bad = np.argwhere(got != want)
            assert len(bad) == 0, "class %d: float32 and exact decisions differ for boxes %s / %s" % (
                k, b[r0 + bad[0][0]], b[r0 + bad[0][1]])
            npairs += got.size
            nsup += int(got.sum())
    return npairs, nsup


@pytest.mark.parametrize("case", NMS_CASES, ids=[c["id"] for c in NMS_CASES])
def test_float32_and_exact_decisions_agree_on_every_case_of_the_gpu_matrix(case):
    pred, images = R.build_case(case)
    for i, im in enumerate(images):
        c = R.candidates(pred[i], case["nc"], case["mode"])
        assert len(c["anchors"]) == im["m"] == case["ms"][i]                 # exactly m candidates pass the filter
        np.testing.assert_array_equal(c["boxes"], im["boxes"][c["anchors"]])  # the centre form decodes exactly
        np.testing.assert_array_equal(c["labels"], im["label"][c["anchors"]])
        _pairwise_agreement(c["boxes"], c["labels"], case["thr"])


@pytest.mark.parametrize("struct,thr", [(s, t) for s in R.STRUCTURES for t in (0.0, 0.5, 0.65, 1.0)
                                        if not (s == "chain" and t == 1.0)])        # no chain at 1.0: nothing suppresses
def test_builders_do_what_they_say_and_scalar_exact_equals_vectorised(struct, thr):
    rng = np.random.default_rng(7)
    m = 90
    b = R.build_boxes(struct, m, thr, rng)
    u = R.to_units(b)
    vec = R.exact_suppress_matrix(u, np.arange(m), thr)
    f32 = np.stack([R.suppresses_row(b[i], b, thr) for i in range(m)])
    for i in range(m):
        for j in range(i + 1, m, 1 if struct in ("exact", "chain") else 7):
            e = R.exact_suppresses(b[i], b[j], thr)
            assert e == vec[i, j] == f32[i, j] == f32[j, i], (struct, thr, i, j)
    keep = R.greedy_nms(b, np.linspace(1, 0.5, m).astype(np.float32), np.zeros(m, int), np.arange(m), thr).tolist()
    if struct == "chain":
        assert keep == list(range(0, m, 2))            # i suppresses i + 1 and not i + 2
    if struct == "disjoint":
        assert keep == list(range(m)) and not f32[~np.eye(m, dtype=bool)].any()
    if struct == "identical":
        assert keep == (list(range(m)) if thr == 1.0 else [0])
    if struct == "exact":                              # pairs 0, 3, 6 ... sit on the threshold: kept; a step above: dropped
        pairs = [(f32[2 * j, 2 * j + 1]) for j in range(m // 2)]
        assert not any(pairs[0::3])
        if thr < 1.0:
            assert all(pairs[1::3])
        assert not any(pairs[2::3])
    if struct == "degenerate":
        assert np.isnan(R.iou_row(b[0], b[:1])[0]) and (len(keep) < m or thr == 1.0)


def test_round_to_f32_is_numpys_rounding():
    rng = np.random.default_rng(0)
    for _ in range(300):
        p, q = int(rng.integers(0, 1 << 24)), int(rng.integers(1, 1 << 24))
        assert R.round_to_f32(Fraction(p, q)) == Fraction(float(np.float32(p) / np.float32(q)))
    assert R.round_to_f32(Fraction(13, 20)) == Fraction(float(np.float32(0.65)))
    assert R.round_to_f32(Fraction(1, 2 ** 150)) == 0 and R.round_to_f32(Fraction(3, 2 ** 150)) == Fraction(1, 2 ** 148)
    with pytest.raises(ValueError):
        R.exact_suppresses([0, 0, 4097 / 4096, 4097 / 4096], [0, 0, 1, 1], 0.5)     # area needs 26 bits


def test_known_answers_by_hand():
    """a = 4x4; b = a shifted by 2 (IoU 8/24 = 1/3); c = the left half of a (IoU 8/16 = 0.5 with a, 4/20 = 0.2 with b);
    z = a zero-area box inside a (IoU 0 with a; 0/0 with its own duplicate z2); d far away."""
    a, b, c = [0, 0, 4, 4], [2, 0, 6, 4], [0, 0, 2, 4]
    z, z2, d = [1, 1, 1, 3], [1, 1, 1, 3], [40, 40, 44, 44]
    np.testing.assert_array_equal(R.iou_row(a, [b, c, z, d]), np.float32([8 / 24, 0.5, 0, 0]))
    assert np.isnan(R.iou_row(z, [z2])[0])
    boxes = np.float32([a, b, c, z, z2, d])
    scores = np.float32([0.9, 0.8, 0.7, 0.6, 0.6, 0.5])
    same = np.zeros(6, int)
    nms = lambda thr, lab=same, an=np.arange(6): R.greedy_nms(boxes, scores, lab, an, thr).tolist()
    assert nms(0.5) == [0, 1, 2, 3, 4, 5]              # IoU(a, c) == 0.5 is not > 0.5; 0/0 does not suppress
    assert nms(0.4) == [0, 1, 3, 4, 5]                 # c goes (0.5 > 0.4)
    assert nms(0.3) == [0, 3, 4, 5]                    # b goes (1/3 > 0.3), and c (a is kept)
    assert nms(0.0) == [0, 3, 4, 5]                    # z: inter 0 with a -> IoU 0, not > 0
    assert nms(0.3, np.array([0, 1, 0, 0, 0, 1])) == [0, 1, 3, 4, 5]         # b in another class survives, c does not
    assert nms(0.5, same, np.array([0, 1, 2, 9, 4, 5])) == [0, 1, 2, 4, 3, 5]        # equal scores: anchor ascending
    assert R.exact_suppresses(a, c, 0.5) is False and R.exact_suppresses(a, c, 0.4999) is True
    assert R.exact_suppresses(z, z2, 0.0) is False and R.exact_suppresses(a, b, 0.3) is True
    # '+1' areas: [0,0,9,9] vs [1,1,10,10] -> 81 / 119
    assert R.exact_suppresses([0, 0, 9, 9], [1, 1, 10, 10], 0.68, one=1.0) is True
    assert R.exact_suppresses([0, 0, 9, 9], [1, 1, 10, 10], 0.69, one=1.0) is False
    assert R.iou_row([0, 0, 9, 9], [[1, 1, 10, 10]], one=1.0)[0] == np.float32(81) / np.float32(119)


def test_to_pred_and_candidates_round_trip_and_first_maximum():
    im = R.build_image(300, 5, 120, scores="few", seed=1)
    for mode in (0, 1):
        pred = R.to_pred([im], 5, mode)
        assert pred.shape == (1, 300, 10) and pred.dtype == np.float32
        c = R.candidates(pred[0], 5, mode)
        assert len(c["anchors"]) == 120 and not np.array_equal(c["anchors"], np.arange(120))   # scattered, not a prefix
        np.testing.assert_array_equal(c["rows"][:, :4], im["boxes"][c["anchors"]])
        np.testing.assert_array_equal(c["scores"], (im["obj"] * im["conf"])[c["anchors"]])
        assert c["scores"].min() == np.float32(R.CONF_THR)                   # the filter is >=
        assert len(np.unique(c["scores"])) <= 2 * len(R.TIE_TABLE)
    p = np.zeros((2, 8), np.float32)
    p[:, :4], p[:, 4], p[0, 6], p[0, 7], p[1, 5] = [1, 1, 2, 2], 1.0, 0.5, 0.5, 0.3
    assert R.candidates(p, 3, 1)["labels"].tolist() == [1, 0]                # first maximum wins
