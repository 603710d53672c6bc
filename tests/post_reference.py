"""An independent, deliberately naive reference of the detection post-processing (glsdet_amd/csrc/post.hip) and the
input builders of its differential tests.  TEST INFRASTRUCTURE ONLY; imports nothing from `oracle` -- it is the second
opinion that tests/test_post_reference.py holds against the oracle and tests/test_post_fuzz.py against the kernels.

Why the GPU tests may demand bit equality.  Every corner coordinate the builders produce is a multiple of 1/64 in
[0, 64) and every box side is at most 32.  In units of 1/64 a coordinate is an integer below 2^12, a side an integer
<= 2^11, an area or an intersection an integer <= 2^22 (units of 1/4096) and `area_a + area_b - inter` an integer
< 2^24: every difference, product and sum inside the IoU is exactly representable in float32, so it does not matter
whether the compiler contracts `a + b * c` into an FMA.  Only the final division rounds, and an IEEE division is
correctly rounded (the library is built without fast-math).  `exact_suppresses` restates the decision in integer /
Fraction arithmetic with that one rounding step; tests/test_post_reference.py checks on the CPU that it agrees with
the float32 formula on every same-class pair of every case below.  The centre form (box_mode 0) stores
cx = (x1 + x2) / 2 (a multiple of 1/128) and w = x2 - x1, so `cx - w / 2` is exact as well.  Scores are products of
dyadic numbers (k / 256, k / 16384, times 1 or 0.5): exact, and equal scores are equal bit for bit.

Order contract of both kernel families: (score descending, anchor ascending); suppression only inside a class."""
from fractions import Fraction

import numpy as np

F32 = np.float32
GRID = 64                  # coordinates are multiples of 1 / GRID in [0, GRID)
MAX_SIDE = 32.0
CONF_THR = 0.25


# --------------------------------------------------------------------------------------------------- float32 formula
def iou_row(a, B, one=0.0):
    """IoU of box a [4] with every row of B [k,4]: float32, in the operation order of nms_mask_kernel / nms_cmask_kernel
    (torchvision's formula; one = 1 gives the '+1' pixel-area convention).  0/0 gives NaN."""
    a, B, one = np.asarray(a, F32), np.asarray(B, F32).reshape(-1, 4), F32(one)
    aarea = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    w = np.maximum(F32(0), np.minimum(a[2], B[:, 2]) - np.maximum(a[0], B[:, 0]) + one)
    h = np.maximum(F32(0), np.minimum(a[3], B[:, 3]) - np.maximum(a[1], B[:, 1]) + one)
    inter = w * h
    barea = (B[:, 2] - B[:, 0] + one) * (B[:, 3] - B[:, 1] + one)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (aarea + barea - inter)


def suppresses_row(a, B, thr, one=0.0):
    """a suppresses row j of B  <=>  IoU > thr in float32; a NaN IoU does not suppress."""
    return iou_row(a, B, one) > F32(thr)


def greedy_nms(boxes, scores, labels, anchors, thr, one=0.0):
    """Sequential greedy NMS.  Candidates are visited in (score desc, anchor asc) order; a candidate is dropped if an
    earlier KEPT candidate of its class has IoU > thr with it.  -> indices of the kept candidates in visiting order."""
    boxes = np.asarray(boxes, F32).reshape(-1, 4)
    scores, labels, anchors = np.asarray(scores, F32), np.asarray(labels), np.asarray(anchors, np.int64)
    m = len(scores)
    order = np.lexsort((anchors, -scores))             # last key is the primary one
    rank = np.empty(m, np.int64)
    rank[order] = np.arange(m)
    kept = []
    for c in np.unique(labels):
        idx = order[labels[order] == c]                # this class, in visiting order
        b = boxes[idx]
        dead = np.zeros(len(idx), bool)
        for i in range(len(idx)):
            if dead[i]:
                continue
            kept.append(idx[i])
            if i + 1 < len(idx):
                dead[i + 1:] |= suppresses_row(b[i], b[i + 1:], thr, one)      # one row at a time, vectorised
    kept = np.asarray(kept, np.int64)
    return kept[np.argsort(rank[kept])] if len(kept) else kept


# --------------------------------------------------------------------------------------------------- exact arithmetic
def _frac(v):
    return Fraction(float(v))                          # a float is a dyadic rational: exact


def round_to_f32(q):
    """Fraction q >= 0 -> the nearest float32 (ties to even) as a Fraction: one correctly rounded step."""
    if q == 0:
        return Fraction(0)
    assert q > 0
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    ulp = Fraction(2) ** (max(e, -126) - 23)
    n = q / ulp
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl * ulp


def exact_suppresses(a, b, thr, one=0.0):
    """The decision `IoU(a, b) > thr` of the kernels, in exact arithmetic: intersection and union as Fractions, then
    the float32 division emulated as ONE correctly rounded step.  Raises if the intersection or the union is not
    representable in float32 -- then the float32 formula would round before the division and the builder is wrong."""
    a, b, one = [_frac(v) for v in a], [_frac(v) for v in b], _frac(one)
    area = lambda r: (r[2] - r[0] + one) * (r[3] - r[1] + one)
    w = max(Fraction(0), min(a[2], b[2]) - max(a[0], b[0]) + one)
    h = max(Fraction(0), min(a[3], b[3]) - max(a[1], b[1]) + one)
    inter = w * h
    union = area(a) + area(b) - inter
    for v in (area(a), area(b), inter, area(a) + area(b), union):
        if v >= 0 and round_to_f32(v) != v:
            raise ValueError("intermediate %s of the IoU is not a float32: the inputs are off the grid" % v)
    if union == 0:
        return False                                   # 0/0 = NaN (inter <= union): never suppresses
    return round_to_f32(inter / union) > _frac(F32(thr))


def _threshold_midpoint(thr):
    """round_to_f32(q) > t  <=>  q > mid, or q == mid and the float above t has an even mantissa (rounding is
    monotonic): mid = the midpoint of t and the next float32 above it."""
    t = F32(thr)
    assert t >= 0
    nxt = np.nextafter(t, F32(np.inf))
    mid = (_frac(t) + _frac(nxt)) / 2
    return mid, (int(nxt.view(np.uint32)) & 1) == 0


def to_units(boxes):
    """grid boxes -> int64 in units of 1/GRID; asserts the grid, the range and the side limit of the module docstring."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4) * GRID
    u = np.rint(b).astype(np.int64)
    assert np.array_equal(u, b), "coordinates off the 1/%d grid" % GRID
    assert u.min(initial=0) >= 0 and u.max(initial=0) < GRID * GRID, "coordinates outside [0, %d)" % GRID
    side = np.concatenate([u[:, 2] - u[:, 0], u[:, 3] - u[:, 1]])
    assert side.min(initial=0) >= 0 and side.max(initial=0) <= MAX_SIDE * GRID, "side above %g or negative" % MAX_SIDE
    return u


def exact_suppress_matrix(units, rows, thr):
    """exact_suppresses(one = 0) of units[rows] against all of units, vectorised in int64 (grid inputs only)."""
    u = np.asarray(units, np.int64)
    a = u[rows][:, None, :]
    area = (u[:, 2] - u[:, 0]) * (u[:, 3] - u[:, 1])
    w = np.maximum(0, np.minimum(a[..., 2], u[None, :, 2]) - np.maximum(a[..., 0], u[None, :, 0]))
    h = np.maximum(0, np.minimum(a[..., 3], u[None, :, 3]) - np.maximum(a[..., 1], u[None, :, 1]))
    inter = w * h
    union = area[rows][:, None] + area[None, :] - inter
    mid, tie_up = _threshold_midpoint(thr)
    if mid.denominator > 2 ** 30:                      # thr = 0: a non-zero IoU is >= 2^-24 here, far above mid
        assert mid < Fraction(1, 2 ** 30)
        return (inter > 0) & (union > 0)
    lhs, rhs = inter * mid.denominator, union * mid.numerator           # < 2^24 * 2^30: no overflow
    return (union > 0) & ((lhs > rhs) | ((lhs == rhs) & tie_up))


# --------------------------------------------------------------------------------------------------- box builders
def _snap(v):
    return np.rint(np.asarray(v, np.float64) * GRID) / GRID


def clusters(rng, m, spread=1.0):
    """m boxes jittered around m // 12 + 1 centres: dense overlap, IoUs all over [0, 1]."""
    k = m // 12 + 1
    ctr = rng.uniform(10, 54, (k, 2))
    size = rng.uniform(3, 10, (k, 2))
    j = rng.integers(0, k, m)
    c = ctr[j] + rng.normal(0, spread, (m, 2))
    wh = size[j] * rng.uniform(0.7, 1.3, (m, 2))
    b = np.concatenate([_snap(c - wh / 2), _snap(c + wh / 2)], 1)
    return np.clip(b, 0, GRID - 1.0 / GRID).astype(F32)


def chain(m, thr, per_row=220):
    """Stepped chains: box i + 1 is box i shifted right by d; IoU(i, i+1) > thr >= IoU(i, i+2), so in index order
    i suppresses i + 1, which then cannot suppress i + 2: the kept set alternates and the dependency chain is as long
    as the row (per_row boxes, rows two units apart and disjoint; 1.5 units apart once two would leave the grid)."""
    d = 0.25
    assert thr < 1.0
    w = None
    for k in range(1, 32 * GRID):                      # smallest width w = k / 64 with (w-d)/(w+d) > thr >= (w-2d)/(w+2d)
        cand = k / GRID
        if cand > 2 * d and (cand - d) / (cand + d) > thr + 1e-3 and (cand - 2 * d) / (cand + 2 * d) < thr - 1e-3:
            w = cand
            break
    if w is None:                                      # thr = 0: every overlapping pair suppresses; use touching steps
        w = 2 * d
    i = np.arange(m)
    step = 2.0 if ((m - 1) // per_row) * 2.0 + 1 < GRID else 1.5       # the boxes are 1 high: rows stay disjoint
    x, y = (i % per_row) * d, (i // per_row) * step
    assert x.max(initial=0) + w < GRID and y.max(initial=0) + 1 < GRID
    return np.stack([x, y, x + w, y + 1.0], 1).astype(F32)


def identical(m):
    return np.tile(np.asarray([[8.5, 9.25, 20.0, 30.75]], F32), (m, 1))


def disjoint(m):
    """m boxes in distinct cells of a 128 x 128 lattice (cell 1/2, box 3/8): no pair overlaps; neighbours do not touch.
    Above 128 * 127 boxes the lattice is 256 x 256 (cell 1/4, box 3/16)."""
    side, cell = (128, 0.5) if m <= 128 * 127 else (256, 0.25)
    assert m <= side * (side - 1)
    i = np.arange(m)
    x, y = (i % side) * cell, (i // side) * cell
    return np.stack([x, y, x + 0.75 * cell, y + 0.75 * cell], 1).astype(F32)


def exact_threshold_pairs(m, thr, rng):
    """Pairs (2j, 2j+1) with a common corner, heights equal, widths q*u and p*u: IoU = p/q exactly.  A third of the
    pairs has p/q == thr as rationals (rounds to the float32 thr: NOT suppressed, the comparison is strict), a third
    lies one step above, a third one step below.  Pairs sit in cells of their own (up to 4096 boxes)."""
    fr = {0.0: (0, 1), 0.5: (1, 2), 0.65: (13, 20), 1.0: (1, 1)}[thr]
    out = np.zeros((m, 4), np.float64)
    for j in range((m + 1) // 2):
        p, q = fr
        p, q = p * 4, q * 4
        p += (0, 1, -1)[j % 3]
        p = min(max(p, 0), q)
        u = int(rng.integers(1, max(1, int(1.4 * GRID) // q) + 1)) / GRID      # q * u <= 1.4: the pair stays in its cell
        cell = j % 2048                                # 32 x 64 cells of 2 x 1; beyond 4096 boxes the cells are reused
        cx, cy = (cell % 32) * 2.0, (cell // 32) * 1.0
        hgt = int(rng.integers(8, 49)) / GRID
        out[2 * j] = [cx, cy, cx + q * u, cy + hgt]
        if 2 * j + 1 < m:
            out[2 * j + 1] = [cx, cy, cx + p * u, cy + hgt] if p else [cx + q * u, cy, cx + q * u + 0.5, cy + hgt]
    assert out.max(initial=0) < GRID
    return out.astype(F32)


def degenerate(m, rng):
    """zero-width, zero-height and point boxes, duplicates of them (0/0), some inside / on the edge of proper boxes"""
    out = np.zeros((m, 4), np.float64)
    for i in range(m):
        x, y = float(rng.integers(0, 8)) * 2.0 + 1.0, float(rng.integers(0, 8)) * 2.0 + 1.0
        kind = i % 5
        w, h = [(0, 0), (0, 1.5), (1.5, 0), (1.5, 1.5), (0, 0)][kind]
        if kind == 4:
            x, y = x + 0.75, y + 0.75                  # a point inside the proper box of the same cell
        out[i] = [x, y, x + w, y + h]
    return out.astype(F32)


STRUCTURES = ("clusters", "chain", "identical", "disjoint", "exact", "degenerate")


def build_boxes(struct, m, thr, rng):
    if struct == "clusters":
        return clusters(rng, m)
    if struct == "chain":
        return chain(m, thr)
    if struct == "identical":
        return identical(m)
    if struct == "disjoint":
        return disjoint(m)
    if struct == "exact":
        return exact_threshold_pairs(m, thr, rng)
    if struct == "degenerate":
        return degenerate(m, rng)
    raise KeyError(struct)


# --------------------------------------------------------------------------------------------------- scores, classes, placement
TIE_TABLE = (64, 100, 128, 200, 255)                   # k / 256; 64 / 256 == CONF_THR: passes (the filter is >=)


def build_scores(kind, m, rng):
    """-> (obj [m], conf [m]) float32 with obj * conf exact and >= CONF_THR.
    distinct: a random permutation of m different values; desc: different values falling with the index;
    few: a handful of values from TIE_TABLE (half of the low ones as 0.5 * 2s); equal: all 0.5.
    Above 8192 candidates distinct / desc take their values from k / 65536, k in [16384, 65536): 16 bits, still exact."""
    obj = np.ones(m, F32)
    assert m <= 49152
    if kind == "distinct":
        conf = (4096 + rng.permutation(8192)[:m]) / 16384.0 if m <= 8192 else (16384 + rng.permutation(49152)[:m]) / 65536.0
    elif kind == "desc":
        conf = (4096 + 8191 - np.arange(m)) / 16384.0 if m <= 8192 else (65535 - np.arange(m)) / 65536.0
    elif kind == "few":
        conf = rng.choice(TIE_TABLE, m) / 256.0
        half = (conf <= 0.5) & (rng.integers(0, 2, m) == 1)
        obj[half] = 0.5
        conf = np.where(half, conf * 2, conf)
    elif kind == "equal":
        conf = np.full(m, 0.5)
    else:
        raise KeyError(kind)
    return obj, conf.astype(F32)


def build_labels(layout, m, nc, rng):
    """class of each of the m passing candidates"""
    if layout == "balanced":
        return rng.integers(0, nc, m)
    if layout.startswith("single:"):
        return np.full(m, int(layout[7:]))
    if layout.startswith("populated:"):
        pool = rng.choice(nc, int(layout[10:]), replace=False)
        lab = pool[rng.integers(0, len(pool), m)]
        k = min(m, len(pool))
        lab[:k] = pool[:k]                             # every class of the pool really occurs
        return lab
    if layout.startswith("sized:"):                    # classes 0, 1, 2, ... of exactly these sizes, the rest in the last class
        sizes = [int(s) for s in layout[6:].split(",")]
        lab = np.concatenate([np.full(s, c) for c, s in enumerate(sizes)] + [np.full(max(0, m - sum(sizes)), nc - 1)])[:m]
        return rng.permutation(lab)
    if layout == "top":                                # the highest class id and two others
        return np.asarray([nc - 1, 0, nc // 2])[rng.integers(0, 3, m)] if m > 1 else np.full(m, nc - 1)
    raise KeyError(layout)


def scatter(rng, A, m):
    """m of the A anchors, ascending, scattered over the whole range (not a prefix)"""
    assert m <= A
    return np.sort(rng.choice(A, m, replace=False))


def build_image(A, nc, m, struct="clusters", layout="balanced", scores="distinct", thr=0.5, seed=0):
    """One image: exactly m passing anchors scattered through A, candidate j at the j-th of them (so anchor order is
    candidate order); every other anchor fails the confidence filter, some of them narrowly.
    -> dict(boxes [A,4] xyxy, obj [A], conf [A], label [A], m)"""
    rng = np.random.default_rng([seed, A, nc, m])
    boxes = clusters(rng, A, spread=3.0)
    obj = np.full(A, 0.5, F32)
    conf = (rng.choice((0, 64, 125, 127), A) / 256.0).astype(F32)           # scores 0 ... 0.248: fail
    label = rng.integers(0, nc, A)
    if m:
        pos = scatter(rng, A, m)
        boxes[pos] = build_boxes(struct, m, thr, rng)
        obj[pos], conf[pos] = build_scores(scores, m, rng)
        label[pos] = build_labels(layout, m, nc, rng)
    to_units(boxes)
    return dict(boxes=boxes, obj=obj, conf=conf, label=label.astype(np.int64), m=m)


def to_pred(images, nc, box_mode):
    """images (build_image dicts, one A) -> float32 [n, A, 5 + nc] as glsdet_nms reads it: box_mode 1 = x1,y1,x2,y2;
    box_mode 0 = cx,cy,w,h (exact, see the module docstring); objectness; the class confidence in the channel of the
    label, zeros elsewhere."""
    A = len(images[0]["obj"])
    pred = np.zeros((len(images), A, 5 + nc), F32)
    for i, im in enumerate(images):
        b = im["boxes"].astype(F32)
        if box_mode == 1:
            pred[i, :, :4] = b
        else:
            pred[i, :, 0], pred[i, :, 1] = (b[:, 0] + b[:, 2]) / F32(2), (b[:, 1] + b[:, 3]) / F32(2)
            pred[i, :, 2], pred[i, :, 3] = b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]
        pred[i, :, 4] = im["obj"]
        pred[i, np.arange(A), 5 + im["label"]] = im["conf"]
    return pred


def candidates(pred_i, nc, box_mode, conf_thr=CONF_THR):
    """nms_filter_kernel restated: class max (first maximum wins), score = obj * conf in float32, score >= conf_thr.
    -> dict(boxes xyxy, scores, labels, anchors, rows [k,7] = x1,y1,x2,y2,obj,conf,label)"""
    p = np.asarray(pred_i, F32)
    conf, lab = p[:, 5:5 + nc].max(1), p[:, 5:5 + nc].argmax(1)
    score = p[:, 4] * conf
    an = np.nonzero(score >= F32(conf_thr))[0]
    if box_mode == 0:
        half_w, half_h = p[an, 2] / F32(2), p[an, 3] / F32(2)
        b = np.stack([p[an, 0] - half_w, p[an, 1] - half_h, p[an, 0] + half_w, p[an, 1] + half_h], 1)
    else:
        b = p[an, :4].copy()
    rows = np.concatenate([b, p[an, 4:5], conf[an, None], lab[an, None].astype(F32)], 1).astype(F32)
    return dict(boxes=b.astype(F32), scores=score[an], labels=lab[an], anchors=an, rows=rows)


def reference_dets(pred_i, nc, box_mode, nms_thr, conf_thr=CONF_THR):
    """-> float32 [K, 7]: what glsdet_nms must write for this image with max_det >= K, row for row."""
    c = candidates(pred_i, nc, box_mode, conf_thr)
    keep = greedy_nms(c["boxes"], c["scores"], c["labels"], c["anchors"], nms_thr)
    return c["rows"][keep]


# --------------------------------------------------------------------------------------------------- the GPU case matrix
COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 5000)
A_DEFAULT = 6000                                       # not a multiple of 64
MIXED = (0, 5000, 70, 4096, 4097, 1)                   # both kernel families write into one dets / count buffer


DENSE_COUNTS = (8192, 8193, 8400, 22050, 32767, 32768)   # every anchor a candidate: 128, 129, 132, 345, 512, 512 mask words
DENSE_A = 8400                                         # a 640 x 640 input; 22050 = the benchmark's 800 x 1344
DENSE_MIXED = (8400, 0, 4097, 70, 4096)                # one launch, max_cand = 8400: the per-image flags pick the family
NMS_MAX = 32768                                        # GLS_NMS_MAXW * 64: the kernels refuse more candidates per image


def _case(cid, ms, A=A_DEFAULT, nc=80, mode=1, thr=0.5, cap=None, **kw):
    """kw: struct / layout / scores (one value for all images), seed.  cap: max_cand = max_det of the GPU run
    (None: the 8192 of tests/test_post_fuzz.py)"""
    return dict(id=cid, ms=tuple(ms), A=A, nc=nc, mode=mode, thr=thr, cap=cap, kw=kw)


def dense_cases():
    """The regime of the reference's evaluation thresholds (confidence 0.01 / 0.0001): every anchor is a candidate, up to
    the kernels' limit of 32768.  A = m (but for one case), max_cand = max_det = A.  At 22050 and above the candidates
    are spread over 40 of 80 classes so that the CPU pair check stays at some 10^7 pairs; rank / mask / scan rank and
    scan all m rows whatever the classes.  The largest single-class cases have 8400 candidates."""
    cs = []
    for i, m in enumerate(DENSE_COUNTS):
        if m in (22050, 32768):
            continue
        cs.append(_case("dense_count%d" % m, [m], A=m, cap=m, mode=i % 2, layout="populated:40",
                        scores=("distinct", "few")[i % 2], seed=100 + i))
    for j, m in enumerate((22050, 32768)):
        cs.append(_case("dense_clusters_%d" % m, [m], A=m, cap=m, mode=j, layout="populated:40", seed=110 + j))
        cs.append(_case("dense_disjoint_%d" % m, [m], A=m, cap=m, mode=1 - j, thr=0.65, struct="disjoint", layout="populated:40",
                        scores="few", seed=112 + j))
    cs.append(_case("dense_nc256_32768", [32768], A=32768, cap=32768, nc=256, mode=0, layout="populated:40", scores="few", seed=114))
    cs.append(_case("dense_A9000_m8400", [8400], A=9000, cap=9000, mode=0, thr=0.65, layout="populated:40", seed=115))
    A = DENSE_A
    cs.append(_case("dense_chain_one_class", [A], A=A, cap=A, struct="chain", layout="single:7", scores="desc", seed=120))
    cs.append(_case("dense_identical_one_class", [A], A=A, cap=A, mode=0, struct="identical", layout="single:79", seed=121))
    cs.append(_case("dense_identical_balanced", [A], A=A, cap=A, struct="identical", scores="few", seed=122))
    cs.append(_case("dense_exact_thr0.5", [A], A=A, cap=A, mode=0, thr=0.5, struct="exact", layout="populated:3", nc=10, seed=123))
    cs.append(_case("dense_exact_thr0.65", [A], A=A, cap=A, thr=0.65, struct="exact", layout="populated:3", nc=10, seed=124))
    cs.append(_case("dense_ties_all_equal", [A], A=A, cap=A, scores="equal", nc=4, seed=125))
    cs.append(_case("dense_ties_few", [A], A=A, cap=A, mode=0, scores="few", nc=4, seed=126))
    cs.append(_case("dense_ties_equal_chain", [A], A=A, cap=A, struct="chain", layout="single:0", scores="equal", nc=4, seed=127))
    cs.append(_case("dense_mixed", DENSE_MIXED, A=A, cap=A, scores="few", nc=10, seed=128))
    cs.append(_case("dense_mixed_distinct_mode0", DENSE_MIXED, A=A, cap=A, mode=0, thr=0.65, seed=129))
    return cs


def nms_cases():
    cs = []
    # candidate counts over the sort's and the blocks' boundaries; ties in the odd ones, both box modes
    for i, m in enumerate(COUNTS):
        cs.append(_case("count%d" % m, [m], scores=("distinct", "few")[i % 2], mode=i % 2, nc=10, seed=i))
    cs.append(_case("mixed", MIXED, scores="few", nc=10, seed=20))
    cs.append(_case("mixed_distinct_mode0", MIXED, mode=0, thr=0.65, seed=21))
    # class layouts x counts
    for m in (65, 1024, 2049, 4096, 5000):
        cs.append(_case("nc1_%d" % m, [m], nc=1, layout="single:0", seed=30))
        cs.append(_case("nc80_balanced_%d" % m, [m], scores="few", seed=31))
        cs.append(_case("nc80_class37_%d" % m, [m], layout="single:37", seed=32))
        cs.append(_case("nc80_populated20_%d" % m, [m], layout="populated:20", scores="few", seed=33))
        cs.append(_case("nc255_top_%d" % m, [m], nc=255, layout="top", scores="few", seed=34))
        cs.append(_case("nc256_oldpath_%d" % m, [m], nc=256, layout="top", scores="few", seed=35))
    cs.append(_case("sized_63_64_65", [192], nc=3, layout="sized:63,64,65", scores="few", seed=36))
    cs.append(_case("sized_63_64_65_rest", [1500], nc=20, layout="sized:63,64,65", seed=37))
    cs.append(_case("sized_oldpath", [4500], nc=20, layout="sized:63,64,65,1,127,128,129", scores="few", seed=38))
    # suppression structures x thresholds, on both paths (m <= 4096: class-segmented; above: rank / mask / scan)
    for thr in (0.0, 0.5, 0.65, 1.0):
        for struct in STRUCTURES:
            if struct == "chain" and thr == 1.0:
                continue                               # nothing suppresses at 1.0: identical covers it
            sc = "desc" if struct == "chain" else "distinct"
            tag = "%s_thr%g" % (struct, thr)
            cs.append(_case(tag + "_seg", [700], thr=thr, struct=struct, layout="single:3", scores=sc, nc=10, seed=40))
            cs.append(_case(tag + "_old", [4200], thr=thr, struct=struct, layout="populated:3", scores=sc, nc=10, seed=41))
    cs.append(_case("chain_one_class_4096", [4096], struct="chain", layout="single:7", scores="desc", seed=42))
    cs.append(_case("chain_equal_scores_seg", [900], struct="chain", layout="single:0", scores="equal", nc=4, seed=43))
    cs.append(_case("chain_equal_scores_old", [4300], struct="chain", layout="single:0", scores="equal", nc=4, seed=44))
    # ties
    for m in (300, 3000, 4100):
        cs.append(_case("ties_few_%d" % m, [m], scores="few", nc=4, seed=50))
        cs.append(_case("ties_all_equal_%d" % m, [m], scores="equal", nc=4, seed=51))
        cs.append(_case("ties_all_equal_disjoint_%d" % m, [m], scores="equal", struct="disjoint", seed=52))
        cs.append(_case("ties_across_classes_%d" % m, [m], scores="few", struct="disjoint", layout="populated:40", seed=53))
    # filter geometry: waves that span images, n * A not a multiple of 64, a large odd A
    cs.append(_case("A100_n5", [100, 0, 37, 64, 99], A=100, nc=3, scores="few", seed=60))
    cs.append(_case("A8191", [5000], A=8191, nc=10, mode=0, seed=61))
    cs.append(_case("A8191_full", [8191], A=8191, nc=10, struct="disjoint", scores="few", seed=62))
    cs.append(_case("A33_n3", [33, 1, 20], A=33, nc=2, seed=63))
    cs += dense_cases()
    ids = [c["id"] for c in cs]
    assert len(set(ids)) == len(ids)
    return cs


def build_case(case):
    """-> (pred float32 [n, A, 5 + nc], images)"""
    kw = dict(case["kw"])
    seed = kw.pop("seed", 0)
    images = [build_image(case["A"], case["nc"], m, thr=case["thr"], seed=seed * 100 + i, **kw) for i, m in enumerate(case["ms"])]
    return to_pred(images, case["nc"], case["mode"]), images
