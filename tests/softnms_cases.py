"""Inputs shared by tests/test_softnms_reference.py (CPU: the margin condition) and tests/test_softnms_fuzz.py (GPU).

`random_rows` gives clustered boxes (most rows overlap something) with free fp32 scores; `dyadic_rows` gives corners on a
grid of 1/4 inside [0, 64) and scores on a grid of 1/64, for the methods whose arithmetic must come out bit for bit.

GAUSSIAN_CASES are fixed seeds.  The gaussian weight is an fp64 `exp` on either side, so decayed scores may differ in
the last fp32 bits; keep sets and orders may be compared only when no decision sits that close, which
test_gaussian_fuzz_seeds_meet_the_margin_condition asserts for every seed below.  A seed that fails it is replaced here,
never filtered at run time."""
import numpy as np


def random_rows(seed, n, nc, integer=False):
    """-> fp32 [n, 6] x1, y1, x2, y2, score, label"""
    rng = np.random.default_rng(seed)
    ctr = rng.uniform(0, 40 + 2 * n ** 0.5, (n, 2))
    half = rng.uniform(2, 14, (n, 2))
    boxes = np.concatenate([ctr - half, ctr + half], 1)
    boxes = np.round(boxes) if integer else boxes
    scores = rng.uniform(0.02, 1.0, n)
    labels = rng.integers(0, nc, n)
    return np.concatenate([boxes, scores[:, None], labels[:, None]], 1).astype(np.float32)


def dyadic_rows(seed, n, nc, span=64, score_grid=64, distinct=False):
    """corners multiples of 1/4, widths and heights 1 .. 16; scores k / score_grid (ties on purpose), or with `distinct`
    a permutation of (1 .. n) / 2^ceil(log2(n + 1)): no two equal"""
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 4 * span, (n, 2)) / 4.0
    wh = rng.integers(4, 65, (n, 2)) / 4.0
    boxes = np.concatenate([lo, lo + wh], 1)
    if distinct:
        scores = (1 + rng.permutation(n)) / float(1 << int(np.ceil(np.log2(n + 1))))
    else:
        scores = rng.integers(1, score_grid + 1, n) / float(score_grid)
    labels = rng.integers(0, nc, n)
    return np.concatenate([boxes, scores[:, None], labels[:, None]], 1).astype(np.float32)


# seed, rows per image, classes, integer-valued boxes, Nt (unused by the gaussian decay), sigma, thresh
GAUSSIAN_CASES = [
    dict(seed=1, counts=[64], nc=1, integer=False, nt=0.3, sigma=0.5, thresh=1e-4),
    dict(seed=2, counts=[64, 0, 37], nc=3, integer=False, nt=0.3, sigma=0.5, thresh=1e-4),
    dict(seed=3, counts=[63, 64], nc=2, integer=True, nt=0.3, sigma=0.5, thresh=1e-4),
    dict(seed=4, counts=[48], nc=10, integer=False, nt=0.3, sigma=0.25, thresh=0.05),
    dict(seed=5, counts=[33, 17, 1], nc=1, integer=True, nt=0.3, sigma=0.5, thresh=1e-4),
    dict(seed=6, counts=[64], nc=1, integer=False, nt=0.3, sigma=0.1, thresh=0.01),
    dict(seed=7, counts=[60, 59], nc=5, integer=False, nt=0.3, sigma=2.0, thresh=1e-4),
]


def gaussian_rows(case):
    return [random_rows(1000 * case["seed"] + b, n, case["nc"], case["integer"]) for b, n in enumerate(case["counts"])]
