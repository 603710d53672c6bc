"""Case lists of the matrix-core non-local kernels (glsdet_amd/csrc/nonlocal_mfma.hip, glsdet_nonlocal_mfma), built with the
constructors of tests/nonlocal_reference.py and held to its exact regime and its a-priori bound.

What the kernels branch on, and where it occurs below:
  * ci, cx in tiles of 64 with 32-wide wave tiles: 32 (one wave tile), 64 (one tile), 96 (a tile and a half), 160 (past 128,
    no power of two), 512 (the width of YOLOX-s dark5), ci != cx (64, 96);
  * pixels in stages of 32 (fp32 Gram) / 64 (fp16 Gram, apply): N = 1, 4 and 6 in one launch (the quadrants of a 4 x 5
    map), 63, 64, 65, 252 and 273 in one launch (one Gram slice next to four), 1025 and 2048 (eight slices);
  * n in {1, 3}; one to four sets; the four unequal quadrants of a 5 x 7 map; in place and to a separate destination;
  * dense maps and windows of a larger map with a channel offset of 32 ('window32').

The exact regime and the order of the sums.  nonlocal_reference.check_regime bounds, per accumulation, the sum of the
MAGNITUDES of the terms (|phi|^T |g| for the Gram, |tw| (|phi|^T |g|)^T for the fold, |M| |theta| for the apply), each
below 2^24 steps, so every partial sum of every order is an exactly representable integer number of steps: the MFMA's
k-ordered chains are as exact as the scalar loops.  `magnitude_sums` states that once more, independently, and the CPU
test asserts it per case.

The 1 / N step is the one place where the regime depends on N: fl32(fl32(N m) fl32(1 / N)) = m fails for N = 63 and 252
from m = 3 on.  The data of those windows is tightened HERE (the reference stays as it is, see `data`): g lives on a
handful of pixels -- the first, the last and both sides of every stage boundary (32, 64, 128, 192) -- in one channel each,
and phi is thinned at those pixels so that |m| <= 2 and nonlocal_reference.good_window(N, 2) holds.  The tightening happens
once, at import of this module, in the reference's per-name cache, so `expected`, `check_regime` and the GPU test all see
the same operands whatever the order of the tests."""
import numpy as np

from tests import nonlocal_reference as R

TIGHT_N = (63, 252)                                              # windows whose 1 / N step is exact for |m| <= 2 only


def layout(kind, h, w, c):
    """(H, W, Ct, h0, w0, c0) of a view in a buffer of its own; every offset and stride a multiple of 16 bytes"""
    if kind == "dense":
        return h, w, c, 0, 0, 0
    assert kind == "window32"
    return h + 3, w + 2, c + 64, 2, 1, 32


EXACT_CASES = [
    #          name                       ci   cx   h   w  n  x / out place  tpg place   out (None: in place)
    R._static("mfma-ci32-c32-1x1",        32,  32,  1,  1, 3, "dense",    "dense",    None),
    R._multi("mfma-quadrants-4x5-ci64",   64,  64,  4,  5, R.quadrants(4, 5), 3, "window32", "window32", None),
    R._static("mfma-ci96-c96-7x9",        96,  96,  7,  9, 1, "dense",    "window32", "dense"),
    R._static("mfma-ci160-c160-8x8",     160, 160,  8,  8, 1, "window32", "dense",    None),
    R._static("mfma-ci512-c512-5x13",    512, 512,  5, 13, 1, "dense",    "dense",    "window32"),
    R._multi("mfma-252+273-ci64-c96",     64,  96, 25, 21, [(0, 12, 0, 21), (12, 25, 0, 21)], 1, "window32", "dense", "dense"),
    R._static("mfma-ci64-c96-25x41",      64,  96, 25, 41, 1, "dense",    "dense",    None),
    R._static("mfma-ci32-c32-32x64",      32,  32, 32, 64, 3, "dense",    "window32", None),
    R._multi("mfma-quadrants-5x7-ci96",   96,  96,  5,  7, R.quadrants(5, 7), 1, "dense", "window32", "window32"),
    R._multi("mfma-three-ci160",         160, 160, 10, 12, [(0, 4, 0, 5), (0, 8, 8, 12), (4, 10, 0, 8)], 1, "window32", "dense", None),
]
GENERIC_CASES = [EXACT_CASES[1], EXACT_CASES[5], EXACT_CASES[7], EXACT_CASES[8],
                 R._static("mfma-generic-ci1280-2x2", 1280, 1280, 2, 2, 1, "dense", "dense", None),
                 R._static("mfma-generic-ci512-13x21", 512, 512, 13, 21, 1, "window32", "dense", "dense")]
FALLBACK_CASE = R._static("mfma-fallback-ci40-c40-5x13", 40, 40, 5, 13, 1, "dense", "dense", None)


_TIGHTENED = set()


def sizes(case):
    return [(w[1] - w[0]) * (w[3] - w[2]) for w in R.windows(case)]


def tight_support(N):
    """the pixels of a TIGHT_N window that carry g: the first and the last pixel, and both sides of every stage boundary
    of the kernels (32: the fp32 Gram's stage, 64: the fp16 Gram's and the apply's tile) that the window has"""
    return sorted({0, N - 1} | {p for edge in (32, 64, 128, 192) for p in (edge - 1, edge) if edge < N})


def data(case):
    """nonlocal_reference.case_data of the case, with the operands of the TIGHT_N windows confined so that |m| <= 2 (see
    the module docstring): g is non-zero on the pixels of tight_support(N) only, in ONE channel per pixel (a different one
    each), and at those pixels a phi channel c1 is non-zero at two of them at most (c1 mod k and c1 + 1 mod k of the k
    support pixels); then M[co][c1] = sum_j phi[c1, j] tw[co, c2(j)] g[c2(j), j] has at most two terms of magnitude one.
    phi stays random at every other pixel, where g is zero.  Modified in place in the reference's per-name cache, once;
    the module runs this for every exact case at import, before anything can have asked for `expected`."""
    d = R.case_data(case)
    if case.name in _TIGHTENED:
        return d
    assert case.name not in R._EXPECT, "expected() of %s was computed before its data was tightened" % case.name
    _TIGHTENED.add(case.name)
    rng = np.random.RandomState(case.seed + 1)
    n, ci = case.n, case.ci
    for q, (h0, h1, w0, w1) in enumerate(R.windows(case)):
        i = d["ints"][q]
        N = i["N"]
        if N not in TIGHT_N:
            continue
        sup = tight_support(N)
        k = len(sup)
        assert k <= ci
        tg = np.zeros_like(i["tg"])
        ch = rng.choice(ci, k, replace=False)
        c1 = np.arange(ci)
        for s_, (j, c2) in enumerate(zip(sup, ch)):
            tg[:, c2, j] = rng.choice([-1, 1], n)
            mine = (c1 % k == s_) | ((c1 + 1) % k == s_)
            i["phi"][:, :, j] = np.where(mine[None, :], rng.choice([-1, 1], (n, ci)), 0)
        i["tg"] = tg
        t = d["tpg"][0]
        t[:, ci:2 * ci, h0:h1, w0:w1] = i["phi"].reshape(n, ci, h1 - h0, w1 - w0)
        t[:, 2 * ci:3 * ci, h0:h1, w0:w1] = (tg * N).reshape(n, ci, h1 - h0, w1 - w0)
    return d


def mmax(case, q):
    i = data(case)["ints"][q]
    return max(int(np.abs(i["tw"] @ (i["phi"][b] @ i["tg"][b].T).T).max()) for b in range(case.n))


def magnitude_sums(case):
    """per set the largest sum of |term| of the three accumulations, in units of the accumulation's step: any order of the
    additions is exact while they stay below 2^24"""
    out = []
    d = data(case)
    for q in range(len(R.windows(case))):
        i = d["ints"][q]
        N = i["N"]
        a = lambda v: np.abs(v).astype(np.int64)
        gram = fold = apply_ = 0
        for b in range(case.n):
            G = a(i["phi"][b]) @ a(i["tg"][b]).T
            gram = max(gram, N * int(G.max()))
            fold = max(fold, N * int((a(i["tw"]) @ G.T).max()))
            M = i["tw"] @ (i["phi"][b] @ i["tg"][b].T).T
            apply_ = max(apply_, int((a(M) @ a(i["theta"][b])).max()))
        out.append({"gram": gram, "fold": fold, "apply": apply_})
    return out


def assert_coverage():
    ex = EXACT_CASES
    assert {c.ci for c in ex if c.ci == c.cx} == {32, 64, 96, 160, 512} and any((c.ci, c.cx) == (64, 96) for c in ex)
    ns = [sizes(c) for c in ex]
    flat = {v for s in ns for v in s}
    assert flat >= {1, 4, 6, 63, 64, 65, 252, 273, 1025, 2048}
    assert any(set(s) >= {4, 6} for s in ns) and any(set(s) >= {252, 273} for s in ns)
    assert {c.n for c in ex} == {1, 3} and {len(s) for s in ns} == {1, 2, 3, 4}
    assert any(list(c.wins) == R.quadrants(5, 7) for c in ex) and len(set(sizes(ex[8]))) == 4
    assert {c.okind is None for c in ex} == {True, False}
    assert {c.xkind for c in ex} == {c.tkind for c in ex} == {"dense", "window32"}
    assert {R.static_slices(v)[0] for v in flat} == {1, 4, 8}
    for c in ex + GENERIC_CASES:
        assert c.ci % 32 == 0 and c.cx % 32 == 0 and c.ci <= 1280 and c.cx <= 1280 and c.tw == 3 * c.ci
    assert any(c.ci == 1280 and sizes(c) == [4] for c in GENERIC_CASES) and any(c.ci == 512 and sizes(c) == [273] for c in GENERIC_CASES)
    assert FALLBACK_CASE.ci % 32 != 0


assert_coverage()
for _c in EXACT_CASES:                                            # the order is explicit: tighten before anyone can read
    data(_c)
