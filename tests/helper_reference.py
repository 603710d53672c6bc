"""Plain references of the 16-byte-per-lane helpers (glsdet_amd/csrc/misc.hip, resdet.hip): pools, image packing, nearest
resampling, strided copies / transposes, GroupNorm and the MPHead proxy scores -- and the case lists that
tests/test_helper_fuzz.py (GPU) and tests/test_helper_reference.py (CPU) share.

Plain numpy, float64 wherever arithmetic is involved; nothing of the engine is imported.  Activations are NCHW.

Contracts the references state (DESIGN.md section 4 repeats them):

  pools      inputs are finite or +-inf.  The kernels keep the larger of two values with `v > m ? v : m`, which DROPS a
             NaN where torch propagates it; NaN inside a pooled window is outside the contract and is not tested.
             Outside the image a window sees -inf (never zero).
  nearest    the source index is torch's float32 formula min((int)floorf(dst * ((float)in / out)), in - 1), NOT the exact
             integer dst * in // out: the two differ on 11 (in, out) pairs with in <= 40, out <= 80 (FLOAT_NE_INT below
             lists the four the cases use).
  GroupNorm  two passes in float64 over the values as stored; the comparison bound is derived in `groupnorm_ref`.
  rounding   every result is the float64 value rounded ONCE to the storage type (`round_to`).
"""
from collections import namedtuple

import numpy as np

FT = {"f16": np.float16, "f32": np.float32}
VN = {"f16": 8, "f32": 4}                                  # elements of one 16-byte vector
NINF = -np.inf
F16_MAX = 65504.0

# ---- the launch rules the kernels publish (misc.hip grid_for / resdet.hip rgrid, groupnorm_sets, copy / transpose chunks)
GRID_CAP_BLOCKS, BLOCK = 256 * 32, 256
GRID_CAP = GRID_CAP_BLOCKS * BLOCK                         # 2^21 threads: more work items than this take the grid-stride loop
GN_SPLIT_CAP, GN_GB_CAP, GN_SETS = 64, 1024, 16
COPY_JOBS = 32                                             # pairs per launch of copy_many / transpose_many
TRANSPOSE_TILE = 64


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7fffffff for k in key])


def round_to(v, dt):
    """float64 -> the storage type, ONE round-to-nearest-even (numpy converts double -> half directly), as float64"""
    with np.errstate(over="ignore"):
        return np.asarray(v, np.float64).astype(FT[dt]).astype(np.float64)


def stored(v, dt):
    """round_to that also asserts nothing overflowed"""
    r = round_to(v, dt)
    assert np.array_equal(np.isinf(r), np.isinf(np.asarray(v, np.float64)))
    return r


def ceil_to(v, m):
    return (v + m - 1) // m * m


# ================================================================================================================ pools
def pool2d_ref(x, k, s, p, fill=NINF):
    """nn.MaxPool2d(k, s, p), floor mode, by an explicit loop over the k x k window; `fill` (-inf) outside the image.
    Inputs finite or +-inf: see the module docstring for NaN."""
    x = np.asarray(x, np.float64)
    assert not np.isnan(x).any(), "NaN inside a pooled window is outside the contract"
    n, c, h, w = x.shape
    ho, wo = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    assert ho >= 1 and wo >= 1 and 2 * p <= k
    xp = np.full((n, c, h + 2 * p, w + 2 * p), fill, np.float64)
    xp[:, :, p:p + h, p:p + w] = x
    out = np.full((n, c, ho, wo), NINF, np.float64)
    for dy in range(k):
        for dx in range(k):
            out = np.maximum(out, xp[:, :, dy:dy + (ho - 1) * s + 1:s, dx:dx + (wo - 1) * s + 1:s])
    return out


def maxpool_ref(x, k, fill=NINF):
    """stride-1 'same' max pool, k odd"""
    assert k % 2 == 1
    return pool2d_ref(x, k, 1, k // 2, fill)


def spp_ref(x):
    """the pools of SPPBottleneck: three INDEPENDENT direct pools (the kernel chains pool5; the reference must not)"""
    return maxpool_ref(x, 5), maxpool_ref(x, 9), maxpool_ref(x, 13)


def pool_data(shape, dt, *key):
    """strictly negative values with some -inf and -65504 entries (zero padding, or the +65504 poison around the view,
    would win every window it enters), exact in `dt`"""
    r = _rng(11, *key)
    v = -np.exp(r.uniform(np.log(0.01), np.log(100.0), size=shape))
    sel = r.random(shape)
    v[sel < 0.06] = NINF
    v[(sel >= 0.06) & (sel < 0.12)] = -F16_MAX
    v = round_to(v, dt)
    assert (v < 0).all()
    return v


MAXPOOL_KS = [1, 3, 5, 13, 31]
MAXPOOL_MAPS = [(1, 1), (2, 3), (7, 5), (20, 24)]
POOL_CS = [8, 24]
SPP_HS, SPP_WS = [1, 7, 8, 9, 13], [1, 15, 16, 17, 29]     # tile 8 x 16, halo 6
POOL2D_KSP = [(3, 2, 1), (2, 2, 0), (1, 2, 0), (3, 1, 1), (3, 3, 0), (5, 2, 2), (2, 1, 1), (7, 4, 3)]


def pool2d_extents(k, p):
    """1 (where the output is non-empty), k, k + 1, 20, 25"""
    return [e for e in (1, k, k + 1, 20, 25) if e + 2 * p - k >= 0]


# ============================================================================================================== packing
def focus_ref(img, cy, dt):
    """Focus space-to-depth: cat(TL, BL, TR, BR) on channels, zero fill up to cy, one rounding.  img [n, cin, H, W]"""
    img = np.asarray(img, np.float64)
    n, cin, H, W = img.shape
    assert H % 2 == 0 and W % 2 == 0 and cy >= 4 * cin
    out = np.zeros((n, cy, H // 2, W // 2), np.float64)
    parts = (img[..., ::2, ::2], img[..., 1::2, ::2], img[..., ::2, 1::2], img[..., 1::2, 1::2])       # TL, BL, TR, BR
    for i, q in enumerate(parts):
        out[:, i * cin:(i + 1) * cin] = q
    return stored(out, dt)


def nchw_pack_ref(img, cy, dt):
    """fp32 NCHW image -> cy channels, zero fill above cin, one rounding"""
    img = np.asarray(img, np.float64)
    n, cin, H, W = img.shape
    assert cy >= cin
    out = np.zeros((n, cy, H, W), np.float64)
    out[:, :cin] = img
    return stored(out, dt)


def image_data(shape, *key):
    """fp32 picture with full mantissas (the conversion to fp16 is a real rounding), |v| < 64"""
    return _rng(12, *key).uniform(-64, 64, size=shape).astype(np.float32)


FOCUS_CASES = [            # (cin, channels of the destination view, destination kind)
    (1, 8, "window"), (2, 16, "window"), (4, 16, "window"), (5, 24, "window"),
    (3, 24, "window"),     # the general path with zero fill in channels 12..23
    (3, 16, "slice48"),    # the fast path on a strided view: a 16-channel slice of a 48-channel buffer
]
FOCUS_HW = [2, 6, 34]
NCHW_CINS = [1, 3, 8, 9, 17]


def focus_is_fast_path(cin, cy):
    return cin == 3 and cy == 16


# =================================================================================================== nearest resampling
def nearest_index(n_in, n_out):
    """torch 'nearest' with size=, evaluated in float32 as the kernel and torch do"""
    scale = np.float32(n_in) / np.float32(n_out)
    idx = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
    return np.minimum(idx, n_in - 1)


def nearest_index_exact(n_in, n_out):
    """the integer formula a tidy-up might substitute (a MUTANT: it differs on the FLOAT_NE_INT pairs)"""
    return np.minimum(np.arange(n_out, dtype=np.int64) * n_in // n_out, n_in - 1)


def upsample_add_ref(fine, coarse, dt, index=nearest_index):
    """fine + nearest(coarse -> fine's size): the float64 sum rounded once.  In fp16 storage the kernel adds in fp32:
    asserted exact here (the data keeps every magnitude in [2^-6, 2^4]), so one rounding is the whole story."""
    fine, coarse = np.asarray(fine, np.float64), np.asarray(coarse, np.float64)
    hi, wi = index(coarse.shape[2], fine.shape[2]), index(coarse.shape[3], fine.shape[3])
    s = fine + coarse[:, :, hi][:, :, :, wi]
    if dt == "f16":
        assert np.array_equal(s.astype(np.float32).astype(np.float64), s), "the fp32 sum of two fp16 values must be exact"
    return stored(s, dt)


def resample_ref(x, f):
    return np.repeat(np.repeat(np.asarray(x), f, axis=2), f, axis=3)


def updown_data(shape, dt, *key):
    """+-magnitudes in [2^-6, 2^4), exact in `dt`"""
    r = _rng(13, *key)
    v = np.exp2(r.uniform(-6, 4, size=shape)) * r.choice([-1.0, 1.0], size=shape)
    v = round_to(v, dt)
    v = np.clip(np.abs(v), 2.0 ** -6, 2.0 ** 4) * np.sign(v)
    return v


UPSAMPLE_PAIRS = [(14, 46), (21, 69), (26, 44), (39, 33), (13, 25), (7, 13), (1, 5), (9, 9)]       # (in, out)
FLOAT_NE_INT = [(14, 46), (21, 69), (26, 44), (39, 33)]
# h takes pair i, w takes pair i + 3 and i + 5: every pair is used on both axes
UPSAMPLE_CASES = [(UPSAMPLE_PAIRS[i], UPSAMPLE_PAIRS[(i + d) % 8]) for i in range(8) for d in (3, 5)]
RESAMPLE_FACTORS = list(range(1, 9))
RESAMPLE_MAPS = [(3, 5), (9, 11)]


# ======================================================================================================= copies
def copy_ref(x):
    return np.asarray(x).copy()


def transpose_ref(x):
    """[1, C, h, w] -> matrix [C, h * w]: row = channel, column = pixel"""
    x = np.asarray(x)
    assert x.shape[0] == 1
    return x[0].reshape(x.shape[1], -1).copy()


def transpose_dest_ref(x, rows, cols, vn, before, drop_partial_tile=False):
    """the whole destination matrix [rows, cols] after the call: [c < C, p < N] = x, columns [N, ceil_vec(N)) zero, every
    later column and every row >= C as `before`.  drop_partial_tile: the MUTANT that forgets the columns of the last,
    partial 64-pixel tile."""
    m = transpose_ref(x)
    C, N = m.shape
    assert rows >= C and cols >= ceil_to(N, vn)
    out = np.array(before, np.float64).reshape(rows, cols).copy()
    out[:C, :ceil_to(N, vn)] = 0.0
    out[:C, :N] = m
    if drop_partial_tile and N % TRANSPOSE_TILE:
        n0 = N // TRANSPOSE_TILE * TRANSPOSE_TILE
        out[:C, n0:ceil_to(N, vn)] = np.array(before, np.float64).reshape(rows, cols)[:C, n0:ceil_to(N, vn)]
    return out


COPY_COUNTS = [32, 33, 64, 65]
TRANSPOSE_COUNTS = [32, 33]
TRANSPOSE_MAPS = [(1, 1), (7, 9), (8, 8), (5, 13), (10, 13)]         # 1, 63, 64, 65, 130 pixels
TRANSPOSE_CS = [8, 64, 72, 136]


def plain_data(shape, dt, *key):
    return round_to(_rng(14, *key).normal(size=shape) * 3.0, dt)


# ============================================================================================================ GroupNorm
def gn_legal(C, groups, dt):
    """the shapes glsdet_groupnorm takes: whole vectors per group, C / vn a divisor of 256"""
    vn = VN[dt]
    return C % groups == 0 and (C // groups) % vn == 0 and C // vn <= 256 and 256 % (C // vn) == 0


def gn_plan(N, C, dt):
    """the launch rule of resdet.hip groupnorm_sets for a set of N pixels -> dict(rows, nsplit, chunk, gb)"""
    rows = 256 // (C // VN[dt])
    nsplit = min(GN_SPLIT_CAP, (N + 255) // 256)
    return dict(rows=rows, nsplit=nsplit, chunk=(N + nsplit - 1) // nsplit, gb=min(GN_GB_CAP, (N + rows * 8 - 1) // (rows * 8)),
                gb_uncapped=(N + rows * 8 - 1) // (rows * 8))


def gn_smallest_gb_capped(C, dt):
    """the smallest (h, w) whose apply grid exceeds the cap of 1024 workgroups: N > 1024 * rows * 8 pixels"""
    rows = 256 // (C // VN[dt])
    n_min = GN_GB_CAP * rows * 8 + 1
    h = 3
    return h, (n_min + h - 1) // h


def _gn_stats(x, groups, mutate=None, dt=None):
    """-> (mean, var) float64 [n, groups].  Two passes.  mutate names a plausible kernel mistake (the MUTANTS of
    tests/test_helper_reference.py), applied to the pixel slices / vector columns of gn_plan."""
    n, C, h, w = x.shape
    N, cpg = h * w, C // groups
    if mutate not in ("drop_last_pixel", "double_pixel", "shift_group"):
        per = x.reshape(n, groups, cpg * N)
        mean = per.mean(2)
        return mean, ((per - mean[:, :, None]) ** 2).mean(2)
    xg = x.reshape(n, C, N)
    weight = np.ones((C, N), np.float64)                   # how often the statistics count each element
    if mutate in ("drop_last_pixel", "double_pixel"):
        pl = gn_plan(N, C, dt)
        for z in range(pl["nsplit"]):
            pend = min(N, (z + 1) * pl["chunk"])
            if pend > z * pl["chunk"]:
                weight[:, pend - 1] = 0.0 if mutate == "drop_last_pixel" else 2.0
    chan_group = np.arange(C) // cpg
    if mutate == "shift_group":                            # every group boundary one vector to the right
        chan_group = np.clip((np.arange(C) - VN[dt]), 0, C - 1) // cpg
    mean, var = np.zeros((n, groups)), np.zeros((n, groups))
    for g in range(groups):
        sel = chan_group == g
        wg = weight[sel]
        cnt = wg.sum()
        with np.errstate(invalid="ignore", divide="ignore"):           # (a shifted boundary may leave the last group empty)
            mean[:, g] = (xg[:, sel] * wg).sum((1, 2)) / cnt
            var[:, g] = (((xg[:, sel] - mean[:, g, None, None]) ** 2) * wg).sum((1, 2)) / cnt
    return mean, var


def groupnorm_ref(x, groups, gamma, beta, eps, act, dt=None, mutate=None):
    """nn.GroupNorm(groups, C) (+ ReLU) in float64, two passes, on the inputs as stored.  -> (y, B).

    B = 2^-21 * (|x * sc| + |sh|) elementwise, sc = gamma * rstd, sh = beta - mean * sc of THIS float64 reference, bounds
    |kernel - y| before the kernel's final conversion to the storage type.  Derivation: the statistics are fp64 (their
    error is far below fp32 resolution); the apply phase rounds to fp32 rstd, mean, gamma * rstd, mean * sc and
    beta - ..., then makes one or two roundings of x * sc + sh (fused or not; fp32 storage adds none, the result IS that
    fp32 value).  Every rounding is 2^-24 relative, and at most four of them touch either term: 4 * 2^-24 = 2^-22 of
    |x * sc| + |sh|.  The factor 2 allows for the float64 reference and the kernel rounding from slightly different
    exact values (eps as float32, the order of the fp64 sums).  Nothing in B is taken from the kernel under test.  For fp16
    storage the caller adds half an ulp of the fp16 result.

    The derivation counts roundings relative to |sh|, so it holds only if sh = beta - mean * sc is rounded ONCE from fp64
    operands: an fp32 mean, rstd or gamma * rstd each leaves 2^-24 |mean * sc| in sh, which exceeds B wherever beta and
    mean * sc cancel and x * sc is small too (1.44 B on c1024_g256_3x5, fp32, measured).  The kernel therefore forms sc and
    sh in fp64 and rounds each once; its error is then at most 2^-24 (|x * sc| + |sh| + |y|) <= 2^-23 (...), a quarter of B.

    eps is used as the float32 value the C ABI receives.  act: "none" | "relu".  (dt / mutate: see _gn_stats.)"""
    x = np.asarray(x, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    n, C, h, w = x.shape
    cpg = C // groups
    mean, var = _gn_stats(x, groups, mutate, dt)
    rstd = 1.0 / np.sqrt(var + float(np.float32(eps)))
    gi = np.arange(C) // cpg
    sc = gamma[None, :] * rstd[:, gi]                                     # [n, C]
    sh = beta[None, :] - mean[:, gi] * sc
    t1, t2 = x * sc[:, :, None, None], np.broadcast_to(sh[:, :, None, None], x.shape)
    y = t1 + t2
    if act == "relu" and mutate != "no_relu":
        y = np.maximum(y, 0.0)
    else:
        assert act in ("none", "relu")
    return y, 2.0 ** -21 * (np.abs(t1) + np.abs(t2))


def half_ulp_f16(want, slack):
    """half an ulp of the fp16 result, taken at |want| + slack (a result that far from `want` may lie in the next binade)"""
    a = np.minimum(np.abs(want) + slack, F16_MAX).astype(np.float16)
    return 0.5 * np.spacing(a).astype(np.float64)


GnCase = namedtuple("GnCase", "name n C groups h w")


def _gn(n, C, g, h, w):
    return GnCase("c%d_g%d_%dx%d" % (C, g, h, w), n, C, g, h, w)


GN_NSPLIT_CASE = _gn(1, 64, 8, 129, 128)                   # more than 16384 pixels: the slice count is capped at 64
GN_BASE_CASES = [_gn(2, 8, 1, 1, 1), _gn(2, 64, 8, 33, 17), _gn(2, 256, 32, 1, 2), _gn(2, 2048, 256, 3, 5), _gn(2, 64, 1, 20, 24),
                 _gn(2, 1024, 256, 3, 5), _gn(2, 64, 16, 7, 11), GN_NSPLIT_CASE]
GN_GB_C = {"f16": 2048, "f32": 1024}                       # C / vn == 256: one pixel row per workgroup, the smallest capped map


def gn_cases(dt):
    """every base case this dtype takes + the case whose apply grid exceeds 1024 workgroups"""
    C = GN_GB_C[dt]
    h, w = gn_smallest_gb_capped(C, dt)
    gb = GnCase("gbcap_c%d_%dx%d" % (C, h, w), 1, C, 256, h, w)
    return [c for c in GN_BASE_CASES if gn_legal(c.C, c.groups, dt)] + [gb]


# unequal extents from 1 x 1 to 129 x 128 (sets 3 and 13 are the largest and the smallest neighbours)
GN_MULTI_EXTENTS = [(7, 11), (1, 2), (33, 17), (129, 128), (3, 5), (20, 24), (1, 1), (16, 16), (2, 129), (9, 9), (64, 5), (5, 64),
                    (17, 15), (1, 1), (31, 8), (12, 21), (6, 43)]
GN_MULTI_C, GN_MULTI_GROUPS = 64, 8


def gn_exact_data(case, dt, act, *key):
    """The exact regime: every (image, group) holds the two values m_g +- a_g in equal numbers at shuffled positions
    (m_g a multiple of 1/4 with |m_g| <= 2, a_g a power of two in 1/4 .. 2), gamma in quarters, beta in eighths, eps = 0.
    Then sum = cnt * m_g and sum of squares = cnt * (m_g^2 + a_g^2) are exact in fp64 (and in fp32 per vector), mean = m_g,
    var = a_g^2, rstd = 1 / a_g exactly, every product of the apply phase is exact and y = (x - m_g) / a_g * gamma + beta =
    +-gamma + beta bit for bit.  Premises asserted: an even element count per group, x and y representable in `dt`.
    -> dict(x, gamma, beta, y)"""
    n, C, groups, h, w = case.n, case.C, case.groups, case.h, case.w
    cpg, N = C // groups, h * w
    assert (N * cpg) % 2 == 0, "the two values need an even element count per group"
    r = _rng(15, n, C, groups, h, w, *key)
    m = r.integers(-8, 9, size=(n, groups)) / 4.0
    a = np.exp2(r.integers(-2, 2, size=(n, groups)).astype(np.float64))
    x = np.empty((n, C, N), np.float64)
    half = np.repeat([1.0, -1.0], N * cpg // 2)
    for b in range(n):
        for g in range(groups):
            x[b, g * cpg:(g + 1) * cpg] = (m[b, g] + a[b, g] * r.permutation(half)).reshape(cpg, N)
    x = x.reshape(n, C, h, w)
    gamma = r.integers(-8, 9, size=C) / 4.0
    gamma[gamma == 0] = 0.75
    beta = r.integers(-8, 9, size=C) / 8.0
    gi = np.arange(C) // cpg
    y = (x - m[:, gi, None, None]) / a[:, gi, None, None] * gamma[None, :, None, None] + beta[None, :, None, None]
    if act == "relu":
        y = np.maximum(y, 0.0)
    assert np.array_equal(round_to(x, dt), x) and np.array_equal(round_to(y, dt), y), "x and y must be exact in " + dt
    assert np.array_equal(y * 8, np.rint(y * 8))
    return dict(x=x, gamma=gamma, beta=beta, y=y)


def gn_generic_data(case, dt, *key, offset=0.0, constant_group=True):
    """x = offset + N(0, 1) as stored; gamma ~ 1 +- 0.3, beta ~ +-0.2; one constant-valued group (image 0, group 0)"""
    r = _rng(16, case.n, case.C, case.h, case.w, *key)
    x = offset + r.normal(size=(case.n, case.C, case.h, case.w))
    if constant_group:
        x[0, :case.C // case.groups] = 1.2998
    x = stored(x, dt)
    gamma = (1.0 + 0.3 * r.normal(size=case.C)).astype(np.float32).astype(np.float64)
    beta = (0.2 * r.normal(size=case.C)).astype(np.float32).astype(np.float64)
    return dict(x=x, gamma=gamma, beta=beta)


GN_OFFSET = {"f32": 2.0 ** 10, "f16": 2.0 ** 4}            # fp16 cannot hold more and keep a unit-variance signal
GN_OFFSET_CASE = GnCase("offset_c256_g32_20x24", 2, 256, 32, 20, 24)


# ========================================================================================================= proxy scores
def proxy_ref(feat, dots, counts, gamma, shift_class=False, subtract_max=True):
    """MPHead.forward_proxy in float64 from the operands as stored: per class c with proxies j,
    gamma * sum_j softmax(gamma * s)_j * s_j,  s_j = dots_j / max(|feat|, 1e-12).
    feat [n, C, h, w], dots [n, P, h, w] -> [n, nc, h, w].  shift_class / subtract_max=False are MUTANTS: class c reads
    from class c + 1's offset; the softmax does not subtract its maximum (and overflows like fp32 would)."""
    feat, dots = np.asarray(feat, np.float64), np.asarray(dots, np.float64)
    norm = np.maximum(np.sqrt((feat * feat).sum(1, keepdims=True)), 1e-12)
    s = dots / norm
    out, pos = [], 0
    P = int(np.sum(counts))
    for c, k in enumerate(counts):
        first = pos if not shift_class else min(pos + k, P - k)
        sub = s[:, first:first + k]
        z = sub * gamma
        if subtract_max:
            e = np.exp(z - z.max(1, keepdims=True))
        else:
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(z.astype(np.float32)).astype(np.float64)          # fp32 exp overflows past 88.7
        with np.errstate(invalid="ignore"):
            out.append((e * sub).sum(1, keepdims=True) / e.sum(1, keepdims=True) * gamma)
        pos += k
    return np.concatenate(out, 1)


PROXY_COUNTS = {
    "one": [1],
    "sixtyfour": [64],
    "mixed17": [2, 3, 1, 5, 4, 8, 64, 4, 3, 3, 1, 7, 2, 9, 6, 5, 11],
    "c256": [1] * 256,
}
ProxyCase = namedtuple("ProxyCase", "name counts n h w C gamma")
PROXY_CASES = [                                            # positions n * h * w: 1, 5, 6, 7, 8 = every remainder mod 4
    ProxyCase("one_p1_c8_g1", "one", 1, 1, 1, 8, 1.0),
    ProxyCase("one_p8_c256_g100", "one", 2, 2, 2, 256, 100.0),
    ProxyCase("sixtyfour_p5_c136_g10", "sixtyfour", 1, 1, 5, 136, 10.0),
    ProxyCase("sixtyfour_p6_c8_g100", "sixtyfour", 2, 3, 1, 8, 100.0),
    ProxyCase("mixed17_p7_c256_g10", "mixed17", 1, 7, 1, 256, 10.0),
    ProxyCase("mixed17_p5_c136_g100", "mixed17", 1, 5, 1, 136, 100.0),
    ProxyCase("mixed17_p6_c8_g1", "mixed17", 1, 2, 3, 8, 1.0),
    ProxyCase("c256_p8_c136_g1", "c256", 2, 1, 4, 136, 1.0),
    ProxyCase("c256_p7_c256_g100", "c256", 1, 1, 7, 256, 100.0),
    ProxyCase("c256_p1_c8_g10", "c256", 1, 1, 1, 8, 10.0),
]
PROXY_TOL = 2e-5                                           # the project's per-op bar for this kernel: * max(1, |want|)


def proxy_data(n, C, h, w, counts, dt, *key):
    """feat as stored (the last position of the last image is an all-zero row when there is more than one position), dots =
    feat . unit proxies rounded to fp32; proxy 0 is parallel to the first feature row, so that gamma * s reaches gamma there
    (gamma = 100 overflows an fp32 softmax that does not subtract its maximum) -> dict(feat, dots)"""
    r = _rng(17, n, C, h, w, len(counts), *key)
    P = int(np.sum(counts))
    feat = r.normal(size=(n, C, h, w))
    if n * h * w > 1:
        feat[n - 1, :, h - 1, w - 1] = 0.0
    feat = stored(feat, dt)
    prox = r.normal(size=(P, C))
    if np.abs(feat[0, :, 0, 0]).max() > 0:                 # proxy 0 points along the first feature: s = 1, gamma * s = gamma
        prox[0] = feat[0, :, 0, 0]
    prox /= np.sqrt((prox * prox).sum(1, keepdims=True))
    dots = np.einsum("bchw,kc->bkhw", feat, prox).astype(np.float32).astype(np.float64)
    return dict(feat=feat, dots=dots)


# =========================================================================================================== grid-stride
GRID_STRIDE_KERNELS = ["maxpool", "pool2d", "resample", "upsample_add", "nchw_pack", "focus_pack", "proxy_scores"]


def grid_stride_extent(kernel, dt):
    """the smallest extents (one image) whose work items exceed GRID_CAP for `kernel`, computed from the cap:
    -> dict(h, w, C, items) of the OUTPUT map (focus_pack: of the packed map, the image is twice as large)"""
    C = 8
    per_pixel = {"nchw_pack": 1, "focus_pack": 1, "proxy_scores": 16}.get(kernel, C // VN[dt])
    pixels = GRID_CAP // per_pixel + 1
    if kernel in ("resample", "upsample_add"):             # an even square-ish map: factor 2 / sizes (in, 2 in)
        side = int(np.ceil(np.sqrt(pixels)))
        side += side % 2
        h, w = side, (pixels + side - 1) // side
        w += w % 2
    else:
        h = 1 << ((pixels.bit_length() - 1) // 2)
        w = (pixels + h - 1) // h
    assert h * w * per_pixel > GRID_CAP >= (h * w - 4 * max(h, w)) * per_pixel          # a few rows past the cap at most
    return dict(h=h, w=w, C=C, items=h * w * per_pixel)
