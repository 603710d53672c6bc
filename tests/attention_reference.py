"""An independent, deliberately naive reference of the data-dependent attention path (glsdet_amd/csrc/adapt.hip, the
windowed non-local block of nonlocal.hip, dwconv.hip) and the input builders of its differential tests.  TEST INFRASTRUCTURE
ONLY; imports nothing from `oracle` -- it is the second opinion that tests/test_attention_reference.py holds against the
oracle and tests/test_attention_fuzz.py against the kernels.

Why the GPU tests may demand equality.  The split is a chain of discrete decisions (`v < thr`, `2 d > total`, i // 2 * 2,
the clamp).  Every map the builders produce holds values k / 2^g with integer k, and every builder ASSERTS that the sum
of |k| over the whole map stays below 2^24: every partial sum, in whatever order a kernel or torch adds it up, is then an
integer of grid units below 2^24 and exactly representable in float32, and so are `0.5 * total` and the threshold
`min + 0.75 (max - min)` (4 min + 3 (max - min) quarter units, asserted below 2^24 as well).  No rounding happens anywhere,
so `split_reference` may restate the decisions in Python ints.  For fp16 storage |k| < 2^11 and 2^-g >= 2^-14 keep every
value an fp16 normal number.

Quadrant order everywhere: 0 lt, 1 lb, 2 rt, 3 rb (bit 0 = below the row split, bit 1 = right of the column split; the
column split is cyl above the row split and cyr from it on)."""
import numpy as np

LIMIT = 1 << 24


# ------------------------------------------------------------------------------------------------ the split, in integers
def split_reference(m):
    """m: integer array [n, H, W] (or an object array of Python ints), the attention map in grid units.  -> (cx, cyl, cyr) of
    Patch_Conv_NonLocal_adapt_new.forward: values under min + 0.75 (max - min) zeroed; row split of the whole map; column
    split of the rows above it and of the rows from it on.  One split for the whole batch."""
    m = np.asarray(m)
    assert m.ndim == 3 and (np.issubdtype(m.dtype, np.integer) or m.dtype == object)
    n, H, W = m.shape
    a = [[[int(v) for v in row] for row in img] for img in m.tolist()]
    mx = max(v for img in a for row in img for v in row)
    mn = min(v for img in a for row in img for v in row)
    for img in a:
        for row in img:
            for j, v in enumerate(row):
                if 4 * v < 4 * mn + 3 * (mx - mn):          # v < min + 0.75 (max - min): strictly
                    row[j] = 0

    def first(sums):
        """sums[i]: the batch's mass at index i"""
        size = len(sums)
        total = sum(sums)
        d = 0
        i = 0
        for i in range(size):
            d += sums[i]
            if 2 * d > total:                               # d > 0.5 total: strictly
                break
        i = i // 2 * 2                                      # (i is size - 1 after an unbroken loop)
        i = 4 if i < 4 else i
        return size - 4 if i > size - 4 else i

    cx = first([sum(sum(a[b][h]) for b in range(n)) for h in range(H)])
    cyl = first([sum(a[b][h][w] for b in range(n) for h in range(cx)) for w in range(W)])
    cyr = first([sum(a[b][h][w] for b in range(n) for h in range(cx, H)) for w in range(W)])
    return cx, cyl, cyr


def split_trace(m):
    """What the case list's coverage assertions need to know about a map: does a running row / column sum hit exactly half
    of its total (a tie the strict `>` must walk past), does a value equal the threshold (kept by the strict `<`)."""
    m = np.asarray(m).astype(object)
    mx, mn = m.max(), m.min()
    thr4 = 4 * mn + 3 * (mx - mn)
    on_thr = bool(((4 * m) == thr4).any()) and mx != mn
    a = np.where(4 * m < thr4, 0, m)
    cx = split_reference(np.asarray(m, np.int64))[0]
    tie = False
    for v in (a.sum((0, 2)), a[:, :cx].sum((0, 1)), a[:, cx:].sum((0, 1))):
        run, total = 0, v.sum()
        for s in v:
            run += s
            tie = tie or (2 * run == total and total != 0)
    return {"tie": tie, "on_threshold": on_thr}


# ------------------------------------------------------------------------------------------------------- dyadic builders
def assert_exact(k, g, f16=True):
    """the precondition of every exact comparison on a map of grid values k / 2^g (module docstring)"""
    k = np.asarray(k, np.int64)
    assert int(np.abs(k).sum()) < LIMIT, "partial sums leave the exact range of float32"
    mx, mn = int(k.max()), int(k.min())
    assert 4 * max(abs(mx), abs(mn)) + 3 * (mx - mn) < LIMIT
    if f16:
        assert int(np.abs(k).max()) < 2048 and 0 <= g <= 14, "not an fp16 normal number with 11 significant bits"
    return k


def to_float(k, g):
    return (np.asarray(k, np.int64).astype(np.float64) / float(1 << g)).astype(np.float32)


def _blobs(n, H, W, blobs, bg=0):
    """background bg and 3 x 3 blobs [(image, row, col, value)] centred at (row, col), clipped at the border"""
    k = np.full((n, H, W), bg, np.int64)
    for b, r, c, v in blobs:
        k[b, max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = v
    return k


def split_maps(n, H, W, seed=0):
    """-> [(name, k [n,H,W] int64, g)]: every structure the split can trip over, on an H x W map of n images (H, W >= 8)."""
    rng = np.random.RandomState(1000 * n + 10 * H + W + seed)
    last = n - 1
    out = []
    add = lambda name, k, g=6: out.append((name, assert_exact(k, g), g))
    hi = max(1, min(255, (LIMIT - 1) // (n * H * W) - 1))          # coarse enough for the exactness assertion
    add("random", rng.randint(0, hi + 1, (n, H, W)))
    add("random_signed", rng.randint(-hi // 2, hi // 2 + 1, (n, H, W)), 8)
    add("blob_before_4", _blobs(n, H, W, [(0, 1, 1, 200)], 3))                      # every centroid under the clamp
    add("blob_after_size_4", _blobs(n, H, W, [(last, H - 2, W - 2, 200)], 3))       # ... over it
    add("blob_top_right_bottom_left", _blobs(n, H, W, [(0, 1, W - 2, 200), (last, H - 2, 1, 200)]))
    add("blob_top_left_bottom_right", _blobs(n, H, W, [(0, 1, 1, 200), (last, H - 2, W - 2, 200)]))     # cyl far from cyr
    if H >= 12 and W >= 12:
        add("blob_on_odd_index", _blobs(n, H, W, [(0, 5, 7, 100)]))                 # running sum passes half at 5 and 7
        add("far_apart_columns", _blobs(n, H, W, [(0, 2, 2, 90), (last, H - 3, W - 3, 100)]))
    # mirror symmetry in both axes: the running sum is EXACTLY half the total in the middle (no break there)
    q = rng.randint(0, min(hi, 63) + 1, (n, (H + 1) // 2, (W + 1) // 2))
    top = np.concatenate([q[:, :, : W // 2], q[:, :, ::-1]], 2) if W % 2 == 0 else np.concatenate([q[:, :, :-1], q[:, :, ::-1]], 2)
    sym = np.concatenate([top[:, : H // 2], top[:, ::-1]], 1) if H % 2 == 0 else np.concatenate([top[:, :-1], top[:, ::-1]], 1)
    add("mirror_symmetric_tie", sym)
    two = np.zeros((n, H, W), np.int64)                            # two equal rows / columns: the tie, undisturbed by a threshold
    two[:, H // 2 - 1, :] = 1
    two[:, H // 2, :] = 1
    add("two_equal_rows_tie", two, 0)
    # values exactly ON the threshold (min 0, max 4a, threshold 3a) carry the mass; they are kept, not zeroed
    t = np.zeros((n, H, W), np.int64)
    t[0, 1, 1] = 64
    t[last, H - 2, :] = 48
    t[last, :, W - 2] = 48
    add("values_on_threshold", t)
    add("constant", np.full((n, H, W), 5, np.int64), 3)            # max == min: threshold = the value, everything kept
    add("all_zero", np.zeros((n, H, W), np.int64), 0)              # the loop never breaks
    add("all_negative", -rng.randint(1, min(hi, 200) + 1, (n, H, W)), 5)
    if n > 1:                                                      # images that would split differently alone
        d = _blobs(n, H, W, [(0, 1, 1, 100), (last, H - 2, W - 2, 60)])
        d[last, H - 3:, :] += 40
        add("images_disagree", d)
    return out


def split_shapes():
    """(n, H, W) of the split tests: 8 x 8 (both clamps coincide), 8 x W, H x 8, odd extents, n in 1, 2, 3, 16, and the
    largest map glsdet_attn_split accepts (n (H + 2 W) + 2048 = 15360 floats of LDS)."""
    return [(1, 8, 8), (2, 8, 20), (3, 20, 8), (1, 13, 17), (2, 12, 20), (3, 15, 21), (16, 12, 20), (16, 9, 11), (1, 24, 36),
            (2, 64, 3296)]


def split_cases():
    """-> [(id, k, g)] over split_shapes()"""
    return [("%dx%dx%d-%s" % (n, H, W, name), k, g) for n, H, W in split_shapes() for name, k, g in split_maps(n, H, W)]


def probe_maps(count=400, seed=7):
    """the sweep the integer reference was first validated on: generated dyadic maps of batch size 1, 2, 3, 16; random, a
    hot blob, constant, mirror-symmetric, values on the threshold"""
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        n = (1, 2, 3, 16)[i % 4]
        H, W = int(rng.randint(8, 25)), int(rng.randint(8, 25))
        kind = i % 5
        if kind == 0:
            k = rng.randint(0, 256, (n, H, W))
        elif kind == 1:
            k = _blobs(n, H, W, [(int(rng.randint(n)), int(rng.randint(H)), int(rng.randint(W)), 200)], int(rng.randint(0, 4)))
            k = k + rng.randint(0, 2, (n, H, W))
        elif kind == 2:
            k = np.full((n, H, W), int(rng.randint(-9, 10)), np.int64)
        elif kind == 3:
            q = rng.randint(0, 64, (n, H, W))
            k = q + q[:, ::-1] + q[:, :, ::-1] + q[:, ::-1, ::-1]
        else:
            k = rng.randint(0, 5, (n, H, W)) * 16
            k[0, 0, 0], k[-1, -1, -1] = 0, 64                      # min 0, max 64: the 48s sit on the threshold
        out.append((assert_exact(k, 6), 6))
    return out


def host_splits(H, W):
    """(cx, cyl, cyr) that a host-written split tensor takes for an H x W map: both clamps on every index, cyl far from
    cyr, and values whose halves are odd (the shift-1 consumers halve them)."""
    s = [(4, 4, 4), (H - 4, W - 4, W - 4), (4, W - 4, 4), (H - 4, 4, W - 4), (6, 10, 6), (10, 6, 14)]
    return [t for t in s if 4 <= t[0] <= H - 4 and 4 <= t[1] <= W - 4 and 4 <= t[2] <= W - 4]


# ---------------------------------------------------------------------------------------------------------- rowsplit
def quadrant_slices(split, shift, q):
    cx, cyl, cyr = (int(s) >> shift for s in split[:3])
    bottom, right = q & 1, q >> 1
    c = cyr if bottom else cyl
    return (slice(cx, None) if bottom else slice(0, cx)), (slice(c, None) if right else slice(0, c))


def rowsplit_reference(a, b, y0, split, mode, q, shift):
    """glsdet_rowsplit on NCHW arrays, by slicing.  y0: what the output buffer held before (mode 4 leaves it untouched
    outside quadrant q; every other mode overwrites everything)."""
    cx = int(split[0]) >> shift
    y = y0.copy() if mode == 4 else np.zeros_like(a)
    if mode == 0:
        y[:, :, :cx] = a[:, :, :cx]
    elif mode == 1:
        y[:, :, cx:] = a[:, :, cx:]
    elif mode == 2:
        y[:, :, :cx] = a[:, :, :cx]
        y[:, :, cx:] = b[:, :, cx:]
    else:
        assert mode in (3, 4)
        r, c = quadrant_slices(split, shift, q)
        y[:, :, r, c] = a[:, :, r, c]
    return y


# ------------------------------------------------------------------------------------------------- windowed non-local
def nonlocal_windows_reference(x, tpg, wout, bout, split, shift):
    """x [n, cx, H, W]; tpg[q] [n, >= 3 ci, H, W] = theta | phi | g of quadrant q's weights over the full map; wout[q]
    [cx, ci]; bout[q] [cx].  float64, the definition per window and pixel:
    out_i = x_i + Wout sum_j (theta_i . phi_j / N) g_j + b."""
    x = np.asarray(x, np.float64)
    out = np.full_like(x, np.nan)
    n = x.shape[0]
    for q in range(4):
        r, c = quadrant_slices(split, shift, q)
        ci = wout[q].shape[1]
        t = np.asarray(tpg[q], np.float64)[:, :, r, c]
        hh, ww = t.shape[2], t.shape[3]
        N = hh * ww
        for b in range(n):
            theta = t[b, 0:ci].reshape(ci, N).T                    # [N, ci]
            phi = t[b, ci:2 * ci].reshape(ci, N).T
            g = t[b, 2 * ci:3 * ci].reshape(ci, N).T
            f = theta @ phi.T / N                                  # [N, N] pairwise
            y = f @ g                                              # [N, ci]
            o = y @ np.asarray(wout[q], np.float64).T + np.asarray(bout[q], np.float64)      # [N, cx]
            out[b, :, r, c] = x[b, :, r, c] + o.T.reshape(-1, hh, ww)
    return out


def membership_reference(shape, split, shift):
    """q + 1 on quadrant q's window, over [n, c, H, W]"""
    m = np.zeros(shape, np.float32)
    for q in range(4):
        r, c = quadrant_slices(split, shift, q)
        m[:, :, r, c] += q + 1
    return m


# ------------------------------------------------------------------------------------------------- elementwise gating
_NP = {"f16": np.float16, "f32": np.float32}


def _store(v64, dtype):
    """float64 -> float32 -> storage dtype: the kernels compute in float32 and convert on the store"""
    with np.errstate(over="ignore"):
        return v64.astype(np.float32).astype(_NP[dtype]).astype(np.float32)


def scale_by_map_reference(x, m, dtype):
    """x [n, c, H, W] * m [n, 1, H, W]"""
    return _store(np.asarray(x, np.float64) * np.asarray(m, np.float64), dtype)


def gate_reference(a, b, m, dtype):
    """m None: a * b; else a * m[:, 0] + b * m[:, 1]"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if m is None:
        return _store(a * b, dtype)
    m = np.asarray(m, np.float64)
    return _store(a * m[:, 0:1] + b * m[:, 1:2], dtype)


def gate_bound(a, b, m, dtype):
    """per-element bound of mode 0 on continuous operands: 2 * 2^-23 (|a g0| + |b g1|) for the float32 arithmetic with or
    without a contracted multiply-add, plus half an ulp of the storage dtype at the reference value"""
    a, b, m = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(m, np.float64)
    mag = np.abs(a * m[:, 0:1]) + np.abs(b * m[:, 1:2])
    ref = a * m[:, 0:1] + b * m[:, 1:2]
    t = _NP[dtype]
    with np.errstate(over="ignore"):
        near = np.abs(ref).astype(t)
        ulp = np.abs(np.nextafter(near, t(np.inf)).astype(np.float64) - near.astype(np.float64))
    return 2.0 * 2.0 ** -23 * mag + 0.5 * ulp


# ------------------------------------------------------------------------------------------------------ depthwise conv
def dwconv_reference(x, w, scale, bias, stride, pad, dilation, act, dtype):
    """x [n, C, H, W] and w [C, 1, R, S] already rounded to the storage dtype; scale, bias [C] float32.
    F.conv2d(groups = C) in float64, * scale + bias, activation in float64, ONE rounding to the storage dtype."""
    import torch
    import torch.nn.functional as F
    C = x.shape[1]
    y = F.conv2d(torch.as_tensor(np.asarray(x, np.float64)), torch.as_tensor(np.asarray(w, np.float64)), None, stride, pad,
                 dilation, C)
    y = y * torch.as_tensor(np.asarray(scale, np.float64)).view(1, C, 1, 1) + torch.as_tensor(np.asarray(bias, np.float64)).view(1, C, 1, 1)
    if act == "relu":
        y = torch.clamp(y, min=0)
    elif act == "lrelu":
        y = torch.where(y > 0, y, np.float64(np.float32(0.1)) * y)
    elif act == "silu":
        y = y / (1 + torch.exp(-y))
    else:
        assert act == "none"
    return y.numpy().astype(_NP[dtype]).astype(np.float32)


def dwconv_dyadic(C, H, W, R, S, seed, n=2):
    """Operands on which every float32 accumulation of a depthwise conv is exact: x = kx / 8, w = kw / 16 with |kx|, |kw|
    <= 15, scale a power of two, bias a multiple of scale / 128 -- acc * scale + bias is an integer of scale / 128 units
    below 2^24 (asserted), so only the store rounds, with or without a contracted multiply-add."""
    rng = np.random.RandomState(seed)
    kx = rng.randint(-15, 16, (n, C, H, W))
    kw = rng.randint(-15, 16, (C, 1, R, S))
    e = rng.randint(-2, 3, C)
    kb = rng.randint(-4096, 4097, C)
    assert R * S * 15 * 15 + 4096 < LIMIT
    x = kx.astype(np.float32) / 8
    w = kw.astype(np.float32) / 16
    scale = (2.0 ** e).astype(np.float32)
    bias = (kb * 2.0 ** e / 128).astype(np.float32)
    return x, w, scale, bias
