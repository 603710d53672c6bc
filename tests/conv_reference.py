"""Exact-arithmetic reference of the conv family (tests/test_conv_exact.py, tests/test_conv_reference.py).

Plain numpy, int64 / float64 only; nothing of the engine is imported.

The data regime makes every fp32 step of the kernels exact, so that their results can be compared BIT FOR BIT:

  x, w     ternary {-1, 0, 1}: exact in fp16 / fp32, every product exact, every partial sum an integer far below 2^24 --
           the fp32 accumulator is exact in ANY summation order (tap-chunk or chunk-tap, either MFMA shape)
  scale    1 + j * 2^-11, j odd (12 significant bits), different for every output channel
  bias     a non-zero integer multiple of 2^-11, |bias| <= 8, different for every output channel
  res      an integer multiple of 2^-3, |res| <= 64 (exact in fp16)
  act      none / relu; both residual orders (act(v) + res, act(v + res))

With |acc| <= 1023: acc * scale has at most 10 + 12 bits, + bias stays a multiple of 2^-11 below 2^12 (23 bits), + res
likewise, max(., 0) is exact: the same value comes out whether or not the compiler contracts the multiply-add.  The one
rounding left is the conversion to the output type: an fp16 output is the float64 value rounded to nearest-even ONCE,
an fp32 output is the float64 value itself.  `check_regime` asserts both conditions (|acc| <= 1023; the float32
step-by-step epilogue equals the float64 one) for the data of a case: they are conditions, never tolerances.

A SECOND conv that consumes stored (rounded) results -- the chained 1x1, the 3x3 of the fused Bottleneck -- no longer
sees ternary inputs: its inputs are multiples of 2^-11.  It stays exact in any order while the sum of |input * weight|
over one output stays below 2^12 (every partial sum is then a multiple of 2^-11 below 2^12: 23 bits) and its scale is
a power of two (`second_scale_bias`: 1 or 1/2); `check_second_regime` asserts that.

Layouts: activations NCHW, weights OIHW (depthwise: [C, 1, R, S]), as torch.nn.functional.conv2d takes them.
"""
from collections import namedtuple

import numpy as np

ACC_MAX = 1023
SECOND_SUM_MAX = 4000.0           # sum |input * weight| of a conv on stored values (+ |bias| <= 8 stays below 2^12)


def _rng(*key):
    return np.random.default_rng([int(k) & 0x7fffffff for k in key])


# ------------------------------------------------------------------------------------------------------------ the data
def ternary(shape, *key):
    return _rng(1, *key).integers(-1, 2, size=shape).astype(np.int64)


def image(shape, *key):
    """integer image, values 0 .. 3 (the stems read fp32 NCHW pictures)"""
    return _rng(2, *key).integers(0, 4, size=shape).astype(np.int64)


def scale_bias(cout, *key):
    """-> (scale, bias) float64 [cout]: scale = 1 + j 2^-11 (j odd), bias = m 2^-11 (m != 0, |bias| <= 8), all different"""
    r = _rng(3, cout, *key)
    j = 2 * r.permutation(1024)[:cout] + 1
    m = r.permutation(2 * 16384)[:cout] - 16384
    m[m >= 0] += 1                                          # skip 0: -16384 .. -1, 1 .. 16384
    scale, bias = 1.0 + j * 2.0 ** -11, m * 2.0 ** -11
    assert len(set(scale)) == cout and len(set(bias)) == cout and np.abs(bias).max() <= 8 and (bias != 0).all()
    return scale, bias


def second_scale_bias(cout, *key):
    """for a conv on stored values: scale a power of two (1, 1/2 alternating from a random phase), bias as scale_bias"""
    _, bias = scale_bias(cout, 7, *key)
    scale = np.where((np.arange(cout) + int(_rng(4, cout, *key).integers(0, 2))) % 2 == 0, 1.0, 0.5)
    return scale, bias


def residual(shape, *key):
    return _rng(5, *key).integers(-512, 513, size=shape).astype(np.float64) / 8.0


# ------------------------------------------------------------------------------------------------------------ the conv
def _taps(x, R, S, stride, pad, dilation, pad_mode="zero"):
    """x [n, c, h, w] -> [R, S, n, c, ho, wo]: the input value each tap sees at each output pixel"""
    n, c, h, w = x.shape
    ho = (h + 2 * pad - dilation * (R - 1) - 1) // stride + 1
    wo = (w + 2 * pad - dilation * (S - 1) - 1) // stride + 1
    assert ho >= 1 and wo >= 1, (x.shape, R, S, stride, pad, dilation)
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), mode="constant" if pad_mode == "zero" else "edge")
    out = np.empty((R, S, n, c, ho, wo), x.dtype)
    for r in range(R):
        for s in range(S):
            out[r, s] = xp[:, :, r * dilation: r * dilation + (ho - 1) * stride + 1: stride,
                           s * dilation: s * dilation + (wo - 1) * stride + 1: stride]
    return out


def conv(x, w, stride=1, pad=0, dilation=1, depthwise=False, mutate=None, drop_k=0):
    """Direct convolution -> accumulator [n, cout, ho, wo], same dtype kind as the operands (int64 for the ternary regime,
    float64 for a conv on stored values).  Integer operands are summed as integers.
    mutate (wrong convs for the mutation check): 'k_tail' the last `drop_k` elements of K = (r, s, ci) are left out;
    'border_tap' the centre tap is left out at the last output column; 'edge_pad' the padding repeats the border value."""
    x, w = np.asarray(x), np.asarray(w)
    integer = x.dtype.kind == "i" and w.dtype.kind == "i"
    dt = np.int64 if integer else np.float64
    x, w = x.astype(dt), w.astype(dt)
    cout, cin, R, S = w.shape
    t = _taps(x, R, S, stride, pad, dilation, "edge" if mutate == "edge_pad" else "zero")
    if mutate == "border_tap":
        t = t.copy()
        t[R // 2, S // 2, :, :, :, -1] = 0
    if depthwise:
        assert cin == 1 and cout == x.shape[1]
        assert mutate != "k_tail"
        return np.einsum("rsnchw,crs->nchw", t, w[:, 0])
    assert cin == x.shape[1], (x.shape, w.shape)
    if mutate == "k_tail":                                  # k = (r * S + s) * cin + ci
        wk = w.transpose(0, 2, 3, 1).reshape(cout, -1).copy()
        wk[:, wk.shape[1] - drop_k:] = 0
        w = wk.reshape(cout, R, S, cin).transpose(0, 3, 1, 2)
    n, _, ho, wo = t.shape[2:]
    # [pixels, K] x [K, cout] in float64: the operands are integers or multiples of 2^-11, every partial sum lies far
    # below 2^53, so the product is the exact sum in any order (and it is what makes 7x7x136 cheap enough for a test)
    a = t.transpose(2, 4, 5, 0, 1, 3).reshape(n * ho * wo, R * S * cin).astype(np.float64)
    b = w.transpose(2, 3, 1, 0).reshape(R * S * cin, cout).astype(np.float64)
    acc = (a @ b).reshape(n, ho, wo, cout).transpose(0, 3, 1, 2)
    if integer:
        assert np.array_equal(acc, np.rint(acc))
        return acc.astype(np.int64)
    return np.ascontiguousarray(acc)


def abs_sum(x, w, stride=1, pad=0):
    """sum |x * w| per output: the bound on every partial sum of a conv on stored values"""
    return conv(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), stride, pad)


# -------------------------------------------------------------------------------------------------------- the epilogue
def _act(v, act):
    assert act in ("none", "relu"), act
    return np.maximum(v, v.dtype.type(0)) if act == "relu" else v


def epilogue(acc, scale, bias, res=None, act="none", res_first=False, dtype=np.float64, mutate=None):
    """act(acc * scale + bias) + res, or act(acc * scale + bias + res) with res_first, every step in `dtype`.
    mutate: 'scale_f16' / 'bias_f16' the vector rounded to fp16 first; 'bias_shift' bias[co + 1] for channel co;
    'swap' the other order of add and activation; 'round_before_add' the value is rounded to fp16 before the residual
    is added (act-then-add: act(v) rounded; add-then-act: v rounded)."""
    scale, bias = np.asarray(scale, np.float64), np.asarray(bias, np.float64)
    if mutate == "scale_f16":
        scale = scale.astype(np.float16).astype(np.float64)
    if mutate == "bias_f16":
        bias = bias.astype(np.float16).astype(np.float64)
    if mutate == "bias_shift":
        bias = np.roll(bias, -1)
    if mutate == "swap":
        res_first = not res_first
    f = lambda a: np.asarray(a).astype(dtype)
    v = f(acc) * f(scale)[None, :, None, None] + f(bias)[None, :, None, None]
    if res is None:
        return _act(v, act)
    if mutate == "round_before_add":
        if res_first:
            return _act(v.astype(np.float16).astype(dtype) + f(res), act)
        return _act(v, act).astype(np.float16).astype(dtype) + f(res)
    return _act(v + f(res), act) if res_first else _act(v, act) + f(res)


def round_to(v, out):
    """the ONE rounding: float64 -> 'f16' (nearest even) / 'f32' (must be exact)"""
    if out == "f16":
        return np.asarray(v, np.float64).astype(np.float16)
    r = np.asarray(v, np.float64).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), v), "an fp32 result of the regime needs no rounding"
    return r


def round_toward_zero_f16(v):
    """the wrong pack of the mutation check: truncation instead of round-to-nearest-even"""
    v = np.asarray(v, np.float64)
    r = v.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(v)
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float16)


def check_regime(acc, scale, bias, res=None, act="none", res_first=False):
    """the two conditions of the regime, for the data of one case; -> the float64 epilogue value"""
    assert np.abs(acc).max() <= ACC_MAX, "case outside the regime: max |acc| = %d" % np.abs(acc).max()
    v64 = epilogue(acc, scale, bias, res, act, res_first, np.float64)
    v32 = epilogue(acc, scale, bias, res, act, res_first, np.float32)
    assert np.array_equal(v32.astype(np.float64), v64), "case outside the regime: the float32 epilogue rounds"
    return v64


def check_second_regime(x, w, acc, scale, bias, res=None, act="none", res_first=False, stride=1, pad=0):
    """the conditions for a conv on stored values (multiples of 2^-11): every partial sum below 2^12, power-of-two
    scales, an exact float32 epilogue; -> the float64 epilogue value"""
    x = np.asarray(x, np.float64)
    assert np.array_equal(x * 2048.0, np.rint(x * 2048.0)), "stored values must be multiples of 2^-11"
    assert abs_sum(x, w, stride, pad).max() <= SECOND_SUM_MAX, "case outside the regime: sum |x w| = %g" % abs_sum(x, w, stride, pad).max()
    assert set(np.unique(scale)) <= {1.0, 0.5}
    v64 = epilogue(acc, scale, bias, res, act, res_first, np.float64)
    v32 = epilogue(acc, scale, bias, res, act, res_first, np.float32)
    assert np.array_equal(v32.astype(np.float64), v64), "case outside the regime: the float32 epilogue rounds"
    return v64


# ------------------------------------------------------------------------------------------------------------ the cases
# res: 0 none, 1 act(v) + res, 2 act(v + res); dst: 'dense' | 'slice' (channel slice) | 'window' (spatial window + channel
# slice: strided in n, h and w); rplace: 'dense' | 'window' (a window of a NaN-filled buffer)
Case = namedtuple("Case", "name n cin cout k stride h w act res dst rplace")


def _c(n, cin, cout, k, stride, h, w, act, res, dst, rplace="dense"):
    name = "n%d_ci%d_co%d_k%d_s%d_%dx%d_%s_r%d_%s%s" % (n, cin, cout, k, stride, h, w, act, res, dst,
                                                         "_rwin" if res and rplace == "window" else "")
    return Case(name, n, cin, cout, k, stride, h, w, act, res, dst, rplace)


# Extents against the pixel tiles of include/glsdet_hip.h (8x16, 8x32, 10x12, 6x21, 10x24, 6x42; flat 64 / 128 / 256):
# 7x5 lies inside every tile, 8x16 is exactly one (128 pixels flat; x3 images = whole flat tiles), 9x17 one pixel past it
# in each direction, 13x43 / 21x25 / 17x33 one past 6x42 / 10x24 (and 6x21 / 10x12 twice) / 8x32.  cin: K chunks of 64 and
# 128 bytes with and without a ragged tail, 1 .. 10 (fp32: 20) K panels; cout: below, at and past 32 / 64 / 128 rows.
CONV_CASES = [
    # 1x1: the persistent LDS-DMA kernel (16..31), the weight-stationary kernel (3), the generic tiles
    _c(3, 8, 8, 1, 1, 7, 5, "none", 0, "dense"),
    _c(1, 24, 40, 1, 1, 8, 16, "relu", 1, "slice"),
    _c(3, 64, 64, 1, 1, 9, 17, "relu", 2, "window", "window"),
    _c(1, 72, 72, 1, 1, 13, 43, "none", 1, "window"),
    _c(3, 128, 128, 1, 1, 8, 16, "relu", 0, "window"),
    _c(1, 136, 136, 1, 1, 17, 33, "relu", 1, "dense", "window"),
    _c(1, 320, 264, 1, 1, 9, 17, "none", 2, "slice"),
    _c(3, 640, 40, 1, 1, 7, 5, "relu", 0, "window"),
    _c(1, 64, 264, 1, 1, 21, 25, "relu", 1, "window", "window"),
    # 3x3 stride 1: the halo family (2, 4, 5, 8..13 and the 10x12 / 6x21 geometries) and the generic kernel
    _c(1, 64, 64, 3, 1, 8, 16, "relu", 1, "dense"),
    _c(3, 64, 72, 3, 1, 9, 17, "relu", 2, "window", "window"),
    _c(1, 128, 136, 3, 1, 13, 43, "none", 0, "window"),
    _c(1, 320, 264, 3, 1, 7, 5, "relu", 1, "slice"),
    _c(1, 24, 40, 3, 1, 21, 25, "relu", 1, "window"),
    _c(1, 72, 128, 3, 1, 17, 33, "relu", 2, "dense", "window"),
    _c(1, 136, 8, 3, 1, 9, 17, "none", 1, "slice"),
    # 5x5, 7x7
    _c(1, 64, 128, 5, 1, 9, 17, "relu", 0, "window"),
    _c(1, 8, 40, 5, 1, 7, 5, "relu", 1, "window", "window"),
    _c(1, 136, 64, 7, 1, 13, 43, "relu", 1, "window"),
    _c(1, 64, 72, 7, 1, 8, 16, "none", 2, "slice"),
    # 3x3 stride 2, odd and even extents
    _c(1, 64, 64, 3, 2, 17, 33, "relu", 1, "window", "window"),
    _c(3, 128, 136, 3, 2, 8, 16, "none", 0, "slice"),
    _c(1, 24, 72, 3, 2, 21, 25, "relu", 2, "dense"),
    _c(1, 320, 40, 3, 2, 13, 43, "relu", 0, "window"),
]

# the predictor form (fp16 operands, fp32 logits, 15 channels padded to 16): one case per 1x1 kernel family
PRED_CASES = [
    _c(3, 64, 16, 1, 1, 9, 17, "none", 0, "window"),
    _c(1, 136, 16, 1, 1, 8, 16, "none", 0, "slice"),
    _c(1, 320, 16, 1, 1, 13, 43, "none", 0, "dense"),
]

# depthwise: k 3 and 7, dilation 1 and 3, stride 1 and 2 (name, n, c, k, stride, dilation, h, w, act)
DwCase = namedtuple("DwCase", "name n c k stride dilation h w act")
DW_CASES = [DwCase("c%d_k%d_s%d_d%d_%dx%d_%s" % (c, k, s, d, h, w, act), n, c, k, s, d, h, w, act)
            for (n, c, k, s, d, h, w, act) in [(2, 24, 3, 1, 1, 9, 17, "relu"), (1, 72, 3, 2, 3, 13, 21, "none"),
                                              (2, 24, 7, 1, 3, 21, 25, "relu"), (1, 40, 7, 2, 1, 17, 33, "none")]]


def case_data(case, pred_cout=None):
    """-> dict x [n, cin, h, w] int64, w [cout, cin, k, k] int64, scale, bias, res (or None), acc, v (float64 value before
    the one rounding); the regime is asserted.  pred_cout: real output channels of a predictor case (the rest: zero
    weights, scale 1, bias 0 -- what Engine.pack_conv pads with)."""
    c = case
    x = ternary((c.n, c.cin, c.h, c.w), 11, *c[1:8])
    w = ternary((c.cout, c.cin, c.k, c.k), 12, *c[1:8])
    scale, bias = scale_bias(c.cout, *c[1:8])
    if pred_cout is not None:
        w[pred_cout:], scale[pred_cout:], bias[pred_cout:] = 0, 1.0, 0.0
    acc = conv(x, w, c.stride, c.k // 2)
    res = residual(acc.shape, 13, *c[1:8]) if c.res else None
    v = check_regime(acc, scale, bias, res, c.act, c.res == 2)
    return {"x": x, "w": w, "scale": scale, "bias": bias, "res": res, "acc": acc, "v": v}


def dw_case_data(case):
    c = case
    x = ternary((c.n, c.c, c.h, c.w), 21, *c[1:8])
    w = ternary((c.c, 1, c.k, c.k), 22, *c[1:8])
    scale, bias = scale_bias(c.c, 23, *c[1:8])
    pad = c.dilation * (c.k - 1) // 2
    acc = conv(x, w, c.stride, pad, c.dilation, depthwise=True)
    v = check_regime(acc, scale, bias, None, c.act)
    return {"x": x, "w": w, "scale": scale, "bias": bias, "acc": acc, "v": v, "pad": pad}


# ------------------------------------------------------------------------------------ glsdet_conv2d_multi: quadrant windows
# The problems are laid out as the GL-fusion neck lays them out: the inputs are the four quadrant windows (lt, lb, rt, rb)
# of ONE map full of real data, so that a 3x3 finds its neighbour's non-zero values directly outside its window and
# must read zeros instead; the outputs are the quadrant windows of ONE buffer.
MultiCase = namedtuple("MultiCase", "name n cin cout k stride h w h0 w0 act res per_image")
MULTI_CASES = [MultiCase("%s_n%d_ci%d_co%d_k%d_s%d_%dx%d_%s_r%d" % ("batched" if pi else "grouped", n, ci, co, k, s, h, w, act, res),
                         n, ci, co, k, s, h, w, h0, w0, act, res, pi)
               for (n, ci, co, k, s, h, w, h0, w0, act, res, pi) in [
                   (2, 64, 72, 3, 1, 13, 19, 6, 9, "relu", 1, False),        # unequal quadrants, ring hints 8..11
                   (1, 64, 136, 3, 2, 17, 33, 9, 16, "none", 0, False),       # stride 2: odd and even quadrant extents
                   (3, 24, 40, 1, 1, 9, 17, 4, 9, "relu", 1, False),          # 1x1, ragged K
                   (3, 64, 40, 3, 1, 10, 18, 5, 9, "relu", 1, True),          # batched: 3 images x 4 equal quadrants = 12
                   (5, 136, 72, 1, 1, 8, 16, 4, 8, "none", 0, True),          # batched: 20 problems, ragged K
               ]]


def out_extent(v, k, stride, pad, dilation=1):
    return (v + 2 * pad - dilation * (k - 1) - 1) // stride + 1


def multi_data(case):
    """-> dict x [n, cin, h, w], quads: list of 4 dicts {win (h0, h1, w0, w1) of x, owin of the output map, w, scale,
    bias}, res (full output map or None), v: the assembled float64 output map [n, cout, Ho, Wo]"""
    c = case
    pad = c.k // 2
    x = ternary((c.n, c.cin, c.h, c.w), 31, *c[1:10])
    hs, ws = [(0, c.h0), (c.h0, c.h)], [(0, c.w0), (c.w0, c.w)]
    oh = [out_extent(b - a, c.k, c.stride, pad) for a, b in hs]
    ow = [out_extent(b - a, c.k, c.stride, pad) for a, b in ws]
    ohs, ows = [(0, oh[0]), (oh[0], oh[0] + oh[1])], [(0, ow[0]), (ow[0], ow[0] + ow[1])]
    res = residual((c.n, c.cout, sum(oh), sum(ow)), 32, *c[1:10]) if c.res else None
    v = np.zeros((c.n, c.cout, sum(oh), sum(ow)))
    quads = []
    for q, (iw, ih) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):             # lt, lb, rt, rb
        (a, b), (l, r) = hs[ih], ws[iw]
        (oa, ob), (ol, orr) = ohs[ih], ows[iw]
        w = ternary((c.cout, c.cin, c.k, c.k), 33, q, *c[1:10])
        scale, bias = scale_bias(c.cout, 34, q, *c[1:10])
        acc = conv(x[:, :, a:b, l:r], w, c.stride, pad)
        rq = res[:, :, oa:ob, ol:orr] if c.res else None
        v[:, :, oa:ob, ol:orr] = check_regime(acc, scale, bias, rq, c.act, c.res == 2)
        quads.append({"win": (a, b, l, r), "owin": (oa, ob, ol, orr), "w": w, "scale": scale, "bias": bias})
    return {"x": x, "quads": quads, "res": res, "v": v}


# --------------------------------------------------------------------------------------------- glsdet_conv2d_chain
ChainCase = namedtuple("ChainCase", "name n cin cout stride h w act res c0 cin2 cout2 act2 skip_y")
CHAIN_CASES = [ChainCase("n%d_ci%d_co%d_s%d_%dx%d_%s_r%d_c%d+%d_co%d_%s%s" % (n, ci, co, s, h, w, act, res, c0, cin2, co2, act2,
                                                                              "_skipy" if sk else ""),
                         n, ci, co, s, h, w, act, res, c0, cin2, co2, act2, sk)
               for (n, ci, co, s, h, w, act, res, c0, cin2, co2, act2, sk) in [
                   (1, 64, 64, 1, 9, 17, "relu", 1, 0, 32, 40, "relu", False),
                   (1, 64, 128, 1, 13, 43, "relu", 0, 64, 64, 72, "none", False),
                   (2, 64, 64, 1, 8, 16, "relu", 0, 0, 64, 128, "relu", True),
                   (1, 64, 64, 2, 17, 33, "relu", 0, 0, 64, 64, "relu", True),
                   (1, 64, 64, 2, 17, 33, "relu", 0, 0, 64, 64, "relu", False),
                   (3, 32, 64, 2, 8, 16, "relu", 0, 0, 64, 40, "none", True),
               ]]


def chain_data(case):
    """3x3 conv (stage 1, the regime) + 1x1 on channels [c0, c0 + cin2) of its STORED result.  out: 'f16' / 'f32' decides
    what is stored: -> function of out giving dict x, w, scale, bias, res, y (stored, as out's numpy type), w2, scale2,
    bias2, y2 (stored)"""
    c = case
    x = ternary((c.n, c.cin, c.h, c.w), 41, *c[1:7])
    w = ternary((c.cout, c.cin, 3, 3), 42, *c[1:7])
    scale, bias = scale_bias(c.cout, 43, *c[1:7])
    acc = conv(x, w, c.stride, 1)
    res = residual(acc.shape, 44, *c[1:7]) if c.res else None
    v = check_regime(acc, scale, bias, res, c.act, c.res == 2)
    w2 = ternary((c.cout2, c.cin2, 1, 1), 45, *c[1:7])
    scale2, bias2 = second_scale_bias(c.cout2, 46, *c[1:7])

    def stored(out):
        y = round_to(v, out)
        x2 = y[:, c.c0:c.c0 + c.cin2].astype(np.float64)
        acc2 = conv(x2, w2)
        v2 = check_second_regime(x2, w2, acc2, scale2, bias2, None, c.act2)
        return {"x": x, "w": w, "scale": scale, "bias": bias, "res": res, "y": y, "w2": w2, "scale2": scale2, "bias2": bias2,
                "y2": round_to(v2, out)}
    return stored


# ----------------------------------------------------------------------------------------------- glsdet_bottleneck
BneckCase = namedtuple("BneckCase", "name n cin0 cm h w res")
BNECK_CASES = [BneckCase("n%d_ci%d_cm%d_%dx%d_r%d" % t, *t)
               for t in [(2, 64, 32, 9, 17, 1), (1, 128, 64, 13, 21, 0), (1, 96, 64, 8, 16, 1), (1, 64, 64, 7, 5, 0)]]


def bneck_data(case):
    """1x1 (the regime, relu) -> hidden, stored; 3x3 stride 1 on the stored hidden values (+ res, relu)"""
    c = case
    x = ternary((c.n, c.cin0, c.h, c.w), 51, *c[1:])
    w1 = ternary((c.cm, c.cin0, 1, 1), 52, *c[1:])
    s1, b1 = scale_bias(c.cm, 53, *c[1:])
    v1 = check_regime(conv(x, w1), s1, b1, None, "relu")
    w2 = ternary((c.cm, c.cm, 3, 3), 54, *c[1:])
    s2, b2 = second_scale_bias(c.cm, 55, *c[1:])
    res = residual(v1.shape, 56, *c[1:]) if c.res else None

    def stored(out):
        hid = round_to(v1, out)
        h64 = hid.astype(np.float64)
        v2 = check_second_regime(h64, w2, conv(h64, w2, 1, 1), s2, b2, res, "relu", False, 1, 1)
        return {"x": x, "w1": w1, "s1": s1, "b1": b1, "hidden": hid, "w2": w2, "s2": s2, "b2": b2, "res": res,
                "y": round_to(v2, out)}
    return stored


# ------------------------------------------------------------------------------------------- glsdet_conv2d_gnstats
GnCase = namedtuple("GnCase", "name n cin cout groups h w act")
GN_CASES = [GnCase("n%d_ci%d_co%d_g%d_%dx%d_%s" % t, *t)
            for t in [(2, 64, 64, 8, 9, 17, "none"), (1, 128, 128, 4, 13, 43, "relu"), (1, 64, 128, 16, 8, 16, "none")]]


def gn_data(case):
    """-> function of out: dict x, w, scale, bias, y (stored), s1 / s2: exact integer sums per (image, group) of the stored
    values and of their squares, in units of 2^-11 and 2^-22 (python ints in object arrays)"""
    c = case
    x = ternary((c.n, c.cin, c.h, c.w), 61, *c[1:7])
    w = ternary((c.cout, c.cin, 3, 3), 62, *c[1:7])
    scale, bias = scale_bias(c.cout, 63, *c[1:7])
    v = check_regime(conv(x, w, 1, 1), scale, bias, None, c.act)

    def stored(out):
        y = round_to(v, out)
        q = y.astype(np.float64) * 2048.0
        assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < 2 ** 24
        q = q.astype(np.int64).reshape(c.n, c.groups, -1)
        return {"x": x, "w": w, "scale": scale, "bias": bias, "y": y, "s1": q.sum(2), "s2": (q * q).sum(2)}
    return stored


# ------------------------------------------------------------------------------------------------------- the stems
def focus(img):
    """space-to-depth of drone/models/base/darknet.py:15-21: channels (TL, BL, TR, BR) x (c0, c1, c2)"""
    return np.concatenate((img[..., ::2, ::2], img[..., 1::2, ::2], img[..., ::2, 1::2], img[..., 1::2, 1::2]), 1)


def maxpool(x, k, stride, pad):
    t = _taps(np.pad(np.asarray(x, np.float64), ((0, 0), (0, 0), (pad, pad), (pad, pad)), constant_values=-np.inf), k, k, stride, 0, 1)
    return t.max(axis=(0, 1))


StemCase = namedtuple("StemCase", "name n cout h w act")
FOCUS_CASES = [StemCase("n%d_co%d_%dx%d_%s" % t, *t) for t in [(2, 32, 16, 32, "relu"), (1, 40, 18, 34, "none")]]
RESNET_STEM_CASES = [StemCase("n%d_co%d_%dx%d_%s" % t, *t) for t in [(2, 64, 16, 32, "relu"), (1, 64, 37, 29, "relu")]]


def focus_data(case, down_cout=None):
    """Focus + 3x3 (the regime; image values 0 .. 3) -> y; with down_cout also the 3x3 stride-2 conv on the STORED y
    (glsdet_focus_conv_down: the stem then has 32 channels and relu)"""
    c = case
    cout = 32 if down_cout else c.cout
    img = image((c.n, 3, c.h, c.w), 71, *c[1:5])
    w = ternary((cout, 12, 3, 3), 72, *c[1:5])
    scale, bias = scale_bias(cout, 73, *c[1:5])
    act = "relu" if down_cout else c.act
    v = check_regime(conv(focus(img), w, 1, 1), scale, bias, None, act)
    w2 = s2 = b2 = None
    if down_cout:
        w2 = ternary((down_cout, 32, 3, 3), 74, *c[1:5])
        s2, b2 = second_scale_bias(down_cout, 75, *c[1:5])

    def stored(out):
        d = {"img": img, "w": w, "scale": scale, "bias": bias, "act": act, "y": round_to(v, out)}
        if down_cout:
            y64 = d["y"].astype(np.float64)
            v2 = check_second_regime(y64, w2, conv(y64, w2, 2, 1), s2, b2, None, c.act, False, 2, 1)
            d.update({"w2": w2, "scale2": s2, "bias2": b2, "y2": round_to(v2, out)})
        return d
    return stored


def resnet_stem_data(case):
    """7x7 stride 2 pad 3 over the 3-channel image (+ relu), and MaxPool2d(3, 2, 1) of the STORED result"""
    c = case
    img = image((c.n, 3, c.h, c.w), 81, *c[1:5])
    w = ternary((64, 3, 7, 7), 82, *c[1:5])
    scale, bias = scale_bias(64, 83, *c[1:5])
    v = check_regime(conv(img, w, 2, 3), scale, bias, None, "relu")

    def stored(out):
        y = round_to(v, out)
        return {"img": img, "w": w, "scale": scale, "bias": bias, "y": y, "pooled": maxpool(y, 3, 2, 1).astype(y.dtype)}
    return stored
