"""Float64 reference of the activation epilogues of the conv family (tests/test_act_exact.py, tests/test_act_reference.py).

Plain numpy + math, float64 / int64 only; nothing of the engine is imported.  tests/conv_reference.py pins the conv family
bit for bit where the activation is `none` or `relu`; this module carries the same idea to SiLU, leaky ReLU, GELU and
sigmoid, which round: the PRE-ACTIVATION is made exact, the activation is evaluated in float64, and a kernel's result is
accepted when it is the rounding of some value within a DERIVED distance `tol` of the float64 value.

Exact pre-activations.  x and w are ternary (or 0 / 1), the accumulator is an integer |acc| <= 1023 (check_regime of
conv_reference), scales are powers of two, biases and residuals dyadic: v = acc * scale + bias (and v + res where the
residual is added before the activation) is exactly representable in float32 whether or not the compiler contracts the
multiply-add.  Every builder asserts this (check_regime, _exact32) and returns v as float64.

Acceptance is an interval, not a share of mismatches.  For every output element the accepted results are the values
rn(y) for y in [ref - tol, ref + tol], i.e. the closed range [rn(ref - tol), rn(ref + tol)] of the output type, rn =
round to nearest even as numpy.astype does it (fp16: overflow to inf included).  +0 and -0 compare equal; NaN is never
accepted for a finite v.  No element is skipped.

Tolerances (u = 2^-24, the unit roundoff of float32; "1 ulp" of an instruction = relative error <= 2u).

  none, relu   tol = 0: no operation rounds.  Repeats the contract of conv_reference at the new value ranges.

  lrelu        v > 0 ? v : 0.1f * v.  f32 engine: tol = 0 against float64(float32(0.1)) * v -- rn of that product to
               float32 IS the one float32 multiply (with a residual added afterwards the reference value of the
               activation is that ROUNDED product: the sum is a second float32 operation on it).  fp16 engine: the float32 product is rounded once more to fp16, a
               double rounding that can differ from rn16 of the exact product only if the float32 rounding (<= u |ref|)
               moves the value across an fp16 rounding boundary: tol = u |ref|.

  silu, fp16 engine  (conv_common.h, both forms)  t = v * -log2e; e = v_exp_f32(t); s = 1 + e; r = v_rcp_f32(s); y = v * r.
               t carries the rounding of the product (u) and of the constant (float32(log2 e) is off by 1.3e-8 relative,
               < u): |dt| <= 2u |t|, so e is off by a factor 1 +- (2u |t| ln 2 = 2u |v|) on top of the instruction's 2u.
               y = v / (1 + e) depends on e through dy/y = -(e / (1 + e)) de/e = -sigma(-v) de/e, so those two terms reach
               the result as (2 |v| + 2) sigma(-v) u <= (2 |v| sigma(-v) + 2) u; the add u, v_rcp_f32 2u, the product u.
               Sum: (6 + 2 |v| sigma(-v)) u; the bound used is tol = (8 + 2 |v| sigma(-v)) u |ref| + 2^-120.  The |v| term
               vanishes for positive v.  The floor 2^-120 covers exp overflowing to inf (result -0) a little before the
               true result leaves the normal range: v < -88.72 gives |ref| < 89 e^-88.72 = 2.6e-37 < 2^-120 = 7.5e-37.

  silu f32 engine, sigmoid f32 engine, silu of dwconv.hip (both dtypes)   v / (1 + expf(-v)), 1 / (1 + expf(-v)):
               expf 1 ulp (2u, times sigma(-v) <= 1), the add u, a correctly rounded divide u: 4u; the bound used is
               tol = 6u |ref| + 2^-120.

  gelu (both engines), sigmoid (fp16 engine)   0.5f * v * (1 + erff(v * 0.70710678f)) cancels for negative v: the
               rounding of 1 + erff is absolute (<= u), so the error is ~ u |v| / 2 whatever the result.  The accuracy of
               erff is not stated in this tree, so the bar is MEASURED, in units g(v) = u (|ref| + |v| / 2): the same
               float32 expression is evaluated on the CPU (numpy float32 steps, math.erf / exp rounded to float32 as the
               primitive) over the whole sweep of `sweep_data`, and the bar is max(4, 2 * that maximum) units -- the
               factor 2 allows a 2-ulp primitive against the correctly rounded one.  `measured_units` does that; the
               kernel's own output never enters.

Residual modes: 0 none; 1 act(v) + res: tol = tol_act + u |ref_sum| (the one float32 add); 2 act(v + res): v + res is
exact (asserted), the activation's tol applies to it.

Value sets: `sweep_data` (1x1: every finite fp16 value as v, plus the thresholds where the implementations change
behaviour), `REGION_CASES` / `region_data` (k x k, strided, depthwise, grouped and stem shapes: random ternary data whose
per-channel scale and bias put every region of REGION_EDGES under test; asserted for every case by `check_coverage`).
"""
import math
from collections import namedtuple

import numpy as np

from tests import conv_reference as R

ACTS = ["none", "silu", "relu", "lrelu", "gelu", "sigmoid"]           # codes 0 .. 5 of include/glsdet_hip.h
DW_ACTS = ["none", "silu", "relu", "lrelu"]                            # what glsdet_dwconv2d accepts
ENGINES = ["f16", "f32"]
U = 2.0 ** -24
FLOOR = 2.0 ** -120
SLOPE = float(np.float32(0.1))                                         # the kernel's constant is 0.1f
LOG2E32 = np.float32(1.44269504088896340736)
SQRT1_2_32 = np.float32(0.70710678118654752)
_FT = {"f16": np.float16, "f32": np.float32}

_erf = np.vectorize(math.erf, otypes=[np.float64])
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


# ------------------------------------------------------------------------------------------- float64 activations
def sigmoid64(v):
    v = np.asarray(v, np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-v))


def act64(v, act):
    """the activation in float64 (v float64, finite)"""
    v = np.asarray(v, np.float64)
    if act == "none":
        return v.copy()
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "lrelu":
        return np.where(v > 0, v, SLOPE * v)
    if act == "silu":
        with np.errstate(over="ignore"):
            return v / (1.0 + np.exp(-v))
    if act == "sigmoid":
        return sigmoid64(v)
    assert act == "gelu", act
    return 0.5 * v * _erfc(-v * math.sqrt(0.5))          # 1 + erf(z) = erfc(-z): no cancellation in the negative tail


# -------------------------------------------------------------------------------------------------- the rounding
def rn(y, out):
    """float64 -> the output type, nearest even, fp16 overflow to inf as numpy.astype does it"""
    with np.errstate(over="ignore"):
        return np.asarray(y, np.float64).astype(_FT[out])


def _exact32(v, what):
    v = np.asarray(v, np.float64)
    assert np.isfinite(v).all() and np.array_equal(v.astype(np.float32).astype(np.float64), v), what + " is not exact in float32"
    return v


# ------------------------------------------------------------------------- float32 emulations of the code forms
# form: 'vec4'   x * rcp(1 + exp2(x * -log2e))      scale_bias_act4<f16> and (through __expf) apply_act<f16>
#       'ieee'   x / (1 + expf(-x))                  apply_act<float>, dwconv.hip in both dtypes
# the scalar forms of sigmoid, GELU and LReLU are the same in every kernel.  Primitives (exp2, exp, erf) are the float64
# functions rounded to float32: a correctly rounded instruction.
def _f32(a):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(a).astype(np.float32)


def emulate_act(v, act, form, mutate=None):
    """v float32 -> float32, every step rounded to float32.  mutate: 'log2e_1.44', 'ln2_for_log2e', 'gelu_tanh',
    'slope_0.01', 'slope_f64', 'swap_sigmoid_silu'."""
    v = _f32(v)
    one = np.float32(1)
    if mutate == "swap_sigmoid_silu" and act in ("silu", "sigmoid"):
        act = "sigmoid" if act == "silu" else "silu"
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        if act == "none":
            return v
        if act == "relu":
            return np.where(np.isnan(v), np.float32(0), np.maximum(v, np.float32(0)))      # fmaxf(NaN, 0) = 0
        if act == "lrelu":
            if mutate == "slope_f64":
                return np.where(v > 0, v, _f32(0.1 * v.astype(np.float64)))
            slope = np.float32(0.01 if mutate == "slope_0.01" else 0.1)
            return np.where(v > 0, v, v * slope)
        if act == "silu" and form == "vec4":
            c = np.float32(1.44) if mutate == "log2e_1.44" else (np.float32(math.log(2.0)) if mutate == "ln2_for_log2e" else LOG2E32)
            t = v * -c
            e = _f32(np.exp2(t.astype(np.float64)))
            r = _f32(1.0 / (e + one).astype(np.float64))
            return v * r
        if act in ("silu", "sigmoid"):
            e = _f32(np.exp(-v.astype(np.float64)))
            return (v if act == "silu" else one) / (one + e)
        assert act == "gelu", act
        if mutate == "gelu_tanh":
            v64 = v.astype(np.float64)
            return _f32(0.5 * v64 * (1.0 + np.tanh(math.sqrt(2.0 / math.pi) * (v64 + 0.044715 * v64 ** 3))))
        z = (v * SQRT1_2_32).astype(np.float64)
        e = _f32(np.where(np.isfinite(z), _erf(np.where(np.isfinite(z), z, 0.0)), np.sign(z)))
        return np.float32(0.5) * v * (one + e)


def form_of(act, engine, dw=False):
    return "ieee" if (engine == "f32" or dw) else "vec4"


def emulate(v, act, engine, res=None, res_mode=0, out=None, dw=False, mutate=None):
    """the whole epilogue after the exact pre-activation, in float32 steps, rounded to the output type (default: the
    engine's).  mutate: those of emulate_act, and 'round_v_f16' (pre-activation rounded to fp16 first), 'swap_res_order',
    'skip_tail' (no activation on the last channels beyond a multiple of 8 -- or the last 8), 'ulp_off' (results of one
    binade one fp16 ulp off), 'clamp_f16' (fp16 overflow saturates at 65504)."""
    out = out or engine
    v = _f32(_exact32(v, "v"))
    if mutate == "swap_res_order" and res_mode:
        res_mode = 3 - res_mode
    if mutate == "round_v_f16":
        with np.errstate(over="ignore"):
            v = _f32(v.astype(np.float16))
    m_act = mutate if mutate in ("log2e_1.44", "ln2_for_log2e", "gelu_tanh", "slope_0.01", "slope_f64", "swap_sigmoid_silu") else None
    form = form_of(act, engine, dw)
    with np.errstate(over="ignore", invalid="ignore"):
        pre = v + _f32(res) if res_mode == 2 else v
        y = emulate_act(pre, act, form, m_act)
        if mutate == "skip_tail":
            c = v.shape[1]
            y = y.copy()
            y[:, c - (c % 8 or 8):] = pre[:, c - (c % 8 or 8):]
        if res_mode == 1:
            y = y + _f32(res)
        got = y.astype(_FT[out])
    if mutate == "ulp_off":
        assert out == "f16"
        lo, hi = ULP_OFF_BINADE[act]
        sel = (got >= np.float16(lo)) & (got < np.float16(hi))
        with np.errstate(over="ignore"):
            got = np.where(sel, np.nextafter(got, np.float16(np.inf)), got).astype(np.float16)
    if mutate == "clamp_f16":
        assert out == "f16"
        got = np.where(np.isinf(got), np.copysign(np.float16(65504), got), got).astype(np.float16)
    return got


ULP_OFF_BINADE = {a: (4.0, 8.0) for a in ACTS}
ULP_OFF_BINADE["sigmoid"] = (0.5, 1.0)                   # a sigmoid never reaches 4 .. 8


# ------------------------------------------------------------------------------------------------ the tolerances
_MEASURED = {}


def unit(v, ref):
    """g(v) = u (|ref| + |v| / 2): the unit of the measured bars"""
    return U * (np.abs(ref) + np.abs(np.asarray(v, np.float64)) / 2)


def measured_units(act):
    """max over the whole sweep of |float32 expression on the CPU - float64 reference| / g(v), for 'gelu' / 'sigmoid'"""
    if act not in _MEASURED:
        v = sweep_data()["v"].ravel()
        ref = act64(v, act)
        err = np.abs(emulate_act(v, act, "ieee").astype(np.float64) - ref)
        g = unit(v, ref)
        assert (err[g == 0] == 0).all()
        _MEASURED[act] = float(np.max(np.where(g > 0, err / np.where(g > 0, g, 1.0), 0.0)))
    return _MEASURED[act]


def bar_units(act):
    return max(4.0, 2.0 * measured_units(act))


def tol_act(v, ref, act, engine, dw=False):
    """the derived distance (module docstring) of one activation result from its float64 value `ref` = act64(v)"""
    v, ref = np.asarray(v, np.float64), np.asarray(ref, np.float64)
    if act in ("none", "relu"):
        return np.zeros_like(ref)
    if act == "lrelu":
        return np.zeros_like(ref) if engine == "f32" else U * np.abs(ref)
    if act == "gelu" or (act == "sigmoid" and engine == "f16"):
        assert not dw
        return bar_units(act) * unit(v, ref)
    if act == "silu" and engine == "f16" and not dw:
        return (8.0 + 2.0 * np.abs(v) * sigmoid64(-v)) * U * np.abs(ref) + FLOOR
    assert act in ("silu", "sigmoid"), act
    return 6.0 * U * np.abs(ref) + FLOOR


def bounds(v, act, engine, res=None, res_mode=0, out=None, dw=False):
    """-> (lo, hi, ref, tol): the accepted closed range [lo, hi] in the output type, the float64 value and its tolerance"""
    out = out or engine
    v = _exact32(v, "v")
    if res_mode == 2:
        v = _exact32(v + res, "v + res")
    ref = act64(v, act)
    tol = tol_act(v, ref, act, engine, dw)
    if act == "lrelu" and engine == "f32":               # bit-exact against float32(float32(0.1) * v): the value IS that product
        ref = ref.astype(np.float32).astype(np.float64)
    if res_mode == 1:
        ref = ref + np.asarray(res, np.float64)
        tol = tol + U * np.abs(ref)
    return rn(ref - tol, out), rn(ref + tol, out), ref, tol


def rejected(got, lo, hi):
    """elementwise: got lies outside [lo, hi] (NaN: always; +-0 compare equal)"""
    got = np.asarray(got)
    assert got.dtype == lo.dtype == hi.dtype and got.shape == lo.shape, (got.dtype, lo.dtype, got.shape, lo.shape)
    with np.errstate(invalid="ignore"):
        return ~((got >= lo) & (got <= hi))


# ------------------------------------------------------------------------------------------------------ the sweep
# (bias, scale): v = bias + m * scale, m = 0 .. 511 -- both sides of every threshold, in steps of `scale`
THRESHOLDS = [
    (-4.0, 2.0 ** -6),            # 0 from both sides (+0 at m = 256), the SiLU minimum at coarse steps
    (-0.0, -2.0 ** -6),           # -0 (m = 0) and 0 .. -8
    (-1.3125, 2.0 ** -12),        # -1.2785: the SiLU minimum, fine steps
    (-21.0, 2.0 ** -6),           # -17.33: an fp16 SiLU goes subnormal, then zero
    (-92.0, 2.0 ** -6),           # -88.72, -89 (expf(-v) overflows), -126 ln 2 = -87.34 (exp2 argument 126)
    (85.0, 2.0 ** -6),            # +87.34, +88.72, +89: exp2 argument -126 / -128, expf(-v) denormal
    (-108.0, 2.0 ** -6),          # -103.97
    (100.0, 2.0 ** -6),           # +103.97 = 150 ln 2: exp(-v) leaves the denormals
    (7.0, 2.0 ** -6),             # +11.1: SiLU equals v in fp16
    (65500.0, 2.0 ** -4),         # 65504 the last finite fp16, 65520 the first value that rounds to inf
    (-65532.0, 2.0 ** -4),        # the same on the negative side
    (-9.0, 2.0 ** -5),            # the negative GELU tail: 1 + erff cancels, then is exactly 0 (v < -5.9)
]
SWEEP_MAIN = 124                  # channels that enumerate the finite fp16 values
SWEEP_COUT = 136                  # + the thresholds: 128 + a tail of 8


def _sweep_channels():
    scale, bias = [], []
    for sign in (1.0, -1.0):
        for e in range(-14, 16):
            for half in (0, 1):
                scale.append(sign * 2.0 ** (e - 10))
                bias.append(sign * (1 + half / 2) * 2.0 ** e)
        scale += [sign * 2.0 ** -24, sign * 2.0 ** -24]                       # the subnormal binade
        bias += [sign * 0.0, sign * 512 * 2.0 ** -24]
    assert len(scale) == SWEEP_MAIN
    for b, s in THRESHOLDS:
        bias.append(b)
        scale.append(s)
    assert len(scale) == SWEEP_COUT
    return np.array(scale), np.array(bias)


_SWEEP = {}
SWEEP_CIN = {"wide": 512, "narrow": 64}


def sweep_data(k="wide"):
    """1x1 stride 1, a 16 x 32 image, all-ones weights, acc = p in 0 .. 511 at pixel p -> dict x, w, scale, bias, acc,
    v [1, SWEEP_COUT, 16, 32] float64 (exact in float32).  Channels 0 .. 123 take every finite fp16 value exactly once
    (asserted); the rest walk across the THRESHOLDS.
    k = 'wide': cin 512, x[p, :p] = 1.  k = 'narrow': cin 64, x[p, :p // 8] = 8 and x[p, p // 8] = p % 8 -- the same acc and
    the same v from a K of 128 (fp16) / 256 (fp32) bytes, which the weight-resident and single-shot 1x1 kernels take."""
    if k not in _SWEEP:
        p = np.arange(512)
        cin = SWEEP_CIN[k]
        c = np.arange(cin)[None, :]
        if k == "wide":
            x = (c < p[:, None]).astype(np.int64)                                                    # [pixel, cin]
        else:
            x = np.where(c < p[:, None] // 8, 8, np.where(c == p[:, None] // 8, p[:, None] % 8, 0)).astype(np.int64)
        x = x.T.reshape(1, cin, 16, 32)
        w = np.ones((SWEEP_COUT, cin, 1, 1), np.int64)
        scale, bias = _sweep_channels()
        acc = R.conv(x, w)
        assert np.array_equal(acc[0, 0].ravel(), p) and x.max() <= 8 and x.min() == 0
        v = R.check_regime(acc, scale, bias, None, "none")
        _exact32(v, "the sweep")
        main = v[:, :SWEEP_MAIN].astype(np.float16)
        assert np.array_equal(main.astype(np.float64), v[:, :SWEEP_MAIN]), "the sweep values are fp16 values"
        finite = np.arange(65536, dtype=np.uint32).astype(np.uint16)
        finite = finite[np.isfinite(finite.view(np.float16))]
        assert np.array_equal(np.sort(main.view(np.uint16).ravel()), finite), "every finite fp16 value exactly once"
        _SWEEP[k] = {"x": x, "w": w, "scale": scale, "bias": bias, "acc": acc, "v": v}
    return _SWEEP[k]


def sweep_residual(res_mode):
    """a residual for the sweep, multiples of 2^-3 with |res| <= 64, a quarter of them zero; where the residual is added
    BEFORE the activation it is zero wherever v + res would round in float32 (v + res must stay exact)"""
    v = sweep_data()["v"]
    res = R.residual(v.shape, 91, res_mode)
    res[R._rng(92, res_mode).integers(0, 4, size=v.shape) == 0] = 0.0
    if res_mode == 2:
        s = v + res
        res[s.astype(np.float32).astype(np.float64) != s] = 0.0
        assert (res != 0).mean() > 0.25
    return res


# ---------------------------------------------------------------------------------------------------- the regions
REGION_EDGES = [-104.0, -88.72, -17.33, -1.2785, 11.1, 88.72, 65504.0]
REGION_NAMES = ["v < -104", "[-104, -88.72)", "[-88.72, -17.33)", "[-17.33, -1.2785)", "[-1.2785, 0)", "{0}", "(0, 11.1]",
                "(11.1, 88.72]", "(88.72, 65504]", "> 65504"]
# centre of the channels aimed at each region (bias; region 5: zero weights and a zero bias)
_REGION_BIAS = [-112.0, -96.0, -48.0, -2.25, -0.5, 0.0, 5.0, 40.0, 120.0, 65536.0]


def region_of(v):
    """index into REGION_NAMES per element"""
    v = np.asarray(v, np.float64)
    r = np.full(v.shape, -1)
    r[v < -104.0] = 0
    r[(v >= -104.0) & (v < -88.72)] = 1
    r[(v >= -88.72) & (v < -17.33)] = 2
    r[(v >= -17.33) & (v < -1.2785)] = 3
    r[(v >= -1.2785) & (v < 0)] = 4
    r[v == 0] = 5
    r[(v > 0) & (v <= 11.1)] = 6
    r[(v > 11.1) & (v <= 88.72)] = 7
    r[(v > 88.72) & (v <= 65504.0)] = 8
    r[v > 65504.0] = 9
    assert (r >= 0).all()
    return r


def check_coverage(pre, what):
    """every region holds at least one pre-activation value of the case"""
    seen = set(np.unique(region_of(pre)).tolist())
    missing = [REGION_NAMES[i] for i in range(len(REGION_NAMES)) if i not in seen]
    assert not missing, "%s: no pre-activation in %s" % (what, ", ".join(missing))


def region_scale_bias(cout, acc_scale_log2):
    """channel c aims at region c % 10: scale 2^acc_scale_log2 (2^(.. - 1) on every other round), bias the region's centre
    + a per-round dyadic offset (+ 3 * 2^-13 where |bias| < 64) -> (scale, bias, zero): zero[c]: the channel's weights are all zero (region {0})"""
    c = np.arange(cout)
    reg, rnd = c % 10, c // 10
    scale = 2.0 ** (acc_scale_log2 - (rnd % 2))
    bias = np.array(_REGION_BIAS)[reg] + np.where(reg == 5, 0.0, rnd * 2.0 ** -4)
    bias = bias + np.where((reg >= 2) & (reg <= 7) & (reg != 5), 3 * 2.0 ** -13, 0.0)      # no fp16 value: rounding v early shows
    scale = np.where(reg == 4, 2.0 ** -10, scale)                  # the narrow region [-1.2785, 0)
    return scale, bias, reg == 5


# kind: 'conv' (glsdet_conv2d / _multi / _chain ... on k x k kernels), 'dw' (depthwise; cin = 1), 'grouped' (groups of
# `cin` channels each, 3x3), 'focus' (Focus + 3x3 over a 3-channel image), 'stem' (7x7 stride 2 over a 3-channel image)
RegionCase = namedtuple("RegionCase", "name kind n cin cout k stride dilation h w")


def _rc(kind, n, cin, cout, k, stride, h, w, dilation=1):
    return RegionCase("%s_n%d_ci%d_co%d_k%d_s%d_d%d_%dx%d" % (kind, n, cin, cout, k, stride, dilation, h, w),
                      kind, n, cin, cout, k, stride, dilation, h, w)


REGION_CASES = [
    _rc("conv", 1, 64, 40, 3, 1, 9, 17),             # one pixel past an 8 x 16 tile, a ragged channel tail
    _rc("conv", 1, 128, 136, 3, 1, 13, 21),          # 128 + 8 output rows, past the 10 x 12 / 6 x 21 tiles
    _rc("conv", 3, 64, 64, 3, 1, 8, 16),             # exactly one tile per image
    _rc("conv", 1, 64, 40, 5, 1, 9, 17),
    _rc("conv", 1, 24, 72, 7, 1, 7, 5),
    _rc("conv", 1, 64, 136, 3, 2, 17, 33),
    _rc("conv", 2, 24, 40, 3, 2, 8, 16),
    _rc("conv", 1, 72, 40, 1, 1, 9, 17),             # a 1x1 with a ragged K, for the entry points that take no sweep
    _rc("dw", 2, 1, 24, 3, 1, 9, 17),
    _rc("dw", 1, 1, 40, 7, 2, 17, 33),
    _rc("dw", 1, 1, 72, 3, 2, 13, 21, dilation=3),
    _rc("grouped", 2, 4, 64, 3, 1, 9, 17),
    _rc("grouped", 1, 8, 128, 3, 2, 13, 21),
    _rc("grouped", 1, 16, 256, 3, 1, 8, 16),
    _rc("focus", 2, 12, 32, 3, 1, 16, 32),
    _rc("focus", 1, 12, 40, 3, 1, 18, 34),
    _rc("stem", 2, 3, 64, 7, 2, 16, 32),
    _rc("stem", 1, 3, 64, 7, 2, 37, 29),
]
_REGION = {}


def region_data(case):
    """-> dict x (what the entry point reads: activations [n, C, h, w], or the 3-channel image of 'focus' / 'stem'), w
    (OIHW; grouped: [cout, cin, 3, 3], group g = output channels of input channels g * cin .. ; dw: [C, 1, k, k]), scale,
    bias, acc, v (float64, exact in float32), pad; the regime and the coverage of v are asserted"""
    if case.name in _REGION:
        return _REGION[case.name]
    c = case
    key = (c.n, c.cin, c.cout, c.k, c.stride, c.dilation, c.h, c.w)
    pad = c.dilation * (c.k - 1) // 2
    scale, bias, zero = region_scale_bias(c.cout, {"dw": -3, "stem": -4}.get(c.kind, -5))
    if c.kind == "dw":
        x = R.ternary((c.n, c.cout, c.h, c.w), 101, *key)
        w = R.ternary((c.cout, 1, c.k, c.k), 102, *key)
        w[zero] = 0
        acc = R.conv(x, w, c.stride, pad, c.dilation, depthwise=True)
    elif c.kind == "grouped":
        x = R.ternary((c.n, c.cout, c.h, c.w), 103, *key)
        w = R.ternary((c.cout, c.cin, 3, 3), 104, *key)
        w[zero] = 0
        acc = np.concatenate([R.conv(x[:, g: g + c.cin], w[g: g + c.cin], c.stride, 1)
                              for g in range(0, c.cout, c.cin)], 1)
    elif c.kind in ("focus", "stem"):
        x = R.image((c.n, 3, c.h, c.w), 105, *key)
        w = R.ternary((c.cout, c.cin, c.k, c.k), 106, *key)
        w[zero] = 0
        acc = R.conv(R.focus(x), w, 1, 1) if c.kind == "focus" else R.conv(x, w, 2, 3)
    else:
        x = R.ternary((c.n, c.cin, c.h, c.w), 107, *key)
        w = R.ternary((c.cout, c.cin, c.k, c.k), 108, *key)
        w[zero] = 0
        acc = R.conv(x, w, c.stride, pad)
    v = _exact32(R.check_regime(acc, scale, bias, None, "none"), c.name)
    check_coverage(v, c.name)
    _REGION[case.name] = {"x": x, "w": w, "scale": scale, "bias": bias, "acc": acc, "v": v, "pad": pad}
    return _REGION[case.name]


def region_residual(case, res_mode):
    """multiples of 2^-3, |res| <= 64, a quarter of them zero; v + res stays exact in float32 and covers every region
    (both asserted where the residual is added before the activation)"""
    v = region_data(case)["v"]
    res = R.residual(v.shape, 111, res_mode, case.n, case.cout, case.h, case.w, case.k)
    res[R._rng(112, res_mode, case.cout, case.h).integers(0, 4, size=v.shape) == 0] = 0.0
    if res_mode == 2:
        check_coverage(_exact32(v + res, case.name + " v + res"), case.name + " v + res")
    return res


# ---------------------------------------------------------------------------- a second stage on stored integers
# The two-stage entry points (conv2d_chain, bottleneck, focus_conv_down) feed a STORED first result to a second conv.  An
# activation output is not exact, so the first stage is given scale 1, bias 0 and relu / none: it stores small integers
# (exact in fp16), every partial sum of the second conv is an integer below 2^24 -- exact in any order -- and the second
# pre-activation is exact in float32 again.
def second_stage(y_int, cout2, k, stride, key, cin_lo=0, cin2=None):
    """y_int: integer-valued stored first stage [n, c, h, w]; a k x k conv (pad k // 2) with ternary weights over channels
    [cin_lo, cin_lo + cin2), region scales and biases -> dict w, scale, bias, v (exact in float32, every region covered)"""
    y_int = np.asarray(y_int)
    assert np.array_equal(y_int, np.rint(y_int)) and np.abs(y_int).max() <= 2048, "the first stage must be exact in fp16"
    cin2 = cin2 or y_int.shape[1] - cin_lo
    x2 = y_int[:, cin_lo: cin_lo + cin2].astype(np.int64)
    w = R.ternary((cout2, cin2, k, k), 201, cout2, cin2, k, stride, *key)
    scale, bias, zero = region_scale_bias(cout2, -5)
    w[zero] = 0
    acc = R.conv(x2, w, stride, k // 2)
    assert R.abs_sum(x2, w, stride, k // 2).max() < 2 ** 24
    v = acc * scale[None, :, None, None] + bias[None, :, None, None]
    v32 = acc.astype(np.float32) * scale.astype(np.float32)[None, :, None, None] + bias.astype(np.float32)[None, :, None, None]
    assert np.array_equal(v32.astype(np.float64), v), "the float32 epilogue of the second stage rounds"
    check_coverage(v, "second stage")
    return {"w": w, "scale": scale, "bias": bias, "acc": acc, "v": v}


CHAIN_CASE = REGION_CASES[2]                              # 3 x 64 -> 64, 3x3, 8 x 16: also the multi / gnstats problem
BNECK_SHAPE = (2, 64, 32, 9, 17)                          # n, cin0, hidden = out channels, h, w
_TWO = {}


def chain_data():
    """-> dict x (that of CHAIN_CASE), w1 (3x3, 64 channels; scale 1, bias 0, relu), y1 (the stored integers), and the
    1x1 second stage over all 64 channels -> 40: w, scale, bias, v"""
    if "chain" not in _TWO:
        x = region_data(CHAIN_CASE)["x"]
        w1 = R.ternary((64, CHAIN_CASE.cin, 3, 3), 211)
        y1 = np.maximum(R.conv(x, w1, 1, 1), 0)
        _TWO["chain"] = dict(second_stage(y1, 40, 1, 1, (211,)), x=x, w1=w1, y1=y1)
    return _TWO["chain"]


def bneck_data(act0):
    """-> dict x, w1 (1x1; scale 1, bias 0, act0 = relu / none), and the 3x3 second stage on the hidden integers"""
    if ("bneck", act0) not in _TWO:
        n, cin0, cm, h, w = BNECK_SHAPE
        x = R.ternary((n, cin0, h, w), 221)
        w1 = R.ternary((cm, cin0, 1, 1), 222)
        acc1 = R.conv(x, w1)
        hid = np.maximum(acc1, 0) if act0 == "relu" else acc1
        _TWO[("bneck", act0)] = dict(second_stage(hid, cm, 3, 1, (223, act0 == "relu")), x=x, w1=w1)
    return _TWO[("bneck", act0)]


def bneck_residual(shape, res_mode):
    res = R.residual(shape, 224, res_mode)
    res[R._rng(225, res_mode).integers(0, 4, size=shape) == 0] = 0.0
    return res


def focus_down_data(case, cout2):
    """-> dict w1 (the 32-channel Focus stem conv; scale 1, bias 0, relu) and the 3x3 stride-2 second stage"""
    if ("down", case.name, cout2) not in _TWO:
        img = region_data(case)["x"]
        w1 = R.ternary((32, 12, 3, 3), 231, case.h)
        y1 = np.maximum(R.conv(R.focus(img), w1, 1, 1), 0)
        _TWO[("down", case.name, cout2)] = dict(second_stage(y1, cout2, 3, 2, (232, case.h)), w1=w1)
    return _TWO[("down", case.name, cout2)]


# ------------------------------------------------------------------------------------------------ glsdet_csp_fused
# The fused CSPLayer (fp16, SiLU compiled in) keeps main, short, h and main' in LDS: only y is visible.  Its first three
# epilogues are therefore given pre-activations at which an fp16 SiLU is EXACT -- v >= 16 ("on" channels: silu(v) = v to
# 2e-6, far below half an fp16 ulp) or v <= -32 ("off" channels: |silu(v)| < 1e-12 rounds to zero) -- so that the values the
# last conv reads are known exactly, and the last epilogue gets the regions.  A first-stage site that applied no activation,
# a leaky ReLU or a sigmoid would change those values and with them y; SiLU and ReLU cannot be told apart there.
CSP_SHAPE = (2, 9, 17)            # n, h, w: past an 8 x 16 tile in both directions


def _saturated_silu(v, what):
    v = np.asarray(v, np.float64)
    assert ((v >= 16) | (v <= -32)).all() and np.abs(v).max() <= 256, what
    s = np.where(v > 0, v, 0.0)
    assert np.array_equal(s.astype(np.float16).astype(np.float64), s), what + ": not fp16 values"
    assert (np.abs(act64(v, "silu") - s) < 2.0 ** -6 * np.spacing(np.maximum(s, 2.0 ** -14).astype(np.float16)).astype(np.float64)).all()
    return s


def _sparse01(shape, ones, *key):
    """0 / 1 weights [cout, cin, k, k] with `ones` ones per output channel"""
    cout = shape[0]
    w = np.zeros((cout, int(np.prod(shape[1:]))), np.int64)
    r = R._rng(301, *key)
    for co in range(cout):
        w[co, r.permutation(w.shape[1])[:ones]] = 1
    return w.reshape(shape)


def csp_data(shortcut):
    """-> dict x [n, 64, h, w] (0 / 1), convs: the four (w, scale, bias) of conv1|conv2, m.0.conv1, m.0.conv2, conv3, and v:
    the exact pre-activation of conv3 (every region covered)"""
    if ("csp", shortcut) in _TWO:
        return _TWO[("csp", shortcut)]
    n, h, w = CSP_SHAPE
    x = R._rng(302).integers(0, 2, size=(n, 64, h, w)).astype(np.int64)

    def stage(inp, wt, pad, off_every, scale_on):
        cout = wt.shape[0]
        off = np.arange(cout) % off_every == off_every - 1                     # the "off" channels
        scale = np.where(off, -1.0, scale_on)
        bias = np.where(off, -32.0, 16.0)
        acc = R.conv(np.asarray(inp, np.float64), wt.astype(np.float64), 1, pad)
        return acc * scale[None, :, None, None] + bias[None, :, None, None], scale, bias

    w12 = _sparse01((64, 64, 1, 1), 24, 1)
    v12, s12, b12 = stage(x, w12, 0, 4, 1.0)
    cat = _saturated_silu(v12, "conv1 | conv2")
    main, short = cat[:, :32], cat[:, 32:]
    wm1 = _sparse01((32, 32, 1, 1), 2, 2)
    vh, sm1, bm1 = stage(main, wm1, 0, 4, 0.5)
    hid = _saturated_silu(vh, "m.0.conv1")
    wm2 = _sparse01((32, 32, 3, 3), 2, 3)
    vm, sm2, bm2 = stage(hid, wm2, 1, 4, 0.5)
    main2 = _saturated_silu(vm, "m.0.conv2")
    if shortcut:
        main2 = main2 + main
        assert np.array_equal(main2.astype(np.float16).astype(np.float64), main2) and main2.max() <= 512
    cat2 = np.concatenate((main2, short), 1)
    w3 = np.zeros((64, 64), np.int64)                                          # +1 on one input, -1 on another
    r = R._rng(303, shortcut)
    for co in range(64):
        a, b = r.permutation(64)[:2]
        w3[co, a], w3[co, b] = 1, -1
    scale3, bias3, zero = region_scale_bias(64, -3)
    w3[zero] = 0
    w3 = w3.reshape(64, 64, 1, 1)
    acc3 = R.conv(cat2, w3.astype(np.float64))
    v3 = _exact32(acc3 * scale3[None, :, None, None] + bias3[None, :, None, None], "conv3 of the CSPLayer")
    v32 = acc3.astype(np.float32) * scale3.astype(np.float32)[None, :, None, None] + bias3.astype(np.float32)[None, :, None, None]
    assert np.array_equal(v32.astype(np.float64), v3)
    check_coverage(v3, "conv3 of the CSPLayer")
    _TWO[("csp", shortcut)] = {"x": x, "v": v3, "convs": [(w12, s12, b12), (wm1, sm1, bm1), (wm2, sm2, bm2), (w3, scale3, bias3)]}
    return _TWO[("csp", shortcut)]
