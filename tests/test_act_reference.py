"""CPU tests of tests/act_reference.py, the float64 reference tests/test_act_exact.py holds the activation epilogues to.

Two things are proved here, without a GPU:

  1. the bars are met by an honest implementation: a numpy float32 emulation of each code form (x * rcp(1 + exp2(x *
     -log2e)), x / (1 + expf(-x)), the scalar sigmoid / GELU / LReLU) passes every case with ZERO rejections;
  2. the reference has teeth: each wrong epilogue a kernel could plausibly implement (MUTANTS) is rejected on EVERY case
     that has the relevant feature -- asserted per case, as tests/test_conv_reference.py does.

The measured CPU maxima the GELU / sigmoid bars are derived from (tests/act_reference.py::measured_units, units of
u (|ref| + |v| / 2) over the whole sweep; asserted below): GELU 1.125, sigmoid 1.981 -- both bars are therefore the floor of
4 units."""
import numpy as np
import pytest

from tests import act_reference as A
from tests import conv_reference as R

# a situation: (case or None for the sweep, residual mode)
SITS = [(None, m) for m in (0, 1, 2)]
SITS += [(c, m) for c in A.REGION_CASES if c.kind == "conv" for m in (0, 1, 2)]
SITS += [(c, 0) for c in A.REGION_CASES if c.kind != "conv"]
_ids = lambda s: "%s_r%d" % (s[0].name if s[0] else "sweep", s[1])
_B = {}


def _sit(sit):
    """-> (data dict, res, dw, acts)"""
    case, m = sit
    d = A.sweep_data() if case is None else A.region_data(case)
    res = None if m == 0 else (A.sweep_residual(m) if case is None else A.region_residual(case, m))
    dw = case is not None and case.kind == "dw"
    return d, res, dw, (A.DW_ACTS if dw else A.ACTS)


def _bounds(sit, act, engine):
    key = (_ids(sit), act, engine)
    if key not in _B:
        d, res, dw, _ = _sit(sit)
        _B[key] = A.bounds(d["v"], act, engine, res, sit[1], dw=dw)
    return _B[key]


def test_the_cases_cover_what_they_claim():
    names = [c.name for c in A.REGION_CASES]
    assert len(set(names)) == len(names)
    conv = [c for c in A.REGION_CASES if c.kind == "conv"]
    assert {c.k for c in conv} == {1, 3, 5, 7} and {c.stride for c in conv} == {1, 2}
    assert {(c.h, c.w) for c in conv} >= {(7, 5), (8, 16), (9, 17)}
    assert {c.cout for c in conv} >= {40, 136}                              # a tail beyond every channel tile
    assert {c.kind for c in A.REGION_CASES} == {"conv", "dw", "grouped", "focus", "stem"}
    assert {(c.k, c.stride, c.dilation) for c in A.REGION_CASES if c.kind == "dw"} == {(3, 1, 1), (7, 2, 1), (3, 2, 3)}
    assert all(c.n * c.h * c.w <= 512 * 3 for c in A.REGION_CASES)


def test_the_sweep_is_exhaustive_and_crosses_every_threshold():
    d = A.sweep_data()                                                      # asserts: every finite fp16 value exactly once
    v = d["v"]
    assert v.shape == (1, A.SWEEP_COUT, 16, 32) and A.SWEEP_COUT % 128 == 8
    assert np.abs(d["acc"]).max() == 511 and d["acc"].min() == 0
    n = A.sweep_data("narrow")                                              # the same values from a K of 64 channels
    assert n["x"].shape == (1, 64, 16, 32) and np.array_equal(n["v"], v) and np.array_equal(n["acc"], d["acc"])
    m, e = np.frexp(np.abs(d["scale"]))
    assert (m == 0.5).all(), "scales are powers of two"
    thr = v[0, A.SWEEP_MAIN:].reshape(len(A.THRESHOLDS), -1)
    for t in (0.0, -1.2785, -17.33, -88.72, 88.72, -89.0, 89.0, -103.97, 103.97, -126 * np.log(2), 126 * np.log(2), 11.1,
              65504.0, 65519.99, -65504.0, -65519.99, -5.9):
        assert any((row < t).any() and (row > t).any() for row in thr), "no channel crosses %r" % t
    assert (v == 0).sum() >= 3 and np.signbit(v[v == 0]).any() and not np.signbit(v[v == 0]).all()        # +0 and -0
    assert (thr == 65520.0).any() and (thr == 65504.0).any() and (thr == -65520.0).any()
    A.check_coverage(v, "the sweep")
    for mode in (1, 2):
        res = A.sweep_residual(mode)
        assert np.array_equal(res * 8, np.rint(res * 8)) and np.abs(res).max() <= 64 and (res != 0).mean() > 0.25


@pytest.mark.parametrize("case", A.REGION_CASES, ids=lambda c: c.name)
def test_region_cases_are_exact_and_cover_every_region(case):
    d = A.region_data(case)                                                 # asserts the regime and the coverage of v
    m, _ = np.frexp(d["scale"])
    assert (m == 0.5).all()
    assert np.array_equal(d["bias"] * 8192, np.rint(d["bias"] * 8192))
    assert np.abs(d["acc"]).max() <= R.ACC_MAX
    A.check_coverage(d["v"], case.name)
    if case.kind == "conv":
        for mode in (1, 2):
            res = A.region_residual(case, mode)                             # asserts exactness and coverage of v + res
            assert np.array_equal(res * 8, np.rint(res * 8)) and np.abs(res).max() <= 64
        A.check_coverage(d["v"] + A.region_residual(case, 2), case.name)


def test_second_stages_on_stored_integers_are_exact_and_cover_every_region():
    """chain, bottleneck and focus_conv_down: the builders assert exactness and coverage; with a residual too"""
    assert A.CHAIN_CASE.n == 3 and A.CHAIN_CASE.k == 3 and A.CHAIN_CASE.cout == 64
    c = A.chain_data()
    assert c["v"].shape == (3, 40, 8, 16) and c["y1"].min() == 0 and np.abs(c["acc"]).max() < 2 ** 24
    for act0 in ("relu", "none"):
        b = A.bneck_data(act0)
        assert b["v"].shape == (A.BNECK_SHAPE[0], A.BNECK_SHAPE[2]) + A.BNECK_SHAPE[3:]
        for mode in (1, 2):
            res = A.bneck_residual(b["v"].shape, mode)
            A.bounds(b["v"], "silu", "f16", res, mode)                          # asserts v + res exact
        A.check_coverage(b["v"] + A.bneck_residual(b["v"].shape, 2), "bottleneck v + res")
    for case in A.REGION_CASES:
        if case.kind == "focus":
            for cout2 in (40, 64):
                A.focus_down_data(case, cout2)


@pytest.mark.parametrize("shortcut", [True, False])
def test_csp_layer_data_saturates_the_inner_silus_and_covers_every_region(shortcut):
    d = A.csp_data(shortcut)                                                # asserts saturation, exactness, coverage
    assert d["v"].shape == (A.CSP_SHAPE[0], 64) + A.CSP_SHAPE[1:]
    assert [c[0].shape for c in d["convs"]] == [(64, 64, 1, 1), (32, 32, 1, 1), (32, 32, 3, 3), (64, 64, 1, 1)]
    for wt, sc, bi in d["convs"][:3]:                                       # "on" and "off" channels at every inner site
        assert set(np.unique(bi)) == {-32.0, 16.0} and (sc[bi < 0] == -1).all()
    # a site without its activation would feed conv3 other values: the off channels are far from zero before the SiLU
    x = d["x"].astype(np.float64)
    w12, s12, b12 = d["convs"][0]
    v12 = R.conv(x, w12.astype(np.float64)) * s12[None, :, None, None] + b12[None, :, None, None]
    assert (v12[:, b12 < 0] <= -32).all() and (v12[:, b12 > 0] >= 16).all()
    honest = A.emulate(d["v"], "silu", "f16")
    lo, hi, _, _ = A.bounds(d["v"], "silu", "f16")
    assert not A.rejected(honest, lo, hi).any()


def test_measured_bars():
    """the CPU maxima of the float32 expressions, in units u (|ref| + |v| / 2) over the whole sweep (this file's docstring
    and DESIGN.md record them)"""
    g, s = A.measured_units("gelu"), A.measured_units("sigmoid")
    print("measured CPU maxima: gelu %.3f units, sigmoid %.3f units" % (g, s))
    assert 0.5 < g < 2.0 and 0.5 < s < 2.0, (g, s)
    assert A.bar_units("gelu") == 4.0 and A.bar_units("sigmoid") == 4.0


def test_float64_activations_at_known_points():
    v = np.array([0.0, 1.0, -1.0, -1.2784645, 20.0, -20.0, -800.0, 800.0])
    assert np.allclose(A.act64(v, "silu")[:4], [0, 0.7310585786300049, -0.2689414213699951, -0.27846454276107], rtol=1e-9, atol=0)
    assert A.act64(v, "silu")[6] == 0 and A.act64(v, "sigmoid")[6] == 0 and A.act64(v, "sigmoid")[7] == 1
    assert np.allclose(A.act64(v, "gelu")[:3], [0, 0.8413447460685429, -0.15865525393145707], rtol=1e-14, atol=0)
    assert np.isclose(A.act64(v, "gelu")[5], -20.0 * 2.753624118606234e-89, rtol=1e-6, atol=0)        # no cancellation
    assert A.act64(v, "lrelu")[2] == -float(np.float32(0.1)) and A.act64(v, "lrelu")[1] == 1.0
    assert np.array_equal(A.act64(v, "relu"), np.maximum(v, 0)) and np.array_equal(A.act64(v, "none"), v)


# ------------------------------------------------------------------------------------------- the honest emulations
@pytest.mark.parametrize("sit", SITS, ids=_ids)
def test_honest_float32_emulations_meet_every_bar(sit):
    d, res, dw, acts = _sit(sit)
    for engine in A.ENGINES:
        for act in acts:
            lo, hi, ref, tol = _bounds(sit, act, engine)
            got = A.emulate(d["v"], act, engine, res, sit[1], dw=dw)
            bad = A.rejected(got, lo, hi)
            assert not bad.any(), "%s %s: %d rejections, first v = %r got %r range [%r, %r]" % (
                engine, act, bad.sum(), d["v"][bad][0], got[bad][0], lo[bad][0], hi[bad][0])
            assert not np.isnan(got).any()


# -------------------------------------------------------------------------------------------------- the mutants
# name -> applies(act, engine, res_mode, dw)
MUTANTS = {
    "log2e_1.44": lambda a, e, m, dw: a == "silu" and e == "f16" and not dw,
    "ln2_for_log2e": lambda a, e, m, dw: a == "silu" and e == "f16" and not dw,
    "gelu_tanh": lambda a, e, m, dw: a == "gelu",
    "slope_0.01": lambda a, e, m, dw: a == "lrelu",
    "slope_f64": lambda a, e, m, dw: a == "lrelu" and e == "f32",
    "swap_sigmoid_silu": lambda a, e, m, dw: a in ("silu", "sigmoid") and not (dw and a == "sigmoid"),
    "act_before_bias": lambda a, e, m, dw: a != "none" and m == 0,
    "round_v_f16": lambda a, e, m, dw: e == "f32" or m != 0 or a not in ("none", "relu"),
    "swap_res_order": lambda a, e, m, dw: m != 0 and a != "none",
    "skip_tail": lambda a, e, m, dw: a != "none",
    "ulp_off": lambda a, e, m, dw: e == "f16",
    "clamp_f16": lambda a, e, m, dw: e == "f16" and a != "sigmoid",
}


def _mutant(name, sit, act, engine):
    d, res, dw, _ = _sit(sit)
    if name == "act_before_bias":
        sc, bi = d["scale"][None, :, None, None], d["bias"][None, :, None, None]
        y = A.emulate_act(A._f32(d["acc"] * sc), act, A.form_of(act, engine, dw)) + A._f32(bi)
        with np.errstate(over="ignore"):
            return y.astype(A._FT[engine])
    return A.emulate(d["v"], act, engine, res, sit[1], dw=dw, mutate=name)


@pytest.mark.parametrize("name", list(MUTANTS))
def test_every_mutant_is_rejected_on_every_case_that_has_the_feature(name):
    seen = 0
    for sit in SITS:
        d, res, dw, acts = _sit(sit)
        for engine in A.ENGINES:
            for act in acts:
                if not MUTANTS[name](act, engine, sit[1], dw):
                    continue
                lo, hi, _, _ = _bounds(sit, act, engine)
                if name == "ulp_off":                  # the feature: honest results in the binade (every case has some)
                    b = A.ULP_OFF_BINADE[act]
                    honest = A.emulate(d["v"], act, engine, res, sit[1], dw=dw)
                    assert ((honest >= b[0]) & (honest < b[1])).any(), "%s %s %s: no result in %r" % (_ids(sit), engine, act, b)
                if name == "clamp_f16":                # the feature: a result that overflows fp16 (every case has some)
                    assert np.isinf(hi).any(), "%s %s %s: no fp16 overflow" % (_ids(sit), engine, act)
                bad = A.rejected(_mutant(name, sit, act, engine), lo, hi)
                assert bad.any(), "%s is invisible on %s (%s engine, %s)" % (name, _ids(sit), engine, act)
                seen += 1
    assert seen >= 8, (name, seen)


# ------------------------------------------------------------------------------------------ the interval acceptance
@pytest.mark.parametrize("act", A.ACTS)
def test_a_neighbouring_fp16_value_is_rejected_wherever_the_tolerance_is_small(act):
    """fp16 engine, the exhaustive channels of the sweep: wherever tol < ulp(ref) / 4 the accepted range holds at most two
    adjacent fp16 values, rn(ref) is one of them and at least one of its neighbours is rejected; for a majority of
    the sweep BOTH neighbours are rejected (the range is the single value rn(ref))"""
    sit = (None, 0)
    lo, hi, ref, tol = (a[:, :A.SWEEP_MAIN] for a in _bounds(sit, act, "f16"))
    c = A.rn(ref, "f16")
    fin = np.isfinite(c)
    with np.errstate(over="ignore"):
        up, dn = np.nextafter(c, np.float16(np.inf)), np.nextafter(c, np.float16(-np.inf))
    ulp = np.where(fin, (up.astype(np.float64) - dn.astype(np.float64)) / 2, np.inf)
    ulp = np.where(np.isinf(up) | np.isinf(dn), 32.0, ulp)                     # the last finite binade
    tight = fin & (tol < ulp / 4)
    assert tight.sum() > tight.size // 2, "%d of %d" % (tight.sum(), tight.size)
    assert not A.rejected(c, lo, hi)[tight].any()
    r_up, r_dn = A.rejected(up, lo, hi), A.rejected(dn, lo, hi)
    assert (r_up | r_dn)[tight].all()
    steps = (hi.view(np.int16).astype(np.int32) - lo.view(np.int16).astype(np.int32))[tight & (lo > 0)]
    assert steps.max(initial=0) <= 1
    both = tight & r_up & r_dn
    assert both.sum() > tight.size // 2, "%d of %d" % (both.sum(), tight.size)


def test_acceptance_special_values():
    z = np.zeros(4, np.float16)
    got = np.array([0.0, -0.0, np.nan, 6e-8], np.float16)
    assert A.rejected(got, z, z).tolist() == [False, False, True, True]          # +-0 equal, NaN never
    inf = np.full(2, np.inf, np.float16)
    assert A.rejected(np.array([np.inf, 65504], np.float16), inf, inf).tolist() == [False, True]
    lo, hi, _, _ = A.bounds(np.array([65519.9375, 65520.0, -65520.0]), "none", "f16")
    assert lo.tolist() == [65504.0, np.inf, -np.inf] and hi.tolist() == lo.tolist()
    lo, hi, _, _ = A.bounds(np.array([-3.0]), "lrelu", "f32")
    assert lo[0] == hi[0] == np.float32(-3.0) * np.float32(0.1)
