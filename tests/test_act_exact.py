"""The activation epilogues of the conv family (glsdet_amd/csrc/conv*.hip, stem.hip, dwconv.hip) against the float64
reference tests/act_reference.py, in both engines and for every activation an entry point accepts.

The pre-activation of every case is exact in float32 (tests/act_reference.py asserts it), so the only error left is the
activation's own.  A result is accepted when it lies in the closed range [rn(ref - tol), rn(ref + tol)] of the output
type, with the DERIVED tol of that module: 0 for none / relu, one float32 rounding for leaky ReLU, a few u of |ref| for
SiLU and the f32 sigmoid, a bar measured on the CPU (never on the kernel) for GELU and the fp16 sigmoid.  No element is
skipped; every destination sits in a sentinel-filled buffer that is compared whole (nothing outside it may change), every
input in a NaN-filled one.

Measured on the CPU (float32 numpy expression, whole sweep, units u (|ref| + |v| / 2)): GELU 1.125, sigmoid 1.981; both
bars are therefore 4 units.  The GPU maxima are printed (-s) by test_conv2d_sweep_* and recorded in DESIGN.md.

  conv2d       every tile_hint of tests/test_hip_fuzz.py::HINTS that accepts the problem: the exhaustive 1x1 sweep (every
               finite fp16 value + the thresholds; three forms with the same values -- K of 512 channels, K of 64
               channels for the weight-resident kernels, 32 output channels per launch for the 32-row tiles) and the
               region cases (k x k, stride 2), each with the three residual modes, into dense and channel-slice (sweep) /
               window (regions) destinations
  bit identity every hint = hint 0, and the 4-vector path (no residual) = the scalar path (GLSDET_ACT_RES_FIRST with an
               all-zero residual), at the sweep.  Zeros are compared as zeros: v + 0 turns -0 into +0 on the scalar path.
  non-finite   bias = +inf, -inf, NaN: what the same float32 expression gives in numpy; relu(NaN) = 0 as
               include/glsdet_hip.h states
  the other entry points, each with every activation its validation code accepts (and a refusal for the others):
               conv2d_multi (grouped and batched), conv2d_chain (first and second activation), bottleneck (second conv,
               with and without residual; the first conv's result is never stored: relu / none keep it exact),
               conv2d_grouped, conv2d_gnstats, focus_conv, focus_conv_down (second conv), resnet_stem,
               resnet_stem_pool (ReLU only), dwconv2d and dwconv2d_dilated (codes 0 .. 3), csp_fused (SiLU only: the
               fourth epilogue site over the regions; the three inner sites, whose results stay in LDS, at values where
               an fp16 SiLU is exact)
A second stage that consumes a stored first stage reads INTEGERS (first stage: scale 1, bias 0, relu / none), so that its
pre-activation is exact again (tests/act_reference.py::second_stage)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import act_reference as A
from tests import conv_reference as R
from tests.test_conv_exact import (MODES, MULTI_TILES, NAN, SENTINEL, _FT, _TT, Placed, _bits, _desc, _image, _pack, _scratch,
                                   _stream, engines)  # noqa: F401  (engines: the module-scoped fixture)
from tests.test_hip_fuzz import HINTS

pytestmark = pytest.mark.gpu

CONV_REGION = [c for c in A.REGION_CASES if c.kind == "conv"]
_kind = lambda k: [c for c in A.REGION_CASES if c.kind == k]
_WANT = {}


def _nhwc(a):
    return np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))


def _want(key, v, act, mode, res=None, res_mode=0, dw=False):
    """the accepted range (NHWC, output type) of one problem, computed once and shared"""
    k = (key, act, mode, res_mode)
    if k not in _WANT:
        lo, hi, ref, _ = A.bounds(v, act, mode, res, res_mode, dw=dw)
        _WANT[k] = (_nhwc(lo), _nhwc(hi), _nhwc(ref))
    return _WANT[k]


def _verdict(dst, lo, hi, index=None):
    """one synchronize + one download -> (the destination's values [n, h, w, c], None or a message): nothing outside
    the destination changed, every element inside lies in [lo, hi]"""
    torch.cuda.synchronize()
    got = dst.full.buf.view(_TT[dst.dt]).cpu().numpy()
    index = index or dst.index
    inside = np.zeros(got.shape, bool)
    dst.grid(inside)[index] = True
    outside = int(((got != dst.host) & ~inside).sum())
    vals = np.ascontiguousarray(dst.grid(got)[index]).view(_FT[dst.dt])
    bad = A.rejected(vals, lo, hi)
    if not bad.any() and not outside:
        return vals, None
    msg = "%d of %d elements outside their range, %d elements OUTSIDE the destination changed" % (int(bad.sum()), bad.size, outside)
    if bad.any():
        i = tuple(int(j[0]) for j in np.nonzero(bad))
        msg += "; first at (n, h, w, c) = %s: got %r, range [%r, %r]" % (i, vals[i], lo[i], hi[i])
    return vals, msg


def _canon(vals):
    """bits with every zero as +0"""
    it = np.int16 if vals.dtype == np.float16 else np.int32
    return np.where(vals == 0, it(0), vals.view(it))


def _res_in(eng, mode, res, shape):
    n, c, h, w = shape
    return Placed(eng, "ring", n, h, w, c, mode, NAN[mode]).put(res).upload()


def _units(vals, ref, v_nhwc):
    """smallest tolerance that would accept every finite result, in units u (|ref| + |v| / 2) (GELU / sigmoid: printed,
    recorded in DESIGN.md).  fp32 results: |got - ref|; fp16 results: the distance from ref to the values that round to
    got (the rounding to fp16 itself is not the activation's error)."""
    g = A.unit(v_nhwc, ref)
    got = vals.astype(np.float64)
    if vals.dtype == np.float16:
        with np.errstate(over="ignore"):
            up = np.nextafter(vals, np.float16(np.inf)).astype(np.float64)
            dn = np.nextafter(vals, np.float16(-np.inf)).astype(np.float64)
        up, dn = np.where(np.isinf(up), 65536.0, up), np.where(np.isinf(dn), -65536.0, dn)
        err = np.maximum(0.0, np.maximum((got + dn) / 2 - ref, ref - (got + up) / 2))
    else:
        err = np.abs(got - ref)
    ok = (g > 0) & np.isfinite(vals)
    return float((err[ok] / g[ok]).max())


# ============================================================================================== (a) glsdet_conv2d
def _hints(launch, dst, lo, hi, tag, failures, hints=HINTS, base=None, must=(0, 1)):
    """launch(hint) on every hint that accepts the problem (GlsdetError = refused): the range check, and the same bits
    as the first hint that ran (or `base`) -> (hints that ran, {hint: values})"""
    from glsdet_amd._lib import GlsdetError
    ran, first, out = [], base, {}
    for hint in hints:
        dst.upload()
        try:
            launch(hint)
        except GlsdetError:
            assert hint not in must, "the automatic choice and the generic kernel must accept every problem"
            continue
        vals, msg = _verdict(dst, lo, hi)
        ran.append(hint)
        out[hint] = vals
        if msg:
            failures.append("%s hint %#x: %s" % (tag, hint, msg))
        if first is None:
            first = _canon(vals)
        else:
            diff = _canon(vals) != first
            if diff.any():
                failures.append("%s hint %#x: %d elements differ in bits from the first result" % (tag, hint, int(diff.sum())))
    return ran, out


def _conv_hints(eng, xin, pk, stride, pad, act, dst, rin, res_first, lo, hi, tag, failures, base=None):
    return _hints(lambda hint: eng.conv(xin.view, pk, stride, pad, act, out=dst.view, res=rin.view if rin else None,
                                        tile_hint=hint, res_first=res_first), dst, lo, hi, tag, failures, base=base)


# Three forms of the sweep, all with the same pre-activations (and therefore the same bits on every variant):
#   wide     cin 512, one launch of 136 channels: the kernels that stream K
#   narrow   cin 64 (K = 128 / 256 bytes), one launch: + the weight-stationary, weight-resident and single-shot 1x1 kernels
#   rows32   cin 64, five launches of <= 32 output channels into channel slices of the destination: + the 32-row tiles
SWEEP_FORMS = ["wide", "narrow", "rows32"]


class Sweep:
    def __init__(self, eng, mode, form, scale=None, bias=None, cout=None):
        k = "wide" if form == "wide" else "narrow"
        d = A.sweep_data(k)
        self.eng, self.cin, self.cout = eng, A.SWEEP_CIN[k], cout or A.SWEEP_COUT
        scale = d["scale"] if scale is None else scale
        bias = d["bias"] if bias is None else bias
        self.xin = Placed(eng, "ring", 1, 16, 32, self.cin, mode, NAN[mode]).put(d["x"]).upload()
        step = 32 if form == "rows32" else self.cout
        self.groups = [(c0, min(c0 + step, self.cout)) for c0 in range(0, self.cout, step)]
        self.packs = [_pack(eng, d["w"][c0:c1], scale[c0:c1], bias[c0:c1], self.cin) for c0, c1 in self.groups]

    def launch(self, hint, act, dst, rin=None, res_first=False):
        whole = len(self.groups) == 1
        for (c0, c1), pk in zip(self.groups, self.packs):
            self.eng.conv(self.xin.view, pk, 1, 0, act, out=dst.view if whole else dst.view.channels(c0, c1),
                          res=None if rin is None else (rin.view if whole else rin.view.channels(c0, c1)),
                          tile_hint=hint, res_first=res_first)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", A.ACTS)
def test_conv2d_sweep_every_variant_every_residual_mode(engines, mode, act):
    """every finite fp16 value and every threshold as the pre-activation, on every hint that takes one of the three
    forms of the 1x1; every result has the bits of the first one"""
    eng = engines[mode]
    v = A.sweep_data()["v"]
    failures, worst, seen = [], 0.0, set()
    with _scratch(eng):
        sweeps = [Sweep(eng, mode, f) for f in SWEEP_FORMS]
        for rm in (0, 1, 2):
            res = A.sweep_residual(rm) if rm else None
            rin = _res_in(eng, mode, res, v.shape) if rm else None
            lo, hi, ref = _want("sweep", v, act, mode, res, rm)
            for kind in ("dense", "slice"):
                dst = Placed(eng, kind, 1, 16, 32, A.SWEEP_COUT, mode, SENTINEL[mode])
                base, done = None, set()
                for form, sw in zip(SWEEP_FORMS, sweeps):
                    ran, out = _hints(lambda h: sw.launch(h, act, dst, rin, rm == 2), dst, lo, hi,
                                      "%s, res mode %d, %s:" % (form, rm, kind), failures, base=base,
                                      hints=[h for h in HINTS if form != "rows32" or h not in done], must=(0, 1) if form != "rows32" else (1,))
                    assert len(ran) >= (3 if form != "rows32" else 1), (form, ran)
                    base = _canon(out[ran[0]]) if base is None else base
                    done |= set(ran)
                    if rm == 0 and act in ("gelu", "sigmoid"):
                        worst = max([worst] + [_units(o, ref, _nhwc(v)) for o in out.values()])
                seen |= done
        print("sweep %s %s ran on %s" % (mode, act, " ".join("%#x" % h for h in sorted(seen))))
        if act in ("gelu", "sigmoid"):
            print("measured GPU maximum, %s engine, %s: %.3f units (bar %.1f)" % (mode, act, worst, A.bar_units(act)))
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", CONV_REGION, ids=lambda c: c.name)
def test_conv2d_regions_every_variant_every_activation(engines, mode, case):
    """k x k, strided and ragged shapes: every region of the value line under every activation and residual mode"""
    eng = engines[mode]
    d = A.region_data(case)
    shape = d["v"].shape
    failures, seen = [], set()
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
        pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
        for rm, kind in ((0, "window"), (1, "slice"), (2, "dense")):
            res = A.region_residual(case, rm) if rm else None
            rin = _res_in(eng, mode, res, shape) if rm else None
            dst = Placed(eng, kind, case.n, shape[2], shape[3], case.cout, mode, SENTINEL[mode])
            for act in A.ACTS:
                lo, hi, _ = _want(case.name, d["v"], act, mode, res, rm)
                ran, _ = _conv_hints(eng, xin, pk, case.stride, d["pad"], act, dst, rin, rm == 2, lo, hi,
                                     "%s res mode %d:" % (act, rm), failures)
                assert len(ran) >= 2, ran
                seen |= set(ran)
    print("%s %s ran on %s" % (case.name, mode, " ".join("%#x" % h for h in sorted(seen))))
    assert not failures, "\n".join(failures[:20])


# include/glsdet_hip.h, tile_hint: "12 / 13 its 8-wave form ... (no residual)" -- also on the other pixel-tile geometries
NO_RESIDUAL_HINTS = {"f16": {12, 13, 0x100 | 13, 0x200 | 13}, "f32": {12, 13, 0x100 | 13, 0x200 | 13}}
NO_RESIDUAL_HINTS["f32"].add(16 + 3)                    # "variant 19 ... takes no residual with an fp32 output" (LDS)


@pytest.mark.parametrize("mode", MODES)
def test_every_variant_and_activation_is_reached(engines, mode):
    """no (variant, activation, residual mode) silently drops out: every hint accepts, with every activation and each of
    the three residual modes, one of the problems the tests above run on every hint -- a form of the sweep or a region case
    (descriptors are recorded into a plan, nothing is launched).  The only exceptions are what the header documents: the
    8-wave ring kernels take no residual, nor does variant 19 of the 1x1 kernel with an fp32 output."""
    from glsdet_amd._lib import GlsdetError
    eng = engines[mode]
    cases = [A.RegionCase("sweep_wide", "conv", 1, 512, A.SWEEP_COUT, 1, 1, 1, 16, 32),
             A.RegionCase("sweep_narrow", "conv", 1, 64, A.SWEEP_COUT, 1, 1, 1, 16, 32),
             A.RegionCase("sweep_rows32", "conv", 1, 64, 32, 1, 1, 1, 16, 32)] + CONV_REGION
    missing = []
    with _scratch(eng):
        ops = {}
        for hint in HINTS:
            for act in A.ACTS:
                for rm in (0, 1, 2):
                    if rm and hint in NO_RESIDUAL_HINTS[mode]:
                        continue
                    for case in cases:
                        if case.name not in ops:
                            pad = case.k // 2
                            ho, wo = R.out_extent(case.h, case.k, case.stride, pad), R.out_extent(case.w, case.k, case.stride, pad)
                            z = np.zeros((case.cout, case.cin, case.k, case.k))
                            ops[case.name] = (eng.tensor(case.n, case.h, case.w, case.cin), eng.tensor(case.n, ho, wo, case.cout),
                                              eng.tensor(case.n, ho, wo, case.cout), _pack(eng, z, np.ones(case.cout), np.zeros(case.cout), case.cin))
                        x, y, r, pk = ops[case.name]
                        plan = eng.new_plan()
                        try:
                            with plan:
                                eng.conv(x, pk, case.stride, case.k // 2, act, out=y, res=r if rm else None, tile_hint=hint, res_first=rm == 2)
                        except GlsdetError:
                            continue
                        assert plan.num_ops == 1
                        break
                    else:
                        missing.append("%#x/%s/res mode %d" % (hint, act, rm))
    assert not missing, "no problem reaches (tile_hint / activation / residual mode) %s on the %s engine" % (", ".join(missing), mode)


# ================================================================================ (b) bit identity between the paths
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("act", A.ACTS)
def test_vector_and_scalar_activation_paths_give_the_same_bits(engines, mode, act):
    """scale_bias_act4 (no residual) against apply_act (GLSDET_ACT_RES_FIRST, an all-zero residual) on every hint, at
    the sweep and the thresholds: the comment in conv_common.h ("results are bit-identical") as a test"""
    eng = engines[mode]
    v = A.sweep_data()["v"]
    failures = []
    with _scratch(eng):
        zero = _res_in(eng, mode, np.zeros(v.shape), v.shape)
        lo, hi, _ = _want("sweep", v, act, mode)
        dst = Placed(eng, "dense", 1, 16, 32, A.SWEEP_COUT, mode, SENTINEL[mode])
        base = None
        for form in SWEEP_FORMS:
            sw = Sweep(eng, mode, form)
            must = (0, 1) if form != "rows32" else (1,)
            ran, vec = _hints(lambda h: sw.launch(h, act, dst), dst, lo, hi, "%s, vector path:" % form, failures, base=base, must=must)
            base = _canon(vec[ran[0]]) if base is None else base
            ran2, _ = _hints(lambda h: sw.launch(h, act, dst, zero, True), dst, lo, hi, "%s, scalar path:" % form, failures, base=base, must=must)
            assert len(ran) >= 3 and len(ran2) >= 3, (form, ran, ran2)
    assert not failures, "\n".join(failures[:20])


# ========================================================================================= (c) non-finite values
def _nonfinite_want(act, mode):
    bias = np.array([np.inf, -np.inf, np.nan], np.float32)
    want = A.emulate_act(bias, act, A.form_of(act, mode)).astype(_FT[mode])
    if act == "relu":
        assert want.tolist()[:2] == [np.inf, 0.0] and want[2] == 0       # include/glsdet_hip.h: relu(NaN) = 0
    return want


@pytest.mark.parametrize("mode", MODES)
def test_non_finite_pre_activations(engines, mode):
    """bias = +inf, -inf, NaN on three channels (scale 1, acc = 0 .. 511): every hint, vector and scalar path, gives what
    the same float32 expression gives in numpy -- and relu(NaN) = 0, as the header states (fmaxf / v_max semantics)"""
    from glsdet_amd._lib import GlsdetError
    eng = engines[mode]
    bias = np.zeros(A.SWEEP_COUT)
    bias[:3] = [np.inf, -np.inf, np.nan]
    failures = []
    with _scratch(eng):
        sweeps = [Sweep(eng, mode, f, np.ones(A.SWEEP_COUT), bias, 8) for f in ("wide", "narrow")]
        zero = _res_in(eng, mode, np.zeros((1, 8, 16, 32)), (1, 8, 16, 32))
        dst = Placed(eng, "slice", 1, 16, 32, 8, mode, SENTINEL[mode])
        for act in A.ACTS:
            want = _nonfinite_want(act, mode)
            fin = A.act64(np.arange(512.0), act)
            for rin in (None, zero):
                ran = set()
                for sw in sweeps:
                    for hint in HINTS:
                        dst.upload()
                        try:
                            sw.launch(hint, act, dst, rin, rin is not None)
                        except GlsdetError:
                            continue
                        ran.add(hint)
                        torch.cuda.synchronize()
                        got = np.ascontiguousarray(dst.grid(dst.full.buf.view(_TT[mode]).cpu().numpy())[dst.index]).view(_FT[mode]).reshape(512, 8)
                        for c in range(3):
                            ok = np.isnan(got[:, c]).all() if np.isnan(want[c]) else (got[:, c] == want[c]).all()
                            if not ok:
                                failures.append("%s hint %#x %s path: act(%r) = %r, want %r" % (
                                    act, hint, "scalar" if rin else "vector", bias[c], got[0, c], want[c]))
                        if not np.allclose(got[:, 3].astype(np.float64), fin, rtol=2e-3, atol=0):
                            failures.append("%s hint %#x: the finite channels next to the non-finite ones are wrong" % (act, hint))
                assert len(ran) >= 6, ran
    assert not failures, "\n".join(failures[:20])


# ======================================================================================== (d) glsdet_conv2d_multi
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", ["grouped", "batched"])
def test_conv2d_multi_every_activation(engines, mode, form):
    """grouped form: the 3 images of a 3x3 case as 3 problems (hints 0, 8 .. 11, generic tiles); batched form: the 9 rows
    of a 1x1 case as 9 problems (a 1x1 of a row window is the row of the 1x1; generic tiles only)"""
    from glsdet_amd._lib import GlsdetError
    eng = engines[mode]
    case = A.CHAIN_CASE if form == "grouped" else [c for c in CONV_REGION if c.k == 1][0]
    d = A.region_data(case)
    shape = d["v"].shape
    failures = []
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
        pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
        dst = Placed(eng, "window", case.n, shape[2], shape[3], case.cout, mode, SENTINEL[mode])
        for rm in (0, 1):
            res = A.region_residual(case, rm) if rm else None
            rin = _res_in(eng, mode, res, shape) if rm else None
            if form == "grouped":
                cut = lambda v: [v.image(b) for b in range(case.n)]
            else:
                cut = lambda v: [v.window(r, r + 1, 0, case.w) for r in range(case.h)]
            xs, outs, ress = cut(xin.view), cut(dst.view), (cut(rin.view) if rin else None)
            assert (2 <= len(xs) <= 8) if form == "grouped" else (9 <= len(xs) <= 32)
            for act in A.ACTS:
                lo, hi, _ = _want(case.name, d["v"], act, mode, res, rm)
                ran = []
                for hint in [0, 8, 9, 10, 11] + MULTI_TILES:
                    dst.upload()
                    try:
                        eng.conv_multi(xs, [pk] * len(xs), case.stride, d["pad"], act, outs=outs, ress=ress, tile_hint=hint)
                    except GlsdetError:
                        assert hint != 0, "the automatic choice must accept every group"
                        continue
                    ran.append(hint)
                    _, msg = _verdict(dst, lo, hi)
                    if msg:
                        failures.append("%s res mode %d hint %#x: %s" % (act, rm, hint, msg))
                assert len(ran) >= 2, ran
    assert not failures, "\n".join(failures[:20])


# ======================================================================================== (e) glsdet_conv2d_chain
@pytest.mark.parametrize("mode", MODES)
def test_conv2d_chain_first_and_second_activation(engines, mode):
    """first activation: y of a region case under every activation (act2 none); second activation: a first stage with
    scale 1, bias 0 and relu stores integers, y2 = act2 of the regions.  Every hint that accepts the pair."""
    from glsdet_amd._lib import ACT, ConvChain
    eng = engines[mode]
    case = A.CHAIN_CASE                                                         # 3 x 64 -> 64, 8 x 16
    d = A.region_data(case)
    s2 = A.chain_data()
    x, w1, y1 = s2["x"], s2["w1"], s2["y1"]
    failures = []
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(x).upload()
        y = Placed(eng, "window", case.n, case.h, case.w, 64, mode, SENTINEL[mode])
        y2 = Placed(eng, "window", case.n, case.h, case.w, 40, mode, SENTINEL[mode])
        pk_reg = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
        pk_int = _pack(eng, w1, np.ones(64), np.zeros(64), case.cin)
        pk2 = _pack(eng, s2["w"], s2["scale"], s2["bias"], 64)
        c = ConvChain()
        c.y2 = y2.view.as_c()
        c.w2, c.scale2, c.bias2 = pk2[0].data_ptr(), pk2[1].data_ptr(), pk2[2].data_ptr()
        c.c0, c.cin2, c.flags = 0, 64, 0
        for which in ("first", "second"):
            for act in A.ACTS:
                if which == "first":
                    pk, a1, a2 = pk_reg, act, "none"
                    lo, hi, _ = _want(case.name, d["v"], act, mode)
                else:
                    pk, a1, a2 = pk_int, "relu", act
                    lo, hi, _ = _want("chain2", s2["v"], act, mode)
                c.act2 = ACT[a2]
                ran = []
                for hint in HINTS:
                    y.upload(), y2.upload()
                    dd = _desc(xin.view, y.view, pk, 1, 1, a1, None, False, hint)
                    if eng.lib.glsdet_conv2d_chain(C.byref(dd), C.byref(c), _stream(eng)) != 0:
                        assert hint != 0, "the automatic choice must take this chained pair: " + eng.lib.glsdet_last_error().decode()
                        continue
                    ran.append(hint)
                    if which == "first":
                        _, msg = _verdict(y, lo, hi)
                    else:
                        bad = y.mismatch(_bits(y1, mode))
                        _, msg = _verdict(y2, lo, hi)
                        msg = ("y: " + bad) if bad else msg
                    if msg:
                        failures.append("%s activation %s hint %#x: %s" % (which, act, hint, msg))
                assert len(ran) >= 2, ran
    assert not failures, "\n".join(failures[:20])


# ========================================================================================== (f) glsdet_bottleneck
@pytest.mark.parametrize("mode", MODES)
def test_bottleneck_second_activation_with_and_without_residual(engines, mode):
    """1x1 (scale 1, bias 0, relu or none: the hidden tensor holds integers and never exists in memory) -> 3x3 with the
    regions, every activation, the three residual modes"""
    eng = engines[mode]
    n, cin0, cm, h, w = A.BNECK_SHAPE
    x, w1 = A.bneck_data("relu")["x"], A.bneck_data("relu")["w1"]
    failures, ran = [], 0
    with _scratch(eng):
        xin = Placed(eng, "ring", n, h, w, cin0, mode, NAN[mode]).put(x).upload()
        hid = Placed(eng, "dense", n, h, w, cm, mode, SENTINEL[mode]).upload()
        dst = Placed(eng, "window", n, h, w, cm, mode, SENTINEL[mode])
        p1 = _pack(eng, w1, np.ones(cm), np.zeros(cm), cin0)
        for act0 in ("relu", "none"):
            s2 = A.bneck_data(act0)
            p2 = _pack(eng, s2["w"], s2["scale"], s2["bias"], cm)
            for rm in (0, 1, 2):
                res = A.bneck_residual(s2["v"].shape, rm) if rm else None
                rin = _res_in(eng, mode, res, s2["v"].shape) if rm else None
                for act in A.ACTS:
                    lo, hi, _ = _want("bneck_%s" % act0, s2["v"], act, mode, res, rm)
                    d1 = _desc(xin.view, hid.view, p1, 1, 0, act0)
                    d2 = _desc(hid.view, dst.view, p2, 1, 1, act, rin.view if rin else None, rm == 2)
                    for hint in (0, 1):
                        dst.upload()
                        if eng.lib.glsdet_bottleneck(C.byref(d1), C.byref(d2), hint, _stream(eng)) != 0:
                            continue
                        ran += 1
                        _, msg = _verdict(dst, lo, hi)
                        if msg:
                            failures.append("act0 %s, %s, res mode %d, hint %d: %s" % (act0, act, rm, hint, msg))
                    assert hid.mismatch(None) is None, "the hidden buffer is not touched"
        assert ran >= 2 * 3 * len(A.ACTS), "the fused Bottleneck must take every activation: %s" % eng.lib.glsdet_last_error().decode()
    assert not failures, "\n".join(failures[:20])


# ==================================================================== (g) glsdet_conv2d_grouped / glsdet_conv2d_gnstats
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _kind("grouped"), ids=lambda c: c.name)
def test_conv2d_grouped_every_activation(engines, mode, case):
    eng = engines[mode]
    d = A.region_data(case)
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    failures = []
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cout, mode, NAN[mode]).put(d["x"]).upload()
        pk = eng.pack_conv_grouped([(f(d["w"]), f(d["scale"]), f(d["bias"]))], case.cout // case.cin)
        assert pk.kernel_takes
        dst = Placed(eng, "window", case.n, d["v"].shape[2], d["v"].shape[3], case.cout, mode, SENTINEL[mode])
        for act in A.ACTS:
            lo, hi, _ = _want(case.name, d["v"], act, mode)
            dst.upload()
            eng.conv_grouped(xin.view, pk, case.stride, act, out=dst.view, expand=False)
            _, msg = _verdict(dst, lo, hi)
            if msg:
                failures.append("%s: %s" % (act, msg))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
def test_conv2d_gnstats_every_activation(engines, mode):
    """the stored values of the ring kernels with GroupNorm partials (the partials themselves: tests/test_conv_exact.py)"""
    eng = engines[mode]
    case = A.CHAIN_CASE
    d = A.region_data(case)
    groups, failures, ran = 8, [], set()
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
        pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
        dst = Placed(eng, "window", case.n, case.h, case.w, case.cout, mode, SENTINEL[mode])
        nbytes = eng.lib.glsdet_conv2d_gnstats_bytes(case.n, case.h, case.w, groups)
        stats = torch.zeros(nbytes // 8, dtype=torch.float64, device=eng.device)
        for act in A.ACTS:
            lo, hi, _ = _want(case.name, d["v"], act, mode)
            for hint in (8, 9, 10, 11):
                dst.upload()
                dd = _desc(xin.view, dst.view, pk, 1, 1, act, hint=hint)
                if eng.lib.glsdet_conv2d_gnstats(C.byref(dd), groups, stats.data_ptr(), _stream(eng)) != 0:
                    continue
                ran.add((act, hint))
                _, msg = _verdict(dst, lo, hi)
                if msg:
                    failures.append("%s hint %d: %s" % (act, hint, msg))
        assert {a for a, _ in ran} == set(A.ACTS), eng.lib.glsdet_last_error().decode()
    assert not failures, "\n".join(failures)


# ================================================================================================= (h) the stems
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _kind("focus"), ids=lambda c: c.name)
def test_focus_conv_and_focus_conv_down_every_activation(engines, mode, case):
    eng = engines[mode]
    d = A.region_data(case)
    failures = []
    with _scratch(eng):
        img = _image(eng, d["x"])
        pk = _pack(eng, d["w"], d["scale"], d["bias"], 16)
        dst = Placed(eng, "slice", case.n, case.h // 2, case.w // 2, case.cout, mode, SENTINEL[mode])
        for act in A.ACTS:
            lo, hi, _ = _want(case.name, d["v"], act, mode)
            dst.upload()
            eng.focus_conv(img, pk, act, out=dst.view)
            _, msg = _verdict(dst, lo, hi)
            if msg:
                failures.append("focus_conv %s: %s" % (act, msg))
        # focus_conv_down: a 32-channel stem with scale 1, bias 0 and relu stores integers; the 3x3 stride-2 conv has the regions
        p1 = _pack(eng, A.focus_down_data(case, 40)["w1"], np.ones(32), np.zeros(32), 16)
        for cout2 in (40, 64):
            s2 = A.focus_down_data(case, cout2)
            p2 = _pack(eng, s2["w"], s2["scale"], s2["bias"], 32)
            dst = Placed(eng, "slice", case.n, s2["v"].shape[2], s2["v"].shape[3], cout2, mode, SENTINEL[mode])
            for act in A.ACTS:
                lo, hi, _ = _want("%s_down%d" % (case.name, cout2), s2["v"], act, mode)
                dst.upload()
                eng.focus_conv_down(img, p1, "relu", p2, act, out=dst.view)
                _, msg = _verdict(dst, lo, hi)
                if msg:
                    failures.append("focus_conv_down %d channels, %s: %s" % (cout2, act, msg))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _kind("stem"), ids=lambda c: c.name)
def test_resnet_stem_every_activation_and_stem_pool_relu(engines, mode, case):
    eng = engines[mode]
    d = A.region_data(case)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    failures = []
    with _scratch(eng):
        img = _image(eng, d["x"])
        pk = eng.pack_resnet_stem(t(d["w"]), t(d["scale"]), t(d["bias"]))
        ho, wo = d["v"].shape[2:]
        dst = Placed(eng, "slice", case.n, ho, wo, 64, mode, SENTINEL[mode])
        for act in A.ACTS:
            lo, hi, _ = _want(case.name, d["v"], act, mode)
            dst.upload()
            eng.resnet_stem(img, pk, act, out=dst.view)
            _, msg = _verdict(dst, lo, hi)
            if msg:
                failures.append("resnet_stem %s: %s" % (act, msg))
        # the pooled form has ReLU compiled in: MaxPool2d(3, 2, 1) of the STORED relu values, exactly (tol = 0)
        pooled = R.maxpool(A.rn(A.act64(d["v"], "relu"), mode), 3, 2, 1).astype(_FT[mode])
        dst = Placed(eng, "slice", case.n, pooled.shape[2], pooled.shape[3], 64, mode, SENTINEL[mode]).upload()
        eng.resnet_stem_pool(img, pk, out=dst.view)
        _, msg = _verdict(dst, _nhwc(pooled), _nhwc(pooled))
        if msg:
            failures.append("resnet_stem_pool: " + msg)
    assert not failures, "\n".join(failures)


# ============================================================================================= (i) depthwise convs
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", _kind("dw"), ids=lambda c: c.name)
def test_dwconv_accepts_codes_0_to_3_and_meets_their_bars(engines, mode, case):
    """dwconv.hip has its own epilogue: accurate expf + an IEEE divide in BOTH dtypes; GELU and sigmoid are refused"""
    from glsdet_amd._lib import GlsdetError
    eng = engines[mode]
    d = A.region_data(case)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    failures = []
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cout, mode, NAN[mode]).put(d["x"]).upload()
        pk = eng.pack_dw(t(d["w"]), t(d["scale"]), t(d["bias"]), case.cout)
        dst = Placed(eng, "window", case.n, d["v"].shape[2], d["v"].shape[3], case.cout, mode, SENTINEL[mode])
        for act in A.ACTS:
            dst.upload()
            if act not in A.DW_ACTS:
                with pytest.raises(GlsdetError):
                    eng.dwconv(xin.view, pk, case.stride, d["pad"], act, out=dst.view, dilation=case.dilation)
                assert dst.mismatch(None) is None
                continue
            lo, hi, _ = _want(case.name, d["v"], act, mode, dw=True)
            eng.dwconv(xin.view, pk, case.stride, d["pad"], act, out=dst.view, dilation=case.dilation)
            _, msg = _verdict(dst, lo, hi)
            if msg:
                failures.append("%s: %s" % (act, msg))
    assert not failures, "\n".join(failures)


# ============================================================================================ (j) glsdet_csp_fused
@pytest.mark.parametrize("shortcut", [True, False], ids=["shortcut", "plain"])
def test_csp_fused_last_epilogue_meets_the_silu_bar_and_the_inner_ones_saturate_exactly(engines, shortcut):
    """fp16 only, SiLU compiled in (any other code is refused).  The three inner epilogues see pre-activations at which an
    fp16 SiLU is exact (v >= 16 or v <= -32: tests/act_reference.py::csp_data), so conv3 reads known values and its
    epilogue -- the fourth site -- is held to the fp16-engine SiLU bar over every region; both tile heights."""
    from glsdet_amd._lib import ACT
    eng = engines["f16"]
    d = A.csp_data(shortcut)
    n, h, w = A.CSP_SHAPE
    lo, hi, _ = _want("csp_%d" % shortcut, d["v"], "silu", "f16")
    failures = []
    with _scratch(eng):
        xin = Placed(eng, "ring", n, h, w, 64, "f16", NAN["f16"]).put(d["x"]).upload()
        dst = Placed(eng, "window", n, h, w, 64, "f16", SENTINEL["f16"])
        packs = [_pack(eng, wt, sc, bi, wt.shape[1]) for wt, sc, bi in d["convs"]]
        desc = eng._csp_desc(xin.view, dst.view, packs, shortcut)
        for hint in (0, 1):
            dst.upload()
            rc = eng.lib.glsdet_csp_fused(C.byref(desc), hint, _stream(eng))
            assert rc == 0, eng.lib.glsdet_last_error().decode()
            _, msg = _verdict(dst, lo, hi)
            if msg:
                failures.append("hint %d: %s" % (hint, msg))
        dst.upload()
        for act in A.ACTS:
            if act != "silu":
                desc.act = ACT[act]
                assert eng.lib.glsdet_csp_fused(C.byref(desc), 0, _stream(eng)) < 0 and "SiLU" in eng.lib.glsdet_last_error().decode()
        assert dst.mismatch(None) is None
    assert not failures, "\n".join(failures)
