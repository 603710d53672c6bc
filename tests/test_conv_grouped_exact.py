"""Bit-exact tests of the grouped 3x3 conv kernel (glsdet_amd/csrc/conv_grouped.hip: glsdet_conv2d_grouped,
Engine.conv_grouped, torch.ops.glsdet.conv2d_grouped) against tests/resnext_reference.py, in both engine dtypes.

The regime of tests/conv_reference.py (ternary weights, small-integer images, 12-bit scales, dyadic biases; asserted by
check_regime for every case) makes each fp32 step exact in any summation order: the output must equal the float64 value
rounded ONCE to the output type, bit for bit -- no tolerance.  Every destination is a sentinel-filled buffer compared whole
(nothing outside the view is written), every input view lies in a buffer whose other elements are NaN (channels on both
sides, a one-pixel ring: the view is strided in n, h and w, and an out-of-map tap that read memory would show).  The case
list (resnext_reference.GROUPED_CASES) and what each case is there for: tests/test_resnext_reference.py proves that each
mistake a kernel of this layout can make changes bits on it."""
import numpy as np
import pytest
import torch

from tests import conv_reference as R
from tests import resnext_reference as X
from tests.test_conv_exact import MODES, NAN, SENTINEL, Placed, _bits, _scratch

pytestmark = pytest.mark.gpu

_TD = {"f16": torch.float16, "f32": torch.float32}
EPS32 = 2.0 ** -23


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32"), "f16": Engine("f16")}


def _pack(eng, w, scale, bias, groups):
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    return eng.pack_conv_grouped([(f(w), f(scale), f(bias))], groups)


_DATA = {}


def _data(case):
    if case.name not in _DATA:
        _DATA[case.name] = X.case_data(case)
    return _DATA[case.name]


def _run(eng, mode, case, expand=False):
    d = _data(case)
    C_ = case.groups * case.cg
    ho, wo = d["acc"].shape[2:]
    want = _bits(R.round_to(d["v"], mode), mode)
    xin = Placed(eng, "ring", case.n, case.h, case.w, C_, mode, NAN[mode]).put(d["x"]).upload()
    dst = Placed(eng, case.dst, case.n, ho, wo, C_, mode, SENTINEL[mode]).upload()
    pk = _pack(eng, d["w"], d["scale"], d["bias"], case.groups)
    assert pk.kernel_takes
    eng.conv_grouped(xin.view, pk, case.stride, case.act, out=dst.view, expand=expand)
    return dst.mismatch(want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", X.GROUPED_CASES, ids=lambda c: c.name)
def test_grouped_kernel_bit_for_bit(engines, mode, case):
    eng = engines[mode]
    with _scratch(eng):
        bad = _run(eng, mode, case)
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
def test_grid_cap_workgroups_walk_on_to_further_pixel_groups(engines, mode):
    """the launch's one cap (768 workgroups): 257 x 256 pixels of 8 channels are 1028 workgroup steps"""
    eng = engines[mode]
    with _scratch(eng):
        bad = _run(eng, mode, X.CAP_CASE)
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in X.GROUPED_CASES if (c.groups, c.cg, c.stride) in ((3, 8, 2), (32, 4, 1), (32, 32, 2))],
                         ids=lambda c: c.name)
def test_block_diagonal_expansion_gives_the_same_bits(engines, mode, case):
    """Engine.conv_grouped(expand=True): the dense conv over all C channels, the lowering of GLSDET_NO_GROUPED_CONV=1"""
    eng = engines[mode]
    with _scratch(eng):
        bad = _run(eng, mode, case, expand=True)
    assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
def test_a_recorded_plan_replays_the_kernel_on_new_input(engines, mode):
    eng = engines[mode]
    case = X.GROUPED_CASES[8]
    assert (case.groups, case.cg, case.h, case.w) == (32, 4, 25, 42)
    with _scratch(eng):
        d = _data(case)
        C_ = case.groups * case.cg
        xin = Placed(eng, "ring", case.n, case.h, case.w, C_, mode, NAN[mode]).put(d["x"]).upload()
        dst = Placed(eng, case.dst, case.n, case.h, case.w, C_, mode, SENTINEL[mode]).upload()
        pk = _pack(eng, d["w"], d["scale"], d["bias"], case.groups)
        plan = eng.new_plan()
        with plan:
            eng.conv_grouped(xin.view, pk, 1, case.act, out=dst.view)
        assert [o["name"] for o in plan.ops()] == ["conv_grouped<%s> 3x3 s1 g32 cg4 blk32x4" % mode]
        assert dst.mismatch(None) is None                     # recording launched nothing
        plan.run()
        assert not dst.mismatch(_bits(R.round_to(d["v"], mode), mode))
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            plan.capture(st)
        st.synchronize()
        x2 = (R.image((case.n, C_, case.h, case.w), 97) - 1)
        v2 = R.check_regime(X.grouped_conv(x2, d["w"], case.groups, 1), d["scale"], d["bias"], None, case.act)
        xin.put(x2).upload()
        dst.upload()
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            plan.launch(st)
        st.synchronize()
        bad = dst.mismatch(_bits(R.round_to(v2, mode), mode))
        assert not bad, bad


@pytest.mark.parametrize("mode", MODES)
def test_autotune_decides_once_under_its_own_key_and_keeps_the_bits(mode):
    """Engine(autotune=True): the grouped kernel is timed against the block-diagonal expansion on its tuned best variant; the
    verdict (0 kernel, -1 expansion) is the faster of the two measured times, is stored under exactly the key ("grouped",
    input geometry, output geometry, groups, stride, dtype) and is asked for once; either way the bits are the reference's"""
    from glsdet_amd.engine import Engine, _in_geo, _out_geo
    eng = Engine(mode, autotune=True)
    case = X.GROUPED_CASES[8]
    seen = {}
    real_conv_grouped = eng.conv_grouped

    def spy_conv_grouped(x, packed, stride, act, out=None, expand=None):
        seen["key"] = ("grouped",) + _in_geo(x) + _out_geo(out) + (packed.groups, stride, out.dtype)
        return real_conv_grouped(x, packed, stride, act, out=out, expand=expand)

    calls = []
    real = eng._measure

    def spy_measure(fn, *a, **k):
        r = real(fn, *a, **k)
        calls.append((fn, r))
        return r

    eng.conv_grouped, eng._measure = spy_conv_grouped, spy_measure
    with _scratch(eng):
        bad = _run(eng, mode, case, expand=None)
        assert not bad, bad
        key = seen["key"]
        eng._tuned.pop(key, None)                              # (another test of this process may have stored it)
        del calls[:]
        bad = _run(eng, mode, case, expand=None)
        assert not bad, bad
        assert key in eng._tuned and eng._tuned[key] in (0, -1)
        us_g = [r for fn, r in calls if fn is eng.lib.glsdet_conv2d_grouped_tune]
        us_d = [r for fn, r in calls if fn is eng.lib.glsdet_conv2d_tune]
        assert len(us_g) == 1 and us_g[0][0] == 0 and us_d and us_d[0][0] == 0
        assert us_g[0][2] > 0 and us_d[0][2] > 0
        assert eng._tuned[key] == (0 if us_g[0][2] <= us_d[0][2] else -1), (us_g, us_d, eng._tuned[key])
        del calls[:]
        bad = _run(eng, mode, case, expand=None)               # the verdict is there: nothing is timed again
        assert not bad, bad
        assert not [fn for fn, _ in calls if fn is eng.lib.glsdet_conv2d_grouped_tune]


# ----------------------------------------------------------------------------------- continuous operands: the a-priori bound
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("groups,cg,stride,h,w", [(3, 8, 1, 9, 9), (32, 4, 2, 9, 8), (5, 16, 1, 7, 5), (8, 32, 1, 8, 8)])
def test_continuous_operands_within_the_fp32_accumulation_bound(engines, mode, groups, cg, stride, h, w):
    """Operands as the engine stores them (rounded to the engine dtype first: their products are then what the kernel
    multiplies).  fp32 accumulation of K = 9 Cg products in any order is off by at most (K - 1) u sum|x w|, the scale
    multiply and the bias add by one u each of |scale| sum|x w| + |bias| (u = 2^-24 = eps32 / 2); the bound below,
    (K + 2) eps32 |scale| sum|x w| + half an output ulp, is twice the first two terms, which covers u |bias| since
    |bias| <= 1 <= (K + 2) |scale| sum|x w| on this data (asserted)."""
    eng = engines[mode]
    ft = np.float16 if mode == "f16" else np.float32
    C_, K = groups * cg, 9 * cg
    rng = np.random.default_rng([groups, cg, stride, h, w])
    x = rng.standard_normal((2, C_, h, w)).astype(ft).astype(np.float64)
    wt = (rng.standard_normal((C_, cg, 3, 3)) * 0.25).astype(ft).astype(np.float64)
    scale = rng.uniform(0.5, 2.0, C_).astype(np.float32).astype(np.float64)
    bias = rng.uniform(-1.0, 1.0, C_).astype(np.float32).astype(np.float64)
    acc = X.grouped_conv(x, wt, groups, stride)
    v = np.maximum(acc * scale[None, :, None, None] + bias[None, :, None, None], 0.0)
    s = X.grouped_abs_sum(x, wt, groups, stride) * np.abs(scale)[None, :, None, None]
    assert ((K + 2) * s >= 1.0).all()
    with _scratch(eng):
        xin = Placed(eng, "ring", 2, h, w, C_, mode, NAN[mode]).put(x).upload()
        ho, wo = acc.shape[2:]
        dst = Placed(eng, "slice", 2, ho, wo, C_, mode, SENTINEL[mode]).upload()
        eng.conv_grouped(xin.view, _pack(eng, wt, scale, bias, groups), stride, "relu", out=dst.view)
        torch.cuda.synchronize()
        got = dst.view.to_nchw().cpu().numpy().astype(np.float64)
    half_ulp = 0.5 * np.spacing(np.maximum(np.abs(v), np.abs(got)).astype(ft)).astype(np.float64)
    bound = (K + 2) * EPS32 * s + half_ulp
    err = np.abs(got - v)
    print("%s g%d cg%d: max err / bound = %.3f" % (mode, groups, cg, float((err / bound).max())))
    assert (err <= bound).all(), float((err / bound).max())


# ------------------------------------------------------------------------------------------------------- the torch op
@pytest.mark.parametrize("mode", MODES)
def test_torch_op_eager_and_replayed_from_one_captured_graph(mode):
    import glsdet_amd.torch_ops as T
    case = X.GROUPED_CASES[9]                                     # 32 x 4, n = 3, stride 2, 8 x 9
    assert (case.groups, case.cg, case.n, case.stride) == (32, 4, 3, 2)
    d = _data(case)
    C_ = case.groups * case.cg
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    w, sc, bi = T.pack_conv_grouped_weight(f(d["w"]), f(d["scale"]), f(d["bias"]), _TD[mode])
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32).transpose(0, 2, 3, 1))).to(_TD[mode]).cuda()
    bits = lambda t: t.cpu().numpy().view(np.int16 if mode == "f16" else np.int32)
    act = 0 if case.act == "none" else 2
    x = nhwc(d["x"])
    y = torch.ops.glsdet.conv2d_grouped(x, w, sc, bi, case.groups, case.stride, act)
    torch.cuda.synchronize()
    assert y.shape == (case.n, 4, 5, C_) and y.dtype == _TD[mode]
    assert np.array_equal(bits(y), _bits(R.round_to(d["v"], mode), mode))
    x2 = R.image((case.n, C_, case.h, case.w), 98) - 1
    v2 = R.check_regime(X.grouped_conv(x2, d["w"], case.groups, case.stride), d["scale"], d["bias"], None, case.act)
    sx = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.glsdet.conv2d_grouped(sx, w, sc, bi, case.groups, case.stride, act)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = torch.ops.glsdet.conv2d_grouped(sx, w, sc, bi, case.groups, case.stride, act)
    sx.copy_(nhwc(x2))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(bits(sy), _bits(R.round_to(v2, mode), mode))
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.conv2d_grouped(x, w, sc, bi, 64, case.stride, act)          # Cg = 2
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.conv2d_grouped(x.cpu(), w.cpu(), sc.cpu(), bi.cpu(), case.groups, case.stride, act)
