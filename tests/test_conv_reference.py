"""CPU tests of tests/conv_reference.py, the exact-arithmetic reference tests/test_conv_exact.py compares the HIP convs
with: its direct conv against torch.nn.functional.conv2d in float64 (exact equality), the regime conditions for every
case the GPU file uses, and a mutation check -- for each wrong epilogue / wrong conv a kernel could plausibly implement,
the mutated reference must differ from the right one on EVERY case that has the relevant feature, which proves that the
data of the regime can see the bug."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import conv_reference as R

ALL_CONV = R.CONV_CASES + R.PRED_CASES
_DATA = {}


def _data(case):
    if case.name not in _DATA:
        _DATA[case.name] = R.case_data(case, 15 if case in R.PRED_CASES else None)
    return _DATA[case.name]


def _t(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def test_the_case_list_covers_what_it_claims():
    names = [c.name for c in ALL_CONV]
    assert len(set(names)) == len(names) and 20 <= len(R.CONV_CASES) <= 24
    assert {c.k for c in R.CONV_CASES} == {1, 3, 5, 7}
    assert {c.cin for c in R.CONV_CASES} == {8, 24, 64, 72, 128, 136, 320, 640}
    assert {c.cout for c in R.CONV_CASES} == {8, 40, 64, 72, 128, 136, 264}
    assert {(c.h, c.w) for c in R.CONV_CASES} == {(7, 5), (8, 16), (9, 17), (13, 43), (21, 25), (17, 33)}
    assert {c.n for c in R.CONV_CASES} == {1, 3}
    assert all(c.cin != 640 or c.k == 1 for c in R.CONV_CASES)
    for k in (1, 3):                                   # per shape class: inside one tile, exactly one, one pixel past it
        assert {(7, 5), (8, 16), (9, 17)} <= {(c.h, c.w) for c in R.CONV_CASES if c.k == k and c.stride == 1}
    s2 = [c for c in R.CONV_CASES if c.stride == 2]
    assert all(c.k == 3 for c in s2) and {c.h % 2 for c in s2} == {0, 1} and {c.w % 2 for c in s2} == {0, 1}
    for k in (1, 3, 7):                                # both residual orders per kernel size (5x5: act-then-add only)
        assert {c.res for c in R.CONV_CASES if c.k == k} >= {1, 2}
    assert {c.dst for c in R.CONV_CASES} == {"dense", "slice", "window"}
    assert {c.rplace for c in R.CONV_CASES if c.res} == {"dense", "window"}
    assert {c.act for c in R.CONV_CASES} == {"none", "relu"}


@pytest.mark.parametrize("case", ALL_CONV, ids=lambda c: c.name)
def test_conv_equals_torch_float64_and_the_regime_holds(case):
    d = _data(case)                                     # (case_data asserts |acc| <= 1023 and the exact float32 epilogue)
    want = F.conv2d(_t(d["x"]), _t(d["w"]), None, case.stride, case.k // 2).numpy()
    assert d["acc"].dtype == np.int64 and np.array_equal(d["acc"], want)
    assert np.abs(d["acc"]).max() <= R.ACC_MAX
    ex = np.array(2.0 ** -11)
    real = 15 if case in R.PRED_CASES else case.cout
    assert np.array_equal(np.rint((d["scale"][:real] - 1) / ex) % 2, np.ones(real))
    assert len(set(d["scale"][:real])) == real and len(set(d["bias"][:real])) == real
    assert np.array_equal(d["bias"] / ex, np.rint(d["bias"] / ex)) and np.abs(d["bias"]).max() <= 8
    if d["res"] is not None:
        assert np.array_equal(d["res"] * 8, np.rint(d["res"] * 8)) and np.abs(d["res"]).max() <= 64
    # the one rounding is a real one on a good part of the outputs, ties included where a residual makes them likely
    v = d["v"]
    inexact = v != v.astype(np.float16).astype(np.float64)
    assert inexact.mean() > 0.1, inexact.mean()
    R.round_to(v, "f32")                                # asserts that fp32 needs no rounding


@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: c.name)
def test_depthwise_conv_equals_torch_float64(case):
    d = R.dw_case_data(case)
    want = F.conv2d(_t(d["x"]), _t(d["w"]), None, case.stride, d["pad"], case.dilation, groups=case.c).numpy()
    assert np.array_equal(d["acc"], want)
    assert {(c.k, c.dilation) for c in R.DW_CASES} == {(3, 1), (3, 3), (7, 1), (7, 3)} and {c.stride for c in R.DW_CASES} == {1, 2}


@pytest.mark.parametrize("case", R.MULTI_CASES, ids=lambda c: c.name)
def test_quadrant_problems_equal_torch_on_each_window(case):
    d = R.multi_data(case)
    for q in d["quads"]:
        a, b, l, r = q["win"]
        oa, ob, ol, orr = q["owin"]
        acc = F.conv2d(_t(d["x"][:, :, a:b, l:r]), _t(q["w"]), None, case.stride, case.k // 2).numpy()
        res = d["res"][:, :, oa:ob, ol:orr] if case.res else None
        assert np.array_equal(d["v"][:, :, oa:ob, ol:orr], R.epilogue(acc, q["scale"], q["bias"], res, case.act, case.res == 2))
    if case.k > 1:                                      # the neighbour's data outside a window is real: not all zero
        a, b, l, r = d["quads"][0]["win"]
        assert np.abs(d["x"][:, :, b, l:r]).sum() > 0 and np.abs(d["x"][:, :, a:b, r]).sum() > 0
    assert not case.per_image or 9 <= 4 * case.n <= 32          # the batched form: one problem per (image, quadrant)


@pytest.mark.parametrize("out", ["f16", "f32"])
@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: c.name)
def test_chained_pair_equals_torch_and_stays_exact(case, out):
    d = R.chain_data(case)(out)                         # (asserts both regimes)
    y64 = d["y"].astype(np.float64)
    acc2 = F.conv2d(_t(y64[:, case.c0:case.c0 + case.cin2]), _t(d["w2"])).numpy()
    want = R.epilogue(acc2, d["scale2"], d["bias2"], None, case.act2)
    assert np.array_equal(d["y2"].astype(np.float64), R.round_to(want, out).astype(np.float64))
    assert {c.stride for c in R.CHAIN_CASES} == {1, 2} and {c.skip_y for c in R.CHAIN_CASES} == {True, False}


@pytest.mark.parametrize("out", ["f16", "f32"])
@pytest.mark.parametrize("case", R.BNECK_CASES, ids=lambda c: c.name)
def test_bottleneck_equals_torch_and_stays_exact(case, out):
    d = R.bneck_data(case)(out)
    hid = torch.relu(F.conv2d(_t(d["x"]), _t(d["w1"])) * _t(d["s1"]).view(1, -1, 1, 1) + _t(d["b1"]).view(1, -1, 1, 1)).numpy()
    assert np.array_equal(d["hidden"].astype(np.float64), R.round_to(hid, out).astype(np.float64))
    v = F.conv2d(_t(d["hidden"].astype(np.float64)), _t(d["w2"]), None, 1, 1) * _t(d["s2"]).view(1, -1, 1, 1) + _t(d["b2"]).view(1, -1, 1, 1)
    v = torch.relu(v).numpy() + (d["res"] if case.res else 0.0)
    assert np.array_equal(d["y"].astype(np.float64), R.round_to(v, out).astype(np.float64))
    assert any(c.cin0 > c.cm for c in R.BNECK_CASES) and {c.res for c in R.BNECK_CASES} == {0, 1}


@pytest.mark.parametrize("out", ["f16", "f32"])
@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: c.name)
def test_groupnorm_sums_are_exact_integers(case, out):
    d = R.gn_data(case)(out)
    y = d["y"].astype(np.float64).reshape(case.n, case.groups, -1)
    assert np.array_equal(d["s1"] / 2048.0, y.sum(2))                     # float64 sums of these few dyadic values are exact too
    assert np.array_equal(d["s2"] / 2048.0 ** 2, (y * y).sum(2))
    assert int(d["s2"].max()) < 2 ** 53


@pytest.mark.parametrize("case", R.FOCUS_CASES + R.RESNET_STEM_CASES, ids=lambda c: c.name)
def test_stems_equal_torch(case):
    if case in R.FOCUS_CASES:
        d = R.focus_data(case, 40)("f16")
        img = _t(d["img"])
        tl, bl, tr, br = img[..., ::2, ::2], img[..., 1::2, ::2], img[..., ::2, 1::2], img[..., 1::2, 1::2]
        v = torch.relu(F.conv2d(torch.cat((tl, bl, tr, br), 1), _t(d["w"]), None, 1, 1) * _t(d["scale"]).view(1, -1, 1, 1) +
                       _t(d["bias"]).view(1, -1, 1, 1)).numpy()
        assert np.array_equal(d["y"], v.astype(np.float16))
        v2 = F.conv2d(_t(d["y"].astype(np.float64)), _t(d["w2"]), None, 2, 1) * _t(d["scale2"]).view(1, -1, 1, 1) + _t(d["bias2"]).view(1, -1, 1, 1)
        v2 = torch.relu(v2).numpy() if case.act == "relu" else v2.numpy()
        assert np.array_equal(d["y2"], v2.astype(np.float16))
        R.focus_data(case)("f32"), R.focus_data(case, 64)("f32")
    else:
        d = R.resnet_stem_data(case)("f16")
        v = torch.relu(F.conv2d(_t(d["img"]), _t(d["w"]), None, 2, 3) * _t(d["scale"]).view(1, -1, 1, 1) + _t(d["bias"]).view(1, -1, 1, 1))
        assert np.array_equal(d["y"], v.numpy().astype(np.float16))
        assert np.array_equal(d["pooled"].astype(np.float64), F.max_pool2d(_t(d["y"].astype(np.float64)), 3, 2, 1).numpy())
        R.resnet_stem_data(case)("f32")


def test_round_toward_zero_helper_truncates():
    v = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11), 0.5, 2049.0, -2051.0])
    assert R.round_toward_zero_f16(v).tolist() == [1.0, 1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 0.5, 2048.0, -2050.0]
    assert R.round_to(v, "f16").tolist() == [1.0, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 0.5, 2048.0, -2052.0]      # ties to even


# ---------------------------------------------------------------------------------------------------- the mutation check
# name -> (applies to the case?, output types whose bits must change)
MUTATIONS = {
    "round_before_add": (lambda c: c.res != 0, ("f16",)),
    "scale_f16": (lambda c: True, ("f16", "f32")),
    "bias_f16": (lambda c: True, ("f16", "f32")),
    "round_toward_zero": (lambda c: True, ("f16",)),
    "swap": (lambda c: c.res != 0 and c.act == "relu", ("f16", "f32")),
    "bias_shift": (lambda c: True, ("f16", "f32")),
    "k_tail": (lambda c: True, ("f16", "f32")),
    "border_tap": (lambda c: True, ("f16", "f32")),
    "edge_pad": (lambda c: c.k > 1, ("f16", "f32")),
}


def _mutated(case, d, name, out):
    res, rf = d["res"], case.res == 2
    if name in ("k_tail", "border_tap", "edge_pad"):
        acc = R.conv(d["x"], d["w"], case.stride, case.k // 2, mutate=name, drop_k=8 if out == "f16" else 4)   # 16 bytes of K
        return R.epilogue(acc, d["scale"], d["bias"], res, case.act, rf)
    if name == "round_toward_zero":
        return d["v"]
    return R.epilogue(d["acc"], d["scale"], d["bias"], res, case.act, rf, mutate=name)


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_every_mutation_is_visible_on_every_case_that_has_the_feature(name):
    applies, outs = MUTATIONS[name]
    seen = 0
    for case in R.CONV_CASES:
        if not applies(case):
            continue
        d = _data(case)
        for out in outs:
            v = _mutated(case, d, name, out)
            if out == "f16":
                got = R.round_toward_zero_f16(v) if name == "round_toward_zero" else v.astype(np.float16)
                differ = got.view(np.uint16) != R.round_to(d["v"], "f16").view(np.uint16)
            else:
                differ = v.astype(np.float32).view(np.uint32) != R.round_to(d["v"], "f32").view(np.uint32)
            assert differ.any(), "%s is invisible on %s (%s output)" % (name, case.name, out)
            seen += 1
    assert seen >= 8, (name, seen)
