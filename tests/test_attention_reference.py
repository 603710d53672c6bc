"""CPU tests of tests/attention_reference.py -- the naive reference tests/test_attention_fuzz.py holds the attention
kernels against -- and of the host-side refusals of those entry points.  Nothing downstream is trusted before this file
passes: the integer split agrees with oracle.adapt_split (the restatement of the reference's Python loops) on every map
the GPU file uses, the float64 definitions agree with the oracle's own blocks, and the case lists still contain every edge
they were written for."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import glsdet_oracle as O
from tests import attention_reference as R
from tests.helpers import block_case

SPLIT_CASES = R.split_cases()


def _oracle_split(k, g, half=False):
    t = torch.from_numpy(R.to_float(k, g))[:, None]
    if half:
        t = t.half().float()
    return tuple(int(v) for v in O.adapt_split(t))


# ------------------------------------------------------------------------------------------------------------ the split
def test_split_reference_agrees_with_the_oracle_on_the_probe_sweep():
    """400 generated dyadic maps, fp32 and fp16-rounded, batch sizes 1, 2, 3, 16: random, a hot 3 x 3 blob, constant,
    mirror-symmetric (a running sum exactly half the total), values exactly on the threshold."""
    seen = set()
    for k, g in R.probe_maps():
        want = R.split_reference(k)
        assert _oracle_split(k, g) == want and _oracle_split(k, g, half=True) == want, (k.shape, want)
        seen.add((want, k.shape[1:]))
    assert any(s[0] == 4 for s, _ in seen) and any(s[0] == hw[0] - 4 for s, hw in seen)          # both clamps occurred
    assert any(s[1] != s[2] for s, _ in seen)
    assert R.split_reference(np.zeros((2, 12, 20), np.int64)) == (8, 16, 16)                     # the unbroken loop


@pytest.mark.parametrize("case", SPLIT_CASES, ids=[c[0] for c in SPLIT_CASES])
def test_split_reference_agrees_with_the_oracle_on_every_gpu_case(case):
    name, k, g = case
    R.assert_exact(k, g)
    assert np.array_equal(R.to_float(k, g).astype(np.float16).astype(np.float32), R.to_float(k, g))     # fp16 holds it
    assert _oracle_split(k, g) == R.split_reference(k)


@pytest.mark.parametrize("tag", ["att_pcnl_adapt_new", "att_pcnl_adapt_new_linear"])
def test_split_reference_agrees_with_the_committed_goldens(att_golden, tag):
    """The comparison test_adaptive_split_is_found_on_the_device... makes against oracle.adapt_split, restated in
    integers: a float32 map IS dyadic (k / 2^64 here, checked), so the exact split exists; the oracle's float32 sums must
    find the same one on these two maps, and on their 2^-10 grid roundings where its sums are exact."""
    sd, x, _ = block_case(att_golden, tag)
    att = O.spatial_attention(sd, "m.attention_map", x)[:, 0]
    k = np.empty(att.shape, object)
    for idx, v in np.ndenumerate(att.numpy()):
        f = Fraction(float(v)) * (1 << 64)
        assert f.denominator == 1
        k[idx] = int(f)
    assert R.split_reference(k) == tuple(O.adapt_split(att[:, None]))
    kq = np.round(att.numpy().astype(np.float64) * 1024).astype(np.int64)
    R.assert_exact(kq, 10)
    assert R.split_reference(kq) == _oracle_split(kq, 10)


def test_the_case_list_still_holds_every_edge():
    """so that a later edit of the builders cannot quietly drop one"""
    got = {"cx": set(), "cyl": set(), "cyr": set()}
    tie = on_thr = differ = False
    for name, k, g in SPLIT_CASES:
        if k.size > 100000:
            continue                                  # the largest map repeats the structures of the small ones
        cx, cyl, cyr = R.split_reference(k)
        H, W = k.shape[1:]
        for key, v, size in (("cx", cx, H), ("cyl", cyl, W), ("cyr", cyr, W)):
            if size > 8:
                got[key] |= {"lo"} if v == 4 else ({"hi"} if v == size - 4 else {"mid"})
        tr = R.split_trace(k)
        tie, on_thr, differ = tie or tr["tie"], on_thr or tr["on_threshold"], differ or abs(cyl - cyr) >= 8
    assert all(v == {"lo", "hi", "mid"} for v in got.values()), got
    assert tie and on_thr and differ
    names = {c[0].split("-", 1)[1] for c in SPLIT_CASES}
    assert {"constant", "all_zero", "all_negative", "images_disagree", "blob_on_odd_index", "far_apart_columns"} <= names
    # ... and each named structure does what its name says
    by = {c[0]: c[1] for c in SPLIT_CASES}
    assert R.split_trace(by["2x12x20-mirror_symmetric_tie"])["tie"] and R.split_trace(by["2x12x20-two_equal_rows_tie"])["tie"]
    assert R.split_reference(by["2x12x20-two_equal_rows_tie"])[0] == 6            # 5 // 2 * 2 = 4 had it stopped on the tie
    assert R.split_trace(by["2x12x20-values_on_threshold"])["on_threshold"]
    assert R.split_reference(by["2x12x20-values_on_threshold"]) == (8, 16, 10)    # (4, 4, 16) had the 48s been zeroed
    assert R.split_reference(by["1x24x36-blob_on_odd_index"]) == (4, 32, 6)       # 5 -> 4, 7 -> 6; nothing above the split
    assert R.split_reference(by["2x12x20-blob_before_4"])[:2] == (4, 4)
    assert R.split_reference(by["2x12x20-blob_after_size_4"])[::2] == (8, 16)
    d = by["2x12x20-images_disagree"]
    assert len({R.split_reference(d[:1]), R.split_reference(d[1:]), R.split_reference(d)}) >= 2
    cyl, cyr = R.split_reference(by["1x24x36-far_apart_columns"])[1:]
    assert cyr - cyl >= 20
    assert R.split_reference(by["16x12x20-all_zero"]) == (8, 16, 16)
    for H, W in ((24, 36), (12, 20)):
        hs = R.host_splits(H, W)
        for i, size in ((0, H), (1, W), (2, W)):
            assert {4, size - 4} <= {s[i] for s in hs}
        assert any(abs(s[1] - s[2]) >= 8 for s in hs) and any((v // 2) % 2 == 1 for s in hs for v in s)


# ---------------------------------------------------------------------------------------------------- rowsplit, by hand
def test_rowsplit_reference_on_a_map_small_enough_to_read():
    a = np.arange(1, 1 + 6 * 6, dtype=np.float32).reshape(1, 1, 6, 6)
    y0 = np.full_like(a, -1)
    split = (4, 2, 4)                                              # shift 1: cx 2, cyl 1, cyr 2
    lt = R.rowsplit_reference(a, None, y0, split, 3, 0, 1)
    assert lt[0, 0, :2, :1].tolist() == [[1], [7]] and lt.sum() == 8
    rb = R.rowsplit_reference(a, None, y0, split, 4, 3, 1)
    assert np.array_equal(rb[0, 0, 2:, 2:], a[0, 0, 2:, 2:]) and (rb[0, 0, :2] == -1).all() and (rb[0, 0, 2:, :2] == -1).all()
    merged = y0
    for q in range(4):
        merged = R.rowsplit_reference(a, None, merged, split, 4, q, 1)
    assert np.array_equal(merged, a)                               # the four quadrants tile the map exactly once
    sel = R.rowsplit_reference(a, -a, y0, split, 2, 0, 0)
    assert np.array_equal(sel[0, 0, :4], a[0, 0, :4]) and np.array_equal(sel[0, 0, 4:], -a[0, 0, 4:])
    assert R.rowsplit_reference(a, None, y0, split, 0, 0, 0)[0, 0, 4:].sum() == 0
    assert R.rowsplit_reference(a, None, y0, split, 1, 0, 0)[0, 0, :4].sum() == 0


# ------------------------------------------------------------------------------------------------ windowed non-local
@pytest.mark.parametrize("split,shift", [((4, 4, 8), 0), ((8, 10, 6), 0), ((12, 20, 8), 1)])
def test_nonlocal_windows_reference_agrees_with_the_oracle_block_on_the_four_slices(split, shift):
    cx, ci, H, W = 16, 8, 12, 14
    names = ("lt", "lb", "rt", "rb")
    x = O.synth_input((2, cx, H, W), 11).double()
    sds, tpg, wout, bout = [], [], [], []
    for i, q in enumerate(names):
        shapes = {"m.g.weight": (ci, cx, 1, 1), "m.g.bias": (ci,), "m.theta.weight": (ci, cx, 1, 1), "m.theta.bias": (ci,),
                  "m.phi.weight": (ci, cx, 1, 1), "m.phi.bias": (ci,), "m.conv_out.weight": (cx, ci, 1, 1), "m.conv_out.bias": (cx,)}
        sd = {k: v.double() for k, v in O.synth_state_dict(shapes, 20 + i).items()}
        sds.append(sd)
        conv = lambda p: torch.nn.functional.conv2d(x, sd[p + ".weight"], sd[p + ".bias"])
        tpg.append(torch.cat([conv("m.theta"), conv("m.phi"), conv("m.g")], 1).numpy())
        wout.append(sd["m.conv_out.weight"].reshape(cx, ci).numpy())
        bout.append(sd["m.conv_out.bias"].numpy())
    got = R.nonlocal_windows_reference(x.numpy(), tpg, wout, bout, split, shift)
    assert not np.isnan(got).any()
    c0, cyl, cyr = (s >> shift for s in split)
    slices = ((slice(0, c0), slice(0, cyl)), (slice(c0, None), slice(0, cyr)), (slice(0, c0), slice(cyl, None)),
              (slice(c0, None), slice(cyr, None)))
    for sd, (r, c) in zip(sds, slices):
        want = O.non_local_block(sd, "m", x[:, :, r, c]).numpy()
        assert np.abs(got[:, :, r, c] - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert np.array_equal(R.membership_reference((1, 1, H, W), split, shift)[0, 0, [0, -1, 0, -1], [0, 0, -1, -1]], [1, 2, 3, 4])


# ------------------------------------------------------------------------------------------------------------- dwconv
def test_dwconv_reference_agrees_with_the_two_depthwise_lines_of_the_lsk_block(att_golden):
    sd, x, _ = block_case(att_golden, "att_lskblock_c32")
    O.TRACE = {}
    try:
        O.lsk_block(sd, "m", x)
        tr = dict(O.TRACE)
    finally:
        O.TRACE = None
    one = np.ones(x.shape[1], np.float32)
    a1 = R.dwconv_reference(x.numpy(), sd["m.conv0.weight"].numpy(), one, sd["m.conv0.bias"].numpy(), 1, 2, 1, "none", "f32")
    assert np.abs(a1 - tr["m.conv0"].numpy()).max() <= 2e-6 * max(1.0, float(tr["m.conv0"].abs().max()))
    a2 = R.dwconv_reference(tr["m.conv0"].numpy(), sd["m.conv_spatial.weight"].numpy(), one, sd["m.conv_spatial.bias"].numpy(),
                            1, 9, 3, "none", "f32")
    assert np.abs(a2 - tr["m.conv_spatial"].numpy()).max() <= 2e-6 * max(1.0, float(tr["m.conv_spatial"].abs().max()))


def test_dwconv_dyadic_operands_are_exact_in_float32():
    """the builder's claim, checked: float32 accumulation in two different orders and float64 give the same bits"""
    x, w, scale, bias = R.dwconv_dyadic(8, 9, 11, 7, 5, 3)
    ref = R.dwconv_reference(x, w, scale, bias, 1, 3, 1, "none", "f32")
    t = torch.nn.functional.conv2d(torch.from_numpy(x), torch.from_numpy(w), None, 1, 3, 1, 8)
    f32 = (t * torch.from_numpy(scale).view(1, 8, 1, 1) + torch.from_numpy(bias).view(1, 8, 1, 1)).numpy()
    assert np.array_equal(f32, ref)
    assert np.array_equal(x.astype(np.float16).astype(np.float32), x) and np.array_equal(w.astype(np.float16).astype(np.float32), w)


def test_gate_references_round_twice_for_fp16():
    a = np.array([[[[1.0 + 2.0 ** -10]]]], np.float32)             # a * b = 1 + 2^-9 + 2^-20 ... picks the double rounding
    b = np.array([[[[1.0 + 2.0 ** -10]]]], np.float32)
    assert R.gate_reference(a, b, None, "f32")[0, 0, 0, 0] == np.float32(a[0, 0, 0, 0] * b[0, 0, 0, 0])
    assert R.gate_reference(a, b, None, "f16")[0, 0, 0, 0] == np.float32(np.float16(np.float32(a[0, 0, 0, 0] * b[0, 0, 0, 0])))
    m = np.array([[[[0.5]], [[0.25]]]], np.float32)
    assert R.gate_reference(a, 4 * b, m, "f32")[0, 0, 0, 0] == np.float32(1.5 * (1.0 + 2.0 ** -10))
    assert R.scale_by_map_reference(a, m[:, 1:], "f32")[0, 0, 0, 0] == np.float32(0.25 * (1.0 + 2.0 ** -10))
    assert np.isinf(R.gate_reference(300 * a, 300 * b, None, "f16")).all()
    assert (R.gate_bound(a, b, m, "f32") > 0).all()


# ------------------------------------------------------------------------------------------------- host-side refusals
def _view(n, h, w, c, base=0x10000, dtype=None):
    from glsdet_amd import _lib
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, _lib.F32 if dtype is None else dtype
    v.sw, v.sh, v.sn = c, w * c, h * w * c
    v.alloc_lo, v.alloc_hi = base, base + n * h * w * c * 4
    return v


@pytest.fixture(scope="module")
def lib():
    """host-side validation only: the pointers are never dereferenced, so this runs without a GPU"""
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


def _refused(lib, rc, name):
    msg = lib.glsdet_last_error().decode()
    assert rc < 0 and name in msg, (rc, msg)


def test_attn_split_refuses_bad_maps_before_any_launch(lib):
    P = C.byref
    _refused(lib, lib.glsdet_attn_split(P(_view(17, 8, 8, 8)), 0x900000, None), "attn_split")
    _refused(lib, lib.glsdet_attn_split(P(_view(2, 7, 8, 8)), 0x900000, None), "attn_split")
    _refused(lib, lib.glsdet_attn_split(P(_view(2, 8, 7, 8)), 0x900000, None), "attn_split")
    _refused(lib, lib.glsdet_attn_split(P(_view(2, 8, 8, 8)), None, None), "attn_split")
    # the largest accepted map: n (h + 2 w) + 2048 = 15360 floats.  Accepted = recorded into a plan (nothing launches)
    n, h, w = R.split_shapes()[-1]
    assert n * (h + 2 * w) + 2048 == 15360
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        assert lib.glsdet_attn_split(P(_view(n, h, w, 8)), 0x900000, None) == 0
        assert lib.glsdet_plan_num_ops(plan) == 1
        _refused(lib, lib.glsdet_attn_split(P(_view(n, h, w + 1, 8)), 0x900000, None), "attn_split")     # one column wider
        assert lib.glsdet_plan_num_ops(plan) == 1
        assert lib.glsdet_plan_end(plan) == 0
    finally:
        lib.glsdet_plan_destroy(plan)


def test_rowsplit_refuses_bad_arguments_before_any_launch(lib):
    from glsdet_amd import _lib
    P = C.byref
    a, y = _view(2, 12, 20, 8), _view(2, 12, 20, 8, base=0x200000)
    _refused(lib, lib.glsdet_rowsplit(P(a), None, P(y), 0x900000, 5, None), "rowsplit")                 # mode 5
    _refused(lib, lib.glsdet_rowsplit(P(a), None, P(y), 0x900000, 2, None), "rowsplit")                 # select without b
    _refused(lib, lib.glsdet_rowsplit(P(a), None, P(y), None, 0, None), "rowsplit")                     # no split
    _refused(lib, lib.glsdet_rowsplit(P(a), None, P(_view(2, 12, 19, 8, base=0x200000)), 0x900000, 0, None), "rowsplit")
    _refused(lib, lib.glsdet_rowsplit(P(a), None, P(_view(2, 12, 20, 16, base=0x200000)), 0x900000, 0, None), "rowsplit")
    y16 = _view(2, 12, 20, 8, base=0x200000, dtype=_lib.F16)
    _refused(lib, lib.glsdet_rowsplit(P(a), None, P(y16), 0x900000, 0, None), "rowsplit")               # dtype
    _refused(lib, lib.glsdet_rowsplit(P(a), P(_view(2, 11, 20, 8, base=0x300000)), P(y), 0x900000, 2, None), "rowsplit")


def test_scale_by_map_refuses_a_map_of_another_dtype_or_extent(lib):
    from glsdet_amd import _lib
    P = C.byref
    x, y = _view(2, 12, 20, 8), _view(2, 12, 20, 8, base=0x200000)
    _refused(lib, lib.glsdet_scale_by_map(P(x), P(_view(2, 12, 20, 8, base=0x300000, dtype=_lib.F16)), P(y), None), "scale_by_map")
    _refused(lib, lib.glsdet_scale_by_map(P(x), P(_view(2, 12, 19, 8, base=0x300000)), P(y), None), "scale_by_map")
    _refused(lib, lib.glsdet_scale_by_map(P(x), P(_view(1, 12, 20, 8, base=0x300000)), P(y), None), "scale_by_map")
    _refused(lib, lib.glsdet_scale_by_map(P(x), None, P(y), None), "scale_by_map")


def test_gate_refuses_a_missing_or_one_channel_map(lib):
    P = C.byref
    a, b, y = _view(2, 12, 20, 8), _view(2, 12, 20, 8, base=0x200000), _view(2, 12, 20, 8, base=0x300000)
    _refused(lib, lib.glsdet_gate(P(a), P(b), None, P(y), 0, None), "gate")                             # mode 0 without a map
    _refused(lib, lib.glsdet_gate(P(a), P(b), P(_view(2, 12, 20, 1, base=0x400000)), P(y), 0, None), "gate")
    _refused(lib, lib.glsdet_gate(P(a), P(b), P(_view(2, 12, 19, 2, base=0x400000)), P(y), 0, None), "gate")
    _refused(lib, lib.glsdet_gate(P(a), P(b), None, P(y), 2, None), "gate")
    _refused(lib, lib.glsdet_gate(P(a), P(_view(2, 12, 20, 16, base=0x200000)), None, P(y), 1, None), "gate")


def _dw_desc(R_=3, S=3, stride=1, pad=1, act=0, yh=12, yw=20, res=False):
    from glsdet_amd import _lib
    d = _lib.ConvDesc()
    d.x, d.y = _view(2, 12, 20, 8), _view(2, yh, yw, 8, base=0x200000)
    d.res = _view(2, yh, yw, 8, base=0x300000) if res else _lib.View()
    d.w, d.scale, d.bias = 0x500000, 0x600000, 0x700000
    d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = R_, S, stride, pad, act, 0
    return d


def test_dwconv_refuses_bad_descriptors_before_any_launch(lib):
    P = C.byref
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        assert lib.glsdet_dwconv2d_dilated(P(_dw_desc()), 1, None) == 0                                 # the descriptor itself is fine
        assert lib.glsdet_dwconv2d_dilated(P(_dw_desc(pad=8)), 8, None) == 0
        assert lib.glsdet_plan_num_ops(plan) == 2
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc()), 0, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc(pad=9)), 9, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc(act=4)), 1, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc(res=True)), 1, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc(yh=11)), 1, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc(yw=21)), 1, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d_dilated(P(_dw_desc(R_=16, pad=8, yh=13, yw=34)), 1, None), "dwconv2d")
        _refused(lib, lib.glsdet_dwconv2d(P(_dw_desc(act=4)), None), "dwconv2d")
        assert lib.glsdet_plan_num_ops(plan) == 2
        assert lib.glsdet_plan_end(plan) == 0
    finally:
        lib.glsdet_plan_destroy(plan)
