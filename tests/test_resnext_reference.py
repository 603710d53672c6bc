"""CPU side of the ResNeXt feature: the tables against the reference's recorded state-dict lists, the torch restatement of the
trunk (tests/resnext_reference.py) against the outputs of the reference's OWN ResNeXt / Bottleneck classes
(tools/make_resnext_golden.py -> tests/golden/resnext_golden.npz, resnext64_golden.npz), the packed weight layout of
glsdet_conv2d_grouped, the planted mistakes its exact-regime cases must catch, every host-side refusal of the entry point,
the mmdet surface class and the three configs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import resnext_reference as X
from tests.helpers import block_case, meta_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUNKS = {"resnext50_32x4d_c2_c5": (32, 4, "resnext_golden.npz"), "resnext50_64x4d_c2_c5": (64, 4, "resnext64_golden.npz")}
BLOCKS = {"resnext_bottleneck_s2_down_g32_cg4": 2, "resnext_bottleneck_s1_g8_cg8": 1, "resnext_bottleneck_s1_g8_cg16": 1,
          "resnext_bottleneck_s1_g8_cg32": 1}
TRUST_GATE = 1e-5                 # BASELINE section 3: a restatement is trusted within 1e-5 of the reference's output


@pytest.fixture(scope="module")
def golds():
    return {f: np.load(os.path.join(ROOT, "tests", "golden", f)) for f in ("resnext_golden.npz", "resnext64_golden.npz")}


def _err(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


# ------------------------------------------------------------------------------------------------------------- tables
def _table(depth, groups, base_width):
    from glsdet_amd.arch import _Table, resnet_table
    t = _Table()
    resnet_table(t, "backbone", depth, groups=groups, base_width=base_width)
    return [(k, list(v)) for k, v in t.items()]


@pytest.mark.parametrize("groups", [32, 64])
def test_tables_equal_the_reference_state_dicts_depth_101(golds, groups):
    ref = [("backbone." + k, s) for k, s in meta_of(golds["resnext_golden.npz"], "tables/resnext101_%dx4d" % groups)]
    assert _table(101, groups, 4) == ref


@pytest.mark.parametrize("tag", sorted(TRUNKS))
def test_tables_equal_the_reference_state_dicts_depth_50(golds, tag):
    groups, bw, f = TRUNKS[tag]
    ref = [(k, list(s)) for k, s in meta_of(golds[f], "block/%s/meta" % tag)["shapes"].items()]
    assert _table(50, groups, bw) == ref
    w = dict(ref)
    assert w["backbone.layer1.0.conv2.weight"] == [4 * groups, 4, 3, 3] and w["backbone.layer4.2.conv2.weight"] == [32 * groups, 32, 3, 3]


@pytest.mark.parametrize("depth", [50, 101])
def test_groups_1_reproduces_the_resnet_table(depth):
    from glsdet_amd.arch import _Table, resdet_state_dict_shapes, resnet_table
    a, b = _Table(), _Table()
    resnet_table(a, "backbone", depth)
    resnet_table(b, "backbone", depth, groups=1, base_width=4)
    assert list(a.items()) == list(b.items())
    assert a["backbone.layer2.0.conv2.weight"] == (128, 128, 3, 3) and a["backbone.layer1.0.conv1.weight"] == (64, 64, 1, 1)
    assert list(resdet_state_dict_shapes("mpdet", depth=depth).items()) == \
        list(resdet_state_dict_shapes("mpdet", depth=depth, groups=1, base_width=4).items())
    x = resdet_state_dict_shapes("gfl", depth=depth, groups=64, base_width=4)
    assert x["backbone.layer3.0.conv2.weight"] == (1024, 16, 3, 3) and x["neck.lateral_convs.0.conv.weight"] == (256, 512, 1, 1)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("tag", sorted(TRUNKS))
def test_restatement_matches_the_reference_trunks(golds, tag):
    sd, x, want = block_case(golds[TRUNKS[tag][2]], tag)
    got = torch.cat([t.flatten(1) for t in X.resnext(sd, "m.backbone", x)], 1)
    assert got.shape == want.shape
    print("%s: %.3e" % (tag, _err(got, want)))
    assert _err(got, want) <= TRUST_GATE


@pytest.mark.parametrize("tag", sorted(BLOCKS))
def test_restatement_matches_the_reference_bottlenecks(golds, tag):
    sd, x, want = block_case(golds["resnext_golden.npz"], tag)
    got = X.bottleneck(sd, "m", x, BLOCKS[tag])
    assert got.shape == want.shape
    assert _err(got, want) <= TRUST_GATE


def test_every_resnext_golden_is_covered(golds):
    tags = {k.split("/")[1] for g in golds.values() for k in g.files if k.startswith("block/")}
    assert tags == set(TRUNKS) | set(BLOCKS)
    for g in golds.values():                      # outputs, BN statistics and JSON metas only
        assert all(k.startswith("tables/") or k.split("/")[2] in ("y", "bn", "meta") for k in g.files)


# ------------------------------------------------------------------------------------------------- the packed layout
@pytest.mark.parametrize("groups,cg", [(2, 4), (3, 8), (5, 16), (32, 4), (64, 4), (8, 32), (64, 32)])
def test_unpack_of_pack_is_the_identity_with_exact_zeros_outside(groups, cg):
    from glsdet_amd.torch_ops import grouped_weight_blocks
    rng = np.random.default_rng([groups, cg])
    w = rng.standard_normal((groups * cg, cg, 3, 3)).astype(np.float32)
    w[w == 0] = 1.0
    packed = grouped_weight_blocks(torch.from_numpy(w)).numpy()
    assert packed.shape == ((groups * cg + 31) // 32, 9, 32, 32)
    back, zeros = X.unpack_blocks(packed, groups, cg)
    assert zeros and np.array_equal(back, w)
    assert np.array_equal(packed, X.pack_blocks_np(w))
    assert int((packed != 0).sum()) == w.size              # nothing twice, nothing lost


def test_pack_refuses_other_group_widths():
    from glsdet_amd.torch_ops import grouped_weight_blocks
    for shape in [(8, 2, 3, 3), (24, 12, 3, 3), (64, 64, 3, 3), (8, 4, 5, 5)]:
        with pytest.raises(ValueError):
            grouped_weight_blocks(torch.zeros(shape))


@pytest.mark.parametrize("case", X.GROUPED_CASES, ids=lambda c: c.name)
def test_expansion_and_block_form_equal_the_grouped_conv(case):
    from tests import conv_reference as R
    d = X.case_data(case)
    dense = R.conv(d["x"], X.expand(d["w"], case.groups), case.stride, 1)
    assert np.array_equal(dense, d["acc"])
    assert np.array_equal(X.blocks_conv(d["x"], X.pack_blocks_np(d["w"]), case.stride), d["acc"])
    xf = d["x"] * 0.37 + 0.11                              # and in float64 on continuous operands
    wf = d["w"] * 0.73 - 0.05
    a = X.grouped_conv(xf, wf, case.groups, case.stride)
    b = R.conv(xf, X.expand(wf, case.groups), case.stride, 1)
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(a).max())


def _applies(mut, c):
    if mut == "s2_origin":
        return c.stride == 2
    if mut == "zero_fill":
        return c.cg < 32                                    # a 32-wide group fills its tile: there is no zero cell to replace
    if mut == "oob_next_row":
        return c.h > 1 and c.w > 1                          # a 1 x 1 map has no neighbouring row
    if mut in ("group_shift", "ci_perm"):
        return True
    raise AssertionError(mut)


@pytest.mark.parametrize("mut", X.MUTATIONS)
def test_planted_mistakes_change_bits_on_every_case_they_apply_to(mut):
    from tests import conv_reference as R
    hit = 0
    for case in X.GROUPED_CASES:
        if not _applies(mut, case):
            continue
        d = X.case_data(case)
        wrong = X.blocks_conv(d["x"], X.pack_blocks_np(d["w"]), case.stride, mutate=mut, cg=case.cg)
        assert wrong.shape == d["acc"].shape
        v = R.epilogue(wrong, d["scale"], d["bias"], None, case.act)
        for out in ("f16", "f32"):
            a, b = v.astype(np.float16 if out == "f16" else np.float32), R.round_to(d["v"], out)
            assert not np.array_equal(a, b), "%s goes unnoticed on %s (%s)" % (mut, case.name, out)
        hit += 1
    assert hit >= 3


def test_the_case_list_holds_what_the_kernel_can_get_wrong():
    cs = X.GROUPED_CASES
    assert {(c.groups, c.cg) for c in cs} >= {(2, 4), (3, 8), (5, 16), (32, 4), (64, 4), (32, 32), (64, 32)}
    assert {(c.h, c.w) for c in cs} >= {(1, 1), (2, 3), (7, 5), (8, 8), (9, 9), (25, 42), (5, 7), (3, 4)}
    assert {c.stride for c in cs} == {1, 2} and {c.n for c in cs} == {1, 3} and {c.act for c in cs} == {"none", "relu"}
    assert {(c.stride, c.h % 2) for c in cs} >= {(2, 0), (2, 1)} and {c.dst for c in cs} == {"dense", "slice", "window"}
    c = X.CAP_CASE
    assert (c.n * c.h * c.w + 63) // 64 > 768 and c.groups * c.cg <= 32


# ----------------------------------------------------------------------------------------------------- host refusals
@pytest.fixture(scope="module")
def lib():
    """host-side validation only: the pointers are never dereferenced, so this runs without a GPU"""
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


def _view(n, h, w, c, base, dtype, alloc=None):
    from glsdet_amd import _lib
    v = _lib.View()
    es = 2 if dtype == _lib.F16 else 4
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = c, w * c, h * w * c
    v.alloc_lo, v.alloc_hi = base, base + (n * h * w * c * es if alloc is None else alloc)
    return v


def _desc(c=128, R_=3, S=3, stride=1, pad=1, act=2, res=False, xdt=None, ydt=None, yc=None, yh=None, yalloc=None, hint=0):
    from glsdet_amd import _lib
    xdt = _lib.F16 if xdt is None else xdt
    ydt = xdt if ydt is None else ydt
    d = _lib.ConvDesc()
    ho, wo = (12 - 1) // stride + 1 if stride else 12, (20 - 1) // stride + 1 if stride else 20
    d.x, d.y = _view(2, 12, 20, c, 0x100000, xdt), _view(2, ho if yh is None else yh, wo, c if yc is None else yc, 0x800000, ydt, yalloc)
    d.res = _view(2, ho, wo, c, 0xA00000, ydt) if res else _lib.View()
    d.w, d.scale, d.bias = 0x500000, 0x600000, 0x700000
    d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = R_, S, stride, pad, act, hint
    return d


def test_grouped_entry_point_refuses_bad_descriptors_before_any_launch(lib):
    from glsdet_amd import _lib
    P = C.byref
    call = lambda d, groups: lib.glsdet_conv2d_grouped(P(d), groups, None)
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        for groups, dt, stride in [(32, _lib.F16, 1), (16, _lib.F32, 2), (8, _lib.F16, 2), (4, _lib.F32, 1)]:     # Cg 4, 8, 16, 32
            assert call(_desc(xdt=dt, stride=stride), groups) == 0, lib.glsdet_last_error()
        assert lib.glsdet_plan_num_ops(plan) == 4
        refused = lambda rc: (rc < 0 and b"conv2d_grouped" in lib.glsdet_last_error()) or pytest.fail(
            "accepted or unnamed: %d %r" % (rc, lib.glsdet_last_error()))
        refused(call(_desc(), 64))                           # Cg = 2
        refused(call(_desc(c=96), 8))                        # Cg = 12
        refused(call(_desc(), 2))                            # Cg = 64
        refused(call(_desc(c=136), 32))                      # C is no multiple of the group count
        refused(call(_desc(yc=64), 32))                      # x.c != y.c
        refused(call(_desc(), 0))
        refused(call(_desc(R_=5, S=5, pad=2), 32))           # 5x5
        refused(call(_desc(R_=3, S=1), 32))
        refused(call(_desc(pad=0), 32))                      # pad 0
        refused(call(_desc(stride=3), 32))                   # stride 3
        refused(call(_desc(res=True), 32))                   # a residual
        refused(call(_desc(xdt=_lib.F16, ydt=_lib.F32), 32)) # mixed dtypes
        refused(call(_desc(yh=11), 32))                      # output extent
        refused(call(_desc(yalloc=2 * 12 * 20 * 128 * 2 - 16), 32))          # a view outside its allocation
        refused(call(_desc(act=0x102), 32))                  # residual-first flag without a residual kernel
        refused(call(_desc(act=6), 32))
        refused(call(_desc(hint=8), 32))                     # one kernel: no variants
        refused(lib.glsdet_conv2d_grouped(None, 32, None))
        d = _desc()
        d.w = 0
        refused(call(d, 32))
        d = _desc()
        d.y = d.x                                            # in place
        refused(call(d, 32))
        best, us = C.c_int32(0), C.c_float(0)
        refused(lib.glsdet_conv2d_grouped_tune(P(_desc()), 64, None, P(best), P(us)))
        assert lib.glsdet_plan_num_ops(plan) == 4
        assert lib.glsdet_plan_end(plan) == 0
    finally:
        lib.glsdet_plan_destroy(plan)


def test_weight_elems_helper(lib):
    f = lib.glsdet_conv_grouped_weight_elems
    assert f(32, 4) == 4 * 9 * 1024 and f(64, 32) == 64 * 9 * 1024 and f(2, 4) == 9 * 1024 and f(3, 8) == 9 * 1024 and f(5, 16) == 3 * 9 * 1024
    assert f(8, 2) == 0 and f(8, 12) == 0 and f(2, 64) == 0 and f(0, 4) == 0 and f(-1, 4) == 0


def test_a_recorded_grouped_op_names_its_kernel(lib):
    name = C.create_string_buffer(160)
    kind, fl, by = C.c_int32(), C.c_double(), C.c_double()
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        assert lib.glsdet_conv2d_grouped(C.byref(_desc(stride=2)), 32, None) == 0
        assert lib.glsdet_plan_end(plan) == 0
        assert lib.glsdet_plan_op_info(plan, 0, C.byref(kind), C.byref(fl), C.byref(by), name, 160) == 0
        assert name.value.decode() == "conv_grouped<f16> 3x3 s2 g32 cg4 blk32x4"
        assert fl.value == 2.0 * 2 * 6 * 10 * 128 * 9 * 4            # the layer's own arithmetic, not the padded tiles'
    finally:
        lib.glsdet_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------------- the surface
def _backbone(**kw):
    from glsdet_amd.mmdet_surface.registry import build_backbone
    cfg = dict(type="ResNeXt", depth=50, groups=32, base_width=4, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
               norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, style="pytorch")
    cfg.update(kw)
    return build_backbone(cfg)


def test_surface_class_lists_the_reference_state_dict(golds):
    import glsdet_amd.mmdet_surface  # noqa: F401  (registers the classes)
    for depth, groups in ((101, 32), (101, 64)):
        ours = [(k, list(v.shape)) for k, v in _backbone(depth=depth, groups=groups).state_dict().items()]
        assert ours == [(k, s) for k, s in meta_of(golds["resnext_golden.npz"], "tables/resnext101_%dx4d" % groups)]
    from glsdet_amd.mmdet_surface.resdet_models import ResNet
    b = _backbone()
    assert isinstance(b, ResNet) and (b.groups, b.base_width, b.depth) == (32, 4, 50)


@pytest.mark.parametrize("kw,word", [(dict(depth=152), "depth"), (dict(style="caffe"), "style"),
                                     (dict(dcn=dict(type="DCN", deform_groups=1, fallback_on_stride=False)), "dcn"),
                                     (dict(plugins=[dict(cfg=dict(type="ContextBlock", ratio=1. / 16), position="after_conv3")]), "plugins")])
def test_surface_refusals_name_the_argument(kw, word):
    import glsdet_amd.mmdet_surface  # noqa: F401
    with pytest.raises(NotImplementedError) as e:
        _backbone(**kw)
    assert word in str(e.value).lower()


def test_surface_refuses_nonsense_group_arguments():
    import glsdet_amd.mmdet_surface  # noqa: F401
    for kw in (dict(groups=0), dict(base_width=0), dict(groups=2.5)):
        with pytest.raises(ValueError):
            _backbone(**kw)


@pytest.mark.parametrize("cfg,kind,groups,head", [("mp_det_x101_32x4d.py", "MPDet", 32, "MPHead"), ("mp_det_x101_64x4d.py", "MPDet", 64, "MPHead"),
                                                  ("coarse_det_x101_32x4d.py", "GFL", 32, "GFLHead")])
def test_configs_build(cfg, kind, groups, head):
    from glsdet_amd.arch import resdet_state_dict_shapes
    from glsdet_amd.mmdet_surface import init_detector
    m = init_detector(os.path.join(ROOT, "configs", "UFPMP-Det", cfg), device="cpu", cfg_options={"model.bbox_head.num_words": 8}
                      if kind == "MPDet" else {})
    assert type(m).__name__ == kind and type(m.backbone).__name__ == "ResNeXt" and type(m.bbox_head).__name__ == head
    assert (m.backbone.depth, m.backbone.groups, m.backbone.base_width) == (101, groups, 4)
    sd = m.state_dict()
    assert tuple(sd["backbone.layer1.0.conv2.weight"].shape) == (4 * groups, 4, 3, 3)
    want = resdet_state_dict_shapes("mpdet" if kind == "MPDet" else "gfl", depth=101, groups=groups, base_width=4)
    names = [k for k in sd if k.startswith("backbone.") or k.startswith("neck.")]
    assert names == [k for k in want if k.startswith("backbone.") or k.startswith("neck.")]
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in names)
