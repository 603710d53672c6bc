"""CPU-only: tests/swin_reference.py against the outputs tests/golden/swin_golden.npz records of the reference's own
SwinTransformer / ShiftWindowMSA / PatchMerging / SwinBlock (tools/make_swin_golden.py), the planted misreadings, the
state-dict tables, the host-side refusals of the three entry points of csrc/swin.hip (no pointer is dereferenced), and the
f16-emulation restatement that settles the dtype of the residual stream."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

from tests import swin_reference as S

MSA_TAGS = ["msa_%dx%d_s%d_h%d" % (h, w, s, nh) for (h, w) in ((7, 7), (4, 4), (8, 9), (15, 13)) for s in (0, 3) for nh in (1, 3)]
# the reference ran in fp32: its own distance from the float64 value, a few 1e-7 per layer relative to the largest output
TOL = 2e-5


def _msa(tag, mis=None):
    h, w, s, nh = map(int, re.match(r"msa_(\d+)x(\d+)_s(\d+)_h(\d+)", tag).groups())
    gain = 32.0 if tag.endswith("gain32") else 1.0
    x = S.block_input(tag).double().reshape(1, h, w, 32 * nh) * gain
    return S.msa(x, S.weights(tag), "attn.", nh, 7, s, mis=mis).reshape(1, h * w, -1)


def _merge(mis=None):
    x = S.block_input("merge_5x7").double().reshape(1, 5, 7, 32)
    return S.merging(x, S.weights("merge_5x7"), "downsample.", mis).reshape(1, 12, 64)


def _block(mis=None):
    x = S.block_input("swinblock").double().reshape(1, 9, 10, 64)
    return S.swin_block(x, S.weights("swinblock"), "block.", 2, 7, 3, mis=mis).reshape(1, 90, 64)


def _trunk(mis=None, **kw):
    outs = S.trunk(S.block_input("trunk_tiny").double(), S.weights("trunk_tiny"), mis=mis, **S.TINY, **kw)
    return torch.cat([t.flatten(1) for t in outs], 1)


def _rel(got, tag):
    want = torch.from_numpy(S.golden()["block/%s/y" % tag]).double()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("tag", MSA_TAGS + ["msa_15x13_s3_h1_gain32"])
def test_window_attention_restatement_meets_the_recorded_modules(tag):
    # gain32: q~ . k sums products of order 32 * 32 / sqrt(32); the reference's fp32 logits are off by up to
    # 34 u sum |q~| |k| ~ 34 * 6e-8 * 250 = 5e-4, which is also the relative error of its softmax weights
    assert _rel(_msa(tag), tag) < (5e-4 if tag.endswith("gain32") else TOL)


def test_merge_block_and_trunk_meet_the_recorded_modules():
    assert _rel(_merge(), "merge_5x7") < TOL
    assert _rel(_block(), "swinblock") < TOL
    sizes = [25 * 29 * 32, 13 * 15 * 64, 7 * 8 * 128, 4 * 4 * 256]      # the odd 25 x 29 stage is padded by the merge; 4 x 4 < window
    got = _trunk()
    assert got.shape[1] == sum(sizes)
    assert _rel(got, "trunk_tiny") < TOL


# (misreading, the fixture that must see it, how it is evaluated)
_PLANTED = [("pad_zero", "msa_8x9_s0_h1", _msa), ("pad_masked", "msa_8x9_s0_h3", _msa), ("mask_inf", "msa_15x13_s3_h1_gain32", _msa),
            ("regions_unpadded", "msa_15x13_s3_h1", _msa), ("regions_unshifted", "msa_7x7_s3_h1", _msa),
            ("roll_sign", "msa_15x13_s3_h3", _msa), ("no_flip", "msa_7x7_s0_h1", _msa), ("scale_after_bias", "msa_4x4_s0_h3", _msa),
            ("unfold_khkwc", "merge_5x7", None), ("merge_pad_after_norm", "merge_5x7", None), ("skip_norm_i", "trunk_tiny", None),
            ("ln_axis", "trunk_tiny", None)]


@pytest.mark.parametrize("mis,tag,fn", _PLANTED, ids=[p[0] for p in _PLANTED])
def test_every_planted_misreading_is_seen_by_its_fixture(mis, tag, fn):
    assert mis in S.MISREADINGS
    got = fn(tag, mis) if fn is not None else (_merge(mis) if tag == "merge_5x7" else _trunk(mis))
    assert _rel(got, tag) > 100 * TOL, "%s passes %s" % (mis, tag)


def test_all_misreadings_are_planted():
    assert sorted(p[0] for p in _PLANTED) == sorted(S.MISREADINGS)


def test_relative_position_index_restatements_agree():
    from glsdet_amd.synth import synth_tensor
    for ws in range(2, 9):
        n2 = ws * ws
        assert np.array_equal(S.rel_index(ws).numpy(), synth_tensor("x.relative_position_index", (n2, n2), 0))
        assert int(S.rel_index(ws).max()) == (2 * ws - 1) ** 2 - 1 and int(S.rel_index(ws).min()) == 0


@pytest.mark.parametrize("name,depths", [("swin_t", (2, 2, 6, 2)), ("swin_s", (2, 2, 18, 2))])
def test_state_dict_tables_are_the_recorded_ones(name, depths):
    want = [(k, tuple(s)) for k, s in json.loads(S.golden()["tables/" + name].tobytes().decode())]
    got = list(S.state_dict_shapes(96, depths, (3, 6, 12, 24)).items())
    assert got == want
    from glsdet_amd.arch import swin_state_dict_shapes
    assert list(swin_state_dict_shapes(depths=depths, prefix="backbone"))[0] == "backbone.patch_embed.projection.weight"


def test_tiny_trunk_table_is_the_fixture_s():
    want = {k[len("backbone."):]: tuple(s) for k, s in S.meta("trunk_tiny")["shapes"].items()}
    assert dict(S.state_dict_shapes(**S.TINY)) == want


# ------------------------------------------------------------------------------------------------ refusals on the host
def _view(n, h, w, c, dtype=0, base=0x10000, extra=0):
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = c, w * c, h * w * c
    v.alloc_lo, v.alloc_hi = base, base + n * h * w * c * es + extra
    return v


def _lib_loaded():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


def _refused(lib, rc, word):
    msg = lib.glsdet_last_error().decode()
    assert rc < 0 and word in msg, (rc, msg)


def test_layernorm_refusals():
    lib = _lib_loaded()
    P = C.byref
    g = 0x40000
    x = _view(2, 5, 7, 96)
    ln = lambda a, b, gam=g, bet=g, eps=1e-5: lib.glsdet_layernorm(P(a) if a else None, P(b) if b else None, gam, bet, eps, None)
    _refused(lib, ln(None, x), "null")
    _refused(lib, ln(x, x, gam=None), "null")
    _refused(lib, ln(_view(2, 5, 7, 40), _view(2, 5, 7, 40)), "multiple of 32")
    _refused(lib, ln(_view(1, 1, 1, 4128), _view(1, 1, 1, 4128)), "multiple of 32")
    _refused(lib, ln(x, _view(2, 5, 8, 96)), "extents")
    _refused(lib, ln(x, _view(2, 5, 7, 64)), "extents")
    _refused(lib, ln(x, x, eps=-1.0), "eps")
    _refused(lib, ln(x, x, eps=float("nan")), "eps")
    _refused(lib, ln(x, x, gam=g + 4), "aligned")
    short = _view(2, 5, 7, 96)
    short.alloc_hi -= 2
    _refused(lib, ln(x, short), "allocation")
    bad = _view(2, 5, 7, 96)
    bad.dtype = 3
    _refused(lib, ln(bad, x), "dtype")
    _refused(lib, ln(x, _view(2, 5, 7, 96, base=0x10000 + 96 * 2, extra=96 * 2)), "overlaps")     # one pixel further
    _refused(lib, ln(x, _view(2, 5, 7, 96, dtype=1)), "overlaps")                  # the same base in another dtype


def test_window_attention_refusals():
    lib = _lib_loaded()
    P = C.byref
    t = 0x40000
    q, y = _view(2, 9, 11, 288), _view(2, 9, 11, 96, base=0x900000)
    wa = lambda a, b, heads=3, ws=7, shift=3, scale=0.17, tab=t, qb=t: lib.glsdet_window_attention(
        P(a) if a else None, P(b) if b else None, tab, qb, heads, ws, shift, scale, None)
    _refused(lib, wa(None, y), "null")
    _refused(lib, wa(q, y, tab=None), "null")
    _refused(lib, wa(q, y, heads=2), "head_dim")                                     # head_dim 48
    _refused(lib, wa(q, y, heads=6), "head_dim")                                     # head_dim 16
    _refused(lib, wa(_view(1, 4, 4, 120), _view(1, 4, 4, 40, base=0x900000), heads=1), "multiple of 32")
    _refused(lib, wa(_view(1, 2, 2, 3 * 1056), _view(1, 2, 2, 1056, base=0x900000), heads=33), "multiple of 32")
    for ws in (1, 9, 0, -7):
        _refused(lib, wa(q, y, ws=ws, shift=0), "window_size")
    for shift in (-1, 7, 8):
        _refused(lib, wa(q, y, shift=shift), "shift")
    _refused(lib, wa(_view(2, 9, 11, 192), y), "qkv must be")
    _refused(lib, wa(_view(2, 9, 12, 288), y), "qkv must be")
    _refused(lib, wa(_view(2, 9, 11, 288, dtype=1), y), "dtypes")
    _refused(lib, wa(q, y, scale=float("inf")), "scale")
    _refused(lib, wa(q, y, tab=t + 2), "aligned")
    _refused(lib, wa(q, _view(2, 9, 11, 96, base=0x10000 + 288 * 2 * 9 * 11)), "overlaps")      # inside qkv's span
    short = _view(2, 9, 11, 96, base=0x900000)
    short.alloc_hi -= 2
    _refused(lib, wa(q, short), "allocation")


def test_patch_merge_refusals():
    lib = _lib_loaded()
    P = C.byref
    x = _view(2, 5, 7, 32)
    pm = lambda a, b: lib.glsdet_patch_merge(P(a) if a else None, P(b) if b else None, None)
    _refused(lib, pm(None, x), "null")
    _refused(lib, pm(x, _view(2, 2, 4, 128, base=0x900000)), "y must be")            # floor instead of ceil
    _refused(lib, pm(x, _view(2, 3, 4, 64, base=0x900000)), "y must be")
    _refused(lib, pm(x, _view(2, 3, 4, 128, dtype=1, base=0x900000)), "dtypes")
    _refused(lib, pm(x, _view(2, 3, 4, 128, base=0x10000 + 64)), "overlaps")
    _refused(lib, pm(_view(1, 4, 4, 12, dtype=1), _view(1, 2, 2, 48, dtype=1, base=0x900000)), "multiple of 8")
    short = _view(2, 3, 4, 128, base=0x900000)
    short.alloc_hi -= 2
    _refused(lib, pm(x, short), "allocation")


# ------------------------------------------------------------------------------------------------ exact-regime generators
@pytest.mark.parametrize("H,W,heads,ws,shift", [(7, 7, 1, 7, 0), (8, 9, 3, 7, 3), (15, 13, 1, 7, 3), (9, 6, 1, 4, 2), (4, 4, 4, 7, 3)])
def test_onehot_operands_keep_their_margin_and_the_bound_holds_in_fp32(H, W, heads, ws, shift):
    qkv, table, bias = S.attention_operands(2, H, W, heads, ws, "onehot", 5)
    assert torch.equal(qkv.half().double(), qkv) and torch.equal(bias.half().double(), bias)
    ex = {}
    y = S.window_attention(qkv, table, bias, heads, ws, shift, extras=ex)
    assert float(ex["margin"].min()) > S.ONEHOT_MARGIN, float(ex["margin"].min())
    # one-hot: every output is one of the v values (or the bias v of a padded winner), to float64's 1e-40
    vals = torch.cat([qkv[..., 2 * 32 * heads:].reshape(-1), bias[2 * 32 * heads:]]).unique()
    assert bool(torch.isin(y.float().double(), vals).all())


def test_regions_operands_average_over_the_mask_region():
    qkv, table, bias = S.attention_operands(1, 8, 9, 1, 7, "regions", 3)
    y = S.window_attention(qkv, table, bias, 1, 7, 3)
    y0 = S.window_attention(qkv, table, bias, 1, 7, 0)
    assert float((y - y0).abs().max()) > 0.05                     # the regions matter
    ym = S.window_attention(qkv, table, bias, 1, 7, 3, mis="regions_unpadded")
    assert float((y - ym).abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------ f16 emulation
def test_f16_emulation_settles_the_residual_stream():
    """fp16 rounding at the kernels' store points (linears, LayerNorm, attention, merge; weights in fp16), with the residual
    stream kept in fp32 (no rounding) or rounded to fp16 after every add: the distance from float64, relative to the largest
    output.  An fp32 stream must not be worse, and is what the builder uses; DESIGN section 4 records both numbers."""
    exact = _trunk()
    e32 = float((_trunk(rnd=S.f16_round) - exact).abs().max() / exact.abs().max())
    e16 = float((_trunk(rnd=S.f16_round, rnd_res=S.f16_round) - exact).abs().max() / exact.abs().max())
    print("f16 emulation of the tiny trunk: fp32 residual stream %.3e, fp16 residual stream %.3e (of max |y|)" % (e32, e16))
    assert e32 < 2e-2 and e16 < 4e-2
    assert e32 <= e16 * 1.05


# ------------------------------------------------------------------------------------------------ surface, configs
@pytest.mark.parametrize("name,depths", [("swin_t", (2, 2, 6, 2)), ("swin_s", (2, 2, 18, 2))])
def test_surface_class_has_the_recorded_names_and_shapes(name, depths):
    from glsdet_amd.mmdet_surface import SwinTransformer
    want = [(k, tuple(s)) for k, s in json.loads(S.golden()["tables/" + name].tobytes().decode())]
    sd = SwinTransformer(depths=depths).state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    k = "stages.0.blocks.1.attn.w_msa.relative_position_index"
    assert sd[k].dtype == torch.int64 and torch.equal(sd[k], S.rel_index(7))


def test_surface_refuses_what_is_not_lowered_and_names_the_argument():
    from glsdet_amd.mmdet_surface import SwinTransformer
    for kw, word in ((dict(use_abs_pos_embed=True), "use_abs_pos_embed"), (dict(with_cp=True), "with_cp"),
                     (dict(act_cfg=dict(type="ReLU")), "act_cfg"), (dict(norm_cfg=dict(type="BN")), "norm_cfg"),
                     (dict(strides=(4, 2, 2, 1)), "strides"), (dict(window_size=12), "window_size"), (dict(window_size=1), "window_size"),
                     (dict(embed_dims=64), "head_dim"), (dict(pretrained="https://example.invalid/swin.pth"), "local"),
                     (dict(init_cfg=dict(type="Pretrained", checkpoint="s3://bucket/swin.pth")), "local")):
        with pytest.raises(NotImplementedError, match=word):
            SwinTransformer(**kw)
    SwinTransformer(drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.3, pretrained="/tmp/none.pth")      # accepted
    with pytest.raises(AssertionError):
        SwinTransformer(patch_size=2)


@pytest.mark.parametrize("cfg,kind", [("coarse_det_swin_t.py", "gfl"), ("mp_det_swin_t.py", "mpdet")])
def test_swin_configs_build_with_the_reference_key_names(cfg, kind):
    import os
    from glsdet_amd.arch import swindet_state_dict_shapes
    from glsdet_amd.mmdet_surface import Config, build_detector
    c = Config.fromfile(os.path.join(S.ROOT, "configs", "UFPMP-Det", cfg))
    m = dict(c.model)
    m.pop("train_cfg", None)
    model = build_detector(m, test_cfg=c.get("test_cfg"))
    want = swindet_state_dict_shapes(kind, out_indices=(1, 2, 3))
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(s) for k, s in want.items()}
    assert [k for k in want if k.startswith("backbone.norm")] == ["backbone.norm%d.%s" % (i, s) for i in (1, 2, 3) for s in ("weight", "bias")]


def test_detector_checks_the_swin_options_against_the_state_dict():
    from glsdet_amd.arch import swindet_state_dict_shapes
    from glsdet_amd.resdet import HipGflDetector
    from glsdet_amd.synth import synth_state_dict
    sd = synth_state_dict(swindet_state_dict_shapes("gfl", out_indices=(1, 2, 3), **S.TINY), 0)
    ok = dict(backbone="swin", out_indices=(1, 2, 3), start_level=0, **S.TINY)
    HipGflDetector("gfl", sd, **ok)                                              # builds nothing yet: no GPU needed
    for bad, word in ((dict(depths=(2, 2, 6, 2)), "stages.2.blocks.2"), (dict(num_heads=(1, 2, 4, 4)), "head_dim"),
                      (dict(window_size=5), "relative_position_bias_table"), (dict(mlp_ratio=2), "ffn.layers.0.0"),
                      (dict(patch_norm=False, dtype="f32"), "do not describe"), (dict(qkv_bias=False), "do not describe"),
                      (dict(out_indices=(0, 1, 2, 3)), "norm0"), (dict(embed_dims=64, num_heads=(2, 4, 8, 16)), "patch_embed"),
                      (dict(window_size=9), "window_size"), (dict(backbone="vit"), "backbone")):
        with pytest.raises(ValueError, match=word):
            HipGflDetector("gfl", sd, **dict(ok, **bad))
    with pytest.raises(TypeError):
        HipGflDetector("gfl", sd, **dict(ok, shift=3))
    bare = synth_state_dict(swindet_state_dict_shapes("gfl", out_indices=(1, 2, 3), patch_norm=False, **S.TINY), 0)
    HipGflDetector("gfl", bare, dtype="f32", **dict(ok, patch_norm=False))
    with pytest.raises(NotImplementedError, match="patch_norm"):                  # refused before anything is emitted
        HipGflDetector("gfl", bare, dtype="f16", **dict(ok, patch_norm=False))
