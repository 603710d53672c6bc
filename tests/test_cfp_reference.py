"""CPU tests of kind `cfp` (the reference's models/cfp/yolox_cfp.py): the state-dict tables, the CPU restatement
tests/cfp_reference.py against what the reference's own modules gave (tests/golden/cfp_golden.npz), the planted mistakes that
the committed data must see, the expanded form of the encoding's logits, the a-priori bound of tests/test_lvc_exact.py, the
drone twin as a parameter container, the exports and every host-side refusal of the three entry points of csrc/evc.hip.
Nothing here needs a GPU: the library calls below are refused before anything is launched and no pointer is dereferenced."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests import cfp_reference as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASE_IDS = [X.case_name(*c) for c in X.CASES]


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("phi", X.TABLE_PHIS)
def test_cfp_table_is_the_reference_modules_state_dict(phi):
    from glsdet_amd.arch import KINDS, state_dict_shapes
    assert "cfp" in KINDS
    want = X.table(phi)
    got = state_dict_shapes("cfp", phi, X.NUM_CLASSES)
    assert [(k, tuple(v)) for k, v in got.items()] == list(want.items())
    assert len(want) == {"tiny": 533, "nano": 713}.get(phi, len(want))


@pytest.mark.parametrize("phi", X.TABLE_PHIS)
def test_cfp_table_is_base_plus_the_71_evcblock_entries(phi):
    from glsdet_amd.arch import state_dict_shapes
    base = state_dict_shapes("base", phi, X.NUM_CLASSES)
    cfp = state_dict_shapes("cfp", phi, X.NUM_CLASSES)
    extra = [k for k in cfp if k not in base]
    assert len(extra) == 71 and all(k.startswith("backbone.evcblock.") for k in extra)
    assert [(k, v) for k, v in cfp.items() if k in base] == list(base.items())
    keys = list(cfp)
    first = keys.index(extra[0])
    assert keys[first - 1].startswith("backbone.C3_n4.") and keys[first + 71].startswith("head.")
    assert keys[first:first + 71] == extra
    assert "backbone.evcblock.l_MLP.linear.weight" in cfp and "backbone.evcblock.lvc.LVC.4.num_batches_tracked" in cfp
    with pytest.raises(ValueError):
        state_dict_shapes("cfq", phi, X.NUM_CLASSES)


# ------------------------------------------------------------------------------------------------------- restatement
@pytest.fixture(scope="module")
def outputs():
    """cfp_forward of every case, computed once"""
    out = {}
    with torch.no_grad():
        for phi, shape in X.CASES:
            out[X.case_name(phi, shape)] = X.cfp_forward(X.weights(phi), X.case_input(phi, shape))
    return out


@pytest.mark.parametrize("case", X.CASES, ids=_CASE_IDS)
def test_restatement_equals_the_reference_module_in_fp32(outputs, case):
    """the bar of tests/test_cross10_reference.py for its restatement"""
    got, want = outputs[X.case_name(*case)], X.recorded(*case)
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    err = X.rel(got, want)
    print("cfp_forward %s: %.3e relative to max(1, |logit|)" % (X.case_name(*case), err))
    assert err <= 1e-6


@pytest.mark.parametrize("case", X.CASES, ids=_CASE_IDS)
def test_restatement_equals_the_reference_module_in_float64(case):
    phi, shape = case
    with torch.no_grad():
        got = X.cfp_forward(X.to64(X.weights(phi)), X.case_input(phi, shape).double())
    assert all(g.dtype == torch.float64 for g in got)
    err = X.rel(got, X.recorded(phi, shape, "out64"))
    print("cfp_forward float64 %s: %.3e" % (X.case_name(*case), err))
    assert err <= 1e-6 * 1e-4                  # float64 against float64: rounding only


@pytest.mark.parametrize("rec", X.BLOCK_RECORDS, ids=[r[0] for r in X.BLOCK_RECORDS])
@pytest.mark.parametrize("kind", X.BLOCK_KINDS)
def test_block_restatements_equal_the_reference_blocks(kind, rec):
    """fp32 within twice the reference's own distance from its float64 evaluation (+ the 1e-6 above), float64 to rounding"""
    name, C, h, w, n = rec
    sd, x = X.block_weights(C), X.block_input(C, h, w, n)
    want32, want64 = X.block_recorded(kind, name), X.block_recorded(kind, name, "out64")
    assert want32.shape == x.shape
    noise = X.rel(want32, want64)
    err32 = X.rel(X.run_block(kind, sd, x), want32)
    err64 = X.rel(X.run_block(kind, X.to64(sd), x.double()), want64)
    print("%s %s: fp32 %.2e (reference's own fp32 noise %.2e), float64 %.2e" % (kind, name, err32, noise, err64))
    assert err32 <= 2 * noise + 1e-6 and err64 <= 1e-10


@pytest.mark.parametrize("rec", X.ENCODING_RECORDS, ids=[r[0] for r in X.ENCODING_RECORDS])
def test_encoding_restatement_and_its_expanded_form(rec):
    """the definition equals the reference's Encoding; the expanded form the kernel evaluates equals the definition in
    float64 to rounding (3e-16 to 6e-16 of max |E| measured)"""
    name, C, h, w, n = rec
    sd, x = X.block_weights(C), X.block_input(C, h, w, n, key=1)
    cw, sc = sd["blk.lvc.LVC.3.codewords"], sd["blk.lvc.LVC.3.scale"]
    assert float(sc.max()) < 0 and float(sc.min()) > -1
    want32, want64 = X.block_recorded("encoding", name), X.block_recorded("encoding", name, "out64")
    assert tuple(want32.shape) == (n, 64, C)
    assert X.rel(X.encoding(x, cw, sc), want32) <= 2 * X.rel(want32, want64) + 1e-6
    d64 = X.encoding(x.double(), cw.double(), sc.double())
    assert X.rel(d64, want64) <= 1e-12
    e64 = X.encoding_expanded(x.double(), cw.double(), sc.double())
    gap = float((e64 - d64).abs().max() / d64.abs().max())
    print("encoding %s: expanded form vs definition %.2e of max |E|" % (name, gap))
    assert gap <= 64 * 2.0 ** -53


# -------------------------------------------------------------------------------------------------- planted mistakes
@pytest.mark.parametrize("name", sorted(X.MISTAKES))
def test_committed_data_sees_the_planted_mistake(name):
    moved = X.mistake_distance(name)
    print("planted %s moves %s by %.3e" % (name, X.MISTAKES[name], moved))
    assert moved >= X.MISTAKE_BAR.get(name, X.SENSITIVITY)
    assert X.MISTAKE_BAR.get(name, X.SENSITIVITY) >= 10 * X.F32_BAR


def test_the_recipe_leaves_the_reference_well_conditioned():
    """the sensitivities above are no artefact of a chaotic net: the reference's fp32 evaluation sits within 1e-6 of its
    float64 one in every case, so the GPU tests' f32 bar stays at its floor"""
    for phi, shape in X.CASES:
        assert X.rel(X.recorded(phi, shape), X.recorded(phi, shape, "out64")) <= 1e-6
    sd = X.weights("tiny")
    ls = sd["backbone.evcblock.l_MLP.layer_scale_2"]
    assert 0.5 <= float(ls.min()) and float(ls.max()) <= 1.5
    var = torch.cat([v for k, v in sd.items() if k.endswith("bn.running_var") and k.startswith("head.")])
    assert float(var.min()) < 2e-3 and float(var.max()) > 0.5


# ------------------------------------------------------------------------------------------------------------- bound
_BOUND_CASES = [(32, 5, 7, 2, 1), (96, 8, 8, 1, 2), (32, 50, 84, 1, 3), (256, 9, 13, 1, 4)]


@pytest.mark.parametrize("C,h,w,n,seed", _BOUND_CASES, ids=["c32-35", "c96-64", "c32-4200", "c256-117"])
def test_the_references_fp32_evaluation_stays_inside_the_bound(C, h, w, n, seed):
    """the bound the GPU test holds glsdet_lvc_encode to is neither vacuous (it is a small multiple of what fp32 really
    does) nor unattainable (the reference's own fp32 evaluation, a different order of the same sums, meets it)"""
    x, cw, sc = X.encode_operands(C, h, w, n, seed, "continuous")
    bound, exact = X.encode_bound(x, cw, sc)
    for form in (X.encoding, X.encoding_expanded):
        err = (form(x, cw, sc).double() - exact).abs()
        ratio = float((err / bound).max())
        print("%s C=%d N=%d: worst error / bound %.3f, error %.2e of max |E|" % (form.__name__, C, h * w, ratio,
                                                                                  float(err.max() / exact.abs().max())))
        assert ratio <= 1.0
    assert float((bound / exact.abs().max()).max()) <= 2e-3        # worst case 1.5e-3 of max |E| here: far below any wrong weight


def test_exact_regimes_are_exact():
    """uniform: every weight 1 / 64 and E the exact sum; one-hot: the margin holds and E is a sum of offsets"""
    for C, h, w in ((32, 3, 7), (96, 8, 8)):
        x, cw, sc = X.encode_operands(C, h, w, 2, 9, "uniform")
        e64 = X.encoding(x.double(), cw.double(), sc.double())
        assert torch.equal(e64.float().double(), e64) and torch.equal(e64 * 512, (e64 * 512).round())
        x, cw, sc = X.encode_operands(C, h, w, 2, 9, "onehot")
        assert X.onehot_margin(x, cw, sc) > X.ONEHOT_MARGIN
        e64 = X.encoding(x.double(), cw.double(), sc.double())
        assert torch.equal(e64 * 4, (e64 * 4).round())
    assert np.exp(-X.ONEHOT_MARGIN) < 2.0 ** -150                     # below half the smallest fp32 denormal: expf gives 0


# -------------------------------------------------------------------------------------------------------------- twin
def test_drone_twin_is_the_reference_container():
    drone = os.path.join(ROOT, "glsdet_amd", "drone")
    saved_path, saved_mods = list(sys.path), {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved_mods:
        del sys.modules[k]
    sys.path.insert(0, drone)
    try:
        import importlib
        mod = importlib.import_module("models.cfp.yolox_cfp")
        body = mod.YoloBody(X.NUM_CLASSES, "tiny")
        assert body.kind == "cfp"
        want = X.table("tiny")
        assert list(body.state_dict().keys()) == list(want)
        assert [tuple(v.shape) for v in body.state_dict().values()] == list(want.values())
        sd = X.weights("tiny")
        body.load_state_dict(sd, strict=True)
        for k in ("backbone.evcblock.lvc.LVC.3.codewords", "backbone.evcblock.l_MLP.layer_scale_2",
                  "backbone.evcblock.l_MLP.linear.weight"):
            assert torch.equal(body.state_dict()[k], sd[k])
        with pytest.raises(RuntimeError):
            body.load_state_dict({q: v for q, v in sd.items() if q != "backbone.evcblock.lvc.LVC.3.scale"}, strict=True)
        body.train()
        with pytest.raises(NotImplementedError):                    # as kind base: inference only
            body(torch.zeros(1, 3, 64, 64))
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved_mods)


def test_phi_l_and_x_have_tables_as_kind_base_has():
    """kind base refuses neither l nor x (its tables exist, the reference builds them): nor does cfp; an unknown phi is a
    KeyError for both"""
    from glsdet_amd.arch import state_dict_shapes
    for phi in ("l", "x"):
        assert len(state_dict_shapes("cfp", phi, 10)) == len(state_dict_shapes("base", phi, 10)) + 71
    for kind in ("base", "cfp"):
        with pytest.raises(KeyError):
            state_dict_shapes(kind, "xl", 10)


def test_bn_eps_by_region():
    from glsdet_amd.nets import BN_EPS, cfp_bn_eps
    assert BN_EPS == 1e-3
    assert cfp_bn_eps("backbone.backbone.dark3.0") == 1e-3
    for p in ("backbone.lateral_conv0", "backbone.C3_p4.m.0.conv2", "head.stems.0", "head.cls_convs.1.0.dconv",
              "backbone.evcblock.bn1", "backbone.evcblock.lvc.LVC.1", "backbone.evcblock.lvc.LVC.4", "backbone.evcblock.l_MLP.dw.pconv"):
        assert cfp_bn_eps(p) == 1e-5, p
    for p in ("bn1", "bn2", "bn3", "residual_bn"):
        assert cfp_bn_eps("backbone.evcblock.lvc.conv_1." + p) == 1e-6


# ----------------------------------------------------------------------------------------------------------- exports
def test_exports():
    from glsdet_amd import _lib
    lib = _lib.load()
    for name in ("glsdet_lvc_encode", "glsdet_lvc_encode_workspace_bytes", "glsdet_lvc_gate", "glsdet_channel_fuse"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.glsdet_abi_version() == 17
    hdr = open(os.path.join(ROOT, "include", "glsdet_hip.h")).read()
    for text in ("glsdet_lvc_encode", "h * w <= 2^24", "k = 0..63", "c = 0..C-1"):
        assert text in hdr
    import glsdet_amd.torch_ops  # noqa: F401
    for op in ("lvc_encode", "lvc_gate", "channel_fuse"):
        assert hasattr(torch.ops.glsdet, op)
    with pytest.raises(RuntimeError, match="MI355X"):
        torch.ops.glsdet.lvc_encode(torch.zeros(1, 2, 2, 32), torch.zeros(64, 32), torch.zeros(64))


def test_workspace_helper_and_slice_rule():
    from glsdet_amd import _lib
    f = _lib.load().glsdet_lvc_encode_workspace_bytes

    def slices(N):
        chunk = 128 * max(1, -(-N // 8192))
        return -(-N // chunk)
    for n, h, w, c in ((1, 1, 1, 32), (2, 8, 16, 96), (1, 1, 129, 32), (3, 50, 84, 256), (8, 80, 80, 640), (1, 128, 65, 64)):
        want = n * slices(h * w) * 64 * (c + 1) * 4
        assert f(n, h, w, c) == (want + 255) // 256 * 256, (n, h, w, c)
    assert slices(128) == 1 and slices(129) == 2 and slices(8192) == 64 and slices(8193) == 33 and slices(1 << 24) == 64
    assert f(2, 10, 13, 32) == f(2, 13, 10, 32) == f(2, 1, 130, 32)            # a function of h * w only
    assert f(0, 4, 4, 32) == 0 and f(1, 0, 4, 32) == 0 and f(1, 4, 4, 40) == 0 and f(1, 4, 4, 0) == 0 and f(1, 4, 4, 672) == 0
    assert f(1, 4096, 4096, 32) > 0 and f(1, 4097, 4096, 32) == 0


# --------------------------------------------------------------------------------------------------- host refusals
def _view(n, h, w, c, dtype=0, base=0x100000, ct=None, extra=0):
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    ct = c if ct is None else ct
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = ct, w * ct, h * w * ct
    v.alloc_lo, v.alloc_hi = base & ~0xFF, base + n * h * w * ct * es + extra
    return v


def _encode(dtype, x=None, cw=0x400000, sc=0x410000, ws=0x500000, ws_bytes=None, E=0x600000):
    from glsdet_amd import _lib
    lib = _lib.load()
    x = _view(2, 6, 10, 96, dtype) if x is None else x
    if ws_bytes is None:
        ws_bytes = lib.glsdet_lvc_encode_workspace_bytes(2, 6, 10, 96)
    rc = lib.glsdet_lvc_encode(C.byref(x) if x != "null" else None, cw, sc, ws, ws_bytes, E, None)
    return rc, lib.glsdet_last_error().decode()


_ENCODE_REFUSALS = [
    ("C 40", lambda d: dict(x=_view(2, 6, 10, 40, d)), "multiple of 32"),
    ("C 672", lambda d: dict(x=_view(2, 6, 10, 672, d)), "multiple of 32"),
    ("C 16", lambda d: dict(x=_view(2, 6, 10, 16, d)), "multiple of 32"),
    ("x base misaligned", lambda d: dict(x=_view(2, 6, 10, 96, d, base=0x100008)), "16-byte"),
    ("x pixel stride misaligned", lambda d: dict(x=_view(2, 6, 10, 96, d, ct=98)), "16-byte"),
    ("x outside its allocation", lambda d: dict(x=_view(2, 6, 10, 96, d, extra=-2)), "leaves its allocation"),
    ("x empty", lambda d: dict(x=_view(2, 0, 10, 96, d)), "empty extent"),
    ("x of no dtype", lambda d: dict(x=_view(2, 6, 10, 96, 2)), "dtype"),
    ("too many pixels", lambda d: dict(x=_view(1, 4097, 4096, 32, d)), "2^24"),
    ("too many images", lambda d: dict(x=_view(65536, 1, 1, 32, d)), "65535"),
    ("null x", lambda d: dict(x="null"), "null"),
    ("null codewords", lambda d: dict(cw=None), "null"),
    ("null scale", lambda d: dict(sc=None), "null"),
    ("null E", lambda d: dict(E=None), "null"),
    ("null ws", lambda d: dict(ws=None), "null"),
    ("codewords misaligned", lambda d: dict(cw=0x400004), "16-byte"),
    ("scale misaligned", lambda d: dict(sc=0x410008), "16-byte"),
    ("E misaligned", lambda d: dict(E=0x600004), "16-byte"),
    ("ws not 256-byte aligned", lambda d: dict(ws=0x500010), "256-byte"),
    ("ws one byte short", lambda d: dict(ws_bytes=-1), "needed"),
]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "f32"])
@pytest.mark.parametrize("what,change,text", _ENCODE_REFUSALS, ids=[r[0] for r in _ENCODE_REFUSALS])
def test_lvc_encode_refuses_on_the_host(dtype, what, change, text):
    from glsdet_amd import _lib
    kw = change(dtype)
    if kw.get("ws_bytes") == -1:
        kw["ws_bytes"] = _lib.load().glsdet_lvc_encode_workspace_bytes(2, 6, 10, 96) - 1
    if what in ("too many pixels", "too many images"):
        kw["ws_bytes"] = 1 << 40
    rc, msg = _encode(dtype, **kw)
    assert rc < 0, what
    assert "lvc_encode" in msg and text in msg, (what, msg)


def test_lvc_gate_refuses_on_the_host():
    from glsdet_amd import _lib
    lib = _lib.load()
    good = dict(E=0x100000, n=2, c=96, a=0x200000, b=0x200100, w=0x300000, bias=0x400000, gam=0x500000)

    def call(**kw):
        a = dict(good, **kw)
        rc = lib.glsdet_lvc_gate(a["E"], a["n"], a["c"], a["a"], a["b"], a["w"], a["bias"], a["gam"], None)
        return rc, lib.glsdet_last_error().decode()
    for kw, text in ((dict(E=None), "null"), (dict(a=None), "null"), (dict(b=None), "null"), (dict(w=None), "null"),
                     (dict(bias=None), "null"), (dict(gam=None), "null"), (dict(n=0), "images"), (dict(n=65536), "images"),
                     (dict(c=40), "multiple of 32"), (dict(c=0), "multiple of 32"), (dict(c=672), "multiple of 32"),
                     (dict(E=0x100004), "16-byte"), (dict(w=0x300008), "16-byte"), (dict(gam=0x500004), "16-byte")):
        rc, msg = call(**kw)
        assert rc < 0 and "lvc_gate" in msg and text in msg, (kw, msg)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "f32"])
def test_channel_fuse_refuses_on_the_host(dtype):
    from glsdet_amd import _lib
    lib = _lib.load()
    a, t, y = _view(2, 6, 10, 96, dtype), _view(2, 6, 10, 96, dtype, base=0x200000), _view(2, 6, 10, 96, dtype, base=0x300000)
    P = lambda v: C.byref(v) if v is not None else None

    def call(a=a, t=t, y=y, v=0x400000, mode=1):
        rc = lib.glsdet_channel_fuse(P(a), P(t), P(y), v, mode, None)
        return rc, lib.glsdet_last_error().decode()
    vn = 8 if dtype == 0 else 4
    for kw, text in ((dict(a=None), "bad argument"), (dict(y=None), "bad argument"), (dict(v=None), "bad argument"),
                     (dict(mode=2), "bad argument"), (dict(mode=-1), "bad argument"), (dict(t=None, mode=1), "bad argument"),
                     (dict(y=_view(2, 6, 9, 96, dtype, base=0x300000)), "a / y mismatch"),
                     (dict(y=_view(2, 6, 10, 96, 1 - dtype, base=0x300000)), "a / y mismatch"),
                     (dict(t=_view(2, 6, 10, 64, dtype, base=0x200000)), "t / y mismatch"),
                     (dict(t=_view(2, 6, 10, 96, 1 - dtype, base=0x200000)), "t / y mismatch"),
                     (dict(a=_view(2, 6, 10, 96, dtype, base=0x100008)), "16-byte"),
                     (dict(t=_view(2, 6, 10, 96, dtype, base=0x200000, ct=96 + vn // 2)), "16-byte"),
                     (dict(y=_view(2, 6, 10, 96, dtype, base=0x300000, extra=-2)), "leaves its allocation"),
                     (dict(v=0x400004), "16-byte")):
        rc, msg = call(**kw)
        assert rc < 0 and "channel_fuse" in msg and text in msg, (kw, msg)
    odd = _view(2, 6, 10, vn + vn // 2, dtype, ct=2 * vn)
    rc, msg = call(a=odd, y=odd, mode=0)
    assert rc < 0 and "channel_fuse" in msg and "multiple of" in msg, msg


def test_groupnorm_takes_the_evc_widths_and_still_refuses_what_it_refused():
    """GroupNorm(1, C) of LightMLPBlock at C = 192 / 384 (tiny / m): C / vn does not divide 256.  Multiples of 32 channels
    are taken now; everything else keeps its refusal and its message (a call that passes the checks would launch, so the
    accepted widths are exercised on the GPU, tests/test_cfp.py)"""
    from glsdet_amd import _lib
    lib = _lib.load()
    g = (C.c_float * 400)()
    for dtype in (0, 1):
        for c in (24, 40, 72):
            x = _view(2, 8, 10, c, dtype)
            assert lib.glsdet_groupnorm(C.byref(x), C.byref(x), 1, g, g, 1e-5, 0, 0x4000, None) < 0
            assert "divisor of 256" in lib.glsdet_last_error().decode()
        x = _view(2, 8, 10, 192, dtype)
        assert lib.glsdet_groupnorm(C.byref(x), C.byref(x), 1, g, g, 1e-5, 0, 0x4001, None) < 0
        assert "aligned" in lib.glsdet_last_error().decode()          # C = 192 passed the width check
        assert lib.glsdet_groupnorm(C.byref(x), C.byref(x), 1, g, g, 1e-5, 1, 0x4000, None) < 0
        assert "act" in lib.glsdet_last_error().decode()
