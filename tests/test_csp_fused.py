"""The dark2 CSPLayer (64 -> 64 channels, hidden 32, one Bottleneck) as ONE launch (glsdet_csp_fused, csrc/conv_csp.hip):
bit identity with the four launches it replaces, the opt-in wiring in NetBuilder.csp / NetBuilder.darknet, the fall-backs, and
(without a GPU) the host-side validation of the entry point."""
import ctypes as C

import pytest
import torch

from oracle import glsdet_oracle as O
from tests.helpers import model_case

F16_TOL = 2e-2      # the bar tests/test_hip_model.py holds a CSPLayer to in fp16: 2e-2 x max|want|


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32"), "f16": Engine("f16")}


def _upload(eng, x, embed=None):
    from tests.test_hip_ops import _to_view
    return _to_view(eng, x, embed=embed)


def _layer(hid=32, n=1, cin=None, seed=5, down_cin=None):
    from glsdet_amd.arch import _Table
    from glsdet_amd.synth import synth_state_dict
    t = _Table()
    if down_cin is not None:
        t.conv_bn("d", down_cin, 2 * hid, 3)
    t.csp("m", cin or 2 * hid, 2 * hid, n, False)
    return synth_state_dict(t, seed)


def _unfused_env(monkeypatch, on=True):
    """the plain four launches, every product on the 32x32x16 MFMA shape the fused kernel is built on"""
    for k in ("GLSDET_NO_CHAIN", "GLSDET_NO_BNECK_FUSION", "GLSDET_NO_M16"):
        if on:
            monkeypatch.setenv(k, "1")
        else:
            monkeypatch.delenv(k, raising=False)


def _run_csp(eng, sd, x, shortcut, out=None, **kw):
    from glsdet_amd.nets import NetBuilder
    plan = eng.new_plan()
    with plan:
        y = NetBuilder(eng, sd).csp("m", x, shortcut, out=out, **kw)
    plan.run()
    torch.cuda.synchronize()
    return y.to_nchw().cpu(), plan


def _packs(eng, sd):
    from glsdet_amd.nets import NetBuilder
    b = NetBuilder(eng, sd)
    part = b._bn_part
    return [eng.pack_conv([part("m.conv1"), part("m.conv2")], 64), eng.pack_conv([part("m.m.0.conv1")], 32),
            eng.pack_conv([part("m.m.0.conv2")], 32), eng.pack_conv([part("m.conv3")], 64)]


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut,batch,hw", [
    (True, 1, (4, 16)),        # one 4 x 16 tile / half an 8 x 16 one
    (True, 2, (20, 24)),       # several tiles, ragged in y and x
    (False, 2, (41, 70)),
    (True, 1, (7, 5)),         # smaller than a tile
    (False, 1, (33, 17)),      # one pixel past a tile boundary in both directions
    (True, 2, (100, 650)),     # 41 tile columns walked in strips of 3: the last strip ends after 2
    (False, 2, (100, 672)),    # 42 tile columns: a whole number of strips
])
def test_whole_layer_equals_the_four_launches_bit_for_bit(engines, monkeypatch, shortcut, batch, hw):
    from glsdet_amd.synth import synth_input
    eng = engines["f16"]
    sd = _layer()
    x = synth_input((batch, 64, hw[0], hw[1]), 9)
    _unfused_env(monkeypatch)
    ref, plan_ref = _run_csp(eng, sd, _upload(eng, x), shortcut)
    got, plan = _run_csp(eng, sd, _upload(eng, x), shortcut, whole=True)
    want = O.csp_layer(sd, "m", x.half().float(), shortcut)
    bar = F16_TOL * max(1.0, float(want.abs().max()))
    print("max |fused - oracle| %.3e, max |unfused - oracle| %.3e, bar %.3e, differing %d" %
          (float((got - want).abs().max()), float((ref - want).abs().max()), bar, int((got != ref).sum())))
    assert (plan.num_ops, plan_ref.num_ops) == (1, 4)
    assert "csp_fused" in plan.ops()[0]["name"] and plan.ops()[0]["kind"] == 0
    assert torch.equal(got, ref)
    assert float((got - want).abs().max()) <= bar and float((ref - want).abs().max()) <= bar


@pytest.mark.gpu
@pytest.mark.parametrize("hint", [0, 1])
@pytest.mark.parametrize("shortcut,hw", [(True, (21, 37)), (False, (9, 130))])
def test_entry_point_both_tile_heights_on_strided_views(engines, monkeypatch, hint, shortcut, hw):
    """x a channel slice of a wider buffer, y written into a channel slice of another one (strided in n, h and w), both
    tile heights; the bytes around the output window stay untouched; the in-place call is refused."""
    from glsdet_amd.engine import _stream_ptr
    from glsdet_amd.synth import synth_input
    eng = engines["f16"]
    sd = _layer()
    x = synth_input((2, 64, hw[0], hw[1]), 11)
    _unfused_env(monkeypatch)
    ref, _ = _run_csp(eng, sd, _upload(eng, x), shortcut)
    xv = _upload(eng, x, embed=(128, 32))
    yv = _upload(eng, torch.full((2, 64, hw[0], hw[1]), 3.0), embed=(192, 64))
    before = yv.buf.clone()
    d = eng._csp_desc(xv, yv, _packs(eng, sd), shortcut)
    rc = eng.lib.glsdet_csp_fused(C.byref(d), hint, _stream_ptr(eng.stream))
    assert rc == 0, eng.lib.glsdet_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(yv.to_nchw().cpu(), ref)
    # nothing outside the window's 64 channels was written
    mask = torch.ones(2, hw[0] + 2, hw[1] + 2, 192, dtype=torch.bool)
    mask[:, 1:-1, 1:-1, 64:128] = False
    a = before.view(torch.float16)[: mask.numel()].view(mask.shape).cpu()
    b = yv.buf.view(torch.float16)[: mask.numel()].view(mask.shape).cpu()
    assert torch.equal(a[mask], b[mask])
    d2 = eng._csp_desc(xv, xv, _packs(eng, sd), shortcut)
    assert eng.lib.glsdet_csp_fused(C.byref(d2), hint, _stream_ptr(eng.stream)) < 0
    assert "in place" in eng.lib.glsdet_last_error().decode()


@pytest.mark.gpu
def test_with_the_downsampling_conv_in_front(engines, monkeypatch):
    """darknet.py:174-195 `Sequential(BaseConv(.., 3, 2), CSPLayer(..))`: the producer is emitted on its own, then the layer
    as one launch: 2 ops, the bits of the separately emitted stride-2 conv followed by the unfused layer."""
    from glsdet_amd.nets import NetBuilder
    from glsdet_amd.synth import synth_input
    eng = engines["f16"]
    sd = _layer(down_cin=32)
    x = synth_input((2, 32, 40, 52), 9)
    _unfused_env(monkeypatch)
    plan0 = eng.new_plan()
    with plan0:
        b = NetBuilder(eng, sd)
        ref = b.csp("m", b.cba("d", _upload(eng, x), 2), True)
    plan0.run()
    torch.cuda.synchronize()
    got, plan = _run_csp(eng, sd, None, True, down=("d", _upload(eng, x)), whole=True)
    assert plan.num_ops == 2 and plan0.num_ops == 5
    assert torch.equal(got, ref.to_nchw().cpu())
    r = lambda v: v.half().float()
    want = O.csp_layer(sd, "m", r(O.base_conv(sd, "d", r(x), 2)), True)
    assert float((got - want).abs().max()) <= F16_TOL * max(1.0, float(want.abs().max()))


@pytest.mark.gpu
def test_default_lowering_is_unchanged(engines, monkeypatch):
    """csp() without the keyword never takes the whole-layer form: the hid-32 layer keeps its three launches (entry, fused
    Bottleneck, conv3), four with the fusions switched off, two / three behind a chained stride-2 conv."""
    from glsdet_amd.synth import synth_input
    eng = engines["f16"]
    sd = _layer(down_cin=32)
    x = synth_input((2, 64, 20, 24), 9)
    _unfused_env(monkeypatch, False)
    _, plan = _run_csp(eng, sd, _upload(eng, x), True)
    _, plan_kw = _run_csp(eng, sd, _upload(eng, x), True, whole=False)
    assert [o["name"] for o in plan.ops()] == [o["name"] for o in plan_kw.ops()]
    assert plan.num_ops == 3 and not any("csp_fused" in o["name"] for o in plan.ops())
    xd = synth_input((2, 32, 40, 52), 9)
    _, pland = _run_csp(eng, sd, None, True, down=("d", _upload(eng, xd)))
    assert pland.num_ops == 3 and not any("csp_fused" in o["name"] for o in pland.ops())
    monkeypatch.setenv("GLSDET_NO_CHAIN", "1")
    monkeypatch.setenv("GLSDET_NO_BNECK_FUSION", "1")
    _, plan4 = _run_csp(eng, sd, _upload(eng, x), True)
    assert plan4.num_ops == 4


@pytest.mark.gpu
@pytest.mark.parametrize("shortcut", [True, False])
def test_border_pixels_with_large_bn_biases(engines, monkeypatch, shortcut):
    """silu(bias) of m.0.conv1 is far from 0 here: the 3x3 must see ZEROS outside the image, not the hidden tensor's value
    at a zero input.  The first / last rows and columns equal the unfused form (and all the others)."""
    from glsdet_amd.synth import synth_input
    eng = engines["f16"]
    sd = _layer(seed=7)
    for k in ("m.conv1", "m.conv2", "m.m.0.conv1", "m.m.0.conv2", "m.conv3"):
        sd[k + ".bn.bias"] = sd[k + ".bn.bias"] + 2.5
    x = synth_input((2, 64, 19, 35), 13)
    _unfused_env(monkeypatch)
    ref, _ = _run_csp(eng, sd, _upload(eng, x), shortcut)
    got, plan = _run_csp(eng, sd, _upload(eng, x), shortcut, whole=True)
    assert plan.num_ops == 1
    for name, sl in (("top", (slice(None), slice(None), 0)), ("bottom", (slice(None), slice(None), -1)),
                     ("left", (slice(None), slice(None), slice(None), 0)), ("right", (slice(None), slice(None), slice(None), -1))):
        assert torch.equal(got[sl], ref[sl]), name
    assert torch.equal(got, ref)
    want = O.csp_layer(sd, "m", x.half().float(), shortcut)
    assert float((got - want).abs().max()) <= F16_TOL * max(1.0, float(want.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode,hid,n,cin", [("f32", 32, 1, 64), ("f16", 64, 1, 128), ("f16", 32, 2, 64), ("f16", 32, 1, 128)])
def test_unsupported_layers_keep_the_old_lowering(engines, monkeypatch, mode, hid, n, cin):
    """f32 engine, hidden 64, two Bottlenecks, 128 input channels: csp(..., whole=True) emits exactly what csp(...) emits
    and still meets the oracle; the entry point refuses such operands before any launch."""
    from glsdet_amd.engine import _stream_ptr
    from glsdet_amd.synth import synth_input
    eng = engines[mode]
    sd = _layer(hid=hid, n=n, cin=cin)
    x = synth_input((2, cin, 20, 24), 9)
    _unfused_env(monkeypatch, False)
    a, plan_a = _run_csp(eng, sd, _upload(eng, x), True)
    b, plan_b = _run_csp(eng, sd, _upload(eng, x), True, whole=True)
    assert [o["name"] for o in plan_a.ops()] == [o["name"] for o in plan_b.ops()]
    assert torch.equal(a, b)
    want = O.csp_layer(sd, "m", x if mode == "f32" else x.half().float(), True)
    assert float((b - want).abs().max()) <= (5e-5 if mode == "f32" else F16_TOL) * max(1.0, float(want.abs().max()))
    xg = (2, 20, 24, cin, 20 * 24 * cin, 24 * cin, cin)
    og = (2, 20, 24, 2 * hid, 20 * 24 * 2 * hid, 24 * 2 * hid, 2 * hid)
    packs64 = _packs(engines["f16"], _layer())
    if mode == "f32" or cin != 64 or hid != 32:
        assert not eng.csp_fused_wins(xg, og, packs64, True)
        xv, yv = _upload(eng, x), eng.tensor(2, 20, 24, 2 * hid)
        d = eng._csp_desc(xv, yv, packs64, True)
        assert eng.lib.glsdet_csp_fused(C.byref(d), 0, _stream_ptr(eng.stream)) < 0
        assert "csp_fused" in eng.lib.glsdet_last_error().decode()


def _compile(kind, sd, x, use_graph):
    from glsdet_amd.detector import HipDetector
    det = HipDetector(kind, sd, dtype="f16")
    c = det.compile(x.shape[0], x.shape[2], x.shape[3], None, use_graph=use_graph)
    for _ in range(2):
        det.run(c, x.cuda())
    torch.cuda.synchronize()
    return [l.to_nchw(l.c).cpu() for l in c.levels], c.plan.ops()


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ["gl_s_seed0", "base_s_seed0"])
@pytest.mark.parametrize("size", ["golden", "1x3x800x1344"])
def test_whole_model_logits_do_not_move(golden, shapes, monkeypatch, tag, size):
    """YOLOX-s with and without the GL-fusion neck, fp16, inside a captured graph as the benchmark runs it: with
    GLSDET_NO_CSP_FUSION the plan is the previous lowering launch for launch (no csp_fused op, one op more: conv1|conv2
    chained onto dark2.0 + fused Bottleneck + conv3 instead of dark2.0 + the layer); the logits are the same bits."""
    meta, sd, x, _, _ = model_case(golden, shapes, tag)
    if size != "golden":
        x = O.synth_input((1, 3, 800, 1344), 321)
    kind = "gl" if tag.startswith("gl") else "base"
    monkeypatch.delenv("GLSDET_NO_CSP_FUSION", raising=False)
    new, ops_new = _compile(kind, sd, x, True)
    monkeypatch.setenv("GLSDET_NO_CSP_FUSION", "1")
    old, ops_old = _compile(kind, sd, x, True)
    assert sum("csp_fused" in o["name"] for o in ops_new) == 1
    assert not any("csp_fused" in o["name"] for o in ops_old)
    assert len(ops_old) == len(ops_new) + 1
    assert len(new) == len(old) == 3
    for a, b in zip(new, old):
        assert torch.equal(a, b)


# ---- no GPU: the entry point refuses malformed operands on the host, before anything is launched (the pointers below are
# never dereferenced)
def _view(n, h, w, c, dtype=0, base=0x10000, extra=0):
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = c, w * c, h * w * c
    v.alloc_lo, v.alloc_hi = base, base + n * h * w * c * es + extra
    return v


def test_entry_point_validates_its_operands_on_the_host():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    lib = _lib.load()
    err = lambda: lib.glsdet_last_error().decode()

    def desc(x, y, **kw):
        d = _lib.CspDesc()
        d.x, d.y = x, y
        for i, q in enumerate(("12", "m1", "m2", "3")):
            setattr(d, "w" + q, 0x400000 + i * 0x10000)
            setattr(d, "scale" + q, 0x500000 + i * 0x1000)
            setattr(d, "bias" + q, 0x600000 + i * 0x1000)
        d.act, d.shortcut = _lib.ACT["silu"], 1
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    x, y = _view(2, 8, 10, 64), _view(2, 8, 10, 64, base=0x200000)
    call = lambda d, hint=0: lib.glsdet_csp_fused(C.byref(d), hint, None)
    assert lib.glsdet_csp_fused(None, 0, None) == -1
    # extents: output of another size, other channel counts
    assert call(desc(x, _view(2, 8, 9, 64, base=0x200000))) == -1 and "extent" in err()
    assert call(desc(_view(2, 8, 10, 128), y)) == -1 and "64 -> 64" in err()
    assert call(desc(x, _view(2, 8, 10, 32, base=0x200000))) == -1 and "64 -> 64" in err()
    # dtype
    assert call(desc(_view(2, 8, 10, 64, dtype=1), _view(2, 8, 10, 64, dtype=1, base=0x200000))) == -1 and "fp16" in err()
    # a view that reaches outside its allocation / a misaligned one / misaligned weights
    short = _view(2, 8, 10, 64)
    short.alloc_hi -= 64
    assert call(desc(short, y)) == -2
    assert call(desc(_view(2, 8, 10, 64, base=0x10002, extra=16), y)) == -3
    assert call(desc(x, y, wm2=0x400008)) == -3 and "aligned" in err()
    assert call(desc(x, y, scale3=0)) == -1 and "null" in err()
    # activation, shortcut flag, hint, in place
    assert call(desc(x, y, act=_lib.ACT["relu"])) == -1 and "SiLU" in err()
    assert call(desc(x, y, shortcut=2)) == -1
    assert call(desc(x, y), hint=2) == -1 and "hint" in err()
    assert call(desc(x, x)) == -1 and "in place" in err()
    best, us = C.c_int32(0), C.c_float(0)
    assert lib.glsdet_csp_fused_tune(C.byref(desc(x, _view(2, 8, 9, 64, base=0x200000))), None, C.byref(best), C.byref(us)) == -1
