"""glsdet_layernorm / glsdet_window_attention / glsdet_patch_merge (csrc/swin.hip) on the GPU, in both storage types.

Every destination is a strided view of a sentinel-filled buffer that is compared WHOLE; NaN surrounds every input view.
  LayerNorm   bit for bit on rows of two values m +- 1.5 with eps = 1.75 (mean m, variance 2.25, var + eps = 4 and
              rstd = 0.5 are exact in any order; gamma, beta multiples of 1 / 4), over C = 32 / 96 / 768 / 1024 and 1 / 63 /
              64 / 65 tokens, all four dtype pairs, one case past the grid cap; generic rows and rows offset by 1e3 within
              swin_reference.layernorm_bound
  attention   'onehot': every row's largest logit more than ONEHOT_MARGIN = 110 above the rest (asserted on the host):
              expf underflows to exactly 0, the weights are exactly one-hot, the output is the winner's v bit for bit --
              padded winners (v = the bias) included.  A row that only the mask decides leads by at most 100, where fp32
              expf gives a subnormal and not 0: such rows are covered by 'regions' (equal logits inside each mask region,
              the weights 1 / count: held to swin_reference.regions_bound, (N + 2) u max |v|, i.e. at most 66 ulp-halves
              for a full 8 x 8 window).  'continuous': within the a-priori per-element bound of
              swin_reference.window_attention(extras=...), derived before any kernel error was seen.
  merge       bit for bit (a permutation with zero fill)
A refused call leaves its destination untouched; all three record into a plan and replay from a captured graph."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import swin_reference as S

pytestmark = pytest.mark.gpu

_TT = {"f16": torch.float16, "f32": torch.float32}
SENTINEL = -77.25


def _lib():
    from glsdet_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Placed:
    """an NHWC view inside a larger device buffer.  layout: 'dense' | 'window' (rows 2.., columns 3.. of a map 3 rows and 4
    columns larger) | 'channels' (channels 32.. of a buffer 64 channels wider)"""

    def __init__(self, shape, dt, layout, fill):
        from glsdet_amd._lib import F16, F32
        from glsdet_amd.engine import TView
        n, h, w, c = shape
        H, W, Ct, h0, w0, c0 = {"dense": (h, w, c, 0, 0, 0), "window": (h + 3, w + 4, c, 2, 3, 0),
                                "channels": (h, w, c + 64, 0, 0, 32)}[layout]
        self.host = torch.full((n, H, W, Ct), fill, dtype=_TT[dt])
        self.box = (slice(None), slice(h0, h0 + h), slice(w0, w0 + w), slice(c0, c0 + c))
        self.dt, self.shape = dt, shape
        self.geo = (TView, (h0 * W + w0) * Ct + c0, n, h, w, c, H * W * Ct, W * Ct, Ct, F16 if dt == "f16" else F32)
        self.dev = None

    def put(self, x):
        self.host[self.box] = x.to(_TT[self.dt])
        return self

    def upload(self):
        self.dev = self.host.cuda().contiguous()
        TView, *rest = self.geo
        self.view = TView(self.dev.view(torch.uint8).reshape(-1), *rest)
        return self

    def read(self):
        return self.dev.cpu()[self.box].double()

    def frame_intact(self, want=None):
        """the whole buffer equals the host image (with `want` in the view), bit for bit; NaN compares by bits"""
        ref = self.host.clone()
        if want is not None:
            ref[self.box] = want.to(_TT[self.dt])
        bits = torch.int16 if self.dt == "f16" else torch.int32
        return torch.equal(self.dev.cpu().view(bits), ref.view(bits))


def _src(x, dt, layout="window"):
    assert torch.equal(x.to(_TT[dt]).double(), x), "the operand must be representable in the storage type"
    return Placed(tuple(x.shape), dt, layout, float("nan")).put(x).upload()


def _dst(shape, dt, layout="window"):
    return Placed(shape, dt, layout, SENTINEL).upload()


def _bits_equal(got, want, dt):
    bits = torch.int16 if dt == "f16" else torch.int32
    return torch.equal((got.to(_TT[dt]) + 0.0).view(bits), (want.to(_TT[dt]) + 0.0).view(bits))


# ------------------------------------------------------------------------------------------------------- LayerNorm
def _ln(src, dst, g, b, eps):
    _l, lib = _lib()
    gd, bd = g.float().cuda(), b.float().cuda()
    _l.check(lib.glsdet_layernorm(C.byref(src.view.as_c()), C.byref(dst.view.as_c()), gd.data_ptr(), bd.data_ptr(), eps,
                                  _stream()), "layernorm")
    torch.cuda.synchronize()
    return dst.read()


def _two_value(shape, seed):
    rng = np.random.default_rng([seed] + list(shape))
    n, h, w, c = shape
    m = rng.integers(-32, 33, (n, h, w, 1)) / 4.0
    sign = np.stack([rng.permutation(np.repeat([1.0, -1.0], c // 2)) for _ in range(n * h * w)]).reshape(n, h, w, c)
    g, b = rng.integers(-8, 9, c) / 4.0, rng.integers(-8, 9, c) / 4.0
    f = lambda t: torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))
    return f(m + 1.5 * sign), f(g), f(b), f(0.75 * sign * g + b)


_TOKENS = {1: (1, 1, 1), 63: (1, 7, 9), 64: (2, 4, 8), 65: (1, 5, 13)}


@pytest.mark.parametrize("dti,dto", [("f16", "f16"), ("f32", "f32"), ("f32", "f16"), ("f16", "f32")])
@pytest.mark.parametrize("C_", [32, 96, 768, 1024])
def test_layernorm_is_exact_on_two_value_rows(C_, dti, dto):
    for t, (n, h, w) in _TOKENS.items():
        x, g, b, want = _two_value((n, h, w, C_), 11)
        src = _src(x, dti, "window" if t != 64 else "channels")
        dst = _dst((n, h, w, C_), dto, "channels" if t % 2 else "window")
        got = _ln(src, dst, g, b, 1.75)
        assert _bits_equal(got, want, dto), (t, float((got - want).abs().max()))
        assert dst.frame_intact(want), "wrote outside the output view"
        assert src.frame_intact(), "the input was written"


@pytest.mark.parametrize("C_", [1536, 4096])
def test_layernorm_on_the_rows_of_the_merges(C_):
    """4C of a merge: 1536 at Swin-T's last one, 4096 the entry point's limit -- two-value rows bit for bit, normal rows
    within the derived bound, fp32 in and fp16 out as the builder calls it, and fp32 to fp32"""
    for dto in ("f16", "f32"):
        x, g, b, want = _two_value((1, 5, 13, C_), 14)
        dst = _dst((1, 5, 13, C_), dto, "channels")
        got = _ln(_src(x, "f32"), dst, g, b, 1.75)
        assert _bits_equal(got, want, dto) and dst.frame_intact(want)
        rng = np.random.default_rng([15, C_])
        x = torch.from_numpy(rng.standard_normal((1, 5, 13, C_))).float().double()
        g = torch.from_numpy(rng.uniform(0.7, 1.3, C_)).float().double()
        b = torch.from_numpy(0.2 * rng.standard_normal(C_)).float().double()
        eps = float(np.float32(1e-5))
        bound, want = S.layernorm_bound(x, g, b, eps, out_f16=dto == "f16")
        err = (_ln(_src(x, "f32"), _dst((1, 5, 13, C_), dto), g, b, eps) - want).abs()
        print("layernorm f32->%s C=%d: worst error / bound %.3f" % (dto, C_, float((err / bound).max())))
        assert bool((err <= bound).all())


def test_layernorm_in_place_on_the_very_same_view():
    x, g, b, want = _two_value((2, 4, 8, 96), 16)
    for dt in ("f16", "f32"):
        buf = _src(x, dt, "window")
        assert _bits_equal(_ln(buf, buf, g, b, 1.75), want, dt) and buf.frame_intact(want)


def test_layernorm_beyond_the_grid_cap():
    shape = (1, 129, 128, 32)                    # 16512 tokens > 4096 workgroups of 4
    x, g, b, want = _two_value(shape, 12)
    for dt in ("f16", "f32"):
        src, dst = _src(x, dt, "dense"), _dst(shape, dt, "window")
        got = _ln(src, dst, g, b, 1.75)
        assert _bits_equal(got, want, dt) and dst.frame_intact(want)


@pytest.mark.parametrize("dti,dto", [("f16", "f16"), ("f32", "f32"), ("f32", "f16"), ("f16", "f32")])
@pytest.mark.parametrize("offset", [0.0, 1e3])
def test_layernorm_meets_the_derived_bound(offset, dti, dto):
    for C_, (n, h, w) in ((32, (1, 5, 13)), (96, (2, 4, 8)), (768, (1, 7, 9)), (1024, (1, 3, 3))):
        rng = np.random.default_rng([13, C_, int(offset)])
        x = torch.from_numpy(rng.standard_normal((n, h, w, C_)) + offset).to(_TT[dti]).double()
        g = torch.from_numpy(rng.uniform(0.7, 1.3, C_)).float().double()
        b = torch.from_numpy(0.2 * rng.standard_normal(C_)).float().double()
        eps = float(np.float32(1e-5))
        bound, want = S.layernorm_bound(x, g, b, eps, out_f16=dto == "f16")
        src, dst = _src(x, dti), _dst((n, h, w, C_), dto)
        got = _ln(src, dst, g, b, eps)
        err = (got - want).abs()
        print("layernorm %s->%s C=%d offset %g: worst error / bound %.3f, error %.2e" % (dti, dto, C_, offset,
                                                                                       float((err / bound).max()), float(err.max())))
        assert bool((err <= bound).all())
        assert dst.frame_intact(got)


# ------------------------------------------------------------------------------------------------------- attention
def _attn(src, dst, table, bias, heads, ws, shift, scale=None):
    _l, lib = _lib()
    td = table.float().cuda().contiguous()
    bd = bias.float().cuda().contiguous() if bias is not None else None
    _l.check(lib.glsdet_window_attention(C.byref(src.view.as_c()), C.byref(dst.view.as_c()), td.data_ptr(),
                                         bd.data_ptr() if bd is not None else None, heads, ws, shift,
                                         float(np.float32(32 ** -0.5 if scale is None else scale)), _stream()), "window_attention")
    torch.cuda.synchronize()
    return dst.read()


# (H, W, heads, n, ws, shift): 7x7 one full window; 4x4 smaller than the window; 8x9, 15x13 padded; 14x14 four full windows;
# ws 4 and 8 once each; 92x92 at ws 2 with n = 2: 4232 windows, past the cap of 4096 workgroups
_ATT = [(7, 7, 1, 1, 7, 0), (7, 7, 3, 2, 7, 3), (4, 4, 1, 1, 7, 3), (4, 4, 4, 2, 7, 0), (8, 9, 3, 1, 7, 3), (8, 9, 1, 2, 7, 0),
        (14, 14, 4, 1, 7, 3), (14, 14, 1, 1, 7, 0), (15, 13, 3, 2, 7, 3), (15, 13, 1, 1, 7, 0), (9, 6, 1, 1, 4, 2),
        (10, 17, 3, 1, 8, 3), (92, 92, 1, 2, 2, 1)]
_SCALE = float(np.float32(32 ** -0.5))


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("H,W,heads,n,ws,shift", _ATT, ids=["%dx%d-h%d-n%d-ws%d-s%d" % c for c in _ATT])
def test_attention_exact_regimes(H, W, heads, n, ws, shift, dt):
    C_ = 32 * heads
    # ---- one-hot
    qkv, table, bias = S.attention_operands(n, H, W, heads, ws, "onehot", 21)
    ex = {}
    want = S.window_attention(qkv, table, bias, heads, ws, shift, scale=_SCALE, extras=ex)
    assert float(ex["margin"].min()) > S.ONEHOT_MARGIN, float(ex["margin"].min())
    if H % ws or W % ws:                          # a padded map: some real rows are won by a padded token (v = the bias)
        assert int(ex["padded_winner"].sum()) >= 4, int(ex["padded_winner"].sum())
    src, dst = _src(qkv, dt), _dst((n, H, W, C_), dt, "channels")
    got = _attn(src, dst, table, bias, heads, ws, shift)
    assert not torch.isnan(got).any(), "NaN: a neighbour of the view was read"
    assert _bits_equal(got, want, dt), "one-hot: %d of %d elements differ, worst %.3e" % (
        int((got != want.float().double()).sum()), got.numel(), float((got - want).abs().max()))
    assert dst.frame_intact(got) and src.frame_intact()
    # ---- equal logits inside each mask region
    qkv, table, bias = S.attention_operands(n, H, W, heads, ws, "regions", 22)
    want = S.window_attention(qkv, table, bias, heads, ws, shift, scale=_SCALE)
    src, dst = _src(qkv, dt), _dst((n, H, W, C_), dt)
    got = _attn(src, dst, table, bias, heads, ws, shift)
    bound = S.regions_bound(4.0, ws * ws, out_f16=dt == "f16")
    err = float((got - want).abs().max())
    print("attention regions %s %dx%d ws %d shift %d: error %.3e, bound %.3e" % (dt, H, W, ws, shift, err, bound))
    assert err <= bound
    assert dst.frame_intact(got)


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("H,W,heads,n,ws,shift", _ATT, ids=["%dx%d-h%d-n%d-ws%d-s%d" % c for c in _ATT])
def test_attention_meets_the_a_priori_bound(H, W, heads, n, ws, shift, dt):
    qkv, table, bias = S.attention_operands(n, H, W, heads, ws, "continuous", 23)
    qkv, bias = qkv.to(_TT[dt]).double(), bias.to(_TT[dt]).double()
    ex = {}
    want = S.window_attention(qkv, table, bias, heads, ws, shift, scale=_SCALE, extras=ex)
    bound = ex["bound"] + (2.0 ** -11 * want.abs() + 2.0 ** -25 if dt == "f16" else 0.0)
    src, dst = _src(qkv, dt), _dst((n, H, W, 32 * heads), dt, "channels")
    got = _attn(src, dst, table, bias, heads, ws, shift)
    err = (got - want).abs()
    print("attention continuous %s %dx%d h%d ws %d shift %d: worst error / bound %.3f, error %.2e" % (
        dt, H, W, heads, ws, shift, float((err / bound).max()), float(err.max())))
    assert bool((err <= bound).all())
    assert dst.frame_intact(got)
    again = _attn(src, _dst((n, H, W, 32 * heads), dt, "channels"), table, bias, heads, ws, shift)
    assert _bits_equal(again, got, dt), "two runs differ"


def test_attention_without_a_qkv_bias_pads_with_zeros():
    qkv, table, _ = S.attention_operands(1, 8, 9, 1, 7, "onehot", 24)
    want = S.window_attention(qkv, table, None, 1, 7, 3, scale=_SCALE)
    got = _attn(_src(qkv, "f32"), _dst((1, 8, 9, 32), "f32"), table, None, 1, 7, 3)
    assert _bits_equal(got, want, "f32")


# ------------------------------------------------------------------------------------------------------- patch merge
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("H,W", [(5, 7), (6, 6), (1, 1), (7, 4)])
@pytest.mark.parametrize("C_", [32, 96])
def test_patch_merge_is_exact(C_, H, W, dt):
    _l, lib = _lib()
    rng = np.random.default_rng([31, C_, H, W])
    x = torch.from_numpy(rng.integers(-512, 513, (2, H, W, C_)) / 64.0)
    want = S.patch_merge(x)
    for li, lo in (("window", "channels"), ("channels", "window"), ("dense", "dense")):
        src, dst = _src(x, dt, li), _dst(tuple(want.shape), dt, lo)
        _l.check(lib.glsdet_patch_merge(C.byref(src.view.as_c()), C.byref(dst.view.as_c()), _stream()), "patch_merge")
        torch.cuda.synchronize()
        assert _bits_equal(dst.read(), want, dt)
        assert dst.frame_intact(want) and src.frame_intact()


# ------------------------------------------------------------------------------------------------------- refusals, plans
def test_refused_calls_launch_nothing():
    _l, lib = _lib()
    qkv, table, bias = S.attention_operands(1, 8, 9, 1, 7, "onehot", 25)
    src, dst = _src(qkv, "f32"), _dst((1, 8, 9, 32), "f32")
    td, bd = table.float().cuda(), bias.float().cuda()
    g = torch.ones(32, device="cuda")
    x32 = _src(qkv[..., :32].contiguous(), "f32")
    m = _dst((1, 4, 5, 128), "f32")
    s = _stream()
    V = lambda p: C.byref(p.view.as_c())
    wide_q, wide_y = _dst((1, 2, 2, 3 * 1056), "f32", "dense"), _dst((1, 2, 2, 1056), "f32", "dense")

    def outside(p):                               # the same view, said to live in an allocation that ends inside it
        v = p.view.as_c()
        v.alloc_hi = v.base + 64
        return v

    inside_src = src.view.as_c()                  # a [1, 8, 9, 32] destination that lies inside qkv's own span
    inside_src.c = 32
    head_x32, shifted_x32 = x32.view.as_c(), x32.view.as_c()     # columns 0..7 and 1..8 of x32: they overlap, and differ
    head_x32.w = shifted_x32.w = x32.view.w - 1
    shifted_x32.base += x32.view.sw * 4
    calls = [
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr(), bd.data_ptr(), 1, 9, 0, 0.17, s),
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr(), bd.data_ptr(), 1, 7, 7, 0.17, s),
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr(), bd.data_ptr(), 2, 7, 3, 0.17, s),
        lambda: lib.glsdet_window_attention(V(src), V(dst), None, bd.data_ptr(), 1, 7, 3, 0.17, s),
        lambda: lib.glsdet_window_attention(V(x32), V(dst), td.data_ptr(), bd.data_ptr(), 1, 7, 3, 0.17, s),
        lambda: lib.glsdet_layernorm(V(x32), V(dst), g.data_ptr(), g.data_ptr(), -1.0, s),
        lambda: lib.glsdet_layernorm(V(x32), V(dst), g.data_ptr(), None, 1e-5, s),
        lambda: lib.glsdet_layernorm(V(src), V(dst), g.data_ptr(), g.data_ptr(), 1e-5, s),
        lambda: lib.glsdet_patch_merge(V(x32), V(dst), s),
        lambda: lib.glsdet_patch_merge(V(src), V(m), s),
        # alignment, width, scale, sign, bounds, overlap
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr() + 2, bd.data_ptr(), 1, 7, 3, 0.17, s),
        lambda: lib.glsdet_window_attention(V(wide_q), V(wide_y), td.data_ptr(), bd.data_ptr(), 33, 7, 3, 0.17, s),
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr(), bd.data_ptr(), 1, 7, 3, float("inf"), s),
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr(), bd.data_ptr(), 1, 7, 3, float("nan"), s),
        lambda: lib.glsdet_window_attention(V(src), V(dst), td.data_ptr(), bd.data_ptr(), 1, -7, 0, 0.17, s),
        lambda: lib.glsdet_window_attention(V(src), C.byref(outside(dst)), td.data_ptr(), bd.data_ptr(), 1, 7, 3, 0.17, s),
        lambda: lib.glsdet_window_attention(V(src), C.byref(inside_src), td.data_ptr(), bd.data_ptr(), 1, 7, 3, 0.17, s),
        lambda: lib.glsdet_layernorm(V(x32), V(dst), g.data_ptr() + 4, g.data_ptr(), 1e-5, s),
        lambda: lib.glsdet_layernorm(V(x32), C.byref(outside(dst)), g.data_ptr(), g.data_ptr(), 1e-5, s),
        lambda: lib.glsdet_layernorm(C.byref(head_x32), C.byref(shifted_x32), g.data_ptr(), g.data_ptr(), 1e-5, s),
        lambda: lib.glsdet_patch_merge(V(x32), C.byref(outside(m)), s),
    ]
    for i, call in enumerate(calls):
        assert call() < 0 and lib.glsdet_last_error(), i
    torch.cuda.synchronize()
    assert dst.frame_intact() and m.frame_intact() and src.frame_intact() and x32.frame_intact() and wide_y.frame_intact()


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_the_three_ops_record_into_a_plan_and_replay_from_a_captured_graph(dt):
    """merge -> LayerNorm (two-value rows after the merge: x holds m +- 1.5 per pixel quadruple) -> attention on one-hot
    operands: recording launches nothing, the eager replay and the graph replay on NEW input give the exact results"""
    from glsdet_amd.engine import Engine
    eng = Engine(dt)
    H, W, heads, ws, shift = 8, 9, 3, 7, 3
    C_ = 32 * heads
    table_bias = S.attention_operands(1, H, W, heads, ws, "onehot", 26)[1:]

    def data(seed):
        qkv = S.attention_operands(1, H, W, heads, ws, "onehot", seed)[0]
        x, g, b, y = _two_value((1, 6, 6, 32), seed)
        return qkv, x, g, b, y

    qkv1, x1, g, b, y1 = data(27)
    qkv2, x2, _, _, y2 = data(28)
    # rows of the merge's 4C = 128 channels stay two-valued only where the four pixels share m: use a per-image m
    x1 = x1 - x1.mean(-1, keepdim=True) + 0.5
    x2 = x2 - x2.mean(-1, keepdim=True) - 1.25
    want_ln = lambda x: (0.5 * (S.patch_merge(x) - x.mean())) * 1.0 + 0.25
    srcq, srcx = _src(qkv1, dt), _src(x1, dt)
    dsta, dstm, dstl = _dst((1, H, W, C_), dt), _dst((1, 3, 3, 128), dt, "dense"), _dst((1, 3, 3, 128), dt, "channels")
    td, bd = (t.float().cuda() for t in table_bias)
    ones, quarter = torch.ones(128, device="cuda"), torch.full((128,), 0.25, device="cuda")
    plan = eng.new_plan()
    with plan:
        eng.patch_merge(srcx.view, out=dstm.view)
        eng.layernorm(dstm.view, ones, quarter, 1.75, out=dstl.view)
        eng.window_attention(srcq.view, td, bd, heads, ws, shift, _SCALE, out=dsta.view)
    torch.cuda.synchronize()
    assert plan.num_ops == 3 and dsta.frame_intact() and dstl.frame_intact(), "recording launched something"

    def check(qkv, x):
        wa = S.window_attention(qkv, table_bias[0], table_bias[1], heads, ws, shift, scale=_SCALE)
        assert _bits_equal(dsta.read(), wa, dt)
        assert _bits_equal(dstm.read(), S.patch_merge(x), dt)
        assert _bits_equal(dstl.read(), want_ln(x), dt)

    plan.run()
    torch.cuda.synchronize()
    check(qkv1, x1)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        plan.capture(st)
    st.synchronize()
    srcq.dev.copy_(srcq.put(qkv2).host)
    srcx.dev.copy_(srcx.put(x2).host)
    with torch.cuda.stream(st):
        plan.launch(st)
    st.synchronize()
    check(qkv2, x2)
