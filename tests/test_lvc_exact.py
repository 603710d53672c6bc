"""glsdet_lvc_encode / glsdet_lvc_gate / glsdet_channel_fuse (csrc/evc.hip) on the GPU, in both storage types.

Bit for bit in the two regimes of tests/cfp_reference.encode_operands in which every fp32 step is exact in any summation
order ('uniform': scale = 0, every weight 1 / 64; 'onehot': every foreign logit more than ONEHOT_MARGIN = 110 below the own
one -- asserted on the host per case -- so that expf gives exactly 0 and the own weight exactly 1), over layouts, slices,
tails and the fold; continuous operands to the a-priori per-element bound of cfp_reference.encode_bound, which
tests/test_cfp_reference.py shows the reference's own fp32 evaluation to meet on the same seeds.  Every output, E included,
lies in a sentinel-filled buffer that is compared whole; NaN surrounds every input view; the workspace starts dirty."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import cfp_reference as X

pytestmark = pytest.mark.gpu

_TT = {"f16": torch.float16, "f32": torch.float32}
SENTINEL = -77.25


def _lib():
    from glsdet_amd import _lib
    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _place(x, dt, layout):
    """x [n, C, h, w] fp32 (representable in dt) -> (TView onto a NaN-filled device buffer, the buffer).
    layout: 'dense' | 'window' (rows 2.., columns 3.. of a map 3 rows and 4 columns larger) | 'channels' (channels 32.. of a
    buffer 64 channels wider)"""
    from glsdet_amd._lib import F16, F32
    from glsdet_amd.engine import TView
    n, c, h, w = x.shape
    H, W, Ct, h0, w0, c0 = {"dense": (h, w, c, 0, 0, 0), "window": (h + 3, w + 4, c, 2, 3, 0), "channels": (h, w, c + 64, 0, 0, 32)}[layout]
    full = torch.full((n, H, W, Ct), float("nan"), dtype=_TT[dt])
    full[:, h0:h0 + h, w0:w0 + w, c0:c0 + c] = x.permute(0, 2, 3, 1).to(_TT[dt])
    buf = full.cuda().contiguous()
    return TView(buf.view(torch.uint8).reshape(-1), (h0 * W + w0) * Ct + c0, n, h, w, c, H * W * Ct, W * Ct, Ct, F16 if dt == "f16" else F32), buf


def _read(view, buf):
    n, h, w, c = view.n, view.h, view.w, view.c
    t = torch.as_strided(buf.reshape(-1), (n, h, w, c), (view.sn, view.sh, view.sw, 1), view.off)
    return t.permute(0, 3, 1, 2).float().cpu()


def _encode(view, cw, sc, dirty=True):
    """-> (E [n, 64, C] fp32 on the host, the whole sentinel-framed output buffer) through the C entry point"""
    _l, lib = _lib()
    n, c = view.n, view.c
    nbytes = lib.glsdet_lvc_encode_workspace_bytes(n, view.h, view.w, c)
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.full((nbytes + 256,), 0xFF if dirty else 0, dtype=torch.uint8, device="cuda")      # NaN bit patterns
    out = torch.full((n * 64 * c + 128,), SENTINEL, dtype=torch.float32, device="cuda")
    cwd, scd = cw.cuda().contiguous(), sc.cuda().contiguous()
    _l.check(lib.glsdet_lvc_encode(C.byref(view.as_c()), cwd.data_ptr(), scd.data_ptr(), ws.data_ptr(), nbytes,
                                   out.data_ptr() + 64 * 4, _stream()), "lvc_encode")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == (0xFF if dirty else 0)).all()), "wrote past the workspace"
    whole = out.cpu()
    assert bool((whole[:64] == SENTINEL).all()) and bool((whole[64 + n * 64 * c:] == SENTINEL).all()), "wrote outside E"
    return whole[64:64 + n * 64 * c].reshape(n, 64, c), whole


# (C, h, w, n, layout): pixel counts 1, 63 / 64 / 65 (a tile +- 1), 127 / 128 / 129 (a slice +- 1), 3 x 7, 135 and 50 x 84
# (two and 33 slices); C = 32 (half a channel chunk), 96 (a chunk and a half), 128, 640 (ten chunks)
_EXACT = [(32, 1, 1, 1, "dense"), (32, 7, 9, 3, "dense"), (32, 8, 8, 1, "dense"), (32, 5, 13, 1, "dense"),
          (96, 1, 127, 1, "dense"), (96, 8, 16, 3, "dense"), (96, 3, 43, 1, "dense"), (128, 3, 7, 3, "dense"),
          (640, 3, 7, 1, "dense"), (640, 9, 15, 1, "dense"), (128, 50, 84, 1, "dense"),
          (96, 5, 6, 3, "window"), (96, 9, 15, 2, "window"), (96, 4, 9, 2, "channels")]


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("C_,h,w,n,layout", _EXACT, ids=["c%d-%dx%d-n%d-%s" % c for c in _EXACT])
def test_encode_is_exact_in_the_two_exact_regimes(C_, h, w, n, layout, dt):
    for regime in ("uniform", "onehot"):
        x, cw, sc = X.encode_operands(C_, h, w, n, 40, regime)
        assert torch.equal(x.to(_TT[dt]).float(), x), "the operands must be representable in the storage type"
        if regime == "onehot":
            margin = X.onehot_margin(x, cw, sc)
            assert margin > X.ONEHOT_MARGIN, margin
        with torch.no_grad():
            want = X.encoding_expanded(x.double(), cw.double(), sc.double())       # all dyadic: exact in float64 as well
        assert torch.equal(want.float().double(), want)
        view, buf = _place(x, dt, layout)
        got, whole = _encode(view, cw, sc)
        assert not torch.isnan(got).any(), "%s: NaN (a neighbour of the view or the dirty workspace was read)" % regime
        # (+ 0.0: a zero keeps no sign -- float64 sums 0 * x over negative x to -0, the kernel's chains start from +0)
        assert torch.equal((got + 0.0).view(torch.int32), (want.float() + 0.0).view(torch.int32)), \
            "%s: %d of %d elements differ, worst %.3e" % (regime, int((got != want.float()).sum()), got.numel(),
                                                          float((got.double() - want).abs().max()))
        assert torch.equal(_read(view, buf.view(_TT[dt])), x), "the input was written"
        again, whole2 = _encode(view, cw, sc, dirty=False)
        assert torch.equal(whole.view(torch.int32), whole2.view(torch.int32)), "two runs differ"


_CONT = [(32, 5, 7, 2, 1), (96, 8, 8, 1, 2), (32, 50, 84, 1, 3), (256, 9, 13, 1, 4)]


@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("C_,h,w,n,seed", _CONT, ids=["c32-35", "c96-64", "c32-4200", "c256-117"])
def test_encode_meets_the_a_priori_bound_on_continuous_operands(C_, h, w, n, seed, dt):
    """the cases and seeds tests/test_cfp_reference.py runs the reference's fp32 evaluation on (f16: x rounded first)"""
    x, cw, sc = X.encode_operands(C_, h, w, n, seed, "continuous")
    x = x.to(_TT[dt]).float()
    bound, exact = X.encode_bound(x, cw, sc)
    view, _ = _place(x, dt, "window")
    got, whole = _encode(view, cw, sc)
    err = (got.double() - exact).abs()
    print("lvc_encode %s C=%d N=%d: worst error / bound %.3f, error %.2e of max |E|" % (
        dt, C_, h * w, float((err / bound).max()), float(err.max() / exact.abs().max())))
    assert bool((err <= bound).all())
    _, whole2 = _encode(view, cw, sc)
    assert torch.equal(whole.view(torch.int32), whole2.view(torch.int32)), "two runs differ"


# ------------------------------------------------------------------------------------------------------------- gate
@pytest.mark.parametrize("C_,n", [(32, 1), (96, 3), (640, 2)])
def test_gate_follows_its_documented_order(C_, n):
    """dyadic data on which every step of the documented chains is exact: the value in front of the sigmoid is then THE
    value, and the result is held to the SIGMOID tolerance of include/glsdet_hip.h (F32: 6 u |y| + 2^-120)"""
    _l, lib = _lib()
    rng = np.random.default_rng([77, C_, n])
    E = rng.integers(-4, 5, (n, 64, C_)) / 2.0
    a = rng.choice([0.5, 1.0], 64)
    b = rng.integers(-2, 3, 64) / 2.0
    W = rng.integers(-2, 3, (C_, C_)) / 16.0
    bias = rng.integers(-4, 5, C_) / 4.0
    v, want = X.gate_fp32(E, a, b, W, bias)
    v64 = bias[None] + np.einsum("oc,nc->no", W, np.maximum(a[None, :, None] * E + b[None, :, None], 0).mean(1))
    assert np.array_equal(v.astype(np.float64), v64), "the test data left the exact regime"
    assert np.abs(v).max() < 16 and v.std() > 0.5                    # neither saturated nor constant
    dev = lambda t: torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32)).cuda()
    out = torch.full((n * C_ + 128,), SENTINEL, dtype=torch.float32, device="cuda")
    ops = [dev(E), dev(a), dev(b), dev(W), dev(bias)]
    _l.check(lib.glsdet_lvc_gate(ops[0].data_ptr(), n, C_, ops[1].data_ptr(), ops[2].data_ptr(), ops[3].data_ptr(),
                                 ops[4].data_ptr(), out.data_ptr() + 256, _stream()), "lvc_gate")
    torch.cuda.synchronize()
    whole = out.cpu().numpy()
    assert (whole[:64] == SENTINEL).all() and (whole[64 + n * C_:] == SENTINEL).all()
    got = whole[64:64 + n * C_].reshape(n, C_).astype(np.float64)
    tol = 6 * 2.0 ** -24 * np.abs(want) + 2.0 ** -120
    assert (np.abs(got - want) <= tol).all(), float((np.abs(got - want) / tol).max())


# ------------------------------------------------------------------------------------------------------------- fuse
@pytest.mark.parametrize("dt", ["f16", "f32"])
@pytest.mark.parametrize("layout", ["dense", "window", "channels"])
def test_channel_fuse_is_exact_on_dyadic_data(dt, layout):
    """a, t multiples of 1/8 in [-4, 4], v multiples of 1/4 in [-2, 2]: a + a v and a + v t are multiples of 1/32 below 12,
    exact in fp32 and representable in fp16 -- bit for bit in both modes, into a fresh view and in place"""
    _l, lib = _lib()
    n, C_, h, w = 3, 96, 5, 7
    rng = np.random.default_rng([78, len(layout)])
    f = lambda t: torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    a, t = f(rng.integers(-32, 33, (n, C_, h, w)) / 8.0), f(rng.integers(-32, 33, (n, C_, h, w)) / 8.0)
    v0, v1 = f(rng.integers(-8, 9, (n, C_)) / 4.0), f(rng.integers(-8, 9, C_) / 4.0)
    want = {0: torch.relu(a + a * v0[:, :, None, None]), 1: a + v1[None, :, None, None] * t}
    for mode in (0, 1):
        assert torch.equal(want[mode].to(_TT[dt]).float(), want[mode])
        for in_place in (False, True):
            av, abuf = _place(a, dt, layout)
            tv, tbuf = _place(t, dt, "window")
            yv, ybuf = (av, abuf) if in_place else _place(torch.full_like(a, SENTINEL), dt, layout)
            before = ybuf.clone()
            vec = (v0 if mode == 0 else v1).cuda()
            _l.check(lib.glsdet_channel_fuse(C.byref(av.as_c()), C.byref(tv.as_c()) if mode == 1 else None, C.byref(yv.as_c()),
                                             vec.data_ptr(), mode, _stream()), "channel_fuse")
            torch.cuda.synchronize()
            got = _read(yv, ybuf.view(_TT[dt]))
            assert torch.equal(got, want[mode]), (mode, in_place)
            # everything around the output view is as it was (NaN compares by bits)
            ref = before.clone()
            torch.as_strided(ref.reshape(-1), (n, h, w, C_), (yv.sn, yv.sh, yv.sw, 1), yv.off).copy_(
                want[mode].permute(0, 2, 3, 1).to(_TT[dt]).cuda())
            bits = torch.int16 if dt == "f16" else torch.int32
            assert torch.equal(ybuf.view(bits), ref.view(bits)), "wrote outside the output view"
            assert torch.equal(_read(tv, tbuf.view(_TT[dt])), t)


# ---------------------------------------------------------------------------------------------- refusals, custom op
def test_a_refused_call_launches_nothing():
    _l, lib = _lib()
    x, cw, sc = X.encode_operands(32, 3, 7, 1, 1, "uniform")
    view, _ = _place(x, "f32", "dense")
    out = torch.full((64 * 32,), SENTINEL, dtype=torch.float32, device="cuda")
    nbytes = lib.glsdet_lvc_encode_workspace_bytes(1, 3, 7, 32)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    rc = lib.glsdet_lvc_encode(C.byref(view.as_c()), cw.cuda().data_ptr(), sc.cuda().data_ptr(), ws.data_ptr(), nbytes - 1,
                               out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert rc < 0 and "needed" in lib.glsdet_last_error().decode()
    assert bool((out == SENTINEL).all())


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_custom_op_eager_and_replayed_from_one_captured_graph(dt):
    import glsdet_amd.torch_ops  # noqa: F401
    C_, h, w, n = 96, 9, 15, 2
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(_TT[dt]).cuda()
    x1, cw, sc = X.encode_operands(C_, h, w, n, 50, "onehot")
    x2, _, _ = X.encode_operands(C_, h, w, n, 51, "onehot")
    cwd, scd = cw.cuda(), sc.cuda()
    want = [X.encoding_expanded(x.double(), cw.double(), sc.double()).float() for x in (x1, x2)]
    eager = torch.ops.glsdet.lvc_encode(nhwc(x2), cwd, scd)
    torch.cuda.synchronize()
    assert eager.shape == (n, 64, C_) and eager.dtype == torch.float32
    assert torch.equal((eager.cpu() + 0.0).view(torch.int32), (want[1] + 0.0).view(torch.int32))
    sx = nhwc(x1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.glsdet.lvc_encode(sx, cwd, scd)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = torch.ops.glsdet.lvc_encode(sx, cwd, scd)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal((sy.cpu() + 0.0).view(torch.int32), (want[0] + 0.0).view(torch.int32))
    sx.copy_(nhwc(x2))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(sy.view(torch.int32), eager.view(torch.int32))
    # the other two ops, on the encoding just made
    a, b = torch.ones(64, device="cuda"), torch.zeros(64, device="cuda")
    Wfc, bfc = torch.zeros(C_, C_, device="cuda"), torch.zeros(C_, device="cuda")
    gam = torch.ops.glsdet.lvc_gate(eager, a, b, Wfc, bfc)
    y = torch.ops.glsdet.channel_fuse(sx, None, gam, 0)
    torch.cuda.synchronize()
    assert torch.equal(gam.cpu(), torch.full((n, C_), 0.5))
    assert torch.equal(y.float().cpu(), torch.relu(1.5 * sx.float().cpu()))
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.lvc_encode(nhwc(x1)[..., :40].contiguous(), cwd[:, :40].contiguous(), scd)
