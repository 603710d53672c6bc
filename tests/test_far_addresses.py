"""Views far from their allocation's base: image strides and bases past 2^31 (and 2^32) bytes, and the conv family's
2 GiB input-allocation limit.  Placements and the reasoning behind them: tests/far_reference.py.

Protocol.  ONE device buffer of 8 GiB + 64 MiB (module fixture), filled with the sentinel byte 0x5A.  A test writes its
operands (inputs surrounded by NaN, destinations by sentinel, as `Placed` of tests/test_conv_exact.py does), launches once,
compares the destination images WITH their margins bit for bit against a host mirror, resets the images it placed and then
checks ON THE DEVICE that all the rest of the buffer still holds the sentinel.  A kernel that truncates an offset to 32 bits
therefore shows as a wrong value or as "bytes outside the destination changed"; it cannot leave the buffer
(tests/test_far_reference.py proves that for every placement).

Expected values are those of the plain references of each operation's own module (tests/*_reference.py), on a small case
of its exact regime; where the existing test of an operation carries a bound, that bound is imported from it.

An entry point may refuse a far operand on the host, with a message that names the limit; the destination must then be
untouched.  Refusals and runs are collected in TABLE and printed when the module ends."""
import collections
import ctypes as C
import time

import numpy as np
import pytest
import torch

from tests import conv_reference as R
from tests import far_reference as F
from tests import helper_reference as HR
from tests.test_conv_exact import NAN, SENTINEL, Placed, _bits, _desc, _image, _pack, _scratch, _stream, _FT, _IT, _TT
from tests.test_helper_fuzz import POISON
from tests.test_hip_fuzz import GEMM_HINTS, HINTS

pytestmark = pytest.mark.gpu

MODES = ["f16", "f32"]
ES = {"f16": 2, "f32": 4}
S64 = int.from_bytes(bytes([F.SENTINEL_BYTE]) * 8, "little")
CHUNK = 1 << 25                                         # int64 elements per device-side comparison: 256 MiB
TABLE = collections.OrderedDict()                       # (entry point, dtype) -> ["placement/role: ran | refused: ..."]
T0 = [None]


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32"), "f16": Engine("f16")}


@pytest.fixture(scope="module")
def bigbuf():
    T0[0] = time.time()
    buf = torch.empty(F.BUF_BYTES, dtype=torch.uint8, device="cuda:0")
    buf.fill_(F.SENTINEL_BYTE)
    torch.cuda.synchronize()
    yield buf
    torch.cuda.synchronize()
    del buf
    torch.cuda.empty_cache()
    print("\nfar-address runs (placement/role), %.1f s for the module" % (time.time() - T0[0]))
    for (name, mode), rows in TABLE.items():
        print("  %-28s %s  %s" % (name, mode, "; ".join(rows)))


def _code(dt):
    from glsdet_amd._lib import F16, F32
    return F16 if dt == "f16" else F32


# ================================================================================================== the far sibling of Placed
class FarPlaced:
    """`Placed` inside the big buffer: the same interface (view, full, put, upload, mismatch, grid, host, index), but the
    mirror covers just the view's own images with their margins; Arena.finish() answers for the rest of the buffer."""

    def __init__(self, arena, v, dt, fill):
        from glsdet_amd.engine import TView
        self.arena, self.v, self.dt = arena, v, dt
        code = _code(dt)
        self.view = TView(arena.alloc, v.off, v.n, v.h, v.w, v.c, v.sn, v.sh, v.sw, code)
        self.full = TView(arena.alloc, (v.block0 - F.ALLOC_LO) // v.es, v.n, v.H, v.W, v.Ct, v.sn, v.sh, v.sw, code)
        self.shape, self.index = (v.n, v.H, v.W, v.Ct), v.index
        self.host = np.full(self.shape, fill, _IT[dt])

    def grid(self, a):
        return a

    def put(self, nchw, index=None):
        self.host[index or self.index] = _bits(nchw, self.dt)
        return self

    def _dev(self, b):
        lo, hi = F.live_ranges(self.v)[b]
        return self.arena.buf[lo:hi]

    def upload(self):
        for b in range(self.v.n):
            self._dev(b).copy_(torch.from_numpy(self.host[b].reshape(-1).view(np.uint8)))
        return self

    def download(self):
        torch.cuda.synchronize()
        return np.stack([self._dev(b).cpu().numpy().view(_IT[self.dt]).reshape(self.shape[1:]) for b in range(self.v.n)])

    def mismatch(self, want_bits, index=None):
        got, want = self.download(), self.host.copy()
        if want_bits is not None:
            want[index or self.index] = want_bits
        bad = got != want
        if not bad.any():
            return None
        inside = np.zeros(want.shape, bool)
        inside[index or self.index] = True
        where = tuple(int(i[0]) for i in np.nonzero(bad))
        as_f = lambda a: a[where].reshape(1).view(_FT[self.dt])[0]
        return "%d of %d destination elements differ, %d elements OUTSIDE the destination changed; first at %s: got %r, want %r" % (
            int((bad & inside).sum()), int(inside.sum()), int((bad & ~inside).sum()), where, as_f(got), as_f(want))

    def reset(self):
        for b in range(self.v.n):
            self._dev(b).fill_(F.SENTINEL_BYTE)


class Arena:
    """the operands one launch placed in the big buffer"""

    def __init__(self, buf):
        self.buf, self.alloc, self.placed, self.extra = buf, buf[F.ALLOC_LO:], [], []

    def far(self, p, n, h, w, c, dt, fill, kind="window"):
        fp = FarPlaced(self, F.place(p, len(self.placed), n, h, w, c, ES[dt], kind), dt, fill)
        self.placed.append(fp)
        return fp

    def finish(self):
        """reset what was placed, then: does every byte of the buffer hold the sentinel?  -> None or a message"""
        torch.cuda.synchronize()
        for fp in self.placed:
            fp.reset()
        for lo, hi in self.extra:
            self.buf[lo:hi].fill_(F.SENTINEL_BYTE)
        self.placed, self.extra = [], []
        words = self.buf.view(torch.int64)
        flags = torch.stack([(words[i: i + CHUNK] != S64).any() for i in range(0, words.numel(), CHUNK)])
        if not bool(flags.any()):
            return None
        first = int(torch.nonzero(flags)[0]) * CHUNK
        chunk = words[first: first + CHUNK]
        at = first + int(torch.nonzero(chunk != S64)[0])
        n_bad = sum(int((words[i: i + CHUNK] != S64).sum()) for i in range(0, words.numel(), CHUNK))
        got = self.buf[at * 8: at * 8 + 16].cpu().numpy().tobytes().hex()
        self.buf.fill_(F.SENTINEL_BYTE)
        return "bytes outside the destination changed: %d 8-byte words of the buffer, the first at byte %#x (4 GiB + %#x): %s" % (
            n_bad, at * 8, at * 8 - F.ALLOC_LO, got)


class Ctx:
    """what an operation's case sees: where its sources and destinations go for this placement and role"""

    def __init__(self, eng, mode, p, role, arena):
        self.eng, self.mode, self.p, self.role, self.arena, self.failures, self.near = eng, mode, p, role, arena, [], []

    def _make(self, far, n, h, w, c, dt, fill, kind):
        if far:
            return self.arena.far(self.p, n, h, w, c, dt, fill, "window" if kind == "ring" else kind)
        self.near.append(Placed(self.eng, kind, n, h, w, c, dt, fill))
        return self.near[-1]

    def src(self, x, fill=None, kind="ring", dt=None):
        dt = dt or self.mode
        n, c, h, w = x.shape
        return self._make(self.role in ("inputs", "both"), n, h, w, c, dt, NAN[dt] if fill is None else fill, kind).put(x).upload()

    def dst(self, shape, kind="window", dt=None, init=None):
        dt = dt or self.mode
        n, c, h, w = shape
        d = self._make(self.role in ("output", "both"), n, h, w, c, dt, SENTINEL[dt], kind)
        if init is not None:
            d.put(init)
        return d.upload()

    def check(self, what, placed, want_bits, index=None):
        bad = placed.mismatch(want_bits, index)
        if bad:
            self.failures.append("%s: %s" % (what, bad))


# The refusals that may occur, pinned: entry point -> (placement/role pairs, the words its message must contain).  These
# four decide "y overlaps x" on the SPANS of the views (first to last element); two views whose images are 2^31 bytes
# apart interleave image by image, so with both operands at mid or far they count as overlapping (include/glsdet_hip.h).
# Everything else must run.
INTERLEAVED = ("mid/both", "far/both")
MAY_REFUSE = {"glsdet_conv2d_grouped": (INTERLEAVED, "y overlaps x"), "glsdet_layernorm": (INTERLEAVED, "y overlaps x"),
              "glsdet_patch_merge": (INTERLEAVED, "y overlaps x"), "glsdet_window_attention": (INTERLEAVED, "y overlaps qkv")}


def _sweep(engines, bigbuf, mode, name, case, roles=F.ROLES):
    """case(cx) at mid, far and base, with the inputs, the output or both far"""
    from glsdet_amd._lib import GlsdetError
    eng, failures, rows = engines[mode], [], TABLE.setdefault((name, mode), [])
    for p in F.PLACEMENTS:
        for role in roles:
            cx = Ctx(eng, mode, p, role, Arena(bigbuf))
            tag = "%s/%s" % (p.name, role)
            with _scratch(eng):
                try:
                    case(cx)
                    rows.append(tag + ": ran")
                except GlsdetError as e:
                    msg = str(e)
                    tags, words = MAY_REFUSE.get(name, ((), ""))
                    if tag not in tags:
                        failures.append("%s: refused, but this run must be taken: %s" % (tag, msg))
                    elif words not in msg:
                        failures.append("%s: refused without naming its rule (%r): %s" % (tag, words, msg))
                    rows.append(tag + ": refused: " + msg.split(": ", 1)[-1])
                    for fp in cx.arena.placed + cx.near:               # a refusal leaves every operand as it was
                        bad = fp.mismatch(None)
                        if bad:
                            failures.append("%s: after the refusal: %s" % (tag, bad))
                failures += ["%s %s" % (tag, f) for f in cx.failures]
                bad = cx.arena.finish()
                if bad:
                    failures.append("%s: %s" % (tag, bad))
    assert not failures, "\n".join(failures)


def test_the_whole_buffer_check_sees_one_changed_byte(bigbuf):
    """the harness itself: one byte, 6 GiB in, outside every placed view"""
    arena = Arena(bigbuf)
    assert arena.finish() is None
    at = 6 * F.GiB + 12345
    bigbuf[at] = 0
    bad = arena.finish()
    assert bad and "%#x" % (at // 8 * 8) in bad, bad
    assert arena.finish() is None


# ===================================================================================================== raw-pointer operations
# ---------------------------------------------------------------------------------------------------------------- pools
def _maxpool(cx):
    x = HR.pool_data((2, 24, 20, 24), cx.mode, 5, 20, 24, 24)
    src, dst = cx.src(x, POISON[cx.mode]), cx.dst(x.shape)
    cx.eng.maxpool(src.view, 5, out=dst.view)
    cx.check("maxpool", dst, _bits(HR.maxpool_ref(x, 5), cx.mode))


def _pool2d(cx):
    x = HR.pool_data((2, 8, 19, 23), cx.mode, 3, 2, 1, 19, 23)
    want = HR.pool2d_ref(x, 3, 2, 1)
    src, dst = cx.src(x, POISON[cx.mode]), cx.dst(want.shape)
    cx.eng.pool2d(src.view, 3, 2, 1, out=dst.view)
    cx.check("pool2d", dst, _bits(want, cx.mode))


def _spp_pools(cx):
    """x and the three outputs are channel slices of ONE buffer (as the model lays them out): one role, both far"""
    c, h, w, mode = 8, 14, 17, cx.mode
    x = HR.pool_data((2, c, h, w), mode, 5, h, w, c)
    buf = cx._make(True, 2, h + 2, w + 2, 4 * c, mode, POISON[mode], "dense")
    inner = (slice(None), slice(1, h + 1), slice(1, w + 1))
    buf.put(x, inner + (slice(0, c),))
    buf.grid(buf.host)[inner + (slice(c, 4 * c),)] = SENTINEL[mode]
    buf.upload()
    v = buf.full.window(1, h + 1, 1, w + 1)
    cx.eng.spp_pools(v.channels(0, c), v.channels(c, 2 * c), v.channels(2 * c, 3 * c), v.channels(3 * c, 4 * c))
    cx.check("spp_pools", buf, _bits(np.concatenate(HR.spp_ref(x), 1), mode), inner + (slice(c, 4 * c),))


# -------------------------------------------------------------------------------------------------------------- packing
def _focus_pack(cx):
    img = HR.image_data((2, 3, 34, 38), 3, 16, 34, 38)
    dst = cx.dst((2, 16, 17, 19))
    cx.eng.focus_pack(_image(cx.eng, img), out=dst.view)
    cx.check("focus_pack", dst, _bits(HR.focus_ref(img, 16, cx.mode), cx.mode))


def _nchw_pack(cx):
    img = HR.image_data((2, 3, 17, 23), 3, 17, 23)
    dst = cx.dst((2, 16, 17, 23))
    cx.eng.nchw_pack(_image(cx.eng, img), out=dst.view)
    cx.check("nchw_pack", dst, _bits(HR.nchw_pack_ref(img, 16, cx.mode), cx.mode))


# ----------------------------------------------------------------------------------------------------------- resampling
def _resample_copy(cx):
    x = HR.plain_data((2, 24, 9, 11), cx.mode, 2, 9, 11)
    want = HR.resample_ref(x, 2)
    src, dst = cx.src(x), cx.dst(want.shape)
    cx.eng.resample(src.view, 2, out=dst.view)
    cx.check("resample_copy", dst, _bits(want, cx.mode))


def _upsample_add(cx):
    (hp, wp), mode = HR.UPSAMPLE_CASES[0], cx.mode
    coarse = HR.updown_data((2, 16, hp[0], wp[0]), mode, 1, hp[0], wp[0])
    fine = HR.updown_data((2, 16, hp[1], wp[1]), mode, 2, hp[1], wp[1])
    cv, fv = cx.src(coarse), cx.dst(fine.shape, init=fine)
    cx.eng.upsample_add(cv.view, fv.view)
    cx.check("upsample_add", fv, _bits(HR.upsample_add_ref(fine, coarse, mode), mode))


def _copy_many(cx):
    """three jobs, each with a base of its own; the last one has two images"""
    srcs, dsts, wants = [], [], []
    for i, (n, h, w) in enumerate([(1, 5, 7), (1, 9, 11), (2, 3, 5)]):
        x = HR.plain_data((n, 24, h, w), cx.mode, 40, i, n, h, w)
        srcs.append(cx.src(x))
        dsts.append(cx.dst(x.shape))
        wants.append(_bits(HR.copy_ref(x), cx.mode))
    cx.eng.copy_many([s.view for s in srcs], [d.view for d in dsts])
    for i, (d, want) in enumerate(zip(dsts, wants)):
        cx.check("copy_many pair %d" % i, d, want)


def _transpose_many(cx):
    """sources far (each job a base of its own); the matrices are allocations of the engine"""
    vn, mode, eng = HR.VN[cx.mode], cx.mode, cx.eng
    srcs, mats, wants = [], [], []
    for i, (h, w) in enumerate([(7, 9), (5, 13)]):
        x = HR.plain_data((1, 72, h, w), mode, 50, i, 72, h, w)
        srcs.append(cx.src(x))
        m = eng.matrix(72 + 8, HR.ceil_to(h * w, vn) + 8)
        m.buf.view(_TT[mode])[:] = SENTINEL[mode]
        rows, pitch = m.buf.numel() // ES[mode] // m.sw, m.sw
        before = np.full(rows * pitch, SENTINEL[mode], _IT[mode]).view(_FT[mode]).astype(np.float64)
        want = HR.transpose_dest_ref(x, rows, pitch, vn, before)
        mats.append(m)
        wants.append(np.ascontiguousarray(want.astype(_FT[mode])).view(_IT[mode]).reshape(-1))
    eng.transpose_many([s.view for s in srcs], mats)
    torch.cuda.synchronize()
    for i, (m, want) in enumerate(zip(mats, wants)):
        if not np.array_equal(m.buf.view(_TT[mode]).cpu().numpy()[: want.size], want):
            cx.failures.append("transpose_many pair %d differs" % i)
    for s_ in srcs:
        cx.check("transpose_many source", s_, None)


# ----------------------------------------------------------------------------------- convolutions outside the descriptor family
def _dw(case, direct):
    def run(cx):
        eng, mode = cx.eng, cx.mode
        d = R.dw_case_data(case)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        xin = cx.src(d["x"])
        dst = cx.dst((case.n, case.c) + d["acc"].shape[2:])
        pk = eng.pack_dw(t(d["w"]), t(d["scale"]), t(d["bias"]), case.c)
        if direct:
            from glsdet_amd._lib import check
            check(eng.lib.glsdet_dwconv2d(C.byref(_desc(xin.view, dst.view, pk, case.stride, d["pad"], case.act)), _stream(eng)), "dwconv2d")
        else:
            eng.dwconv(xin.view, pk, case.stride, d["pad"], case.act, out=dst.view, dilation=case.dilation)
        cx.check("dwconv", dst, _bits(R.round_to(d["v"], mode), mode))
    return run


def _conv_grouped(cx):
    from tests import resnext_reference as X
    from tests.test_conv_grouped_exact import _pack as gpack
    case = X._g(3, 8, 2, 1, 9, 11, "relu", "window")
    d = X.case_data(case)
    xin = cx.src(d["x"])
    dst = cx.dst((2, 24) + d["acc"].shape[2:])
    pk = gpack(cx.eng, d["w"], d["scale"], d["bias"], case.groups)
    assert pk.kernel_takes
    cx.eng.conv_grouped(xin.view, pk, case.stride, case.act, out=dst.view, expand=False)
    cx.check("conv2d_grouped", dst, _bits(R.round_to(d["v"], cx.mode), cx.mode))


# ---------------------------------------------------------------------------------------------------------------- adapt
def _f(a):
    return np.asarray(a, np.float32)


def _gate(cx):
    from tests import attention_reference as AR
    from tests.test_attention_fuzz import _elementwise_inputs
    a, b, _ = _elementwise_inputs(cx.mode, 2, 24, 9, 11, 24)
    av, bv, yv = cx.src(a), cx.src(b), cx.dst(a.shape)
    cx.eng.gate(av.view, bv.view, None, out=yv.view)
    cx.check("gate", yv, _bits(_f(AR.gate_reference(a, b, None, cx.mode)), cx.mode))


def _scale_by_map(cx):
    from tests import attention_reference as AR
    from tests.test_attention_fuzz import _elementwise_inputs
    a, _, m = _elementwise_inputs(cx.mode, 2, 24, 9, 11, 25)
    m8 = np.concatenate([m, np.full((2, 7, 9, 11), 1e4, np.float32)], 1)
    av, mv, yv = cx.src(a), cx.src(m8), cx.dst(a.shape)
    cx.eng.scale_by_map(av.view, mv.view, out=yv.view)
    cx.check("scale_by_map", yv, _bits(_f(AR.scale_by_map_reference(a, m, cx.mode)), cx.mode))


def _rowsplit(cx):
    from tests import attention_reference as AR
    from tests.test_attention_fuzz import FULL, HOST_SPLITS, _rowsplit_inputs, _split_tensor
    a, b, y0 = _rowsplit_inputs(cx.mode, 2, 24, FULL[0], FULL[1], 224)
    av, bv = cx.src(a), cx.src(b)
    for op, q in ((2, 0), (4, 3)):
        yv = cx.dst(a.shape, init=y0)
        cx.eng.rowsplit(av.view, bv.view if op == 2 else None, _split_tensor(cx.eng, HOST_SPLITS[1]), op, out=yv.view, quadrant=q, shift=0)
        cx.check("rowsplit mode %d" % op, yv, _bits(_f(AR.rowsplit_reference(a, b, y0, HOST_SPLITS[1], op, q, 0)), cx.mode))


def _attn_split(cx):
    """the map is channel 0 of a far view; the result is four integers in a tensor of the engine"""
    from tests import attention_reference as AR
    from tests.test_attention_fuzz import POISON_CASES
    name, k, g = [c for c in POISON_CASES if c[0].startswith("2x12x20-")][0]
    m = np.full((k.shape[0], 8) + k.shape[1:], 3e4, np.float32)
    m[:, 0] = AR.to_float(k, g)
    att = cx.src(m)
    split = cx.eng.attn_split(att.view)
    torch.cuda.synchronize()
    if tuple(split.cpu().tolist()) != AR.split_reference(k) + (0,):
        cx.failures.append("attn_split: device %s, reference %s" % (split.cpu().tolist(), AR.split_reference(k)))


# ------------------------------------------------------------------------------------------------------------ non-local
def _nonlocal(case):
    """tests/test_nonlocal_exact.py's Launch with its operands placed by the context: x, theta|phi|g are sources, out the
    destination (an in-place case is far in every role)"""
    def run(cx):
        from tests import nonlocal_reference as NR
        from tests import test_nonlocal_exact as T

        def placed(eng, kind, n, h, w, c, dt, fill):
            far = cx.role == "both" or (cx.role == "inputs") == (fill == NAN[dt]) or case.okind is None
            return cx._make(far, n, h, w, c, dt, fill, "window")
        keep, T.NlPlaced = T.NlPlaced, placed
        try:
            run_ = T.Launch(cx.eng, cx.mode, case, NR.case_data(case))
        finally:
            T.NlPlaced = keep
        rc = run_.call()
        if rc != 0:
            from glsdet_amd._lib import GlsdetError
            raise GlsdetError(cx.eng.lib.glsdet_last_error().decode())
        cx.failures += run_.failures(run_.want(NR.expected(case)))
    return run


def _nl_cases():
    from tests import nonlocal_reference as NR
    two = lambda c: c._replace(n=2, name=c.name + "-n2")
    return two(NR.STATIC_CASES[1]), two(NR.MULTI_CASES[3]), two(NR.SPLIT_CASES[0])


_NL_STATIC, _NL_MULTI, _NL_SPLIT = _nl_cases()


def _nonlocal_mfma(cx):
    """tests/test_nonlocal_mfma.py's MfmaLaunch, its operands placed by the context"""
    from glsdet_amd._lib import GlsdetError
    from tests import nonlocal_mfma_cases as M
    from tests import nonlocal_reference as NR
    from tests import test_nonlocal_mfma as T
    case = M.EXACT_CASES[8]._replace(n=2, name=M.EXACT_CASES[8].name + "-n2")

    def placed(eng, kind, n, h, w, c, dt, fill):
        return cx._make(cx.role == "both" or (cx.role == "inputs") == (fill == NAN[dt]), n, h, w, c, dt, fill, "window")
    keep, T.MfmaPlaced = T.MfmaPlaced, placed
    try:
        run = T.MfmaLaunch(cx.eng, cx.mode, case, M.data(case))
    finally:
        T.MfmaPlaced = keep
    if run.call() != 0:
        raise GlsdetError(cx.eng.lib.glsdet_last_error().decode())
    cx.failures += run.failures(run.want(NR.expected(case)))


def _vals(p, index=None):
    """a placed view's device content -> (float64 NCHW, raw bits NHWC)"""
    if isinstance(p, FarPlaced):
        bits = np.ascontiguousarray(p.download()[index or p.index])
    else:
        torch.cuda.synchronize()
        bits = np.ascontiguousarray(p.grid(p.full.buf.view(_TT[p.dt]).cpu().numpy())[index or p.index])
    return bits.view(_FT[p.dt]).astype(np.float64).transpose(0, 3, 1, 2), bits


def _channel_maxmean(cx):
    """max exact, mean within the tolerance of tests/test_attention_fuzz.py test_channel_maxmean_wrapping_negative_and_wide"""
    from tests.test_attention_fuzz import MAXMEAN_MEAN_TOL, _rounded
    x = _rounded(-np.abs(np.random.RandomState(64).standard_normal((2, 64, 9, 11))) - 0.5, cx.mode)
    src, dst = cx.src(x), cx.dst((2, 8, 9, 11))
    cx.eng.channel_maxmean(src.view, out=dst.view)
    got, bits = _vals(dst)
    cx.check("channel_maxmean surroundings", dst, bits)
    if not np.array_equal(got[:, 0], x.max(1)) or np.abs(got[:, 1] - x.astype(np.float64).mean(1)).max() > MAXMEAN_MEAN_TOL[cx.mode] \
            or np.abs(got[:, 2:]).max() != 0.0:
        cx.failures.append("channel_maxmean: wrong values")


# ---------------------------------------------------------------------------------------------------- GroupNorm and proxy
def _groupnorm(cx):
    """exact regime out of place (bit for bit), then generic data in place within the bound B of helper_reference"""
    from tests.test_helper_fuzz import _dev, _gn_call
    eng, mode, case = cx.eng, cx.mode, HR.GN_BASE_CASES[1]
    assert case.n == 2
    d = HR.gn_exact_data(case, mode, "none", 0)
    xin, dst = cx.src(d["x"]), cx.dst(d["x"].shape)
    _gn_call(eng, xin.view, dst.view, case.groups, _dev(eng, d["gamma"]), _dev(eng, d["beta"]), 0.0, "none")
    cx.check("groupnorm exact", dst, _bits(d["y"], mode))
    cx.check("groupnorm exact, the source", xin, None)
    g = HR.gn_generic_data(case, mode, 0)
    want, B = HR.groupnorm_ref(g["x"], case.groups, g["gamma"], g["beta"], 1e-5, "relu")
    tol = B + (HR.half_ulp_f16(want, B) if mode == "f16" else 0.0)
    xin = cx._make(True, 2, case.h, case.w, case.C, mode, NAN[mode], "window").put(g["x"]).upload()
    eng.groupnorm(xin.view, case.groups, _dev(eng, g["gamma"]), _dev(eng, g["beta"]), 1e-5, "relu")
    got, bits = _vals(xin)
    cx.check("groupnorm generic surroundings", xin, bits)
    ratio = float(np.max(np.abs(got - want) / np.maximum(tol, 1e-300)))
    if not ratio <= 1.0:
        cx.failures.append("groupnorm generic: max err / bound %.3f" % ratio)


def _groupnorm_multi(cx):
    """in place: source and destination are one view (one role, both far)"""
    from tests.test_helper_fuzz import _dev
    eng, mode = cx.eng, cx.mode
    cases = [HR.GnCase("multi%d" % i, 2, HR.GN_MULTI_C, HR.GN_MULTI_GROUPS, h, w) for i, (h, w) in enumerate([(7, 11), (9, 9), (1, 2)])]
    data = [HR.gn_exact_data(c, mode, "relu", 0) for c in cases]
    xs = [cx._make(True, 2, c.h, c.w, c.C, mode, NAN[mode], "window").put(d["x"]).upload() for c, d in zip(cases, data)]
    eng.groupnorm_multi([x.view for x in xs], HR.GN_MULTI_GROUPS, [_dev(eng, d["gamma"]) for d in data],
                        [_dev(eng, d["beta"]) for d in data], 0.0, "relu")
    for c, d, x in zip(cases, data, xs):
        cx.check("groupnorm_multi %s" % c.name, x, _bits(d["y"], mode))


def _groupnorm_multi_pre(cx):
    """tests/test_helper_fuzz.py's mixed call: set 0 (far) carries the partial sums of its conv, set 1 (far) does not"""
    import os
    from tests.test_helper_fuzz import _dev
    eng, mode = cx.eng, cx.mode
    C_, G = HR.GN_MULTI_C, HR.GN_MULTI_GROUPS
    old = os.environ.get("GLSDET_GN_FUSION")
    os.environ["GLSDET_GN_FUSION"] = "1"
    try:
        gen = np.random.default_rng(7)
        x = HR.round_to(gen.normal(size=(2, C_, 9, 17)), mode)
        w = gen.normal(size=(C_, C_, 3, 3)) / np.sqrt(9 * C_)
        pk = eng.pack_conv([(torch.from_numpy(w).float(), torch.ones(C_), torch.zeros(C_))], C_)
        xin = Placed(eng, "dense", 2, 9, 17, C_, mode, NAN[mode]).put(x).upload()
        y0 = cx._make(True, 2, 9, 17, C_, mode, SENTINEL[mode], "window").upload()
        _, st = eng.conv_gnstats(xin.view, pk, 1, G, out=y0.view)
        assert st is not None, "the statistics form must apply to a 3x3 stride-1 conv"
        raw, _ = _vals(y0)
        c1 = HR.GnCase("multi0", 2, C_, G, 7, 11)
        d1 = HR.gn_exact_data(c1, mode, "relu", 0)
        x1 = cx._make(True, 2, 7, 11, C_, mode, NAN[mode], "window").put(d1["x"]).upload()
        g0 = HR.gn_generic_data(HR.GnCase("pre", 2, C_, G, 9, 17), mode, 3)
        eng.groupnorm_multi([y0.view, x1.view], G, [_dev(eng, g0["gamma"]), _dev(eng, d1["gamma"])],
                            [_dev(eng, g0["beta"]), _dev(eng, d1["beta"])], 0.0, "relu", pre=[st, None])
        cx.check("groupnorm_multi_pre, the set without statistics", x1, _bits(d1["y"], mode))
        want, B = HR.groupnorm_ref(raw, G, g0["gamma"], g0["beta"], 0.0, "relu")
        tol = B + (HR.half_ulp_f16(want, B) if mode == "f16" else 0.0)
        got, bits = _vals(y0)
        cx.check("groupnorm_multi_pre surroundings", y0, bits)
        ratio = float(np.max(np.abs(got - want) / np.maximum(tol, 1e-300)))
        if not ratio <= 1.0:
            cx.failures.append("groupnorm_multi_pre: max err / bound %.3f" % ratio)
    finally:
        if old is None:
            del os.environ["GLSDET_GN_FUSION"]
        else:
            os.environ["GLSDET_GN_FUSION"] = old


def _proxy_scores(cx):
    case = [c for c in HR.PROXY_CASES if c.n == 2][0]
    counts, mode = HR.PROXY_COUNTS[case.counts], cx.mode
    d = HR.proxy_data(case.n, case.C, case.h, case.w, counts, mode, 0)
    want = HR.proxy_ref(d["feat"], d["dots"], counts, case.gamma)
    P, nc = d["dots"].shape[1], len(counts)
    ch = lambda k: (slice(None), slice(None), slice(None), slice(0, k))
    far_in, far_out = cx.role in ("inputs", "both"), cx.role in ("output", "both")
    fv = cx.src(d["feat"])
    dv = cx._make(far_in, 2, case.h, case.w, HR.ceil_to(P, 8) + 8, "f32", NAN["f32"], "dense").put(d["dots"], ch(P)).upload()
    ov = cx._make(far_out, 2, case.h, case.w, HR.ceil_to(nc, 8) + 8, "f32", SENTINEL["f32"], "dense").upload()
    cx.eng.proxy_scores(fv.view, dv.view, counts, case.gamma, out=ov.view)
    got, bits = _vals(ov, ch(nc))
    cx.check("proxy_scores surroundings", ov, bits, ch(nc))
    ratio = float(np.max(np.abs(got - want) / (HR.PROXY_TOL * np.maximum(1.0, np.abs(want)))))
    if not (np.isfinite(got).all() and ratio <= 1.0):
        cx.failures.append("proxy_scores: max err / tolerance %.3f" % ratio)


# ---------------------------------------------------------------------------------------------------------------- stems
def _focus_stems(cx):
    eng, mode, case = cx.eng, cx.mode, R.FOCUS_CASES[0]
    d = R.focus_data(case)(mode)
    img = _image(eng, d["img"])
    dst = cx.dst((case.n, case.cout, case.h // 2, case.w // 2), "slice")
    eng.focus_conv(img, _pack(eng, d["w"], d["scale"], d["bias"], 16), case.act, out=dst.view)
    cx.check("focus_conv", dst, _bits(d["y"], mode))
    d = R.focus_data(case, 40)(mode)
    dst = cx.dst((case.n, 40) + d["y2"].shape[2:], "slice")
    eng.focus_conv_down(img, _pack(eng, d["w"], d["scale"], d["bias"], 16), "relu", _pack(eng, d["w2"], d["scale2"], d["bias2"], 32), case.act, out=dst.view)
    cx.check("focus_conv_down", dst, _bits(d["y2"], mode))


def _resnet_stems(cx):
    eng, mode, case = cx.eng, cx.mode, R.RESNET_STEM_CASES[0]
    d = R.resnet_stem_data(case)(mode)
    img = _image(eng, d["img"])
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    pk = eng.pack_resnet_stem(t(d["w"]), t(d["scale"]), t(d["bias"]))
    for what, want, run in (("resnet_stem", d["y"], lambda o: eng.resnet_stem(img, pk, "relu", out=o)),
                            ("resnet_stem_pool", d["pooled"], lambda o: eng.resnet_stem_pool(img, pk, out=o))):
        dst = cx.dst((case.n, 64, want.shape[2], want.shape[3]), "slice")
        run(dst.view)
        cx.check(what, dst, _bits(want, mode))


# ----------------------------------------------------------------------------------------------------------------- Swin
def _nchw(t):
    return t.permute(0, 3, 1, 2).numpy()


def _layernorm(cx):
    from glsdet_amd._lib import check
    from tests.test_swin_exact import _two_value
    x, g, b, want = _two_value((2, 4, 8, 96), 11)
    src, dst = cx.src(_nchw(x)), cx.dst((2, 96, 4, 8))
    gd, bd = g.float().cuda(), b.float().cuda()
    check(cx.eng.lib.glsdet_layernorm(C.byref(src.view.as_c()), C.byref(dst.view.as_c()), gd.data_ptr(), bd.data_ptr(), 1.75, _stream(cx.eng)), "layernorm")
    cx.check("layernorm", dst, _bits(_nchw(want), cx.mode))
    cx.check("layernorm, the source", src, None)


def _patch_merge(cx):
    from glsdet_amd._lib import check
    from tests import swin_reference as S
    x = torch.from_numpy(np.random.default_rng([31, 32, 5, 7]).integers(-512, 513, (2, 5, 7, 32)) / 64.0)
    want = S.patch_merge(x)
    src, dst = cx.src(_nchw(x)), cx.dst(tuple(_nchw(want).shape))
    check(cx.eng.lib.glsdet_patch_merge(C.byref(src.view.as_c()), C.byref(dst.view.as_c()), _stream(cx.eng)), "patch_merge")
    cx.check("patch_merge", dst, _bits(_nchw(want), cx.mode))


def _window_attention(cx):
    """the one-hot regime of tests/test_swin_exact.py: exact in both dtypes (shifted windows, a padded map)"""
    from glsdet_amd._lib import check
    from tests import swin_reference as S
    from tests.test_swin_exact import _SCALE
    H, W, heads, n, ws, shift = 15, 13, 3, 2, 7, 3
    qkv, table, bias = S.attention_operands(n, H, W, heads, ws, "onehot", 21)
    want = S.window_attention(qkv, table, bias, heads, ws, shift, scale=_SCALE)
    src, dst = cx.src(_nchw(qkv)), cx.dst((n, 32 * heads, H, W))
    td, bd = table.float().cuda().contiguous(), bias.float().cuda().contiguous()
    check(cx.eng.lib.glsdet_window_attention(C.byref(src.view.as_c()), C.byref(dst.view.as_c()), td.data_ptr(), bd.data_ptr(), heads, ws, shift,
                                             _SCALE, _stream(cx.eng)), "window_attention")
    wantb = _bits(_nchw(want), cx.mode)
    wantb = np.where(wantb == np.array(-0.0, _FT[cx.mode]).view(_IT[cx.mode]), 0, wantb)        # (+ 0.0, as the existing test compares)
    cx.check("window_attention", dst, wantb)
    cx.check("window_attention, the source", src, None)


# ------------------------------------------------------------------------------------------------------------------ EVC
def _lvc_encode(cx):
    """x far (a source); E and the workspace are plain device arrays"""
    from glsdet_amd._lib import check
    from tests import cfp_reference as X
    lib = cx.eng.lib
    x, cw, sc = X.encode_operands(96, 9, 15, 2, 40, "uniform")
    with torch.no_grad():
        want = X.encoding_expanded(x.double(), cw.double(), sc.double())
    src = cx.src(x.numpy())
    nbytes = lib.glsdet_lvc_encode_workspace_bytes(2, 9, 15, 96)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device="cuda")
    out = torch.zeros(2 * 64 * 96, dtype=torch.float32, device="cuda")
    cwd, scd = cw.cuda().contiguous(), sc.cuda().contiguous()
    check(lib.glsdet_lvc_encode(C.byref(src.view.as_c()), cwd.data_ptr(), scd.data_ptr(), ws.data_ptr(), nbytes, out.data_ptr(), _stream(cx.eng)), "lvc_encode")
    torch.cuda.synchronize()
    got = out.cpu().reshape(2, 64, 96)
    if not torch.equal((got + 0.0).view(torch.int32), (want.float() + 0.0).view(torch.int32)):
        cx.failures.append("lvc_encode: %d elements differ" % int((got != want.float()).sum()))
    cx.check("lvc_encode, the source", src, None)


def _channel_fuse(cx):
    from glsdet_amd._lib import check
    rng = np.random.default_rng([78, 5])
    f = lambda t: torch.from_numpy(np.ascontiguousarray(t, dtype=np.float32))
    a, t = f(rng.integers(-32, 33, (2, 96, 5, 7)) / 8.0), f(rng.integers(-32, 33, (2, 96, 5, 7)) / 8.0)
    v0, v1 = f(rng.integers(-8, 9, (2, 96)) / 4.0), f(rng.integers(-8, 9, 96) / 4.0)
    want = {0: torch.relu(a + a * v0[:, :, None, None]), 1: a + v1[None, :, None, None] * t}
    av, tv = cx.src(a.numpy()), cx.src(t.numpy())
    for mode in (0, 1):
        yv = cx.dst(tuple(a.shape))
        vec = (v0 if mode == 0 else v1).cuda()
        check(cx.eng.lib.glsdet_channel_fuse(C.byref(av.view.as_c()), C.byref(tv.view.as_c()) if mode == 1 else None, C.byref(yv.view.as_c()),
                                             vec.data_ptr(), mode, _stream(cx.eng)), "channel_fuse")
        cx.check("channel_fuse mode %d" % mode, yv, _bits(want[mode].numpy(), cx.mode))


# ------------------------------------------------------------------------------------------------------ post-processing
def _decode(ex):
    """three level views far; strides = None on a non-square input; the bound is decode_reference.BOUND"""
    def run(cx):
        from glsdet_amd._lib import View, check
        from tests import decode_reference as D
        eng, nc, n, (in_h, in_w) = cx.eng, 3, 2, (64, 96)
        g = torch.Generator().manual_seed(17)
        xs = [HR.round_to((torch.randn(n, 5 + nc, h, w, generator=g) * 2.0).numpy(), cx.mode).astype(np.float32) for h, w in ((8, 11), (4, 5), (2, 3))]
        levels = [cx.src(x) for x in xs]
        A = sum(x.shape[2] * x.shape[3] for x in xs)
        out = torch.full((n, A, 5 + nc), float("nan"), dtype=torch.float32, device=eng.device)
        arr = (View * 3)(*[l.view.as_c() for l in levels])
        if ex:
            check(eng.lib.glsdet_yolox_decode_ex(arr, 3, nc, in_h, in_w, None, 1, 2, out.data_ptr(), out.numel(), None, _stream(eng)), "yolox_decode_ex")
        else:
            check(eng.lib.glsdet_yolox_decode(arr, 3, nc, in_h, in_w, None, 0, out.data_ptr(), out.numel(), None, _stream(eng)), "yolox_decode")
        torch.cuda.synchronize()
        want = D.decode_f64([torch.from_numpy(x) for x in xs], nc, in_h, in_w, None, 1 if ex else 0, None, 2 if ex else 3)
        err = D.rel_err(out.cpu(), want)
        if not err <= D.BOUND:
            cx.failures.append("yolox_decode: max |err| / (|x| + 1) = %.3e" % err)
        for l in levels:
            cx.check("yolox_decode, a level", l, None)
    return run


RAW_OPS = collections.OrderedDict([
    ("glsdet_maxpool2d", _maxpool),
    ("glsdet_pool2d", _pool2d),
    ("glsdet_spp_pools", _spp_pools),
    ("glsdet_focus_pack", _focus_pack),
    ("glsdet_nchw_pack", _nchw_pack),
    ("glsdet_resample_copy", _resample_copy),
    ("glsdet_upsample_add", _upsample_add),
    ("glsdet_copy_many", _copy_many),
    ("glsdet_transpose_many", _transpose_many),
    ("glsdet_dwconv2d", _dw(R.DW_CASES[0], True)),
    ("glsdet_dwconv2d_dilated", _dw(R.DW_CASES[2], False)),
    ("glsdet_conv2d_grouped", _conv_grouped),
    ("glsdet_gate", _gate),
    ("glsdet_scale_by_map", _scale_by_map),
    ("glsdet_rowsplit", _rowsplit),
    ("glsdet_attn_split", _attn_split),
    ("glsdet_nonlocal", _nonlocal(_NL_STATIC)),
    ("glsdet_nonlocal_multi", _nonlocal(_NL_MULTI)),
    ("glsdet_nonlocal_split", _nonlocal(_NL_SPLIT)),
    ("glsdet_nonlocal_mfma", _nonlocal_mfma),
    ("glsdet_channel_maxmean", _channel_maxmean),
    ("glsdet_groupnorm", _groupnorm),
    ("glsdet_groupnorm_multi", _groupnorm_multi),
    ("glsdet_groupnorm_multi_pre", _groupnorm_multi_pre),
    ("glsdet_proxy_scores", _proxy_scores),
    ("glsdet_focus_conv", _focus_stems),                # + glsdet_focus_conv_down
    ("glsdet_resnet_stem", _resnet_stems),              # + glsdet_resnet_stem_pool
    ("glsdet_layernorm", _layernorm),
    ("glsdet_patch_merge", _patch_merge),
    ("glsdet_window_attention", _window_attention),
    ("glsdet_lvc_encode", _lvc_encode),
    ("glsdet_channel_fuse", _channel_fuse),
    ("glsdet_yolox_decode", _decode(False)),
    ("glsdet_yolox_decode_ex", _decode(True)),
])
INPUTS_ONLY = {"glsdet_attn_split", "glsdet_lvc_encode", "glsdet_transpose_many", "glsdet_yolox_decode", "glsdet_yolox_decode_ex"}      # nothing but sources is a view
OUTPUT_ONLY = {"glsdet_focus_pack", "glsdet_nchw_pack", "glsdet_focus_conv", "glsdet_resnet_stem"}                                      # the image is a plain array
BOTH_ONLY = {"glsdet_spp_pools", "glsdet_groupnorm_multi", "glsdet_groupnorm_multi_pre"}          # in place / one shared buffer: source and destination are one view


F32_ONLY = {"glsdet_yolox_decode", "glsdet_yolox_decode_ex"}                                                                            # "levels must be fp32"
RAW_RUNS = [(name, mode) for name in RAW_OPS for mode in MODES if mode == "f32" or name not in F32_ONLY]


@pytest.mark.parametrize("name,mode", RAW_RUNS, ids=["%s-%s" % (n[len("glsdet_"):], m) for n, m in RAW_RUNS])
def test_raw_pointer_operation_far(engines, bigbuf, mode, name):
    roles = ("inputs",) if name in INPUTS_ONLY else ("output",) if name in OUTPUT_ONLY else ("both",) if name in BOTH_ONLY else F.ROLES
    _sweep(engines, bigbuf, mode, name, RAW_OPS[name], roles)


# ------------------------------------------------------------------------------------------------------------------- GFL
def _far_fp32_view(arena, p):
    """tests/test_resdet.py's _fp32_view (fp32 NHWC, channels padded to 8 with zeros), placed far"""
    def view(eng, x_nchw):
        n, c, h, w = x_nchw.shape
        x = np.zeros((n, (c + 7) // 8 * 8, h, w), np.float32)
        x[:, :c] = x_nchw.numpy()
        return arena.far(p, n, h, w, x.shape[1], "f32", NAN["f32"]).put(x).upload().view
    return view


@pytest.mark.parametrize("p", F.PLACEMENTS, ids=lambda p: p.name)
@pytest.mark.parametrize("entry", ["gfl_detect", "gfl_candidates"])
def test_gfl_cls_and_reg_views_far(engines, bigbuf, monkeypatch, entry, p):
    """the existing comparisons with the naive references (tests/test_post_fuzz.py, tests/test_tta_fuzz.py), unchanged:
    rows, counts, labels and order; only the ten level views are placed far instead of near"""
    import tests.test_post_fuzz as PF
    import tests.test_resdet as TR
    import tests.test_tta_fuzz as TT
    arena = Arena(bigbuf)
    monkeypatch.setattr(TR, "_fp32_view", _far_fp32_view(arena, p))
    case = PF.GFL_CASES[0]
    if entry == "gfl_detect":
        PF.test_gfl_detect_vs_oracle_generic_integral_saturation_and_cuts(engines, case)
    else:
        TT.test_gfl_candidates_vs_oracle_pre_nms(engines["f32"], case)
    assert len(arena.placed) == 10
    for fp in arena.placed:
        assert fp.mismatch(None) is None, "a level view was written"
    TABLE.setdefault(("glsdet_" + entry, "f32"), []).append(p.name + "/inputs: ran")
    bad = arena.finish()
    assert not bad, bad


# ================================================================================================================ conv family
class EdgePlaced:
    """a conv input inside buf[:alloc] (tests/far_reference.py edge_view): image 0 starts at byte 0, the last image ends
    with the last 16 bytes of EDGE; dense=True: a dense view that ends there (the x_lin path of the 1x1 kernels).  Every
    element between the view's own is NaN."""

    def __init__(self, arena, x, dt, alloc=F.EDGE, dense=False):
        from glsdet_amd.engine import TView
        n, c, h, w = x.shape
        es = ES[dt]
        if dense:
            sw, sh, sn = c, w * c, h * w * c
            off, span = F.EDGE // es - n * sn, sn
        else:
            v = F.edge_view(n, h, w, c, es)
            off, sn, sh, sw, span = v.off, v.sn, v.sh, v.sw, v.span_bytes // es
        assert (off * es) % F.VEC == 0 and (off + (n - 1) * sn + span) * es == F.EDGE <= alloc
        self.arena, self.dt, self.n = arena, dt, n
        self.view = TView(arena.buf[:alloc], off, n, h, w, c, sn, sh, sw, _code(dt))
        self.ranges = [((off + b * sn) * es, (off + b * sn + span) * es) for b in range(n)]
        self.host = np.full((n, span), NAN[dt], _IT[dt])
        bits = _bits(x, dt)
        for b in range(n):
            np.lib.stride_tricks.as_strided(self.host[b], (h, w, c), (sh * es, sw * es, es))[...] = bits[b]
        for b, (lo, hi) in enumerate(self.ranges):
            arena.buf[lo:hi].copy_(torch.from_numpy(self.host[b].view(np.uint8)))
        arena.extra += self.ranges

    def mismatch(self, want_bits=None):
        torch.cuda.synchronize()
        for b, (lo, hi) in enumerate(self.ranges):
            if not np.array_equal(self.arena.buf[lo:hi].cpu().numpy().view(_IT[self.dt]), self.host[b]):
                return "image %d of the input was written" % b
        return None


def _k(name):
    """kernel family of a recorded op name"""
    fam = name.split("<")[0].split("[")[0]
    return fam + (" +1x1" if "+1x1" in name else "") + (" +gn stats" if "+gn stats" in name else "")


def _recorded_name(eng, launch):
    """the name of the op `launch` records (nothing runs); raises GlsdetError where the entry point refuses"""
    plan = eng.new_plan()
    with plan:
        launch()
    assert plan.num_ops == 1
    return plan.ops()[0]["name"]


_CONV_DATA = {}


def _conv_data(case, pad):
    key = (case.name, pad)
    if key not in _CONV_DATA:
        c = case
        x = R.ternary((c.n, c.cin, c.h, c.w), 11, *c[1:8])
        w = R.ternary((c.cout, c.cin, c.k, c.k), 12, *c[1:8])
        scale, bias = R.scale_bias(c.cout, *c[1:8])
        acc = R.conv(x, w, c.stride, pad)
        res = R.residual(acc.shape, 13, *c[1:8]) if c.res else None
        _CONV_DATA[key] = {"x": x, "w": w, "scale": scale, "bias": bias, "res": res, "acc": acc,
                           "v": R.check_regime(acc, scale, bias, res, c.act, c.res == 2)}
    return _CONV_DATA[key]


# n = 2, 19 x 23: more than one tile of every pixel-tile shape, ragged in both directions.  cin 64 = whole K steps (the
# per-tap UT path of conv_igemm_kernel), cin 24 = ragged K steps (its non-UT path); cout 72 / 24: the 64- and 128-row tiles
# and the 32-row tiles of conv_gemm.hip; res 2 = GLSDET_ACT_RES_FIRST
EDGE_CASES = [R._c(2, 64, 64, 3, 1, 19, 23, "relu", 1, "dense"), R._c(2, 64, 72, 3, 2, 19, 23, "relu", 0, "dense"),
              R._c(2, 24, 40, 3, 1, 19, 23, "none", 0, "dense"), R._c(2, 64, 72, 1, 1, 19, 23, "relu", 2, "dense"),
              R._c(2, 64, 24, 1, 1, 19, 23, "none", 1, "dense"), R._c(2, 64, 72, 1, 1, 19, 23, "none", 0, "dense")]
FAR_OUT_CASES = [EDGE_CASES[0], EDGE_CASES[3], EDGE_CASES[4]]


def _conv_on(eng, mode, case, pad, x, y, res, hints, reached, failures, tag, must_refuse=()):
    """the conv on every hint that takes it; y: a (Far)Placed, re-uploaded per hint -> hints that ran"""
    from glsdet_amd._lib import GlsdetError
    d = _conv_data(case, pad)
    want = _bits(R.round_to(d["v"], mode), mode)
    pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
    ran = []
    for hint in hints:
        launch = lambda: eng.conv(x.view, pk, case.stride, pad, case.act, out=y.view, res=res.view if res else None,
                                  tile_hint=hint, res_first=case.res == 2)
        try:
            name = _recorded_name(eng, launch)
        except GlsdetError as e:
            assert hint not in (0, 1), "%s: hints 0 and 1 must accept every problem: %s" % (tag, e)
            if hint in must_refuse and F.SPAN_TEXT not in str(e):
                failures.append("%s hint %#x: refused, but not with %r: %s" % (tag, hint, F.SPAN_TEXT, e))
            continue
        if hint in must_refuse:
            failures.append("%s hint %#x: %s takes a y / res span of 2^31 - 1 bytes or more" % (tag, hint, name))
            continue
        y.upload()
        launch()
        bad = y.mismatch(want)
        ran.append(hint)
        reached.add(_k(name))
        if case.k == 1 and name.startswith("conv_igemm"):
            reached.add("x_lin" if x.view.sn == x.view.h * x.view.sh and x.view.sh == x.view.w * x.view.sw else "x strided 1x1")
        if name.startswith("conv_igemm<"):
            kb = int(name.split(",kb")[1].split(">")[0])
            reached.add("conv_igemm UT" if (case.cin * ES[mode]) % kb == 0 else "conv_igemm non-UT")
        if bad:
            failures.append("%s hint %#x (%s): %s" % (tag, hint, name, bad))
    return ran


def _near_res(eng, case, d, mode):
    if not case.res:
        return None
    n, c, h, w = d["res"].shape
    return Placed(eng, "ring", n, h, w, c, mode, NAN[mode]).put(d["res"]).upload()


@pytest.mark.parametrize("mode", MODES)
def test_conv_family_input_at_the_edge_of_the_descriptor_range(engines, bigbuf, mode):
    """x inside buf[: 2^31 - 256]: image 0 AT byte 0 (the negative tap offsets of pad 1 wrap below x_off = 0), image 1 ends
    with the allocation's last 16 bytes; y dense at `base`.  Every hint that accepts, pad k // 2 and pad 0, bit for bit; and
    the kernels this reached, by op name."""
    from glsdet_amd._lib import ACT, ConvChain, GlsdetError
    eng, failures, reached, hints_ran = engines[mode], [], set(), set()
    multi_reached = set()                                    # kernels of glsdet_conv2d_multi, by the family of the recorded name
    arena = Arena(bigbuf)

    def done(tag):
        bad = arena.finish()
        if bad:
            failures.append("%s: %s" % (tag, bad))

    for case in EDGE_CASES:
        for pad in sorted({case.k // 2, 0}):
            for dense in ((False, True) if case.k == 1 else (False,)):
                tag = "%s pad %d%s" % (case.name, pad, " dense" if dense else "")
                with _scratch(eng):
                    d = _conv_data(case, pad)
                    x = EdgePlaced(arena, d["x"], mode, dense=dense)
                    n, c, h, w = d["v"].shape
                    y = arena.far(F.BASE, n, h, w, c, mode, SENTINEL[mode], "dense")
                    ran = _conv_on(eng, mode, case, pad, x, y, _near_res(eng, case, d, mode), HINTS, reached, failures, tag)
                    assert {0, 1} <= set(ran), (tag, ran)
                    hints_ran |= set(ran)
                    if x.mismatch():
                        failures.append("%s: %s" % (tag, x.mismatch()))
                    done(tag)

    # ---- conv2d_multi: the four quadrant windows of ONE edge-placed map; the grouped ring kernels (8, 10) must take them
    mc = R.MultiCase("far_multi", 2, 64, 72, 3, 1, 13, 19, 6, 9, "relu", 1, False)
    d = R.multi_data(mc)
    with _scratch(eng):
        x = EdgePlaced(arena, d["x"], mode)
        n, c, Ho, Wo = d["v"].shape
        y = arena.far(F.BASE, n, Ho, Wo, c, mode, SENTINEL[mode], "dense")
        rin = Placed(eng, "ring", n, Ho, Wo, c, mode, NAN[mode]).put(d["res"]).upload()
        pks = [_pack(eng, q["w"], q["scale"], q["bias"], mc.cin) for q in d["quads"]]
        xs = [x.view.window(*q["win"]) for q in d["quads"]]
        outs, ress = [y.view.window(*q["owin"]) for q in d["quads"]], [rin.view.window(*q["owin"]) for q in d["quads"]]
        want = _bits(R.round_to(d["v"], mode), mode)
        for hint in (0, 8, 10, (64 << 16) | 64):
            launch = lambda: eng.conv_multi(xs, pks, 1, 1, "relu", outs=outs, ress=ress, tile_hint=hint)
            try:
                name = _recorded_name(eng, launch)
            except GlsdetError as e:
                # 64 input channels are whole 128-byte chunks in both dtypes: the grouped ring kernels take the class
                assert hint not in (0, 8, 10), "conv2d_multi hint %d must take this shape class: %s" % (hint, e)
                continue
            y.upload()
            launch()
            fam = _k(name)                                   # conv_halo_ring[_k64]_multi, or the generic conv_igemm_<form>
            ring = fam.startswith("conv_halo_ring") and fam.endswith("_multi")
            assert ring or hint not in (8, 10), "hint %d names the grouped ring kernel, %s ran" % (hint, name)
            assert not ring or hint in (0, 8, 10), "an explicit tile names the generic kernel, %s ran" % name
            multi_reached.add(fam)
            bad = y.mismatch(want)
            if bad:
                failures.append("conv2d_multi hint %#x (%s): %s" % (hint, name, bad))
        done("conv2d_multi")

    # ---- conv2d_chain, conv2d_gnstats, bottleneck: direct calls, as tests/test_conv_exact.py makes them
    cc = R.ChainCase("far_chain", 2, 64, 64, 1, 19, 23, "relu", 1, 0, 32, 40, "relu", False)
    d = R.chain_data(cc)(mode)
    with _scratch(eng):
        x = EdgePlaced(arena, d["x"], mode)
        y = arena.far(F.BASE, 2, 19, 23, 64, mode, SENTINEL[mode], "dense")
        y2 = arena.far(F.BASE, 2, 19, 23, 40, mode, SENTINEL[mode], "dense")
        rin = Placed(eng, "ring", 2, 19, 23, 64, mode, NAN[mode]).put(d["res"]).upload()
        pk, pk2 = _pack(eng, d["w"], d["scale"], d["bias"], 64), _pack(eng, d["w2"], d["scale2"], d["bias2"], 32)
        c = ConvChain()
        c.y2 = y2.view.as_c()
        c.w2, c.scale2, c.bias2 = pk2[0].data_ptr(), pk2[1].data_ptr(), pk2[2].data_ptr()
        c.act2, c.c0, c.cin2, c.flags = ACT["relu"], 0, 32, 0
        ran = []
        for hint in HINTS:
            dd = _desc(x.view, y.view, pk, 1, 1, "relu", rin.view, False, hint)
            plan = eng.new_plan()
            with plan:
                rc = eng.lib.glsdet_conv2d_chain(C.byref(dd), C.byref(c), _stream(eng))
            if rc != 0:
                assert hint != 0, eng.lib.glsdet_last_error().decode()
                continue
            name = plan.ops()[0]["name"]
            y.upload(), y2.upload()
            assert eng.lib.glsdet_conv2d_chain(C.byref(dd), C.byref(c), _stream(eng)) == 0
            ran.append(hint)
            reached.add(_k(name))
            for what, buf, want in (("y", y, _bits(d["y"], mode)), ("y2", y2, _bits(d["y2"], mode))):
                bad = buf.mismatch(want)
                if bad:
                    failures.append("conv2d_chain hint %#x (%s) %s: %s" % (hint, name, what, bad))
        assert len(ran) >= 2, ran
        done("conv2d_chain")

    gc = R.GnCase("far_gn", 2, 64, 64, 8, 19, 23, "none")
    d = R.gn_data(gc)(mode)
    with _scratch(eng):
        x = EdgePlaced(arena, d["x"], mode)
        y = arena.far(F.BASE, 2, 19, 23, 64, mode, SENTINEL[mode], "dense")
        pk = _pack(eng, d["w"], d["scale"], d["bias"], 64)
        stats = torch.zeros(eng.lib.glsdet_conv2d_gnstats_bytes(2, 19, 23, 8) // 8, dtype=torch.float64, device=eng.device)
        ran = []
        for hint in (8, 9, 10, 11):
            y.upload()
            stats.zero_()
            dd = _desc(x.view, y.view, pk, 1, 1, "none", hint=hint)
            if eng.lib.glsdet_conv2d_gnstats(C.byref(dd), 8, stats.data_ptr(), _stream(eng)) != 0:
                continue
            ran.append(hint)
            reached.add("+gn stats")
            bad = y.mismatch(_bits(d["y"], mode))
            if bad:
                failures.append("conv2d_gnstats hint %d y: %s" % (hint, bad))
            p = stats.cpu().numpy().reshape(2, -1, 8, 2)
            for k, unit, want in ((0, 2048.0, d["s1"]), (1, 2048.0 ** 2, d["s2"])):
                if not np.array_equal(np.rint(p[..., k] * unit).astype(np.int64).sum(1), want):
                    failures.append("conv2d_gnstats hint %d: the partial sums (%d) do not reduce to the exact sums" % (hint, k))
        assert ran, eng.lib.glsdet_last_error().decode()
        done("conv2d_gnstats")

    bc = R.BneckCase("far_bneck", 2, 64, 32, 19, 23, 1)
    d = R.bneck_data(bc)(mode)
    with _scratch(eng):
        x = EdgePlaced(arena, d["x"], mode)
        y = arena.far(F.BASE, 2, 19, 23, 32, mode, SENTINEL[mode], "dense")
        rin = Placed(eng, "ring", 2, 19, 23, 32, mode, NAN[mode]).put(d["res"]).upload()
        hid = Placed(eng, "dense", 2, 19, 23, 32, mode, SENTINEL[mode]).upload()
        p1, p2 = _pack(eng, d["w1"], d["s1"], d["b1"], 64), _pack(eng, d["w2"], d["s2"], d["b2"], 32)
        d1, d2 = _desc(x.view, hid.view, p1, 1, 0, "relu"), _desc(hid.view, y.view, p2, 1, 1, "relu", rin.view)
        ran = []
        for hint in (0, 1):
            y.upload()
            if eng.lib.glsdet_bottleneck(C.byref(d1), C.byref(d2), hint, _stream(eng)) != 0:
                continue
            ran.append(hint)
            reached.add("conv_bneck")
            for what, bad in (("y", y.mismatch(_bits(d["y"], mode))), ("hidden", hid.mismatch(None))):
                if bad:
                    failures.append("bottleneck hint %d %s: %s" % (hint, what, bad))
        assert ran, "the fused Bottleneck must take this case: " + eng.lib.glsdet_last_error().decode()
        done("bottleneck")

    if mode == "f16":
        _csp_at_the_edge(eng, arena, reached, failures)
        done("csp_fused")

    print("%s: kernels reached with the input at the edge: %s" % (mode, ", ".join(sorted(reached | multi_reached))))
    assert not failures, "\n".join(failures)
    assert set(GEMM_HINTS) <= hints_ran, "persistent 1x1 variants not reached: %s" % sorted(set(GEMM_HINTS) - hints_ran)
    need = {"conv_igemm UT", "conv_igemm non-UT", "x_lin", "x strided 1x1", "conv_gemm", "conv_gemm1", "conv1x1_ws",
            "conv_bneck", "+gn stats"} | ({"csp_fused"} if mode == "f16" else set())
    assert need <= reached, "not reached: %s" % sorted(need - reached)
    assert any(k.endswith(" +1x1") for k in reached), "the chained form was not reached"
    assert any(k.startswith("conv_halo") and "s2" in k for k in reached) and any(k.startswith("conv_halo_ring") for k in reached), sorted(reached)
    ring_multi = {k for k in multi_reached if k.startswith("conv_halo_ring") and k.endswith("_multi")}
    assert ring_multi and multi_reached - ring_multi, "conv2d_multi: the grouped ring and the generic kernel must both run: %s" % sorted(multi_reached)


def _csp_at_the_edge(eng, arena, reached, failures):
    """csp_fused has no exact regime (SiLU): as tests/test_csp_fused.py, bit for bit against the four plain launches of the
    same layer (other kernels, near operands) and within its bound of the oracle"""
    from glsdet_amd.synth import synth_input
    from oracle import glsdet_oracle as O
    from tests.test_csp_fused import F16_TOL, _layer, _packs, _upload
    sd, x = _layer(), synth_input((2, 64, 19, 23), 11).half().float()
    with _scratch(eng):
        packs = _packs(eng, sd)
        ref = eng._tmp(2, 19, 23, 64)
        eng._csp_unfused(_upload(eng, x), packs, True, ref, lambda xi, pk, pad, o, res: eng.conv(xi, pk, 1, pad, "silu", out=o, res=res, tile_hint=1))
        torch.cuda.synchronize()
        want = ref.to_nchw().cpu()
        oracle = O.csp_layer(sd, "m", x, True)
        assert float((want - oracle).abs().max()) <= F16_TOL * max(1.0, float(oracle.abs().max()))
        xe = EdgePlaced(arena, x.numpy(), "f16")
        for hint in (0, 1):
            y = Placed(eng, "window", 2, 19, 23, 64, "f16", SENTINEL["f16"]).upload()
            d = eng._csp_desc(xe.view, y.view, packs, True)
            rc = eng.lib.glsdet_csp_fused(C.byref(d), hint, _stream(eng))
            assert rc == 0, eng.lib.glsdet_last_error().decode()
            reached.add("csp_fused")
            bad = y.mismatch(_bits(want.numpy(), "f16"))
            if bad:
                failures.append("csp_fused hint %d: %s" % (hint, bad))
        if xe.mismatch():
            failures.append("csp_fused: " + xe.mismatch())


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("alloc", [F.JUST_IN, F.JUST_OUT, F.OVER], ids=["just_in", "just_out", "over"])
def test_conv_family_input_allocation_limit(engines, bigbuf, mode, alloc):
    """the same view in an allocation of 2^31 - 2 bytes: accepted and exact; 2^31 - 1 and 2^31: GlsdetError with the
    library's "2 GiB descriptor range", the destination and the whole buffer keep their bits"""
    from glsdet_amd._lib import GlsdetError
    eng, failures, arena = engines[mode], [], Arena(bigbuf)
    for case in (EDGE_CASES[0], EDGE_CASES[3]):
        with _scratch(eng):
            d = _conv_data(case, case.k // 2)
            x = EdgePlaced(arena, d["x"], mode, alloc=alloc)
            n, c, h, w = d["v"].shape
            y = arena.far(F.BASE, n, h, w, c, mode, SENTINEL[mode], "dense").upload()
            res = _near_res(eng, case, d, mode)
            if alloc == F.JUST_IN:
                ran = _conv_on(eng, mode, case, case.k // 2, x, y, res, [0, 1], set(), failures, case.name)
                assert ran == [0, 1]
            else:
                pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
                for hint in (0, 1):
                    with pytest.raises(GlsdetError, match=F.LIMIT_TEXT):
                        eng.conv(x.view, pk, case.stride, case.k // 2, case.act, out=y.view, res=res.view, tile_hint=hint, res_first=case.res == 2)
                failures += [m for m in (y.mismatch(None), x.mismatch()) if m]
            bad = arena.finish()
            if bad:
                failures.append(bad)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("p", F.PLACEMENTS, ids=lambda p: p.name)
def test_conv2d_output_and_residual_far(engines, bigbuf, mode, p):
    """x small and near; y and res at the placement.  Hints 0 and 1 run and are exact (the epilogues of conv_common.h,
    conv.hip, conv_halo.hip and conv1x1.hip address y and res through 64-bit offsets).  At mid and far the SPAN of y and res
    is 2^31 - 1 bytes or more: every hint of GEMM_HINTS refuses with "does not apply" (32-bit y / res offsets).  At base the
    span is small (only the base is far), so those variants may run, and must then be exact.  Every other hint runs exactly
    or refuses with a message.  One case has GLSDET_ACT_RES_FIRST (res 2)."""
    eng, failures, arena = engines[mode], [], Arena(bigbuf)
    rows = TABLE.setdefault(("glsdet_conv2d", mode), [])
    for case in FAR_OUT_CASES:
        with _scratch(eng):
            d = _conv_data(case, case.k // 2)
            x = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
            n, c, h, w = d["v"].shape
            y = arena.far(p, n, h, w, c, mode, SENTINEL[mode])
            res = arena.far(p, n, h, w, c, mode, NAN[mode]).put(d["res"]).upload()
            span = ((n - 1) * y.v.sn + (h - 1) * y.v.sh + (w - 1) * y.v.sw + c) * ES[mode]
            must = GEMM_HINTS if span >= 2 ** 31 - 1 else ()
            assert (p.name == "base") == (not must)
            ran = _conv_on(eng, mode, case, case.k // 2, x, y, res, HINTS, set(), failures, "%s at %s" % (case.name, p.name), must)
            assert {0, 1} <= set(ran), ran
            rows.append("%s/output %s: ran %d hints%s" % (p.name, case.name, len(ran), ", persistent 1x1 variants refused: does not apply" if must else ""))
            if res.mismatch(None):
                failures.append("res was written: " + res.mismatch(None))
            bad = arena.finish()
            if bad:
                failures.append("%s at %s: %s" % (case.name, p.name, bad))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("p", F.PLACEMENTS, ids=lambda p: p.name)
def test_chain_bottleneck_gnstats_multi_outputs_far(engines, bigbuf, mode, p):
    """y, res and the chained y2 at the placement, x near: hints 0 and 1 (gnstats: its ring hints) exact"""
    from glsdet_amd._lib import ACT, ConvChain
    eng, failures, arena = engines[mode], [], Arena(bigbuf)

    def done(tag):
        bad = arena.finish()
        if bad:
            failures.append("%s: %s" % (tag, bad))

    near = lambda x: Placed(eng, "ring", x.shape[0], x.shape[2], x.shape[3], x.shape[1], mode, NAN[mode]).put(x).upload()
    far_in = lambda r: arena.far(p, r.shape[0], r.shape[2], r.shape[3], r.shape[1], mode, NAN[mode]).put(r).upload()
    far_out = lambda c: arena.far(p, 2, 19, 23, c, mode, SENTINEL[mode])
    note = lambda name: TABLE.setdefault((name, mode), []).append(p.name + "/output: ran")

    cc = R.ChainCase("far_chain", 2, 64, 64, 1, 19, 23, "relu", 1, 0, 32, 40, "relu", False)
    d = R.chain_data(cc)(mode)
    with _scratch(eng):
        x, y, y2, rin = near(d["x"]), far_out(64), far_out(40), far_in(d["res"])
        pk, pk2 = _pack(eng, d["w"], d["scale"], d["bias"], 64), _pack(eng, d["w2"], d["scale2"], d["bias2"], 32)
        c = ConvChain()
        c.y2 = y2.view.as_c()
        c.w2, c.scale2, c.bias2 = pk2[0].data_ptr(), pk2[1].data_ptr(), pk2[2].data_ptr()
        c.act2, c.c0, c.cin2, c.flags = ACT["relu"], 0, 32, 0
        for hint in (0, 1):
            y.upload(), y2.upload()
            dd = _desc(x.view, y.view, pk, 1, 1, "relu", rin.view, False, hint)
            assert eng.lib.glsdet_conv2d_chain(C.byref(dd), C.byref(c), _stream(eng)) == 0, eng.lib.glsdet_last_error().decode()
            for what, buf, want in (("y", y, _bits(d["y"], mode)), ("y2", y2, _bits(d["y2"], mode))):
                bad = buf.mismatch(want)
                if bad:
                    failures.append("conv2d_chain hint %d %s: %s" % (hint, what, bad))
        note("glsdet_conv2d_chain")
        done("conv2d_chain")

    bc = R.BneckCase("far_bneck", 2, 64, 32, 19, 23, 1)
    d = R.bneck_data(bc)(mode)
    with _scratch(eng):
        x, y, rin = near(d["x"]), far_out(32), far_in(d["res"])
        hid = Placed(eng, "dense", 2, 19, 23, 32, mode, SENTINEL[mode]).upload()
        p1, p2 = _pack(eng, d["w1"], d["s1"], d["b1"], 64), _pack(eng, d["w2"], d["s2"], d["b2"], 32)
        d1, d2 = _desc(x.view, hid.view, p1, 1, 0, "relu"), _desc(hid.view, y.view, p2, 1, 1, "relu", rin.view)
        ran = 0
        for hint in (0, 1):
            y.upload()
            if eng.lib.glsdet_bottleneck(C.byref(d1), C.byref(d2), hint, _stream(eng)) != 0:
                continue
            ran += 1
            bad = y.mismatch(_bits(d["y"], mode))
            if bad:
                failures.append("bottleneck hint %d: %s" % (hint, bad))
        assert ran, eng.lib.glsdet_last_error().decode()
        note("glsdet_bottleneck")
        done("bottleneck")

    gc = R.GnCase("far_gn", 2, 64, 64, 8, 19, 23, "none")
    d = R.gn_data(gc)(mode)
    with _scratch(eng):
        x, y = near(d["x"]), far_out(64)
        pk = _pack(eng, d["w"], d["scale"], d["bias"], 64)
        stats = torch.zeros(eng.lib.glsdet_conv2d_gnstats_bytes(2, 19, 23, 8) // 8, dtype=torch.float64, device=eng.device)
        ran = 0
        for hint in (8, 9, 10, 11):
            y.upload()
            dd = _desc(x.view, y.view, pk, 1, 1, "none", hint=hint)
            if eng.lib.glsdet_conv2d_gnstats(C.byref(dd), 8, stats.data_ptr(), _stream(eng)) != 0:
                continue
            ran += 1
            bad = y.mismatch(_bits(d["y"], mode))
            if bad:
                failures.append("conv2d_gnstats hint %d: %s" % (hint, bad))
        assert ran, eng.lib.glsdet_last_error().decode()
        note("glsdet_conv2d_gnstats")
        done("conv2d_gnstats")

    mc = R.MultiCase("far_multi", 2, 64, 72, 3, 1, 13, 19, 6, 9, "relu", 1, False)
    d = R.multi_data(mc)
    with _scratch(eng):
        x = near(d["x"])
        n, c, Ho, Wo = d["v"].shape
        y, rin = arena.far(p, n, Ho, Wo, c, mode, SENTINEL[mode]), far_in(d["res"])
        pks = [_pack(eng, q["w"], q["scale"], q["bias"], mc.cin) for q in d["quads"]]
        xs = [x.view.window(*q["win"]) for q in d["quads"]]
        outs, ress = [y.view.window(*q["owin"]) for q in d["quads"]], [rin.view.window(*q["owin"]) for q in d["quads"]]
        for hint in (0, (64 << 16) | 64):
            y.upload()
            eng.conv_multi(xs, pks, 1, 1, "relu", outs=outs, ress=ress, tile_hint=hint)
            bad = y.mismatch(_bits(R.round_to(d["v"], mode), mode))
            if bad:
                failures.append("conv2d_multi hint %#x: %s" % (hint, bad))
        note("glsdet_conv2d_multi")
        done("conv2d_multi")
    assert not failures, "\n".join(failures)


def test_csp_fused_refuses_a_far_output(engines, bigbuf):
    """its y is addressed through a 32-bit descriptor too: a y whose ALLOCATION is 2^31 - 1 bytes or more is refused with the
    library's "2 GiB descriptor range", and nothing is written"""
    from tests.test_csp_fused import _layer, _packs
    eng, arena = engines["f16"], Arena(bigbuf)
    rows = TABLE.setdefault(("glsdet_csp_fused", "f16"), [])
    with _scratch(eng):
        packs = _packs(eng, _layer())
        x = Placed(eng, "ring", 2, 19, 23, 64, "f16", NAN["f16"]).upload()
        for p in F.PLACEMENTS:
            y = arena.far(p, 2, 19, 23, 64, "f16", SENTINEL["f16"]).upload()
            d = eng._csp_desc(x.view, y.view, packs, True)
            assert eng.lib.glsdet_csp_fused(C.byref(d), 0, _stream(eng)) < 0
            msg = eng.lib.glsdet_last_error().decode()
            assert F.LIMIT_TEXT in msg, msg
            assert y.mismatch(None) is None
            rows.append("%s/output: refused: %s" % (p.name, msg))
            assert arena.finish() is None
