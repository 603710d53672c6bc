"""Bit-exact tests of the conv family (glsdet_amd/csrc/conv*.hip, stem.hip, dwconv.hip) against tests/conv_reference.py.

The data regime of that module (ternary operands, 12-bit scales, dyadic biases and residuals) makes every fp32 step of
the kernels exact in any summation order, so each output must equal the float64 value rounded ONCE to the output type,
bit for bit, on every kernel variant.  There is no tolerance in this file.  Four contracts are checked per variant:

  1. destination views: dense, a channel slice, and a spatial window + channel slice (strided in n, h and w: the
     per-chunk division path of the epilogues);
  2. nothing outside the destination is written: the destination buffer is pre-filled with a sentinel bit pattern
     and the WHOLE allocation is compared as raw integers after every launch;
  3. nothing outside the input view influences the result: inputs and residuals sit in buffers whose every other
     element is NaN (channels on both sides, a one-pixel ring) -- 0 x NaN would show;
  4. one rounding: with a residual the fp16 epilogue rounds act(conv * scale + bias) + res once; scale and bias stay
     fp32; the pack rounds to nearest even; the order of add and activation and the bias index are pinned by the data
     (tests/test_conv_reference.py proves that each such mistake changes bits on every case that has the feature).

Hints: every tile_hint of tests/test_hip_fuzz.py.  No hint of that list is documented in include/glsdet_hip.h as
inapplicable to a dtype, so test_every_variant_is_reached demands a case for each in both engines."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from tests import conv_reference as R
from tests.test_hip_fuzz import GEMM_HINTS, GEO_HINTS, HINTS

pytestmark = pytest.mark.gpu

MODES = ["f16", "f32"]
_FT = {"f16": np.float16, "f32": np.float32}
_IT = {"f16": np.int16, "f32": np.int32}
_TT = {"f16": torch.int16, "f32": torch.int32}
SENTINEL = {"f16": 0x5A5A, "f32": 0x5A5A5A5A}           # a finite pattern no result of the regime has in every element
NAN = {"f16": 0x7E00, "f32": 0x7FC00000}
RING_HINTS = [8, 9, 10, 11, 12, 13] + GEO_HINTS
TILE_HINTS = [h for h in HINTS if h >= 0x10000]
INAPPLICABLE = {"f16": set(), "f32": set()}             # hints the header documents as not existing for a dtype: none


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32"), "f16": Engine("f16")}


@contextlib.contextmanager
def _scratch(eng):
    """buffers a test allocates through the engine are released when it ends"""
    mark = len(eng._keep)
    try:
        yield
    finally:
        torch.cuda.synchronize()
        del eng._keep[mark:]


class Placed:
    """A view inside a buffer of its own, with a host mirror of the WHOLE allocation as raw integers."""

    def __init__(self, eng, kind, n, h, w, c, dt, fill):
        from glsdet_amd._lib import F16, F32
        self.dt, self.eng = dt, eng
        code = F16 if dt == "f16" else F32
        if kind == "dense":
            H, W, Ct, h0, w0, c0 = h, w, c, 0, 0, 0
        elif kind == "slice":                           # channel slice of a concat buffer
            H, W, Ct, h0, w0, c0 = h, w, c + 24, 0, 0, 16
        elif kind == "window":                          # spatial window + channel slice: strided in n, h and w
            H, W, Ct, h0, w0, c0 = h + 3, w + 2, c + 24, 2, 1, 16
        else:                                           # "ring": channels on both sides and a one-pixel ring
            assert kind == "ring"
            H, W, Ct, h0, w0, c0 = h + 2, w + 2, c + 16, 1, 1, 8
        self.full = eng.tensor(n, H, W, Ct, code)
        self.view = self.full
        if (H, W) != (h, w):
            self.view = self.view.window(h0, h0 + h, w0, w0 + w)
        if Ct != c:
            self.view = self.view.channels(c0, c0 + c)
        self.shape = (n, H, W, Ct)
        self.index = (slice(None), slice(h0, h0 + h), slice(w0, w0 + w), slice(c0, c0 + c))
        self.host = np.full(self.full.buf.numel() // np.dtype(_IT[dt]).itemsize, fill, _IT[dt])

    def grid(self, flat):
        n, H, W, Ct = self.shape
        return flat[: n * H * W * Ct].reshape(n, H, W, Ct)

    def put(self, nchw, index=None):
        """values (NCHW, any float type that holds them exactly) -> the view's place in the host mirror"""
        self.grid(self.host)[index or self.index] = _bits(nchw, self.dt)
        return self

    def upload(self):
        self.full.buf.view(_TT[self.dt])[:] = torch.from_numpy(self.host).to(self.eng.device)
        return self

    def mismatch(self, want_bits, index=None):
        """one synchronize + one download: the whole allocation against mirror + expected bits; -> None or a message"""
        torch.cuda.synchronize()
        got = self.full.buf.view(_TT[self.dt]).cpu().numpy()
        want = self.host.copy()
        if want_bits is not None:
            self.grid(want)[index or self.index] = want_bits
        bad = got != want
        if not bad.any():
            return None
        inside = np.zeros(want.shape, bool)
        self.grid(inside)[index or self.index] = True
        first = int(np.nonzero(bad)[0][0])
        where = tuple(int(i) for i in np.unravel_index(first, self.shape)) if first < int(np.prod(self.shape)) else ("tail", first)
        as_f = lambda a: a[first: first + 1].view(_FT[self.dt])[0]
        return "%d of %d destination elements differ, %d elements OUTSIDE the destination changed; first at %s: got %r, want %r" % (
            int((bad & inside).sum()), int(inside.sum()), int((bad & ~inside).sum()), where, as_f(got), as_f(want))


def _bits(nchw, dt):
    return np.ascontiguousarray(np.asarray(nchw).astype(_FT[dt]).transpose(0, 2, 3, 1)).view(_IT[dt])


def _pack(eng, w, scale, bias, cin):
    return eng.pack_conv([(torch.from_numpy(np.asarray(w, np.float32)), torch.from_numpy(np.asarray(scale, np.float32)),
                           torch.from_numpy(np.asarray(bias, np.float32)))], cin)


def _desc(x, y, pk, stride, pad, act, res=None, res_first=False, hint=0):
    from glsdet_amd._lib import ACT, ConvDesc, View
    d = ConvDesc()
    d.x, d.y, d.res = x.as_c(), y.as_c(), (res.as_c() if res is not None else View())
    d.w, d.scale, d.bias = pk[0].data_ptr(), pk[1].data_ptr(), pk[2].data_ptr()
    d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = pk[4], pk[5], stride, pad, ACT[act], hint
    if res_first and res is not None:
        d.act |= 0x100
    return d


def _stream(eng):
    from glsdet_amd.engine import _stream_ptr
    return _stream_ptr(eng.stream)


_DATA = {}


def _case_data(case):
    if case.name not in _DATA:
        _DATA[case.name] = R.case_data(case, 15 if case in R.PRED_CASES else None)
    return _DATA[case.name]


# ============================================================================================== (a) glsdet_conv2d
def _run_conv_case(eng, mode, case, hints, pred=False):
    """the case on every hint of `hints` that accepts it -> (hints that ran, failure messages)"""
    from glsdet_amd._lib import F32, GlsdetError
    d = _case_data(case)
    out_t = "f32" if pred else mode
    cout = 15 if pred else case.cout
    ho, wo = d["acc"].shape[2:]
    want = _bits(R.round_to(d["v"], out_t), out_t)
    xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
    rin = None
    if case.res:
        rin = Placed(eng, "ring" if case.rplace == "window" else "dense", case.n, ho, wo, case.cout, out_t, NAN[out_t]).put(d["res"]).upload()
    dst = Placed(eng, case.dst, case.n, ho, wo, case.cout, out_t, SENTINEL[out_t])
    pk = _pack(eng, d["w"][:cout], d["scale"][:cout], d["bias"][:cout], case.cin)
    ran, failures = [], []
    for hint in hints:
        dst.upload()
        try:
            eng.conv(xin.view, pk, case.stride, case.k // 2, case.act, out=dst.view, res=rin.view if rin else None,
                     out_dtype=F32 if pred else None, tile_hint=hint, res_first=case.res == 2)
        except GlsdetError:
            assert hint not in (0, 1), "the automatic choice and the generic kernel must accept every problem"
            continue
        bad = dst.mismatch(want)
        ran.append(hint)
        if bad:
            failures.append("hint %#x: %s" % (hint, bad))
    return ran, failures


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.CONV_CASES, ids=lambda c: c.name)
def test_conv2d_every_variant_bit_for_bit(engines, mode, case):
    eng = engines[mode]
    with _scratch(eng):
        ran, failures = _run_conv_case(eng, mode, case, HINTS)
    print("%s %s ran on %s" % (case.name, mode, " ".join("%#x" % h for h in ran)))
    assert not failures, "\n".join(failures)
    assert len(ran) >= 2


@pytest.mark.parametrize("mode", MODES)
def test_every_variant_is_reached(engines, mode):
    """no variant silently drops out of the suite: every hint accepts at least one case of CONV_CASES in this dtype
    (descriptors are recorded into a plan, nothing is launched: acceptance is decided on the host)"""
    from glsdet_amd._lib import GlsdetError
    eng = engines[mode]
    missing = []
    with _scratch(eng):
        ops = {}
        for hint in HINTS:
            if hint in INAPPLICABLE[mode]:
                continue
            for case in R.CONV_CASES:
                if case.name not in ops:
                    ho, wo = R.out_extent(case.h, case.k, case.stride, case.k // 2), R.out_extent(case.w, case.k, case.stride, case.k // 2)
                    z = np.zeros((case.cout, case.cin, case.k, case.k))
                    ops[case.name] = (eng.tensor(case.n, case.h, case.w, case.cin), eng.tensor(case.n, ho, wo, case.cout),
                                      eng.tensor(case.n, ho, wo, case.cout) if case.res else None,
                                      _pack(eng, z, np.ones(case.cout), np.zeros(case.cout), case.cin))
                x, y, r, pk = ops[case.name]
                plan = eng.new_plan()
                try:
                    with plan:
                        eng.conv(x, pk, case.stride, case.k // 2, case.act, out=y, res=r, tile_hint=hint, res_first=case.res == 2)
                except GlsdetError:
                    continue
                assert plan.num_ops == 1
                break
            else:
                missing.append("%#x" % hint)
    assert not missing, "no case of CONV_CASES reaches tile_hint %s on the %s engine" % (", ".join(missing), mode)


@pytest.mark.parametrize("case", [c for c in R.CONV_CASES if c.k > 1], ids=lambda c: c.name)
def test_ring_kernels_on_the_32x32x16_mfma_shape(engines, monkeypatch, case):
    """the fp16 ring kernels once more on the MFMA shape they were first written on (GLSDET_NO_M16=1, read per launch)"""
    monkeypatch.setenv("GLSDET_NO_M16", "1")
    eng = engines["f16"]
    with _scratch(eng):
        ran, failures = _run_conv_case(eng, "f16", case, [0, 1] + RING_HINTS)
    assert not failures, "\n".join(failures)
    assert len(ran) >= 2


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", [c for c in R.CONV_CASES if c.k == 1], ids=lambda c: c.name)
def test_persistent_1x1_kernel_with_three_workgroups_per_xcd(engines, monkeypatch, mode, case):
    """GLSDET_GEMM_SLOTS_PER_XCD=3: every workgroup walks many pixel tiles, so the operand ring, the residual DMAs and
    the epilogues run across tile boundaries"""
    monkeypatch.setenv("GLSDET_GEMM_SLOTS_PER_XCD", "3")
    eng = engines[mode]
    with _scratch(eng):
        ran, failures = _run_conv_case(eng, mode, case, [1] + GEMM_HINTS)
    assert not failures, "\n".join(failures)
    assert len(ran) >= 2


def test_predictor_form_fp32_logits_of_fp16_operands(engines):
    """out_dtype = F32 on the f16 engine, 15 output channels padded to 16: the logits are the float64 values exactly;
    every 1x1 variant that takes 32 padded cout rows runs at least one case"""
    eng = engines["f16"]
    seen, failures = set(), []
    for case in R.PRED_CASES:
        with _scratch(eng):
            ran, bad = _run_conv_case(eng, "f16", case, [0, 1] + GEMM_HINTS + TILE_HINTS, pred=True)
        assert len(ran) >= 2
        seen |= set(ran)
        failures += ["%s %s" % (case.name, b) for b in bad]
    assert not failures, "\n".join(failures)
    assert {21, 25, 31, (32 << 16) | 128} <= seen, sorted(seen)          # the 32-row tiles of conv_gemm.hip and conv.hip


# ======================================================================================== (b) glsdet_conv2d_multi
MULTI_TILES = [(64 << 16) | 64, (64 << 16) | 128, (128 << 16) | 128, (64 << 16) | 64 | 0x8000, (128 << 16) | 128 | 0x8000]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.MULTI_CASES, ids=lambda c: c.name)
def test_conv2d_multi_on_the_quadrant_windows_of_shared_buffers(engines, mode, case):
    """the neck's layout: inputs = quadrant windows of ONE map (the neighbour's real data lies directly outside each
    window, a 3x3 must see zeros there), outputs = quadrant windows of ONE buffer with a sentinel ring: afterwards the
    whole output allocation equals the assembled reference and the ring is intact.  Grouped form (4 problems; hints 0,
    8..11, co << 16 | px) and batched form (one problem per image and quadrant, 9..32; generic tiles only)."""
    from glsdet_amd._lib import GlsdetError
    eng = engines[mode]
    d = R.multi_data(case)
    Ho, Wo = d["v"].shape[2:]
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
        rin = Placed(eng, "ring", case.n, Ho, Wo, case.cout, mode, NAN[mode]).put(d["res"]).upload() if case.res else None
        dst = Placed(eng, "window", case.n, Ho, Wo, case.cout, mode, SENTINEL[mode])
        packs = [_pack(eng, q["w"], q["scale"], q["bias"], case.cin) for q in d["quads"]]
        xs, outs, ress, pks = [], [], [], []
        for b in (range(case.n) if case.per_image else [None]):
            img = (lambda v: v.image(b)) if case.per_image else (lambda v: v)
            for q, pk in zip(d["quads"], packs):
                xs.append(img(xin.view).window(*q["win"]))
                outs.append(img(dst.view).window(*q["owin"]))
                ress.append(img(rin.view).window(*q["owin"]) if rin else None)
                pks.append(pk)
        assert (9 <= len(xs) <= 32) if case.per_image else (2 <= len(xs) <= 8)
        want = _bits(R.round_to(d["v"], mode), mode)
        ran, failures = [], []
        for hint in [0, 8, 9, 10, 11] + MULTI_TILES:
            dst.upload()
            try:
                eng.conv_multi(xs, pks, case.stride, case.k // 2, case.act, outs=outs, ress=ress, tile_hint=hint)
            except GlsdetError:
                assert hint != 0, "the automatic choice must accept every group"
                assert not (case.per_image and hint >= 0x10000), "the batched form takes every generic tile"
                continue
            assert not (case.per_image and 8 <= hint <= 11), "more than eight problems run on the generic tiles only"
            bad = dst.mismatch(want)
            ran.append(hint)
            if bad:
                failures.append("hint %#x: %s" % (hint, bad))
        print("%s %s ran on %s" % (case.name, mode, " ".join("%#x" % h for h in ran)))
        assert not failures, "\n".join(failures)
        assert len(ran) >= 2
        if not case.per_image and case.k == 3 and (case.cin * (2 if mode == "f16" else 4)) % 128 == 0:
            assert 10 in ran and (case.stride == 2 or 8 in ran), ran        # the grouped ring kernel did take its problems


# ======================================================================================== (c) glsdet_conv2d_chain
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.CHAIN_CASES, ids=lambda c: c.name)
def test_conv2d_chain_both_results_bit_for_bit(engines, mode, case):
    """y and y2 into embedded destinations, both exact (y2 consumes the ROUNDED y, the reference does too); with
    GLSDET_CHAIN_SKIP_Y the whole buffer of y keeps its bits ("it is not stored"); every hint that accepts the pair."""
    from glsdet_amd._lib import ACT, ConvChain
    eng = engines[mode]
    d = R.chain_data(case)(mode)
    ho, wo = d["y"].shape[2:]
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
        rin = Placed(eng, "ring", case.n, ho, wo, case.cout, mode, NAN[mode]).put(d["res"]).upload() if case.res else None
        y = Placed(eng, "window", case.n, ho, wo, case.cout, mode, SENTINEL[mode])
        y2 = Placed(eng, "window", case.n, ho, wo, case.cout2, mode, SENTINEL[mode])
        pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
        pk2 = _pack(eng, d["w2"], d["scale2"], d["bias2"], case.cin2)
        c = ConvChain()
        c.y2 = y2.view.as_c()
        c.w2, c.scale2, c.bias2 = pk2[0].data_ptr(), pk2[1].data_ptr(), pk2[2].data_ptr()
        c.act2, c.c0, c.cin2, c.flags = ACT[case.act2], case.c0, case.cin2, 1 if case.skip_y else 0
        ran, failures = [], []
        for hint in HINTS:
            y.upload(), y2.upload()
            dd = _desc(xin.view, y.view, pk, case.stride, 1, case.act, rin.view if rin else None, False, hint)
            if eng.lib.glsdet_conv2d_chain(C.byref(dd), C.byref(c), _stream(eng)) != 0:
                assert hint != 0, "the automatic choice must take this chained pair: " + eng.lib.glsdet_last_error().decode()
                continue
            ran.append(hint)
            for what, buf, want in (("y", y, None if case.skip_y else _bits(d["y"], mode)), ("y2", y2, _bits(d["y2"], mode))):
                bad = buf.mismatch(want)
                if bad:
                    failures.append("hint %#x %s: %s" % (hint, what, bad))
        print("%s %s ran on %s" % (case.name, mode, " ".join("%#x" % h for h in ran)))
        assert not failures, "\n".join(failures)
        assert len(ran) >= 2, ran


# ========================================================================================== (d) glsdet_bottleneck
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.BNECK_CASES, ids=lambda c: c.name)
def test_bottleneck_bit_for_bit_and_the_hidden_buffer_is_untouched(engines, mode, case):
    eng = engines[mode]
    d = R.bneck_data(case)(mode)
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin0, mode, NAN[mode]).put(d["x"]).upload()
        rin = Placed(eng, "ring", case.n, case.h, case.w, case.cm, mode, NAN[mode]).put(d["res"]).upload() if case.res else None
        hid = Placed(eng, "dense", case.n, case.h, case.w, case.cm, mode, SENTINEL[mode]).upload()
        dst = Placed(eng, "window", case.n, case.h, case.w, case.cm, mode, SENTINEL[mode])
        p1, p2 = _pack(eng, d["w1"], d["s1"], d["b1"], case.cin0), _pack(eng, d["w2"], d["s2"], d["b2"], case.cm)
        d1 = _desc(xin.view, hid.view, p1, 1, 0, "relu")
        d2 = _desc(hid.view, dst.view, p2, 1, 1, "relu", rin.view if rin else None)
        want = _bits(d["y"], mode)
        ran, failures = [], []
        for hint in (0, 1):
            dst.upload()
            if eng.lib.glsdet_bottleneck(C.byref(d1), C.byref(d2), hint, _stream(eng)) != 0:
                continue
            ran.append(hint)
            for what, bad in (("y", dst.mismatch(want)), ("hidden (its base is not touched)", hid.mismatch(None))):
                if bad:
                    failures.append("hint %d %s: %s" % (hint, what, bad))
        assert not failures, "\n".join(failures)
        assert ran, "the fused Bottleneck must take %s: %s" % (case.name, eng.lib.glsdet_last_error().decode())


# ====================================================================================== (e) glsdet_conv2d_gnstats
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.GN_CASES, ids=lambda c: c.name)
def test_conv2d_gnstats_partials_reduce_to_the_exact_sums(engines, mode, case):
    """the fp64 partials (per image, 8 x 16 tile, wave, group) are sums of dyadic numbers: reduced per (image, group)
    they equal the reference's integer sums of the STORED values and of their squares exactly"""
    eng = engines[mode]
    d = R.gn_data(case)(mode)
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.cin, mode, NAN[mode]).put(d["x"]).upload()
        dst = Placed(eng, "window", case.n, case.h, case.w, case.cout, mode, SENTINEL[mode])
        pk = _pack(eng, d["w"], d["scale"], d["bias"], case.cin)
        nbytes = eng.lib.glsdet_conv2d_gnstats_bytes(case.n, case.h, case.w, case.groups)
        tiles = ((case.h + 7) // 8) * ((case.w + 15) // 16)
        assert nbytes == case.n * tiles * 4 * case.groups * 2 * 8
        stats = torch.zeros(nbytes // 8, dtype=torch.float64, device=eng.device)
        ran, failures = [], []
        for hint in (8, 9, 10, 11):
            dst.upload()
            stats.zero_()
            dd = _desc(xin.view, dst.view, pk, 1, 1, case.act, hint=hint)
            if eng.lib.glsdet_conv2d_gnstats(C.byref(dd), case.groups, stats.data_ptr(), _stream(eng)) != 0:
                continue
            ran.append(hint)
            bad = dst.mismatch(_bits(d["y"], mode))
            if bad:
                failures.append("hint %d y: %s" % (hint, bad))
            p = stats.cpu().numpy().reshape(case.n, tiles * 4, case.groups, 2)
            for k, unit, want in ((0, 2048.0, d["s1"]), (1, 2048.0 ** 2, d["s2"])):
                q = p[..., k] * unit
                if not np.array_equal(q, np.rint(q)) or np.abs(q).max() >= 2.0 ** 62:
                    failures.append("hint %d: a partial %s is not a sum of the stored values (not a multiple of 1 / %g)"
                                    % (hint, ("sum", "sum of squares")[k], unit))
                    continue
                got = q.astype(np.int64).sum(1)
                if not np.array_equal(got, want):
                    i = tuple(int(v[0]) for v in np.nonzero(got != want))
                    failures.append("hint %d: %s of (image, group) %s: got %d, want %d (units of 1 / %g)"
                                    % (hint, ("sum", "sum of squares")[k], i, got[i], want[i], unit))
        assert not failures, "\n".join(failures)
        assert ran, eng.lib.glsdet_last_error().decode()


# ================================================================================================= (f) the stems
def _image(eng, img):
    t = torch.from_numpy(np.asarray(img, np.float32)).contiguous().to(eng.device)
    eng._keep.append(t)
    return t


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.FOCUS_CASES, ids=lambda c: c.name)
def test_focus_conv_and_focus_conv_down_bit_for_bit(engines, mode, case):
    eng = engines[mode]
    with _scratch(eng):
        d = R.focus_data(case)(mode)
        img = _image(eng, d["img"])
        dst = Placed(eng, "slice", case.n, case.h // 2, case.w // 2, case.cout, mode, SENTINEL[mode]).upload()
        eng.focus_conv(img, _pack(eng, d["w"], d["scale"], d["bias"], 16), case.act, out=dst.view)
        bad = dst.mismatch(_bits(d["y"], mode))
        assert not bad, "focus_conv: " + bad
        for cout2 in (40, 64):
            d = R.focus_data(case, cout2)(mode)
            ho, wo = d["y2"].shape[2:]
            dst = Placed(eng, "slice", case.n, ho, wo, cout2, mode, SENTINEL[mode]).upload()
            eng.focus_conv_down(img, _pack(eng, d["w"], d["scale"], d["bias"], 16), "relu",
                                _pack(eng, d["w2"], d["scale2"], d["bias2"], 32), case.act, out=dst.view)
            bad = dst.mismatch(_bits(d["y2"], mode))
            assert not bad, "focus_conv_down, %d channels: %s" % (cout2, bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.RESNET_STEM_CASES, ids=lambda c: c.name)
def test_resnet_stem_and_stem_pool_bit_for_bit(engines, mode, case):
    eng = engines[mode]
    d = R.resnet_stem_data(case)(mode)
    with _scratch(eng):
        img = _image(eng, d["img"])
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        pk = eng.pack_resnet_stem(t(d["w"]), t(d["scale"]), t(d["bias"]))
        for what, want, run in (("resnet_stem", d["y"], lambda o: eng.resnet_stem(img, pk, "relu", out=o)),
                                ("resnet_stem_pool", d["pooled"], lambda o: eng.resnet_stem_pool(img, pk, out=o))):
            dst = Placed(eng, "slice", case.n, want.shape[2], want.shape[3], 64, mode, SENTINEL[mode]).upload()
            run(dst.view)
            bad = dst.mismatch(_bits(want, mode))
            assert not bad, "%s: %s" % (what, bad)


# ============================================================================================= (g) depthwise convs
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.DW_CASES, ids=lambda c: c.name)
def test_dwconv_nan_surroundings_and_exact_values(engines, mode, case):
    eng = engines[mode]
    d = R.dw_case_data(case)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    with _scratch(eng):
        xin = Placed(eng, "ring", case.n, case.h, case.w, case.c, mode, NAN[mode]).put(d["x"]).upload()
        ho, wo = d["acc"].shape[2:]
        dst = Placed(eng, "window", case.n, ho, wo, case.c, mode, SENTINEL[mode]).upload()
        pk = eng.pack_dw(t(d["w"]), t(d["scale"]), t(d["bias"]), case.c)
        eng.dwconv(xin.view, pk, case.stride, d["pad"], case.act, out=dst.view, dilation=case.dilation)
        bad = dst.mismatch(_bits(R.round_to(d["v"], mode), mode))
        assert not bad, bad
