"""Bit-exact tests of the non-local block kernels (nl_gram / nl_fold / nl_apply / nl_window, glsdet_amd/csrc/nonlocal.hip) behind
glsdet_nonlocal, glsdet_nonlocal_multi, glsdet_nonlocal_split and torch.ops.glsdet.nonlocal_dot, against
tests/nonlocal_reference.py.

The data regime of that module makes every float32 step of the three kernels exact in any summation order, so each output
must equal the float64 definition rounded ONCE to the output type, bit for bit; tests/test_nonlocal_reference.py proves on
the CPU that every case is inside the regime and that a dropped tile, slice or chunk, a wrong N, a transposed Gram or P,
another set's weights or an invN one ulp off changes bits.  There is no tolerance in the exact tests.  Per launch:

  1. the destination allocation is pre-filled with a sentinel (NaN when the block runs in place) and compared WHOLE as raw
     integers: nothing outside the windows changes;
  2. x and theta | phi | g sit in NaN-poisoned buffers (a ring, neighbouring channels, the rest of the map, the channels
     past 3 ci): 0 x NaN would show; the inputs are compared whole afterwards, too;
  3. the output equals the once-rounded float64 reference in every bit;
  4. the workspace has exactly the documented n_sets n (8 ci^2 + cx ci) floats, followed by a sentinel guard that must
     stay untouched.  Every launch is one direct ctypes call.

The case lists, the mirrors of the kernels' vec / vec_t / vec_o predicates and their cross-coverage are asserted when
tests/nonlocal_reference.py is imported; nothing is skipped or filtered at run time.

Continuous operands (test_*_generic_operands_within_the_a_priori_bound) are held to the per-element bound of
nonlocal_reference.generic_reference_and_bound, which is derived, not measured.  max |err| / B per case, as printed on an
MI355X (fp16: the half ulp of the one final rounding is nearly all of B, so a ratio close to 1 is what a correct kernel
gives; fp32: the worst-case summation bound is far from a typical error):

    case                                      f16     f32
    static  ci24-c30-5x13                     0.961   0.013
    static  ci136-c200-13x21                  0.641   0.001
    static  ci16-c8-25x41-odd                 0.877   0.002
    multi   quadrants-3x107-ci16-c40          0.986   0.028
    multi   three-windows-ci24-c30-odd        0.969   0.014
    split   split-ci8-c8-n3-4.5.7-shift0      0.993   0.050
    split   split-ci64-c36-n3-20.4.31-shift0  0.877   0.003
    split   split-ci136-c200-n1-12.18.22-shift1  0.743   0.002"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nonlocal_reference as R
from tests.test_attention_fuzz import _split_tensor
from tests.test_conv_exact import NAN, SENTINEL, Placed, _bits, _scratch, _stream, engines  # noqa: F401  (engines: the fixture)
from tests.test_conv_exact import _FT, _IT, _TT

pytestmark = pytest.mark.gpu

MODES = ["f16", "f32"]
GUARD = 4096                                             # floats behind the workspace
GUARD_BITS = 0x5A5A5A5A
_IDS = lambda c: c.name


class NlPlaced(Placed):
    """Placed on the layouts of nonlocal_reference.layout: any channel count (30 stays 30), and the 'odd' kind whose
    channel offset and pixel stride are no multiple of a 16-byte access"""

    def __init__(self, eng, kind, n, h, w, c, dt, fill):
        from glsdet_amd._lib import F16, F32
        from glsdet_amd.engine import TView
        self.dt, self.eng = dt, eng
        code = F16 if dt == "f16" else F32
        H, W, Ct, h0, w0, c0 = R.layout(kind, h, w, c, dt)
        buf = eng.raw(n * H * W * Ct * np.dtype(_IT[dt]).itemsize)
        self.full = TView(buf, 0, n, H, W, Ct, H * W * Ct, W * Ct, Ct, code)
        self.view = TView(buf, (h0 * W + w0) * Ct + c0, n, h, w, c, H * W * Ct, W * Ct, Ct, code)
        self.shape = (n, H, W, Ct)
        self.index = (slice(None), slice(h0, h0 + h), slice(w0, w0 + w), slice(c0, c0 + c))
        self.host = np.full(buf.numel() // np.dtype(_IT[dt]).itemsize, fill, _IT[dt])

    def read(self):
        """the view's elements (one synchronize + one download) -> (float64 NCHW, raw bits NHWC)"""
        torch.cuda.synchronize()
        got = self.full.buf.view(_TT[self.dt]).cpu().numpy()
        bits = np.ascontiguousarray(self.grid(got)[self.index])
        return bits.view(_FT[self.dt]).astype(np.float64).transpose(0, 3, 1, 2), bits


def _f32(eng, a):
    return eng.upload(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


class Launch:
    """the operands of one case on the device, and the direct ctypes call of its entry point"""

    def __init__(self, eng, mode, case, d):
        self.eng, self.mode, self.case = eng, mode, case
        n, ci, cx = case.n, case.ci, case.cx
        inplace = case.okind is None
        self.x = NlPlaced(eng, case.xkind, n, case.FH, case.FW, cx, mode, NAN[mode]).put(d["x"]).upload()
        self.out = self.x if inplace else NlPlaced(eng, case.okind, n, case.FH, case.FW, cx, mode, SENTINEL[mode]).upload()
        self.tpg = [NlPlaced(eng, case.tkind, n, case.FH, case.FW, case.tw, mode, NAN[mode]).put(t).upload() for t in d["tpg"]]
        self.wout = [_f32(eng, w) for w in d["wout"]]
        self.bout = [_f32(eng, b) for b in d["bout"]]
        self.sets = len(R.windows(case))
        self.floats = self.sets * n * (8 * ci * ci + cx * ci)          # include/glsdet_hip.h: the workspace of the entry points
        self.ws = torch.full((self.floats + GUARD,), GUARD_BITS, dtype=torch.int32, device=eng.device)
        eng._keep.append(self.ws)
        self.split = _split_tensor(eng, case.split) if case.kind == "split" else None

    def views(self, placed):
        from glsdet_amd._lib import View
        if self.case.kind == "split":
            return (View * 1)(placed.view.as_c())
        return (View * self.sets)(*[placed.view.window(*w).as_c() for w in R.windows(self.case)])

    def call(self, **over):
        """-> the entry point's return code.  over: operands replaced for the argument-error tests"""
        from glsdet_amd._lib import View
        lib, case, st = self.eng.lib, self.case, _stream(self.eng)
        ptrs = lambda ts: (C.c_void_p * len(ts))(*[t if t is None else t.data_ptr() for t in ts])
        x, out = over.get("x", self.views(self.x)), over.get("out", self.views(self.out))
        wa, ba = ptrs(over.get("wout", self.wout)), ptrs(over.get("bout", self.bout))
        ci, ws = over.get("ci", case.ci), self.ws.data_ptr()
        if case.kind == "split":
            ta = over.get("tpg", (View * 4)(*[t.view.as_c() for t in self.tpg]))
            return lib.glsdet_nonlocal_split(x, ta, ci, wa, ba, ws, out, self.split.data_ptr(), over.get("shift", case.shift), st)
        ta = over.get("tpg", self.views(self.tpg[0]))
        if case.kind == "static":
            return lib.glsdet_nonlocal(x, ta, ci, wa[0], ba[0], ws, out, st)
        return lib.glsdet_nonlocal_multi(x, ta, over.get("n_sets", self.sets), ci, wa, ba, ws, out, st)

    def want(self, value):
        """the destination's map as raw bits: what it held, with `value` (float64 NCHW, NaN where no set writes) rounded once"""
        mode = self.mode
        held = self.out.grid(self.out.host)[self.out.index].copy()
        keep = np.isnan(value).transpose(0, 2, 3, 1)
        bits = _bits(R.round_to(np.nan_to_num(value), mode), mode)
        return np.where(keep, held, bits)

    def failures(self, want_bits):
        """contracts 1 - 4 after a launch -> messages"""
        bad = []
        msg = self.out.mismatch(want_bits)
        if msg:
            bad.append("out: " + msg)
        if self.out is not self.x and self.x.mismatch(None):
            bad.append("x was written: " + self.x.mismatch(None))
        for q, t in enumerate(self.tpg):
            if t.mismatch(None):
                bad.append("theta|phi|g %d was written: %s" % (q, t.mismatch(None)))
        ws = self.ws.cpu().numpy()
        if (ws[self.floats:] != GUARD_BITS).any():
            bad.append("%d elements behind the documented workspace were written" % int((ws[self.floats:] != GUARD_BITS).sum()))
        if not (ws[: self.floats] != GUARD_BITS).any():
            bad.append("the workspace was not used")
        return bad


def _run_exact(engines, mode, case):
    eng = engines[mode]
    with _scratch(eng):
        run = Launch(eng, mode, case, R.case_data(case))
        rc = run.call()
        assert rc == 0, eng.lib.glsdet_last_error().decode()
        bad = run.failures(run.want(R.expected(case)))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.STATIC_CASES, ids=_IDS)
def test_nonlocal_bit_for_bit(engines, mode, case):
    _run_exact(engines, mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.MULTI_CASES, ids=_IDS)
def test_nonlocal_multi_on_windows_of_one_buffer_bit_for_bit(engines, mode, case):
    """1..4 sets with unequal extents and their own weights, as the static quadrants of an odd-sized map and as arbitrary
    windows; the pixels of the map that no set owns keep their bits"""
    _run_exact(engines, mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.SPLIT_CASES, ids=_IDS)
def test_nonlocal_split_bit_for_bit(engines, mode, case):
    """the split is a host-written int32[4] device tensor; nl_window derives offset, N, jchunk and 1 / N from it.  Every
    pixel of the map is written exactly once: no sentinel and no NaN is left inside it"""
    assert not np.isnan(R.expected(case)).any()
    _run_exact(engines, mode, case)


@pytest.mark.parametrize("mode", MODES)
def test_nonlocal_dot_op_bit_for_bit(mode):
    import glsdet_amd.torch_ops  # noqa: F401
    case = R.DOT_CASE
    d = R.case_data(case)
    tt = torch.float16 if mode == "f16" else torch.float32
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))).to(tt).cuda()
    x, tpg = nhwc(d["x"]), nhwc(d["tpg"][0])
    assert not torch.isnan(tpg).any()
    y = torch.ops.glsdet.nonlocal_dot(x, tpg, case.ci, torch.from_numpy(d["wout"][0].astype(np.float32)).cuda(),
                                      torch.from_numpy(d["bout"][0].astype(np.float32)).cuda())
    torch.cuda.synchronize()
    assert y.dtype == tt and tuple(y.shape) == tuple(x.shape)
    got = y.cpu().numpy().view(_IT[mode])
    assert np.array_equal(got, _bits(R.round_to(R.expected(case), mode), mode))
    assert np.array_equal(x.cpu().numpy().view(_IT[mode]), _bits(d["x"], mode)), "x was written"


# ------------------------------------------------------------------------------------------------------ argument errors
def _two_sets_with(run, eng, mode, n=None, c=None):
    """x (= out) and theta | phi | g views of a two-set call whose second set has other channels or another image count"""
    from glsdet_amd._lib import View
    case = run.case
    n, c = n or case.n, c or case.cx
    ox = NlPlaced(eng, "dense", n, case.FH, case.FW, c, mode, NAN[mode]).upload()
    ot = NlPlaced(eng, "dense", n, case.FH, case.FW, case.tw, mode, NAN[mode]).upload()
    w = R.windows(case)
    xs = (View * 2)(run.x.view.window(*w[0]).as_c(), ox.view.window(*w[1]).as_c())
    return dict(x=xs, out=xs, tpg=(View * 2)(run.tpg[0].view.window(*w[0]).as_c(), ot.view.window(*w[1]).as_c()))


@pytest.mark.parametrize("mode", MODES)
def test_argument_errors_are_reported_and_nothing_is_written(engines, mode):
    from glsdet_amd._lib import GlsdetError, View, check
    eng = engines[mode]
    other = "f32" if mode == "f16" else "f16"
    multi, split, static = R.MULTI_CASES[3], R.SPLIT_CASES[1], R.STATIC_CASES[1]
    assert multi.okind and split.okind and static.okind and len(multi.wins) == 2
    with _scratch(eng):
        runs = {c.kind: Launch(eng, mode, c, R.case_data(c)) for c in (multi, split, static)}
        m, s, t = runs["multi"], runs["split"], runs["static"]
        narrow = lambda run: NlPlaced(eng, "dense", run.case.n, run.case.FH, run.case.FW, 3 * run.case.ci - 8, mode, NAN[mode]).upload()
        wrong_t = lambda run: NlPlaced(eng, "dense", run.case.n, run.case.FH, run.case.FW, run.case.tw, other, NAN[other]).upload()
        wrong_o = lambda run: NlPlaced(eng, "dense", run.case.n, run.case.FH, run.case.FW, run.case.cx, other, SENTINEL[other]).upload()
        bad_calls = [
            ("n_sets 0", m, dict(n_sets=0)),
            ("n_sets 5", m, dict(n_sets=5)),
            ("sets that disagree in channels", m, _two_sets_with(m, eng, mode, c=m.case.cx + 8)),
            ("sets that disagree in n", m, _two_sets_with(m, eng, mode, n=m.case.n + 1)),
            ("multi: tpg.c < 3 ci", m, dict(tpg=m.views(narrow(m)))),
            ("static: tpg.c < 3 ci", t, dict(tpg=t.views(narrow(t)))),
            ("split: tpg.c < 3 ci", s, dict(tpg=(View * 4)(*[narrow(s).view.as_c() for _ in range(4)]))),
            ("multi: tpg of another dtype", m, dict(tpg=m.views(wrong_t(m)))),
            ("static: out of another dtype", t, dict(out=t.views(wrong_o(t)))),
            ("split: tpg of another dtype", s, dict(tpg=(View * 4)(*[wrong_t(s).view.as_c() for _ in range(4)]))),
            ("split: out of another dtype", s, dict(out=s.views(wrong_o(s)))),
            ("split_shift 2", s, dict(shift=2)),
            ("split_shift -1", s, dict(shift=-1)),
            ("multi: a null wout", m, dict(wout=[m.wout[0], None])),
            ("multi: a null bout", m, dict(bout=[None, m.bout[1]])),
            ("static: a null wout", t, dict(wout=[None])),
            ("split: a null wout", s, dict(wout=s.wout[:3] + [None])),
            ("split: a null bout", s, dict(bout=[None] + s.bout[1:])),
        ]
        for what, run, over in bad_calls:
            with pytest.raises(GlsdetError):
                check(run.call(**over), what)
            torch.cuda.synchronize()
            for name, buf in (("out", run.out), ("x", run.x)):
                assert buf.mismatch(None) is None, "%s: %s changed" % (what, name)
            assert (run.ws.cpu().numpy() == GUARD_BITS).all(), "%s: the workspace was written" % what
        for run in (m, s, t):                                            # the same operands, unmodified, are accepted
            assert run.call() == 0, eng.lib.glsdet_last_error().decode()
            assert not run.failures(run.want(R.expected(run.case)))


# -------------------------------------------------------------------------------------- continuous operands, a-priori bound
def _run_generic(engines, mode, case):
    eng = engines[mode]
    d = R.generic_data(case, mode, 1000 + case.seed)
    ref, bound, term = R.generic_reference_and_bound(case, d, mode)
    with _scratch(eng):
        run = Launch(eng, mode, case, d)
        assert run.call() == 0, eng.lib.glsdet_last_error().decode()
        got, bits = run.out.read()
        inside = ~np.isnan(ref)
        held = run.out.grid(run.out.host)[run.out.index]
        rest = run.failures(np.where(inside.transpose(0, 2, 3, 1), bits, held))      # all but the values: the four contracts
    assert not rest, "\n".join(rest)
    assert not np.isnan(got[inside]).any()
    ratio = float((np.abs(got[inside] - ref[inside]) / bound[inside]).max())
    print("nonlocal %s %s %s: max |err| / B = %.3f, largest non-local term %.2f" % (case.kind, case.name, mode, ratio, np.nanmax(np.abs(term))))
    assert np.nanmax(np.abs(term)) > 0.25                                # the block contributes: a wrong 1 / N is seen
    assert (np.abs(got[inside] - ref[inside]) <= bound[inside]).all(), "max |err| / B = %.3f" % ratio


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.GENERIC_CASES["static"], ids=_IDS)
def test_nonlocal_generic_operands_within_the_a_priori_bound(engines, mode, case):
    _run_generic(engines, mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.GENERIC_CASES["multi"], ids=_IDS)
def test_nonlocal_multi_generic_operands_within_the_a_priori_bound(engines, mode, case):
    _run_generic(engines, mode, case)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.GENERIC_CASES["split"], ids=_IDS)
def test_nonlocal_split_generic_operands_within_the_a_priori_bound(engines, mode, case):
    _run_generic(engines, mode, case)
