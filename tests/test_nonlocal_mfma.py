"""The matrix-core non-local kernels (nlm_gram / nlm_fold / nlm_apply, glsdet_amd/csrc/nonlocal_mfma.hip) behind
glsdet_nonlocal_mfma, Engine.nonlocal_multi(mfma=True) and torch.ops.glsdet.nonlocal_dot_mfma, against
tests/nonlocal_reference.py on the cases of tests/nonlocal_mfma_cases.py.

Exact regime: every float32 step is exact in any order of the sums (tests/test_cross10_reference.py asserts per case that
the regime bounds sums of magnitudes), so the output must equal the float64 definition rounded ONCE to the output type, bit
for bit, whatever order the MFMA sums in.  The contracts of tests/test_nonlocal_exact.py hold per launch: the destination
allocation is sentinel-filled and compared WHOLE, x and theta | phi | g sit in NaN-poisoned buffers and are compared whole
afterwards, the workspace has exactly glsdet_nonlocal_mfma_workspace_bytes followed by a guard that stays untouched.

Continuous operands are held to nonlocal_reference.generic_reference_and_bound, unchanged: it bounds any order of
one-rounding fp32 additions, which is what v_mfma_f32_32x32x2_f32 does; for the fp16 Gram (v_mfma_f32_32x32x16_f16) it
assumes the MFMA's internal additions are no worse."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import nonlocal_mfma_cases as M
from tests import nonlocal_reference as R
from tests.test_conv_exact import NAN, SENTINEL, _bits, _scratch, _stream, engines  # noqa: F401  (engines: the fixture)
from tests.test_conv_exact import _FT, _IT, _TT
from tests.test_nonlocal_exact import GUARD, GUARD_BITS, Launch, NlPlaced

pytestmark = pytest.mark.gpu

MODES = ["f16", "f32"]
_IDS = lambda c: c.name


class MfmaPlaced(NlPlaced):
    """NlPlaced on the layouts of nonlocal_mfma_cases.layout ('dense', 'window32')"""

    def __init__(self, eng, kind, n, h, w, c, dt, fill):
        from glsdet_amd._lib import F16, F32
        from glsdet_amd.engine import TView
        self.dt, self.eng = dt, eng
        code = F16 if dt == "f16" else F32
        H, W, Ct, h0, w0, c0 = M.layout(kind, h, w, c)
        buf = eng.raw(n * H * W * Ct * np.dtype(_IT[dt]).itemsize)
        self.full = TView(buf, 0, n, H, W, Ct, H * W * Ct, W * Ct, Ct, code)
        self.view = TView(buf, (h0 * W + w0) * Ct + c0, n, h, w, c, H * W * Ct, W * Ct, Ct, code)
        self.shape = (n, H, W, Ct)
        self.index = (slice(None), slice(h0, h0 + h), slice(w0, w0 + w), slice(c0, c0 + c))
        self.host = np.full(buf.numel() // np.dtype(_IT[dt]).itemsize, fill, _IT[dt])


def _f32(eng, a):
    return eng.upload(torch.from_numpy(np.ascontiguousarray(a, np.float32)))


class MfmaLaunch(Launch):
    """the operands of one case on the device and the direct ctypes call of glsdet_nonlocal_mfma (old=True: of
    glsdet_nonlocal_multi on the same operands)"""

    def __init__(self, eng, mode, case, d):
        self.eng, self.mode, self.case = eng, mode, case
        n, ci, cx = case.n, case.ci, case.cx
        self.x = MfmaPlaced(eng, case.xkind, n, case.FH, case.FW, cx, mode, NAN[mode]).put(d["x"]).upload()
        self.out = self.x if case.okind is None else MfmaPlaced(eng, case.okind, n, case.FH, case.FW, cx, mode, SENTINEL[mode]).upload()
        self.tpg = [MfmaPlaced(eng, case.tkind, n, case.FH, case.FW, case.tw, mode, NAN[mode]).put(t).upload() for t in d["tpg"]]
        self.wout = [_f32(eng, w) for w in d["wout"]]
        self.bout = [_f32(eng, b) for b in d["bout"]]
        self.sets = len(R.windows(case))
        self.bytes = eng.lib.glsdet_nonlocal_mfma_workspace_bytes(n, self.sets, ci, cx)
        assert self.bytes == (self.sets * n * (8 * ci * ci + cx * ci) * 4 + 255) // 256 * 256
        self.floats = self.bytes // 4
        self.ws = torch.full((self.floats + GUARD,), GUARD_BITS, dtype=torch.int32, device=eng.device)
        assert self.ws.data_ptr() % 256 == 0
        eng._keep.append(self.ws)
        self.split = None

    def call(self, old=False):
        lib, case, st = self.eng.lib, self.case, _stream(self.eng)
        ptrs = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
        x, out, ta = self.views(self.x), self.views(self.out), self.views(self.tpg[0])
        if old:
            return lib.glsdet_nonlocal_multi(x, ta, self.sets, case.ci, ptrs(self.wout), ptrs(self.bout), self.ws.data_ptr(), out, st)
        return lib.glsdet_nonlocal_mfma(x, ta, self.sets, case.ci, ptrs(self.wout), ptrs(self.bout), self.ws.data_ptr(),
                                        self.bytes, out, st)

    def views(self, placed):
        from glsdet_amd._lib import View
        return (View * self.sets)(*[placed.view.window(*w).as_c() for w in R.windows(self.case)])


# ------------------------------------------------------------------------------------------------------ exact regime
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", M.EXACT_CASES, ids=_IDS)
def test_nonlocal_mfma_bit_for_bit(engines, mode, case):
    eng = engines[mode]
    d = M.data(case)
    with _scratch(eng):
        run = MfmaLaunch(eng, mode, case, d)
        rc = run.call()
        assert rc == 0, eng.lib.glsdet_last_error().decode()
        bad = run.failures(run.want(R.expected(case)))
    assert not bad, "\n".join(bad)


# -------------------------------------------------------------------------------------- continuous operands, the bound
_GENERIC = {}


def _generic(case, mode):
    """(data, reference, bound, term) of a case, computed once and shared by the tests below"""
    key = (case.name, mode)
    if key not in _GENERIC:
        d = R.generic_data(case, mode, 1000 + case.seed)
        _GENERIC[key] = (d,) + R.generic_reference_and_bound(case, d, mode)
    return _GENERIC[key]


def _launch_generic(eng, mode, case, old=False):
    d, ref, bound, term = _generic(case, mode)
    run = MfmaLaunch(eng, mode, case, d)
    assert run.call(old=old) == 0, eng.lib.glsdet_last_error().decode()
    got, bits = run.out.read()
    inside = ~np.isnan(ref)
    held = run.out.grid(run.out.host)[run.out.index]
    rest = run.failures(np.where(inside.transpose(0, 2, 3, 1), bits, held))          # all but the values: the four contracts
    assert not rest, "\n".join(rest)
    assert not np.isnan(got[inside]).any()
    return got, bits, inside


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", M.GENERIC_CASES, ids=_IDS)
def test_nonlocal_mfma_generic_operands_within_the_a_priori_bound(engines, mode, case):
    eng = engines[mode]
    d, ref, bound, term = _generic(case, mode)
    with _scratch(eng):
        got, bits, inside = _launch_generic(eng, mode, case)
    ratio = float((np.abs(got[inside] - ref[inside]) / bound[inside]).max())
    print("nonlocal_mfma %s %s: max |err| / B = %.3f, largest non-local term %.2f" % (case.name, mode, ratio, np.nanmax(np.abs(term))))
    assert np.nanmax(np.abs(term)) > 0.25                                # the block contributes: a wrong 1 / N is seen
    assert (np.abs(got[inside] - ref[inside]) <= bound[inside]).all(), "max |err| / B = %.3f" % ratio


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", M.GENERIC_CASES, ids=_IDS)
def test_nonlocal_mfma_against_the_scalar_kernels(engines, mode, case):
    """the same continuous operands through glsdet_nonlocal_multi: both are within B of the reference, so fp32 outputs
    differ by at most 2 B; fp16 outputs by at most ONE fp16 ulp per element, the ulp of the larger of the two outputs.
    That holds wherever x + bout + term does not cancel: the two fp32 sums are 1e-7 of the addends apart, far below the
    output's ulp, so they round to the same fp16 number or to neighbours.  Where the sum cancels below an eighth of
    |x| + |bout| + |term| the output's ulp shrinks under what the fp32 sums resolve and no two summation orders are an ulp
    of the RESULT apart (measured on an MI355X: up to 4 ulp of an output of 1e-3 next to addends of 1); those elements are
    counted -- they must stay a minority -- and held to one fp16 ulp of the ADDENDS' magnitude, an absolute bar that does
    not grow with the a-priori bound."""
    eng = engines[mode]
    d, ref, bound, term = _generic(case, mode)
    with _scratch(eng):
        new, nbits, inside = _launch_generic(eng, mode, case)
        old, obits, _ = _launch_generic(eng, mode, case, old=True)
    diff = np.abs(new[inside] - old[inside])
    if mode == "f32":
        ratio = float((diff / (2 * bound[inside])).max())
        print("nonlocal_mfma vs nonlocal_multi %s f32: max |diff| / 2B = %.4f" % (case.name, ratio))
        assert (diff <= 2 * bound[inside]).all(), ratio
        return
    x, tm, rf = d["x"][inside], term[inside], ref[inside]
    mag = np.abs(x) + np.abs(rf - x - tm) + np.abs(tm)                   # |x| + |bout| + |term|
    out = np.maximum(np.abs(new[inside]), np.abs(old[inside]))
    ulp16 = lambda v: np.spacing(v.astype(np.float16)).astype(np.float64)
    cancelled = out < mag / 8
    print("nonlocal_mfma vs nonlocal_multi %s f16: %.2f %% of the elements differ; %.1f %% cancel below 1/8 of their addends; max %.2f ulp "
          "of the output where they do not, %.2f ulp of the addends where they do" % (
              case.name, 100 * float((diff > 0).mean()), 100 * float(cancelled.mean()), float((diff / ulp16(out))[~cancelled].max()),
              float((diff / ulp16(mag))[cancelled].max()) if cancelled.any() else 0.0))
    assert cancelled.mean() < 0.25
    assert (diff[~cancelled] <= ulp16(out)[~cancelled]).all()
    assert (diff[cancelled] <= ulp16(mag)[cancelled]).all()


# ----------------------------------------------------------------------------------------------- Engine.nonlocal_multi
def _engine_run(eng, mode, case, d, mfma, separate, names=None):
    """Engine.nonlocal_multi on dense device tensors of the case -> the output's raw bits (NHWC)"""
    from glsdet_amd._lib import F16, F32
    code = F16 if mode == "f16" else F32
    tt = torch.float16 if mode == "f16" else torch.float32
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(np.nan_to_num(np.asarray(a)).transpose(0, 2, 3, 1))).to(tt)
    x, t = eng.tensor(case.n, case.FH, case.FW, case.cx, code), eng.tensor(case.n, case.FH, case.FW, case.tw, code)
    x.buf.view(tt)[: x.n * x.sn] = nhwc(d["x"]).reshape(-1).to(eng.device)
    t.buf.view(tt)[: t.n * t.sn] = nhwc(d["tpg"][0]).reshape(-1).to(eng.device)
    o = eng.tensor(case.n, case.FH, case.FW, case.cx, code) if separate else x
    wins = R.windows(case)
    call = lambda: eng.nonlocal_multi([x.window(*w) for w in wins], [t.window(*w) for w in wins], case.ci, [_f32(eng, w) for w in d["wout"]],
                                      [_f32(eng, b) for b in d["bout"]], outs=[o.window(*w) for w in wins] if separate else None, mfma=mfma)
    if names is not None:                                            # recorded, not launched: which entry point was taken
        from glsdet_amd.engine import Plan
        plan = Plan(eng.lib)
        with plan:
            call()
        names.extend(op["name"] for op in plan.ops())
    ys = call()
    assert len(ys) == len(wins)
    torch.cuda.synchronize()
    return o.buf.view(_TT[mode])[: o.n * o.sn].cpu().numpy().reshape(case.n, case.FH, case.FW, case.cx)


@pytest.mark.parametrize("mode", MODES)
def test_engine_mfma_true_takes_the_new_kernels_and_false_the_old(engines, mode):
    """in the exact regime both give the once-rounded reference; with continuous operands mfma=False equals a direct
    glsdet_nonlocal_multi call and mfma=True a direct glsdet_nonlocal_mfma call bit for bit, and a recorded plan names the
    entry point that was taken (default arguments keep every existing caller's kernels)"""
    eng = engines[mode]
    case = M.EXACT_CASES[8]                                          # the four quadrants of a 5 x 7 map
    want = _bits(R.round_to(np.nan_to_num(R.expected(case)), mode), mode)
    with _scratch(eng):
        for mfma in (False, True):
            for separate in (False, True):
                got = _engine_run(eng, mode, case, M.data(case), mfma, separate)
                assert np.array_equal(got, want), (mfma, separate)
        gcase = M.GENERIC_CASES[3]
        d = _generic(gcase, mode)[0]
        dense = R._multi("mfma-dense-twin", gcase.ci, gcase.cx, gcase.FH, gcase.FW, gcase.wins, gcase.n, "dense", "dense", None)
        for mfma in (False, True):                                   # continuous operands: the dispatch shows in the op name
            run = MfmaLaunch(eng, mode, dense, d)                    # and in bit equality with the direct call of that entry
            assert run.call(old=not mfma) == 0
            direct, dbits = run.out.read()
            names = []
            via_engine = _engine_run(eng, mode, gcase, d, mfma, False, names)
            assert np.array_equal(via_engine, dbits), mfma
            assert len(names) == 1 and ("nonlocal_mfma" in names[0]) == mfma, names


@pytest.mark.parametrize("mode", MODES)
def test_engine_falls_back_where_a_precondition_fails(engines, mode):
    """ci = 40: Engine.nonlocal_multi(mfma=True) does not raise and equals mfma=False bit for bit"""
    eng = engines[mode]
    case = M.FALLBACK_CASE
    d = R.generic_data(case, mode, 77)
    with _scratch(eng):
        a = _engine_run(eng, mode, case, d, True, True)
        b = _engine_run(eng, mode, case, d, False, True)
    assert np.array_equal(a, b) and not np.isnan(a.view(_FT[mode]).astype(np.float64)).any()


# ------------------------------------------------------------------------------------------- torch op, graph capture
@pytest.mark.parametrize("mode", MODES)
def test_nonlocal_dot_mfma_op_eager_and_captured(mode):
    import glsdet_amd.torch_ops  # noqa: F401
    case = R._static("mfma-dot-ci64-c96-5x13", 64, 96, 5, 13, 3, "dense", "dense", "dense")
    tt = torch.float16 if mode == "f16" else torch.float32
    nhwc = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a).transpose(0, 2, 3, 1))).to(tt).cuda()
    d = R.case_data(case)
    R.check_regime(case, d)
    x, tpg = nhwc(d["x"]), nhwc(d["tpg"][0])
    wout, bout = torch.from_numpy(d["wout"][0].astype(np.float32)).cuda(), torch.from_numpy(d["bout"][0].astype(np.float32)).cuda()
    y = torch.ops.glsdet.nonlocal_dot_mfma(x, tpg, case.ci, wout, bout)
    torch.cuda.synchronize()
    assert y.dtype == tt and tuple(y.shape) == tuple(x.shape)
    assert np.array_equal(y.cpu().numpy().view(_IT[mode]), _bits(R.round_to(R.expected(case), mode), mode))
    assert np.array_equal(x.cpu().numpy().view(_IT[mode]), _bits(d["x"], mode)), "x was written"
    with pytest.raises(RuntimeError):
        torch.ops.glsdet.nonlocal_dot_mfma(x[..., :40].contiguous(), tpg[..., :120].contiguous(), 40, wout[:40, :40].contiguous(), bout[:40])
    # captured once, replayed on new input: bit-equal to eager, and equal across two replays
    g2 = R.generic_data(case, mode, 5)
    x2, t2 = nhwc(g2["x"]), nhwc(g2["tpg"][0])
    eager = torch.ops.glsdet.nonlocal_dot_mfma(x2, t2, case.ci, wout, bout).clone()
    sx, st = x.clone(), tpg.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        torch.ops.glsdet.nonlocal_dot_mfma(sx, st, case.ci, wout, bout)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sy = torch.ops.glsdet.nonlocal_dot_mfma(sx, st, case.ci, wout, bout)
    sx.copy_(x2)
    st.copy_(t2)
    graph.replay()
    torch.cuda.synchronize()
    first = sy.clone()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first.view(_TT[mode]), eager.view(_TT[mode])) and torch.equal(sy.view(_TT[mode]), first.view(_TT[mode]))
