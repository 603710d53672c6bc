"""CPU tests of kind `cross10` (the reference's models/new/yolox10.py): the state-dict tables, the CPU restatement
tests/cross10_reference.py against the outputs the reference's own module gave (tests/golden/cross10_golden.npz), the drone
twin as a parameter container, the host-side refusals and the workspace helper of glsdet_nonlocal_mfma, and the case list
of the matrix-core kernels (tests/nonlocal_mfma_cases.py).  Nothing here needs a GPU: the library calls below are refused
before anything is launched and no pointer is dereferenced.

The case-list tests at the end validate test DATA (that every kernel case lies inside the exact regime of
tests/nonlocal_reference.py); they hold the feature only through the one line that asks the engine's precondition mirror
whether the kernels take the case."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from tests import cross10_reference as X
from tests import nonlocal_mfma_cases as M
from tests import nonlocal_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASE_IDS = [X.case_name(*c) for c in X.CASES]


# ------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("phi", X.TABLE_PHIS)
def test_cross10_table_is_the_reference_modules_state_dict(phi):
    from glsdet_amd.arch import KINDS, state_dict_shapes
    assert "cross10" in KINDS
    want = X.table(phi)
    got = state_dict_shapes("cross10", phi, X.NUM_CLASSES)
    assert [(k, tuple(v)) for k, v in got.items()] == list(want.items())
    assert len(want) == {"tiny": 654, "nano": 882}.get(phi, len(want))


@pytest.mark.parametrize("phi", X.TABLE_PHIS)
def test_cross_table_is_cross10_without_the_three_blocks(phi):
    from glsdet_amd.arch import state_dict_shapes
    cross = state_dict_shapes("cross", phi, X.NUM_CLASSES)
    c10 = state_dict_shapes("cross10", phi, X.NUM_CLASSES)
    extra = [k for k in c10 if k not in cross]
    assert len(extra) == 3 * 38 and all(k.startswith("backbone.Patch_conv_feat") for k in extra)
    assert [(k, v) for k, v in c10.items() if k in cross] == list(cross.items())
    keys = list(c10)
    first = keys.index(extra[0])
    assert keys[first - 1].startswith("backbone.C3_n4.") and keys[first + len(extra)].startswith("head.")
    assert keys[first:first + len(extra)] == extra


# ------------------------------------------------------------------------------------------------------- composition
@pytest.fixture(scope="module")
def outputs():
    """cross10_forward of every case, computed once"""
    out = {}
    with torch.no_grad():
        for phi, shape in X.CASES:
            out[X.case_name(phi, shape)] = X.cross10_forward(X.weights(phi), X.case_input(phi, shape))
    return out


@pytest.mark.parametrize("case", X.CASES, ids=_CASE_IDS)
def test_composition_equals_the_reference_module(outputs, case):
    got, want = outputs[X.case_name(*case)], X.recorded(*case)
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    err = X.rel(got, want)
    print("cross10_forward %s: %.3e relative to max(1, |logit|)" % (X.case_name(*case), err))
    assert err <= 1e-6


@pytest.mark.parametrize("case", X.CASES, ids=_CASE_IDS)
def test_the_nonlocal_term_moves_the_logits(outputs, case):
    """the condition that makes the end-to-end tests see the non-local kernels: without the twelve conv_out the logits
    move by at least 100 x the GPU test's f32 bar"""
    phi, shape = case
    sd = X.weights(phi)
    zeroed = [k for k in sd if ".conv_out." in k]
    assert len(zeroed) == 24                                      # twelve weights, twelve biases
    for k in zeroed:
        sd[k] = torch.zeros_like(sd[k])
    with torch.no_grad():
        moved = X.rel(X.cross10_forward(sd, X.case_input(phi, shape)), outputs[X.case_name(phi, shape)])
    print("cross10 %s: conv_out zeroed moves the logits by %.3e" % (X.case_name(phi, shape), moved))
    assert moved >= 100 * X.F32_BAR


# -------------------------------------------------------------------------------------------------------------- twin
def test_drone_twin_is_the_reference_container():
    drone = os.path.join(ROOT, "glsdet_amd", "drone")
    saved_path, saved_mods = list(sys.path), {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.")}
    for k in saved_mods:
        del sys.modules[k]
    sys.path.insert(0, drone)
    try:
        import importlib
        mod = importlib.import_module("models.new.yolox10")
        body = mod.YoloBody(X.NUM_CLASSES, "tiny")
        want = X.table("tiny")
        assert list(body.state_dict().keys()) == list(want)
        assert [tuple(v.shape) for v in body.state_dict().values()] == list(want.values())
        sd = X.weights("tiny")
        body.load_state_dict(sd, strict=True)
        k = "backbone.Patch_conv_feat3.feat_patchconv_rb_nonlocal.conv_out.weight"
        assert torch.equal(body.state_dict()[k], sd[k])
        with pytest.raises(RuntimeError):
            body.load_state_dict({q: v for q, v in sd.items() if q != k}, strict=True)
    finally:
        sys.path[:] = saved_path
        for k in [k for k in sys.modules if k == "models" or k.startswith("models.")]:
            del sys.modules[k]
        sys.modules.update(saved_mods)


# --------------------------------------------------------------------------------------------------- host refusals
def _view(n, h, w, c, dtype=0, base=0x10000, ct=None, extra=0):
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    ct = c if ct is None else ct
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = ct, w * ct, h * w * ct
    lo = base & ~0xFF
    v.alloc_lo, v.alloc_hi = lo, base + n * h * w * ct * es + extra
    return v


class _Call:
    """a well-formed two-set call of glsdet_nonlocal_mfma on fake addresses; fields are replaced per refusal"""

    def __init__(self, dtype=0):
        from glsdet_amd import _lib
        self.lib = _lib.load()
        self.n, self.ci, self.cx, self.dtype = 2, 64, 96, dtype
        self.x = [_view(2, 4, 5, 96, dtype, 0x100000), _view(2, 3, 5, 96, dtype, 0x200000)]
        self.t = [_view(2, 4, 5, 192, dtype, 0x300000), _view(2, 3, 5, 192, dtype, 0x400000)]
        self.o = list(self.x)
        self.w, self.b = [0x500000, 0x510000], [0x520000, 0x520400]
        self.ws = 0x600000
        self.ws_bytes = self.lib.glsdet_nonlocal_mfma_workspace_bytes(2, 2, 64, 96)

    def __call__(self):
        from glsdet_amd._lib import View
        k = len(self.x)
        arr = lambda vs: (View * max(k, 1))(*vs)
        ptr = lambda ps: (C.c_void_p * max(k, 1))(*ps)
        rc = self.lib.glsdet_nonlocal_mfma(arr(self.x), arr(self.t), self.n, self.ci, ptr(self.w), ptr(self.b), self.ws,
                                           self.ws_bytes, arr(self.o), None)
        return rc, self.lib.glsdet_last_error().decode()


def _refusals():
    def sets(k):
        def f(c):
            c.n = k
        return f

    def field(name, value):
        def f(c):
            setattr(c, name, value)
        return f

    def second(name, view):
        def f(c):
            lst = list(getattr(c, name))
            lst[1] = view(c)
            setattr(c, name, lst)
            if name == "x":
                c.o = list(lst)
        return f
    d = lambda c: c.dtype
    return [
        ("n_sets 0", sets(0), "sets"),
        ("n_sets 5", sets(5), "sets"),
        ("ci 40", field("ci", 40), "ci must be a multiple of 32"),
        ("ci 0", field("ci", 0), "ci must be a multiple of 32"),
        ("ci 1312", field("ci", 1312), "ci must be a multiple of 32"),
        ("cx 40", lambda c: (setattr(c, "x", [_view(2, 4, 5, 40, d(c), 0x100000), _view(2, 3, 5, 40, d(c), 0x200000)]),
                             setattr(c, "o", list(c.x))), "x channels must be a multiple of 32"),
        ("cx 1312", lambda c: (setattr(c, "x", [_view(2, 4, 5, 1312, d(c), 0x100000), _view(2, 3, 5, 1312, d(c), 0x200000)]),
                               setattr(c, "o", list(c.x))), "x channels must be a multiple of 32"),
        ("sets disagree in n", second("x", lambda c: _view(3, 3, 5, 96, d(c), 0x200000)), "agree in n and channels"),
        ("sets disagree in channels", second("x", lambda c: _view(2, 3, 5, 128, d(c), 0x200000)), "agree in n and channels"),
        ("tpg.c < 3 ci", second("t", lambda c: _view(2, 3, 5, 160, d(c), 0x400000)), "theta|phi|g"),
        ("tpg of another extent", second("t", lambda c: _view(2, 4, 5, 192, d(c), 0x400000)), "theta|phi|g"),
        ("out of another extent", second("o", lambda c: _view(2, 5, 3, 96, d(c), 0x700000)), "extent mismatch"),
        ("x base not 16-byte aligned", second("x", lambda c: _view(2, 3, 5, 96, d(c), 0x200008)), "16-byte"),
        ("tpg pixel stride not 16-byte aligned", second("t", lambda c: _view(2, 3, 5, 192, d(c), 0x400000, ct=194)), "16-byte"),
        ("out window offset not 16-byte aligned", second("o", lambda c: _view(2, 3, 5, 96, d(c), 0x700004)), "16-byte"),
        ("tpg of another dtype", second("t", lambda c: _view(2, 3, 5, 192, 1 - d(c), 0x400000)), "one dtype"),
        ("out of another dtype", second("o", lambda c: _view(2, 3, 5, 96, 1 - d(c), 0x700000)), "one dtype"),
        ("a dtype that is neither", lambda c: (setattr(c, "x", [_view(2, 4, 5, 96, 2, 0x100000), _view(2, 3, 5, 96, 2, 0x200000)]),
                                               setattr(c, "o", list(c.x))), "dtype"),
        ("an empty window", second("x", lambda c: _view(2, 0, 5, 96, d(c), 0x200000)), "empty extent"),
        ("a view outside its allocation", second("t", lambda c: _view(2, 3, 5, 192, d(c), 0x400000, extra=-2)), "leaves its allocation"),
        ("ws not 256-byte aligned", field("ws", 0x600010), "256-byte aligned"),
        ("ws one byte short", lambda c: setattr(c, "ws_bytes", c.ws_bytes - 1), "needed"),
        ("a null ws", field("ws", None), "null"),
        ("a null wout", lambda c: setattr(c, "w", [c.w[0], None]), "null weight"),
        ("a misaligned bout", lambda c: setattr(c, "b", [c.b[0], 0x520404]), "16-byte"),
    ]


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "f32"])
@pytest.mark.parametrize("what,change,text", _refusals(), ids=[r[0] for r in _refusals()])
def test_nonlocal_mfma_refuses_on_the_host(dtype, what, change, text):
    call = _Call(dtype)
    change(call)
    rc, msg = call()
    assert rc < 0, what
    assert "nonlocal_mfma" in msg and text in msg, (what, msg)


def test_nonlocal_mfma_null_arrays_are_refused():
    from glsdet_amd import _lib
    lib = _lib.load()
    assert lib.glsdet_nonlocal_mfma(None, None, 1, 32, None, None, None, 0, None, None) < 0
    assert "nonlocal_mfma" in lib.glsdet_last_error().decode()


def test_nonlocal_mfma_workspace_helper():
    from glsdet_amd import _lib
    f = _lib.load().glsdet_nonlocal_mfma_workspace_bytes
    base = f(2, 2, 64, 96)
    assert base == 2 * 2 * (8 * 64 * 64 + 96 * 64) * 4 and base % 256 == 0
    assert f(1, 1, 32, 32) > 0
    assert f(2, 3, 64, 96) > base and f(2, 2, 96, 96) > base and f(2, 2, 64, 128) > base and f(3, 2, 64, 96) > base
    prev = 0
    for ci in range(32, 1281, 32):
        cur = f(8, 4, ci, ci)
        assert cur > prev and cur % 256 == 0 and cur >= 4 * 8 * (8 * ci * ci + ci * ci) * 4
        prev = cur
    assert f(0, 1, 32, 32) == 0 and f(1, 5, 32, 32) == 0 and f(1, 1, 0, 32) == 0


def _cpu_views(case, dt):
    """the case's x / tpg / out views on host buffers (addresses and strides only; nothing reads them)"""
    from glsdet_amd._lib import F16, F32
    from glsdet_amd.engine import TView
    code, es = (F16, 2) if dt == "f16" else (F32, 4)

    def place(kind, c):
        H, W, Ct, h0, w0, c0 = M.layout(kind, case.FH, case.FW, c)
        buf = torch.zeros(case.n * H * W * Ct * es + 64, dtype=torch.uint8)
        buf = buf[(-buf.data_ptr()) % 64:]
        return TView(buf, (h0 * W + w0) * Ct + c0, case.n, case.FH, case.FW, c, H * W * Ct, W * Ct, Ct, code)
    x, t = place(case.xkind, case.cx), place(case.tkind, case.tw)
    o = x if case.okind is None else place(case.okind, case.cx)
    wins = R.windows(case)
    return [x.window(*w) for w in wins], [t.window(*w) for w in wins], [o.window(*w) for w in wins]


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_engine_precondition_mirror_matches_the_case_lists(dt):
    """Engine.nonlocal_mfma_takes is plain arithmetic on views: every kernel case is taken, the fallback case and a
    misaligned window are not"""
    from glsdet_amd.engine import Engine
    takes = lambda xs, ts, os_, ci: Engine.nonlocal_mfma_takes(None, xs, ts, ci, os_)
    for case in M.EXACT_CASES + M.GENERIC_CASES:
        xs, ts, os_ = _cpu_views(case, dt)
        assert takes(xs, ts, os_, case.ci), case.name
    xs, ts, os_ = _cpu_views(M.FALLBACK_CASE, dt)
    assert not takes(xs, ts, os_, M.FALLBACK_CASE.ci)
    xs, ts, os_ = _cpu_views(M.EXACT_CASES[3], dt)
    assert not takes(xs, ts, os_, 40) and not takes(xs * 5, ts * 5, os_ * 5, M.EXACT_CASES[3].ci)
    xs[0].off += 2
    assert not takes(xs, ts, os_, M.EXACT_CASES[3].ci)


def _tv(n, h, w, c, dt, ct=None, off=0, skew=0):
    from glsdet_amd._lib import F16, F32
    from glsdet_amd.engine import TView
    code, es = (F16, 2) if dt == "f16" else (F32, 4)
    ct = c if ct is None else ct
    buf = torch.zeros(n * h * w * ct * es + 128, dtype=torch.uint8)
    buf = buf[(-buf.data_ptr()) % 64 + skew:]
    return TView(buf, off, n, h, w, c, h * w * ct, w * ct, ct, code)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_engine_precondition_mirror_refuses_what_the_entry_refuses(dt):
    """one negative per precondition of glsdet_nonlocal_mfma that can be told from views (the others -- the workspace -- are
    the engine's own allocation).  Should the two ever drift apart, Engine.nonlocal_multi still falls back: a refusal of the
    entry launches nothing and leads to the scalar kernels."""
    from glsdet_amd.engine import Engine
    other = "f32" if dt == "f16" else "f16"
    W = torch.zeros(64, dtype=torch.float32)

    def takes(x=None, t=None, o=None, ci=64, sets=2, wouts=(), bouts=()):
        xs = [x or _tv(2, 4, 5, 96, dt) for _ in range(sets)]
        ts = [t or _tv(2, 4, 5, 192, dt) for _ in range(sets)]
        os_ = [o or v for v in xs] if o is None else [o] * sets
        return Engine.nonlocal_mfma_takes(None, xs, ts, ci, os_, wouts, bouts)
    assert takes()
    assert not takes(sets=0) and not takes(sets=5)
    assert not takes(ci=40) and not takes(ci=0) and not takes(ci=1312, t=_tv(2, 4, 5, 3 * 1312, dt))
    assert not takes(x=_tv(2, 4, 5, 40, dt)) and not takes(x=_tv(2, 4, 5, 1312, dt))
    assert not takes(t=_tv(2, 4, 5, 160, dt)) and not takes(t=_tv(2, 3, 5, 192, dt)) and not takes(t=_tv(3, 4, 5, 192, dt))
    assert not takes(o=_tv(2, 5, 4, 96, dt)) and not takes(o=_tv(2, 4, 5, 96, other)) and not takes(t=_tv(2, 4, 5, 192, other))
    assert not takes(x=_tv(2, 4, 5, 96, dt, skew=8)) and not takes(t=_tv(2, 4, 5, 192, dt, ct=194)) and not takes(x=_tv(2, 4, 5, 96, dt, ct=128, off=2))
    mixed = Engine.nonlocal_mfma_takes(None, [_tv(2, 4, 5, 96, dt), _tv(3, 4, 5, 96, dt)], [_tv(2, 4, 5, 192, dt), _tv(3, 4, 5, 192, dt)], 64,
                                       [_tv(2, 4, 5, 96, dt), _tv(3, 4, 5, 96, dt)])
    assert not mixed
    assert not Engine.nonlocal_mfma_takes(None, [_tv(2, 4, 5, 96, dt), _tv(2, 4, 5, 128, dt)], [_tv(2, 4, 5, 192, dt)] * 2, 64,
                                          [_tv(2, 4, 5, 96, dt), _tv(2, 4, 5, 128, dt)])
    assert takes(wouts=[W[:32]], bouts=[W[32:]]) and not takes(wouts=[W[1:33]]) and not takes(bouts=[W[3:35]])
    assert not takes(x=_tv(32768, 1, 1, 96, dt), t=_tv(32768, 1, 1, 192, dt))              # n * sets above the grid's 65535


# ---------------------------------------------------------------------------------------------------- the case list
@pytest.mark.parametrize("case", M.EXACT_CASES, ids=lambda c: c.name)
def test_kernel_case_is_inside_the_exact_regime(case):
    from glsdet_amd.engine import Engine
    for dt in ("f16", "f32"):                                        # the kernels take the case as it is laid out on the device
        xs, ts, os_ = _cpu_views(case, dt)
        assert Engine.nonlocal_mfma_takes(None, xs, ts, case.ci, os_), (case.name, dt)
    d = M.data(case)
    stats, inexact = R.check_regime(case, d)
    for q, s in enumerate(stats):
        assert R.good_window(s["N"], None if s["N"] not in M.TIGHT_N else 2), (case.name, s)
        assert s["mmax"] == M.mmax(case, q) and (s["N"] not in M.TIGHT_N or s["mmax"] <= 2)
    for sums in M.magnitude_sums(case):
        assert max(sums.values()) < R.LIMIT, (case.name, sums)      # sums of magnitudes: exact in ANY order
    assert np.array_equal(R.expected(case)[~np.isnan(R.expected(case))],
                          R.integer_value(case, d)[~np.isnan(R.expected(case))])


def test_regime_bounds_sums_of_magnitudes_not_signed_sums():
    """operands whose signed sums vanish but whose magnitudes reach 2^24 steps are refused by check_regime: the regime
    bounds sums of magnitudes, which is what lets the MFMA's summation order differ from the scalar kernels'"""
    case = R._static("mfma-regime-probe", 32, 32, 2, 2, 1, "dense", "dense", None)
    d = dict(R.case_data(case))
    i = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in d["ints"][0].items()}
    sign = np.where(np.arange(4) % 2 == 0, 1, -1)
    i["phi"] = np.broadcast_to((1 << 15) * sign, (1, 32, 4)).copy()           # cancels over the pixels
    i["tg"] = np.ones((1, 32, 4), np.int64)
    i["tw"] = np.ones((32, 32), np.int64)
    assert np.abs(i["phi"][0] @ i["tg"][0].T).max() == 0                     # every signed Gram sum is zero ...
    Gabs = np.abs(i["phi"][0]) @ np.abs(i["tg"][0]).T
    assert 4 * int(Gabs.max()) < R.LIMIT <= 4 * int((np.abs(i["tw"]) @ Gabs.T).max())   # ... the fold's magnitudes are not small
    with pytest.raises(AssertionError, match="fold"):
        R.check_regime(case, dict(d, ints=[i]))
