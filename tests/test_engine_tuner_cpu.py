"""Call trace of Engine's conv family against a stand-in library, on the CPU.

Engine decides at build time which launches a network gets: it fills the ConvDesc structs, asks the tuners, compares the
fused forms with the launches they replace and stores the verdicts under flat tuple keys (bench_tuning.json is keyed on
them).  None of that needs a GPU.  Here `_lib.load` returns a recorder whose `*_tune` entry points answer with scripted
(rc, best, us) triples; every scenario drives public Engine methods only and its trace -- every C-ABI call with all
descriptor fields, addresses as "operand + byte offset", the tune table and the shadow log afterwards -- must equal
tests/golden/engine_tuner_trace.json, which was recorded before the helpers of the conv family were factored out.

    python tests/test_engine_tuner_cpu.py --write      # record the golden again (only when behaviour changes on purpose)
"""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from glsdet_amd import _lib, engine                                   # noqa: E402
from glsdet_amd._lib import ConvChain, ConvDesc, CspDesc, F16, F32, View    # noqa: E402
from glsdet_amd.engine import Engine, TView, ceil_to                   # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "engine_tuner_trace.json")
SWITCHES = ("GLSDET_TUNE_CACHE", "GLSDET_FORCE_HINT", "GLSDET_FORCE_MULTI_HINT", "GLSDET_FUSE_CREDIT_US", "GLSDET_FORCE_BNECK",
            "GLSDET_GN_FUSION", "GLSDET_NO_GROUP", "GLSDET_NO_BATCH")


class FakeLib:
    """Records every entry-point call.  `*_tune` calls pop (rc, best, us) from `tunes`; a launch is refused (-1) when its
    name is in `refuse_names` or its tile hint in `refuse_hints`, and otherwise fills its outputs with a constant that
    depends on the entry point and the hint (NaN in the first element for a hint in `nan_hints`), so that the shadow
    records are not all zero."""

    def __init__(self):
        self.calls, self.tunes = [], []
        self.refuse_names, self.refuse_hints, self.nan_hints = set(), set(), set()
        self.named, self.eng = [], None

    def __getattr__(self, name):
        if not name.startswith("glsdet_"):
            raise AttributeError(name)
        return lambda *a: self._call(name, *a)

    # ---- addresses -> "operand+offset"
    def addr(self, p, lo=None, hi=None):
        if not p:
            return None
        pools = self.named + [("keep%d" % i, t) for i, t in enumerate(self.eng._keep if self.eng is not None else [])]
        for name, t in pools:
            a = t.data_ptr()
            if a <= p < a + max(t.numel() * t.element_size(), 1):
                return "%s+%d" % (name, p - a)
        if lo is not None:                       # a buffer the engine made for one comparison and dropped again
            return "tmp%d+%d" % (hi - lo, p - lo)
        return "?"

    def view(self, v):
        if not v.base:
            return None
        return [self.addr(v.base, v.alloc_lo, v.alloc_hi), v.n, v.h, v.w, v.c, v.sn, v.sh, v.sw, v.dtype, v.alloc_hi - v.alloc_lo]

    def ser(self, a):
        a = getattr(a, "_obj", a)                # C.byref(x)
        if isinstance(a, View):
            return self.view(a)
        if isinstance(a, ConvDesc):
            return {"x": self.view(a.x), "y": self.view(a.y), "res": self.view(a.res), "w": self.addr(a.w), "scale": self.addr(a.scale),
                    "bias": self.addr(a.bias), "RSspat": [a.R, a.S, a.stride, a.pad, a.act, a.tile_hint]}
        if isinstance(a, ConvChain):
            return {"y2": self.view(a.y2), "w2": self.addr(a.w2), "scale2": self.addr(a.scale2), "bias2": self.addr(a.bias2),
                    "act2": a.act2, "c0": a.c0, "cin2": a.cin2, "flags": a.flags}
        if isinstance(a, CspDesc):
            d = {"x": self.view(a.x), "y": self.view(a.y), "act": a.act, "shortcut": a.shortcut}
            d.update({k: self.addr(getattr(a, k)) for k, _ in CspDesc._fields_[2:-2]})
            return d
        if isinstance(a, C.Array):
            return [self.ser(v) for v in a]
        if isinstance(a, (C.c_int32, C.c_float)):
            return "out"
        if isinstance(a, int) and not isinstance(a, bool) and a > 1 << 24:
            return self.addr(a)
        return a

    # ---- what a launch leaves in memory
    @staticmethod
    def fill(v, val, nan):
        if not v.base:
            return
        es, dt = (2, np.float16) if v.dtype == F16 else (4, np.float32)
        need = ((v.n - 1) * v.sn + (v.h - 1) * v.sh + (v.w - 1) * v.sw + v.c) * es
        if v.base < v.alloc_lo or v.base + need > v.alloc_hi:
            return
        raw = np.ctypeslib.as_array((C.c_uint8 * need).from_address(v.base)).view(dt)
        arr = np.lib.stride_tricks.as_strided(raw, (v.n, v.h, v.w, v.c), (v.sn * es, v.sh * es, v.sw * es, es))
        arr[...] = val
        if nan:
            arr[0, 0, 0, 0] = np.nan

    def _call(self, name, *a):
        o = [getattr(v, "_obj", v) for v in a]
        rec = {"fn": name, "args": [self.ser(v) for v in a]}
        self.calls.append(rec)
        if name == "glsdet_conv_kpad":
            return ceil_to(o[0] * o[1] * o[2], 32)
        if name == "glsdet_conv_cout_pad":
            return ceil_to(o[0], 32)
        if name == "glsdet_conv_weight_elems":
            return ceil_to(o[3], 32) * ceil_to(o[0] * o[1] * o[2], 32)
        if name == "glsdet_conv2d_gnstats_bytes":
            return o[0] * o[3] * 2 * 4 * ceil_to(o[1] * o[2], 64) // 64
        if name == "glsdet_last_error":
            return b"scripted refusal"
        if name.endswith("_tune"):
            assert self.tunes, "%s: a tune call the scenario did not script" % name
            rc, best, us = self.tunes.pop(0)
            o[-2].value, o[-1].value = best, us
            rec["ret"] = rc
            return rc
        first = o[0][0] if isinstance(o[0], C.Array) else o[0]
        hint = {"glsdet_bottleneck": lambda: o[2], "glsdet_csp_fused": lambda: o[1]}.get(name, lambda: first.tile_hint)()
        rc = -1 if name in self.refuse_names or hint in self.refuse_hints else 0
        rec["ret"] = rc
        if rc == 0:
            val, nan = 1.0 + 0.125 * (hint & 7), hint in self.nan_hints
            if name == "glsdet_conv2d_multi":
                for d in list(o[0])[:o[1]]:
                    self.fill(d.y, val, nan)
            elif name == "glsdet_conv2d_chain":
                if not o[1].flags & 1:
                    self.fill(first.y, val, False)
                self.fill(o[1].y2, val + 2, nan)
            elif name == "glsdet_bottleneck":
                self.fill(o[1].y, val + 4, nan)
            elif name == "glsdet_csp_fused":
                self.fill(first.y, val + 6, nan)
            else:
                self.fill(first.y, val, nan)
        return rc


def _norm(v):
    """JSON-stable: NaN as a string (NaN != NaN), tuples as lists"""
    if isinstance(v, float) and math.isnan(v):
        return "nan"
    if isinstance(v, (list, tuple)):
        return [_norm(x) for x in v]
    if isinstance(v, dict):
        return {k: _norm(x) for k, x in v.items()}
    return v


class Harness:
    def __init__(self, mp, autotune=True, dtype="f16", tunes=(), env=None):
        for k in SWITCHES:
            mp.delenv(k, raising=False)
        for k, v in (env or {}).items():
            mp.setenv(k, v)
        self.lib = FakeLib()
        self.lib.tunes = list(tunes)
        mp.setattr(_lib, "load", lambda: self.lib)
        mp.setattr(torch.cuda, "is_available", lambda: True)
        mp.setattr(engine, "_stream_ptr", lambda stream=None: 0)
        mp.setattr(engine, "_SHARED_TUNED", {})
        self.eng = Engine(dtype, device="cpu", autotune=autotune)
        self.lib.eng = self.eng

    def note(self, what, value=None):
        self.lib.calls.append({"note": what, "value": _norm(value)})

    def name(self, nm, t):
        self.lib.named.append((nm, t))
        return t

    def t(self, nm, n, h, w, c, dtype=None):
        v = self.eng.tensor(n, h, w, c, dtype)
        self.name(nm, v.buf)
        return v

    def pack(self, nm, cout, cin, R, S=None):
        pk = self.eng.pack_conv([(torch.zeros(cout, cin, R, S or R), torch.ones(cout), torch.zeros(cout))], ceil_to(cin, 8))
        for q, t in zip(("w", "scale", "bias"), pk[:3]):
            self.name(nm + "." + q, t)
        return pk

    def raises(self, what, fn):
        try:
            fn()
            self.note(what, "returned")
        except _lib.GlsdetError as e:
            self.note(what, "GlsdetError: " + str(e))

    def result(self):
        e = self.eng
        assert not self.lib.tunes, "scripted tune answers nobody asked for: %r" % (self.lib.tunes,)
        return {"calls": self.lib.calls,
                # repr: True is not 1 and 1.0 is not 1 in a key, though they compare (and hash) equal
                "tuned": sorted([repr(k), v] for k, v in e._tuned.items()),
                "dirty": getattr(e, "_tune_dirty", False),
                "shadow_log": None if e.shadow is None else [_norm(dict(r, shape=repr(r["shape"]))) for r in e.shadow["log"]]}


def geo(v):
    return (v.n, v.h, v.w, v.c, v.sn, v.sh, v.sw)


# ---------------------------------------------------------------------------------------------- scenarios
# One tiny geometry: 1 x 6 x 11, 64 / 32 channels.  The x of most scenarios is the left window of a wider tensor, so that
# sizes and strides differ in every key.
N, H_, W_ = 1, 6, 11
SCENARIOS = {}


def scenario(**kw):
    def deco(fn, kw=kw):
        SCENARIOS[kw.pop("name", fn.__name__)] = (fn, kw)
        return fn
    return deco


def _x(h, c=64, nm="x"):
    return h.t(nm, N, H_, W_ + 2, c).window(0, H_, 0, W_)


@scenario(tunes=[(0, 5, 10.0), (0, 6, 11.0), (0, 2, 12.0), (0, 4, 9.0)])
def conv(h):
    x, pk, res = _x(h), h.pack("w", 32, 64, 3), h.t("res", N, H_, W_, 32)
    y = h.eng.conv(x, pk, 1, 1, "silu")
    h.note("out", geo(y))
    h.eng.conv(x, pk, 1, 1, "silu", out=y)                                        # second call: no tune
    h.eng.conv(x, pk, 1, 1, "relu", out=y, res=res)                               # residual: a key of its own
    h.eng.conv(x, pk, 1, 1, "relu", out=y, res=res, res_first=True)               # same key, other act flag
    h.eng.conv(x, pk, 1, 1, "relu", out=y, res_first=True)                        # res_first without res: no flag
    h.eng.conv(x, pk, 1, 1, "none", out=y, tile_hint=7)                           # caller's hint: no tune
    y2 = h.eng.conv(x, pk, 2, 1, "lrelu", out_dtype=F32)                          # stride 2, fp32 output
    h.note("out2", geo(y2) + (y2.dtype,))
    h.eng.conv(x.channels(8, 40), h.pack("w1", 40, 32, 1), 1, 0, "gelu")         # channel window, 1x1, cout 40


@scenario(tunes=[(-3, 0, 0.0)])
def conv_tune_refused(h):
    x, pk = _x(h), h.pack("w", 32, 64, 3)
    h.raises("conv", lambda: h.eng.conv(x, pk, 1, 1, "silu"))


@scenario()
def conv_launch_refused(h):
    x, pk = _x(h), h.pack("w", 32, 64, 3)
    h.lib.refuse_names.add("glsdet_conv2d")
    h.eng.autotune = False
    h.raises("conv", lambda: h.eng.conv(x, pk, 1, 1, "silu"))


def _chain(h, skip_y=False, with_res=False, twice=True):
    x, pk, pk2 = _x(h), h.pack("w", 64, 64, 3), h.pack("w2", 40, 32, 1)
    out, out2 = h.t("y", N, H_, W_, 64), h.t("cat", N, H_, W_, 96).channels(8, 48)
    res = h.t("res", N, H_, W_, 64) if with_res else None
    for i in range(2 if twice else 1):
        h.note("conv_chain", h.eng.conv_chain(x, pk, 1, 1, "silu", out, res, pk2, "relu", 32, 32, out2, res_first=with_res, skip_y=skip_y))


CHAIN_TUNES = {"below": [(0, 5, 50.0), (0, 2, 40.0), (0, 3, 60.0)], "above": [(0, 5, 120.0), (0, 2, 40.0), (0, 3, 60.0)],
               "equal": [(0, 5, 97.0), (0, 2, 40.0), (0, 3, 60.0)], "just_above": [(0, 5, 97.5), (0, 2, 40.0), (0, 3, 60.0)],
               "fused_refused": [(-1, 5, 1.0)], "first_part_refused": [(0, 5, 500.0), (-1, 0, 0.0)],
               "second_part_refused": [(0, 5, 500.0), (0, 2, 40.0), (-1, 0, 0.0)], "hint_zero": [(0, 0, 50.0), (0, 2, 40.0), (0, 3, 60.0)]}
for _k, _t in CHAIN_TUNES.items():
    scenario(name="chain/" + _k, tunes=_t)(_chain)
scenario(name="chain/skip_y_below", tunes=CHAIN_TUNES["below"])(lambda h: _chain(h, skip_y=True))
scenario(name="chain/res_first_above", tunes=CHAIN_TUNES["above"])(lambda h: _chain(h, with_res=True))
scenario(name="chain/credit", tunes=[(0, 5, 100.0), (0, 2, 40.0), (0, 3, 60.0)], env={"GLSDET_FUSE_CREDIT_US": "3.5"})(_chain)
scenario(name="chain/credit_short", tunes=[(0, 5, 100.0), (0, 2, 40.0), (0, 3, 60.0)], env={"GLSDET_FUSE_CREDIT_US": "2.5"})(_chain)
scenario(name="chain/force_bneck_is_not_read", tunes=CHAIN_TUNES["above"], env={"GLSDET_FORCE_BNECK": "1"})(_chain)


@scenario(name="chain/launch_refused", autotune=False)
def _chain_launch_refused(h):
    h.lib.refuse_names.add("glsdet_conv2d_chain")
    _chain(h, twice=False)


def _bneck(h, with_res=True, cm=32):
    x = _x(h)
    pk1, pk2 = h.pack("w1", cm, 64, 1), h.pack("w2", cm, cm, 3)
    out, hid = h.t("y", N, H_, W_ + 1, cm).window(0, H_, 1, W_ + 1), h.t("hid", N, H_, W_, cm)
    res = h.t("res", N, H_, W_, cm) if with_res else None
    for i in range(2):
        h.note("bottleneck", h.eng.bottleneck(x, pk1, "silu", pk2, "silu", out, res, hid))


BNECK_TUNES = {"below": [(0, 5, 50.0), (0, 2, 40.0), (0, 3, 60.0)], "above": [(0, 5, 120.0), (0, 2, 40.0), (0, 3, 60.0)],
               "equal": [(0, 5, 97.0), (0, 2, 40.0), (0, 3, 60.0)], "fused_refused": [(-1, 5, 1.0)],
               "first_part_refused": [(0, 5, 500.0), (-1, 0, 0.0)], "second_part_refused": [(0, 5, 500.0), (0, 2, 40.0), (-1, 0, 0.0)],
               "hint_zero": [(0, 0, 50.0), (0, 2, 40.0), (0, 3, 60.0)]}
for _k, _t in BNECK_TUNES.items():
    scenario(name="bneck/" + _k, tunes=_t)(_bneck)
scenario(name="bneck/no_res_above", tunes=BNECK_TUNES["above"])(lambda h: _bneck(h, with_res=False))
scenario(name="bneck/force_bneck", tunes=BNECK_TUNES["above"], env={"GLSDET_FORCE_BNECK": "1"})(_bneck)
scenario(name="bneck/credit", tunes=[(0, 5, 100.0), (0, 2, 40.0), (0, 3, 60.0)], env={"GLSDET_FUSE_CREDIT_US": "3.5"})(_bneck)
scenario(name="bneck/not_applicable")(lambda h: _bneck(h, cm=40))


def _csp_packs(h):
    return [h.pack("w12", 64, 64, 1), h.pack("wm1", 32, 32, 1), h.pack("wm2", 32, 32, 3), h.pack("w3", 64, 64, 1)]


def _csp(h, shortcut=True):
    x, out = _x(h), h.t("cat", N, H_, W_, 128).channels(64, 128)
    packs = _csp_packs(h)
    for i in range(2):
        h.note("csp_fused_wins", h.eng.csp_fused_wins(geo(x), geo(out), packs, shortcut))
    h.note("csp_fused", h.eng.csp_fused(x, packs, shortcut, out))
    # what the layer's key would be for views the tuner never saw
    h.note("csp_fused other geometry", h.eng.csp_fused(h.t("x2", N, H_, W_, 64), packs, shortcut, out))


_SEP4 = [(0, 1, 20.0), (0, 2, 30.0), (0, 3, 40.0), (0, 4, 10.0)]
CSP_TUNES = {"below": [(0, 5, 50.0)] + _SEP4, "above": [(0, 5, 120.0)] + _SEP4, "equal": [(0, 5, 97.0)] + _SEP4,
             "fused_refused": [(-1, 5, 1.0)], "part_refused": [(0, 5, 500.0)] + _SEP4[:2] + [(-1, 0, 0.0)] + _SEP4[3:],
             "hint_zero": [(0, 0, 50.0)] + _SEP4}
for _k, _t in CSP_TUNES.items():
    scenario(name="csp/" + _k, tunes=_t)(_csp)
scenario(name="csp/no_shortcut_above", tunes=CSP_TUNES["above"])(lambda h: _csp(h, shortcut=False))
scenario(name="csp/credit", tunes=[(0, 5, 100.0)] + _SEP4, env={"GLSDET_FUSE_CREDIT_US": "3.5"})(_csp)
scenario(name="csp/force_bneck_is_not_read", tunes=CSP_TUNES["above"], env={"GLSDET_FORCE_BNECK": "1"})(_csp)


@scenario(name="csp/not_eligible")
def _csp_not_eligible(h):
    x, out, packs = _x(h), h.t("y", N, H_, W_, 64), _csp_packs(h)
    h.note("c 32", h.eng.csp_fused_wins(geo(x.channels(0, 32)), geo(out), packs, True))
    h.note("sizes", h.eng.csp_fused_wins(geo(x.window(0, 5, 0, W_)), geo(out), packs, True))
    h.note("packs", h.eng.csp_fused_wins(geo(x), geo(out), packs[::-1], True))
    h.lib.refuse_names.add("glsdet_csp_fused")
    h.note("launch refused", h.eng.csp_fused(x, packs, True, out))


def _group(h, n=3, with_res=False, outs=True):
    xs = [_x(h, nm="x%d" % i) for i in range(n)]
    pks = [h.pack("w%d" % i, 32, 64, 3) for i in range(n)]
    ys = [h.t("y%d" % i, N, H_, W_, 32) for i in range(n)] if outs else None
    ress = [h.t("r%d" % i, N, H_, W_, 32) if i != 1 else None for i in range(n)] if with_res else None
    for i in range(2):
        h.raises("conv_group", lambda: h.note("outs", [geo(y) for y in h.eng.conv_group(xs, pks, 1, 1, "relu", outs=ys, ress=ress)]))


_ONE3 = [(0, 1, 30.0), (0, 2, 30.0), (0, 3, 40.0)]
# (the problems of a group share one plain-conv key here: the separate form tunes once)
GROUP_TUNES = {"below": _ONE3 + [(0, 9, 90.0)], "above": _ONE3 + [(0, 9, 96.0)] + _ONE3[:1], "equal": _ONE3 + [(0, 9, 95.0)] + _ONE3[:1],
               "single_refused": 2 * (_ONE3[:1] + [(-2, 0, 0.0)]), "multi_refused": 2 * (_ONE3 + [(-2, 0, 0.0)]),
               "hint_zero": _ONE3 + [(0, 0, 50.0)]}
for _k, _t in GROUP_TUNES.items():
    scenario(name="group/" + _k, tunes=_t)(_group)
scenario(name="group/res_below", tunes=GROUP_TUNES["below"])(lambda h: _group(h, with_res=True))
scenario(name="group/allocates_outs", tunes=GROUP_TUNES["below"])(lambda h: _group(h, outs=False))
scenario(name="group/credit", tunes=_ONE3 + [(0, 9, 99.0)], env={"GLSDET_FUSE_CREDIT_US": "2.5"})(_group)
scenario(name="group/credit_short", tunes=_ONE3 + [(0, 9, 100.5)] + _ONE3[:1], env={"GLSDET_FUSE_CREDIT_US": "2.5"})(_group)
scenario(name="group/one", tunes=_ONE3[:1])(lambda h: _group(h, n=1))
scenario(name="group/five", tunes=_ONE3[:1])(lambda h: _group(h, n=5))
scenario(name="group/no_group", tunes=_ONE3[:1], env={"GLSDET_NO_GROUP": "1"})(_group)
scenario(name="group/autotune_off", autotune=False)(_group)


def _many(h, with_res=False, n=12, odd=False):
    xs = [h.t("x%d" % i, N, H_, W_, 64) for i in range(n)]
    pks = [h.pack("w%d" % i, 40, 64, 1) for i in range(n)]
    ys = [h.t("y%d" % i, N, H_, W_ + (1 if odd and i == 10 else 0), 40).window(0, H_, 0, W_) for i in range(n)]
    ress = [h.t("r%d" % i, N, H_, W_, 40) for i in range(n)] if with_res else None
    for i in range(2):
        h.raises("conv_many", lambda: h.eng.conv_many(xs, pks, 1, 0, "none", ys, ress=ress))


scenario(name="many/plain", tunes=[(0, 9, 20.0)])(_many)
scenario(name="many/res", tunes=[(0, 9, 20.0)])(lambda h: _many(h, with_res=True))
scenario(name="many/40", tunes=[(0, 9, 20.0)])(lambda h: _many(h, n=40))           # 32 + 8: one tuned launch, one plain
scenario(name="many/44", tunes=[(0, 9, 20.0), (0, 8, 20.0)])(lambda h: _many(h, n=44))      # 32 + 12: two keys
scenario(name="many/unequal")(lambda h: _many(h, odd=True))
scenario(name="many/no_batch", env={"GLSDET_NO_BATCH": "1"})(_many)
scenario(name="many/tune_refused", tunes=[(-2, 0, 0.0), (-2, 0, 0.0)])(_many)
scenario(name="many/autotune_off", autotune=False)(_many)


def _gnstats(h, pad=1):
    x, pk = _x(h), h.pack("w", 64, 64, 3)
    y = h.t("y", N, H_ + 2 * pad - 2, W_ + 2 * pad - 2, 64)
    for i in range(2):
        o, stats = h.eng.conv_gnstats(x, pk, pad, 8, out=y)
        h.note("conv_gnstats", [geo(o), None if stats is None else h.lib.addr(stats.data_ptr())])


_GN = {"GLSDET_GN_FUSION": "1"}
# the statistics pass the fused form saves is credited 1 * 6 * 11 * 64 * 2 / 4e6 = 0.002 us here: no fp32 timing sits exactly
# on the threshold, so "equal" is the plain conv's own time and "just_above" the next step up
scenario(name="gnstats/below", tunes=[(0, 9, 50.0), (0, 2, 60.0)], env=_GN)(_gnstats)
scenario(name="gnstats/above", tunes=[(0, 9, 61.0), (0, 2, 60.0), (0, 2, 60.0)], env=_GN)(_gnstats)
scenario(name="gnstats/equal", tunes=[(0, 9, 60.0), (0, 2, 60.0)], env=_GN)(_gnstats)
scenario(name="gnstats/just_above", tunes=[(0, 9, 60.01), (0, 2, 60.0), (0, 2, 60.0)], env=_GN)(_gnstats)
scenario(name="gnstats/fused_refused", tunes=[(-1, 9, 1.0), (0, 2, 60.0)], env=_GN)(_gnstats)
scenario(name="gnstats/plain_refused", tunes=[(0, 9, 500.0), (-1, 0, 0.0)], env=_GN)(_gnstats)
scenario(name="gnstats/autotune_off", autotune=False, env=_GN)(_gnstats)
scenario(name="gnstats/switch_off", tunes=[(0, 2, 60.0)])(_gnstats)
scenario(name="gnstats/pad0", tunes=[(0, 2, 60.0)], env=_GN)(lambda h: _gnstats(h, pad=0))


@scenario(name="gnstats/launch_refused", autotune=False, env=_GN)
def _gnstats_launch_refused(h):
    h.lib.refuse_names.add("glsdet_conv2d_gnstats")
    _gnstats(h)


def _forced(h):
    x, pk = _x(h), h.pack("w", 32, 64, 3)
    y = h.eng.conv(x, pk, 1, 1, "silu")
    h.eng.conv(x, pk, 1, 1, "silu", out=y, tile_hint=7)              # a caller's hint is not overridden
    xs, pks = [x, _x(h, nm="xb")], [pk, h.pack("wb", 32, 64, 3)]
    h.eng.conv_multi(xs, pks, 1, 1, "silu")
    h.eng.conv_multi(xs, pks, 1, 1, "silu", tile_hint=6)


_FORCE = {"GLSDET_FORCE_HINT": "0x21", "GLSDET_FORCE_MULTI_HINT": "34"}
scenario(name="forced/taken", tunes=[(0, 5, 10.0)], env=_FORCE)(_forced)


@scenario(name="forced/refused_falls_back", tunes=[(0, 5, 10.0)], env=_FORCE)
def _forced_refused(h):
    h.lib.refuse_hints.update((0x21, 34))
    _forced(h)


def _shadow(h):
    e = h.eng
    e.shadow = {"hint": 3, "multi": 4, "log": []}
    x, pk, pkb = _x(h), h.pack("w", 64, 64, 3), h.pack("wb", 64, 64, 3)
    y = e.conv(x, pk, 1, 1, "silu")
    e.conv(x, pk, 1, 1, "silu", out=y, tile_hint=7)                   # not shadowed
    e.conv_multi([x, _x(h, nm="xb")], [pk, pkb], 1, 1, "silu")
    pk2 = h.pack("w2", 40, 32, 1)
    out2 = h.t("cat", N, H_, W_, 96).channels(8, 48)
    for skip_y in (False, True):
        h.note("conv_chain", e.conv_chain(x, pk, 1, 1, "silu", y, None, pk2, "relu", 32, 32, out2, skip_y=skip_y))
    pk1 = h.pack("w1", 64, 64, 1)
    h.note("bottleneck", e.bottleneck(x, pk1, "silu", pk, "silu", y, h.t("res", N, H_, W_, 64), h.t("hid", N, H_, W_, 64)))
    h.note("csp_fused", e.csp_fused(x, _csp_packs(h), True, y))


# conv (one key, then the chain's two-part comparison reuses nothing: chain, bneck tune on their own)
_SHADOW_TUNES = [(0, 5, 10.0), (0, 5, 50.0), (0, 2, 40.0), (0, 3, 60.0), (0, 5, 50.0), (0, 2, 40.0), (0, 3, 60.0),
                 (0, 5, 50.0), (0, 2, 40.0), (0, 3, 60.0)]
scenario(name="shadow/all", tunes=_SHADOW_TUNES)(_shadow)
scenario(name="shadow/autotune_off", autotune=False)(_shadow)


@scenario(name="shadow/nan_in_variant", tunes=_SHADOW_TUNES)
def _shadow_nan_variant(h):
    h.lib.nan_hints.update((3, 4))            # the variants under test: _shadow_end reports them, the fused checks do not see them
    _shadow(h)


@scenario(name="shadow/nan_in_real_output", tunes=_SHADOW_TUNES)
def _shadow_nan_real(h):
    h.lib.nan_hints.add(5)                    # the tuned launches: only the fused checks report a NaN of the real output
    _shadow(h)


@scenario(name="shadow/variant_declines", tunes=_SHADOW_TUNES)
def _shadow_declines(h):
    h.lib.refuse_hints.update((3, 4))
    _shadow(h)


@scenario(tunes=[(0, 5, 10.0)])
def as_weight(h):
    e = h.eng
    m = e.matrix(20, 64)
    h.name("m", m.buf)
    bias = h.name("host_bias", torch.arange(20, dtype=torch.float32))
    bdev = e.bias_vector(20)
    h.name("bdev", bdev.buf)
    plain, with_bias, with_bias2, with_dev, plain2 = (e.as_weight(m, 0.5), e.as_weight(m, 0.5, bias=bias), e.as_weight(m, 0.5, bias=bias),
                                                      e.as_weight(m, 0.5, bias_dev=bdev), e.as_weight(m, 0.5))
    other = e.as_weight(m, 0.25, bias_dev=bdev)
    for nm, pk in (("plain", plain), ("bias", with_bias), ("bias again", with_bias2), ("bias_dev", with_dev), ("plain again", plain2),
                   ("other alpha", other)):
        h.note(nm, [h.lib.addr(p.data_ptr()) for p in pk[:3]] + list(pk[3:]))
    h.note("same scale vector", [pk[1] is plain[1] for pk in (with_bias, with_bias2, with_dev, plain2, other)])
    h.note("same zero vector", plain[2] is plain2[2])
    h.note("same bias vector", with_bias[2] is with_bias2[2])
    h.note("cached vectors", sorted(repr(k[:2]) for k in e._vecs))
    h.note("scale values", [float(plain[1][0]), float(other[1][0]), float(with_bias[2][3]), float(plain[2].abs().max())])
    e.conv(_x(h), with_dev, 1, 0, "none")


@scenario()
def dwconv(h):
    x = _x(h)
    pk = h.eng.pack_dw(torch.zeros(64, 1, 3, 3), torch.ones(64), torch.zeros(64), 64)
    for q, t in zip(("w", "scale", "bias"), pk[:3]):
        h.name("dw." + q, t)
    h.note("out", geo(h.eng.dwconv(x, pk, 1, 1, "relu")))
    h.note("out dilated", geo(h.eng.dwconv(x, pk, 2, 2, "none", dilation=2)))


@scenario(name="autotune_off", autotune=False)
def _autotune_off(h):
    _chain(h)
    _bneck(h)
    _csp(h)


def record():
    out = {}
    for name, (fn, kw) in SCENARIOS.items():
        with pytest.MonkeyPatch.context() as mp:
            h = Harness(mp, **kw)
            fn(h)
            out[name] = h.result()
    return json.loads(json.dumps(out))


# ---------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def traces():
    return record()


def _golden(cache=[]):
    if not cache:
        with open(GOLDEN) as f:
            cache.append(json.load(f))
    return cache[0]


def test_the_golden_covers_every_scenario_and_no_other():
    assert sorted(_golden()) == sorted(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_trace_equals_the_recorded_one(traces, name):
    got, want = traces[name], _golden()[name]
    for i, (g, w) in enumerate(zip(got["calls"], want["calls"])):
        assert g == w, "%s: call %d differs" % (name, i)
    assert len(got["calls"]) == len(want["calls"])
    assert got["tuned"] == want["tuned"]
    assert got["shadow_log"] == want["shadow_log"]
    assert got["dirty"] == want["dirty"]


def test_the_scenarios_decide_both_ways():
    """the scripted timings straddle the thresholds: each fused form is kept in one scenario and dropped in another (a golden
    recorded from timings that all fall on one side would pin nothing)"""
    def verdict(name, kind):
        vs = [v for k, v in _golden()[name]["tuned"] if k.startswith("('%s'" % kind)]
        assert len(vs) == 1, (name, vs)
        return vs[0]
    for form, kind in (("chain", "chain"), ("bneck", "bneck"), ("csp", "csp1"), ("group", "multi"), ("gnstats", "gnstats")):
        assert verdict(form + "/below", kind) >= 0 and verdict(form + "/above", kind) == -1
    for form, kind in (("chain", "chain"), ("bneck", "bneck"), ("csp", "csp1"), ("gnstats", "gnstats")):
        assert verdict(form + "/fused_refused", kind) == -1
    assert verdict("chain/credit", "chain") >= 0 and verdict("chain/credit_short", "chain") == -1
    assert verdict("group/credit", "multi") >= 0 and verdict("group/credit_short", "multi") == -1
    assert verdict("bneck/force_bneck", "bneck") >= 0 and verdict("chain/force_bneck_is_not_read", "chain") == -1
    for name, kind in (("chain/first_part_refused", "chain"), ("bneck/second_part_refused", "bneck"), ("csp/part_refused", "csp1"),
                       ("gnstats/plain_refused", "gnstats")):
        assert verdict(name, kind) >= 0


def test_tune_dirty_follows_misses_and_saves(tmp_path):
    path = tmp_path / "tune.json"
    with pytest.MonkeyPatch.context() as mp:
        h = Harness(mp, tunes=[(0, 5, 10.0), (0, 5, 50.0), (0, 2, 40.0), (0, 3, 60.0)], env={"GLSDET_TUNE_CACHE": str(path)})
        e = h.eng
        assert e._tune_dirty is False
        e.save_tune_cache()
        assert not path.exists()                            # nothing measured: nothing written
        x, pk = _x(h), h.pack("w", 32, 64, 3)
        y = e.conv(x, pk, 1, 1, "silu")
        assert e._tune_dirty is True
        e.save_tune_cache()
        assert e._tune_dirty is False and path.exists()
        e.conv(x, pk, 1, 1, "silu", out=y)                  # a hit
        assert e._tune_dirty is False
        _chain(h)
        assert e._tune_dirty is True
        e.save_tune_cache()
        assert e._tune_dirty is False
        with open(path) as f:
            assert {tuple(json.loads(k)): v for k, v in json.load(f)["f16"].items()} == dict(e._tuned) and len(e._tuned) == 2
        # a second engine starts from the file and measures nothing
        h2 = Harness(mp, env={"GLSDET_TUNE_CACHE": str(path)})
        assert dict(h2.eng._tuned) == dict(e._tuned) and h2.eng._tune_dirty is False
        h2.eng.conv(_x(h2), h2.pack("w", 32, 64, 3), 1, 1, "silu")
        assert h2.eng._tune_dirty is False


def _view(g, dtype, c=None):
    n, h, w, cc, sn, sh, sw = g
    return TView(torch.zeros(16, dtype=torch.uint8), 0, n, h, w, cc if c is None else c, sn, sh, sw, dtype)


def _pk(cout, R, S):
    p = engine._Ptr(0)
    return (p, p, p, cout, R, S)


@pytest.mark.parametrize("dtype", ["f16", "f32"])
def test_every_key_of_the_committed_cache_is_asked_for_again(dtype):
    """bench_tuning.json, entry by entry: the Engine call each key came from, rebuilt from the key alone, must find it --
    no tune call, no new entry.  (A key that came out differently would be measured again, silently.)"""
    with open(os.path.join(ROOT, "bench_tuning.json")) as f:
        table = {tuple(json.loads(k)): v for k, v in json.load(f)[dtype].items()}
    with pytest.MonkeyPatch.context() as mp:
        h = Harness(mp, dtype=dtype)
        e, dt = h.eng, h.eng.dt
        e._tuned.update(table)
        kinds = set()
        for key in table:
            kind = key[0] if isinstance(key[0], str) else "plain"
            kinds.add(kind)
            h.lib.calls.clear()
            if kind == "plain":
                R, S, stride, pad, has_res, odt = key[11:]
                oh, ow = (key[1] + 2 * pad - R) // stride + 1, (key[2] + 2 * pad - S) // stride + 1
                out = _view((key[0], oh, ow) + key[7:11], odt)
                e.conv(_view(key[:7], dt), _pk(key[7], R, S), stride, pad, "silu", out=out, res=out if has_res else None)
            elif kind == "chain":
                R, S, stride, pad, has_res, odt, c0, cin2 = key[12:20]
                oh, ow = (key[2] + 2 * pad - R) // stride + 1, (key[3] + 2 * pad - S) // stride + 1
                out, out2 = _view((key[1], oh, ow) + key[8:12], odt), _view((key[1], oh, ow) + key[20:24], odt)
                e.conv_chain(_view(key[1:8], dt), _pk(key[8], R, S), stride, pad, "silu", out, out if has_res else None,
                             _pk(key[20], 1, 1), "silu", c0, cin2, out2, skip_y=key[24])
            elif kind == "bneck":
                cm, has_res, odt = key[8], key[12], key[13]
                out = _view(key[1:4] + (cm,) + key[9:12], odt)
                hid = _view(key[1:4] + (cm,) + key[9:12], odt)
                x = _view(key[1:8], odt)
                assert e.bottleneck(x, _pk(cm, 1, 1), "silu", _pk(cm, 3, 3), "silu", out, out if has_res else None, hid) == (table[key] >= 0)
            elif kind == "multi":
                n, stride, pad, R, S = key[1:6]
                per = [key[6 + 13 * i: 19 + 13 * i] for i in range(n)]
                assert len(key) == 6 + 13 * n
                xs = [_view(p[:7], dt) for p in per]
                outs = [_view((p[0], (p[1] + 2 * pad - R) // stride + 1, (p[2] + 2 * pad - S) // stride + 1) + p[7:11], p[12]) for p in per]
                e.conv_group(xs, [_pk(p[7], R, S) for p in per], stride, pad, "silu", outs=outs,
                             ress=[o if p[11] else None for o, p in zip(outs, per)])
            elif kind == "batch":
                k, act = key[1], key[2]
                g = key[3:]
                xs = [_view(g[:7], g[7]) for _ in range(k)]
                outs = [_view(g[11:18], g[18]) for _ in range(k)]
                ress = None if g[19] == -1 else [_view(g[11:14] + (g[22],) + g[19:22], g[18]) for _ in range(k)]
                e.conv_many(xs, [_pk(g[8], g[9], g[10]) for _ in range(k)], 1, 0, act, outs, ress=ress)
            else:
                raise AssertionError("a key form this test does not know: %r" % (key,))
            assert not [c for c in h.lib.calls if c.get("fn", "").endswith("_tune")], key
            assert dict(e._tuned) == table, key
        assert getattr(e, "_tune_dirty", False) is False
        assert kinds >= {"plain", "chain", "bneck", "multi"}


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        with open(GOLDEN, "w") as f:
            f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in record().items()) + "\n}\n")
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
