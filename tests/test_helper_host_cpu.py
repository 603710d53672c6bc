"""CPU-only: the host contract of the 16-byte-per-lane helper entry points (csrc/misc.hip, adapt.hip, resdet.hip, evc.hip,
swin.hip, dwconv.hip, stem.hip) and the "y overlaps x" rule of conv2d_grouped / bottleneck / csp_fused, through the built
library with fabricated views whose pointers are never dereferenced.

One call table (run_table below) is run with every call made between glsdet_plan_begin and glsdet_plan_end, so that nothing is
launched: an accepted call must record exactly one op with its (kind, flops, bytes, name), a refused one must return its
code, leave its full glsdet_last_error() text and record nothing; where a call has two faults the one checked first wins.

Every expected value is read from tests/golden/helper_host_contract.json, which tools/make_helper_host_golden.py recorded
by running this same table against the library of the commit before these entry points shared their host front (fa89b3a,
selected with GLSDET_LIB_PATH); none is derived from the code under test."""
import ctypes as C
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "helper_host_contract.json")
ARG, BOUNDS, ALIGN = -1, -2, -3
P = 0x10000000                  # fabricated pointers: P + k * 1 MiB, 16-byte (and 256-byte) aligned


def _lib():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


def V(n, h, w, c, dt, slot, ct=0, off=0):
    """a dense NHWC view (pixel stride ct or c) `off` elements into slot `slot`; its allocation ends 64 bytes after it"""
    from glsdet_amd import _lib
    es = 2 if dt == 0 else 4
    ct = ct or c
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = P + (slot << 20) + off * es, n, h, w, c, dt
    v.sw, v.sh, v.sn = ct, w * ct, h * w * ct
    v.alloc_lo = P + (slot << 20)
    v.alloc_hi = v.base + ((n - 1) * v.sn + (h - 1) * v.sh + (w - 1) * v.sw + c) * es + 64
    return v


def _outside(v):
    v.alloc_hi -= 66            # two bytes short of the view's last element


def _arr(vs):
    from glsdet_amd import _lib
    return None if vs is None else (_lib.View * len(vs))(*vs)


def _ptrs(ps):
    return None if ps is None else (C.c_void_p * len(ps))(*ps)


def _desc(x, y, R, S, stride, pad, act=1, hint=0):
    from glsdet_amd import _lib
    d = _lib.ConvDesc()
    d.x, d.y, d.R, d.S, d.stride, d.pad, d.act, d.tile_hint = x, y, R, S, stride, pad, act, hint
    d.w, d.scale, d.bias = P + (40 << 20), P + (41 << 20), P + (42 << 20)
    return d


class Entry:
    """args(dt) -> the dict of an accepted call; call(lib, a) makes it; views: the view operands in the order the entry point
    checks them, as (key, need16) -- a key may name a list of views, whose last one is then the one mutated; ptrs: the other
    pointer operands; faults: {label: mutation of the dict}"""

    def __init__(self, name, args, call, views, ptrs=(), faults=None, dtypes=(0, 1)):
        self.name, self.args, self.call, self.views, self.ptrs, self.faults, self.dtypes = name, args, call, views, ptrs, faults or {}, dtypes

    def view(self, a, key):
        if "." in key:                                  # a member of a descriptor
            d, m = key.split(".")
            return getattr(a[d], m)
        return a[key][-1] if isinstance(a[key], list) else a[key]

    def cases(self):
        """{label: mutation}: the accepted call, the generic faults of every operand, the entry point's own, and one call with
        two faults (the first two operands both outside their allocation, or a null pointer and the view outside)"""
        out = {"accepted": lambda a: None}
        for key in [k for k, _ in self.views if "." not in k] + list(self.ptrs):
            out["null " + key] = lambda a, key=key: a.__setitem__(key, None)
        for key, need16 in self.views:
            out["%s outside its allocation" % key] = lambda a, key=key: _outside(self.view(a, key))
            out["%s base 8 bytes off%s" % (key, "" if need16 else " (no 16-byte need)")] = \
                lambda a, key=key: setattr(self.view(a, key), "base", self.view(a, key).base + 8)
            if need16:
                out["%s with its pixel stride one element off" % key] = lambda a, key=key: setattr(self.view(a, key), "sw", self.view(a, key).sw + 1)
                out["%s with its row stride one element off" % key] = lambda a, key=key: setattr(self.view(a, key), "sh", self.view(a, key).sh + 1)
            out["%s of dtype 7" % key] = lambda a, key=key: setattr(self.view(a, key), "dtype", 7)
            out["%s with no rows" % key] = lambda a, key=key: setattr(self.view(a, key), "h", 0)
        out.update(self.faults)
        if len(self.views) > 1:
            (k0, _), (k1, _) = self.views[:2]
            out["two faults: %s and %s outside their allocations" % (k0, k1)] = \
                lambda a: (_outside(self.view(a, k1)), _outside(self.view(a, k0)))
        elif self.ptrs and self.views:
            k0, p0 = self.views[0][0], self.ptrs[0]
            out["two faults: null %s and %s outside its allocation" % (p0, k0)] = \
                lambda a: (_outside(self.view(a, k0)), a.__setitem__(p0, None))
        return out


def S(key, value):
    return lambda a: a.__setitem__(key, value)


def R(key, *view_args, **kw):
    """replace the view a[key] (the last one of a list) by V(*view_args, dtype of the call, ...)"""
    def f(a):
        v = V(*view_args[:4], kw.get("dt", a["dt"]) if kw.get("dt") != "other" else 1 - a["dt"], view_args[4], ct=kw.get("ct", 0),
              off=kw.get("off", 0))
        if isinstance(a[key], list):
            a[key][-1] = v
        else:
            a[key] = v
    return f


def both(*fs):
    return lambda a: [f(a) for f in fs]


def _entries(lib):
    E = []
    img, w, sc, bi = P + (30 << 20), P + (40 << 20), P + (41 << 20), P + (42 << 20)

    # ---- misc.hip
    E.append(Entry("focus_pack", lambda dt: dict(img=img, n=2, cin=3, H=8, W=12, y=V(2, 4, 6, 16, dt, 1)),
                   lambda a: lib.glsdet_focus_pack(a["img"], a["n"], a["cin"], a["H"], a["W"], a["y"], None), [("y", True)], ["img"],
                   {"H odd": S("H", 7), "W odd": S("W", 11), "n 0": S("n", 0), "cin 0": S("cin", 0), "y.h 5": R("y", 2, 5, 6, 16, 1),
                    "y.c 8 < 4 cin": R("y", 2, 4, 6, 8, 1), "cin 4, y.c 16 (generic path)": S("cin", 4),
                    "two faults: H odd and y.h 5": both(S("H", 7), R("y", 2, 5, 6, 16, 1))}))
    E.append(Entry("maxpool2d", lambda dt: dict(x=V(2, 5, 7, 16, dt, 0), y=V(2, 5, 7, 16, dt, 1), k=5),
                   lambda a: lib.glsdet_maxpool2d(a["x"], a["y"], a["k"], None), [("x", True), ("y", True)], (),
                   {"k 4": S("k", 4), "k 0": S("k", 0), "k 33": S("k", 33), "k -1": S("k", -1), "k 31": S("k", 31),
                    "y.w 8": R("y", 2, 5, 8, 16, 1), "y of the other dtype": R("y", 2, 5, 7, 16, 1, dt="other"),
                    "12 channels": both(R("x", 2, 5, 7, 12, 0, ct=16), R("y", 2, 5, 7, 12, 1, ct=16)),
                    "12 channels, pixel stride 12": both(R("x", 2, 5, 7, 12, 0), R("y", 2, 5, 7, 12, 1)),
                    "two faults: k 4 and y.w 8": both(S("k", 4), R("y", 2, 5, 8, 16, 1))}))
    E.append(Entry("spp_pools", lambda dt: dict(x=V(2, 9, 17, 16, dt, 0), y5=V(2, 9, 17, 16, dt, 1), y9=V(2, 9, 17, 16, dt, 2),
                                                y13=V(2, 9, 17, 16, dt, 3)),
                   lambda a: lib.glsdet_spp_pools(a["x"], a["y5"], a["y9"], a["y13"], None),
                   [("x", True), ("y5", True), ("y9", True), ("y13", True)], (),
                   {"y9.h 8": R("y9", 2, 8, 17, 16, 2), "y13 of the other dtype": R("y13", 2, 9, 17, 16, 3, dt="other"),
                    "y9 with another pixel stride": R("y9", 2, 9, 17, 16, 2, ct=32),
                    "12 channels": both(*[R(k, 2, 9, 17, 12, i, ct=16) for i, k in enumerate(("x", "y5", "y9", "y13"))]),
                    "two faults: y9.h 8 and y13 outside": both(R("y9", 2, 8, 17, 16, 2), lambda a: _outside(a["y13"]))}))
    E.append(Entry("channel_maxmean", lambda dt: dict(x=V(2, 5, 7, 32, dt, 0), y=V(2, 5, 7, 8, dt, 1)),
                   lambda a: lib.glsdet_channel_maxmean(a["x"], a["y"], None), [("x", True), ("y", True)], (),
                   {"y.c 16": R("y", 2, 5, 7, 16, 1), "y of the other dtype": R("y", 2, 5, 7, 8, 1, dt="other"), "y.h 6": R("y", 2, 6, 7, 8, 1),
                    "y.n 1": R("y", 1, 5, 7, 8, 1), "x.c 12": R("x", 2, 5, 7, 12, 0, ct=16)}))
    E.append(Entry("resample_copy", lambda dt: dict(x=V(2, 3, 4, 16, dt, 0), y=V(2, 6, 8, 16, dt, 1), factor=2),
                   lambda a: lib.glsdet_resample_copy(a["x"], a["y"], a["factor"], None), [("x", True), ("y", True)], (),
                   {"factor 0": S("factor", 0), "factor 9": S("factor", 9), "factor 1 with a doubled y": S("factor", 1),
                    "factor 1 (copy)": both(S("factor", 1), R("y", 2, 3, 4, 16, 1)), "y.h 7": R("y", 2, 7, 8, 16, 1),
                    "y.c 24": R("y", 2, 6, 8, 24, 1), "y of the other dtype": R("y", 2, 6, 8, 16, 1, dt="other"),
                    "12 channels": both(R("x", 2, 3, 4, 12, 0, ct=16), R("y", 2, 6, 8, 12, 1, ct=16)),
                    "two faults: factor 9 and y.h 7": both(S("factor", 9), R("y", 2, 7, 8, 16, 1))}))
    many = lambda a, f: f(_arr(a["x"]), _arr(a["y"]), a["count"], None)
    E.append(Entry("copy_many", lambda dt: dict(x=[V(1, 4, 5, 16, dt, q) for q in range(3)], y=[V(1, 4, 5, 16, dt, 8 + q) for q in range(3)],
                                                count=3),
                   lambda a: many(a, lib.glsdet_copy_many), [("x", True), ("y", True)], (),
                   {"count 0": S("count", 0), "count 4097": S("count", 4097), "count 1": S("count", 1),
                    "pair 2 of the other dtype": both(R("x", 1, 4, 5, 16, 2, dt="other"), R("y", 1, 4, 5, 16, 10, dt="other")),
                    "pair 2: y.c 24": R("y", 1, 4, 5, 24, 10), "pair 2: y.h 5": R("y", 1, 5, 5, 16, 10),
                    "12 channels": lambda a: [a[k].__setitem__(q, V(1, 4, 5, 12, a["dt"], s + q, ct=16)) for k, s in (("x", 0), ("y", 8))
                                              for q in range(3)],
                    "two faults: pair 0's y outside and pair 2's x outside": lambda a: (_outside(a["y"][0]), _outside(a["x"][2]))}))
    E.append(Entry("transpose_many", lambda dt: dict(x=[V(1, 4, 5, 16, dt, q) for q in range(3)],
                                                     y=[V(1, 1, 16, 24, dt, 8 + q) for q in range(3)], count=3),
                   lambda a: many(a, lib.glsdet_transpose_many), [("x", True), ("y", True)], (),
                   {"count 0": S("count", 0), "count 4097": S("count", 4097), "pair 2: x.n 2": R("x", 2, 4, 5, 16, 2),
                    "pair 2: y.h 2": R("y", 1, 2, 16, 24, 10), "pair 2: 8 rows for 16 channels": R("y", 1, 1, 8, 24, 10),
                    "pair 2: 16 columns for 20 pixels": R("y", 1, 1, 16, 16, 10), "pair 2: x of the other dtype": R("x", 1, 4, 5, 16, 2, dt="other"),
                    "pair 2: x.c 24": R("x", 1, 4, 5, 24, 2),
                    "12 channels": lambda a: [a["x"].__setitem__(q, V(1, 4, 5, 12, a["dt"], q, ct=16)) for q in range(3)]}))

    # ---- adapt.hip
    E.append(Entry("attn_split", lambda dt: dict(att=V(2, 16, 16, 1, dt, 0), split=P + (20 << 20)),
                   lambda a: lib.glsdet_attn_split(a["att"], a["split"], None), [("att", False)], ["split"],
                   {"4 rows": R("att", 2, 4, 16, 1, 0), "4 columns": R("att", 2, 16, 4, 1, 0), "17 images": R("att", 17, 16, 16, 1, 0),
                    "16 maps of 400 x 400": R("att", 16, 400, 400, 1, 0), "two faults: 4 rows and 17 images": R("att", 17, 4, 16, 1, 0)}))
    rs = lambda dt: dict(a=V(2, 6, 8, 16, dt, 0), b=V(2, 6, 8, 16, dt, 1), y=V(2, 6, 8, 16, dt, 2), split=P + (20 << 20), mode=2)
    E.append(Entry("rowsplit", rs, lambda a: lib.glsdet_rowsplit(a["a"], a["b"], a["y"], a["split"], a["mode"], None),
                   [("a", True), ("y", True), ("b", True)], ["split"],
                   {"mode 5": S("mode", 5), "mode 15": S("mode", 15), "mode 0": S("mode", 0), "mode 1 without b": both(S("mode", 1), S("b", None)),
                    "mode 3, quadrant 2": S("mode", 3 | 2 << 4), "mode 4, quadrant 1, shifted": S("mode", 4 | 1 << 4 | 1 << 8),
                    "mode 0 with a broken b (unused)": both(S("mode", 0), lambda a: _outside(a["b"])), "y.w 9": R("y", 2, 6, 9, 16, 2),
                    "y of the other dtype": R("y", 2, 6, 8, 16, 2, dt="other"), "b.c 24": R("b", 2, 6, 8, 24, 1),
                    "b of the other dtype": R("b", 2, 6, 8, 16, 1, dt="other"),
                    "two faults: mode 5 and a outside": both(S("mode", 5), lambda a: _outside(a["a"]))}))
    E.append(Entry("scale_by_map", lambda dt: dict(x=V(2, 5, 7, 16, dt, 0), map=V(2, 5, 7, 1, dt, 1), y=V(2, 5, 7, 16, dt, 2)),
                   lambda a: lib.glsdet_scale_by_map(a["x"], a["map"], a["y"], None), [("x", True), ("map", False), ("y", True)], (),
                   {"map of the other dtype": R("map", 2, 5, 7, 1, 1, dt="other"), "map.h 6": R("map", 2, 6, 7, 1, 1),
                    "y.c 24": R("y", 2, 5, 7, 24, 2), "y of the other dtype": R("y", 2, 5, 7, 16, 2, dt="other"),
                    "two faults: map outside and y outside": lambda a: (_outside(a["y"]), _outside(a["map"]))}))
    E.append(Entry("gate", lambda dt: dict(a=V(2, 5, 7, 16, dt, 0), b=V(2, 5, 7, 16, dt, 1), map=V(2, 5, 7, 2, dt, 2), y=V(2, 5, 7, 16, dt, 3),
                                           mode=0),
                   lambda a: lib.glsdet_gate(a["a"], a["b"], a["map"], a["y"], a["mode"], None),
                   [("a", True), ("b", True), ("y", True), ("map", False)], (),
                   {"mode 2": S("mode", 2), "mode -1": S("mode", -1), "mode 1": S("mode", 1), "mode 1 without a map": both(S("mode", 1), S("map", None)),
                    "mode 1 with a broken map (unused)": both(S("mode", 1), lambda a: _outside(a["map"])), "map.c 1": R("map", 2, 5, 7, 1, 2),
                    "map.w 8": R("map", 2, 5, 8, 2, 2), "map of the other dtype": R("map", 2, 5, 7, 2, 2, dt="other"),
                    "b.c 24": R("b", 2, 5, 7, 24, 1), "a of the other dtype": R("a", 2, 5, 7, 16, 0, dt="other"),
                    "two faults: mode 2 and a outside": both(S("mode", 2), lambda a: _outside(a["a"]))}))

    # ---- resdet.hip
    E.append(Entry("nchw_pack", lambda dt: dict(img=img, n=2, cin=3, H=5, W=7, y=V(2, 5, 7, 8, dt, 1)),
                   lambda a: lib.glsdet_nchw_pack(a["img"], a["n"], a["cin"], a["H"], a["W"], a["y"], None), [("y", True)], ["img"],
                   {"n 0": S("n", 0), "cin 0": S("cin", 0), "cin 9 > y.c": S("cin", 9), "H 6": S("H", 6), "y.c 12": R("y", 2, 5, 7, 12, 1, ct=16)}))
    E.append(Entry("pool2d", lambda dt: dict(x=V(2, 9, 11, 16, dt, 0), y=V(2, 5, 6, 16, dt, 1), k=3, stride=2, pad=1),
                   lambda a: lib.glsdet_pool2d(a["x"], a["y"], a["k"], a["stride"], a["pad"], None), [("x", True), ("y", True)], (),
                   {"k 0": S("k", 0), "k 32": S("k", 32), "stride 0": S("stride", 0), "pad -1": S("pad", -1), "pad 2 (2 pad > k)": S("pad", 2),
                    "y.h 6": R("y", 2, 6, 6, 16, 1), "y.c 24": R("y", 2, 5, 6, 24, 1), "y of the other dtype": R("y", 2, 5, 6, 16, 1, dt="other"),
                    "12 channels": both(R("x", 2, 9, 11, 12, 0, ct=16), R("y", 2, 5, 6, 12, 1, ct=16)),
                    "two faults: k 0 and y.h 6": both(S("k", 0), R("y", 2, 6, 6, 16, 1))}))
    E.append(Entry("upsample_add", lambda dt: dict(coarse=V(2, 3, 4, 16, dt, 0), fine=V(2, 6, 8, 16, dt, 1)),
                   lambda a: lib.glsdet_upsample_add(a["coarse"], a["fine"], None), [("coarse", True), ("fine", True)], (),
                   {"fine of the other dtype": R("fine", 2, 6, 8, 16, 1, dt="other"), "fine.n 3": R("fine", 3, 6, 8, 16, 1),
                    "fine.c 24": R("fine", 2, 6, 8, 24, 1), "fine 7 x 9 (any size)": R("fine", 2, 7, 9, 16, 1),
                    "12 channels": both(R("coarse", 2, 3, 4, 12, 0, ct=16), R("fine", 2, 6, 8, 12, 1, ct=16))}))
    gam, bet, stats = [P + (43 << 20), P + (43 << 20) + 0x1000], [P + (44 << 20), P + (44 << 20) + 0x1000], P + (45 << 20)
    gn = lambda dt: dict(x=[V(2, 5, 7, 64, dt, 0), V(2, 3, 4, 64, dt, 1)], y=[V(2, 5, 7, 64, dt, 2), V(2, 3, 4, 64, dt, 3)], n_sets=2, groups=8,
                         gamma=list(gam), beta=list(bet), eps=1e-5, act=2, stats=stats, pre=[None, P + (46 << 20)])
    gn_faults = {"groups 0": S("groups", 0), "groups 257": S("groups", 257), "groups 3": S("groups", 3), "groups 64 (1 channel each)": S("groups", 64),
                 "groups 1": S("groups", 1), "act silu": S("act", 1), "act none": S("act", 0), "stats 4 bytes off": S("stats", stats + 4),
                 "last y.w 5": lambda a: a["y"].__setitem__(-1, V(2, a["x"][-1].h, 5, 64, a["dt"], 3)),
                 "last x, y of the other dtype": lambda a: (a["x"].__setitem__(-1, V(2, a["x"][-1].h, a["x"][-1].w, 64, 1 - a["dt"], 1)),
                                                            a["y"].__setitem__(-1, V(2, a["x"][-1].h, a["x"][-1].w, 64, 1 - a["dt"], 3))),
                 "two faults: act silu and x outside": both(S("act", 1), lambda a: _outside(a["x"][-1]))}
    multi_faults = dict(gn_faults, **{"n_sets 0": S("n_sets", 0), "n_sets 17": S("n_sets", 17), "n_sets 1": S("n_sets", 1),
                                      "set 1 with 96 channels": both(R("x", 2, 3, 4, 96, 1), R("y", 2, 3, 4, 96, 3)),
                                      "set 1 with 3 images": both(R("x", 3, 3, 4, 64, 1), R("y", 3, 3, 4, 64, 3)),
                                      "null gamma of set 1": lambda a: a["gamma"].__setitem__(1, None),
                                      "null beta of set 1": lambda a: a["beta"].__setitem__(1, None)})
    E.append(Entry("groupnorm", lambda dt: dict(gn(dt), x=[V(2, 5, 7, 64, dt, 0)], y=[V(2, 5, 7, 64, dt, 2)]),
                   lambda a: lib.glsdet_groupnorm(_arr(a["x"]), _arr(a["y"]), a["groups"], a["gamma"] and a["gamma"][0], a["beta"] and a["beta"][0],
                                                  a["eps"], a["act"], a["stats"], None),
                   [("x", True), ("y", True)], ["gamma", "beta", "stats"],
                   dict(gn_faults, **{"192 channels, 1 group (EVC)": both(R("x", 2, 5, 7, 192, 0), R("y", 2, 5, 7, 192, 2), S("groups", 1)),
                                      "40 channels, 5 groups": both(R("x", 2, 5, 7, 40, 0), R("y", 2, 5, 7, 40, 2), S("groups", 5))})))
    E.append(Entry("groupnorm_multi", gn,
                   lambda a: lib.glsdet_groupnorm_multi(_arr(a["x"]), _arr(a["y"]), a["n_sets"], a["groups"], _ptrs(a["gamma"]), _ptrs(a["beta"]),
                                                        a["eps"], a["act"], a["stats"], None),
                   [("x", True), ("y", True)], ["gamma", "beta", "stats"], multi_faults))
    E.append(Entry("groupnorm_multi_pre", gn,
                   lambda a: lib.glsdet_groupnorm_multi_pre(_arr(a["x"]), _arr(a["y"]), a["n_sets"], a["groups"], _ptrs(a["gamma"]),
                                                            _ptrs(a["beta"]), a["eps"], a["act"], a["stats"], _ptrs(a["pre"]), None),
                   [("x", True), ("y", True)], ["gamma", "beta", "stats", "pre"],
                   dict(multi_faults, **{"every set with conv partials": lambda a: a["pre"].__setitem__(0, P + (47 << 20)),
                                         "conv partials 4 bytes off": lambda a: a["pre"].__setitem__(1, P + (46 << 20) + 4)})))

    def proxy(dt):
        return dict(feat=V(2, 5, 7, 32, dt, 0), dots=V(2, 5, 7, 6, 1, 1), counts=[2, 3, 1], nc=3, gamma=0.5, out=V(2, 5, 7, 3, 1, 2))

    def proxy_call(a):
        counts = None if a["counts"] is None else (C.c_int32 * 256)(*a["counts"])       # read by the host: real memory
        return lib.glsdet_proxy_scores(a["feat"], a["dots"], counts, a["nc"], a["gamma"], a["out"], None)
    E.append(Entry("proxy_scores", proxy, proxy_call, [("feat", True), ("dots", False), ("out", False)], ["counts"],
                   {"fp16 dots": R("dots", 2, 5, 7, 6, 1, dt=0), "fp16 out": R("out", 2, 5, 7, 3, 2, dt=0), "0 classes": S("nc", 0),
                    "257 classes": S("nc", 257), "a class with no proxy": S("counts", [2, 0, 1]), "a class with 65 proxies": S("counts", [2, 65, 1]),
                    "260 proxies": both(S("counts", [60] * 5), S("nc", 5)), "dots.c 5 < P": R("dots", 2, 5, 7, 5, 1, dt=1),
                    "out.c 2 < classes": R("out", 2, 5, 7, 2, 2, dt=1), "dots.w 8": R("dots", 2, 5, 8, 6, 1, dt=1), "out.n 1": R("out", 1, 5, 7, 3, 2, dt=1),
                    "feat.c 12": R("feat", 2, 5, 7, 12, 0, ct=16),
                    "two faults: fp16 dots and 0 classes": both(R("dots", 2, 5, 7, 6, 1, dt=0), S("nc", 0))}))

    # ---- evc.hip
    need = lib.glsdet_lvc_encode_workspace_bytes(2, 5, 7, 64)
    E.append(Entry("lvc_encode", lambda dt: dict(x=V(2, 5, 7, 64, dt, 0), cw=w, scale=sc, ws=P + (45 << 20), ws_bytes=need, E=P + (46 << 20)),
                   lambda a: lib.glsdet_lvc_encode(a["x"], a["cw"], a["scale"], a["ws"], a["ws_bytes"], a["E"], None), [("x", True)],
                   ["cw", "scale", "ws", "E"],
                   {"48 channels": R("x", 2, 5, 7, 48, 0), "16 channels": R("x", 2, 5, 7, 16, 0), "672 channels": R("x", 2, 5, 7, 672, 0),
                    "640 channels": both(R("x", 2, 5, 7, 640, 0), S("ws_bytes", 1 << 30)), "2^24 + 1 pixels": R("x", 1, 1, (1 << 24) + 1, 64, 0),
                    "65536 images": both(R("x", 65536, 1, 1, 64, 0), S("ws_bytes", 1 << 40)), "codewords 8 bytes off": S("cw", w + 8),
                    "scale 4 bytes off": S("scale", sc + 4), "E 8 bytes off": S("E", P + (46 << 20) + 8), "workspace 16 bytes off": S("ws", P + (45 << 20) + 16),
                    "workspace one byte short": S("ws_bytes", need - 1), "workspace of 0 bytes": S("ws_bytes", 0),
                    "two faults: 48 channels and codewords 8 bytes off": both(R("x", 2, 5, 7, 48, 0), S("cw", w + 8))}, ))
    lg = ("E", "a_k", "b_k", "fc_w", "fc_b", "gam")
    E.append(Entry("lvc_gate", lambda dt: dict({k: P + ((50 + i) << 20) for i, k in enumerate(lg)}, n=2, C=64),
                   lambda a: lib.glsdet_lvc_gate(a["E"], a["n"], a["C"], a["a_k"], a["b_k"], a["fc_w"], a["fc_b"], a["gam"], None), [], lg,
                   {"n 0": S("n", 0), "n 65536": S("n", 65536), "n 65535": S("n", 65535), "C 48": S("C", 48), "C 0": S("C", 0), "C 672": S("C", 672),
                    "C 640": S("C", 640), "E 8 bytes off": S("E", P + (50 << 20) + 8), "fc_w 4 bytes off": S("fc_w", P + (53 << 20) + 4),
                    "gam 8 bytes off": S("gam", P + (55 << 20) + 8), "a_k 4 bytes off (no need)": S("a_k", P + (51 << 20) + 4),
                    "two faults: n 0 and C 48": both(S("n", 0), S("C", 48)), "two faults: C 48 and E 8 bytes off": both(S("C", 48), S("E", P + (50 << 20) + 8))},
                   dtypes=(0,)))
    E.append(Entry("channel_fuse", lambda dt: dict(a=V(2, 5, 7, 16, dt, 0), t=V(2, 5, 7, 16, dt, 1), y=V(2, 5, 7, 16, dt, 2), v=P + (50 << 20), mode=1),
                   lambda a: lib.glsdet_channel_fuse(a["a"], a["t"], a["y"], a["v"], a["mode"], None), [("a", True), ("y", True), ("t", True)], ["v"],
                   {"mode 2": S("mode", 2), "mode -1": S("mode", -1), "mode 0": S("mode", 0), "mode 0 without t": both(S("mode", 0), S("t", None)),
                    "mode 0 with a broken t (unused)": both(S("mode", 0), lambda a: _outside(a["t"])), "v 8 bytes off": S("v", P + (50 << 20) + 8),
                    "y.h 6": R("y", 2, 6, 7, 16, 2), "y of the other dtype": R("y", 2, 5, 7, 16, 2, dt="other"), "t.c 24": R("t", 2, 5, 7, 24, 1),
                    "t of the other dtype": R("t", 2, 5, 7, 16, 1, dt="other"),
                    "12 channels": both(*[R(k, 2, 5, 7, 12, i, ct=16) for i, k in enumerate(("a", "t", "y"))]),
                    "two faults: v 8 bytes off and t.c 24": both(S("v", P + (50 << 20) + 8), R("t", 2, 5, 7, 24, 1))}))

    # ---- swin.hip (span-only overlap rule)
    E.append(Entry("layernorm", lambda dt: dict(x=V(2, 5, 7, 64, dt, 0), y=V(2, 5, 7, 64, dt, 1), gamma=gam[0], beta=bet[0], eps=1e-5),
                   lambda a: lib.glsdet_layernorm(a["x"], a["y"], a["gamma"], a["beta"], a["eps"], None), [("x", True), ("y", True)], ["gamma", "beta"],
                   {"y of the other dtype": R("y", 2, 5, 7, 64, 1, dt="other"), "y.w 8": R("y", 2, 5, 8, 64, 1),
                    "48 channels": both(R("x", 2, 5, 7, 48, 0), R("y", 2, 5, 7, 48, 1)), "16 channels": both(R("x", 2, 5, 7, 16, 0), R("y", 2, 5, 7, 16, 1)),
                    "4128 channels": both(R("x", 1, 1, 2, 4128, 0), R("y", 1, 1, 2, 4128, 1)),
                    "4096 channels": both(R("x", 1, 1, 2, 4096, 0), R("y", 1, 1, 2, 4096, 1)),
                    "in place (the same view)": R("y", 2, 5, 7, 64, 0), "in place, in the other dtype": R("y", 2, 5, 7, 64, 0, dt="other"),
                    "y one pixel into x": R("y", 2, 5, 7, 64, 0, off=64), "y a channel slice beside x": both(R("x", 2, 5, 7, 64, 0, ct=128),
                                                                                                        R("y", 2, 5, 7, 64, 0, ct=128, off=64)),
                    "eps 0": S("eps", 0.0), "eps -1e-5": S("eps", -1e-5), "eps nan": S("eps", float("nan")), "eps inf": S("eps", float("inf")),
                    "gamma 8 bytes off": S("gamma", gam[0] + 8), "beta 4 bytes off": S("beta", bet[0] + 4),
                    "two faults: y.w 8 and eps nan": both(R("y", 2, 5, 8, 64, 1), S("eps", float("nan")))}))
    E.append(Entry("patch_merge", lambda dt: dict(x=V(2, 5, 7, 16, dt, 0), y=V(2, 3, 4, 64, dt, 1)),
                   lambda a: lib.glsdet_patch_merge(a["x"], a["y"], None), [("x", True), ("y", True)], (),
                   {"y of the other dtype": R("y", 2, 3, 4, 64, 1, dt="other"), "y starting in x's last pixel": R("y", 2, 3, 4, 64, 0, off=2 * 5 * 7 * 16 - 8),
                    "y a channel slice beside x": both(R("x", 2, 5, 7, 16, 0, ct=128), R("y", 2, 3, 4, 64, 0, ct=128, off=64)),
                    "12 channels": both(R("x", 2, 5, 7, 12, 0, ct=16), R("y", 2, 3, 4, 48, 1)), "y.h 2": R("y", 2, 2, 4, 64, 1),
                    "y.c 32": R("y", 2, 3, 4, 32, 1), "two faults: y of the other dtype and y.h 2": R("y", 2, 2, 4, 64, 1, dt="other")}))
    tab, qb = P + (43 << 20), P + (44 << 20)
    E.append(Entry("window_attention", lambda dt: dict(qkv=V(2, 7, 9, 192, dt, 0), y=V(2, 7, 9, 64, dt, 1), table=tab, qb=qb, heads=2, ws=4, shift=1,
                                                       scale=0.125),
                   lambda a: lib.glsdet_window_attention(a["qkv"], a["y"], a["table"], a["qb"], a["heads"], a["ws"], a["shift"], a["scale"], None),
                   [("qkv", True), ("y", True)], ["table", "qb"],
                   {"y of the other dtype": R("y", 2, 7, 9, 64, 1, dt="other"), "48 channels": both(R("qkv", 2, 7, 9, 144, 0), R("y", 2, 7, 9, 48, 1)),
                    "1056 channels": both(R("qkv", 1, 2, 2, 3168, 0), R("y", 1, 2, 2, 1056, 1), S("heads", 33)), "qkv.c 128": R("qkv", 2, 7, 9, 128, 0),
                    "qkv.h 8": R("qkv", 2, 8, 9, 192, 0), "y inside qkv's span": R("y", 2, 7, 9, 64, 0, ct=192, off=64), "heads 3": S("heads", 3),
                    "heads 0": S("heads", 0), "window 1": S("ws", 1), "window 9": S("ws", 9), "window 8, shift 7": both(S("ws", 8), S("shift", 7)),
                    "shift 4": S("shift", 4), "shift -1": S("shift", -1), "shift 0": S("shift", 0), "scale inf": S("scale", float("inf")),
                    "scale nan": S("scale", float("nan")), "bias table 2 bytes off": S("table", tab + 2), "qkv bias 2 bytes off": S("qb", qb + 2),
                    "two faults: heads 3 and window 9": both(S("heads", 3), S("ws", 9))}))

    # ---- dwconv.hip
    def dw_call(a):
        return lib.glsdet_dwconv2d_dilated(None if a["d"] is None else C.byref(a["d"]), a["dil"], None)
    E.append(Entry("dwconv2d_dilated", lambda dt: dict(d=_desc(V(2, 9, 11, 16, dt, 0), V(2, 9, 11, 16, dt, 1), 3, 3, 1, 1), dil=1), dw_call,
                   [("d.x", True), ("d.y", True)], ["d"],
                   {"dilation 0": S("dil", 0), "dilation 9": S("dil", 9),
                    "dilation 2, pad 2": both(S("dil", 2), lambda a: setattr(a["d"], "pad", 2)),
                    "dilation 2 (y too large)": S("dil", 2), "y.c 24": lambda a: setattr(a["d"], "y", V(2, 9, 11, 24, a["dt"], 1)),
                    "y of the other dtype": lambda a: setattr(a["d"], "y", V(2, 9, 11, 16, 1 - a["dt"], 1)),
                    "12 channels": lambda a: (setattr(a["d"], "x", V(2, 9, 11, 12, a["dt"], 0, ct=16)), setattr(a["d"], "y", V(2, 9, 11, 12, a["dt"], 1, ct=16))),
                    "R 0": lambda a: setattr(a["d"], "R", 0), "S 16": lambda a: setattr(a["d"], "S", 16), "stride 5": lambda a: setattr(a["d"], "stride", 5),
                    "stride 0": lambda a: setattr(a["d"], "stride", 0), "pad -1": lambda a: setattr(a["d"], "pad", -1),
                    "a residual": lambda a: setattr(a["d"], "res", V(2, 9, 11, 16, a["dt"], 2)), "y.h 8": lambda a: setattr(a["d"], "y", V(2, 8, 11, 16, a["dt"], 1)),
                    "null weight": lambda a: setattr(a["d"], "w", None), "null bias": lambda a: setattr(a["d"], "bias", None),
                    "weight 8 bytes off": lambda a: setattr(a["d"], "w", w + 8), "act 4": lambda a: setattr(a["d"], "act", 4),
                    "act -1": lambda a: setattr(a["d"], "act", -1), "act 3": lambda a: setattr(a["d"], "act", 3),
                    "two faults: dilation 0 and x outside": both(S("dil", 0), lambda a: _outside(a["d"].x))}))

    # ---- stem.hip
    stem = lambda H, W, y: (lambda dt: dict(img=img, n=2, cin=3, H=H, W=W, w=w, scale=sc, bias=bi, act=1, y=V(*y, dt, 1)))
    stem_faults = lambda name, y, minhw: {
        "cin 4": S("cin", 4), "n 0": S("n", 0), "H %d" % minhw: S("H", minhw), "img 4 bytes off": S("img", img + 4), "img 2 bytes off": S("img", img + 2),
        "weight 8 bytes off": S("w", w + 8), "scale 4 bytes off": S("scale", sc + 4), "bias 8 bytes off": S("bias", bi + 8),
        "y.h + 1": R("y", y[0], y[1] + 1, y[2], y[3], 1), "y.n 1": R("y", 1, y[1], y[2], y[3], 1), "y.c 24": R("y", y[0], y[1], y[2], 24, 1),
        "y.c 12": R("y", y[0], y[1], y[2], 12, 1, ct=16), "y.c 72": R("y", y[0], y[1], y[2], 72, 1), "act 6": S("act", 6), "act -1": S("act", -1),
        "act 5": S("act", 5), "two faults: cin 4 and y outside": both(S("cin", 4), lambda a: _outside(a["y"])),
        "two faults: y outside and act 6": both(lambda a: _outside(a["y"]), S("act", 6))}
    E.append(Entry("focus_conv", stem(16, 24, (2, 8, 12, 32)),
                   lambda a: lib.glsdet_focus_conv(a["img"], a["n"], a["cin"], a["H"], a["W"], a["w"], a["scale"], a["bias"], a["act"], a["y"], None),
                   [("y", True)], ["img", "w", "scale", "bias"],
                   dict(stem_faults("focus_conv", (2, 8, 12, 32), 1), **{"H odd": S("H", 15), "y.c 64 (the wide tile)": R("y", 2, 8, 12, 64, 1)})))
    E.append(Entry("focus_conv_down", lambda dt: dict(stem(16, 24, (2, 4, 6, 64))(dt), w2=P + (47 << 20), scale2=P + (48 << 20), bias2=P + (49 << 20),
                                                      act2=1, c1=32),
                   lambda a: lib.glsdet_focus_conv_down(a["img"], a["n"], a["cin"], a["H"], a["W"], a["w"], a["scale"], a["bias"], a["act"], a["c1"],
                                                        a["w2"], a["scale2"], a["bias2"], a["act2"], a["y"], None),
                   [("y", True)], ["img", "w", "scale", "bias", "w2", "scale2", "bias2"],
                   dict(stem_faults("focus_conv_down", (2, 4, 6, 64), 2), **{"H odd": S("H", 15), "c1 16": S("c1", 16), "act2 6": S("act2", 6),
                                                                            "w2 8 bytes off": S("w2", P + (47 << 20) + 8), "y.c 32": R("y", 2, 4, 6, 32, 1)})))
    E.append(Entry("resnet_stem", stem(32, 40, (2, 16, 20, 64)),
                   lambda a: lib.glsdet_resnet_stem(a["img"], a["n"], a["cin"], a["H"], a["W"], a["w"], a["scale"], a["bias"], a["act"], a["y"], None),
                   [("y", True)], ["img", "w", "scale", "bias"], stem_faults("resnet_stem", (2, 16, 20, 64), 6)))
    E.append(Entry("resnet_stem_pool", stem(32, 40, (2, 8, 10, 64)),
                   lambda a: lib.glsdet_resnet_stem_pool(a["img"], a["n"], a["cin"], a["H"], a["W"], a["w"], a["scale"], a["bias"], a["y"], None),
                   [("y", True)], ["img", "w", "scale", "bias"], stem_faults("resnet_stem_pool", (2, 8, 10, 64), 6)))
    return E


# ---- the "y overlaps x" rule of the three conv entry points that take channel slices of one concat buffer -------------------
def _overlap_views(dt, c):
    """{label: (x, y)}: x is [2, 6, 8, c]; the concat buffer has 2 c channels per pixel"""
    cat = lambda off: V(2, 6, 8, c, dt, 0, ct=2 * c, off=off)
    skew = cat(c)
    skew.sn += 2 * c                                    # a disjoint slice by its offset, but of another image stride
    skew.alloc_hi += 2 * c * 4
    last = V(2, 6, 8, c, dt, 0, off=2 * 6 * 8 * c - 8)  # begins 8 elements before the end of a dense x
    last.alloc_hi = P + (2 << 20)
    half = cat(c // 2 + 8)
    return {"disjoint buffers": (V(2, 6, 8, c, dt, 0), V(2, 6, 8, c, dt, 1)), "slices [0, c) -> [c, 2c) of one buffer": (cat(0), cat(c)),
            "slices [c, 2c) -> [0, c) of one buffer": (cat(c), cat(0)), "slices that share channels": (cat(0), half),
            "slices that share channels, y first": (half, cat(0)), "the same view": (cat(0), cat(0)),
            "equal spans, another image stride": (cat(0), skew), "y starting in x's last pixel": (V(2, 6, 8, c, dt, 0), last)}


def _overlap_cases(lib):
    from glsdet_amd import _lib
    out = {}
    for dt in (0, 1):
        for label, (x, y) in _overlap_views(dt, 64).items():
            out["conv2d_grouped/%d/%s" % (dt, label)] = lambda x=x, y=y: lib.glsdet_conv2d_grouped(C.byref(_desc(x, y, 3, 3, 1, 1)), 8, None)
            hid = V(2, 6, 8, 64, dt, 3)
            out["bottleneck/%d/%s" % (dt, label)] = lambda x=x, y=y, hid=hid: lib.glsdet_bottleneck(
                C.byref(_desc(x, hid, 1, 1, 1, 0)), C.byref(_desc(hid, y, 3, 3, 1, 1)), 0, None)
    for label, (x, y) in _overlap_views(0, 64).items():
        d = _lib.CspDesc()
        d.x, d.y, d.act, d.shortcut = x, y, 1, 1
        for i, (k, _) in enumerate(_lib.CspDesc._fields_[2:14]):
            setattr(d, k, P + ((40 + i) << 20))
        out["csp_fused/0/" + label] = lambda d=d: lib.glsdet_csp_fused(C.byref(d), 0, None)
    return out


def _in_plan(lib, call):
    """(rc, message, [(kind, flops, bytes, name)]) of one call made while a plan records"""
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        try:
            rc = call()
            msg = lib.glsdet_last_error().decode() if rc else ""
        finally:
            assert lib.glsdet_plan_end(plan) == 0
        ops = []
        for i in range(lib.glsdet_plan_num_ops(plan)):
            kind, flops, nbytes, name = C.c_int32(), C.c_double(), C.c_double(), C.create_string_buffer(192)
            assert lib.glsdet_plan_op_info(plan, i, C.byref(kind), C.byref(flops), C.byref(nbytes), name, 192) == 0
            ops.append([kind.value, flops.value, nbytes.value, name.value.decode()])
        return {"rc": rc, "msg": msg, "ops": ops}
    finally:
        lib.glsdet_plan_destroy(plan)


def run_table(lib):
    """{"entry/dtype/label": {"rc", "msg", "ops"}} of every case of the table"""
    out = {}
    for e in _entries(lib):
        for dt in e.dtypes:
            for label, mutate in e.cases().items():
                a = e.args(dt)
                a["dt"] = dt
                mutate(a)
                out["%s/%d/%s" % (e.name, dt, label)] = _in_plan(lib, lambda: e.call(a))
    for key, call in _overlap_cases(lib).items():
        out[key] = _in_plan(lib, call)
    return out


ENTRY_POINTS = ("focus_pack", "maxpool2d", "spp_pools", "channel_maxmean", "resample_copy", "copy_many", "transpose_many", "attn_split",
                "rowsplit", "scale_by_map", "gate", "nchw_pack", "pool2d", "upsample_add", "groupnorm", "groupnorm_multi",
                "groupnorm_multi_pre", "proxy_scores", "lvc_encode", "lvc_gate", "channel_fuse", "layernorm", "patch_merge",
                "window_attention", "dwconv2d_dilated", "focus_conv", "focus_conv_down", "resnet_stem", "resnet_stem_pool")
OVERLAP = ("conv2d_grouped", "bottleneck", "csp_fused")

_state = {}


def _results():
    if not _state:
        with open(GOLDEN) as f:
            _state["want"] = json.load(f)
        _state["got"] = run_table(_lib())
    return _state["got"], _state["want"]


def test_the_table_and_the_recorded_contract_hold_the_same_cases():
    got, want = _results()
    assert sorted(got) == sorted(want)
    assert {k.split("/")[0] for k in got} == set(ENTRY_POINTS + OVERLAP)


@pytest.mark.parametrize("entry", ENTRY_POINTS + OVERLAP)
def test_codes_messages_and_recorded_ops_are_those_of_the_parent(entry):
    got, want = _results()
    keys = [k for k in want if k.split("/")[0] == entry]
    assert keys
    for k in keys:
        assert got[k] == want[k], k
        if got[k]["rc"]:
            assert got[k]["rc"] in (ARG, BOUNDS, ALIGN) and got[k]["msg"] and got[k]["ops"] == [], k      # refused: nothing recorded
        else:
            assert len(got[k]["ops"]) == 1, k


@pytest.mark.parametrize("entry", ENTRY_POINTS)
def test_the_table_covers_what_the_contract_names(entry):
    """per entry point: an accepted call per dtype that records one op, refusals, a call with two faults whose winner is recorded,
    and per view operand a refusal with GLSDET_E_BOUNDS (plus GLSDET_E_ALIGN, for a base and for a stride, where the operand needs 16-byte alignment)"""
    _, want = _results()
    mine = {k: v for k, v in want.items() if k.split("/")[0] == entry}
    for dt in {k.split("/")[1] for k in mine}:
        acc = mine["%s/%s/accepted" % (entry, dt)]
        assert acc["rc"] == 0 and len(acc["ops"]) == 1
    assert any(v["rc"] == ARG for v in mine.values())
    assert any("two faults" in k and v["rc"] for k, v in mine.items())
    if entry != "lvc_gate":                              # (no view operand)
        assert any(k.endswith("outside its allocation") and v["rc"] == BOUNDS for k, v in mine.items())
        assert any("base 8 bytes off" in k and v["rc"] == ALIGN for k, v in mine.items()) or entry == "attn_split"
        assert any("stride one element off" in k and v["rc"] == ALIGN for k, v in mine.items()) or entry == "attn_split"


@pytest.mark.parametrize("entry", OVERLAP)
def test_the_overlap_rule_of_the_conv_entry_points(entry):
    """disjoint buffers and disjoint channel slices of one concat buffer (both orders) are accepted; shared channels, equal spans
    with other strides and a y that starts inside x's last pixel are refused"""
    _, want = _results()
    for dt in (0,) if entry == "csp_fused" else (0, 1):
        res = {k.split("/", 2)[2]: v for k, v in want.items() if k.startswith("%s/%d/" % (entry, dt))}
        for label in ("disjoint buffers", "slices [0, c) -> [c, 2c) of one buffer", "slices [c, 2c) -> [0, c) of one buffer"):
            assert res[label]["rc"] == 0 and len(res[label]["ops"]) == 1, (entry, dt, label, res[label])
        for label in ("slices that share channels", "slices that share channels, y first", "the same view", "equal spans, another image stride",
                      "y starting in x's last pixel"):
            assert res[label]["rc"] == ARG and "y overlaps x" in res[label]["msg"], (entry, dt, label, res[label])
