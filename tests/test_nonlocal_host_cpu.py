"""CPU-only: the host side of the four non-local entry points (csrc/nonlocal.hip, csrc/nonlocal_mfma.hip, both on
csrc/nonlocal_common.h), through the built library with fabricated views whose pointers are never dereferenced.

Every malformed call must be refused with the return code below and a message that names its entry point, and an accepted
call recorded into a plan must give exactly one op with the kind, name, flops and bytes below.  All expected values were
taken from the library of the commit before the entry points shared their set builder (9e88810), by running these same
calls against it; none is derived from the code under test."""
import ctypes as C

import pytest

ARG, BOUNDS, ALIGN = -1, -2, -3
ENTRIES = ("nonlocal", "nonlocal_multi", "nonlocal_split", "nonlocal_mfma")
PREFIX = {"nonlocal": "nonlocal", "nonlocal_multi": "nonlocal", "nonlocal_split": "nonlocal_split", "nonlocal_mfma": "nonlocal_mfma"}


def _lib():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib, _lib.load()


def _view(n, h, w, c, dtype, base, ct=0, extra=0):
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    ct = ct or c
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = ct, w * ct, h * w * ct
    v.alloc_lo, v.alloc_hi = base & ~0xFF, base + n * h * w * ct * es + extra
    return v


class Call:
    """Two sets of 2 x {3, 4} x 5 x 96 with ci = 64 (five slots, so that a set count of 5 reads fabricated views too); the
    split entry takes one 2 x 4 x 5 map (slot 0 of x / out) and four projections of it."""

    def __init__(self, entry, dt):
        self.entry, self.dt = entry, dt
        split = entry == "nonlocal_split"
        hs = [4] * 5 if split else [3 + (q & 1) for q in range(5)]
        self.x = [_view(2, hs[q], 5, 96, dt, 0x100000 + 0x100000 * q) for q in range(5)]
        self.o = [_view(2, hs[q], 5, 96, dt, 0x2000000 + 0x100000 * q) for q in range(5)]
        self.t = [_view(2, hs[q], 5, 192, dt, 0x1000000 + 0x100000 * q) for q in range(5)]
        self.w = [0x3000000 + 0x10000 * q for q in range(5)]
        self.b = [0x3100000 + 0x400 * q for q in range(5)]
        self.n_sets, self.ci = 2, 64
        self.ws, self.ws_bytes = 0x4000000, 1 << 30
        self.split, self.shift = 0x5000000, 0
        self.null = None               # name of an operand to pass as a null pointer

    def run(self, lib):
        from glsdet_amd import _lib
        arr = lambda vs: (_lib.View * 5)(*vs)
        ptrs = lambda ps: (C.c_void_p * 5)(*ps)
        a = {"x": arr(self.x), "tpg": arr(self.t), "out": arr(self.o), "wout": ptrs(self.w), "bout": ptrs(self.b), "ws": self.ws,
             "split": self.split}
        if self.null:
            a[self.null] = None
        if self.entry == "nonlocal":
            w = None if self.null == "wout" else self.w[0]
            b = None if self.null == "bout" else self.b[0]
            return lib.glsdet_nonlocal(a["x"], a["tpg"], self.ci, w, b, a["ws"], a["out"], None)
        if self.entry == "nonlocal_multi":
            return lib.glsdet_nonlocal_multi(a["x"], a["tpg"], self.n_sets, self.ci, a["wout"], a["bout"], a["ws"], a["out"], None)
        if self.entry == "nonlocal_split":
            return lib.glsdet_nonlocal_split(a["x"], a["tpg"], self.ci, a["wout"], a["bout"], a["ws"], a["out"], a["split"], self.shift,
                                             None)
        return lib.glsdet_nonlocal_mfma(a["x"], a["tpg"], self.n_sets, self.ci, a["wout"], a["bout"], a["ws"], self.ws_bytes, a["out"],
                                        None)


def _set(c, q, **kw):
    """replace the named ones of x / o / t of set q by a view (n, h, w, c[, dtype]) at the slot's address"""
    dt = c.dt
    for key, base in (("x", 0x100000), ("o", 0x2000000), ("t", 0x1000000)):
        if key in kw:
            getattr(c, key)[q] = _view(*kw[key][:4], kw[key][4] if len(kw[key]) > 4 else dt, base + 0x100000 * q,
                                       extra=kw.get("extra", 0))


# label -> (entries it applies to, mutation).  The faulty set is the last one an entry reads: set 1 of the two-set calls,
# set 0 of glsdet_nonlocal, projection 1 of the split.
def _faults():
    multi = ("nonlocal_multi", "nonlocal_mfma")
    f = {}
    for op in ("x", "tpg", "out", "wout", "bout", "ws"):
        f["null " + op] = (ENTRIES, lambda c, op=op: setattr(c, "null", op))
    f["null split"] = (("nonlocal_split",), lambda c: setattr(c, "null", "split"))
    f["n_sets 0"] = (multi, lambda c: setattr(c, "n_sets", 0))
    f["n_sets 5"] = (multi, lambda c: setattr(c, "n_sets", 5))
    f["ci 0"] = (ENTRIES, lambda c: setattr(c, "ci", 0))
    f["tpg.c < 3 ci"] = (ENTRIES, lambda c: _set(c, c.last, t=(2, c.x[c.last].h, 5, 160)))
    f["sets disagree in n"] = (multi, lambda c: _set(c, 1, x=(3, 4, 5, 96), o=(3, 4, 5, 96)))
    f["sets disagree in channels"] = (multi, lambda c: _set(c, 1, x=(2, 4, 5, 128), o=(2, 4, 5, 128)))
    f["tpg of another dtype"] = (ENTRIES, lambda c: _set(c, c.last, t=(2, c.x[c.last].h, 5, 192, 1 - c.dt)))
    f["out of another dtype"] = (ENTRIES, lambda c: _set(c, c.first, o=(2, c.x[c.first].h, 5, 96, 1 - c.dt)))
    f["x / out extent mismatch"] = (ENTRIES, lambda c: _set(c, c.first, o=(2, c.x[c.first].h, 6, 96)))
    f["tpg / x extent mismatch"] = (ENTRIES, lambda c: _set(c, c.last, t=(2, c.x[c.last].h + 1, 5, 192)))
    f["a view outside its allocation"] = (ENTRIES, lambda c: _set(c, c.last, t=(2, c.x[c.last].h, 5, 192), extra=-2))
    f["an empty window"] = (ENTRIES, lambda c: _set(c, c.first, x=(2, 0, 5, 96), o=(2, 0, 5, 96)))
    f["null wout of the last set"] = (("nonlocal_multi", "nonlocal_split", "nonlocal_mfma"), lambda c: c.w.__setitem__(c.last, None))
    f["null bout of the last set"] = (("nonlocal_multi", "nonlocal_split", "nonlocal_mfma"), lambda c: c.b.__setitem__(c.last, None))
    f["split_shift 2"] = (("nonlocal_split",), lambda c: setattr(c, "shift", 2))
    f["split_shift -1"] = (("nonlocal_split",), lambda c: setattr(c, "shift", -1))
    # what only the matrix-core entry refuses
    mf = ("nonlocal_mfma",)
    f["ci 40"] = (mf, lambda c: setattr(c, "ci", 40))
    f["ci 1312"] = (mf, lambda c: setattr(c, "ci", 1312))
    f["cx 40"] = (mf, lambda c: _set(c, 0, x=(2, 3, 5, 40), o=(2, 3, 5, 40)))
    f["x base not 16-byte aligned"] = (mf, lambda c: c.x.__setitem__(1, _view(2, 4, 5, 96, c.dt, 0x200008)))
    f["tpg stride not 16-byte aligned"] = (mf, lambda c: c.t.__setitem__(1, _view(2, 4, 5, 192, c.dt, 0x1100000, ct=194)))
    f["ws not 256-byte aligned"] = (mf, lambda c: setattr(c, "ws", 0x4000010))
    f["ws one byte short"] = (mf, lambda c: setattr(c, "ws_bytes", c.need - 1))
    f["a misaligned bout"] = (mf, lambda c: c.b.__setitem__(1, 0x3100404))
    return f


def _call(entry, dt, lib):
    c = Call(entry, dt)
    c.first = 0
    c.last = 0 if entry == "nonlocal" else 1
    c.need = lib.glsdet_nonlocal_mfma_workspace_bytes(2, 2, 64, 96)
    return c


# return codes of 9e88810 where they are not GLSDET_E_ARG
NOT_ARG = {"a view outside its allocation": BOUNDS, "x base not 16-byte aligned": ALIGN, "tpg stride not 16-byte aligned": ALIGN,
           "ws not 256-byte aligned": ALIGN, "a misaligned bout": ALIGN}

# (kind, flops, bytes, name) of the one op an accepted call records, on 9e88810, for (fp16, fp32)
RECORDED = {
    "nonlocal": ((4, 115200.0, 23040.0, "nonlocal(gram+fold+apply)"), (4, 115200.0, 46080.0, "nonlocal(gram+fold+apply)")),
    "nonlocal_multi": ((4, 320000.0, 53760.0, "nonlocal_multi(gram+fold+apply)"), (4, 320000.0, 107520.0, "nonlocal_multi(gram+fold+apply)")),
    "nonlocal_split": ((4, 51200.0, 30720.0, "nonlocal_split(gram+fold+apply, device-side quadrants)"),
                       (4, 51200.0, 61440.0, "nonlocal_split(gram+fold+apply, device-side quadrants)")),
    "nonlocal_mfma": ((4, 4579328.0, 53760.0, "nonlocal_mfma(gram+fold+apply)"), (4, 4579328.0, 107520.0, "nonlocal_mfma(gram+fold+apply)")),
}


def sweep(lib):
    """{(entry, dtype, label): (rc, message)} of every fault on every entry it applies to"""
    out = {}
    for label, (entries, mutate) in _faults().items():
        for entry in entries:
            for dt in (0, 1):
                c = _call(entry, dt, lib)
                mutate(c)
                rc = c.run(lib)
                out[(entry, dt, label)] = (rc, lib.glsdet_last_error().decode())
    return out


def record(lib, entry, dt):
    """the ops an accepted call leaves in a plan: [(kind, flops, bytes, name)]"""
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        try:
            rc = _call(entry, dt, lib).run(lib)
        finally:
            assert lib.glsdet_plan_end(plan) == 0
        assert rc == 0, lib.glsdet_last_error().decode()
        ops = []
        for i in range(lib.glsdet_plan_num_ops(plan)):
            kind, flops, nbytes, name = C.c_int32(), C.c_double(), C.c_double(), C.create_string_buffer(128)
            assert lib.glsdet_plan_op_info(plan, i, C.byref(kind), C.byref(flops), C.byref(nbytes), name, 128) == 0
            ops.append((kind.value, flops.value, nbytes.value, name.value.decode()))
        return ops
    finally:
        lib.glsdet_plan_destroy(plan)


def test_every_malformed_call_is_refused_with_its_code_and_its_name():
    _, lib = _lib()
    res = sweep(lib)
    assert len(res) == 162                                            # _faults: every label on its entries, both dtypes
    for (entry, dt, label), (rc, msg) in sorted(res.items()):
        where = "%s, dtype %d, %s: rc %d, %r" % (entry, dt, label, rc, msg)
        assert rc == NOT_ARG.get(label, ARG), where
        assert msg.startswith(PREFIX[entry] + ":") or msg.startswith(PREFIX[entry] + "."), where


@pytest.mark.parametrize("entry", ENTRIES)
def test_an_accepted_call_records_one_op(entry):
    _, lib = _lib()
    for dt in (0, 1):
        assert record(lib, entry, dt) == [RECORDED[entry][dt]], (entry, dt)


def test_a_refused_call_records_nothing():
    _, lib = _lib()
    plan = lib.glsdet_plan_create()
    assert lib.glsdet_plan_begin(plan) == 0
    try:
        for entry in ENTRIES:
            c = _call(entry, 0, lib)
            c.w[c.last] = None
            assert c.run(lib) == ARG, entry
    finally:
        assert lib.glsdet_plan_end(plan) == 0
    assert lib.glsdet_plan_num_ops(plan) == 0
    lib.glsdet_plan_destroy(plan)


@pytest.mark.parametrize("n,sets,ci,cx", [(1, 1, 32, 32), (2, 2, 64, 96), (8, 4, 1280, 1280)])
def test_python_and_library_agree_on_the_workspace(n, sets, ci, cx):
    mod, lib = _lib()
    floats = mod.nonlocal_workspace_floats(sets, n, ci, cx)
    assert floats == sets * n * (8 * ci * ci + cx * ci)               # the tests' own copy of the formula
    assert (floats * 4 + 255) // 256 * 256 == lib.glsdet_nonlocal_mfma_workspace_bytes(n, sets, ci, cx)
