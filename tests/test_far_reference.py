"""CPU-only: the arithmetic of tests/far_reference.py, the coverage of tests/test_far_addresses.py, and the host-side
2 GiB limits of the conv family (fake pointers, recorded into a plan: nothing is launched, nothing is dereferenced)."""
import ast
import ctypes as C
import os

import pytest

from tests import far_reference as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES = (2, 4)


def _overlap(a, b):
    return a[0] < b[1] and b[0] < a[1]


def _all_slots(p, es, block=F.MAX_BLOCK):
    """the live byte ranges of a test that fills every slot with two images of the largest block"""
    sn = p.sn_bytes if p.sn_bytes is not None else block
    return [(p.base + s * F.SLOT + b * sn, p.base + s * F.SLOT + b * sn + block) for s in range(F.MAX_SLOTS) for b in range(2)]


# ------------------------------------------------------------------------------------------------------- 1: placements
@pytest.mark.parametrize("p", F.PLACEMENTS, ids=lambda p: p.name)
@pytest.mark.parametrize("es", ES)
def test_every_placement_lies_inside_the_allocation_and_images_do_not_overlap(p, es):
    live = _all_slots(p, es)
    for lo, hi in live:
        assert F.ALLOC_LO <= lo and hi <= F.BUF_BYTES, (p.name, lo, hi)
    for i, a in enumerate(live):
        for b in live[i + 1:]:
            assert not _overlap(a, b), (p.name, a, b)
    # a real view: the largest conv case of tests/test_far_addresses.py, every kind
    for kind in ("dense", "slice", "window", "ring"):
        v = F.place(p, F.MAX_SLOTS - 1, 2, 19, 23, 64, es, kind)
        assert (v.sn * es) % F.VEC == 0 and (v.off * es) % F.VEC == 0
        last = v.off + (v.n - 1) * v.sn + (v.h - 1) * v.sh + (v.w - 1) * v.sw + v.c          # one past the last element
        assert 0 <= v.off and F.ALLOC_LO + last * es <= F.BUF_BYTES
        lo, hi = F.live_ranges(v)[-1]
        assert lo <= F.ALLOC_LO + (last - v.c) * es and F.ALLOC_LO + last * es <= hi
    if p.sn_bytes is not None:
        assert p.sn_bytes >= 2 ** 31 and p.base - F.ALLOC_LO < 2 ** 31                  # far by its image stride
    else:
        assert p.base - F.ALLOC_LO >= 2 ** 31                                          # far by its base


def test_far_strides_overflow_what_they_are_meant_to_overflow():
    assert F.MID.sn_bytes >= 2 ** 31 and F.MID.sn_bytes < 2 ** 32              # a signed 32-bit byte offset
    assert F.FAR.sn_bytes >= 2 ** 32                                            # an unsigned one too
    assert F.FAR.sn_bytes // 2 >= 2 ** 31 and F.FAR.sn_bytes // 4 < 2 ** 31     # fp16: a signed 32-bit ELEMENT offset
    assert F.BUF_BYTES == 8 * F.GiB + 64 * F.MiB


# --------------------------------------------------------------------------------------------- 2, 3: truncation images
@pytest.mark.parametrize("p", F.PLACEMENTS, ids=lambda p: p.name)
@pytest.mark.parametrize("es", ES)
def test_truncated_addresses_stay_inside_the_buffer_and_outside_every_live_view(p, es):
    """for EVERY slot and the largest block (a smaller block is a subset of it): the union of what any test may place"""
    live = _all_slots(p, es)
    sn = p.sn_bytes if p.sn_bytes is not None else F.MAX_BLOCK
    seen = 0
    for slot in range(F.MAX_SLOTS):
        for lo, hi in F.block_truncations(p.base + slot * F.SLOT, sn, 2, F.MAX_BLOCK, es):
            seen += 1
            assert 0 <= lo and hi <= F.BUF_BYTES, (p.name, slot, lo, hi)
            for a in live:
                assert not _overlap((lo, hi), a), (p.name, slot, (lo, hi), a)
    assert seen, "a placement no 32-bit truncation can get wrong tests nothing"
    # the same through the public function, on a real shape
    for lo, hi in F.truncation_images(p, 2, 19, 23, 64, es, slot=3):
        assert 0 <= lo and hi <= F.BUF_BYTES
        assert not any(_overlap((lo, hi), a) for a in F.live_ranges(F.place(p, 3, 2, 19, 23, 64, es)))


@pytest.mark.parametrize("es", ES)
def test_the_edge_view_touches_both_ends_of_its_allocation(es):
    for (h, w, c) in ((19, 23, 64), (19, 23, 16), (9, 11, 64)):
        v = F.edge_view(2, h, w, c, es)
        (lo0, hi0), (lo1, hi1) = F.edge_ranges(v)
        assert lo0 == 0 and hi1 == F.EDGE and hi0 <= lo1
        assert F.EDGE < F.JUST_IN < F.JUST_OUT == 2 ** 31 - 1 < F.OVER == 2 ** 31
        # the outputs of these tests (dense at `base`, the near ones in allocations of their own) and what a truncated
        # offset of theirs would address lie past every prefix used as an input allocation
        y = F.place(F.BASE, 0, 2, h, w, 64, es, "dense")
        for lo, hi in F.live_ranges(y) + F.truncation_images(F.BASE, 2, h, w, 64, es, kind="dense"):
            assert F.OVER <= lo and hi <= F.BUF_BYTES


# ---------------------------------------------------------------------------------------------------------- 4: coverage
_VIEW_TYPES = ("View", "ConvDesc", "ConvChain", "CspDesc")


def _view_taking(sigs):
    from glsdet_amd import _lib
    ptrs = tuple(C.POINTER(getattr(_lib, t)) for t in _VIEW_TYPES)
    return sorted(name for name, (_, args) in sigs.items() if any(a in ptrs for a in args) and not name.endswith("_tune"))


def _missing(sigs):
    return [name for name in _view_taking(sigs) if name not in F.FAR_CASES]


def _gpu_tests():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_far_addresses.py")).read())
    return {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}


def _raw_ops():
    """the keys of RAW_OPS, read from the source (the module itself needs torch and a GPU-side import chain)"""
    src = open(os.path.join(ROOT, "tests", "test_far_addresses.py")).read()
    body = src[src.index("RAW_OPS = collections.OrderedDict(["):]
    body = body[: body.index("\n])")]
    return {line.split('"')[1] for line in body.splitlines() if line.strip().startswith('("glsdet_')}


def test_every_view_taking_export_has_a_far_case():
    from glsdet_amd import _lib
    assert len(_view_taking(_lib._SIGS)) >= 40
    assert not _missing(_lib._SIGS), "no far-address case in tests/far_reference.py FAR_CASES for: " + ", ".join(_missing(_lib._SIGS))
    tests = _gpu_tests()
    raw = _raw_ops()
    for name, test in F.FAR_CASES.items():
        assert name in _lib._SIGS, name + " is not an export"
        assert test in tests, "%s: tests/test_far_addresses.py has no %s" % (name, test)
        if test == F.RAW:
            assert F.RAW_PAIRS.get(name, name) in raw, "%s: no case in RAW_OPS of tests/test_far_addresses.py" % name
    assert set(F.EDGE_TEST.split()) <= tests


def test_a_new_view_taking_export_fails_the_coverage_test():
    from glsdet_amd import _lib
    sigs = dict(_lib._SIGS)
    sigs["glsdet_some_new_op"] = (C.c_int, [C.POINTER(_lib.View), C.c_void_p])
    sigs["glsdet_some_new_op_tune"] = (C.c_int, [C.POINTER(_lib.View), C.c_void_p])
    sigs["glsdet_some_size_helper"] = (C.c_int64, [C.c_int32])
    assert _missing(sigs) == ["glsdet_some_new_op"]


# --------------------------------------------------------------------------------------------- 5: the host-side limits
LO = 0x100000000000                     # fake device addresses, far apart, 256-byte aligned
ALLOCS = [(F.JUST_IN, True), (F.JUST_OUT, False), (F.OVER, False)]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


def _view(k, n, h, w, c, dtype, alloc=None, sn=None):
    """operand k: a dense view at the start of an allocation of its own (alloc bytes, default: what it needs)"""
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    v = _lib.View()
    base = LO + k * (1 << 36)
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = c, w * c, sn if sn is not None else h * w * c
    need = ((n - 1) * v.sn + h * w * c) * es
    v.alloc_lo, v.alloc_hi = base, base + (alloc if alloc is not None else need)
    assert (alloc or need) >= need
    return v


def _desc(x, y, k, stride=1, hint=0, res=None, act=2):
    from glsdet_amd import _lib
    d = _lib.ConvDesc()
    d.x, d.y = x, y
    if res is not None:
        d.res = res
    d.w, d.scale, d.bias = LO + (40 << 36), LO + (41 << 36), LO + (42 << 36)
    d.R = d.S = k
    d.stride, d.pad, d.act, d.tile_hint = stride, k // 2, act, hint
    return d


def _recorded(lib, call):
    """run `call` while a plan records -> (return code, ops recorded, message)"""
    plan = lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(plan) == 0
        rc = call()
        assert lib.glsdet_plan_end(plan) == 0
        return rc, lib.glsdet_plan_num_ops(plan), lib.glsdet_last_error().decode()
    finally:
        lib.glsdet_plan_destroy(plan)


def _entry_points(lib, dtype, xalloc):
    """name -> call, every conv-family entry point on a 2 x 9 x 17 x 64 input whose allocation is xalloc bytes"""
    from glsdet_amd import _lib
    x = lambda: _view(0, 2, 9, 17, 64, dtype, xalloc)
    y = lambda k=1, c=64: _view(k, 2, 9, 17, c, dtype)
    calls = {}
    for hint in (0, 1):
        calls["glsdet_conv2d hint %d" % hint] = lambda hint=hint: lib.glsdet_conv2d(C.byref(_desc(x(), y(), 3, hint=hint)), None)

    def multi():
        d = (_lib.ConvDesc * 2)(_desc(x(), y(1), 3), _desc(x(), y(2), 3))
        return lib.glsdet_conv2d_multi(d, 2, None)
    calls["glsdet_conv2d_multi"] = multi

    def chain():
        c = _lib.ConvChain()
        c.y2 = y(3)
        c.w2, c.scale2, c.bias2 = LO + (43 << 36), LO + (44 << 36), LO + (45 << 36)
        c.act2, c.c0, c.cin2, c.flags = 2, 0, 64, 0
        return lib.glsdet_conv2d_chain(C.byref(_desc(x(), y(), 3)), C.byref(c), None)
    calls["glsdet_conv2d_chain"] = chain
    calls["glsdet_bottleneck"] = lambda: lib.glsdet_bottleneck(C.byref(_desc(x(), y(4), 1)), C.byref(_desc(y(4), y(5), 3)), 0, None)
    calls["glsdet_conv2d_gnstats"] = lambda: lib.glsdet_conv2d_gnstats(C.byref(_desc(x(), y(), 3, hint=10, act=0)), 8, LO + (46 << 36), None)
    return calls


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "f32"])
@pytest.mark.parametrize("alloc,accepted", ALLOCS, ids=["2^31-2", "2^31-1", "2^31"])
def test_conv_family_input_allocation_limit(lib, dtype, alloc, accepted):
    for name, call in _entry_points(lib, dtype, alloc).items():
        rc, ops, msg = _recorded(lib, call)
        if accepted:
            assert rc == 0 and ops >= 1, "%s refuses an input allocation of %d bytes: %s" % (name, alloc, msg)
        else:
            assert rc < 0 and ops == 0 and F.LIMIT_TEXT in msg, "%s, input allocation of %d bytes: rc %d, %r" % (name, alloc, rc, msg)


def _csp(lib, xalloc, yalloc):
    from glsdet_amd import _lib
    d = _lib.CspDesc()
    d.x, d.y = _view(0, 2, 9, 17, 64, 0, xalloc), _view(1, 2, 9, 17, 64, 0, yalloc)
    for i, (q, k) in enumerate((q, k) for q in ("12", "m1", "m2", "3") for k in ("w", "scale", "bias")):
        setattr(d, k + q, LO + ((50 + i) << 36))
    d.act, d.shortcut = 1, 1
    return lambda: lib.glsdet_csp_fused(C.byref(d), 0, None)


@pytest.mark.parametrize("alloc,accepted", ALLOCS, ids=["2^31-2", "2^31-1", "2^31"])
@pytest.mark.parametrize("operand", ["x", "y"])
def test_csp_fused_allocation_limit_on_x_and_on_y(lib, operand, alloc, accepted):
    rc, ops, msg = _recorded(lib, _csp(lib, alloc if operand == "x" else None, alloc if operand == "y" else None))
    if accepted:
        assert rc == 0 and ops >= 1, "csp_fused refuses %s in an allocation of %d bytes: %s" % (operand, alloc, msg)
    else:
        assert rc < 0 and ops == 0 and F.LIMIT_TEXT in msg, (operand, alloc, rc, msg)


@pytest.mark.parametrize("dtype", [0, 1], ids=["f16", "f32"])
@pytest.mark.parametrize("operand", ["y", "res"])
def test_persistent_1x1_variants_decline_a_y_or_res_span_past_2_gib(lib, dtype, operand):
    """span = bytes from the view's first to its last element.  2^31 - 1 and more: every hint of GEMM_HINTS refuses with
    "does not apply" (its y / res offsets are 32-bit), hints 0 and 1 accept; one vector less: the variants that take the
    problem at all still take it"""
    from tests.test_hip_fuzz import GEMM_HINTS
    es = 2 if dtype == 0 else 4
    image = 9 * 17 * 64
    sn_out = -(-(2 ** 31 - 1 - image * es) // 16) * 16 // es           # smallest vector-aligned stride with span >= 2^31 - 1
    sn_in = sn_out - 16 // es
    assert (sn_out + image) * es >= 2 ** 31 - 1 > (sn_in + image) * es

    def call(hint, sn):
        wide = _view(2, 2, 9, 17, 64, dtype, sn=sn)
        y, res = (wide, _view(3, 2, 9, 17, 64, dtype)) if operand == "y" else (_view(3, 2, 9, 17, 64, dtype), wide)
        return lambda: lib.glsdet_conv2d(C.byref(_desc(_view(0, 2, 9, 17, 64, dtype), y, 1, hint=hint, res=res)), None)

    taken = []
    for hint in GEMM_HINTS:
        rc, ops, msg = _recorded(lib, call(hint, sn_out))
        assert rc < 0 and ops == 0 and F.SPAN_TEXT in msg, "hint %d takes a %s span of 2^31 - 1 bytes or more: rc %d, %r" % (hint, operand, rc, msg)
        if _recorded(lib, call(hint, sn_in))[0] == 0:
            taken.append(hint)
    assert taken, "no persistent 1x1 variant takes this problem even below the limit: the refusals above prove nothing"
    for hint in (0, 1):
        rc, ops, msg = _recorded(lib, call(hint, sn_out))
        assert rc == 0 and ops == 1, "hint %d must take a far %s: %s" % (hint, operand, msg)
