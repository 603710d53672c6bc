"""CPU-only: the registry of tests/replay_cases.py is complete and every case records a well-formed op; the recording
state of glsdet_plan (begin / end / destroy, set_branch).  Recording never touches the device: every pointer here is
fabricated (256-byte aligned, with alloc_lo / alloc_hi around the views)."""
import ctypes as C
import math

import pytest

KINDS = range(0, 9)                     # include/glsdet_hip.h, glsdet_plan_op_info: 0 conv .. 8 proxy scores


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def cases(lib):
    from tests import replay_cases as RC
    return [c.bind_fake(i) for i, c in enumerate(RC.cases())]


def _info(lib, plan):
    out = []
    for i in range(lib.glsdet_plan_num_ops(plan)):
        kind, flops, nbytes, name = C.c_int32(), C.c_double(), C.c_double(), C.create_string_buffer(192)
        assert lib.glsdet_plan_op_info(plan, i, C.byref(kind), C.byref(flops), C.byref(nbytes), name, 192) == 0
        out.append((kind.value, flops.value, nbytes.value, name.value))
    return out


def test_the_registry_holds_exactly_the_launching_exports(lib):
    """_SIGS minus the fixed exclusion list: an export added without a case fails here"""
    from tests import replay_cases as RC
    assert sorted(RC.registry()) == RC.required_exports()
    assert len(RC.EXCLUDED) == 12 and len(RC.required_exports()) >= 60


def test_the_shape_dependent_ops_have_a_second_case(lib):
    from tests import replay_cases as RC
    reg = RC.registry()
    for name in ("soft_nms", "nonlocal_mfma", "lvc_encode", "window_attention", "csp_fused", "bottleneck"):
        assert len(reg["glsdet_" + name]) >= 2, name
    assert len({c.key for c in RC.cases()}) == len(RC.cases())


def test_every_case_has_a_reference_or_says_why_not(lib):
    from tests import replay_cases as RC
    for c in RC.cases():
        assert c.has_want or c.note, c.key
    assert sum(c.has_want for c in RC.cases()) >= 45


def test_every_case_has_two_data_sets_and_the_stateful_ones_three(lib):
    from tests import replay_cases as RC
    for c in RC.cases():
        assert c.n_sets >= 2, c.key
        assert any(b.role in ("out", "inout") for b in c.bufs.values()), c.key
        if c.key.split("@")[0] in RC.STATEFUL:
            assert c.n_sets == 3, c.key


def test_every_case_records_a_well_formed_op_that_outlives_its_host_arguments(lib, cases):
    for c in cases:
        plan = lib.glsdet_plan_create()
        try:
            assert lib.glsdet_plan_begin(plan) == 0
            try:
                c.record(lib)
            finally:
                assert lib.glsdet_plan_end(plan) == 0
            ops = _info(lib, plan)
            assert len(ops) >= 1, c.key
            for kind, flops, nbytes, name in ops:
                assert kind in KINDS, (c.key, kind, name)
                assert math.isfinite(flops) and flops >= 0 and math.isfinite(nbytes) and nbytes >= 0, (c.key, flops, nbytes)
                assert 0 < len(name) < 160, (c.key, name)
            c.destroy_host_args()
            assert not c.kept
            assert _info(lib, plan) == ops, c.key
        finally:
            lib.glsdet_plan_destroy(plan)


def test_destroy_host_args_overwrites_what_was_passed(lib, cases):
    c = [q for q in cases if q.key == "yolox_decode_ex"][0]
    plan = lib.glsdet_plan_create()
    assert lib.glsdet_plan_begin(plan) == 0
    c.record(lib)
    assert lib.glsdet_plan_end(plan) == 0
    kept = list(c.kept)
    assert len(kept) == 2 and c.destroy_host_args() == 2                       # the level views and the strides
    for obj in kept:
        assert bytes(C.string_at(C.addressof(obj), C.sizeof(obj))) == b"\xA5" * C.sizeof(obj)
    lib.glsdet_plan_destroy(plan)


# ------------------------------------------------------------------------------------------------------ recording state
def test_a_second_plan_cannot_begin_while_one_records_and_only_the_recording_plan_can_end(lib, cases):
    a, b = lib.glsdet_plan_create(), lib.glsdet_plan_create()
    try:
        assert lib.glsdet_plan_begin(a) == 0
        assert lib.glsdet_plan_begin(b) == -1 and b"already recording" in lib.glsdet_last_error()
        assert lib.glsdet_plan_end(b) == -1 and b"not the one" in lib.glsdet_last_error()
        cases[1].record(lib)                                                   # still recorded into a
        cases[1].destroy_host_args()
        assert lib.glsdet_plan_num_ops(a) == 1 and lib.glsdet_plan_num_ops(b) == 0
        assert lib.glsdet_plan_end(a) == 0
        assert lib.glsdet_plan_end(a) == -1
    finally:
        lib.glsdet_plan_destroy(a)
        lib.glsdet_plan_destroy(b)


def test_destroying_the_recording_plan_ends_the_recording(lib):
    a, b = lib.glsdet_plan_create(), lib.glsdet_plan_create()
    assert lib.glsdet_plan_begin(a) == 0
    lib.glsdet_plan_destroy(a)
    try:
        assert lib.glsdet_plan_begin(b) == 0                                   # nothing is recording any more
        assert lib.glsdet_plan_end(b) == 0
    finally:
        lib.glsdet_plan_destroy(b)


def test_set_branch_range_and_the_join_op(lib, cases):
    """recording level only: no plan with a non-zero branch is replayed here"""
    c = cases[1]
    assert lib.glsdet_plan_set_branch(-1) == -1 and lib.glsdet_plan_set_branch(9) == -1
    assert b"not in [0,8]" in lib.glsdet_last_error()
    plan = lib.glsdet_plan_create()
    try:
        for b in (1, 8, 0, 0):                                                 # outside a recording: no join anywhere
            assert lib.glsdet_plan_set_branch(b) == 0
        assert lib.glsdet_plan_begin(plan) == 0
        try:
            assert lib.glsdet_plan_set_branch(0) == 0                          # 0 -> 0: not a return
            c.record(lib)
            for b in (1, 2):
                assert lib.glsdet_plan_set_branch(b) == 0
                c.record(lib)
            assert lib.glsdet_plan_set_branch(0) == 0                          # the one return to branch 0
            assert lib.glsdet_plan_set_branch(0) == 0
            c.record(lib)
        finally:
            assert lib.glsdet_plan_set_branch(0) == 0
            assert lib.glsdet_plan_end(plan) == 0
        c.destroy_host_args()
        ops = _info(lib, plan)
        assert [o[3] for o in ops].count(b"join") == 1 and len(ops) == 5
        assert ops[3][3] == b"join" and ops[3][0] == -1
        assert lib.glsdet_plan_set_branch(3) == 0 and lib.glsdet_plan_set_branch(0) == 0
        assert len(_info(lib, plan)) == 5                                      # outside a recording: nothing is appended
    finally:
        assert lib.glsdet_plan_set_branch(0) == 0
        lib.glsdet_plan_destroy(plan)
