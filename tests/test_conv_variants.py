"""CPU-only: WHICH kernel every tile_hint selects, pinned row by row.

The exact-arithmetic suites (test_conv_exact, test_hip_fuzz, test_csp_fused) pin what every conv variant computes; a
change that routed, say, hint 9 to the 64-row kernel would pass them all and only cost speed.  Recording into a plan
never touches the device, so the op name each (entry point, problem, hint) records -- or its refusal -- is compared here
with tests/golden/conv_variant_table.json (tools/make_conv_variant_table.py)."""
import json
import os
import re

import pytest

from tools import make_conv_variant_table as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the tiles / variants that are compiled (csrc/conv.hip, conv_gemm.hip, conv_halo.hip)
IGEMM_TILES = {"conv_igemm": {(128, 128), (64, 128), (32, 128), (64, 64), (128, 256)},
               "conv_igemm_multi": {(128, 128), (64, 128), (64, 64)},
               "conv_igemm_batch": {(128, 128), (64, 128), (64, 64)}}
GEMM_VARIANTS = {(64, 64, 4, 128, False), (128, 64, 3, 128, False), (64, 128, 3, 128, False), (128, 128, 3, 128, False),
                 (128, 128, 4, 64, False), (32, 128, 3, 128, False), (64, 128, 3, 128, True), (128, 64, 4, 128, True),
                 (64, 64, 4, 128, True), (32, 128, 4, 128, True), (128, 128, 3, 128, True), (64, 64, 6, 64, False),
                 (128, 64, 4, 64, False)}
GEMM1_TILES = {(64, 64), (64, 128), (32, 128)}
HALO_TILES = {(8, 16), (10, 12), (6, 21)}
RING8_TILES = {(8, 32), (10, 24), (6, 42)}


@pytest.fixture(scope="module")
def table():
    import __graft_entry__ as g
    g.build()
    with open(os.path.join(ROOT, "tests", "golden", "conv_variant_table.json")) as f:
        want = json.load(f)
    return want, T.rows()


def test_the_table_covers_every_hint_of_the_fuzz_suite():
    from tests import test_hip_fuzz          # (importing it touches no device)
    assert set(test_hip_fuzz.HINTS) <= set(T.HINTS)
    assert {6, 7, 14, 15, 32, 0x10d, 0x30a, (16 << 16) | 64} <= set(T.HINTS)


def test_every_hint_selects_the_recorded_variant(table):
    want, got = table
    assert len(got) >= 1000
    want = {(case, hint): op for case, ops in want.items() for op, hints in ops.items() for hint in hints}
    assert len(want) == len(got), "the fixture is not of this tool's case list"
    bad = []
    for entry, case, hint, op in got:
        w = want[(entry + " " + case, hint)]
        if w != ("REFUSED" if op.startswith("REFUSED") else op):       # refusals: the outcome is pinned, not the wording
            bad.append("%s %s hint %#x: want %r, got %r" % (entry, case, hint, w, op))
    assert not bad, "\n".join(bad)


def test_undocumented_hints_are_refused_when_the_op_is_built(table):
    for entry, case, hint, op in table[1]:
        if hint in T.UNDOCUMENTED:
            assert op.startswith("REFUSED"), (entry, case, hex(hint), op)
        if hint in (6, 7):
            assert op.startswith("REFUSED") and ("no longer exist" in op or entry != "conv2d"), (entry, case, hint, op)


def _check_name(op):
    """an accepted row must name a kernel that is compiled: nothing is recorded that can only fail at launch"""
    m = re.match(r"(conv_igemm(?:_multi|_batch)?)(?:\[\d+\])?<f\d+,f\d+,(\d+)x(\d+),kb(\d+)>", op)
    if m:
        return (int(m.group(2)), int(m.group(3))) in IGEMM_TILES[m.group(1)] and int(m.group(4)) in (64, 128)
    m = re.match(r"conv_gemm<f\d+,f\d+,(\d+)x(\d+),ns(\d+),kb(\d+)(,wres)?>", op)
    if m:
        return tuple(int(v) for v in m.groups()[:4]) + (m.group(5) is not None,) in GEMM_VARIANTS
    m = re.match(r"conv_gemm1<f\d+,f\d+,(\d+)x(\d+)>", op)
    if m:
        return (int(m.group(1)), int(m.group(2))) in GEMM1_TILES
    m = re.match(r"conv_halo_ring8(?:_k64)?<f\d+,128x(\d+)x(\d+)>", op)
    if m:
        return (int(m.group(1)), int(m.group(2))) in RING8_TILES
    m = re.match(r"conv_halo(?:_wp|_ring|_ring_k64|_ring_k64_s2)?(?:_s2)?(?:_multi\[\d+\])?<f\d+,(\d+)x(\d+)x(\d+)>", op)
    if m:
        return int(m.group(1)) in (64, 128) and (int(m.group(2)), int(m.group(3))) in HALO_TILES
    m = re.match(r"conv1x1_ws<f\d+,(\d+)x64>", op)
    if m:
        return int(m.group(1)) in (64, 128)
    return False                        # a kernel family this test does not know


def test_no_accepted_row_names_a_kernel_that_is_not_compiled(table):
    bad = ["%s %s hint %#x: %s" % r for r in table[1] if not r[3].startswith("REFUSED") and not _check_name(r[3])]
    assert not bad, "\n".join(bad)
    assert _check_name("conv_igemm<f16,f16,64x64,kb128> 1x1 s1 cin64 cout64") and not _check_name("conv_igemm<f16,f16,16x64,kb128> x")
    assert not _check_name("conv_igemm_multi[4]<f16,f16,128x256,kb128> x")
