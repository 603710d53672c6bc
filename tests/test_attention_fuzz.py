"""Differential tests of the data-dependent attention path, entry point by entry point: glsdet_attn_split, glsdet_rowsplit,
glsdet_scale_by_map, glsdet_gate (glsdet_amd/csrc/adapt.hip), glsdet_nonlocal_split (nonlocal.hip, nl_window),
glsdet_dwconv2d_dilated (dwconv.hip) and glsdet_channel_maxmean, in both engine dtypes.

Decisions and copies are compared EXACTLY with the naive reference of tests/attention_reference.py: the split on dyadic
maps whose float32 sums are order-independent (that module's docstring; tests/test_attention_reference.py holds the
integer reference against the oracle on every map used here), rowsplit and the window geometry bit for bit, the
elementwise products and the dyadic depthwise convolutions bit for bit with one rounding.  Arithmetic on continuous
operands keeps the project's existing per-op tolerances (tests/test_hip_ops.py).  Consumers take their split from a
host-written int32[4] device tensor, so the test chooses the windows, not attn_split.  No case is skipped or filtered at run
time: the preconditions are asserted when the case lists are built.

Measured on an MI355X, test_nonlocal_split_arithmetic prints over its 24 cases a relative error of the windowed
non-local block of 6.7e-08 .. 2.6e-07 in fp32 (largest: ci136-c8-n3-20.32.32-shift0) and 2.6e-04 .. 3.9e-04 in fp16
(largest: ci64-c8-n3-20.32.32-shift1), against its bounds 1e-4 / 2e-2; tests/test_nonlocal_exact.py holds the same
kernels bit for bit and to an a-priori per-element bound."""
import numpy as np
import pytest
import torch

from tests import attention_reference as R

pytestmark = pytest.mark.gpu

TOL = {"f32": 2e-5, "f16": 4e-3}            # tests/test_hip_ops.py TOL: per op, times max(1, |ref|)
NL_TOL = {"f32": 1e-4, "f16": 2e-2}         # tests/test_hip_ops.py test_nonlocal
MODES = ["f32", "f16"]
WRAP = 8192 * 256                           # the elementwise kernels cap their grid at 8192 blocks of 256 threads


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32"), "f16": Engine("f16")}


def _view(eng, a, embed=None):
    from tests.test_hip_ops import _to_view
    return _to_view(eng, torch.as_tensor(np.asarray(a, np.float32)), embed=embed)


def _rounded(a, mode):
    a = np.asarray(a, np.float32)
    with np.errstate(over="ignore"):
        return a.astype(np.float16).astype(np.float32) if mode == "f16" else a


def _get(v, c=None):
    torch.cuda.synchronize()
    return v.to_nchw(c).cpu().numpy()


def _same_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r"
                             % (what, int(bad.sum()), bad.size, i, got[i], want[i]))


def _border_intact(v, ctot):
    """an embedded view (_to_view(embed=)): everything of its buffer outside the window still holds the poison"""
    from glsdet_amd.engine import _TORCH_DT
    torch.cuda.synchronize()
    n, h, w = v.n, v.h + 2, v.w + 2
    t = v.buf.view(_TORCH_DT[v.dtype])[: n * h * w * ctot].view(n, h, w, ctot).float().cpu()
    c0 = (v.off - v.sh - v.sw) % ctot
    t[:, 1:-1, 1:-1, c0:c0 + v.c] = 7.0
    return bool((t == 7.0).all())


def _split_tensor(eng, split):
    t = torch.tensor(list(split) + [0], dtype=torch.int32, device=eng.device)
    eng._keep.append(t)
    return t


def _rel(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max()) / max(1.0, float(np.abs(ref).max()))


# =========================================================================================================== attn_split
SPLIT_CASES = R.split_cases()
SPLIT_RUNS = [(c, v) for c in SPLIT_CASES for v in (("channel0", "window") if c[1].size <= 100000 else ("channel0",))]
_EXPECT = {}


def _expected_split(case):
    if case[0] not in _EXPECT:
        _EXPECT[case[0]] = R.split_reference(case[1])
    return _EXPECT[case[0]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case,view", SPLIT_RUNS, ids=["%s-%s" % (c[0], v) for c, v in SPLIT_RUNS])
def test_attn_split_equals_the_integer_reference(engines, mode, case, view):
    """the map as channel 0 of an 8-channel tensor / as a strided window (border of 1, channels 8..15) of a larger buffer"""
    eng = engines[mode]
    name, k, g = case
    m = np.zeros((k.shape[0], 8) + k.shape[1:], np.float32)
    m[:, 0] = R.to_float(k, g)
    att = _view(eng, m, embed=(24, 8) if view == "window" else None)
    split = eng.attn_split(att)
    torch.cuda.synchronize()
    got = split.cpu().tolist()
    print("%s %s: device %s, reference %s" % (name, mode, got, _expected_split(case)))
    assert tuple(got[:3]) == _expected_split(case) and got[3] == 0


POISON_CASES = [c for c in SPLIT_CASES if c[0].startswith(("2x12x20-", "3x15x21-"))]
assert len(POISON_CASES) >= 20


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", POISON_CASES, ids=[c[0] for c in POISON_CASES])
def test_attn_split_reads_channel_0_only(engines, mode, case):
    eng = engines[mode]
    name, k, g = case
    rng = np.random.RandomState(5)
    m = rng.choice(np.array([3e4, -3e4, np.inf, -np.inf, np.nan, 1e-3], np.float32), (k.shape[0], 8) + k.shape[1:])
    m[:, 0] = R.to_float(k, g)
    split = eng.attn_split(_view(eng, m))
    torch.cuda.synchronize()
    assert tuple(split.cpu().tolist()) == _expected_split(case) + (0,)


# ============================================================================================================= rowsplit
FULL = (24, 36)                                          # the map the host-written splits refer to
HOST_SPLITS = R.host_splits(*FULL)
assert len(HOST_SPLITS) == 6


def _rowsplit_inputs(mode, n, C, H, W, seed):
    rng = np.random.RandomState(seed)
    a, b, y0 = (_rounded(rng.standard_normal((n, C, H, W)), mode) for _ in range(3))
    return a, b, y0


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided"])
@pytest.mark.parametrize("C", [8, 24, 200])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("op", [0, 1, 2, 3, 4])
def test_rowsplit_bit_for_bit(engines, mode, strided, C, shift, op):
    """every host-written split (both clamps, cyl != cyr, odd halves under shift) x every quadrant, on an output prefilled
    with a pattern: modes 0..3 overwrite all of it, mode 4 leaves it alone outside its quadrant"""
    eng = engines[mode]
    H, W = FULL[0] >> shift, FULL[1] >> shift
    a, b, y0 = _rowsplit_inputs(mode, 2, C, H, W, 100 * op + C + shift)
    emb = (C + 16, 8) if strided else None
    av, bv = _view(eng, a, emb), _view(eng, b, emb)
    split_t = _split_tensor(eng, HOST_SPLITS[0])
    for split in HOST_SPLITS:
        split_t.copy_(torch.tensor(list(split) + [0], dtype=torch.int32))
        for q in (range(4) if op >= 3 else [0]):
            yv = _view(eng, y0, emb)
            eng.rowsplit(av, bv if op == 2 else None, split_t, op, out=yv, quadrant=q, shift=shift)
            want = R.rowsplit_reference(a, b, y0, split, op, q, shift)
            _same_bits(_get(yv), want, "mode %d quadrant %d split %s shift %d" % (op, q, split, shift))
            assert not strided or _border_intact(yv, C + 16)
    _same_bits(_get(av), a, "a was written")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("split", HOST_SPLITS, ids=["%d-%d-%d" % s for s in HOST_SPLITS])
def test_rowsplit_four_merges_tile_the_map_exactly_once(engines, mode, split, shift):
    """the four mode-4 calls of NetBuilder.patch_conv_nonlocal_adapt into one buffer: every pixel comes from exactly one of
    the four sources (the buffer starts as NaN, the sources are constants 100 (q + 1) plus a per-pixel pattern, rounded to
    the storage dtype as the engine stores them: fp16 keeps only quarters above 256)"""
    eng = engines[mode]
    H, W, C = FULL[0] >> shift, FULL[1] >> shift, 24
    pattern = np.random.RandomState(3).randint(-64, 64, (2, C, H, W)).astype(np.float32) / 8
    srcs = [_rounded(pattern + 100.0 * (q + 1), mode) for q in range(4)]
    Q = _view(eng, np.full((2, C, H, W), np.nan, np.float32))
    split_t = _split_tensor(eng, split)
    for q in range(4):
        eng.rowsplit(_view(eng, srcs[q]), None, split_t, 4, out=Q, quadrant=q, shift=shift)
    member = R.membership_reference(pattern.shape, split, shift)
    assert set(np.unique(member)) == {1.0, 2.0, 3.0, 4.0}
    _same_bits(_get(Q), _rounded(pattern + 100.0 * member, mode), "merge")


@pytest.mark.parametrize("mode", MODES)
def test_rowsplit_grid_stride_loop_wraps(engines, mode):
    eng = engines[mode]
    H, W, C = 1100, 2048, 8
    assert H * W * (C // (8 if mode == "f16" else 4)) > WRAP
    rng = np.random.RandomState(9)
    a = rng.randint(-1000, 1000, (1, C, H, W)).astype(np.float32)
    y0 = np.full((1, C, H, W), -3.0, np.float32)
    split = (700, 900, 1200)
    split_t = _split_tensor(eng, split)
    yv = _view(eng, y0)
    eng.rowsplit(_view(eng, a), None, split_t, 4, out=yv, quadrant=3)
    _same_bits(_get(yv), R.rowsplit_reference(a, None, y0, split, 4, 3, 0), "wrap, mode 4")
    eng.rowsplit(_view(eng, a), None, split_t, 1, out=yv)
    _same_bits(_get(yv), R.rowsplit_reference(a, None, y0, split, 1, 0, 0), "wrap, mode 1")


# ======================================================================================================= nonlocal_split
def _nl_cases():
    """(ci, x channels, n, split, shift): every (ci, channels) pair, the other dimensions cycling so that each value of
    each meets each ci; windows from 4 x 4 (2 x 2 under shift) up to most of the map"""
    out = []
    pair = 0
    for ci in (8, 16, 64, 136):
        for cx in (8, 40, 200):
            for rep in range(2):
                out.append((ci, cx, (1, 3)[rep], HOST_SPLITS[len(out) % len(HOST_SPLITS)], (pair + rep) % 2))
            pair += 1
    assert {c[3] for c in out} == set(HOST_SPLITS) and {(c[0], c[4]) for c in out} == {(a, s) for a in (8, 16, 64, 136) for s in (0, 1)}
    return out


NL_CASES = _nl_cases()
NL_IDS = ["ci%d-c%d-n%d-%d.%d.%d-shift%d" % ((c[0], c[1], c[2]) + c[3] + (c[4],)) for c in NL_CASES]


def _nl_run(eng, mode, x, tpg, wout, bout, split, shift, ci):
    xv = _view(eng, x)
    tv = [_view(eng, t) for t in tpg]
    wd = [eng.upload(torch.as_tensor(w)) for w in wout]
    bd = [eng.upload(torch.as_tensor(b)) for b in bout]
    out = _view(eng, np.full(x.shape, np.nan, np.float32))
    eng.nonlocal_split(xv, tv, ci, wd, bd, out, _split_tensor(eng, split), shift)
    return _get(out)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", NL_CASES, ids=NL_IDS)
def test_nonlocal_split_window_geometry_is_exact(engines, mode, case):
    """conv_out weights zero, bias q + 1: out - x is the window-membership map, exactly, and no pixel keeps its NaN"""
    ci, cx, n, split, shift = case
    H, W = FULL[0] >> shift, FULL[1] >> shift
    rng = np.random.RandomState(ci + cx)
    x = rng.randint(-32, 32, (n, cx, H, W)).astype(np.float32) / 8
    tpg = [_rounded(rng.standard_normal((n, 3 * ci, H, W)), mode) for _ in range(4)]
    wout = [np.zeros((cx, ci), np.float32) for _ in range(4)]
    bout = [np.full(cx, q + 1, np.float32) for q in range(4)]
    got = _nl_run(engines[mode], mode, x, tpg, wout, bout, split, shift, ci)
    _same_bits(got - x, R.membership_reference(x.shape, split, shift), "window membership")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", NL_CASES, ids=NL_IDS)
def test_nonlocal_split_arithmetic(engines, mode, case):
    """random theta | phi | g handed in directly (the only roundings are the kernel's own) against the float64 definition,
    within the tolerance of test_hip_ops.test_nonlocal"""
    ci, cx, n, split, shift = case
    H, W = FULL[0] >> shift, FULL[1] >> shift
    rng = np.random.RandomState(7 * ci + cx)
    x = _rounded(rng.standard_normal((n, cx, H, W)), mode)
    tpg = []
    for q in range(4):
        theta = rng.uniform(-1, 1, (n, ci, H, W))
        phi_g = rng.uniform(0, 1, (n, 2 * ci, H, W))                     # a Gram of mean N / 4: the 1 / N matters
        tpg.append(_rounded(np.concatenate([theta, phi_g], 1), mode))
    wout = [(rng.uniform(-1, 1, (cx, ci)) * 4 / ci).astype(np.float32) for _ in range(4)]
    bout = [rng.standard_normal(cx).astype(np.float32) for _ in range(4)]
    got = _nl_run(engines[mode], mode, x, tpg, wout, bout, split, shift, ci)
    ref = R.nonlocal_windows_reference(x, tpg, wout, bout, split, shift)
    assert not np.isnan(got).any()
    term = ref - x                                                       # what the block adds, without its bias
    for q in range(4):
        r, c = R.quadrant_slices(split, shift, q)
        term[:, :, r, c] -= bout[q][None, :, None, None]
    err = _rel(got, ref)
    print("nonlocal_split %s %s: rel err %.3e, largest non-local term %.2f" % (NL_IDS[NL_CASES.index(case)], mode, err, np.abs(term).max()))
    assert np.abs(term).max() > 0.25                                     # the block contributes: a wrong 1 / N is seen
    assert err <= NL_TOL[mode]


# ================================================================================================== scale_by_map / gate
def _special_pairs():
    """(a, b) whose product is a signed zero, an fp16 subnormal (exact and rounded), at and over the fp16 overflow edge"""
    return np.array([(0.0, -1.0), (-0.0, 5.0), (-0.0, -0.0), (2.0 ** -10, 2.0 ** -12), ((1 + 2.0 ** -10) * 2.0 ** -12, 2.0 ** -11),
                     (3 * 2.0 ** -13, 2.0 ** -12), (300.0, 300.0), (-300.0, 300.0), (65504.0, 1.0), (255.875, 256.0),
                     (255.9375, 256.0), (2.0 ** -14, 0.5), (2.0 ** -24, 0.5), (-2.0 ** -24, 0.5)], np.float32).T


def _elementwise_inputs(mode, n, C, H, W, seed):
    rng = np.random.RandomState(seed)
    a = rng.standard_normal((n, C, H, W)).astype(np.float32)
    b = rng.standard_normal((n, C, H, W)).astype(np.float32)
    m = rng.uniform(0, 1, (n, 1, H, W)).astype(np.float32)
    sa, sb = _special_pairs()
    k = len(sa)
    a[0, 0].flat[:k], b[0, 0].flat[:k] = sa, sb                          # gate mode 1
    a[0, 1].flat[:k], m[0, 0].flat[:k] = sa, sb                          # scale_by_map: channel 1 times the map
    return _rounded(a, mode), _rounded(b, mode), _rounded(m, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, 24, 200])
@pytest.mark.parametrize("variant", ["dense", "strided", "y_is_a", "y_is_b"])
def test_gate_product_bit_for_bit(engines, mode, C, variant):
    eng = engines[mode]
    a, b, _ = _elementwise_inputs(mode, 2, C, 9, 11, C)
    emb = (C + 16, 8) if variant == "strided" else None
    av, bv = _view(eng, a, emb), _view(eng, b, emb)
    yv = {"y_is_a": av, "y_is_b": bv}.get(variant) or _view(eng, np.full(a.shape, np.nan, np.float32), emb)
    eng.gate(av, bv, None, out=yv)
    _same_bits(_get(yv), R.gate_reference(a, b, None, mode), "a * b")
    assert emb is None or _border_intact(yv, C + 16)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, 24, 200])
@pytest.mark.parametrize("variant", ["dense", "strided"])
def test_scale_by_map_bit_for_bit(engines, mode, C, variant):
    eng = engines[mode]
    a, _, m = _elementwise_inputs(mode, 2, C, 9, 11, C + 1)
    emb = (C + 16, 8) if variant == "strided" else None
    m8 = np.concatenate([m, np.full((2, 7, 9, 11), 1e4, np.float32)], 1)           # only channel 0 is the map
    yv = _view(eng, np.full(a.shape, np.nan, np.float32), emb)
    eng.scale_by_map(_view(eng, a, emb), _view(eng, m8, (24, 8) if emb else None), out=yv)
    _same_bits(_get(yv), R.scale_by_map_reference(a, m, mode), "map * x")
    assert emb is None or _border_intact(yv, C + 16)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("op", ["gate", "scale_by_map"])
def test_elementwise_grid_stride_loops_wrap(engines, mode, op):
    eng = engines[mode]
    H, W, C = 1100, 2048, 8
    assert H * W * (C // (8 if mode == "f16" else 4)) > WRAP
    a, b, m = _elementwise_inputs(mode, 1, C, H, W, 77)
    yv = _view(eng, np.full(a.shape, np.nan, np.float32))
    if op == "gate":
        eng.gate(_view(eng, a), _view(eng, b), None, out=yv)
        _same_bits(_get(yv), R.gate_reference(a, b, None, mode), "wrap")
    else:
        eng.scale_by_map(_view(eng, a), _view(eng, m), out=yv)
        _same_bits(_get(yv), R.scale_by_map_reference(a, m, mode), "wrap")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, 24, 200])
@pytest.mark.parametrize("variant", ["dense", "strided", "y_is_a", "y_is_b"])
def test_gate_mix_on_dyadic_operands_bit_for_bit(engines, mode, C, variant):
    """a, b = k / 8 (|k| <= 255), g0 != g1 = j / 16: a g0 + b g1 is an integer of 1 / 128 units below 2^14 -- exact in
    float32 with or without a contracted multiply-add, one rounding on an fp16 store.  A swap of g0 / g1 or a second read
    of map channel 0 changes the value"""
    eng = engines[mode]
    rng = np.random.RandomState(C)
    a = rng.randint(-255, 256, (2, C, 9, 11)).astype(np.float32) / 8
    b = rng.randint(-255, 256, (2, C, 9, 11)).astype(np.float32) / 8
    j0 = rng.randint(0, 17, (2, 1, 9, 11))
    j1 = (j0 + rng.randint(1, 17, (2, 1, 9, 11))) % 17
    assert (j0 != j1).all() and int(np.abs(a * 8).max() * 16 * 2) < R.LIMIT
    m = np.concatenate([j0, j1], 1).astype(np.float32) / 16
    emb = (C + 16, 8) if variant == "strided" else None
    av, bv = _view(eng, a, emb), _view(eng, b, emb)
    yv = {"y_is_a": av, "y_is_b": bv}.get(variant) or _view(eng, np.full(a.shape, np.nan, np.float32), emb)
    eng.gate(av, bv, _view(eng, m, (24, 8) if emb else None), out=yv)
    _same_bits(_get(yv), R.gate_reference(a, b, m, mode), "a g0 + b g1")
    assert emb is None or _border_intact(yv, C + 16)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("C", [8, 24, 200])
def test_gate_mix_on_continuous_operands_is_bounded(engines, mode, C):
    """|err| <= 2 * 2^-23 (|a g0| + |b g1|) + half an ulp of the storage dtype, per element"""
    eng = engines[mode]
    rng = np.random.RandomState(C + 5)
    a, b = (_rounded(rng.standard_normal((2, C, 9, 11)), mode) for _ in range(2))
    m = _rounded(rng.uniform(0, 1, (2, 2, 9, 11)), mode)
    got = _get(eng.gate(_view(eng, a), _view(eng, b), _view(eng, m)))
    ref = np.asarray(a, np.float64) * m[:, 0:1] + np.asarray(b, np.float64) * m[:, 1:2]
    excess = np.abs(got - ref) - R.gate_bound(a, b, m, mode)
    print("gate mix %s C=%d: max |err| %.3e, largest excess over the bound %.3e" % (mode, C, np.abs(got - ref).max(), excess.max()))
    assert (excess <= 0).all()


# =============================================================================================================== dwconv
def _dw_run(eng, mode, x, w, scale, bias, stride, pad, dil, act, strided):
    C = x.shape[1]
    pk = eng.pack_dw(torch.as_tensor(w), torch.as_tensor(scale), torch.as_tensor(bias), C)
    R_, S = w.shape[2:]
    ho = (x.shape[2] + 2 * pad - dil * (R_ - 1) - 1) // stride + 1
    wo = (x.shape[3] + 2 * pad - dil * (S - 1) - 1) // stride + 1
    assert ho >= 1 and wo >= 1
    emb = (C + 16, 8) if strided else None
    yv = _view(eng, np.full((x.shape[0], C, ho, wo), np.nan, np.float32), emb)
    eng.dwconv(_view(eng, x, emb), pk, stride, pad, act, out=yv, dilation=dil)
    got = _get(yv)
    assert emb is None or _border_intact(yv, C + 16)
    return got


def _dw_pads(k, dil):
    full = dil * (k - 1) // 2
    return [0, k // 2, full, full + 1]


DW_GEOM = [(k, s, d) for k in (3, 5, 7) for s in (1, 2, 3) for d in (1, 2, 3)]
DW_HW = (21, 23)                       # odd, and 21 >= the 19 taps' reach of 7 x 7 dilation 3 without padding
assert all(DW_HW[0] - d * (k - 1) - 1 >= 0 for k, s, d in DW_GEOM)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,stride,dil", DW_GEOM)
def test_dwconv_dyadic_bit_for_bit(engines, mode, k, stride, dil):
    """all four paddings (0, k // 2, dilation (k - 1) / 2, one more), C cycling through 8 / 24 / 200, `none` and `relu`,
    dense and strided: every float32 accumulation is exact, the store rounds once"""
    i = DW_GEOM.index((k, stride, dil))
    for j, pad in enumerate(_dw_pads(k, dil)):
        C = (8, 24, 200)[(i + j) % 3]
        act = ("none", "relu")[(i + j) % 2]
        x, w, scale, bias = R.dwconv_dyadic(C, DW_HW[0], DW_HW[1], k, k, 31 * i + j)
        got = _dw_run(engines[mode], mode, x, w, scale, bias, stride, pad, dil, act, strided=(i + j) % 4 < 2)
        _same_bits(got, R.dwconv_reference(x, w, scale, bias, stride, pad, dil, act, mode), "C %d pad %d %s" % (C, pad, act))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k,stride,dil", DW_GEOM)
def test_dwconv_lrelu_silu_on_continuous_operands(engines, mode, k, stride, dil):
    i = DW_GEOM.index((k, stride, dil))
    for j, pad in enumerate(_dw_pads(k, dil)):
        C = (8, 24, 200)[(i + j + 1) % 3]
        act = ("lrelu", "silu")[(i + j) % 2]
        rng = np.random.RandomState(17 * i + j)
        x = _rounded(rng.standard_normal((2, C) + DW_HW), mode)
        w = _rounded(rng.standard_normal((C, 1, k, k)) * 0.2, mode)
        scale, bias = rng.uniform(0.5, 1.5, C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
        got = _dw_run(engines[mode], mode, x, w, scale, bias, stride, pad, dil, act, strided=(i + j) % 4 >= 2)
        ref = R.dwconv_reference(x, w, scale, bias, stride, pad, dil, act, mode).astype(np.float64)
        err = _rel(got, ref)
        assert err <= TOL[mode], "C %d pad %d %s: %.3e" % (C, pad, act, err)


DW_ODD = [
    # R, S, H, W, stride, pad, dil: rectangular taps, and inputs smaller than the dilated kernel's reach (output 1 x 1)
    (3, 7, 13, 17, 1, 3, 1), (7, 1, 13, 17, 2, 3, 2), (1, 5, 9, 16, 1, 0, 3), (5, 3, 11, 15, 3, 2, 1),
    (3, 3, 5, 5, 1, 1, 3), (3, 3, 5, 6, 2, 1, 3), (7, 7, 3, 3, 1, 9, 3), (5, 5, 1, 1, 1, 2, 1),
]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", DW_ODD, ids=["%dx%d-%dx%d-s%d-p%d-d%d" % g for g in DW_ODD])
def test_dwconv_rectangular_taps_and_tiny_inputs_bit_for_bit(engines, mode, geom):
    R_, S, H, W, stride, pad, dil = geom
    for C, act, strided in ((8, "none", False), (24, "relu", True), (200, "none", True)):
        x, w, scale, bias = R.dwconv_dyadic(C, H, W, R_, S, H * W + C)
        got = _dw_run(engines[mode], mode, x, w, scale, bias, stride, pad, dil, act, strided)
        _same_bits(got, R.dwconv_reference(x, w, scale, bias, stride, pad, dil, act, mode), "C %d" % C)


def test_the_tiny_dwconv_cases_do_reach_one_output_pixel():
    """(no GPU work: a property of the case list)"""
    outs = {((H + 2 * p - d * (R_ - 1) - 1) // s + 1, (W + 2 * p - d * (S - 1) - 1) // s + 1) for R_, S, H, W, s, p, d in DW_ODD
            if H < d * (R_ - 1) + 1 and W < d * (S - 1) + 1}
    assert (1, 1) in outs and any(R_ != S for R_, S, *_ in DW_ODD)


@pytest.mark.parametrize("mode", MODES)
def test_dwconv_grid_stride_loop_wraps(engines, mode):
    H, W, C = 1100, 2048, 8
    assert H * W * (C // (8 if mode == "f16" else 4)) > WRAP
    x, w, scale, bias = R.dwconv_dyadic(C, H, W, 3, 3, 1, n=1)
    got = _dw_run(engines[mode], mode, x, w, scale, bias, 1, 1, 1, "none", False)
    _same_bits(got, R.dwconv_reference(x, w, scale, bias, 1, 1, 1, "none", mode), "wrap")


# ======================================================================================================= channel_maxmean
MAXMEAN_MEAN_TOL = {"f32": 1e-6, "f16": 2e-3}           # tests/test_attention.py test_channel_maxmean; tests/test_far_addresses.py imports it
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,negative", [((1, 8, 200, 200), False), ((2, 64, 9, 11), True), ((2, 512, 9, 11), False),
                                            ((1, 512, 40, 30), True)], ids=["wrap", "all_negative", "c512", "c512_negative"])
def test_channel_maxmean_wrapping_negative_and_wide(engines, mode, shape, negative):
    """one wave per pixel, at most 8192 * 4 waves: 200 x 200 pixels wrap.  Max exact (an all-negative pixel shows the max's
    initial value), mean within the tolerance of tests/test_attention.py test_channel_maxmean"""
    eng = engines[mode]
    assert shape != (1, 8, 200, 200) or shape[2] * shape[3] > 8192 * 4
    rng = np.random.RandomState(shape[1])
    x = rng.standard_normal(shape).astype(np.float32)
    if negative:
        x = -np.abs(x) - 0.5
    x = _rounded(x, mode)
    out = eng.channel_maxmean(_view(eng, x, embed=(shape[1] + 16, 8)))
    got = _get(out, 8)
    assert np.array_equal(got[:, 0], x.max(1))
    assert np.abs(got[:, 1] - x.astype(np.float64).mean(1)).max() <= MAXMEAN_MEAN_TOL[mode]
    assert np.abs(got[:, 2:]).max() == 0.0
