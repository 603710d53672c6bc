"""Differential edge tests of the 16-byte-per-lane helpers (glsdet_amd/csrc/misc.hip, resdet.hip) against the plain
references of tests/helper_reference.py: max pools, the fused SPP pools, Focus / NCHW packing, nearest resampling,
upsample-add, copy_many / transpose_many, GroupNorm (single and multi-set) and the MPHead proxy scores.

The harness is that of tests/test_conv_exact.py (`Placed`):

  * operands are channel slices of wider buffers with a one-pixel border, strided in n, h and w;
  * the destination allocation is filled with a sentinel bit pattern before the call and compared WHOLE afterwards:
    everything outside the output window must keep its bits;
  * sources are surrounded by a poison that would change the answer if read: +65504 around pool inputs (it wins every
    maximum), NaN elsewhere;
  * comparisons are bit for bit, except GroupNorm on generic data (the bound B derived in helper_reference.groupnorm_ref,
    + half an fp16 ulp in fp16 storage) and the proxy scores (the project's per-op bar 2e-5 * max(1, |want|)).

tests/test_helper_reference.py proves on the CPU that the data of these cases tells each plausible mistake from the
right answer."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helper_reference as R
from tests.test_conv_exact import NAN, SENTINEL, Placed, _bits, _image, _scratch, _FT, _IT

pytestmark = pytest.mark.gpu

MODES = ["f16", "f32"]
POISON = {"f16": 0x7BFF, "f32": 0x477FE000}              # +65504: larger than every pooled value
_ALL = slice(None)


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32"), "f16": Engine("f16")}


def _src(eng, x, dt, fill, kind="ring"):
    n, c, h, w = x.shape
    return Placed(eng, kind, n, h, w, c, dt, fill).put(x).upload()


def _dst(eng, shape, dt, kind="window"):
    n, c, h, w = shape
    return Placed(eng, kind, n, h, w, c, dt, SENTINEL[dt]).upload()


def _values(p, index=None):
    """the view's current device content as float64 NCHW + its raw bits (NHWC)"""
    torch.cuda.synchronize()
    got = p.full.buf.view({"f16": torch.int16, "f32": torch.int32}[p.dt]).cpu().numpy()
    bits = np.ascontiguousarray(p.grid(got)[index or p.index])
    return bits.view(_FT[p.dt]).astype(np.float64).transpose(0, 3, 1, 2), bits


def _dev(eng, a):
    return eng.upload(torch.from_numpy(np.asarray(a, np.float32)))


def _check(failures, what, bad):
    if bad:
        failures.append("%s: %s" % (what, bad))


# ================================================================================================================ pools
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("k", R.MAXPOOL_KS)
def test_maxpool_bit_for_bit_on_maps_smaller_than_the_window(engines, mode, k):
    eng, failures = engines[mode], []
    for (h, w) in R.MAXPOOL_MAPS:
        for c in R.POOL_CS:
            with _scratch(eng):
                x = R.pool_data((2, c, h, w), mode, k, h, w, c)
                src, dst = _src(eng, x, mode, POISON[mode]), _dst(eng, x.shape, mode)
                eng.maxpool(src.view, k, out=dst.view)
                _check(failures, "%dx%d c%d" % (h, w, c), dst.mismatch(_bits(R.maxpool_ref(x, k), mode)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("c", R.POOL_CS)
def test_spp_pools_equal_three_direct_pools_inside_one_concat_buffer(engines, mode, c):
    """x and the three outputs are channel slices of ONE [x | p5 | p9 | p13] buffer with a +65504 border"""
    eng, failures = engines[mode], []
    for h in R.SPP_HS:
        for w in R.SPP_WS:
            with _scratch(eng):
                x = R.pool_data((2, c, h, w), mode, 5, h, w, c)
                buf = Placed(eng, "dense", 2, h + 2, w + 2, 4 * c, mode, POISON[mode])
                inner = (_ALL, slice(1, h + 1), slice(1, w + 1))
                buf.put(x, inner + (slice(0, c),))
                buf.grid(buf.host)[inner + (slice(c, 4 * c),)] = SENTINEL[mode]
                buf.upload()
                v = buf.full.window(1, h + 1, 1, w + 1)
                eng.spp_pools(v.channels(0, c), v.channels(c, 2 * c), v.channels(2 * c, 3 * c), v.channels(3 * c, 4 * c))
                want = np.concatenate(R.spp_ref(x), 1)
                _check(failures, "%dx%d" % (h, w), buf.mismatch(_bits(want, mode), inner + (slice(c, 4 * c),)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("ksp", R.POOL2D_KSP, ids=lambda t: "k%d_s%d_p%d" % t)
def test_pool2d_bit_for_bit(engines, mode, ksp):
    k, s, p = ksp
    eng, failures = engines[mode], []
    for h in R.pool2d_extents(k, p):
        for w in R.pool2d_extents(k, p):
            with _scratch(eng):
                x = R.pool_data((2, 8, h, w), mode, k, s, p, h, w)
                want = R.pool2d_ref(x, k, s, p)
                src, dst = _src(eng, x, mode, POISON[mode]), _dst(eng, want.shape, mode)
                eng.pool2d(src.view, k, s, p, out=dst.view)
                _check(failures, "%dx%d" % (h, w), dst.mismatch(_bits(want, mode)))
    assert not failures, "\n".join(failures)


# ============================================================================================================== packing
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.FOCUS_CASES, ids=lambda c: "cin%d_c%d_%s" % c)
def test_focus_pack_general_and_fast_path(engines, mode, case):
    cin, cy, kind = case
    eng, failures = engines[mode], []
    for H in R.FOCUS_HW:
        for W in R.FOCUS_HW:
            with _scratch(eng):
                img = R.image_data((2, cin, H, W), cin, cy, H, W)
                want = _bits(R.focus_ref(img, cy, mode), mode)
                if kind == "slice48":
                    dst = Placed(eng, "dense", 2, H // 2, W // 2, 48, mode, SENTINEL[mode]).upload()
                    view, index = dst.full.channels(16, 32), (_ALL, _ALL, _ALL, slice(16, 32))
                else:
                    dst = _dst(eng, (2, cy, H // 2, W // 2), mode)
                    view, index = dst.view, None
                eng.focus_pack(_image(eng, img), out=view)
                _check(failures, "%dx%d" % (H, W), dst.mismatch(want, index))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("cin", R.NCHW_CINS)
def test_nchw_pack_zero_fills_a_wider_strided_destination(engines, mode, cin):
    eng, failures = engines[mode], []
    cy = R.ceil_to(cin, 8) + 8
    for (h, w) in ((1, 1), (5, 7), (17, 23)):
        with _scratch(eng):
            img = R.image_data((2, cin, h, w), cin, h, w)
            dst = _dst(eng, (2, cy, h, w), mode)
            eng.nchw_pack(_image(eng, img), out=dst.view)
            _check(failures, "%dx%d" % (h, w), dst.mismatch(_bits(R.nchw_pack_ref(img, cy, mode), mode)))
    assert not failures, "\n".join(failures)


# =================================================================================================== nearest resampling
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("factor", R.RESAMPLE_FACTORS)
def test_resample_every_factor(engines, mode, factor):
    eng, failures = engines[mode], []
    for (h, w) in R.RESAMPLE_MAPS:
        with _scratch(eng):
            x = R.plain_data((2, 24, h, w), mode, factor, h, w)
            want = R.resample_ref(x, factor)
            src, dst = _src(eng, x, mode, NAN[mode]), _dst(eng, want.shape, mode)
            eng.resample(src.view, factor, out=dst.view)
            _check(failures, "%dx%d" % (h, w), dst.mismatch(_bits(want, mode)))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.UPSAMPLE_CASES, ids=lambda c: "h%dto%d_w%dto%d" % (c[0] + c[1]))
def test_upsample_add_one_rounding_and_the_float_nearest_index(engines, mode, case):
    hp, wp = case
    eng = engines[mode]
    with _scratch(eng):
        coarse = R.updown_data((2, 16, hp[0], wp[0]), mode, 1, hp[0], wp[0])
        fine = R.updown_data((2, 16, hp[1], wp[1]), mode, 2, hp[1], wp[1])
        cv = _src(eng, coarse, mode, NAN[mode])
        fv = Placed(eng, "window", 2, hp[1], wp[1], 16, mode, SENTINEL[mode]).put(fine).upload()
        eng.upsample_add(cv.view, fv.view)
        bad = fv.mismatch(_bits(R.upsample_add_ref(fine, coarse, mode), mode))
        assert not bad, bad


# =============================================================================================================== copies
def _copy_pairs(eng, mode, extents, c=24):
    srcs, dsts, wants = [], [], []
    for i, (n, h, w) in enumerate(extents):
        x = R.plain_data((n, c, h, w), mode, 40, i, n, h, w)
        srcs.append(_src(eng, x, mode, NAN[mode]))
        dsts.append(_dst(eng, x.shape, mode))
        wants.append(_bits(R.copy_ref(x), mode))
    return srcs, dsts, wants


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", R.COPY_COUNTS + ["lopsided"])
def test_copy_many_chunk_edges_and_a_lopsided_launch(engines, mode, count):
    """32 / 33 / 64 / 65 pairs (the launches take 32 each); one launch in which one pair has 200 x the pixels of the
    others (the grid is sized by the largest, every other pair's workgroups mostly idle); pairs of two images"""
    eng = engines[mode]
    if count == "lopsided":
        extents = [(1, 2, 3), (1, 1, 6), (1, 30, 40), (2, 1, 3), (1, 3, 2)]
        assert max(n * h * w for n, h, w in extents) == 200 * 6
    else:
        rng = np.random.default_rng(count)
        extents = [(int(rng.integers(1, 3)), int(rng.integers(1, 9)), int(rng.integers(1, 12))) for _ in range(count)]
        extents[-1] = (2, 3, 5)
    with _scratch(eng):
        srcs, dsts, wants = _copy_pairs(eng, mode, extents)
        eng.copy_many([s.view for s in srcs], [d.view for d in dsts])
        failures = []
        for i, (d, want) in enumerate(zip(dsts, wants)):
            _check(failures, "pair %d %s" % (i, extents[i]), d.mismatch(want))
        assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("count", R.TRANSPOSE_COUNTS)
@pytest.mark.parametrize("c", R.TRANSPOSE_CS)
def test_transpose_many_tiles_tails_and_untouched_surroundings(engines, mode, c, count):
    """pixel counts 1, 63, 64, 65, 130 against the 64 x 64 tile; columns [N, ceil_vec(N)) zero, later columns and the
    rows >= C keep the sentinel (the whole matrix allocation is compared)"""
    eng, vn = engines[mode], R.VN[mode]
    it = {"f16": torch.int16, "f32": torch.int32}[mode]
    with _scratch(eng):
        srcs, mats, wants = [], [], []
        for i in range(count):
            h, w = R.TRANSPOSE_MAPS[i % len(R.TRANSPOSE_MAPS)]
            x = R.plain_data((1, c, h, w), mode, 50, i, c, h, w)
            srcs.append(_src(eng, x, mode, NAN[mode]))
            m = eng.matrix(c + 8, R.ceil_to(h * w, vn) + 8)
            m.buf.view(it)[:] = SENTINEL[mode]
            rows, pitch = m.buf.numel() // (2 if mode == "f16" else 4) // m.sw, m.sw
            before = np.full(rows * pitch, SENTINEL[mode], _IT[mode]).view(_FT[mode]).astype(np.float64)
            want = R.transpose_dest_ref(x, rows, pitch, vn, before)
            mats.append(m)
            wants.append(np.ascontiguousarray(want.astype(_FT[mode])).view(_IT[mode]).reshape(-1))
        eng.transpose_many([s.view for s in srcs], mats)
        torch.cuda.synchronize()
        failures = []
        for i, (m, want) in enumerate(zip(mats, wants)):
            got = m.buf.view(it).cpu().numpy()[: want.size]
            bad = np.nonzero(got != want)[0]
            if bad.size:
                failures.append("pair %d (%d pixels): %d elements differ, first at row %d column %d" % (
                    i, srcs[i].view.h * srcs[i].view.w, bad.size, bad[0] // m.sw, bad[0] % m.sw))
        assert not failures, "\n".join(failures)


# ============================================================================================================ GroupNorm
# every case in every storage type that takes its C / groups (whole vectors per group, C / vn a divisor of 256)
GN_PARAMS = [(mode, case) for mode in MODES for case in R.gn_cases(mode)]


def _gn_call(eng, x, y, groups, gamma, beta, eps, act):
    """glsdet_groupnorm through the C entry point (x and y may be different views)"""
    from glsdet_amd._lib import ACT, check
    from glsdet_amd.engine import _stream_ptr
    ws = eng.raw(eng.lib.glsdet_groupnorm_workspace_bytes(x.n, groups))
    check(eng.lib.glsdet_groupnorm(C.byref(x.as_c()), C.byref(y.as_c()), groups, gamma.data_ptr(), beta.data_ptr(), eps,
                                   ACT[act], ws.data_ptr(), _stream_ptr(eng.stream)), "groupnorm")


@pytest.mark.parametrize("mode,case", GN_PARAMS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_groupnorm_exact_regime_bit_for_bit(engines, mode, case):
    """two values m +- a per group, gamma in quarters, beta in eighths, eps = 0: the result is +-gamma + beta exactly;
    act none and relu; in place, and out of place into a differently strided y"""
    eng, failures = engines[mode], []
    d = R.gn_exact_data(case, mode, "none", 0)
    ga, be = _dev(eng, d["gamma"]), _dev(eng, d["beta"])
    big = d["x"].size > 1 << 22          # the two large maps: relu in place and none out of place only (seconds of transfers)
    for act in ("none", "relu"):
        want = _bits(d["y"] if act == "none" else np.maximum(d["y"], 0.0), mode)
        if not big or act == "relu":
            with _scratch(eng):
                xin = _src(eng, d["x"], mode, NAN[mode])
                _gn_call(eng, xin.view, xin.view, case.groups, ga, be, 0.0, act)
                _check(failures, "%s in place" % act, xin.mismatch(want))
        if not big or act == "none":
            with _scratch(eng):
                xin, dst = _src(eng, d["x"], mode, NAN[mode]), _dst(eng, d["x"].shape, mode)
                _gn_call(eng, xin.view, dst.view, case.groups, ga, be, 0.0, act)
                _check(failures, "%s out of place" % act, dst.mismatch(want))
                _check(failures, "%s out of place, the source" % act, xin.mismatch(None))
    assert not failures, "\n".join(failures)


def _gn_within_bound(eng, mode, case, d, what):
    """relu, in place, eps = 1e-5 against groupnorm_ref within B (+ half an fp16 ulp) -> max(error / bound)"""
    want, B = R.groupnorm_ref(d["x"], case.groups, d["gamma"], d["beta"], 1e-5, "relu")
    tol = B + (R.half_ulp_f16(want, B) if mode == "f16" else 0.0)
    with _scratch(eng):
        xin = _src(eng, d["x"], mode, NAN[mode])
        eng.groupnorm(xin.view, case.groups, _dev(eng, d["gamma"]), _dev(eng, d["beta"]), 1e-5, "relu")
        got, bits = _values(xin)
        outside = xin.mismatch(bits)
    err = np.abs(got - want)
    ratio = float(np.max(err / np.maximum(tol, 1e-300)))
    pure = float(np.max(err / np.maximum(B, 1e-300)))
    print("groupnorm %s %s %s: max |err| %.3e, max err / bound %.3f, max err / B %.3f" % (what, mode, case.name, err.max(), ratio, pure))
    assert not outside, outside
    assert np.isfinite(got).all()
    return ratio


@pytest.mark.parametrize("mode,case", GN_PARAMS, ids=lambda v: v if isinstance(v, str) else v.name)
def test_groupnorm_generic_data_within_the_derived_bound(engines, mode, case):
    """N(0, 1) data with one constant-valued group (variance 0: rstd = 1 / sqrt(eps))"""
    ratio = _gn_within_bound(engines[mode], mode, case, R.gn_generic_data(case, mode, 0), "generic")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("mode", MODES)
def test_groupnorm_offset_data_within_the_derived_bound(engines, mode):
    """x = r + N(0, 1), r = 2^10 (fp32) / 2^4 (fp16): E[x^2] - mean^2 cancels 20 bits; the statistics must square and sum
    every element in fp64.  A CPU emulation of the kernel's arithmetic order on this data (not a GPU run): fp32, max
    err / B = 16.5 with per-vector fp32 sums of squares (as gn_stats_kernel had them) and 0.21 with every element widened;
    fp16, 0.99 of B + half an ulp either way (fp16 squares are exact in fp32, the final rounding dominates)."""
    case = R.GN_OFFSET_CASE
    d = R.gn_generic_data(case, mode, 1, offset=R.GN_OFFSET[mode], constant_group=False)
    assert abs(d["x"].mean() - R.GN_OFFSET[mode]) < 0.1
    ratio = _gn_within_bound(engines[mode], mode, case, d, "offset")
    assert ratio <= 1.0, ratio


def _multi_sets(eng, mode, extents, n=2):
    cases = [R.GnCase("multi%d" % i, n, R.GN_MULTI_C, R.GN_MULTI_GROUPS, h, w) for i, (h, w) in enumerate(extents)]
    data = [R.gn_exact_data(c, mode, "relu", 0) for c in cases]
    xs = [_src(eng, d["x"], mode, NAN[mode]) for d in data]
    return cases, data, xs


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("sets", [R.GN_SETS, R.GN_SETS + 1])
def test_groupnorm_multi_sets_of_unequal_extents_each_on_its_own(engines, mode, sets):
    """16 sets in one call (the grid is sized by the largest set: the others leave by their own slice and row counts);
    17 sets make two launches.  Every set is compared on its own, bit for bit."""
    eng = engines[mode]
    with _scratch(eng):
        cases, data, xs = _multi_sets(eng, mode, R.GN_MULTI_EXTENTS[:sets])
        eng.groupnorm_multi([x.view for x in xs], R.GN_MULTI_GROUPS, [_dev(eng, d["gamma"]) for d in data],
                            [_dev(eng, d["beta"]) for d in data], 0.0, "relu")
        failures = []
        for c, d, x in zip(cases, data, xs):
            _check(failures, "%s %dx%d" % (c.name, c.h, c.w), x.mismatch(_bits(d["y"], mode)))
        assert not failures, "\n".join(failures)


@pytest.mark.parametrize("mode", MODES)
def test_groupnorm_multi_mixed_call_with_and_without_conv_statistics(engines, monkeypatch, mode):
    """set 0 carries the partial sums its 3x3 conv wrote (glsdet_conv2d_gnstats), set 1 does not: set 0 within the
    bound on the conv's stored output, set 1 (exact regime, another extent) bit for bit"""
    monkeypatch.setenv("GLSDET_GN_FUSION", "1")
    eng = engines[mode]
    C_, G = R.GN_MULTI_C, R.GN_MULTI_GROUPS
    with _scratch(eng):
        gen = np.random.default_rng(7)
        x = R.round_to(gen.normal(size=(2, C_, 17, 33)), mode)
        w = gen.normal(size=(C_, C_, 3, 3)) / np.sqrt(9 * C_)
        pk = eng.pack_conv([(torch.from_numpy(w).float(), torch.ones(C_), torch.zeros(C_))], C_)
        xin = _src(eng, x, mode, NAN[mode], kind="dense")
        y0 = Placed(eng, "dense", 2, 17, 33, C_, mode, SENTINEL[mode]).upload()
        _, st = eng.conv_gnstats(xin.view, pk, 1, G, out=y0.view)
        assert st is not None, "the statistics form must apply to a 3x3 stride-1 conv"
        raw, _ = _values(y0)
        cases, data, xs = _multi_sets(eng, mode, [(7, 11)])
        g0 = R.gn_generic_data(R.GnCase("pre", 2, C_, G, 17, 33), mode, 3)
        eng.groupnorm_multi([y0.view, xs[0].view], G, [_dev(eng, g0["gamma"]), _dev(eng, data[0]["gamma"])],
                            [_dev(eng, g0["beta"]), _dev(eng, data[0]["beta"])], 0.0, "relu", pre=[st, None])
        bad = xs[0].mismatch(_bits(data[0]["y"], mode))
        assert not bad, "the set without conv statistics: " + bad
        want, B = R.groupnorm_ref(raw, G, g0["gamma"], g0["beta"], 0.0, "relu")
        tol = B + (R.half_ulp_f16(want, B) if mode == "f16" else 0.0)
        got, _ = _values(y0)
        ratio = float(np.max(np.abs(got - want) / np.maximum(tol, 1e-300)))
        print("groupnorm pre-statistics set %s: max err / bound %.3f" % (mode, ratio))
        assert ratio <= 1.0, ratio


# ========================================================================================================= proxy scores
def _proxy_run(eng, mode, feat, dots, counts, gamma, kind="ring"):
    """-> (scores [n, nc, h, w] float64, message about anything outside the first nc channels that changed)"""
    n, _, h, w = feat.shape
    P, nc = dots.shape[1], len(counts)
    fv = _src(eng, feat, mode, NAN[mode], kind=kind)
    dv = Placed(eng, "dense", n, h, w, R.ceil_to(P, 8) + 8, "f32", NAN["f32"]).put(dots, (_ALL, _ALL, _ALL, slice(0, P))).upload()
    ov = Placed(eng, "dense", n, h, w, R.ceil_to(nc, 8) + 8, "f32", SENTINEL["f32"]).upload()
    eng.proxy_scores(fv.view, dv.view, counts, gamma, out=ov.view)
    index = (_ALL, _ALL, _ALL, slice(0, nc))
    got, bits = _values(ov, index)
    return got, bits, ov.mismatch(bits, index)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", R.PROXY_CASES, ids=lambda c: c.name)
def test_proxy_scores_against_the_float64_softmax(engines, mode, case):
    eng, counts = engines[mode], R.PROXY_COUNTS[case.counts]
    d = R.proxy_data(case.n, case.C, case.h, case.w, counts, mode, 0)
    want = R.proxy_ref(d["feat"], d["dots"], counts, case.gamma)
    with _scratch(eng):
        got, _, outside = _proxy_run(eng, mode, d["feat"], d["dots"], counts, case.gamma)
    ratio = float(np.max(np.abs(got - want) / (R.PROXY_TOL * np.maximum(1.0, np.abs(want)))))
    print("proxy_scores %s %s: max err / tolerance %.3f" % (case.name, mode, ratio))
    assert not outside, outside
    assert np.isfinite(got).all() and ratio <= 1.0, ratio
    if case.n * case.h * case.w > 1:
        assert not got[case.n - 1, :, case.h - 1, case.w - 1].any()          # the all-zero feature row scores 0


# =========================================================================================================== grid-stride
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kernel", R.GRID_STRIDE_KERNELS)
def test_grid_stride_loop_beyond_the_cap_of_8192_workgroups(engines, mode, kernel):
    """more work items than 2^21 threads: every thread takes a second trip of its `i += gridDim.x * blockDim.x` loop"""
    eng = engines[mode]
    e = R.grid_stride_extent(kernel, mode)
    h, w, c = e["h"], e["w"], e["C"]
    assert e["items"] > R.GRID_CAP
    with _scratch(eng):
        if kernel in ("maxpool", "pool2d"):
            x = R.pool_data((1, c, h, w), mode, 60, h, w)
            src, dst = _src(eng, x, mode, POISON[mode], kind="dense"), _dst(eng, x.shape, mode, kind="dense")
            if kernel == "maxpool":
                eng.maxpool(src.view, 3, out=dst.view)
                want = R.maxpool_ref(x, 3)
            else:
                eng.pool2d(src.view, 1, 1, 0, out=dst.view)
                want = R.pool2d_ref(x, 1, 1, 0)
        elif kernel == "resample":
            x = R.plain_data((1, c, h // 2, w // 2), mode, 61)
            src, dst = _src(eng, x, mode, NAN[mode], kind="dense"), _dst(eng, (1, c, h, w), mode, kind="dense")
            eng.resample(src.view, 2, out=dst.view)
            want = R.resample_ref(x, 2)
        elif kernel == "upsample_add":
            coarse, fine = R.updown_data((1, c, h // 2, w // 2), mode, 62), R.updown_data((1, c, h, w), mode, 63)
            src = _src(eng, coarse, mode, NAN[mode], kind="dense")
            dst = Placed(eng, "dense", 1, h, w, c, mode, SENTINEL[mode]).put(fine).upload()
            eng.upsample_add(src.view, dst.view)
            want = R.upsample_add_ref(fine, coarse, mode)
        elif kernel == "nchw_pack":
            img = R.image_data((1, 1, h, w), 64)
            dst = _dst(eng, (1, c, h, w), mode, kind="dense")
            eng.nchw_pack(_image(eng, img), out=dst.view)
            want = R.nchw_pack_ref(img, c, mode)
        elif kernel == "focus_pack":
            img = R.image_data((1, 1, 2 * h, 2 * w), 65)
            dst = _dst(eng, (1, c, h, w), mode, kind="dense")
            eng.focus_pack(_image(eng, img), out=dst.view)
            want = R.focus_ref(img, c, mode)
        else:
            # no float64 reference can be met bit for bit: the scores repeat with a period of 1024 positions, a launch of
            # one period (below the cap, held to the usual bar) says which bits every later period must show
            counts, period = [2, 3], 1024
            base = R.proxy_data(1, c, 1, period, counts, mode, 66)
            small, small_bits, _ = _proxy_run(eng, mode, base["feat"], base["dots"], counts, 10.0, kind="dense")
            want = R.proxy_ref(base["feat"], base["dots"], counts, 10.0)
            assert (np.abs(small - want) <= R.PROXY_TOL * np.maximum(1.0, np.abs(want))).all()
            pos = np.arange(h * w) % period
            feat = base["feat"][:, :, 0, pos].reshape(1, c, h, w)
            dots = base["dots"][:, :, 0, pos].reshape(1, -1, h, w)
            _, bits, outside = _proxy_run(eng, mode, feat, dots, counts, 10.0, kind="dense")
            assert not outside, outside
            assert np.array_equal(bits.reshape(h * w, -1), small_bits.reshape(period, -1)[pos])
            return
        assert dst.full.buf.numel() < 70e6                          # bytes
        bad = dst.mismatch(_bits(want, mode))
        assert not bad, bad


# ================================================================================================================ reach
def test_every_path_is_reached(engines):
    """fails when the case lists lose an edge this file exists for (the kernels' launch rules are restated in
    helper_reference: gn_plan, GRID_CAP, COPY_JOBS); the multi-set call is recorded into a plan and must be ONE op"""
    assert any(not R.focus_is_fast_path(cin, cy) for cin, cy, _ in R.FOCUS_CASES), "the Focus general path"
    assert any(R.focus_is_fast_path(cin, cy) and kind == "slice48" for cin, cy, kind in R.FOCUS_CASES)
    assert any(not np.array_equal(R.nearest_index(*p), R.nearest_index_exact(*p)) for hp, wp in R.UPSAMPLE_CASES for p in (hp, wp)), \
        "a pair on which the float and the integer nearest index differ"
    for mode in MODES:
        plans = [R.gn_plan(c.h * c.w, c.C, mode) for c in R.gn_cases(mode)]
        assert any(p["nsplit"] == R.GN_SPLIT_CAP and c.h * c.w > 256 * R.GN_SPLIT_CAP for c, p in zip(R.gn_cases(mode), plans)), "the nsplit cap"
        assert any(p["gb_uncapped"] > R.GN_GB_CAP for p in plans), "the gb cap"
        for kernel in R.GRID_STRIDE_KERNELS:
            assert R.grid_stride_extent(kernel, mode)["items"] > R.GRID_CAP, kernel
        eng = engines[mode]
        with _scratch(eng):
            xs = [eng.tensor(1, h, w, R.GN_MULTI_C) for h, w in R.GN_MULTI_EXTENTS[:R.GN_SETS]]
            ga = [_dev(eng, np.ones(R.GN_MULTI_C))] * len(xs)
            plan = eng.new_plan()
            with plan:
                eng.groupnorm_multi(xs, R.GN_MULTI_GROUPS, ga, ga, 1e-5, "relu")
            ops = plan.ops()
            assert len(ops) == 1 and ops[0]["name"].startswith("groupnorm_multi"), ops          # a multi-set call
    assert any(c > R.COPY_JOBS for c in R.COPY_COUNTS) and R.COPY_JOBS in R.COPY_COUNTS and R.COPY_JOBS + 1 in R.TRANSPOSE_COUNTS
