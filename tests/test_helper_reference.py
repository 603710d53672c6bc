"""CPU tests of tests/helper_reference.py, the plain references tests/test_helper_fuzz.py compares the pooling, packing,
resampling, copy, GroupNorm and proxy kernels with: each reference against torch in float64, the float32 nearest formula
against F.interpolate, the premises of the exact GroupNorm regime for every GPU case, the case lists against the edges
they claim, a mutation check (for each mistake a kernel could plausibly make, the mutated reference must differ from the
right one on the GPU cases' OWN data), and the host-side refusals of the entry points that tests/test_abi.py does not
already assert (recorded into a plan, so nothing could be launched even if a call were accepted)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import helper_reference as R

MODES = ["f16", "f32"]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


# =================================================================================================== against torch
@pytest.mark.parametrize("k,s,p", R.POOL2D_KSP + [(k, 1, k // 2) for k in R.MAXPOOL_KS])
def test_pools_equal_torch_float64(k, s, p):
    for h in R.pool2d_extents(k, p):
        for w in R.pool2d_extents(k, p):
            x = R.pool_data((2, 8, h, w), "f16", k, s, p, h, w)
            big = np.where(np.isinf(x), -1e300, x)                   # torch pads with -inf too; keep its input finite
            want = F.max_pool2d(_t(big), k, s, p).numpy()
            got = R.pool2d_ref(x, k, s, p)
            assert np.array_equal(np.where(np.isinf(got), -1e300, got), want), (k, s, p, h, w)


def test_spp_is_three_direct_pools():
    x = R.pool_data((2, 8, 13, 29), "f32", 1)
    big = _t(np.where(np.isinf(x), -1e300, x))
    for got, k in zip(R.spp_ref(x), (5, 9, 13)):
        assert np.array_equal(np.where(np.isinf(got), -1e300, got), F.max_pool2d(big, k, 1, k // 2).numpy())


def test_pool_reference_refuses_nan():
    x = np.zeros((1, 8, 3, 3))
    x[0, 0, 1, 1] = np.nan
    with pytest.raises(AssertionError):
        R.maxpool_ref(x, 3)


def _all_nearest_pairs():
    pairs = set(R.UPSAMPLE_PAIRS)
    for dt in MODES:
        e = R.grid_stride_extent("upsample_add", dt)
        pairs |= {(e["h"] // 2, e["h"]), (e["w"] // 2, e["w"])}
    return sorted(pairs)


def test_nearest_index_equals_torch_on_every_pair_the_gpu_file_uses():
    for n_in, n_out in _all_nearest_pairs():
        x = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        want = F.interpolate(x, size=(1, n_out), mode="nearest").view(-1).numpy().astype(np.int64)
        assert np.array_equal(R.nearest_index(n_in, n_out), want), (n_in, n_out)
    for pair in R.UPSAMPLE_PAIRS:
        differs = not np.array_equal(R.nearest_index(*pair), R.nearest_index_exact(*pair))
        assert differs == (pair in R.FLOAT_NE_INT), pair


@pytest.mark.parametrize("dt", MODES)
def test_upsample_add_and_resample_equal_torch(dt):
    for (hp, wp) in R.UPSAMPLE_CASES:
        coarse = R.updown_data((2, 8, hp[0], wp[0]), dt, 1, hp[0], wp[0])
        fine = R.updown_data((2, 8, hp[1], wp[1]), dt, 2, hp[1], wp[1])
        assert 2.0 ** -6 <= np.abs(fine).min() and np.abs(fine).max() <= 2.0 ** 4
        up = F.interpolate(_t(coarse).float(), size=(hp[1], wp[1]), mode="nearest").double().numpy()
        assert np.array_equal(R.upsample_add_ref(fine, coarse, dt), R.round_to(fine + up, dt))
    x = R.plain_data((2, 8, 3, 5), dt, 3)
    for f in R.RESAMPLE_FACTORS:
        want = F.interpolate(_t(x), scale_factor=f, mode="nearest").numpy() if f > 1 else x
        assert np.array_equal(R.resample_ref(x, f), want)


def test_packing_references():
    img = R.image_data((2, 3, 6, 34), 1)
    t = torch.from_numpy(img)
    want = torch.cat((t[..., ::2, ::2], t[..., 1::2, ::2], t[..., ::2, 1::2], t[..., 1::2, 1::2]), 1)
    for dt, cast in (("f32", lambda v: v), ("f16", lambda v: v.half().float())):
        got = R.focus_ref(img, 24, dt)
        assert np.array_equal(got[:, :12], cast(want).double().numpy()) and not got[:, 12:].any()
        got = R.nchw_pack_ref(img, 16, dt)
        assert np.array_equal(got[:, :3], cast(t).double().numpy()) and not got[:, 3:].any()
    assert (R.focus_ref(img, 24, "f16") != R.focus_ref(img, 24, "f32")).mean() > 0.3        # a real rounding
    x = R.plain_data((1, 8, 5, 13), "f32", 2)
    assert np.array_equal(R.transpose_ref(x), _t(x).view(8, -1).numpy()) and np.array_equal(R.copy_ref(x), x)


@pytest.mark.parametrize("dt", MODES)
def test_groupnorm_ref_equals_torch_float64(dt):
    for case in [c for c in R.gn_cases(dt) if c.h * c.w <= 1000]:
        d = R.gn_generic_data(case, dt, 0)
        for act in ("none", "relu"):
            want = F.group_norm(_t(d["x"]), case.groups, _t(d["gamma"]), _t(d["beta"]), float(np.float32(1e-5)))
            want = torch.relu(want) if act == "relu" else want
            got, B = R.groupnorm_ref(d["x"], case.groups, d["gamma"], d["beta"], 1e-5, act)
            # (torch sums in another order: far below the fp32 resolution B stands for)
            assert np.abs(got - want.numpy()).max() <= 1e-9 * max(1.0, np.abs(got).max()), case.name
            assert B.shape == got.shape and (B > 0).any() and (B >= 0).all()
            assert (B <= 2.0 ** -20 * (np.abs(got) + 2 * np.abs(d["beta"]).max() + 1e3)).all()


def test_proxy_ref_equals_the_oracle_in_float64():
    from oracle import mpdet_oracle as M
    for name, counts in R.PROXY_COUNTS.items():
        r = np.random.default_rng(len(counts))
        feat, prox = r.normal(size=(6, 24)), r.normal(size=(int(np.sum(counts)), 24))
        unit = prox / np.sqrt((prox * prox).sum(1, keepdims=True))
        dots = feat @ unit.T
        for gamma in (1.0, 10.0, 100.0):
            want = M.forward_proxy(_t(feat), _t(prox), counts, gamma).numpy()
            got = R.proxy_ref(feat.T.reshape(1, 24, 6, 1), dots.T.reshape(1, -1, 6, 1), counts, gamma)[0, :, :, 0].T
            assert np.abs(got - want).max() <= 1e-10 * max(1.0, np.abs(want).max()), (name, gamma)


# ========================================================================================= the exact GroupNorm regime
@pytest.mark.parametrize("dt", MODES)
def test_exact_regime_premises_hold_for_every_gpu_case(dt):
    """gn_exact_data asserts its own premises (even count, representable x and y); here in addition: the float64
    two-pass reference reproduces the closed form EXACTLY, both values of a group occur, and relu does clip something"""
    cases = R.gn_cases(dt) + [R.GnCase("multi%d" % i, 1, R.GN_MULTI_C, R.GN_MULTI_GROUPS, h, w)
                              for i, (h, w) in enumerate(R.GN_MULTI_EXTENTS)]
    for case in cases:
        assert R.gn_legal(case.C, case.groups, dt), case
        for act in ("none", "relu"):
            d = R.gn_exact_data(case, dt, act, 0)
            if case.C * case.h * case.w > 1 << 22:
                continue                                            # (the builder's own asserts ran; skip the slow re-derivation)
            y, _ = R.groupnorm_ref(d["x"], case.groups, d["gamma"], d["beta"], 0.0, act)
            assert np.array_equal(y, d["y"]), case.name
            cpg = case.C // case.groups
            per = d["x"].reshape(case.n, case.groups, -1)
            assert all(len(np.unique(per[b, g])) == 2 for b in range(case.n) for g in range(case.groups))
            if act == "relu" and case.C * case.h * case.w >= 64:
                none = R.gn_exact_data(case, dt, "none", 0)["y"]
                assert (none < 0).any() and (d["y"] >= 0).all()
            assert cpg % R.VN[dt] == 0


# ============================================================================================== the case lists
def test_the_case_lists_cover_the_edges_they_claim():
    assert R.MAXPOOL_KS == [1, 3, 5, 13, 31] and set(R.MAXPOOL_MAPS) == {(1, 1), (2, 3), (7, 5), (20, 24)} and R.POOL_CS == [8, 24]
    assert min(h for h, _ in R.MAXPOOL_MAPS) < 3 and any(h < 31 and w < 31 for h, w in R.MAXPOOL_MAPS)       # maps smaller than k
    assert R.SPP_HS == [1, 7, 8, 9, 13] and R.SPP_WS == [1, 15, 16, 17, 29]
    assert set(R.POOL2D_KSP) == {(3, 2, 1), (2, 2, 0), (1, 2, 0), (3, 1, 1), (3, 3, 0), (5, 2, 2), (2, 1, 1), (7, 4, 3)}
    for k, s, p in R.POOL2D_KSP:
        ext = R.pool2d_extents(k, p)
        assert {k, k + 1, 20, 25} <= set(ext) and ((1 in ext) == (1 + 2 * p - k >= 0))
    # Focus: the general path (everything but cin == 3 into 16 channels), the fast path on a strided view, zero fill
    assert {c[0] for c in R.FOCUS_CASES} == {1, 2, 3, 4, 5} and R.FOCUS_HW == [2, 6, 34]
    assert (3, 24, "window") in R.FOCUS_CASES and (3, 16, "slice48") in R.FOCUS_CASES
    assert sum(R.focus_is_fast_path(c[0], c[1]) for c in R.FOCUS_CASES) == 1
    assert any(cy > 4 * cin for cin, cy, _ in R.FOCUS_CASES if not R.focus_is_fast_path(cin, cy))
    assert R.NCHW_CINS == [1, 3, 8, 9, 17]
    assert R.RESAMPLE_FACTORS == [1, 2, 3, 4, 5, 6, 7, 8] and R.RESAMPLE_MAPS == [(3, 5), (9, 11)]
    assert set(R.UPSAMPLE_PAIRS) == {(14, 46), (21, 69), (26, 44), (39, 33), (13, 25), (7, 13), (1, 5), (9, 9)}
    assert {c[0] for c in R.UPSAMPLE_CASES} == set(R.UPSAMPLE_PAIRS) == {c[1] for c in R.UPSAMPLE_CASES}
    assert set(R.FLOAT_NE_INT) <= set(R.UPSAMPLE_PAIRS) and len(R.FLOAT_NE_INT) == 4
    assert R.COPY_COUNTS == [32, 33, 64, 65] and R.COPY_JOBS == 32 and R.TRANSPOSE_COUNTS == [32, 33]
    assert [h * w for h, w in R.TRANSPOSE_MAPS] == [1, 63, 64, 65, 130] and R.TRANSPOSE_CS == [8, 64, 72, 136]
    assert any((h * w) % 4 for h, w in R.TRANSPOSE_MAPS)
    # GroupNorm: groups == 1, one vector per group, C / vn == 256, the slice cap, the apply-grid cap, multi-set extents
    for dt in MODES:
        cases, vn = R.gn_cases(dt), R.VN[dt]
        assert any(c.groups == 1 for c in cases) and any(c.C // c.groups == vn for c in cases)
        assert any(c.C // vn == 256 for c in cases)
        plans = [R.gn_plan(c.h * c.w, c.C, dt) for c in cases]
        assert any(c.h * c.w > 16384 for c in cases) and any(p["nsplit"] == R.GN_SPLIT_CAP for p in plans)
        capped = [(c, p) for c, p in zip(cases, plans) if p["gb_uncapped"] > R.GN_GB_CAP]
        assert len(capped) == 1
        c, p = capped[0]                                            # ... and it is the smallest such map for its C
        assert p["gb"] == R.GN_GB_CAP and R.gn_plan(c.h * c.w - c.h, c.C, dt)["gb_uncapped"] <= R.GN_GB_CAP
        assert c.C * c.h * c.w * (2 if dt == "f16" else 4) < 70e6
    names16, names32 = {c.name for c in R.gn_cases("f16")}, {c.name for c in R.gn_cases("f32")}
    assert {"c8_g1_1x1", "c64_g8_33x17", "c256_g32_1x2", "c2048_g256_3x5", "c64_g1_20x24", "c64_g8_129x128"} <= names16
    assert {"c1024_g256_3x5", "c64_g16_7x11", "c64_g8_129x128"} <= names32
    assert len(R.GN_MULTI_EXTENTS) == 17 > R.GN_SETS and (1, 1) in R.GN_MULTI_EXTENTS[:16] and (129, 128) in R.GN_MULTI_EXTENTS[:16]
    assert len(set(R.GN_MULTI_EXTENTS[:16])) >= 15
    assert R.GN_OFFSET == {"f32": 1024.0, "f16": 16.0}
    # proxy scores
    assert [len(v) for v in R.PROXY_COUNTS.values()] == [1, 1, 17, 256] and R.PROXY_COUNTS["sixtyfour"] == [64]
    assert max(R.PROXY_COUNTS["mixed17"]) == 64 and min(R.PROXY_COUNTS["mixed17"]) == 1 and sum(R.PROXY_COUNTS["mixed17"]) <= 256
    assert {c.counts for c in R.PROXY_CASES} == set(R.PROXY_COUNTS)
    assert {c.n * c.h * c.w for c in R.PROXY_CASES} == {1, 5, 6, 7, 8}
    assert {c.C for c in R.PROXY_CASES} == {8, 136, 256} and {c.gamma for c in R.PROXY_CASES} == {1.0, 10.0, 100.0}
    assert R.PROXY_TOL == 2e-5
    # grid-stride: one case per kernel, each beyond the cap of 2^21 threads, no tensor above 70 MB
    assert R.GRID_CAP == 1 << 21
    assert R.GRID_STRIDE_KERNELS == ["maxpool", "pool2d", "resample", "upsample_add", "nchw_pack", "focus_pack", "proxy_scores"]
    for dt in MODES:
        for kern in R.GRID_STRIDE_KERNELS:
            e = R.grid_stride_extent(kern, dt)
            assert e["items"] > R.GRID_CAP
            assert e["h"] * e["w"] * 8 * 4 < 70e6 and e["h"] * e["w"] * 4 * 4 < 70e6        # 8 channels of fp32; the 2 x 2 image


# ======================================================================================================== mutants
def _differs(a, b):
    return not np.array_equal(np.nan_to_num(a, nan=1e300, posinf=1e301, neginf=-1e301),
                              np.nan_to_num(b, nan=1e300, posinf=1e301, neginf=-1e301))


@pytest.mark.parametrize("dt", MODES)
def test_pool_mutants_are_told_apart_by_the_gpu_data(dt):
    for k in R.MAXPOOL_KS:
        seen_minus = seen_plus = False
        for (h, w) in R.MAXPOOL_MAPS:
            for c in R.POOL_CS:
                x = R.pool_data((2, c, h, w), dt, k, h, w, c)
                good = R.maxpool_ref(x, k)
                if k // 2 >= 1:                                      # (k == 1 has no padding to get wrong)
                    assert _differs(good, R.maxpool_ref(x, k, fill=0.0)), ("zero padding", k, h, w)
                    seen_minus |= _differs(good, R.maxpool_ref(x, k - 2))
                seen_plus |= k + 2 > 31 or _differs(good, R.maxpool_ref(x, k + 2))
        assert seen_plus and (seen_minus or k == 1), ("window radius off by one", k)
    for k, s, p in R.POOL2D_KSP:
        for h in R.pool2d_extents(k, p):
            x = R.pool_data((2, 8, h, 20), dt, k, s, p, h, 20)
            if p:
                assert _differs(R.pool2d_ref(x, k, s, p), R.pool2d_ref(x, k, s, p, fill=0.0)), (k, s, p, h)
    hits = 0
    for h in R.SPP_HS:
        for w in R.SPP_WS:
            x = R.pool_data((2, 8, h, w), dt, 5, h, w)
            p5, p9, p13 = R.spp_ref(x)
            assert _differs(p5, R.maxpool_ref(x, 5, fill=0.0))
            hits += _differs(p9, R.maxpool_ref(x, 7))               # pool9 built as a single 7-pool
            if h >= 8 and w >= 15:
                assert _differs(p9, R.maxpool_ref(x, 7)) and _differs(p13, R.maxpool_ref(x, 11)), (h, w)
    assert hits >= 16


@pytest.mark.parametrize("dt", MODES)
def test_packing_and_resampling_mutants_are_told_apart(dt):
    for cin, cy, _ in R.FOCUS_CASES:
        for H in R.FOCUS_HW:
            img = R.image_data((2, cin, H, 34), cin, cy, H, 34)
            good = R.focus_ref(img, cy, dt)
            swapped = good.copy()                                    # TR / BL swapped
            swapped[:, cin:2 * cin], swapped[:, 2 * cin:3 * cin] = good[:, 2 * cin:3 * cin], good[:, cin:2 * cin]
            assert _differs(good, swapped), (cin, cy, H)
    for hp, wp in R.UPSAMPLE_CASES:
        coarse = R.updown_data((2, 16, hp[0], wp[0]), dt, 1, hp[0], wp[0])
        fine = R.updown_data((2, 16, hp[1], wp[1]), dt, 2, hp[1], wp[1])
        good = R.upsample_add_ref(fine, coarse, dt)
        mutant = R.upsample_add_ref(fine, coarse, dt, index=R.nearest_index_exact)
        assert _differs(good, mutant) == (hp in R.FLOAT_NE_INT or wp in R.FLOAT_NE_INT), (hp, wp)
    assert sum(hp in R.FLOAT_NE_INT or wp in R.FLOAT_NE_INT for hp, wp in R.UPSAMPLE_CASES) >= 8
    vn = R.VN[dt]
    for (h, w) in R.TRANSPOSE_MAPS:
        x = R.plain_data((1, 8, h, w), dt, h, w)
        rows, cols = 16, R.ceil_to(h * w, vn) + 8
        before = np.full((rows, cols), 777.0)
        good = R.transpose_dest_ref(x, rows, cols, vn, before)
        assert (good[8:] == 777.0).all() and (good[:8, R.ceil_to(h * w, vn):] == 777.0).all()
        assert not good[:8, h * w:R.ceil_to(h * w, vn)].any()
        mutant = R.transpose_dest_ref(x, rows, cols, vn, before, drop_partial_tile=True)
        assert _differs(good, mutant) == bool((h * w) % R.TRANSPOSE_TILE), (h, w)


@pytest.mark.parametrize("dt", MODES)
def test_groupnorm_mutants_are_told_apart(dt):
    """exact regime: a mutant must change bits; generic regime: it must leave the bound B (+ half an fp16 ulp)"""
    for case in [c for c in R.gn_cases(dt) if c.C * c.h * c.w <= 1 << 21]:
        N, vn = case.h * case.w, R.VN[dt]
        d = R.gn_exact_data(case, dt, "relu", 0)
        g = R.gn_generic_data(case, dt, 0)
        want, B = R.groupnorm_ref(g["x"], case.groups, g["gamma"], g["beta"], 1e-5, "relu")
        tol = B + (R.half_ulp_f16(want, B) if dt == "f16" else 0.0)
        muts = ["no_relu"]
        if N > 1:
            muts += ["drop_last_pixel", "double_pixel"]
        if case.groups > 1:
            muts.append("shift_group")
        for mut in muts:
            y, _ = R.groupnorm_ref(d["x"], case.groups, d["gamma"], d["beta"], 0.0, "relu", dt=dt, mutate=mut)
            if mut in ("drop_last_pixel", "double_pixel") and N * (case.C // case.groups) < 64:
                pass                                                 # (a handful of values: the dropped ones may balance)
            else:
                assert _differs(y, d["y"]), (case.name, mut, "exact")
            y, _ = R.groupnorm_ref(g["x"], case.groups, g["gamma"], g["beta"], 1e-5, "relu", dt=dt, mutate=mut)
            assert (np.abs(y - want) > tol).any(), (case.name, mut, "generic")


def test_proxy_mutants_are_told_apart():
    shifted = overflow = 0
    for case in R.PROXY_CASES:
        counts = R.PROXY_COUNTS[case.counts]
        for dt in MODES:
            d = R.proxy_data(case.n, case.C, case.h, case.w, counts, dt, 0)
            want = R.proxy_ref(d["feat"], d["dots"], counts, case.gamma)
            assert np.isfinite(want).all()
            tol = R.PROXY_TOL * np.maximum(1.0, np.abs(want))
            if len(counts) > 1:
                bad = R.proxy_ref(d["feat"], d["dots"], counts, case.gamma, shift_class=True)
                assert (np.abs(bad - want) > tol).any(), case.name
                shifted += 1
            if case.gamma == 100.0:
                bad = R.proxy_ref(d["feat"], d["dots"], counts, case.gamma, subtract_max=False)
                assert not np.isfinite(bad).all() or (np.abs(bad - want) > tol).any(), case.name
                overflow += 1
    assert shifted >= 8 and overflow >= 6


# ============================================================================================= host-side refusals
def _view(n, h, w, c, dtype=0, base=0x10000, pitch=None, extra=0):
    """a view on a fake address (never dereferenced: every call below is refused, and is recorded into a plan anyway);
    pitch: the pixel stride, so that a channel count that is no multiple of 8 still passes the alignment check"""
    from glsdet_amd import _lib
    es = 2 if dtype == 0 else 4
    sw = pitch or c
    v = _lib.View()
    v.base, v.n, v.h, v.w, v.c, v.dtype = base, n, h, w, c, dtype
    v.sw, v.sh, v.sn = sw, w * sw, h * w * sw
    v.alloc_lo, v.alloc_hi = base, base + n * h * w * sw * es + extra
    return v


def test_helper_entry_points_refuse_malformed_calls_on_the_host():
    import __graft_entry__ as g
    g.build()
    from glsdet_amd import _lib
    lib = _lib.load()
    P = C.byref
    err = lambda: lib.glsdet_last_error().decode()
    plan = lib.glsdet_plan_create()
    assert lib.glsdet_plan_begin(plan) == 0                 # recording: an accepted call would be stored, never launched
    try:
        def refused(rc, word):
            assert rc < 0 and word in err(), (rc, err())

        x, y = _view(2, 8, 10, 16), _view(2, 8, 10, 16, base=0x90000)
        x12, y12 = _view(2, 8, 10, 12, pitch=16), _view(2, 8, 10, 12, base=0x90000, pitch=16)
        # channels that are no multiple of 8, for each entry point that moves 16-byte vectors
        refused(lib.glsdet_maxpool2d(P(x12), P(y12), 3, None), "maxpool2d")
        refused(lib.glsdet_spp_pools(P(x12), P(y12), P(y12), P(y12), None), "spp_pools")
        refused(lib.glsdet_pool2d(P(x12), P(_view(2, 4, 5, 12, base=0x90000, pitch=16)), 3, 2, 1, None), "pool2d")
        refused(lib.glsdet_resample_copy(P(x12), P(y12), 1, None), "resample_copy")
        refused(lib.glsdet_upsample_add(P(x12), P(y12), None), "upsample_add")
        refused(lib.glsdet_copy_many(P(x12), P(y12), 1, None), "copy_many")
        one12 = _view(1, 8, 10, 12, pitch=16)
        refused(lib.glsdet_transpose_many(P(one12), P(_view(1, 1, 16, 80, base=0x90000)), 1, None), "transpose_many")
        refused(lib.glsdet_nchw_pack(0x2000, 2, 3, 8, 10, P(y12), None), "nchw_pack")
        ga = (C.c_float * 64)()
        refused(lib.glsdet_groupnorm(P(x12), P(x12), 1, ga, ga, 1e-5, 2, 0x4000, None), "groupnorm")
        cnt = (C.c_int32 * 2)(3, 2)
        d32, o32 = _view(2, 8, 10, 8, dtype=1, base=0x90000), _view(2, 8, 10, 8, dtype=1, base=0xA0000)
        refused(lib.glsdet_proxy_scores(P(x12), P(d32), cnt, 2, 10.0, P(o32), None), "proxy_scores")
        # maxpool2d: even k, k > 31
        refused(lib.glsdet_maxpool2d(P(x), P(y), 4, None), "odd")
        refused(lib.glsdet_maxpool2d(P(x), P(y), 33, None), "odd")
        # pool2d: 2 * pad > k, stride < 1, wrong output width
        refused(lib.glsdet_pool2d(P(x), P(_view(2, 5, 6, 16, base=0x90000)), 3, 2, 2, None), "pool2d")
        refused(lib.glsdet_pool2d(P(x), P(y), 1, 0, 0, None), "pool2d")
        refused(lib.glsdet_pool2d(P(x), P(_view(2, 4, 6, 16, base=0x90000)), 3, 2, 1, None), "pool2d")
        # resample: factor 0 and 9
        refused(lib.glsdet_resample_copy(P(x), P(y), 0, None), "factor")
        refused(lib.glsdet_resample_copy(P(x), P(_view(2, 72, 90, 16, base=0x90000)), 9, None), "factor")
        # copy_many / transpose_many: 0 and 4097 pairs, more than one image, a matrix too small
        one, mat = _view(1, 8, 10, 16), _view(1, 1, 16, 80, base=0x90000)
        for count in (0, 4097):
            refused(lib.glsdet_copy_many(P(x), P(y), count, None), "copy_many")
            refused(lib.glsdet_transpose_many(P(one), P(mat), count, None), "transpose_many")
        refused(lib.glsdet_transpose_many(P(x), P(mat), 1, None), "one image")
        refused(lib.glsdet_transpose_many(P(one), P(_view(1, 1, 8, 80, base=0x90000)), 1, None), "too small")      # rows < C
        refused(lib.glsdet_transpose_many(P(one), P(_view(1, 1, 16, 72, base=0x90000)), 1, None), "too small")     # cols < pixels
        # GroupNorm: C % groups, (C / groups) % vn, 256 % (C / vn); 0 and 17 sets
        refused(lib.glsdet_groupnorm(P(x), P(x), 5, ga, ga, 1e-5, 2, 0x4000, None), "groupnorm")
        refused(lib.glsdet_groupnorm(P(x), P(x), 4, ga, ga, 1e-5, 2, 0x4000, None), "groupnorm")                    # 4 per group < 8
        x24 = _view(2, 8, 10, 24)
        refused(lib.glsdet_groupnorm(P(x24), P(x24), 1, ga, ga, 1e-5, 2, 0x4000, None), "divisor of 256")
        gp = (C.c_void_p * 1)(C.addressof(ga))
        for sets in (0, R.GN_SETS + 1):
            refused(lib.glsdet_groupnorm_multi(P(x), P(x), sets, 2, gp, gp, 1e-5, 2, 0x4000, None), "sets")
        # proxy scores: a class of 65 proxies, more than 256 proxies in all, 0 and 257 classes
        refused(lib.glsdet_proxy_scores(P(x), P(d32), (C.c_int32 * 2)(3, 65), 2, 10.0, P(o32), None), "proxies")
        refused(lib.glsdet_proxy_scores(P(x), P(d32), (C.c_int32 * 5)(64, 64, 64, 64, 1), 5, 10.0, P(o32), None), "256")
        for nc in (0, 257):
            refused(lib.glsdet_proxy_scores(P(x), P(d32), (C.c_int32 * 257)(*([1] * 257)), nc, 10.0, P(o32), None), "num_classes")
        # Focus: odd H, odd W, fewer than 4 * cin channels
        f16v = _view(2, 4, 5, 16)
        refused(lib.glsdet_focus_pack(0x2000, 2, 3, 9, 10, P(f16v), None), "focus_pack")
        refused(lib.glsdet_focus_pack(0x2000, 2, 3, 8, 11, P(f16v), None), "focus_pack")
        refused(lib.glsdet_focus_pack(0x2000, 2, 5, 8, 10, P(f16v), None), "focus_pack")
    finally:
        assert lib.glsdet_plan_end(plan) == 0
        n_ops = lib.glsdet_plan_num_ops(plan)
        lib.glsdet_plan_destroy(plan)
    assert n_ops == 0, "a malformed call was accepted"
