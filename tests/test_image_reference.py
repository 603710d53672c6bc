"""CPU: the references and case tables of tests/image_reference.py, before tests/test_image_fuzz.py trusts them on the
GPU -- the two cv2 restatements against each other and against the exact bilinear, the host tables against Pillow
including the size at which Pillow changes its pass order, `rescale_size`, and the condition that keeps the tables
honest: every branch of the kernels is reached by a case."""
import math

import numpy as np
import pytest
from PIL import Image

from oracle import preprocess_oracle as P
from oracle import ufp_oracle as U
from tests import image_reference as R


# ------------------------------------------------------------------------------------------------ the cv2 restatements
def _u8_pairs():
    """every (uint8 source, dw, dh) the GPU file resizes in fixed point: the resize cases and every mosaic crop"""
    out = [("resize %d" % i, R.resize_source(h, w, True, i), nw, nh) for i, (h, w, nh, nw, _, _) in enumerate(R.RESIZE_CASES)]
    for name in R.MOSAIC_SCENES:
        out += [("%s %d" % (name, j), crop, dw, dh) for j, (crop, dw, dh) in enumerate(R.mosaic_crops(name))]
    return out


U8_PAIRS = _u8_pairs()


def test_the_two_cv2_restatements_agree_bit_for_bit():
    """the oracle's vectorised numpy form and the per-pixel integer form, written independently from the same description"""
    assert len(U8_PAIRS) >= len(R.RESIZE_CASES) + 12
    for name, src, dw, dh in U8_PAIRS:
        a, b = U.cv2_resize_linear_u8(src, dw, dh), R.cv2_linear_u8_scalar(src, dw, dh)
        assert a.shape == b.shape == (dh, dw, 3) and a.dtype == b.dtype == np.uint8, name
        assert np.array_equal(a, b), name


def test_fixed_point_resize_stays_within_the_derived_bound_of_the_exact_bilinear(capsys):
    """v - E in [FIXED_POINT_BOUND]: the derivation (coefficient rounding, the truncating shifts by 4 and by 16, the
    final rounding) is the comment above FIXED_POINT_BOUND in tests/image_reference.py; it gives about -1.007 .. +0.749
    grey levels.  Nothing in it is measured.  Measured on these cases: -0.77 .. +0.54 (printed)."""
    lo, hi = R.FIXED_POINT_BOUND
    assert -1.01 < lo < -1.0 and 0.74 < hi < 0.75
    worst_lo = worst_hi = 0.0
    for name, src, dw, dh in U8_PAIRS:
        if src.shape[:2] == (dh, dw):
            continue                                                     # a copy: nothing to bound
        gap = R.cv2_linear_u8_scalar(src, dw, dh).astype(np.float64) - R.bilinear_exact(src, dw, dh)
        worst_lo, worst_hi = min(worst_lo, float(gap.min())), max(worst_hi, float(gap.max()))
        assert lo <= gap.min() and gap.max() <= hi, (name, gap.min(), gap.max())
    with capsys.disabled():
        print("\nfixed-point resize minus exact bilinear over %d resizes: %.4f .. %+.4f grey levels (bound %.4f .. %+.4f)"
              % (len(U8_PAIRS), worst_lo, worst_hi, lo, hi))
    assert worst_lo < -0.5 and worst_hi > 0.45                           # the cases do exercise the truncation


def test_the_cases_tell_a_rounded_shift_from_the_truncated_one():
    """`(r0 + 8) >> 4` instead of `r0 >> 4` changes a pixel only where the half unit survives both later truncations.  The
    mosaic kernel and the uint8 resize kernel each hold their own copy of that line, so each family of cases has to see
    the mistake on its own data: the resize cases, and the crops of the mosaic scenes."""
    def seen(pairs):
        return [name for name, src, dw, dh in pairs
                if not np.array_equal(R.cv2_linear_u8_scalar(src, dw, dh), R.cv2_linear_u8_scalar(src, dw, dh, mutate="round4"))]
    assert len(seen([p for p in U8_PAIRS if p[0].startswith("resize")])) >= 3
    assert seen([p for p in U8_PAIRS if not p[0].startswith("resize")]) == ["stretch 0"]     # dyadic fractions cannot see it


def test_float_bilinear_of_the_oracle_is_the_exact_bilinear_on_the_same_taps():
    for i, (h, w, nh, nw, _, _) in enumerate(R.RESIZE_CASES):
        src = R.resize_source(h, w, False, i)
        np.testing.assert_allclose(U.resize_linear_f(src.astype(np.float64), nw, nh), R.bilinear_exact(src, nw, nh), rtol=0, atol=1e-10)
    src = R.resize_source(13, 19, False, 6)
    assert np.array_equal(U.resize_normalize(src, 19, 13), R.normalize_bgr(src))           # same size: the normalised source


def test_known_answers_of_the_scalar_restatement():
    a = np.array([[[0, 0, 0], [100, 200, 40]]], np.uint8)
    r = R.cv2_linear_u8_scalar(a, 4, 2)
    assert r[0, :, 0].tolist() == [0, 25, 75, 100] and r[1, :, 1].tolist() == [0, 50, 150, 200]
    assert [R.linear_tap(d, 4, 1) for d in range(4)] == [(0, 0, 0.0)] * 4
    assert R.linear_tap(35, 36, 9) == (8, 8, 0.0) and R.linear_tap(0, 36, 9) == (0, 1, 0.0)


def test_resize_normalize_is_the_test_pipeline_at_its_own_size():
    img = R.resize_source(37, 53, True, 1)
    want, meta = U.mmdet_test_pipeline(img, img_scale=(64, 32))
    nh, nw = meta["img_shape"][:2]
    assert (nh, nw) == (32, 46) and meta["pad_shape"] == (32, 64, 3)
    assert np.array_equal(want[0, :, :nh, :nw], U.resize_normalize(img, nw, nh)) and not want[0, :, :, nw:].any()


# ------------------------------------------------------------------------------------------------ tables and Pillow's pass order
def _pillow(img, oh, ow):
    return np.array(Image.fromarray(img, "RGB").resize((ow, oh), Image.BICUBIC))


@pytest.mark.parametrize("case", R.BICUBIC_CASES, ids=lambda c: "%dx%d_to_%dx%d" % c)
def test_tables_with_horizontal_first_passes_equal_pillow(case):
    from glsdet_amd.preprocess import pil_pass_order
    ih, iw, oh, ow = case
    assert ih <= 100 * iw and pil_pass_order((ih, iw), (oh, ow)) == "hv"
    img = R.image_u8(ih, iw, 3)
    assert np.array_equal(R.two_pass(img, (oh, ow)), _pillow(img, oh, ow))
    nh, nw, _, _ = R.letterbox_geometry((ih, iw), (oh, ow))
    if nh >= 1 and nw >= 1:
        assert np.array_equal(R.two_pass(img, (nh, nw)), _pillow(img, nh, nw))
        assert pil_pass_order((ih, iw), (nh, nw)) == "hv"
    # and the oracle the GPU file compares with is Pillow plus the normalisation
    assert np.array_equal(P.drone_preprocess(img, (oh, ow), False)[0], R.normalize_drone(_pillow(img, oh, ow)))


def test_pillow_pass_order_boundary():
    """At in_h == 100 * in_w Pillow still resamples horizontally first; one row more, with a shrinking height, it goes
    vertically first and the horizontal-first result is no longer Pillow's.  The second half pins the boundary: a Pillow
    that moves it fails here, and `pil_pass_order` has to follow."""
    from glsdet_amd.preprocess import pil_pass_order
    ih, iw, oh, ow = R.ORDER_BOUNDARY["at"]
    assert ih == 100 * iw and oh < ih and pil_pass_order((ih, iw), (oh, ow)) == "hv"
    img = R.image_u8(ih, iw, 5)
    assert np.array_equal(R.two_pass(img, (oh, ow), "hv"), _pillow(img, oh, ow))
    assert not np.array_equal(R.two_pass(img, (oh, ow), "vh"), _pillow(img, oh, ow))        # the orders do differ on this data
    ih, iw, oh, ow = R.ORDER_BOUNDARY["beyond"]
    assert ih == 100 * iw + 1 and oh < ih and pil_pass_order((ih, iw), (oh, ow)) == "vh"
    img = R.image_u8(ih, iw, 5)
    assert np.array_equal(R.two_pass(img, (oh, ow), "vh"), _pillow(img, oh, ow))
    assert not np.array_equal(R.two_pass(img, (oh, ow), "hv"), _pillow(img, oh, ow))


def test_pil_pass_order_rule():
    from glsdet_amd.preprocess import pil_pass_order
    assert pil_pass_order((800, 8), (64, 64)) == "hv" and pil_pass_order((801, 8), (64, 64)) == "vh"
    assert pil_pass_order((801, 8), (801, 64)) == "hv" and pil_pass_order((801, 8), (900, 64)) == "hv"      # the height does not shrink
    assert pil_pass_order((801, 8), (800, 8)) == "vh" and pil_pass_order((101, 1), (100, 1)) == "vh"
    assert pil_pass_order((100, 1), (5, 1)) == "hv" and pil_pass_order((1080, 1920), (640, 640)) == "hv"
    assert pil_pass_order((8, 801), (4, 64)) == "hv"                                                        # no rule for wide frames


# ------------------------------------------------------------------------------------------------ rescale_size
def test_rescale_size_equals_the_oracle_where_the_scaled_edge_lands_on_a_half():
    from glsdet_amd.ufp.stage2 import rescale_size
    halves = 0
    for scale in [(1333, 800), (64, 32), (800, 1333), (224, 160)]:
        for w, h in [(2001, 1600), (1600, 2001), (65, 64), (64, 65), (3, 2), (2667, 1601), (101, 50), (1333, 800), (97, 131),
                     (641, 320), (5, 320), (2665, 1600), (1, 1), (53, 37)]:
            (nw, nh), f = U.rescale_size((w, h), scale)
            assert rescale_size((w, h), scale) == (nw, nh)
            halves += int((w * f) % 1 == 0.5 or (h * f) % 1 == 0.5)
    assert halves >= 8
    assert rescale_size((2001, 1600), (1333, 800)) == (1001, 800) and rescale_size((65, 64), (64, 32)) == (33, 32)


# ------------------------------------------------------------------------------------------------ every path is reached
def _mosaic_branches(name):
    """the branches of ufp_mosaic_kernel a scene reaches, from its chip list alone"""
    H, W = R.MOSAIC_IMAGE_HW
    chips, cw, ch = R.MOSAIC_SCENES[name]
    cw, ch = math.ceil(cw), math.ceil(ch)
    got, rects = set(), []
    if not chips:
        got.add("empty")
    for raw, (x1, y1, w, h, nx, ny, s) in zip(chips, R.floored(chips)):
        assert 0 <= x1 < W and 0 <= y1 < H and s >= 1, (name, raw)
        if w == 0 or h == 0:
            got.add("w == 0" if w == 0 else "h == 0")
            continue
        assert nx >= 0 and ny >= 0 and nx + w * s <= cw and ny + h * s <= ch, (name, raw)          # the contract
        sw, sh = min(w, W - x1), min(h, H - y1)
        got.add("scale %d" % s)
        if sw < w:
            got.add("clip right")
        if sh < h:
            got.add("clip bottom")
        got.add("copy" if (sw, sh) == (w * s, h * s) else "resize")
        if (sw, sh) == (1, 1):
            got.add("1x1 crop")
        elif sw == 1 or sh == 1:
            got.add("1xN crop")
        if (sw, sh) != (w * s, h * s) and any(R.linear_tap(d, w * s, sw)[0] + 1 > sw - 1 for d in range(w * s)):
            got.add("i1 clamps")
        r = (nx, ny, nx + w * s, ny + h * s)
        if any(min(r[2], q[2]) > max(r[0], q[0]) and min(r[3], q[3]) > max(r[1], q[1]) for q in rects):
            got.add("overwrite")
        rects.append(r)
        if any(float(np.float32(v)) != v for v in raw):
            got.add("fractional")
        if any(math.floor(float(np.float32(v))) != math.floor(v) for v in raw):
            got.add("float32 rounds up")
    if cw != R.MOSAIC_SCENES[name][1] or ch != R.MOSAIC_SCENES[name][2]:
        got.add("fractional canvas")
    return got


def test_every_branch_of_the_kernels_is_reached_by_a_case():
    mosaic = set().union(*[_mosaic_branches(n) for n in R.MOSAIC_SCENES])
    assert mosaic >= {"clip right", "clip bottom", "copy", "resize", "overwrite", "w == 0", "h == 0", "i1 clamps", "scale 1",
                      "scale 2", "scale 4", "1x1 crop", "1xN crop", "fractional", "float32 rounds up", "fractional canvas",
                      "empty"}, mosaic
    assert "float32 rounds up" in _mosaic_branches("fractional") and "overwrite" in _mosaic_branches("overlap")
    # resize + normalise: the same path, no padding, the clamp of the second tap, one-pixel sources and results, both mixed directions
    rc = R.RESIZE_CASES
    assert (1, 1, 5, 7) in [c[:4] for c in rc] and (1, 9, 4, 36) in [c[:4] for c in rc] and (9, 1, 36, 4) in [c[:4] for c in rc]
    assert (37, 53, 1, 1) in [c[:4] for c in rc]
    assert any((nh, nw) == (h, w) for h, w, nh, nw, _, _ in rc)                                        # same
    assert any(nh == h and nw != w for h, w, nh, nw, _, _ in rc)
    assert any(2 * nh == h and 2 * nw == w for h, w, nh, nw, _, _ in rc)
    assert any((ph, pw) == (nh, nw) for _, _, nh, nw, ph, pw in rc)
    assert any(nw > w and nh < h for h, w, nh, nw, _, _ in rc) and any(nw < w and nh > h for h, w, nh, nw, _, _ in rc)
    assert all(ph >= nh and pw >= nw for _, _, nh, nw, ph, pw in rc) and any(ph > nh and pw > nw for _, _, nh, nw, ph, pw in rc)
    for h, w, nh, nw, _, _ in rc[:3]:                                                                  # i1 clamps to src - 1, not by s >= src - 1 alone
        assert all(R.linear_tap(d, nw, w)[1] == w - 1 for d in range(nw) if R.linear_tap(d, nw, w)[0] == w - 1)
    assert any(R.linear_tap(d, 36, 9)[:2] == (8, 8) for d in range(36))
    # bicubic: tap counts, one-pixel shapes, both mixed directions, the identity, letterboxes with odd remainders
    bc = R.BICUBIC_CASES
    assert any(R.ksize(ih, oh) >= 101 for ih, iw, oh, ow in bc) and any(R.ksize(iw, ow) >= 101 for ih, iw, oh, ow in bc)
    assert any(ow > iw and oh < ih for ih, iw, oh, ow in bc) and any(ow < iw and oh > ih for ih, iw, oh, ow in bc)
    assert any((ih, iw) == (1, 1) for ih, iw, _, _ in bc) and any((oh, ow) == (1, 1) for _, _, oh, ow in bc)
    assert any(ih == 1 and iw > 1 for ih, iw, _, _ in bc) and any(iw == 1 and ih > 1 for ih, iw, _, _ in bc)
    assert any((ih, iw) == (oh, ow) for ih, iw, oh, ow in bc) and all(ih <= 100 * iw for ih, iw, _, _ in bc)
    runs = R.bicubic_runs()
    assert sum(lb for _, lb in runs) == len(bc) - 3 and (5, True) not in runs     # one-pixel result, the two 101-tap shapes: a side of 0
    geo = [R.letterbox_geometry(bc[i][:2], bc[i][2:]) + bc[i][2:] for i, lb in runs if lb]
    assert any((H - nh) % 2 == 1 for nh, nw, oy, ox, H, W in geo) and any((W - nw) % 2 == 1 for nh, nw, oy, ox, H, W in geo)
    assert any(oy > 0 for _, _, oy, _, _, _ in geo) and any(ox > 0 for _, _, _, ox, _, _ in geo)
    # beyond the grid cap: the first case for the rows pass, the second for the columns pass
    (ih, iw, oh, ow), (jh, jw, ph, pw) = R.BICUBIC_CAP_CASES
    assert ih * ow > R.GRID_CAP >= oh * ow and ph * pw > R.GRID_CAP >= jh * pw and ih <= 100 * iw
