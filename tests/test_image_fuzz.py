"""GPU: the kernels that turn a decoded frame into a network input, against the references of tests/image_reference.py
(which tests/test_image_reference.py holds to Pillow, to each other and to the exact bilinear on the CPU):

* `glsdet_pil_resize_normalize` against `oracle.preprocess_oracle.drone_preprocess` (Pillow itself),
* `glsdet_ufp_mosaic` against `oracle.ufp_oracle.display_merge_result`,
* `glsdet_resize_normalize_pad[_u8]_ex` against `oracle.ufp_oracle.resize_normalize` at the case's own nh / nw.

The entry points are called through ctypes.  Every destination is a sentinel-filled buffer larger than the call needs and
is compared whole; every comparison is exact."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import preprocess_oracle as P
from oracle import ufp_oracle as U
from tests import image_reference as R

pytestmark = pytest.mark.gpu
SENT = -12345.5
GUARD = 1024                                     # elements behind every destination that must keep the sentinel


@pytest.fixture(scope="module")
def lib():
    from glsdet_amd import _lib
    return _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ bicubic
DRONE_MEAN = (0.485, 0.456, 0.406)
DRONE_STD = (0.229, 0.224, 0.225)
_tables = {}


def _table(n_in, n_out):
    from glsdet_amd.preprocess import pil_bicubic_tables
    if (n_in, n_out) not in _tables:
        b, k, ks = pil_bicubic_tables(n_in, n_out)
        _tables[(n_in, n_out)] = (_dev(b), _dev(k), ks)
    return _tables[(n_in, n_out)]


def _pil(lib, src, out_hw, dst, dst_hw, off, tmp=None, xks=None, yks=None, null=None):
    """one call of glsdet_pil_resize_normalize on device tensors; `dst` is a tensor whose first element is the plane's
    origin.  -> (return code, tmp with its guard bytes)"""
    ih, iw = src.shape[:2]
    oh, ow = out_hw
    xb, xk, xs = _table(iw, ow)
    yb, yk, ys = _table(ih, oh)
    if tmp is None:
        tmp = torch.full((ih * ow * 3 + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")       # exactly in_h * out_w * 3, then guard
    mean, std = (C.c_double * 3)(*DRONE_MEAN), (C.c_double * 3)(*DRONE_STD)
    rc = lib.glsdet_pil_resize_normalize(src.data_ptr(), ih, iw, None if null == "xb" else xb.data_ptr(),
                                         None if null == "xk" else xk.data_ptr(), xs if xks is None else xks, ow,
                                         None if null == "yb" else yb.data_ptr(), None if null == "yk" else yk.data_ptr(),
                                         ys if yks is None else yks, oh, tmp.data_ptr(), dst.data_ptr(), dst_hw[0], dst_hw[1],
                                         off[0], off[1], mean, std, _stream())
    torch.cuda.synchronize()
    return rc, tmp


def _want_plain(img, out_hw):
    return P.drone_preprocess(img, out_hw, False)[0]


@pytest.mark.parametrize("run", R.bicubic_runs(), ids=lambda r: "%dx%d_to_%dx%d" % R.BICUBIC_CASES[r[0]] + ("_letterbox" if r[1] else ""))
def test_bicubic_equals_pillow(lib, run):
    """every case of the table through DronePreprocessor (letterboxed wherever the letterbox exists), and without the
    letterbox once more through the C entry point into a sentinel-filled buffer with a tmp of exactly in_h * out_w * 3 bytes"""
    from glsdet_amd.preprocess import DronePreprocessor
    i, lb = run
    ih, iw, oh, ow = R.BICUBIC_CASES[i]
    img = R.image_u8(ih, iw, 20 + i)
    want = P.drone_preprocess(img, (oh, ow), lb)
    got = DronePreprocessor()([img], (oh, ow), lb)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want)
    if not lb:
        buf = torch.full((3 * oh * ow + GUARD,), SENT, dtype=torch.float32, device="cuda")
        rc, tmp = _pil(lib, _dev(img), (oh, ow), buf, (oh, ow), (0, 0))
        assert rc == 0
        assert np.array_equal(buf[: 3 * oh * ow].cpu().numpy().reshape(3, oh, ow), want[0])
        assert bool((buf[3 * oh * ow:] == SENT).all()) and bool((tmp[ih * ow * 3:] == 0xA5).all())


@pytest.mark.parametrize("corner", [(0, 0), (0, 1), (1, 0), (1, 1)], ids=["top_left", "top_right", "bottom_left", "bottom_right"])
def test_bicubic_window_in_a_corner_of_a_larger_canvas_of_a_batch(lib, corner):
    """The 9 x 11 result goes into a corner of the 30 x 24 canvas of batch entry 1 of 3: the pixels around the window, the
    other two entries, the elements behind the batch and the bytes behind tmp keep their sentinel.  (The canvas leaves
    more room below the window than beside it, so a launch that confused the two offsets would still stay inside it.)"""
    (ih, iw), (oh, ow), (H, W) = (23, 17), (9, 11), (30, 24)
    assert W - ow <= H - oh
    oy, ox = corner[0] * (H - oh), corner[1] * (W - ow)
    img = R.image_u8(ih, iw, 31)
    batch = torch.full((3 * 3 * H * W + GUARD,), SENT, dtype=torch.float32, device="cuda")
    planes = batch[: 3 * 3 * H * W].view(3, 3, H, W)
    rc, tmp = _pil(lib, _dev(img), (oh, ow), planes[1], (H, W), (oy, ox))
    assert rc == 0
    want = np.full((3, 3, H, W), SENT, np.float32)
    want[1, :, oy:oy + oh, ox:ox + ow] = _want_plain(img, (oh, ow))
    assert np.array_equal(planes.cpu().numpy(), want)
    assert bool((batch[3 * 3 * H * W:] == SENT).all()) and bool((tmp[ih * ow * 3:] == 0xA5).all())
    assert not bool((tmp[: ih * ow * 3] == 0xA5).all())


def test_bicubic_tensor_input_and_out_reuse():
    """torch.Tensor sources (host and device) and a caller's `out`, used twice: the second, letterboxed call has to
    overwrite everything the first one left, the gray border included"""
    from glsdet_amd.preprocess import DronePreprocessor
    p = DronePreprocessor()
    a, b, c = R.image_u8(40, 30, 1), R.image_u8(31, 45, 2), R.image_u8(64, 96, 3)
    out = torch.full((3, 3, 64, 96), SENT, dtype=torch.float32, device="cuda")
    got = p([torch.from_numpy(a), torch.from_numpy(b).cuda(), c], (64, 96), False, out=out)
    assert got is out
    for j, im in enumerate((a, b, c)):
        assert np.array_equal(out[j].cpu().numpy(), _want_plain(im, (64, 96))), j
    got = p([torch.from_numpy(c).cuda(), a, torch.from_numpy(b)], (64, 96), True, out=out)
    assert got is out
    for j, im in enumerate((c, a, b)):
        assert np.array_equal(out[j].cpu().numpy(), P.drone_preprocess(im, (64, 96), True)[0]), j
    with pytest.raises(AssertionError):
        p([a], (64, 96), out=out)                                          # a batch of another size


def test_bicubic_refusals_launch_nothing(lib):
    src = _dev(R.image_u8(12, 10, 4))
    buf = torch.full((3 * 8 * 9 + GUARD,), SENT, dtype=torch.float32, device="cuda")

    def refused(word, **kw):
        args = dict(out_hw=(6, 7), dst=buf, dst_hw=(8, 9), off=(0, 0))
        args.update(kw)
        rc, tmp = _pil(lib, src, **args)
        msg = lib.glsdet_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)
        assert bool((buf == SENT).all()) and bool((tmp == 0xA5).all()), word
        return msg

    assert "6x7" in refused("does not fit", off=(3, 0)) and "(3,0)" in lib.glsdet_last_error().decode()      # 3 + 6 > 8
    refused("does not fit", off=(0, 3))                                                                     # 3 + 7 > 9
    refused("does not fit", off=(-1, 0))
    refused("does not fit", off=(0, -1))
    refused("does not fit", dst_hw=(5, 9))
    assert "(x)" in refused("coefficient table", xks=0)
    assert "(y)" in refused("coefficient table", yks=-3)
    for null, axis in (("xb", "(x)"), ("xk", "(x)"), ("yb", "(y)"), ("yk", "(y)")):
        assert axis in refused("coefficient table", null=null)
    rc, _ = _pil(lib, src, (6, 7), buf, (8, 9), (2, 2))                                                     # and the call that fits, runs
    assert rc == 0 and not bool((buf[: 3 * 8 * 9] == SENT).all()) and bool((buf[3 * 8 * 9:] == SENT).all())


@pytest.mark.parametrize("case", R.BICUBIC_CAP_CASES, ids=["rows_pass", "columns_pass"])
def test_bicubic_beyond_the_grid_cap(lib, case):
    """in_h * out_w (the rows pass) or out_h * out_w (the columns pass) just above 65535 * 256 threads: the grid-stride
    loop has to come round a second time"""
    ih, iw, oh, ow = case
    assert max(ih * ow, oh * ow) > R.GRID_CAP
    img = R.image_u8(ih, iw, 40)
    want = torch.from_numpy(_want_plain(img, (oh, ow)))
    buf = torch.full((3 * oh * ow + GUARD,), SENT, dtype=torch.float32, device="cuda")
    rc, tmp = _pil(lib, _dev(img), (oh, ow), buf, (oh, ow), (0, 0))
    assert rc == 0
    assert torch.equal(buf[: 3 * oh * ow].view(3, oh, ow), want.cuda())
    assert bool((buf[3 * oh * ow:] == SENT).all()) and bool((tmp[ih * ow * 3:] == 0xA5).all())


def test_preprocessor_refuses_a_frame_pillow_resamples_vertically_first():
    from glsdet_amd.preprocess import DronePreprocessor
    p = DronePreprocessor()
    ih, iw, oh, ow = R.ORDER_BOUNDARY["beyond"]
    with pytest.raises(ValueError, match="100 \\* in_w"):
        p([R.image_u8(ih, iw, 5)], (oh, ow))
    with pytest.raises(ValueError, match="100 \\* in_w"):
        p([R.image_u8(8, 8, 5), R.image_u8(ih, iw, 5)], (oh, ow))                 # the second of a batch
    ih, iw, oh, ow = R.ORDER_BOUNDARY["at"]                                # the last size on the horizontal-first side is served
    img = R.image_u8(ih, iw, 5)
    assert np.array_equal(p([img], (oh, ow)).cpu().numpy(), P.drone_preprocess(img, (oh, ow), False))


# ------------------------------------------------------------------------------------------------ mosaic
def _mosaic(lib, img, chips_f32, ch, cw):
    """one call of glsdet_ufp_mosaic; chips already floored -> the whole sentinel-filled buffer"""
    buf = torch.full((ch * cw * 3 + GUARD,), SENT, dtype=torch.float32, device="cuda")
    n = len(chips_f32)
    cdev = _dev(np.asarray(chips_f32, np.float32).reshape(-1, 7)) if n else None
    rc = lib.glsdet_ufp_mosaic(img.data_ptr(), img.shape[0], img.shape[1], cdev.data_ptr() if n else None, n, buf.data_ptr(), ch, cw,
                               _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.glsdet_last_error().decode()
    return buf


@pytest.mark.parametrize("name", list(R.MOSAIC_SCENES))
def test_mosaic_scene_equals_display_merge_result(lib, name):
    """through the C entry point (fields floored in float64 here) and through UfpSecondStage.mosaic (floored by the host
    code under test: the `fractional` scene holds 3 - 1e-9, which is 3.0 once it is a float32)"""
    from glsdet_amd.ufp import UfpSecondStage
    chips, w, h = R.MOSAIC_SCENES[name]
    img = R.mosaic_image()
    want = U.display_merge_result(img, chips, w, h)
    ch, cw = math.ceil(h), math.ceil(w)
    assert want.shape == (ch, cw, 3)
    buf = _mosaic(lib, _dev(img), np.floor(np.asarray(chips, np.float64)), ch, cw)
    assert np.array_equal(buf[: ch * cw * 3].cpu().numpy().reshape(ch, cw, 3).astype(np.float64), want)
    assert bool((buf[ch * cw * 3:] == SENT).all())
    got = UfpSecondStage().mosaic(_dev(img), chips, w, h)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy().astype(np.float64), want)
    if name == "empty":
        assert not want.any()                                              # all zero over the sentinel
    else:
        assert want.any()


def test_mosaic_beyond_the_grid_cap(lib):
    """a 4100 x 4093 canvas (more than 65535 * 256 pixels) with a small chip in each corner, checked on the device: zero
    outside the four rectangles, the oracle's values inside"""
    ch, cw = 4100, 4093
    assert ch * cw > R.GRID_CAP
    img = R.mosaic_image()
    #         x1  y1  w  h   nx            ny            s
    chips = [[3, 4, 9, 7, 0, 0, 2],
             [44, 20, 10, 6, cw - 20, 0, 2],                               # clipped at the right border of the image
             [20, 10, 5, 5, 0, ch - 20, 4],
             [30, 30, 8, 9, cw - 8, ch - 9, 1]]                            # the copy path, ends on the last pixel of the canvas
    buf = _mosaic(lib, _dev(img), chips, ch, cw)
    want = torch.zeros(ch, cw, 3, dtype=torch.float32, device="cuda")
    for x1, y1, w, h, nx, ny, s in chips:
        rect = U.display_merge_result(img, [[x1, y1, w, h, 0, 0, s]], w * s, h * s)
        assert rect.any()
        want[ny:ny + h * s, nx:nx + w * s] = torch.from_numpy(rect.astype(np.float32)).cuda()
    assert torch.equal(buf[: ch * cw * 3].view(ch, cw, 3), want)
    assert bool((buf[ch * cw * 3:] == SENT).all())


# ------------------------------------------------------------------------------------------------ resize + normalise
def _resize(lib, src, nh, nw, ph, pw):
    """glsdet_resize_normalize_pad[_u8]_ex, flip 0 -> the whole sentinel-filled buffer"""
    u8 = src.dtype == torch.uint8
    buf = torch.full((3 * ph * pw + GUARD,), SENT, dtype=torch.float32, device="cuda")
    mean, std = (C.c_double * 3)(*R.MEAN_RGB), (C.c_double * 3)(*R.STD_RGB)
    fn = lib.glsdet_resize_normalize_pad_u8_ex if u8 else lib.glsdet_resize_normalize_pad_ex
    rc = fn(src.data_ptr(), src.shape[0], src.shape[1], nh, nw, buf.data_ptr(), ph, pw, mean, std, 0, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.glsdet_last_error().decode()
    return buf


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("i", range(len(R.RESIZE_CASES)), ids=["%dx%d_to_%dx%d_in_%dx%d" % c for c in R.RESIZE_CASES])
def test_resize_normalize_pad_equals_the_oracle_exactly(lib, i, u8):
    """uint8: integer arithmetic, then the same float steps.  float: the same float64 operations in the same order
    (contraction is off in the kernel), so equality is by construction, not by tolerance."""
    h, w, nh, nw, ph, pw = R.RESIZE_CASES[i]
    src = R.resize_source(h, w, u8, i)
    assert np.array_equal(U.MEAN, R.MEAN_RGB) and np.array_equal(U.STD, R.STD_RGB)
    want = np.zeros((3, ph, pw), np.float32)                               # the pad region is exactly 0
    want[:, :nh, :nw] = U.resize_normalize(src, nw, nh)
    buf = _resize(lib, _dev(src), nh, nw, ph, pw)
    got = buf[: 3 * ph * pw].cpu().numpy().reshape(3, ph, pw)
    assert np.array_equal(got, want), "%d elements differ, max %g" % ((got != want).sum(), np.abs(got - want).max())
    assert bool((buf[3 * ph * pw:] == SENT).all())
    if (nh, nw) == (h, w):                                                 # the same size returns the normalised source
        assert np.array_equal(got[:, :nh, :nw], R.normalize_bgr(src.astype(np.float32)))


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
def test_pipeline_input_with_a_small_img_scale(u8):
    """img_scale (64, 32): a 37 x 53 picture becomes 32 x 46 inside 32 x 64; the meta dict is the test pipeline's"""
    from glsdet_amd.ufp import UfpSecondStage
    src = R.resize_source(37, 53, u8, 3)
    want, meta = U.mmdet_test_pipeline(src, img_scale=(64, 32))
    for stage, kw in ((UfpSecondStage(img_scale=(64, 32)), {}), (UfpSecondStage(), dict(img_scale=(64, 32)))):
        got, m = stage.pipeline_input(_dev(src), **kw)
        assert tuple(got.shape) == want.shape == (1, 3, 32, 64)
        assert m["img_shape"] == meta["img_shape"] == (32, 46, 3) and m["pad_shape"] == meta["pad_shape"] == (32, 64, 3)
        assert m["ori_shape"] == meta["ori_shape"] == (37, 53, 3) and m["flip"] is False and m["flip_direction"] is None
        assert m["scale_factor"].dtype == np.float32 and np.array_equal(m["scale_factor"], meta["scale_factor"])
        assert np.array_equal(got.cpu().numpy(), want)
        assert not got[0, :, :, 46:].any()
