"""References and case tables for the kernels that turn a decoded frame into a network input: the PIL bicubic resize
(`glsdet_pil_resize_normalize`), the UFP mosaic (`glsdet_ufp_mosaic`) and the two cv2-style resize + normalise kernels
(`glsdet_resize_normalize_pad[_u8][_ex]`).  TEST INFRASTRUCTURE ONLY; no GPU.

What each kernel is compared with:

* bicubic -- `oracle.preprocess_oracle.drone_preprocess`, which calls Pillow itself: the independent reference.
  `two_pass` below is the kernels' integer arithmetic on the product's host tables, in either pass order; the CPU file
  holds it to `Image.resize` and pins the size boundary at which Pillow changes the order.
* mosaic, uint8 resize -- `oracle.ufp_oracle` (numpy, vectorised).  cv2 is not importable, so that file is a
  restatement; `cv2_linear_u8_scalar` here is a second one, written from the description in that file's docstring
  (per output pixel, Python ints), and `bilinear_exact` is the real-valued bilinear on the same taps.  The CPU file
  holds the two restatements to each other bit for bit and both to the exact value within `FIXED_POINT_BOUND`.
* float resize -- the oracle's float64 bilinear; the kernel makes the same float64 operations in the same order
  (contraction off), so the comparison is exact.

The case tables are data; `tests/test_image_reference.py` computes from them that every branch of the kernels is
reached."""
import math

import numpy as np

F32 = np.float32

# ------------------------------------------------------------------------------------------------ bicubic
# (in_h, in_w, out_h, out_w).  Every case keeps in_h <= 100 * in_w: above that, with a shrinking height, Pillow's
# Image.resize runs the VERTICAL pass first (PIL/Image.py), the kernels always the horizontal one, and the two orders
# differ in a quarter of the pixels.  The product refuses such frames (glsdet_amd.preprocess.pil_pass_order); they are
# not behaviour to compare.  The boundary itself is pinned on the CPU (ORDER_BOUNDARY below).
BICUBIC_CASES = [
    (77, 123, 64, 96),        # both down
    (31, 45, 64, 96),         # both up
    (40, 30, 20, 90),         # width up, height down
    (30, 40, 90, 20),         # width down, height up
    (1, 1, 5, 7),             # one source pixel
    (37, 53, 1, 1),           # one output pixel
    (1, 9, 4, 36),            # a 1-high source
    (9, 1, 36, 4),            # a 1-wide source
    (500, 24, 20, 33),        # vertical tap count 101 (scale 25), width up
    (24, 500, 33, 20),        # horizontal tap count 101
    (16, 24, 16, 24),         # same size: both passes are the identity
    (33, 20, 65, 50),         # letterboxed: odd remainders
    (21, 32, 21, 50),         # the height stays
]
# (in_h, in_w, out_h, out_w) on the two sides of Pillow's order rule `in_h > 100 * in_w and out_h < in_h`
ORDER_BOUNDARY = dict(at=(800, 8, 64, 13), beyond=(801, 8, 64, 13))
# beyond the grid cap of 65535 x 256 threads, one per kernel: in_h * out_w for the rows pass, out_h * out_w for the columns
GRID_CAP = 65535 * 256
BICUBIC_CAP_CASES = [(4200, 48, 8, 4000), (40, 40, 4100, 4100)]


def ksize(n_in, n_out):
    """tap count of Pillow's bicubic table (support 2 * max(scale, 1))"""
    return int(math.ceil(2.0 * max(float(n_in) / n_out, 1.0))) * 2 + 1


def letterbox_geometry(in_hw, canvas_hw):
    """utils.py:24-31 -> (nh, nw, oy, ox); nh or nw may be 0, which Pillow refuses: such a case has no letterbox"""
    (ih, iw), (H, W) = in_hw, canvas_hw
    scale = min(W / iw, H / ih)
    nw, nh = int(iw * scale), int(ih * scale)
    return nh, nw, (H - nh) // 2, (W - nw) // 2


def bicubic_runs():
    """-> [(case index, letterbox)] for every case, letterboxed wherever the letterbox exists"""
    runs = []
    for i, (ih, iw, oh, ow) in enumerate(BICUBIC_CASES):
        runs.append((i, False))
        nh, nw, _, _ = letterbox_geometry((ih, iw), (oh, ow))
        if nh >= 1 and nw >= 1:
            runs.append((i, True))
    return runs


def image_u8(h, w, seed):
    """uint8 HWC noise with saturated patches (the clip8 of the bicubic overshoot needs 0 next to 255)"""
    rng = np.random.default_rng([seed, h, w, 0x1A6E])
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    img[: max(1, h // 3), : max(1, w // 3)] = 255
    img[h - max(1, h // 4):, w - max(1, w // 4):] = 0
    if h > 2 and w > 2:
        img[h // 2, :, :] = np.where(np.arange(w)[:, None] % 2 == 0, 255, 0)         # a line of alternating extremes
    return img


def _one_pass(a, n_out):
    """resample axis 1 of uint8 [rows, n_in, 3] with the product's tables, in Pillow's fixed point"""
    from glsdet_amd.preprocess import pil_bicubic_tables
    b, k, _ = pil_bicubic_tables(a.shape[1], n_out)
    out = np.empty((a.shape[0], n_out, 3), np.uint8)
    for xx in range(n_out):
        x0, cnt = int(b[xx, 0]), int(b[xx, 1])
        s = (1 << 21) + (a[:, x0:x0 + cnt].astype(np.int64) * k[xx, :cnt].astype(np.int64)[None, :, None]).sum(1)
        out[:, xx] = np.clip(s >> 22, 0, 255)
    return out


def two_pass(img, out_hw, order="hv"):
    """the kernels' arithmetic: 'hv' horizontal then vertical (what the device does), 'vh' the other order"""
    oh, ow = out_hw
    if order == "hv":
        return _one_pass(_one_pass(img, ow).transpose(1, 0, 2), oh).transpose(1, 0, 2)
    assert order == "vh"
    return _one_pass(_one_pass(img.transpose(1, 0, 2), oh).transpose(1, 0, 2), ow)


def normalize_drone(u8_hwc):
    """preprocess_input + HWC -> CHW on an already resized uint8 picture (numpy's mixed float32 / float64 steps)"""
    f = u8_hwc.astype(np.float32)
    f /= 255.0
    f -= np.array([0.485, 0.456, 0.406])
    f /= np.array([0.229, 0.224, 0.225])
    return np.ascontiguousarray(f.transpose(2, 0, 1))


# ------------------------------------------------------------------------------------------------ cv2 INTER_LINEAR, twice more
def linear_tap(d, dst, src):
    """OpenCV's per-axis set-up for output index d: -> (i0, i1, fraction as float32).  The scale is the reciprocal of the
    double ratio dst / src, the source coordinate is rounded to float32 once, taps beyond either border collapse onto
    the border pixel with fraction 0."""
    scale = 1.0 / (float(dst) / float(src))
    f = F32((d + 0.5) * scale - 0.5)
    s = int(math.floor(float(f)))
    f = F32(f - F32(s))
    if s < 0:
        s, f = 0, F32(0)
    if s >= src - 1:
        s, f = src - 1, F32(0)
    return s, min(s + 1, src - 1), f


def _coef(f):
    """the two 11-bit coefficients of a fraction: (1 - f) and f, each times 2048, rounded to nearest even"""
    return int(round(float(F32(1) - f) * 2048.0)), int(round(float(f) * 2048.0))


def cv2_linear_u8_scalar(src, dw, dh, mutate=None):
    """cv2.resize(src, (dw, dh), INTER_LINEAR) on uint8 HWC, one output pixel at a time in Python ints: the horizontal
    pass keeps 11 fraction bits (r = p0 * a0 + p1 * a1), the vertical pass is
    ((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16), then (+ 2) >> 2 and the cast to uint8.  An equal size is a copy.
    mutate (the mutation check only): 'round4' rounds r0 >> 4 instead of truncating it."""
    sh, sw = src.shape[:2]
    if (sw, sh) == (dw, dh):
        return src.copy()
    out = np.empty((dh, dw, src.shape[2]), np.uint8)
    xt = [linear_tap(x, dw, sw) for x in range(dw)]
    for y in range(dh):
        y0, y1, fy = linear_tap(y, dh, sh)
        b0, b1 = _coef(fy)
        for x in range(dw):
            x0, x1, fx = xt[x]
            a0, a1 = _coef(fx)
            for c in range(src.shape[2]):
                r0 = int(src[y0, x0, c]) * a0 + int(src[y0, x1, c]) * a1
                r1 = int(src[y1, x0, c]) * a0 + int(src[y1, x1, c]) * a1
                if mutate == "round4":
                    r0 += 8
                v = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
                out[y, x, c] = min(max(v, 0), 255)
    return out


def bilinear_exact(src, dw, dh):
    """the real-valued bilinear on the same taps and the same float32 fractions, in float64 -> [dh, dw, c].
    (Pixels are integers below 2^8 and fractions have 24 bits, so every product is exact in float64 and the three sums
    round at 2^-45: exact for the purpose of a bound of one grey level.)"""
    sh, sw = src.shape[:2]
    s = src.astype(np.float64)
    out = np.empty((dh, dw, src.shape[2]))
    for y in range(dh):
        y0, y1, fy = linear_tap(y, dh, sh)
        for x in range(dw):
            x0, x1, fx = linear_tap(x, dw, sw)
            fx_, fy_ = float(fx), float(fy)
            top = s[y0, x0] * (1.0 - fx_) + s[y0, x1] * fx_
            bot = s[y1, x0] * (1.0 - fx_) + s[y1, x1] * fx_
            out[y, x] = top * (1.0 - fy_) + bot * fy_
    return out


# How far the fixed-point pixel v may lie from the exact bilinear E (both in grey levels), from the arithmetic alone:
#   coefficients  a = rint(2048 w) with w = fx or the float32 difference 1 - fx (off by at most 2^-25): |a - 2048 w| <= EC;
#                 a0 + a1 <= 2049, likewise b0 + b1.
#   horizontal    r = p0 a0 + p1 a1 = 2048 h + e, |e| <= 2 * 255 * EC, with h the exact horizontal value; r <= 255 * 2049.
#   r >> 4        t = floor(r / 16), an integer r: 0 <= r / 16 - t <= 15/16;  t <= TMAX = floor(255 * 2049 / 16).
#   (b t) >> 16   u = floor(b t / 65536): 0 <= b t / 65536 - u < 1, twice.
#   (u0+u1+2)>>2  rounds (u0 + u1) / 4 half up: the result minus (u0 + u1) / 4 is in {0, -1/4, +1/2, +1/4}.
#   One grey level is 2048 * 2048 = 16 * 65536 * 4 units of b * r.  So v - E is made of
#     horizontal coefficients  +- (b0 + b1) * 510 EC / 2048^2          <= 2049 * 510 EC / 2^22
#     vertical coefficients    +- 2 EC * TMAX / (65536 * 4)
#     the shift by 4           in [-(b0 + b1) * (15/16) / (65536 * 4), 0]
#     the shift by 16          in (-2/4, 0]
#     the final rounding       in [-1/4, +1/2]
#   and the cast to uint8 only moves v towards E, which lies in [0, 255].
_EC = 0.5 + 2.0 ** -14
_TMAX = (255 * 2049) // 16
_COEF = 2049 * 510 * _EC / 2.0 ** 22 + 2 * _EC * _TMAX / 262144.0
FIXED_POINT_BOUND = (-(_COEF + 2049 * (15.0 / 16.0) / 262144.0 + 0.5 + 0.25), _COEF + 0.5)      # about (-1.007, +0.749)


# ------------------------------------------------------------------------------------------------ mosaic scenes
MOSAIC_IMAGE_HW = (40, 50)
# name -> (chips [x1, y1, w, h, nx, ny, s], canvas width, canvas height).  A chip's crop is img[y1:y1+h, x1:x1+w] clipped
# by the image border, magnified to (w s) x (h s) and written at (nx, ny); every field is floored first; a later chip
# overwrites an earlier one.  Contract (the reference script raises outside it): x1 < W, y1 < H, the rectangle inside the
# canvas.
MOSAIC_SCENES = {
    "clip": ([[44, 5, 10, 8, 0, 0, 1],            # clipped by the right border at scale 1: a 6-wide crop stretched to 10
              [10, 36, 6, 7, 12, 0, 2],           # clipped by the bottom border, scale 2
              [47, 38, 5, 4, 26, 0, 4],           # clipped by both, scale 4
              [3, 4, 9, 11, 0, 20, 1],            # inside, scale 1: the copy path
              [20, 10, 7, 5, 12, 20, 2],          # inside, scale 2
              [30, 20, 4, 3, 30, 20, 4]],         # inside, scale 4, ends 2 short of the canvas edge
             48, 32),
    "overlap": ([[0, 0, 12, 10, 2, 3, 2],         # 24 x 20 at (2, 3)
                 [20, 15, 8, 8, 10, 8, 1],        # wholly inside the first: the later one wins
                 [0, 0, 12, 10, 14, 12, 1],       # inside the first, partly over the second
                 [49, 39, 1, 1, 30, 24, 4],       # a 1 x 1 crop (the last pixel of the image)
                 [5, 7, 5, 1, 28, 0, 2],          # a 1-high crop
                 [9, 2, 1, 6, 36, 4, 4]],         # a 1-wide crop, ends at the canvas edge
                40, 30),
    "zero": ([[5, 5, 0, 6, 0, 0, 2],              # w == 0
              [5, 5, 6, 0, 0, 0, 2],              # h == 0
              [11, 13, 6, 5, 3, 2, 2],
              [2, 2, 0, 0, 4, 4, 4]],
             20, 14),
    # fractional fields: 3 - 1e-9 is 3.0 in float32 (the host has to floor in float64), 1 - 1e-9 floors to a width of 0
    "fractional": ([[3 - 1e-9, 4.7, 6.5, 5.99, 2.2, 1.9, 2.0],
                    [8.5, 9.25, 1 - 1e-9, 4.0, 0.0, 0.0, 2.0],
                    [45.99, 2.5, 7.75, 3.999, 15.5, 2.01, 1.0]],      # clipped: x1 = 45, w = 7 -> 5 columns
                   22.3, 12.5),
    # an 11 x 11 corner stretched to 28 x 26: fractions that are dyadic on neither axis.  On dyadic ones (an unclipped chip
    # at scale 2 or 4) r is a multiple of 16 and `r >> 4` loses nothing, so only such a crop pins that shift to truncation
    # (five of its pixels change when it rounds: tests/test_image_reference.py)
    "stretch": ([[39, 29, 14, 13, 0, 0, 2]], 28, 26),
    "empty": ([], 7.2, 5.0),
}


def floored(chips):
    """the seven fields as the reference floors them (math.floor on Python floats) -> int rows"""
    return [[int(math.floor(v)) for v in c] for c in chips]


def mosaic_image():
    """BGR noise without flat patches: the chips clipped by both borders take the bottom right corner, and a constant
    crop would resize to itself under any coefficients"""
    h, w = MOSAIC_IMAGE_HW
    return np.random.default_rng([77, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)


def mosaic_crops(name):
    """-> [(crop uint8, dw, dh)] for the chips of a scene that draw anything"""
    img = mosaic_image()
    out = []
    for x1, y1, w, h, nx, ny, s in floored(MOSAIC_SCENES[name][0]):
        if w and h:
            out.append((img[y1:y1 + h, x1:x1 + w], w * s, h * s))
    return out


# ------------------------------------------------------------------------------------------------ resize + normalise cases
# (h, w, nh, nw, ph, pw): a source of h x w resized to nh x nw inside a zero-padded ph x pw
RESIZE_CASES = [
    (1, 1, 5, 7, 8, 8),               # one source pixel
    (1, 9, 4, 36, 6, 40),             # 1 x N, four-fold up: the second tap clamps on the right
    (9, 1, 36, 4, 40, 6),             # N x 1
    (37, 53, 1, 1, 3, 5),             # one output pixel
    (20, 30, 10, 15, 12, 16),         # an exact 2x reduction (every fraction is 0.5)
    (17, 23, 17, 40, 20, 41),         # nh == h, nw != w
    (13, 19, 13, 19, 16, 32),         # the same size: the uint8 kernel copies
    (21, 34, 29, 45, 29, 45),         # ph == nh and pw == nw: no padding
    (40, 30, 25, 47, 32, 64),         # width up, height down
    (30, 40, 47, 25, 64, 32),         # width down, height up
    (37, 53, 23, 31, 32, 32),         # both down, not by an integer
]
MEAN_RGB = (123.675, 116.28, 103.53)
STD_RGB = (58.395, 57.12, 57.375)


def resize_source(h, w, u8, seed):
    """BGR source of a resize case: uint8, or float32 with fractions (the mosaic is integral; the kernel must not rely on it)"""
    rng = np.random.default_rng([seed, h, w, int(u8)])
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if u8:
        return img
    return (img.astype(np.float32) + rng.random((h, w, 3), dtype=np.float32)).astype(np.float32)


def normalize_bgr(img_hwc):
    """Normalize(to_rgb) of the test pipeline on a float picture -> CHW float32 (mixed float32 / float64 like mmcv)"""
    rgb = img_hwc[:, :, ::-1].astype(np.float32)
    rgb = (rgb.astype(np.float64) - np.array(MEAN_RGB)).astype(np.float32)
    rgb = (rgb.astype(np.float64) * (1.0 / np.array(STD_RGB))).astype(np.float32)
    return np.ascontiguousarray(rgb.transpose(2, 0, 1))
