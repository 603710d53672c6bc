"""Placements of NHWC views far from their allocation's base, as plain integers (no torch, no GPU).

tests/test_far_addresses.py puts every operand of every view-taking entry point into ONE device buffer of BUF_BYTES bytes
filled with the sentinel byte 0x5A.  The kernels see the part of it that starts ALLOC_LO bytes in as "the allocation"
(glsdet_view.alloc_lo .. alloc_hi), so a view's base, its image stride, or both are more than 2^31 bytes away from
alloc_lo:

    name   base (bytes from the buffer's start)     image stride sn (bytes)
    mid    4 GiB + 1 MiB                            2^31 + 2^20 + 256
    far    4 GiB + 1 MiB                            2^32 + 3 * 2^20 + 256
    base   4 GiB + 2^31 + 1 MiB + 4096              dense

Within an image the strides are those of the "window" kind of tests/test_conv_exact.py (`Placed`): a channel slice inside
a wider pixel, with a spatial margin.  The k-th operand of a test sits SLOT bytes after the (k - 1)-th.

Why the allocation starts 4 GiB in: a kernel that truncates an offset to 32 bits -- a byte offset or an element offset,
signed or unsigned, counted from the view's base or from alloc_lo -- must still address inside the buffer (a fault on a
shared card is not a test result), and must land where no operand of the test lives, so that it reads or writes sentinel
and shows as a wrong value or as "bytes outside the destination changed".  `truncation_images` lists those landing
places; tests/test_far_reference.py proves both properties for every slot and the largest block a test may place.

The conv family reads its input through 32-bit descriptor offsets and refuses an input allocation of 2^31 - 1 bytes or
more ("exceeds the 2 GiB descriptor range").  Its input placements are prefixes of the same buffer (EDGE, JUST_IN,
JUST_OUT, OVER): image 0 of the `edge_view` starts at byte 0 and image 1 ends with the last 16 bytes of EDGE."""
from collections import namedtuple

KiB, MiB, GiB = 1 << 10, 1 << 20, 1 << 30
BUF_BYTES = 8 * GiB + 64 * MiB
ALLOC_LO = 4 * GiB                      # views are handed to the kernels as views of buf[ALLOC_LO:]
SLOT = 4 * MiB                          # distance between the operands of one test
MAX_BLOCK = MiB - 256                   # one image with its margins is at most this large, and a test has at most
MAX_SLOTS = 15                          # ... this many far operands: tests/test_far_reference.py proves the rest from these two
SENTINEL_BYTE = 0x5A
VEC = 16                                # bytes of one vector access: every image starts on a multiple of it

Placement = namedtuple("Placement", "name base sn_bytes")          # sn_bytes None: dense
MID = Placement("mid", 4 * GiB + 1 * MiB, 2 ** 31 + 2 ** 20 + 256)
FAR = Placement("far", 4 * GiB + 1 * MiB, 2 ** 32 + 3 * 2 ** 20 + 256)
BASE = Placement("base", 4 * GiB + 2 ** 31 + 1 * MiB + 4096, None)
PLACEMENTS = (MID, FAR, BASE)
ROLES = ("inputs", "output", "both")    # which operands are far

# conv-family input allocations: prefixes of the buffer
EDGE = 2 ** 31 - 256                    # the largest multiple of 256 the guard admits
JUST_IN, JUST_OUT, OVER = 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31
LIMIT_TEXT = "2 GiB descriptor range"   # the library's wording (conv.hip, conv_csp.hip)
SPAN_TEXT = "does not apply"            # ... and that of a variant whose 32-bit y / res offsets do not reach


def geometry(kind, h, w, c):
    """(H, W, Ct, h0, w0, c0) of tests/test_conv_exact.py's `Placed`: the padded image and the view's corner in it"""
    if kind == "dense":
        return h, w, c, 0, 0, 0
    if kind == "slice":
        return h, w, c + 24, 0, 0, 16
    if kind == "window":
        return h + 3, w + 2, c + 24, 2, 1, 16
    assert kind == "ring", kind
    return h + 2, w + 2, c + 16, 1, 1, 8


View = namedtuple("View", "off sn sh sw n h w c es block0 block_bytes H W Ct index")
# off, sn, sh, sw: TView arguments, in ELEMENTS, off counted from ALLOC_LO; block0: byte offset (from the buffer's start)
# of image 0 with its margins, block_bytes its size; image b's block starts at block0 + b * sn * es


def place(p, slot, n, h, w, c, es, kind="window"):
    H, W, Ct, h0, w0, c0 = geometry(kind, h, w, c)
    block = H * W * Ct * es
    sn_bytes = p.sn_bytes if p.sn_bytes is not None else block
    assert sn_bytes % es == 0 and sn_bytes % VEC == 0 and (Ct * es) % VEC == 0 and (c0 * es) % VEC == 0
    block0 = p.base + slot * SLOT
    assert block0 % VEC == 0 and 0 <= slot < MAX_SLOTS and block <= MAX_BLOCK, (slot, block)
    sw, sh, sn = Ct, W * Ct, sn_bytes // es
    off = (block0 - ALLOC_LO) // es + h0 * sh + w0 * sw + c0
    index = (slice(None), slice(h0, h0 + h), slice(w0, w0 + w), slice(c0, c0 + c))
    return View(off, sn, sh, sw, n, h, w, c, es, block0, block, H, W, Ct, index)


def live_ranges(v):
    """byte ranges [lo, hi) of the buffer that the view's images (with their margins) occupy"""
    return [(v.block0 + b * v.sn * v.es, v.block0 + b * v.sn * v.es + v.block_bytes) for b in range(v.n)]


def _wrap(x, signed):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if signed and x >= (1 << 31) else x


def truncation_images(p, n, h, w, c, es, slot=0, kind="window"):
    """Where a kernel that truncates an offset to 32 bits would address instead of each image of the view: byte ranges
    [lo, hi) from the buffer's start.  The offset is the image's byte offset or element offset, taken as signed or
    unsigned, counted from the view's block or from alloc_lo; offsets inside an image are far below 2^31 and move the
    range rigidly.  Truncations that change nothing are left out."""
    v = place(p, slot, n, h, w, c, es, kind)
    return block_truncations(v.block0, v.sn * es, n, v.block_bytes, es)


def block_truncations(block0, sn_bytes, n, block_bytes, es):
    """truncation_images for n blocks of block_bytes bytes, sn_bytes apart, the first at byte block0 of the buffer"""
    out = set()
    for b in range(n):
        true = block0 + b * sn_bytes
        for origin in (block0, ALLOC_LO):
            d = true - origin                                     # a byte offset; d // es the element offset
            for signed in (False, True):
                for got in (_wrap(d, signed), _wrap(d // es, signed) * es):
                    if got != d:
                        out.add((origin + got, origin + got + block_bytes))
    return sorted(out)


# ------------------------------------------------------------------------------------------- conv-family input at the edge
EdgeView = namedtuple("EdgeView", "off sn sh sw n h w c es span_bytes")


def edge_view(n, h, w, c, es, alloc=EDGE):
    """x for the conv family inside buf[:alloc]: a channel slice of a wider pixel in a wider row; image 0 starts AT byte 0
    (with pad 1 its negative tap offsets wrap below x_off = 0), the last element of image n - 1 lies in the last 16 bytes"""
    sw, sh = c + 24, (w + 2) * (c + 24)
    span = (h - 1) * sh + (w - 1) * sw + c                          # elements of one image, first to last
    assert alloc % (VEC * 16) == 0 and (span * es) % VEC == 0 and n >= 2
    sn = (alloc // es - span) // (n - 1)
    assert (sn * es) % VEC == 0 and (n - 1) * sn + span == alloc // es, "image n - 1 must end with the allocation"
    return EdgeView(0, sn, sh, sw, n, h, w, c, es, span * es)


def edge_ranges(v):
    return [(b * v.sn * v.es, b * v.sn * v.es + v.span_bytes) for b in range(v.n)]


# ----------------------------------------------------------------------------------------------------------- the cases
# entry point -> the test of tests/test_far_addresses.py that places its views far.  tests/test_far_reference.py demands an
# entry for every export of glsdet_amd._lib._SIGS that takes a view or a conv descriptor (the *_tune names measure, they
# compute nothing new) and that the named test exists; a test of the RAW kind runs the case RAW_OPS[name] of that module.
RAW = "test_raw_pointer_operation_far"
EDGE_TEST = "test_conv_family_input_at_the_edge_of_the_descriptor_range"
OUT_TEST = "test_chain_bottleneck_gnstats_multi_outputs_far"
FAR_CASES = {
    # the conv family: input at the edge of / past the descriptor range, outputs far
    "glsdet_conv2d": "test_conv2d_output_and_residual_far",
    "glsdet_conv2d_multi": OUT_TEST, "glsdet_conv2d_chain": OUT_TEST, "glsdet_bottleneck": OUT_TEST, "glsdet_conv2d_gnstats": OUT_TEST,
    "glsdet_csp_fused": "test_csp_fused_refuses_a_far_output",
    # raw-pointer operations: mid, far and base; inputs, output, both
    "glsdet_dwconv2d": RAW, "glsdet_dwconv2d_dilated": RAW, "glsdet_conv2d_grouped": RAW,
    "glsdet_maxpool2d": RAW, "glsdet_spp_pools": RAW, "glsdet_channel_maxmean": RAW, "glsdet_resample_copy": RAW, "glsdet_copy_many": RAW,
    "glsdet_transpose_many": RAW, "glsdet_pool2d": RAW, "glsdet_upsample_add": RAW,
    "glsdet_focus_pack": RAW, "glsdet_nchw_pack": RAW,
    "glsdet_focus_conv": RAW, "glsdet_focus_conv_down": RAW, "glsdet_resnet_stem": RAW, "glsdet_resnet_stem_pool": RAW,
    "glsdet_groupnorm": RAW, "glsdet_groupnorm_multi": RAW, "glsdet_groupnorm_multi_pre": RAW, "glsdet_proxy_scores": RAW,
    "glsdet_attn_split": RAW, "glsdet_rowsplit": RAW, "glsdet_scale_by_map": RAW, "glsdet_gate": RAW,
    "glsdet_nonlocal": RAW, "glsdet_nonlocal_multi": RAW, "glsdet_nonlocal_split": RAW, "glsdet_nonlocal_mfma": RAW,
    "glsdet_lvc_encode": RAW, "glsdet_channel_fuse": RAW,
    "glsdet_layernorm": RAW, "glsdet_patch_merge": RAW, "glsdet_window_attention": RAW,
    "glsdet_yolox_decode": RAW, "glsdet_yolox_decode_ex": RAW,
    "glsdet_gfl_detect": "test_gfl_cls_and_reg_views_far", "glsdet_gfl_candidates": "test_gfl_cls_and_reg_views_far",
}
# RAW_OPS keys that run a second entry point in the same case
RAW_PAIRS = {"glsdet_focus_conv_down": "glsdet_focus_conv", "glsdet_resnet_stem_pool": "glsdet_resnet_stem"}
