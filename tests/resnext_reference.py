"""Reference of the grouped 3x3 conv (glsdet_conv2d_grouped) and of the ResNeXt trunk built on it
(tests/test_resnext_reference.py, tests/test_conv_grouped_exact.py, tests/test_resnext.py).

numpy float64 / int64 and torch-CPU only; nothing of the engine is imported.

  grouped_conv        the definition: per group tests/conv_reference.conv on the group's channels, concatenated
  expand              the block-diagonal dense weights [C, C, 3, 3] of a grouped conv
  unpack_blocks       the packed operand of include/glsdet_hip.h ([ceil(C / 32)][9][32][32]) -> weights [C, Cg, 3, 3] and
                      whether everything outside the diagonal blocks is an exact zero
  blocks_conv         the conv AS THE KERNEL READS IT: per 32-channel block, the packed 32 x 32 tiles against the block's
                      input channels; `mutate` plants the mistakes a kernel of this layout can make
  case_data           the exact regime of tests/conv_reference.py for a grouped case (ternary weights, small-integer
                      images, 12-bit scales, dyadic biases; check_regime asserts it)
  bottleneck / resnext   torch-CPU restatement of resnext.py:12-85 / the trunk (the dtype of its operands)
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_reference as R

BN_EPS = 1e-5
STAGE_BLOCKS = {50: (3, 4, 6, 3), 101: (3, 4, 23, 3)}
MUTATIONS = ("group_shift", "ci_perm", "s2_origin", "zero_fill", "oob_next_row")


# ----------------------------------------------------------------------------------------------------------- the conv
def grouped_conv(x, w, groups, stride=1, pad=1):
    """x [n, C, h, w], w [C, Cg, R, S] -> accumulator [n, C, ho, wo] (int64 for integer operands, else float64)"""
    x, w = np.asarray(x), np.asarray(w)
    c, cg = w.shape[0], w.shape[1]
    assert c == groups * cg == x.shape[1], (x.shape, w.shape, groups)
    return np.concatenate([R.conv(x[:, g * cg:(g + 1) * cg], w[g * cg:(g + 1) * cg], stride, pad) for g in range(groups)], 1)


def grouped_abs_sum(x, w, groups, stride=1, pad=1):
    return grouped_conv(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)), groups, stride, pad)


def expand(w, groups):
    w = np.asarray(w)
    c, cg = w.shape[0], w.shape[1]
    assert c == groups * cg
    dense = np.zeros((c, c) + w.shape[2:], w.dtype)
    for g in range(groups):
        dense[g * cg:(g + 1) * cg, g * cg:(g + 1) * cg] = w[g * cg:(g + 1) * cg]
    return dense


def unpack_blocks(packed, groups, cg):
    """packed [nblk, 9, 32, 32] = [block][tap][co_l][ci_l] -> (w [C, Cg, 3, 3], outside_is_zero)"""
    packed = np.asarray(packed)
    c = groups * cg
    nblk = (c + 31) // 32
    assert packed.shape == (nblk, 9, 32, 32), packed.shape
    w = np.zeros((c, cg, 3, 3), packed.dtype)
    inside = np.zeros(packed.shape, bool)
    for co in range(c):
        b, co_l, ci0 = co // 32, co % 32, ((co // cg) * cg) % 32
        w[co] = packed[b, :, co_l, ci0:ci0 + cg].T.reshape(cg, 3, 3)
        inside[b, :, co_l, ci0:ci0 + cg] = True
    return w, bool((packed[~inside] == 0).all())


def _wrap_pad(x):
    """[n, c, h, w] -> [n, c, h + 2, w + 2]: zero rows above and below, but the column left / right of a row holds what
    lies before / behind that row in memory (the last pixel of the previous row, the first of the next)"""
    n, c, h, w = x.shape
    xp = np.zeros((n, c, h + 2, w + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    xp[:, :, 1:h, w + 1] = x[:, :, 1:, 0]
    xp[:, :, 2:h + 1, 0] = x[:, :, :-1, w - 1]
    return xp


def blocks_conv(x, packed, stride=1, mutate=None, cg=None):
    """The conv over packed 32 x 32 tiles: output channels [32 b, 32 b + 32) from input channels of the same range.
    mutate: 'group_shift' a group reads the next group's input channels; 'ci_perm' the input channels of a block in reverse
    order; 's2_origin' the window of output pixel o starts at o * stride instead of o * stride - 1; 'zero_fill' the zero
    cells of a tile hold the neighbouring group's weights; 'oob_next_row' a tap left / right of the map reads the
    neighbouring row's pixel."""
    x, packed = np.asarray(x), np.asarray(packed)
    assert mutate is None or mutate in MUTATIONS
    n, c, h, w = x.shape
    nblk = packed.shape[0]
    if mutate == "group_shift":
        x = np.roll(x, -cg, axis=1)
    xp = np.zeros((n, nblk * 32, h, w), x.dtype)
    xp[:, :c] = x
    outs = []
    for b in range(nblk):
        xb = xp[:, 32 * b:32 * b + 32]
        wb = packed[b].reshape(3, 3, 32, 32).transpose(2, 3, 0, 1)          # [co_l, ci_l, r, s]
        if mutate == "ci_perm":
            xb = xb[:, ::-1]
        if mutate == "zero_fill":
            wb = wb.copy()
            for co_l in range(32):
                ci0 = (co_l // cg) * cg
                for g in range(32 // cg):
                    if g * cg != ci0:
                        wb[co_l, g * cg:(g + 1) * cg] = wb[(co_l + g * cg - ci0) % 32, g * cg:(g + 1) * cg]
        if mutate == "s2_origin":
            acc = R.conv(np.pad(xb, ((0, 0), (0, 0), (0, 2), (0, 2))), wb, stride, 0)[:, :, :(h - 1) // stride + 1, :(w - 1) // stride + 1]
        elif mutate == "oob_next_row":
            acc = R.conv(_wrap_pad(xb), wb, stride, 0)
        else:
            acc = R.conv(xb, wb, stride, 1)
        outs.append(acc)
    return np.concatenate(outs, 1)[:, :c]


def pack_blocks_np(w):
    """the layout of include/glsdet_hip.h, stated independently of glsdet_amd.torch_ops.grouped_weight_blocks"""
    w = np.asarray(w)
    c, cg = w.shape[0], w.shape[1]
    nblk = (c + 31) // 32
    out = np.zeros((nblk, 9, 32, 32), w.dtype)
    for co in range(c):
        ci0 = ((co // cg) * cg) % 32
        out[co // 32, :, co % 32, ci0:ci0 + cg] = w[co].reshape(cg, 9).T
    return out


# ---------------------------------------------------------------------------------------------------------- the cases
# dst: 'dense' | 'slice' | 'window' (tests/test_conv_exact.Placed); xin: 'ring' (NaN on all sides) always
GCase = namedtuple("GCase", "name groups cg n stride h w act dst")


def _g(groups, cg, n, stride, h, w, act, dst):
    return GCase("g%d_cg%d_n%d_s%d_%dx%d_%s_%s" % (groups, cg, n, stride, h, w, act, dst), groups, cg, n, stride, h, w, act, dst)


# The kernel walks 16-pixel groups of the flat pixel range, four per workgroup: 8 x 8 = 64 pixels is exactly one workgroup's
# step, 9 x 9 one pixel more in each direction; 1 x 1, 2 x 3, 7 x 5 lie inside one group / one step.  C = 8 is below one
# 32-channel block, 24 and 80 end in a block tail, 128 .. 2048 are whole blocks.  Stride 2 on even and odd extents
# (8 -> 4, 9 -> 5).  25 x 42 is the C5 map of the benchmark.
GROUPED_CASES = [
    _g(2, 4, 1, 1, 1, 1, "none", "dense"),
    _g(2, 4, 3, 1, 2, 3, "relu", "slice"),
    _g(2, 4, 1, 2, 9, 9, "relu", "window"),
    _g(3, 8, 1, 1, 7, 5, "relu", "window"),
    _g(3, 8, 3, 2, 8, 8, "none", "slice"),
    _g(5, 16, 1, 1, 8, 8, "relu", "dense"),
    _g(5, 16, 3, 1, 9, 9, "none", "window"),
    _g(5, 16, 1, 2, 9, 8, "relu", "slice"),
    _g(32, 4, 1, 1, 25, 42, "relu", "slice"),
    _g(32, 4, 3, 2, 8, 9, "none", "window"),
    _g(64, 4, 1, 1, 9, 9, "relu", "slice"),
    _g(64, 4, 1, 2, 8, 8, "relu", "dense"),
    _g(32, 32, 1, 1, 5, 7, "relu", "slice"),
    _g(32, 32, 1, 2, 5, 7, "none", "window"),
    _g(64, 32, 1, 1, 3, 4, "relu", "dense"),
]
# the launch has ONE cap: 768 workgroups (of 64 pixels x one channel block); with C = 8 (one block) a map of 257 x 256
# pixels is 1028 workgroup steps, so some workgroups walk on to a second step
CAP_CASE = _g(2, 4, 1, 1, 257, 256, "relu", "dense")


def _scale_bias(cout, *key):
    """conv_reference.scale_bias has 1024 different scales: wider layers take them in runs of 1024"""
    parts = [R.scale_bias(min(1024, cout - i), i, *key) for i in range(0, cout, 1024)]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def case_data(case):
    """-> dict x [n, C, h, w] int64 (values -1 .. 2), w [C, Cg, 3, 3] ternary, scale, bias, acc, v (float64, before the one
    rounding); the regime is asserted"""
    c = case
    C_ = c.groups * c.cg
    key = (c.groups, c.cg, c.n, c.stride, c.h, c.w)
    x = R.image((c.n, C_, c.h, c.w), 91, *key) - 1
    w = R.ternary((C_, c.cg, 3, 3), 92, *key)
    scale, bias = _scale_bias(C_, 93, *key)
    acc = grouped_conv(x, w, c.groups, c.stride)
    v = R.check_regime(acc, scale, bias, None, c.act)
    return {"x": x, "w": w, "scale": scale, "bias": bias, "acc": acc, "v": v}


# ------------------------------------------------------------------------------------------------ the trunk, in torch
def _bn(sd, p, x):
    return F.batch_norm(x, sd[p + ".running_mean"], sd[p + ".running_var"], sd[p + ".weight"], sd[p + ".bias"], False, 0.0, BN_EPS)


def f16_store(t):
    """fp16-storage emulation: what the HIP path's f16 mode stores is rounded to fp16; everything else stays fp32"""
    return t.half().float()


def bottleneck(sd, p, x, stride, store=None):
    """resnext.py:12-85 on resnet.py:263-303, style 'pytorch': conv2 is the grouped, strided 3x3; the group count is
    conv2's input width over its weight's second extent.  store (f16_store): applied where the HIP path stores a tensor --
    every conv weight, conv1 / conv2 after BN + ReLU, the downsample branch, the block's output."""
    q = store or (lambda t: t)
    out = q(torch.relu(_bn(sd, p + ".bn1", F.conv2d(x, q(sd[p + ".conv1.weight"])))))
    w2 = q(sd[p + ".conv2.weight"])
    out = q(torch.relu(_bn(sd, p + ".bn2", F.conv2d(out, w2, None, stride, 1, 1, out.shape[1] // w2.shape[1]))))
    out = _bn(sd, p + ".bn3", F.conv2d(out, q(sd[p + ".conv3.weight"])))
    identity = x
    if p + ".downsample.0.weight" in sd:
        identity = q(_bn(sd, p + ".downsample.1", F.conv2d(x, q(sd[p + ".downsample.0.weight"]), None, stride)))
    return q(torch.relu(out + identity))


def resnext(sd, p, x, depth=50, out_indices=(0, 1, 2, 3), store=None):
    q = store or (lambda t: t)
    pre = p + "." if p else ""
    x = torch.relu(_bn(sd, pre + "bn1", F.conv2d(q(x), q(sd[pre + "conv1.weight"]), None, 2, 3)))
    x = q(F.max_pool2d(x, 3, 2, 1))
    outs = []
    for i, nblocks in enumerate(STAGE_BLOCKS[depth]):
        for j in range(nblocks):
            x = bottleneck(sd, "%slayer%d.%d" % (pre, i + 1, j), x, 2 if (j == 0 and i > 0) else 1, store)
        if i in out_indices:
            outs.append(x)
    return outs


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
