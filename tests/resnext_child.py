"""The HIP lowerings tests/test_resnext.py compares, as functions -- and as a program: `python -m tests.resnext_child OUT.npz`
runs them in a process of its own (the test starts it with GLSDET_NO_GROUPED_CONV=1: conv2 of every Bottleneck then goes
through the block-diagonal dense conv) and writes what they computed to OUT.npz.  No reference tree, fixtures only."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUNKS = {"resnext50_32x4d_c2_c5": "resnext_golden.npz", "resnext50_64x4d_c2_c5": "resnext64_golden.npz"}
BLOCKS = {"resnext_bottleneck_s2_down_g32_cg4": 2, "resnext_bottleneck_s1_g8_cg8": 1, "resnext_bottleneck_s1_g8_cg16": 1,
          "resnext_bottleneck_s1_g8_cg32": 1}
EXACT = dict(groups=32, cg=4, n=1, stride=2, h=9, w=9)          # the exact-regime conv2 + bn2 + relu of exact_block()


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name))


def hip_case(eng, gold, tag):
    """the fixture case `tag` on the HIP path -> the output in the fixture's layout (NCHW fp32, trunks: C2..C5 flattened)"""
    from glsdet_amd.resdet import ResDetBuilder
    from tests.helpers import block_case
    from tests.test_hip_ops import _to_view
    sd, x, _ = block_case(gold, tag)
    b = ResDetBuilder(eng, sd)
    if tag in TRUNKS:
        f = b.resnet("m.backbone", x.cuda().float().contiguous())
        torch.cuda.synchronize()
        return torch.cat([t.to_nchw(t.c).cpu().flatten(1) for t in f], 1)
    y = b.bottleneck("m", _to_view(eng, x), BLOCKS[tag])
    torch.cuda.synchronize()
    return y.to_nchw().cpu()


def exact_block_data():
    """conv2 + bn2 + relu of a Bottleneck in the exact regime of tests/conv_reference.py.  The BN folds without a rounding:
    running_var = 2^40 (+ eps is 2^40 again in float64: sqrt = 2^20), running_mean = 0, weight = scale 2^20, bias = bias."""
    from tests import conv_reference as R
    from tests import resnext_reference as X
    e = EXACT
    C_ = e["groups"] * e["cg"]
    x = R.image((e["n"], C_, e["h"], e["w"]), 95) - 1
    w = R.ternary((C_, e["cg"], 3, 3), 96)
    scale, bias = R.scale_bias(C_, 97)
    v = R.check_regime(X.grouped_conv(x, w, e["groups"], e["stride"]), scale, bias, None, "relu")
    f = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    sd = {"m.conv2.weight": f(w), "m.bn2.weight": f(scale * 2.0 ** 20), "m.bn2.bias": f(bias),
          "m.bn2.running_mean": torch.zeros(C_), "m.bn2.running_var": torch.full((C_,), 2.0 ** 40)}
    return sd, x, v


def exact_block(eng):
    """-> (stored result NCHW fp32, names of the ops a plan records for it)"""
    from glsdet_amd.resdet import ResDetBuilder
    from tests.test_hip_ops import _to_view
    sd, x, _ = exact_block_data()
    b = ResDetBuilder(eng, sd)
    xv = _to_view(eng, torch.from_numpy(x.astype(np.float32)))
    y = b._conv2("m", xv, EXACT["stride"])
    torch.cuda.synchronize()
    plan = eng.new_plan()
    with plan:
        b._conv2("m", xv, EXACT["stride"])
    return y.to_nchw().cpu(), [o["name"] for o in plan.ops()]


def main(out_path):
    from glsdet_amd.engine import Engine
    out = {}
    for mode in ("f32", "f16"):
        eng = Engine(mode)
        for tag, f in list(TRUNKS.items()) + [(t, "resnext_golden.npz") for t in BLOCKS]:
            out["%s/%s" % (mode, tag)] = hip_case(eng, golden(f), tag).numpy()
        y, names = exact_block(eng)
        out["%s/exact" % mode] = y.numpy()
        out["%s/exact_ops" % mode] = np.frombuffer("\n".join(names).encode(), np.uint8)
    np.savez(out_path, **out)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    main(sys.argv[1])
