"""CPU restatement of the reference's models/new/yolox10.py forward, composed from functions of oracle.glsdet_oracle (imported
only), and the fixture it is held against (tests/golden/cross10_golden.npz, tools/make_cross10_golden.py: the reference's
own module, run behind one aliased import).

    csp_darknet -> feat_i + Patch_Conv_NonLocal_new(feat_i) on dark3 / dark4 / dark5 (new/yolox10.py:257-266)
                -> the PAFPN lines of oracle.pafpn (new/yolox10.py:268-328) -> cross_scale_head

The sum rides in the channel_conv's `res` (act(bn(conv)) + feat: a float addition commutes, so this is the reference's
feat + block(feat) bit for bit), which is also where the HIP path adds it: under oracle.fp16_storage() the one rounding
falls after the add, as in the kernel's epilogue."""
import os

import numpy as np
import torch

from glsdet_amd.synth import synth_input, synth_state_dict
from oracle import glsdet_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cross10_golden.npz")
SEED = 3
NUM_CLASSES = 10
GAIN = {"tiny": 4.0, "nano": 16.0, "s": 4.0, "m": 4.0}          # tools/make_cross10_golden.py
CASES = [("tiny", (2, 3, 128, 160)), ("tiny", (1, 3, 160, 224)), ("nano", (1, 3, 96, 160)), ("s", (1, 3, 64, 96))]
TABLE_PHIS = ("tiny", "nano", "s", "m")
F32_BAR = 1e-4                                                   # the floor of the GPU test's f32 bar (tests/test_cross10.py)
QUADRANTS = ("lt", "lb", "rt", "rb")


def case_name(phi, shape):
    return "%s_%s" % (phi, "x".join(str(v) for v in shape))


_G = {}


def golden():
    if "g" not in _G:
        _G["g"] = np.load(GOLDEN)
    return _G["g"]


def table(phi):
    """the recorded {key: shape} of the reference module, in its order"""
    g = golden()
    names, shapes = g["table/%s/names" % phi], g["table/%s/shapes" % phi]
    return {str(k): tuple(int(v) for v in s if v >= 0) for k, s in zip(names, shapes)}


def weights(phi):
    """the fixture's weight recipe: bn.weight x 0.5 outside Patch_conv_*, every *_nonlocal.*.weight x GAIN[phi]"""
    sd = synth_state_dict(table(phi), SEED)
    for k in sd:
        if k.endswith("bn.weight") and "Patch_conv_" not in k:
            sd[k] = sd[k] * 0.5
        if "_nonlocal." in k and k.endswith(".weight"):
            sd[k] = sd[k] * GAIN[phi]
    return sd


def case_input(phi, shape):
    return synth_input(shape, int(golden()["case/%s/seed" % case_name(phi, shape)]))


def recorded(phi, shape, which="out32"):
    g = golden()
    return [torch.from_numpy(g["case/%s/%s/%d" % (case_name(phi, shape), which, k)]) for k in range(3)]


def residual_patch_nonlocal(sd, p, x):
    """x + Patch_Conv_NonLocal_new(x) (new/yolox10.py:262-266 on Non_local_family.py:208-252)"""
    lt, lb, rt, rb = O._quadrants(x)
    q = {nm: O.non_local_block(sd, "%s.feat_patchconv_%s_nonlocal" % (p, nm), t) for nm, t in zip(QUADRANTS, (lt, lb, rt, rb))}
    both = torch.cat((torch.cat((q["lt"], q["rt"]), 3), torch.cat((q["lb"], q["rb"]), 3)), 2)
    if p + ".channel_conv.weight" in sd:
        return O.plain_conv(sd, p + ".channel_conv", both, post=lambda t: t + x)
    return O.base_conv(sd, p + ".channel_conv", both, res=x)


def cross10_forward(sd, x):
    """models.new.yolox10.YoloBody.forward -> the three raw outputs [n, 5 + nc, H_l, W_l]"""
    p = "backbone"
    f = O.csp_darknet(sd, p + ".backbone", x)
    feat1, feat2, feat3 = (residual_patch_nonlocal(sd, "%s.Patch_conv_feat%d" % (p, i + 1), f[nm])
                           for i, nm in enumerate(("dark3", "dark4", "dark5")))
    P5 = O.base_conv(sd, p + ".lateral_conv0", feat3)
    t = O.csp_layer(sd, p + ".C3_p4", torch.cat((O._up2(P5), feat2), 1), False)
    P4 = O.base_conv(sd, p + ".reduce_conv1", t)
    P3_out = O.csp_layer(sd, p + ".C3_p3", torch.cat((O._up2(P4), feat1), 1), False)
    d = O.any_conv(sd, p + ".bu_conv2", P3_out, 2)
    P4_out = O.csp_layer(sd, p + ".C3_n3", torch.cat((d, P4), 1), False)
    d = O.any_conv(sd, p + ".bu_conv1", P4_out, 2)
    P5_out = O.csp_layer(sd, p + ".C3_n4", torch.cat((d, P5), 1), False)
    return O.cross_scale_head(sd, "head", (f["dark2"], P3_out, P4_out, P5_out))


def rel(a, b):
    """max over the levels of |a - b| / max(1, |b|)"""
    return max(float(((u.double() - v.double()).abs() / v.double().abs().clamp(min=1)).max()) for u, v in zip(a, b))
