"""Records tests/golden/cross10_golden.npz: what the reference's own models/new/yolox10.py computes (CPU, fp32 and
.double()) on small inputs, and its state_dict tables.

    python tools/make_cross10_golden.py <reference checkout>/yolox-drone

The reference file imports `models.decouple.darknet`, which its checkout does not have; the reference's own
models/new/darknet.py (the same classes, exposes dark2) is registered under that name in sys.modules -- the one aliased
import behind which the reference runs unchanged.  The head's stray prints are swallowed.

Weights are glsdet_amd.synth.synth_state_dict(table, SEED) with the recipe `weights()` below, so only names, shapes and
outputs are stored.  The recipe matters: with the usual bn.weight x 0.5 everywhere, removing the whole non-local term moves
the logits by about 2e-4 relative and a test of it would be blind.  Here bn.weight x 0.5 applies OUTSIDE Patch_conv_* only
and every *_nonlocal.*.weight is multiplied by GAIN[phi]; the generator asserts that zeroing the twelve conv_out moves the
logits by at least SENSITIVITY relative to max(1, |logit|) in every case (tests/test_cross10_reference.py asserts it again
on the restatement)."""
import contextlib
import importlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glsdet_amd.synth import synth_input, synth_state_dict      # noqa: E402

SEED = 3
NUM_CLASSES = 10
GAIN = {"tiny": 4.0, "nano": 16.0, "s": 4.0, "m": 4.0}          # nano: 4 gives 5.4e-4 only; raised until SENSITIVITY holds
SENSITIVITY = 1e-2                                             # 100 x the GPU test's f32 bar (1e-4)
CASES = [("tiny", (2, 3, 128, 160), 100), ("tiny", (1, 3, 160, 224), 101), ("nano", (1, 3, 96, 160), 102),
         ("s", (1, 3, 64, 96), 103)]
TABLE_PHIS = ("tiny", "nano", "s", "m")


def case_name(phi, shape):
    return "%s_%s" % (phi, "x".join(str(v) for v in shape))


def weights(table, phi):
    """the synthesized state_dict of the fixture for a {key: shape} table in the reference's order"""
    sd = synth_state_dict(table, SEED)
    for k in sd:
        if k.endswith("bn.weight") and "Patch_conv_" not in k:
            sd[k] = sd[k] * 0.5
        if "_nonlocal." in k and k.endswith(".weight"):
            sd[k] = sd[k] * GAIN[phi]
    return sd


def load_reference(checkout):
    sys.path.insert(0, checkout)
    sys.modules["models.decouple"] = importlib.import_module("models.new")
    sys.modules["models.decouple.darknet"] = importlib.import_module("models.new.darknet")
    return importlib.import_module("models.new.yolox10")


def run(model, x):
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        return [o.clone() for o in model(x)]


def rel(a, b):
    return max(float(((u.double() - v.double()).abs() / v.double().abs().clamp(min=1)).max()) for u, v in zip(a, b))


def main(checkout):
    ref = load_reference(checkout)
    out = {}
    for phi in TABLE_PHIS:
        m = ref.YoloBody(NUM_CLASSES, phi)
        sd = m.state_dict()
        out["table/%s/names" % phi] = np.array(list(sd.keys()))
        shapes = np.full((len(sd), 4), -1, np.int64)
        for i, v in enumerate(sd.values()):
            shapes[i, :v.dim()] = list(v.shape)
        out["table/%s/shapes" % phi] = shapes
        print(phi, len(sd), "keys")
    for phi, shape, seed in CASES:
        m = ref.YoloBody(NUM_CLASSES, phi).eval()
        table = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        sd = weights(table, phi)
        m.load_state_dict(sd, strict=True)
        x = synth_input(shape, seed)
        y32 = run(m, x)
        y64 = run(m.double(), x.double())
        m.float()
        zero = {k: (torch.zeros_like(v) if ".conv_out." in k else v) for k, v in sd.items()}
        m.load_state_dict(zero, strict=True)
        y0 = run(m, x)
        name = case_name(phi, shape)
        sens, noise = rel(y0, y32), rel(y32, y64)
        print("%-22s max |logit| %.3f  fp32 vs fp64 %.2e  conv_out zeroed %.2e" % (name, max(float(o.abs().max()) for o in y32), noise, sens))
        assert sens >= SENSITIVITY, "the non-local term moves the logits of %s by %.2e only: raise GAIN[%r]" % (name, sens, phi)
        out["case/%s/seed" % name] = np.int64(seed)
        for k, (a, b) in enumerate(zip(y32, y64)):
            out["case/%s/out32/%d" % (name, k)] = a.numpy()
            out["case/%s/out64/%d" % (name, k)] = b.numpy()
    path = os.path.join(ROOT, "tests", "golden", "cross10_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
