"""Records tests/golden/cfp_golden.npz: what the reference's own models/cfp/yolox_cfp.py and models/cfp/evc_blocks.py compute
(CPU, fp32 and .double()) on small inputs, and the state_dict tables of the four phis.

    python tools/make_cfp_golden.py <reference checkout>/yolox-drone

models/cfp/Functions.py imports DropPath, trunc_normal_, register_model, to_2tuple and two constants from `timm`, which need
not be installed: at drop_path = 0 DropPath is never instantiated and the rest is initialisation.  A stand-in written here
(timm_stand_in) is registered in sys.modules, the way tools/make_cross10_golden.py aliases `models.decouple`; the reference's
files are imported unchanged.

Weights are glsdet_amd.synth.synth_state_dict(table, SEED) with tests/cfp_reference.recipe, so only names, shapes and outputs
are stored.  The recipe matters.  With the reference's init, layer_scale_* = 1e-5 hides the whole MLP branch, and a
running_var near 1 hides every eps.  The recipe has layer scales of order 1, Encoding.scale in (-1, 0), codewords of order
0.3 and running variances down to 1e-3 in neck and head (1e-5 in ConvBlock), with each gamma scaled so that the layer's gain
stays put.  This generator ASSERTS that every planted mistake of tests/cfp_reference.MISTAKES moves the record named for it
by at least SENSITIVITY (tools/make_cross10_golden.py's) relative to max(1, |value|) -- the erf / tanh GELU, a 1e-3 effect by
nature, by tests/cfp_reference.MISTAKE_BAR; tests/test_cfp_reference.py asserts it again on the committed file."""
import contextlib
import importlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glsdet_amd.synth import synth_state_dict      # noqa: E402
from tests import cfp_reference as X                # noqa: E402


def timm_stand_in():
    """the names models/cfp/Functions.py:18-21 imports, as modules in sys.modules"""
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    mod("timm")
    mod("timm.models")
    mod("timm.models.layers", DropPath=torch.nn.Identity, trunc_normal_=torch.nn.init.trunc_normal_)
    mod("timm.models.layers.helpers", to_2tuple=lambda v: v if isinstance(v, (tuple, list)) else (v, v))
    mod("timm.models.registry", register_model=lambda fn: fn)
    mod("timm.data", IMAGENET_DEFAULT_MEAN=(0.485, 0.456, 0.406), IMAGENET_DEFAULT_STD=(0.229, 0.224, 0.225))


def load_reference(checkout):
    sys.path.insert(0, checkout)
    timm_stand_in()
    return importlib.import_module("models.cfp.yolox_cfp"), importlib.import_module("models.cfp.evc_blocks")


def run(fn, x):
    with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
        y = fn(x)
    return [o.clone() for o in y] if isinstance(y, (list, tuple)) else y.clone()


def main(checkout):
    ref, blocks = load_reference(checkout)
    out = {}
    for phi in X.TABLE_PHIS:
        sd = ref.YoloBody(X.NUM_CLASSES, phi).state_dict()
        out["table/%s/names" % phi] = np.array(list(sd.keys()))
        shapes = np.full((len(sd), 4), -1, np.int64)
        for i, v in enumerate(sd.values()):
            shapes[i, :v.dim()] = list(v.shape)
        out["table/%s/shapes" % phi] = shapes
        print(phi, len(sd), "keys,", sum(v.numel() for k, v in sd.items() if "num_batches" not in k and "running" not in k), "parameters")
    for i, (phi, shape) in enumerate(X.CASES):
        m = ref.YoloBody(X.NUM_CLASSES, phi).eval()
        sd = X.recipe(synth_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, X.SEED))
        m.load_state_dict(sd, strict=True)
        seed = 200 + i
        x = X.synth_input(shape, seed)
        y32 = run(m, x)
        y64 = run(m.double(), x.double())
        name = X.case_name(phi, shape)
        print("%-22s max |logit| %.3f  fp32 vs fp64 %.2e" % (name, max(float(o.abs().max()) for o in y32), X.rel(y32, y64)))
        out["case/%s/seed" % name] = np.int64(seed)
        for k, (a, b) in enumerate(zip(y32, y64)):
            out["case/%s/out32/%d" % (name, k)] = a.numpy()
            out["case/%s/out64/%d" % (name, k)] = b.numpy()
    for name, C, h, w, n in X.ENCODING_RECORDS:
        m = blocks.EVCBlock(C, C).eval()
        m.load_state_dict({k[4:]: v for k, v in X.block_weights(C).items()}, strict=True)
        x = X.block_input(C, h, w, n, key=1)
        out["block/encoding/%s/out32" % name] = run(m.lvc.LVC[3], x).numpy()
        out["block/encoding/%s/out64" % name] = run(m.double().lvc.LVC[3], x.double()).numpy()
    for name, C, h, w, n in X.BLOCK_RECORDS:
        m = blocks.EVCBlock(C, C).eval()
        m.load_state_dict({k[4:]: v for k, v in X.block_weights(C).items()}, strict=True)
        x = X.block_input(C, h, w, n)
        for kind, fn in (("lvc", lambda: m.lvc), ("l_MLP", lambda: m.l_MLP), ("evc", lambda: m)):
            m.float()
            out["block/%s/%s/out32" % (kind, name)] = run(fn(), x).numpy()
            m.double()
            out["block/%s/%s/out64" % (kind, name)] = run(fn(), x.double()).numpy()
            print("block %-6s %-9s max |out| %.3f" % (kind, name, float(np.abs(out["block/%s/%s/out32" % (kind, name)]).max())))
    path = X.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")
    X._G.clear()
    for phi, shape in X.CASES:
        with torch.no_grad():
            print("restatement %-22s vs recorded fp32 %.2e" % (X.case_name(phi, shape),
                                                             X.rel(X.cfp_forward(X.weights(phi), X.case_input(phi, shape)), X.recorded(phi, shape))))
    blind = []
    for name in X.MISTAKES:
        d = X.mistake_distance(name)
        print("planted %-22s moves its record by %.2e" % (name, d))
        if d < X.MISTAKE_BAR.get(name, X.SENSITIVITY):
            blind.append(name)
    assert not blind, "the fixture would not see the mistakes %s: change the recipe" % blind


if __name__ == "__main__":
    main(sys.argv[1])
