#!/usr/bin/env python3
"""Fixture generator of the ResNeXt backbone -- runs only where a checkout of the reference is at hand.  It executes the
reference's OWN mmdet/models/backbones/resnext.py (ResNeXt, its Bottleneck) on resnet.py / utils/res_layer.py, loaded by
file path under their package names with the mmcv building blocks stood in (tests/golden/make_golden.py::
_mmcv_building_blocks: the recipe of its resdet_cases), on seeded weights and inputs (fill / synth_input / calibrate_bn of
that file), and writes tests/golden/resnext_golden.npz and resnext64_golden.npz (the 64x4d trunk: one file would pass the
1 MiB of a committed file):

  block/<tag>/y, block/<tag>/bn/<key>, block/<tag>/meta     outputs, calibrated BN statistics, {shapes, in_shape, seed}
  tables/<variant>                                          JSON: the state-dict names / shapes, in order, of
                                                            ResNeXt(101, 32, 4) and ResNeXt(101, 64, 4)

Only data: no weights (they are a function of name, shape and seed), no program text.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_resnext_golden.py <reference checkout>
"""
import importlib.util
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.dont_write_bytecode = True


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def main(ref):
    G = _load("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    torch.set_grad_enabled(False)
    G._mmcv_building_blocks()
    root = os.path.join(ref, "yolox-ufp", "mmdet", "models")
    for pkg in ("mmdet", "mmdet.models", "mmdet.models.utils", "mmdet.models.backbones"):
        G._stub(pkg).__path__ = []
    reg = type("Registry", (), {"register_module": lambda self, *a, **k: (lambda c: c)})()
    G._stub("mmdet.models.builder").BACKBONES = reg
    rl = G._load_ref_module("mmdet.models.utils.res_layer", os.path.join(root, "utils", "res_layer.py"))
    sys.modules["mmdet.models.utils"].ResLayer = rl.ResLayer
    G._load_ref_module("mmdet.models.backbones.resnet", os.path.join(root, "backbones", "resnet.py"))
    rx = G._load_ref_module("mmdet.models.backbones.resnext", os.path.join(root, "backbones", "resnext.py"))

    def net(depth, groups, base_width):
        return rx.ResNeXt(depth=depth, groups=groups, base_width=base_width, num_stages=4, out_indices=(0, 1, 2, 3), frozen_stages=1,
                          norm_cfg=dict(type="BN", requires_grad=True), norm_eval=True, style="pytorch")

    class Trunk(torch.nn.Module):
        def __init__(self, groups, base_width):
            super().__init__()
            self.backbone = net(50, groups, base_width)

        def forward(self, x):
            return torch.cat([t.flatten(1) for t in self.backbone(x)], 1)

    def down(cin, cout, stride):
        return torch.nn.Sequential(torch.nn.Conv2d(cin, cout, 1, stride, bias=False), torch.nn.BatchNorm2d(cout))

    out = {}
    block = G.make_block(out)
    block("resnext50_32x4d_c2_c5", lambda: Trunk(32, 4), (1, 3, 64, 96), calibrate=True)
    # width = floor(planes * base_width / 64) * groups: 32 groups x Cg 4, stride 2 on odd extents, with downsample
    block("resnext_bottleneck_s2_down_g32_cg4", lambda: rx.Bottleneck(128, 64, groups=32, base_width=4, stride=2, style="pytorch",
                                                                       downsample=down(128, 256, 2)), (1, 128, 11, 13), seed=2, calibrate=True)
    for cg, seed in ((8, 3), (16, 4), (32, 5)):        # 8 groups x Cg: planes 32, base_width = 2 Cg
        block("resnext_bottleneck_s1_g8_cg%d" % cg, lambda: rx.Bottleneck(128, 32, groups=8, base_width=2 * cg, stride=1, style="pytorch"),
              (1, 128, 10, 12), seed=seed, calibrate=True)
    for groups in (32, 64):
        sd = net(101, groups, 4).state_dict()
        out["tables/resnext101_%dx4d" % groups] = np.frombuffer(json.dumps([[k, list(v.shape)] for k, v in sd.items()]).encode(), np.uint8)
    out64 = {}                                         # a file of its own: together they would pass the 1 MiB of a committed file
    G.make_block(out64)("resnext50_64x4d_c2_c5", lambda: Trunk(64, 4), (1, 3, 40, 56), seed=1, calibrate=True)
    for name, arrays in (("resnext_golden.npz", out), ("resnext64_golden.npz", out64)):
        path = os.path.join(ROOT, "tests", "golden", name)
        np.savez_compressed(path, **arrays)
        print(name, len(arrays), "arrays,", os.path.getsize(path), "bytes")
        assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
