#!/usr/bin/env python3
"""Fixture generator of the Swin trunk -- runs only where a checkout of the reference is at hand.  It executes the
reference's OWN mmdet/models/backbones/swin.py (WindowMSA, ShiftWindowMSA, SwinBlock, SwinBlockSequence, SwinTransformer)
and mmdet/models/utils/transformer.py (AdaptivePadding, PatchEmbed, PatchMerging), loaded by file path under their package
names, on seeded weights and inputs (fill / synth_input / make_block of tests/golden/make_golden.py) and writes
tests/golden/swin_golden.npz:

  block/<tag>/y, block/<tag>/meta     outputs and {shapes, in_shape, seed} of
      trunk_tiny                       SwinTransformer(embed_dims 32, depths (2,2,2,2), heads (1,2,4,8), window 7) on 1x3x100x116:
                                       the four norm{i} outputs, each flattened (NCHW), concatenated
      msa_<H>x<W>_s<shift>_h<heads>    ShiftWindowMSA(32 * heads, heads, 7, shift) on a [1, H * W, C] sequence
      msa_15x13_s3_h1_gain32           the same on 32 x the input: logits hundreds apart, where a mask of -100 lets tokens through
      merge_5x7                        PatchMerging(32, 64) on [1, 35, 32]
      swinblock                        SwinBlock(64, 2, 256, 7, shift=True) on [1, 9 * 10, 64]
  tables/swin_t, tables/swin_s         JSON: the state-dict names / shapes, in order

The mmcv names these two files import are stood in below; each stand-in is the documented behaviour of the mmcv 1.x function
for the arguments passed here:
  build_norm_layer(dict(type='LN'), c)   -> ('ln', nn.LayerNorm(c))
  build_conv_layer(dict(type='Conv2d'))  -> nn.Conv2d
  build_dropout                          -> nn.Identity (inference: DropPath and Dropout are the identity)
  FFN                                    -> mmcv 1.x's module tree: layers = Sequential(Sequential(Linear, act, Dropout), Linear,
                                            Dropout), i.e. the state-dict names layers.0.0.* and layers.1.*; forward(x, identity)
                                            returns identity + layers(x).  THE ffn.* KEY NAMES OF THE FIXTURE REST ON THIS STAND-IN.
  to_2tuple                              -> (v, v) for a scalar, any iterable (a tuple, the string 'corner') unchanged
  BaseModule, ModuleList                 -> nn.Module with init_cfg, nn.ModuleList
Weights are a function of (name, shape, seed) (glsdet_amd.synth.synth_tensor): LayerNorm gamma / beta and the bias tables are
filled non-trivially (the reference's init makes them 1, 0 and 0).  relative_position_index is a buffer of the reference; the
filler recomputes it, and this script checks the filler's value against the reference's own buffer for every window size it
uses.  Only data: no weights, no program text.

    PYTHONDONTWRITEBYTECODE=1 python tools/make_swin_golden.py <reference checkout>
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

TINY = dict(embed_dims=32, depths=(2, 2, 2, 2), num_heads=(1, 2, 4, 8), window_size=7)
MSA_SIZES = ((7, 7), (4, 4), (8, 9), (15, 13))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _mmcv_transformer_names(G):
    nn = torch.nn
    mmcv = G._mmcv_building_blocks()
    cnn, runner = mmcv.cnn, mmcv.runner
    BaseModule = runner.BaseModule

    def build_norm_layer(cfg, num_features, postfix=""):
        assert cfg["type"] == "LN"
        return "ln" + str(postfix), nn.LayerNorm(num_features, eps=cfg.get("eps", 1e-5))

    def build_conv_layer(cfg, *a, **k):
        assert cfg is None or cfg["type"] == "Conv2d"
        return nn.Conv2d(*a, **k)

    def build_activation_layer(cfg):
        assert cfg["type"] == "GELU"
        return nn.GELU()

    def build_dropout(cfg):
        return nn.Identity()

    class Sequential(nn.Sequential):
        pass

    class FFN(BaseModule):
        def __init__(self, embed_dims=256, feedforward_channels=1024, num_fcs=2, act_cfg=dict(type="ReLU", inplace=True),
                     ffn_drop=0.0, dropout_layer=None, add_identity=True, init_cfg=None, **kwargs):
            super().__init__(init_cfg)
            assert num_fcs >= 2
            layers, cin = [], embed_dims
            for _ in range(num_fcs - 1):
                layers.append(Sequential(nn.Linear(cin, feedforward_channels), build_activation_layer(act_cfg), nn.Dropout(ffn_drop)))
                cin = feedforward_channels
            layers.append(nn.Linear(feedforward_channels, embed_dims))
            layers.append(nn.Dropout(ffn_drop))
            self.layers = Sequential(*layers)
            self.dropout_layer = build_dropout(dropout_layer) if dropout_layer else nn.Identity()
            self.add_identity = add_identity

        def forward(self, x, identity=None):
            out = self.layers(x)
            if not self.add_identity:
                return self.dropout_layer(out)
            if identity is None:
                identity = x
            return identity + self.dropout_layer(out)

    class Registry:
        def register_module(self, *a, **k):
            return lambda c: c

    unused = type("Unused", (nn.Module,), {})
    cnn.build_norm_layer, cnn.build_conv_layer, cnn.build_activation_layer = build_norm_layer, build_conv_layer, build_activation_layer
    cnn.constant_init = cnn.trunc_normal_init = cnn.xavier_init = None
    bricks = G._stub("mmcv.cnn.bricks")
    G._stub("mmcv.cnn.bricks.registry", TRANSFORMER_LAYER=Registry(), TRANSFORMER_LAYER_SEQUENCE=Registry())
    G._stub("mmcv.cnn.bricks.transformer", FFN=FFN, build_dropout=build_dropout, BaseTransformerLayer=unused,
            TransformerLayerSequence=unused, build_transformer_layer_sequence=None, MultiScaleDeformableAttention=unused)
    G._stub("mmcv.cnn.utils")
    G._stub("mmcv.cnn.utils.weight_init", trunc_normal_=None)
    G._stub("mmcv.ops")
    G._stub("mmcv.ops.multi_scale_deform_attn", MultiScaleDeformableAttention=unused)
    G._stub("mmcv.runner.base_module", BaseModule=BaseModule)
    runner.ModuleList, runner._load_checkpoint = nn.ModuleList, None
    # mmcv's _ntuple returns every iterable unchanged -- a string ('corner') included
    G._stub("mmcv.utils", to_2tuple=lambda v: v if hasattr(v, "__iter__") else (v, v))
    cnn.bricks = bricks
    return Registry


def main(ref):
    G = _load("make_golden", os.path.join(ROOT, "tests", "golden", "make_golden.py"))
    from glsdet_amd.synth import synth_tensor
    torch.set_grad_enabled(False)
    Registry = _mmcv_transformer_names(G)
    root = os.path.join(ref, "yolox-ufp", "mmdet", "models")
    for pkg in ("mmdet", "mmdet.models", "mmdet.models.utils", "mmdet.models.backbones"):
        G._stub(pkg).__path__ = []
    G._stub("mmdet.utils", get_root_logger=None)
    G._stub("mmdet.models.builder").BACKBONES = Registry()
    G._stub("mmdet.models.utils.builder").TRANSFORMER = Registry()
    G._stub("mmdet.models.utils.ckpt_convert", swin_converter=None)
    tr = G._load_ref_module("mmdet.models.utils.transformer", os.path.join(root, "utils", "transformer.py"))
    sw = G._load_ref_module("mmdet.models.backbones.swin", os.path.join(root, "backbones", "swin.py"))
    nn = torch.nn

    for ws in range(2, 9):          # the filler's relative_position_index is the reference's own buffer
        own = sw.WindowMSA(32, 1, (ws, ws)).relative_position_index
        assert np.array_equal(own.numpy(), synth_tensor("relative_position_index", tuple(own.shape), 0)), ws

    class Trunk(nn.Module):
        def __init__(self, **kw):
            super().__init__()
            self.backbone = sw.SwinTransformer(**kw)

        def forward(self, x):
            return torch.cat([t.flatten(1) for t in self.backbone(x)], 1)

    class OnMap(nn.Module):
        """a module whose forward takes (sequence, hw_shape)"""

        def __init__(self, name, mod, hw, gain=1.0):
            super().__init__()
            self.add_module(name, mod)
            self.name, self.hw, self.gain = name, hw, gain

        def forward(self, x):
            y = getattr(self, self.name)(x * self.gain, self.hw)
            return y[0] if isinstance(y, tuple) else y

    out = {}
    block = G.make_block(out)
    block("trunk_tiny", lambda: Trunk(**TINY), (1, 3, 100, 116))
    seed = 1
    for (h, w) in MSA_SIZES:
        for shift in (0, 3):
            for heads in (1, 3):
                block("msa_%dx%d_s%d_h%d" % (h, w, shift, heads),
                      lambda: OnMap("attn", sw.ShiftWindowMSA(32 * heads, heads, 7, shift), (h, w)), (1, h * w, 32 * heads), seed=seed)
                seed += 1
    # input x 32: logits hundreds apart, the one fixture on which a mask of -100 and a mask of -inf differ
    block("msa_15x13_s3_h1_gain32", lambda: OnMap("attn", sw.ShiftWindowMSA(32, 1, 7, 3), (15, 13), gain=32.0), (1, 195, 32), seed=39)
    block("merge_5x7", lambda: OnMap("downsample", tr.PatchMerging(32, 64), (5, 7)), (1, 35, 32), seed=40)
    block("swinblock", lambda: OnMap("block", sw.SwinBlock(64, 2, 256, 7, shift=True), (9, 10)), (1, 90, 64), seed=41)
    for name, kw in (("swin_t", dict(depths=(2, 2, 6, 2))), ("swin_s", dict(depths=(2, 2, 18, 2)))):
        sd = sw.SwinTransformer(embed_dims=96, num_heads=(3, 6, 12, 24), **kw).state_dict()
        out["tables/" + name] = np.frombuffer(json.dumps([[k, list(v.shape)] for k, v in sd.items()]).encode(), np.uint8)
    path = os.path.join(ROOT, "tests", "golden", "swin_golden.npz")
    np.savez_compressed(path, **out)
    print("swin_golden.npz", len(out), "arrays,", os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1 << 20


if __name__ == "__main__":
    main(sys.argv[1])
