"""The Swin trunk on the GPU: ResDetBuilder.swin / swin_block and the three kernels of csrc/swin.hip around the 1x1 conv
kernels, against what tests/golden/swin_golden.npz records of the reference's own modules; HipGflDetector(backbone='swin'),
the surface class and the Swin-T config.

Tolerances.  Every result is compared with the float64 restatement of tests/swin_reference.py (which
tests/test_swin_reference.py holds to the recorded outputs within 2e-5), relative to its largest output:
  f32   4 x the distance of the reference's OWN fp32 output (the recorded one) from the float64 value, measured here per
        fixture (2e-7 .. 7e-7).  The kernels compute the same fp32 arithmetic in another order; the factor is the one
        difference in order that matters: a matrix-core product is ONE sequential fmaf chain over K, the reference's CPU
        GEMM keeps at least 16 partial sums (its vector width), and the random-walk error of a sum of K roundings cut into
        16 chains is sqrt(16) = 4 times smaller.
  f16   twice the distance of the f16-emulation restatement (fp16 rounding at every store point of the kernels, fp32
        residual stream) from float64, measured here on the same fixture: the margin of 2 is for accumulation order."""
import os

import numpy as np
import pytest
import torch

from tests import swin_reference as S
from tests.test_swin_reference import MSA_TAGS

pytestmark = pytest.mark.gpu


def _engine(mode):
    from glsdet_amd.engine import Engine
    return Engine(mode)


def _view(eng, x_nhwc, dtype=None):
    """NHWC float tensor -> a dense TView of `dtype` (default: the engine's)"""
    from glsdet_amd.engine import _TORCH_DT
    n, h, w, c = x_nhwc.shape
    v = eng.tensor(n, h, w, c, dtype)
    v.buf.view(_TORCH_DT[v.dtype])[: x_nhwc.numel()] = x_nhwc.flatten().to(_TORCH_DT[v.dtype]).to(eng.device)
    return v


def _nhwc(v):
    return v.to_nchw().permute(0, 2, 3, 1).double().cpu()


def _check(tag, got, exact, emu, mode):
    recorded = torch.from_numpy(S.golden()["block/%s/y" % tag]).double().reshape(exact.shape)
    scale = float(exact.abs().max())
    err = float((got - exact).abs().max()) / scale
    noise = float((recorded - exact).abs().max()) / scale
    e16 = float((emu - exact).abs().max()) / scale
    tol = 4 * noise if mode == "f32" else 2 * e16
    print("%s %s: error %.3e of max |y|, tolerance %.3e (reference fp32 %.3e, f16 emulation %.3e)" % (tag, mode, err, tol, noise, e16))
    assert noise < 2e-5
    assert err <= tol


@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("tag", MSA_TAGS)
def test_msa_modules_meet_the_recorded_ones(tag, mode):
    import re
    from glsdet_amd.resdet import ResDetBuilder
    h, w, s, nh = map(int, re.match(r"msa_(\d+)x(\d+)_s(\d+)_h(\d+)", tag).groups())
    wts = S.weights(tag)
    x = S.block_input(tag).double().reshape(1, h, w, 32 * nh)
    eng = _engine(mode)
    b = ResDetBuilder(eng, {k: v.float() for k, v in wts.items()})
    p = "attn.w_msa"
    qkv = b._linear(p + ".qkv", _view(eng, x))
    o = eng.window_attention(qkv, b._dev("t", wts[p + ".relative_position_bias_table"]), b._dev("b", wts[p + ".qkv.bias"]),
                             nh, 7, s, float(np.float32(32 ** -0.5)))
    y = b._linear(p + ".proj", o)
    torch.cuda.synchronize()
    rnd = S.f16_round if mode == "f16" else S.ident
    _check(tag, _nhwc(y), S.msa(x, wts, "attn.", nh, 7, s), S.msa(rnd(x), wts, "attn.", nh, 7, s, rnd=rnd), mode)


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_merge_and_block_meet_the_recorded_ones(mode):
    from glsdet_amd.engine import F32
    from glsdet_amd.resdet import ResDetBuilder
    rnd = S.f16_round if mode == "f16" else S.ident
    eng = _engine(mode)
    # PatchMerging on 5 x 7 (both odd): merge -> LayerNorm over 4C -> reduction
    wts = S.weights("merge_5x7")
    x = S.block_input("merge_5x7").double().reshape(1, 5, 7, 32)
    b = ResDetBuilder(eng, {k: v.float() for k, v in wts.items()})
    u = b._ln("downsample.norm", eng.patch_merge(_view(eng, x)), eng.dt)
    y = b._linear("downsample.reduction", u)
    torch.cuda.synchronize()
    _check("merge_5x7", _nhwc(y), S.merging(x, wts, "downsample."), S.merging(rnd(x), wts, "downsample.", rnd=rnd), mode)
    # SwinBlock(64, 2 heads, shift 3) on 9 x 10, on the fp32 residual stream
    wts = S.weights("swinblock")
    x = S.block_input("swinblock").double().reshape(1, 9, 10, 64)
    b = ResDetBuilder(eng, {k: v.float() for k, v in wts.items()})
    y = b.swin_block("block", _view(eng, x, F32), 2, 7, 3)
    torch.cuda.synchronize()
    assert y.dtype == F32
    _check("swinblock", _nhwc(y), S.swin_block(x, wts, "block.", 2, 7, 3), S.swin_block(x, wts, "block.", 2, 7, 3, rnd=rnd), mode)


@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_tiny_trunk_meets_the_recorded_one(mode):
    from glsdet_amd.resdet import ResDetBuilder
    rnd = S.f16_round if mode == "f16" else S.ident
    wts = S.weights("trunk_tiny")
    img = S.block_input("trunk_tiny")
    eng = _engine(mode)
    b = ResDetBuilder(eng, {k: v.float() for k, v in wts.items()})
    outs = b.swin("backbone", img.to(eng.device).contiguous(), **S.TINY)
    torch.cuda.synchronize()
    assert [(o.h, o.w, o.c) for o in outs] == [(25, 29, 32), (13, 15, 64), (7, 8, 128), (4, 4, 256)]
    got = torch.cat([o.to_nchw().double().cpu().flatten(1) for o in outs], 1)
    cat = lambda ts: torch.cat([t.flatten(1) for t in ts], 1)
    exact = cat(S.trunk(img.double(), wts, **S.TINY))
    emu = cat(S.trunk(img.double(), wts, rnd=rnd, **S.TINY)) if mode == "f16" else exact
    _check("trunk_tiny", got, exact, emu, mode)


# ------------------------------------------------------------------------------------------------ detector
_DET = dict(backbone="swin", out_indices=(1, 2, 3), start_level=0, **S.TINY)


def _det_sd(kind, seed=3, **swin):
    from glsdet_amd.arch import swindet_state_dict_shapes
    from glsdet_amd.synth import synth_state_dict
    return synth_state_dict(swindet_state_dict_shapes(kind, out_indices=(1, 2, 3), **(swin or S.TINY)), seed)


@pytest.mark.parametrize("mode", ["f32", "f16"])
@pytest.mark.parametrize("kind", ["gfl", "mpdet"])
def test_swin_detector_eager_graph_and_detect(kind, mode):
    from glsdet_amd.resdet import HipGflDetector
    from glsdet_amd.synth import synth_input
    from oracle import mpdet_oracle as M
    det = HipGflDetector(kind, _det_sd(kind), dtype=mode, **_DET)
    x1, x2 = synth_input((2, 3, 64, 96), 11).cuda(), synth_input((2, 3, 64, 96), 12).cuda()
    cls, reg = det.forward_raw(x1)
    assert [tuple(c.shape[2:]) for c in cls] == [(8, 12), (4, 6), (2, 3), (1, 2), (1, 1)]
    assert all(c.shape[1] == 10 for c in cls) and all(r.shape[1] == 68 for r in reg)
    assert all(bool(torch.isfinite(t).all()) for t in cls + reg)
    cls2, _ = det.forward_raw(x2)
    assert float((cls2[0] - cls[0]).abs().max()) > 1e-3                          # the output follows the input
    # detect() = forward_raw + the post-processing of the restatement (gfl_head.py get_bboxes)
    thr = 0.3 if kind == "gfl" else 0.05
    res = det.detect(x1, score_thr=thr, iou_thr=0.6, nms_pre=1000, max_per_img=100)
    want = M.gfl_get_bboxes([c.cpu() for c in cls], [r.cpu() for r in reg], [8, 16, 32, 64, 128], [(64, 96, 3)] * 2, thr, 1000,
                            0.6, 100)
    key = lambda d, l: np.lexsort((d[:, 1], d[:, 0], -d[:, 4], l))
    for (d, l), (wd, wl) in zip(res, want):
        d, l, wd, wl = np.asarray(d), np.asarray(l), np.asarray(wd), np.asarray(wl)
        assert len(l) == len(wl) > 0, (len(l), len(wl))
        i, j = key(d, l), key(wd, wl)
        np.testing.assert_array_equal(l[i], wl[j])
        np.testing.assert_allclose(d[i, :4], wd[j, :4], atol=1e-3, rtol=1e-5)
        np.testing.assert_allclose(d[i, 4], wd[j, 4], atol=1e-6)
    # a captured plan, replayed on new input, gives the bits of the eager plan on that input
    post = dict(score_thr=thr, iou_thr=0.6, nms_pre=1000, max_per_img=100)
    c1 = det.compile(2, 64, 96, post)
    det.run(c1, x2)
    eager = det.collect(c1)
    c2 = det.compile(2, 64, 96, post, use_graph=True)
    det.run(c2, x1)
    det.run(c2, x2)
    torch.cuda.synchronize()
    for (a, la), (b, lb) in zip(eager, det.collect(c2)):
        assert np.array_equal(a, b) and np.array_equal(la, lb)


def test_surface_built_from_the_swin_config_at_the_tiny_widths():
    from glsdet_amd.mmdet_surface import Config, build_detector
    from glsdet_amd.resdet import HipGflDetector
    from glsdet_amd.synth import synth_input
    c = Config.fromfile(os.path.join(S.ROOT, "configs", "UFPMP-Det", "coarse_det_swin_t.py"))
    m = dict(c.model)
    m.pop("train_cfg", None)
    m["backbone"] = dict(m["backbone"], embed_dims=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])
    m["neck"] = dict(m["neck"], in_channels=[64, 128, 256])
    m["test_cfg"] = dict(m["test_cfg"], score_thr=0.3)
    model = build_detector(m)
    sd = _det_sd("gfl")
    model.load_state_dict(sd)
    model.eval()
    x = synth_input((1, 3, 64, 96), 13)
    meta = dict(img_shape=(64, 96, 3), ori_shape=(64, 96, 3), pad_shape=(64, 96, 3), scale_factor=np.ones(4, np.float32), flip=False)
    res = model(return_loss=False, rescale=False, img=[x], img_metas=[[meta]])
    assert len(res) == 1 and len(res[0]) == 10 and all(r.shape[1] == 5 for r in res[0])
    # (the surface tunes its kernels per problem; a second detector of the process reuses those verdicts)
    direct = HipGflDetector("gfl", sd, dtype=model.hip_dtype, autotune=True, **_DET).detect(x.cuda(), score_thr=0.3, iou_thr=0.6, nms_pre=1000,
                                                                            max_per_img=100, img_shapes=[(64, 96, 3)])
    d, l = direct[0]
    assert sum(len(r) for r in res[0]) == len(l)
    for k in range(10):
        assert np.array_equal(res[0][k], np.asarray(d)[np.asarray(l) == k])


def test_swin_t_at_full_width_on_one_224_image():
    from glsdet_amd.resdet import HipGflDetector
    from glsdet_amd.synth import synth_input
    sd = _det_sd("gfl", seed=5, embed_dims=96)
    det = HipGflDetector("gfl", sd, dtype="f16", backbone="swin", out_indices=(1, 2, 3), start_level=0)
    cls, reg = det.forward_raw(synth_input((1, 3, 224, 224), 14).cuda())
    assert [tuple(c.shape) for c in cls] == [(1, 10, 28, 28), (1, 10, 14, 14), (1, 10, 7, 7), (1, 10, 4, 4), (1, 10, 2, 2)]
    assert [tuple(r.shape[1:2]) for r in reg] == [(68,)] * 5
    assert all(bool(torch.isfinite(t).all()) for t in cls + reg)
