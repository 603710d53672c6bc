"""Kind `cross10` on the GPU (the reference's models/new/yolox10.py): HipDetector against the outputs the reference's own
module gave (tests/golden/cross10_golden.npz), in the rules of tests/test_hip_model.py (f32) and tests/test_f16_emulation.py
(f16); the residual Patch_Conv_NonLocal_new block against the oracle; the captured plan; the drone twin's harness flow.
tests/test_cross10_reference.py shows on the CPU that the recorded logits move by at least 100 x the f32 bar when the
non-local term is removed, so these comparisons see the matrix-core kernels."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import glsdet_oracle as O
from tests import cross10_reference as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASE_IDS = [X.case_name(*c) for c in X.CASES]
LOGIT_TOL = 1e-4


@pytest.fixture
def drone_path(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "glsdet_amd", "drone"))
    for mod in list(sys.modules):
        if mod == "models" or mod.startswith("models."):
            monkeypatch.delitem(sys.modules, mod)


# -------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", X.CASES, ids=_CASE_IDS)
def test_cross10_f32_meets_north_star_tolerance(case):
    """bar max(1e-4, 2 x noise) relative to max(1, |logit|), noise = the recorded reference-vs-fp64 distance"""
    from glsdet_amd.detector import HipDetector
    phi, shape = case
    sd, x = X.weights(phi), X.case_input(phi, shape)
    want, truth = X.recorded(phi, shape), X.recorded(phi, shape, "out64")
    noise = X.rel(want, truth)
    det = HipDetector("cross10", sd, dtype="f32")
    got = [g.cpu() for g in det.forward_raw(x.cuda())]
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    err_ref, err_truth = X.rel(got, want), X.rel(got, truth)
    print("cross10 f32 %s: hip-vs-reference %.2e  hip-vs-fp64 %.2e  reference-vs-fp64 %.2e" % (X.case_name(phi, shape), err_ref, err_truth, noise))
    bar = max(LOGIT_TOL, 2.0 * noise)
    assert err_ref <= bar and err_truth <= bar


@pytest.mark.parametrize("case", X.CASES[:2], ids=_CASE_IDS[:2])
def test_cross10_f16_is_as_close_to_the_reference_as_fp16_storage_allows(case):
    from glsdet_amd.detector import HipDetector
    phi, shape = case
    sd, x = X.weights(phi), X.case_input(phi, shape)
    outs = X.recorded(phi, shape)
    got = [g.cpu() for g in HipDetector("cross10", sd, dtype="f16").forward_raw(x.cuda())]
    with torch.no_grad(), O.fp16_storage():
        emu = X.cross10_forward(sd, x)
    scale = max(float(w.abs().max()) for w in outs)
    cat = lambda a, b: torch.cat([(p - q).flatten() for p, q in zip(a, b)])
    r, e = cat(got, outs), cat(emu, outs)
    rms = lambda t: float(t.pow(2).mean().sqrt()) / scale
    print("cross10 f16 %s: HIP vs reference max %.4f rms %.5f | emulation vs reference max %.4f rms %.5f (x max|logit| = %.2f)" % (
        X.case_name(phi, shape), float(r.abs().max()) / scale, rms(r), float(e.abs().max()) / scale, rms(e), scale))
    assert rms(r) <= 1.5 * rms(e) + 1e-4
    assert float(r.abs().max()) / scale <= 2.0 * float(e.abs().max()) / scale + 1e-3


# -------------------------------------------------------------------------------------------------------- block level
def _block_sd(C, seed, gain=4.0):
    from glsdet_amd.arch import _Table, gl_fusion_table
    t = _Table()
    gl_fusion_table(t, "blk", C, "non_linear")
    sd = O.synth_state_dict(t, seed)
    for k in sd:
        if "_nonlocal." in k and k.endswith(".weight"):
            sd[k] = sd[k] * gain
    return sd


def _block_hip(sd, x, dtype, mfma, res):
    from glsdet_amd.engine import Engine
    from glsdet_amd.nets import NetBuilder
    eng = Engine(dtype)
    b = NetBuilder(eng, sd)
    n, C, H, W = x.shape
    xv = eng.tensor(n, H, W, C)
    tt = torch.float16 if dtype == "f16" else torch.float32
    xv.buf.view(tt)[: n * H * W * C] = x.permute(0, 2, 3, 1).contiguous().to(tt).reshape(-1).cuda()
    y = b.patch_conv_nonlocal_new("blk", xv, res=xv if res else None, mfma=mfma)
    torch.cuda.synchronize()
    return y.to_nchw(C).cpu(), xv.to_nchw(C).cpu()


_BLOCKS = [(96, 16, 20, 2), (384, 5, 7, 1)]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("C,H,W,n", _BLOCKS, ids=["c96-16x20", "c384-5x7"])
def test_residual_block_on_the_matrix_cores_matches_the_oracle(dtype, C, H, W, n):
    """patch_conv_nonlocal_new(res=x, mfma=True) against oracle.patch_conv_nonlocal_new + x; x stays intact"""
    sd = _block_sd(C, 11)
    x = O.synth_input((n, C, H, W), 12)
    if dtype == "f16":
        x = x.half().float()
    with torch.no_grad():
        want = O.patch_conv_nonlocal_new(sd, "blk", x) + x
        plain = O.base_conv(sd, "blk.channel_conv", x) + x              # the same without the four non-local blocks
    got, x_after = _block_hip(sd, x, dtype, True, True)
    assert torch.equal(x_after, x), "the block's input was written"
    scale = max(1.0, float(want.abs().max()))
    err = float((got - want).abs().max())
    print("residual block C=%d %dx%d %s: max |err| %.2e, |want|max %.2f, the non-local blocks contribute %.2e" % (
        C, H, W, dtype, err, float(want.abs().max()), float((want - plain).abs().max())))
    assert float((want - plain).abs().max()) > 100 * 5e-5 * scale     # the comparison sees the blocks
    assert err <= (5e-5 * scale if dtype == "f32" else 4e-3 * scale)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_default_arguments_keep_the_scalar_kernels(dtype):
    """patch_conv_nonlocal_new() as every existing caller invokes it (in place, no res, mfma=False) equals the parent's
    lowering spelled out: theta|phi|g by conv_group, Engine.nonlocal_multi with its old signature on the windows of x,
    channel_conv -- bit for bit.  And mfma=False with res takes the same scalar kernels into a fresh buffer."""
    from glsdet_amd.engine import Engine
    from glsdet_amd.nets import NetBuilder
    C, H, W, n = 96, 9, 11, 2
    sd = _block_sd(C, 21)
    x = O.synth_input((n, C, H, W), 22)
    tt = torch.float16 if dtype == "f16" else torch.float32
    got, _ = _block_hip(sd, x, dtype, False, False)
    eng = Engine(dtype)
    b = NetBuilder(eng, sd)
    xv = eng.tensor(n, H, W, C)
    xv.buf.view(tt)[: n * H * W * C] = x.permute(0, 2, 3, 1).contiguous().to(tt).reshape(-1).cuda()
    wins = [xv.window(0, H // 2, 0, W // 2), xv.window(H // 2, H, 0, W // 2), xv.window(0, H // 2, W // 2, W), xv.window(H // 2, H, W // 2, W)]
    names = ["blk.feat_patchconv_%s_nonlocal" % q for q in ("lt", "lb", "rt", "rb")]
    packs = [b._pack(p + ".tpg", [b._plain_part(p + ".theta"), b._plain_part(p + ".phi"), b._plain_part(p + ".g")], C) for p in names]
    tpgs = eng.conv_group(wins, packs, 1, 0, "none")
    wouts = [eng.upload(sd[p + ".conv_out.weight"].float().reshape(-1, C)) for p in names]
    bouts = [eng.upload(sd[p + ".conv_out.bias"].float()) for p in names]
    eng.nonlocal_multi(wins, tpgs, C, wouts, bouts)
    want = b.cba("blk.channel_conv", xv)
    torch.cuda.synchronize()
    assert torch.equal(got, want.to_nchw(C).cpu())
    with_res, x_after = _block_hip(sd, x, dtype, False, True)
    xq = x.to(tt).float()
    assert torch.equal(x_after, xq)
    scale = max(1.0, float(got.abs().max()))
    assert float((with_res - (got + xq)).abs().max()) <= (5e-5 if dtype == "f32" else 4e-3) * scale     # act(conv) + res


# ------------------------------------------------------------------------------------------------------ captured plan
def test_cross10_plan_graph_replay_equals_eager():
    from glsdet_amd.detector import HipDetector
    phi, shape = X.CASES[1]
    sd = X.weights(phi)
    det = HipDetector("cross10", sd, dtype="f16")
    xs = [X.case_input(phi, shape).cuda(), O.synth_input(shape, 7).cuda()]
    eager = [[t.clone() for t in det.forward_raw(x)] for x in xs]
    c = det.compile(shape[0], shape[2], shape[3], None, use_graph=True)
    for x, want in zip(xs + xs[:1], eager + eager[:1]):
        det.run(c, x)
        torch.cuda.synchronize()
        for p, l in zip(want, c.levels):
            assert torch.equal(p, l.to_nchw(5 + X.NUM_CLASSES))
    names = [o["name"] for o in c.plan.ops()]
    assert sum("nonlocal_mfma" in nm for nm in names) == 3, [nm for nm in names if "nonlocal" in nm]


def test_cross10_takes_the_matrix_core_kernels_where_they_were_measured_faster(monkeypatch):
    """Engine.NONLOCAL_MFMA_FROM: the s case's dark5 is 2 x 3, its quadrants have at most 2 pixels, below
    the smallest measured quadrant: that level keeps the scalar kernels, dark3 / dark4 (24 and 6 pixels) do not;
    GLSDET_NONLOCAL_MFMA=0 / 1 force either family for measurements"""
    from glsdet_amd.detector import HipDetector
    phi, shape = X.CASES[3]
    sd = X.weights(phi)

    def nonlocal_ops():
        c = HipDetector("cross10", sd, dtype="f16").compile(shape[0], shape[2], shape[3], None)
        return [o["name"] for o in c.plan.ops() if o["name"].startswith("nonlocal")]
    monkeypatch.delenv("GLSDET_NONLOCAL_MFMA", raising=False)
    assert ["mfma" in nm for nm in nonlocal_ops()] == [True, True, False]
    monkeypatch.setenv("GLSDET_NONLOCAL_MFMA", "0")
    assert ["mfma" in nm for nm in nonlocal_ops()] == [False, False, False]
    monkeypatch.setenv("GLSDET_NONLOCAL_MFMA", "1")
    assert ["mfma" in nm for nm in nonlocal_ops()] == [True, True, True]


# --------------------------------------------------------------------------------------------------------------- twin
def test_cross10_twin_harness_flow_equals_detect(drone_path, monkeypatch):
    from glsdet_amd.detector import HipDetector
    monkeypatch.setenv("GLSDET_AUTOTUNE", "0")                   # both sides on the same kernel choices: same logits
    phi, shape = X.CASES[0]
    H, W = shape[2:]
    sd, x = X.weights(phi), X.case_input(phi, shape)
    det = HipDetector("cross10", sd, dtype="f32")
    dec, dets = det.detect(x.cuda(), 0.3, 0.5)
    m = importlib.import_module("models.new.yolox10")
    ub = importlib.import_module("models.core.utils_bbox")
    net = m.YoloBody(X.NUM_CLASSES, phi, dtype="f32")
    net.load_state_dict(sd)
    with torch.no_grad():
        outputs = net.eval()(x.cuda())
        twin_dec = ub.decode_outputs(outputs, [H, W])
        res = ub.non_max_suppression(twin_dec, X.NUM_CLASSES, [H, W], np.array([H, W]), False, conf_thres=0.3, nms_thres=0.5)
    assert torch.equal(torch.as_tensor(dec).contiguous().cpu().view(torch.int32), torch.as_tensor(twin_dec).contiguous().cpu().view(torch.int32))
    assert sum(len(d) for d in dets) > 0, "nothing detected: the comparison would be empty"
    for d, r in zip(dets, res):
        if len(d) == 0:
            assert r is None
            continue
        assert r is not None and r.shape == d.shape
        np.testing.assert_array_equal(r[:, 4:], d[:, 4:])
        px = d[:, [1, 0, 3, 2]].astype(np.float64) * np.array([H, W, H, W])
        np.testing.assert_allclose(r[:, :4], px, rtol=1e-5, atol=1e-3)
    print("cross10 twin: detections per image %s" % [len(d) for d in dets])
