"""Kind `cfp` on the GPU (the reference's models/cfp/yolox_cfp.py): EVCBlock, LVCBlock and LightMLPBlock against the outputs
the reference's own modules gave (tests/golden/cfp_golden.npz) and the restatement tests/cfp_reference.py; HipDetector on
the four golden cases; the captured plan; detect(); the drone twin.  The bars are those of tests/test_cross10.py: f32 logits
within max(1e-4, 2 x the reference's own fp32-vs-float64 distance) relative to max(1, |logit|); f16 rms within 1.5 x (max within
2 x) of the fp16-storage emulation's distance from the reference; blocks within 5e-5 (f32) / 4e-3 (f16) of max(1, |want|max).
tests/test_cfp_reference.py shows on the CPU that the recorded data move by at least 100 x the f32 bar under every planted
misreading of the block (10 x for the GELU form), so these comparisons see the new kernels."""
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from oracle import glsdet_oracle as O
from tests import cfp_reference as X

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CASE_IDS = [X.case_name(*c) for c in X.CASES]
LOGIT_TOL = 1e-4                                     # tests/test_cross10.py
BLOCK_TOL = {"f32": 5e-5, "f16": 4e-3}               # tests/test_cross10.py, the residual block
_TT = {"f16": torch.float16, "f32": torch.float32}


@pytest.fixture
def drone_path(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "glsdet_amd", "drone"))
    for mod in list(sys.modules):
        if mod == "models" or mod.startswith("models."):
            monkeypatch.delitem(sys.modules, mod)


# -------------------------------------------------------------------------------------------------------- block level
def _block_hip(kind, sd, x, dtype, trace=None):
    from glsdet_amd.engine import Engine
    from glsdet_amd.nets import NetBuilder, cfp_bn_eps
    eng = Engine(dtype)
    b = NetBuilder(eng, sd)
    b.bn_eps, b.trace = cfp_bn_eps, trace
    n, C, H, W = x.shape
    xv = eng.tensor(n, H, W, C)
    xv.buf.view(_TT[dtype])[: n * H * W * C] = x.permute(0, 2, 3, 1).contiguous().to(_TT[dtype]).reshape(-1).cuda()
    y = {"lvc": lambda: b.lvc("blk.lvc", xv), "l_MLP": lambda: b.light_mlp("blk.l_MLP", xv), "evc": lambda: b.evc("blk", xv)}[kind]()
    torch.cuda.synchronize()
    return y.to_nchw(C).cpu(), xv.to_nchw(C).cpu()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("rec", X.BLOCK_RECORDS, ids=[r[0] for r in X.BLOCK_RECORDS])
@pytest.mark.parametrize("kind", X.BLOCK_KINDS)
def test_block_matches_the_reference_block_and_the_restatement(kind, rec, dtype):
    name, C, h, w, n = rec
    sd, x = X.block_weights(C), X.block_input(C, h, w, n)
    want = X.block_recorded(kind, name)
    if dtype == "f16":                               # the recorded outputs belong to the fp32 input: the restatement on the rounded one
        x = x.half().float()
        want = X.run_block(kind, sd, x)
    got, x_after = _block_hip(kind, sd, x, dtype)
    assert torch.equal(x_after, x), "the block's input was written"
    scale = max(1.0, float(want.abs().max()))
    err, err_restated = float((got - want).abs().max()), float((got - X.run_block(kind, sd, x)).abs().max())
    print("%s %s %s: max |err| vs reference %.2e, vs restatement %.2e, |want|max %.2f" % (kind, name, dtype, err, err_restated, scale))
    assert err <= BLOCK_TOL[dtype] * scale and err_restated <= BLOCK_TOL[dtype] * scale


@pytest.mark.parametrize("rec", X.BLOCK_RECORDS, ids=[r[0] for r in X.BLOCK_RECORDS])
def test_encoding_and_gate_inside_the_block_match_the_restatement(rec):
    """the fp32 encoding and gate vector that NetBuilder.lvc traces, against the float64 restatement fed the same tensor"""
    name, C, h, w, n = rec
    sd, x = X.block_weights(C), X.block_input(C, h, w, n)
    trace = {}
    _block_hip("lvc", sd, x, "f32", trace)
    z = trace["blk.lvc.LVC.0"]
    s64 = X.to64(sd)
    E = X.encoding(z.double(), s64["blk.lvc.LVC.3.codewords"], s64["blk.lvc.LVC.3.scale"])
    bound, _ = X.encode_bound(z, sd["blk.lvc.LVC.3.codewords"], sd["blk.lvc.LVC.3.scale"])
    assert bool(((trace["blk.lvc.encoding"].double() - E).abs() <= bound).all())
    assert trace["blk.lvc.gam"].shape == (n, C)
    assert float(trace["blk.lvc.gam"].min()) > 0 and float(trace["blk.lvc.gam"].max()) < 1


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("C", [192, 384, 96])
def test_groupnorm_of_one_group_at_the_evc_widths(dtype, C):
    """GroupNorm(1, C) at the widths of tiny / m (C / vn no divisor of 256: the widened host check) and at a width the
    kernel always took, against torch in float64; one rounding to the storage type on top of the fp32 affine step"""
    from glsdet_amd.engine import Engine
    eng = Engine(dtype)
    n, H, W = 2, 7, 9
    x = O.synth_input((n, C, H, W), C).to(_TT[dtype]).float() * 3 + 1
    x = x.to(_TT[dtype]).float()
    gamma, beta = O.synth_input((C,), C + 1) * 0.3 + 1, O.synth_input((C,), C + 2) * 0.2
    xv = eng.tensor(n, H, W, C)
    xv.buf.view(_TT[dtype])[: n * H * W * C] = x.permute(0, 2, 3, 1).contiguous().to(_TT[dtype]).reshape(-1).cuda()
    y = eng.groupnorm(xv, 1, eng.upload(gamma), eng.upload(beta), 1e-5, "none", out=eng.tensor(n, H, W, C))
    torch.cuda.synchronize()
    want = torch.nn.functional.group_norm(x.double(), 1, gamma.double(), beta.double(), 1e-5)
    err = (y.to_nchw(C).cpu().double() - want).abs()
    u = 2.0 ** -11 if dtype == "f16" else 2.0 ** -24
    assert bool((err <= 4 * u * want.abs().clamp(min=1)).all()), float(err.max())
    assert torch.equal(xv.to_nchw(C).cpu(), x)


def test_layer_scales_of_1e_5_survive_fp16():
    """At the reference's initial layer scales (1e-5) a second layer scale folded into fp16 weights underflows
    (1e-5 x weights of order 0.02 lies below the smallest fp16 normal); it rides in mlp.fc2's fp32 epilogue instead.
    On an input of order 3e-3, whose fp16 ulp (2e-6) is far below the branch's contribution, the block must move its input
    by what the float64 restatement says -- up to the two fp16 stores (y1 and the output) of values of the input's size."""
    C, h, w, n = 64, 5, 7, 2
    sd = X.block_weights(C)
    for k in ("blk.l_MLP.layer_scale_1", "blk.l_MLP.layer_scale_2"):
        sd[k] = torch.full_like(sd[k], 1e-5)
    # fc2 weights of 0.01 (folded: 1e-7, two steps of the fp16 denormal grid, 19 % off) behind mostly positive hidden units,
    # so that the 256 terms add up to a contribution the fp16 output can show
    sd["blk.l_MLP.mlp.fc2.weight"] = torch.full_like(sd["blk.l_MLP.mlp.fc2.weight"], 0.01)
    sd["blk.l_MLP.mlp.fc1.bias"] = sd["blk.l_MLP.mlp.fc1.bias"] + 2.0
    x = (0.003 * X.block_input(C, h, w, n)).half().float()
    with torch.no_grad():
        moved = X.light_mlp(X.to64(sd), "blk.l_MLP", x.double()) - x.double()
    got, _ = _block_hip("l_MLP", sd, x, "f16")
    got = got.double() - x.double()
    rms = lambda t: float(t.pow(2).mean().sqrt())
    store = 2 * 2.0 ** -11 * float(x.abs().max()) / 3 ** 0.5        # two roundings, each uniform within half an ulp of |x|max
    print("fp16 l_MLP at layer scales 1e-5: moved %.3e (float64), got-vs-float64 %.3e, two stores allow %.3e" % (rms(moved), rms(got - moved), store))
    assert rms(moved) > 4 * store, "the test would not see the branch"
    assert rms(got - moved) <= store
    assert rms(got) > 0.5 * rms(moved)


# -------------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("case", X.CASES, ids=_CASE_IDS)
def test_cfp_f32_meets_north_star_tolerance(case):
    """bar max(1e-4, 2 x noise) relative to max(1, |logit|), noise = the recorded reference-vs-fp64 distance"""
    from glsdet_amd.detector import HipDetector
    phi, shape = case
    sd, x = X.weights(phi), X.case_input(phi, shape)
    want, truth = X.recorded(phi, shape), X.recorded(phi, shape, "out64")
    noise = X.rel(want, truth)
    det = HipDetector("cfp", sd, dtype="f32")
    got = [g.cpu() for g in det.forward_raw(x.cuda())]
    assert [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    err_ref, err_truth = X.rel(got, want), X.rel(got, truth)
    print("cfp f32 %s: hip-vs-reference %.2e  hip-vs-fp64 %.2e  reference-vs-fp64 %.2e" % (X.case_name(phi, shape), err_ref, err_truth, noise))
    bar = max(LOGIT_TOL, 2.0 * noise)
    assert err_ref <= bar and err_truth <= bar


@pytest.mark.parametrize("case", X.CASES[:2], ids=_CASE_IDS[:2])
def test_cfp_f16_is_as_close_to_the_reference_as_fp16_storage_allows(case):
    from glsdet_amd.detector import HipDetector
    phi, shape = case
    sd, x = X.weights(phi), X.case_input(phi, shape)
    outs = X.recorded(phi, shape)
    got = [g.cpu() for g in HipDetector("cfp", sd, dtype="f16").forward_raw(x.cuda())]
    with torch.no_grad(), O.fp16_storage():
        emu = X.cfp_forward(sd, x)
    scale = max(float(w.abs().max()) for w in outs)
    cat = lambda a, b: torch.cat([(p - q).flatten() for p, q in zip(a, b)])
    r, e = cat(got, outs), cat(emu, outs)
    rms = lambda t: float(t.pow(2).mean().sqrt()) / scale
    print("cfp f16 %s: HIP vs reference max %.4f rms %.5f | emulation vs reference max %.4f rms %.5f (x max|logit| = %.2f)" % (
        X.case_name(phi, shape), float(r.abs().max()) / scale, rms(r), float(e.abs().max()) / scale, rms(e), scale))
    assert rms(r) <= 1.5 * rms(e) + 1e-4
    assert float(r.abs().max()) / scale <= 2.0 * float(e.abs().max()) / scale + 1e-3


def test_cfp_plan_graph_replay_equals_eager():
    from glsdet_amd.detector import HipDetector
    phi, shape = X.CASES[1]
    sd = X.weights(phi)
    det = HipDetector("cfp", sd, dtype="f16")
    xs = [X.case_input(phi, shape).cuda(), O.synth_input(shape, 7).cuda()]
    eager = [[t.clone() for t in det.forward_raw(x)] for x in xs]
    c = det.compile(shape[0], shape[2], shape[3], None, use_graph=True)
    for x, want in zip(xs + xs[:1], eager + eager[:1]):
        det.run(c, x)
        torch.cuda.synchronize()
        for p, l in zip(want, c.levels):
            assert torch.equal(p, l.to_nchw(5 + X.NUM_CLASSES))
    names = [o["name"] for o in c.plan.ops()]
    assert sum(nm.startswith("lvc_encode") for nm in names) == 1 and sum(nm.startswith("lvc_gate") for nm in names) == 1
    assert sum(nm.startswith("channel_fuse") for nm in names) == 2 and sum(nm.startswith("groupnorm") for nm in names) == 2


def test_unknown_kind_and_odd_sizes_are_refused_as_for_base():
    from glsdet_amd.detector import HipDetector
    sd = X.weights("tiny")
    for kind in ("base", "cfp"):
        with pytest.raises(ValueError, match="multiples of 32"):
            HipDetector(kind, sd, dtype="f16").compile(1, 100, 160)
    with pytest.raises(ValueError, match="unknown detector kind"):
        HipDetector("cfq", sd, dtype="f16").compile(1, 64, 64)


# --------------------------------------------------------------------------------------------------------------- twin
def test_cfp_twin_harness_flow_equals_detect(drone_path, monkeypatch):
    from glsdet_amd.detector import HipDetector
    monkeypatch.setenv("GLSDET_AUTOTUNE", "0")                   # both sides on the same kernel choices: same logits
    phi, shape = X.CASES[0]
    H, W = shape[2:]
    sd, x = X.weights(phi), X.case_input(phi, shape)
    det = HipDetector("cfp", sd, dtype="f32")
    dec, dets = det.detect(x.cuda(), 0.3, 0.5)
    m = importlib.import_module("models.cfp.yolox_cfp")
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
    print("cfp twin: detections per image %s" % [len(d) for d in dets])


def test_cfp_twin_round_trip_gives_the_recorded_outputs(drone_path, monkeypatch):
    """a reference-named state dict loads into the twin, comes back unchanged, and the twin gives the recorded outputs"""
    monkeypatch.setenv("GLSDET_AUTOTUNE", "0")
    phi, shape = X.CASES[3]
    sd = X.weights(phi)
    m = importlib.import_module("models.cfp.yolox_cfp")
    net = m.YoloBody(X.NUM_CLASSES, phi, dtype="f32")
    net.load_state_dict(sd, strict=True)
    back = net.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    other = m.YoloBody(X.NUM_CLASSES, phi, dtype="f32")
    other.load_state_dict(back, strict=True)
    with torch.no_grad():
        got = [g.cpu() for g in other.eval()(X.case_input(phi, shape))]
    want, truth = X.recorded(phi, shape), X.recorded(phi, shape, "out64")
    assert X.rel(got, want) <= max(LOGIT_TOL, 2.0 * X.rel(want, truth))
