"""GPU: the sigmoid mask of the YOLOX decode (glsdet_yolox_decode_ex; bit 0 objectness, bit 1 classes) through every
layer that carries it -- the C ABI, Engine.decode, torch.ops.glsdet.yolox_decode, HipDetector.detect(decode_mode=...)
and the drone twin's five decode functions (drone/models/core/utils_bbox.py:36-306).

    vs float64          every mask x both box formats x 1 / 3 / 8 levels, |err| / (|x| + 1) <= 1e-5 (the decode bound of
                        tests/test_post_fuzz.py) against tests/decode_reference.decode_f64
    vs the reference    the five functions by name against tests/golden/decode_modes_golden.npz (recorded from the
                        reference on the CPU), same bound; `decode_outputs` is the control that the bound is fair
    exactness           (a) mask 3 == glsdet_yolox_decode, (b) the box channels do not depend on the mask, (c) a channel
                        outside the mask is the input logit, (d) a channel inside it is the mask-3 value: all bit for bit
    NMS                 raw-logit predictions (negative scores, scores above 1) through glsdet_nms == the sequential
                        reference of tests/post_reference.py, keep set, order and values
The reference checkout is never read here."""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest
import torch

from tests import decode_reference as D
from tests import post_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"default": 3, "obj_sigmoid": 1, "no_sigmoid": 0, "cls_sigmoid": 2}


@pytest.fixture(scope="module")
def eng():
    from glsdet_amd.engine import Engine
    return Engine("f32")


@pytest.fixture()
def drone_path(monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "glsdet_amd", "drone"))
    for mod in list(sys.modules):
        if mod == "models" or mod.startswith("models."):
            monkeypatch.delitem(sys.modules, mod)


def _level_view(eng, x_nchw, embed):
    """fp32 NHWC level on the device (the construction of tests/test_post_fuzz.py).  embed: the level is a window of a
    wider, taller buffer (channel stride above 5 + nc, a spatial border) whose every other element is NaN."""
    from glsdet_amd.engine import F32, TView
    n, c, h, w = x_nchw.shape
    if not embed:
        ctot, c0, border = c, 0, 0
    else:
        ctot, c0, border = c + 11, 3, 1
    H, W = h + 2 * border, w + 2 * border
    t = torch.full((n, H, W, ctot), float("nan"))
    t[:, border:border + h, border:border + w, c0:c0 + c] = x_nchw.permute(0, 2, 3, 1)
    buf = eng.raw(t.numel() * 4)
    buf.view(torch.float32)[: t.numel()] = t.flatten().to(eng.device)
    return TView(buf, (border * W + border) * ctot + c0, n, h, w, c, H * W * ctot, W * ctot, ctot, F32)


def _bits(t):
    return torch.as_tensor(t).contiguous().cpu().view(torch.int32)


def _flat_logits(xs, nc):
    """[n, 5 + nc, h, w] levels -> [n, A, 5 + nc] in the decode's anchor order"""
    return torch.cat([x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1])[..., : 5 + nc] for x in xs], 1).contiguous()


GEOMETRIES = [
    dict(id="fmt0_3lv_nonsquare_nostrides", mode=0, sizes=[(12, 16), (6, 8), (3, 4)], hw=(96, 160), strides=None, nc=10, embed=False, sf=False),
    dict(id="fmt1_3lv_nonsquare_nostrides_sf", mode=1, sizes=[(12, 16), (6, 8), (3, 4)], hw=(96, 160), strides=None, nc=3, embed=True, sf=True),
    dict(id="fmt0_1lv_strides_embedded", mode=0, sizes=[(7, 9)], hw=(56, 72), strides=[8], nc=1, embed=True, sf=False),
    dict(id="fmt1_1lv_strides", mode=1, sizes=[(5, 13)], hw=(80, 208), strides=[16], nc=80, embed=False, sf=False),
    dict(id="fmt0_8lv_strides_embedded", mode=0, sizes=[(17, 23), (9, 12), (9, 12), (5, 6), (3, 3), (2, 2), (1, 3), (1, 1)], hw=(136, 184),
         strides=[8, 16, 16, 32, 48, 64, 96, 128], nc=4, embed=True, sf=False),
    dict(id="fmt1_8lv_nostrides_sf", mode=1, sizes=[(17, 23), (9, 12), (9, 12), (5, 6), (3, 3), (2, 2), (1, 3), (1, 1)], hw=(136, 184),
         strides=None, nc=2, embed=False, sf=True),
]


def _inputs(case, n=3):
    """random head outputs: size logits over the whole +-20 range, saturated (+-20, +-40), denormal and zero score logits"""
    nc = case["nc"]
    g = torch.Generator().manual_seed(100 + len(case["id"]))
    xs = []
    for h, w in case["sizes"]:
        x = torch.randn(n, 5 + nc, h, w, generator=g) * 2.0
        x[:, 2:4] = torch.rand(n, 2, h, w, generator=g) * 40.0 - 20.0
        x[0, 2, 0, 0], x[0, 3, 0, 0] = 20.0, -20.0
        x[0, 4, 0, 0], x[0, 5, 0, 0], x[1, 4, 0, 0], x[1, 5, 0, 0] = 20.0, -20.0, 40.0, -40.0
        x[2, 4, 0, 0], x[2, 5, 0, 0] = -40.0, 40.0
        x[2, 4, -1, -1], x[2, 5, -1, -1], x[1, 4, -1, -1], x[1, 5, -1, -1] = 1e-40, -1e-40, -0.0, 1.4e-45      # denormals, -0
        xs.append(x)
    sf = (torch.rand(n, 4, generator=g) + 0.5) if case["sf"] else None
    return xs, sf


def _decode(eng, case, xs, sf, mask):
    in_h, in_w = case["hw"]
    out = eng.decode([_level_view(eng, x, case["embed"]) for x in xs], case["nc"], in_h, in_w, strides=case["strides"],
                     mode=case["mode"], scale_factors=sf.cuda().contiguous() if sf is not None else None, sigmoid=mask)
    torch.cuda.synchronize()
    return out.cpu()


def _decode_old_entry(eng, case, xs, sf):
    """glsdet_yolox_decode, the entry point without a mask, as Engine.decode called it before"""
    from glsdet_amd._lib import View, check
    from glsdet_amd.engine import _stream_ptr
    levels = [_level_view(eng, x, case["embed"]) for x in xs]
    n, A, nc = xs[0].shape[0], sum(h * w for h, w in case["sizes"]), case["nc"]
    out = torch.full((n, A, 5 + nc), float("nan"), device=eng.device)
    arr = (View * len(levels))(*[l.as_c() for l in levels])
    st = (C.c_int32 * len(levels))(*case["strides"]) if case["strides"] is not None else None
    sfd = sf.cuda().contiguous() if sf is not None else None
    check(eng.lib.glsdet_yolox_decode(arr, len(levels), nc, case["hw"][0], case["hw"][1], st, case["mode"], out.data_ptr(),
                                      out.numel(), sfd.data_ptr() if sfd is not None else None, _stream_ptr(eng.stream)),
          "yolox_decode")
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------ vs float64
@pytest.mark.parametrize("mask", [0, 1, 2, 3])
@pytest.mark.parametrize("case", GEOMETRIES, ids=[c["id"] for c in GEOMETRIES])
def test_decode_every_mask_vs_float64_formula(eng, case, mask):
    """both box formats; 1, 3 and 8 levels; strides = None on non-square inputs whose grids are not in_w / w wide and
    explicit strides; scale factors; level views embedded in NaN-filled buffers.  Bound: 1e-5 on |x| + 1."""
    xs, sf = _inputs(case)
    in_h, in_w = case["hw"]
    if case["strides"] is None:
        assert any(in_h / h != in_w / w for h, w in case["sizes"])
    got = _decode(eng, case, xs, sf, mask)
    want = D.decode_f64(xs, case["nc"], in_h, in_w, case["strides"], case["mode"], sf, mask)
    assert got.shape == want.shape == (3, sum(h * w for h, w in case["sizes"]), 5 + case["nc"])
    assert bool(torch.isfinite(got).all())
    err = D.rel_err(got, want)
    print("decode %s mask %d: max |err| / (|x| + 1) = %.3e" % (case["id"], mask, err))
    assert err <= D.BOUND


# ------------------------------------------------------------------------------------------------ exactness
@pytest.mark.parametrize("case", GEOMETRIES, ids=[c["id"] for c in GEOMETRIES])
def test_mask_exactness_conditions(eng, case):
    """Not tolerances: (a) the new entry with mask 3 == the old entry; for every mask (b) channels 0..3 == the mask-3
    output, (c) every channel outside the mask == the input logit (+-40, denormals and -0 included), (d) every channel
    inside the mask == the mask-3 output -- all compared as 32-bit patterns."""
    xs, sf = _inputs(case)
    nc = case["nc"]
    raw = _bits(_flat_logits(xs, nc))
    assert int((_flat_logits(xs, nc)[..., 4:].abs() == 40.0).sum()) >= 4
    tiny = _flat_logits(xs, nc)[..., 4:6].abs()
    assert bool(((tiny > 0) & (tiny < 1.1754944e-38)).any())                     # denormal inputs are really there
    full = _bits(_decode(eng, case, xs, sf, 3))
    old = _bits(_decode_old_entry(eng, case, xs, sf))
    assert torch.equal(full, old), "(a) mask 3 differs from glsdet_yolox_decode"
    for mask in (0, 1, 2, 3):
        got = _bits(_decode(eng, case, xs, sf, mask))
        assert torch.equal(got[..., :4], full[..., :4]), "(b) boxes depend on mask %d" % mask
        obj_ref, cls_ref = (full if mask & 1 else raw), (full if mask & 2 else raw)
        assert torch.equal(got[..., 4], obj_ref[..., 4]), "(%s) objectness, mask %d" % ("d" if mask & 1 else "c", mask)
        assert torch.equal(got[..., 5:], cls_ref[..., 5:]), "(%s) classes, mask %d" % ("d" if mask & 2 else "c", mask)
    assert not torch.equal(full[..., 4:], raw[..., 4:])


# ------------------------------------------------------------------------------------------------ vs the reference golden
@pytest.fixture(scope="module")
def decode_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "decode_modes_golden.npz"))


@pytest.mark.parametrize("name", sorted(D.VARIANTS))
def test_twin_function_reproduces_the_reference_golden_from_a_foreign_nchw_list(drone_path, decode_golden, name):
    """the reference's function names on the drop-in module, fed plain [B, 5 + nc, H, W] tensors (the staging route)"""
    ub = importlib.import_module("models.core.utils_bbox")
    g = decode_golden
    levels = [torch.from_numpy(g["level%d" % l]) for l in range(3)]
    before = [x.clone() for x in levels]
    got = getattr(ub, name)(levels, [int(v) for v in g["input_shape"]])
    torch.cuda.synchronize()
    want = g["ref/" + name]
    assert got.is_cuda and tuple(got.shape) == want.shape and got.dtype == torch.float32
    err = D.rel_err(got.cpu(), want)
    print("%s vs the reference's float32 output: max |err| / (|x| + 1) = %.3e" % (name, err))
    assert err <= D.BOUND
    assert all(_bits(a).equal(_bits(b)) for a, b in zip(levels, before)), "the twin mutated its input"
    mode, mask = D.VARIANTS[name]
    raw = _flat_logits(levels, int(g["num_classes"]))
    if not mask & 1:
        assert _bits(got[..., 4]).equal(_bits(raw[..., 4]))
    if not mask & 2:
        assert _bits(got[..., 5:]).equal(_bits(raw[..., 5:]))


def test_twin_functions_on_the_raw_outputs_of_a_real_forward(drone_path, golden, shapes, monkeypatch):
    """the native route: RawOutputs of the twin's own forward carry their NHWC levels; every function decodes those
    and gives, bit for bit, what it gives for the same logits as a plain NCHW list"""
    from tests.helpers import model_case
    monkeypatch.setenv("GLSDET_AUTOTUNE", "0")
    meta, sd, x, outs, _ = model_case(golden, shapes, "gl_tiny_seed0")
    m = importlib.import_module("models.block.non_local.yolo_patch_nonlocal_plus")
    ub = importlib.import_module("models.core.utils_bbox")
    net = m.YoloBody(10, meta["phi"], dtype="f32")
    net.load_state_dict(sd)
    input_shape = meta["in_shape"][2:]
    with torch.no_grad():
        outputs = net.eval()(x.cuda())
    assert outputs.compiled is not None
    A = sum(o.shape[2] * o.shape[3] for o in outs)
    full = ub.decode_outputs(outputs, input_shape)
    for name, (mode, mask) in D.VARIANTS.items():
        got = getattr(ub, name)(outputs, input_shape)
        plain = getattr(ub, name)([o.clone() for o in outputs], input_shape)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (x.shape[0], A, 15) == tuple(full.shape)
        assert _bits(got).equal(_bits(plain)), name
        raw = _flat_logits([o.cpu() for o in outputs], 10)
        assert D.rel_err(got.cpu(), D.decode_f64([o.cpu() for o in outputs], 10, input_shape[0], input_shape[1], None, mode, None, mask)) <= D.BOUND
        if mask == 0:
            assert _bits(got[..., 4:]).equal(_bits(raw[..., 4:]))


# ------------------------------------------------------------------------------------------------ NMS on raw-logit predictions
NMS_IN = (128, 256)                                    # powers of two: the normalised boxes stay dyadic
NMS_SIZES = [(16, 32), (8, 16), (4, 8)]                # strides 8, 16, 32 (= in_h / h; strides are not passed)
NMS_NC = 3


def _nms_logits(n=3):
    """Head outputs whose decoded boxes lie on a dyadic grid: offsets are multiples of 1/8 of a cell, size logits 0
    (side = stride), so (t + g) * s, the division by 128 / 256 and the NMS's cx -+ w / 2 are all exact in float32 and
    every IoU term is a small integer multiple of 2^-15 -- one correctly rounded division decides, as in
    tests/post_reference.py.  Offsets are k + h / 2 + j / 8 cells (k = -1, 0, 1; h = 1 for a quarter of them; j = 0, 1):
    boxes of neighbouring anchors coincide (IoU 1), sit an eighth of a side apart on one axis (0.78) or on both (0.62),
    or half a side and more (<= 0.33) -- suppression on either side of both thresholds used below; 20 blocks of 3 x 3
    anchors of the finest level all point at one cell (up to an eighth), so a good part of the candidates is suppressed.
    Score logits:
    normal(0, 2.5) objectness, normal(-0.5, 2.5) classes -- negative x negative products, products above 1 and negative
    products all occur (asserted where they are used); a few anchors force them."""
    g = torch.Generator().manual_seed(77)
    xs = []
    for h, w in NMS_SIZES:
        x = torch.zeros(n, 5 + NMS_NC, h, w)
        x[:, 0:2] = (torch.randint(-1, 2, (n, 2, h, w), generator=g).float() +
                     torch.randint(0, 4, (n, 2, h, w), generator=g).clamp(min=2).float() / 2.0 - 1.0 +
                     torch.randint(0, 2, (n, 2, h, w), generator=g).float() / 8.0)
        if (h, w) == NMS_SIZES[0]:                     # 3 x 3 blocks of anchors that all point at their block's centre cell
            pat = torch.tensor([1.0, 0.0, -1.0])
            jit = torch.randint(0, 2, (n, 2, 6, 30), generator=g).float() / 8.0
            x[:, 0, 4:10, 0:30] = pat.repeat(10)[None, None, :] + jit[:, 0]
            x[:, 1, 4:10, 0:30] = pat.repeat(2)[None, :, None] + jit[:, 1]
        x[:, 4] = torch.randn(n, h, w, generator=g) * 2.5
        x[:, 5:] = torch.randn(n, NMS_NC, h, w, generator=g) * 2.5 - 0.5
        x[:, 4, 1, 1], x[:, 5:, 1, 1] = -3.0, torch.tensor([-2.0, -2.5, -4.0])[None, :]       # (-3) * (-2) = 6
        x[:, 4, 1, 2], x[:, 5:, 1, 2] = -3.5, torch.tensor([-2.5, -2.0, -4.0])[None, :]       # its neighbour, another class
        x[:, 4, 2, 1], x[:, 5:, 2, 1] = 2.5, torch.tensor([-1.0, -1.5, -3.0])[None, :]        # negative product: rejected
        xs.append(x)
    return xs


@pytest.mark.parametrize("conf,thr", [(0.01, 0.65), (0.5, 0.4)], ids=["harness_defaults", "conf0.5_iou0.4"])
@pytest.mark.parametrize("fmt", [0, 1], ids=["cxcywh_norm", "xyxy_px"])
@pytest.mark.parametrize("mask", [0, 1, 2])
def test_nms_on_raw_logit_predictions_equals_the_sequential_reference(eng, mask, fmt, conf, thr):
    """decode with the mask -> glsdet_nms -> every image equal to tests/post_reference.reference_dets on the same
    prediction: counts, keep set, order and all seven columns, bit for bit"""
    xs = _nms_logits()
    n, A = xs[0].shape[0], sum(h * w for h, w in NMS_SIZES)
    pred_t = eng.decode([_level_view(eng, x, True) for x in xs], NMS_NC, NMS_IN[0], NMS_IN[1], mode=fmt, sigmoid=mask)
    nb = eng.nms_buffers(n, A, A, A)
    dets, count, status = eng.nms(pred_t, NMS_NC, fmt, conf, thr, nb)
    torch.cuda.synchronize()
    pred, dets, count = pred_t.cpu().numpy(), dets.cpu().numpy(), count.cpu().numpy()
    assert int(status.item()) == 0
    # the grid the exactness argument needs (checked on what the decode really produced)
    unit = np.asarray([256.0, 128.0, 256.0, 128.0]) if fmt == 0 else np.ones(4)
    scaled = pred[..., :4].astype(np.float64) * unit
    assert np.array_equal(scaled, np.rint(scaled)) and np.abs(scaled).max() < 1024
    # what the inputs must contain
    obj, best = pred[..., 4], pred[..., 5:].max(-1)
    score = obj * best
    assert (score > 1.0).any() and (score < 0).any()                              # above 1: kept candidates; negative: rejected
    if mask == 0:
        assert ((obj < 0) & (best < 0) & (score >= np.float32(conf))).any()       # a product of two negative logits passes
    elif mask == 1:
        assert ((obj >= 0) & (obj <= 1)).all() and (best < 0).any() and (best > 1).any()
    else:
        assert ((pred[..., 5:] >= 0) & (pred[..., 5:] <= 1)).all() and (obj < 0).any() and (obj > 1).any()
    for i in range(n):
        cand = R.candidates(pred[i], NMS_NC, fmt, conf)
        ref = R.reference_dets(pred[i], NMS_NC, fmt, thr, conf)
        K = len(ref)
        print("mask %d image %d: %d candidates, reference keeps %d, kernel %d; scores %.3g .. %.3g" % (
            mask, i, len(cand["scores"]), K, count[i], cand["scores"].min(), cand["scores"].max()))
        assert 0 < K < len(cand["scores"]), "image %d needs a kept and a suppressed candidate" % i
        assert cand["scores"].max() > 1.0
        got = dets[i, : int(count[i])]
        assert count[i] == K and count[n + i] == K, (i, count.tolist(), K)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (i, int((got != ref).any(1).argmax()))


# ------------------------------------------------------------------------------------------------ the harness flow
@pytest.mark.parametrize("decode_mode", sorted(NAMES))
def test_detect_decode_mode_equals_the_twin_harness_flow(drone_path, golden, shapes, monkeypatch, decode_mode):
    """HipDetector.detect(..., decode_mode=m) against yolo.py:143-150 on the drop-in modules (YoloBody -> decode_func
    -> non_max_suppression), same weights and image, at the harness's default thresholds.  The twin returns
    [y1, x1, y2, x2] in pixels of `image_shape` (utils_bbox.py:8-33), detect x1, y1, x2, y2 normalised."""
    from glsdet_amd.detector import HipDetector
    from tests.helpers import model_case
    monkeypatch.setenv("GLSDET_AUTOTUNE", "0")                   # both sides on the same kernel choices: same logits
    meta, sd, x, _, _ = model_case(golden, shapes, "gl_tiny_seed0")
    H, W = meta["in_shape"][2:]
    det = HipDetector("gl", sd, dtype="f32")
    dec, dets = det.detect(x.cuda(), 0.01, 0.65, decode_mode=decode_mode)
    m = importlib.import_module("models.block.non_local.yolo_patch_nonlocal_plus")
    ub = importlib.import_module("models.core.utils_bbox")
    net = m.YoloBody(10, meta["phi"], dtype="f32")
    net.load_state_dict(sd)
    with torch.no_grad():
        outputs = net.eval()(x.cuda())
        twin_dec = getattr(ub, D.HARNESS_MODES[decode_mode])(outputs, [H, W])
        res = ub.non_max_suppression(twin_dec, 10, [H, W], np.array([H, W]), False, conf_thres=0.01, nms_thres=0.65)
    assert _bits(dec).equal(_bits(twin_dec))
    want = D.decode_f64([o.cpu() for o in outputs], 10, H, W, None, 0, None, NAMES[decode_mode])
    assert D.rel_err(dec.cpu(), want) <= D.BOUND
    assert sum(len(d) for d in dets) > 0, "nothing detected: the comparison would be empty"
    for d, r in zip(dets, res):
        if len(d) == 0:
            assert r is None
            continue
        assert r is not None and r.shape == d.shape
        np.testing.assert_array_equal(r[:, 4:], d[:, 4:])                              # obj, class conf, class: same order
        px = d[:, [1, 0, 3, 2]].astype(np.float64) * np.array([H, W, H, W])
        np.testing.assert_allclose(r[:, :4], px, rtol=1e-5, atol=1e-3)
    print("%s: detections per image %s" % (decode_mode, [len(d) for d in dets]))


def test_detect_rejects_an_unknown_decode_mode(golden, shapes):
    from glsdet_amd.detector import HipDetector
    from tests.helpers import model_case
    meta, sd, x, _, _ = model_case(golden, shapes, "gl_tiny_seed0")
    with pytest.raises(ValueError, match="decode_mode"):
        HipDetector("gl", sd, dtype="f32").detect(x.cuda(), 0.3, 0.5, decode_mode="bogus")


def test_compile_keys_plans_by_the_sigmoid_mask(golden, shapes):
    from glsdet_amd.detector import HipDetector
    from tests.helpers import model_case
    meta, sd, x, _, _ = model_case(golden, shapes, "gl_tiny_seed0")
    det = HipDetector("gl", sd, dtype="f32")
    n, _, H, W = x.shape
    a = det.compile(n, H, W, dict(conf_thres=0.3, nms_thres=0.5))
    b = det.compile(n, H, W, dict(conf_thres=0.3, nms_thres=0.5, sigmoid=1))
    assert a is not b and det.compile(n, H, W, dict(conf_thres=0.3, nms_thres=0.5, sigmoid=1)) is b
    det.run(a, x.cuda())
    det.run(b, x.cuda())
    torch.cuda.synchronize()
    assert _bits(a.decoded[..., :5]).equal(_bits(b.decoded[..., :5])) and not _bits(a.decoded[..., 5:]).equal(_bits(b.decoded[..., 5:]))


# ------------------------------------------------------------------------------------------------ torch op
@pytest.mark.parametrize("mode", [0, 1])
def test_torch_op_carries_the_mask(eng, mode):
    import glsdet_amd.torch_ops  # noqa: F401
    nc, in_h, in_w = 10, 96, 160
    g = torch.Generator().manual_seed(5)
    xs = [torch.randn(2, 16, h, w, generator=g) * 3.0 for h, w in ((12, 20), (6, 10), (3, 5))]      # 16 channels: NHWC % 8
    levels = [x.permute(0, 2, 3, 1).contiguous().cuda() for x in xs]
    strides = [in_h // x.shape[2] for x in xs] if mode == 1 else None
    for s in (0, 1, 2, 3):
        got = torch.ops.glsdet.yolox_decode(levels, nc, in_h, in_w, mode, sigmoid=s)
        want = eng.decode([_level_view(eng, x, False) for x in xs], nc, in_h, in_w, strides=strides, mode=mode, sigmoid=s)
        torch.cuda.synchronize()
        assert tuple(got.shape) == (2, 315, 15) and _bits(got).equal(_bits(want)), s
    assert _bits(torch.ops.glsdet.yolox_decode(levels, nc, in_h, in_w, mode)).equal(_bits(got))      # positional call: mask 3
    meta = torch.ops.glsdet.yolox_decode([l.to("meta") for l in levels], nc, in_h, in_w, mode, 2)
    assert meta.device.type == "meta" and tuple(meta.shape) == (2, 315, 15) and meta.dtype == torch.float32
    for bad in (-1, 4):
        with pytest.raises(RuntimeError, match="sigmoid_mask"):
            torch.ops.glsdet.yolox_decode(levels, nc, in_h, in_w, mode, sigmoid=bad)
