"""Differential edge-case tests of the detection post-processing kernels (glsdet_amd/csrc/post.hip): both NMS families
(class-segmented sort / cmask / cscan, and rank / mask / scan) behind glsdet_nms, glsdet_gfl_detect,
glsdet_ufp_backmap_merge, glsdet_yolox_decode and glsdet_pack_detections.

NMS is compared BIT FOR BIT with the naive sequential reference of tests/post_reference.py: the kernels copy values, and
the inputs lie on a dyadic grid on which the IoU arithmetic is exact up to one correctly rounded division
(tests/test_post_reference.py proves on the CPU, for every case used here, that the float32 decisions equal the
exact-arithmetic ones).  The old kernel family is reached through candidate counts above 4096 and num_classes = 256,
never through an environment switch.  The dense cases (post_reference.dense_cases) run it where every anchor is a
candidate, up to the 32768 rows the kernels accept, with max_cand = max_det = A."""
import numpy as np
import pytest
import torch

from oracle import glsdet_oracle as O
from oracle import mpdet_oracle as M
from oracle import ufp_oracle as U
from tests import post_reference as R

pytestmark = pytest.mark.gpu

MAX_CAND = 8192
NMS_CASES = R.nms_cases()


@pytest.fixture(scope="module")
def engines():
    from glsdet_amd.engine import Engine
    return {"f32": Engine("f32")}


@pytest.fixture(scope="module")
def nbcache():
    """one workspace per (n, A, max_cand, max_det), reused by every case of that geometry -- as production replays
    one plan on one workspace: every case also runs on whatever the previous one left behind"""
    return {}


def _buffers(eng, nbcache, n, A, max_cand, max_det):
    key = (n, A, max_cand, max_det)
    if key not in nbcache:
        nbcache[key] = eng.nms_buffers(n, A, max_cand, max_det)
    return nbcache[key]


def _explain(got, ref):
    """keep-set diff of two [k,7] detection arrays, for the assertion message"""
    g, r = {tuple(x) for x in got.tolist()}, {tuple(x) for x in ref.tolist()}
    first = next((i for i in range(min(len(got), len(ref))) if not np.array_equal(got[i], ref[i])), min(len(got), len(ref)))
    return "kept %d, reference %d; %d rows only in the kernel's set, %d only in the reference's; first difference at row %d" % (
        len(got), len(ref), len(g - r), len(r - g), first)


def _run_nms(eng, nbcache, pred, nc, mode, thr, max_det=MAX_CAND, max_cand=MAX_CAND, refs=None):
    """glsdet_nms on pred; every image equal to the reference, all 7 columns, and the two counters"""
    n, A = pred.shape[:2]
    nb = _buffers(eng, nbcache, n, A, max_cand, max_det)
    t = torch.from_numpy(pred).cuda()
    dets, count, status = eng.nms(t, nc, mode, R.CONF_THR, thr, nb)
    torch.cuda.synchronize()
    dets, count = dets.cpu().numpy(), count.cpu().numpy()
    assert int(status.item()) == 0
    for i in range(n):
        ref = refs[i] if refs is not None else R.reference_dets(pred[i], nc, mode, thr)
        K = len(ref)
        print("image %d: kept %d (before max_det) / %d, reference %d" % (i, count[n + i], count[i], K))
        got = dets[i, : max(0, min(int(count[i]), max_det))]
        assert count[n + i] == K and count[i] == min(K, max_det), (i, count.tolist(), K, _explain(got, ref[:max_det]))
        assert np.array_equal(got, ref[:max_det]), (i, _explain(got, ref[:max_det]))
        np.testing.assert_array_equal(got, ref[:max_det])
    return dets, count


@pytest.mark.parametrize("case", NMS_CASES, ids=[c["id"] for c in NMS_CASES])
def test_nms_equals_the_sequential_reference(engines, nbcache, case):
    pred, _ = R.build_case(case)
    cap = case["cap"] or MAX_CAND
    _run_nms(engines["f32"], nbcache, pred, case["nc"], case["mode"], case["thr"], max_det=cap, max_cand=cap)


@pytest.mark.parametrize("m", [4095, 4096])
def test_nms_full_workspace_of_4096_has_no_second_path(engines, nbcache, m):
    """max_cand = 4096: the rank / mask / scan kernels are not launched at all, so an image that fills the workspace to
    the last candidate must be finished by the class-segmented kernels"""
    pred = R.to_pred([R.build_image(R.A_DEFAULT, 10, m, scores="few", seed=75)], 10, 0)
    _run_nms(engines["f32"], nbcache, pred, 10, 0, 0.65, max_det=4096, max_cand=4096)


@pytest.mark.parametrize("m", [1000, 5000, R.DENSE_A], ids=["class_segmented", "rank_mask_scan", "every_anchor_of_8400"])
def test_nms_max_det_around_the_kept_count(engines, nbcache, m):
    """max_det in {1, 64, K - 1, K, K + 1}: count[i] = min(K, max_det), count[n + i] = K, the first max_det rows.
    m = 8400: A = max_cand = m, every anchor a candidate."""
    A, cap = (R.A_DEFAULT, MAX_CAND) if m < R.A_DEFAULT else (m, m)
    pred = R.to_pred([R.build_image(A, 10, m, scores="few", seed=70)], 10, 1)
    ref = R.reference_dets(pred[0], 10, 1, 0.5)
    K = len(ref)
    assert 64 < K < m
    for md in (1, 64, K - 1, K, K + 1):
        _run_nms(engines["f32"], nbcache, pred, 10, 1, 0.5, max_det=md, max_cand=cap, refs=[ref])


def test_nms_workspace_reuse_and_determinism(engines):
    """one workspace: a 5000-candidate image (rank / mask / scan), then 70 candidates, then none (both class-segmented):
    each equals the reference although the workspace holds the larger earlier result; the same input twice gives
    bit-identical dets and count."""
    eng, cache = engines["f32"], {}
    outs = []
    for m in (5000, 70, 0, 5000, 5000):
        pred = R.to_pred([R.build_image(R.A_DEFAULT, 10, m, scores="few", seed=80)], 10, 1)
        dets, count = _run_nms(eng, cache, pred, 10, 1, 0.5)
        outs.append((dets.copy(), count.copy()))
    assert len(cache) == 1
    for a, b in ((outs[0], outs[3]), (outs[3], outs[4])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("m,max_cand", [(500, 64), (5000, 4096), (6000, 4097), (9000, 8400)])
def test_nms_overflow_is_flagged_and_returns_input_rows(engines, m, max_cand):
    """more candidates than max_cand: status bit 1, count <= max_det, every returned row is a row of the input.  (Which
    candidates are retained depends on their arrival order, by design: nothing more is asserted.)"""
    eng = engines["f32"]
    A = max(R.A_DEFAULT, m)
    pred = R.to_pred([R.build_image(A, 10, m, scores="few", seed=90)], 10, 1)
    rows = {tuple(x) for x in R.candidates(pred[0], 10, 1)["rows"].tolist()}
    nb = eng.nms_buffers(1, A, max_cand, 300)
    dets, count, status = eng.nms(torch.from_numpy(pred).cuda(), 10, 1, R.CONF_THR, 0.5, nb)
    torch.cuda.synchronize()
    count = count.cpu().numpy()
    assert int(status.item()) & 1
    assert 0 < count[0] <= 300 and count[0] <= count[1] <= max_cand
    for row in dets[0, : count[0]].cpu().numpy().tolist():
        assert tuple(row) in rows


def _layout_bytes(n, max_cand, with_mask=True):
    """nms_layout of post.hip restated in Python integers: every array rounded up to 256 bytes; the mask holds
    ceil(max_cand / 64) 8-byte words per candidate"""
    nw = (max_cand + 63) // 64
    parts = [n * 8] + [n * max_cand * k for k in (16, 16, 4, 4, 16, 16)]
    parts += [n * max_cand * nw * 8] if with_mask else []
    parts += [n * max_cand * 8, n * (256 + 256 + 260 + 260) * 4]
    return sum((p + 255) // 256 * 256 for p in parts)


@pytest.mark.parametrize("n,max_cand", [(1, R.NMS_MAX), (1, R.NMS_MAX - 1), (3, 22050), (2, 8400), (32, R.NMS_MAX)])
def test_nms_workspace_bytes_equals_the_layout_sum(engines, n, max_cand):
    """the n * max_cand * nw * 8 byte mask dominates: 128 MiB for one image of 32768 candidates, 4 GiB for 32 of them
    (above 2^31 and 2^32: a product taken in 32 bits would show).  Only the size is asked for; nothing is allocated."""
    want = _layout_bytes(n, max_cand)
    assert want > n * max_cand * ((max_cand + 63) // 64) * 8
    if (n, max_cand) == (1, R.NMS_MAX):
        assert want - _layout_bytes(n, max_cand, False) == 128 << 20
    if n == 32:
        assert want > 1 << 32
    assert int(engines["f32"].lib.glsdet_nms_workspace_bytes(n, max_cand, max_cand)) == want


def test_nms_refuses_more_than_32768_candidates_on_the_host(engines):
    """max_cand = 32769 is an argument error (GLSDET_E_ARG = -1) whose text names the limit; the check comes before the op
    is built, so nothing is launched: the outputs keep their sentinel values.  32768 with the same buffers is accepted
    up to the workspace check (GLSDET_E_CAPACITY = -5: the 256-byte workspace is too small), again without a launch."""
    lib = engines["f32"].lib
    pred = torch.zeros(1, 64, 6).cuda()
    dets, count = torch.full((1, 4, 7), -7.0).cuda(), torch.full((2,), -7, dtype=torch.int32).cuda()
    status, ws = torch.full((1,), -7, dtype=torch.int32).cuda(), torch.zeros(512, dtype=torch.uint8).cuda()
    wsp = (ws.data_ptr() + 255) // 256 * 256
    call = lambda mc: lib.glsdet_nms(pred.data_ptr(), 1, 64, 1, 1, 0.25, 0.5, mc, 4, dets.data_ptr(), count.data_ptr(),
                                     status.data_ptr(), wsp, 256, None)
    assert call(R.NMS_MAX + 1) == -1
    msg = lib.glsdet_last_error().decode()
    assert "32768" in msg and "32769" in msg, msg
    assert call(R.NMS_MAX) == -5
    torch.cuda.synchronize()
    assert (dets == -7.0).all() and (count == -7).all() and int(status.item()) == -7


# ------------------------------------------------------------------------------------------------ gfl_detect
GFL_SIZES = [(37, 53), (19, 27), (10, 14), (5, 7), (3, 4)]          # no H * W is a multiple of 64
GFL_STRIDES = [8, 16, 32, 64, 128]
GFL_IN = (296, 424)
GFL_SHAPES = [(290, 400, 3), (296, 424, 3)]                         # image 0 is clamped inside the padded input
GFL_SF = [[1.5, 1.25, 1.5, 1.25], [0.5, 0.5, 0.5, 0.5]]
GFL_CASES = [
    dict(id="rm16_nc10", seed=0, nc=10, reg_max=16, thr=0.05, bias=-3.0, nms_pre=1000, iou=0.6, maxdet=100, rescale=False),
    dict(id="rm16_nc1_cut", seed=1, nc=1, reg_max=16, thr=0.05, bias=-1.0, nms_pre=200, iou=0.6, maxdet=3000, rescale=True),
    dict(id="rm16_nc80", seed=7, nc=80, reg_max=16, thr=0.5, bias=-3.0, nms_pre=1000, iou=0.6, maxdet=2000, rescale=False),
    dict(id="rm7_nc10_cut", seed=3, nc=10, reg_max=7, thr=0.3, bias=-3.0, nms_pre=150, iou=0.5, maxdet=40, rescale=True),
    dict(id="rm7_nc1", seed=4, nc=1, reg_max=7, thr=0.05, bias=-2.0, nms_pre=1000, iou=0.6, maxdet=3000, rescale=False),
    dict(id="rm7_nc80_cut", seed=5, nc=80, reg_max=7, thr=0.5, bias=-3.0, nms_pre=300, iou=0.6, maxdet=100, rescale=True),
]
GFL_DENSE_CASES = [                                                 # level sizes of their own (the others share GFL_SIZES)
    # every (position, class) pair passes (sigmoid > 0): 48 * 64 * 10 = 30720 pairs on level 0, beyond the 8192 a level
    # holds by default; max_cand is sized for them
    dict(id="rm16_nc10_every_pair_30720_cut", seed=8, nc=10, reg_max=16, thr=0.0, bias=-3.0, nms_pre=1000, iou=0.6, maxdet=3000,
         rescale=False, sizes=[(48, 64), (24, 32), (12, 16), (6, 8), (3, 4)], input=(384, 512), shapes=[(380, 500, 3), (384, 512, 3)],
         max_cand=30720),
]


def _gfl_inputs(case, n=2):
    """random head outputs; class 0 is saturated (logit +40: sigmoid == 1.0f, equal scores) at a few positions of levels
    0 and 2 and switched off (-40) at a few others.  Only ONE class is saturated: the oracle orders equal scores of
    different classes class first, the kernels anchor first (tests/test_post_reference.py)."""
    g = torch.Generator().manual_seed(1000 + case["seed"])
    sizes = case.get("sizes", GFL_SIZES)
    cls = [torch.randn(n, case["nc"], h, w, generator=g) * 1.5 + case["bias"] for h, w in sizes]
    reg = [torch.randn(n, 4 * (case["reg_max"] + 1), h, w, generator=g) * 2.0 for h, w in sizes]
    for l, pos in ((0, [(0, 0), (5, 17), (5, 18), (20, 40), (36, 52)]), (2, [(3, 3), (9, 13)])):
        for b in range(n):
            for y, x in pos:
                cls[l][b, 0, y, x] = 40.0
                cls[l][b, 0, (y + 7) % sizes[l][0], x] = -40.0
    return cls, reg


def _gfl_reference(case, cls, reg, dtype):
    """oracle pre-NMS candidates evaluated in `dtype`, then its per-class NMS.  -> per image (boxes, scores, labels, keep)"""
    sf = GFL_SF if case["rescale"] else None
    pre = M.gfl_pre_nms([c.to(dtype) for c in cls], [r.to(dtype) for r in reg], GFL_STRIDES, case.get("shapes", GFL_SHAPES), case["thr"],
                        case["nms_pre"], sf, case["reg_max"])
    out = []
    for boxes, scores, labels in pre:
        bn, sn, ln = boxes.numpy(), scores.numpy(), labels.numpy()
        keep = O.batched_nms(bn, sn, ln.astype(np.float32), case["iou"])[: case["maxdet"]] if len(sn) else np.zeros(0, np.int64)
        out.append((bn, sn, ln, keep))
    return out


def _gfl_seed_conditions(case, cls, reg):
    """the conditions the seeds were chosen for (asserted, never skipped): the float32 and the float64 oracle keep the
    same candidates in the same order; no level has equal scores across its nms_pre cut; and no two candidates of
    DIFFERENT classes have bit-equal float32 scores next to each other in the result -- the oracle orders those class
    first, the kernels by candidate index (the documented difference of tests/test_post_reference.py; with 80 classes
    and ~2000 scores in (0.5, 1) such a coincidence is not rare).
    -> (f32 reference, f64 reference, levels cut by nms_pre)"""
    r32, r64 = _gfl_reference(case, cls, reg, torch.float32), _gfl_reference(case, cls, reg, torch.float64)
    for (b32, s32, l32, k32), (b64, s64, l64, k64) in zip(r32, r64):
        assert np.array_equal(l32, l64), "float32 / float64 oracles select different candidates: pick another seed"
        assert np.array_equal(k32, k64), "float32 / float64 oracles keep different sets: pick another seed"
        full = O.batched_nms(b32, s32, l32.astype(np.float32), case["iou"]) if len(s32) else k32
        assert np.array_equal(full, full[np.lexsort((full, -s32[full]))]), "equal scores in different classes: pick another seed"
    ncut = 0
    for c in cls:
        for b in range(c.shape[0]):
            sc = c[b].permute(1, 2, 0).reshape(-1).sigmoid()
            vs = torch.sort(sc[sc > case["thr"]], descending=True)[0]
            if len(vs) > case["nms_pre"]:
                ncut += 1
                assert vs[case["nms_pre"] - 1] > vs[case["nms_pre"]], "equal scores across the nms_pre cut: pick another seed"
    return r32, r64, ncut


@pytest.mark.parametrize("case", GFL_CASES + GFL_DENSE_CASES, ids=[c["id"] for c in GFL_CASES + GFL_DENSE_CASES])
def test_gfl_detect_vs_oracle_generic_integral_saturation_and_cuts(engines, case):
    """glsdet_gfl_detect against oracle.mpdet_oracle (gfl_pre_nms + batched_nms + max_per_img): labels, counts and the
    order are equal; scores to 1e-6 (the existing test's bound); box coordinates to max(1e-3, 2 x the float32 oracle's
    own distance from the float64 evaluation of the same formula).
    Measured on an MI355X, maximum over the six cases: kernel vs float64 1.15e-4 (per case 4.8e-5, 1.15e-4, 6.3e-5,
    2.9e-5, 2.8e-5, 3.8e-5), float32 oracle vs float64 6.6e-5 (4.3e-5, 6.6e-5, 4.8e-5, 4.4e-5, 2.8e-5, 4.0e-5), both in
    pixels; twice the oracle's error is below 1e-3 everywhere, so the 1e-3 floor is the bound that applies."""
    from tests.test_resdet import _fp32_view
    eng = engines["f32"]
    n, nc = 2, case["nc"]
    cls, reg = _gfl_inputs(case, n)
    r32, r64, ncut = _gfl_seed_conditions(case, cls, reg)
    assert ncut > 0 or "cut" not in case["id"]                             # a level holds more than nms_pre candidates
    nb = eng.gfl_buffers(n, 5, case.get("max_cand", 2 * MAX_CAND), case["nms_pre"], case["maxdet"])
    hw = torch.tensor([[s[0], s[1]] for s in case.get("shapes", GFL_SHAPES)], dtype=torch.float32).cuda()
    sft = torch.tensor(GFL_SF, dtype=torch.float32).cuda() if case["rescale"] else None
    in_h, in_w = case.get("input", GFL_IN)
    views = [_fp32_view(eng, c) for c in cls], [_fp32_view(eng, r) for r in reg]
    if "max_cand" in case:
        # the same input at the default capacity of a level (8192): reported, never a silently truncated result
        passing = max(int((c[b].sigmoid() > case["thr"]).sum()) for c in cls for b in range(n))
        assert MAX_CAND < passing <= case["max_cand"]
        small = eng.gfl_buffers(n, 5, MAX_CAND, case["nms_pre"], case["maxdet"])
        _, _, st = eng.gfl_detect(views[0], views[1], GFL_STRIDES, nc, case["reg_max"], in_h, in_w, case["thr"], case["iou"], small,
                                  img_hw=hw, scale_factors=sft)
        torch.cuda.synchronize()
        assert int(st.item()) & 1
    dets, count, status = eng.gfl_detect(views[0], views[1], GFL_STRIDES, nc, case["reg_max"], in_h, in_w, case["thr"],
                                         case["iou"], nb, img_hw=hw, scale_factors=sft)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    count, dets = count.cpu().numpy(), dets.cpu().numpy()
    err_k = err_o = 0.0
    for i in range(n):
        b32, s32, l32, keep = r32[i]
        b64 = r64[i][0]
        full = len(O.batched_nms(b32, s32, l32.astype(np.float32), case["iou"])) if len(s32) else 0
        assert count[i] == len(keep) and count[n + i] == full, (count.tolist(), len(keep), full)
        got = dets[i, : count[i]]
        np.testing.assert_array_equal(got[:, 6].astype(np.int64), l32[keep])
        np.testing.assert_allclose(got[:, 4], s32[keep], atol=1e-6, rtol=0)
        if len(keep):
            assert s32[keep][0] == 1.0 and (s32[keep] == 1.0).sum() >= 2      # the saturated positions lead, tied
            err_k = max(err_k, float(np.abs(got[:, :4].astype(np.float64) - b64[keep]).max()))
            err_o = max(err_o, float(np.abs(b32[keep].astype(np.float64) - b64[keep]).max()))
    print("gfl %s: kernel vs float64 %.3e, float32 oracle vs float64 %.3e, kept %s" % (case["id"], err_k, err_o, count[:n]))
    assert count[:n].min() > 0
    if case["maxdet"] < 1000:
        assert (count[n:] > case["maxdet"]).any()                           # max_det really cuts
    assert err_k <= max(1e-3, 2 * err_o), (err_k, err_o)


# ------------------------------------------------------------------------------------------------ ufp_backmap_merge
def _ufp_rows(chips, cw, seed, per_chip=6, ncls=3):
    """several detections inside every chip's canvas rectangle, in jittered pairs so that the merge NMS bites; sorted
    by score as a detector returns them"""
    rng = np.random.default_rng(seed)
    rows = []
    for chip in chips:
        ox, oy, w, h, nx, ny, s = [np.floor(v) for v in chip]
        for _ in range(per_chip):
            bw, bh = rng.uniform(4, max(5, w * s / 3)), rng.uniform(4, max(5, h * s / 3))
            x, y = nx + rng.uniform(0, max(1, w * s - bw)), ny + rng.uniform(0, max(1, h * s - bh))
            for jitter in range(2):
                rows.append([x + jitter, y + jitter, x + bw + jitter, y + bh + jitter, rng.uniform(0.05, 1), 0, rng.integers(0, ncls)])
    rows.append([cw * 0.9, -5, cw * 1.4, 30, 0.99, 0, 1])                # mostly outside every chip: dropped
    rows = np.asarray(rows, np.float32)
    rows[:, 5] = rows[:, 4]
    return rows[np.argsort(-rows[:, 4], kind="stable")]


def _merge(rows, chips, ncls, count=None, pad=0, **kw):
    from glsdet_amd.ufp import UfpSecondStage
    dets = torch.zeros(len(rows) + pad, 7)
    dets[: len(rows)] = torch.from_numpy(np.asarray(rows, np.float32).reshape(-1, 7))
    c = len(rows) if count is None else count
    return UfpSecondStage().merge(dets.cuda(), torch.tensor([c, c], dtype=torch.int32).cuda(), chips, ncls, **kw)


def _per_class(rows, ncls):
    return [rows[rows[:, 6] == c][:, :5] for c in range(ncls)]


@pytest.mark.parametrize("trial", [5, 6, 8, 11])
def test_ufp_merge_scenes_vs_restatement(trial):
    from tests.test_ufp import _scene
    _, chips, cw, ch = _scene(trial)
    rows = _ufp_rows(chips, cw, trial)
    assert len(np.unique(rows[:, 4])) == len(rows)                       # tie free: the oracle's order is defined
    want = U.map_back_and_merge(_per_class(rows, 3), chips, num_classes=3)
    # a count above the rows of dets is clamped to them (trial 6, 11); rows behind count are ignored (trial 5, 8)
    got = _merge(rows, chips, 3, count=len(rows) + 50, pad=0) if trial in (6, 11) else _merge(rows, chips, 3, pad=9)
    assert sum(len(w) for w in want) > 10
    for c in range(3):
        assert len(got[c]) == len(want[c]), (c, len(got[c]), len(want[c]))
        np.testing.assert_allclose(got[c], want[c], rtol=1e-5, atol=1e-3)


def test_ufp_merge_without_chips_is_empty():
    rows = np.float32([[1, 1, 20, 20, 0.9, 0.9, 0], [30, 30, 50, 50, 0.8, 0.8, 1]])
    got = _merge(rows, [], 2)
    assert [len(g) for g in got] == [0, 0] and got[0].shape == (0, 5)


def test_ufp_merge_equal_scores_the_later_entry_ranks_first():
    """canchor = -(chip * max_det + det): among equal scores the LATER entry of the reference's list is visited first
    (its `scores.argsort()[::-1]`).  a and c overlap (IoU 400/482 with '+1' areas > 0.6), all three scores are equal:
    visiting c, b, a keeps [c, b]; the opposite sign would keep [a, b]."""
    chip = [[0, 0, 100, 100, 0, 0, 1]]                                   # identity back-mapping
    a, b, c = [10, 10, 30, 30], [50, 50, 70, 70], [11, 11, 31, 31]
    rows = np.float32([a + [0.8, 0.8, 0], b + [0.8, 0.8, 0], c + [0.8, 0.8, 0], [60, 10, 80, 30, 0.8, 0.8, 1]])
    want = U.map_back_and_merge(_per_class(rows, 2), chip, num_classes=2)
    assert want[0][:, :4].tolist() == [c, b]                            # the reference's own rule (stable for short lists)
    got = _merge(rows, chip, 2)
    assert got[0][:, :4].tolist() == [c, b] and got[1][:, :4].tolist() == [[60, 10, 80, 30]]
    np.testing.assert_array_equal(got[0], want[0])
    # the same detection list under two chips (the second magnifies by 2 and maps back onto other coordinates):
    # entries of the later chip rank first among equal scores
    chips = [[0, 0, 100, 100, 0, 0, 1], [200, 200, 20, 20, 100, 0, 2]]
    rows = np.float32([a + [0.8, 0.8, 0], [104, 4, 124, 24, 0.8, 0.8, 0], c + [0.8, 0.8, 0]])
    want = U.map_back_and_merge(_per_class(rows, 1), chips, num_classes=1)
    got = _merge(rows, chips, 1)
    assert want[0][:, :4].tolist() == [[202, 202, 212, 212], c]
    np.testing.assert_array_equal(got[0], want[0])


@pytest.mark.parametrize("iof_thr,edge,inside", [(0.5, [-10, 0, 10, 10], [-9, 0, 11, 10]), (0.9, [-10, 0, 90, 10], [-9, 0, 91, 10]),
                                                 (0.25, [-30, 20, 10, 60], [-29, 20, 11, 60])])
def test_ufp_merge_iof_exactly_at_the_threshold_is_dropped(iof_thr, edge, inside):
    """integer coordinates: `edge` has exactly iof_thr of its area inside the chip's rectangle (100 / 200, 900 / 1000,
    400 / 1600: the float32 quotient is the float32 threshold) -> not mapped, the test is `>`; `inside` is one pixel
    further in -> mapped."""
    chip = [[0, 0, 100, 100, 0, 0, 1]]
    assert U.compute_iof(edge, [0, 0, 100, 100]) == iof_thr < U.compute_iof(inside, [0, 0, 100, 100])
    assert np.float32(U.compute_iof(edge, [0, 0, 100, 100])) == np.float32(iof_thr)
    for box, n_want in ((edge, 0), (inside, 1)):
        rows = np.float32([box + [0.7, 0.7, 0]])
        want = U.map_back_and_merge(_per_class(rows, 1), chip, num_classes=1, iof_thr=iof_thr)
        got = _merge(rows, chip, 1, iof_thr=iof_thr)
        assert len(want[0]) == n_want == len(got[0])
        np.testing.assert_array_equal(got[0], want[0])


def test_ufp_merge_reports_too_small_a_candidate_buffer():
    from tests.test_ufp import _scene
    _, chips, cw, ch = _scene(5)
    rows = _ufp_rows(chips, cw, 5)
    nmatch = sum(len(w) for w in U.map_back_and_merge(_per_class(rows, 3), chips, num_classes=3, nms_thr=1e9))
    assert nmatch > 16
    with pytest.raises(RuntimeError, match="max_cand"):
        _merge(rows, chips, 3, max_cand=16)
    assert sum(len(g) for g in _merge(rows, chips, 3, nms_thr=1e9, max_cand=nmatch)) == nmatch      # exactly enough


# ------------------------------------------------------------------------------------------------ yolox_decode
def _level_view(eng, x_nchw, embed):
    """fp32 NHWC level on the device.  embed: the level is a window of a wider, taller buffer (channel stride above
    5 + nc, a spatial border) whose every other element is NaN."""
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


def _decode_f64(levels, nc, in_h, in_w, strides, mode, sf):
    """the decode formula in float64 (utils_bbox.py:266-305 for mode 0, yolox_head.py:298-308 for mode 1); with
    strides = None the stride of BOTH axes is in_h / h"""
    out = []
    for l, x in enumerate(levels):
        n, c, h, w = x.shape
        p = x.double().permute(0, 2, 3, 1).reshape(n, h * w, c)[..., : 5 + nc].clone()
        s = float(strides[l]) if strides is not None else in_h / h
        gy, gx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        cx, cy = (p[..., 0] + gx.flatten()) * s, (p[..., 1] + gy.flatten()) * s
        bw, bh = torch.exp(p[..., 2]) * s, torch.exp(p[..., 3]) * s
        if mode == 0:
            p[..., 0], p[..., 1], p[..., 2], p[..., 3] = cx / in_w, cy / in_h, bw / in_w, bh / in_h
        else:
            box = torch.stack([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2], -1)
            p[..., :4] = box / sf.double()[:, None, :] if sf is not None else box
        p[..., 4:] = torch.sigmoid(p[..., 4:])
        out.append(p)
    return torch.cat(out, 1)


DECODE_CASES = [
    dict(id="mode0_3lv_nonsquare_nostrides", mode=0, sizes=[(12, 16), (6, 8), (3, 4)], hw=(96, 160), strides=None, nc=10, embed=False, sf=False),
    dict(id="mode1_3lv_nonsquare_nostrides_sf", mode=1, sizes=[(12, 16), (6, 8), (3, 4)], hw=(96, 160), strides=None, nc=3, embed=True, sf=True),
    dict(id="mode0_1lv_strides_embedded", mode=0, sizes=[(7, 9)], hw=(56, 72), strides=[8], nc=1, embed=True, sf=False),
    dict(id="mode1_1lv_strides", mode=1, sizes=[(5, 13)], hw=(80, 208), strides=[16], nc=80, embed=False, sf=False),
    dict(id="mode0_8lv_strides", mode=0, sizes=[(17, 23), (9, 12), (9, 12), (5, 6), (3, 3), (2, 2), (1, 3), (1, 1)], hw=(136, 184),
         strides=[8, 16, 16, 32, 48, 64, 96, 128], nc=4, embed=True, sf=False),
    dict(id="mode1_8lv_nostrides_sf", mode=1, sizes=[(17, 23), (9, 12), (9, 12), (5, 6), (3, 3), (2, 2), (1, 3), (1, 1)], hw=(136, 184),
         strides=None, nc=2, embed=False, sf=True),
]


@pytest.mark.parametrize("case", DECODE_CASES, ids=[c["id"] for c in DECODE_CASES])
def test_yolox_decode_vs_float64_formula(engines, case):
    """both modes; 1, 3 and 8 levels; strides = None on a non-square input whose level grids are NOT in_w / w wide
    (pins stride = in_h / h for both axes); explicit strides; scale_factors; level views with a channel stride above
    5 + nc inside NaN-filled buffers; size logits up to +-20.  Bound: the existing test's 1e-5 on |x| + 1."""
    eng = engines["f32"]
    n, nc = 3, case["nc"]
    g = torch.Generator().manual_seed(len(case["id"]))
    xs = []
    for h, w in case["sizes"]:
        x = torch.randn(n, 5 + nc, h, w, generator=g) * 2.0
        x[:, 2:4] = torch.rand(n, 2, h, w, generator=g) * 40.0 - 20.0       # exp over the whole +-20 range
        x[0, 2, 0, 0], x[0, 3, 0, 0] = 20.0, -20.0
        x[0, 4, 0, 0], x[0, 5, 0, 0], x[1, 4, 0, 0], x[1, 5, 0, 0] = 20.0, -20.0, 40.0, -40.0       # saturated sigmoid
        xs.append(x)
    sf = (torch.rand(n, 4, generator=g) + 0.5) if case["sf"] else None
    in_h, in_w = case["hw"]
    if case["strides"] is None:
        assert any(in_h / h != in_w / w for h, w in case["sizes"])
    got = eng.decode([_level_view(eng, x, case["embed"]) for x in xs], nc, in_h, in_w, strides=case["strides"], mode=case["mode"],
                     scale_factors=sf.cuda().contiguous() if sf is not None else None)
    torch.cuda.synchronize()
    want = _decode_f64(xs, nc, in_h, in_w, case["strides"], case["mode"], sf)
    got = got.cpu().double()
    assert got.shape == want.shape == (n, sum(h * w for h, w in case["sizes"]), 5 + nc)
    assert bool(torch.isfinite(got).all())
    err = float(((got - want).abs() / (want.abs() + 1.0)).max())
    print("decode %s: max |err| / (|x| + 1) = %.3e" % (case["id"], err))
    assert err <= 1e-5


# ------------------------------------------------------------------------------------------------ pack_detections
@pytest.mark.parametrize("cap", [5, 12, 20], ids=["cap_below_max_det", "cap_equal_max_det", "cap_above_max_det"])
def test_pack_detections_equals_the_documented_record(engines, cap):
    """out[img][0 .. cap) = the first min(count, max_det, cap) rows, zero rows behind them; out[img][cap] = (rows kept
    here, count before max_det, 0 ...) -- the format documented above pack_dets_kernel, restated in numpy.  Counts: 0,
    below cap, equal to cap, above cap, above max_det."""
    eng = engines["f32"]
    max_det = 12
    kept = [0, 3, cap, min(cap + 2, max_det), max_det + 7, 1]         # (a count above max_det is clamped to it)
    total = [0, 3, cap + 30, 40, 5000, 1]
    n = len(kept)
    rng = np.random.default_rng(cap)
    dets = rng.uniform(-5, 700, (n, max_det, 7)).astype(np.float32)      # rows behind count hold stale values
    nb = dict(dets=torch.from_numpy(dets).cuda(), count=torch.tensor(kept + total, dtype=torch.int32).cuda(), max_det=max_det)
    got = eng.pack_detections(nb, cap)
    got.fill_(float("nan"))                                              # every float of the record must be written
    got = eng.pack_detections(nb, cap)
    torch.cuda.synchronize()
    want = np.zeros((n, cap + 1, 7), np.float32)
    for i in range(n):
        k = min(kept[i], max_det, cap)
        want[i, :k] = dets[i, :k]
        want[i, cap, 0], want[i, cap, 1] = k, total[i]
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
