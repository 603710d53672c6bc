"""Records tests/golden/ufp_pack_golden.npz: float32 edge scenes of unified foreground packing and what the reference's
own UnifiedForegroundPacking (ufp/UFPMP-Det-Tools/ufp, pure numpy, imported at generation time only) returns for them.

    python tools/make_ufp_pack_golden.py <reference checkout>/ufp/UFPMP-Det-Tools

A scene is (boxes float32 [n,4] xyxy, labels int64 [n], both in the detector's output order; expand; image W, H); the
reference is called on the class-major rows, as the two-stage driver calls the packer.  Hand-built scenes come first;
scenes that need a property no hand can set (a fill class, a contraction-sensitive pair, a last probe that is
infeasible) are found by a seeded search with tests/ufp_pack_reference.py and asserted here.  The tests read only the
.npz: tests/test_ufp_pack_reference.py pins the restatement to it, tests/test_ufp_pack_fuzz.py the kernel."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import ufp_pack_reference as R                       # noqa: E402

F = np.float32
BIG = (4000, 3000)


def scene(boxes, labels=None, expand=1.0, wh=BIG):
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    lab = np.zeros(len(b), np.int64) if labels is None else np.asarray(labels, np.int64)
    assert len(lab) == len(b)
    return b, lab, float(expand), int(wh[0]), int(wh[1])


def run(sc, mistakes=(), trace=None):
    return R.ufp_pack(sc[0], sc[1], sc[2], sc[3], sc[4], mistakes, trace)


def same(a, b):
    ca, cb = np.asarray(a[0], np.float64).reshape(-1, 7), np.asarray(b[0], np.float64).reshape(-1, 7)
    return ca.shape == cb.shape and np.array_equal(ca.view(np.int64), cb.view(np.int64)) and float(a[1]) == float(b[1]) \
        and float(a[2]) == float(b[2])


def grid_scene(rng, n, sizes_w, sizes_h):
    """n boxes of sizes drawn from small sets, one per cell of a sparse grid (no merges at expand 1), magnification 1"""
    cells = rng.permutation(48)[:n]
    b = []
    for c in cells:
        x0, y0 = 40.0 + 480.0 * (c % 8), 40.0 + 480.0 * (c // 8)
        w, h = float(rng.choice(sizes_w)), float(rng.choice(sizes_h))
        b.append([x0, y0, x0 + w, y0 + h])
    return scene(b)


def search(pred, make, tries=20000):
    for t in range(tries):
        sc = make(np.random.default_rng([t, 0x5EA]))
        if pred(sc):
            return sc, t
    raise SystemExit("no scene found")


def hand_scenes():
    s = {}
    s["n0"] = scene(np.zeros((0, 4)))
    s["n1"] = scene([[100, 100, 164, 228]], expand=1.5)
    s["n2"] = scene([[100, 100, 164, 228], [900, 700, 1100, 820]], [1, 0], expand=1.5)
    # union 128 x 64 = 4096 + 4096: equal, not smaller -> two regions
    s["edge_share_dyadic"] = scene([[64, 64, 128, 128], [128, 64, 192, 128]])
    # A + B merge (200 x 100 < 10000 + 11000); C fits the grown region only (300 x 100 < 20000 + 10500, but > 10000 + 10500)
    A, B, C = [0, 0, 100, 100], [90, 0, 200, 100], [195, 0, 300, 100]
    # (a far box in between keeps the region order apart from that of a row C that swallows A + B later)
    s["chain_after_growth"] = scene([A, B, [2000, 2000, 2100, 2100], C])
    # C comes BEFORE the hit: row A must not go back to it; row C then swallows the earlier, grown A
    s["before_first_hit"] = scene([A, C, B])
    s["swallow_earlier"] = scene([[500, 500, 640, 640], A, [2000, 2000, 2100, 2100], C, B], [0, 0, 1, 1, 1])
    # mean object area at the magnification thresholds: (x2-x1+1) * (y2-y1+1)
    s["area_1024"] = scene([[0, 0, 31, 31]])
    s["area_1024_minus_ulp"] = scene([[0, 0, 31.0 - 2.0 ** -19, 31]])
    s["area_9216"] = scene([[0, 0, 95, 95]])
    s["area_9216_minus_ulp"] = scene([[0, 0, 95.0 - 2.0 ** -17, 95]])
    s["three_box_region"] = scene([[100, 100, 130, 130], [110, 105, 141, 138], [95, 112, 130, 144]], expand=1.5)
    s["clipped_borders"] = scene([[2, 200, 40, 260], [600, 100, 639, 180], [300, 1, 380, 30], [200, 440, 290, 479],
                                  [0, 0, 30, 25], [610, 450, 639, 479]], [0, 1, 2, 3, 0, 1], expand=1.5, wh=(640, 480))
    s["equal_heights"] = scene([[40, 40, 140, 160], [600, 40, 750, 160], [1200, 40, 1330, 160], [1800, 40, 1910, 160]])
    s["equal_sizes_2_3"] = scene([[40, 40, 168, 168], [600, 40, 700, 180], [1200, 40, 1328, 168], [1800, 40, 1900, 180],
                                  [2400, 40, 2500, 180], [40, 600, 260, 790]])
    # 1401 x 6 = 8406 < 9216 -> magnification 2 -> 2800 wide, beyond the widest strip
    s["wider_than_2666"] = scene([[100, 100, 1500, 105], [200, 600, 330, 720], [900, 900, 960, 1000]])
    rng = np.random.default_rng(77)
    c = rng.uniform(0.2, 0.8, (12, 2)) * [900, 600]
    wh = np.exp(rng.uniform(np.log(10), np.log(150), (12, 2)))
    s["interleaved_labels"] = scene(np.concatenate([c - wh / 2, c + wh / 2], 1), [9, 2, 7, 2, 0, 9, 5, 0, 7, 2, 5, 9], 1.5, (900, 600))
    for n in (63, 64, 65, 127, 128, 129):
        s["boxes_%d" % n] = R.random_scene(1000 + n, n=n)
    return s


def searched_scenes():
    s = {}

    def pair(rng):
        x = np.sort(rng.uniform(10, 500, 3)).astype(np.float32)
        y = np.sort(rng.uniform(10, 400, 2)).astype(np.float32)
        return scene([[x[0], y[0], x[1], y[1]], [x[1], y[0], x[2], y[1]]])
    s["edge_share_contraction"], t = search(lambda sc: not same(run(sc), run(sc, ("fused_both",))), pair)
    print("contraction-sensitive edge-sharing pair after %d tries" % (t + 1))

    def small(rng):
        return grid_scene(rng, int(rng.integers(3, 7)), (100, 200, 300), (100, 200, 300))

    def real(rng):
        n = int(rng.integers(3, 8))
        return grid_scene(rng, n, rng.uniform(100, 400, 4).astype(np.float32), rng.uniform(100, 400, 4).astype(np.float32))
    def rich(rng):                                   # a narrow tall pick beside small squares: class 4, third and fourth branch
        return grid_scene(rng, int(rng.integers(3, 7)), (50, 100, 200, 300, 1000), (100, 200, 300, 400))
    for key, make in (("rank1", small), ("rank2", small), ("rank3", small), ("rank4a", real), ("rank4b", real),
                      ("rank4c", rich), ("rank4d", rich)):
        def has(sc, key=key):
            tr = {}
            run(sc, trace=tr)
            return tr.get(key, 0) > 0
        s["fill_" + key], t = search(has, make)
        print("fill %s after %d tries" % (key, t + 1))

    def infeasible(sc):
        tr = {}
        run(sc, trace=tr)
        return tr["last_infeasible"] and not same(run(sc), run(sc, ("best_feasible_probe",)))
    s["last_probe_infeasible"], t = search(infeasible, lambda rng: R.random_scene(int(rng.integers(1 << 30)), max_n=12))
    print("infeasible last probe after %d tries" % (t + 1))
    return s


def main(ref_root):
    sys.path.insert(0, ref_root)
    from ufp import UnifiedForegroundPacking
    scenes = hand_scenes()
    scenes.update(searched_scenes())
    # every planted mistake must show on a committed scene: add a searched one where the hand-built ones are blind
    for mk in R.MISTAKES:
        if not any(not same(run(sc), run(sc, (mk,))) for sc in scenes.values() if len(sc[0]) <= 12):
            scenes["shows_" + mk], t = search(lambda sc, mk=mk: not same(run(sc), run(sc, (mk,))),
                                              lambda rng: R.random_scene(int(rng.integers(1 << 30)), max_n=10,
                                                                         integer=bool(rng.integers(2))))
            print("mistake %s: searched scene after %d tries" % (mk, t + 1))
    # properties the hand-built scenes claim
    assert len(run(scenes["edge_share_dyadic"])[0]) == 2 and len(run(scenes["chain_after_growth"])[0]) == 2
    assert [c[6] for c in run(scenes["area_1024"])[0]] == [2.0] and [c[6] for c in run(scenes["area_1024_minus_ulp"])[0]] == [4.0]
    assert [c[6] for c in run(scenes["area_9216"])[0]] == [1.0] and [c[6] for c in run(scenes["area_9216_minus_ulp"])[0]] == [2.0]
    b = scenes["area_1024_minus_ulp"][0][0]
    assert F(F(F(b[2] - b[0]) + F(1)) * F(F(b[3] - b[1]) + F(1))) == np.nextafter(F(1024), F(0))
    b = scenes["area_9216_minus_ulp"][0][0]
    assert F(F(F(b[2] - b[0]) + F(1)) * F(F(b[3] - b[1]) + F(1))) == np.nextafter(F(9216), F(0))
    assert max(c[2] * c[6] for c in run(scenes["wider_than_2666"])[0]) > 2666
    data = {"names": np.array(sorted(scenes)), "numpy_version": np.array(np.__version__)}
    for name, sc in scenes.items():
        boxes, labels, expand, W, H = sc
        order = np.argsort(labels, kind="stable")
        chips, cw, ch = UnifiedForegroundPacking(boxes[order].copy(), expand, [W, H])
        assert same((chips, cw, ch), run(sc)), name
        data[name + "/boxes"], data[name + "/labels"] = boxes, labels
        data[name + "/params"] = np.array([expand, W, H], np.float64)
        data[name + "/chips"] = np.asarray(chips, np.float64).reshape(-1, 7)
        data[name + "/canvas"] = np.asarray([cw, ch], np.float64)
    out = os.path.join(ROOT, "tests", "golden", "ufp_pack_golden.npz")
    np.savez_compressed(out, **data)
    print("wrote %s: %d scenes, %d bytes, numpy %s" % (out, len(scenes), os.path.getsize(out), np.__version__))


if __name__ == "__main__":
    main(sys.argv[1])
