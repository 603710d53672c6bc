"""Records tests/golden/vocap_golden.npz: what the reference's own `get_map` (models/core/utils_map.py of the drone
checkout) computes and writes on small scenes, at the overlap thresholds 0.5 and 0.75.

    python tools/make_vocap_golden.py <reference checkout>/yolox-drone             # record the fixture
    python tools/make_vocap_golden.py <reference checkout>/yolox-drone --check N   # N seeded scenes, nothing written

The reference file is loaded by path.  Only plotting is stubbed: `cv2` and `matplotlib.pyplot` in sys.modules (the file
imports both at its top) and the module attribute `draw_plot_func`.  `voc_ap` and `log_average_miss_rate` are WRAPPED, not
replaced: the wrappers copy the arguments, call the original and record what it returns.  `get_map(thr, True, path)` is
the reference's own call (with draw_plot=False it never creates results/ and fails on results.txt).

Per scene the fixture holds the input file texts and, per threshold, results.txt as bytes, the printed lines and per class
rec / prec / ap / mrec / mpre / lamr / mr / fppi (per-class arrays concatenated in class order, `n_det` gives the split).
Only data goes into the fixture.  The hand-built scenes cover what tests/test_vocap_reference.py lists; every planted
mistake of tests/voc_reference.py must change one of them (asserted here), and so must the restatement agree with
every record (asserted here, too).  --check runs seeded scenes through the reference and the restatement and reports the
mismatches."""
import contextlib
import importlib.util
import io
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import voc_reference as R                            # noqa: E402

THRESHOLDS = (0.5, 0.75)


class _Absorb:
    def __getattr__(self, name):
        return self

    def __call__(self, *a, **k):
        return self


def load_reference(checkout):
    path = os.path.join(checkout, "models", "core", "utils_map.py")
    sys.modules["cv2"] = types.ModuleType("cv2")
    try:
        import matplotlib  # noqa: F401
    except ImportError:
        sys.modules["matplotlib"] = types.ModuleType("matplotlib")
    plt = types.ModuleType("matplotlib.pyplot")
    plt.__getattr__ = lambda name: _Absorb()
    sys.modules["matplotlib.pyplot"] = plt
    spec = importlib.util.spec_from_file_location("reference_utils_map", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.draw_plot_func = lambda *a, **k: None
    calls = {"voc_ap": [], "lamr": []}
    orig_ap, orig_lamr = mod.voc_ap, mod.log_average_miss_rate

    def voc_ap(rec, prec):
        args = (list(rec), list(prec))
        out = orig_ap(rec, prec)
        calls["voc_ap"].append((args, (out[0], list(out[1]), list(out[2]))))
        return out

    def log_average_miss_rate(precision, fp_cumsum, num_images):
        args = (np.array(precision, copy=True), np.array(fp_cumsum, copy=True), num_images)
        out = orig_lamr(precision, fp_cumsum, num_images)
        calls["lamr"].append((args, out))
        return out
    mod.voc_ap, mod.log_average_miss_rate = voc_ap, log_average_miss_rate
    return mod, calls


def run_reference(mod, calls, gt_texts, dr_texts, thr):
    with tempfile.TemporaryDirectory() as tmp:
        for sub, texts in (("ground-truth", gt_texts), ("detection-results", dr_texts)):
            os.makedirs(os.path.join(tmp, sub))
            for fid, text in texts.items():
                with open(os.path.join(tmp, sub, fid + ".txt"), "w") as f:
                    f.write(text)
        calls["voc_ap"].clear()
        calls["lamr"].clear()
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            mod.get_map(thr, True, path=tmp)
        with open(os.path.join(tmp, "results", "results.txt"), "rb") as f:
            results = f.read()
    rec = {"results": results, "printed": buf.getvalue().splitlines(), "classes": []}
    for k in ("rec", "prec", "ap", "mrec", "mpre", "lamr", "mr", "fppi", "n_det"):
        rec[k] = []
    for ((r, p), (ap, mrec, mpre)), ((_, _, _), (lamr, mr, fppi)) in zip(calls["voc_ap"], calls["lamr"]):
        rec["n_det"].append(len(r))
        rec["rec"].append([float(x) for x in r])
        rec["prec"].append([float(x) for x in p])
        rec["ap"].append(float(ap))
        rec["mrec"].append([float(x) for x in mrec])
        rec["mpre"].append([float(x) for x in mpre])
        rec["lamr"].append(float(lamr))
        rec["mr"].append([float(x) for x in mr] if len(r) else [])       # the reference returns the scalars 1 / 0
        rec["fppi"].append([float(x) for x in fppi] if len(r) else [])   # for a class without detections
    assert len(calls["voc_ap"]) == len(calls["lamr"])
    return rec


def restate(gt_texts, dr_texts, thr, mistakes=()):
    ev = R.evaluate(gt_texts, dr_texts, thr, mistakes)
    text, printed = R.results_text(ev)
    rec = {"results": text.encode(), "printed": printed}
    for k in ("rec", "prec", "ap", "mrec", "mpre", "lamr", "mr", "fppi", "n_det"):
        rec[k] = [ev["per_class"][c][k] for c in ev["classes"]]
    rec["lamr"] = [float(x) for x in rec["lamr"]]
    return rec


def differences(want, got, lamr_rtol=1e-12):
    bad = [k for k in ("results", "printed", "rec", "prec", "ap", "mrec", "mpre", "mr", "fppi", "n_det") if want[k] != got[k]]
    if len(want["lamr"]) != len(got["lamr"]) or any(abs(a - b) > lamr_rtol * abs(a) for a, b in zip(want["lamr"], got["lamr"])):
        bad.append("lamr")
    return bad


def ulp_below_half():
    """bottom edge y of a detection 0 0 9 y whose overlap with the ground truth 0 0 9 9 is the double just below 0.5"""
    want = float(np.nextafter(0.5, 0.0))
    y = 4.0
    for _ in range(4096):
        y = float(np.nextafter(y, 0.0))
        ov = R.overlap([0.0, 0.0, 9.0, y], [0.0, 0.0, 9.0, 9.0])
        if ov == want:
            return y
        assert ov >= want, "stepped over the double below 0.5"
    raise AssertionError("no bottom edge gives the double below 0.5")


def hand_scenes():
    y = ulp_below_half()
    s = {}
    # IoU exactly on the threshold (50 / 100), then a repeated match on the same ground truth; recall is 1.0 before the end
    s["on_threshold_and_repeat"] = ({"a": "car 0 0 9 9\n"}, {"a": "car 0.9 0 0 9 4\ncar 0.8 0 0 9 4\ncar 0.3 0 0 9 9\n"})
    s["one_ulp_below"] = ({"a": "car 0 0 9 9\n"}, {"a": "car 0.9 0 0 9 %s\n" % repr(y)})
    # two ground truths of equal IoU: the first (regular) one wins, the second detection meets it used
    s["tie_first_wins"] = ({"a": "car 0 0 9 9\ncar 0 0 9 9 difficult\n"}, {"a": "car 0.9 0 0 9 9\ncar 0.8 0 0 9 9\n"})
    # touching boxes overlap by one pixel (image a), boxes one pixel apart do not overlap at all (image b)
    s["plus_one_rule"] = ({"a": "car 10 0 19 9\n", "b": "car 11 0 20 9\n"},
                          {"a": "car 0.9 0 0 10 9\n", "b": "car 0.9 0 0 10 9\ncar 0.6 11 0 20 9\n"})
    # matches on a difficult ground truth score neither way, twice; a difficult-only class (bus) is no class at all,
    # its detections count in the last block only; all scores above 0.5
    s["difficult"] = ({"a": "car 0 0 9 9 difficult\ncar 20 20 29 29\nbus 0 0 5 5 difficult\n"},
                      {"a": "car 0.9 0 0 9 9\ncar 0.8 0 0 9 9\ncar 0.7 20 20 29 29\ncar 0.6 50 50 59 59\nbus 0.95 0 0 5 5\n"})
    # equal scores across files keep file order; no score above 0.5 (0.5 itself is not); van: recall never changes
    s["equal_scores"] = ({"a": "car 0 0 9 9\nvan 40 40 49 49\n", "b": "car 0 0 9 9\n"},
                         {"a": "car 0.5 30 30 39 39\nvan 0.5 0 0 9 9\nvan 0.4 1 1 8 8\n", "b": "car 0.5 0 0 9 9\n"})
    # an empty detection file, a class with ground truths and no detections (person), a class only in detections (dog)
    s["empty_and_missing"] = ({"a": "car 0 0 9 9\nperson 1 1 5 5\n", "b": "car 0 0 9 9\n"},
                              {"a": "", "b": "car 0.7 0 0 9 9\ndog 0.9 1 1 5 5\n"})
    # person lives in one image of three: n_img = 1 moves the picked miss rates; false positive first, then the match
    s["n_img_of_class"] = ({"a": "person 0 0 9 9\ncar 30 30 39 39\n", "b": "car 0 0 9 9\n", "c": "car 5 5 20 20\n"},
                           {"a": "person 0.9 40 40 49 49\nperson 0.8 0 0 9 9\n", "b": "car 0.9 0 0 9 9\n",
                            "c": "car 0.95 5 5 20 20\ncar 0.2 40 40 50 50\n"})
    # a class name with a blank, non-integer coordinates
    s["blank_in_name"] = ({"a": "traffic light 0 0 9 9\ntraffic light 20.5 20.25 29.75 29.5\ncar 1 1 2 2\n"},
                          {"a": "traffic light 0.9 0 0 9 9\ntraffic light 0.85 20.25 20.5 29.5 29.75\n"
                                "traffic light 0.55 0.5 0.25 9.75 9.5\ncar 0.1 1 1 2 2\n"})
    # thirds and sevenths: products that round, so a fused sum over all indices differs
    gt = "".join("car %d 0 %d 9\n" % (12 * k, 12 * k + 9) for k in range(7))
    dr = "".join("car %s %d 0 %d %d\n" % (repr(round(0.95 - 0.06 * k, 2)), 12 * (k % 7), 12 * (k % 7) + 9, 9 if k % 3 != 1 else 2)
                 for k in range(13))
    s["sevenths"] = ({"a": gt}, {"a": dr})
    return s


def main():
    if len(sys.argv) < 2:
        raise SystemExit(__doc__)
    mod, calls = load_reference(sys.argv[1])
    if "--check" in sys.argv:
        n = int(sys.argv[sys.argv.index("--check") + 1])
        bad = 0
        for seed in range(1000, 1000 + n):
            gt_texts, dr_texts = R.random_scene(seed)
            for thr in THRESHOLDS:
                d = differences(run_reference(mod, calls, gt_texts, dr_texts, thr), restate(gt_texts, dr_texts, thr))
                if d:
                    bad += 1
                    print("seed %d thr %g: %s differ" % (seed, thr, d))
        print("--check: %d seeded scenes x %d thresholds, %d mismatches" % (n, len(THRESHOLDS), bad))
        raise SystemExit(1 if bad else 0)

    scenes = hand_scenes()
    for seed in range(8):
        scenes["seed_%d" % seed] = R.random_scene(seed)
    out = {"names": np.array(list(scenes)), "thresholds": np.array(THRESHOLDS)}
    records = {}
    for name, (gt_texts, dr_texts) in scenes.items():
        ids = sorted(gt_texts)
        out[name + "/ids"] = np.array(ids)
        out[name + "/gt"] = np.array([gt_texts[i] for i in ids])
        out[name + "/dr"] = np.array([dr_texts[i] for i in ids])
        for thr in THRESHOLDS:
            rec = run_reference(mod, calls, gt_texts, dr_texts, thr)
            records[name, thr] = rec
            d = differences(rec, restate(gt_texts, dr_texts, thr))
            assert not d, (name, thr, d)
            p = "%s/%g/" % (name, thr)
            out[p + "results"] = np.frombuffer(rec["results"], dtype=np.uint8)
            out[p + "printed"] = np.array(rec["printed"])
            out[p + "n_det"] = np.array(rec["n_det"], dtype=np.int64)
            for k in ("ap", "lamr"):
                out[p + k] = np.array(rec[k], dtype=np.float64)
            for k in ("rec", "prec", "mrec", "mpre", "mr", "fppi"):
                out[p + k] = np.array([x for row in rec[k] for x in row], dtype=np.float64)
    for mistake in R.MISTAKES:
        seen = [n for (n, thr), rec in records.items() if differences(rec, restate(*scenes[n], thr, mistakes=(mistake,)))]
        assert seen, "no committed scene sees the planted mistake " + mistake
        print("%-22s seen by %s" % (mistake, sorted(set(seen))))
    path = os.path.join(ROOT, "tests", "golden", "vocap_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d scenes, %d bytes" % (path, len(scenes), os.path.getsize(path)))


if __name__ == "__main__":
    main()
