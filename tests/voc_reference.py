"""A deliberately naive restatement of VOC-style mAP as the drone harness computes it (get_map of
drone/models/core/utils_map.py:294-813 with voc_ap :99-140 and log_average_miss_rate :26-62; the contract of
glsdet_voc_ap in include/glsdet_hip.h): plain Python floats, lists and dicts, one detection and one ground truth at a
time, no files inside the matching.  Only the log-average miss rate's exp(mean(log(.))) goes through numpy, as in the
reference.

A scene is a pair of dicts {file id: text}: the ground-truth files and the detection-result files.  Class names that
contain the word `difficult` are out of scope (the reference tests `"difficult" in line` on the whole line).

`mistakes` plants one wrong reading each; tests/test_vocap_reference.py demands that every one of them changes a
committed scene."""
import math

import numpy as np

MISTAKES = ("tie_ge", "thr_gt", "no_plus1", "difficult_fp", "difficult_used", "unstable_sort", "ascending_sort",
            "score_ge", "n_img_all", "ap_all_fma", "suffix_short", "map_over_det_classes")


CLASS_NAMES = ("car", "person", "traffic light", "van")


def _num(v):
    return "%d" % v if float(v) == int(v) else repr(float(v))


def random_scene(seed, max_images=12, max_classes=4, max_gt=12, max_det=28):
    """A seeded scene of 1 .. 12 images, 1 .. 4 classes and 0 .. 40 boxes per image -> (gt_texts, dr_texts).  Boxes sit on
    a 64-pixel canvas so that overlaps, repeated matches and equal IoUs are common; half of the detections are jittered
    copies of ground truths (a quarter of them on quarter-pixel coordinates), scores come in steps of 0.05 so that equal
    scores across files are common; the first image always holds a non-difficult ground truth."""
    rng = np.random.default_rng(seed)
    n_img = int(rng.integers(1, max_images + 1))
    names = CLASS_NAMES[:int(rng.integers(1, max_classes + 1))]
    gt_texts, dr_texts = {}, {}
    for i in range(n_img):
        fid = "img_%03d" % int(rng.integers(0, 1000)) + "_%d" % i
        gts, lines = [], []
        for g in range(int(rng.integers(0 if i else 1, max_gt + 1))):
            x, y = int(rng.integers(0, 48)), int(rng.integers(0, 48))
            w, h = int(rng.integers(8, 24)), int(rng.integers(8, 24))     # stays a box under a jitter of 3 per side
            name = names[int(rng.integers(0, len(names)))]
            difficult = bool(rng.random() < 0.15) and not (i == 0 and g == 0)
            gts.append((name, x, y, x + w, y + h))
            lines.append("%s %d %d %d %d%s" % (name, x, y, x + w, y + h, " difficult" if difficult else ""))
        gt_texts[fid] = "\n".join(lines) + ("\n" if lines else "")
        lines = []
        for d in range(int(rng.integers(0, max_det + 1))):
            if gts and rng.random() < 0.5:
                name, x0, y0, x1, y1 = gts[int(rng.integers(0, len(gts)))]
                step = 0.25 if rng.random() < 0.25 else 1.0
                box = [v + step * int(rng.integers(-3, 4)) for v in (x0, y0, x1, y1)]
                if rng.random() < 0.3:
                    box = [x0, y0, x1, y1]
            else:
                name = names[int(rng.integers(0, len(names)))]
                x, y = int(rng.integers(0, 48)), int(rng.integers(0, 48))
                box = [x, y, x + int(rng.integers(3, 24)), y + int(rng.integers(3, 24))]
            score = 0.05 * int(rng.integers(1, 20)) if rng.random() < 0.7 else float(rng.random())
            lines.append("%s %s %s" % (name, repr(round(score, 4)), " ".join(_num(v) for v in box)))
        dr_texts[fid] = "\n".join(lines) + ("\n" if lines else "")
    return gt_texts, dr_texts


def load_golden():
    """tests/golden/vocap_golden.npz -> (the archive, {scene name: (gt_texts, dr_texts)})"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocap_golden.npz"))
    scenes = {}
    for name in g["names"].tolist():
        ids = g[name + "/ids"].tolist()
        scenes[name] = (dict(zip(ids, g[name + "/gt"].tolist())), dict(zip(ids, g[name + "/dr"].tolist())))
    return g, scenes


def parse_gt_line(line):
    """-> (class name, [l, t, r, b] floats, difficult): everything before the last 4 (5 when difficult) fields is the name"""
    f = line.split()
    if "difficult" in line:
        return " ".join(f[:-5]), [float(x) for x in f[-5:-1]], True
    return " ".join(f[:-4]), [float(x) for x in f[-4:]], False


def parse_dr_line(line):
    """-> (class name, float(confidence), [l, t, r, b] floats)"""
    f = line.split()
    return " ".join(f[:-5]), float(f[-5]), [float(x) for x in f[-4:]]


def lines_of(text):
    return [x.strip() for x in text.splitlines()]


def parse_scene(gt_texts, dr_texts):
    """-> (ids in sorted-file order, {id: [(class, box, difficult)]}, {id: [(class, score, box)]}, {first token: lines})"""
    if not gt_texts:
        raise FileNotFoundError("no ground-truth files")
    for i in gt_texts:
        if i not in dr_texts:
            raise FileNotFoundError("detection-results/%s.txt" % i)
    for i in dr_texts:
        if i not in gt_texts:
            raise FileNotFoundError("ground-truth/%s.txt" % i)
    ids = sorted(gt_texts, key=lambda i: i + ".txt")
    gts = {i: [parse_gt_line(l) for l in lines_of(gt_texts[i])] for i in ids}
    drs = {i: [parse_dr_line(l) for l in lines_of(dr_texts[i])] for i in ids}
    det_counter = {}                      # :682-690 counts by the FIRST token of the line
    for i in ids:
        for l in lines_of(dr_texts[i]):
            k = l.split()[0]
            det_counter[k] = det_counter.get(k, 0) + 1
    return ids, gts, drs, det_counter


def _fma(a, b, c):
    """a*b + c with one rounding (only the planted mistake `ap_all_fma` uses it)"""
    from fractions import Fraction
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def voc_ap(rec, prec, mistakes=()):
    mrec = [0.0] + list(rec) + [1.0]
    mpre = [0.0] + list(prec) + [0.0]
    # the planted short start skips the last precision itself (one further back the skipped step is max(x, 0): no change)
    start = len(mpre) - (4 if "suffix_short" in mistakes else 2)
    for i in range(start, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    if "ap_all_fma" in mistakes:
        for i in range(1, len(mrec)):
            ap = _fma(mrec[i] - mrec[i - 1], mpre[i], ap)
        return ap, mrec, mpre
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return ap, mrec, mpre


def miss_rates(rec, fp, n_images):
    """log_average_miss_rate :26-62 on (rec, cumulative fp, n_images) -- the reference hands `rec` to the parameter it
    calls `precision` (:617).  -> lamr, mr list, fppi list, the nine picked miss rates"""
    if len(rec) == 0:
        return 0, [], [], [1.0] * 9
    fppi = [float(f) / float(n_images) for f in fp]
    mr = [1 - r for r in rec]
    fppi_tmp = [-1.0] + fppi
    mr_tmp = [1.0] + mr
    ref = [float(x) for x in np.logspace(-2.0, 0.0, num=9)]
    picked = []
    for r in ref:
        j = 0
        for k, v in enumerate(fppi_tmp):
            if v <= r:
                j = k
        picked.append(mr_tmp[j])
    lamr = math.exp(np.mean(np.log(np.maximum(1e-10, np.array(picked)))))
    return lamr, mr, fppi, picked


def overlap(bb, bbgt, mistakes=()):
    """-> ov, or None when the boxes do not overlap by the +1 rule"""
    one = 0 if "no_plus1" in mistakes else 1
    bi = [max(bb[0], bbgt[0]), max(bb[1], bbgt[1]), min(bb[2], bbgt[2]), min(bb[3], bbgt[3])]
    iw = bi[2] - bi[0] + one
    ih = bi[3] - bi[1] + one
    if iw > 0 and ih > 0:
        ua = (bb[2] - bb[0] + one) * (bb[3] - bb[1] + one) + (bbgt[2] - bbgt[0] + one) * (bbgt[3] - bbgt[1] + one) - iw * ih
        return iw * ih / ua
    return None


def evaluate(gt_texts, dr_texts, min_overlap, mistakes=()):
    ids, gts, drs, det_counter = parse_scene(gt_texts, dr_texts)
    gt_counter, img_counter = {}, {}
    for i in ids:
        seen = []
        for name, _, difficult in gts[i]:
            if difficult:
                continue
            gt_counter[name] = gt_counter.get(name, 0) + 1
            if name not in seen:
                img_counter[name] = img_counter.get(name, 0) + 1
                seen.append(name)
    gt_classes = sorted(gt_counter)
    out = {"classes": gt_classes, "per_class": {}, "gt_counter": gt_counter, "det_counter": det_counter}
    sum_ap = 0.0
    for name in gt_classes:
        dets = [(s, i, b) for i in ids for (n, s, b) in drs[i] if n == name]
        if "ascending_sort" in mistakes:
            dets.sort(key=lambda d: d[0])
        elif "unstable_sort" in mistakes:
            dets = dets[::-1]
            dets.sort(key=lambda d: d[0], reverse=True)          # equal scores end up in reversed order
        else:
            dets.sort(key=lambda d: d[0], reverse=True)
        used = {i: [False] * len(gts[i]) for i in ids}
        nd = len(dets)
        tp, fp, score = [0] * nd, [0] * nd, [0.0] * nd
        score05_idx = 0
        for idx, (s, i, bb) in enumerate(dets):
            score[idx] = s
            if (s >= 0.5) if "score_ge" in mistakes else (s > 0.5):
                score05_idx = idx
            ovmax, match = -1, -1
            for g, (gname, bbgt, difficult) in enumerate(gts[i]):
                if gname != name:
                    continue
                ov = overlap(bb, bbgt, mistakes)
                if ov is None:
                    continue
                if (ov >= ovmax) if "tie_ge" in mistakes else (ov > ovmax):
                    ovmax, match = ov, g
            if (ovmax > min_overlap) if "thr_gt" in mistakes else (ovmax >= min_overlap):
                if gts[i][match][2]:
                    if "difficult_fp" in mistakes:
                        fp[idx] = 1
                    elif "difficult_used" in mistakes:
                        if used[i][match]:
                            fp[idx] = 1
                        used[i][match] = True
                elif not used[i][match]:
                    tp[idx] = 1
                    used[i][match] = True
                else:
                    fp[idx] = 1
            else:
                fp[idx] = 1
        for arr in (fp, tp):
            c = 0
            for k in range(nd):
                c += arr[k]
                arr[k] = c
        n_gt = gt_counter[name]
        rec = [float(tp[k]) / max(n_gt, 1) for k in range(nd)]
        prec = [float(tp[k]) / max(fp[k] + tp[k], 1) for k in range(nd)]
        ap, mrec, mpre = voc_ap(rec, prec, mistakes)
        f1 = [rec[k] * prec[k] * 2 / (1 if prec[k] + rec[k] == 0 else prec[k] + rec[k]) for k in range(nd)]
        n_images = len(ids) if "n_img_all" in mistakes else img_counter[name]
        lamr, mr, fppi, mr9 = miss_rates(rec, fp, n_images)
        sum_ap += ap
        out["per_class"][name] = dict(ap=ap, tp=tp, fp=fp, rec=rec, prec=prec, f1=f1, score=score, score05_idx=score05_idx,
                                      mrec=mrec, mpre=mpre, lamr=lamr, mr=mr, fppi=fppi, mr9=mr9, n_gt=n_gt, n_images=n_images,
                                      n_det=nd, n_tp=tp[-1] if nd else 0)
    n_div = len([k for k in det_counter]) if "map_over_det_classes" in mistakes else len(gt_classes)
    out["mAP"] = sum_ap / n_div
    return out


def results_text(ev):
    """results/results.txt of :435-718 and the printed lines of :609-613, :675 -> (text, [lines])"""
    t = "# AP and precision/recall per class\n"
    printed = []
    for name in ev["classes"]:
        c = ev["per_class"][name]
        text = "{0:.2f}%".format(c["ap"] * 100) + " = " + name + " AP "
        t += text + "\n Precision: " + str(['%.2f' % x for x in c["prec"]]) + "\n Recall :" + \
            str(['%.2f' % x for x in c["rec"]]) + "\n\n"
        if c["n_det"] > 0:
            s = c["score05_idx"]
            printed.append(text + "\t||\tscore_threhold=0.5 : " + "F1=" + "{0:.2f}".format(c["f1"][s]) + " ; Recall=" +
                           "{0:.2f}%".format(c["rec"][s] * 100) + " ; Precision=" + "{0:.2f}%".format(c["prec"][s] * 100))
        else:
            printed.append(text + "\t||\tscore_threhold=0.5 : F1=0.00% ; Recall=0.00% ; Precision=0.00%")
    text = "mAP = {0:.2f}%".format(ev["mAP"] * 100)
    t += "\n# mAP of all classes\n" + text + "\n"
    printed.append(text)
    t += "\n# Number of ground-truth objects per class\n"
    for name in sorted(ev["gt_counter"]):
        t += name + ": " + str(ev["gt_counter"][name]) + "\n"
    t += "\n# Number of detected objects per class\n"
    for name in sorted(ev["det_counter"]):
        n_det = ev["det_counter"][name]
        n_tp = ev["per_class"][name]["n_tp"] if name in ev["per_class"] else 0
        t += name + ": " + str(n_det) + " (tp:" + str(n_tp) + ", fp:" + str(n_det - n_tp) + ")\n"
    return t, printed
