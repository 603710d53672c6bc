"""VOC-style mAP with the matching, the curves and the AP on the GPU: the score the drone harness reports.

`get_map(MINOVERLAP, draw_plot, path='./map_out')` has the signature of the reference's
drone/models/core/utils_map.py:294 (called at get_map.py:121-124) and is its replacement:

    from glsdet_amd.eval.voc import get_map
    get_map(0.5, True, path="map_out")       # reads map_out/ground-truth, map_out/detection-results

It writes `path/results/results.txt` byte for byte as the reference does and prints the same lines, and returns what
`VocEval.evaluate` returns.  The plots are not lowered: `draw_plot=True` is accepted, one warning line says so.

`VocEval` takes the same data from memory (`add_ground_truth`, `add_detections`) or from the two directories
(`load_dirs`).  Parsing, the stable sort by `float(confidence)` descending and the CSR arrays stay on the host in numpy;
ONE `torch.ops.glsdet.voc_ap` call (glsdet_voc_ap, include/glsdet_hip.h) serves every class and every threshold.  The
log-average miss rate is `exp(mean(log(maximum(1e-10, .))))` of the nine miss rates the kernel picks, applied on the host
with numpy as the reference does.  There is no CPU matching path: without the HIP library `evaluate` raises.

File semantics (:322-430): ground-truth files sorted, a missing partner file raises FileNotFoundError (the reference
prints and calls sys.exit(0)); the class list is the sorted classes with at least one non-difficult ground truth and
mAP = sum / len(that list); detections are enumerated in sorted-file order, then line order, and sorted stably by score
descending (`np.lexsort`, stable, on (-score, class)); a class name is everything before the last 4 fields (5 for a
detection and for a difficult ground truth) joined by single blanks.  The block "Number of detected objects per class"
counts by the FIRST token of the line, as :682-690 does.  Out of scope: class names that contain the word `difficult`
(the reference tests `"difficult" in line` on the whole line), and image ids that contain ".txt"."""
from __future__ import annotations

import glob
import os
import shutil
import warnings
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np
import torch

from .. import _lib

__all__ = ["VocEval", "check_layout", "get_map"]


def _gt_row(line: str):
    f = line.split()
    if "difficult" in line:
        return " ".join(f[:-5]), f[-5:-1], True
    return " ".join(f[:-4]), f[-4:], False


def _dr_row(line: str):
    f = line.split()
    return " ".join(f[:-5]), f[-5], f[-4:], f[0]


def check_layout(cls_off, pair_off, pair_det, gt_off, n_dt: int, n_gt_boxes: int) -> None:
    """What glsdet_voc_ap cannot check without reading device memory back: the three offset arrays rise from 0 to their
    array's length without a step down, every pair owns a detection, and pair_det holds every detection index once."""
    for a, top, what in ((cls_off, n_dt, "cls_off"), (pair_off, n_dt, "pair_off"), (gt_off, n_gt_boxes, "gt_off")):
        a = np.asarray(a)
        if a.ndim != 1 or a.size < 1 or int(a[0]) != 0 or int(a[-1]) != top or bool((np.diff(a.astype(np.int64)) < 0).any()):
            raise ValueError("voc_ap: %s must rise from 0 to %d without a step down" % (what, top))
    if len(pair_off) != len(gt_off):
        raise ValueError("voc_ap: pair_off and gt_off describe different numbers of pairs")
    if bool((np.diff(np.asarray(pair_off).astype(np.int64)) < 1).any()):
        raise ValueError("voc_ap: every pair owns at least one detection")
    if not np.array_equal(np.sort(np.asarray(pair_det).astype(np.int64)), np.arange(n_dt)):
        raise ValueError("voc_ap: pair_det must hold every detection index exactly once")


class VocEval:
    """Collects ground truths and detections per image; evaluate() scores them on the GPU.

    rows of add_ground_truth: (class_name, left, top, right, bottom) or (..., difficult); rows of add_detections:
    (class_name, confidence, left, top, right, bottom).  Every image needs both calls (possibly with no rows), as every
    ground-truth file needs its detection file."""

    def __init__(self, classes: Optional[Sequence[str]] = None, device: str = "cuda:0"):
        self.classes = None if classes is None else list(classes)      # restricts the evaluated classes when given
        self.device = device
        self._gt: Dict[str, list] = {}
        self._dr: Dict[str, list] = {}

    # ------------------------------------------------------------------ input
    def add_ground_truth(self, image_id: str, rows: Iterable) -> None:
        out = self._gt.setdefault(str(image_id), [])
        for r in rows:
            out.append((str(r[0]), float(r[1]), float(r[2]), float(r[3]), float(r[4]), bool(r[5]) if len(r) > 5 else False))

    def add_detections(self, image_id: str, rows: Iterable) -> None:
        out = self._dr.setdefault(str(image_id), [])
        for r in rows:
            name = str(r[0])
            out.append((name, float(r[1]), float(r[2]), float(r[3]), float(r[4]), float(r[5]), name.split()[0]))

    def load_dirs(self, gt_dir: str, dr_dir: str) -> "VocEval":
        gt_files = sorted(glob.glob(gt_dir + "/*.txt"))
        if not gt_files:
            raise FileNotFoundError("Error: No ground-truth files found!")
        for path in gt_files:
            fid = os.path.basename(os.path.normpath(path.split(".txt", 1)[0]))
            partner = os.path.join(dr_dir, fid + ".txt")
            if not os.path.exists(partner):
                raise FileNotFoundError("Error. File not found: {}\n".format(partner))
            with open(path) as f:
                rows = [_gt_row(x.strip()) for x in f.readlines()]
            self.add_ground_truth(fid, [(n, *b, d) for n, b, d in rows])
        for path in sorted(glob.glob(dr_dir + "/*.txt")):
            fid = os.path.basename(os.path.normpath(path.split(".txt", 1)[0]))
            partner = os.path.join(gt_dir, fid + ".txt")
            if not os.path.exists(partner):
                raise FileNotFoundError("Error. File not found: {}\n".format(partner))
            with open(path) as f:
                rows = [_dr_row(x.strip()) for x in f.readlines()]
            out = self._dr.setdefault(fid, [])
            for n, s, b, first in rows:
                out.append((n, float(s), float(b[0]), float(b[1]), float(b[2]), float(b[3]), first))
        return self

    # ------------------------------------------------------------------ host preparation
    def _prepare(self):
        for i in self._gt:
            if i not in self._dr:
                raise FileNotFoundError("Error. File not found: detection results of image {}\n".format(i))
        for i in self._dr:
            if i not in self._gt:
                raise FileNotFoundError("Error. File not found: ground truth of image {}\n".format(i))
        if not self._gt:
            raise FileNotFoundError("Error: No ground-truth files found!")
        ids = sorted(self._gt, key=lambda i: i + ".txt")                # the reference sorts the file paths
        gt_rows = [(k, r) for k, i in enumerate(ids) for r in self._gt[i]]
        dr_rows = [(k, r) for k, i in enumerate(ids) for r in self._dr[i]]
        gt_counter: Dict[str, int] = {}
        for _, r in gt_rows:
            if not r[5]:
                gt_counter[r[0]] = gt_counter.get(r[0], 0) + 1
        det_counter: Dict[str, int] = {}
        for _, r in dr_rows:
            det_counter[r[6]] = det_counter.get(r[6], 0) + 1
        classes = sorted(gt_counter)
        if self.classes is not None:
            classes = [c for c in classes if c in self.classes]
        if not classes:
            raise ValueError("VocEval: no class has a non-difficult ground truth")
        index = {c: k for k, c in enumerate(classes)}
        C, I = len(classes), len(ids)

        g_cls = np.array([index.get(r[0], -1) for _, r in gt_rows], dtype=np.int64)
        g_img = np.array([k for k, _ in gt_rows], dtype=np.int64)
        g_box = np.array([r[1:5] for _, r in gt_rows], dtype=np.float64).reshape(-1, 4)
        g_dif = np.array([r[5] for _, r in gt_rows], dtype=np.uint8)
        keep = g_cls >= 0
        g_cls, g_img, g_box, g_dif = g_cls[keep], g_img[keep], g_box[keep], g_dif[keep]
        regular = g_dif == 0
        n_gt = np.bincount(g_cls[regular], minlength=C).astype(np.int32)
        n_img = np.bincount(np.unique(g_cls[regular] * I + g_img[regular]) // I, minlength=C).astype(np.int32)

        d_cls = np.array([index.get(r[0], -1) for _, r in dr_rows], dtype=np.int64)
        d_img = np.array([k for k, _ in dr_rows], dtype=np.int64)
        d_score = np.array([r[1] for _, r in dr_rows], dtype=np.float64)
        d_box = np.array([r[2:6] for _, r in dr_rows], dtype=np.float64).reshape(-1, 4)
        keep = d_cls >= 0
        d_cls, d_img, d_score, d_box = d_cls[keep], d_img[keep], d_score[keep], d_box[keep]
        order = np.lexsort((-d_score, d_cls))               # stable: equal scores keep file, then line order
        d_cls, d_img, d_score, d_box = d_cls[order], d_img[order], d_score[order], d_box[order]
        ND = len(d_cls)
        cls_off = np.zeros(C + 1, dtype=np.int32)
        cls_off[1:] = np.cumsum(np.bincount(d_cls, minlength=C))

        d_key = d_cls * I + d_img
        pair_key, pair_cnt = np.unique(d_key, return_counts=True)
        pair_det = np.argsort(d_key, kind="stable").astype(np.int32)    # ascending rank inside a pair
        pair_off = np.zeros(len(pair_key) + 1, dtype=np.int32)
        pair_off[1:] = np.cumsum(pair_cnt)
        g_key = g_cls * I + g_img
        g_order = np.argsort(g_key, kind="stable")                      # file order inside a pair
        lo = np.searchsorted(g_key[g_order], pair_key, side="left")
        hi = np.searchsorted(g_key[g_order], pair_key, side="right")
        gt_off = np.zeros(len(pair_key) + 1, dtype=np.int32)
        gt_off[1:] = np.cumsum(hi - lo)
        take = g_order[np.repeat(lo - gt_off[:-1], hi - lo) + np.arange(int(gt_off[-1]))] if len(pair_key) else g_order[:0]
        return dict(classes=classes, ids=ids, gt_counter=gt_counter, det_counter=det_counter, n_gt=n_gt, n_img=n_img,
                    dt_box=np.ascontiguousarray(d_box), score=d_score, cls_off=cls_off, pair_off=pair_off, pair_det=pair_det,
                    gt_off=gt_off, gt_box=np.ascontiguousarray(g_box[take]), gt_difficult=np.ascontiguousarray(g_dif[take]), ND=ND)

    # ------------------------------------------------------------------ the device call
    def evaluate(self, min_overlap: Union[float, Sequence[float]] = 0.5):
        """-> {"classes", "per_class": {name: {ap, tp, fp, rec, prec, f1, rec05, prec05, score05_idx, lamr, mr9, mpre, score,
        n_gt, n_images, n_det, n_tp}}, "mAP", "min_overlap", "gt_counter", "det_counter"}; tp / fp / rec / prec are the
        cumulative curves in rank order, f1 / rec05 / prec05 the values at score05_idx.  A sequence of thresholds gives a
        list of such dicts from the same single launch."""
        import glsdet_amd.torch_ops  # noqa: F401  (registers torch.ops.glsdet.voc_ap)
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.GlsdetLibraryError("glsdet_amd needs an MI355X visible to PyTorch-ROCm (no CPU fallback)")
        single = isinstance(min_overlap, (int, float))
        thr = np.array([min_overlap] if single else list(min_overlap), dtype=np.float64)
        if thr.size < 1:
            raise ValueError("VocEval.evaluate: at least one overlap threshold")
        h = self._prepare()
        check_layout(h["cls_off"], h["pair_off"], h["pair_det"], h["gt_off"], h["ND"], len(h["gt_difficult"]))
        dev = torch.device(self.device)
        up = lambda a: torch.from_numpy(a).to(dev)
        out = torch.ops.glsdet.voc_ap(up(h["dt_box"]), up(h["score"]), up(h["cls_off"]), up(h["pair_off"]), up(h["pair_det"]),
                                      up(h["gt_off"]), up(h["gt_box"]), up(h["gt_difficult"]), up(h["n_gt"]), up(h["n_img"]),
                                      up(thr), up(np.logspace(-2.0, 0.0, num=9)), False)
        tp, fp, rec, prec, mpre, cls_out = (o.cpu().numpy() for o in out)        # the copies synchronise
        results = []
        for t in range(len(thr)):
            per_class, sum_ap = {}, 0.0
            for k, name in enumerate(h["classes"]):
                d0, d1 = int(h["cls_off"][k]), int(h["cls_off"][k + 1])
                o = cls_out[t, k]
                mr9 = o[6:15].copy()
                lamr = float(np.exp(np.mean(np.log(np.maximum(1e-10, mr9))))) if d1 > d0 else 0      # :43-47, :60
                ap = float(o[0])
                sum_ap += ap
                per_class[name] = dict(ap=ap, tp=tp[t, d0:d1], fp=fp[t, d0:d1], rec=rec[t, d0:d1], prec=prec[t, d0:d1],
                                       mpre=mpre[t, d0:d1], score=h["score"][d0:d1], f1=float(o[3]), rec05=float(o[4]),
                                       prec05=float(o[5]), score05_idx=int(o[2]), lamr=lamr, mr9=mr9, n_gt=int(h["n_gt"][k]),
                                       n_images=int(h["n_img"][k]), n_det=d1 - d0, n_tp=int(o[1]))
            results.append(dict(classes=h["classes"], per_class=per_class, mAP=sum_ap / len(h["classes"]),
                                min_overlap=float(thr[t]), gt_counter=h["gt_counter"], det_counter=h["det_counter"]))
        return results[0] if single else results


def _results_text(ev) -> tuple:
    """results.txt of :435-718 and the lines :609-613, :675 print"""
    parts = ["# AP and precision/recall per class\n"]
    printed = []
    for name in ev["classes"]:
        c = ev["per_class"][name]
        text = "{0:.2f}%".format(c["ap"] * 100) + " = " + name + " AP "
        parts.append(text + "\n Precision: " + str(['%.2f' % x for x in c["prec"].tolist()]) + "\n Recall :" +
                     str(['%.2f' % x for x in c["rec"].tolist()]) + "\n\n")
        if c["n_det"] > 0:
            printed.append(text + "\t||\tscore_threhold=0.5 : " + "F1=" + "{0:.2f}".format(c["f1"]) + " ; Recall=" +
                           "{0:.2f}%".format(c["rec05"] * 100) + " ; Precision=" + "{0:.2f}%".format(c["prec05"] * 100))
        else:
            printed.append(text + "\t||\tscore_threhold=0.5 : F1=0.00% ; Recall=0.00% ; Precision=0.00%")
    text = "mAP = {0:.2f}%".format(ev["mAP"] * 100)
    parts.append("\n# mAP of all classes\n" + text + "\n")
    printed.append(text)
    parts.append("\n# Number of ground-truth objects per class\n")
    for name in sorted(ev["gt_counter"]):
        parts.append(name + ": " + str(ev["gt_counter"][name]) + "\n")
    parts.append("\n# Number of detected objects per class\n")
    for name in sorted(ev["det_counter"]):
        n_det = ev["det_counter"][name]
        n_tp = ev["per_class"][name]["n_tp"] if name in ev["per_class"] else 0
        parts.append(name + ": " + str(n_det) + " (tp:" + str(n_tp) + ", fp:" + str(n_det - n_tp) + ")\n")
    return "".join(parts), printed


def get_map(MINOVERLAP, draw_plot, path='./map_out'):
    """The reference's get_map (utils_map.py:294): scores path/detection-results against path/ground-truth at the overlap
    MINOVERLAP, writes path/results/results.txt, prints the per-class and mAP lines and returns VocEval.evaluate()'s dict."""
    ev = VocEval().load_dirs(os.path.join(path, 'ground-truth'), os.path.join(path, 'detection-results')).evaluate(float(MINOVERLAP))
    results_dir = os.path.join(path, 'results')
    if os.path.exists(results_dir):
        shutil.rmtree(results_dir)
    os.makedirs(results_dir)
    if draw_plot:
        warnings.warn("get_map: draw_plot is accepted, the plots are not drawn; the numbers go to results/results.txt", stacklevel=2)
    text, printed = _results_text(ev)
    with open(os.path.join(results_dir, "results.txt"), 'w') as f:
        f.write(text)
    for line in printed:
        print(line)
    return ev
