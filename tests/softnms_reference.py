"""A deliberately naive restatement of the Soft-NMS contract of include/glsdet_hip.h (glsdet_soft_nms; the reference is
py_cpu_softnms / batched_soft_nms, drone/merge_results.py:41-130): one candidate pair at a time, scalar loops, the same
index bookkeeping, no vectorised step that could share a mistake with the kernel.

Arithmetic: Python floats are IEEE fp64 and every operator rounds on its own, which is what numpy does one ufunc at a
time; `_f32` is the one rounding to fp32 of an update.  The gaussian weight goes through `np.exp` on an fp64 scalar, the
function the reference calls.

`mutant` plants one deliberate mistake (tests/test_softnms_reference.py shows that the recorded data sees each):
    "swap_le"      swap on `<=` instead of `<`
    "last_max"     last position of the maximum instead of the first
    "rotate"       rotate positions i..m instead of swapping i and m
    "area_no_plus1" areas without the +1
    "fp64_scores"  the score kept in fp64 between updates, rounded once at the end
    "nt_ge"        `>=` at Nt
    "thresh_ge"    `>=` at thresh
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "softnms_golden.npz")
METHODS = {"linear": 1, "gaussian": 2, "hard": 3}
INF = float("inf")


def load_golden(path=GOLDEN):
    """-> {key: array or str}: the inverse of tools/make_softnms_golden.pack"""
    import json
    z = np.load(path)
    out = {}
    for key, ent in json.loads(str(z["index"])).items():
        if ent[0] == "text":
            out[key] = ent[1]
        else:
            dt, off, shape = ent
            out[key] = z[dt][off: off + int(np.prod(shape, dtype=np.int64))].reshape(shape)
    return out


def _f32(x):
    return float(np.float32(x))


def segment(boxes, scores, method, nt=0.3, sigma=0.5, thresh=1e-4, mutant=None):
    """One class segment: boxes fp32 [N, 4] (x1, y1, x2, y2 -- the reference's column names differ, its arithmetic is
    symmetric in the two axes), scores fp32 [N], method 1 linear / 2 gaussian / anything else hard.
    -> dict: scores  fp32 [N]  decayed scores by POSITION (what the reference leaves in `sc`)
             index   int  [N]  original index by position
             keep    int  [K]  original indices with decayed score > fp32(thresh), in position order (the return value)
             updates int  [N]  by ORIGINAL index: how many updates the score received
             sel_gap float     smallest (largest - second largest) / largest over the candidates of any selection
                               (gaussian only; inf for the other methods)
             thr_gap float     smallest |score - thresh| / thresh over the final scores"""
    b = [[float(v) for v in row] for row in np.asarray(boxes, np.float32).reshape(-1, 4)]
    s = [float(v) for v in np.asarray(scores, np.float32).reshape(-1)]
    N = len(s)
    idx = list(range(N))
    plus = 0.0 if mutant == "area_no_plus1" else 1.0
    area = [(r[2] - r[0] + plus) * (r[3] - r[1] + plus) for r in b]
    upd = [0] * N
    sel_gap = INF
    nt, sigma = float(nt), float(sigma)
    th = _f32(thresh)
    for i in range(N):
        if i != N - 1:
            m = i + 1
            for k in range(i + 2, N):                       # first maximum of score[i+1:]
                if s[k] > s[m] or (mutant == "last_max" and s[k] == s[m]):
                    m = k
            if method == 2:                                 # gap between the two largest candidates of score[i:]
                v1, v2 = -INF, -INF                         # (the gaussian tests need it; the other methods are exact)
                for k in range(i, N):
                    if s[k] > v1:
                        v1, v2 = s[k], v1
                    elif s[k] > v2:
                        v2 = s[k]
                if v1 > 0:
                    sel_gap = min(sel_gap, (v1 - v2) / v1)
            if s[i] < s[m] or (mutant == "swap_le" and s[i] <= s[m]):
                if mutant == "rotate":
                    for arr in (b, s, idx, area):
                        arr.insert(i, arr.pop(m))
                else:
                    for arr in (b, s, idx, area):
                        arr[i], arr[m] = arr[m], arr[i]
        bi, ai = b[i], area[i]
        for k in range(i + 1, N):
            bk = b[k]
            w = min(bi[2], bk[2]) - max(bi[0], bk[0]) + 1.0
            w = max(0.0, w)
            h = min(bi[3], bk[3]) - max(bi[1], bk[1]) + 1.0
            h = max(0.0, h)
            inter = w * h
            ovr = inter / (ai + area[k] - inter)
            over = ovr >= nt if mutant == "nt_ge" else ovr > nt
            if method == 1:
                weight = 1.0 - ovr if over else 1.0
            elif method == 2:
                weight = float(np.exp(np.float64(-(ovr * ovr) / sigma)))
            else:
                weight = 0.0 if over else 1.0
            s[k] = weight * s[k] if mutant == "fp64_scores" else _f32(weight * s[k])
            upd[idx[k]] += 1
    s = [_f32(v) for v in s]
    keep = [idx[p] for p in range(N) if (s[p] >= th if mutant == "thresh_ge" else s[p] > th)]
    thr_gap = min([abs(v - th) / th for v in s], default=INF) if th > 0 else INF
    updates = np.zeros(N, np.int64)
    updates[:] = upd
    return {"scores": np.asarray(s, np.float32), "index": np.asarray(idx, np.int64), "keep": np.asarray(keep, np.int64),
            "updates": updates, "sel_gap": sel_gap, "thr_gap": thr_gap}


def batched(boxes, scores, labels, method, nt=0.3, sigma=0.5, thresh=1e-4, rescore=False, mutant=None):
    """batched_soft_nms: per class present the rows in ascending original index through `segment`.
    -> dict: order   int [K]   kept original indices by original score descending (rescore: decayed score), ties to the
                               lower original index
             decayed fp32 [n]  decayed score by original index;  updates int [n];  sel_gap, thr_gap: the minima"""
    boxes = np.asarray(boxes, np.float32).reshape(-1, 4)
    scores = np.asarray(scores, np.float32).reshape(-1)
    labels = np.asarray(labels).reshape(-1)
    n = len(scores)
    dec = np.zeros(n, np.float32)
    upd = np.zeros(n, np.int64)
    kept = []
    sel_gap = thr_gap = INF
    for c in sorted(set(labels.tolist())):
        rows = [r for r in range(n) if labels[r] == c]
        seg = segment(boxes[rows], scores[rows], method, nt, sigma, thresh, mutant)
        for p in range(len(rows)):
            dec[rows[seg["index"][p]]] = seg["scores"][p]
        for j in range(len(rows)):
            upd[rows[j]] = seg["updates"][j]
        kept += [rows[j] for j in seg["keep"]]
        sel_gap, thr_gap = min(sel_gap, seg["sel_gap"]), min(thr_gap, seg["thr_gap"])
    key = dec if rescore else scores
    order = sorted(kept, key=lambda r: (-float(key[r]), r))
    return {"order": np.asarray(order, np.int64), "decayed": dec, "updates": upd, "sel_gap": sel_gap, "thr_gap": thr_gap}


def detections(rows, method, nt=0.3, sigma=0.5, thresh=1e-4, rescore=False, max_det=None):
    """rows fp32 [n, >=6] x1, y1, x2, y2, score, label (one image of glsdet_soft_nms's input)
    -> (dets fp32 [min(K, max_det), 7] = box, original score, decayed score, label;  K;  the `batched` dict)"""
    rows = np.asarray(rows, np.float32)
    rows = rows.reshape(-1, rows.shape[-1] if rows.ndim == 2 else 6)
    r = batched(rows[:, :4], rows[:, 4], rows[:, 5].astype(np.int64), method, nt, sigma, thresh, rescore)
    o = r["order"]
    dets = np.concatenate([rows[o, :4], rows[o, 4:5], r["decayed"][o, None], rows[o, 5:6]], axis=1).astype(np.float32)
    K = len(o)
    return (dets if max_det is None else dets[:max_det]), K, r


def merged_lines(rows, classes, method=2, nt=0.3, sigma=0.5, thresh=1e-4):
    """drone/merge_results.py:144-172 with batched_soft_nms as the call: rows [n, 6] as parsed from the result files
    -> the lines of the merged file ("<class> <float(score)> <int corners>", the ORIGINAL score)."""
    rows = np.asarray(rows, np.float32).reshape(-1, 6)
    r = batched(rows[:, :4], rows[:, 4], rows[:, 5].astype(np.int64), method, nt, sigma, thresh)
    return ["%s %s %s %s %s %s\n" % (classes[int(rows[j, 5])], float(rows[j, 4]), int(rows[j, 0]), int(rows[j, 1]),
                                     int(rows[j, 2]), int(rows[j, 3])) for j in r["order"]]
