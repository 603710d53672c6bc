"""Records tests/golden/softnms_golden.npz: the outputs of the reference's own `py_cpu_softnms` and `batched_soft_nms`
(drone/merge_results.py:41-130) on small cases.

    python tools/make_softnms_golden.py <reference checkout>/yolox-drone/merge_results.py

The file cannot be imported: at module level it opens a hard-coded class list and imports torchvision.  It is parsed
with `ast` and only the two FunctionDefs `py_cpu_softnms` and `batched_soft_nms` are executed, in a namespace that holds
`numpy` and `torch`.  `batched_soft_nms` hard-codes Nt=0.3, sigma=0.5, thresh=0.0001, method=2 in its call; for the
other parameter sets the four keyword constants of that one call are replaced in the syntax tree before it is compiled,
nothing else.  Nothing of the reference's text is written to the fixture.

The .npz holds one flat array per dtype and a JSON index (see `pack`); tests/softnms_reference.load_golden turns it back
into the keys below.
Per case `c<i>`: boxes fp32 [n, 4], scores fp32 [n], labels int64 [n], and per parameter set `p<j>` (params fp64 [4] =
method, Nt, sigma, thresh):
    scores   fp32  what py_cpu_softnms leaves in its `sc` argument (decayed scores by POSITION), the classes present
                   concatenated in ascending class order
    keep     int64 its return value per class (indices into the class's rows, position order), concatenated
    nkeep    int64 [classes present] lengths of the above
    order    int64 batched_soft_nms's return value (its torch.sort leaves the order of EQUAL scores unspecified)
Per scene `s<i>`: the text of two result files (a, b) and of the merged file (out).  The merged text is THIS SCRIPT'S
composition: merge_results.py:144-172 re-enacted line by line (parse both files to rows, torch.Tensor, torch.cat, the
suppression call, index, "%s %s %s %s %s %s" with float(score) and int(corners)) with `batched_soft_nms` -- the call the
reference ships commented out at :159-163 -- in the place of `boxes.batched_nms`.  The reference never ran it that way.
The tests read only the .npz."""
import ast
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from glsdet_amd.eval.results import VISDRONE_CLASSES, parse_detection_results  # noqa: E402

REF_PARAMS = (2, 0.3, 0.5, 0.0001)
BASE_PARAMS = [REF_PARAMS, (1, 0.3, 0.5, 0.0001), (3, 0.3, 0.5, 0.0001)]
EXTRA_PARAMS = [(1, 0.5, 0.5, 0.25), (3, 0.5, 0.5, 0.0001), (2, 0.3, 0.25, 0.05), (1, 0.3, 0.5, 0.25), (3, 0.3, 0.5, 0.001)]
KEYS = ("Nt", "sigma", "thresh", "method")


def load_reference(path):
    """-> namespace(params) with the two functions compiled for one parameter set"""
    tree = ast.parse(open(path, encoding="utf-8").read())
    fns = {n.name: n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("py_cpu_softnms", "batched_soft_nms")}
    assert len(fns) == 2

    def namespace(params):
        method, nt, sigma, thresh = params
        want = {"Nt": nt, "sigma": sigma, "thresh": thresh, "method": method}
        batched = copy.deepcopy(fns["batched_soft_nms"])
        calls = [n for n in ast.walk(batched) if isinstance(n, ast.Call) and getattr(n.func, "id", None) == "py_cpu_softnms"]
        assert len(calls) == 1 and sorted(k.arg for k in calls[0].keywords) == sorted(KEYS)
        for k in calls[0].keywords:
            k.value = ast.Constant(want[k.arg])
        mod = ast.fix_missing_locations(ast.Module(body=[fns["py_cpu_softnms"], batched], type_ignores=[]))
        ns = {"np": np, "torch": torch}
        exec(compile(mod, "<reference soft-nms functions>", "exec"), ns)
        return ns

    return namespace


def random_case(rng, n, nc, integer, quant):
    """clustered boxes so that most rows overlap something; quant: scores on a grid of 1/quant (ties) or free"""
    ctr = rng.uniform(0, 40 + 2 * n ** 0.5, (n, 2))
    half = rng.uniform(2, 14, (n, 2))
    boxes = np.concatenate([ctr - half, ctr + half], 1)
    boxes = np.round(boxes) if integer else boxes
    if quant:
        scores = rng.integers(1, quant + 1, n) / quant
    else:
        scores = rng.uniform(0.02, 1.0, n)
    return boxes.astype(np.float32), scores.astype(np.float32), rng.integers(0, nc, n).astype(np.int64)


def crafted_case():
    """one class per situation: ovr == 0.3 exactly (3 / 10), ovr == 0.5 exactly (2 / 4), a linear decay that lands exactly on
    a threshold of 0.25, a score that IS fp32(1e-4), three bit-equal twins, equal scores whose order the swaps decide"""
    rows = [([0, 0, 5, 0], 0.9, 0), ([3, 0, 9, 0], 0.8, 0),
            ([0, 0, 2, 0], 0.75, 1), ([1, 0, 3, 0], 0.5, 1),
            ([0, 0, 2, 0], 0.75, 2), ([1, 0, 3, 0], 0.5, 2), ([40, 40, 44, 44], 0.25, 2),
            ([0, 0, 4, 4], np.float32(0.0001), 3), ([20, 20, 24, 24], 0.5, 3),
            ([2, 2, 9, 9], 0.5, 4), ([2, 2, 9, 9], 0.5, 4), ([2, 2, 9, 9], 0.5, 4),
            ([0, 0, 7, 7], 0.5, 5), ([4, 0, 11, 7], 0.75, 5), ([2, 2, 9, 9], 0.5, 5), ([6, 2, 13, 9], 0.75, 5),
            ([1, 3, 8, 10], 0.5, 5), ([5, 5, 12, 12], 0.75, 5), ([0, 4, 7, 11], 0.5, 5)]
    return (np.float32([r[0] for r in rows]), np.float32([r[1] for r in rows]), np.int64([r[2] for r in rows]))


def cases():
    rng = np.random.default_rng(41300)
    out = [(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), BASE_PARAMS),
           crafted_case() + (BASE_PARAMS + EXTRA_PARAMS,)]
    sizes = [1, 2, 3, 4, 5, 7, 9, 12, 16, 20, 24, 28, 33, 40, 48, 56, 63, 64, 65, 72, 80, 80]
    for j, n in enumerate(sizes):
        for integer in (True, False):
            nc = [1, 2, 3, 10, 5][(j + integer) % 5]
            quant = [0, 8, 0, 4][(j + 2 * integer) % 4]
            params = BASE_PARAMS + ([EXTRA_PARAMS[(j + integer) % len(EXTRA_PARAMS)]] if j % 2 == 0 else [])
            out.append(random_case(rng, n, nc, integer, quant) + (params,))
    return out


def scene_files(rng, n_a, n_b):
    """two result files of one picture: b repeats most of a's objects a few pixels off, as a second detector would"""
    def lines(boxes, scores, labels):
        return "".join("%s %s %d %d %d %d\n" % (VISDRONE_CLASSES[l], str(s)[:6], b[0], b[1], b[2], b[3])
                       for b, s, l in zip(boxes, scores, labels))
    ctr = rng.uniform(20, 220, (n_a, 2))
    half = rng.uniform(4, 18, (n_a, 2))
    lab = rng.integers(0, 4, n_a)
    a = np.concatenate([ctr - half, ctr + half], 1).astype(np.int64)
    # distinct scores: the reference's final torch.sort leaves the order of equal scores unspecified, and the merged text
    # is compared as text
    draw = ((500 + rng.permutation(9000)[: 2 * n_a]) / 10000.0).astype(np.float32)
    sa = draw[:n_a]
    pick = rng.permutation(n_a)[:n_b]
    b = a[pick] + rng.integers(-4, 5, (len(pick), 4))
    sb = draw[n_a: n_a + len(pick)]
    la, lb = lab, lab[pick]
    if n_b:
        # a crowd: the same object reported five times per file a pixel apart with low scores, next to one confident
        # row.  With the reference's sigma = 0.5 and thresh = 1e-4 a row is dropped only after several such decays
        # (a single weight is never below exp(-2)), so without a crowd the soft rule keeps every row.
        crowd = np.int64([150, 150, 190, 200]) + rng.integers(-1, 2, (10, 4))
        sc = ((100 + rng.permutation(300)[:10]) / 10000.0).astype(np.float32)
        sc[0] = np.float32(0.9731)
        a, sa, la = np.concatenate([a, crowd[:5]]), np.concatenate([sa, sc[:5]]), np.concatenate([la, np.full(5, 3)])
        b, sb, lb = np.concatenate([b, crowd[5:]]), np.concatenate([sb, sc[5:]]), np.concatenate([lb, np.full(5, 3)])
    return lines(a, sa, la), lines(b, sb, lb)


def merged_text(ns, texts, tmp):
    """merge_results.py:144-172, the soft call taken (see the module docstring)"""
    index = {c: i for i, c in enumerate(VISDRONE_CLASSES)}
    cur = []
    for k, t in enumerate(texts):
        p = os.path.join(tmp, "f%d.txt" % k)
        with open(p, "w") as f:
            f.write(t)
        cur.append(torch.Tensor(parse_detection_results(p, index)))
    detections = torch.cat(cur, dim=0)
    positive_indexes = ns["batched_soft_nms"](detections[:, :4], detections[:, 4], detections[:, 5])
    detections = detections[positive_indexes]
    out = ""
    for i in range(detections.shape[0]):
        d = detections[i]
        out += "%s %s %s %s %s %s\n" % (VISDRONE_CLASSES[int(d[5])], float(d[4]), int(d[0]), int(d[1]), int(d[2]), int(d[3]))
    return out


def pack(data):
    """a thousand small arrays cost more in zip headers than in content: one flat array per dtype and a JSON index
    {key: [dtype, offset, shape]} (tests/softnms_reference.load_golden is the inverse); texts go into the index itself"""
    import json
    flat, index = {}, {}
    for key, v in data.items():
        v = np.asarray(v)
        if v.dtype.kind == "U":
            index[key] = ["text", str(v)]
            continue
        dt = v.dtype.name
        assert dt in ("float32", "float64", "int64")
        off = sum(len(a) for a in flat.setdefault(dt, []))
        flat[dt].append(v.reshape(-1))
        index[key] = [dt, off, list(v.shape)]
    out = {dt: np.concatenate(parts) for dt, parts in flat.items()}
    out["index"] = np.array(json.dumps(index))
    return out


def main(path):
    import tempfile
    namespace = load_reference(path)
    data = {}
    cs = cases()
    data["n_cases"] = np.int64(len(cs))
    for ci, (boxes, scores, labels, params) in enumerate(cs):
        data["c%d/boxes" % ci], data["c%d/scores" % ci], data["c%d/labels" % ci] = boxes, scores, labels
        data["c%d/n_params" % ci] = np.int64(len(params))
        for pi, prm in enumerate(params):
            ns = namespace(prm)
            method, nt, sigma, thresh = prm
            sc_all, keep_all, nkeep = [], [], []
            for c in sorted(set(labels.tolist())):
                rows = np.where(labels == c)[0]
                sc = scores[rows].copy()
                keep = ns["py_cpu_softnms"](boxes[rows].copy(), sc, Nt=nt, sigma=sigma, thresh=thresh, method=method)
                assert sc.dtype == np.float32
                sc_all.append(sc)
                keep_all.append(np.asarray(keep, np.int64))
                nkeep.append(len(keep))
            key = "c%d/p%d/" % (ci, pi)
            data[key + "params"] = np.float64(prm)
            data[key + "scores"] = np.concatenate(sc_all) if sc_all else np.zeros(0, np.float32)
            data[key + "keep"] = np.concatenate(keep_all) if keep_all else np.zeros(0, np.int64)
            data[key + "nkeep"] = np.int64(nkeep)
            t_scores = torch.from_numpy(scores.copy())
            order = ns["batched_soft_nms"](torch.from_numpy(boxes.copy()), t_scores, torch.from_numpy(labels.copy()))
            assert torch.equal(t_scores, torch.from_numpy(scores))          # the caller's scores are not modified
            data[key + "order"] = order.numpy().astype(np.int64)
    rng = np.random.default_rng(41301)
    ns = namespace(REF_PARAMS)
    with tempfile.TemporaryDirectory() as tmp:
        for si, (na, nb) in enumerate(((30, 24), (45, 45), (12, 0))):
            a, b = scene_files(rng, na, nb)
            data["s%d/a" % si], data["s%d/b" % si] = np.array(a), np.array(b)
            data["s%d/out" % si] = np.array(merged_text(ns, (a, b), tmp))
    data["n_scenes"] = np.int64(3)
    out = os.path.join(ROOT, "tests", "golden", "softnms_golden.npz")
    np.savez_compressed(out, **pack(data))
    print("wrote %s: %d cases, %d bytes, numpy %s, torch %s" % (out, len(cs), os.path.getsize(out), np.__version__, torch.__version__))


if __name__ == "__main__":
    main(sys.argv[1])
