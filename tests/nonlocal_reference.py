"""float64 reference, exact-arithmetic data regime and case lists of the non-local block kernels (nl_gram / nl_fold /
nl_apply and nl_window of glsdet_amd/csrc/nonlocal.hip, behind glsdet_nonlocal, glsdet_nonlocal_multi, glsdet_nonlocal_split).

The reference (`nonlocal_block`) is the definition in its original order, on one window: f = theta phi^T / N (N x N),
y = f g, out = x + y Wout^T + b.  The kernels re-associate it (G = phi^T g, P = Wout G^T / N, out = x + theta P^T + b);
`regrouped` evaluates that form and exists only for the mutation checks and the float32 order checks of
tests/test_nonlocal_reference.py -- no expected value comes from it.

The exact regime (`case_data`, asserted per case by `check_regime`): theta, phi ternary; g = N * ternary with N the
window's pixel count (N <= 2048, exact in fp16); Wout = ternary * 2^-S; bout, x multiples of 2^-3.  Then the Gram sums are
N * integer, the fold sums N * m * 2^-S, and P = fl32(acc * fl32(1 / N)) returns m * 2^-S exactly when `invn_exact(N, max
|m|)` holds (it does not for every N: 7, 15, 63, 255, 1000 fail).  phi and g are non-zero on K support pixels only, K
chosen so that in every accumulation the sum of the absolute values of the terms, in units of their common step, stays
below 2^24: every float32 step of the kernels is then exact in any summation order, and the output is the exact value
rounded ONCE to the output type.  The float64 evaluation in the definition's order carries the rounding of k / N (about
N ci 2^-53 relative to a step of 2^-S); the true value is a multiple of 2^-S, so `on_grid` asserts the distance to the
nearest multiple is below 2^-30 and returns that multiple; test_nonlocal_reference.py holds it against an evaluation in
integers that never divides."""
import collections

import numpy as np

from tests.attention_reference import quadrant_slices
from tests.conv_reference import round_to  # noqa: F401  (the ONE rounding; re-exported for the tests)

LIMIT = 1 << 24
S = 10                                       # Wout = ternary * 2^-S: an odd multiple of 2^-10 above 1 is no fp16 number
STEP = 2.0 ** -S
FULL = (24, 36)                              # the map the host-written splits of the split cases refer to
KC = 128                                     # GLS_NL_KC: chunk of c1 (apply) / c2 (fold)
_VN = {"f16": 8, "f32": 4}                   # elements per 16-byte access

Case = collections.namedtuple("Case", "name kind n ci cx FH FW wins split shift tw xkind tkind okind seed")


# ------------------------------------------------------------------------------------------------------ the definition
def nonlocal_block(x, theta, phi, g, wout, bout, divisor=None, jweight=None, c1mask=None, c2mask=None):
    """One Non_local_Block on one window, float64, in the definition's order.  x [cx, h, w]; theta, phi, g [ci, h, w];
    wout [cx, ci]; bout [cx] -> [cx, h, w].  The keyword arguments exist for the mutation checks: another divisor than
    N (0: none), a weight per position j of the sum over j, channel masks of the theta . phi product (c1) and of g (c2)."""
    x = np.asarray(x, np.float64)
    ci, h, w = np.shape(theta)
    N = h * w
    th = np.asarray(theta, np.float64).reshape(ci, N).T                  # [N, ci]
    ph = np.asarray(phi, np.float64).reshape(ci, N).T
    gg = np.asarray(g, np.float64).reshape(ci, N).T
    if c1mask is not None:
        th = th * c1mask
    if c2mask is not None:
        gg = gg * c2mask
    f = th @ ph.T                                                        # [N, N] pairwise
    if divisor != 0:
        f = f / (N if divisor is None else divisor)
    if jweight is not None:
        f = f * np.asarray(jweight, np.float64)[None, :]
    y = f @ gg                                                           # [N, ci]
    o = y @ np.asarray(wout, np.float64).T + np.asarray(bout, np.float64)
    return x + o.T.reshape(-1, h, w)


def regrouped(x, theta, phi, g, wout, bout, invn=None, p_transposed=False, gram_from=None):
    """the kernels' association in float64: G = phi^T g, P = (Wout G^T) * invn, out = x + b + theta P^T.  invn: a float32
    value (the product acc * invn is then rounded to float32 as nl_fold stores it); p_transposed: nl_apply reads the
    [cx][ci] buffer as if it were [ci][cx]; gram_from: (phi, g) of another image"""
    x = np.asarray(x, np.float64)
    ci, h, w = np.shape(theta)
    N = h * w
    th = np.asarray(theta, np.float64).reshape(ci, N).T
    ph, gg = (np.asarray(a, np.float64).reshape(ci, N).T for a in (gram_from or (phi, g)))
    G = ph.T @ gg                                                        # [c1, c2]
    acc = np.asarray(wout, np.float64) @ G.T                             # [cx, c1]
    if invn is None:
        P = acc / N
    else:
        assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
        P = (acc.astype(np.float32) * np.float32(invn)).astype(np.float64)
    if p_transposed:
        cx = P.shape[0]
        flat = P.reshape(-1)
        P = flat[np.arange(ci)[None, :] * cx + np.arange(cx)[:, None]]
    o = th @ P.T + np.asarray(bout, np.float64)
    return x + o.T.reshape(-1, h, w)


# --------------------------------------------------------------------------------------------- mirrors of the launchers
def static_slices(N):
    """(nsplit, jchunk) of glsdet_nonlocal_multi"""
    ns = 8 if N >= 1024 else (4 if N >= 256 else 1)
    return ns, ((N + ns - 1) // ns + 63) // 64 * 64


def split_slices(N):
    """(nsplit, jchunk) of nl_window"""
    return 8, ((N + 7) // 8 + 63) // 64 * 64


def slices(case, N):
    return split_slices(N) if case.kind == "split" else static_slices(N)


def windows(case):
    """(h0, h1, w0, w1) per set, on the case's map"""
    if case.kind != "split":
        return list(case.wins)
    out = []
    for q in range(4):
        r, c = quadrant_slices(case.split, case.shift, q)
        r0, r1, _ = r.indices(case.FH)
        c0, c1, _ = c.indices(case.FW)
        out.append((r0, r1, c0, c1))
    return out


def layout(kind, h, w, c, dt):
    """a view's place in a buffer of its own -> (H, W, Ct, h0, w0, c0): the kinds of tests/test_conv_exact.py's Placed
    (with the channel count padded to 8 only in the embedded kinds, so that 30 channels can have aligned strides), plus
    'odd': a channel offset and a pixel stride that are no multiple of a 16-byte access in either dtype"""
    c8 = (c + 7) // 8 * 8
    if kind == "dense":
        return h, w, c, 0, 0, 0
    if kind == "slice":
        return h, w, c8 + 24, 0, 0, 16
    if kind == "window":
        return h + 3, w + 2, c8 + 24, 2, 1, 16
    assert kind == "odd"
    ct = c + 11 if (c + 11) % 4 else c + 13
    return h + 2, w + 2, ct, 1, 1, 5


def aligned(kind, h, w, c, dt, extra=0):
    """strides, view offset and `extra` (nl_window's offset) are multiples of a 16-byte access (buffers are 256-aligned)"""
    H, W, Ct, h0, w0, c0 = layout(kind, h, w, c, dt)
    vn = _VN[dt]
    return all(v % vn == 0 for v in (Ct, W * Ct, H * W * Ct, (h0 * W + w0) * Ct + c0, extra))


def window_offsets(case, kind, c, dt):
    """nl_window's xo / to / oo per set for a full-map view of `kind`: 0 unless the split lives on the device"""
    if case.kind != "split":
        return [0] * len(case.wins)
    H, W, Ct = layout(kind, case.FH, case.FW, c, dt)[:3]
    return [(h0 * W + w0) * Ct for h0, _, w0, _ in windows(case)]


def predicates(case, dt):
    """the kernels' vec (nl_gram), vec_t and vec_o (nl_apply) per set.  Static sets are windows of the placed map: their
    offset is part of the view's base; split sets take it from nl_window"""
    out = []
    vn = _VN[dt]
    for q, (h0, h1, w0, w1) in enumerate(windows(case)):
        def ok(kind, c):
            H, W, Ct, r0, s0, c0 = layout(kind, case.FH, case.FW, c, dt)
            off = ((r0 + h0) * W + s0 + w0) * Ct + c0
            if case.kind == "split":                                      # base and window offset are checked separately
                return aligned(kind, case.FH, case.FW, c, dt, window_offsets(case, kind, c, dt)[q])
            return all(v % vn == 0 for v in (Ct, W * Ct, H * W * Ct, off))
        vec_t = ok(case.tkind, case.tw)
        vec = vec_t and case.ci % 16 == 0
        vec_o = ok(case.xkind, case.cx) and ok(case.okind or case.xkind, case.cx) and case.cx % vn == 0 and min(case.ci, KC) >= 32
        out.append({"vec": vec, "vec_t": vec_t, "vec_o": vec_o})
    return out


# ------------------------------------------------------------------------------------------------------ the 1 / N step
def invn_exact(N, mmax):
    """fl32(fl32(N m) * fl32(1 / N)) == m for every integer 1 <= m <= mmax (N m < 2^24, so the product N m is exact)"""
    assert N * max(mmax, 1) < LIMIT
    m = np.arange(1, max(mmax, 1) + 1, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(N)
    return bool(np.array_equal((m * np.float32(N)) * inv, m))


def good_window(N, mmax=None):
    """the predicate over the widest range of m a case can have: |m| <= min(2^24 / N, 2^16)"""
    return N <= 2048 and invn_exact(N, min((LIMIT - 1) // N, 1 << 16) if mmax is None else mmax)


# ------------------------------------------------------------------------------------------------------------ the data
def support_size(N, ci):
    """K support pixels of phi and g: fold sums N ci K steps at most, apply ci^2 K: both below 2^23"""
    return max(1, min(N, (LIMIT // 2) // (N * ci), (LIMIT // 2) // (ci * ci)))


def _support(rng, case, N):
    """K positions: the last pixel (the partial tile), the first of every non-empty Gram slice, the rest random"""
    K = support_size(N, case.ci)
    ns, jchunk = slices(case, N)
    must = {N - 1} | {z * jchunk for z in range(ns) if z * jchunk < N}
    if N % 64:
        must.add(N // 64 * 64)
    must = sorted(must)[:K] if K < len(must) else sorted(must)
    rest = [j for j in rng.permutation(N) if j not in set(must)][: K - len(must)]
    mask = np.zeros(N, np.int64)
    mask[must + rest] = 1
    return mask


_DATA = {}


def case_data(case):
    """-> {x [n, cx, FH, FW], tpg: one map per set of a split case, else ONE shared map [n, tw, FH, FW] (NaN outside the
    windows and in the channels past 3 ci), wout [sets][cx, ci], bout [sets][cx], ints: per set the integer operands}"""
    if case.name in _DATA:
        return _DATA[case.name]
    rng = np.random.RandomState(case.seed)
    n, ci, cx = case.n, case.ci, case.cx
    wins = windows(case)
    x = rng.randint(-128, 129, (n, cx, case.FH, case.FW)) / 8.0
    maps = [np.full((n, case.tw, case.FH, case.FW), np.nan) for _ in range(len(wins) if case.kind == "split" else 1)]
    wout, bout, ints = [], [], []
    for q, (h0, h1, w0, w1) in enumerate(wins):
        h, w = h1 - h0, w1 - w0
        N = h * w
        mask = _support(rng, case, N)
        theta = rng.randint(-1, 2, (n, ci, N))
        phi = rng.randint(-1, 2, (n, ci, N)) * mask
        tg = rng.randint(-1, 2, (n, ci, N)) * mask
        t = maps[q if case.kind == "split" else 0]
        assert np.isnan(t[:, :, h0:h1, w0:w1]).all(), "the windows of a case do not overlap"
        t[:, :3 * ci, h0:h1, w0:w1] = np.concatenate([theta, phi, tg * N], 1).reshape(n, 3 * ci, h, w)
        tw_ = rng.randint(-1, 2, (cx, ci))
        wout.append(tw_ * STEP)
        bout.append(rng.randint(-32, 33, cx) / 8.0)
        ints.append({"theta": theta, "phi": phi, "tg": tg, "tw": tw_, "N": N})
    _DATA[case.name] = {"x": x, "tpg": maps, "wout": wout, "bout": bout, "ints": ints}
    return _DATA[case.name]


def generic_data(case, mode, seed):
    """continuous operands on the case's geometry, as tests/test_attention_fuzz.py draws them: theta in U(-1, 1), phi and
    g in U(0, 1) (a Gram of mean N / 4: the 1 / N matters), rounded to the engine's dtype; NaN where case_data has it"""
    rng = np.random.RandomState(seed)
    ft = np.float16 if mode == "f16" else np.float32
    r = lambda a: np.asarray(a, np.float32).astype(ft).astype(np.float64)
    n, ci, cx = case.n, case.ci, case.cx
    wins = windows(case)
    x = r(rng.standard_normal((n, cx, case.FH, case.FW)))
    maps = [np.full((n, case.tw, case.FH, case.FW), np.nan) for _ in range(len(wins) if case.kind == "split" else 1)]
    wout, bout = [], []
    for q, (h0, h1, w0, w1) in enumerate(wins):
        h, w = h1 - h0, w1 - w0
        t = np.concatenate([rng.uniform(-1, 1, (n, ci, h, w)), rng.uniform(0, 1, (n, 2 * ci, h, w))], 1)
        maps[q if case.kind == "split" else 0][:, :3 * ci, h0:h1, w0:w1] = r(t)
        wout.append((rng.uniform(-1, 1, (cx, ci)) * 4 / ci).astype(np.float32).astype(np.float64))
        bout.append(rng.standard_normal(cx).astype(np.float32).astype(np.float64))
    return {"x": x, "tpg": maps, "wout": wout, "bout": bout}


# ------------------------------------------------------------------------------------------- the reference over a case
def _tmap(case, d, q):
    return d["tpg"][q if case.kind == "split" else 0]


def _walk_with_window_width(case, t, win):
    """the window's pixels as a kernel finds them that steps rows by the window's width instead of the map's row stride"""
    h0, h1, w0, w1 = win
    h, w = h1 - h0, w1 - w0
    p = h0 * case.FW + w0 + np.arange(h * w)
    return t[:, :, p // case.FW, p % case.FW].reshape(t.shape[0], t.shape[1], h, w)


MUTATIONS = ["n_of_the_map", "n_one_row_off", "n_one_column_off", "no_division", "phi_g_exchanged", "p_transposed",
             "tail_tile_dropped", "slice_dropped", "slice_twice", "c1_chunk_dropped", "c2_chunk_dropped", "gram_block_dropped",
             "window_width_as_row_stride", "weights_of_another_set", "bias_of_another_set", "gram_of_image_0",
             "term_rounded_early"]


def term_needs_rounding(case, q):
    """some non-local term of set q (without x and the bias) is no fp16 number: rounding it early loses bits"""
    i = case_data(case)["ints"][q]
    for b in range(case.n):
        term = ((i["tw"] @ (i["phi"][b] @ i["tg"][b].T).T) @ i["theta"][b]) * STEP
        if (term.astype(np.float16).astype(np.float64) != term).any():
            return True
    return False


def mutation_applies(case, name, q, out, z=0):
    """has set q of the case the feature the mutation `name` is about?  (z: the Gram slice of the two slice mutations)"""
    h0, h1, w0, w1 = windows(case)[q]
    h, w = h1 - h0, w1 - w0
    N = h * w
    ns, jchunk = slices(case, N)
    return {"n_of_the_map": (h, w) != (case.FH, case.FW), "n_one_row_off": True, "n_one_column_off": True, "no_division": N > 1,
            "phi_g_exchanged": True, "p_transposed": True, "tail_tile_dropped": N % 64 != 0 and N > 64,
            "slice_dropped": ns > 1 and z * jchunk < N, "slice_twice": ns > 1 and z * jchunk < N,
            "c1_chunk_dropped": case.ci > KC, "c2_chunk_dropped": case.ci > KC, "gram_block_dropped": case.ci % 16 != 0 and case.ci > 16,
            "window_width_as_row_stride": w < case.FW and h > 1, "weights_of_another_set": len(windows(case)) > 1,
            "bias_of_another_set": len(windows(case)) > 1, "gram_of_image_0": case.n > 1, "term_rounded_early": out == "f16" and term_needs_rounding(case, q)}[name]


def reference(case, d, mutate=None, z=0, only=None):
    """float64 [n, cx, FH, FW]: `nonlocal_block` per set and image on the set's window, NaN where no set writes.
    mutate: one of MUTATIONS (a wrong kernel); only: the sets to evaluate (default: all)"""
    ci = case.ci
    out = np.full(d["x"].shape, np.nan)
    wins = windows(case)
    for q, win in enumerate(wins):
        h0, h1, w0, w1 = win
        h, w = h1 - h0, w1 - w0
        N = h * w
        if only is not None and q not in only:
            continue
        mut = mutate
        t = _tmap(case, d, q)
        tw = _walk_with_window_width(case, t, win) if mut == "window_width_as_row_stride" else t[:, :, h0:h1, w0:w1]
        o = (q + 1) % len(wins)
        wout = d["wout"][o if mut == "weights_of_another_set" else q]
        bout = d["bout"][o if mut == "bias_of_another_set" else q]
        ns, jchunk = slices(case, N)
        kw = {}
        if mut == "n_of_the_map":
            kw["divisor"] = case.FH * case.FW
        elif mut == "n_one_row_off":
            kw["divisor"] = (h + 1) * w
        elif mut == "n_one_column_off":
            kw["divisor"] = h * (w + 1)
        elif mut == "no_division":
            kw["divisor"] = 0
        elif mut in ("tail_tile_dropped", "slice_dropped", "slice_twice"):
            jw = np.ones(N)
            if mut == "tail_tile_dropped":
                jw[N // 64 * 64:] = 0
            else:
                jw[z * jchunk: (z + 1) * jchunk] = 0 if mut == "slice_dropped" else 2
            kw["jweight"] = jw
        elif mut == "c1_chunk_dropped":
            kw["c1mask"] = (np.arange(ci) < KC).astype(np.float64)
        elif mut == "c2_chunk_dropped":
            kw["c2mask"] = (np.arange(ci) < KC).astype(np.float64)
        elif mut == "gram_block_dropped":
            kw["c1mask"] = kw["c2mask"] = (np.arange(ci) < ci // 16 * 16).astype(np.float64)
        for b in range(case.n):
            x = d["x"][b, :, h0:h1, w0:w1]
            theta, phi, g = tw[b, :ci], tw[b, ci:2 * ci], tw[b, 2 * ci:3 * ci]
            if mut == "phi_g_exchanged":
                phi, g = g, phi
            if mut == "p_transposed":
                v = regrouped(x, theta, phi, g, wout, bout, p_transposed=True)
            elif mut == "gram_of_image_0" and b > 0:
                v = regrouped(x, theta, phi, g, wout, bout, gram_from=(tw[0, ci:2 * ci], tw[0, 2 * ci:3 * ci]))
            elif mut == "term_rounded_early":
                term = nonlocal_block(np.zeros_like(x), theta, phi, g, wout, np.zeros_like(bout))
                v = x + bout[:, None, None] + term.astype(np.float16).astype(np.float64)
            else:
                v = nonlocal_block(x, theta, phi, g, wout, bout, **kw)
            out[b, :, h0:h1, w0:w1] = v
    return out


def on_grid(v):
    """a float64 value of the exact regime -> the multiple of 2^-S it stands for (NaN stays NaN)"""
    r = np.rint(v / STEP) * STEP
    ok = np.isnan(v) | (np.abs(v - r) < 2.0 ** -30)
    assert ok.all(), "not a value of the exact regime: %g off the grid" % np.nanmax(np.abs(v - r))
    return r


_EXPECT = {}


def expected(case):
    """the exact value of every output element of the case (float64, NaN where no set writes), computed once"""
    if case.name not in _EXPECT:
        _EXPECT[case.name] = on_grid(reference(case, case_data(case)))
    return _EXPECT[case.name]


def integer_value(case, d):
    """the same value without a division: G = phi^T (g / N), M = tw G^T, out = x + b + 2^-S theta M^T, in int64"""
    out = np.full(d["x"].shape, np.nan)
    for q, (h0, h1, w0, w1) in enumerate(windows(case)):
        i = d["ints"][q]
        for b in range(case.n):
            G = i["phi"][b] @ i["tg"][b].T                               # [c1, c2], in units of N
            M = i["tw"] @ G.T                                            # [cx, c1]
            term = (M @ i["theta"][b]).astype(np.float64) * STEP         # [cx, N]
            out[b, :, h0:h1, w0:w1] = d["x"][b, :, h0:h1, w0:w1] + d["bout"][q][:, None, None] + term.reshape(-1, h1 - h0, w1 - w0)
    return out


def check_regime(case, d):
    """the conditions of the exact regime for the data of one case -> per set {N, K, mmax, ...} (asserts otherwise)"""
    stats = []
    for q, (h0, h1, w0, w1) in enumerate(windows(case)):
        i = d["ints"][q]
        N = i["N"]
        assert N == (h1 - h0) * (w1 - w0) and N <= 2048
        g16 = (i["tg"] * N).astype(np.float16)
        assert np.array_equal(g16.astype(np.int64), i["tg"] * N), "g = N * ternary is exact in fp16"
        a = lambda v: np.abs(v).astype(np.int64)
        mmax = 0
        for b in range(case.n):
            Gabs = a(i["phi"][b]) @ a(i["tg"][b]).T
            assert N * int(Gabs.max()) < LIMIT, "Gram: %d steps" % (N * int(Gabs.max()))
            fold = N * int((a(i["tw"]) @ Gabs.T).max())
            assert fold < LIMIT, "fold: %d steps" % fold
            M = i["tw"] @ (i["phi"][b] @ i["tg"][b].T).T
            mmax = max(mmax, int(np.abs(M).max()))
            apply_ = int((a(M) @ a(i["theta"][b])).max())
            assert apply_ < LIMIT, "apply: %d steps" % apply_
            term = np.abs(M @ i["theta"][b]).reshape(case.cx, h1 - h0, w1 - w0) * STEP
            adds = (np.abs(d["x"][b, :, h0:h1, w0:w1]) + np.abs(d["bout"][q])[:, None, None] + term) / STEP
            assert adds.max() < LIMIT, "final adds: %d steps" % adds.max()
        assert mmax > 0, "the block contributes"
        assert invn_exact(N, mmax), "fl32(N m * fl32(1 / N)) != m for some |m| <= %d at N = %d" % (mmax, N)
        stats.append({"N": N, "K": support_size(N, case.ci), "mmax": mmax})
    v = expected(case)
    v = v[~np.isnan(v)]
    assert np.abs(v).max() < 65504
    with np.errstate(over="ignore"):
        inexact = float((v.astype(np.float16).astype(np.float64) != v).mean())
    assert inexact >= 0.25, "only %.0f %% of the outputs exercise the fp16 rounding" % (100 * inexact)
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return stats, inexact


# ------------------------------------------------------------------------------------------------ the a-priori bound
def generic_reference_and_bound(case, d, mode):
    """continuous operands: (ref, bound, term), float64 [n, cx, FH, FW] (NaN where no set writes), with u = 2^-24
        A = (1 / N) sum_c1 |theta| sum_c2 |Wout| sum_j |phi| |g|
        B = 1.01 (N + 2 ci + 6) u A + 3 u (|x| + |bout| + |term|) + half an ulp of the output type at |ref|
    the first addend bounds the three float32 summations (N, ci and ci terms, in any order) and the rounding of 1 / N and
    of the product with it; the second the two final additions"""
    u = 2.0 ** -24
    ci = case.ci
    ref = reference(case, d)
    bound, term = np.full(ref.shape, np.nan), np.full(ref.shape, np.nan)
    ft = np.float16 if mode == "f16" else np.float32
    for q, (h0, h1, w0, w1) in enumerate(windows(case)):
        h, w = h1 - h0, w1 - w0
        N = h * w
        t = np.abs(_tmap(case, d, q)[:, :3 * ci, h0:h1, w0:w1]).reshape(case.n, 3 * ci, N)
        for b in range(case.n):
            G = t[b, ci:2 * ci] @ t[b, 2 * ci:].T                        # [c1, c2]
            A = ((np.abs(d["wout"][q]) @ G.T) @ t[b, :ci] / N).reshape(-1, h, w)
            x, r = d["x"][b, :, h0:h1, w0:w1], ref[b, :, h0:h1, w0:w1]
            bo = d["bout"][q][:, None, None]
            tm = r - x - bo
            half_ulp = np.spacing(np.abs(r).astype(ft)).astype(np.float64) / 2
            bound[b, :, h0:h1, w0:w1] = 1.01 * (N + 2 * ci + 6) * u * A + 3 * u * (np.abs(x) + np.abs(bo) + np.abs(tm)) + half_ulp
            term[b, :, h0:h1, w0:w1] = tm
    return ref, bound, term


# ------------------------------------------------------------------------------------------------------ the case lists
def _static(name, ci, cx, h, w, n, xkind, tkind, okind, extra=0):
    return Case(name, "static", n, ci, cx, h, w, ((0, h, 0, w),), None, 0, 3 * ci + extra, xkind, tkind, okind, len(name) + ci + cx + h * w)


def _multi(name, ci, cx, FH, FW, wins, n, xkind, tkind, okind, extra=0):
    return Case(name, "multi", n, ci, cx, FH, FW, tuple(wins), None, 0, 3 * ci + extra, xkind, tkind, okind, len(name) + ci + cx + FH * FW)


def _split(ci, cx, n, split, shift, xkind, tkind, okind, extra=0):
    name = "split-ci%d-c%d-n%d-%d.%d.%d-shift%d" % ((ci, cx, n) + tuple(split) + (shift,))
    return Case(name, "split", n, ci, cx, FULL[0] >> shift, FULL[1] >> shift, None, tuple(split), shift, 3 * ci + extra, xkind, tkind,
                okind, ci + cx + sum(split))


def quadrants(H, W):
    """the static quadrants of the neck: h // 2, w // 2 of the map, in the order lt, lb, rt, rb"""
    h, w = H // 2, W // 2
    return [(0, h, 0, w), (h, H, 0, w), (0, h, w, W), (h, H, w, W)]


STATIC_CASES = [
    #       name                     ci   cx   h   w  n  x / out place    tpg place  out (None: in place)
    _static("ci8-c8-4x5",             8,   8,  4,  5, 3, "dense",  "dense",  None),
    _static("ci16-c40-8x8",          16,  40,  8,  8, 1, "slice",  "slice",  "window"),
    _static("ci24-c30-5x13",         24,  30,  5, 13, 3, "slice",  "window", None),
    _static("ci64-c36-9x17-wide",    64,  36,  9, 17, 1, "window", "window", "slice", 8),
    _static("ci136-c200-13x21",     136, 200, 13, 21, 1, "dense",  "slice",  None),
    _static("ci264-c40-16x16",      264,  40, 16, 16, 1, "window", "dense",  "dense"),
    _static("ci64-c40-32x32",        64,  40, 32, 32, 1, "dense",  "dense",  None),
    _static("ci16-c8-25x41-odd",     16,   8, 25, 41, 1, "odd",    "odd",    "odd"),
    _static("ci64-c200-30x35",       64, 200, 30, 35, 1, "slice",  "dense",  None),
    _static("ci8-c36-1x127",          8,  36,  1, 127, 3, "dense", "odd",    "dense"),
    _static("ci64-c40-9x17-odd-x",   64,  40,  9, 17, 1, "odd",    "slice",  None),
    _static("ci64-c36-5x13-odd-t",   64,  36,  5, 13, 1, "window", "odd",    "dense"),
    _static("ci264-c30-4x5",        264,  30,  4,  5, 3, "dense",  "slice",  None),
    _static("ci24-c200-8x8-wide",    24, 200,  8,  8, 1, "dense",  "dense",  "slice", 8),
    _static("ci136-c8-5x13-odd",    136,   8,  5, 13, 1, "odd",    "odd",    None),
]
DOT_CASE = _static("dot-ci16-c40-5x13", 16, 40, 5, 13, 3, "dense", "dense", "dense")

MULTI_CASES = [
    _multi("quadrants-3x107-ci16-c40", 16, 40, 3, 107, quadrants(3, 107), 3, "window", "slice", None),
    _multi("quadrants-3x99-ci64-c36", 64, 36, 3, 99, quadrants(3, 99), 1, "slice", "odd", "window"),
    _multi("one-window-ci8-c8", 8, 8, 12, 30, [(2, 6, 3, 8)], 3, "dense", "dense", None),
    _multi("two-windows-ci64-c40", 64, 40, 17, 24, [(0, 4, 0, 5), (4, 17, 2, 23)], 1, "slice", "window", "dense"),
    _multi("three-windows-ci24-c30-odd", 24, 30, 16, 20, [(0, 5, 0, 13), (0, 4, 14, 19), (6, 15, 1, 18)], 3, "odd", "odd", None),
    _multi("four-windows-ci136-c200", 136, 200, 20, 30, [(0, 4, 0, 5), (0, 8, 8, 16), (8, 13, 0, 13), (9, 18, 13, 30)], 1, "window", "dense", None, 8),
]

SPLITS = [  # (split, shift): both clamps of every index (4 and extent - 4), cyl != cyr, no power-of-two window
    ((4, 5, 7), 0), ((12, 18, 22), 0), ((20, 32, 5), 0), ((20, 4, 31), 0), ((12, 18, 22), 1), ((20, 4, 12), 1), ((20, 32, 25), 1),
]
SPLIT_SHAPES = [(8, 8, 3, "dense", "dense", None), (16, 40, 1, "slice", "slice", "window"), (24, 30, 1, "slice", "window", None),
                (64, 36, 3, "window", "window", "slice", 8), (136, 200, 1, "dense", "slice", None), (264, 40, 1, "window", "dense", "dense"),
                (64, 40, 1, "odd", "odd", None)]
SPLIT_CASES = [_split(s[0], s[1], s[2], sp, sh, *s[3:]) for s, (sp, sh) in zip(SPLIT_SHAPES, SPLITS)]

ALL_CASES = STATIC_CASES + [DOT_CASE] + MULTI_CASES + SPLIT_CASES
GENERIC_CASES = {"static": [STATIC_CASES[2], STATIC_CASES[4], STATIC_CASES[7]], "multi": [MULTI_CASES[0], MULTI_CASES[4]],
                 "split": [SPLIT_CASES[0], SPLIT_CASES[3], SPLIT_CASES[4]]}


def assert_coverage():
    """every axis the kernels branch on occurs; raises at import of the test files otherwise"""
    st = STATIC_CASES
    assert {c.ci for c in st} == {8, 16, 24, 64, 136, 264} and {c.cx for c in st} == {8, 30, 36, 40, 200}
    assert {c.FH * c.FW for c in st} >= {20, 64, 65, 153, 127, 1024, 1025, 1050} and {c.FH * c.FW for c in st} & {256, 273}
    assert all(c.FW > 1 for c in st) and [c for c in st if c.FH == 1] == [c for c in st if c.FH * c.FW == 127]
    assert {c.n for c in st} == {1, 3} and {c.okind is None for c in st} == {True, False}
    assert {c.xkind for c in st} == {c.tkind for c in st} == {"dense", "slice", "window", "odd"}
    assert any(c.tw > 3 * c.ci for c in st)
    for group in (STATIC_CASES, MULTI_CASES, SPLIT_CASES):
        for dt in ("f16", "f32"):
            for p in ("vec", "vec_t", "vec_o"):
                assert {s[p] for c in group for s in predicates(c, dt)} == {True, False}, (group[0].kind, dt, p)
    assert any(predicates(c, "f32")[0]["vec_o"] and not predicates(c, "f16")[0]["vec_o"] for c in st if c.cx == 36)
    assert not any(s["vec_o"] for c in st if c.cx == 30 for dt in ("f16", "f32") for s in predicates(c, dt))
    assert {static_slices(c.FH * c.FW)[0] for c in st} == {1, 4, 8}
    empty = lambda c: any(z * slices(c, N)[1] >= N for N in [(w[1] - w[0]) * (w[3] - w[2]) for w in windows(c)] for z in range(slices(c, N)[0]))
    assert any(empty(c) for c in st) and all(empty(c) for c in SPLIT_CASES)
    assert {len(c.wins) for c in MULTI_CASES} == {1, 2, 3, 4} and {c.ci for c in MULTI_CASES} >= {8, 24, 64, 136}
    for c in MULTI_CASES:
        sizes = [(w[1] - w[0]) * (w[3] - w[2]) for w in c.wins]
        assert len(set(sizes)) == len(sizes) or len(sizes) == 1, "unequal extents"
    assert any(c.FH % 2 and c.FW % 2 and list(c.wins) == quadrants(c.FH, c.FW) for c in MULTI_CASES)
    assert any(min(s) < 64 and max(s) > 128 for s in [[(w[1] - w[0]) * (w[3] - w[2]) for w in c.wins] for c in MULTI_CASES])
    assert len(SPLIT_CASES) >= 6 and {c.shift for c in SPLIT_CASES} == {0, 1} and {c.ci for c in SPLIT_CASES} == {8, 16, 24, 64, 136, 264}
    H, W = FULL
    assert {c.split[0] for c in SPLIT_CASES} >= {4, H - 4} and {v for c in SPLIT_CASES for v in c.split[1:]} >= {4, W - 4}
    for c in SPLIT_CASES:
        sizes = [(w[1] - w[0]) * (w[3] - w[2]) for w in windows(c)]
        assert c.split[1] != c.split[2] and sum(sizes) == c.FH * c.FW
        assert all(good_window(N) and N & (N - 1) for N in sizes), (c.name, sizes)
    assert any(min((w[1] - w[0]) * (w[3] - w[2]) for w in windows(c)) < 64 for c in SPLIT_CASES)
    for c in ALL_CASES:
        assert c.ci % 8 == 0 and c.tw >= 3 * c.ci
        for q, w in enumerate(windows(c)):
            assert 0 <= w[0] < w[1] <= c.FH and 0 <= w[2] < w[3] <= c.FW


assert_coverage()
