"""CPU proof that the cases of tests/test_nonlocal_exact.py can tell a wrong non-local kernel from the right one.

For every case of tests/nonlocal_reference.py: the conditions of the exact regime hold (so every float32 step of the
kernels is exact and the output is the float64 value rounded once), the definition-order float64 value equals an
evaluation in integers that never divides, and a float32 evaluation in three orders reproduces it bit for bit.  For every
mistake a kernel could plausibly make (MUTATIONS), the mutated reference differs in bits from the right one on EVERY
window that has the feature, in both output types; an invN one float32 ulp off changes bits as well."""
import numpy as np
import pytest

from tests import nonlocal_reference as R

OUTS = ["f16", "f32"]


def _bits(v, out):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(np.float16 if out == "f16" else np.float32).view(np.int16 if out == "f16" else np.int32)


def _window(a, win):
    return a[:, :, win[0]:win[1], win[2]:win[3]]


def test_the_case_lists_cover_what_they_claim():
    R.assert_coverage()
    names = [c.name for c in R.ALL_CASES]
    assert len(set(names)) == len(names)
    assert all(c in R.ALL_CASES for group in R.GENERIC_CASES.values() for c in group)
    # the 1 / N step: the good and the bad window sizes the regime was chosen around
    assert all(R.good_window(N) for N in (9, 20, 21, 35, 45, 49, 65, 77, 81, 127, 129, 135, 143, 153, 187, 257, 273, 299, 323, 1023, 1025, 1050))
    assert all(R.good_window(1 << k) for k in range(12))
    assert not any(R.good_window(N) for N in (7, 15, 30, 60, 63, 117, 120, 255, 1000))


@pytest.mark.parametrize("case", R.ALL_CASES, ids=lambda c: c.name)
def test_the_regime_holds_and_the_definition_equals_the_integer_value(case):
    d = R.case_data(case)
    stats, inexact = R.check_regime(case, d)
    print("%s: %s; %.0f %% of the outputs are no fp16 numbers" % (case.name, stats, 100 * inexact))
    want, got = R.integer_value(case, d), R.expected(case)
    assert np.array_equal(np.isnan(want), np.isnan(got)) and np.array_equal(want[~np.isnan(want)], got[~np.isnan(got)])
    for q, win in enumerate(R.windows(case)):                            # no NaN of the poisoned surroundings inside a window
        assert not np.isnan(_window(got, win)).any()
        assert R.good_window(stats[q]["N"], stats[q]["mmax"])
    if case.kind == "split":                                             # every pixel of the map is written exactly once
        assert not np.isnan(got).any()
        assert sum((w[1] - w[0]) * (w[3] - w[2]) for w in R.windows(case)) == case.FH * case.FW


# ------------------------------------------------------------------------------------------- float32, in three orders
def _sum32(terms, order, chunk):
    """float32 sum over axis 0, one addition at a time: forward, reversed, or chunk by chunk with the partial sums added last"""
    t = np.ascontiguousarray(terms, np.float32)
    if order == "reversed":
        t = t[::-1]
    if order != "chunked":
        return np.cumsum(t, 0, dtype=np.float32)[-1]
    parts = [np.cumsum(t[i:i + chunk], 0, dtype=np.float32)[-1] for i in range(0, len(t), chunk)]
    return np.cumsum(np.stack(parts), 0, dtype=np.float32)[-1]


def _float32_value(case, d, q, b, order):
    """the kernels' three stages in float32 arithmetic on set q, image b -> float64 [cx, h, w]"""
    h0, h1, w0, w1 = R.windows(case)[q]
    N, ci = (h1 - h0) * (w1 - w0), case.ci
    t = R._tmap(case, d, q)[b, :3 * ci, h0:h1, w0:w1].reshape(3 * ci, N).astype(np.float32)
    theta, phi, g = t[:ci], t[ci:2 * ci], t[2 * ci:]
    live = np.nonzero((phi != 0).any(0) | (g != 0).any(0))[0]            # a zero term changes no float32 sum
    ns, jchunk = R.slices(case, N)
    if order == "chunked":                                               # slice by slice, the slices added in order
        parts = [np.cumsum(phi[:, j][:, None, :].T * g[:, j][None, :, :].T, 0, dtype=np.float32)[-1]
                 for j in (live[(live >= z * jchunk) & (live < (z + 1) * jchunk)] for z in range(ns)) if len(j)]
        G = np.cumsum(np.stack(parts), 0, dtype=np.float32)[-1]          # [c2, c1]
    else:
        G = _sum32(phi[:, live][:, None, :].T * g[:, live][None, :, :].T, order, 0)
    G = G.T                                                              # [c1, c2]
    w32 = d["wout"][q].astype(np.float32)
    acc = _sum32(np.moveaxis(w32[:, None, :] * G[None, :, :], 2, 0), order, R.KC)       # terms [c2][cx][c1]
    P = acc * (np.float32(1.0) / np.float32(N))
    out = np.empty((case.cx, N), np.float32)
    for i0 in range(0, N, 128):
        terms = theta[:, i0:i0 + 128].T[None, :, :] * P[:, None, :]      # [cx, pixels, c1]
        out[:, i0:i0 + 128] = _sum32(np.moveaxis(terms, 2, 0), order, R.KC)
    x32 = d["x"][b, :, h0:h1, w0:w1].reshape(case.cx, N).astype(np.float32)
    v = (x32 + d["bout"][q].astype(np.float32)[:, None]) + out
    return v.astype(np.float64).reshape(case.cx, h1 - h0, w1 - w0)


@pytest.mark.parametrize("case", R.ALL_CASES, ids=lambda c: c.name)
def test_float32_in_three_orders_gives_the_float64_value(case):
    d = R.case_data(case)
    want = R.expected(case)
    for q, win in enumerate(R.windows(case)):
        b = q % case.n
        for order in ("forward", "reversed", "chunked"):
            assert np.array_equal(_float32_value(case, d, q, b, order), _window(want, win)[b]), (q, order)


# -------------------------------------------------------------------------------------------------------- the mutations
@pytest.mark.parametrize("name", R.MUTATIONS)
def test_every_mutation_is_visible_on_every_window_that_has_the_feature(name):
    seen = 0
    for case in R.ALL_CASES:
        d = R.case_data(case)
        right = R.expected(case)
        for q, win in enumerate(R.windows(case)):
            N = (win[1] - win[0]) * (win[3] - win[2])
            for z in (range(R.slices(case, N)[0]) if name.startswith("slice_") else [0]):
                applies = [o for o in OUTS if R.mutation_applies(case, name, q, o, z)]
                if not applies:
                    continue
                wrong = _window(R.reference(case, d, mutate=name, z=z, only=[q]), win)
                if name == "gram_of_image_0":
                    wrong, ok = wrong[1:], _window(right, win)[1:]
                else:
                    ok = _window(right, win)
                for out in applies:
                    seen += 1
                    assert (_bits(wrong, out) != _bits(ok, out)).any(), "%s is invisible on %s set %d slice %d in %s" % (name, case.name, q, z, out)
    assert seen >= 4, "no case has the feature of %s" % name


def test_a_mutation_of_one_set_is_not_needed_to_change_the_others():
    """(the harness of the check above: the unmutated evaluation of a single set equals the expected value there)"""
    case = R.MULTI_CASES[1]
    for q, win in enumerate(R.windows(case)):
        got = R.on_grid(_window(R.reference(case, R.case_data(case), only=[q]), win))
        assert np.array_equal(got, _window(R.expected(case), win))


INVN_CASES = [c for c in (R.STATIC_CASES[3], R.STATIC_CASES[8], R.SPLIT_CASES[0], R.SPLIT_CASES[1])]


@pytest.mark.parametrize("case", INVN_CASES, ids=lambda c: c.name)
def test_an_invn_one_ulp_off_changes_bits(case):
    """nl_window divides on the device, the static path on the host: both must give the correctly rounded float32 quotient"""
    d = R.case_data(case)
    kinds = {c.kind for c in INVN_CASES}
    assert kinds == {"static", "split"}
    for q, win in enumerate(R.windows(case)):
        h0, h1, w0, w1 = win
        N = (h1 - h0) * (w1 - w0)
        assert N & (N - 1), "a power of two has an exact reciprocal"
        inv = np.float32(1.0) / np.float32(N)
        ci = case.ci
        t = R._tmap(case, d, q)[0, :, h0:h1, w0:w1]
        args = (d["x"][0, :, h0:h1, w0:w1], t[:ci], t[ci:2 * ci], t[2 * ci:3 * ci], d["wout"][q], d["bout"][q])
        right = _window(R.expected(case), win)[0]
        assert np.array_equal(R.regrouped(*args, invn=inv), right)
        for off in (np.nextafter(inv, np.float32(0)), np.nextafter(inv, np.float32(1))):
            wrong = R.regrouped(*args, invn=off)
            for out in OUTS:
                assert (_bits(wrong, out) != _bits(right, out)).any(), (case.name, q, float(off), out)


def test_the_generic_cases_have_a_term_that_contributes_and_a_finite_bound():
    """the a-priori bound B of tests/nonlocal_reference.py generic_reference_and_bound on the continuous operands of the GPU
    tests: defined on every written element, and the non-local term is not lost beside x and the bias"""
    for group in R.GENERIC_CASES.values():
        for case in group:
            for mode in ("f32", "f16"):
                ref, bound, term = R.generic_reference_and_bound(case, R.generic_data(case, mode, 1), mode)
                inside = ~np.isnan(ref)
                assert np.array_equal(inside, ~np.isnan(bound)) and (bound[inside] > 0).all() and np.isfinite(bound[inside]).all()
                assert np.nanmax(np.abs(term)) > 0.25
                print("%s %s: median bound %.2e, max |ref| %.2f" % (case.name, mode, np.median(bound[inside]), np.nanmax(np.abs(ref))))
