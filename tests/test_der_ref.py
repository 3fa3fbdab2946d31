"""CPU tests that pin tests/der_ref.py, the exact reference sd_der is held against (tests/test_der.py): hand-computed cases of every option, and the
brute-force mapping against scipy's assignment solver."""
from fractions import Fraction

import numpy as np
import pytest

import der_ref as dr


@pytest.mark.parametrize("name", sorted(dr.hand_cases()))
def test_hand_computed_cases(name):
    ref, hyp, opt, want = dr.hand_cases()[name]
    got = dr.der(ref, hyp, **opt)
    for k in dr.COMPONENTS:
        assert got[k] == Fraction(want[k]), (name, k, got[k], want[k])
    assert got["der"] == Fraction(want["missed"] + want["false_alarm"] + want["confusion"]) / Fraction(want["total"])
    assert got["total"] == got["correct"] + got["confusion"] + got["missed"]


def test_the_named_properties():
    c = dr.hand_cases()
    one = dr.der(*c["empty hypothesis"][:2])
    assert one["der"] == 1 and one["missed"] == one["total"] == 10 and one["map"] == {}
    perm = dr.der(*c["permuted labels"][:2])
    assert perm["der"] == 0 and perm["map"] == {5: 0, 0: 1, 1: 2}
    ov = dr.der(*c["overlap, one speaker throughout"][:2])
    assert ov["missed"] == 2                                      # the overlap length
    ref, hyp, opt, _ = c["collar swallows a short turn"]
    assert dr.der(ref, hyp)["total"] == Fraction(16.25) and dr.der(ref, hyp, **opt)["total"] == 15      # the 0.25 s turn is gone, and 0.25 s at each of four edges
    ref, hyp, opt, _ = c["skip overlap"]
    assert dr.der(ref, hyp)["total"] == 12 and dr.der(ref, hyp, **opt)["n"] == 2
    ref, hyp, opt, _ = c["uem cuts a turn"]
    assert dr.der(ref, hyp)["confusion"] == 2 and dr.der(ref, hyp, **opt)["confusion"] == 1
    nothing = dr.der([], [])
    assert nothing["der"] is None and nothing["total"] == 0 and nothing["n"] == 0
    only_fa = dr.der([], [(1.0, 3.0, 4)])
    assert only_fa["der"] is None and only_fa["false_alarm"] == 2


def test_brute_force_mapping_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    for seed in range(200):
        ref, hyp, o = dr.random_case(10_000 + seed)
        R, H, co = dr.cooccurrence(ref, hyp, **o)
        if not R or not H:
            continue
        _, best = dr.best_mapping(R, H, co)
        # scipy works on the co-occurrences rounded to f64 (each below 2^7 s, so rounded by at most 2^-47): the pairing it finds is optimal for the
        # rounded matrix, and its exact value is within twice that rounding per pair of the exact optimum
        mf = np.array([[float(co[(a, b)]) for b in H] for a in R])
        r, c = opt.linear_sum_assignment(mf, maximize=True)
        got = sum(co[(R[i], H[j])] for i, j in zip(r, c))
        assert best - got <= 2 * min(len(R), len(H)) * Fraction(1, 2 ** 47), (seed, float(got), float(best))
        assert got <= best
