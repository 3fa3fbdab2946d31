"""Exact reference of sd_der (include/sdhip.h): the rule of pyannote.metrics' DiarizationErrorRate in rational arithmetic.  Every input double is
taken as the fraction it is, every interval length and every sum is exact; the one-to-one mapping is found by trying every pairing, which limits
the reference to cases with at most 6 labels a side.  The only f64 operation is the one the header names: the edges of a collar zone are the f64
values t - collar / 2 and t + collar / 2.  tests/test_der_ref.py pins this file on hand-computed cases and against scipy's assignment solver."""
import itertools
from fractions import Fraction

import numpy as np

COMPONENTS = ("total", "missed", "false_alarm", "confusion", "correct")
MAX_LABELS = 6


def _intervals(ref, hyp, uem, collar, skip_overlap):
    """the scored elementary intervals in ascending time: [(D, A, B)] with D a Fraction, A / B the frozensets of labels that are on"""
    ref = [(float(a), float(b), int(k)) for a, b, k in ref]
    hyp = [(float(a), float(b), int(k)) for a, b, k in hyp]
    zones = []
    if collar > 0:
        for a, b, _ in ref:
            for t in (a, b):
                zones.append((t - float(collar) / 2, t + float(collar) / 2))          # f64, as the header says
    spans = None if uem is None else [(float(t[0]), float(t[1])) for t in uem]
    cuts = sorted({x for a, b, _ in ref + hyp for x in (a, b)} | {x for z in zones for x in z} | {x for z in (spans or []) for x in z})
    out = []
    for x0, x1 in zip(cuts, cuts[1:]):                   # (comparisons of doubles are exact; only lengths and sums need fractions)
        inside = lambda a, b: a <= x0 and x1 <= b
        if spans is not None and not any(inside(a, b) for a, b in spans):
            continue
        if any(inside(a, b) for a, b in zones):
            continue
        A = frozenset(k for a, b, k in ref if inside(a, b))
        B = frozenset(k for a, b, k in hyp if inside(a, b))
        if (not A and not B) or (skip_overlap and len(A) >= 2):
            continue
        out.append((Fraction(x1) - Fraction(x0), A, B))
    return out


def cooccurrence(ref, hyp, uem=None, collar=0.0, skip_overlap=False):
    """(reference labels, hypothesis labels, {(a, b): exact co-occurrence duration over the scored intervals})"""
    iv = _intervals(ref, hyp, uem, collar, skip_overlap)
    R = sorted({int(t[2]) for t in ref})
    H = sorted({int(t[2]) for t in hyp})
    co = {(a, b): Fraction(0) for a in R for b in H}
    for D, A, B in iv:
        for a in A:
            for b in B:
                co[(a, b)] += D
    return R, H, co


def best_mapping(R, H, co):
    """({reference label: hypothesis label}, its summed co-occurrence): every one-to-one pairing tried"""
    assert len(R) <= MAX_LABELS and len(H) <= MAX_LABELS, "brute force: at most %d labels a side" % MAX_LABELS
    small, large, flip = (R, H, False) if len(R) <= len(H) else (H, R, True)
    best, best_val = {}, Fraction(-1)
    for perm in itertools.permutations(large, len(small)):
        val = sum((co[(p, s)] if flip else co[(s, p)]) for s, p in zip(small, perm))
        if val > best_val:
            best_val, best = val, ({p: s for s, p in zip(small, perm)} if flip else dict(zip(small, perm)))
    return best, max(best_val, Fraction(0))


def components_for(iv, r2h):
    c = dict.fromkeys(COMPONENTS, Fraction(0))
    for D, A, B in iv:
        ok = sum(1 for a in A if r2h.get(a) in B)
        c["total"] += len(A) * D
        c["missed"] += max(0, len(A) - len(B)) * D
        c["false_alarm"] += max(0, len(B) - len(A)) * D
        c["correct"] += ok * D
        c["confusion"] += (min(len(A), len(B)) - ok) * D
    return c


def der(ref, hyp, uem=None, collar=0.0, skip_overlap=False):
    """the exact components (Fractions), der (a Fraction, None when total == 0), n = the scored elementary intervals, extent = their summed length,
    map = {hypothesis label: reference label} of one optimal pairing"""
    iv = _intervals(ref, hyp, uem, collar, skip_overlap)
    R, H, co = cooccurrence(ref, hyp, uem, collar, skip_overlap)
    r2h, _ = best_mapping(R, H, co)
    r2h = {a: b for a, b in r2h.items() if co[(a, b)] > 0}
    out = components_for(iv, r2h)
    out["der"] = (out["missed"] + out["false_alarm"] + out["confusion"]) / out["total"] if out["total"] > 0 else None
    out["n"] = len(iv)
    out["extent"] = sum((D for D, _, _ in iv), Fraction(0))
    out["map"] = {b: a for a, b in r2h.items()}
    return out


def correct_of(ref, hyp, h2r, uem=None, collar=0.0, skip_overlap=False):
    """exact `correct` under a given mapping {hypothesis label: reference label}"""
    iv = _intervals(ref, hyp, uem, collar, skip_overlap)
    return components_for(iv, {a: b for b, a in h2r.items()})["correct"]


# ---- the cases both test files run
def hand_cases():
    """name -> (ref, hyp, options, expected exact components as floats that are exact in binary)"""
    return {
        "empty hypothesis": ([(0.0, 10.0, 0)], [], {}, dict(total=10, missed=10, false_alarm=0, confusion=0, correct=0)),
        "permuted labels": ([(0.0, 4.0, 0), (4.0, 9.0, 1), (9.0, 12.0, 2), (12.0, 13.0, 0)], [(0.0, 4.0, 5), (4.0, 9.0, 0), (9.0, 12.0, 1), (12.0, 13.0, 5)], {},
                            dict(total=13, missed=0, false_alarm=0, confusion=0, correct=13)),
        "overlap, one hypothesised": ([(0.0, 6.0, 0), (4.0, 10.0, 1)], [(0.0, 6.0, 0)], {}, dict(total=12, missed=6, false_alarm=0, confusion=0, correct=6)),
        "overlap, one speaker throughout": ([(0.0, 10.0, 0), (4.0, 6.0, 1)], [(0.0, 10.0, 3)], {}, dict(total=12, missed=2, false_alarm=0, confusion=0, correct=10)),
        "collar swallows a short turn": ([(0.0, 10.0, 0), (12.0, 12.25, 1), (14.0, 20.0, 0)], [(0.0, 20.0, 0)], dict(collar=0.5),
                                         dict(total=9.75 - 0.25 + 19.75 - 14.25, missed=0, false_alarm=(11.75 - 10.25) + (13.75 - 12.5), confusion=0, correct=9.5 + 5.5)),
        "skip overlap": ([(0.0, 6.0, 0), (4.0, 10.0, 1)], [(0.0, 5.0, 0), (5.0, 10.0, 1)], dict(skip_overlap=True), dict(total=8, missed=0, false_alarm=0, confusion=0, correct=8)),
        "uem cuts a turn": ([(0.0, 10.0, 0), (10.0, 20.0, 1)], [(0.0, 12.0, 0), (12.0, 20.0, 1)], dict(uem=[(5.0, 11.0), (15.0, 30.0)]),
                            dict(total=11, missed=0, false_alarm=0, confusion=1, correct=10)),
        "false alarm and confusion": ([(0.0, 4.0, 0), (6.0, 10.0, 1)], [(0.0, 5.0, 2), (5.0, 10.0, 2)], {}, dict(total=8, missed=0, false_alarm=2, confusion=4, correct=4)),
    }


def random_case(seed):
    """(ref, hyp, options): 1-6 labels a side, 0-60 turns a side, times on the 1/16000 s grid within 120 s, overlapping turns of one label included; two
    cases in five carry a uem, a collar or skip_overlap"""
    rng = np.random.default_rng(seed)

    def side():
        labels = rng.choice(40, size=int(rng.integers(1, MAX_LABELS + 1)), replace=False)
        turns = []
        for _ in range(int(rng.integers(0, 61))):
            a = int(rng.integers(0, 120 * 16000))
            b = min(120 * 16000, a + int(rng.integers(0, 12 * 16000)))
            turns.append((a / 16000.0, b / 16000.0, int(rng.choice(labels))))
        return turns

    ref, hyp = side(), side()
    if rng.random() < 0.3 and ref:                       # a hypothesis that follows the reference: boundaries that coincide, high correct
        perm = rng.permutation(40)
        hyp = [(a, b, int(perm[k])) for a, b, k in ref if rng.random() < 0.8] + hyp[:5]
        keep = sorted({q[2] for q in hyp})[:MAX_LABELS]
        hyp = [t for t in hyp if t[2] in keep]
    opt = {}
    if rng.random() < 0.4:
        kind = int(rng.integers(0, 3))
        if kind == 0:
            edges = np.sort(rng.integers(0, 125 * 16000, size=4)) / 16000.0
            opt["uem"] = [(float(edges[0]), float(edges[1])), (float(edges[2]), float(edges[3]))]
        elif kind == 1:
            opt["collar"] = float(rng.choice([0.25, 0.5, 0.1]))
        else:
            opt["skip_overlap"] = True
    return ref, hyp, opt
