"""CPU tests of the enrolled-flow reference (tests/enrolled_ref.py): pinned to the oracle where nobody is claimed, to the arg-max over the used
voiceprints where everybody is, and told apart from four plausible wrong rules by the committed cases."""
import numpy as np
import pytest

from oracle import orc

import enrolled_ref as er
import speakers_ref as sr


def _result(r):
    return r["K"], r["hard"].tobytes(), r["counts"].tobytes(), r["enrolled"].tobytes(), np.nan_to_num(r["centroids"], nan=-7.0).tobytes()


@pytest.mark.parametrize("small", [0, 5])
def test_nobody_claimed_is_the_oracles_plain_job(small):
    emb = sr.planted_embeddings(small=small)
    hard, K, tl = orc.clustering(emb)
    cen, cnt = sr.centroids(emb, tl)
    for gal, t in ((er.far_row(cen), 0.0), (er.far_row(cen), 0.5), (np.vstack([er.far_row(cen), -cen[0:1]]), 0.5)):
        r = er.clustering(emb, gal, t)
        assert r["G"] == 0 and not r["claimed"].any() and r["dist"].min() > t
        assert r["K"] == K == 3 and np.array_equal(r["hard"], hard) and np.array_equal(r["train_labels"], tl)
        assert np.array_equal(r["centroids"], cen) and np.array_equal(r["counts"], cnt) and list(r["enrolled"]) == [-1] * K


@pytest.mark.parametrize("name", ["closed", "closed small", "duplicates"])
def test_closed_set_is_the_arg_max_over_the_used_voiceprints(name):
    emb, gal, t = er.case(name)
    assert t == 2.0
    r = er.clustering(emb, gal, t)
    flat = emb.reshape(-1, sr.DIM)
    ok = ~np.isnan(flat[:, 0])
    U = [int(m) for m in r["enrolled"]]
    assert r["claimed"].all() and r["L"] == 0 and r["n_unclaimed"] == 0 and r["K"] == r["G"] == len(U) == 3 and min(U) >= 0
    D = sr.cosine_distances(flat[ok], gal[U])
    assert np.array_equal(r["hard"].reshape(-1)[ok], np.argmax(2.0 - D, 1)) and not r["hard"].reshape(-1)[~ok].any()
    assert np.array_equal(r["centroids"], gal[U]) and r["counts"].sum() == ok.sum()
    if name == "duplicates":
        assert U == [0, 1, 3]                                                 # rows 2 and 4 repeat rows 0 and 1: never the first minimum


def test_the_cases_cover_what_the_gpu_tests_rely_on():
    facts = {n: er.clustering(*er.case(n)) for n in er.CASES}
    h = facts["hybrid"]
    assert 0 < h["claimed"].sum() < h["N"] and h["G"] == 2 and h["L"] >= 1 and list(h["enrolled"][:2]) == [0, 1]
    assert facts["hybrid small"]["to_enrolled"] >= 1 and facts["partial"]["to_enrolled"] >= 1      # a small leftover cluster goes to a voiceprint
    assert facts["partial"]["L"] >= 2
    assert facts["one row"]["claimed"].sum() == 1 and facts["one row"]["dist"].min() == er.case("one row")[2]
    assert facts["one left"]["n_unclaimed"] == 1 and facts["closed"]["n_unclaimed"] == 0
    assert facts["far"]["G"] == 0 and facts["far small"]["G"] == 0
    t = facts["tie small"]
    assert t["G"] == 1 and t["claimed"].sum() == 1 and t["L"] == 3


@pytest.mark.parametrize("mistake", er.MISTAKES)
def test_each_wrong_rule_changes_a_committed_case(mistake):
    changed = [n for n in er.CASES if _result(er.clustering(*er.case(n))) != _result(er.clustering(*er.case(n), mistake=mistake))]
    assert changed, mistake
    expect = {"last minimum": "duplicates", "strict claim": "one row", "mcs from unclaimed": "hybrid small", "candidates reversed": "tie small"}[mistake]
    assert expect in changed


def test_normalisation_rounds_the_norm_to_float32():
    X = np.random.default_rng(3).standard_normal((7, 192))
    Xn = er.normalize_f32(X)
    nrm = np.sqrt(er.sequential_sqnorm(X))
    assert np.array_equal(Xn, X / nrm.astype(np.float32).astype(np.float64)[:, None]) and not np.array_equal(Xn, X / nrm[:, None])
    # ... which is what the oracle's own clustering does before its linkage: the same labels on the same rows
    emb = sr.planted_embeddings()
    flat = emb.reshape(-1, sr.DIM)
    rows = flat[~np.isnan(flat[:, 0])]
    lab, K = orc.cluster_embeddings(rows, min_cluster_size=1)
    assert np.array_equal(orc.ahc(er.normalize_f32(rows), float(orc.THRESH_F32))[0] - 1, lab) and K == lab.max() + 1
