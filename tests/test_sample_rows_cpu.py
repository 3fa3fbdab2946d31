"""CPU tests of the "max_num_embeddings" rule (include/sdhip.h: options, sd_sample_rows): the known answers of the key, the library's selection against
tests/sample_ref.py, the properties the header states (nested samples, stability under growth, uniformity), the refusals, the command line's usage
errors, and the reference of a sampled clustering call pinned on the fixtures of the reference's own Python."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import sdhip
from oracle import orc

import sample_ref as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")


def test_known_answers_of_the_key():
    assert sf.key(0, 0) == 5197578548964807871
    assert sf.key(0, 1) == 12035550249420947055
    assert sf.key(-1, 0) == 4922461756044938104
    assert sf.key(1, 0) == 15916886550466581944
    # ... and the library ranks by the same key: the one row kept of two is the one with the smaller key
    assert list(sdhip.sample_rows([0, 1], 1, 0)) == [0]
    for seed in (0, 1, -1):
        for i in range(0, 40, 2):
            want = i if sf.key(seed, i) < sf.key(seed, i + 1) else i + 1
            assert list(sdhip.sample_rows([i, i + 1], 1, seed)) == [want]


def test_library_selection_against_the_reference_on_random_cases():
    rng = np.random.default_rng(77)
    edge_seeds = (-2 ** 63, 2 ** 63 - 1, 0, -1)
    cases = [([], 1, 0), ([], -1, 5), ([3], 1, 0), (list(range(10)), 10, 3), (list(range(10)), 11, 3), (list(range(10)), -1, 3),
             (list(range(10)), 1, -2 ** 63), (list(range(10)), 1, 2 ** 63 - 1), ([0, 2 ** 31 - 1], 1, 9)]
    while len(cases) < 1000:
        n = int(rng.integers(0, 200))
        rows = np.sort(rng.choice(1000 if len(cases) % 2 else max(n, 1), n, replace=False)) if n else np.zeros(0, np.int64)      # with gaps / dense
        mx = int(rng.choice([1, max(n - 1, 1), n + 1, int(rng.integers(1, 220)), -1]))
        seed = int(rng.choice(edge_seeds)) if len(cases) % 7 == 0 else int(rng.integers(-2 ** 63, 2 ** 63 - 1, dtype=np.int64))
        cases.append(([int(r) for r in rows], mx, seed))
    seen_cut = 0
    for rows, mx, seed in cases:
        got = sdhip.sample_rows(rows, mx, seed)
        want = sf.sample(rows, mx, seed)
        assert got.dtype == np.int32 and list(got) == want, (rows, mx, seed)
        assert len(want) == (len(rows) if mx == -1 else min(len(rows), mx))
        seen_cut += len(want) < len(rows)
    assert seen_cut > 300


def test_samples_are_nested():
    rows = list(range(0, 600, 3))
    for seed in (0, 7, -5):
        prev = set()
        for m in range(1, len(rows) + 2):
            cur = set(sdhip.sample_rows(rows, m, seed).tolist())
            assert prev <= cur and len(cur) == min(m, len(rows))
            prev = cur


def test_appending_a_row_removes_at_most_one():
    prev = set(sdhip.sample_rows(list(range(100)), 20, 7).tolist())
    changed = 0
    for n in range(101, 401):
        cur = set(sdhip.sample_rows(list(range(n)), 20, 7).tolist())
        assert len(prev - cur) <= 1 and cur - prev <= {n - 1}
        changed += bool(prev - cur)
        prev = cur
    assert changed >= 5                     # (the sample does move: 20 / n of the appended rows enter it)


@pytest.mark.parametrize("m,n,seeds", [(10, 50, range(0, 2000)), (10, 50, range(-1000, 1000)), (15, 60, range(5000, 7000))])
def test_every_row_is_selected_about_equally_often(m, n, seeds):
    rows = list(range(n))
    count = np.zeros(n)
    for seed in seeds:
        count[sdhip.sample_rows(rows, m, seed)] += 1
    p, trials = m / n, len(seeds)
    dev = np.abs(count - trials * p) / np.sqrt(trials * p * (1 - p))
    print("%d of %d over %d seeds: largest deviation %.2f standard deviations" % (m, n, trials, dev.max()))
    assert dev.max() <= 4.0


def test_refusals():
    for bad in (0, -2):
        with pytest.raises(sdhip.SdError) as e:
            sdhip.sample_rows([1, 2, 3], bad, 0)
        assert e.value.code == 1 and "max_num" in str(e.value)
    for rows in ([2, 1], [1, 1], [-1, 0]):      # not ascending, not distinct, negative
        with pytest.raises(sdhip.SdError):
            sdhip.sample_rows(rows, 1, 0)
    # the option itself needs a context, which needs a GPU: its refusals (0 and -2, with the message) are asserted in tests/test_sampled_clustering.py


def test_command_line_usage_errors():
    for args in (["--max-num-embeddings"], ["--max-num-embeddings", "0"], ["--max-num-embeddings", "-2"], ["--max-num-embeddings", "12x"],
                 ["--max-num-embeddings", "99999999999999999999"], ["--max-num-embeddings", "100", "--dump-steps", "/tmp"], ["--clustering-seed"], ["--clustering-seed", "1.5"], ["--clustering-seed", "abc"]):
        out = subprocess.run([EXE, "seg.sdw", "emb.sdw", "a.wav"] + args, capture_output=True, text=True, timeout=60)
        assert out.returncode == 2 and out.stderr.startswith("usage: "), (args, out.returncode, out.stderr)
    # good values pass the argument check: the run then ends where it would without them (no GPU here, or no such model file)
    out = subprocess.run([EXE, "seg.sdw", "emb.sdw", "a.wav", "--max-num-embeddings", "-1", "--clustering-seed", "-9223372036854775808"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 1 and not out.stderr.startswith("usage: ")


def test_reference_with_a_sample_that_holds_every_row_is_the_oracle(golden_dir):
    path = os.path.join(golden_dir, "ref_clustering.npz")
    want = open(os.path.join(golden_dir, "ref_clustering.sha256")).read().split()[0]
    assert hashlib.sha256(open(path, "rb").read()).hexdigest() == want
    gold = np.load(path)
    for name in gold["cases"]:
        emb = gold["%s_q" % name].astype(np.float64) / 64.0
        emb[gold["%s_nan" % name]] = np.nan
        nc, mn, mx, constrained = [int(v) for v in gold["%s_kw" % name]]
        kw = {"num_clusters": nc, "min_clusters": mn, "max_clusters": mx}
        L = len(sf.train_rows(emb))
        hard, K, _ = orc.clustering_full(emb, constrained=bool(constrained), **kw)
        assert np.array_equal(hard, gold["%s_hard" % name])
        for m in (L, L + 1, -1):
            got = sf.sampled_clustering(emb, m, seed=3, constrained=bool(constrained), **kw)
            assert got["K"] == K and np.array_equal(got["hard"], hard), (name, m)
            assert len(got["selected"]) == L and got["counts"].sum() == L
        if L > 4 and not constrained:
            # ... and below L it is another job: the centroids are means of the sample alone, yet every row still gets a label
            part = sf.sampled_clustering(emb, L // 2, seed=3, **kw)
            assert part["counts"].sum() == L // 2 and part["hard"].shape == hard.shape
