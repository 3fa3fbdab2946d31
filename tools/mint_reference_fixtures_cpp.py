"""Records the answers of the reference's compiled code (oracle/_ref: clustering.cpp, WavReader, the speakerDiarizer.cpp glue) for
every call the tests make of it, into tests/golden/ref_cpp_calls.npz.  Where oracle/_ref is absent -- every machine without the
reference tree -- oracle/orc.py replays them, keyed by a hash of each call's inputs.

Run where the reference tree exists, after build():   python tools/mint_reference_fixtures_cpp.py
The CPU tests that call the reference are run in this process with recording on; the calls the GPU tests of
tests/test_reference_cpp_glue.py make of the reference (none of which needs a GPU itself) are made here with the same inputs."""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)
os.environ["SD_REF_RECORD"] = "1"

import numpy as np  # noqa: E402
import pytest  # noqa: E402

from oracle import orc  # noqa: E402


def gpu_test_calls():
    """the reference calls of test_hip_finalize_gives_the_reference_cpp_turns and test_hip_stage_entry_points_against_the_reference_cpp"""
    spec = importlib.util.spec_from_file_location("tcg", os.path.join(ROOT, "tests", "test_reference_cpp_glue.py"))
    t = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(t)
    G = orc.RefGlue()
    for seconds in (600.0, 3600.0):
        pcm, scores, e32, n, nc = t.planted(seconds)
        G.finalize(scores, e32.astype(np.float64), n)
    rng = np.random.default_rng(77)
    c = 120
    seg = t.rng_scores(rng, c)
    n = (c - 1) * 8000 + 80000 + 555
    b_ref = G.binarize(seg)
    G.select_masks(b_ref)
    G.speaker_count(b_ref, n)
    for seed in range(12):
        X = t.loose_set(seed)
        cc = -(-len(X) // 3)
        emb = np.full((cc * 3, 192), np.nan)
        emb[:len(X)] = X
        G.clustering(emb.reshape(cc, 3, 192))
        if t.python_rule_labels(X) is not None:
            G.cluster_embeddings(X)
    seg, b, hard, n = t.random_job(9, 150, tail=321)
    cnt_ref, win_ref = G.speaker_count(b, n)
    bin_ref, fr = G.reconstruct(seg, hard, cnt_ref, win_ref, n)
    G.to_annotation(bin_ref, fr[0])


def main():
    if orc.refglue() is None or orc.ref() is None:
        raise SystemExit("oracle/_ref is not built: run build() where the reference tree exists")
    rc = pytest.main(["-q", "-p", "no:cacheprovider", "-m", "not gpu", os.path.join(ROOT, "tests", "test_reference_cpp_glue.py"),
                      os.path.join(ROOT, "tests", "test_oracle.py") + "::test_linkage_vs_scipy_and_reference",
                      os.path.join(ROOT, "tests", "test_oracle.py") + "::test_tie_heavy_sets_match_the_reference_build",
                      os.path.join(ROOT, "tests", "test_oracle.py") + "::test_wav_readers_against_the_reference_reader"])
    if rc != 0:
        raise SystemExit("the tests failed against the live reference build: nothing recorded")
    gpu_test_calls()
    n = orc.save_recording()
    print("%d calls recorded -> %s (%.1f kB)" % (n, os.path.relpath(orc.REF_CALLS, ROOT), os.path.getsize(orc.REF_CALLS) / 1e3))


if __name__ == "__main__":
    main()
