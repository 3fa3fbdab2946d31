"""Every kernel of csrc/frontend.hip (k_mask_prefix, k_wav_lens, k_compact_active, k_stft_fbank, k_identity_prefix) on its own, against the float64
references of tests/frontend_ref.py.

Diarizer.frontend_prepare_case / frontend_features_case / frontend_signals_case (sd_test_frontend_* of include/sdhip_test.h) run the front end through the
functions run_embed, sd_frontend and sd_embed_signals call, in the form the product runs: the compacted active list, row spaces of min(501, nvalid + 65)
rows, a last tile that is partial, first_item and origin other than 0, more live items than workgroups.  The masks are followed by 256 x 293 NaN, the
waveform slice has 256 NaN in front of it and behind it, every output is preset to a canary and has 256 slack entries (rows) behind it.  The cases and
their operands live in tests/frontend_cases.py; tests/test_frontend_ref.py pins the references to the oracle, holds a float32 restatement of the kernel's
arithmetic to every tolerance below on every case (no element left out) and shows that every tolerance is at least ten times smaller than what each of
some twenty single mistakes does on a case of this file.

Exact parts (prefix, counts, wav_lens as bits, nnorm, nvalid, flags, alist, cidx, the compacted arrays, n_active): bit for bit, 1 .. 2 100 items.

k_stft_fbank.  Every element of every stored row is held to a bound computed from the float64 running quantities, u = 2^-24, gamma_n = n u / (1 - n u):
  E     both FFTs are fp64 (the kernel's 16 x 25 mixed-radix one and numpy's): each bin within 64 x 2^-53 x |X|_2 of the true value, |X|_2 = 20 |x w|_2
        (Higham, Accuracy and Stability, 24.2: log2(N) x eta with eta ~ 7 u for computed twiddles), twice.  The window product is exact in fp64.
  dP    two values within E of each other, each cast to float32, differ by 2 u |.| + E; two products and a sum, or a product and an FMA, add gamma_2:
        dP = (gamma_2 + 4.5 u) P + 2.1 E (|re| + |im|) + 2.1 E^2 + 2^-125
  dM    an FMA chain over the c stored weights of the filter: gamma_c sum |w| P + (1 + gamma_c) sum |w| dP
  ddb   10 / ln 10 x dM / max(M - dM, 1e-10) (nothing where M + dM <= 1e-10: both sides sit on the floor), + (2 L + 1) u |dB| for log10f good to L ulp
        and the product with 10, + 6e-8 (the float32 constant 1e-10f is not 1e-10)
  dmax  the largest ddb among the cells that can be the maximum (dB + ddb >= max (dB - ddb)), + u |floor| for the subtraction of 80
  dy    ddb above the floor, dmax below it, the larger of the two where the bounds cannot tell
  mean  mean of dy over the nnorm frames + gamma_(nnorm / 3 + 3) x mean |y| (three interleaved partial sums, joined, divided)
  out   dy + dmean + u |out|
L = 2 is ASSUMED: the Makefile compiles with -O3 and neither -ffast-math nor a device-libs fast-math option, so log10f is OCML's default-precision
routine; the ROCm documentation installed with the toolchain states no ulp figure for it (the HIP programming guide published by AMD lists 2 ulp for
log10f).  Typical tolerances: 5e-5 .. 1e-3 dB (tests/test_frontend_ref.py prints them).

Where the maximum lies.  With q = len * 501 the last selected sample sits in frame nvalid - 1 at window position about 199 + 159.7 frac(q) - 0.32 floor(q);
for frac(q) above about one half, frame nvalid holds the item's tail nearer the window's centre.  A burst in the last 50 selected samples of the 820- and
of the 2 731-sample item (q = 5.14, 17.10) is therefore loudest below nvalid (frames 5 and 17 of 6 and 18), while in the 3 004-sample item of case
"signals" (the first 11 mask frames, q = 18.81, nvalid 19, 84 rows) it is loudest in frame 19: outside nvalid, inside the stored rows.  That item is
where "maximum over the first nvalid frames only" shows in the compact form (tests/test_frontend_ref.py: 57 000 tolerances), beside the sig_mode case.

The looping case is built for the MI355X: frontend_cases.GRID = 512 = 2 x 256 compute units.  On a part with another count the looping test fails on its
grid assertion, which says so; the grid it compares is the one frontend_features recorded for its launch.

Measured on the MI355X, max(error / tolerance) per family (the float32 restatement on the CPU in brackets):
    rows (need 80 .. 501, nvalid 436 / 437)       0.181  (0.201)
    masks (skip_dead_rows 1 and 0)                0.249  (0.206)
    end of the audio                              0.133  (0.077)
    position (first_item 0 / 32 / 96, origin)     0.275  (0.262)
    signals (1e-4, 1e-6, silence, DC, bursts)     0.243  (0.210)
    tones on bins 0, 12, 13, 25, 187 .. 200       0.327  (0.217)
    every bin (three one-bin banks)               0.225  (0.226)
    asymmetric window                             0.198  (0.234)
    tie (nnorm 250, nvalid 251)                   0.085  (0.088)
    loop (1 056 items on 512 workgroups)          0.326  (0.319)      thinned to 713 items: the same bits per item
    sig_mode B = 1 / 33 / 1 with all rows         0.118 / 0.313 / 0.118  (0.114 / 0.351)
No ratio above 1, so nothing here speaks against L = 2; the exact parts are equal bit for bit at every item count.
The whole file: 47 tests in 4.2 s (0.6 s of it the context), the looping test 0.53 s, every other test at or below 0.15 s.
"""
import numpy as np
import pytest

import sdhip
import frontend_cases as K
import frontend_ref as R
from oracle import nn_oracle as nn

pytestmark = pytest.mark.gpu

CANARY = np.float32(K.CANARY)
SLACK = sdhip.FE_SLACK
SD_ERR_ARG = 1


def report(what, err, tol):
    q = err / tol
    ratio = float(q.max())
    print("RATIO %-60s max(error / tolerance) = %.3f" % (what, ratio))
    assert ratio <= 1.0, "%s: %d values beyond the tolerance, max(error / tolerance) = %.3f, first at %s (error %.3g, tolerance %.3g)" % (
        what, (q > 1).sum(), ratio, np.argwhere(q > 1)[0], err[q > 1][0], tol[q > 1][0])
    return ratio


@pytest.fixture(scope="module")
def pack_diarizer(diarizer, weights, tmp_path_factory):
    """a context per window / mel bank of frontend_cases.PACKS, opened when first asked for"""
    win, mel = K.tables("product")
    assert np.array_equal(weights[3]["stft.window"], win) and np.array_equal(weights[3]["fbank.matrix"], mel)
    made = {"product": diarizer}
    d = tmp_path_factory.mktemp("fe_packs")

    def get(pack):
        if pack not in made:
            w, m = K.tables(pack)
            ep = str(d / (pack + ".sdw"))
            nn.save_pack(ep, dict(weights[3], **{"stft.window": w, "fbank.matrix": m}))
            made[pack] = sdhip.Diarizer(weights[0], ep)
        return made[pack]

    yield get
    for k, v in made.items():
        if k != "product":
            v.close()


# ---------------------------------------------------------------- exact parts
def _guarded(got, n, canary, what):
    assert (got[n:] == canary).all(), "%s: %d slack entries were overwritten" % (what, (got[n:] != canary).sum())
    return got[:n]


@pytest.mark.parametrize("compact", [True, False])
@pytest.mark.parametrize("items", K.PREPARE_ITEMS)
def test_prepare_exact(diarizer, items, compact):
    masks = K.prepare_masks(items)
    exp = K.prepare_expected(masks, compact)
    got = diarizer.frontend_prepare_case(masks, compact=compact, icanary=K.ICANARY, fcanary=CANARY)
    what = "%d items%s" % (items, ", compact" if compact else "")
    pre = _guarded(got["prefix"], items * 296, K.ICANARY, what + " prefix").reshape(items, 296)
    assert np.array_equal(pre[:, :294], exp["prefix"]) and (pre[:, 294:] == K.ICANARY).all(), what
    for k in ("counts", "nnorm", "nvalid", "flags"):
        assert np.array_equal(_guarded(got[k], items, K.ICANARY, what + " " + k), exp[k]), (what, k)
    assert np.array_equal(_guarded(got["wav_lens"], items, CANARY, what + " wav_lens").view(np.int32), exp["wav_lens"].view(np.int32)), what
    if compact:
        na = exp["n_active"]
        assert got["n_active"].tolist() == [na] + [K.ICANARY] * 3, what
        assert np.array_equal(_guarded(got["cidx"], items, K.ICANARY, what + " cidx"), exp["cidx"]), what
        for k in ("alist", "nnorm_c", "nvalid_c"):
            assert np.array_equal(_guarded(got[k], na, K.ICANARY, what + " " + k), exp[k]), (what, k)     # nothing behind the live items either


def test_rounding_tie_and_refusal(diarizer):
    masks = np.stack([K.first_frames(14), K.first_frames(28)])
    got = diarizer.frontend_prepare_case(masks)
    assert got["counts"][:2].tolist() == [3823, 7646] and got["wav_lens"][0] == 0.5
    assert got["nnorm"][:2].tolist() == [250, 501] and got["nvalid"][:2].tolist() == [251, 501]
    with pytest.raises(sdhip.SdError) as e:
        diarizer.frontend_prepare_case(masks, first_item=5)
    assert e.value.code == SD_ERR_ARG


# ---------------------------------------------------------------- k_stft_fbank
def _check(what, feats, rowoff, ref):
    rows, na = ref["rows_all"], len(ref["rowoff"]) - 1
    assert feats.shape == (rows + SLACK, R.FEAT_LD)
    assert (feats[rows:] == CANARY).all(), "%s: %d guard elements behind the rows were overwritten" % (what, (feats[rows:] != CANARY).sum())
    assert np.array_equal(rowoff[:na + 1], ref["rowoff"]) and (rowoff[na + 1:] == -1).all(), what
    live = feats[:rows]
    assert np.isfinite(live).all(), "%s: %d values are not finite (a guard in front of or behind the slice, or behind the masks, was read), first at %s" % (
        what, (~np.isfinite(live)).sum(), np.argwhere(~np.isfinite(live))[0])
    assert not (live == CANARY).any(), "%s: %d elements inside the stored rows were never written" % (what, (live == CANARY).sum())
    assert not live[:, R.NMELS:].any(), what + ": the pad columns 80 .. 95 must be exactly 0"
    return report(what, np.abs(live[:, :R.NMELS].astype(np.float64) - ref["exp"]), ref["tol"])


def _run(pack_diarizer, name):
    c, ref = K.feature_case(name), K.reference(name)
    feats, rowoff, cidx, info = pack_diarizer(c["pack"]).frontend_features_case(c["wav"], c["n_total"], c["origin"], c["first_item"], c["masks"],
                                                                                ref["rows_all"], skip_dead_rows=c["skip"], canary=CANARY)
    assert np.array_equal(cidx, ref["cidx"]), name + ": cidx (a dropped item has -1 and no rows)"
    assert info["n_active"] == len(ref["alist"]) and info["rows_all"] == ref["rows_all"] and 1 <= info["grid"] <= info["n_active"]
    return feats, rowoff, info, ref


@pytest.mark.parametrize("name", [n for n in K.FEATURE_CASES if not n.startswith("loop")])
def test_features(pack_diarizer, name):
    feats, rowoff, info, ref = _run(pack_diarizer, name)
    _check("k_stft_fbank %s [%s]" % (name, K.FAMILY.get(name, "position")), feats, rowoff, ref)


def test_features_persistent_loop(pack_diarizer):
    """1 056 live items on min(2 x compute units, live items) = 512 workgroups: every workgroup takes a second item, 32 a third; the workgroup that has just
    finished a full-length item 120 dB louder takes a three-frame item of the quietest audio (workgroups 0 and 511 among them).  Then the same operands
    with every third short item switched off: every later item runs in another slot, on another workgroup, after another predecessor, and must
    return the same bits."""
    feats, rowoff, info, ref = _run(pack_diarizer, "loop")
    assert info["grid"] == K.GRID < info["n_active"], "the case is built for the MI355X's grid of %d (2 x 256 compute units); the launch reports %r" % (K.GRID, info)
    _check("k_stft_fbank loop (%d items on %d workgroups)" % (info["n_active"], info["grid"]), feats, rowoff, ref)
    feats2, rowoff2, info2, ref2 = _run(pack_diarizer, "loop_thinned")
    assert info2["grid"] == K.GRID < info2["n_active"] < info["n_active"]
    _check("k_stft_fbank loop, thinned (%d items)" % info2["n_active"], feats2, rowoff2, ref2)
    moved = 0
    for a2, i in enumerate(ref2["alist"]):
        a = ref["cidx"][i]
        r, r2 = feats[rowoff[a]:rowoff[a + 1]], feats2[rowoff2[a2]:rowoff2[a2 + 1]]
        assert r.shape == r2.shape and np.array_equal(r.view(np.int32), r2.view(np.int32)), "item %d: slot %d and slot %d give other bits" % (i, a, a2)
        moved += a != a2
    assert moved > 600


@pytest.mark.parametrize("B,skip", [(1, True), (33, True), (1, False)])
def test_features_signals(diarizer, B, skip):
    sig, lens = K.signals_case(B)
    ref = K.signals_reference(B, skip)
    feats, rowoff, info, prefix, counts = diarizer.frontend_signals_case(sig, lens, ref["rows_all"], skip_dead_rows=skip, icanary=K.ICANARY, canary=CANARY)
    assert info["n_active"] == B and info["rows_all"] == ref["rows_all"] and 1 <= info["grid"] <= B
    # k_identity_prefix: every mask frame selected
    pre = _guarded(prefix, B * 296, K.ICANARY, "identity prefix").reshape(B, 296)
    assert (pre[:, :294] == R.frame_start(np.arange(294))[None, :]).all() and (pre[:, 294:] == K.ICANARY).all()
    assert (_guarded(counts, B, K.ICANARY, "identity counts") == R.CHUNK).all()
    _check("k_stft_fbank sig_mode B=%d%s" % (B, "" if skip else ", all rows"), feats, rowoff, ref)


def test_signals_lengths_refused(diarizer):
    sig, lens = K.signals_case(1)
    below = np.nextafter(K.smallest_len(), np.float32(0))
    for bad in (below, 0.0, 1.0000001, np.nan):
        with pytest.raises(sdhip.SdError) as e:
            diarizer.frontend_signals_case(sig, np.array([bad], np.float32), 501)
        assert e.value.code == SD_ERR_ARG


def test_features_refusals(diarizer):
    """a chunk of a live item in front of the slice, a slice that ends before the audio its last chunk holds, a row count other than the plan's"""
    c, ref = K.feature_case("pos_32_1"), K.reference("pos_32_1")
    run = lambda wav, n_total, origin, rows: diarizer.frontend_features_case(wav, n_total, origin, 32, c["masks"], rows, canary=CANARY)
    for args in ((c["wav"][1:], c["n_total"], c["origin"] + 1, ref["rows_all"]), (c["wav"][:-5001], c["n_total"], c["origin"], ref["rows_all"]),
                 (c["wav"], c["n_total"], c["origin"], ref["rows_all"] + 1)):
        with pytest.raises(sdhip.SdError) as e:
            run(*args)
        assert e.value.code == SD_ERR_ARG
    feats, rowoff, cidx, info = run(c["wav"][:-5000], c["n_total"], c["origin"], ref["rows_all"])      # the slice may end where the last chunk ends
    _check("k_stft_fbank pos_32_1, slice ending with the last chunk", feats, rowoff, ref)
