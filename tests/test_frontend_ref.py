"""CPU side of tests/test_frontend_kernels.py: the references of tests/frontend_ref.py are pinned to the oracle, the float32 restatement of the
kernel's arithmetic stays inside every tolerance on every case of the GPU file (no element left out), and every tolerance tells the listed mistakes
from the reference by a factor of ten or more on a case of the GPU file that is named here."""
import os
import re

import numpy as np
import pytest

import frontend_cases as K
import frontend_ref as R
from conftest import PKG
from oracle import nn_oracle as nn, orc


# ---------------------------------------------------------------- the reference is the oracle's
def test_frame_rule_is_the_kernels():
    per_frame = np.diff(R.frame_start(np.arange(R.FRAMES + 1)))
    assert per_frame.sum() == R.CHUNK and R.frame_start(0) == 0 and R.frame_start(R.FRAMES) == R.CHUNK
    assert np.array_equal(per_frame, np.bincount((np.arange(R.CHUNK, dtype=np.int64) * R.FRAMES) // R.CHUNK, minlength=R.FRAMES))
    assert np.array_equal(per_frame, R.FRAME_LEN) and set(per_frame) == {273, 274}
    src = open(os.path.join(PKG, "csrc", "frontend.hip")).read()
    assert re.search(r"int frame_start\(int f\) \{ return \(int\)\(\(\(int64_t\)SD_CHUNK \* f \+ \(SD_FRAMES - 1\)\) / SD_FRAMES\); \}", src)


@pytest.mark.parametrize("name", ["masks", "end", "tie", "asym"])
def test_reference_is_the_oracle(name):
    c, p = K.feature_case(name), K.reference(name)
    win, mel = K.tables(c["pack"])
    assert c["origin"] == 0 and c["first_item"] == 0
    items = len(c["masks"])
    sigs = np.zeros((items, R.CHUNK), np.float32)
    for i in range(items):
        sig, n = orc.mask_compact(orc.crop(c["wav"], (i // 3) * 8000), c["masks"][i])
        assert n == p["counts"][i]
        mine = K.item_signal(c, i, p["on"][i])
        assert np.array_equal(sig[:n], mine[:n]) and not mine[n:].any()
        sigs[i, :n] = sig[:n]
    lens, ts, an = orc.wav_lens(p["counts"].astype(np.int64))
    my_lens, nnorm, nvalid, flags = R.wav_lens(p["counts"])
    assert np.array_equal(lens.view(np.int32), my_lens.view(np.int32)) and np.array_equal(flags.astype(bool), ts | an)
    live = p["alist"]
    st = nn.stft_ref(sigs[live], win)
    f = nn.fbank_norm_ref(st, lens[live], mel, dtype=__import__("torch").float64).numpy()
    for a, i in enumerate(live):
        it = R.Item(sigs[i], int(p["counts"][i]), win, mel, int(nnorm[i]), R.T)
        assert np.abs(it.out - f[a]).max() <= 1e-9, (name, i, np.abs(it.out - f[a]).max())
        r0, r1 = p["rowoff"][a], p["rowoff"][a + 1]
        assert np.array_equal(it.out[:r1 - r0], p["exp"][r0:r1])


def test_lengths_rule_on_the_prepare_masks():
    for items in (70, 1025):
        m = K.prepare_masks(items)
        e = K.prepare_expected(m, True)
        for b0 in range(0, items, 32):
            lens, ts, an = orc.wav_lens(e["counts"][b0:b0 + 32].astype(np.int64))
            assert np.array_equal(lens.view(np.int32), e["wav_lens"][b0:b0 + 32].view(np.int32))
            assert np.array_equal(ts | an, e["flags"][b0:b0 + 32].astype(bool))
        per_frame = np.bincount((np.arange(80000, dtype=np.int64) * 293) // 80000, minlength=293)
        with np.errstate(invalid="ignore"):
            assert np.array_equal(e["counts"], ((m > 0.5) * per_frame[None, :]).sum(1))


def test_rounding_ties_exist_and_round_to_even():
    pairs = K.tie_pairs()
    assert (14, 28) in pairs and sum(float(K.len_times_T(a, b)) == 250.5 for a, b in pairs) >= 31          # halves: 3 823 / 7 646, ...
    assert K.PRE[14] == 3823 and K.PRE[28] == 7646 and float(K.len_times_T(14, 28)) == 250.5
    lens, nn_, nv, flags = R.wav_lens(np.array([K.PRE[14], K.PRE[28]]))
    assert nn_.tolist() == [250, 501] and nv.tolist() == [251, 501] and not flags.any()
    p = K.reference("tie")
    assert p["nnorm"][0] == 250 and p["nvalid"][0] == 251 and p["rowoff"].tolist() == [0, 316, 817]


def test_rows_case_covers_the_row_counts():
    need = np.diff(K.reference("rows")["rowoff"]).tolist()
    for want in (80, 81, 96, 97, 500, 501):
        assert want in need, (want, need)
    p = K.reference("rows")
    assert {436, 437} <= set(p["nvalid"][p["alist"]].tolist())
    assert np.diff(K.reference("masks")["rowoff"]).tolist() == [501, 315, 88, 105, 71]           # 71: three frames, the shortest live item
    assert (np.diff(K.reference("masks_all_rows")["rowoff"]) == 501).all()


def test_frames_past_the_stored_rows_hold_no_sample():
    """DESIGN.md, front end: frame t reads the compacted samples [160 t - 200, 160 t + 200), so only frames t < cnt / 160 + 1.25 hold a sample; an item
    stores nvalid + 65 rows and nvalid = ceil(float32(cnt / max) * 501) >= cnt * 501 / 80000 > cnt / 160.  Over every prefix length and both extremes of
    the batch maximum (the item itself, a full item)"""
    for a in range(1, R.FRAMES + 1):
        cnt = int(K.PRE[a])
        if cnt < R.MIN_SAMPLES:
            continue
        for mx in (cnt, R.CHUNK):
            lens, nn_, nv, flags = R.wav_lens(np.array([cnt, mx]))
            need = int(R.need_rows(nv[0]))
            assert R.computed_frames(cnt) <= cnt / 160 + 2.25 and R.computed_frames(cnt) <= need, (a, mx)       # frames 0 .. floor(cnt / 160 + 1.25)
            assert need == R.T or need - R.computed_frames(cnt) >= 63


def test_every_bin_reads_its_own_line():
    """all-ones window, one bin per filter: every interior frame holds 20 log10 |X_k| of the periodic signal, each bin on its own"""
    rng = np.random.default_rng(77)
    k = np.arange(201)
    a, phi = 0.01 * 10.0 ** (-2.0 * k / 200.0), rng.uniform(0.2, 1.2, 201)
    line = 20 * np.log10(np.where((k == 0) | (k == 200), 400 * a * np.abs(np.cos(phi)), 200 * a))
    seen = []
    for name, (b0, nb, pair) in K.BIN_PACKS.items():
        c = K.feature_case(name)
        it = R.Item(K.item_signal(c, 0, R.mask_on(c["masks"])[0]), 80000, *K.tables(name), 501, 501)
        assert np.abs(it.db[2:499, :nb] - line[None, b0:b0 + nb]).max() < 1e-3
        assert (it.db[:, nb:79] == -100).all()
        seen += list(range(b0, b0 + nb))
    assert seen == list(range(201))


def test_signal_cases_reach_the_floor_and_the_clamp():
    """case "signals": noise at 1e-6 has cells under the 1e-10 floor and a maximum low enough for the floor to show; the bursts clamp most cells"""
    c, p = K.feature_case("signals"), K.reference("signals")
    tabs = K.tables("product")

    def item(i):
        return R.Item(K.item_signal(c, i, p["on"][i]), int(p["counts"][i]), tabs[0], tabs[1], int(p["nnorm"][i]), 501)

    quiet = item(30 + 2)
    assert (quiet.db[:498] == -100).mean() > 0.05 and quiet.vmax < -20
    for sig in (4, 5, 6):
        for k in (0, 1, 2):
            it = item(30 * sig + k)
            assert (it.db[:it.nf] < it.floor).mean() > 0.5, (sig, k)
    # where the last 50 selected samples are loudest depends on frac(len * 501): in the 820- and the 2 731-sample item (5.14, 17.10) frame nvalid - 1 holds
    # them nearest the window's centre; in the 3 004-sample item (18.81) frame nvalid = 19 does: its maximum lies outside nvalid and inside the 84 stored rows
    for k, nv in ((0, 6), (1, 18)):
        it = item(30 * 4 + k)
        assert p["nvalid"][30 * 4 + k] == nv and np.unravel_index(it.db.argmax(), it.db.shape)[0] < nv and it.floor < it.db[nv].max() < it.db[nv - 1].max()
    it = item(K.MARGIN_ITEM)
    a = p["cidx"][K.MARGIN_ITEM]
    nv, need = int(p["nvalid"][K.MARGIN_ITEM]), int(p["rowoff"][a + 1] - p["rowoff"][a])
    assert p["counts"][K.MARGIN_ITEM] == 3004 and (nv, need) == (19, 84)
    assert nv <= np.unravel_index(it.db.argmax(), it.db.shape)[0] < need and it.db[:nv].max() < it.vmax - 1          # dB: thousands of tolerances


# ---------------------------------------------------------------- the restatement stays inside every tolerance
def _restate(c_sig, cnt, tabs, nnorm, exp, tol, t_end, **kw):
    out, db = R.f32_item(c_sig, cnt, tabs[0], tabs[1], nnorm, len(exp), t_end=t_end, **kw)
    assert np.isfinite(out).all() or kw.get("mut")
    with np.errstate(invalid="ignore"):
        q = np.abs(out.astype(np.float64) - exp) / tol
    return float(np.nan_to_num(q, nan=np.inf).max()), db


def _item(name, a, **wrong):
    """operands of live item a of a feature case -> (signal, cnt, tables, nnorm, exp, tol, t_end)"""
    c, p = K.feature_case(name), K.reference(name)
    i = int(p["alist"][a])
    r0, r1 = p["rowoff"][a], p["rowoff"][a + 1]
    return (K.item_signal(c, i, p["on"][i], **wrong), int(p["counts"][i]), K.tables(c["pack"]), int(p["nnorm"][i]), p["exp"][r0:r1], p["tol"][r0:r1], r1 - r0)


@pytest.mark.parametrize("name", K.FEATURE_CASES)
def test_restatement_inside_every_tolerance(name):
    p = K.reference(name)
    assert (p["tol"] > 0).all() and np.isfinite(p["tol"]).all() and np.isfinite(p["exp"]).all()
    worst = max(_restate(*_item(name, a))[0] for a in range(len(p["alist"])))
    print("RATIO cpu restatement %-20s max(error / tolerance) = %.3f, largest tolerance %.2e dB, median %.2e" % (name, worst, p["tol"].max(), np.median(p["tol"])))
    assert worst <= 1.0


@pytest.mark.parametrize("B", [1, 33])
def test_restatement_inside_every_tolerance_signals(B):
    sig, lens = K.signals_case(B)
    p = K.signals_reference(B)
    tabs = K.tables("product")
    worst = 0.0
    for i in range(B):
        r0, r1 = p["rowoff"][i], p["rowoff"][i + 1]
        worst = max(worst, _restate(sig[i], 80000, tabs, int(p["nnorm"][i]), p["exp"][r0:r1], p["tol"][r0:r1], R.T)[0])
    print("RATIO cpu restatement sig_mode B=%d max(error / tolerance) = %.3f" % (B, worst))
    assert worst <= 1.0
    if B == 33:
        assert set(p["nnorm"].tolist()) == {1, 7, 250, 501} and set(p["nvalid"].tolist()) == {1, 7, 251, 501}


# ---------------------------------------------------------------- every tolerance tells the mistakes from the reference
def _live(name, item):
    return int(K.reference(name)["cidx"][item])


MISTAKES = [
    # (mistake, case of the GPU file, item of the case)
    ("window_symmetric", "masks", 0), ("window_reversed", "asym", 0), ("pad_199", "masks", 0), ("hop_shift", "masks", 0),
    ("drop_first_weight_40", "masks", 0), ("drop_last_weight_40", "masks", 0), ("swap_bins_100", "bins79", 0), ("swap_bins_100", "masks", 0), ("half_bin_200", "bins158", 0),
    ("half_bin_0", "bins0", 0), ("no_floor", "signals", 30 + 2), ("top_db_79_9", "signals", 30 * 4 + 2), ("div_plus", "masks", 0), ("div_minus", "masks", 0),
    ("div_plus", "masks", 4), ("div_minus", "masks", 4), ("max_nvalid_only", "signals", K.MARGIN_ITEM),
]


@pytest.mark.parametrize("mut,name,item", MISTAKES)
def test_arithmetic_mistakes_are_ten_times_outside(mut, name, item):
    ratio, _ = _restate(*_item(name, _live(name, item)), mut=mut, nvalid=int(K.reference(name)["nvalid"][item]))
    print("MISTAKE %-24s on %-10s item %3d: max(error / tolerance) = %.3g" % (mut, name, item, ratio))
    assert ratio >= 10.0


def test_window_reversal_is_invisible_under_the_products_window():
    """why the asymmetric pack exists: the periodic Hamming window has win[k] == win[400 - k] to the last bit or two of float32"""
    ratio, _ = _restate(*_item("masks", 0), mut="window_reversed")
    assert ratio < 3.0


@pytest.mark.parametrize("wrong,name,item", [(dict(floor_src=True), "masks", 1), (dict(origin_err=1), "pos_32_1", 0), (dict(origin_err=-1), "pos_0_0", 1)])
def test_gather_mistakes_are_ten_times_outside(wrong, name, item):
    ratio, _ = _restate(*_item(name, _live(name, item), **wrong))
    print("MISTAKE %-24s on %-10s item %3d: max(error / tolerance) = %.3g" % (wrong, name, item, ratio))
    assert ratio >= 10.0


def test_samples_past_the_end_must_read_zero():
    """case "end": items 3 and 5 select frames the recording ends in; item 4 selects only frames behind its end.  A gather that reads on (the next
    chunk's samples, whatever follows in the buffer) instead of zero is far outside on all three"""
    c, p = K.feature_case("end"), K.reference("end")
    longer = dict(c, wav=np.concatenate([c["wav"], K.noise(40000, 99)]))
    for item in (3, 4, 5):
        a = _live("end", item)
        op = list(_item("end", a))
        op[0] = K.item_signal(longer, item, p["on"][item], past_end="next")
        ratio, _ = _restate(*op)
        assert ratio >= 10.0, (item, ratio)
    assert p["counts"][4] == K.PRE[293] - K.PRE[200] and not K.item_signal(c, 4, p["on"][4]).any()      # counted, and all zero


@pytest.mark.parametrize("rule", ["ceil", "half_up"])
def test_nnorm_rule_mistakes_are_ten_times_outside(rule):
    """case "tie", item 0: len * 501 = 250.5; ceil and round-half-up both average 251 frames.  ceil alone also shows on every item off a tie ("masks" item 4: 5.14)"""
    for name, item in (("tie", 0),) + ((("masks", 4),) if rule == "ceil" else ()):
        p = K.reference(name)
        wrong = R.wav_lens(p["counts"], nnorm_rule=rule)[1]
        assert wrong[item] == p["nnorm"][item] + 1
        op = list(_item(name, _live(name, item)))
        op[3] = int(wrong[item])
        assert _restate(*op)[0] >= 10.0


@pytest.mark.parametrize("mut", ["max_nvalid_only", "max_stored_only"])
def test_maximum_mistakes_are_ten_times_outside_on_the_signals_case(mut):
    """sig_mode, B = 1, wav_lens 0.5: the loudest content lies behind the 316 stored rows, content 20 dB below it behind the 251 valid frames.  (The
    compact form shows the first mistake on case "signals", item MARGIN_ITEM: test_arithmetic_mistakes_are_ten_times_outside.)"""
    sig, lens = K.signals_case(1)
    p = K.signals_reference(1)
    assert p["nvalid"][0] == 251 and p["rows_all"] == 316
    ratio, _ = _restate(sig[0], 80000, K.tables("product"), int(p["nnorm"][0]), p["exp"], p["tol"], R.T, mut=mut, nvalid=251)
    print("MISTAKE %-24s on sig_mode B=1: max(error / tolerance) = %.3g" % (mut, ratio))
    assert ratio >= 10.0


def test_stale_scratch_row_is_ten_times_outside_on_the_loop_case():
    """case "loop": slot 512 (three frames, the quietest audio) runs on workgroup 0 right after slot 0 (a full item, 120 dB louder).  Were the last of its 71
    frames not stored, the scratch row would still hold slot 0's dB there"""
    p = K.reference("loop")
    assert len(p["alist"]) == K.LOOP_ITEMS > K.GRID and np.array_equal(p["cidx"], np.arange(K.LOOP_ITEMS))
    need = np.diff(p["rowoff"])
    full = K.loop_full_slots()
    assert 0 in full and K.GRID - 1 in full and (need[full] == 501).all() and all(need[s + K.GRID] == 71 for s in full if s < K.GRID)
    short = np.delete(need, full)
    assert short.min() == 71 and short.max() == 83
    t = K.reference("loop_thinned")
    assert len(t["alist"]) > K.GRID and len(t["alist"]) < K.LOOP_ITEMS - 300
    assert np.array_equal(np.asarray(p["nnorm"])[t["alist"]], np.asarray(t["nnorm"])[t["alist"]])
    op0 = _item("loop", 0)
    _, db0 = R.f32_item(op0[0], op0[1], op0[2][0], op0[2][1], op0[3], op0[6], t_end=op0[6])
    ratio, _ = _restate(*_item("loop", K.GRID), mut="stale_row", stale=db0)
    ok, _ = _restate(*_item("loop", K.GRID), stale=db0)
    assert ratio >= 10.0 and ok <= 1.0


def test_exact_part_mistakes_change_the_named_cases():
    """`>= 0.5` and a maximum over all items instead of the batch of 32: prepare case of 70 items (tolerance 0: any change counts)"""
    m = K.prepare_masks(70)
    e = K.prepare_expected(m, True)
    assert (m == 0.5).any() and (m == K.ABOVE_HALF).any() and np.isnan(m).any()
    ge = K.prepare_expected(m, True, ge=True)
    assert not np.array_equal(ge["counts"], e["counts"]) and not np.array_equal(ge["prefix"], e["prefix"])
    allmax = K.prepare_expected(m, True, batch=0)
    assert not np.array_equal(allmax["wav_lens"], e["wav_lens"]) and not np.array_equal(allmax["nvalid"], e["nvalid"])
    # the cases cover what they are meant to: a dead batch, a small maximum, runs of dead items across the 1024 step
    e2 = K.prepare_expected(K.prepare_masks(2100), True)
    assert (e2["cidx"][1019:1027] == -1).all() and (e2["cidx"][2043:2051] == -1).all() and e2["cidx"][1027] >= 0
    assert e2["flags"][32:64].all() and 5 * 273 <= e2["counts"][64:96].max() <= 5 * 274
    assert 1024 < e2["n_active"] < 2100
