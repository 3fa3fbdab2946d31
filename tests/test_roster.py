"""GPU tests of the speaker roster on streams and on the last job (sd_stream_set_roster, sd_last_roster_ids, sd_roster_update_last): a roster only renames
labels -- turns, order, confidences, centroids and launch counts are those of a stream without one --; on the planted 75 s recording of
tests/stream_cases.py, pushed in pieces of 10 s, the ids are those of tests/roster_ref.py on the oracle's jobs, with and without a window of one block;
group calls equal single-driven twins; recordings of a pack are linked by centroid; an enrolled gallery, max_num_embeddings and a failing call."""
import numpy as np
import pytest

import roster_cases as rcs
import roster_ref
import sdhip
import stream_cases as sc
import synth

pytestmark = pytest.mark.gpu

SD_ERR_ARG = 1
STATS = ("conv_gemm", "conv_gemm_f32", "lstm_rec", "stft_mel", "asp_pool", "asp_stats", "se_apply", "se_mean", "binarize_masks", "count", "pdist", "linkage",
         "row_nn", "activations", "topk", "speaker_dist", "gallery_norms", "nearest_gallery", "clusters_K", "items_live")


def table_bits(t):
    cen, n, seen = t[:3]
    return cen.tobytes(), n.tolist(), seen.tolist()


def lib_table(r):
    return table_bits(r.speakers()) + (r.info()[1],)


def job(d):
    cen, cnt = d.last_speakers()
    return d.last_confidence().tobytes(), cen.tobytes(), cnt.tolist()


def drive(d, s, pcm, ends):
    """push up to every end and ask for the turns: [(turns, job bytes, roster ids)] and the launch counts of the whole run"""
    d.reset_stats()
    out, pos = [], 0
    for n in ends:
        s.push(pcm[pos:n])
        pos = n
        turns = s.turns()
        out.append((turns, job(d), d.last_roster_ids().tolist()))
    return out, {k: d.kernel_stats(k)["launches"] for k in STATS}


def test_a_roster_only_renames_the_labels(diarizer):
    d, pcm = diarizer, sc.pcm75()
    with sdhip.Roster() as r, d.stream() as plain, d.stream() as named:      # (the streams close first: a roster refuses to close while attached)
        named.set_roster(r)
        a, stats_a = drive(d, plain, pcm, rcs.PREFIXES)
        b, stats_b = drive(d, named, pcm, rcs.PREFIXES)
        assert stats_a == stats_b and stats_a["clusters_K"] == len(rcs.PREFIXES) and stats_a["conv_gemm"] > 0      # nothing is launched that was not launched before
        for (ta, ja, ia), (tb, jb, ib) in zip(a, b):
            assert ia == [] and len(ib) >= 1 and len(set(ib)) == len(ib)
            assert tb == sdhip.relabel_turns_map(ta, ib) and len(tb) >= 1                # same turns in the same order under the map
            assert ja == jb                                                                # confidences, centroids and counts: the same bytes
        again = named.turns()                                                              # nothing pushed: the same ids
        assert again == b[-1][0] and d.last_roster_ids().tolist() == b[-1][2]
        P = r.info()[0]
        with pytest.raises(sdhip.SdError) as e:
            r.close()                                                                      # a stream still holds it
        assert e.value.code == SD_ERR_ARG and r.info()[0] == P
        with sdhip.Roster(8) as small:
            with pytest.raises(sdhip.SdError) as e:
                named.set_roster(small)                                                    # d mismatch
            assert e.value.code == SD_ERR_ARG
            with pytest.raises(sdhip.SdError) as e:
                small.update_last(d)
            assert e.value.code == SD_ERR_ARG and small.info() == (0, 0, 8)
        assert named.turns() == again                                                      # the refused attach changed nothing
        named.set_roster(None)
        assert named.turns() == a[-1][0] and d.last_roster_ids().tolist() == []            # detached: raw labels again
    d.reset_stats()


class Planted:
    """the planted tables of the 75 s recording on the device; point(origin) aims the context's planted rows at the chunk a windowed stream starts with"""

    def __init__(self, d):
        import torch
        scores, emb = sc.planted75()
        dev = torch.device("cuda", 0)
        self.d = d
        self.sc, self.em = torch.from_numpy(np.array(scores)).to(dev), torch.from_numpy(np.array(emb)).to(dev)
        torch.cuda.synchronize()

    def point(self, origin):
        c0 = origin // sc.HOP
        self.d.set_planted(self.sc.data_ptr() + c0 * 293 * 3 * 4, self.em.data_ptr() + c0 * 3 * 192 * 4, 0, sc.CHUNKS - c0)

    def off(self):
        self.d.set_planted(0, 0, 0, 0)


@pytest.mark.parametrize("window", [None, 1])
def test_planted_ids_are_the_reference_s_and_stay_on_their_talkers(diarizer, window):
    d, pcm = diarizer, sc.pcm75()
    run = rcs.planted_run(window)
    fixed = rcs.majority_map(run)
    assert sorted(fixed) == sorted(fixed.values()) == [0, 1, 2, 3]                         # one fixed bijection of ids and talkers
    planted = Planted(d)
    try:
        with sdhip.Roster() as r, d.stream() as s:
            s.set_roster(r)
            if window is not None:
                s.set_window(window)
            planted.point(0)
            pos, raw_of = 0, {}
            for n, origin, ids, hard, table in run:
                s.push(pcm[pos:n])
                pos = n
                assert s.origin() == origin
                planted.point(origin)
                turns = s.turns()
                got = d.last_roster_ids()
                assert got.tolist() == ids.tolist(), (n, got, ids)
                assert lib_table(r) == table_bits(table) + (table[3],), n
                cen, cnt = d.last_speakers()
                want_cen, want_cnt, _ = rcs.planted_job(origin, n)
                assert cen.tobytes() == want_cen.tobytes() and cnt.tolist() == want_cnt.tolist(), n
                if window is None:
                    ref_turns, _ = sc.planted_oracle(n)
                    assert turns == roster_ref.relabel(list(ref_turns), ids), n
                assert {k for _, _, k in turns} <= set(ids.tolist()) and len(turns) >= 1
                for k, i in enumerate(ids.tolist()):
                    raw_of.setdefault(fixed[i], []).append(k)
            assert r.info()[0] == 4
            assert any(len(set(ks)) > 1 for ks in raw_of.values()), raw_of                 # a talker's raw label changes between updates: not vacuous
            if window is not None:
                who = {t: i for i, t in fixed.items()}
                assert who[0] not in run[5][2].tolist() and who[0] in run[6][2].tolist()  # talker 0 left the window at 60 s and is back under his id at 70 s
                assert s.origin() == 3 * rcs.BLOCK
    finally:
        planted.off()


def test_group_calls_equal_single_driven_twins(diarizer, tmp_path):
    d = diarizer
    recs = [synth.make_pcm(40.0, seed=6100 + i)[:n] for i, n in enumerate((600000, 360000, 328001))]
    ends = ((250000, 200000, 100000), (590000, 340000, 328000), (600000, 360000, 328001))
    g = [d.stream() for _ in recs]
    t = [d.stream() for _ in recs]
    rg = [sdhip.Roster() for _ in recs]
    rt = [sdhip.Roster() for _ in recs]
    try:
        for s, r in zip(g + t, rg + rt):
            s.set_roster(r)
        pos = [0, 0, 0]
        for end in ends:
            d.stream_push_many(g, [rec[p:e] for rec, p, e in zip(recs, pos, end)])
            for s, rec, p, e in zip(t, recs, pos, end):
                s.push(rec[p:e])
            pos = list(end)
            got = d.stream_turns_many(g)
            for i in range(3):
                d.many_select(i)
                ids, jb = d.last_roster_ids().tolist(), job(d)
                want = t[i].turns()
                assert got[i] == want and len(want) >= 1, (end, i)
                assert ids == d.last_roster_ids().tolist() and len(ids) >= 1 and jb == job(d), (end, i)
                assert lib_table(rg[i]) == lib_table(rt[i]), (end, i)
        # a group call that is refused leaves every roster as it was
        before = [lib_table(r) for r in rg]
        d.set_dump_dir(str(tmp_path))
        try:
            with pytest.raises(sdhip.SdError):
                d.stream_turns_many(g)
        finally:
            d.set_dump_dir(None)
        assert [lib_table(r) for r in rg] == before
    finally:
        for s in g + t:
            s.close()
        for r in rg + rt:
            r.close()


def test_update_last_links_the_recordings_of_a_pack(diarizer):
    d = diarizer
    a, b = synth.make_pcm(25.0, seed=7), synth.make_pcm(22.0, seed=8)
    turns = d.diarize_many([a, b, a])
    assert all(isinstance(t, list) and len(t) >= 1 for t in turns)
    with sdhip.Roster() as r:
        ids, cens = [], []
        for i in range(3):
            d.many_select(i)
            cens.append(d.last_speakers())
            ids.append(r.update_last(d))
            assert d.last_roster_ids().tolist() == ids[i].tolist() and len(set(ids[i].tolist())) == len(ids[i]) >= 1
        assert cens[2][0].tobytes() == cens[0][0].tobytes()
        assert ids[2].tolist() == ids[0].tolist()                                          # recording 2 is recording 0 again: its ids, at distance 0
        ref = roster_ref.Roster(192)
        for i in range(3):
            assert ref.update(cens[i][0], cens[i][1]).tolist() == ids[i].tolist()
        assert lib_table(r) == table_bits(ref.table()) + (3,)
        named = sdhip.relabel_turns_map(turns[2], ids[2])
        assert [(s, e) for s, e, _ in named] == [(s, e) for s, e, _ in turns[2]]
    d.diarize(a)
    assert d.last_roster_ids().tolist() == []                                              # no roster took part in this job


@pytest.mark.parametrize("case", ["enrolled", "sampled"])
def test_next_to_an_enrolled_gallery_and_under_max_num_embeddings(diarizer, case):
    """the roster names whatever label columns the job has: compared with the reference fed that job's last_speakers and the plain twin's labels"""
    d, pcm = diarizer, sc.pcm75()
    planted = Planted(d)
    try:
        planted.point(0)
        if case == "enrolled":
            d.diarize(pcm[:640000])
            cen, _ = d.last_speakers()
            d.set_enrolled(cen[:1])                                                        # the first speaker of the first 40 s is a known person
        else:
            d.set_option("max_num_embeddings", 40)
        with sdhip.Roster() as r, d.stream() as s:
            s.set_roster(r)
            ref = roster_ref.Roster(192)
            pos = 0
            for n in rcs.PREFIXES[1::2]:
                s.push(pcm[pos:n])
                pos = n
                turns = s.turns()
                ids = d.last_roster_ids()
                cen, cnt = d.last_speakers()
                assert len(ids) == len(cen) and len(set(ids.tolist())) == len(ids) and {k for _, _, k in turns} <= set(ids.tolist())
                s.set_roster(None)
                raw = s.turns()                                                            # the same job without the roster: raw labels
                s.set_roster(r)
                assert turns == sdhip.relabel_turns_map(raw, ids), n
                # detaching dropped what the stream kept, so every update here runs by centroid alone: steps B - D of the reference
                assert ref.update(cen, cnt, t=sdhip.SPEAKER_MATCH_THRESHOLD_DEFAULT).tolist() == ids.tolist(), n
                assert lib_table(r) == table_bits(ref.table()) + (ref.updates,), n
            assert r.info()[0] >= 2
    finally:
        planted.off()
        d.set_enrolled(None)
        d.set_option("max_num_embeddings", -1)


def test_a_failing_turns_call_leaves_roster_and_stream_as_they_were(diarizer, tmp_path):
    d, pcm = diarizer, sc.pcm75()
    planted = Planted(d)
    try:
        planted.point(0)
        with sdhip.Roster() as r, sdhip.Roster() as r2, d.stream() as s, d.stream() as twin:
            s.set_roster(r)
            twin.set_roster(r2)
            for x in (s, twin):
                x.push(pcm[:480000])
                x.turns()
                x.push(pcm[480000:800000])
            before = lib_table(r)
            d.set_dump_dir(str(tmp_path))
            try:
                with pytest.raises(sdhip.SdError) as e:
                    s.turns()
                assert e.value.code == SD_ERR_ARG
            finally:
                d.set_dump_dir(None)
            assert lib_table(r) == before
            good = s.turns()
            ids = d.last_roster_ids().tolist()
            assert good == twin.turns() and ids == d.last_roster_ids().tolist()          # what they would have been
            assert lib_table(r) == lib_table(r2)
    finally:
        planted.off()


@pytest.mark.parametrize("window", [None, "16"])
def test_command_line_prints_roster_ids_in_every_update(diarizer, weights, golden_dir, window):
    """--stream 10 --stream-roster --stream-updates on the reference's 1-min wav: every update block and the final block carry the labels a stream with a
    roster gives for the same pushes (absolute times under --stream-window)"""
    import os
    import subprocess
    path = os.path.join(golden_dir, "multi-speaker_1min.wav")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
    pcm, _, _ = sdhip.read_wav(path)
    cmd = [exe, weights[0], weights[1], path, "--stream", "10", "--stream-roster", "--stream-updates"] + (["--stream-window", window] if window else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("== ")]
    rule = "-" * 52
    d, want = diarizer, []
    with sdhip.Roster() as r, d.stream() as s:
        s.set_roster(r)
        if window:
            s.set_window(1)
        for lo in range(0, len(pcm), rcs.PIECE):
            s.push(pcm[lo:lo + rcs.PIECE])
            off = s.origin() / 16000.0
            want.append([sdhip.format_turn((a + off, b + off, k)) for a, b, k in s.turns()])
        final = [sdhip.format_turn((a + off, b + off, k)) for a, b, k in s.turns()]
        assert r.info()[0] >= 1
    assert len(heads) == len(want) == 6
    for q, i in enumerate(heads):
        end = heads[q + 1] if q + 1 < len(heads) else next(j for j in range(i, len(lines)) if lines[j].startswith("-----------"))
        assert lines[i + 1:end] == want[q], (q, lines[i:end], want[q])
    i0 = lines.index(rule)
    assert lines[i0 + 1:lines.index(rule, i0 + 1)] == final and len(final) >= 1
