"""GPU tests of streams at another sample rate than 16 kHz (sd_stream_set_input_rate, sd_stream_end_input, sd_stream_input_info; csrc/resample.hip:
k_resample_jobs; csrc/resample_book.h; csrc/stream.hip).  The contract, bit for bit: after any sequence of pushes at rate sr the stream
is the plain stream to which sd_resample(all n inputs)[0 .. F(n)) was pushed, and after sd_stream_end_input the plain stream to which all of it was.

Samples are compared on noise (about 6 000 inputs: 23 .. 47 tiles of 256 outputs, every piece schedule that can go wrong at a tile or a filter
wing), turns on real seeded networks: 170 000 inputs at 8 kHz are 340 000 outputs, one sealed block of 32 chunks and pending chunks behind it
(a block seals at 328 001 samples), 937 125 inputs at 44.1 kHz the same."""
import os
import subprocess

import numpy as np
import pytest

import resample_stream_ref as rr
import sdhip
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
SD_ERR_ARG = 1
N_NOISE = 6000
SAMPLE_RATES = (8000, 11025, 32000, 44100, 48000)

_ref_cache = {}


def noise_case(d, sr):
    """(int16 inputs, the same as f32, sd_resample of all of them) per rate: computed once, read-only"""
    if sr not in _ref_cache:
        pcm, x = rr.noise(N_NOISE, 900 + sr)
        y = d.resample(x, sr)
        y.setflags(write=False)
        assert len(y) == rr.out_len(N_NOISE, sr)
        _ref_cache[sr] = (pcm, x, y)
    return _ref_cache[sr]


def push_as(s, form, pcm, x, lo, hi):
    """inputs [lo, hi) in one of the three forms; all three hand over the same f32 values (int16 / 32768 is exact)"""
    if form == "pcm":
        s.push(pcm[lo:hi])
    elif form == "f32":
        s.push_f32(x[lo:hi])
    else:
        import torch
        t = torch.from_numpy(np.array(pcm[lo:hi])).to("cuda:0")
        torch.cuda.synchronize()
        s.push_dev(t.data_ptr(), hi - lo)


def schedules(sr):
    """name -> the ends of the pieces, ascending, the last one N_NOISE"""
    L, M, J = rr.plan(sr)
    rng = np.random.default_rng(31 + sr)
    out = {"all at once": [N_NOISE]}
    if sr == 8000:
        out["one sample at a time through the first 2J + 5 inputs"] = list(range(1, 2 * J + 6)) + [N_NOISE]
    ends, n = [], 0
    while n < N_NOISE:
        n = min(N_NOISE, n + int(rng.integers(1, 701)))
        ends.append(n)
    out["random pieces of 1 .. 700"] = ends
    # output m becomes final with input i = floor(m M / L) + J, i.e. at n = i + 1: pieces that end one sample before, at and after that input
    ends = []
    for m in (0, 1, 255, 256, 300, 777, 2048):
        i = (m * M) // L + J
        ends += [i, i + 1, i + 2]
    out["pieces ending around the input that makes an output final"] = sorted(e for e in set(ends) if e < N_NOISE) + [N_NOISE]
    # a push that makes 400 / 600 outputs final spans two / three tiles of 256 outputs
    two, three = -(-400 * M // L), -(-600 * M // L)
    ends, n = [], J + 7
    for k in range(4):
        ends.append(n)
        n += two if k % 2 == 0 else three
    out["pushes that span two and three tiles"] = ends + [N_NOISE]
    return out


def check_after_push(d, s, sr, n, x, y):
    f = rr.final_len(n, sr)
    assert s.input_info() == (sr, n, f, 0), (sr, n)
    assert s.info()[0] == f, (sr, n)
    tail, first = s._tail()
    assert first == 0 and len(tail) == f, (sr, n, len(tail), f)
    assert tail.tobytes() == y[:f].tobytes(), (sr, n)                              # the final outputs of the whole recording
    assert tail.tobytes() == d.resample(x[:n], sr)[:f].tobytes(), (sr, n)          # ... and of the prefix pushed so far


@pytest.mark.parametrize("sr", SAMPLE_RATES)
def test_samples_of_every_piece_schedule_are_the_bytes_of_sd_resample(diarizer, sr):
    pcm, x, y = noise_case(diarizer, sr)
    forms = ("pcm", "f32", "dev")
    for name, ends in schedules(sr).items():
        assert ends == sorted(ends) and ends[-1] == N_NOISE and ends[0] >= 1, name
        outs = [rr.final_len(b, sr) - rr.final_len(a, sr) for a, b in zip([0] + ends[:-1], ends)]
        if "tiles" in name:
            assert any(256 < o <= 512 for o in outs) and any(512 < o <= 768 for o in outs), (name, outs)
        if "final" in name:
            assert min(outs) == 0 and 1 <= min(o for o in outs if o) <= 3, (name, outs)
        print("%d Hz, %s: %d pushes, outputs per push %d .. %d" % (sr, name, len(ends), min(outs), max(outs)))
        with diarizer.stream() as s:
            s.set_input_rate(sr)
            assert s.input_info() == (sr, 0, 0, 0)
            lo = 0
            for k, hi in enumerate(ends):
                push_as(s, forms[k % 3], pcm, x, lo, hi)
                check_after_push(diarizer, s, sr, hi, x, y)
                lo = hi
            s.end_input()
            tail, first = s._tail()
            assert first == 0 and tail.tobytes() == y.tobytes(), (sr, name)
            assert s.input_info() == (sr, N_NOISE, len(y), 1) and s.info()[0] == len(y)
            s.end_input()                                                              # a second one: SD_OK, nothing happens
            assert s._tail()[0].tobytes() == y.tobytes() and s.input_info() == (sr, N_NOISE, len(y), 1)
            with pytest.raises(sdhip.SdError) as e:
                s.push_f32(x[:10])
            assert e.value.code == SD_ERR_ARG and s._tail()[0].tobytes() == y.tobytes()


@pytest.mark.parametrize("sr", SAMPLE_RATES)
def test_a_loud_last_input_reaches_no_output_that_was_final_without_it(diarizer, sr):
    """the noise has amplitude 0.5; an input 90 dB above that, 0.5 * 10^4.5, behind n - 1 inputs must leave the F(n - 1) outputs that were final
    without it as they are, and it does show right behind them"""
    pcm, x, y = noise_case(diarizer, sr)
    n = 2500
    loud = np.float32(0.5 * 10.0 ** 4.5)
    f = rr.final_len(n - 1, sr)
    with diarizer.stream() as s:
        s.set_input_rate(sr)
        s.push_f32(x[:n - 1])
        before = s._tail()[0].copy()
        assert len(before) == f and f > 500
        xl = np.concatenate([x[:n - 1], [loud]]).astype(np.float32)
        yl = diarizer.resample(xl, sr)
        assert before.tobytes() == yl[:f].tobytes()
        assert f < len(yl) and np.abs(yl[f:]).max() > 100.0 and np.abs(yl[:f]).max() < 2.0
        s.push_f32(xl[n - 1:])
        f2 = rr.final_len(n, sr)
        tail = s._tail()[0]
        assert len(tail) == f2 and tail[:f].tobytes() == before.tobytes() and tail.tobytes() == yl[:f2].tobytes()


# ------------------------------------------------------------------ stream equivalence on real seeded networks

def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def turn_bytes(turns):
    return np.array([(s, e, l) for s, e, l in turns], np.float64).tobytes()


def snapshot(d, s, roster=False):
    """everything a stream shows after a turns call: info, origin, turns or error code, the job's confidences / centroids / counts, every cached row"""
    info = s.info()
    try:
        t = s.turns()
        cen, cnt = d.last_speakers()
        job = (turn_bytes(t), d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes(), d.last_roster_ids().tobytes() if roster else b"")
    except sdhip.SdError as e:
        t, job = e.code, None
    seg, emb = s.read(0, s.info()[2])
    return info, s.origin(), t, job, seg, emb


def same_snapshot(a, b):
    return a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and (a[2] == b[2] if not isinstance(a[2], list) else isinstance(b[2], list)) \
        and same_bits(a[4], b[4]) and same_bits(a[5], b[5])


_speech_cache = {}


def speech_at(sr, n_in, seed):
    """n_in int16 inputs "at sr": synthetic 16 kHz speech-like audio read at the positions of the input samples (nearest earlier sample), so that
    what the stream resamples back resembles the audio the seeded networks give turns for"""
    key = (sr, n_in, seed)
    if key not in _speech_cache:
        n16 = n_in * 16000 // sr + 16000
        p = synth.make_pcm(n16 / 16000.0 + 1.0, seed=seed)
        x = p[(np.arange(n_in, dtype=np.int64) * 16000) // sr].copy()
        x.setflags(write=False)
        _speech_cache[key] = x
    return _speech_cache[key]


def check_equivalence(d, sr, pcm, ends, window=None, with_roster=False):
    """a stream at sr fed pcm in pieces ending at `ends`, against a plain stream fed y[F_prev : F_k] with push_f32 -- under the same window and with a
    roster of its own where asked -- after every round and after end_input; at the end against the whole path on sd_resample of everything"""
    x = pcm.astype(np.float32) / np.float32(32768.0)
    y = d.resample(x, sr)
    rosters = [sdhip.Roster(), sdhip.Roster()] if with_roster else [None, None]
    a, b = d.stream(), d.stream()
    try:
        a.set_input_rate(sr)
        for s, r in zip((a, b), rosters):
            if window is not None:
                s.set_window(window)
            if r is not None:
                s.set_roster(r)
        lo, f_prev = 0, 0
        for k, hi in enumerate(ends + ["end"]):
            if hi == "end":
                a.end_input()
                f = len(y)
            else:
                (a.push if k % 2 == 0 else a.push_f32)((pcm if k % 2 == 0 else x)[lo:hi])
                f = rr.final_len(hi, sr)
                lo = hi
            if f > f_prev:
                b.push_f32(y[f_prev:f])
            f_prev = f
            assert a.input_info() == (sr, lo, f, 1 if hi == "end" else 0)
            sa, sb = snapshot(d, a, with_roster), snapshot(d, b, with_roster)
            print("%d Hz, round %s: info %s, origin %d, %s" % (sr, hi, sa[0], sa[1], "%d turns" % len(sa[2]) if isinstance(sa[2], list) else "code %d" % sa[2]))
            assert same_snapshot(sa, sb), (sr, hi, sa[0], sb[0])
            assert a._tail()[0].tobytes() == b._tail()[0].tobytes() and a._tail()[1] == b._tail()[1]
        return sa, y
    finally:
        for s in (a, b):
            s.set_roster(None)
            s.close()
        for r in rosters:
            if r is not None:
                r.close()


def test_a_stream_at_8_khz_is_the_plain_stream_fed_the_final_outputs(diarizer):
    pcm = speech_at(8000, 170000, 8100)
    last, y = check_equivalence(diarizer, 8000, pcm, [100000, 170000])
    assert len(y) == 340000 and last[0] == (340000, 32, sdhip.num_chunks(340000)[0])      # one sealed block, pending chunks behind it
    whole = diarizer.diarize_f32(y)
    cen, cnt = diarizer.last_speakers()
    assert len(whole) >= 1 and last[3] == (turn_bytes(whole), diarizer.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes(), b"")


def test_a_stream_at_44100_hz_through_three_uneven_rounds(diarizer):
    pcm = speech_at(44100, 937125, 4410)
    last, y = check_equivalence(diarizer, 44100, pcm, [50000, 905000, 937125])
    assert len(y) == 340000 and last[0][1] == 32
    whole = diarizer.diarize_f32(y)
    cen, cnt = diarizer.last_speakers()
    assert len(whole) >= 1 and last[3] == (turn_bytes(whole), diarizer.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes(), b"")


def test_window_and_roster_see_the_16_khz_samples_only(diarizer):
    """600 000 outputs seal two blocks; under set_window(1) the first one is forgotten, and both streams name their speakers through a roster"""
    pcm = speech_at(8000, 300000, 8200)
    last, y = check_equivalence(diarizer, 8000, pcm, [170000, 300000], window=1, with_roster=True)
    assert len(y) == 600000 and last[1] == 256000 and last[0][1] == 32 and isinstance(last[2], list) and len(last[2]) >= 1


# ------------------------------------------------------------------ group calls

GROUP_RATES = (None, 8000, 44100, 48000)
GROUP_ENDS = ((60000, 60000, 100000), (50, 100000, 170000), (40, 40, 300000), (0, 250000, 400000))
GROUP_LAUNCHES = (0, 1, 1)      # round 1: 50 and 40 inputs make no output final (J = 68 and 186); afterwards one launch whatever the number of rated streams


def group_piece(i, k):
    pcm = speech_at(GROUP_RATES[i] or 16000, GROUP_ENDS[i][2], 7000 + i)
    return pcm[(GROUP_ENDS[i][k - 1] if k else 0):GROUP_ENDS[i][k]]


_group_solo = []


def group_solo(d):
    """each of the four streams driven alone with single pushes: per round and stream (snapshot, tail, input_info)"""
    if not _group_solo:
        streams = [d.stream() for _ in GROUP_RATES]
        try:
            for s, sr in zip(streams, GROUP_RATES):
                if sr:
                    s.set_input_rate(sr)
            for k in range(3):
                _group_solo.append([])
                for i, s in enumerate(streams):
                    s.push(group_piece(i, k))
                    _group_solo[-1].append((snapshot(d, s), s._tail(), s.input_info()))
        finally:
            for s in streams:
                s.close()
    return _group_solo


@pytest.mark.parametrize("form", ["pcm", "f32"])
def test_group_push_of_plain_and_rated_streams(diarizer, form):
    d = diarizer
    want = group_solo(d)
    assert want[2][1][0][0][1] == 32 and isinstance(want[2][1][0][2], list)      # the 8 kHz stream seals its block in the last round
    streams = [d.stream() for _ in GROUP_RATES]
    try:
        for s, sr in zip(streams, GROUP_RATES):
            if sr:
                s.set_input_rate(sr)
        for k in range(3):
            pcs = [group_piece(i, k) for i in range(len(streams))]
            assert k != 1 or len(pcs[0]) == 0 and len(pcs[2]) == 0
            d.reset_stats()
            if form == "pcm":
                d.stream_push_many(streams, pcs)
            else:
                d.stream_push_many_f32(streams, [p.astype(np.float32) / np.float32(32768.0) for p in pcs])
            assert d.kernel_stats("resample_jobs")["launches"] == GROUP_LAUNCHES[k], k
            assert d.kernel_stats("resample")["launches"] == 0
            got = d.stream_turns_many(streams)
            for i, s in enumerate(streams):
                snap, tail, inp = want[k][i]
                assert s.input_info() == inp and s.info() == snap[0], (k, i)
                assert s._tail()[0].tobytes() == tail[0].tobytes() and s._tail()[1] == tail[1], (k, i)
                if isinstance(snap[2], list):
                    assert isinstance(got[i], list) and turn_bytes(got[i]) == snap[3][0], (k, i)
                    d.many_select(i)
                    cen, cnt = d.last_speakers()
                    assert (d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes()) == snap[3][1:4], (k, i)
                else:
                    assert got[i] == snap[2], (k, i)
                seg, emb = s.read(0, s.info()[2])
                assert same_bits(seg, snap[4]) and same_bits(emb, snap[5]), (k, i)
    finally:
        d.reset_stats()
        for s in streams:
            s.close()


def test_a_call_of_plain_streams_only_launches_what_it_launched(diarizer):
    """two plain streams alone in a group push, and the same two with a rated stream beside them whose piece makes no output final: the launch
    counts of the existing profiled kernels are the same, and neither call resamples"""
    d = diarizer
    names = ("lstm_rec", "stft_mel", "conv_gemm_f32", "asp_pool", "se_apply", "resample", "resample_jobs")
    pcs = [speech_at(16000, 340000, 7100), speech_at(16000, 100000, 7000)]
    counts = []
    for with_rated in (False, True):
        streams = [d.stream(), d.stream()] + ([d.stream()] if with_rated else [])
        try:
            if with_rated:
                streams[2].set_input_rate(8000)
            d.reset_stats()
            d.stream_push_many(streams, pcs + ([speech_at(8000, 170000, 8100)[:60]] if with_rated else []))
            counts.append({k: d.kernel_stats(k)["launches"] for k in names})
            assert [s.info()[0] for s in streams] == [340000, 100000] + ([0] if with_rated else [])
        finally:
            d.reset_stats()
            for s in streams:
                s.close()
    print(counts)
    assert counts[0] == counts[1] and counts[0]["lstm_rec"] > 0 and counts[0]["resample_jobs"] == 0 and counts[0]["resample"] == 0


# ------------------------------------------------------------------ refusals

def test_refusals_leave_the_stream_as_it_was(diarizer):
    d = diarizer
    pcm, x, y = noise_case(d, 8000)

    def shown(s):
        return s.info(), s.input_info(), s._tail()[0].tobytes(), s._tail()[1]

    def refused(call):
        with pytest.raises(sdhip.SdError) as e:
            call()
        assert e.value.code == SD_ERR_ARG

    with d.stream() as s:                                        # the rate after a push; a rate <= 0; a refused rate pair
        for bad in (0, -8000):
            before = shown(s)
            refused(lambda: s.set_input_rate(bad))
            assert shown(s) == before
        # rate pairs sd_resample refuses: 500 001 Hz needs a tap table of 4 213 x 16 000 entries (the limit is 2^26), a tile of 2 MHz an input span of
        # 48 722 floats (the limit is 160 KiB)
        for bad in (500001, 2000000):
            before = shown(s)
            refused(lambda: s.set_input_rate(bad))
            refused(lambda: d.resample(x[:100], bad))
            assert shown(s) == before
        s.set_input_rate(8000)                                   # (and the stream is still as good as new)
        s.push_f32(x)
        assert s._tail()[0].tobytes() == y[:rr.final_len(N_NOISE, 8000)].tobytes()
    with d.stream() as s:
        s.push_f32(x[:100])
        before = shown(s)
        refused(lambda: s.set_input_rate(8000))
        assert shown(s) == before == ((100, 0, 1), (16000, 100, 100, 0), x[:100].tobytes(), 0)
        refused(s.end_input)                                     # end_input on a plain stream
        assert shown(s) == before
    with d.stream() as s:
        s.set_input_rate(8000)
        s.push_f32(x[:1000])
        before = shown(s)
        refused(lambda: s.set_input_rate(44100))
        assert shown(s) == before
        s.end_input()
        before = shown(s)
        refused(lambda: s.push(pcm[:10]))                        # a push after end_input, single and in a group
        refused(lambda: d.stream_push_many([s], [pcm[:10]]))
        assert shown(s) == before and before[1] == (8000, 1000, 2000, 1)
        d.stream_push_many([s], [pcm[:0]])                       # (nothing for that stream is legal)
        assert shown(s) == before
    with d.stream() as a, d.stream() as b:                       # rate 16 000 = no resampler: the bytes of an untouched stream
        a.set_input_rate(16000)
        for k, (lo, hi) in enumerate(((0, 1), (1, 700), (700, 6000))):
            push_as(a, ("pcm", "f32", "dev")[k], pcm, x, lo, hi)
            push_as(b, ("pcm", "f32", "dev")[k], pcm, x, lo, hi)
            assert shown(a) == shown(b) and shown(a)[1] == (16000, hi, hi, 0)
        assert a._tail()[0].tobytes() == x.tobytes()
        a.end_input()                                            # ... and its input closes like any other: SD_OK, nothing emitted, no push afterwards
        assert shown(a) == (shown(b)[0], (16000, N_NOISE, N_NOISE, 1), x.tobytes(), 0)
        a.end_input()
        refused(lambda: a.push(pcm[:10]))
        refused(lambda: a.push_f32(x[:10]))
        refused(lambda: d.stream_push_many([a, b], [pcm[:10], pcm[:0]]))
        d.stream_push_many([a, b], [pcm[:0], pcm[:0]])
        assert shown(a) == (shown(b)[0], (16000, N_NOISE, N_NOISE, 1), x.tobytes(), 0)
        refused(lambda: a.set_input_rate(8000))
        refused(b.end_input)                                     # (b never had a rate)


def test_a_stream_at_16000_hz_closes_and_keeps_its_turns(diarizer):
    """set_input_rate(16000); push; end_input: the turns, the job and the cached rows of the plain stream fed the same samples, before and after"""
    pcm = speech_at(16000, 340000, 7100)
    with diarizer.stream() as a, diarizer.stream() as b:
        a.set_input_rate(16000)
        for lo, hi in ((0, 100000), (100000, 340000)):
            a.push(pcm[lo:hi])
            b.push(pcm[lo:hi])
        want = snapshot(diarizer, b)
        assert same_snapshot(snapshot(diarizer, a), want) and isinstance(want[2], list) and want[0][1] == 32
        a.end_input()
        assert a.input_info() == (16000, 340000, 340000, 1) and b.input_info() == (16000, 340000, 340000, 0)
        assert same_snapshot(snapshot(diarizer, a), want)


# ------------------------------------------------------------------ command line

def test_cli_streams_8_khz_samples_from_stdin(diarizer, weights):
    pcm = speech_at(8000, 170000, 8100)
    with diarizer.stream() as s:
        s.set_input_rate(8000)
        for lo in range(0, len(pcm), 16000):                     # --stream 2: pieces of 2 s of audio = 16 000 inputs
            s.push(pcm[lo:lo + 16000])
        s.end_input()
        want = [sdhip.format_turn(t) for t in s.turns()]
    assert len(want) >= 1
    out = subprocess.run([EXE, weights[0], weights[1], "-", "--stream", "2", "--stream-rate", "8000"], input=pcm.tobytes(), capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if "-->" in l]
    assert lines[-len(want):] == want and len(lines) == len(want)


def test_cli_stream_rate_16000_prints_what_the_plain_stream_run_prints(weights):
    pcm = speech_at(16000, 340000, 7100)
    runs = []
    for extra in ([], ["--stream-rate", "16000"]):
        out = subprocess.run([EXE, weights[0], weights[1], "-", "--stream", "2"] + extra, input=pcm.tobytes(), capture_output=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        runs.append([l for l in out.stdout.decode().splitlines() if "-->" in l])
    assert runs[0] == runs[1] and len(runs[0]) >= 1
