"""GPU tests of streams in their own encoding (sd_stream_set_input_format, sd_stream_push_audio*, sd_stream_push_many_audio*; csrc/stream.hip,
csrc/stream_ingest.hip: k_group_ingest; csrc/stream_ingest_plan.h).  The contract, bit for bit: with x the mono floats that steps 1 and 2
of the rule (tests/ingest_ref.py: frames) define on all frames pushed so far, the stream is the stream with the same input rate (or none) to which x was
pushed with push_f32 -- after single pushes, group pushes and any mix of them.

Samples are compared on 6 000 frames of noise with the piece schedules of tests/test_stream_rate.py, turns on the seeded networks: a stereo 8 kHz
mu-law call of 170 000 frames is 340 000 samples per leg, one sealed block of 32 chunks and pending chunks behind it."""
import os
import subprocess

import numpy as np
import pytest

import ingest_ref as G
import resample_stream_ref as rr
import sdhip
from test_many_audio import encode
from test_stream_rate import same_snapshot, snapshot, speech_at, turn_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
SD_ERR_ARG = 1
N_NOISE = 6000
ENCS = (G.ENC_S16, G.ENC_F32, G.ENC_MULAW, G.ENC_ALAW)


def noise(enc, count, seed):
    g = np.random.default_rng(seed)
    if enc == G.ENC_F32:
        return (g.standard_normal(count) * 0.25).astype(np.float32)
    if enc == G.ENC_S16:
        return g.integers(-32768, 32768, count).astype(np.int16)
    return g.integers(0, 256, count).astype(np.uint8)


def schedules(sr):
    """tests/test_stream_rate.py's: all at once, random pieces of 1 .. 700, one frame at a time through the first 2J + 5 frames"""
    _, _, J = rr.plan(sr) if sr != 16000 else (1, 1, 68)
    rng = np.random.default_rng(31 + sr)
    ends, n = [], 0
    while n < N_NOISE:
        n = min(N_NOISE, n + int(rng.integers(1, 701)))
        ends.append(n)
    return {"all at once": [N_NOISE], "random pieces of 1 .. 700": ends, "pieces of 1 frame": list(range(1, 2 * J + 6)) + [N_NOISE]}


def shown(s):
    return s.info(), s.input_info(), s._tail()[0].tobytes(), s._tail()[1]


@pytest.mark.parametrize("channels, channel", [(1, 0), (2, 1)])
@pytest.mark.parametrize("enc", ENCS)
def test_samples_of_every_piece_schedule_are_the_bytes_of_the_f32_twin(diarizer, enc, channels, channel):
    d = diarizer
    el = noise(enc, N_NOISE * channels, 100 * enc + channels)
    x = G.frames(el, enc, channels, channel, N_NOISE)
    for sr in (16000, 8000):
        y = x if sr == 16000 else d.resample(x, sr)
        for name, ends in schedules(sr).items():
            with d.stream() as a, d.stream() as b:
                if sr != 16000:                                                # the rate before the format on one schedule, after it on the others
                    b.set_input_rate(sr)
                    if name == "all at once":
                        a.set_input_rate(sr)
                a.set_input_format(enc, channels, channel)
                if sr != 16000 and name != "all at once":
                    a.set_input_rate(sr)
                assert a.input_format() == (enc, channels, channel, 1) and b.input_format() == (G.ENC_S16, 1, 0, 0)
                lo = 0
                for k, hi in enumerate(ends):
                    piece = el[lo * channels:hi * channels]
                    if k % 3 == 1:
                        d.stream_push_many_audio([a], [piece])                 # a group call of one among the single calls
                    else:
                        a.push_audio(piece)
                    b.push_f32(x[lo:hi])
                    assert shown(a) == shown(b), (sr, name, hi)
                    assert a.input_info()[1] == hi                             # n_in counts frames
                    lo = hi
                if sr != 16000:
                    a.end_input()
                    b.end_input()
                assert shown(a) == shown(b) and a._tail()[0].tobytes() == y.tobytes(), (sr, name)


# ------------------------------------------------------------------ equivalence on the seeded networks

_cache = {}


def stereo_call():
    """(the interleaved mu-law codes of a stereo 8 kHz call of 170 000 frames, the floats of leg 0, of leg 1), read-only"""
    if "call" not in _cache:
        legs = [encode(G.mulaw_table(), speech_at(8000, 170000, 8300 + q)) for q in (0, 1)]
        codes = np.stack(legs, 1).reshape(-1)
        out = (codes, G.frames(codes, G.ENC_MULAW, 2, 0, 170000), G.frames(codes, G.ENC_MULAW, 2, 1, 170000))
        for v in out:
            v.setflags(write=False)
        _cache["call"] = out
    return _cache["call"]


def job_of(d):
    cen, cnt = d.last_speakers()
    return d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes()


def test_both_legs_of_a_stereo_call_from_one_array(diarizer):
    d = diarizer
    codes, x0, x1 = stereo_call()
    legs = [d.stream(), d.stream()]
    twins = [d.stream(), d.stream()]
    try:
        for q, (s, t) in enumerate(zip(legs, twins)):
            s.set_input_rate(8000)
            s.set_input_format(G.ENC_MULAW, 2, q)
            t.set_input_rate(8000)
        last = None
        for lo in list(range(0, 170000, 80000)) + ["end"]:                     # pieces of 10 s
            if lo == "end":
                for s in legs + twins:
                    s.end_input()
            else:
                hi = min(lo + 80000, 170000)
                piece = codes[2 * lo:2 * hi]
                d.reset_stats()
                d.stream_push_many_audio(legs, [piece, piece])                 # the same array for both legs
                assert d.kernel_stats("group_ingest")["launches"] == 1 and d.kernel_stats("resample_jobs")["launches"] == 1
                d.reset_stats()
                twins[0].push_f32(x0[lo:hi])
                twins[1].push_f32(x1[lo:hi])
            last = []
            for s, t in zip(legs, twins):
                sa, sb = snapshot(d, s), snapshot(d, t)
                assert same_snapshot(sa, sb) and s.input_info() == t.input_info(), lo
                assert s._tail()[0].tobytes() == t._tail()[0].tobytes() and s._tail()[1] == t._tail()[1], lo
                last.append(sa)
        assert last[0][0] == (340000, 32, sdhip.num_chunks(340000)[0]) and isinstance(last[0][2], list) and isinstance(last[1][2], list)
        assert len(last[0][2]) >= 1 and len(last[1][2]) >= 1
        # ... and the final turns are those of sd_diarize_many_audio for the two descriptors of everything pushed
        whole = d.diarize_many_audio([sdhip.Audio(codes, 8000, G.ENC_MULAW, 2, q) for q in (0, 1)])
        for q in (0, 1):
            d.many_select(q)
            assert turn_bytes(whole[q]) == last[q][3][0] and job_of(d) == last[q][3][1:4], q
    finally:
        d.reset_stats()
        for s in legs + twins:
            s.close()


MIXED = ((G.ENC_ALAW, 1, 0, 8000, (60000, 100000, 170000)), (G.ENC_S16, 1, 0, None, (40000, 40000, 100000)), (G.ENC_F32, 2, -1, 16000, (0, 90000, 120000)))


def mixed_elements(i):
    enc, channels, channel, sr, ends = MIXED[i]
    key = ("mixed", i)
    if key not in _cache:
        n = ends[-1]
        voice = speech_at(sr or 16000, n, 8400 + i)
        if enc == G.ENC_ALAW:
            el = encode(G.alaw_table(), voice)
        elif enc == G.ENC_S16:
            el = np.array(voice)
        else:
            side = np.roll(voice.astype(np.int32), 777) // 2
            el = (np.stack([voice, side], 1).reshape(-1).astype(np.float32) / np.float32(32768.0))
        el.setflags(write=False)
        _cache[key] = (el, G.frames(el, enc, channels, channel, n))
    return _cache[key]


def open_mixed(d, i, formatted):
    enc, channels, channel, sr, _ = MIXED[i]
    s = d.stream()
    if sr:
        s.set_input_rate(sr)
    if formatted:
        s.set_input_format(enc, channels, channel)
    return s


def mixed_piece(i, k, floats=False):
    el, x = mixed_elements(i)
    ends = MIXED[i][4]
    lo, hi = (ends[k - 1] if k else 0), ends[k]
    return x[lo:hi] if floats else el[lo * MIXED[i][1]:hi * MIXED[i][1]]


def mixed_twins(d):
    """each of the three streams as an unformatted stream of the same rate fed frames() with push_f32, alone: per round and stream (snapshot, shown)"""
    if "twins" not in _cache:
        out = []
        streams = [open_mixed(d, i, False) for i in range(3)]
        try:
            for k in range(3):
                out.append([])
                for i, s in enumerate(streams):
                    s.push_f32(mixed_piece(i, k, floats=True))
                    out[-1].append((snapshot(d, s), shown(s)))
        finally:
            for s in streams:
                s.close()
        _cache["twins"] = out
    return _cache["twins"]


@pytest.mark.parametrize("order, single", [((0, 1, 2), None), ((2, 0, 1), 0), ((1, 2, 0), 2)])
def test_a_group_of_mixed_formats_and_rates(diarizer, order, single):
    """an A-law mono 8 kHz stream, an int16 16 kHz stream with the format (S16, 1, 0) and a float stereo-mean stream with rate 16 000, in two list
    orders and with the pieces of one stream going through single push_audio calls between the group calls"""
    d = diarizer
    want = mixed_twins(d)
    assert want[2][0][0][0][1] == 32 and isinstance(want[2][0][0][2], list)                # the 8 kHz stream seals its block in the last round
    streams = {i: open_mixed(d, i, True) for i in range(3)}
    try:
        for k in range(3):
            group = [i for i in order if i != single]
            if single is not None and k % 2 == 0:
                streams[single].push_audio(mixed_piece(single, k))
            d.reset_stats()
            d.stream_push_many_audio([streams[i] for i in group], [mixed_piece(i, k) for i in group])
            assert d.kernel_stats("group_ingest")["launches"] == 1 and d.kernel_stats("resample_jobs")["launches"] <= 1, k
            assert d.kernel_stats("group_append")["launches"] == 0 and d.kernel_stats("pcm_to_f32")["launches"] == 0 and d.kernel_stats("resample")["launches"] == 0, k
            if single is not None and k % 2 == 1:
                streams[single].push_audio(mixed_piece(single, k))
            got = d.stream_turns_many([streams[i] for i in order])
            for at, i in enumerate(order):
                snap, sh = want[k][i]
                assert shown(streams[i]) == sh, (k, i)
                if isinstance(snap[2], list):
                    assert isinstance(got[at], list) and turn_bytes(got[at]) == snap[3][0], (k, i)
                    d.many_select(at)
                    assert job_of(d) == snap[3][1:4], (k, i)
                else:
                    assert got[at] == snap[2], (k, i)
                assert same_snapshot(snapshot(d, streams[i]), snap), (k, i)
    finally:
        d.reset_stats()
        for s in streams.values():
            s.close()


def test_typed_group_pushes_launch_what_they_launched(diarizer):
    """a typed group push on streams without a format before and after an _audio group push: the same counts, and no k_group_ingest"""
    d = diarizer
    names = ("lstm_rec", "stft_mel", "conv_gemm_f32", "asp_pool", "se_apply", "resample", "resample_jobs", "group_append", "pcm_to_f32", "group_ingest")
    pcs = [speech_at(16000, 340000, 7100), speech_at(8000, 50000, 8100)]

    def typed():
        streams = [d.stream(), d.stream()]
        try:
            streams[1].set_input_rate(8000)
            d.reset_stats()
            d.stream_push_many(streams, pcs)
            c = {k: d.kernel_stats(k)["launches"] for k in names}
            assert [s.info()[0] for s in streams] == [340000, rr.final_len(50000, 8000)]
            return c
        finally:
            d.reset_stats()
            for s in streams:
                s.close()

    before = typed()
    codes = stereo_call()[0]
    with d.stream() as a, d.stream() as b:
        for q, s in enumerate((a, b)):
            s.set_input_format(G.ENC_MULAW, 2, q)
            s.set_input_rate(8000)
        d.reset_stats()
        d.stream_push_many_audio([a, b], [codes[:100000], codes[:100000]])
        c = {k: d.kernel_stats(k)["launches"] for k in names}
        assert c["group_ingest"] == 1 and c["resample_jobs"] == 1 and c["group_append"] == 0 and c["pcm_to_f32"] == 0 and c["resample"] == 0, c
    after = typed()
    print(before)
    assert before == after and before["group_ingest"] == 0 and before["group_append"] == 1 and before["resample_jobs"] == 1 and before["lstm_rec"] > 0


# ------------------------------------------------------------------ the device forms

def test_the_device_forms_equal_the_host_forms(diarizer):
    import torch
    d = diarizer
    cases = [(G.ENC_S16, 2, -1, None), (G.ENC_F32, 1, 0, 8000), (G.ENC_MULAW, 2, 1, 8000), (G.ENC_ALAW, 3, 0, None)]
    host, dev, keep = [], [], []
    try:
        for k, (enc, channels, channel, sr) in enumerate(cases):
            for group in (host, dev):
                s = d.stream()
                group.append(s)
                if sr:
                    s.set_input_rate(sr)
                s.set_input_format(enc, channels, channel)
        els = [noise(enc, 3000 * channels, 600 + k) for k, (enc, channels, _, _) in enumerate(cases)]
        for lo, hi, grouped in ((0, 1, False), (1, 1000, True), (1000, 1001, True), (1001, 3000, False)):
            pieces = [el[lo * c[1]:hi * c[1]] for el, c in zip(els, cases)]
            tens = [torch.from_numpy(np.array(p).view(np.uint8)).to("cuda:0") for p in pieces]
            keep.append(tens)
            torch.cuda.synchronize()
            if grouped:
                d.stream_push_many_audio(host, pieces)
                d.stream_push_many_audio_dev(dev, [t.data_ptr() for t in tens], [hi - lo] * len(cases))
            else:
                for s, p in zip(host, pieces):
                    s.push_audio(p)
                for s, t in zip(dev, tens):
                    s.push_audio_dev(t.data_ptr(), hi - lo)
            for k, (h, v) in enumerate(zip(host, dev)):
                assert shown(h) == shown(v) and h.input_info()[1] == hi, (k, hi)
        # a pointer that is not aligned to its element is refused, single and in a group, and nothing is touched
        t16 = torch.from_numpy(np.zeros(64, np.uint8)).to("cuda:0")
        torch.cuda.synchronize()
        for k in (0, 1):                                                       # int16 and float
            before = shown(dev[k])
            for call in (lambda: dev[k].push_audio_dev(t16.data_ptr() + 1, 4), lambda: d.stream_push_many_audio_dev([dev[2], dev[k]], [t16.data_ptr() + 1, t16.data_ptr() + 1], [4, 4])):
                with pytest.raises(sdhip.SdError) as e:
                    call()
                assert e.value.code == SD_ERR_ARG and shown(dev[k]) == before
            if k == 1:
                with pytest.raises(sdhip.SdError) as e:
                    dev[k].push_audio_dev(t16.data_ptr() + 2, 4)               # even, but not a multiple of 4
                assert e.value.code == SD_ERR_ARG and shown(dev[k]) == before
        before = shown(dev[2])
        dev[2].push_audio_dev(t16.data_ptr() + 1, 4)                           # one-byte elements have no alignment
        assert dev[2].input_info()[1] == before[1][1] + 4
    finally:
        for s in host + dev:
            s.close()


# ------------------------------------------------------------------ refusals

def refused(call, word=None):
    with pytest.raises(sdhip.SdError) as e:
        call()
    assert e.value.code == SD_ERR_ARG, e.value
    if word:
        assert word in str(e.value), e.value


def test_refusals_leave_the_stream_as_it_was(diarizer):
    d = diarizer
    codes = noise(G.ENC_MULAW, 4000, 77)
    pcm = noise(G.ENC_S16, 2000, 78)
    x = G.frames(codes, G.ENC_MULAW, 2, 1, 2000)
    with d.stream() as s:                                                      # bad formats; the stream stays without one
        before = (shown(s), s.input_format())
        for bad in ((4, 1, 0), (-1, 1, 0), (G.ENC_MULAW, 0, 0), (G.ENC_MULAW, -2, 0), (G.ENC_MULAW, 2, 2), (G.ENC_MULAW, 2, -2), (G.ENC_S16, 1, 1)):
            refused(lambda: s.set_input_format(*bad))
            assert (shown(s), s.input_format()) == before == (((0, 0, 0), (16000, 0, 0, 0), b"", 0), (G.ENC_S16, 1, 0, 0))
        refused(lambda: s.push_audio(pcm[:10]), "no input format")             # an _audio push without a format, single and in a group
        refused(lambda: d.stream_push_many_audio([s], [pcm[:10]]), "stream 0")
        refused(lambda: d.stream_push_many_audio_dev([s], [0], [0 - 1]))
        d.stream_push_many_audio([s], [pcm[:0]])                               # (nothing for that stream is legal)
        assert (shown(s), s.input_format()) == before
        s.push(pcm[:100])                                                      # the typed pushes go on, and now the format comes too late
        before = (shown(s), s.input_format())
        refused(lambda: s.set_input_format(G.ENC_MULAW, 2, 1), "before the first sample")
        assert (shown(s), s.input_format()) == before
    with d.stream() as s, d.stream() as plain:                                 # a stream with a format takes the _audio pushes only
        s.set_input_format(G.ENC_MULAW, 2, 1)
        s.set_input_format(G.ENC_MULAW, 2, 1)                                  # (again before the first sample: legal)
        s.set_input_rate(8000)
        s.push_audio(codes[:2000])
        before = (shown(s), s.input_format(), shown(plain))
        assert before[0][1] == (8000, 1000, rr.final_len(1000, 8000), 0)
        import torch
        t = torch.from_numpy(np.array(pcm[:64])).to("cuda:0")
        torch.cuda.synchronize()
        for call in (lambda: s.push(pcm[:10]), lambda: s.push_f32(x[:10]), lambda: s.push_dev(t.data_ptr(), 10), lambda: s.push(pcm[:0])):
            refused(call, "_audio pushes only")
        for call in (lambda: d.stream_push_many([plain, s], [pcm[:10], pcm[:10]]), lambda: d.stream_push_many_f32([plain, s], [x[:10], x[:10]]),
                     lambda: d.stream_push_many_dev([plain, s], [t.data_ptr(), t.data_ptr()], [10, 10])):
            refused(call, "stream 1")
        assert (shown(s), s.input_format(), shown(plain)) == before            # ... and the plain stream of the refused call got nothing
        d.stream_push_many([plain, s], [pcm[:10], pcm[:0]])                    # its row with n = 0 is legal
        assert shown(s) == before[0] and plain.info()[0] == 10
        refused(lambda: s.set_input_format(G.ENC_ALAW, 2, 1), "before the first sample")       # a format after a sample
        refused(lambda: s.set_input_rate(16000))
        lib, h = sdhip.lib(), s._handle()
        before = (shown(s), s.input_format())
        buf = np.zeros(16, np.uint8)
        for frames, ptr in ((-1, buf.ctypes.data), (2 ** 40 + 1, buf.ctypes.data), (4, None)):
            # frames < 0, frames > SD_MANY_MAX_SAMPLES, a null pointer with frames > 0
            assert lib.sd_stream_push_audio(h, ptr, frames) == SD_ERR_ARG and lib.sd_stream_push_audio_dev(h, ptr, frames) == SD_ERR_ARG, frames
            hs = (sdhip.C.c_void_p * 2)(plain._handle().value, h.value)
            ps = (sdhip.C.c_void_p * 2)(buf.ctypes.data, ptr)
            ns = (sdhip.C.c_int64 * 2)(0, frames)
            assert lib.sd_stream_push_many_audio(hs, ps, ns, 2) == SD_ERR_ARG and b"stream 1" in lib.sd_last_error(d._h), frames
            assert (shown(s), s.input_format()) == before
        refused(lambda: s.push_audio(codes[:100].astype(np.int16)), "uint8")   # the binding converts nothing: another dtype, a partial frame
        refused(lambda: d.stream_push_many_audio([s], [codes[:101]]), "whole number of frames")
        assert (shown(s), s.input_format()) == before
        s.push_audio(codes[:0])                                                # no frames: legal, nothing happens
        d.stream_push_many_audio([s, plain], [codes[:0], codes[:0]])
        assert (shown(s), s.input_format()) == before
        s.end_input()                                                          # a closed input
        before = shown(s)
        refused(lambda: s.push_audio(codes[:20]), "closed")
        refused(lambda: d.stream_push_many_audio([plain, s], [codes[:0], codes[:20]]), "closed")
        refused(lambda: s.set_input_format(G.ENC_MULAW, 2, 0))
        assert shown(s) == before and before[1] == (8000, 1000, 2000, 1)
    with d.stream() as s:                                                      # a piece beyond SD_INGEST_MAX_BYTES = 2^42: 2^40 frames of 8 float channels
        s.set_input_format(G.ENC_F32, 8, -1)
        before = shown(s)
        buf = np.zeros(16, np.float32)
        assert sdhip.lib().sd_stream_push_audio(s._handle(), buf.ctypes.data, 2 ** 40) == SD_ERR_ARG and b"SD_INGEST_MAX_BYTES" in sdhip.lib().sd_last_error(d._h)
        hs = (sdhip.C.c_void_p * 1)(s._handle().value)
        ps = (sdhip.C.c_void_p * 1)(buf.ctypes.data)
        ns = (sdhip.C.c_int64 * 1)(2 ** 40)
        assert sdhip.lib().sd_stream_push_many_audio(hs, ps, ns, 1) == SD_ERR_ARG and b"stream 0" in sdhip.lib().sd_last_error(d._h)
        assert shown(s) == before
    with d.stream() as a, d.stream() as b:                                     # what group_check refuses: the same stream twice
        for s in (a, b):
            s.set_input_format(G.ENC_S16, 1, 0)
        refused(lambda: d.stream_push_many_audio([a, a], [pcm[:10], pcm[:10]]), "twice")
        assert shown(a) == ((0, 0, 0), (16000, 0, 0, 0), b"", 0)
        # ... and the format (S16, 1, 0) gives the bytes of push
        a.push_audio(pcm)
        b.set_input_format(G.ENC_S16, 1, 0)
        with d.stream() as c:
            c.push(pcm)
            assert shown(a) == shown(c)


# ------------------------------------------------------------------ command line

def test_cli_streams_one_leg_of_a_stereo_mulaw_call_from_stdin(diarizer, weights):
    codes = stereo_call()[0]
    with diarizer.stream() as s:
        s.set_input_format(G.ENC_MULAW, 2, 1)
        s.set_input_rate(8000)
        for lo in range(0, 170000, 16000):                                     # --stream 2: pieces of 2 s of audio = 16 000 frames
            s.push_audio(codes[2 * lo:2 * (lo + 16000)])
        s.end_input()
        want = [sdhip.format_turn(t) for t in s.turns()]
    assert len(want) >= 1
    args = [EXE, weights[0], weights[1], "-", "--stream", "2", "--stream-rate", "8000", "--stream-encoding", "mulaw", "--stream-channels", "2", "--stream-channel", "1"]
    out = subprocess.run(args, input=codes.tobytes() + b"\xff", capture_output=True, timeout=300)      # one byte of a partial frame behind the call
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.decode().splitlines() if "-->" in l]
    assert lines[-len(want):] == want and len(lines) == len(want)
    assert b"partial frame" in out.stderr
