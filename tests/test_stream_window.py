"""GPU tests of the sliding window of sd_stream (sd_stream_forget, sd_stream_set_window, sd_stream_origin): after a forget the stream is, bit for bit,
a new stream to which the kept samples were pushed -- turns, confidences, centroids, info and every cached row are those of the whole path on
pcm[origin:n] --, immediately and after further pushes; the window's policy equals the forgets by hand; a windowed stream in a group call equals its
single-driven twin.  The recording is the 75 s one of tests/stream_cases.py (four sealed blocks), with the real networks."""
import numpy as np
import pytest

import sdhip
import stream_cases as sc

pytestmark = pytest.mark.gpu

SD_ERR_ARG = 1
BLOCK = 256000                                   # samples of a block of 32 chunks


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def stream_state(d, s):
    """everything a stream answers with: turns, confidences, centroids and counts, info, and all cached rows (bytes: NaN payloads included)"""
    turns = s.turns()
    conf = d.last_confidence()
    cen, cnt = d.last_speakers()
    info = s.info()
    seg, emb = s.read(0, info[2])
    return turns, _bits(conf), _bits(cen), list(cnt), info, _bits(seg), _bits(emb)


def whole_path(d, pcm):
    turns = d.diarize(pcm)
    conf = d.last_confidence()
    cen, cnt = d.last_speakers()
    return turns, _bits(conf), _bits(cen), list(cnt)


def assert_is_suffix(d, s, pcm, n, origin):
    """the stream holds samples [origin, n) of pcm and nothing tells it from the whole path, or from a fresh stream, on them"""
    assert s.origin() == origin and origin % BLOCK == 0
    kept = n - origin
    got = stream_state(d, s)
    assert got[4] == (kept, sc.sealed(kept), sc.total(kept)), (n, origin, got[4])
    assert got[:4] == whole_path(d, pcm[origin:n]), (n, origin)
    with d.stream() as f:
        f.push(pcm[origin:n])
        assert f.origin() == 0
        assert stream_state(d, f) == got, (n, origin)
    return got


def forget_by_rule(n, origin, keep_blocks):
    """the origin after forget(keep_blocks) of a stream that holds samples [origin, n)"""
    drop = sc.sealed(n - origin) - 32 * keep_blocks
    return origin + max(0, drop) * sc.HOP


@pytest.mark.parametrize("k", [0, 1, 2])
def test_forget_leaves_a_fresh_stream_of_the_kept_samples(diarizer, k):
    pcm = sc.pcm75()
    d = diarizer
    with d.stream() as s:
        pos = origin = 0
        drops, turns_seen = 0, []
        for n in (600123, 840000, 1200000):
            for e in [e for e in sc.PUSH_ENDS if pos < e <= n]:
                s.push(pcm[pos:e])
                pos = e
            turns_seen.append(len(assert_is_suffix(d, s, pcm, n, origin)[0]))      # after further pushes (the first round: before any forget)
            want = forget_by_rule(n, origin, k)
            s.forget(k)                                                # with pending rows in place ...
            drops += want > origin
            origin = want
            first = assert_is_suffix(d, s, pcm, n, origin)             # ... immediately
            s.forget(k)                                                # nothing left to drop: a no-op
            assert stream_state(d, s) == first and s.origin() == origin
        assert origin == BLOCK * (4 - k) and drops >= (1 if k == 2 else 2) and max(turns_seen) >= 1


def test_forget_with_nothing_sealed_and_the_refusals(diarizer):
    pcm = sc.pcm75()
    d = diarizer
    with d.stream() as s:
        s.forget(0)                                                    # an empty stream
        assert s.origin() == 0 and s.info() == (0, 0, 0)
        s.push(pcm[:300000])                                           # 28 full chunks: nothing sealed
        before = stream_state(d, s)
        for k in (0, 1, 5):
            s.forget(k)
        assert s.origin() == 0 and stream_state(d, s) == before and before[4] == (300000, 0, sc.total(300000))
        s.push(pcm[300000:600123])                                     # two blocks sealed: keeping two or more drops nothing
        s.forget(2)
        s.forget(7)
        assert s.origin() == 0 and s.info()[1] == 64
        for call in (lambda: s.forget(-1), lambda: s.set_window(-2)):
            with pytest.raises(sdhip.SdError) as e:
                call()
            assert e.value.code == SD_ERR_ARG
        assert s.origin() == 0 and s.info() == (600123, 64, sc.total(600123))
        try:
            d.set_option("ecapa_precision", 3)                         # precision options changed: refused like the other calls
            for call in (lambda: s.forget(0), lambda: s.set_window(1)):
                with pytest.raises(sdhip.SdError) as e:
                    call()
                assert e.value.code == SD_ERR_ARG
        finally:
            d.set_option("ecapa_precision", 0)
        assert s.origin() == 0 and s.info() == (600123, 64, sc.total(600123))
        s.set_window(-1)                                               # off: a push that seals forgets nothing
        s.push(pcm[600123:900000])
        assert s.origin() == 0 and s.info()[1] == sc.sealed(900000) == 96


def test_the_window_is_the_forgets_by_hand(diarizer):
    pcm = sc.pcm75()
    d = diarizer
    with d.stream() as w, d.stream() as h:
        w.set_window(1)
        pos = 0
        for n in sc.PUSH_ENDS:
            w.push(pcm[pos:n])
            h.push(pcm[pos:n])
            h.forget(1)
            pos = n
            origin = BLOCK * max(0, sc.sealed(n) // 32 - 1)
            assert w.origin() == h.origin() == origin, n
            assert w.info() == h.info() == (n - origin, sc.sealed(n - origin), sc.total(n - origin)), n
            if n in (336001, 600123, 1200000):
                assert stream_state(d, w) == stream_state(d, h), n
        assert w.origin() == 3 * BLOCK
        assert_is_suffix(d, w, pcm, sc.N, 3 * BLOCK)
        w.set_window(0)                                                # a smaller window takes effect at the next push that seals, not before
        assert w.origin() == 3 * BLOCK


def test_command_line_window_prints_absolute_times(diarizer, weights, golden_dir):
    import os
    import subprocess
    path = os.path.join(golden_dir, "multi-speaker_1min.wav")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")
    pcm, _, _ = sdhip.read_wav(path)
    assert len(pcm) == 944000 and sc.sealed(len(pcm)) == 96
    rule = "-" * 52
    for seconds, blocks in (("16", 1), ("20.5", 2)):                   # ceil(SECONDS / 16) blocks stay
        out = subprocess.run([exe, weights[0], weights[1], path, "--stream", "10", "--stream-window", seconds], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i0 = lines.index(rule)
        got = lines[i0 + 1:lines.index(rule, i0 + 1)]
        origin = BLOCK * (3 - blocks)
        want = [sdhip.format_turn((s + origin / 16000.0, e + origin / 16000.0, k)) for s, e, k in diarizer.diarize(pcm[origin:])]
        assert got == want and len(got) >= 1, seconds
    # the header of an update block gives the seconds pushed; its chunk counts are those of the audio still held
    upd = subprocess.run([exe, weights[0], weights[1], path, "--stream", "10", "--stream-window", "16", "--stream-updates"], capture_output=True, text=True, timeout=600)
    assert upd.returncode == 0, upd.stderr
    heads = [l for l in upd.stdout.splitlines() if l.startswith("== ")]
    held = len(pcm) - 2 * BLOCK
    assert len(heads) == 6 and heads[0] == "== 10 s, 0/11 chunks" and heads[-1] == "== 59 s, %d/%d chunks" % (sc.sealed(held), sc.total(held))


def test_a_windowed_stream_in_a_group_equals_its_twin(diarizer):
    pcm = sc.pcm75()
    other = pcm[100000:]                                               # another recording for the plain stream of the group
    d = diarizer
    with d.stream() as gw, d.stream() as gp, d.stream() as tw, d.stream() as tp:
        gw.set_window(1)
        tw.set_window(1)
        pa = pb = 0
        for na, nb in ((328001, 200000), (600123, 584001), (1200000, 1100000)):      # the last push seals two blocks of the windowed stream at once
            d.stream_push_many([gw, gp], [pcm[pa:na], other[pb:nb]])
            tw.push(pcm[pa:na])
            tp.push(other[pb:nb])
            pa, pb = na, nb
            origin = BLOCK * max(0, sc.sealed(na) // 32 - 1)
            assert gw.origin() == tw.origin() == origin and gp.origin() == tp.origin() == 0
            assert gw.info() == tw.info() and gp.info() == tp.info() == (nb, sc.sealed(nb), sc.total(nb))
            got = d.stream_turns_many([gw, gp])
            group = []
            for i, g in enumerate((gw, gp)):
                d.many_select(i)
                cen, cnt = d.last_speakers()
                seg, emb = g.read(0, g.info()[2])
                group.append((got[i], _bits(d.last_confidence()), _bits(cen), list(cnt), g.info(), _bits(seg), _bits(emb)))
            assert group[0] == stream_state(d, tw), na
            assert group[1] == stream_state(d, tp), nb
        assert gw.origin() == 3 * BLOCK
        assert group[0][:4] == whole_path(d, pcm[3 * BLOCK:])
