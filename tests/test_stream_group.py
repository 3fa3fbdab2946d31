"""GPU tests of the group calls of the incremental path (sd_stream_push_many*, sd_stream_turns_many; csrc/stream.hip): after any sequence
of group and single calls every stream holds the bytes it holds when it is driven alone -- info, turns or error code, confidences, centroids, counts,
enrolled rows, cached scores and embeddings -- whatever shares the call, in whatever order, under other batch sizes, in the fp16 mode and with an
enrolled gallery; the refusals; that a call leaves alone what has nothing to do in it.

Real seeded networks on synth.make_pcm audio, a stream per final length, each with audio of its own.  The lengths are the smallest at which each
mechanism can go wrong (chunks by slide()'s rule, sd.cpp:1419 / 1457; a block of 32 chunks is sealed once 32 chunks end in front of the last sample):
  1        no chunk: SD_ERR_SHORT                          100      one chunk, no frame
  80 001   two chunks, the last one short                  123 457  7 chunks: the skinny side, a batch of its own
  203 000  16 full chunks: the tile side, nothing sealed   328 000  31 full chunks + 1: one sample short of sealing
  328 001  seals exactly one block, a short last chunk behind it
  360 000  one block + 4 pending chunks: a tile-side range shorter than 14, which reaches forward into its slot's zero chunks
  600 000  two blocks, sealed in ONE call
Three rounds of pushes (ENDS) with uneven pieces: the 360 000 stream seals in round 1, the 600 000 one both blocks in round 2, the 328 001 one in
round 3; six pieces are empty."""
import ctypes as C

import numpy as np
import pytest

import sdhip
import synth

pytestmark = pytest.mark.gpu

SD_ERR_ARG, SD_ERR_HIP, SD_ERR_SHORT = 1, 2, 4
LENGTHS = (1, 100, 80001, 123457, 203000, 328000, 328001, 360000, 600000)
ENDS = ((0, 1, 1), (100, 100, 100), (30000, 80000, 80001), (0, 100001, 123457), (203000, 203000, 203000), (150000, 327999, 328000),
        (100000, 328000, 328001), (330000, 340000, 360000), (20000, 590000, 600000))
ROUNDS = 3

_pcm_cache = {}
_solo_cache = {}


def recordings():
    """one recording per final length, each with audio of its own (read-only)"""
    if not _pcm_cache:
        for r, n in enumerate(LENGTHS):
            p = synth.make_pcm(n / 16000.0 + 1.0, seed=5200 + r)[:n].copy()
            p.setflags(write=False)
            _pcm_cache[r] = p
    return [_pcm_cache[r] for r in range(len(LENGTHS))]


def piece(r, k):
    return recordings()[r][(ENDS[r][k - 1] if k else 0):ENDS[r][k]]


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def turn_bytes(turns):
    return np.array([(s, e, l) for s, e, l in turns], np.float64).tobytes()


def job_bytes(d):
    cen, cnt = d.last_speakers()
    return d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes(), d.last_enrolled().tobytes()


def state(s):
    """what a stream holds after a turns call: (info, scores, embeddings) of every chunk"""
    info = s.info()
    seg, emb = s.read(0, info[2])
    return info, seg, emb


def same_state(a, b):
    return a[0] == b[0] and same_bits(a[1], b[1]) and same_bits(a[2], b[2])


def solo(d, key=""):
    """every stream driven alone with push / turns: per round and stream (turns | code, job bytes | None, state).  Computed once per configuration
    (key names the options the caller has set) and shared by the tests"""
    if key not in _solo_cache:
        out = []
        streams = [d.stream() for _ in LENGTHS]
        try:
            for k in range(ROUNDS):
                row = []
                for r, s in enumerate(streams):
                    s.push(piece(r, k))
                    assert s.info()[0] == ENDS[r][k]
                    try:
                        t = s.turns()
                        row.append((t, job_bytes(d), state(s)))
                    except sdhip.SdError as e:
                        row.append((e.code, None, state(s)))
                out.append(row)
        finally:
            for s in streams:
                s.close()
        _solo_cache[key] = out
    return _solo_cache[key]


def push_group(d, streams, rows, k, form="pcm"):
    pcs = [piece(r, k) for r in rows]
    if form == "pcm":
        d.stream_push_many(streams, pcs)
    elif form == "f32":
        d.stream_push_many_f32(streams, [p.astype(np.float32) / np.float32(32768.0) for p in pcs])
    else:
        import torch
        dev = [torch.from_numpy(np.array(p)).to("cuda:0") if len(p) else None for p in pcs]
        torch.cuda.synchronize()
        d.stream_push_many_dev(streams, [t.data_ptr() if t is not None else 0 for t in dev], [len(p) for p in pcs])


def check_group(d, want, rows, tag, form="pcm"):
    """the streams `rows` of the table driven through the group calls, in this order of the list; every round against the streams driven alone"""
    streams = [d.stream() for _ in rows]
    try:
        for k in range(ROUNDS):
            push_group(d, streams, rows, k, form)
            for s, r in zip(streams, rows):
                n = ENDS[r][k]
                assert s.info() == (n, sdhip.sealed_chunks(n), sdhip.num_chunks(n)[0]), (tag, k, r)
            got = d.stream_turns_many(streams)
            assert len(got) == len(rows)
            for i, (s, r) in enumerate(zip(streams, rows)):
                t, job, st = want[k][r]
                print("%s: round %d, stream of %d samples at %d: %s" % (tag, k, LENGTHS[r], ENDS[r][k], "%d turns" % len(t) if isinstance(t, list) else "code %d" % t))
                if not isinstance(t, list):
                    assert got[i] == t, (tag, k, r)
                    with pytest.raises(sdhip.SdError) as e:
                        d.many_select(i)
                    assert e.value.code == SD_ERR_ARG
                else:
                    assert isinstance(got[i], list) and turn_bytes(got[i]) == turn_bytes(t), (tag, k, r)
                    d.many_select(i)
                    assert job_bytes(d) == job, (tag, k, r)
                assert same_state(state(s), st), (tag, k, r)
    finally:
        for s in streams:
            s.close()


def test_group_calls_equal_the_streams_driven_alone_and_the_whole_path(diarizer):
    recs = recordings()
    want = solo(diarizer)
    assert want[0][0][0] == want[2][0][0] == SD_ERR_SHORT and want[2][1][0] == []
    for r in range(2, len(LENGTHS)):
        assert len(want[2][r][0]) >= 1, LENGTHS[r]
        assert turn_bytes(want[2][r][0]) == turn_bytes(diarizer.diarize(recs[r])), LENGTHS[r]      # the last round: sd_diarize of the concatenation
    assert [want[2][r][2][0][1] for r in range(len(LENGTHS))] == [0, 0, 0, 0, 0, 0, 32, 32, 64]
    check_group(diarizer, want, list(range(len(LENGTHS))), "forward")
    ms = diarizer.stage_ms()
    assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[3] >= ms[0] + ms[1] + ms[2] - 1e-6


def test_list_order_and_a_list_of_one_do_not_matter(diarizer):
    want = solo(diarizer)
    check_group(diarizer, want, list(range(len(LENGTHS)))[::-1], "reverse")
    for r in (0, 3, 6, 7, 8):
        check_group(diarizer, want, [r], "alone %d" % r)


@pytest.mark.parametrize("cb", [7, 33])
def test_other_segmentation_batch_sizes(diarizer, cb):
    diarizer.set_option("seg_batch_chunks", cb)
    try:
        check_group(diarizer, solo(diarizer, "cb%d" % cb), list(range(len(LENGTHS))), "batches of %d" % cb)
    finally:
        diarizer.set_option("seg_batch_chunks", 4096)


def test_single_and_group_calls_mix_and_fresh_rows_are_not_inferred_again(diarizer):
    want = solo(diarizer)
    rows = (3, 7, 8)
    launches = lambda: diarizer.kernel_stats("lstm_rec")["launches"]
    streams = [diarizer.stream() for _ in rows]
    try:
        for s, r in zip(streams, rows):
            s.push(piece(r, 0))                                  # alone
        push_group(diarizer, streams, rows, 1)                   # in a group
        for i, (s, r) in enumerate(zip(streams, rows)):          # its own turns() ...
            t = s.turns()
            assert turn_bytes(t) == turn_bytes(want[1][r][0]) and job_bytes(diarizer) == want[1][r][1] and same_state(state(s), want[1][r][2]), r
        before = [state(s) for s in streams]
        diarizer.reset_stats()
        got = diarizer.stream_turns_many(streams)                # ... then the group's: pending_n == n everywhere, nothing goes through a network
        assert launches() == 0
        for i, (s, r) in enumerate(zip(streams, rows)):
            assert turn_bytes(got[i]) == turn_bytes(want[1][r][0]), r
            diarizer.many_select(i)
            assert job_bytes(diarizer) == want[1][r][1] and same_state(state(s), before[i]), r
        push_group(diarizer, streams, rows, 2)
        assert launches() == 0                                   # round 3 seals nothing in these three
        got = diarizer.stream_turns_many(streams[:2])            # the group's turns for two, its own for the third
        assert launches() > 0
        t2 = streams[2].turns()
        for i, (s, r) in enumerate(zip(streams, rows)):
            assert turn_bytes(got[i] if i < 2 else t2) == turn_bytes(want[2][r][0]) and same_state(state(s), want[2][r][2]), r
    finally:
        diarizer.reset_stats()
        for s in streams:
            s.close()


@pytest.mark.parametrize("form", ["f32", "dev"])
def test_float_and_device_pushes_give_the_bytes_of_the_16_bit_host_push(diarizer, form):
    check_group(diarizer, solo(diarizer), list(range(len(LENGTHS))), form, form=form)


def test_enrolled_gallery_applies_to_every_stream(diarizer):
    diarizer.diarize(recordings()[7])
    cen, cnt = diarizer.last_speakers()
    assert len(cnt) >= 1 and cnt.max() >= 1
    diarizer.set_enrolled(cen[int(np.argmax(cnt))][None, :])      # the voiceprint of the dominant speaker of the 360 000-sample recording
    try:
        want = solo(diarizer, "enrolled")
        assert (np.frombuffer(want[2][7][1][3], np.int32) == 0).any()      # that stream finds its own speaker again
        check_group(diarizer, want, list(range(len(LENGTHS))), "enrolled")
    finally:
        diarizer.set_enrolled(None)


def test_fp16_mode(diarizer):
    diarizer.set_option("ecapa_precision", 1)
    try:
        check_group(diarizer, solo(diarizer, "prec1"), list(range(len(LENGTHS))), "ecapa_precision 1")
    finally:
        diarizer.set_option("ecapa_precision", 0)


def test_refusals_touch_nothing(diarizer, weights, tmp_path):
    import torch
    L = sdhip.lib()
    want = solo(diarizer)
    rows = (7, 2)
    a, b = diarizer.stream(), diarizer.stream()
    other = sdhip.Diarizer(weights[0], weights[1])
    try:
        push_group(diarizer, [a, b], rows, 0)
        assert all(isinstance(t, list) for t in diarizer.stream_turns_many([a, b]))
        before = [state(a), state(b)]
        more = piece(8, 1)
        two = (C.c_void_p * 2)(a._s.value, b._s.value)
        pcm2 = (C.c_void_p * 2)(more.ctypes.data, more.ctypes.data)
        n2 = (C.c_int64 * 2)(len(more), len(more))

        def push(hs, pcm, n, S):
            return [f(hs, pcm, n, S) for f in (L.sd_stream_push_many, L.sd_stream_push_many_f32, L.sd_stream_push_many_dev)]

        def turns(hs, S, with_arrays=True):
            tp, nt, st = (C.c_void_p * 2)(), (C.c_int64 * 2)(7, 7), (C.c_int32 * 2)(7, 7)
            rc = L.sd_stream_turns_many(hs, S, tp if with_arrays else None, nt, st)
            assert list(nt) == [7, 7] and list(st) == [7, 7] and not any(tp)
            return rc

        def refused(hs, pcm=pcm2, n=n2, S=2):
            assert push(hs, pcm, n, S) == [SD_ERR_ARG] * 3
            assert turns(hs, S) == SD_ERR_ARG

        refused(None)
        refused(two, S=0)
        refused(two, S=-1)
        refused((C.c_void_p * 2)(a._s.value, None))                                       # a null stream
        refused((C.c_void_p * 2)(a._s.value, a._s.value))                                 # the same stream twice
        assert push(two, None, n2, 2) == push(two, pcm2, None, 2) == [SD_ERR_ARG] * 3     # null arrays
        assert turns(two, 2, with_arrays=False) == SD_ERR_ARG
        assert push(two, (C.c_void_p * 2)(more.ctypes.data, None), n2, 2) == [SD_ERR_ARG] * 3      # a null sample pointer with n > 0
        assert push(two, pcm2, (C.c_int64 * 2)(len(more), -1), 2) == [SD_ERR_ARG] * 3
        with other.stream() as far:                                                       # streams of two contexts, either first
            refused((C.c_void_p * 2)(a._s.value, far._s.value))
            refused((C.c_void_p * 2)(far._s.value, a._s.value))
            assert far.info() == (0, 0, 0)
        diarizer.set_option("ecapa_precision", 1)                                         # another precision than the streams were opened under
        try:
            refused(two)
        finally:
            diarizer.set_option("ecapa_precision", 0)
        sc = torch.zeros((2, 293, 3), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        diarizer.set_planted(sc.data_ptr(), 0, 0, 2)
        try:
            refused(two)
        finally:
            diarizer.set_planted(0, 0, 0, 0)
        diarizer.set_dump_dir(str(tmp_path))
        try:
            assert turns(two, 2) == SD_ERR_ARG
        finally:
            diarizer.set_dump_dir(None)
        assert not list(tmp_path.iterdir())
        assert same_state(state(a), before[0]) and same_state(state(b), before[1])

        # SD_ERR_HIP in the middle of a group call (a workspace request refused like an exhausted GPU): every stream of the call is unusable, and a
        # list that holds one of them is refused
        with other.stream() as p, other.stream() as q, other.stream() as fresh:
            other.set_option("ws_limit_mb", 1)
            try:
                with pytest.raises(sdhip.SdError) as e:
                    other.stream_push_many([p, q], [recordings()[8], recordings()[7]])
                assert e.value.code == SD_ERR_HIP
            finally:
                other.set_option("ws_limit_mb", 0)
            for call in (lambda: other.stream_push_many([fresh, q], [more, more]), lambda: other.stream_turns_many([fresh, p])):
                with pytest.raises(sdhip.SdError) as e:
                    call()
                assert e.value.code == SD_ERR_ARG
            assert fresh.info() == (0, 0, 0)

        # ... and the same two streams go on once nothing stands in the way; a stream without a chunk has its code and the others their turns
        with diarizer.stream() as empty:
            diarizer.stream_push_many([a, empty, b], [piece(7, 1), recordings()[0], piece(2, 1)])
            got = diarizer.stream_turns_many([a, empty, b])
            assert got[1] == SD_ERR_SHORT and turn_bytes(got[0]) == turn_bytes(want[1][7][0]) and turn_bytes(got[2]) == turn_bytes(want[1][2][0])
            assert same_state(state(a), want[1][7][2]) and same_state(state(b), want[1][2][2])
    finally:
        a.close()
        b.close()
        other.close()


def test_a_group_call_changes_no_row_of_a_stream_with_nothing_to_do(diarizer):
    """neighbours in the list and outside it: a stream that gets no sample and seals nothing keeps every cached row and its pending rows' freshness
    through the pushes and inferences of the others; one outside the list likewise.  The rows behind `total` in a cache and the floats behind a tail's
    padding belong to later chunks and samples of the same stream: that they are intact is what the equalities of the later rounds in this file rest on"""
    want = solo(diarizer)
    idle, outside, busy1, busy2 = (diarizer.stream() for _ in range(4))
    try:
        for s, r in ((idle, 7), (outside, 6)):
            for k in range(ROUNDS):
                s.push(piece(r, k))
            s.turns()
        keep = [state(idle), state(outside)]
        assert same_state(keep[0], want[2][7][2]) and same_state(keep[1], want[2][6][2])
        none = np.zeros(0, np.int16)
        for k in range(ROUNDS):
            diarizer.stream_push_many([busy1, idle, busy2], [piece(8, k), none, piece(5, k)])
            assert same_state(state(idle), keep[0]) and same_state(state(outside), keep[1]), k      # (read() refuses stale pending rows: they are still fresh)
            got = diarizer.stream_turns_many([busy1, idle, busy2])
            assert turn_bytes(got[1]) == turn_bytes(want[2][7][0]) and turn_bytes(got[0]) == turn_bytes(want[k][8][0])
            assert same_state(state(idle), keep[0]) and same_state(state(outside), keep[1]), k
            assert same_state(state(busy1), want[k][8][2]) and same_state(state(busy2), want[k][5][2]), k
        assert turn_bytes(outside.turns()) == turn_bytes(want[2][6][0])
    finally:
        for s in (idle, outside, busy1, busy2):
            s.close()
