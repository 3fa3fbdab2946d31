"""GPU tests of sd_diarize_many* (csrc/many.hip; include/sdhip.h): every recording of a pack gets what sd_diarize gives for it alone on the same
context -- turns, confidences, centroids, counts, enrolled rows -- compared as bytes, whatever shares the pack, in whatever order, under other batch
sizes, in the fp16 mode and with an enrolled gallery; the refusals; the command line's --many.

The lengths are the smallest at which each mechanism of the packed path can go wrong (chunks by slide()'s rule, sd.cpp:1419 / 1457):
  80 000   one chunk, exactly full                      80 001   two chunks, the last one short (72 001 samples)
  88 000   two chunks, the last one exactly full        123 457  seven chunks, a short last chunk of odd length
  203 000  twice, different audio: 16 full chunks -- past the 13 up to which PyanNet's dense layers take the skinny kernel, so the two share
           tile-side batches -- and equal short last chunks          360 000  36 chunks: crosses a 32-chunk slot and the embedding batches of 32 items
  100      one chunk too short for a single frame: zero scores, no turn          1  no chunk: SD_ERR_SHORT"""
import os
import subprocess
import wave

import numpy as np
import pytest

import sdhip
import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
SD_ERR_ARG, SD_ERR_SHORT = 1, 4
LENGTHS = (80000, 80001, 88000, 123457, 203000, 203000, 360000, 100, 1)
SILENT_OK = (100, 1)      # the loop itself gives these no turn


_pcm_cache = {}


def recordings():
    """one recording per length, each with audio of its own (read-only)"""
    if not _pcm_cache:
        for r, n in enumerate(LENGTHS):
            p = synth.make_pcm(n / 16000.0 + 1.0, seed=4100 + r)[:n].copy()
            p.setflags(write=False)
            _pcm_cache[r] = p
        assert not np.array_equal(_pcm_cache[4], _pcm_cache[5])
    return [_pcm_cache[r] for r in range(len(LENGTHS))]


def job_bytes(d):
    cen, cnt = d.last_speakers()
    return d.last_confidence().tobytes(), cen.tobytes(), cnt.tobytes(), d.last_enrolled().tobytes()


def turn_bytes(turns):
    return np.array([(s, e, l) for s, e, l in turns], np.float64).tobytes()


def loop(d, recs):
    """the plain loop of sd_diarize calls: per recording (turns | error code, the job's bytes)"""
    out = []
    for p in recs:
        try:
            t = d.diarize(p)
            out.append((t, job_bytes(d)))
        except sdhip.SdError as e:
            out.append((e.code, None))
    return out


def check_pack(d, recs, want, tag):
    got = d.diarize_many(recs)
    assert len(got) == len(recs)
    for r, (g, (t, job)) in enumerate(zip(got, want)):
        print("%s: recording %d (%d samples): %s" % (tag, r, len(recs[r]), "%d turns" % len(t) if isinstance(t, list) else "code %d" % t))
        if not isinstance(t, list):
            assert g == t, (tag, r)
            with pytest.raises(sdhip.SdError) as e:
                d.many_select(r)
            assert e.value.code == SD_ERR_ARG
            continue
        assert isinstance(g, list) and len(g) == len(t) and turn_bytes(g) == turn_bytes(t), (tag, r)
        d.many_select(r)
        assert job_bytes(d) == job, (tag, r)
    return got


def test_pack_equals_the_loop_in_any_order_and_alone(diarizer):
    recs = recordings()
    want = loop(diarizer, recs)
    for p, (t, _) in zip(recs, want):
        if len(p) == 1:
            assert t == SD_ERR_SHORT
        else:
            assert isinstance(t, list) and (len(t) >= 1 or len(p) in SILENT_OK), len(p)
    assert want[7][0] == []
    got = check_pack(diarizer, recs, want, "forward")
    assert got[8] == SD_ERR_SHORT
    ms = diarizer.stage_ms()
    assert ms[0] > 0 and ms[1] > 0 and ms[2] > 0 and ms[3] >= ms[0] + ms[1] + ms[2] - 1e-6
    check_pack(diarizer, recs[::-1], want[::-1], "reverse")
    for r in (3, 6, 8):
        check_pack(diarizer, [recs[r]], [want[r]], "alone %d" % r)
    # the f32 and device forms read the same samples
    f32 = diarizer.diarize_many_f32([p.astype(np.float32) / np.float32(32768.0) for p in recs])
    assert [g if isinstance(g, int) else turn_bytes(g) for g in f32] == [g if isinstance(g, int) else turn_bytes(g) for g in got]
    import torch
    dev = [torch.from_numpy(np.array(p)).to("cuda:0") for p in recs]
    torch.cuda.synchronize()
    on_dev = diarizer.diarize_many_dev([t.data_ptr() for t in dev], [len(p) for p in recs])
    assert [g if isinstance(g, int) else turn_bytes(g) for g in on_dev] == [g if isinstance(g, int) else turn_bytes(g) for g in got]


def test_batch_boundaries_inside_and_across_recordings(diarizer):
    recs = recordings()
    diarizer.set_option("seg_batch_chunks", 7)
    diarizer.set_option("emb_batch_items", 96)
    try:
        check_pack(diarizer, recs, loop(diarizer, recs), "batches 7 / 96")
        diarizer.set_option("seg_batch_chunks", 20)      # 36 chunks = batches of 20 and 16, both past the skinny kernel's 13; 6 full chunks stay on it
        check_pack(diarizer, recs, loop(diarizer, recs), "batches 20 / 96")
    finally:
        diarizer.set_option("seg_batch_chunks", 4096)
        diarizer.set_option("emb_batch_default", 1)


def test_fp16_mode(diarizer):
    recs = recordings()
    diarizer.set_option("ecapa_precision", 1)
    try:
        check_pack(diarizer, recs, loop(diarizer, recs), "ecapa_precision 1")
    finally:
        diarizer.set_option("ecapa_precision", 0)


def test_enrolled_gallery_applies_to_every_recording(diarizer):
    recs = recordings()
    diarizer.diarize(recs[6])
    cen, cnt = diarizer.last_speakers()
    assert len(cnt) >= 1 and cnt.max() >= 1
    diarizer.set_enrolled(cen[int(np.argmax(cnt))][None, :])      # the voiceprint of the dominant speaker of the 36-chunk recording
    try:
        want = loop(diarizer, recs)
        assert (np.frombuffer(want[6][1][3], np.int32) == 0).any()      # that recording finds its own speaker again
        check_pack(diarizer, recs, want, "enrolled")
    finally:
        diarizer.set_enrolled(None)


def test_refusals_touch_nothing(diarizer, tmp_path):
    import ctypes as C
    import torch
    recs = recordings()
    before = diarizer.diarize(recs[3])
    job = job_bytes(diarizer)
    L = sdhip.lib()

    def raw(rows, n, R):
        turns, nt, st = (C.c_void_p * 4)(), (C.c_int64 * 4)(7, 7, 7, 7), (C.c_int32 * 4)(7, 7, 7, 7)
        rc = L.sd_diarize_many(diarizer._h, rows, n, R, turns, nt, st)
        assert list(nt) == [7] * 4 and list(st) == [7] * 4 and not any(turns)
        return rc

    two = (C.c_void_p * 2)(recs[0].ctypes.data, recs[2].ctypes.data)
    n2 = (C.c_int64 * 2)(len(recs[0]), len(recs[2]))
    assert raw(two, n2, 0) == SD_ERR_ARG and raw(two, n2, -3) == SD_ERR_ARG
    assert raw((C.c_void_p * 2)(recs[0].ctypes.data, None), n2, 2) == SD_ERR_ARG
    assert raw(two, (C.c_int64 * 2)(len(recs[0]), 8000 * (sdhip_max_chunks() + 40)), 2) == SD_ERR_ARG      # the pack's row counts would leave int
    diarizer.set_dump_dir(str(tmp_path))
    try:
        assert raw(two, n2, 2) == SD_ERR_ARG
    finally:
        diarizer.set_dump_dir(None)
    sc = torch.zeros((2, 293, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    diarizer.set_planted(sc.data_ptr(), 0, 0, 2)
    try:
        assert raw(two, n2, 2) == SD_ERR_ARG
    finally:
        diarizer.set_planted(0, 0, 0, 0)
    assert not os.listdir(str(tmp_path))
    assert job_bytes(diarizer) == job                                 # the last job is still the one from before
    again = diarizer.diarize(recs[3])
    assert turn_bytes(again) == turn_bytes(before) and job_bytes(diarizer) == job
    ok = diarizer.diarize_many([recs[0], recs[2]])                    # ... and the same recordings are accepted once nothing stands in the way
    assert all(isinstance(t, list) for t in ok)


def sdhip_max_chunks():
    import re
    hdr = open(os.path.join(ROOT, "include", "sdhip.h")).read()
    return int(re.search(r"#define SD_MANY_MAX_CHUNKS (\d+)", hdr).group(1))


def _write_wav(path, pcm):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(np.ascontiguousarray(pcm, "<i2").tobytes())


def test_cli_many_prints_what_the_single_file_runs_print(weights, tmp_path):
    recs = recordings()
    exe = os.path.join(PKG, "speakerDiarizer")
    paths = []
    for r in (0, 3, 4):
        paths.append(str(tmp_path / ("rec%d.wav" % r)))
        _write_wav(paths[-1], recs[r])
    missing = str(tmp_path / "absent.wav")
    lst = tmp_path / "list.txt"
    lst.write_text("# three recordings and one that is not there\n" + paths[0] + "\n" + missing + "\n\n" + paths[1] + "\r\n" + paths[2])
    single = []
    for p in paths:
        out = subprocess.run([exe, weights[0], weights[1], p], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        single.append([l for l in out.stdout.splitlines() if l.startswith("[")])
    assert all(len(s) >= 1 for s in single)
    rttm = tmp_path / "rttm"
    rttm.mkdir()
    out = subprocess.run([exe, weights[0], weights[1], "--many", str(lst), "--rttm", str(rttm)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 1, out.stderr                             # one file of the list could not be read
    blocks, cur = {}, None
    for l in out.stdout.splitlines():
        if l.startswith("== "):
            cur = l[3:]
            blocks[cur] = []
        else:
            blocks[cur].append(l)
    assert list(blocks) == [paths[0], missing + ": cannot read PCM wav", paths[1], paths[2]]
    for p, s in zip(paths, single):
        assert blocks[p] == s, p
        lines = open(str(rttm / (os.path.basename(p)[:-4] + ".rttm"))).read().splitlines()
        assert len(lines) == len(s) and all(l.startswith("SPEAKER " + p + " 1 ") for l in lines)
    out = subprocess.run([exe, weights[0], weights[1], "--many", str(lst), "--stream", "1"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "--many" in out.stderr


def test_cli_many_reads_off_rate_and_stereo_files_as_the_single_file_run_does(weights, tmp_path):
    """--many under --resample, --downmix and --assume-16k: each file's block holds the turn lines of the single-file run with the flags that affect that
    file; without a flag the 44.1 kHz file is refused in its block, with the reason, and the others are diarized"""
    import struct
    exe = os.path.join(PKG, "speakerDiarizer")
    rule = "-" * 52

    def wav(path, samples, sr, channels=1):
        data = np.asarray(samples, np.int16).tobytes()
        fmt = struct.pack("<HHIIHH", 1, channels, sr, sr * channels * 2, channels * 2, 16)
        path.write_bytes(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data)

    def single(args):
        out = subprocess.run([exe, weights[0], weights[1]] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i0 = lines.index(rule)
        return lines[i0 + 1:lines.index(rule, i0 + 1)]

    def many(flags):
        out = subprocess.run([exe, weights[0], weights[1], "--many", str(lst)] + flags, capture_output=True, text=True, timeout=300)
        blocks, cur = {}, None
        for l in out.stdout.splitlines():
            if l.startswith("== "):
                cur = l[3:]
                blocks[cur] = []
            else:
                blocks[cur].append(l)
        return out, blocks

    pcm = synth.make_pcm(21.0, seed=3)
    t44 = np.arange(int(len(pcm) * 44100 / 16000)) * (16000.0 / 44100.0)
    pcm44 = np.rint(np.interp(t44, np.arange(len(pcm)), pcm.astype(np.float64))).astype(np.int16)
    left = pcm.astype(np.int32)
    right = np.roll(left, 4000) // 2
    m44, st = str(tmp_path / "m44.wav"), str(tmp_path / "st.wav")
    wav(tmp_path / "m44.wav", pcm44, 44100)
    wav(tmp_path / "st.wav", np.stack([left, right], 1).reshape(-1), 16000, channels=2)
    lst = tmp_path / "list.txt"
    lst.write_text(m44 + "\n" + st + "\n")
    st_plain = single([st])
    assert len(st_plain) >= 1
    for flags, want44, want_st in ((["--resample"], single([m44, "--resample"]), st_plain),
                                   (["--assume-16k", "--downmix"], single([m44, "--assume-16k"]), single([st, "--downmix"]))):
        assert len(want44) >= 1 and len(want_st) >= 1
        out, blocks = many(flags)
        assert out.returncode == 0, out.stderr
        assert list(blocks) == [m44, st] and blocks[m44] == want44 and blocks[st] == want_st, flags
    out, blocks = many([])
    assert out.returncode == 1
    head = [b for b in blocks if b.startswith(m44 + ": ")]
    assert list(blocks) == head + [st] and len(head) == 1 and "44100" in head[0] and "--resample" in head[0]
    assert blocks[head[0]] == [] and blocks[st] == st_plain
