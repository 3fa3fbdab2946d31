"""GPU tests of sd_diarize_many_audio* (csrc/many.hip, csrc/ingest.hip; include/sdhip.h, "recordings in their own rate and encoding") on the seeded
networks: every recording of a pack -- mu-law 8 kHz mono, A-law 8 kHz stereo of which channel 1 is taken, int16 44.1 kHz as the mean of two channels,
float 16 kHz, int16 16 kHz, 0.2 s, and recordings without a chunk -- gets, byte for byte, what diarize_f32 gives for its 16 kHz mono samples y_r alone:
turns, confidences, centroids, counts, status.  y_r is built on the host from the reference decode (tests/ingest_ref.py) and the library's own
sd_resample.

The 0.2 s recording has one short chunk by slide()'s rule (sd.cpp:1457: any two samples make a chunk), so its status is what diarize_f32 gives for it;
SD_ERR_SHORT is shown by the recordings whose y has no chunk: n = 0, and one frame at 16 kHz."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import ingest_ref as G
import sdhip
import synth
from test_many import job_bytes, turn_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
SD_ERR_ARG, SD_ERR_SHORT = 1, 4


def encode(table, v):
    """the code of each law nearest to the int16 values v"""
    order = np.argsort(table, kind="stable")
    s = table[order]
    i = np.clip(np.searchsorted(s, v), 1, 255)
    pick = np.where(np.abs(s[i - 1] - v) <= np.abs(s[i] - v), i - 1, i)
    return order[pick].astype(np.uint8)


def at_rate(pcm, sr):
    t = np.arange(int(len(pcm) * sr / 16000)) * (16000.0 / sr)
    return np.rint(np.interp(t, np.arange(len(pcm)), pcm.astype(np.float64))).astype(np.int16)


_cache = {}


def recordings():
    """[(name, elements, sample_rate, encoding, channels, channel)], read-only"""
    if not _cache:
        a, b, c, d, e, f = (synth.make_pcm(sec, seed=5200 + i) for i, sec in enumerate((11.0, 7.0, 9.0, 25.0, 6.0, 0.2)))
        a8, b8 = a[::2], b[::2]
        other = (np.roll(b8.astype(np.int32), 1234) // 3).astype(np.int16)
        c44 = at_rate(c, 44100)
        side = (np.roll(c44.astype(np.int32), 999) // 2).astype(np.int16)
        recs = [("mulaw_8k", encode(G.mulaw_table(), a8), 8000, G.ENC_MULAW, 1, 0),
                ("alaw_8k_stereo_ch1", np.stack([encode(G.alaw_table(), other), encode(G.alaw_table(), b8)], 1).reshape(-1), 8000, G.ENC_ALAW, 2, 1),
                ("s16_44k_mean", np.stack([c44, side], 1).reshape(-1), 44100, G.ENC_S16, 2, -1),
                ("f32_16k", (d.astype(np.float32) / np.float32(32768.0)), 16000, G.ENC_F32, 1, 0),
                ("s16_16k", e, 16000, G.ENC_S16, 1, 0),
                ("s16_16k_0.2s", f, 16000, G.ENC_S16, 1, 0),
                ("mulaw_8k_empty", np.zeros(0, np.uint8), 8000, G.ENC_MULAW, 1, 0),
                ("f32_16k_one_frame", np.full(1, 0.25, np.float32), 16000, G.ENC_F32, 1, 0)]
        for r in recs:
            r[1].setflags(write=False)
        _cache["recs"] = recs
    return _cache["recs"]


def audio(rec):
    _, el, sr, enc, ch, c = rec
    return sdhip.Audio(el, sr, enc, ch, c)


def host_samples(d, rec):
    """y_r: the reference decode and channel rule, then the library's own sd_resample"""
    name, el, sr, enc, ch, c = rec
    if name not in _cache:
        x = G.frames(el, enc, ch, c, len(el) // ch)
        y = x if sr == 16000 or len(x) == 0 else d.resample(x, sr)
        assert len(y) == sdhip.audio_len16(audio(rec)) == G.len16(len(x), sr)
        y.setflags(write=False)
        _cache[name] = y
    return _cache[name]


def alone(d, recs):
    """per recording what diarize_f32 gives for y_r alone: (turns | error code, the job's bytes)"""
    if "alone" not in _cache:
        out = []
        for rec in recs:
            y = host_samples(d, rec)
            try:
                t = d.diarize_f32(y) if len(y) else SD_ERR_SHORT
                out.append((t, job_bytes(d)) if isinstance(t, list) else (t, None))
            except sdhip.SdError as e:
                out.append((e.code, None))
        _cache["alone"] = out
    return _cache["alone"]


def check(d, got, want, tag):
    assert len(got) == len(want)
    for r, (g, (t, job)) in enumerate(zip(got, want)):
        if not isinstance(t, list):
            assert g == t, (tag, r)
            with pytest.raises(sdhip.SdError):
                d.many_select(r)
            continue
        assert isinstance(g, list) and turn_bytes(g) == turn_bytes(t), (tag, r)
        d.many_select(r)
        assert job_bytes(d) == job, (tag, r)


def test_every_recording_equals_diarize_f32_of_its_16_khz_samples_in_two_orders(diarizer):
    recs = recordings()
    want = alone(diarizer, recs)
    for rec, (t, _) in zip(recs[:5], want):
        assert isinstance(t, list) and len(t) >= 1, rec[0]
    assert isinstance(want[5][0], list) and want[6][0] == SD_ERR_SHORT and want[7][0] == SD_ERR_SHORT
    check(diarizer, diarizer.diarize_many_audio([audio(r) for r in recs]), want, "forward")
    order = [7, 2, 0, 6, 4, 1, 5, 3]
    check(diarizer, diarizer.diarize_many_audio([audio(recs[i]) for i in order]), [want[i] for i in order], "shuffled")


def test_the_packed_waveform_is_the_one_many_f32_leaves_and_the_launch_counts(diarizer):
    recs = recordings()
    ys = [host_samples(diarizer, r) for r in recs]
    live = [y for y in ys if len(y) > 1]
    _, total = sdhip.many_plan([len(y) for y in live])
    count = total * 8000 + 512
    names = ("many_ingest", "resample", "resample_jobs", "many_pack", "stft_mel", "lstm_rec", "asp_pool", "binarize_masks")
    diarizer.diarize_many_audio([audio(r) for r in recs])                        # (the tap tables are built and cached here)

    def counted(call):
        diarizer.reset_stats()
        out = call()
        return out, {k: diarizer.kernel_stats(k)["launches"] for k in names}

    f32, before = counted(lambda: diarizer.diarize_many_f32(live))
    pack_f32 = diarizer.read_ws("many_wav", np.float32, count)
    got, mine = counted(lambda: diarizer.diarize_many_audio([audio(r) for r in recs]))
    pack = diarizer.read_ws("many_wav", np.float32, count)
    assert pack.tobytes() == pack_f32.tobytes() and not np.isnan(pack).any() and np.abs(pack).max() > 0.01
    assert mine["many_ingest"] == 1 and mine["resample"] == 0 and mine["resample_jobs"] == 0 and mine["many_pack"] == 0
    assert {k: v for k, v in mine.items() if k != "many_ingest"} == {k: v for k, v in before.items() if k != "many_ingest"}
    f32_again, after = counted(lambda: diarizer.diarize_many_f32(live))
    assert before["many_ingest"] == 0 and after == before and before["lstm_rec"] > 0 and before["stft_mel"] > 0
    key = lambda out: [g if isinstance(g, int) else turn_bytes(g) for g in out]
    assert key(f32) == key(f32_again) == key([g for g, y in zip(got, ys) if len(y) > 1])


def test_int16_16_khz_call_equals_diarize_many_and_the_dev_form_the_host_form(diarizer):
    import torch
    recs = recordings()
    key = lambda out: [g if isinstance(g, int) else turn_bytes(g) for g in out]
    pcm = [recs[4][1], recs[5][1], recs[4][1][:88001]]
    plain = diarizer.diarize_many(pcm)
    jobs = []
    for r in range(len(pcm)):
        diarizer.many_select(r)
        jobs.append(job_bytes(diarizer))
    mine = diarizer.diarize_many_audio([sdhip.Audio(p, 16000, G.ENC_S16) for p in pcm])
    assert key(mine) == key(plain)
    for r in range(len(pcm)):
        diarizer.many_select(r)
        assert job_bytes(diarizer) == jobs[r]
    host = diarizer.diarize_many_audio([audio(r) for r in recs])
    dev = [torch.from_numpy(np.array(r[1]).view(np.uint8)).to("cuda:0") if len(r[1]) else None for r in recs]
    torch.cuda.synchronize()
    on_dev = diarizer.diarize_many_audio_dev([sdhip.Audio(t.data_ptr() if t is not None else 0, r[2], r[3], r[4], r[5], n=len(r[1]) // r[4]) for t, r in zip(dev, recs)])
    assert key(on_dev) == key(host)


def test_refusals_name_the_recording_and_touch_nothing(diarizer, tmp_path):
    import torch
    recs = recordings()
    good = [audio(recs[4]), audio(recs[0])]
    key = lambda out: [g if isinstance(g, int) else turn_bytes(g) for g in out]
    before = key(diarizer.diarize_many_audio(good))
    diarizer.many_select(1)
    job = job_bytes(diarizer)
    L = sdhip.lib()

    def refused(descs, fn=None, names=None):
        arr = (sdhip.AudioDesc * len(descs))(*descs)
        turns, nt, st = (C.c_void_p * 4)(), (C.c_int64 * 4)(7, 7, 7, 7), (C.c_int32 * 4)(7, 7, 7, 7)
        rc = (fn or L.sd_diarize_many_audio)(diarizer._h, arr, len(descs), turns, nt, st)
        assert rc == SD_ERR_ARG and list(nt) == [7] * 4 and list(st) == [7] * 4 and not any(turns)
        msg = L.sd_last_error(diarizer._h).decode()
        if names is not None:
            assert "recording %d" % names in msg, msg
        return msg

    def with_(i, **kw):
        d = [g.desc() for g in good]
        for k, v in kw.items():
            setattr(d[i], k, v)
        return d

    refused(with_(1, data=None), names=1)
    refused(with_(0, n=-1), names=0)
    refused(with_(1, encoding=4), names=1)
    refused(with_(1, channels=0), names=1)
    refused(with_(0, channel=1), names=0)
    refused(with_(0, channel=-2), names=0)
    refused(with_(1, sample_rate=0), names=1)
    refused(with_(1, sample_rate=1680001), names=1)                 # resample_check: the tap table
    refused(with_(1, sample_rate=1680000), names=1)                 # resample_jobs' rule: the span and the tile's outputs in LDS
    refused(with_(0, n=8000 * (357199 + 40), data=1 << 20))          # the pack limits, counted on len16 (nothing is read before the refusal)
    s16 = torch.zeros(200000, dtype=torch.int16, device="cuda:0")
    torch.cuda.synchronize()
    on_dev = [sdhip.AudioDesc(s16.data_ptr() + 1, 100000, 16000, G.ENC_S16, 1, 0)]
    refused(on_dev, fn=L.sd_diarize_many_audio_dev, names=0)         # a device pointer not aligned to its element
    diarizer.set_dump_dir(str(tmp_path))
    try:
        refused([g.desc() for g in good])
    finally:
        diarizer.set_dump_dir(None)
    sc = torch.zeros((2, 293, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    diarizer.set_planted(sc.data_ptr(), 0, 0, 2)
    try:
        refused([g.desc() for g in good])
    finally:
        diarizer.set_planted(0, 0, 0, 0)
    cen, _ = diarizer.last_speakers()
    diarizer.set_enrolled(cen[:1])
    diarizer.set_option("num_clusters", 2)
    try:
        refused([g.desc() for g in good])                            # an enrolled refusal: a gallery with a fixed number of clusters
    finally:
        diarizer.set_option("num_clusters", -1)
        diarizer.set_enrolled(None)
    assert not os.listdir(str(tmp_path)) and job_bytes(diarizer) == job
    assert key(diarizer.diarize_many_audio(good)) == before            # a following plain call: its bytes unchanged


def write_wav(path, tag, bits, channels, sr, data):
    data = np.ascontiguousarray(data).tobytes()
    fmt = struct.pack("<HHIIHH", tag, channels, sr, sr * channels * bits // 8, channels * bits // 8, bits)
    open(str(path), "wb").write(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data)


def test_cli_many_reads_g711_and_off_rate_files_as_the_single_file_run_reads_their_decoded_samples(weights, tmp_path):
    """a --many list of a mu-law 8 kHz wav, an A-law stereo wav under --downmix and a 44.1 kHz PCM wav under --resample: each block equals the single-file
    run, with --resample, of a 16-bit PCM wav that holds the host-decoded samples at the same rate; without --downmix the G.711 stereo file is refused on
    its own line and the others are still diarized"""
    recs = recordings()
    exe = os.path.join(PKG, "speakerDiarizer")
    rule = "-" * 52
    mu, al, pcm44 = recs[0], recs[1], recs[2]
    mono44 = pcm44[1][0::2]
    files = {"mu.wav": (7, 8, 1, 8000, mu[1]), "al.wav": (6, 8, 2, 8000, al[1]), "p44.wav": (1, 16, 1, 44100, mono44)}
    for name, spec in files.items():
        write_wav(tmp_path / name, *spec)
    # the decoded twins: mu-law -> int16 mono; A-law stereo -> the mean of the two decoded channels, which --downmix of a 16-bit stereo file computes
    write_wav(tmp_path / "mu_pcm.wav", 1, 16, 1, 8000, G.mulaw_table()[mu[1]].astype(np.int16))
    write_wav(tmp_path / "al_pcm.wav", 1, 16, 2, 8000, G.alaw_table()[al[1]].astype(np.int16))

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

    p = {k: str(tmp_path / k) for k in ("mu.wav", "al.wav", "p44.wav", "mu_pcm.wav", "al_pcm.wav")}
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join([p["mu.wav"], p["al.wav"], p["p44.wav"]]) + "\n")
    want = {p["mu.wav"]: single([p["mu_pcm.wav"], "--resample"]), p["al.wav"]: single([p["al_pcm.wav"], "--resample", "--downmix"]),
            p["p44.wav"]: single([p["p44.wav"], "--resample"])}
    assert all(len(v) >= 1 for v in want.values())
    out, blocks = many(["--resample", "--downmix"])
    assert out.returncode == 0, out.stderr
    assert blocks == want
    out, blocks = many(["--resample"])
    assert out.returncode == 1
    head = [b for b in blocks if b.startswith(p["al.wav"] + ": ")]
    assert len(head) == 1 and "--downmix" in head[0] and blocks[head[0]] == []
    assert list(blocks) == [p["mu.wav"], head[0], p["p44.wav"]] and blocks[p["mu.wav"]] == want[p["mu.wav"]] and blocks[p["p44.wav"]] == want[p["p44.wav"]]
