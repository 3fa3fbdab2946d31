"""GPU tests of the incremental path (sd_stream_*): after any sequence of pushes the stream's answer is bit-identical to the whole path on the
concatenation of what was pushed -- turns, order, labels, confidences, and the cached scores and embeddings behind them -- and no complete chunk
goes through a network twice.  The recording is the 75 s one of tests/stream_cases.py."""
import os
import subprocess

import numpy as np
import pytest

import sdhip
import synth
import stream_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd")
SD_ERR_ARG, SD_ERR_SHORT = 1, 4


def push_to(stream, pcm, ends, start=0):
    for e in ends:
        stream.push(pcm[start:e])
        start = e
    return start


def same_conf(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a, b, equal_nan=True)


def test_every_prefix_equals_the_whole_path_with_the_real_networks(diarizer):
    pcm = sc.pcm75()
    with diarizer.stream() as s:
        assert s.info() == (0, 0, 0)
        pos = 0
        for n in sc.PUSH_ENDS:
            s.push(pcm[pos:n])
            pos = n
            assert s.info() == (n, sc.sealed(n), sc.total(n)), n
            if n == 1:
                with pytest.raises(sdhip.SdError) as e1:
                    s.turns()
                with pytest.raises(sdhip.SdError) as e2:
                    diarizer.diarize(pcm[:n])
                assert e1.value.code == e2.value.code == SD_ERR_SHORT
                continue
            got = s.turns()
            conf = diarizer.last_confidence()
            want = diarizer.diarize(pcm[:n])
            print("n = %d: %d turns, sealed %d / %d" % (n, len(got), sc.sealed(n), sc.total(n)))
            assert got == want, n
            assert same_conf(conf, diarizer.last_confidence()), n
            assert s.info() == (n, sc.sealed(n), sc.total(n)), n
        assert len(got) >= 1 and sc.sealed(sc.N) == 128


def test_cached_rows_are_the_bits_of_segment_and_embed(diarizer):
    pcm = sc.pcm75()
    wav = pcm.astype(np.float32) / np.float32(32768.0)
    first = None
    with diarizer.stream() as s:
        pos = 0
        for n in (328001, 584001, 1200000):
            s.push(pcm[pos:n])
            pos = n
            with pytest.raises(sdhip.SdError) as e:      # pending rows are stale until turns() has run
                s.read(0, sc.total(n))
            assert e.value.code == SD_ERR_ARG
            s.turns()
            seg, emb = s.read(0, sc.total(n))
            ref_seg = diarizer.segment(wav[:n])
            assert same_bits(seg, ref_seg), n
            _, masks, _ = diarizer.postseg(ref_seg)
            ref_emb = diarizer.embed(wav[:n], masks)
            assert same_bits(emb, ref_emb), n
            assert np.isfinite(emb[:, 0]).sum() >= 3
            if first is None:
                first = s.read(0, 32)
        again = s.read(0, 32)
        assert same_bits(first[0], again[0]) and same_bits(first[1], again[1])
        only_seg, none = s.read(3, 5, emb=False)
        assert none is None and same_bits(only_seg, seg[3:5])
        for lo, hi in ((-1, 4), (5, 4), (0, 142)):
            with pytest.raises(sdhip.SdError) as e:
                s.read(lo, hi)
            assert e.value.code == SD_ERR_ARG


@pytest.mark.parametrize("plant_emb", [False, True])
def test_planted_prefixes_equal_the_whole_path_and_the_oracle(diarizer, plant_emb):
    import torch
    pcm = sc.pcm75()
    scores, emb = sc.planted75()
    dev = torch.device("cuda", 0)
    d_pcm = torch.from_numpy(np.array(pcm)).to(dev)
    d_sc, d_em = torch.from_numpy(np.array(scores)).to(dev), torch.from_numpy(np.array(emb)).to(dev)
    torch.cuda.synchronize()
    diarizer.set_planted(d_sc.data_ptr(), d_em.data_ptr() if plant_emb else 0, 0, sc.CHUNKS)
    try:
        with diarizer.stream() as s:
            pos = 0
            for n in sc.PLANTED_PREFIXES:
                s.push(pcm[pos:n])
                pos = n
                got = s.turns()
                assert got == diarizer.diarize_dev(d_pcm.data_ptr(), n), n
                assert len(got) >= 1
                if plant_emb:
                    ref, K = sc.planted_oracle(n)
                    assert got == list(ref) and K >= 2 and len(got) >= 4, n
                seg, _ = s.read(0, sc.total(n), emb=False)
                assert np.array_equal(seg, scores[:sc.total(n)])
    finally:
        diarizer.set_planted(0, 0, 0, 0)


def test_each_chunk_goes_through_the_networks_once(diarizer):
    pcm = sc.pcm75()
    more = synth.make_pcm(80.0, sc.SEED)[sc.N:sc.N + 8000]
    items = lambda: diarizer.kernel_stats("items_live")["bytes"]
    with diarizer.stream() as s:
        diarizer.reset_stats()
        for i in range(0, sc.N, 8000):
            s.push(pcm[i:i + 8000])
        assert items() == 3 * 128                       # the four sealed blocks, nothing else
        t1 = s.turns()
        assert items() == 3 * sc.CHUNKS
        assert s.turns() == t1
        assert items() == 3 * sc.CHUNKS                 # nothing pushed: no inference
        s.push(more)
        n = sc.N + 8000
        assert s.info() == (n, sc.sealed(n), sc.total(n)) == (n, 128, 142)
        assert items() == 3 * sc.CHUNKS                 # no block sealed
        s.turns()
        assert items() == 3 * sc.CHUNKS + 3 * (sc.total(n) - sc.sealed(n))
    diarizer.reset_stats()


def test_pieces_and_sample_formats_do_not_change_a_bit(diarizer):
    import torch
    pcm = sc.pcm75()
    wav = pcm.astype(np.float32) / np.float32(32768.0)
    d_pcm = torch.from_numpy(np.array(pcm)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()

    def run(feed):
        with diarizer.stream() as s:
            feed(s)
            assert s.info() == (sc.N, 128, 141)
            t = s.turns()
            return t, diarizer.last_confidence(), s.read(0, sc.CHUNKS)

    def pieces(size, how):
        def feed(s):
            for k, i in enumerate(range(0, sc.N, size)):
                j = min(i + size, sc.N)
                kind = how if how != "mixed" else ("pcm", "f32", "dev")[k % 3]
                if kind == "pcm":
                    s.push(pcm[i:j])
                elif kind == "f32":
                    s.push_f32(wav[i:j])
                else:
                    s.push_dev(d_pcm.data_ptr() + 2 * i, j - i)
        return feed

    base = run(pieces(sc.N, "pcm"))
    assert base[0] == diarizer.diarize(pcm) and len(base[0]) >= 1
    for size, how in ((8000, "pcm"), (7919, "pcm"), (100003, "f32"), (100003, "dev"), (50021, "mixed")):
        t, conf, (seg, emb) = run(pieces(size, how))
        assert t == base[0] and same_conf(conf, base[1]), (size, how)
        assert same_bits(seg, base[2][0]) and same_bits(emb, base[2][1]), (size, how)


def test_two_streams_and_other_entry_points_interleave(diarizer):
    a = sc.pcm75()
    b = synth.make_pcm(45.0, 5)
    other = synth.make_pcm(20.0, 11)
    whole_other = diarizer.diarize(other)
    speech_other = diarizer.activity(other, "speech")
    with diarizer.stream() as sa, diarizer.stream() as sb:
        pa = pb = 0
        for step in range(4):
            ea, eb = min(len(a), pa + 300001), min(len(b), pb + 180001)
            sa.push(a[pa:ea])
            assert diarizer.diarize(other) == whole_other
            sb.push(b[pb:eb])
            assert diarizer.activity(other, "speech") == speech_other
            pa, pb = ea, eb
            ta = sa.turns()
            tb = sb.turns()
            assert ta == sa.turns()                     # sb's call in between did not disturb sa's pending rows
            assert ta == diarizer.diarize(a[:pa]), step
            assert tb == diarizer.diarize(b[:pb]), step
        assert (pa, pb) == (len(a), len(b)) and sa.info()[1] == 128 and sb.info()[1] == sc.sealed(len(b)) == 64


def test_options_apply_at_turns_and_precision_is_fixed_at_open(diarizer, tmp_path):
    pcm = sc.pcm75()
    try:
        with diarizer.stream() as s:
            s.push(pcm[:700000])
            t_auto = s.turns()
            diarizer.set_option("num_clusters", 2)
            t_two = s.turns()
            assert t_two == diarizer.diarize(pcm[:700000])
            diarizer.set_option("num_clusters", -1)
            assert s.turns() == t_auto == diarizer.diarize(pcm[:700000])
            # another precision: the cache would be mixed
            diarizer.set_option("ecapa_precision", 3)
            for call in (lambda: s.push(pcm[700000:700001]), s.turns):
                with pytest.raises(sdhip.SdError) as e:
                    call()
                assert e.value.code == SD_ERR_ARG
            assert s.info() == (700000, sc.sealed(700000), sc.total(700000))
            diarizer.set_option("ecapa_precision", 0)
            s.push(pcm[700000:])
            assert s.turns() == diarizer.diarize(pcm)
            # the step files describe one whole-path inference
            diarizer.set_dump_dir(str(tmp_path), 1)
            with pytest.raises(sdhip.SdError) as e:
                s.turns()
            assert e.value.code == SD_ERR_ARG
            diarizer.set_dump_dir(None)
            assert s.turns() == diarizer.diarize(pcm)
            assert not os.listdir(str(tmp_path))
        diarizer.set_option("ecapa_precision", 3)
        with diarizer.stream() as s3:
            push_to(s3, pcm, (328001, 900000, sc.N))
            assert s3.turns() == diarizer.diarize(pcm)
            diarizer.set_option("ecapa_precision", 0)
            with pytest.raises(sdhip.SdError) as e:
                s3.turns()
            assert e.value.code == SD_ERR_ARG
    finally:
        diarizer.set_option("ecapa_precision", 0)
        diarizer.set_option("num_clusters", -1)
        diarizer.set_dump_dir(None)


def test_a_stream_left_open_is_freed_with_its_context(weights):
    d = sdhip.Diarizer(weights[0], weights[1])
    s = d.stream()
    s.push(sc.pcm75()[:400000])
    assert s.info() == (400000, 32, sc.total(400000))
    d.close()                                           # sd_destroy closes the stream
    with pytest.raises(sdhip.SdError):
        s.info()
    s.close()


def test_command_line_streams_a_file_and_stdin(weights, golden_dir):
    path = os.path.join(golden_dir, "multi-speaker_1min.wav")
    exe = os.path.join(PKG, "speakerDiarizer")
    rule = "-" * 52

    def turn_lines(stdout):
        lines = stdout.splitlines()
        i0 = lines.index(rule)
        return lines[i0 + 1:lines.index(rule, i0 + 1)]

    base = [exe, weights[0], weights[1]]
    plain = subprocess.run(base + [path], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr
    want = turn_lines(plain.stdout)
    assert len(want) >= 1
    out = subprocess.run(base + [path, "--stream", "10"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert turn_lines(out.stdout) == want
    assert [l for l in out.stdout.splitlines() if not l.endswith("ms")] == [l for l in plain.stdout.splitlines() if not l.endswith("ms")]
    pcm, sr, ch = sdhip.read_wav(path)
    piped = subprocess.run(base + ["-", "--stream", "10"], input=pcm.tobytes(), capture_output=True, timeout=600)
    assert piped.returncode == 0, piped.stderr
    assert turn_lines(piped.stdout.decode()) == want
    # a piece longer than the reader's 1 Mi-sample buffer, the input ending exactly on a buffer boundary inside it: the partial piece gets its block
    long_in = np.resize(pcm, 1 << 20)
    one = subprocess.run(base + ["-", "--stream", "70", "--stream-updates"], input=long_in.tobytes(), capture_output=True, timeout=600)
    assert one.returncode == 0, one.stderr
    assert [l for l in one.stdout.decode().splitlines() if l.startswith("== ")] == ["== 65.536 s, 96/123 chunks"]
    upd = subprocess.run(base + [path, "--stream", "10", "--stream-updates"], capture_output=True, text=True, timeout=600)
    assert upd.returncode == 0, upd.stderr
    lines = upd.stdout.splitlines()
    heads = [i for i, l in enumerate(lines) if l.startswith("== ")]
    pieces = -(-len(pcm) // 160000)
    assert len(heads) == pieces == 6
    assert lines[heads[0]] == "== 10 s, 0/11 chunks" and lines[heads[-1]] == "== 59 s, 96/109 chunks"
    first_rule = lines.index("-----------")
    assert lines[heads[-1] + 1:first_rule] == want and turn_lines(upd.stdout) == want


def test_command_line_reads_off_rate_and_stereo_files_as_the_plain_run_does(weights, tmp_path):
    """--resample, --downmix, --assume-16k and the default interleaved read under --stream: the turn lines of the run without the flag, and the same
    refusal of a 44.1 kHz file"""
    import struct
    exe = os.path.join(PKG, "speakerDiarizer")
    rule = "-" * 52

    def wav(path, samples, sr, channels=1):
        data = np.asarray(samples, np.int16).tobytes()
        fmt = struct.pack("<HHIIHH", 1, channels, sr, sr * channels * 2, channels * 2, 16)
        path.write_bytes(b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVE" + b"fmt " + struct.pack("<I", 16) + fmt + b"data" + struct.pack("<I", len(data)) + data)

    def turn_lines(args):
        out = subprocess.run([exe, weights[0], weights[1]] + args, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr
        lines = out.stdout.splitlines()
        i0 = lines.index(rule)
        return lines[i0 + 1:lines.index(rule, i0 + 1)]

    pcm = synth.make_pcm(21.0, seed=3)
    t44 = np.arange(int(len(pcm) * 44100 / 16000)) * (16000.0 / 44100.0)
    pcm44 = np.rint(np.interp(t44, np.arange(len(pcm)), pcm.astype(np.float64))).astype(np.int16)
    left = pcm.astype(np.int32)
    right = np.roll(left, 4000) // 2
    wav(tmp_path / "m44.wav", pcm44, 44100)
    wav(tmp_path / "st.wav", np.stack([left, right], 1).reshape(-1), 16000, channels=2)
    for name, flags in (("m44.wav", ["--resample"]), ("m44.wav", ["--assume-16k"]), ("st.wav", []), ("st.wav", ["--downmix"])):
        want = turn_lines([str(tmp_path / name)] + flags)
        assert len(want) >= 1
        assert turn_lines([str(tmp_path / name)] + flags + ["--stream", "3.7"]) == want, (name, flags)
    out = subprocess.run([exe, weights[0], weights[1], str(tmp_path / "m44.wav"), "--stream", "5"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 1 and "44100" in out.stderr and "--resample" in out.stderr
