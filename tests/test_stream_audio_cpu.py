"""CPU tests of the host side of streams in their own encoding (sd_stream_set_input_format, sd_stream_push_audio*, sd_stream_push_many_audio*; DESIGN
7.13): the planner (csrc/stream_ingest_plan.h) as a stand-alone program under AddressSanitizer + UBSan (tools/sanitize/stream_ingest_main.cpp, built by
tools/sanitize/build_stream_ingest.sh) -- the sharing classes, the bytes that go up, the placement of the uploads, every refusal with the stream it names,
rows of no frames, and 300 random tables against a naive second implementation inside the program -- the hook's header and the mirrored interface, and the
usage errors of the command line.  Nothing is loaded into python under a sanitizer."""
import os
import re
import subprocess

import pytest

import sdhip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "pyannote-audio_speaker-diarization_cpp_amd", "speakerDiarizer")

_lines = []


def program_lines(tmp_path_factory):
    """the program is built and run once"""
    if not _lines:
        exe = str(tmp_path_factory.mktemp("si") / "stream_ingest_asan")
        b = subprocess.run(["bash", os.path.join(ROOT, "tools", "sanitize", "build_stream_ingest.sh"), exe], capture_output=True, text=True, timeout=600)
        assert b.returncode == 0, b.stderr[-3000:]             # the compiler is the one the library is built with: a failure here is a failure
        out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and out.stdout.endswith("stream ingest ok\n"), (out.stdout[-600:], out.stderr[-3000:])
        assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr and "BAD" not in out.stdout, out.stderr[-3000:]
        _lines.extend(out.stdout.splitlines())
    return _lines


def cases(lines):
    """name -> (rows=.. uploads=.. total=.., [row fields], [upload fields])"""
    out = {}
    for l in lines:
        if l.startswith("case "):
            name, rest = l[5:].split(" -> ", 1)
            parts = rest.split(" | ")
            out[name] = (parts[0], [p for p in parts[1:] if p.startswith("cls=")], [p for p in parts[1:] if p.startswith("off=")])
    return out


def test_legs_of_one_call_share_one_upload_and_other_sources_do_not(tmp_path_factory):
    c = cases(program_lines(tmp_path_factory))
    for name in ("two legs", "two legs, the later one first"):
        head, rows, ups = c[name]
        assert head == "rows=2 uploads=1 total=2000" and ups == ["off=0 bytes=2000"], name       # 1 000 stereo frames of one byte, counted once
        assert [r.split()[0] for r in rows] == ["cls=0", "cls=0"], name
    # the same pointer with other frames, channels or encoding, and another pointer: separate uploads
    assert c["same pointer, other frames"][0].startswith("rows=2 uploads=2") and c["same pointer, other frames"][2] == ["off=0 bytes=1999", "off=2000 bytes=1998"]
    assert c["same pointer, other channels"][2] == ["off=0 bytes=1999", "off=2000 bytes=1000"]
    assert c["same pointer, other encoding"][2] == ["off=0 bytes=1999", "off=2000 bytes=1999"]
    assert c["other pointer"][2] == ["off=0 bytes=1999", "off=2000 bytes=2000"]
    # the device form uploads nothing and its rows read the callers' pointers
    assert c["device form"][0] == "rows=2 uploads=0 total=0" and [r.split()[0] for r in c["device form"][1]] == ["cls=-1", "cls=-1"]


def test_only_the_bytes_the_rule_reads_go_up(tmp_path_factory):
    c = cases(program_lines(tmp_path_factory))
    # ingest_src_bytes: 10 frames of 3 int16 are 60 bytes; channel 0 stops two elements early, legs 0 and 1 take the larger count, the mean takes all
    assert c["channel 0 of 3, int16"][2] == ["off=0 bytes=56"]
    assert c["channels 0 and 1 of 3, int16"][0].startswith("rows=2 uploads=1 total=58") and c["channels 0 and 1 of 3, int16"][2] == ["off=0 bytes=58"]
    assert c["mean of 3, float"][2] == ["off=0 bytes=120"]


def test_uploads_are_placed_congruent_to_the_head_of_their_destination(tmp_path_factory):
    c = cases(program_lines(tmp_path_factory))
    # destinations 0, 1, 2, 3 floats behind a 16-byte boundary have heads 0, 3, 2, 1; one byte per frame: offset + head is a multiple of 16
    ups = [tuple(int(v.split("=")[1]) for v in u.split()) for u in c["heads 0 3 2 1, mono mu-law"][2]]
    assert ups == [(0, 5), (13, 5), (30, 5), (47, 5)] and [(o + h) % 16 for (o, _), h in zip(ups, (0, 3, 2, 1))] == [0, 0, 0, 0]
    # four bytes per frame, heads 3 and 1
    ups = [tuple(int(v.split("=")[1]) for v in u.split()) for u in c["heads 3 1, stereo int16"][2]]
    assert ups == [(4, 20), (28, 28)] and [(o + 4 * h) % 16 for (o, _), h in zip(ups, (3, 1))] == [0, 0]


def test_rows_of_no_frames_make_no_row_and_no_upload(tmp_path_factory):
    c = cases(program_lines(tmp_path_factory))
    assert c["frames 0"] == ("rows=1 uploads=1 total=8", ["cls=0 len=8 room=8 ch=0"], ["off=0 bytes=8"])
    assert c["nothing at all"] == ("rows=0 uploads=0 total=0", [], [])


def test_every_refusal_names_its_stream(tmp_path_factory):
    lines = program_lines(tmp_path_factory)
    got = dict(l[8:].rsplit(" -> ", 1) for l in lines if l.startswith("refusal "))
    ok, no_format, frames, null_data, too_big, align = "0 bad=-1", "1 bad=%d", "2 bad=%d", "3 bad=%d", "4 bad=%d", "5 bad=%d"
    assert got == {"fine": ok, "frames < 0": frames % 1, "frames = 2^40": ok, "frames = 2^40 + 1": frames % 2, "no format": no_format % 1,
                   "null data": null_data % 0, "bytes = 2^42": ok, "bytes = 2^42 + 4": too_big % 1, "bytes of channel 0 of 4 = 2^42 - 6": ok,
                   "2^40 frames of 2^31 - 1 float channels": too_big % 0, "odd int16 pointer, host form": ok,
                   "odd int16 pointer, device form": align % 1, "float pointer + 2, device form": align % 0, "odd G.711 pointer, device form": ok}


def test_random_tables_agree_with_the_naive_implementation(tmp_path_factory):
    rounds = [l for l in program_lines(tmp_path_factory) if l.startswith("round ")]
    assert len(rounds) == 300 and not any("BAD" in l for l in rounds)
    shared = 0
    for l in rounds:
        rows, ups = (int(v) for v in re.search(r"(\d+) rows, (\d+) uploads", l).groups())
        assert ups <= rows
        shared += ups < rows
    assert shared >= 50                                      # rows that share an upload are common among them


def test_the_hook_has_a_header_of_its_own_and_the_interface_is_mirrored():
    L = sdhip.lib()
    hook = set(re.findall(r"^int (sd_[a-z0-9_]+)\(", open(os.path.join(ROOT, "include", "sdhip_stream_ingest_test.h")).read(), re.M))
    assert hook == set(sdhip.STREAM_INGEST_TEST_EXPORTS) == {"sd_test_group_ingest"} and hasattr(L, "sd_test_group_ingest")
    assert "sd_test_group_ingest" not in open(os.path.join(ROOT, "include", "sdhip_test.h")).read()
    for name in ("sd_stream_set_input_format", "sd_stream_input_format", "sd_stream_push_audio", "sd_stream_push_audio_dev", "sd_stream_push_many_audio",
                 "sd_stream_push_many_audio_dev"):
        assert name in sdhip.EXPORTS and hasattr(L, name)
    for name in ("set_input_format", "input_format", "push_audio", "push_audio_dev"):
        assert callable(getattr(sdhip.Stream, name))
    for name in ("stream_push_many_audio", "stream_push_many_audio_dev", "group_ingest_case"):
        assert callable(getattr(sdhip.Diarizer, name))


@pytest.mark.parametrize("args, word", [
    (["missing.wav", "--stream-encoding", "mulaw"], "--stream-encoding"),                                     # without --stream
    (["missing.wav", "--stream", "2", "--stream-encoding", "mulaw"], "--stream-encoding"),                    # with a wav path instead of -
    (["missing.wav", "--stream", "2", "--stream-channels", "2"], "--stream-channels"),
    (["-", "--stream-channel", "1"], "--stream-channel give"),                                                # - without --stream
    (["missing.wav", "--stream", "2", "--stream-channel", "mean"], "--stream-channel"),
    (["-", "--stream", "2", "--stream-encoding", "pcm"], "--stream-encoding"), (["-", "--stream", "2", "--stream-encoding", "MULAW"], "--stream-encoding"),
    (["-", "--stream", "2", "--stream-encoding"], "--stream-encoding"),
    (["-", "--stream", "2", "--stream-channels", "0"], "--stream-channels"), (["-", "--stream", "2", "--stream-channels", "-2"], "--stream-channels"),
    (["-", "--stream", "2", "--stream-channels", "2.5"], "--stream-channels"), (["-", "--stream", "2", "--stream-channels", "two"], "--stream-channels"),
    (["-", "--stream", "2", "--stream-channels"], "--stream-channels"),
    (["-", "--stream", "2", "--stream-channel", "-1"], "--stream-channel"), (["-", "--stream", "2", "--stream-channel", "left"], "--stream-channel"),
    (["-", "--stream", "2", "--stream-channel", "1"], "--stream-channel"),                                    # channel 1 of the one default channel
    (["-", "--stream", "2", "--stream-channels", "2", "--stream-channel", "2"], "--stream-channel"),
    (["-", "--stream", "2", "--stream-channel"], "--stream-channel"),
])
def test_cli_usage_errors_of_the_stream_format_exit_2_before_anything_touches_the_gpu(args, word):
    out = subprocess.run([EXE, "seg.sdw", "emb.sdw"] + args, input=b"", capture_output=True, timeout=60)
    assert out.returncode == 2, (out.returncode, out.stderr[-500:])
    assert b"usage" in out.stderr and word.encode() in out.stderr, out.stderr[-500:]
