"""k_many_ingest (csrc/ingest.hip) alone, through sd_test_many_ingest (include/sdhip_ingest_test.h): ONE launch through launch_many_ingest on the rows of
tests/ingest_cases.py, the whole returned buffer -- every slot, the floats between them, 256 floats behind the destination -- compared byte for byte
with tests/ingest_ref.py.

  16 kHz rows     pure decode and copy: all four encodings, all 256 codes of each law in one row, 1 .. 3 channels with every channel and the mean,
                  1 .. 773 frames, bases at every alignment mod 4
  off-rate rows   8 000, 11 025, 32 000, 44 100 and 48 000 Hz against input_ref.resample_exact on the tap table read back from the device through the
                  existing sd_test_resample; 1 .. 773 outputs with 255 / 256 / 257, inputs shorter than one wing, one frame.  The smallest G.711
                  magnitudes (8 * 2^-15) stay in: input_ref's no-subnormal guard accepts every product of them with the taps.
  mixed9          nine rows of mixed encodings and rates and the pad row in one launch
  the tie         an off-rate row of each encoding equals the same samples decoded on the host and run through the existing k_resample_jobs
                  (sd_test_resample_jobs): the new staging against the existing kernel, no reference in between

The sources carry the hook's guards behind them -- NaN, 0x7fff, the law's largest magnitude -- so a read past the last element the rule reads shows."""
import numpy as np
import pytest

import ingest_cases as IC
import ingest_ref as G
import sdhip
from test_input_kernels import same, table

pytestmark = pytest.mark.gpu

FC = IC.FCANARY


def tables(d, name):
    return {sr: table(d, sr) for sr in IC.rates_of(name)}


@pytest.mark.parametrize("name", IC.DIRECT)
def test_rows_at_16_khz_are_decode_and_copy(diarizer, name):
    rows, src, dst_len = IC.case(name)
    out = diarizer.many_ingest_case(rows, src, dst_len, canary=FC)
    same("k_many_ingest %s" % name, out, IC.expected(name, {}))


@pytest.mark.parametrize("name", IC.RATE_CASES)
def test_off_rate_rows_are_resample_exact_on_the_devices_table(diarizer, name):
    rows, src, dst_len = IC.case(name)
    out = diarizer.many_ingest_case(rows, src, dst_len, canary=FC)
    same("k_many_ingest %s" % name, out, IC.expected(name, tables(diarizer, name)))


def test_nine_mixed_rows_and_the_pad_row_in_one_launch(diarizer):
    rows, src, dst_len = IC.case("mixed9")
    out = diarizer.many_ingest_case(rows, src, dst_len, canary=FC)
    same("k_many_ingest mixed9", out, IC.expected("mixed9", tables(diarizer, "mixed9")))


@pytest.mark.parametrize("sr", [8000, 44100])
def test_off_rate_rows_equal_k_resample_jobs_on_the_decoded_samples(diarizer, sr):
    rows, src, dst_len, jobs, x, arena, pairs = IC.tie_case(sr)
    out = diarizer.many_ingest_case(rows, src, dst_len, canary=FC)
    ref = diarizer.resample_jobs_case(jobs, x, arena, canary=FC)
    assert not np.isnan(out).any()
    for base, dst_off, count in pairs:
        assert count >= 600 and out[base:base + count].tobytes() == ref[dst_off:dst_off + count].tobytes()


def test_hook_refusals_come_before_any_launch(diarizer):
    rows, src, dst_len = IC.case("mixed9")
    def bad(r, col, v, **kw):
        t = np.array(rows)
        t[r, col] = v
        out = diarizer.many_ingest_case(t, kw.get("src", src), kw.get("dst_len", dst_len), canary=FC, refused=True)
        assert (out == 0).all()                                                 # nothing came back: nothing was launched
    bad(0, 0, 4)                                # an unknown encoding
    bad(0, 1, 0)                                # channels < 1
    bad(1, 2, 2)                                # channel outside [-1, channels)
    bad(0, 3, 0)                                # a rate of 0
    bad(0, 4, -1)                               # n < 0
    bad(0, 5, len(src))                         # a source that leaves src
    bad(4, 5, int(rows[4][5]) + 1)              # an int16 source at an odd byte
    bad(0, 6, int(rows[1][6]))                  # two rows share a destination
    bad(0, 7, 10)                               # len16 > len
    bad(8, 7, int(rows[8][7]) + dst_len)        # a slot that leaves the destination
    bad(0, 3, 1680001)                          # a rate pair resample_check refuses (its tap table)
    bad(0, 3, 1680000)                          # the largest span k_resample accepts: with the tile's outputs next to it, it does not fit the LDS
