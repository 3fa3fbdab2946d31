"""k_group_ingest (csrc/stream_ingest.hip) alone, through sd_test_group_ingest (include/sdhip_stream_ingest_test.h): ONE launch per case through
launch_group_ingest on rows chosen here, the whole returned buffer -- every row, its pad zeros, the canaries between the rows and the 256 floats behind
the destination -- compared byte for byte with tests/ingest_ref.py's frames() placed by the few lines of numpy in expected().

A row is (encoding, channels, channel, n, src_off in bytes, dst_off, room): dst[dst_off, dst_off + n) = the frames, 512 zeros behind, nothing at or
behind dst[dst_off + room].  The hook lays every distinct source out at src_off mod 16 bytes behind a 16-byte boundary with the guards behind the last
element the rule reads -- NaN, 0x7fff, the law's largest magnitude -- so the test chooses which rows can take the kernel's wide loads (one and two
channels whose frame `head` is aligned), and a read past the last element shows.  Shapes are the smallest at which the kernel can go wrong: lengths
around one group of four, 255 / 256 / 257 (a block of 64 groups of 4 per wave) and 1 023 / 1 024 / 1 025 (256 groups: one block), every alignment of
the destination mod 4 and of the source mod 16, rooms that cut the frames, the zeros and nothing; one row of 2 100 000 frames reaches the x stride
(2 048 blocks of 256 groups of 4 = 2 097 152 floats) and 1 025 rows the y stride (1 024)."""
import numpy as np
import pytest

import ingest_ref as G
import sdhip

pytestmark = pytest.mark.gpu

FC = np.float32(-7776.0)
PAD = 512                                                  # SD_TAIL_PAD
SLACK = G.SLACK
ENCS = (G.ENC_S16, G.ENC_F32, G.ENC_MULAW, G.ENC_ALAW)
ES = {G.ENC_S16: 2, G.ENC_F32: 4, G.ENC_MULAW: 1, G.ENC_ALAW: 1}
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 1023, 1024, 1025)
MISTAKES = ("channel_stride", "pad_zeros_missing", "one_element_past_the_last", "room_ignored")


def elements(enc, count, seed):
    g = np.random.default_rng(seed)
    if enc == G.ENC_F32:
        return (g.standard_normal(count) * 0.25).astype(np.float32)
    if enc == G.ENC_S16:
        return g.integers(-32768, 32768, count).astype(np.int16)
    return g.integers(0, 256, count).astype(np.uint8)


def guard_value(enc):
    """what the hook's guard element decodes to"""
    if enc == G.ENC_F32:
        return np.float32(np.nan)
    if enc == G.ENC_S16:
        return np.float32(32767.0 / 32768.0)
    return G.decode(np.array([G.GUARD_CODE[enc]], np.uint8), enc)[0]


class Table:
    """rows with their sources: add() places a source at the next byte offset that is `src_mod` mod 16, share() names an earlier one again"""

    def __init__(self):
        self.rows, self.parts, self.at, self.dst = [], [], 0, 5

    def add(self, enc, channels, channel, n, dst_mod, room_extra, src_mod=0, el=None, seed=0):
        el = elements(enc, n * channels, seed) if el is None else np.ascontiguousarray(el, G.DTYPES[enc])
        assert len(el) == n * channels and src_mod % ES[enc] == 0
        gap = (src_mod - self.at) % 16
        self.parts.append(np.zeros(gap, np.uint8))
        self.at += gap
        so = self.at
        self.parts.append(el.view(np.uint8))
        self.at += el.nbytes
        return self.place(enc, channels, channel, n, so, dst_mod, room_extra)

    def place(self, enc, channels, channel, n, so, dst_mod, room_extra):
        """room_extra: room = n + room_extra (negative: the room cuts the frames)"""
        self.dst += 3 + (dst_mod - (self.dst + 3)) % 4
        room = max(n + room_extra, 0)
        self.rows.append((enc, channels, channel, n, so, self.dst, room))
        self.dst += max(room, 1) + 2
        return len(self.rows) - 1

    def share(self, r, channel, dst_mod, room_extra):
        enc, channels, _, n, so, _, _ = self.rows[r]
        return self.place(enc, channels, channel, n, so, dst_mod, room_extra)

    def done(self):
        src = np.concatenate(self.parts) if self.parts else np.zeros(0, np.uint8)
        return np.array(self.rows, np.int64).reshape(-1, 7), src, self.dst + 9


def expected(rows, src, dst_len, mistake=None):
    """the numpy restatement: frames() of every row placed in a buffer of canaries.  `mistake` plants one of MISTAKES"""
    out = np.full(dst_len + SLACK, FC, np.float32)
    for enc, channels, channel, n, so, dof, room in np.asarray(rows, np.int64).reshape(-1, 7).tolist():
        el = src[so:so + n * channels * ES[enc]].view(G.DTYPES[enc])
        y = G.frames(el, enc, channels, channel, n, "channel_stride" if mistake == "channel_stride" else None)
        if mistake == "one_element_past_the_last" and n > 0:
            # a load that runs one element over: the last frame takes the element behind the one the rule names -- behind the last channel that is the
            # hook's guard (only the rows that read the last element of their source can show it: a mono row, the last channel, the mean)
            last = np.concatenate([G.decode(el, enc), [guard_value(enc)]]).astype(np.float32)
            if channel >= 0:
                y = y.copy()
                y[-1] = last[(n - 1) * channels + channel + 1]
            else:
                s = np.float32(0.0)
                for q in range(channels):
                    s = np.float32(s + last[(n - 1) * channels + q + 1])
                y = y.copy()
                y[-1] = np.float32(s / np.float32(channels))
        end = n + PAD if mistake == "room_ignored" else min(n + PAD, room)
        k = min(n, end)
        out[dof:dof + k] = y[:k]
        if mistake != "pad_zeros_missing":
            out[dof + k:dof + end] = 0.0
    return out


def same(name, got, want):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, name
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError("%s: %d of %d floats differ, the first at %d: got %r, want %r" % (name, len(bad), len(got), bad[0], got[bad[0]], want[bad[0]]))


def run(d, name, rows, src, dst_len):
    out = d.group_ingest_case(rows, src, dst_len, canary=float(FC))
    same("k_group_ingest %s" % name, out, expected(rows, src, dst_len))
    return out


ROOMS = (0, 1, PAD - 1, PAD, PAD + 37)                     # room = len + these


def forms_table(enc):
    """every channel form x every length x every destination offset mod 4, the source offsets and the rooms cycling; then, for one and two channels,
    every source offset mod 16 x every destination offset"""
    t, k, es = Table(), 0, ES[enc]
    for channels in (1, 2, 3, 5):
        for channel in sorted({-1, 0, channels - 1}):
            for n in LENGTHS:
                for dst_mod in range(4):
                    t.add(enc, channels, channel, n, dst_mod, ROOMS[k % 5], src_mod=((k + k // 4) * es) % 16, seed=1000 * enc + k)      # (k // 4: every pair with dst_mod)
                    k += 1
    for channels, channel in ((1, 0), (2, 0), (2, 1), (2, -1)):
        for src_mod in range(0, 16, es):
            for dst_mod in range(4):
                for n in (5, 8, 257):
                    t.add(enc, channels, channel, n, dst_mod, PAD, src_mod=src_mod, seed=1000 * enc + k)
                    k += 1
    return t.done()


@pytest.mark.parametrize("enc", ENCS)
def test_every_form_length_offset_and_room(diarizer, enc):
    rows, src, dst_len = forms_table(enc)
    assert {int(r[4]) % 16 for r in rows} == set(range(0, 16, ES[enc])) and {int(r[5]) % 4 for r in rows} == {0, 1, 2, 3}
    assert {int(r[6] - r[3]) for r in rows} == set(ROOMS) and {int(r[3]) for r in rows} == set(LENGTHS)
    for channels in (1, 2, 3, 5):                                          # every source offset with every destination offset, for every channel count
        assert {(int(r[4]) % 16, int(r[5]) % 4) for r in rows if r[1] == channels} == {(a, b) for a in range(0, 16, ES[enc]) for b in range(4)}, channels
    run(diarizer, "forms of encoding %d" % enc, rows, src, dst_len)


def test_rooms_that_cut_the_frames(diarizer):
    """room < len: the frames stop at the room and nothing behind it is read or written"""
    t = Table()
    for k, (enc, channels, channel) in enumerate(((G.ENC_MULAW, 1, 0), (G.ENC_S16, 2, 1), (G.ENC_F32, 3, -1), (G.ENC_ALAW, 2, -1))):
        for cut in (1, 4, 5, 300):
            t.add(enc, channels, channel, 301, k, -cut, seed=50 + k)
    rows, src, dst_len = t.done()
    run(diarizer, "rooms below len", rows, src, dst_len)


def test_all_256_codes_of_both_laws_in_one_row_each(diarizer):
    t = Table()
    for enc in (G.ENC_MULAW, G.ENC_ALAW):
        t.add(enc, 1, 0, 256, 0, PAD, el=np.arange(256, dtype=np.uint8))
        t.add(enc, 1, 0, 256, 1, PAD, src_mod=3, el=np.arange(256, dtype=np.uint8)[::-1])
    rows, src, dst_len = t.done()
    out = run(diarizer, "all codes", rows, src, dst_len)
    for r, enc in ((0, G.ENC_MULAW), (2, G.ENC_ALAW)):
        dof = int(rows[r][5])
        tab = G.mulaw_table() if enc == G.ENC_MULAW else G.alaw_table()
        assert np.array_equal(out[dof:dof + 256], (tab / 32768.0).astype(np.float32)) and len(set(tab.tolist())) >= 255


def test_float_specials_pass_through(diarizer):
    """NaN with a payload, +-0, +-inf and denormals in rows that pick a channel leave as the bits they came; a mean keeps +-0 as the host's loop does"""
    bits = np.array([0x7FC00000, 0xFFC12345, 0x7F800001, 0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x3F800000, 0x00800000, 0x80000001], np.uint32)
    sp = bits.view(np.float32)
    t = Table()
    t.add(G.ENC_F32, 1, 0, 12, 0, PAD, el=sp)                               # the wide path (aligned) ...
    t.add(G.ENC_F32, 1, 0, 12, 0, PAD, src_mod=4, el=sp)                    # ... and the element-wise one
    two = np.stack([sp, sp[::-1]], 1).reshape(-1)
    t.add(G.ENC_F32, 2, 1, 12, 1, PAD, el=two)
    t.add(G.ENC_F32, 2, 0, 12, 2, PAD, src_mod=8, el=two)
    zeros = np.array([0.0, -0.0, -0.0, -0.0, 0.0, 0.0, 1.0, -1.0, -0.0, 0.5, -0.0, -0.0], np.float32)
    t.add(G.ENC_F32, 2, -1, 6, 0, PAD, el=zeros)
    t.add(G.ENC_F32, 3, -1, 4, 3, PAD, el=zeros)
    rows, src, dst_len = t.done()
    out = run(diarizer, "float specials", rows, src, dst_len)
    for r in (0, 1):
        dof = int(rows[r][5])
        assert np.array_equal(out[dof:dof + 12].view(np.uint32), bits)


def rounding_triple():
    """three int16 whose mean by the correctly rounded division differs from a multiplication by float32(1 / 3)"""
    g = np.random.default_rng(3)
    v = g.integers(-32768, 32768, (4000, 3)).astype(np.int16)
    x = (v.astype(np.float64) / 32768.0).astype(np.float32)
    s = ((x[:, 0] + x[:, 1]).astype(np.float32) + x[:, 2]).astype(np.float32)
    differ = np.flatnonzero((s / np.float32(3.0)).astype(np.float32) != (s * (np.float32(1.0) / np.float32(3.0))).astype(np.float32))
    assert len(differ) >= 10
    return v[differ[:64]].reshape(-1)


def test_the_mean_of_three_channels_is_the_correctly_rounded_division(diarizer):
    el = rounding_triple()
    n = len(el) // 3
    t = Table()
    t.add(G.ENC_S16, 3, -1, n, 0, PAD, el=el)
    t.add(G.ENC_S16, 3, -1, n, 3, PAD, src_mod=2, el=el)
    rows, src, dst_len = t.done()
    out = run(diarizer, "mean of three", rows, src, dst_len)
    wrong = G.frames(el, G.ENC_S16, 3, -1, n, "reciprocal_multiply")
    dof = int(rows[0][5])
    assert (out[dof:dof + n] != wrong).all()                                # every frame of this row tells the two apart


def test_1025_rows_in_one_launch(diarizer):
    t = Table()
    for k in range(1025):
        enc = ENCS[k % 4]
        t.add(enc, 1 + k % 3, (k % 3) - 1 if k % 3 else 0, 1 + k % 9, k % 4, (PAD, 0, 3)[k % 3], src_mod=(k * ES[enc]) % 16, seed=7000 + k)
    rows, src, dst_len = t.done()
    assert len(rows) == 1025
    run(diarizer, "1025 rows", rows, src, dst_len)


def test_one_row_of_2_100_000_frames(diarizer):
    """2 048 blocks x 256 threads x 4 floats = 2 097 152: the groups behind that are reached by the x stride, with 64-bit indices"""
    n = 2100000
    t = Table()
    t.add(G.ENC_MULAW, 1, 0, n, 1, PAD, src_mod=3, seed=11)
    t.add(G.ENC_ALAW, 2, 1, 9, 0, PAD, seed=12)
    rows, src, dst_len = t.done()
    assert n + PAD > 2048 * 256 * 4
    run(diarizer, "a long row", rows, src, dst_len)


def test_rows_that_share_a_source(diarizer):
    """the legs of a stereo call and three rows on one 3-channel source: the same device bytes, the guards behind the largest count among them"""
    t = Table()
    a = t.add(G.ENC_MULAW, 2, 0, 1001, 0, PAD, seed=21)
    t.share(a, 1, 3, PAD)
    b = t.add(G.ENC_S16, 3, 0, 515, 1, PAD, src_mod=2, seed=22)
    t.share(b, -1, 2, 7)
    t.share(b, 1, 0, PAD)
    c = t.add(G.ENC_ALAW, 2, 1, 64, 2, 0, src_mod=0, seed=23)             # the later leg first
    t.share(c, 0, 1, PAD)
    rows, src, dst_len = t.done()
    assert rows[0][4] == rows[1][4] and rows[2][4] == rows[3][4] == rows[4][4]
    run(diarizer, "shared sources", rows, src, dst_len)


def wide_table(shift):
    """rows that can all take the wide loads -- one and two channels, frame `head` of the source on a 16-byte boundary -- or, with shift = 1, the same rows
    with every source one element further on, which none of them can"""
    t, k = Table(), 0
    for enc in ENCS:
        es = ES[enc]
        for channels, channel in ((1, 0), (1, -1), (2, 0), (2, 1), (2, -1)):
            for dst_mod in range(4):
                head = (-dst_mod) % 4
                for n in (4, 9, 256, 1030):
                    el = elements(enc, n * channels, 9000 + k)
                    t.add(enc, channels, channel, n, dst_mod, PAD, src_mod=(-head * es * channels + shift * es) % 16, el=el)
                    k += 1
    return t.done()


def test_wide_loads_and_element_loads_give_the_same_bytes(diarizer):
    outs = []
    for shift in (0, 1):
        rows, src, dst_len = wide_table(shift)
        for enc, channels, channel, n, so, dof, room in rows.tolist():
            head = (-dof) % 4
            aligned = (so + head * ES[enc] * channels) % min(16, 4 * ES[enc] * channels) == 0
            assert aligned == (shift == 0), (shift, enc, channels, so, dof)
        outs.append(run(diarizer, "wide table, shift %d" % shift, rows, src, dst_len))
    assert outs[0].tobytes() == outs[1].tobytes()


# ------------------------------------------------------------------ the cases can tell planted mistakes apart

def named_cases():
    t = Table()
    a = t.add(G.ENC_MULAW, 2, 0, 1001, 0, PAD, seed=21)
    t.share(a, 1, 3, PAD)
    legs = t.done()
    t = Table()
    t.add(G.ENC_S16, 1, 0, 257, 1, PAD, seed=31)
    t.add(G.ENC_ALAW, 2, -1, 8, 0, PAD, seed=32)
    last = t.done()
    t = Table()
    t.add(G.ENC_F32, 1, 0, 5, 2, 1, seed=33)
    t.add(G.ENC_MULAW, 1, 0, 300, 0, PAD - 1, seed=34)
    rooms = t.done()
    return {"channel_stride": ("the legs of a stereo call", legs), "pad_zeros_missing": ("the legs of a stereo call", legs),
            "one_element_past_the_last": ("rows that read the last element of their source", last), "room_ignored": ("rooms that cut the zeros", rooms)}


@pytest.mark.parametrize("mistake", MISTAKES)
def test_a_planted_mistake_changes_a_byte_of_a_named_case(diarizer, mistake):
    name, (rows, src, dst_len) = named_cases()[mistake]
    good, bad = expected(rows, src, dst_len), expected(rows, src, dst_len, mistake)
    assert good.tobytes() != bad.tobytes(), (mistake, name)
    for other in MISTAKES:                                                  # and every mistake is caught by some named case
        n2, (r2, s2, d2) = named_cases()[other]
        assert expected(r2, s2, d2).tobytes() != expected(r2, s2, d2, other).tobytes()
    same("k_group_ingest %s" % name, diarizer.group_ingest_case(rows, src, dst_len, canary=float(FC)), good)


def test_hook_refusals_come_before_any_launch(diarizer):
    t = Table()
    t.add(G.ENC_S16, 2, 0, 100, 0, PAD, seed=41)
    t.add(G.ENC_MULAW, 1, 0, 100, 0, PAD, seed=42)
    rows, src, dst_len = t.done()

    def bad(r, col, v):
        tab = np.array(rows)
        tab[r, col] = v
        out = diarizer.group_ingest_case(tab, src, dst_len, canary=float(FC), refused=True)
        assert (out == 0).all()                                             # nothing came back: nothing was launched
    bad(0, 0, 4)                                # an unknown encoding
    bad(0, 1, 0)                                # channels < 1
    bad(0, 2, 2)                                # channel outside [-1, channels)
    bad(1, 3, -1)                               # n < 0
    bad(1, 4, len(src))                         # a source that leaves src
    bad(0, 4, 1)                                # an int16 source at an odd byte
    bad(1, 5, int(rows[0][5]))                  # two rows share a destination
    bad(1, 6, dst_len)                          # a room that leaves the destination
