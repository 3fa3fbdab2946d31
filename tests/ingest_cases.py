"""The cases of k_many_ingest and of the rule behind sd_diarize_many_audio*, shared by tests/test_ingest_ref.py (CPU: on the float32 rounding of the
oracle's taps) and tests/test_ingest_kernel.py (GPU: on the tap table read back from the device).  A case is a table of rows for
Diarizer.many_ingest_case, the bytes of its sources and the length of the destination; expected() is ingest_ref.ingest_ref on it, computed once.

Shapes are the smallest at which the kernel can go wrong: 1 .. 773 outputs with 255 / 256 / 257 (one short of a tile, a tile, one more; three tiles and
a bit), inputs shorter than one wing of the filter, one frame, every alignment of the base mod 4 (a full tile leaves as 16-byte stores only on an
aligned base), 1 .. 3 channels with every channel and the mean, all 256 codes of both laws."""
import functools

import numpy as np

import ingest_ref as G
import input_cases as K
import input_ref as R

SLACK = G.SLACK
FCANARY = K.FCANARY
ENCS = (G.ENC_S16, G.ENC_F32, G.ENC_MULAW, G.ENC_ALAW)
ENC_NAMES = {G.ENC_S16: "s16", G.ENC_F32: "f32", G.ENC_MULAW: "mulaw", G.ENC_ALAW: "alaw"}
OFF_RATES = (8000, 11025, 32000, 44100, 48000)
CHANNEL_FORMS = ((1, 0), (1, -1), (2, 0), (2, 1), (2, -1), (3, 0), (3, 1), (3, 2), (3, -1))
COUNTS = (1, 2, 3, 255, 256, 257, 773)


def elements(enc, count, seed):
    """`count` elements of an encoding: int16 over the whole range, floats of magnitude 2^-10 .. 1, G.711 codes over all 256; exact zeros among them"""
    g = K.rng(enc, count, seed)
    if enc == G.ENC_F32:
        return np.array(K.signal(count, 1000 + seed))
    if enc == G.ENC_S16:
        v = g.integers(-32768, 32768, count).astype(np.int16)
        v[g.random(count) < 1 / 16] = 0
        return v
    return g.integers(0, 256, count).astype(np.uint8)


def layout(specs, seed, pad_row=False):
    """specs: (enc, channels, channel, sr, n, zeros behind len16, base mod 4[, elements]) -> (rows [R][8] int64, src uint8, dst_len).  Sources follow
    one another at 4-byte aligned offsets; slots follow one another with 5 .. 8 untouched floats between them."""
    rows, parts, at, base = [], [], 0, 3
    for i, sp in enumerate(specs):
        enc, channels, channel, sr, n, extra, mod = sp[:7]
        el = sp[7] if len(sp) > 7 else elements(enc, n * channels, seed * 1000 + i)
        assert len(el) == n * channels
        b = np.ascontiguousarray(el, G.DTYPES[enc]).view(np.uint8)
        b = np.concatenate([b, np.zeros((-len(b)) % 4, np.uint8)])
        base += 5
        base += (mod - base) % 4
        ln = G.len16(n, sr) + extra
        rows.append((enc, channels, channel, sr, n, at if n else -1, base, ln))
        parts.append(b)
        at += len(b)
        base += ln
    if pad_row:
        base += (-base) % 4
        rows.append((G.ENC_F32, 1, 0, 16000, 0, -1, base, R.TAIL_PAD))
        base += R.TAIL_PAD
    src = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return K.frozen(np.array(rows, np.int64)), K.frozen(src), base + 7


def _direct(enc):
    specs = []
    if enc in (G.ENC_MULAW, G.ENC_ALAW):
        specs.append((enc, 1, 0, 16000, 256, 1, 0, np.arange(256, dtype=np.uint8)))      # all 256 codes of the law in one row
    k = 0
    for channels, channel in CHANNEL_FORMS:
        for n in COUNTS:
            specs.append((enc, channels, channel, 16000, n, (0, 1, 3, 300)[k % 4], k % 4 if n != 256 else (k // 4) % 4))
            k += 1
    return specs


def _off_rate(sr):
    L, M, J = R.plan(sr)
    specs, k = [], 0
    for enc in ENCS:
        for no in (1, 255, 256, 257, 773):
            specs.append((enc, 1, 0, sr, K.n_for(sr, no), (0, 1, 300, 2)[k % 4], k % 4))
            k += 1
        for n in (1, 2, J, J + 1):                                                       # inputs shorter than one wing, one frame
            specs.append((enc, 1, 0, sr, n, 1 + k % 3, k % 4))                         # (above 16 kHz one frame gives no output: the slot is zeros)
            k += 1
        specs.append((enc, 2, 1, sr, K.n_for(sr, 300), 4, k % 4))
        specs.append((enc, 3, -1, sr, K.n_for(sr, 257), 0, 0))
        k += 2
    return specs


def _mixed9():
    """nine rows of mixed encodings and rates in one launch: slots longer than len16 by 1 .. 80 000 zeros, a row with n = 0, a full tile on an unaligned
    base (the scalar store path) next to full tiles on aligned ones, and the pad row behind them"""
    return [(G.ENC_MULAW, 1, 0, 8000, 1500, 1, 0),
            (G.ENC_ALAW, 2, 1, 8000, 700, 80000, 0),
            (G.ENC_S16, 2, -1, 44100, 2000, 517, 1),      # len16 = 725: two full tiles on an unaligned base
            (G.ENC_F32, 1, 0, 16000, 1024, 256, 0),       # full tiles on an aligned base, a whole tile of zeros
            (G.ENC_S16, 1, 0, 16000, 1000, 24, 2),
            (G.ENC_F32, 1, 0, 16000, 0, 300, 3),          # n = 0: zeros only
            (G.ENC_ALAW, 3, -1, 11025, 900, 7, 0),
            (G.ENC_MULAW, 2, -1, 48000, 3000, 1024, 0),
            (G.ENC_F32, 3, 2, 32000, 1100, 33, 1)]


SPECS = {"direct_%s" % ENC_NAMES[e]: (lambda e=e: (_direct(e), False)) for e in ENCS}
SPECS.update({"rate_%d" % sr: (lambda sr=sr: (_off_rate(sr), False)) for sr in OFF_RATES})
SPECS["mixed9"] = lambda: (_mixed9(), True)
CASES = list(SPECS)
DIRECT = [k for k in CASES if k.startswith("direct_")]
RATE_CASES = [k for k in CASES if k.startswith("rate_")]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (rows, src, dst_len)"""
    specs, pad = SPECS[name]()
    return layout(specs, CASES.index(name), pad)


def rates_of(name):
    return sorted({int(r[3]) for r in case(name)[0] if r[3] != 16000})


_TABLES = {}


@functools.lru_cache(maxsize=None)
def _expected(name, mistake, on_cpu):
    rows, src, dst_len = case(name)
    return K.frozen(G.ingest_ref(rows, src, _TABLES, dst_len, FCANARY, mistake))


def expected(name, tables=None, mistake=None):
    """tables: sample_rate -> the table read back from the device (None: the float32 rounding of the oracle's taps)"""
    for sr in rates_of(name):
        _TABLES[sr] = K.cpu_table(sr) if tables is None else tables[sr]
    return _expected(name, mistake, tables is None)


# the case that shows each planted mistake of ingest_ref.MISTAKES
SHOWN_BY = {"mulaw_bias_forgotten": "direct_mulaw", "alaw_e0_branch": "direct_alaw", "sign_flipped": "direct_mulaw", "channel_stride": "direct_s16",
            "mean_f64": "direct_f32", "reciprocal_multiply": "direct_s16", "zeros_missing": "mixed9", "last_input_readable": "rate_8000"}


def tie_case(sr):
    """an off-rate row of each encoding, and the same samples decoded on the host as rows of Diarizer.resample_jobs_case: -> (ingest rows, src, dst_len,
    jobs rows, x, arena, [(base, dst_off, count)])"""
    specs = [(enc, 2 if enc in (G.ENC_ALAW, G.ENC_S16) else 1, -1 if enc == G.ENC_S16 else 0, sr, K.n_for(sr, 600), 0, 0) for enc in ENCS]
    rows, src, dst_len = layout(specs, 900 + sr)
    jobs, xs, pairs, x_off, dst_off = [], [], [], 0, 0
    for enc, channels, channel, _, n, so, base, ln in rows:
        es = np.dtype(G.DTYPES[int(enc)]).itemsize
        x = G.frames(src[so:so + n * channels * es].view(G.DTYPES[int(enc)]), int(enc), int(channels), int(channel), int(n))
        jobs.append((sr, 0, 0, n, n, 0, ln, x_off, dst_off))
        pairs.append((int(base), dst_off, int(ln)))
        xs.append(x)
        x_off += n
        dst_off += (int(ln) + 3) // 4 * 4
    return rows, src, dst_len, jobs, np.concatenate(xs), dst_off, pairs
