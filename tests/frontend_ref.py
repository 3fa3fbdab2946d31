"""Float64 references of the embedding front end (csrc/frontend.hip), their per-element tolerances, and a float32 restatement of the kernel's
arithmetic in which single rules can be replaced by a wrong one (tests/test_frontend_ref.py).  Plain numpy; no GPU, no torch.

Rules (the reference's sd.cpp / threeModel.py lines are cited in frontend.hip):
  mask      frame f of 293 is on where mask > 0.5 and holds the chunk's samples [ceil(80000 f / 293), ceil(80000 (f + 1) / 293))
  compact   the samples of the frames that are on, in order; a sample at or past the end of the recording reads as zero (it still counts)
  lengths   per batch of 32 consecutive items: max = the largest count; the whole batch is dead when max < 640, an item is dead when its count < 640;
            len = float32(cnt) / float32(max) (1 for a dead item); nnorm = round-half-even(len * 501), nvalid = clamp(ceil(len * 501), 1, 501), both on
            the float32 product
  STFT      n_fft 400, hop 160, centre (200 zeros on both sides), window as stored; real and imaginary part cast to float32
  features  power -> mel -> 10 log10(max(., 1e-10)) -> max(., maximum over all 501 frames - 80) -> minus the mean over the first nnorm frames
"""
import numpy as np

CHUNK, FRAMES, HOP, T, NFFT, NBINS, NMELS, FEAT_LD, MIN_SAMPLES, MARGIN = 80000, 293, 160, 501, 400, 201, 80, 96, 640, 65
U = 2.0 ** -24
U64 = 2.0 ** -53
LOG10F_ULP = 2.0            # ASSUMED accuracy of the device log10f in ulp (tests/test_frontend_kernels.py says where the figure comes from)
FFT_C = 64.0                # Higham, Accuracy and Stability, 24.2: |dX|_2 <= log2(N) eta |X|_2, eta ~ 7 u64 with computed twiddles: 9 x 7 = 63 for N = 400


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U / (1.0 - n * U)


def frame_start(f):
    return (CHUNK * np.asarray(f, np.int64) + FRAMES - 1) // FRAMES


FRAME_LEN = (frame_start(np.arange(1, FRAMES + 1)) - frame_start(np.arange(FRAMES))).astype(np.int64)      # 273 or 274


def mask_on(masks, ge=False):
    m = np.asarray(masks, np.float32)
    with np.errstate(invalid="ignore"):
        return (m >= np.float32(0.5)) if ge else (m > np.float32(0.5))


def mask_prefix(masks, ge=False):
    """-> prefix [items][294] (selected samples before mask frame f), counts [items]"""
    on = mask_on(masks, ge)
    pre = np.zeros((on.shape[0], FRAMES + 1), np.int64)
    pre[:, 1:] = np.cumsum(on * FRAME_LEN[None, :], axis=1)
    return pre.astype(np.int32), pre[:, -1].astype(np.int32)


def lens_of(len32, nnorm_rule="even"):
    """float32 relative lengths -> nnorm, nvalid"""
    lt = (np.asarray(len32, np.float32) * np.float32(T)).astype(np.float32)
    if nnorm_rule == "even":
        nn = np.rint(lt)
    elif nnorm_rule == "ceil":
        nn = np.ceil(lt)
    else:
        nn = np.floor(lt.astype(np.float64) + 0.5)         # half up
    return nn.astype(np.int32), np.clip(np.ceil(lt), 1, T).astype(np.int32)


def wav_lens(counts, batch=32, nnorm_rule="even"):
    """-> len float32 [items], nnorm, nvalid, flags (1 = dead)"""
    counts = np.asarray(counts, np.int64)
    n = len(counts)
    lens, flags = np.ones(n, np.float32), np.zeros(n, np.int32)
    for b0 in range(0, n, batch if batch else n):
        c = counts[b0:b0 + (batch if batch else n)]
        mx = c.max()
        short = c < MIN_SAMPLES
        l = np.where(short, np.float32(1), c.astype(np.float32) / np.float32(max(mx, 1))).astype(np.float32)
        if mx < MIN_SAMPLES:
            l[:] = 1
        lens[b0:b0 + len(c)] = l
        flags[b0:b0 + len(c)] = short | (mx < MIN_SAMPLES)
    nn, nv = lens_of(lens, nnorm_rule)
    return lens, nn, nv, flags


def compact_active(flags):
    """-> alist [n_active], cidx [items]"""
    live = np.asarray(flags) == 0
    alist = np.flatnonzero(live).astype(np.int32)
    cidx = np.full(len(flags), -1, np.int32)
    cidx[alist] = np.arange(len(alist), dtype=np.int32)
    return alist, cidx


def need_rows(nvalid, skip_dead_rows=True):
    return np.minimum(T, np.asarray(nvalid) + MARGIN) if skip_dead_rows else np.full(np.shape(nvalid), T)


def compacted(wav, origin, n_total, chunk_start, on, floor_src=False, past_end="zero", origin_err=0):
    """the compacted signal [80000] float32 of one item: wav[0] is sample `origin` of a recording of n_total samples"""
    sig = np.zeros(CHUNK, np.float32)
    f = np.flatnonzero(on)
    if not len(f):
        return sig
    starts = (CHUNK * f) // FRAMES if floor_src else frame_start(f)
    src = np.concatenate([np.arange(s, s + l) for s, l in zip(starts, FRAME_LEN[f])]) + chunk_start
    ok = src < n_total
    idx = src - origin + origin_err
    if past_end == "zero":
        sig[:len(src)][ok] = wav[idx[ok]]
    else:                                   # the mistake: what lies behind the end in the buffer (the caller passes a longer buffer)
        sig[:len(src)] = wav[idx]
    return sig


def sparse_bank(mel):
    """fbank.matrix [201][80] -> lo [80], cnt [80]: per filter the run from its first to its last non-zero bin (weights.cpp)"""
    mel = np.asarray(mel, np.float32)
    lo, cnt = np.zeros(NMELS, np.int64), np.zeros(NMELS, np.int64)
    for m in range(NMELS):
        nz = np.flatnonzero(mel[:, m])
        if len(nz):
            lo[m], cnt[m] = nz[0], nz[-1] - nz[0] + 1
    return lo, cnt


def frames_of(sig, n_frames, pad=200, hop=HOP, shift=0):
    """[n_frames][400] float64 view of the centred, zero-padded signal"""
    x = np.concatenate([np.zeros(pad), np.asarray(sig[:hop * n_frames + NFFT + 1], np.float64), np.zeros(NFFT + 1)])
    idx = hop * np.arange(n_frames)[:, None] + np.arange(NFFT)[None, :] + shift
    return x[idx]


def computed_frames(cnt):
    """frames whose window holds a sample below cnt: frame t reads the compacted samples [160 t - 200, 160 t + 200)"""
    return int(min(T, max(0, (cnt + 200 + HOP - 1) // HOP)))


class Item:
    """the float64 reference of one item with its running quantities, and the per-element tolerance derived from them"""

    def __init__(self, sig, cnt, window, mel, nnorm, rows):
        mel64 = np.asarray(mel, np.float32).astype(np.float64)
        lo, c = sparse_bank(mel)
        nf = computed_frames(cnt)                                # the others are exactly zero signal: power 0, -100 dB
        fr = frames_of(sig, nf)
        xw = fr * np.asarray(window, np.float32).astype(np.float64)[None, :]
        X = np.fft.rfft(xw, axis=1)
        re, im = X.real.astype(np.float32).astype(np.float64), X.imag.astype(np.float32).astype(np.float64)
        P = re * re + im * im
        M = P @ mel64
        a = np.maximum(M, 1e-10)
        # frames at and past max(rows, nf) are -100 dB like every frame past nf, and no output row: the arrays end there (the maximum over them is
        # the maximum over all 501 frames)
        Tn = min(T, max(int(rows), nf, int(nnorm)))
        db = np.full((Tn, NMELS), -100.0)
        db[:nf] = 10.0 * np.log10(a)
        self.vmax = db.max()
        floor = self.vmax - 80.0
        y = np.maximum(db, floor)
        self.mean = y[:nnorm].mean(axis=0)
        self.db, self.y, self.floor, self.nf, self.nnorm, self.rows = db, y, floor, nf, int(nnorm), int(rows)
        self.out = (y - self.mean[None, :])[:rows]
        # ---- tolerance
        # both FFTs (the kernel's mixed-radix one and this file's) in fp64: every bin within E of the true value
        E = 2.0 * FFT_C * U64 * np.sqrt(NFFT) * np.sqrt((xw * xw).sum(axis=1))[:, None]
        # two values within E of each other, each cast to f32: 2 u |.| + E apart; two products and a sum (or one product and an FMA): gamma_2
        dP = (gamma(2) + 4.5 * U) * P + 2.1 * E * (np.abs(re) + np.abs(im)) + 2.1 * E * E + 2.0 ** -125
        absmel = np.abs(mel64)
        dM = gamma(c)[None, :] * (P @ absmel) + (1.0 + gamma(c))[None, :] * (dP @ absmel)
        # log10 of max(., 1e-10): mean-value bound on the smaller argument; exactly nothing where both sides sit on the floor.  6e-8: 1e-10f is not 1e-10
        dlog = np.where(M + dM <= 1e-10, 0.0, (10.0 / np.log(10.0)) * dM / np.maximum(a - dM, 1e-10))
        ddb = np.zeros((Tn, NMELS))
        ddb[:nf] = dlog
        ddb += (2.0 * LOG10F_ULP + 1.0) * U * (np.abs(db) + ddb) + 6e-8
        # the maximum moves by no more than the cells that can be it
        cand = db + ddb >= (db - ddb).max()
        dfloor = ddb[cand].max() + U * (abs(floor) + 1.0)
        dy = np.where(db - ddb > floor + dfloor, ddb, np.where(db + ddb < floor - dfloor, dfloor, np.maximum(ddb, dfloor)))
        dmean = dy[:nnorm].mean(axis=0) + gamma(nnorm // 3 + 3) * np.abs(y[:nnorm]).mean(axis=0)
        tol = dy + dmean[None, :]
        tol = tol + U * (np.abs(y - self.mean[None, :]) + tol)
        self.tol, self.ddb, self.dfloor = tol[:rows], ddb, dfloor


def f32_item(sig, cnt, window, mel, nnorm, rows, mut=None, t_end=None, stale=None, nvalid=None):
    """the kernel's arithmetic restated in float32 numpy: STFT in float64, cast, power as two products and a sum, an FMA chain over the stored run
    of each filter (emulated in float64 with one rounding per step), float32 log, three interleaved partial sums joined in order.
    t_end: frames computed (None = all 501; the compact form computes `rows`); stale [501][80]: what the scratch holds at frames not computed.
    mut: one wrong rule by name (test_frontend_ref.py)."""
    mut = mut or ""
    f32 = np.float32
    win = np.asarray(window, np.float32).astype(np.float64)
    if mut == "window_symmetric":
        win = (0.54 - 0.46 * np.cos(2 * np.pi * np.arange(NFFT) / (NFFT - 1.0))).astype(np.float32).astype(np.float64)
    if mut == "window_reversed":
        win = win[(NFFT - np.arange(NFFT)) % NFFT]
    mel = np.asarray(mel, np.float32)
    lo, c = sparse_bank(mel)
    t_end = T if t_end is None else int(t_end)
    fr = frames_of(sig, t_end, pad=199 if mut == "pad_199" else 200, shift=1 if mut == "hop_shift" else 0)
    X = np.fft.rfft(fr * win[None, :], axis=1)
    re, im = X.real.astype(f32), X.imag.astype(f32)
    if mut.startswith("swap_bins_"):
        k = int(mut.split("_")[-1])
        re[:, [k, k + 1]] = re[:, [k + 1, k]]; im[:, [k, k + 1]] = im[:, [k + 1, k]]
    P = (re * re).astype(f32) + (im * im).astype(f32)
    if mut == "half_bin_200":
        P[:, 200] *= f32(0.5)
    if mut == "half_bin_0":
        P[:, 0] *= f32(0.5)
    M = np.zeros((t_end, NMELS), f32)
    for m in range(NMELS):
        b0, b1 = 0, int(c[m])
        if mut == "drop_first_weight_%d" % m:
            b0 = 1
        if mut == "drop_last_weight_%d" % m:
            b1 -= 1
        acc = np.zeros(t_end, f32)
        for b in range(b0, b1):
            acc = (acc.astype(np.float64) + P[:, lo[m] + b].astype(np.float64) * np.float64(mel[lo[m] + b, m])).astype(f32)      # one rounding: an FMA
        M[:, m] = acc
    with np.errstate(divide="ignore"):
        a = M if mut == "no_floor" else np.maximum(M, f32(1e-10))
        v = (f32(10.0) * np.log10(a).astype(f32)).astype(f32)
    db = np.full((T, NMELS), f32(-100.0)) if stale is None else np.array(stale, f32)
    db[:t_end] = v
    if mut == "stale_row":                                        # the last frame of the item's last tile is not stored: the scratch keeps what it held
        db[t_end - 1] = stale[t_end - 1]
    if mut == "max_nvalid_only":
        vmax = v[:nvalid].max()
    elif mut == "max_stored_only":
        vmax = v[:rows].max()
    else:
        vmax = v.max()                                           # the computed frames
    floor = f32(vmax - f32(79.9 if mut == "top_db_79_9" else 80.0))
    y = np.maximum(db, floor)
    div = nnorm + {"div_plus": 1, "div_minus": -1}.get(mut, 0)
    parts = []
    for g in range(3):
        s = f32(0)
        for val in y[g:nnorm:3]:
            s = s + val
        parts.append(s)
    mean = ((parts[0] + parts[1]).astype(f32) + parts[2]).astype(f32) / f32(div)
    return (y[:rows] - mean[None, :]).astype(f32), db
