"""Operands, expected values and tolerances of tests/test_frontend_kernels.py (GPU) -- built here so that tests/test_frontend_ref.py can hold the float32
restatement of the kernel to every tolerance, and show what every tolerance rejects, on the CPU.  Nothing here touches the GPU.

A feature case is a dict: wav (the held slice), n_total, origin, first_item, masks [items][293], skip (option skip_dead_rows), pack (which window / mel
bank: PACKS).  reference(name) computes, once per process, the row plan and the expected feature rows with their tolerances.  The item of a call is the
triple (chunk, speaker): item i reads the chunk that starts at sample ((first_item + i) // 3) * 8000, so the three items of a chunk share their audio and
differ in their masks.  Signals that must not mix sit ten chunks (30 items) apart; the items between them are dead (nothing selected).
"""
import functools

import numpy as np

import frontend_ref as R

CANARY = -7776.0
ICANARY = -7776
GRID = 512                   # the grid k_stft_fbank takes on the MI355X (2 x 256 compute units) once more items are live: the looping case is built for it
ABOVE_HALF = np.nextafter(np.float32(0.5), np.float32(1))
BELOW_HALF = np.nextafter(np.float32(0.5), np.float32(0))
PRE = np.concatenate([[0], np.cumsum(R.FRAME_LEN)])          # samples of the first a mask frames


# ---------------------------------------------------------------- windows and banks
@functools.lru_cache(None)
def product_tables():
    import torch
    import weightpack
    return torch.hamming_window(400).numpy().astype(np.float32), np.asarray(weightpack.mel_matrix(), np.float32)


def onehot_bank(first_bin, n, pair=None):
    """filter m < n stores exactly one weight of 1, at bin first_bin + m; filter 79 stores the two bins of `pair` (a gain on one bin of a one-bin filter
    is a constant per channel, which the mean normalisation removes: only beside another bin does bin 0 or bin 200 show its weight)"""
    mel = np.zeros((R.NBINS, R.NMELS), np.float32)
    for m in range(n):
        mel[first_bin + m, m] = 1.0
    if pair:
        mel[list(pair), 79] = 1.0
    return mel


BIN_PACKS = {"bins0": (0, 79, (0, 1)), "bins79": (79, 79, None), "bins158": (158, 43, (199, 200))}


@functools.lru_cache(None)
def tables(pack):
    """-> window [400], fbank.matrix [201][80] of a pack of PACKS"""
    win, mel = product_tables()
    if pack == "product":
        return win, mel
    if pack == "asym":                                       # strictly increasing: win[k] != win[400 - k] everywhere
        return (0.1 + 0.9 * np.arange(400) / 399.0).astype(np.float32), mel
    return np.ones(400, np.float32), onehot_bank(*BIN_PACKS[pack])


PACKS = ("product", "asym") + tuple(BIN_PACKS)


# ---------------------------------------------------------------- masks
def first_frames(a):
    m = np.zeros(R.FRAMES, np.float32)
    m[:a] = 1
    return m


def frames_mask(idx):
    m = np.zeros(R.FRAMES, np.float32)
    m[np.asarray(idx, np.int64)] = 1
    return m


def len_times_T(a, b):
    return np.float32(np.float32(PRE[a]) / np.float32(PRE[b])) * np.float32(R.T)


@functools.lru_cache(None)
def tie_pairs():
    """(a, b): the first a and the first b mask frames in one batch give len * 501 = k + 0.5 exactly in float32"""
    return [(a, b) for b in range(3, R.FRAMES + 1) for a in range(3, b) if float(len_times_T(a, b)) % 1.0 == 0.5]


@functools.lru_cache(None)
def pair_for_nvalid(nv):
    """(a, b), b smallest: the first a frames beside the first b frames (the batch maximum) have nvalid = nv"""
    for b in range(3, R.FRAMES + 1):
        for a in range(3, b):
            if int(np.ceil(len_times_T(a, b))) == nv:
                return a, b
    raise ValueError(nv)


def prepare_masks(items, seed=5):
    """masks for the exact parts: batches of 32 cycle through five kinds; the values that are on / off are drawn from the edge values"""
    rng = np.random.default_rng(seed)
    on_vals = np.array([1, 2, ABOVE_HALF, 0.75, 1e30], np.float32)
    off_vals = np.array([0, 0.5, -1, np.nan, BELOW_HALF, -np.inf], np.float32)
    ties = tie_pairs()
    masks = np.zeros((items, R.FRAMES), bool)
    for i in range(items):
        b, j = divmod(i, 32)
        kind = b % 5
        m = np.zeros(R.FRAMES, bool)
        if kind == 0:                                        # the shapes
            shape = j % 8
            if shape == 0: m[:] = True
            elif shape == 2: m[0] = True
            elif shape == 3: m[292] = True
            elif shape == 4: m[j % 5:j % 5 + 2] = True      # two frames: 546 or 547 samples
            elif shape == 5: m[:3] = True
            elif shape == 6: m[j % 2::2] = True
            elif shape == 7: m[rng.random(R.FRAMES) < 0.3] = True
        elif kind == 1:                                      # a whole batch under 640 samples
            m[:j % 3] = True
        elif kind == 2:                                      # a small batch maximum: five frames
            m[10:10 + (2, 3, 4, 5)[j % 4]] = True
        elif kind == 3:                                      # rounding ties
            a, bb = ties[(b // 5) % len(ties)]                # (14, 28) first: 3 823 and 7 646 samples
            m[:(a if j % 2 == 0 else bb)] = True
        else:                                                # live and dead interleaved
            if j % 2 == 0: m[rng.integers(0, 250):][:rng.integers(3, 40)] = True
        if (i >= 1019 and i % 1024 >= 1019) or (i >= 1024 and i % 1024 < 3):       # a run of dead items across every 1024-item step
            m[:] = False
        masks[i] = m
    vals = np.where(masks, on_vals[rng.integers(0, len(on_vals), masks.shape)], off_vals[rng.integers(0, len(off_vals), masks.shape)])
    return vals.astype(np.float32)


PREPARE_ITEMS = (1, 31, 32, 33, 70, 1023, 1024, 1025, 2048, 2100)


def prepare_expected(masks, compact, **wrong):
    """the exact parts of sd_test_frontend_prepare from frontend_ref (wrong: ge=True, batch=0 -- the mistakes of test_frontend_ref.py)"""
    prefix, counts = R.mask_prefix(masks, ge=wrong.get("ge", False))
    lens, nn, nv, flags = R.wav_lens(counts, batch=wrong.get("batch", 32))
    out = dict(prefix=prefix, counts=counts, wav_lens=lens, nnorm=nn, nvalid=nv, flags=flags)
    if compact:
        alist, cidx = R.compact_active(flags)
        out.update(alist=alist, cidx=cidx, nnorm_c=nn[alist], nvalid_c=nv[alist], n_active=len(alist))
    return out


# ---------------------------------------------------------------- signals
def noise(n, seed, scale=1.0):
    return (scale * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def tone(n, k, amp=0.5):
    return (amp * np.cos(2 * np.pi * k * np.arange(n) / 400.0 + 0.3)).astype(np.float32)


def every_bin(n):
    """400-periodic: sum_k a_k cos(2 pi k n / 400 + phi_k), a_k falling 40 dB from bin 0 to bin 200, fixed random phases"""
    rng = np.random.default_rng(77)
    k = np.arange(201)
    a, phi = 0.01 * 10.0 ** (-2.0 * k / 200.0), rng.uniform(0.2, 1.2, 201)
    t = np.arange(400)
    period = (a[:, None] * np.cos(2 * np.pi * k[:, None] * t[None, :] / 400.0 + phi[:, None])).sum(0)
    return np.tile(period, n // 400 + 1)[:n].astype(np.float32)


THREE = np.stack([first_frames(3), first_frames(10), first_frames(R.FRAMES)])        # 820 samples (the shortest live item), 2 731, everything


def _spread(signals, masks3=THREE, other=None):
    """one chunk per signal, ten chunks apart, three items each (masks3; other = {signal: its own three masks}); everything between is dead"""
    S = len(signals)
    wav = np.zeros(80000 * S, np.float32)
    masks = np.zeros((30 * S, R.FRAMES), np.float32)
    for s, sig in enumerate(signals):
        wav[80000 * s:80000 * (s + 1)] = sig
        masks[30 * s:30 * s + 3] = (other or {}).get(s, masks3)
    return wav, masks


MARGIN_SIGNAL = 7            # of case "signals": its first item (MARGIN_ITEM) has its loudest frame outside nvalid and inside the stored rows
MARGIN_ITEM = 30 * MARGIN_SIGNAL


def _burst(base_seed, at):
    x = noise(80000, base_seed, 1e-4)                        # the burst: 90 dB above the floor
    for lo, hi in at:
        x[lo:hi] = noise(hi - lo, base_seed + 1, 1e-4 * 10 ** 4.5)
    return x


@functools.lru_cache(None)
def feature_case(name):
    c = dict(origin=0, first_item=0, skip=True, pack="product", name=name)
    if name == "rows":
        # need = 71 (with `masks`), 80, 81, 96, 97, 500, 501 (nvalid 436 and 437: the cap of nvalid + 65) and a full item: one batch of 32 per target,
        # the first a frames beside the first b frames, the rest dead
        targets = (15, 16, 31, 32, 435, 436, 437)
        masks = np.zeros((32 * len(targets), R.FRAMES), np.float32)
        for k, nv in enumerate(targets):
            a, b = pair_for_nvalid(nv)
            masks[32 * k + 4], masks[32 * k + 17] = first_frames(a), first_frames(b)
        c.update(masks=masks, wav=noise(((len(masks) - 1) // 3) * 8000 + 80000, 11))
    elif name in ("masks", "masks_all_rows"):
        # all on, alternating, scattered single frames, only the last frames of the chunk, three frames (need 71), two frames (dead), nothing
        masks = np.stack([first_frames(293), frames_mask(np.arange(1, 293, 2)), frames_mask([0, 7, 19, 20, 58, 101, 150, 151, 152, 201, 250, 291, 292]),
                          frames_mask(np.arange(270, 293)), first_frames(3), first_frames(2), first_frames(0)])
        c.update(masks=masks, wav=noise(2 * 8000 + 80000, 12), skip=name == "masks")
    elif name == "end":
        # chunk 1 (items 3 .. 5) starts at 8000; the recording ends at 58137, inside a selected frame of items 3 and 5; item 4 selects only frames past it
        masks = np.stack([first_frames(293), first_frames(100), frames_mask(np.arange(0, 293, 2)),
                          first_frames(293), frames_mask(np.arange(200, 293)), frames_mask(np.arange(1, 293, 2))])
        c.update(masks=masks, wav=noise(58137, 13))
    elif name.startswith("pos_"):
        # pos_<first_item>_<0 | 1 | 2>: origin 0, the slice starting exactly at the first chunk needed, and that with the recording ending inside the last chunk
        _, fi, mode = name.split("_")
        fi, mode = int(fi), int(mode)
        masks = np.stack([first_frames(293), frames_mask(np.arange(1, 293, 2)), first_frames(3), first_frames(0), first_frames(40), frames_mask(np.arange(250, 293))])
        first, last = (fi // 3) * 8000, ((fi + 5) // 3) * 8000 + 80000
        n_total = last - 30011 if mode == 2 else last + 5000
        full = noise(n_total, 14)
        origin = 0 if mode == 0 else first
        c.update(masks=masks, first_item=fi, origin=origin, wav=full[origin:], n_total=n_total)
    elif name == "signals":
        gap = noise(80000, 21)
        gap[1000:30000] = 0; gap[50000:50160] = 0; gap[60000:60001] = 0                     # stretches of digital silence inside an item
        sigs = [noise(80000, 20, 1e-4), noise(80000, 26, 1e-6), gap, (0.5 + noise(80000, 22, 1e-3)).astype(np.float32),
                _burst(23, [(770, 820), (2681, 2731)]),          # the last 50 selected samples of the 3- and of the 10-frame item
                _burst(24, [(0, 50)]),                           # frame 0
                _burst(25, [(560, 610), (2480, 2530)]),          # the last frame below nvalid (5 of 6, 17 of 18) and no later one
                # the burst in the margin: the first 11 mask frames are 3 004 samples, len * 501 = 18.81, nvalid 19, 84 rows; the last 50 selected samples
                # lie in frame 18 at window positions 274 .. 323 and in frame 19 at 114 .. 163, nearer the window's centre: the maximum is frame 19's
                _burst(27, [(2954, 3004)])]
        c.update(zip(("wav", "masks"), _spread(sigs, other={MARGIN_SIGNAL: np.stack([first_frames(11), first_frames(0), first_frames(R.FRAMES)])})))
    elif name == "tones":
        c.update(zip(("wav", "masks"), _spread([tone(80000, k) for k in (0, 12, 13, 25, 187, 188, 199, 200)])))
    elif name.startswith("bins"):
        c.update(masks=first_frames(293)[None, :].copy(), wav=every_bin(80000), pack=name)
    elif name == "asym":
        c.update(masks=np.stack([first_frames(293), frames_mask(np.arange(1, 293, 2)), first_frames(3)]), wav=noise(80000, 31), pack="asym")
    elif name == "tie":
        # 3 823 and 7 646 samples: len * 501 = 250.5 exactly: nnorm 250, nvalid 251
        c.update(masks=np.stack([first_frames(14), first_frames(28), first_frames(0)]), wav=noise(80000, 32))
    elif name in ("loop", "loop_thinned"):
        c.update(loop_operands(name == "loop_thinned"))
    else:
        raise KeyError(name)
    c.setdefault("n_total", c["origin"] + len(c["wav"]))
    return c


LOOP_ITEMS = 33 * 32


def loop_full_slots():
    return [32 * b + (17 * b) % 32 for b in range(LOOP_ITEMS // 32)]           # one per batch; 0 and 511 (= GRID - 1) among them


def loop_operands(thinned):
    """1 056 live items on a grid of 512: 3 .. 10 mask frames each (71 .. 83 rows) but one full-length item per batch of 32, which reads mostly the loud
    audio between the short items' samples (60 dB above them).  The item GRID slots behind a full one below 512 is a three-frame item on audio another
    60 dB down: the workgroup that has just finished the loudest, longest item takes the quietest, shortest one.  thinned: every third short item that
    is neither of those is switched off, so every later item moves to another slot, workgroup and predecessor while its operands stay what they were."""
    rng = np.random.default_rng(41)
    n_chunks = LOOP_ITEMS // 3
    wav = noise((n_chunks - 1) * 8000 + 80000, 40)
    full = loop_full_slots()
    quiet = [s + GRID for s in full if s < GRID]
    masks = np.zeros((LOOP_ITEMS, R.FRAMES), np.float32)
    for i in range(LOOP_ITEMS):
        masks[i] = first_frames(R.FRAMES if i in full else 3 if i in quiet else int(rng.integers(3, 11)))
    scale = np.ones(len(wav))
    for ck in range(n_chunks):
        scale[8000 * ck:8000 * ck + 2731] = 1e-3                                       # what the short items read
    for s in quiet:
        scale[8000 * (s // 3):8000 * (s // 3) + 820] = 1e-6
    if thinned:
        keep = set(full) | set(quiet)
        for i in range(1, LOOP_ITEMS, 3):
            if i not in keep:
                masks[i] = 0
    return dict(masks=masks, wav=(wav * scale).astype(np.float32))


FEATURE_CASES = ("rows", "masks", "masks_all_rows", "end") + tuple("pos_%d_%d" % (f, m) for f in (0, 32, 96) for m in (0, 1, 2)) + (
    "signals", "tones", "bins0", "bins79", "bins158", "asym", "tie", "loop", "loop_thinned")
FAMILY = {"rows": "rows", "masks": "masks", "masks_all_rows": "masks", "end": "end", "signals": "signals", "tones": "tones", "bins0": "every bin",
          "bins79": "every bin", "bins158": "every bin", "asym": "asym window", "tie": "tie", "loop": "loop", "loop_thinned": "loop"}


def plan(c):
    """the exact side of a feature case: counts, lens, live items, row offsets"""
    on = R.mask_on(c["masks"])
    prefix, counts = R.mask_prefix(c["masks"])
    lens, nn, nv, flags = R.wav_lens(counts)
    alist, cidx = R.compact_active(flags)
    need = R.need_rows(nv[alist], c["skip"])
    rowoff = np.concatenate([[0], np.cumsum(need)]).astype(np.int32)
    return dict(on=on, counts=counts, nnorm=nn, nvalid=nv, alist=alist, cidx=cidx, rowoff=rowoff, rows_all=int(rowoff[-1]))


def item_signal(c, i, on, **wrong):
    return R.compacted(c["wav"], c["origin"], c["n_total"], ((c["first_item"] + int(i)) // 3) * 8000, on, **wrong)


@functools.lru_cache(None)
def reference(name):
    """-> plan + exp / tol [rows_all][80] (float64) and per live item (vmax, floor, frames with signal)"""
    c = feature_case(name)
    p = plan(c)
    win, mel = tables(c["pack"])
    if name == "loop_thinned":                               # the items that are left have the operands they had: their rows are those of "loop"
        full = reference("loop")
        keep = p["alist"]
        for k in ("counts", "nnorm", "nvalid"):
            assert np.array_equal(p[k][keep], full[k][keep])
        assert np.array_equal(np.diff(p["rowoff"]), np.diff(full["rowoff"])[full["cidx"][keep]])
        rows = np.concatenate([np.arange(full["rowoff"][a], full["rowoff"][a + 1]) for a in full["cidx"][keep]])
        p.update(exp=full["exp"][rows], tol=full["tol"][rows], objs=[full["objs"][a] for a in full["cidx"][keep]])
        return p
    exp, tol, objs = np.zeros((p["rows_all"], R.NMELS)), np.zeros((p["rows_all"], R.NMELS)), []
    for a, i in enumerate(p["alist"]):
        r0, r1 = p["rowoff"][a], p["rowoff"][a + 1]
        it = R.Item(item_signal(c, i, p["on"][i]), int(p["counts"][i]), win, mel, int(p["nnorm"][i]), r1 - r0)
        exp[r0:r1], tol[r0:r1] = it.out, it.tol
        objs.append((it.vmax, it.floor, it.nf))
    p.update(exp=exp, tol=tol, objs=objs)
    return p


# ---------------------------------------------------------------- sig_mode
def smallest_len():
    """the smallest wav_lens sd_embed_signals accepts: the smallest float32 whose product with 501 rounds to 1"""
    x = np.float32(0.5 / 501)
    while np.rint(np.float32(x * np.float32(R.T))) < 1:
        x = np.nextafter(x, np.float32(1))
    return x


@functools.lru_cache(None)
def signals_case(B):
    """B rows of 80000 samples and their lengths: 0.5 (the tie: nnorm 250, nvalid 251), 0.013, the smallest accepted and 1.0, in turn.  Behind
    len * 80000 every row holds content 60 dB above what lies in front, half of it behind the stored rows as well: the maximum over all 501 frames is
    neither the maximum over the first nvalid frames nor the one over the stored rows."""
    lens = np.array([(1.0, 0.5, 0.013, smallest_len())[(i + 1) % 4] for i in range(B)], np.float32)
    sig = np.zeros((B, 80000), np.float32)
    for i in range(B):
        x = noise(80000, 50 + i, 1e-3)
        cut = int(np.ceil(float(lens[i]) * 80000)) + 400
        if cut < 80000:
            x[cut:] = noise(80000 - cut, 150 + i, 1.0)
            x[cut:cut + (80000 - cut) // 2] *= np.float32(0.1)
        sig[i] = x
    return sig, lens


@functools.lru_cache(None)
def signals_reference(B, skip=True):
    sig, lens = signals_case(B)
    nn, nv = R.lens_of(lens)
    need = R.need_rows(nv, skip)
    rowoff = np.concatenate([[0], np.cumsum(need)]).astype(np.int32)
    win, mel = tables("product")
    exp, tol, objs = np.zeros((rowoff[-1], R.NMELS)), np.zeros((rowoff[-1], R.NMELS)), []
    for i in range(B):
        it = R.Item(sig[i], 80000, win, mel, int(nn[i]), int(need[i]))
        exp[rowoff[i]:rowoff[i + 1]], tol[rowoff[i]:rowoff[i + 1]] = it.out, it.tol
        objs.append((it.vmax, it.floor, it.nf))
    return dict(nnorm=nn, nvalid=nv, rowoff=rowoff, rows_all=int(rowoff[-1]), exp=exp, tol=tol, objs=objs)
