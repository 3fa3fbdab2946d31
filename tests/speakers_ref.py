"""float64 / integer references of the known-speaker entries (include/sdhip.h: sd_last_speakers, sd_span_masks, sd_voiceprint*, sd_speaker_distances,
sd_match_speakers) in numpy, and the inputs the CPU and the GPU tests share.  Every sum is sequential: one row, or one dimension, at a time."""
import functools

import numpy as np

CHUNK, HOP, FRAMES, DIM, RATE = 80000, 8000, 293, 192, 16000
MIN_SAMPLES = 640                        # sd.cpp:44


# ------------------------------------------------------------------ centroids
def sequential_mean(rows):
    """rows [n][d] -> sum row by row in ascending order, divided by n"""
    s = np.zeros(rows.shape[1], np.float64)
    for r in rows:
        s = s + r
    return s / float(len(rows))


def centroids(emb, train_labels):
    """emb [M][d] float64 with NaN rows, train_labels [N] = the final cluster of every train row (rows whose first element is not NaN, sd.cpp:2224),
    in row order -> (centroids [K][d], counts [K]): the means of the un-normalised train rows, members in ascending row order"""
    flat = np.asarray(emb, np.float64).reshape(-1, np.shape(emb)[-1])
    train = flat[~np.isnan(flat[:, 0])]
    lab = np.asarray(train_labels)
    assert len(lab) == len(train)
    if len(train) == 0:
        return np.full((1, flat.shape[1]), np.nan), np.zeros(1, np.int64)
    K = int(lab.max()) + 1
    cen = np.stack([sequential_mean(train[lab == k]) for k in range(K)])
    return cen, np.bincount(lab, minlength=K).astype(np.int64)


def planted_embeddings(chunks=40, clusters=3, nan_fraction=0.25, seed=21, small=0):
    """[chunks][3][192] float64 (f32-valued, as the embedding stage yields them): `clusters` well separated directions + noise, a NaN row
    with probability nan_fraction; small > 0: the last `small` live rows form one more cluster of their own"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((clusters + 1, DIM)) * 2.0
    M = chunks * 3
    which = rng.integers(0, clusters, M)
    dead = rng.random(M) < nan_fraction
    if small:
        live = np.flatnonzero(~dead)
        which[live[-small:]] = clusters
    X = cen[which] + 0.3 * rng.standard_normal((M, DIM))
    emb = X.astype(np.float32).astype(np.float64)
    emb[dead] = np.nan
    return emb.reshape(chunks, 3, DIM)


# ------------------------------------------------------------------ span masks
def frame_start(f):
    """first sample of mask frame f of a chunk: frame_start of csrc/frontend.hip = ceil(80000 f / 293)"""
    return (CHUNK * np.asarray(f, np.int64) + (FRAMES - 1)) // FRAMES


def num_chunks(n):
    i = cnt = 0
    if n > CHUNK:
        cnt = (n - CHUNK + HOP - 1) // HOP
        i = cnt * HOP
    if i + 1 < n:
        cnt += 1
    return cnt


def _to_sample(t, n):
    s = t * float(RATE)
    return n if s >= n else min(n, max(0, int(round(s))))          # round(): half to even, as llrint


def span_samples(spans, label, n):
    """[(start, end, label)] -> merged [first, end) sample pairs: round-half-even of t * 16000, clamped to [0, n]; None or (no span, label < 0) = everything"""
    if spans is None or (len(spans) == 0 and label < 0):
        return [(0, n)]
    v = []
    for a, b, l in spans:
        if label >= 0 and l != label:
            continue
        ia, ib = _to_sample(a, n), _to_sample(b, n)
        if ib > ia:
            v.append((ia, ib))
    out = []
    for a, b in sorted(v):
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], b))
        else:
            out.append((a, b))
    return out


def span_masks(n, spans, label=-1):
    """[chunks * 3][293] float32: row 3c frame f is 1 iff sample c * 8000 + frame_start(f) < n lies in a span; rows 3c + 1, 3c + 2 are zero"""
    c = num_chunks(n)
    inside = np.zeros(n + CHUNK + 1, bool)
    for a, b in span_samples(spans, label, n):
        inside[a:b] = True
    m = np.zeros((c * 3, FRAMES), np.float32)
    fs = frame_start(np.arange(FRAMES))
    for ck in range(c):
        s = ck * HOP + fs
        m[3 * ck] = inside[s] & (s < n)
    return m


def live_windows(masks):
    """rows 3c whose selected samples reach 640 inside their batch of 32 items by the reference's rule (sd.cpp:2479, 2501): with rows 3c + 1, 3c + 2 empty
    that is `count >= 640` -- the batch maximum only matters when it is below 640 itself, and then every row of the batch is dead anyway"""
    per_frame = np.diff(frame_start(np.arange(FRAMES + 1)))
    return ((masks[0::3] > 0.5) * per_frame[None, :]).sum(1) >= MIN_SAMPLES


def voiceprint(emb_rows):
    """emb_rows [chunks * 3][192] float32 of Diarizer.embed -> (mean of the non-NaN rows 3c in float64, ascending, sequential; their number)"""
    rows = np.asarray(emb_rows)[0::3]
    live = rows[~np.isnan(rows[:, 0])].astype(np.float64)
    if len(live) == 0:
        return np.full(DIM, np.nan), 0
    return sequential_mean(live), len(live)


# ------------------------------------------------------------------ distances and matching
def cosine_distances(cen, gal):
    """[K][M]: 1 - dot / (sqrt(m1) * sqrt(m2)), dot, m1, m2 summed over the dimensions in ascending order (sd.cpp:476-498); a centroid row whose first
    element is NaN gives a NaN row"""
    cen, gal = np.asarray(cen, np.float64), np.asarray(gal, np.float64)
    K, d = cen.shape
    M = len(gal)
    dot, m1, m2 = np.zeros((K, M)), np.zeros((K, 1)), np.zeros((1, M))
    for i in range(d):
        dot = dot + cen[:, i:i + 1] * gal[None, :, i]
        m1 = m1 + cen[:, i:i + 1] * cen[:, i:i + 1]
        m2 = m2 + gal[None, :, i] * gal[None, :, i]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = 1.0 - (dot / (np.sqrt(m1) * np.sqrt(m2)))
    out[np.isnan(cen[:, 0])] = np.nan
    return out


def greedy_match(dist, threshold):
    """pairs with dist <= threshold in (dist, k, m) order, taken when both sides are free -> (match [K] or -1, distance [K] or NaN)"""
    K, M = dist.shape
    pairs = sorted((dist[k, m], k, m) for k in range(K) for m in range(M) if dist[k, m] <= threshold)
    match, best = np.full(K, -1, np.int32), np.full(K, np.nan)
    used = set()
    for v, k, m in pairs:
        if match[k] < 0 and m not in used:
            match[k], best[k] = m, v
            used.add(m)
    return match, best


@functools.lru_cache(maxsize=None)
def distance_case(K, M, d, integers):
    """(centroids, gallery), computed once, read-only"""
    rng = np.random.default_rng(1000 * K + 7 * M + d + int(integers))
    if integers:
        cen, gal = rng.integers(-4, 5, (K, d)).astype(np.float64), rng.integers(-4, 5, (M, d)).astype(np.float64)
        cen[np.abs(cen).sum(1) == 0, 0] = 1.0
        gal[np.abs(gal).sum(1) == 0, 0] = 1.0
    else:
        cen, gal = rng.standard_normal((K, d)), rng.standard_normal((M, d))
    cen.setflags(write=False)
    gal.setflags(write=False)
    return cen, gal
