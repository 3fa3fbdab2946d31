"""The cases of tests/test_input_kernels.py (GPU) and tests/test_input_ref.py (CPU): operands and expected results of the kernels in front of the two
networks, each built once (functools caches; arrays are read-only) with the references of tests/input_ref.py.  The shapes are the smallest at which each
path of a kernel exists; the reasons stand beside them.

Resampler inputs are exact zeros or magnitudes in [2^-10, 1] (input_ref.resample_exact asserts that no product and no partial sum is a float32 subnormal).
The expected bytes of the resampler depend on the tap table, which the GPU test reads back from the device: resample_expected / jobs_expected take the
tables as an argument; on the CPU cpu_table() stands in (the float32 rounding of the oracle's h)."""
import functools
import itertools

import numpy as np

import input_ref as R
from oracle import resample_oracle as ro

SLACK = R.SLACK
FCANARY = np.float32(-7776.0)
HCANARY = 0xC0DE
PAD = R.TAIL_PAD


def rng(*seed):
    return np.random.default_rng([20250] + [int(s) for s in seed])


def frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def signal(n, seed):
    """n float32: magnitudes 2^-10 .. 1 with random signs, one in sixteen an exact zero"""
    g = rng(n, seed)
    v = np.exp2(-10.0 * g.random(n)) * np.where(g.random(n) < 0.5, -1.0, 1.0)
    v[g.random(n) < 1 / 16] = 0.0
    return frozen(v.astype(np.float32))


@functools.lru_cache(maxsize=None)
def cpu_table(in_sr):
    """the float32 rounding of the oracle's taps: what stands in for the device's table where there is no device"""
    h64, inside = R.tap_table_ref(in_sr)
    return frozen(np.where(inside, h64, 0.0).astype(np.float32) + np.float32(0))


# ---------------------------------------------------------------- k_resample
# L = 2 | L = 1, a single phase | 640 phases | L = 160, M = 441 | L = 16 000: the phase changes with every output, 2.2 M taps | a span of 65 492 bytes:
# k_resample_jobs needs the dynamic-LDS attribute and k_resample does not | both need it | the largest span resample_check accepts
SMALL_RATES = (8000, 48000, 11025, 44100, 16001)
LARGE_RATES = (672000, 688000, 1680000)
RATES = SMALL_RATES + LARGE_RATES


def n_for(in_sr, n_out):
    """the smallest n with sd_resample_len(n) >= n_out (at 8 000 Hz the length is 2 n: an odd n_out is asked for by argument)"""
    L, M, J = R.plan(in_sr)
    n = max(n_out * M // L - 2, 1)
    while ro.out_len(n, in_sr, 16000) < n_out:
        n += 1
    return n


def _resample_cases():
    c = {}
    for sr in RATES:
        # one output, one short of a tile, a tile, one more, three tiles and a bit; the rates with thousands of taps: one output, a tile and one more
        for no in ((1, 255, 256, 257, 773) if sr in SMALL_RATES else (1, 257) if sr != 1680000 else (257,)):
            n = n_for(sr, no)
            c["%d_out%d" % (sr, no)] = (sr, n, -1 if ro.out_len(n, sr, 16000) == no else no)
    for sr in (8000, 48000):                                                           # an input shorter than one wing, than both
        J = R.plan(sr)[2]
        for n in (1, 2, J, J + 1, 2 * J + 1):
            c["%d_n%d" % (sr, n)] = (sr, n, -1)
    c["44100_out300_of_773"] = (44100, n_for(44100, 773), 300)                         # n_out smaller than sd_resample_len
    c["11025_out256_of_773"] = (11025, n_for(11025, 773), 256)
    return c


RESAMPLE = _resample_cases()
RESAMPLE_1680000 = [k for k in RESAMPLE if k.startswith("1680000_")]
RESAMPLE_REST = [k for k in RESAMPLE if k not in RESAMPLE_1680000]
ORACLE = ["%d_out773" % sr for sr in SMALL_RATES if sr != 8000] + ["8000_out256"] + ["%d_out257" % sr for sr in LARGE_RATES]      # whole recordings: resample_oracle.resample applies
assert all(RESAMPLE[k][2] == -1 for k in ORACLE)


def resample_case(name):
    """-> (x, in_sr, n_out as the hook takes it, the outputs that come back)"""
    sr, n, n_out = RESAMPLE[name]
    return signal(n, sr), sr, n_out, ro.out_len(n, sr, 16000) if n_out < 0 else n_out


_TABLES = {}      # in_sr -> the table the next expected result is computed on; the caches below are keyed by whose table it is (the device's or cpu_table)


@functools.lru_cache(maxsize=None)
def _resample_expected(name, mistake, on_cpu):
    x, sr, _, no = resample_case(name)
    return frozen(R.resample_ref(x, sr, no, _TABLES[sr], FCANARY, mistake))


def resample_expected(name, taps=None, mistake=None):
    """taps: the table read back from the device (None: cpu_table)"""
    sr = RESAMPLE[name][0]
    _TABLES[sr] = cpu_table(sr) if taps is None else taps
    return _resample_expected(name, mistake, taps is None)


@functools.lru_cache(maxsize=None)
def oracle_expected(name):
    x, sr, _, _ = resample_case(name)
    y64, bound = R.oracle_bound(x, sr)
    return frozen(y64), frozen(bound)


def synthetic_table_case(mistake=None):
    """CPU only: the restatement on a table of random numbers, whose row j = +J is not zero (input_ref's note on "last_tap_dropped")"""
    L, M, J = 3, 2, 5
    taps = signal((2 * J + 1) * L, 77).reshape(2 * J + 1, L) + np.float32(2.0)
    return R.resample_exact(signal(40, 78), 0, 40, 0, 50, taps, L, M, J, mistake)


# ---------------------------------------------------------------- impulses
def impulse_cases():
    """name -> (in_sr, n, [(k, amp)]): powers of two at inputs 0, 1, J, n - 1 - J, n - 1 and at M places in the middle that cover every residue mod M,
    every two of one signal at least 2J + 2 apart (so the five edge places take three signals)"""
    out = {}
    for sr in (8000, 48000):
        L, M, J = R.plan(sr)
        gap = 2 * J + 2
        step = gap + (1 - gap) % M                   # = 1 mod M
        n = (M + 4) * step + gap
        mid = [2 * gap + q * step for q in range(M)]
        assert len({k % M for k in mid}) == M and mid[-1] + gap <= n - 1 - J
        amps = [2.0 ** -e for e in range(12)]
        for tag, edge in (("a", [0, n - 1]), ("b", [1, n - 1 - J]), ("c", [J])):
            ks = sorted(edge + mid)
            out["%d_%s" % (sr, tag)] = (sr, n, [(k, amps[i] * (-1.0) ** i) for i, k in enumerate(ks)])
    return out


IMPULSES = impulse_cases()


def impulse_signal(name):
    sr, n, imp = IMPULSES[name]
    x = np.zeros(n, np.float32)
    for k, a in imp:
        x[k] = a
    return x, sr


# ---------------------------------------------------------------- k_resample_jobs
def _row(x_parts, arena_at, in_sr, m_first, count, pad, dst_mod, back=0, cut=0, extra=40, seed=0):
    """one row: outputs [m_first, +count) at rate in_sr.  The inputs held start `back` in front of the first one the row sums (0: from input 0), reach
    `extra` behind the last one it sums, and the last `cut` of the inputs it sums lie at or behind n_limit.  Its place in the arena: the next float
    that is dst_mod past a 16-byte boundary, three canaries in front of it."""
    L, M, J = R.plan(in_sr)
    need = (m_first * M) // L - J
    first = max(need - back, 0) if back else 0
    last = ((m_first + count - 1) * M) // L + J
    held = last + 1 + extra - first
    n_limit = last + 1 - cut if cut else first + held
    x_off = sum(len(p) for p in x_parts)
    x_parts.append(signal(held, 1000 * in_sr % 9973 + seed))
    dst = (arena_at[0] + 3 + 3) // 4 * 4 + dst_mod
    arena_at[0] = dst + count + pad
    return (in_sr, pad, first, held, n_limit, m_first, count, x_off, dst)


def _jobs_cases():
    c = {}

    def case(name, specs):
        parts, at = [], [0]
        rows = [_row(parts, at, seed=i, **s) for i, s in enumerate(specs)]
        c[name] = (rows, frozen(np.concatenate(parts)), at[0] + 5)

    # R = 1: three tiles, two of them whole and 16-byte aligned (the 16-byte stores), the zero pad behind the last
    case("R1_8000", [dict(in_sr=8000, m_first=0, count=600, pad=512, dst_mod=0)])
    # R = 2: two rate pairs in one launch, m_first not a multiple of 256, inputs held from `first` > 0 on, n_limit in front of the last inputs summed
    case("R2_mixed", [dict(in_sr=11025, m_first=300, count=257, pad=1, dst_mod=1, back=7), dict(in_sr=44100, m_first=1001, count=255, pad=0, dst_mod=2, back=1, cut=90)])
    # R = 9: every count, pad and destination alignment, all five small rate pairs
    counts, pads = (1, 255, 256, 257, 600, 256, 512, 3, 300), (0, 1, 512, 700, 0, 512, 1, 700, 512)
    case("R9", [dict(in_sr=SMALL_RATES[i % 5], m_first=(0, 77, 256, 1000, 12345)[i % 5] if i != 5 else 0, count=counts[i], pad=pads[i], dst_mod=(i + 1) % 4 if i != 5 else 0,
                     back=(0, 3, 0, 50, 1)[i % 5] if i != 5 else 0, cut=(0, 0, 5, 0, 40)[i % 5]) for i in range(9)])
    # a span above 64 KB less the kernel's static LDS, alone: the launch needs the dynamic-LDS attribute, k_resample at this rate does not
    case("R1_672000", [dict(in_sr=672000, m_first=5, count=300, pad=512, dst_mod=3, back=2)])
    # a small-span row beside a large-span one: dynamic LDS is the call's largest span
    case("R2_688000_beside_8000", [dict(in_sr=688000, m_first=0, count=257, pad=1, dst_mod=2), dict(in_sr=8000, m_first=256, count=512, pad=700, dst_mod=0, back=9, cut=3)])
    return c


JOBS = _jobs_cases()


def jobs_case(name):
    return JOBS[name]


@functools.lru_cache(maxsize=None)
def _jobs_expected(name, mistake, on_cpu):
    rows, x, arena = JOBS[name]
    return frozen(R.resample_jobs_ref(rows, x, _TABLES, arena, FCANARY, mistake))


def jobs_expected(name, tables=None, mistake=None):
    """tables: in_sr -> the table read back from the device (None: cpu_table)"""
    for sr in {r[0] for r in JOBS[name][0]}:
        _TABLES[sr] = cpu_table(sr) if tables is None else tables[sr]
    return _jobs_expected(name, mistake, tables is None)


def jobs_refused_case():
    """1 680 000 Hz: resample_check accepts the span (163 704 bytes), with the kernel's static kilobyte the workgroup would need 164 728 > 163 840"""
    parts, at = [], [0]
    rows = [_row(parts, at, in_sr=1680000, m_first=0, count=10, pad=4, dst_mod=0)]
    return rows, np.concatenate(parts), at[0] + 5


# ---------------------------------------------------------------- the copy kernels
KINDS = {"append_f32": (0, np.float32), "append_pcm": (0, np.int16), "scatter": (1, np.float32), "tail_move": (2, np.float32)}
LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025)


def _samples(n, dtype, seed):
    g = rng(n, seed)
    if dtype == np.int16:
        v = g.integers(-32768, 32768, n).astype(np.int16)
        v[:: 97] = -32768
        v[1:: 97] = 32767
        return v
    return (g.standard_normal(n) * 0.3).astype(np.float32)


def _layout(specs, dtype, seed):
    """specs: (dst_mod, src_aligned, len, room) per row -> (src, rows, dst_len).  A row's destination starts dst_mod floats past a 16-byte boundary with
    at least four canaries between it and its neighbours; its source is aligned where the destination's first boundary falls (the wide path) or one
    element off (the narrow one)."""
    rows, s_at, d_at = [], 0, 0
    for dm, aligned, ln, room in specs:
        head = (4 - dm) % 4
        so = s_at + (-(s_at + head)) % 4 + (0 if aligned else 1)
        do = (d_at + 4 + 3) // 4 * 4 + dm
        rows.append((so, do, ln, room))
        s_at, d_at = so + ln, do + room
    return frozen(_samples(s_at + 1, dtype, seed)), frozen(np.array(rows, np.int64)), d_at + 8


@functools.lru_cache(maxsize=None)
def group_case(kind, name):
    """-> (which, src, rows [R][4], dst_len)"""
    which, dtype = KINDS[kind]
    pad = 0 if which == 1 else PAD
    if name == "combo":          # every destination alignment x both source paths x every length x every room
        specs = []
        for dm, al, ln in itertools.product(range(4), (True, False), LENS):
            for room in sorted({0, max(ln - 1, 0), ln, ln + 1, max(ln + pad - 1, 0), ln + pad, ln + pad + 37}):
                specs.append((dm, al, ln, room))
    elif name == "R1":
        specs = [(3, True, 1029, 1029 + pad)]
    elif name == "R3":
        specs = [(1, False, 700, 5000), (0, True, 0, 10), (2, True, 64, 64)]
    elif name == "R1025":        # past the grid's cap of 1 024 table rows
        specs = [(r % 4, r % 3 != 0, r % 13, r % 13 + (r % 5) * 3) for r in range(1025)]
    elif name == "long":         # past the cap of 2 048 blocks along a row
        specs = [(1, True, 2100000, 2100000 + pad + 3)]
    elif name == "neighbours":   # destinations 4 bytes apart and back to back: a store one float too wide lands in the neighbour
        src = _samples(64, dtype, 5)
        return which, frozen(src), frozen(np.array([(0, 3, 5, 5), (8, 9, 7, 7), (17, 16, 6, 6), (24, 22, 9, 9)], np.int64)), 40
    else:
        raise KeyError(name)
    src, rows, dst_len = _layout(specs, dtype, len(specs))
    return which, src, rows, dst_len


GROUP = ("combo", "R1", "R3", "R1025", "long", "neighbours")


@functools.lru_cache(maxsize=None)
def group_expected(kind, name, mistake=None):
    which, src, rows, dst_len = group_case(kind, name)
    return frozen(R.group_copy_ref(which, src, rows, dst_len, FCANARY, mistake))


TAIL_MOVE = (0, 1, 3, 4, 5, 8000, 8001, 8003)


@functools.lru_cache(maxsize=None)
def tail_move_case(ln):
    """k_tail_move: a source 16-byte aligned but not at its arena's start, the destination at the start of its own"""
    return 3, frozen(_samples(ln + 8, np.float32, ln)), frozen(np.array([(8, 0, ln, ln + PAD)], np.int64)), ln + PAD + 3


@functools.lru_cache(maxsize=None)
def tail_move_expected(ln, mistake=None):
    which, src, rows, dst_len = tail_move_case(ln)
    return frozen(R.group_copy_ref(which, src, rows, dst_len, FCANARY, mistake))


# ---------------------------------------------------------------- many.hip
PACK = ("mixed_f32", "mixed_pcm", "R1025_f32", "R1025_pcm")


@functools.lru_cache(maxsize=None)
def pack_case(name):
    """-> (src, rows [R][4] = (src_off or -1, n, base, len), dst_len)"""
    dtype = np.float32 if name.endswith("f32") else np.int16
    if name.startswith("mixed"):
        dst_len = 604000
        rows = [(0, 1000, 0, 1500),                      # samples, then zeros
                (1000, 777, 1501, 777),                  # n = len: no zeros; one canary in front of it
                (-1, 0, 2300, 512),                      # the product's own zero row: a null source
                (1777, 600000, 2900, 600100),            # past the cap of 2 048 blocks along a row
                (601777, 300, dst_len - 100, 400),       # base + len > dst_len: cut inside the samples
                (0, 5, dst_len + 7, 9)]                  # wholly behind the destination
        return frozen(_samples(602100, dtype, 1)), frozen(np.array(rows, np.int64)), dst_len
    rows, s, b = [], 0, 0
    for r in range(1025):                                # past the grid's cap of 1 024 table rows
        n = r % 7
        rows.append((s, n, b, n + r % 3))
        s, b = s + n, b + n + r % 3 + 1
    return frozen(_samples(s + 1, dtype, 2)), frozen(np.array(rows, np.int64)), b - 2


@functools.lru_cache(maxsize=None)
def pack_expected(name, mistake=None):
    src, rows, dst_len = pack_case(name)
    return frozen(R.many_pack_ref(src, rows, dst_len, FCANARY, mistake))


GAPS = {"edges": ([(0, 0), (3, 2), (5, 1), (10, 4), (20, 0), (38, 9), (50, 2)], 40),      # count 0, adjacent gaps, a gap reaching past total_chunks, one wholly behind
        "G1025": ([(2 * g, 1) for g in range(1025)], 2049)}


@functools.lru_cache(maxsize=None)
def gaps_expected(name, mistake=None):
    return frozen(R.gap_masks_ref(GAPS[name][0], GAPS[name][1], FCANARY, mistake))


# ---------------------------------------------------------------- the weight forms
SHAPES = {"k3_c8_80of96": (3, 8, 96, 80),       # the front layer's 80 channels in rows of 96; 1 920 elements: more than one block
          "k1_c5_7of32": (1, 5, 32, 7),         # 35 elements: not a multiple of 64, one partial wave
          "k2_c3_33of64": (2, 3, 64, 33),       # 198 elements: whole waves and a partial one, a second 32-channel chunk with one channel
          "k1_c40_64of64": (1, 40, 64, 64)}     # no pad channels
FILLS = ("mixed", "tiny", "huge", "zero")
WEIGHTS = ["%s_%s" % (s, f) for s in SHAPES for f in FILLS]


@functools.lru_cache(maxsize=None)
def weight_case(name):
    """-> (w [K][Cout][CinPad] float32 with NaN and 7.0 in the pad channels, cin).  Finite weights only."""
    shape, fill = name.rsplit("_", 1)
    K, Cout, CinPad, cin = SHAPES[shape]
    g = rng(K, Cout, cin, FILLS.index(fill))
    v = g.standard_normal((K, Cout, cin))
    if fill == "mixed":           # magnitudes down to 2^-17 of the largest and beyond: lo halves normal, subnormal and zero
        v = v * np.exp2(-22.0 * g.random((K, Cout, cin)))
        v[0, 0, 0] = 3.0
        v[0, 0, 1] = 3.0 * 2.0 ** -17
        v[0, 0, 2] = -3.0 * 2.0 ** -17 * (1 + 2.0 ** -10)
    elif fill == "tiny":
        v = v * 1e-30
    elif fill == "huge":
        v = v * 1e30
    else:                         # zeros of BOTH signs: a conversion that loses the sign of -0.0 shows here (k_w16x did)
        v = v * 0.0
    w = np.empty((K, Cout, CinPad), np.float32)
    w[:, :, :cin] = v
    w[:, :, cin:] = np.where(np.arange(CinPad - cin) % 2 == 0, np.nan, 7.0)
    return frozen(w), cin


@functools.lru_cache(maxsize=None)
def planes_expected(name, mistake=None):
    w, cin = weight_case(name)
    return frozen(R.w16_planes_ref(w, cin, HCANARY, mistake))


@functools.lru_cache(maxsize=None)
def split_expected(name, mistake=None):
    w, cin = weight_case(name)
    h, inv = R.w16x_ref(w, cin, HCANARY, mistake)
    return frozen(h), inv


# ---------------------------------------------------------------- which cases show which mistake (tests/test_input_ref.py)
FAMILIES = {
    "resample": (["11025_out257", "44100_out257", "8000_out257", "48000_out257", "16001_out257", "8000_n68"], lambda n, m=None: resample_expected(n, None, m)),
    "synthetic": (["random_table"], lambda n, m=None: synthetic_table_case(m)),
    "jobs": (list(JOBS), lambda n, m=None: jobs_expected(n, None, m)),
    "group": (["%s/%s" % (k, n) for k in KINDS for n in GROUP if n != "long"], lambda n, m=None: group_expected(*n.split("/"), mistake=m)),
    "tail_move": ([str(n) for n in TAIL_MOVE], lambda n, m=None: tail_move_expected(int(n), m)),
    "pack": (list(PACK), pack_expected),
    "gaps": (list(GAPS), gaps_expected),
    "planes": (WEIGHTS, planes_expected),
    "split": (WEIGHTS, lambda n, m=None: split_expected(n, m)[0]),
    "split_scale": (WEIGHTS, lambda n, m=None: np.array([split_expected(n, m)[1]])),
}
SHOWN_BY = {
    "first_tap_dropped": ["resample", "jobs"], "last_tap_dropped": ["synthetic"], "one_accumulator": ["resample", "jobs"],
    "rounded_product": ["resample", "jobs"], "phase_off_by_one": ["resample", "jobs"], "i0_rounded_up": ["resample", "jobs"],
    "n_limit_ignored": ["resample", "jobs"], "rs_pad_short": ["jobs"],
    "pad_short": ["group", "tail_move"], "room_ignored": ["group"], "src_cut": ["group"], "div_32767": ["group", "pack"],
    "len_unclamped": ["pack"], "gap_unclamped": ["gaps"],
    "truncated": ["planes", "split"], "residue_unscaled": ["split"], "pad_in_max": ["split", "split_scale"], "exponent_off_by_one": ["split", "split_scale"],
}
