// activity.hip -- speech / overlapped-speech regions from the segmentation scores alone (compiled with -ffp-contract=off):
//   the overlap-add of PipelineHelper::aggregate with skip_average = false, missing = 0.0      sd.cpp:1167-1311
//   (+ the Hamming-weighted branch the reference names and leaves as assert(false),              sd.cpp:1211-1215, 1259)
//   to_annotation + Track::support + Track::removeShort on the one-column timeline               sd.cpp:2852-2935, 911-953
// pyannote's VoiceActivityDetection / OverlappedSpeechDetection reduce the three local speakers of every chunk frame to one value
// (the largest = speech, the second largest = overlap; their pre_aggregation_hook) and hand the chunks to aggregate().  Here every
// output frame gathers the <= 11 chunks that cover it straight from the raw f32 scores, in ascending chunk order (the k_activations
// pattern of reconstruct.hip: deterministic, no atomics), and the hysteresis of to_annotation -- the first timeline of this library
// with onset != offset -- stays on the device as a scan:
//   every frame is a map on {inactive, active}: frame 0 the constant v > onset, every other frame inactive -> v > onset,
//   active -> !(v < offset); a NaN compares false both ways and is the identity.  Composing such maps is associative, so
//   k_activity_maps reduces each tile of ACT_TILE frames to its composite map (and its number of regions opened, for either entry
//   state), k_activity_scan scans the tiles in one wave, and k_activity_regions replays each tile from its entry state and writes the
//   (first frame, closing frame) index pair of region q into slot q -- the slot comes from the scanned counts, not from an atomic ticket.
// The host turns indices into timestamps and applies support / removeShort (a few hundred regions per hour of audio).
#include "common.h"
#include "exact_fp.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

static const double kFrameStep = 0.016875, kFrameDur = 0.016875;      // sd.cpp:2430-2431

#define ACT_TILE 1024                  // frames per tile = threads per workgroup of k_activity_maps / k_activity_regions
#define ACT_WAVES (ACT_TILE / 64)

// ---------------------------------------------------------------- k_activity_scores : one thread per output frame
// out[f] = sum_c w[j] r(c, j) / max(sum_c w[j], eps) over the chunks c that cover frame f with a frame j = f - sfr[c] whose three scores are
// numbers; r = largest (kind 0) or second largest (kind 1) of the three; w = 1, or the Hamming table; 0.0 (missing) where no chunk contributes
__global__ void k_activity_scores(const float* __restrict__ seg, const int* __restrict__ sfr, int64_t chunks, int kind,
                                  const double* __restrict__ hamming /* [293] or null */, double* __restrict__ out, int64_t nf)
{
    const int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    const double per_chunk = 0.5 / 0.016875;
    int64_t lo = (int64_t)((double)(f - (SD_FRAMES - 1)) / per_chunk) - 2; if (lo < 0) lo = 0;
    int64_t hi = (int64_t)((double)f / per_chunk) + 2; if (hi > chunks - 1) hi = chunks - 1;
    double sum = 0.0, cnt = 0.0;
    bool any = false;
    for (int64_t c = lo; c <= hi; ++c) {
        const int64_t j = f - sfr[c];
        if (j < 0 || j >= SD_FRAMES) continue;
        const float* s = seg + (c * SD_FRAMES + j) * SD_SPEAKERS;
        const float a = s[0], b = s[1], d = s[2];
        if (a != a || b != b || d != d) continue;                             // a NaN score: the reduced value is missing and masked out, sd.cpp:1197-1201
        const float mn = a < b ? a : b, mx = a < b ? b : a;
        const float r = kind == 0 ? (mx < d ? d : mx) : (mx < d ? mx : (mn < d ? d : mn));
        const double w = hamming ? hamming[j] : 1.0;
        sum += (double)r * w;                                                 // score * mask * hamming_window, sd.cpp:1259-1260
        cnt += w;                                                             // sd.cpp:1261
        any = true;
    }
    out[f] = any ? sum / (cnt < DBL_EPSILON ? DBL_EPSILON : cnt) : 0.0;       // sd.cpp:1288, 1302 (missing = 0.0)
}

// ---------------------------------------------------------------- the hysteresis maps
// a map on {inactive = 0, active = 1} in two bits: bit s = the state it sends state s to.  0 / 3 constants, 2 identity, 1 toggle
// (offset > onset and a score strictly between the two)
__device__ __forceinline__ unsigned frame_map(double v, bool first, double onset, double offset)
{
    const unsigned up = v > onset ? 1u : 0u;                                  // sd.cpp:2908 / the initial state, sd.cpp:2888
    const unsigned stay = v < offset ? 0u : 1u;                               // sd.cpp:2898
    return first ? up * 3u : (up | stay << 1);
}
__device__ __forceinline__ unsigned map_then(unsigned a, unsigned b)          // a first, then b
{
    return ((b >> (a & 1u)) & 1u) | (((b >> ((a >> 1) & 1u)) & 1u) << 1);
}
// the 64 maps of a wave as three ballots; the state after lane `lane` for entry state s needs no cross-lane traffic beyond them:
// the last constant map at or below the lane fixes the state, the toggles after it flip it
struct WaveMaps { unsigned long long cst, tog, val; };
__device__ __forceinline__ WaveMaps wave_maps(unsigned m)
{
    WaveMaps w;
    w.cst = __ballot(m == 0u || m == 3u);
    w.tog = __ballot(m == 1u);
    w.val = __ballot((m & 1u) != 0u);
    return w;
}
__device__ __forceinline__ unsigned state_after(const WaveMaps& w, int lane, unsigned s)
{
    unsigned long long span = (2ull << lane) - 1ull;                          // lanes 0 .. lane (lane 63: the shift leaves 0, minus 1 = all)
    const unsigned long long c = w.cst & span;
    if (c) {
        const int p = 63 - __clzll((long long)c);
        s = (unsigned)(w.val >> p) & 1u;
        span &= ~((2ull << p) - 1ull);                                        // lanes p + 1 .. lane
    }
    return s ^ ((unsigned)__popcll(w.tog & span) & 1u);
}
__device__ __forceinline__ unsigned state_before(const WaveMaps& w, int lane, unsigned s)
{
    return lane == 0 ? s : state_after(w, lane - 1, s);
}

// pass 1: tile -> its composite map and the regions it opens when entered inactive / active
__global__ void __launch_bounds__(ACT_TILE) k_activity_maps(const double* __restrict__ sc, int64_t rows, double onset, double offset,
                                                            uint8_t* __restrict__ tmap, int* __restrict__ ton /* [tiles][2] */)
{
    __shared__ unsigned wmap[ACT_WAVES];
    __shared__ int won[2][ACT_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * ACT_TILE + threadIdx.x;
    const unsigned m = i < rows ? frame_map(sc[i], i == 0, onset, offset) : 2u;
    const WaveMaps w = wave_maps(m);
    if (lane == 0) wmap[wv] = state_after(w, 63, 0u) | state_after(w, 63, 1u) << 1;
    __syncthreads();
#pragma unroll
    for (unsigned e = 0; e < 2; ++e) {
        unsigned we = e;
        for (int k = 0; k < wv; ++k) we = (wmap[k] >> we) & 1u;
        const unsigned prev = state_before(w, lane, we), cur = state_after(w, lane, we);
        const int n = __popcll(__ballot(prev == 0u && cur == 1u));
        if (lane == 0) won[e][wv] = n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = 2u; int n0 = 0, n1 = 0;
        for (int k = 0; k < ACT_WAVES; ++k) { t = map_then(t, wmap[k]); n0 += won[0][k]; n1 += won[1][k]; }
        tmap[blockIdx.x] = (uint8_t)t;
        ton[2 * blockIdx.x] = n0; ton[2 * blockIdx.x + 1] = n1;
    }
}

// the scan over the tiles, one wave: lane l owns the tiles [l per, (l + 1) per).  tentry[t] = state in which tile t is entered,
// tbase[t] = regions opened before tile t, summary = { regions in all, final state }
__global__ void __launch_bounds__(64) k_activity_scan(const uint8_t* __restrict__ tmap, const int* __restrict__ ton, int tiles,
                                                      uint8_t* __restrict__ tentry, int* __restrict__ tbase, int* __restrict__ summary)
{
    const int lane = threadIdx.x;
    const int per = (tiles + 63) / 64;
    const int t0 = lane * per < tiles ? lane * per : tiles;
    const int t1 = t0 + per < tiles ? t0 + per : tiles;
    unsigned m = 2u;
    for (int t = t0; t < t1; ++t) m = map_then(m, tmap[t]);
    const WaveMaps w = wave_maps(m);
    const unsigned s0 = state_before(w, lane, 0u);                            // nothing is active before frame 0
    unsigned s = s0;
    int cnt = 0;
    for (int t = t0; t < t1; ++t) { tentry[t] = (uint8_t)s; cnt += ton[2 * t + (int)s]; s = ((unsigned)tmap[t] >> s) & 1u; }
    int incl = cnt;
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    int run = incl - cnt;
    unsigned q = s0;
    for (int t = t0; t < t1; ++t) { tbase[t] = run; run += ton[2 * t + (int)q]; q = ((unsigned)tmap[t] >> q) & 1u; }
    if (lane == 63) { summary[0] = incl; summary[1] = (int)s; }               // (a lane without tiles carries the state of the lanes before it)
}

// pass 2: replay every tile from its entry state; the frame that opens region q writes pairs[q].x, the frame that closes it pairs[q].y.
// Regions closed before a tile = regions opened before it - its entry state.
__global__ void __launch_bounds__(ACT_TILE) k_activity_regions(const double* __restrict__ sc, int64_t rows, double onset, double offset,
                                                               const uint8_t* __restrict__ tentry, const int* __restrict__ tbase,
                                                               int2* __restrict__ pairs, int cap)
{
    __shared__ unsigned wmap[ACT_WAVES];
    __shared__ int won[ACT_WAVES], woff[ACT_WAVES];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * ACT_TILE + threadIdx.x;
    const unsigned m = i < rows ? frame_map(sc[i], i == 0, onset, offset) : 2u;
    const WaveMaps w = wave_maps(m);
    if (lane == 0) wmap[wv] = state_after(w, 63, 0u) | state_after(w, 63, 1u) << 1;
    __syncthreads();
    const unsigned entry = tentry[blockIdx.x];
    unsigned we = entry;
    for (int k = 0; k < wv; ++k) we = (wmap[k] >> we) & 1u;
    const unsigned prev = state_before(w, lane, we), cur = state_after(w, lane, we);
    const bool on = prev == 0u && cur == 1u, off = prev == 1u && cur == 0u;
    const unsigned long long on_mask = __ballot(on), off_mask = __ballot(off);
    if (lane == 0) { won[wv] = __popcll(on_mask); woff[wv] = __popcll(off_mask); }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    if (on) {
        int slot = tbase[blockIdx.x] + __popcll(on_mask & below);
        for (int k = 0; k < wv; ++k) slot += won[k];
        if (slot >= 0 && slot < cap) pairs[slot].x = (int)i;
    }
    if (off) {
        int slot = tbase[blockIdx.x] - (int)entry + __popcll(off_mask & below);
        for (int k = 0; k < wv; ++k) slot += woff[k];
        if (slot >= 0 && slot < cap) pairs[slot].y = (int)i;
    }
}

// ---------------------------------------------------------------- host
int64_t activity_frames_host(int64_t chunks)                                  // num_frames of aggregate(), sd.cpp:1232-1234
{
    if (chunks <= 0) return 0;
    return closest_frame_host(0.0, kFrameStep, kFrameDur, 0.0 + 5.0 + (double)(chunks - 1) * 0.5) + 1;
}
// frames that lie wholly in the zero padding of the last chunk are dropped
int64_t activity_rows_host(int64_t nf, int64_t n_samples)
{
    return std::min(nf, closest_frame_host(0.0, kFrameStep, kFrameDur, (double)n_samples / 16000.0) + 1);
}

int run_activity_scores(sd_ctx* c, const float* d_seg, int64_t chunks, int kind, double* d_scores, int64_t nf)
{
    if (chunks <= 0 || nf <= 0) return SD_OK;
    std::vector<int> sfr((size_t)chunks);
    double start = 0.0;
    for (int64_t i = 0; i < chunks; ++i) { sfr[(size_t)i] = (int)closest_frame_host(0.0, kFrameStep, kFrameDur, start); start += 0.5; }     // sd.cpp:1251-1253
    WS(c, int, d_sfr, "act_sfr", chunks);
    HIPCHK(c, hipMemcpyAsync(d_sfr, sfr.data(), (size_t)chunks * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const double* d_ham = nullptr;
    double ham[SD_FRAMES];
    if (c->activity_hamming) {
        for (int j = 0; j < SD_FRAMES; ++j) ham[j] = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)j / (double)(SD_FRAMES - 1));      // np.hamming(293), sd.cpp:1213
        WS(c, double, d_h, "act_hamming", SD_FRAMES);
        HIPCHK(c, hipMemcpyAsync(d_h, ham, sizeof(ham), hipMemcpyHostToDevice, c->stream));
        d_ham = d_h;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));                               // the host tables above may go
    ProfScope ps(c, "activity_scores", 0, (double)chunks * SD_FRAMES * 3 * 4.0 + (double)nf * 8.0);
    hipLaunchKernelGGL(k_activity_scores, GRID1(nf), 0, c->stream, d_seg, d_sfr, chunks, kind, d_ham, d_scores, nf);
    KCHECK(c);
    return SD_OK;
}

// d_scores [rows] -> turns (label = `label`) with the context's onset / offset / min_duration_on / min_duration_off
int run_activity_regions(sd_ctx* c, const double* d_scores, int64_t rows, int label, std::vector<sd_turn>& turns)
{
    turns.clear();
    if (rows <= 0) return SD_OK;
    if (rows > ((int64_t)1 << 30)) SD_FAIL(c, SD_ERR_ARG, "activity timeline of %lld frames: frame indices are 32-bit", (long long)rows);
    const int tiles = (int)((rows + ACT_TILE - 1) / ACT_TILE);
    const int cap = (int)(rows / 2 + 1);                                      // a region needs a frame to open and, but for the last one, a frame to close
    WS(c, uint8_t, d_tmap, "act_tmap", 2 * (size_t)tiles);
    WS(c, int, d_ton, "act_tcnt", 3 * (size_t)tiles + 2);
    WS(c, int2, d_pairs, "act_pairs", cap);
    uint8_t* d_tentry = d_tmap + tiles;
    int* d_tbase = d_ton + 2 * (size_t)tiles;
    int* d_summary = d_tbase + tiles;
    const double onset = c->activity_onset, offset = c->activity_offset;
    {
        ProfScope ps(c, "activity_maps", 0, (double)rows * 8.0);
        hipLaunchKernelGGL(k_activity_maps, dim3((unsigned)tiles), dim3(ACT_TILE), 0, c->stream, d_scores, rows, onset, offset, d_tmap, d_ton);
        KCHECK(c);
    }
    {
        ProfScope ps(c, "activity_scan", 0, (double)tiles * 18.0);
        hipLaunchKernelGGL(k_activity_scan, dim3(1), dim3(64), 0, c->stream, d_tmap, d_ton, tiles, d_tentry, d_tbase, d_summary);
        KCHECK(c);
    }
    {
        ProfScope ps(c, "activity_regions", 0, (double)rows * 8.0);
        hipLaunchKernelGGL(k_activity_regions, dim3((unsigned)tiles), dim3(ACT_TILE), 0, c->stream, d_scores, rows, onset, offset, d_tentry, d_tbase, d_pairs, cap);
        KCHECK(c);
    }
    int summary[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(summary, d_summary, sizeof(summary), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int nr = summary[0];
    if (nr < 0 || nr > cap) SD_FAIL(c, SD_ERR_HIP, "activity scan counted %d regions in %lld frames", nr, (long long)rows);
    if (nr == 0) return SD_OK;
    std::vector<int2> pairs((size_t)nr);
    HIPCHK(c, hipMemcpy(pairs.data(), d_pairs, (size_t)nr * sizeof(int2), hipMemcpyDeviceToHost));
    if (summary[1]) pairs[(size_t)nr - 1].y = (int)(rows - 1);                // still active at the end: closed at the last timestamp, sd.cpp:2916-2920
    auto ts = [](int i) { const double s = 0.0 + (double)i * kFrameStep, e = s + kFrameDur; return (s + e) / 2; };      // sd.cpp:2865-2867
    std::vector<sd_turn> segs((size_t)nr);
    for (int q = 0; q < nr; ++q) segs[(size_t)q] = {ts(pairs[(size_t)q].x), ts(pairs[(size_t)q].y), label, 0};
    const double min_off = c->activity_min_off, min_on = c->activity_min_on;
    if (min_off > 0.0) {                                                      // Track::support, sd.cpp:911-941 (the regions are in time order already)
        std::vector<sd_turn> merged;
        sd_turn cur = segs[0];
        for (size_t i = 1; i < segs.size(); ++i) {
            const sd_turn& nx = segs[i];
            double gap;
            if (cur.start < nx.start) gap = (cur.end >= nx.start) ? 0.0 : nx.start - cur.end;      // Segment::gap, sd.cpp:831-855
            else gap = (cur.start <= nx.end) ? 0.0 : cur.start - nx.end;
            if (gap < min_off) { cur.start = std::min(cur.start, nx.start); cur.end = std::max(cur.end, nx.end); }
            else { merged.push_back(cur); cur = nx; }
        }
        merged.push_back(cur);
        segs.swap(merged);
    }
    if (min_on > 0) {                                                         // Track::removeShort never looks at the first region, sd.cpp:943-953
        size_t w = 1;
        for (size_t i = 1; i < segs.size(); ++i) if (!((segs[i].end - segs[i].start) < min_on)) segs[w++] = segs[i];
        segs.resize(w);
    }
    std::sort(segs.begin(), segs.end(), [](const sd_turn& a, const sd_turn& b) { return a.start < b.start; });      // Annotation::finalResult, sd.cpp:973
    turns.swap(segs);
    return SD_OK;
}
