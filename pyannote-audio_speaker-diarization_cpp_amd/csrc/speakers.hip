// speakers.hip -- known speakers (compiled with -ffp-contract=off): the kernels behind sd_span_masks, sd_voiceprint*, sd_speaker_distances and the
// enrolled gallery (sd_set_enrolled, sd_nearest_speakers, the enrolled branch of run_clustering)
//   k_span_masks       the mask rows of getEmbedding's items (sd.cpp:2436-2561) from time spans instead of from the segmentation scores
//   k_voiceprint_mean  the mean of the embeddings of the live windows, summed as assign_embeddings sums a centroid         sd.cpp:2149-2167
//   k_speaker_dist     cosine distance of every centroid to every row of a gallery, the reference's sequential sums        sd.cpp:476-498
//   k_row_sqnorms      m2 of every gallery row, once per gallery                                                           sd.cpp:476-498
//   k_nearest_gallery  nearest gallery row (first minimum) and its distance for every train row, no N x M table            sd.cpp:476-498, 293-316
// A voiceprint is computed exactly as the diarizer computes its own embeddings -- same chunks (sd.cpp:1419, 1457), same item grid, same batches of 32
// through run_embed -- with one difference: the mask of item 3c says "these samples of chunk c lie in a span" and items 3c + 1, 3c + 2 are empty, so the
// existing compaction drops them before any arithmetic.  That makes a voiceprint commensurable with the centroids run_clustering keeps (cluster.hip).
#include "common.h"
#include "exact_fp.h"
#include <algorithm>
#include <cmath>

// first sample of mask frame f of a chunk: frame_start of frontend.hip (samples j with j * 293 / 80000 == f start at ceil(80000 f / 293))
__device__ __forceinline__ int span_frame_start(int f) { return (int)(((int64_t)SD_CHUNK * f + (SD_FRAMES - 1)) / SD_FRAMES); }

// ---------------------------------------------------------------- k_span_masks : one thread per (chunk, mask frame)
// masks[3c][f] = 1.0 iff sample c * 8000 + frame_start(f) lies before n and inside one of the spans; rows 3c + 1 and 3c + 2 are zero.
// spans [ns][2] = [first, end) in samples, sorted, disjoint (spans_to_samples below): the last span that starts at or before the sample decides
__global__ void k_span_masks(const int64_t* __restrict__ spans, int ns, int64_t chunks, int64_t n, float* __restrict__ masks)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= chunks * SD_FRAMES) return;
    const int64_t ck = idx / SD_FRAMES;
    const int f = (int)(idx - ck * SD_FRAMES);
    const int64_t s = ck * SD_HOP + span_frame_start(f);
    bool on = false;
    if (s < n) {
        int lo = 0, hi = ns;                          // spans[0 .. lo) start at or before s
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (spans[2 * mid] <= s) lo = mid + 1; else hi = mid; }
        on = lo > 0 && s < spans[2 * (lo - 1) + 1];
    }
    float* row = masks + (size_t)ck * SD_SPEAKERS * SD_FRAMES + f;
    row[0] = on ? 1.0f : 0.0f;
    row[SD_FRAMES] = 0.0f;
    row[2 * SD_FRAMES] = 0.0f;
}

// ---------------------------------------------------------------- k_voiceprint_mean : one workgroup, one thread per dimension
// out[q] = mean over the chunks c, ascending, whose row 3c is not NaN (first element, sd.cpp:2224) of (double)emb[3c][q]: a sequential f64 sum divided
// by the number of such rows (k_cluster_means' rule); *n_live = that number, out = NaN when it is 0.  Eight rows in flight, added in chunk order
// (a dead row adds +0.0, which leaves a sum that started at +0.0 as it is).
__global__ __launch_bounds__(SD_EMB_DIM) void k_voiceprint_mean(const float* __restrict__ emb, int64_t chunks, double* __restrict__ out, int64_t* __restrict__ n_live)
{
    const int q = threadIdx.x;
    const size_t ld = (size_t)SD_SPEAKERS * SD_EMB_DIM;
    double s = 0.0;
    int64_t cnt = 0;
    int64_t ck = 0;
    for (; ck + 8 <= chunks; ck += 8) {
        float first[8], v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { first[u] = emb[(size_t)(ck + u) * ld]; v[u] = emb[(size_t)(ck + u) * ld + q]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const bool live = first[u] == first[u]; s += live ? (double)v[u] : 0.0; cnt += live ? 1 : 0; }
    }
    for (; ck < chunks; ++ck) {
        const float first = emb[(size_t)ck * ld], v = emb[(size_t)ck * ld + q];
        const bool live = first == first;
        s += live ? (double)v : 0.0; cnt += live ? 1 : 0;
    }
    out[q] = cnt > 0 ? s / (double)cnt : NAN;
    if (q == 0) *n_live = cnt;
}

// ---------------------------------------------------------------- k_speaker_dist : one workgroup per tile of SPK_TM gallery rows, one lane per row
// dist[k][m] = 1 - dot / (sqrt(m1) * sqrt(m2)) with dot, m1 (centroid k) and m2 (gallery row m) accumulated over i ascending, each its own sequential
// f64 sum (sd.cpp:476-498; the bits of k_assign and cos_dist_host of cluster.hip).  Laid out for a long gallery: the rows of the tile are staged through
// LDS in slices of SPK_TI dimensions -- 16 consecutive lanes fetch the 128 contiguous bytes of one row's slice, nobody strides a whole row per lane --
// and every lane then walks its own row's slice in ascending i (row pitch SPK_TI + 1 doubles: the 32 lanes of a ds_read_b64 group fall on 32 different
// bank pairs).  Centroids go in tiles of SPK_TK, their slices read from LDS by all lanes at once (a broadcast); any K works, the gallery tile is read
// again for every centroid tile.  A centroid whose first element is NaN (a cluster without a train row) is skipped: NaN distances, no error.  A zero
// norm of any other centroid or of any gallery row sets *err (the reference throws, sd.cpp:493-495).
// Bounds: gallery rows m0 + r < M and dimensions i0 + q < d are checked at the staging loads, k0 + k < K at the centroid loads and at the stores.
#define SPK_TM 128
#define SPK_TK 8
#define SPK_TI 16
#define SPK_LD (SPK_TI + 1)
__global__ __launch_bounds__(SPK_TM) void k_speaker_dist(const double* __restrict__ cen, int K, const double* __restrict__ gal, int64_t M, int d,
                                                         double* __restrict__ dist /*[K][M]*/, int* __restrict__ err)
{
    __shared__ double sg[SPK_TM * SPK_LD];
    __shared__ double sc[SPK_TK * SPK_TI];
    const int tid = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * SPK_TM, m = m0 + tid;
    for (int k0 = 0; k0 < K; k0 += SPK_TK) {
        const int kn = K - k0 < SPK_TK ? K - k0 : SPK_TK;
        double dot[SPK_TK], m1[SPK_TK], m2 = 0.0;
#pragma unroll
        for (int k = 0; k < SPK_TK; ++k) { dot[k] = 0.0; m1[k] = 0.0; }
        for (int i0 = 0; i0 < d; i0 += SPK_TI) {
            const int in = d - i0 < SPK_TI ? d - i0 : SPK_TI;
            __syncthreads();                                                  // everybody has read the previous slice
            for (int e = tid; e < SPK_TM * SPK_TI; e += SPK_TM) {
                const int r = e / SPK_TI, q = e % SPK_TI;
                sg[r * SPK_LD + q] = (m0 + r < M && q < in) ? gal[(size_t)(m0 + r) * d + i0 + q] : 0.0;
            }
            for (int e = tid; e < SPK_TK * SPK_TI; e += SPK_TM) {
                const int k = e / SPK_TI, q = e % SPK_TI;
                sc[e] = (k < kn && q < in) ? cen[(size_t)(k0 + k) * d + i0 + q] : 0.0;
            }
            __syncthreads();
            for (int q = 0; q < in; ++q) {                                    // i = i0 + q ascending: the order of the three sums is the reference's
                const double g = sg[tid * SPK_LD + q];
                m2 += g * g;
#pragma unroll
                for (int k = 0; k < SPK_TK; ++k) { const double cv = sc[k * SPK_TI + q]; dot[k] += cv * g; m1[k] += cv * cv; }
            }
        }
        if (m < M) {
            if (m2 == 0.0) *err = 1;
#pragma unroll
            for (int k = 0; k < SPK_TK; ++k) {
                if (k >= kn) continue;
                const double c0 = cen[(size_t)(k0 + k) * d];
                double v = NAN;
                if (c0 == c0) {
                    if (m1[k] == 0.0 || m2 == 0.0) *err = 1;
                    else v = 1.0 - (dot[k] / (sqrt(m1[k]) * sqrt(m2)));
                }
                dist[(size_t)(k0 + k) * M + m] = v;
            }
        }
    }
}


// ---------------------------------------------------------------- k_row_sqnorms : one thread per row
// m2[m] = sum over i ascending of V[m][i] * V[m][i]: the sequential sum every cosine distance of this file takes for its second operand (sd.cpp:476-498).
// The bits do not depend on what the row is paired with, so a gallery computes them once.
__global__ void k_row_sqnorms(const double* __restrict__ V, int64_t M, int d, double* __restrict__ m2)
{
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const double* r = V + (size_t)m * d;
    double s = 0.0;
    for (int i = 0; i < d; ++i) s += r[i] * r[i];
    m2[m] = s;
}

// ---------------------------------------------------------------- k_nearest_gallery : one workgroup per tile of NG_R train rows, one lane per row
// best[n] = the smallest m that attains min over m of dist(n, m), dist[n] = that minimum; dist(n, m) = 1 - dot / (sqrt(m1) * sqrt(m2)) of train row
// x = E[tidx[n]] (tidx == NULL: E[n]) and gallery row m: dot and m1 sequential f64 sums over i ascending, m2 from k_row_sqnorms -- the bits of
// k_speaker_dist for the same pair, k_speaker_dist with the roles of the two operands exchanged.  Nothing of size N x M exists: every lane keeps a running
// (min, arg-min).  The NG_R rows of the tile are staged once in LDS at an odd pitch (d | 1 doubles: the lanes of a ds_read_b64 group fall on different bank
// pairs; NG_R x 193 doubles = 99 KB for d = 192, above the 64 KB a launch gets without asking: run_nearest_gallery sets the kernel's dynamic-LDS
// attribute); rows longer than NG_DMAX stay in global memory and every lane walks its own.  The gallery streams through in tiles of NG_TK rows: wave w
// of the NG_WAVES waves takes the tiles t with t % NG_WAVES == w, its gallery addresses are the same in every lane (scalar loads, one broadcast operand per
// multiply), tiles and rows inside a tile in ascending m with a strict <.  The waves' results meet in LDS, combined in wave order by
// "smaller distance, or the same distance and a smaller m": whatever the split, the first minimum of the whole gallery wins.
// A zero-norm train row sets *err (the reference throws, sd.cpp:493-495); gallery rows are checked where the gallery is set (m2 > 0, finite).
// Bounds: train rows n0 + r < N at the staging loads, at the row pointer of the global form and at the stores; gallery rows m0 + k < M at the loads (a row
// past the end reads row M - 1 and its result is dropped) and at the compare.
#define NG_R 64
#define NG_TK 8
#define NG_WAVES 4
#define NG_DMAX 192
template <bool IN_LDS>
__device__ __forceinline__ void nearest_scan(const double* xr, double m1, const double* __restrict__ V, const double* __restrict__ gm2, int64_t M, int d,
                                             int wave, double& bd, int& bm)
{
    const double s1 = sqrt(m1);
    for (int64_t m0 = (int64_t)wave * NG_TK; m0 < M; m0 += (int64_t)NG_WAVES * NG_TK) {
        const double* vp[NG_TK];
        double dot[NG_TK];
#pragma unroll
        for (int k = 0; k < NG_TK; ++k) { const int64_t m = m0 + k < M ? m0 + k : M - 1; vp[k] = V + (size_t)m * d; dot[k] = 0.0; }
#pragma unroll 4
        for (int i = 0; i < d; ++i) {                                        // i ascending: the order of every dot sum is the reference's
            const double x = xr[i];
#pragma unroll
            for (int k = 0; k < NG_TK; ++k) dot[k] += x * vp[k][i];
        }
#pragma unroll
        for (int k = 0; k < NG_TK; ++k) {
            if (m0 + k >= M) continue;
            const double v = 1.0 - (dot[k] / (s1 * sqrt(gm2[m0 + k])));
            if (v < bd) { bd = v; bm = (int)(m0 + k); }
        }
    }
}
__global__ __launch_bounds__(NG_R * NG_WAVES) void k_nearest_gallery(const double* __restrict__ E, const int* __restrict__ tidx, int64_t N,
                                                                     const double* __restrict__ V, const double* __restrict__ gm2, int64_t M, int d,
                                                                     int* __restrict__ best, double* __restrict__ dist, int* __restrict__ err)
{
    extern __shared__ __attribute__((aligned(16))) double ng_x[];            // [NG_R][d | 1] when d <= NG_DMAX, else nothing
    __shared__ double wd[NG_WAVES][NG_R];
    __shared__ int wm[NG_WAVES][NG_R];
    const int tid = threadIdx.x, lane = tid & (NG_R - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / NG_R);             // the same in all 64 lanes: gallery addresses stay scalar
    const int64_t n0 = (int64_t)blockIdx.x * NG_R, n = n0 + lane;
    const bool in_lds = d <= NG_DMAX;
    const int pitch = d | 1;
    if (in_lds) {
        for (int e = tid; e < NG_R * d; e += NG_R * NG_WAVES) {
            const int r = e / d, q = e - r * d;
            double v = 0.0;
            if (n0 + r < N) { const int64_t row = tidx ? (int64_t)tidx[n0 + r] : n0 + r; v = E[(size_t)row * d + q]; }
            ng_x[r * pitch + q] = v;
        }
        __syncthreads();
    }
    const int64_t nr = n < N ? n : N - 1;                                    // a lane past the end walks the last row; nothing of it is stored
    const double* xg = E + (size_t)(tidx ? (int64_t)tidx[nr] : nr) * d;
    const double* xl = ng_x + lane * pitch;
    double m1 = 0.0;
    if (in_lds) for (int i = 0; i < d; ++i) m1 += xl[i] * xl[i];
    else        for (int i = 0; i < d; ++i) m1 += xg[i] * xg[i];
    double bd = INFINITY; int bm = -1;
    if (in_lds) nearest_scan<true>(xl, m1, V, gm2, M, d, wave, bd, bm);
    else        nearest_scan<false>(xg, m1, V, gm2, M, d, wave, bd, bm);
    wd[wave][lane] = bd; wm[wave][lane] = bm;
    __syncthreads();
    if (wave == 0 && n < N) {
#pragma unroll
        for (int w = 1; w < NG_WAVES; ++w) {
            const double v = wd[w][lane]; const int m = wm[w][lane];
            if (m >= 0 && (bm < 0 || v < bd || (v == bd && m < bm))) { bd = v; bm = m; }
        }
        if (m1 == 0.0) *err = 1;
        best[n] = bm < 0 ? 0 : bm;                                           // no distance compared smaller than +inf (NaN in the row): row 0, NaN
        dist[n] = bm < 0 ? NAN : bd;
    }
}
static std::atomic<unsigned> g_attr_ng{0};                                    // devices whose k_nearest_gallery has its dynamic-LDS attribute

// ---------------------------------------------------------------- host
// every span has 0 <= start <= end, both numbers (sd_voiceprint*'s SD_ERR_ARG rule); pure check, nothing of the context is touched before it passes
int check_spans(sd_ctx* c, const sd_turn* spans, int64_t n_spans, const char* who)
{
    if (n_spans < 0) SD_FAIL(c, SD_ERR_ARG, "%s: negative span count", who);
    if (!spans) return SD_OK;
    for (int64_t i = 0; i < n_spans; ++i) {
        const double a = spans[i].start, b = spans[i].end;
        if (!(a >= 0.0) || !(b >= a)) SD_FAIL(c, SD_ERR_ARG, "%s: span %lld is [%g, %g]: times must be numbers with 0 <= start <= end", who, (long long)i, a, b);
    }
    return SD_OK;
}

// spans with label `label` (all of them when label < 0; spans == NULL, or no span at all with label < 0: the whole recording) -> [first, end) in samples:
// llrint(t * 16000) clamped to [0, n], overlapping and touching spans merged, empty ones dropped; sorted
void spans_to_samples(const sd_turn* spans, int64_t n_spans, int32_t label, int64_t n, std::vector<int64_t>& out)
{
    out.clear();
    if (!spans || (n_spans == 0 && label < 0)) { out.push_back(0); out.push_back(n); return; }
    auto to_sample = [n](double t) { const double s = t * (double)SD_SAMPLE_RATE; if (s >= (double)n) return n; const int64_t v = (int64_t)llrint(s); return v < 0 ? (int64_t)0 : (v > n ? n : v); };
    std::vector<std::pair<int64_t, int64_t>> v;
    for (int64_t i = 0; i < n_spans; ++i) {
        if (label >= 0 && spans[i].label != label) continue;
        const int64_t a = to_sample(spans[i].start), b = to_sample(spans[i].end);
        if (b > a) v.emplace_back(a, b);
    }
    std::sort(v.begin(), v.end());
    for (const auto& s : v) {
        if (!out.empty() && s.first <= out.back()) { if (s.second > out.back()) out.back() = s.second; }
        else { out.push_back(s.first); out.push_back(s.second); }
    }
}

// d_masks [chunks * 3][293] of an n-sample recording from merged sample spans (spans_to_samples)
int run_span_masks(sd_ctx* c, const std::vector<int64_t>& spans, int64_t chunks, int64_t n, float* d_masks)
{
    if (chunks <= 0) return SD_OK;
    const int64_t ns = (int64_t)spans.size() / 2;
    if (ns > 0x3fffffff) SD_FAIL(c, SD_ERR_ARG, "too many spans (%lld)", (long long)ns);
    WS(c, int64_t, d_spans, "spk_spans", 2 * ns + 2);
    if (ns > 0) {
        HIPCHK(c, hipMemcpyAsync(d_spans, spans.data(), (size_t)(2 * ns) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));                           // the caller's vector may go
    }
    ProfScope ps(c, "span_masks", 0, (double)chunks * SD_SPEAKERS * SD_FRAMES * 4.0);
    hipLaunchKernelGGL(k_span_masks, GRID1(chunks * SD_FRAMES), 0, c->stream, d_spans, (int)ns, chunks, n, d_masks);
    KCHECK(c);
    return SD_OK;
}

// d_emb [chunks * 3][192] f32 -> h_mean [192], *n_live; synchronises the stream
int run_voiceprint_mean(sd_ctx* c, const float* d_emb, int64_t chunks, double* h_mean, int64_t* n_live)
{
    WS(c, double, d_out, "spk_mean", SD_EMB_DIM + 1);                         // [192] mean, then the count in the last 8 bytes
    int64_t* d_cnt = (int64_t*)(d_out + SD_EMB_DIM);
    {
        ProfScope ps(c, "voiceprint_mean", 0, (double)chunks * SD_EMB_DIM * 4.0);
        hipLaunchKernelGGL(k_voiceprint_mean, dim3(1), dim3(SD_EMB_DIM), 0, c->stream, d_emb, chunks, d_out, d_cnt);
        KCHECK(c);
    }
    double host[SD_EMB_DIM + 1];
    HIPCHK(c, hipMemcpyAsync(host, d_out, sizeof(host), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    memcpy(h_mean, host, SD_EMB_DIM * sizeof(double));
    memcpy(n_live, host + SD_EMB_DIM, sizeof(int64_t));
    return SD_OK;
}

// h_dist [K][M] = cosine distances of d_cen [K][d] to d_gal [M][d]; SD_ERR_NUMERIC on a zero-norm row; synchronises the stream
int run_speaker_dist(sd_ctx* c, const double* d_cen, int64_t K, const double* d_gal, int64_t M, int d, double* d_dist, double* h_dist)
{
    if (K <= 0 || M <= 0) return SD_OK;
    const int64_t tiles = (M + SPK_TM - 1) / SPK_TM;
    if (K > 0x7fffffff || tiles > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "speaker distances: %lld x %lld is out of range", (long long)K, (long long)M);
    WS(c, int, d_err, "spk_err", 4);
    HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), c->stream));
    {
        const double passes = (double)((K + SPK_TK - 1) / SPK_TK);
        ProfScope ps(c, "speaker_dist", 6.0 * (double)K * (double)M * d, passes * (double)M * d * 8.0 + (double)K * (double)M * 8.0);
        hipLaunchKernelGGL(k_speaker_dist, dim3((unsigned)tiles), dim3(SPK_TM), 0, c->stream, d_cen, (int)K, d_gal, M, d, d_dist, d_err);
        KCHECK(c);
    }
    int herr = 0;
    HIPCHK(c, hipMemcpyAsync(h_dist, d_dist, (size_t)K * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (herr) SD_FAIL(c, SD_ERR_NUMERIC, "zero-magnitude centroid or gallery row (reference throws, sd.cpp:493-495)");
    return SD_OK;
}

// d_m2 [M] = the squared norms of the gallery rows (k_row_sqnorms); asynchronous on the stream
int run_gallery_norms(sd_ctx* c, const double* d_gal, int64_t M, int d, double* d_m2)
{
    if (M <= 0) return SD_OK;
    ProfScope ps(c, "gallery_norms", 2.0 * (double)M * d, (double)M * d * 8.0);
    hipLaunchKernelGGL(k_row_sqnorms, GRID1(M), 0, c->stream, d_gal, M, d, d_m2);
    KCHECK(c);
    return SD_OK;
}

// d_best [N], d_dist [N] = nearest gallery row (first minimum) and its distance of the rows d_E[d_tidx[n]] (d_tidx == NULL: d_E[n]); d_m2 from
// run_gallery_norms.  Device memory beyond the operands: nothing but the error flag.  Synchronises the stream; SD_ERR_NUMERIC on a zero-norm train row
int run_nearest_gallery(sd_ctx* c, const double* d_E, const int* d_tidx, int64_t N, const double* d_gal, const double* d_m2, int64_t M, int d,
                        int* d_best, double* d_dist)
{
    if (N <= 0 || M <= 0) return SD_OK;
    const int64_t tiles = (N + NG_R - 1) / NG_R;
    if (tiles > 0x7fffffff || M > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "nearest speakers: %lld x %lld is out of range", (long long)N, (long long)M);
    const size_t lds = d <= NG_DMAX ? (size_t)NG_R * (size_t)(d | 1) * sizeof(double) : 0;
    if (!conv_set_dyn_lds(c, g_attr_ng, {(const void*)k_nearest_gallery}, (size_t)NG_R * (NG_DMAX | 1) * sizeof(double)))
        SD_FAIL(c, SD_ERR_HIP, "nearest speakers: the device refuses %zu bytes of LDS per workgroup", (size_t)NG_R * (NG_DMAX | 1) * sizeof(double));
    WS(c, int, d_err, "spk_err", 4);
    HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), c->stream));
    {
        ProfScope ps(c, "nearest_gallery", 2.0 * (double)N * (double)M * d, (double)tiles * (double)M * d * 8.0 + (double)N * d * 8.0);
        hipLaunchKernelGGL(k_nearest_gallery, dim3((unsigned)tiles), dim3(NG_R * NG_WAVES), lds, c->stream, d_E, d_tidx, N, d_gal, d_m2, M, d, d_best, d_dist, d_err);
        KCHECK(c);
    }
    int herr = 0;
    HIPCHK(c, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (herr) SD_FAIL(c, SD_ERR_NUMERIC, "zero-magnitude embedding against the gallery (reference throws, sd.cpp:493-495)");
    return SD_OK;
}
