// cut.hip -- many cuts of one dendrogram (sdhip.h: sd_cut_*; compiled with -ffp-contract=off like cluster.hip and reconstruct.hip, whose bits it must give).
// A cut object holds everything of a finalize (pipeline.cpp) that does not depend on "clustering_threshold", "min_cluster_size" and "num_clusters":
// scores, count, f64 embeddings, the gathered train rows and the dendrogram.  sd_cut_turns_many then calls run_clustering's own finish of a cut
// (cluster_cut, cluster.hip) once per cut and runs the three stages that touch every embedding row or every frame ONCE for all cuts of a group:
//   k_assign_cuts        k_assign + k_mark_inactive: every row against the centroids of all cuts (one concatenated table), arg-max inside each cut's segment
//   k_activations_cuts   k_activations' activation_sum (recon_dev.h) for all cuts: act[t][f][k], K_t columns for cut t
//   k_topk_cuts          k_topk's topk_row (recon_dev.h) for all cuts
// followed by one copy of all binary matrices and reconstruct.hip's to_annotation_host per cut.
#include "common.h"
#include "exact_fp.h"
#include "cosine_rule.h"
#include "recon_dev.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

struct sd_cut {
    sd_ctx* c = nullptr;
    int64_t chunks = 0, n = 0, M = 0, N = 0, nf = 0;
    DevBuf seg, e64, X, Xn, nact, count, sfr;       // scores [chunks][293][3] f32, embeddings [M][192] f64, train rows [N][192] (as they are / normalised), active frames [M], count [nf], first frame [chunks]
    std::vector<int> tidx, h_nact;                  // the train rows (sd.cpp:2224), a host copy of nact (the inactive rule where a cut has no device assignment)
    std::vector<double> Z;                          // the linkage matrix [N - 1][4]
    ReconFrames g;
};

// the largest t in [0, n) with off[t] * scale <= x (off ascending, off[0] = 0)
__device__ inline int seg_of(const int* __restrict__ off, int n, int64_t scale, int64_t x)
{
    int lo = 0, hi = n - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if ((int64_t)off[mid] * scale <= x) lo = mid; else hi = mid - 1; }
    return lo;
}

// m2[j] of centroid j, the sequential sum of k_assign (sd.cpp:476-498): once per table instead of once per (row, centroid)
__global__ void k_cut_cen_norms(const double* __restrict__ cen, int K, int d, double* __restrict__ m2)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= K) return;
    const double* cc = cen + (size_t)j * d;
    double s = 0.0;
    for (int i = 0; i < d; ++i) s += cc[i] * cc[i];
    m2[j] = s;
}

// One wave per embedding row.  The centroids of the Tn cuts of a launch lie in one table, cut q in rows [coff[q], coff[q + 1]); the lanes spread over the
// rows of the table (k_assign's lanes spread over one cut's K: 60 of 64 idle at K = 4), then over the cuts, each lane scanning the segment of its cuts in
// ascending order.  As in k_assign: dot, m1, m2 three sequential sums over d, 2 - cosine_distance (cosine_rule.h), first maximum wins (strict >), a NaN
// row goes to cluster 0 with a NaN best score, a zero magnitude raises *err.  A table longer than the LDS tile is taken tile by tile; the one cut that
// spans a tile boundary is carried in the registers of the lane that owns it (cut q belongs to lane q % 64 in every tile).
// hard[slot[q]][row] = the arg-max inside cut q, or -2 where the row has no active frame (k_mark_inactive, sd.cpp:3172-3191); best[q][row] = its score.
#define CUT_TILE 1024
__global__ __launch_bounds__(64) void k_assign_cuts(const double* __restrict__ E, int64_t M, int d, const double* __restrict__ cen, const double* __restrict__ cen_m2,
                                                    const int* __restrict__ coff, const int* __restrict__ slot, int Tn, const int* __restrict__ nact,
                                                    int* __restrict__ hard, double* __restrict__ best_out, int* __restrict__ err)
{
    __shared__ double soft[CUT_TILE];
    const int64_t row = blockIdx.x;
    const int lane = threadIdx.x;
    const double* e = E + (size_t)row * d;
    double m1 = 0.0;
    for (int i = 0; i < d; ++i) m1 += e[i] * e[i];
    const bool inactive = nact[row] == 0;
    const int total = coff[Tn];
    int cbest = 0; double cmv = -DBL_MAX, csb = NAN;                 // the cut that spans the boundary behind the tile before
    for (int j0 = 0; j0 < total; j0 += CUT_TILE) {
        const int kn = total - j0 < CUT_TILE ? total - j0 : CUT_TILE;
        for (int j = lane; j < kn; j += 64) {
            const double* cc = cen + (size_t)(j0 + j) * d;
            double dot = 0.0;
            for (int i = 0; i < d; ++i) dot += e[i] * cc[i];
            const double m2 = cen_m2[j0 + j];
            bool zero = false;
            soft[j] = 2.0 - cosine_distance(dot, m1, m2, &zero);
            if (zero) *err = 1;
        }
        __syncthreads();
        const int q_lo = seg_of(coff, Tn, 1, j0), q_hi = seg_of(coff, Tn, 1, j0 + kn - 1);
        for (int q = q_lo + ((lane - q_lo) & 63); q <= q_hi; q += 64) {
            const int a = coff[q], b = coff[q + 1];
            const int s0 = a > j0 ? a : j0, s1 = b < j0 + kn ? b : j0 + kn;
            int best; double mv, sb;
            if (a >= j0) { best = 0; mv = -DBL_MAX; sb = soft[a - j0]; }      // best stays 0 when no score compares greater (NaN row -> cluster 0)
            else { best = cbest; mv = cmv; sb = csb; }
            for (int j = s0; j < s1; ++j) { const double v = soft[j - j0]; if (v > mv) { mv = v; best = j - a; sb = v; } }
            if (b <= j0 + kn) {
                hard[(size_t)slot[q] * M + row] = inactive ? -2 : best;
                best_out[(size_t)q * M + row] = sb;                  // NaN for rows without an embedding
            } else { cbest = best; cmv = mv; csb = sb; }
        }
        __syncthreads();
    }
}

// k_activations (reconstruct.hip) for the Tg cuts of a group: element e of act = (cut t, frame f, cluster k) with act[t] = [nact][K_t] at koff[t] * nact,
// K_t = koff[t + 1] - koff[t]; hard [Tg][chunks * 3]
__global__ void k_activations_cuts(const float* __restrict__ seg, const int* __restrict__ hard_all, const int* __restrict__ sfr, int64_t chunks,
                                   const int* __restrict__ koff, int Tg, double* __restrict__ act, int64_t nact)
{
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= nact * koff[Tg]) return;
    const int t = seg_of(koff, Tg, nact, idx);
    const int K = koff[t + 1] - koff[t];
    const int64_t r = idx - (int64_t)koff[t] * nact;
    const int64_t f = r / K;
    const int k = (int)(r - f * K);
    act[idx] = activation_sum(seg, hard_all + (size_t)t * chunks * SD_SPEAKERS, sfr, chunks, f, k);
}

// k_topk (reconstruct.hip) for the Tg cuts of a group: binary[t] = [rows][K_t] at koff[t] * rows
__global__ void k_topk_cuts(const double* __restrict__ act, const int32_t* __restrict__ count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow,
                            const int* __restrict__ koff, int Tg, int64_t nact, uint8_t* __restrict__ binary)
{
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= rows * Tg) return;
    const int t = (int)(id / rows);
    const int64_t i = id - (int64_t)t * rows;
    const int K = koff[t + 1] - koff[t];
    topk_row(act + (int64_t)koff[t] * nact + (ar0 + i) * K, binary + (int64_t)koff[t] * rows + i * K, K, i < crow ? count[cr0 + i] : 0);
}

// the launches of the four kernels (cut_group, the test hooks); asynchronous on c->stream
int launch_cut_cen_norms(sd_ctx* c, const double* d_cen, int total, int d, double* d_m2)
{
    hipLaunchKernelGGL(k_cut_cen_norms, GRID1(total), 0, c->stream, d_cen, total, d, d_m2);
    KCHECK(c);
    return SD_OK;
}
int launch_assign_cuts(sd_ctx* c, const double* E, int64_t M, int d, const double* d_cen, const double* d_m2, const int* d_coff, const int* d_slot, int Tn,
                       const int* d_nact, int* d_hard, double* d_best, int* d_err)
{
    hipLaunchKernelGGL(k_assign_cuts, dim3((unsigned)M), dim3(64), 0, c->stream, E, M, d, d_cen, d_m2, d_coff, d_slot, Tn, d_nact, d_hard, d_best, d_err);
    KCHECK(c);
    return SD_OK;
}
int launch_activations_cuts(sd_ctx* c, const float* d_seg, const int* d_hard, const int* d_sfr, int64_t chunks, const int* d_koff, int Tg, int64_t sumK,
                            double* d_act, int64_t nact)
{
    hipLaunchKernelGGL(k_activations_cuts, dim3((unsigned)((nact * sumK + 255) / 256)), dim3(256), 0, c->stream, d_seg, d_hard, d_sfr, chunks, d_koff, Tg, d_act, nact);
    KCHECK(c);
    return SD_OK;
}
int launch_topk_cuts(sd_ctx* c, const double* d_act, const int32_t* d_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow, const int* d_koff, int Tg,
                     int64_t nact, uint8_t* d_binary)
{
    hipLaunchKernelGGL(k_topk_cuts, dim3((unsigned)((rows * Tg + 255) / 256)), dim3(256), 0, c->stream, d_act, d_count, ar0, cr0, rows, crow, d_koff, Tg, nact, d_binary);
    KCHECK(c);
    return SD_OK;
}

// ---------------------------------------------------------------- open
int cut_refusal(sd_ctx* c, const char* who)
{
    if (c->enr_M > 0) SD_FAIL(c, SD_ERR_ARG, "%s: a gallery is enrolled: its flow clusters other rows than the dendrogram of a cut holds (clear the gallery)", who);
    if (!c->dump_dir.empty()) SD_FAIL(c, SD_ERR_ARG, "%s: a dump directory is set: the step files describe one finalize (clear it)", who);
    return SD_OK;
}

static void cut_free(sd_cut* k)
{
    for (DevBuf* b : {&k->seg, &k->e64, &k->X, &k->Xn, &k->nact, &k->count, &k->sfr}) b->release();
    delete k;
}

// everything of finalize / run_clustering in front of the cut of the dendrogram, into buffers of the cut's own
static int cut_fill(sd_ctx* c, sd_cut* k, const float* d_seg, const float* d_emb)
{
    const int d = SD_EMB_DIM;
    const int64_t chunks = k->chunks, M = k->M, nf = k->nf;
    const size_t seg_bytes = (size_t)chunks * SD_FRAMES * 3 * sizeof(float);
    if (k->seg.reserve(seg_bytes) || k->e64.reserve((size_t)M * d * sizeof(double)) || k->nact.reserve((size_t)M * sizeof(int)) ||
        k->count.reserve((size_t)nf * sizeof(int32_t)) || k->sfr.reserve((size_t)chunks * sizeof(int)))
        SD_FAIL(c, SD_ERR_HIP, "sd_cut_open: hipMalloc of the cut's buffers failed");
    HIPCHK(c, hipMemcpyAsync(k->seg.p, d_seg, seg_bytes, hipMemcpyDeviceToDevice, c->stream));
    WS(c, uint8_t, d_bin, "fin_bin", chunks * SD_FRAMES * 3);
    int rc;
    if ((rc = finalize_front(c, k->seg.as<float>(), d_emb, chunks, d_bin, k->nact.as<int>(), k->count.as<int32_t>(), nullptr, k->e64.as<double>()))) return rc;
    reconstruct_frames(chunks, nf, k->n, k->g);
    HIPCHK(c, hipMemcpyAsync(k->sfr.p, k->g.sfr.data(), (size_t)chunks * sizeof(int), hipMemcpyHostToDevice, c->stream));
    k->h_nact.resize((size_t)M);
    HIPCHK(c, hipMemcpyAsync(k->h_nact.data(), k->nact.p, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if ((rc = train_rows(c, k->e64.as<double>(), M, d, k->tidx))) return rc;      // a10; its synchronisation carries h_nact too
    k->N = (int64_t)k->tidx.size();
    if (k->N < 1) return SD_OK;
    // a10 - a12 through cluster.hip's own step: X, Xn and the dendrogram
    double* X = nullptr; double* Xn = nullptr;
    if ((rc = cluster_rows(c, k->e64.as<double>(), k->tidx, d, &X, &Xn, k->Z))) return rc;
    const size_t xb = (size_t)k->N * d * sizeof(double);
    if (k->X.reserve(xb) || k->Xn.reserve(xb)) SD_FAIL(c, SD_ERR_HIP, "sd_cut_open: hipMalloc of the cut's buffers failed");
    HIPCHK(c, hipMemcpyAsync(k->X.p, X, xb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(k->Xn.p, Xn, xb, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

int cut_open_dev(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, sd_cut** out)
{
    *out = nullptr;
    if (int rf = cut_refusal(c, "sd_cut_open")) return rf;
    sd_cut* k = new sd_cut();
    k->c = c; k->chunks = chunks; k->n = n; k->M = chunks * SD_SPEAKERS; k->nf = count_frames_host(chunks);
    const int rc = cut_fill(c, k, d_seg, d_emb);
    if (rc) { (void)hipStreamSynchronize(c->stream); cut_free(k); return rc; }
    c->cuts.push_back(k);
    *out = k;
    return SD_OK;
}

extern "C" int sd_cut_open_dev(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, sd_cut** cut)
{
    ENTER(c);
    if (!d_seg || !d_emb || !cut || chunks <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_cut_open_dev: bad argument");
    return cut_open_dev(c, d_seg, d_emb, chunks, n, cut);
}

extern "C" void sd_cut_close(sd_cut* k)
{
    if (!k) return;
    sd_ctx* c = k->c;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->cuts.erase(std::remove(c->cuts.begin(), c->cuts.end(), k), c->cuts.end());
    cut_free(k);
}

extern "C" int sd_cut_dendrogram(const sd_cut* k, double* h_Z, int64_t cap, int64_t* N)
{
    if (!k || cap < 0) return SD_ERR_ARG;
    if (N) *N = k->N;
    const int64_t rows = (int64_t)k->Z.size() / 4;
    if (h_Z) memcpy(h_Z, k->Z.data(), (size_t)std::min(rows, cap) * 4 * sizeof(double));
    return SD_OK;
}

extern "C" int sd_cut_info(const sd_cut* k, int64_t* chunks, int64_t* n_samples, int64_t* train_rows)
{
    if (!k) return SD_ERR_ARG;
    if (chunks) *chunks = k->chunks;
    if (n_samples) *n_samples = k->n;
    if (train_rows) *train_rows = k->N;
    return SD_OK;
}

// ---------------------------------------------------------------- evaluate
namespace {
struct CutJob {
    ClusterSpec spec;                                         // the three options, resolved, and the context's min_clusters / max_clusters
    ClusterPlan p;                                            // cluster_cut's: trivial (one cluster, no centroid table), else the nl final labels of the train rows
    std::vector<int> hard;                                    // [M] behind the inactive rule
    std::vector<double> best;                                 // [M]
    int Kr = 1;                                               // label columns of the reconstruction (sd.cpp:2803-2812)
    std::vector<sd_turn> turns;
};

// the cuts [g0, g1) of one group: assignment, activations, top-k and the copy back once for all of them, then the turns of each
int cut_group(sd_cut* k, std::vector<CutJob>& jobs, size_t g0, size_t g1, JobResult* last /* non-null: jobs[g1 - 1] is the last cut of the call; its centroid part is filled */)
{
    sd_ctx* c = k->c;
    const int d = SD_EMB_DIM;
    const int64_t M = k->M, chunks = k->chunks;
    const int Tg = (int)(g1 - g0);
    int rc;
    WS(c, int, d_hard, "cut_hard", (size_t)Tg * M);
    std::vector<int> nontriv;                                                        // positions in the group
    for (int t = 0; t < Tg; ++t) {
        CutJob& j = jobs[g0 + (size_t)t];
        j.hard.assign((size_t)M, 0); j.best.assign((size_t)M, NAN);
        if (!j.p.trivial) nontriv.push_back(t);
    }
    const bool constrained_assign = c->constrained_assignment && (M % SD_SPEAKERS) == 0;
    const double* X = k->X.as<double>();
    const double* e64 = k->e64.as<double>();
    if (!nontriv.empty() && !constrained_assign) {
        const int Tn = (int)nontriv.size();
        std::vector<int> coff((size_t)Tn + 1, 0);
        for (int q = 0; q < Tn; ++q) coff[(size_t)q + 1] = coff[(size_t)q] + jobs[g0 + (size_t)nontriv[(size_t)q]].p.nl;
        const int total = coff[(size_t)Tn];
        WS(c, double, d_cen, "cl_cen", (size_t)total * d);                           // the whole table first: final_means then fills it cut by cut without moving it
        for (int q = 0; q < Tn; ++q) {
            CutJob& j = jobs[g0 + (size_t)nontriv[(size_t)q]];
            double* cen = nullptr;
            if ((rc = final_means(c, X, d, j.p.lab, j.p.nl, coff[(size_t)q], j.p.order, j.p.off, &cen))) return rc;
            if (cen != d_cen) SD_FAIL(c, SD_ERR_HIP, "sd_cut_turns_many: the centroid table moved");
        }
        WS(c, double, d_m2, "cut_m2", total);
        WS(c, int, d_coff, "cut_coff", Tn + 1);
        WS(c, int, d_slot, "cut_slot", Tn);
        WS(c, double, d_best, "cut_best", (size_t)Tn * M);
        WS(c, int, d_err, "cl_err", 4);
        HIPCHK(c, hipMemcpyAsync(d_coff, coff.data(), (size_t)(Tn + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_slot, nontriv.data(), (size_t)Tn * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), c->stream));
        if ((rc = launch_cut_cen_norms(c, d_cen, total, d, d_m2))) return rc;
        {
            ProfScope ps(c, "assign_cuts", 2.0 * (double)M * total * d, (double)M * d * 8.0 + (double)total * d * 8.0);
            if ((rc = launch_assign_cuts(c, e64, M, d, d_cen, d_m2, d_coff, d_slot, Tn, k->nact.as<int>(), d_hard, d_best, d_err))) return rc;
        }
        int herr = 0;
        for (int q = 0; q < Tn; ++q) {
            CutJob& j = jobs[g0 + (size_t)nontriv[(size_t)q]];
            HIPCHK(c, hipMemcpyAsync(j.hard.data(), d_hard + (size_t)nontriv[(size_t)q] * M, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(j.best.data(), d_best + (size_t)q * M, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        if (last && !jobs[g1 - 1].p.trivial) {
            last->cen.resize((size_t)jobs[g1 - 1].p.nl * d);
            HIPCHK(c, hipMemcpyAsync(last->cen.data(), d_cen + (size_t)coff[(size_t)Tn - 1] * d, last->cen.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (herr) SD_FAIL(c, SD_ERR_NUMERIC, "zero-magnitude embedding or centroid in assignment (reference throws, sd.cpp:493-495)");
    }
    for (int t = 0; t < Tg; ++t) {
        CutJob& j = jobs[g0 + (size_t)t];
        if (!j.p.trivial && !constrained_assign) continue;
        if (!j.p.trivial) {                                                          // the constrained arg-max needs the whole score table: cut by cut through assign_all
            double* cen = nullptr;
            if ((rc = final_means(c, X, d, j.p.lab, j.p.nl, 0, j.p.order, j.p.off, &cen))) return rc;
            std::vector<int64_t> counts((size_t)j.p.nl);
            for (int q = 0; q < j.p.nl; ++q) counts[(size_t)q] = j.p.off[(size_t)q + 1] - j.p.off[(size_t)q];
            JobResult one;                                                           // the centroids of a cut that is not the call's last are not kept
            if ((rc = assign_all(c, e64, M, d, cen, j.p.nl, counts, j.hard, nullptr, &j.best, nullptr, (last && t == Tg - 1) ? *last : one))) return rc;
        }
        for (int64_t i = 0; i < M; ++i) if (k->h_nact[(size_t)i] == 0) j.hard[(size_t)i] = -2;      // sd.cpp:3172-3191
        HIPCHK(c, hipMemcpyAsync(d_hard + (size_t)t * M, j.hard.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    if (last) {
        CutJob& j = jobs[g1 - 1];
        if (j.p.trivial) {
            // one cluster, label 0: the mean of the train rows (a NaN row with count 0 when there is none), as run_clustering leaves it
            last->cen_counts.assign(1, k->N);
            if ((rc = mean_of_rows(c, e64, d, k->tidx, last->cen))) return rc;
        } else {
            last->cen_counts.resize((size_t)j.p.nl);
            for (int q = 0; q < j.p.nl; ++q) last->cen_counts[(size_t)q] = j.p.off[(size_t)q + 1] - j.p.off[(size_t)q];
        }
        last->cen_d = d;
        last->cen_K = (int)last->cen_counts.size();
    }
    // a15 - a17 for all cuts: column counts, activations, top-k, one copy back
    std::vector<int> koff((size_t)Tg + 1, 0);
    for (int t = 0; t < Tg; ++t) {
        CutJob& j = jobs[g0 + (size_t)t];
        int Kr = 0;
        for (int h : j.hard) if (h > Kr) Kr = h;
        j.Kr = Kr + 1;                                                               // sd.cpp:2803-2812
        koff[(size_t)t + 1] = koff[(size_t)t] + j.Kr;
        j.turns.clear();
    }
    const ReconFrames& g = k->g;
    const int64_t nact = g.nact, rows = g.rows, sumK = koff[(size_t)Tg];
    if (nact * sumK > 0x7fffffffLL * 256 || rows * (int64_t)Tg > 0x7fffffffLL * 256) SD_FAIL(c, SD_ERR_ARG, "sd_cut_turns_many: a group of %d cuts with %lld label columns is too large (lower cut_group_bytes)", Tg, (long long)sumK);
    WS(c, int, d_koff, "cut_koff", Tg + 1);
    WS(c, double, d_act, "cut_act", (size_t)nact * sumK);
    HIPCHK(c, hipMemcpyAsync(d_koff, koff.data(), (size_t)(Tg + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "activations_cuts", 0, (double)chunks * SD_FRAMES * 3 * 4.0 + (double)nact * sumK * 8.0);
        if ((rc = launch_activations_cuts(c, k->seg.as<float>(), d_hard, k->sfr.as<int>(), chunks, d_koff, Tg, sumK, d_act, nact))) return rc;
    }
    if (rows <= 0) { HIPCHK(c, hipStreamSynchronize(c->stream)); return SD_OK; }    // reference would index an empty vector here (sd.cpp:2735)
    int64_t crow = g.crow_all;
    if (crow > rows) crow = rows;                                                    // sd.cpp:2745
    WS(c, uint8_t, d_binary, "cut_binary", (size_t)rows * sumK);
    {
        ProfScope ps(c, "topk_cuts", 0, (double)rows * sumK * 9.0);
        if ((rc = launch_topk_cuts(c, d_act, k->count.as<int32_t>(), g.ar0, g.cr0, rows, crow, d_koff, Tg, nact, d_binary))) return rc;
    }
    std::vector<uint8_t> binary((size_t)rows * sumK);
    HIPCHK(c, hipMemcpyAsync(binary.data(), d_binary, binary.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<uint8_t> one;
    for (int t = 0; t < Tg; ++t) {
        CutJob& j = jobs[g0 + (size_t)t];
        one.assign(binary.begin() + (size_t)koff[(size_t)t] * rows, binary.begin() + (size_t)koff[(size_t)t + 1] * rows);
        to_annotation_host(one, rows, j.Kr, (double)g.astart, j.turns);
    }
    return SD_OK;
}

int cut_turns_many(sd_cut* k, const sd_cut_spec* specs, int64_t T, sd_turn** turns, int64_t* n_turns, int32_t* K)
{
    sd_ctx* c = k->c;
    if (int rf = cut_refusal(c, "sd_cut_turns_many")) return rf;
    if (!specs || T < 1 || T > 0x7fffffff || !turns || !n_turns) SD_FAIL(c, SD_ERR_ARG, "sd_cut_turns_many: bad argument (T >= 1)");
    std::vector<CutJob> jobs((size_t)T);
    for (int64_t t = 0; t < T; ++t) {
        const sd_cut_spec& s = specs[t];
        CutJob& j = jobs[(size_t)t];
        if (s.threshold != s.threshold) j.spec.threshold = c->clustering_threshold;
        else if (s.threshold >= 0.0 && s.threshold <= 2.0) j.spec.threshold = s.threshold;
        else SD_FAIL(c, SD_ERR_ARG, "sd_cut_turns_many: spec %lld: the threshold must lie in [0, 2] (NaN = the context's)", (long long)t);
        if (s.min_cluster_size < 0) SD_FAIL(c, SD_ERR_ARG, "sd_cut_turns_many: spec %lld: min_cluster_size must be at least 1 (0 = the context's)", (long long)t);
        j.spec.min_cluster_size = s.min_cluster_size == 0 ? c->min_cluster_size : s.min_cluster_size;
        if (s.num_clusters < -1) SD_FAIL(c, SD_ERR_ARG, "sd_cut_turns_many: spec %lld: num_clusters must be -1 (unset), 0 (the context's) or a count", (long long)t);
        j.spec.num_clusters = s.num_clusters == 0 ? c->num_clusters : s.num_clusters;
        j.spec.min_clusters = c->min_clusters; j.spec.max_clusters = c->max_clusters;
    }
    for (int64_t t = 0; t < T; ++t) { turns[t] = nullptr; n_turns[t] = 0; if (K) K[t] = 0; }
    int rc;
    for (CutJob& j : jobs) if ((rc = cluster_cut(c, k->Z, k->N, k->X.as<double>(), SD_EMB_DIM, j.spec, j.p, nullptr))) return rc;
    // groups: the longest runs of consecutive cuts whose activation tables [nact][nl] (nl bounds the label columns) fit the budget
    JobResult last;                                                                  // committed once, at the end: a call that fails leaves the context's record alone
    const double budget = (double)(c->cut_group_bytes > 0 ? c->cut_group_bytes : 1);
    for (size_t g0 = 0; g0 < jobs.size();) {
        size_t g1 = g0; double bytes = 0;
        while (g1 < jobs.size()) {
            const double b = (double)k->g.nact * jobs[g1].p.nl * sizeof(double);
            if (g1 > g0 && bytes + b > budget) break;
            bytes += b; ++g1;
        }
        if ((rc = cut_group(k, jobs, g0, g1, g1 == jobs.size() ? &last : nullptr))) return rc;
        g0 = g1;
    }
    // the context describes cut T - 1 as after that finalize (sd_last_speakers, sd_last_enrolled, sd_last_confidence)
    const CutJob& jl = jobs.back();
    c->stash.clustered = false;
    turn_confidence(jl.turns, jl.hard, jl.best, k->chunks, last.conf);
    c->last = std::move(last);                                                       // (enrolled stays empty: a cut refuses a gallery)
    for (int64_t t = 0; t < T; ++t) {
        if ((rc = turns_out(c, jobs[(size_t)t].turns, &turns[t], &n_turns[t]))) { for (int64_t q = 0; q < t; ++q) { free(turns[q]); turns[q] = nullptr; n_turns[q] = 0; } return rc; }
        if (K) K[t] = jobs[(size_t)t].Kr;
    }
    return SD_OK;
}
}

extern "C" int sd_cut_turns_many(sd_cut* k, const sd_cut_spec* specs, int64_t T, sd_turn** turns, int64_t* n_turns, int32_t* K)
{
    if (!k) return SD_ERR_ARG;
    ENTER(k->c);
    return cut_turns_many(k, specs, T, turns, n_turns, K);
}

extern "C" int sd_cut_turns(sd_cut* k, const sd_cut_spec* spec, sd_turn** turns, int64_t* n_turns, int32_t* K)
{
    return sd_cut_turns_many(k, spec, 1, turns, n_turns, K);
}
