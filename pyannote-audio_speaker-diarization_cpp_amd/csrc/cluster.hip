// cluster.hip -- the clustering stage around the linkage: which embeddings take part, the cut of the dendrogram, the assignment of every embedding
// (compiled with -ffp-contract=off: every fp64 result is bit-identical to the reference's x86 build, which decides speaker numbering).
//   a10 filter_embeddings                      sd.cpp:2214-2259
//   a11 Cluster::cluster (normalise, size split, small->large reassign, renumber)  sd.cpp:2300-2422
//   a13 Clustering::fcluster(criterion=distance)                                   cl.cpp:121-232, 442-457
//   a14 assign_embeddings (centroids, cosine cdist, argmax)                        sd.cpp:2119-2212
//   constrained arg-max and the hyper-parameter recut                              clustering/Clustering.py
// a12, Clustering::linkage, is run_linkage in linkage.hip.  fcluster is O(N) pointer chasing and runs on the host: it and the rest of the host arithmetic
// of a cut (number-of-clusters rules, re-cut, size split) are cluster_host.h; cluster_cut below is the one finish of a cut, for run_clustering and cut.hip.
#include "common.h"
#include "exact_fp.h"
#include "cosine_rule.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

// ---------------------------------------------------------------- row gather + L2 normalise (a10/a11)
// Xout[i] = X[tidx[i]] (un-normalised copy), Xn[i] = row / (double)(float)sqrt(sum x^2)
// Helper::L2Norm returns float (sd.cpp:332-340): the norm is rounded to f32 before the divide.
__global__ void k_gather_normalize(const double* __restrict__ X, const int* __restrict__ tidx, int64_t N, int d,
                                   double* __restrict__ Xout, double* __restrict__ Xn)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const double* r = X + (size_t)tidx[i] * d;
    double s = 0.0;
    for (int q = 0; q < d; ++q) s += r[q] * r[q];
    const double nrm = (double)(float)sqrt(s);
    for (int q = 0; q < d; ++q) {
        const double v = r[q];
        if (Xout) Xout[(size_t)i * d + q] = v;
        Xn[(size_t)i * d + q] = (nrm != 0.0) ? v / nrm : v;
    }
}

// the one launch of k_gather_normalize (cluster_rows, linkage_rows, the test hook): Xout may be null; asynchronous on c->stream
int launch_gather_normalize(sd_ctx* c, const double* d_emb, const int* d_tidx, int64_t N, int d, double* Xout, double* Xn)
{
    hipLaunchKernelGGL(k_gather_normalize, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, c->stream, d_emb, d_tidx, N, d, Xout, Xn);
    KCHECK(c);
    return SD_OK;
}

// a12 with its copy back: the linkage matrix of the N >= 2 rows of d_Xn on the host ([N - 1][4]); fewer rows: no linkage runs and Z is empty
int run_linkage_host(sd_ctx* c, const double* d_Xn, int64_t N, int d, int method, int metric, std::vector<double>& Z)
{
    Z.clear();
    if (N < 2) return SD_OK;
    WS(c, double, dZ, "cl_Z", (N - 1) * 4);
    int rc = run_linkage(c, d_Xn, N, d, dZ, method, metric);
    if (rc) return rc;
    Z.resize((size_t)(N - 1) * 4);
    HIPCHK(c, hipMemcpyAsync(Z.data(), dZ, Z.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

// ---------------------------------------------------------------- cluster means (sequential in member order)
// members of cluster k are order[off[k] .. off[k+1]) in ascending row index: same summation order as
// Helper::calculateClusterMeans (sd.cpp:442-473) and the centroid loop of assign_embeddings (sd.cpp:2149-2167)
__global__ void k_cluster_means(const double* __restrict__ X, int d, const int* __restrict__ order, const int* __restrict__ off,
                                double* __restrict__ cen)
{
    const int k = blockIdx.x;
    const int a = off[k], b = off[k + 1];
    for (int q = threadIdx.x; q < d; q += blockDim.x) {     // a block holds at most 1 024 threads: a thread walks q, q + blockDim.x, ..., each with a sum of its own
        double s = 0.0;
        int t = a;
        for (; t + 16 <= b; t += 16) {          // 16 rows in flight, added in member order (the sum itself stays sequential)
            double v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = X[(size_t)order[t + u] * d + q];
#pragma unroll
            for (int u = 0; u < 16; ++u) s += v[u];
        }
        for (; t < b; ++t) s += X[(size_t)order[t] * d + q];
        cen[(size_t)k * d + q] = s / (double)(b - a);
    }
}
// the one launch of k_cluster_means (reassign_small, final_means, mean_of_rows, the test hook): one block per cluster, one thread per element up to the
// 1 024 threads of a block; asynchronous on c->stream
int launch_cluster_means(sd_ctx* c, const double* X, int d, const int* d_order, const int* d_off, int nl, double* d_cen)
{
    const int threads = std::min(((d + 63) / 64) * 64, 1024);
    hipLaunchKernelGGL(k_cluster_means, dim3(nl), dim3(threads), 0, c->stream, X, d, d_order, d_off, d_cen);
    KCHECK(c);
    return SD_OK;
}

// cosine distance with the reference's sequential sums (sd.cpp:476-498; cosine_rule.h); soft = 2 - d; argmax first-max-wins
#define ASSIGN_TILE 1024
__global__ __launch_bounds__(64) void k_assign(const double* __restrict__ E, int64_t M, int d, const double* __restrict__ cen, int K,
                                               int* __restrict__ hard, int* __restrict__ err, double* __restrict__ soft_out /*[M][K] or null*/,
                                               double* __restrict__ best_out /*[M] or null*/)
{
    // arg-max over the K clusters in tiles of ASSIGN_TILE scores (any number of clusters fits the fixed LDS tile); first maximum wins,
    // as Helper::argmax does (sd.cpp:293-316): tiles in ascending k, strict > inside and across tiles
    __shared__ double soft[ASSIGN_TILE];
    const int64_t row = blockIdx.x;
    const double* e = E + (size_t)row * d;
    int best = 0; double mv = -DBL_MAX, sb = NAN; bool first = true;
    for (int k0 = 0; k0 < K; k0 += ASSIGN_TILE) {
        const int kn = K - k0 < ASSIGN_TILE ? K - k0 : ASSIGN_TILE;
        for (int k = threadIdx.x; k < kn; k += 64) {
            const double* cc = cen + (size_t)(k0 + k) * d;
            double dot = 0.0, m1 = 0.0, m2 = 0.0;
            for (int i = 0; i < d; ++i) { dot += e[i] * cc[i]; m1 += e[i] * e[i]; m2 += cc[i] * cc[i]; }
            bool zero = false;
            soft[k] = 2.0 - cosine_distance(dot, m1, m2, &zero);
            if (zero) *err = 1;
            if (soft_out) soft_out[(size_t)row * K + k0 + k] = soft[k];
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (first) { sb = soft[0]; first = false; }             // best stays 0 when no score compares greater (NaN row -> cluster 0)
            for (int k = 0; k < kn; ++k) if (soft[k] > mv) { mv = soft[k]; best = k0 + k; sb = soft[k]; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        hard[row] = best;
        if (best_out) best_out[row] = sb;                          // NaN for rows without an embedding
    }
}

// ---------------------------------------------------------------- constrained_argmax (clustering/Clustering.py:81-94)
// hard[c] = linear_sum_assignment(soft[c] (3 x K), maximize=True): every local speaker of a chunk goes to a DIFFERENT cluster.
// The Python delegates to scipy.optimize.linear_sum_assignment (third-party, unpinned by the reference); its published
// algorithm -- Crouse's shortest-augmenting-path rectangular LSAP as implemented in scipy's rectangular_lsap.cpp (1.6 and
// later): rows in order, `remaining` columns filled in reverse, ties towards an unassigned column, transpose when there are
// fewer clusters than speakers -- is restated here step by step, because rows without an embedding become CONSTANT rows
// (nan_to_num with the global minimum) and which optimal assignment comes out of the many equal ones is decided by exactly
// those details.  nr <= nc <= LSAP_MAXC after the optional transpose.
#define LSAP_MAXC 64
__host__ __device__ inline void lsap_solve(int nr, int nc, const double* cost /*[nr][nc], minimised*/, int* col4row)
{
    double u[SD_SPEAKERS] = {0, 0, 0}, v[LSAP_MAXC], spc[LSAP_MAXC];
    int path[LSAP_MAXC], row4col[LSAP_MAXC], remaining[LSAP_MAXC];
    bool SR[SD_SPEAKERS], SC[LSAP_MAXC];
    for (int j = 0; j < nc; ++j) { v[j] = 0.0; path[j] = -1; row4col[j] = -1; }
    for (int i = 0; i < nr; ++i) col4row[i] = -1;
    for (int cur = 0; cur < nr; ++cur) {
        double minVal = 0.0;
        int num_remaining = nc;
        for (int it = 0; it < nc; ++it) remaining[it] = nc - it - 1;
        for (int i = 0; i < nr; ++i) SR[i] = false;
        for (int j = 0; j < nc; ++j) { SC[j] = false; spc[j] = INFINITY; }
        int sink = -1, i = cur;
        while (sink == -1) {
            int index = -1; double lowest = INFINITY;
            SR[i] = true;
            for (int it = 0; it < num_remaining; ++it) {
                const int j = remaining[it];
                const double r = minVal + cost[i * nc + j] - u[i] - v[j];
                if (r < spc[j]) { path[j] = i; spc[j] = r; }
                if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) { lowest = spc[j]; index = it; }
            }
            minVal = lowest;
            if (index < 0) return;                              // infeasible (cannot happen with finite costs)
            const int j = remaining[index];
            if (row4col[j] == -1) sink = j; else i = row4col[j];
            SC[j] = true;
            remaining[index] = remaining[--num_remaining];
        }
        u[cur] += minVal;
        for (int r = 0; r < nr; ++r) if (SR[r] && r != cur) u[r] += minVal - spc[col4row[r]];
        for (int j = 0; j < nc; ++j) if (SC[j]) v[j] -= minVal - spc[j];
        int j = sink;
        while (true) {
            const int r = path[j];
            row4col[j] = r;
            const int t = col4row[r]; col4row[r] = j; j = t;
            if (r == cur) break;
        }
    }
}
__host__ __device__ inline void constrained_argmax_chunk(const double* soft /*[3][K]*/, int K, double fill, int* hard3)
{
    double cost[SD_SPEAKERS * LSAP_MAXC];
    int c4r[SD_SPEAKERS];
    hard3[0] = hard3[1] = hard3[2] = -2;
    if (K >= SD_SPEAKERS) {
        for (int s = 0; s < SD_SPEAKERS; ++s) for (int k = 0; k < K; ++k) { const double x = soft[s * K + k]; cost[s * K + k] = -((x != x) ? fill : x); }
        lsap_solve(SD_SPEAKERS, K, cost, c4r);
        for (int s = 0; s < SD_SPEAKERS; ++s) hard3[s] = c4r[s] >= 0 ? c4r[s] : -2;
    } else {                                                    // fewer clusters than speakers: scipy transposes
        for (int k = 0; k < K; ++k) for (int s = 0; s < SD_SPEAKERS; ++s) { const double x = soft[s * K + k]; cost[k * SD_SPEAKERS + s] = -((x != x) ? fill : x); }
        lsap_solve(K, SD_SPEAKERS, cost, c4r);
        for (int k = 0; k < K; ++k) if (c4r[k] >= 0) hard3[c4r[k]] = k;
    }
}
__global__ void k_constrained_argmax(const double* __restrict__ soft, int64_t chunks, int K, double fill, int* __restrict__ hard)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= chunks) return;
    int h[3];
    constrained_argmax_chunk(soft + (size_t)c * SD_SPEAKERS * K, K, fill, h);
    hard[c * 3] = h[0]; hard[c * 3 + 1] = h[1]; hard[c * 3 + 2] = h[2];
}

// the launches of k_assign and k_constrained_argmax (assign_all, the test hooks): one wave per row / one thread per chunk; asynchronous on c->stream
int launch_assign(sd_ctx* c, const double* E, int64_t M, int d, const double* cen, int K, int* hard, int* err, double* soft, double* best)
{
    hipLaunchKernelGGL(k_assign, dim3((unsigned)M), dim3(64), 0, c->stream, E, M, d, cen, K, hard, err, soft, best);
    KCHECK(c);
    return SD_OK;
}
int launch_constrained_argmax(sd_ctx* c, const double* soft, int64_t chunks, int K, double fill, int* hard)
{
    hipLaunchKernelGGL(k_constrained_argmax, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, c->stream, soft, chunks, K, fill, hard);
    KCHECK(c);
    return SD_OK;
}

static double cos_dist_host(const double* a, const double* b, int d, bool* err)      // sd.cpp:476-498
{
    double dot = 0.0, m1 = 0.0, m2 = 0.0;
    for (int i = 0; i < d; ++i) { dot += a[i] * b[i]; m1 += a[i] * a[i]; m2 += b[i] * b[i]; }
    return cosine_distance(dot, m1, m2, err);
}

// ---------------------------------------------------------------- the steps of run_clustering: the plain flow and the enrolled flow call the same ones
// a10 / a11 / a12: rows idx[0 .. N) of d_emb gathered (X) and normalised with the f32 norm (Xn), then the dendrogram of them (Z on the host; empty for N < 2).
// The method is one of the three hyper-parameters of Clustering.py:251-276; its default is the constant the reference hard-codes (sd.cpp:2049-2056: centroid).
// Clustering.py:317-333: centroid, median and ward are euclidean-only and run on the unit-normalised rows (Xn, with the port's f32 norm); the other four run
// on the rows as they are with the cosine metric.  Threshold and minimum cluster size act behind this step: cluster_cut, or the enrolled flow's own steps.
int cluster_rows(sd_ctx* c, const double* d_emb, const std::vector<int>& idx, int d, double** Xout, double** Xnout, std::vector<double>& Z)
{
    const int64_t N = (int64_t)idx.size();
    WS(c, int, d_tidx, "cl_tidx", N);
    WS(c, double, X, "cl_X", N * d);
    WS(c, double, Xn, "cl_Xn", N * d);
    HIPCHK(c, hipMemcpyAsync(d_tidx, idx.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_gather_normalize(c, d_emb, d_tidx, N, d, X, Xn)) return rc;
    const int method = c->clustering_method;
    const int metric = linkage_metric_of(method);
    *Xout = X; *Xnout = Xn;
    // a group call ran the dendrogram of these rows ahead of the job (finalize_jobs, many.hip: the same kernels on the same train rows); it is taken once
    if (c->ahead_N == N && N >= 2) { Z.swap(c->ahead_Z); c->ahead_N = -1; return SD_OK; }
    return run_linkage_host(c, metric == SD_METRIC_EUCLIDEAN ? Xn : X, N, d, method, metric, Z);
}

// The rows cluster_rows hands to the linkage for the train rows idx of d_emb, into out [N][d] on the device (asynchronous): the same kernel, so the same bits
int linkage_rows(sd_ctx* c, const double* d_emb, const std::vector<int>& idx, int d, double* out)
{
    const int64_t N = (int64_t)idx.size();
    if (N < 1) return SD_OK;
    WS(c, int, d_tidx, "cl_tidx", N);
    HIPCHK(c, hipMemcpyAsync(d_tidx, idx.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (linkage_metric_of((int)c->clustering_method) == SD_METRIC_EUCLIDEAN) return launch_gather_normalize(c, d_emb, d_tidx, N, d, nullptr, out);
    WS(c, double, Xn, "cl_Xn", N * d);
    return launch_gather_normalize(c, d_emb, d_tidx, N, d, out, Xn);
}

// a11: every small cluster goes to the nearest candidate -- first the G rows of `enrolled` (host, [G][d]; the enrolled flow), then the large clusters in
// ascending id -- by the cosine distance of the means of the UN-normalised rows (sd.cpp:2386), the reference's float minVal loop (sd.cpp:2396).  The rows of a
// cluster that goes to an enrolled candidate get label -1; the labels that survive are renumbered 0 .. nl - 1 in sorted-id order (findUniqueClusters,
// sd.cpp:519-548).
static int reassign_small(sd_ctx* c, const double* X, int d, const std::vector<int>& order, const std::vector<int>& off, const std::vector<int>& large,
                          const std::vector<int>& small, const double* enrolled, int G, std::vector<int>& lab, int& nl)
{
    const size_t N = order.size();
    WS(c, int, d_order, "cl_order", N);
    WS(c, int, d_off, "cl_off", nl + 1);
    WS(c, double, d_cen, "cl_cen", (size_t)nl * d);
    HIPCHK(c, hipMemcpyAsync(d_order, order.data(), N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, off.data(), (size_t)(nl + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_cluster_means(c, X, d, d_order, d_off, nl, d_cen)) return rc;   // means of UN-normalised rows (sd.cpp:2386)
    std::vector<double> cen((size_t)nl * d);
    HIPCHK(c, hipMemcpyAsync(cen.data(), d_cen, cen.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    bool err = false;
    std::vector<int> remap((size_t)nl);
    for (int k = 0; k < nl; ++k) remap[(size_t)k] = k;
    for (int sk : small) {
        float minVal = FLT_MAX; int best = -1;                                      // float accumulator, sd.cpp:2396
        for (size_t a = 0; a < (size_t)G + large.size(); ++a) {
            const double* cand = a < (size_t)G ? enrolled + a * (size_t)d : &cen[(size_t)large[a - (size_t)G] * d];
            const double dd = cos_dist_host(cand, &cen[(size_t)sk * d], d, &err);
            if (dd < minVal) { minVal = (float)dd; best = (int)a; }
        }
        if (best >= 0) remap[(size_t)sk] = best < G ? -1 : large[(size_t)(best - G)];
    }
    if (err) SD_FAIL(c, SD_ERR_NUMERIC, "zero-magnitude cluster centroid (reference throws, sd.cpp:493-495)");
    for (auto& v : lab) v = remap[(size_t)v];
    // findUniqueClusters: renumber 0..K-1 in sorted-id order (sd.cpp:519-548)
    std::vector<int> seen((size_t)nl, -1);
    for (int v : lab) if (v >= 0) seen[(size_t)v] = 0;
    int nk = 0;
    for (int k = 0; k < nl; ++k) if (seen[(size_t)k] == 0) seen[(size_t)k] = nk++;
    for (auto& v : lab) if (v >= 0) v = seen[(size_t)v];
    nl = nk;
    return SD_OK;
}

// One cut of the dendrogram Z of the N train rows X (cluster_rows): cluster_plan (cluster_host.h), then the all-small rule or the small -> large pass.  p.lab /
// p.nl are final afterwards (p.order / p.off: the membership before the pass); p.trivial: one cluster, nothing was read.  first_cut: see cluster_plan.
int cluster_cut(sd_ctx* c, const std::vector<double>& Z, int64_t N, const double* X, int d, const ClusterSpec& spec, ClusterPlan& p, std::vector<int>* first_cut)
{
    cluster_plan(Z, N, spec, p, first_cut);
    if (p.trivial) return SD_OK;
    if (p.large.empty()) {
        // reference: assert(false) in assert-enabled builds (sd.cpp:2368), all-zero labels otherwise (sd.cpp:2371-2375)
        std::fill(p.lab.begin(), p.lab.end(), 0);
        p.nl = 1;
    } else if (!p.small.empty()) return reassign_small(c, X, d, p.order, p.off, p.large, p.small, nullptr, 0, p.lab, p.nl);
    return SD_OK;
}

// a14, first half: the means of the nl final clusters (un-normalised rows of X, members in ascending row order) into rows [G, G + nl) of the centroid table
// "cl_cen"; rows [0, G) are left to the caller (the enrolled flow's voiceprints).  order / off describe the membership afterwards.
int final_means(sd_ctx* c, const double* X, int d, const std::vector<int>& lab, int nl, int G, std::vector<int>& order, std::vector<int>& off, double** cen_out)
{
    group_by_label(lab, nl, order, off);
    WS(c, int, d_order2, "cl_order", std::max<size_t>(order.size(), 1));      // (no new cluster at all: the enrolled flow with every row claimed)
    WS(c, int, d_off2, "cl_off", nl + 1);
    WS(c, double, d_cen2, "cl_cen", (size_t)(G + nl) * d);
    HIPCHK(c, hipMemcpyAsync(d_order2, order.data(), order.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off2, off.data(), (size_t)(nl + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if (nl > 0)
        if (int rc = launch_cluster_means(c, X, d, d_order2, d_off2, nl, d_cen2 + (size_t)G * d)) return rc;
    *cen_out = d_cen2;
    return SD_OK;
}

// a14, second half: cosine cdist of ALL M rows to the K centroids, arg-max (or the constrained arg-max); the centroids and their counts become the centroid
// part of `res` (what sd_last_speakers describes once the caller commits it), cen_K last: 0 stays 0 where this fails.  *soft_out (may be NULL) = the [M][K]
// score table where one was written, else null.
int assign_all(sd_ctx* c, const double* d_emb, int64_t M, int d, const double* d_cen2, int K, const std::vector<int64_t>& counts,
                      std::vector<int>& hard, int* Kout, std::vector<double>* soft_best, double** soft_out, JobResult& res)
{
    const bool dumping = !c->dump_dir.empty();
    WS(c, int, d_hard, "cl_hard", M);
    WS(c, int, d_err, "cl_err", 4);
    HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), c->stream));
    const bool constrained_assign = c->constrained_assignment && (M % SD_SPEAKERS) == 0;
    // the full [M][K] score table only for the constrained assignment (it needs every score); the confidence needs the best score alone
    double* d_soft = nullptr; double* d_best = nullptr;
    if (constrained_assign || dumping) { WS(c, double, t_soft, "cl_soft", (size_t)M * K); d_soft = t_soft; }
    if (constrained_assign || soft_best) { WS(c, double, t_best, "cl_best", M); d_best = t_best; }
    if (int rc = launch_assign(c, d_emb, M, d, d_cen2, K, d_hard, d_err, d_soft, d_best)) return rc;
    int herr = 0;
    HIPCHK(c, hipMemcpyAsync(hard.data(), d_hard, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (soft_best) HIPCHK(c, hipMemcpyAsync(soft_best->data(), d_best, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    res.cen.resize((size_t)K * d);                                  // the centroids ride this synchronisation (sd_last_speakers)
    HIPCHK(c, hipMemcpyAsync(res.cen.data(), d_cen2, res.cen.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (herr) SD_FAIL(c, SD_ERR_NUMERIC, "zero-magnitude embedding or centroid in assignment (reference throws, sd.cpp:493-495)");
    if (constrained_assign) {
        // Clustering.py:83: NaN (rows without an embedding) -> the smallest soft score of the whole recording
        std::vector<double> hs((size_t)M * K);
        HIPCHK(c, hipMemcpy(hs.data(), d_soft, hs.size() * sizeof(double), hipMemcpyDeviceToHost));
        double fill = INFINITY;
        for (double x : hs) if (x == x && x < fill) fill = x;
        if (fill == INFINITY) fill = 0.0;
        const int64_t chunks = M / SD_SPEAKERS;
        if (K <= LSAP_MAXC) {
            if (int rc = launch_constrained_argmax(c, d_soft, chunks, K, fill, d_hard)) return rc;
            HIPCHK(c, hipMemcpyAsync(hard.data(), d_hard, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        } else SD_FAIL(c, SD_ERR_ARG, "constrained assignment supports up to %d clusters (found %d)", LSAP_MAXC, K);
        if (soft_best)                                             // confidence follows the cluster actually assigned
            for (int64_t i = 0; i < M; ++i) (*soft_best)[(size_t)i] = hard[(size_t)i] >= 0 ? hs[(size_t)i * K + hard[(size_t)i]] : NAN;
    }
    if (Kout) *Kout = K;
    res.cen_counts = counts;
    res.cen_d = d;
    res.cen_K = K;
    if (soft_out) *soft_out = d_soft;
    return SD_OK;
}

// the refusals of a call that clusters under an enrolled gallery (sdhip.h); nothing is touched
int enrolled_refusal(sd_ctx* c, int d, int num_clusters, int min_clusters, int max_clusters)
{
    if (c->enr_M <= 0) return SD_OK;
    if (num_clusters != -1 || min_clusters != -1 || max_clusters != -1)
        SD_FAIL(c, SD_ERR_ARG, "a gallery is enrolled: num_clusters / min_clusters / max_clusters have no meaning next to enrolled speakers (clear one of the two)");
    if (!c->dump_dir.empty()) SD_FAIL(c, SD_ERR_ARG, "a gallery is enrolled: the step files describe the reference's flow (clear the gallery or the dump directory)");
    if (d != c->enr_d) SD_FAIL(c, SD_ERR_ARG, "the enrolled gallery has rows of %d dimensions, this call clusters rows of %d", c->enr_d, d);
    return SD_OK;
}

// The enrolled flow (sdhip.h, "enrolled speakers", steps 1 - 9).  tidx = the N >= 1 train rows.  *taken = false: no row was claimed (G = 0), nothing of the
// context's results has been written and the caller goes on with the plain flow.
// Steps 5 - 7 call the steps of a cut themselves instead of cluster_cut, because three rules differ from the plain flow: there is no trivial exit (one
// unclaimed row is a cluster of its own next to the candidates), there is no all-small rule while a candidate is enrolled (small clusters can always go to
// a candidate), and the minimum cluster size comes from N, all train rows, not from N', the unclaimed ones.
static int clustering_enrolled(sd_ctx* c, const double* d_emb, int64_t M, int d, const std::vector<int>& tidx, std::vector<int>& hard, int* Kout,
                               std::vector<double>* soft_best, bool* taken)
{
    *taken = false;
    const int64_t N = (int64_t)tidx.size();
    // 1 nearest
    WS(c, int, d_tidx, "ng_tidx", N);
    WS(c, int, d_best, "ng_best", N);
    WS(c, double, d_dist, "ng_dist", N);
    HIPCHK(c, hipMemcpyAsync(d_tidx, tidx.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    int rc = run_nearest_gallery(c, d_emb, d_tidx, N, c->enr_gal.as<double>(), c->enr_m2.as<double>(), c->enr_M, d, d_best, d_dist);
    if (rc) return rc;
    std::vector<int> g((size_t)N);
    std::vector<double> gd((size_t)N);
    HIPCHK(c, hipMemcpy(g.data(), d_best, (size_t)N * sizeof(int), hipMemcpyDeviceToHost));
    HIPCHK(c, hipMemcpy(gd.data(), d_dist, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    // 2 claim, 3 used speakers
    const double t = c->speaker_match_threshold;
    std::vector<int> U;
    for (int64_t i = 0; i < N; ++i) if (gd[(size_t)i] <= t) U.push_back(g[(size_t)i]);
    std::sort(U.begin(), U.end());
    U.erase(std::unique(U.begin(), U.end()), U.end());
    const int G = (int)U.size();
    if (G == 0) return SD_OK;
    *taken = true;
    std::vector<int64_t> counts((size_t)G, 0);
    std::vector<int> ridx;                                                   // 4: R, the unclaimed train rows (row numbers of d_emb)
    for (int64_t i = 0; i < N; ++i) {
        if (gd[(size_t)i] <= t) counts[(size_t)(std::lower_bound(U.begin(), U.end(), g[(size_t)i]) - U.begin())]++;
        else ridx.push_back(tidx[(size_t)i]);
    }
    const size_t mcs = resolve_min_cluster_size(c->min_cluster_size, N);     // from N, not N'
    std::vector<double> cand((size_t)G * d);
    for (int a = 0; a < G; ++a) memcpy(&cand[(size_t)a * d], &c->enr_host[(size_t)U[(size_t)a] * d], (size_t)d * sizeof(double));
    // 5 - 7: the new clusters of R
    std::vector<int> lab, order, off;
    int L = 0;
    double* X = nullptr; double* Xn = nullptr;
    if (!ridx.empty()) {
        std::vector<double> Z;
        if ((rc = cluster_rows(c, d_emb, ridx, d, &X, &Xn, Z))) return rc;
        fcluster_host(Z, (int64_t)ridx.size(), c->clustering_threshold, lab);
        for (auto& v : lab) { v -= 1; if (v + 1 > L) L = v + 1; }
        group_by_label(lab, L, order, off);
        std::vector<int> large, small;
        split_by_size(off, L, mcs, large, small);
        if (!small.empty() && (rc = reassign_small(c, X, d, order, off, large, small, cand.data(), G, lab, L))) return rc;
    }
    double* d_cen2 = nullptr;
    if ((rc = final_means(c, X, d, lab, L, G, order, off, &d_cen2))) return rc;
    // 8: the table [V[U[0]] .. V[U[G-1]], mean_0 .. mean_{L-1}]
    HIPCHK(c, hipMemcpyAsync(d_cen2, cand.data(), cand.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < L; ++k) counts.push_back(off[(size_t)k + 1] - off[(size_t)k]);
    if ((rc = assign_all(c, d_emb, M, d, d_cen2, G + L, counts, hard, Kout, soft_best, nullptr, c->last))) return rc;
    c->last.enrolled.assign((size_t)(G + L), -1);                           // 9
    for (int a = 0; a < G; ++a) c->last.enrolled[(size_t)a] = U[(size_t)a];
    return SD_OK;
}

// a10: the rows of d_emb [M][d] whose first element is not NaN (sd.cpp:2224), ascending; synchronises the stream.  Under "max_num_embeddings" the
// sample of them (cluster_host.h: sample_rows) -- from here on the sample IS the train rows, as in Clustering.py:69-76
int train_rows(sd_ctx* c, const double* d_e64, int64_t M, int d, std::vector<int>& tidx)
{
    std::vector<double> first((size_t)M);
    HIPCHK(c, hipMemcpy2DAsync(first.data(), sizeof(double), d_e64, (size_t)d * sizeof(double), sizeof(double), (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    tidx.clear();
    for (int64_t i = 0; i < M; ++i) if (!std::isnan(first[(size_t)i])) tidx.push_back((int)i);
    if (c->max_num_embeddings >= 0 && (int64_t)tidx.size() > c->max_num_embeddings) {
        static_assert(sizeof(int) == sizeof(int32_t), "row indices are 32-bit");
        std::vector<int32_t> kept;
        sample_rows(tidx.data(), (int64_t)tidx.size(), c->max_num_embeddings, c->clustering_seed, kept);
        tidx.swap(kept);
    }
    return SD_OK;
}

// The centroid of the one-cluster exit: the mean of the train rows by the rule of a14 (the single row itself), a NaN row when there is none; synchronises
int mean_of_rows(sd_ctx* c, const double* d_emb, int d, const std::vector<int>& tidx, std::vector<double>& h_cen)
{
    const size_t N = tidx.size();
    h_cen.assign((size_t)d, NAN);
    if (N == 0) return SD_OK;
    const int off1[2] = {0, (int)N};
    WS(c, int, d_order1, "cl_order", N);
    WS(c, int, d_off1, "cl_off", 2);
    WS(c, double, d_cen1, "cl_cen", (size_t)d);
    HIPCHK(c, hipMemcpyAsync(d_order1, tidx.data(), N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off1, off1, sizeof(off1), hipMemcpyHostToDevice, c->stream));
    if (int rc = launch_cluster_means(c, d_emb, d, d_order1, d_off1, 1, d_cen1)) return rc;
    HIPCHK(c, hipMemcpyAsync(h_cen.data(), d_cen1, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

// d_emb: [M][d] f64 (NaN rows = no embedding), M = chunks*3.  hard: [M].  c->last: centroids and `enrolled` are this call's; `conf` is the caller's (finalize)
int run_clustering(sd_ctx* c, const double* d_emb, int64_t M, int d, std::vector<int>& hard, int* Kout,
                   int num_clusters, int min_clusters, int max_clusters, std::vector<double>* soft_best)
{
    if (int rf = enrolled_refusal(c, d, num_clusters, min_clusters, max_clusters)) return rf;
    if (c->max_num_embeddings >= 0 && !c->dump_dir.empty())
        SD_FAIL(c, SD_ERR_ARG, "max_num_embeddings is set: the step files describe the reference's flow, which clusters every train row (unset it or clear the dump directory)");
    hard.assign((size_t)M, 0);
    if (soft_best) soft_best->assign((size_t)M, NAN);
    if (Kout) *Kout = 1;
    const bool dumping = !c->dump_dir.empty();
    c->stash.clustered = false;
    JobResult& res = c->last;
    res.cen_K = 0;                                                  // sd_last_speakers describes this call from its successful end on
    res.enrolled.clear();                                           // ... and sd_last_enrolled: -1 for every label unless the enrolled flow says otherwise
    res.hard.clear(); res.roster_ids.clear();                       // ... and sd_last_roster_ids: no roster has named this job
    if (M <= 0) return SD_OK;
    int rc;
    std::vector<int> tidx;
    if ((rc = train_rows(c, d_emb, M, d, tidx))) return rc;
    const int64_t N = (int64_t)tidx.size();
    if (c->enr_M > 0 && N > 0) {                                    // enrolled speakers claim their rows first; no row claimed: the plain flow, untouched
        bool taken = false;
        int rce = clustering_enrolled(c, d_emb, M, d, tidx, hard, Kout, soft_best, &taken);
        if (rce || taken) return rce;
    }
    const ClusterSpec spec = {c->clustering_threshold, c->min_cluster_size, num_clusters, min_clusters, max_clusters};
    if (resolve_num_clusters(spec, N).trivial) {                    // all zeros (sd.cpp:2081-2088), before any linkage runs
        // one cluster, label 0: its centroid is the mean of the train rows (a NaN row with count 0 when there is none)
        res.cen_counts.assign(1, N);
        res.cen_d = d;
        if ((rc = mean_of_rows(c, d_emb, d, tidx, res.cen))) return rc;
        res.cen_K = 1;
        return SD_OK;
    }
    // a12, then a13 + a11: the dendrogram and its cut
    std::vector<double> Zh;
    double* X = nullptr; double* Xn = nullptr;
    if ((rc = cluster_rows(c, d_emb, tidx, d, &X, &Xn, Zh))) return rc;
    ClusterPlan p;
    if ((rc = cluster_cut(c, Zh, N, X, d, spec, p, dumping ? &c->stash.clusters : nullptr))) return rc;
    const int nl = p.nl;
    // a14: centroids of the final clusters (un-normalised train rows), cosine cdist of ALL rows, argmax
    double* d_cen2 = nullptr; double* d_soft = nullptr;
    if ((rc = final_means(c, X, d, p.lab, nl, 0, p.order, p.off, &d_cen2))) return rc;
    std::vector<int64_t> counts((size_t)nl);
    for (int k = 0; k < nl; ++k) counts[(size_t)k] = p.off[(size_t)k + 1] - p.off[(size_t)k];
    if ((rc = assign_all(c, d_emb, M, d, d_cen2, nl, counts, hard, Kout, soft_best, &d_soft, res))) return rc;
    if (dumping) {
        StepStash& S = c->stash;
        S.clustered = true; S.N = N; S.K = nl; S.cluster_res = p.lab; S.hard_pre = hard;
        S.X.resize((size_t)N * d); S.Xn.resize((size_t)N * d); S.soft.resize((size_t)M * nl);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(S.X.data(), X, S.X.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(S.Xn.data(), Xn, S.Xn.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(S.soft.data(), d_soft, S.soft.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SD_OK;
}
