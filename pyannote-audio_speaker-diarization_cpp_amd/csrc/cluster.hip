// cluster.hip -- the clustering stage around the linkage: which embeddings take part, the cut of the dendrogram, the assignment of every embedding
// (compiled with -ffp-contract=off: every fp64 result is bit-identical to the reference's x86 build, which decides speaker numbering).
//   a10 filter_embeddings                      sd.cpp:2214-2259
//   a11 Cluster::cluster (normalise, size split, small->large reassign, renumber)  sd.cpp:2300-2422
//   a13 Clustering::fcluster(criterion=distance)                                   cl.cpp:121-232, 442-457
//   a14 assign_embeddings (centroids, cosine cdist, argmax)                        sd.cpp:2119-2212
//   constrained arg-max and the hyper-parameter recut                              clustering/Clustering.py
// a12, Clustering::linkage, is run_linkage in linkage.hip.  fcluster is O(N) pointer chasing and runs on the host.
#include "common.h"
#include "exact_fp.h"
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

// fcluster(criterion="distance"), cl.cpp:121-232 + 442-457.  Node ids grow with merge order, so the
// per-node max merge height is a forward pass; labels follow the reference's visiting order: internal
// left subtree, internal right subtree, then the leaf children of the node.
void fcluster_host(const std::vector<double>& Z, int64_t n, double cutoff, std::vector<int>& T)
{
    T.assign((size_t)n, 0);
    if (n == 1) { T[0] = 1; return; }
    if (n < 2) return;
    std::vector<double> MD((size_t)n - 1);
    for (int64_t k = 0; k < n - 1; ++k) {
        double mx = Z[k * 4 + 2];
        const int64_t lc = (int64_t)Z[k * 4 + 0], rc = (int64_t)Z[k * 4 + 1];
        if (lc >= n && MD[lc - n] > mx) mx = MD[lc - n];
        if (rc >= n && MD[rc - n] > mx) mx = MD[rc - n];
        MD[k] = mx;
    }
    struct Fr { int64_t node; int label; int state; };
    std::vector<Fr> st;
    st.push_back({2 * n - 2, 0, 0});
    int ncl = 0;
    while (!st.empty()) {
        Fr& f = st.back();
        const int64_t k = f.node - n;
        const int64_t lc = (int64_t)Z[k * 4 + 0], rc = (int64_t)Z[k * 4 + 1];
        if (f.state == 0) {
            if (f.label == 0 && MD[k] <= cutoff) f.label = ++ncl;
            f.state = 1;
            if (lc >= n) { const int lab = f.label; st.push_back({lc, lab, 0}); continue; }
        }
        if (f.state == 1) {
            f.state = 2;
            if (rc >= n) { const int lab = f.label; st.push_back({rc, lab, 0}); continue; }
        }
        if (lc < n) T[lc] = f.label ? f.label : ++ncl;
        if (rc < n) T[rc] = f.label ? f.label : ++ncl;
        st.pop_back();
    }
}

int run_cluster_labels(sd_ctx* c, const double* d_Xn, int64_t N, int d, double cutoff, std::vector<int>& labels1, std::vector<double>* Zout, int method, int metric)
{
    labels1.assign((size_t)N, 0);
    if (N == 1) { labels1[0] = 1; return SD_OK; }
    if (N < 2) return SD_OK;
    WS(c, double, dZ, "cl_Z", (N - 1) * 4);
    int rc = run_linkage(c, d_Xn, N, d, dZ, method, metric);
    if (rc) return rc;
    std::vector<double> Z((size_t)(N - 1) * 4);
    HIPCHK(c, hipMemcpyAsync(Z.data(), dZ, Z.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    fcluster_host(Z, N, cutoff, labels1);
    if (Zout) Zout->swap(Z);
    return SD_OK;
}

// ---------------------------------------------------------------- cluster means (sequential in member order)
// members of cluster k are order[off[k] .. off[k+1]) in ascending row index: same summation order as
// Helper::calculateClusterMeans (sd.cpp:442-473) and the centroid loop of assign_embeddings (sd.cpp:2149-2167)
__global__ void k_cluster_means(const double* __restrict__ X, int d, const int* __restrict__ order, const int* __restrict__ off,
                                double* __restrict__ cen)
{
    const int k = blockIdx.x, q = threadIdx.x;
    if (q >= d) return;
    double s = 0.0;
    const int a = off[k], b = off[k + 1];
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

// cosine distance with the reference's sequential sums (sd.cpp:476-498); soft = 2 - d; argmax first-max-wins
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
            if (m1 == 0.0 || m2 == 0.0) { *err = 1; soft[k] = NAN; }
            else soft[k] = 2.0 - (1.0 - (dot / (sqrt(m1) * sqrt(m2))));
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

static double cos_dist_host(const double* a, const double* b, int d, bool* err)      // sd.cpp:476-498
{
    double dot = 0.0, m1 = 0.0, m2 = 0.0;
    for (int i = 0; i < d; ++i) { dot += a[i] * b[i]; m1 += a[i] * a[i]; m2 += b[i] * b[i]; }
    if (m1 == 0.0 || m2 == 0.0) { *err = true; return NAN; }
    return 1.0 - (dot / (sqrt(m1) * sqrt(m2)));
}

// group rows by label (ascending row order inside each group); a row with a negative label belongs to no group
void group_by_label(const std::vector<int>& lab, int nl, std::vector<int>& order, std::vector<int>& off)
{
    off.assign((size_t)nl + 1, 0);
    for (int v : lab) if (v >= 0) off[(size_t)v + 1]++;
    for (int k = 0; k < nl; ++k) off[(size_t)k + 1] += off[(size_t)k];
    order.resize((size_t)off[(size_t)nl]);
    std::vector<int> pos(off.begin(), off.end() - 1);
    for (size_t i = 0; i < lab.size(); ++i) if (lab[i] >= 0) order[(size_t)pos[(size_t)lab[i]]++] = (int)i;
}

// Constrained number of clusters -- the branch the reference leaves unimplemented (assert(false), sd.cpp:2368-2369);
// specification = the Python it was ported from, clustering/Clustering.py:352-399: re-cut the dendrogram by merge
// index, walking away from the tuned threshold, until the number of large clusters is (closest to) num_clusters.
void constrained_recut(const std::vector<double>& Z, int64_t N, double threshold, size_t mcs, int num_clusters, std::vector<int>& lab)
{
    std::vector<double> Zi(Z);
    for (int64_t k = 0; k < N - 1; ++k) Zi[(size_t)k * 4 + 2] = (double)k;          // Clustering.py:353-354
    std::vector<int64_t> order((size_t)N - 1);
    for (int64_t k = 0; k < N - 1; ++k) order[(size_t)k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        return fabs(Z[(size_t)a * 4 + 2] - threshold) < fabs(Z[(size_t)b * 4 + 2] - threshold); });   // :362
    auto count_large = [&](const std::vector<int>& t1) {
        int mx = 0; for (int v : t1) if (v > mx) mx = v;
        std::vector<size_t> cnt((size_t)mx + 1, 0);
        for (int v : t1) cnt[(size_t)v]++;
        int nlarge = 0; for (size_t v = 1; v < cnt.size(); ++v) if (cnt[v] >= mcs) nlarge++;
        return nlarge;
    };
    int64_t best_iteration = N - 1; int best_large = 1;                               // :356-357
    std::vector<int> t1;
    bool exact = false;
    for (int64_t it : order) {
        if (Zi[(size_t)it * 4 + 3] < (double)mcs) continue;                           // :366-368
        fcluster_host(Zi, N, (double)it, t1);                                         // :371
        const int nlarge = count_large(t1);
        if (std::abs(nlarge - num_clusters) < std::abs(best_large - num_clusters)) { best_iteration = it; best_large = nlarge; }   // :377-381
        if (nlarge == num_clusters) { exact = true; break; }                          // :384-385
    }
    if (!exact) fcluster_host(Zi, N, (double)best_iteration, t1);                     // :388-391
    lab.resize((size_t)N);
    for (int64_t i = 0; i < N; ++i) lab[(size_t)i] = t1[(size_t)i] - 1;
}

// ---------------------------------------------------------------- the steps of run_clustering: the plain flow and the enrolled flow call the same ones
// a10 / a11 / a12 / a13: rows idx[0 .. N) of d_emb gathered (X) and normalised with the f32 norm (Xn), then the labels of the dendrogram cut, 0-based, nl of them.
// Method, threshold and minimum cluster size are the three hyper-parameters of Clustering.py:251-276; their defaults are the constants the
// reference hard-codes (sd.cpp:2049-2056: centroid, the float-typed threshold promoted to double, 15).  Clustering.py:317-333: centroid, median and ward
// are euclidean-only and run on the unit-normalised rows (Xn, with the port's f32 norm); the other four run on the rows as they are with the cosine metric.
int cluster_rows(sd_ctx* c, const double* d_emb, const std::vector<int>& idx, int d, double** Xout, double** Xnout, std::vector<int>& lab, int* nlout,
                 std::vector<double>* Zh)
{
    const int64_t N = (int64_t)idx.size();
    WS(c, int, d_tidx, "cl_tidx", N);
    WS(c, double, X, "cl_X", N * d);
    WS(c, double, Xn, "cl_Xn", N * d);
    HIPCHK(c, hipMemcpyAsync(d_tidx, idx.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_gather_normalize, dim3((unsigned)((N + 127) / 128)), dim3(128), 0, c->stream, d_emb, d_tidx, N, d, X, Xn);
    KCHECK(c);
    const int method = c->clustering_method;
    const bool euclid = method == SD_LINKAGE_CENTROID || method == SD_LINKAGE_MEDIAN || method == SD_LINKAGE_WARD;
    int rc = run_cluster_labels(c, euclid ? Xn : X, N, d, c->clustering_threshold, lab, Zh, method, euclid ? SD_METRIC_EUCLIDEAN : SD_METRIC_COSINE);
    if (rc) return rc;
    int nl = 0;
    for (auto& v : lab) { v -= 1; if (v + 1 > nl) nl = v + 1; }
    *Xout = X; *Xnout = Xn; *nlout = nl;
    return SD_OK;
}

// a11: which clusters reach mcs rows (clusters without a row are neither)
void split_by_size(const std::vector<int>& off, int nl, size_t mcs, std::vector<int>& large, std::vector<int>& small)
{
    large.clear(); small.clear();
    for (int k = 0; k < nl; ++k) {
        const size_t cnt = (size_t)(off[(size_t)k + 1] - off[(size_t)k]);
        if (cnt == 0) continue;
        if (cnt >= mcs) large.push_back(k); else small.push_back(k);
    }
}

// a11: every small cluster goes to the nearest candidate -- first the G rows of `enrolled` (host, [G][d]; the enrolled flow), then the large clusters in
// ascending id -- by the cosine distance of the means of the UN-normalised rows (sd.cpp:2386), the reference's float minVal loop (sd.cpp:2396).  The rows of a
// cluster that goes to an enrolled candidate get label -1; the labels that survive are renumbered 0 .. nl - 1 in sorted-id order (findUniqueClusters,
// sd.cpp:519-548).
int reassign_small(sd_ctx* c, const double* X, int d, const std::vector<int>& order, const std::vector<int>& off, const std::vector<int>& large,
                          const std::vector<int>& small, const double* enrolled, int G, std::vector<int>& lab, int& nl)
{
    const size_t N = order.size();
    WS(c, int, d_order, "cl_order", N);
    WS(c, int, d_off, "cl_off", nl + 1);
    WS(c, double, d_cen, "cl_cen", (size_t)nl * d);
    HIPCHK(c, hipMemcpyAsync(d_order, order.data(), N * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_off, off.data(), (size_t)(nl + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_cluster_means, dim3(nl), dim3(((d + 63) / 64) * 64), 0, c->stream, X, d, d_order, d_off, d_cen);   // means of UN-normalised rows (sd.cpp:2386)
    KCHECK(c);
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
    if (nl > 0) {
        hipLaunchKernelGGL(k_cluster_means, dim3(nl), dim3(((d + 63) / 64) * 64), 0, c->stream, X, d, d_order2, d_off2, d_cen2 + (size_t)G * d);
        KCHECK(c);
    }
    *cen_out = d_cen2;
    return SD_OK;
}

// a14, second half: cosine cdist of ALL M rows to the K centroids, arg-max (or the constrained arg-max); the centroids and their counts become what
// sd_last_speakers describes.  *soft_out (may be NULL) = the [M][K] score table where one was written, else null.
int assign_all(sd_ctx* c, const double* d_emb, int64_t M, int d, const double* d_cen2, int K, const std::vector<int64_t>& counts,
                      std::vector<int>& hard, int* Kout, std::vector<double>* soft_best, double** soft_out)
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
    hipLaunchKernelGGL(k_assign, dim3((unsigned)M), dim3(64), 0, c->stream, d_emb, M, d, d_cen2, K, d_hard, d_err, d_soft, d_best);
    KCHECK(c);
    int herr = 0;
    HIPCHK(c, hipMemcpyAsync(hard.data(), d_hard, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (soft_best) HIPCHK(c, hipMemcpyAsync(soft_best->data(), d_best, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    c->last_cen.resize((size_t)K * d);                              // the centroids ride this synchronisation (sd_last_speakers)
    HIPCHK(c, hipMemcpyAsync(c->last_cen.data(), d_cen2, c->last_cen.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
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
            hipLaunchKernelGGL(k_constrained_argmax, dim3((unsigned)((chunks + 63) / 64)), dim3(64), 0, c->stream, d_soft, chunks, K, fill, d_hard);
            KCHECK(c);
            HIPCHK(c, hipMemcpyAsync(hard.data(), d_hard, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        } else SD_FAIL(c, SD_ERR_ARG, "constrained assignment supports up to %d clusters (found %d)", LSAP_MAXC, K);
        if (soft_best)                                             // confidence follows the cluster actually assigned
            for (int64_t i = 0; i < M; ++i) (*soft_best)[(size_t)i] = hard[(size_t)i] >= 0 ? hs[(size_t)i * K + hard[(size_t)i]] : NAN;
    }
    if (Kout) *Kout = K;
    c->last_cen_counts = counts;
    c->last_cen_d = d;
    c->last_cen_K = K;
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
    const size_t mcs = std::min<size_t>((size_t)c->min_cluster_size, std::max<size_t>(1, (size_t)std::round(0.1 * (double)N)));     // from N, not N'
    std::vector<double> cand((size_t)G * d);
    for (int a = 0; a < G; ++a) memcpy(&cand[(size_t)a * d], &c->enr_host[(size_t)U[(size_t)a] * d], (size_t)d * sizeof(double));
    // 5 - 7: the new clusters of R
    std::vector<int> lab, order, off;
    int L = 0;
    double* X = nullptr; double* Xn = nullptr;
    if (!ridx.empty()) {
        if ((rc = cluster_rows(c, d_emb, ridx, d, &X, &Xn, lab, &L, nullptr))) return rc;
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
    if ((rc = assign_all(c, d_emb, M, d, d_cen2, G + L, counts, hard, Kout, soft_best, nullptr))) return rc;
    c->last_enrolled.assign((size_t)(G + L), -1);                           // 9
    for (int a = 0; a < G; ++a) c->last_enrolled[(size_t)a] = U[(size_t)a];
    return SD_OK;
}

// d_emb: [M][d] f64 (NaN rows = no embedding), M = chunks*3.  hard: [M]
int run_clustering(sd_ctx* c, const double* d_emb, int64_t M, int d, std::vector<int>& hard, int* Kout,
                   int num_clusters, int min_clusters, int max_clusters, std::vector<double>* soft_best)
{
    if (int rf = enrolled_refusal(c, d, num_clusters, min_clusters, max_clusters)) return rf;
    hard.assign((size_t)M, 0);
    if (soft_best) soft_best->assign((size_t)M, NAN);
    if (Kout) *Kout = 1;
    const bool dumping = !c->dump_dir.empty();
    c->stash.clustered = false;
    c->last_cen_K = 0;                                              // sd_last_speakers describes this call from its successful end on
    c->last_enrolled.clear();                                       // ... and sd_last_enrolled: -1 for every label unless the enrolled flow says otherwise
    if (M <= 0) return SD_OK;
    // a10: rows whose first element is not NaN (sd.cpp:2224)
    std::vector<double> first((size_t)M);
    HIPCHK(c, hipMemcpy2DAsync(first.data(), sizeof(double), d_emb, (size_t)d * sizeof(double), sizeof(double), (size_t)M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> tidx;
    for (int64_t i = 0; i < M; ++i) if (!std::isnan(first[(size_t)i])) tidx.push_back((int)i);
    const int64_t N = (int64_t)tidx.size();
    if (c->enr_M > 0 && N > 0) {                                    // enrolled speakers claim their rows first; no row claimed: the plain flow, untouched
        bool taken = false;
        int rce = clustering_enrolled(c, d_emb, M, d, tidx, hard, Kout, soft_best, &taken);
        if (rce || taken) return rce;
    }
    // set_num_clusters (sd.cpp:2261-2296; with num_clusters given, max = num_clusters as in Clustering.py:27-41 --
    // the port's `max_clusters == num_clusters;` is a no-op typo, sd.cpp:2278)
    const bool constrained = (num_clusters != -1) || (min_clusters != -1) || (max_clusters != -1);
    if (num_clusters != -1) { min_clusters = num_clusters; max_clusters = num_clusters; }
    if (min_clusters == -1) min_clusters = 1;
    if (max_clusters == -1) max_clusters = (int)N;
    min_clusters = std::max(1, std::min((int)N, min_clusters));
    max_clusters = std::max(1, std::min((int)N, max_clusters));
    if (min_clusters > max_clusters) min_clusters = max_clusters;
    if (min_clusters == max_clusters) num_clusters = min_clusters;
    if (N < 2 || max_clusters < 2) {                                // all zeros (sd.cpp:2081-2088)
        // one cluster, label 0: its centroid is the mean of the train rows by the rule of a14 below (the single row itself; a NaN row with count 0 when there is none)
        c->last_cen.assign((size_t)d, NAN);
        c->last_cen_counts.assign(1, N);
        c->last_cen_d = d;
        if (N > 0) {
            const int off1[2] = {0, (int)N};
            WS(c, int, d_order1, "cl_order", N);
            WS(c, int, d_off1, "cl_off", 2);
            WS(c, double, d_cen1, "cl_cen", (size_t)d);
            HIPCHK(c, hipMemcpyAsync(d_order1, tidx.data(), (size_t)N * sizeof(int), hipMemcpyHostToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d_off1, off1, sizeof(off1), hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_cluster_means, dim3(1), dim3(((d + 63) / 64) * 64), 0, c->stream, d_emb, d, d_order1, d_off1, d_cen1);
            KCHECK(c);
            HIPCHK(c, hipMemcpyAsync(c->last_cen.data(), d_cen1, (size_t)d * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        c->last_cen_K = 1;
        return SD_OK;
    }
    // a12+a13
    const double thr = c->clustering_threshold;
    std::vector<int> lab;
    std::vector<double> Zh;
    double* X = nullptr; double* Xn = nullptr;
    int nl = 0;
    int rc = cluster_rows(c, d_emb, tidx, d, &X, &Xn, lab, &nl, &Zh);
    if (rc) return rc;
    if (dumping) c->stash.clusters = lab;
    // a11: size split
    size_t mcs = std::min<size_t>((size_t)c->min_cluster_size, std::max<size_t>(1, (size_t)std::round(0.1 * (double)N)));     // sd.cpp:2308, Clustering.py:309-311
    std::vector<int> order, off;
    group_by_label(lab, nl, order, off);
    if (constrained) {
        int nlarge0 = 0;
        for (int k = 0; k < nl; ++k) if ((size_t)(off[(size_t)k + 1] - off[(size_t)k]) >= mcs) nlarge0++;
        int target = (min_clusters == max_clusters) ? min_clusters : -1;
        if (nlarge0 < min_clusters) target = min_clusters;                                            // sd.cpp:2361-2366
        if (nlarge0 > max_clusters) target = max_clusters;
        if (target != -1) {
            constrained_recut(Zh, N, thr, mcs, target, lab);
            nl = 0;
            for (int v : lab) if (v + 1 > nl) nl = v + 1;
            group_by_label(lab, nl, order, off);
        }
    }
    std::vector<int> large, small;
    split_by_size(off, nl, mcs, large, small);
    if (large.empty()) {
        // reference: assert(false) in assert-enabled builds (sd.cpp:2368), all-zero labels otherwise (sd.cpp:2371-2375)
        std::fill(lab.begin(), lab.end(), 0);
        nl = 1;
    } else if (!small.empty()) {
        if ((rc = reassign_small(c, X, d, order, off, large, small, nullptr, 0, lab, nl))) return rc;
    }
    // a14: centroids of the final clusters (un-normalised train rows), cosine cdist of ALL rows, argmax
    double* d_cen2 = nullptr; double* d_soft = nullptr;
    if ((rc = final_means(c, X, d, lab, nl, 0, order, off, &d_cen2))) return rc;
    std::vector<int64_t> counts((size_t)nl);
    for (int k = 0; k < nl; ++k) counts[(size_t)k] = off[(size_t)k + 1] - off[(size_t)k];
    if ((rc = assign_all(c, d_emb, M, d, d_cen2, nl, counts, hard, Kout, soft_best, &d_soft))) return rc;
    if (dumping) {
        StepStash& S = c->stash;
        S.clustered = true; S.N = N; S.K = nl; S.cluster_res = lab; S.hard_pre = hard;
        S.X.resize((size_t)N * d); S.Xn.resize((size_t)N * d); S.soft.resize((size_t)M * nl);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        HIPCHK(c, hipMemcpy(S.X.data(), X, S.X.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(S.Xn.data(), Xn, S.Xn.size() * sizeof(double), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(S.soft.data(), d_soft, S.soft.size() * sizeof(double), hipMemcpyDeviceToHost));
    }
    return SD_OK;
}
