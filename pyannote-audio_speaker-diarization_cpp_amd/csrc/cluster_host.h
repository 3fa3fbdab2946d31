// cluster_host.h -- the host arithmetic of one cut of a dendrogram, up to the point where centroids are needed: fcluster (a13), the number-of-clusters rules,
// the constrained re-cut and the size split (a11).  run_clustering (cluster.hip) and every cut of sd_cut_turns_many (cut.hip) go through cluster_plan.
// Plain C++ without a GPU header: the library and the stand-alone sanitizer program (tools/cluster_plan_check.cpp) include the same text.  No expression
// has the form a * b + c on doubles: a build with and one without FMA contraction give the same bits.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include "../../include/sdhip.h"

// Clustering.py:317-333: centroid, median and ward are euclidean-only and run on the unit-normalised rows; the other four methods run on the rows as
// they are with the cosine metric
inline int linkage_metric_of(int method)
{
    return method == SD_LINKAGE_CENTROID || method == SD_LINKAGE_MEDIAN || method == SD_LINKAGE_WARD ? SD_METRIC_EUCLIDEAN : SD_METRIC_COSINE;
}

// fcluster(criterion="distance"), cl.cpp:121-232 + 442-457.  Node ids grow with merge order, so the
// per-node max merge height is a forward pass; labels follow the reference's visiting order: internal
// left subtree, internal right subtree, then the leaf children of the node.
inline void fcluster_host(const std::vector<double>& Z, int64_t n, double cutoff, std::vector<int>& T)
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

// group rows by label (ascending row order inside each group); a row with a negative label belongs to no group
inline void group_by_label(const std::vector<int>& lab, int nl, std::vector<int>& order, std::vector<int>& off)
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
inline void constrained_recut(const std::vector<double>& Z, int64_t N, double threshold, size_t mcs, int num_clusters, std::vector<int>& lab)
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

// a11: which clusters reach mcs rows (clusters without a row are neither)
inline void split_by_size(const std::vector<int>& off, int nl, size_t mcs, std::vector<int>& large, std::vector<int>& small)
{
    large.clear(); small.clear();
    for (int k = 0; k < nl; ++k) {
        const size_t cnt = (size_t)(off[(size_t)k + 1] - off[(size_t)k]);
        if (cnt == 0) continue;
        if (cnt >= mcs) large.push_back(k); else small.push_back(k);
    }
}

// What one cut is made with: the hyper-parameters that act behind the linkage (Clustering.py:251-276) and the caller's constraints on the count (-1 = unset)
struct ClusterSpec { double threshold; int min_cluster_size, num_clusters, min_clusters, max_clusters; };

// set_num_clusters (sd.cpp:2261-2296; with num_clusters given, max = num_clusters as in Clustering.py:27-41 -- the port's `max_clusters == num_clusters;`
// is a no-op typo, sd.cpp:2278).  constrained = the caller set any of the three; trivial = the "all zeros" exit (sd.cpp:2081-2088): one cluster, no linkage
struct ClusterCounts { int min_clusters, max_clusters; bool constrained, trivial; };
inline ClusterCounts resolve_num_clusters(const ClusterSpec& s, int64_t N)
{
    ClusterCounts r;
    r.constrained = (s.num_clusters != -1) || (s.min_clusters != -1) || (s.max_clusters != -1);
    r.min_clusters = s.min_clusters; r.max_clusters = s.max_clusters;
    if (s.num_clusters != -1) { r.min_clusters = s.num_clusters; r.max_clusters = s.num_clusters; }
    if (r.min_clusters == -1) r.min_clusters = 1;
    if (r.max_clusters == -1) r.max_clusters = (int)N;
    r.min_clusters = std::max(1, std::min((int)N, r.min_clusters));
    r.max_clusters = std::max(1, std::min((int)N, r.max_clusters));
    if (r.min_clusters > r.max_clusters) r.min_clusters = r.max_clusters;
    r.trivial = N < 2 || r.max_clusters < 2;
    return r;
}

// the minimum cluster size as it is used: the option, lowered for few rows (sd.cpp:2308, Clustering.py:309-311)
inline size_t resolve_min_cluster_size(int option, int64_t N) { return std::min<size_t>((size_t)option, std::max<size_t>(1, (size_t)std::round(0.1 * (double)N))); }

// max_num_embeddings (Clustering.py:12, 69-76; commented out in the port, sd.cpp:2231-2249): which train rows are clustered when there are more than
// max_num of them.  The reference shuffles and keeps the first max_num; here the rows with the max_num smallest keys stay, ascending by row: the same
// uniform sample, but a function of (seed, row index) alone.  fin is a bijection of 64-bit words and G is odd, so distinct rows have distinct keys
// (no tie rule); the sample for m is a subset of the one for m + 1; a row appended to the list pushes at most one row out.
inline uint64_t sample_fin(uint64_t x)
{
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
inline uint64_t sample_key(int64_t seed, int64_t i)
{
    const uint64_t G = 0x9E3779B97F4A7C15ull;
    return sample_fin(sample_fin((uint64_t)seed + G) + (uint64_t)i * G);
}
// rows [n] ascending -> out: all of them where max_num is -1 or n <= max_num, else the max_num rows with the smallest keys, ascending.  Returns the count
inline int64_t sample_rows(const int32_t* rows, int64_t n, int64_t max_num, int64_t seed, std::vector<int32_t>& out)
{
    if (max_num < 0 || n <= max_num) { out.assign(rows, rows + (n > 0 ? n : 0)); return n > 0 ? n : 0; }
    std::vector<uint64_t> key((size_t)n);
    for (int64_t q = 0; q < n; ++q) key[(size_t)q] = sample_key(seed, rows[q]);
    std::vector<uint64_t> sorted(key);
    std::nth_element(sorted.begin(), sorted.begin() + (max_num - 1), sorted.end());
    const uint64_t limit = sorted[(size_t)max_num - 1];                              // the largest key that stays
    out.clear();
    for (int64_t q = 0; q < n; ++q) if (key[(size_t)q] <= limit) out.push_back(rows[q]);
    return (int64_t)out.size();
}

// Everything of a cut up to the point where centroids are needed: the 0-based labels of the N rows after the cut at spec.threshold and, where the
// constraints ask for it (sd.cpp:2361-2366), after the re-cut; nl labels; the membership (order / off of group_by_label); the clusters that reach mcs
// rows and those that do not.  trivial: one cluster, label 0 for every row, nothing else filled.
struct ClusterPlan { bool trivial = false; size_t mcs = 1; int nl = 1; std::vector<int> lab, order, off, large, small; };
inline void cluster_plan(const std::vector<double>& Z, int64_t N, const ClusterSpec& spec, ClusterPlan& p, std::vector<int>* first_cut = nullptr /* the labels before any re-cut */)
{
    const ClusterCounts nc = resolve_num_clusters(spec, N);
    p = ClusterPlan();
    p.trivial = nc.trivial;
    p.mcs = resolve_min_cluster_size(spec.min_cluster_size, N);
    if (p.trivial) { p.lab.assign((size_t)N, 0); if (first_cut) *first_cut = p.lab; return; }
    auto count_labels = [&]() { p.nl = 0; for (int v : p.lab) if (v + 1 > p.nl) p.nl = v + 1; };
    fcluster_host(Z, N, spec.threshold, p.lab);                                      // a13
    for (auto& v : p.lab) v -= 1;
    count_labels();
    if (first_cut) *first_cut = p.lab;
    group_by_label(p.lab, p.nl, p.order, p.off);
    if (nc.constrained) {
        int nlarge0 = 0;
        for (int k = 0; k < p.nl; ++k) if ((size_t)(p.off[(size_t)k + 1] - p.off[(size_t)k]) >= p.mcs) nlarge0++;
        int target = (nc.min_clusters == nc.max_clusters) ? nc.min_clusters : -1;
        if (nlarge0 < nc.min_clusters) target = nc.min_clusters;                     // sd.cpp:2361-2366
        if (nlarge0 > nc.max_clusters) target = nc.max_clusters;
        if (target != -1) {
            constrained_recut(Z, N, spec.threshold, p.mcs, target, p.lab);
            count_labels();
            group_by_label(p.lab, p.nl, p.order, p.off);
        }
    }
    split_by_size(p.off, p.nl, p.mcs, p.large, p.small);
}
