// linkage_batch_plan.h -- which linkage jobs of one call share a launch (run_linkage_many, linkage_batch.hip), and in which groups.  Host arithmetic only,
// no HIP: tools/linkage_batch_plan_check.cpp builds it alone under the sanitizers (tests/test_linkage_many_plan_cpu.py).
//
// A job is BATCHED iff run_linkage (linkage.hip) would take it straight to the one-workgroup heap kernel -- its plan has G <= 1: today N < 1500, or option
// linkage_wgs = 0 / 1 -- and 2 <= N and N - 1 <= LINKAGE_HEAP_LDS, so that the heap of every batched job lives in LDS.  Every other job (N >= 1500 under the
// automatic geometry, N < 2, a heap beyond LDS) is SINGLE and goes through run_linkage unchanged, in list order.
// Batched jobs are sorted by descending N (stable: equal N keep list order) -- the launch issues its workgroups in that order, so its tail is short -- and cut,
// in that order, into groups whose workspaces stay within a byte budget; a job that alone exceeds the budget is a group of its own.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

constexpr int LINKAGE_HEAP_LDS = 2048;          // entries of k_linkage_heap's LDS heap (linkage_heap.hip asserts that its HEAP_LDS is this)
constexpr int64_t LINKAGE_BATCH_MAX_JOBS = 32768;      // jobs of one group: blockIdx.z of the distance kernel

// The first decision of linkage_plan (linkage.hip, which calls this): the cooperative workgroups of a job of N rows; <= 1 = the one-workgroup heap kernel.
// wgs / one_xcd: the options linkage_wgs / linkage_one_xcd; num_cu: the device's.
inline int linkage_route_wgs(int64_t wgs, int64_t one_xcd, int num_cu, int64_t N)
{
    int G = (int)wgs;
    if (G < 0 && one_xcd != 0 && num_cu >= 256 && N >= 1500 && N < 70000) G = 32;      // the one-XCD form (linkage_plan: auto_onex)
    if (G < 0) G = N >= 90000 ? 128 : N >= 8000 ? 64 : N >= 1500 ? 32 : 0;
    if (G > num_cu) G = num_cu;
    return G;
}

struct LinkageRoute { int64_t wgs, one_xcd; int num_cu; };
inline bool linkage_job_batched(const LinkageRoute& r, int64_t N)
{
    return N >= 2 && N - 1 <= LINKAGE_HEAP_LDS && linkage_route_wgs(r.wgs, r.one_xcd, r.num_cu, N) <= 1;
}

// Device bytes of one batched job: the condensed matrix, sizes / ids / neighbours (int), bounds (double), Z.  Every part starts on a multiple of 8 bytes.
inline int64_t linkage_job_ints(int64_t N) { return 3 * ((N + 1) & ~(int64_t)1); }
inline int64_t linkage_job_bytes(int64_t N)
{
    return N * (N - 1) / 2 * 8 + linkage_job_ints(N) * 4 + N * 8 + (N - 1) * 32;
}

struct LinkageBatchPlan {
    std::vector<int64_t> single;        // job numbers, list order
    std::vector<int64_t> order;         // batched job numbers, descending N (stable)
    std::vector<int64_t> group_end;     // group g = order[group_end[g - 1] .. group_end[g]) (group_end[-1] = 0)
};
inline void linkage_batch_plan(const int64_t* N, int64_t J, const LinkageRoute& r, int64_t budget_bytes, LinkageBatchPlan& p)
{
    p.single.clear(); p.order.clear(); p.group_end.clear();
    for (int64_t j = 0; j < J; ++j) (linkage_job_batched(r, N[j]) ? p.order : p.single).push_back(j);
    std::stable_sort(p.order.begin(), p.order.end(), [&](int64_t a, int64_t b) { return N[a] > N[b]; });
    int64_t bytes = 0, first = 0;
    for (int64_t k = 0; k < (int64_t)p.order.size(); ++k) {
        const int64_t b = linkage_job_bytes(N[p.order[(size_t)k]]);
        if (k > first && (bytes + b > budget_bytes || k - first >= LINKAGE_BATCH_MAX_JOBS)) { p.group_end.push_back(k); first = k; bytes = 0; }
        bytes += b;
    }
    if (!p.order.empty()) p.group_end.push_back((int64_t)p.order.size());
}
