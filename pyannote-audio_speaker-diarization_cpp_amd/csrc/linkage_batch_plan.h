// linkage_batch_plan.h -- which linkage jobs of one call share a launch (run_linkage_many, linkage_batch.hip), and in which groups.  Host arithmetic only,
// no HIP: tools/linkage_batch_plan_check.cpp builds it alone under the sanitizers (tests/test_linkage_many_plan_cpu.py).
//
// A job is BATCHED iff run_linkage (linkage.hip) would take it straight to the one-workgroup heap kernel -- its plan has G <= 1: today N < 1500, or option
// linkage_wgs = 0 / 1 -- and 2 <= N and N - 1 <= LINKAGE_HEAP_LDS, so that the heap of every batched job lives in LDS.  Every other job (N >= 1500 under the
// automatic geometry, N < 2, a heap beyond LDS) is SINGLE and goes through run_linkage unchanged, in list order.
// Batched jobs are sorted by descending N (stable: equal N keep list order) -- the launch issues its workgroups in that order, so its tail is short -- and cut,
// in that order, into groups whose workspaces stay within a byte budget; a job that alone exceeds the budget is a group of its own.
// Second half of the file: the cooperative geometry of one job (linkage_geometry, which linkage.hip's linkage_plan calls) and linkage_xcd_plan, which takes
// the single jobs of the one-XCD cooperative class eight to a launch (tools/linkage_xcd_plan_check.cpp, tests/test_linkage_xcd_plan_cpu.py).
// Last part: what run_linkage's plan says about the heap replay (linkage_tie_plan, linkage_hx_form) and linkage_xcd_zero_plan, which keeps the jobs of an XCD
// launch that tie at height 0 in the batch (tools/linkage_xcd_zero_plan_check.cpp, tests/test_linkage_xcd_zero_plan_cpu.py).
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

// ---------------------------------------------------------------- the cooperative geometry of one job, and the jobs that run one per XCD
// What linkage_plan (linkage.hip, which calls this) decides by arithmetic alone: workgroups, threads, columns per workgroup, the matrix form, the kernel and
// whether all workgroups sit on one XCD.  `square_ok` = false: the square matrix could not be allocated.  G <= 1: the one-workgroup heap kernel, the rest unused.
// The limits of k_linkage_rg's geometry (linkage_rg.hip asserts that its own constants are these):
constexpr int LINKAGE_RG_GMAX = 128, LINKAGE_RG_U = 4, LINKAGE_RG_T_MAX = 1024, LINKAGE_RG_SLOT = 40;
constexpr int LINKAGE_SYNC_HOST_WORDS = 32;      // the words of a sync block the host reads (linkage_dev.h: SYNC_HOST_WORDS); all k_linkage_rg touches
struct LinkageOpts { int64_t wgs, one_xcd, threads, square, kernel, prefetch; int num_cu; };      // the options linkage_* of those names; the device's CUs
struct LinkageGeom { int G, TH, cap; bool square, use_rg, onex; };
inline bool linkage_rg_fits_geom(int64_t N, int G, int TH)
{
    if (G < 2 || G > LINKAGE_RG_GMAX) return false;
    const int64_t colsB = (N + G - 1) / G;
    return colsB <= (int64_t)(TH <= 512 ? 8 : LINKAGE_RG_U) * TH && TH <= LINKAGE_RG_T_MAX;         // (8 columns per thread: the <= 512-thread forms only -- register budget)
}
// the form of k_linkage_rg a geometry takes: whether the helper wave runs, the threads launched with it, and whether a thread has more than 4 columns
inline void linkage_rg_form(int G, int TH, int cap, int& helper, int& TT, bool& wide)
{
    if (helper && (TH > 448 || G > 64)) helper = 0;         // (one slot per lane in the helper's fold; 16 waves at most)
    TT = TH + (helper ? 64 : 0);
    wide = (int64_t)(cap - 1) > (int64_t)LINKAGE_RG_U * TH;
}
inline LinkageGeom linkage_geometry(const LinkageOpts& o, int64_t N, bool square_ok)
{
    LinkageGeom p = {};
    // auto geometry (measured on clustered data, profiles/r01_linkage_scaling.txt, r02_linkage_stamps.txt, r03_linkage_*.txt): up to N = 30 000
    // the one-XCD form with one workgroup on each of the XCD's 32 CUs; above, all XCDs
    // (r03, square form: one XCD wins up to N ~ 70 000 -- 384 ms against 443 at N = 50 158, 719 against 715 at N = 75 090 -- all XCDs above: 987 ms against 1 064 at
    // N = 100 174; all XCDs: 64 workgroups up to ~90 000 rows, 128 above)
    const bool auto_onex = (int)o.wgs < 0 && o.one_xcd != 0 && o.num_cu >= 256 && N >= 1500 && N < 70000;
    int G = linkage_route_wgs(o.wgs, o.one_xcd, o.num_cu, N);
    int TH = (int)o.threads;
    // measured (r03, square form, N = 12 602, one XCD, three boxes): 32 x 256 75.2 / 82.7 / 76.8 ms, 32 x 512 84.4 / 77.2 / 85.0 ms -- the
    // boxes disagree, 256 wins on two of three; all XCDs 128 x 512 0.99 s at N = 100 174 (128 x 256: 1.10 s)
    // one XCD, larger N: 512 threads (N = 18 867: 121 ms against 126; N = 25 274: 170 against 179; N = 50 158: 384 against 465)
    if (TH <= 0) TH = auto_onex ? (N >= 16000 ? 512 : 256) : N >= 8000 ? 512 : 256;
    TH = TH >= 1024 ? 1024 : TH >= 512 ? 512 : TH >= 256 ? 256 : 128;      // (not below 128: the kernels fill their G <= 128 candidate slots with `tid < G`)
    p.G = G; p.TH = TH;
    if (G <= 1) return p;
    // square form (full N x N matrix, row-only bulk accesses) while the square fits beside everything else; the condensed form above that
    const bool square = square_ok && (o.square < 0 ? (double)N * (double)N * 8.0 <= 170e9 : o.square != 0);
    // k_linkage_rg's own automatic geometry (r05, planted embeddings, 256 threads; profiles/r05_linkage_rg.txt): one XCD with 32 workgroups only while a thread
    // has one or two columns -- N = 12 602: 72.7 ms with 32 (one XCD), 72.6 with 64 (all XCDs); N = 18 867: 127.7 / 120.0; N = 25 274: 179.1 / 165.2 (128: 169.1;
    // k_linkage_mw 170.2); N = 50 158: 462.8 / 372.8 (128: 366.3; k_linkage_mw 381.8); N = 100 174: 128 workgroups 819 ms (64: 875; k_linkage_mw 996)
    if (o.wgs < 0 && square && o.kernel != 0 && N >= 1500) {
        G = N < 16000 ? 32 : N < 45000 ? 64 : 128;
        if (G > o.num_cu) G = o.num_cu;
    }
    if ((N + G - 1) / G > 3400) G = (int)((N + 3399) / 3400);      // active-row lists and bounds live in LDS: 32 B per owned row (109 KB + 43 KB static)
    // one-XCD form while two workgroups per CU of one XCD (32 CUs) can hold the job; above, all XCDs' memory pipelines are worth more
    const bool onex = o.one_xcd != 0 && G <= 32 && o.num_cu >= 256;
    // square form: k_linkage_rg (register state, sizes / ty in the slots) where its geometry fits -- at most 4 columns per thread -- else k_linkage_mw
    bool use_rg = square && o.kernel != 0;
    // measured (r05, planted embeddings): N = 12 602, one XCD, 32 workgroups: 256 threads 72.7 ms, 512 threads 81.2, 128 threads 76.6 (k_linkage_mw 76.7);
    // N = 100 174, all XCDs, 128 workgroups: 256 threads 819 ms, 512 threads 829 (k_linkage_mw 996); 64 x 512: 875
    if (use_rg && o.threads <= 0) TH = 256;
    if (use_rg && !linkage_rg_fits_geom(N, G, TH)) {
        int t2 = TH;
        while (t2 < 1024 && !linkage_rg_fits_geom(N, G, t2)) t2 *= 2;
        if (linkage_rg_fits_geom(N, G, t2) && (o.threads <= 0 || o.kernel > 0)) TH = t2; else use_rg = false;
    }
    p.G = G; p.TH = TH; p.cap = (int)((N + G - 1) / G) + 1;
    p.square = square; p.use_rg = use_rg; p.onex = onex;
    return p;
}

// A job is XCD-BATCHED iff option linkage_batch_xcd is on, run_linkage would take it to the one-XCD form of k_linkage_rg<true, 256, 4, METHOD> -- its geometry
// with the square matrix has G >= 2, use_rg, onex, at most 4 columns per thread and at most 256 threads with the helper wave; a method code k_linkage_rg is
// built for; option linkage_force_heap off --, its workspaces fit the byte budget, and at least two such jobs of the call share (G, threads, helper): under the
// automatic options 1500 <= N < 16 000 on a device of 256 CUs.  k_linkage_rg_jobs runs up to eight of them in one cooperative launch, job x on XCD x.
struct LinkageXcdOpts { int64_t on; LinkageOpts o; int method; bool force_heap; int64_t budget_bytes; };
struct LinkageXcdKey { int G, TH, helper; };
inline bool operator==(const LinkageXcdKey& a, const LinkageXcdKey& b) { return a.G == b.G && a.TH == b.TH && a.helper == b.helper; }
// device bytes of one XCD-batched job: the square matrix; ids and neighbours (int); the two bounds (double); Z; the two slot sets; one sync block
inline int64_t linkage_xcd_ints(int64_t N) { return 2 * ((N + 1) & ~(int64_t)1); }
inline int64_t linkage_xcd_bytes(int64_t N, int G)
{
    return N * N * 8 + linkage_xcd_ints(N) * 4 + 2 * N * 8 + (N - 1) * 32 + (int64_t)2 * G * LINKAGE_RG_SLOT * 8 + LINKAGE_SYNC_HOST_WORDS * 4;
}
// the class conditions of one job (all but "two of a kind"); key: its launch geometry
inline bool linkage_job_xcd(const LinkageXcdOpts& x, int64_t N, LinkageXcdKey* key = nullptr)
{
    if (x.on == 0 || x.force_heap || x.method < 0 || x.method > 6 || N < 2 || N > 0x7fffffff / 4) return false;
    const LinkageGeom g = linkage_geometry(x.o, N, true);
    if (g.G < 2 || !g.use_rg || !g.onex) return false;
    int helper = x.o.prefetch != 0 ? 1 : 0, TT; bool wide;
    linkage_rg_form(g.G, g.TH, g.cap, helper, TT, wide);
    if (wide || TT > 256 || linkage_xcd_bytes(N, g.G) > x.budget_bytes) return false;
    if (key) *key = LinkageXcdKey{g.G, g.TH, helper};
    return true;
}

constexpr int LINKAGE_XCD_JOBS = 8;             // jobs of one launch: one per XCD
struct LinkageXcdPlan {
    std::vector<int64_t> single;        // job numbers that keep run_linkage's route, in the order they came in
    std::vector<int64_t> order;         // XCD-batched job numbers, descending N (stable)
    std::vector<LinkageXcdKey> key;     // ... the launch geometry of each
    std::vector<int64_t> group_end;     // groups (shared preparation, one set of workspaces) of order, as in LinkageBatchPlan
    std::vector<int64_t> launch_end;    // launches of order: at most LINKAGE_XCD_JOBS consecutive jobs of one group and one key
};
// over `cand`, the jobs linkage_batch_plan left single (job numbers into N, in list order)
inline void linkage_xcd_plan(const int64_t* N, const std::vector<int64_t>& cand, const LinkageXcdOpts& x, LinkageXcdPlan& p)
{
    p.single.clear(); p.order.clear(); p.key.clear(); p.group_end.clear(); p.launch_end.clear();
    std::vector<LinkageXcdKey> keys(cand.size(), LinkageXcdKey{0, 0, 0});
    std::vector<char> in(cand.size(), 0);
    for (size_t a = 0; a < cand.size(); ++a) in[a] = linkage_job_xcd(x, N[cand[a]], &keys[a]) ? 1 : 0;
    std::vector<size_t> pick;
    for (size_t a = 0; a < cand.size(); ++a) {
        int64_t alike = 0;
        if (in[a]) for (size_t b = 0; b < cand.size(); ++b) alike += in[b] && keys[b] == keys[a];
        if (alike >= 2) pick.push_back(a); else p.single.push_back(cand[a]);
    }
    std::stable_sort(pick.begin(), pick.end(), [&](size_t a, size_t b) { return N[cand[a]] > N[cand[b]]; });
    int64_t bytes = 0, first = 0, lfirst = 0;
    for (int64_t k = 0; k < (int64_t)pick.size(); ++k) {
        const size_t a = pick[(size_t)k];
        const int64_t b = linkage_xcd_bytes(N[cand[a]], keys[a].G);
        const bool new_group = k > first && (bytes + b > x.budget_bytes || k - first >= LINKAGE_BATCH_MAX_JOBS);
        if (new_group) { p.group_end.push_back(k); first = k; bytes = 0; }
        if (k > lfirst && (new_group || k - lfirst >= LINKAGE_XCD_JOBS || !(keys[a] == p.key.back()))) { p.launch_end.push_back(k); lfirst = k; }
        bytes += b;
        p.order.push_back(cand[a]); p.key.push_back(keys[a]);
    }
    if (!pick.empty()) { p.group_end.push_back((int64_t)pick.size()); p.launch_end.push_back((int64_t)pick.size()); }
}

// ---------------------------------------------------------------- ties at height 0 inside the XCD batch (option linkage_batch_xcd_zero)
// The limits of k_linkage_hx's geometry (linkage_hx.hip asserts that its own constants are these) and what run_linkage's plan decides about the heap replay by
// arithmetic alone (linkage.hip's linkage_plan calls linkage_tie_plan; linkage_hx_run calls linkage_hx_form).
constexpr int LINKAGE_HX_T = 256, LINKAGE_HX_U = 4, LINKAGE_HX_GMAX = 128, LINKAGE_HX_LDS_HEAP = 8191;
inline bool linkage_hx_fits_geom(int64_t N, int workers)
{
    if (workers < 1 || workers > LINKAGE_HX_GMAX || N < 3) return false;
    return (N + workers - 1) / workers <= (int64_t)LINKAGE_HX_U * LINKAGE_HX_T;
}
// a tie can go to k_linkage_hx (square matrix, option linkage_tie_kernel, a geometry that fits): one XCD first, worker workgroups
struct LinkageTie { bool replay, hx_onex; int workers; };
inline LinkageTie linkage_tie_plan(int64_t tie_kernel, int64_t one_xcd, int num_cu, int64_t N, bool square)
{
    LinkageTie t = {false, false, 0};
    if (!square || tie_kernel == 0) return t;
    bool hx_onex = one_xcd != 0 && num_cu >= 256 && linkage_hx_fits_geom(N, 31);
    int workers = hx_onex ? 31 : (N >= 60000 ? 127 : 63);
    if (tie_kernel > 1) { workers = (int)tie_kernel; hx_onex = hx_onex && workers <= 31; }
    if (workers + 1 > num_cu) workers = num_cu - 1;
    t.replay = linkage_hx_fits_geom(N, workers); t.workers = workers; t.hx_onex = hx_onex;
    return t;
}
// k_linkage_hx's dynamic LDS: 16-bit keys and positions of all entries (n <= 65 535) + as many heap values as fit beside them, at most levels 0-12.
// The 16-bit form keeps 4 N bytes of keys and positions in LDS beside ~27 KB of static LDS: it is taken only while those leave room for at least
// 1 024 heap values inside the budget (N <= 31 232); from there to 65 535 rows the request would exceed the CU's 160 KB and every cooperative launch
// would be refused -- those sizes take the 32-bit form, as does every size under option linkage_hx_wide.  lc: heap values in LDS; the bytes to ask for.
inline void linkage_hx_form(int64_t N, bool wide, bool& s16, int& lc, size_t& dyn)
{
    const size_t budget = 130 * 1024;
    s16 = N <= 65535 && !wide && (size_t)4 * (size_t)N + 8 * 1024 <= budget;
    const size_t kp_bytes = s16 ? (size_t)4 * (size_t)N : 0;
    int64_t lc64 = kp_bytes < budget ? (int64_t)((budget - kp_bytes) / 8) : 0;
    if (lc64 > LINKAGE_HX_LDS_HEAP) lc64 = LINKAGE_HX_LDS_HEAP;
    if (lc64 > N - 1) lc64 = N - 1;
    lc = (int)lc64;
    dyn = (((size_t)lc * 8 + kp_bytes) + 15) & ~(size_t)15;
}

// A job of an XCD launch (linkage_xcd_plan) that did not finish there joins the ZERO SET iff option linkage_batch_xcd_zero is 1, it stopped at a tie whose
// height has exactly the bits of 0.0, in front of its first merge (row 0 of its Z, zeroed before the launch, still has size 0 -- what LinkageJob::coop reads),
// option linkage_zero_phase is on, its plan alone would send the tie to the one-XCD form of k_linkage_hx (replay && hx_onex), and option linkage_hx_wide is
// off (only the 16-bit form of k_linkage_hx_jobs is built).  Everything else is redone alone, with the first reason that applies.
struct LinkageXcdZeroOpts { int64_t on, zero_phase, tie_kernel, one_xcd; bool hx_wide; int num_cu; };
struct LinkageXcdZeroJob { int64_t N; LinkageXcdKey key; bool ran, timeout, tie; uint64_t tie_bits; bool untouched; };      // a job and how its first launch ended
enum LinkageZeroWhy { ZERO_IN = 0, ZERO_KEY_OFF, ZERO_NOT_RUN, ZERO_TIMEOUT, ZERO_NO_TIE, ZERO_TIE_ABOVE, ZERO_AFTER_MERGE, ZERO_PHASE_OFF, ZERO_NO_ONEX_REPLAY, ZERO_WIDE };
inline LinkageZeroWhy linkage_job_xcd_zero(const LinkageXcdZeroOpts& o, const LinkageXcdZeroJob& j, int* workers = nullptr)
{
    if (o.on != 1) return ZERO_KEY_OFF;
    if (!j.ran) return ZERO_NOT_RUN;
    if (j.timeout) return ZERO_TIMEOUT;
    if (!j.tie) return ZERO_NO_TIE;
    if (j.tie_bits != 0) return ZERO_TIE_ABOVE;      // (-0.0 too: run_linkage compares the value, but a distance is a square root or a cosine rule's clamp, never -0)
    if (!j.untouched) return ZERO_AFTER_MERGE;
    if (o.zero_phase == 0) return ZERO_PHASE_OFF;
    const LinkageTie t = linkage_tie_plan(o.tie_kernel, o.one_xcd, o.num_cu, j.N, true);
    if (!t.replay || !t.hx_onex) return ZERO_NO_ONEX_REPLAY;
    bool s16; int lc; size_t dyn;
    linkage_hx_form(j.N, o.hx_wide, s16, lc, dyn);
    if (!s16) return ZERO_WIDE;
    if (workers) *workers = t.workers;
    return ZERO_IN;
}
// device bytes a job needs beyond linkage_xcd_bytes to go through the zero launches: heap values, keys and positions; the command record and the workers'
// reply records (granules); the workers' two change lists of `cap` entries each; size and ty.  Every part starts on a multiple of 8 bytes.
inline int64_t linkage_xcd_zero_cap(int64_t N, int workers) { return (N + workers - 1) / workers; }
inline int64_t linkage_xcd_zero_ints(int64_t N, int workers) { return 4 * ((N + 1) & ~(int64_t)1) + ((workers * linkage_xcd_zero_cap(N, workers) + 1) & ~(int64_t)1); }
inline int64_t linkage_xcd_zero_doubles(int64_t N, int workers) { return N + workers * linkage_xcd_zero_cap(N, workers); }
inline int64_t linkage_xcd_zero_granules(int workers) { return 16 + (int64_t)8 * workers; }
inline int64_t linkage_xcd_zero_bytes(int64_t N, int workers)
{
    return linkage_xcd_zero_ints(N, workers) * 4 + linkage_xcd_zero_doubles(N, workers) * 8 + linkage_xcd_zero_granules(workers) * 8;
}
struct LinkageXcdZeroPlan {
    std::vector<LinkageZeroWhy> why;    // per job of the input: ZERO_IN = in a launch, else why it is redone alone
    std::vector<int64_t> order;         // the zero set: indices into the input, in input (= plan) order
    std::vector<int> workers;           // ... the worker workgroups of each
    std::vector<int64_t> launch_end;    // launches of order: at most LINKAGE_XCD_JOBS consecutive jobs with equal (G, TH, helper, workers)
};
inline void linkage_xcd_zero_plan(const LinkageXcdZeroJob* jobs, int64_t n, const LinkageXcdZeroOpts& o, LinkageXcdZeroPlan& p)
{
    p.why.assign((size_t)n, ZERO_KEY_OFF); p.order.clear(); p.workers.clear(); p.launch_end.clear();
    int64_t lfirst = 0;
    for (int64_t k = 0; k < n; ++k) {
        int w = 0;
        p.why[(size_t)k] = linkage_job_xcd_zero(o, jobs[k], &w);
        if (p.why[(size_t)k] != ZERO_IN) continue;
        const int64_t at = (int64_t)p.order.size();
        if (at > lfirst && (at - lfirst >= LINKAGE_XCD_JOBS || !(jobs[k].key == jobs[p.order.back()].key) || w != p.workers.back())) { p.launch_end.push_back(at); lfirst = at; }
        p.order.push_back(k); p.workers.push_back(w);
    }
    if (!p.order.empty()) p.launch_end.push_back((int64_t)p.order.size());
}
