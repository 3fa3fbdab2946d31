// linkage_hx.hip -- k_linkage_hx: the reference's fast_linkage (cl.cpp:289-406) replayed EXACTLY -- indexed binary heap included
// (cl.cpp:28-119) -- with the O(n) parts of every step spread over G worker workgroups.
//
// Why: on data with exact ties (duplicated embeddings: looped audio, digital silence) the merge order among equal heights is whatever
// the reference's heap hands out first, and that depends on the whole history of its array; the cooperative kernels (k_linkage_rg /
// k_linkage_mw) take a merge only while the closest pair is unique and stop at the first tie.  Until round 5 the whole job then went
// to k_linkage_heap, ONE workgroup: 786 ms at N = 14 382 (the raw 1-h workload), 10x the tie-free time.  Here the heap is still replayed
// operation by operation by one thread (workgroup 0, the "master", which owns no columns), but
//   * the Lance-Williams update, the neighbour patches (cl.cpp:361-392) and the NN(y) search (cl.cpp:395-404) of a merge run on the
//     workers, each on its own contiguous range of columns of the full N x N matrix (k_linkage_rg's layout: row y is rewritten, not
//     mirrored; the current copy of an entry lives in the row of the cluster that was a merge's survivor last, index `ty`);
//   * the rows whose lower bound dropped (the reference's change_value calls inside the z loop, IN ASCENDING z) come back as one
//     ordered list per worker -- workers own ascending column ranges, so concatenating the lists in worker order is ascending z;
//   * a stale heap top (cl.cpp:329-338) is rescanned by all workers, each its own columns of that row;
//   * the top 8 191 heap entries (levels 0-12) live in the master's LDS, the rest in global memory.
// Hand-offs are k_linkage_rg's 8-byte {payload, tag} granules: one command record master -> workers, one reply record per worker.
// Z is bit-identical to the reference for every input (tests/test_gpu_parity.py: ties, lattices, duplicates).
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_linkage_hx's fence-free hand-offs (sc1 loads / stores, 8-byte tagged granules) are written for gfx950 only"
#endif

#define HX_T 256
#define HX_U 4            // columns per worker thread
#define HX_GMAX 128       // workers
#define HX_CMDW 10        // command: op, x, y, dist (2), nx, ny, tx, ty, k
#define HX_REPW 4         // reply: count of changed rows | NN partial: column, value (2)
#define HX_STAGE 2048     // changed rows staged in the master's LDS per pass
#define HX_LDS_HEAP 8191  // heap entries kept in LDS (levels 0 .. 12)
#define HX_OP_SCAN 1
#define HX_OP_MERGE 2
#define HX_OP_QUIT 3

// the reference's heap (cl.cpp:28-119) over two tiers of storage; every operation below is the reference's, swap by swap
// Storage: the values of the first `lc` entries (the top levels) in LDS, the rest in global memory; keys and positions in LDS as 16-bit
// numbers when n <= 65 535 (S16), else in global memory.  A sift moves ONE element along a path: it is held in registers and written once
// at its final place, the elements it passes are shifted by one level -- the array the reference's swap-by-swap loops leave behind
// (cl.cpp:44-78: every swap exchanges the moving element with the next one on the path), with a third of the memory traffic.
template <bool S16>
struct HxHeap {
    double* lv; double* gv; unsigned short* lk16; unsigned short* lp16; int* gk; int* gp; int lc; int size;
    __device__ __forceinline__ double V(int i) const { return i < lc ? lv[i] : gv[i]; }
    __device__ __forceinline__ void setV(int i, double v) { if (i < lc) lv[i] = v; else gv[i] = v; }
    __device__ __forceinline__ int K(int i) const { if constexpr (S16) return (int)lk16[i]; else return gk[i]; }
    __device__ __forceinline__ void setK(int i, int k) { if constexpr (S16) lk16[i] = (unsigned short)k; else gk[i] = k; }
    __device__ __forceinline__ int P(int key) const { if constexpr (S16) return (int)lp16[key]; else return gp[key]; }
    __device__ __forceinline__ void setP(int key, int i) { if constexpr (S16) lp16[key] = (unsigned short)i; else gp[key] = i; }
};
template <bool S16> __device__ __forceinline__ void hx_swap(HxHeap<S16>& h, int a, int b)                          // cl.cpp:70-78
{
    const double va = h.V(a), vb = h.V(b);
    h.setV(a, vb); h.setV(b, va);
    const int ka = h.K(a), kb = h.K(b);
    h.setK(a, kb); h.setK(b, ka);
    h.setP(ka, b); h.setP(kb, a);
}
template <bool S16> __device__ __forceinline__ void hx_down(HxHeap<S16>& h, int idx)                                // cl.cpp:53-68
{
    const double v = h.V(idx);
    const int k = h.K(idx);
    const int start = idx;
    int ch = 2 * idx + 1;
    while (ch < h.size) {
        double vc = h.V(ch);
        if (ch + 1 < h.size) { const double v1 = h.V(ch + 1); if (v1 < vc) { vc = v1; ch += 1; } }
        if (v > vc) { const int kc = h.K(ch); h.setV(idx, vc); h.setK(idx, kc); h.setP(kc, idx); idx = ch; ch = 2 * idx + 1; }
        else break;
    }
    if (idx != start) { h.setV(idx, v); h.setK(idx, k); h.setP(k, idx); }
}
template <bool S16> __device__ __forceinline__ void hx_up(HxHeap<S16>& h, int idx)                                  // cl.cpp:44-51
{
    const double v = h.V(idx);
    const int k = h.K(idx);
    const int start = idx;
    while (idx > 0) {
        const int par = (idx - 1) >> 1;
        const double vp = h.V(par);
        if (!(vp > v)) break;
        const int kp = h.K(par);
        h.setV(idx, vp); h.setK(idx, kp); h.setP(kp, idx);
        idx = par;
    }
    if (idx != start) { h.setV(idx, v); h.setK(idx, k); h.setP(k, idx); }
}
template <bool S16> __device__ __forceinline__ void hx_change(HxHeap<S16>& h, int key, double v)                    // cl.cpp:108-117
{
    const int idx = h.P(key);
    const double old = h.V(idx);
    h.setV(idx, v);
    if (v < old) hx_up(h, idx); else hx_down(h, idx);
}
// change_value for a value known to have DROPPED (the rows of cl.cpp:381-392: dist < min_dist[z]): the same as hx_change without reading the old value
template <bool S16> __device__ __forceinline__ void hx_decrease(HxHeap<S16>& h, int key, double v)
{
    const int idx = h.P(key);
    h.setV(idx, v);
    hx_up(h, idx);
}

template <bool ONEX, bool S16, int METHOD>
__global__ __launch_bounds__(HX_T) void k_linkage_hx(double* D, int n, int* cid, int* size, int* tyv, int* nb, double* md, double* Z,
                                                     double* g_hval, int* g_hkey, int* g_hpos, MwGran* cmd /*[16]*/, MwGran* rep /*[G][8]*/,
                                                     int* chg_z /*[G][cap]*/, double* chg_v /*[G][cap]*/, unsigned* sync, int cap, int G /*workers*/, int lc,
                                                     double stop_above /*stop in front of the first merge higher than this (inf = never); sync[SYNC_MERGES] = merges done*/)
{
    constexpr unsigned hx_xcc = 0;      // the one-XCD form runs on XCC 0
#include "linkage_hx_body.inc"
}

// The batched twin of k_linkage_hx<true, true, METHOD>: 8 (G + 1) workgroups, up to 8 jobs, job x on XCD x, each up to its first merge above height 0 (DESIGN
// 7.10).  A workgroup reads the XCC it sits on; with a job of that number it runs k_linkage_hx's own body (linkage_hx_body.inc) on that job's matrix, heap
// arrays, command / reply granules, change lists and sync block: the ticket it takes there is the job's, and it is the master or worker ticket - 1 of that job
// on the geometry (workers, cap, lc) the job has alone.  Two jobs share no word.  The plain-store hand-offs (STX<true>) need every participant of a job on one
// XCD's L2: each of them has read that it sits on XCC x.  How the dispatcher deals the workgroups decides only whether G + 1 of them arrive; if not, the bounded
// poll ends that job alone (SYNC_TIMEOUT in its block) and the host runs it again by itself.  A raised error slot: nobody touches the job.
// Dynamic LDS is the launch's (the largest job's); a job lays its own lc and n out in it.
template <int METHOD>
__global__ __launch_bounds__(HX_T) void k_linkage_hx_jobs(const LinkageHxJob* __restrict__ jobs, int nj, int G /*workers*/, const int* __restrict__ errs)
{
    __shared__ int s_job;
    if (threadIdx.x == 0) {
        const int xcc = (int)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));       // HW_REG_XCC_ID[3:0]
        s_job = (xcc < nj && jobs[xcc].n >= 3 && !errs[jobs[xcc].err]) ? xcc : -1;
    }
    __syncthreads();
    if (s_job < 0) return;
    const LinkageHxJob jb = jobs[s_job];
    const unsigned hx_xcc = (unsigned)s_job;
    constexpr bool ONEX = true, S16 = true;
    double* D = jb.D; const int n = jb.n; int* cid = jb.cid; int* size = jb.size; int* tyv = jb.ty; int* nb = jb.nb; double* md = jb.md; double* Z = jb.Z;
    double* g_hval = jb.hval; int* g_hkey = jb.hkey; int* g_hpos = jb.hpos; MwGran* cmd = jb.cmd; MwGran* rep = jb.rep; int* chg_z = jb.chg_z; double* chg_v = jb.chg_v;
    unsigned* sync = jb.sync; const int cap = jb.cap, lc = jb.lc;
    const double stop_above = 0.0;          // the merges at height 0 only: k_linkage_rg_jobs<M, true> goes on from there
#include "linkage_hx_body.inc"
}

// ---------------------------------------------------------------- launchers (run_linkage, linkage.hip; run_linkage_many, linkage_batch.hip)
static_assert(HX_T == LINKAGE_HX_T && HX_U == LINKAGE_HX_U && HX_GMAX == LINKAGE_HX_GMAX && HX_LDS_HEAP == LINKAGE_HX_LDS_HEAP, "linkage_batch_plan.h plans with these limits");
bool linkage_hx_fits(int64_t N, int workers) { return linkage_hx_fits_geom(N, workers); }
// the caller (run_linkage_many) has planned the launch with linkage_job_xcd_zero: workers <= 31, every job of the 16-bit form, max_dyn the largest job's request
hipError_t linkage_hx_jobs_launch(sd_ctx* c, int method, int workers, const LinkageHxJob* d_jobs, int nj, size_t max_dyn, const int* d_errs)
{
    const void* f = nullptr;
    if (workers >= 1 && workers <= 31 && nj >= 1 && nj <= LINKAGE_XCD_JOBS) lw_dispatch(method, [&](auto M) { f = (const void*)k_linkage_hx_jobs<M.value>; });
    if (!f) return hipErrorInvalidValue;
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)max_dyn);
    (void)hipGetLastError();
    void* args[] = {&d_jobs, &nj, &workers, &d_errs};
    // cooperative launch: all workgroups are resident together, or the launch is refused (the workgroups of a job poll each other's granules)
    return hipLaunchCooperativeKernel(f, dim3(8 * (workers + 1)), dim3(HX_T), args, max_dyn, c->stream);
}
// D: full N x N matrix, nb / md: exact nearest neighbours above each row (k_pdist_sq + k_row_nn); size = 1, cid = iota, tyv = -1
int linkage_hx_run(sd_ctx* c, int method, bool onex, int workers, double* D, int64_t N, int* cid, int* size, int* tyv, int* nb, double* md, double* d_Z, bool* stopped,
                   double stop_above, int64_t* merges_done, bool* launched)
{
    *stopped = false;
    if (merges_done) *merges_done = 0;
    if (launched) *launched = false;
    const int G = workers;
    const int cap = (int)((N + G - 1) / G);
    // dynamic LDS (linkage_batch_plan.h's linkage_hx_form, which the batch shares): the 16-bit form where it fits, else -- and under option linkage_hx_wide, on
    // any size: tests -- the 32-bit key / position form (a 4-hour job with ties fell through to the one-workgroup heap kernel when the 16-bit
    // form's request exceeded the CU's LDS)
    bool s16; int lc; size_t dyn;
    linkage_hx_form(N, c->linkage_hx_wide, s16, lc, dyn);
    WS(c, double, hv, "cl_hval", N);
    WS(c, int, hk, "cl_hkey", N);
    WS(c, int, hp, "cl_hpos", N);
    WS(c, MwGran, cmd, "hx_cmd", 16 + (int64_t)8 * G);
    WS(c, int, chz, "hx_chg_z", (int64_t)G * cap);
    WS(c, double, chv, "hx_chg_v", (int64_t)G * cap);
    WS(c, unsigned, sync, "cl_sync", SYNC_WORDS);
    HIPCHK(c, hipMemsetAsync(cmd, 0, (size_t)(16 + 8 * G) * sizeof(MwGran), c->stream));
    HIPCHK(c, hipMemsetAsync(sync, 0, SYNC_WORDS * sizeof(unsigned), c->stream));
    MwGran* rep = cmd + 16;
    const void* f = nullptr;
    lw_dispatch(method, [&](auto M) {
        f = onex ? (s16 ? (const void*)k_linkage_hx<true, true, M.value> : (const void*)k_linkage_hx<true, false, M.value>)
                 : (s16 ? (const void*)k_linkage_hx<false, true, M.value> : (const void*)k_linkage_hx<false, false, M.value>);
    });
    if (!f) SD_FAIL(c, SD_ERR_ARG, "k_linkage_hx: no linkage method %d", method);
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    (void)hipGetLastError();
    int n_i = (int)N, cap_i = cap, G_i = G, lc_i = lc;
    void* args[] = {&D, &n_i, &cid, &size, &tyv, &nb, &md, &d_Z, &hv, &hk, &hp, &cmd, &rep, &chz, &chv, &sync, &cap_i, &G_i, &lc_i, &stop_above};
    hipError_t le;
    {
        ProfScope ps(c, "linkage_hx", 0, 24.0 * (double)N * (double)N);
        le = hipLaunchCooperativeKernel(f, dim3(onex ? 8 * (G + 1) : G + 1), dim3(HX_T), args, dyn, c->stream);
    }
    if (le != hipSuccess) { (void)hipGetLastError(); *stopped = true; return SD_OK; }
    if (launched) *launched = true;
    unsigned h[8] = {0};
    HIPCHK(c, hipMemcpyAsync(h, sync, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stats["linkage_hx_stale_scans"].flops += (double)h[SYNC_ROUNDS];
    if (h[SYNC_TIMEOUT]) *stopped = true;                  // a hand-off timed out (or, one XCD: too few workgroups found themselves on XCC 0)
    if (merges_done) *merges_done = (int64_t)h[SYNC_MERGES];
    return SD_OK;
}
