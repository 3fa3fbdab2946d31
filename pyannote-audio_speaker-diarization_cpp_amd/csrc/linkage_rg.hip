// linkage_rg.hip -- k_linkage_rg: the cooperative centroid linkage (Clustering::linkage's fast_linkage, cl.cpp:289-406) with the
// per-column state in REGISTERS and everything a merge needs travelling in the slots.
//
// Same algorithm, same matrix layout and same exchange as k_linkage_mw<*, true> (linkage_mw.hip: full N x N distance matrix, a workgroup
// owns a contiguous range of COLUMNS, row y is rewritten and not mirrored, the current copy of an entry lives in the row of the cluster
// that was a merge's survivor last -- index `ty` --, two-level lower bounds, cooperative refresh of stale rows, 8-byte tagged granules),
// so Z is the same bit for bit.  What differs is where a merge round spends its time (profiles/r05_linkage_*.txt):
//   * a thread keeps the bound / second bound / neighbour / freshness / size / ty of its (at most 4) columns in registers; the pass
//     reads no LDS and the candidate it publishes carries the sizes and ty of BOTH clusters of its pair.  The merge that follows
//     therefore starts from what the digest hands over: no per-workgroup size / ty arrays in global memory, no dependent loads
//     (k_linkage_mw's prefetch_pair: the size loads were waited for in front of the row loads -- the loop-invariant part of the
//     Lance-Williams formula is hoisted above the pass) and no global copies of the bounds at all;
//   * the "second pair at the merge height" flag rides in the block reduction, Z is written by its one thread without a barrier, the
//     slot is published by one store instruction (lane w stores word w): one workgroup barrier between the pass and the publish
//     instead of four;
//   * a row without an active column above it gets the exact bound +inf at once (columns are only ever removed) instead of a stale
//     bound that costs a refresh round later.
// Ties: as k_linkage_mw, a merge is taken only while the closest pair is unique; otherwise sync[SYNC_TIE] is raised and run_linkage hands the
// job to the kernel that replays the reference's heap.
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_linkage_rg's fence-free slot exchange (sc1 loads / stores, 8-byte tagged granules) is written for gfx950 only"
#endif

#define RG_T_MAX 1024
#define RG_U 4            // columns per thread (register state): a workgroup owns at most 4 * blockDim.x columns
#define RG_KR 4           // stale rows refreshed per retry round
#define RG_GMAX 128       // workgroups
#define RG_SLOT 40        // granules between two slots
#define RG_CW 9           // words of a candidate: bound (2), row, neighbour, flags, size of row / of neighbour, ty of row / of neighbour
#define RG_QW 7           // words of a row partial: minimum (2), its column, second value (2), size and ty of that column's cluster
#define RG_MW 16          // merge round: candidate + NN(y) partial ("row x had a second pair at the merge height" is bit 2 of the candidate's flag word)
#define RG_ROWTIE 4

struct RCand { double v; int i, y, fl, szi, szy, tyi, tyy; };
struct RQ { double v; int i; double v2; int sz, ty; };

__device__ __forceinline__ RCand rc_none() { RCand c; c.v = INFINITY; c.i = -1; c.y = -1; c.fl = 0; c.szi = 0; c.szy = 0; c.tyi = -1; c.tyy = -1; return c; }
__device__ __forceinline__ RQ rq_none() { RQ q; q.v = INFINITY; q.i = -1; q.v2 = INFINITY; q.sz = 0; q.ty = -1; return q; }

// sequential accumulation of one row into a thread's running candidate (rules of cand_acc / cbetter, linkage_mw.hip)
__device__ __forceinline__ void rc_acc(RCand& m, double v, int z, int y, int fl, int szi, int szy, int tyi, int tyy)
{
    if (m.i < 0 || v < m.v) { m.v = v; m.i = z; m.y = y; m.fl = fl; m.szi = szi; m.szy = szy; m.tyi = tyi; m.tyy = tyy; }
    else if (v == m.v) {
        const int tie = (v < INFINITY) ? CAND_TIE : 0;
        if (z < m.i) { m.fl = fl | tie | (m.fl & CAND_TIE); m.i = z; m.y = y; m.szi = szi; m.szy = szy; m.tyi = tyi; m.tyy = tyy; }
        else m.fl |= tie;
    }
}
__device__ __forceinline__ RCand rc_better(RCand a, RCand b)
{
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    if (b.v < a.v) return b;
    if (b.v == a.v) {
        RCand r = (b.i < a.i) ? b : a;
        if (a.i != b.i && a.v < INFINITY) r.fl |= CAND_TIE | ((a.fl | b.fl) & CAND_TIE);
        return r;
    }
    return a;
}
// Wave minimum of doubles through 32-bit integer DPP steps.  A double's bits, sign-folded (negative: all bits flipped, else the sign bit
// set), order as unsigned integers exactly as the doubles do (no NaN here; -0 sorts below +0, which never meets it: distances are
// square roots of non-negative sums).  The high words go through six v_min_u32 DPP steps -- one instruction each, where v_min_f64 needs
// two DPP moves and a quarter-rate fp64 instruction per step --; only if several lanes share the smallest high word do the low words follow.
// Returns the minimum and the ballot of the lanes that hold exactly it.
__device__ __forceinline__ unsigned wave_min_u32(unsigned v)
{
    v = min(v, (unsigned)dppi<0xB1, 0xF>((int)v)); v = min(v, (unsigned)dppi<0x4E, 0xF>((int)v)); v = min(v, (unsigned)dppi<0x141, 0xF>((int)v));
    v = min(v, (unsigned)dppi<0x140, 0xF>((int)v)); v = min(v, (unsigned)dppi<0x142, 0xA>((int)v)); v = min(v, (unsigned)dppi<0x143, 0xC>((int)v));
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ double wave_argmin_d(double v, unsigned long long& mask)
{
    const unsigned h0 = (unsigned)__double2hiint(v), l0 = (unsigned)__double2loint(v);
    const unsigned sgn = (unsigned)((int)h0 >> 31);
    const unsigned hi = h0 ^ (sgn | 0x80000000u), lo = l0 ^ sgn;
    const unsigned mh = wave_min_u32(hi);
    const bool a = hi == mh;
    unsigned long long ma = __ballot(a);
    if (ma & (ma - 1)) { const unsigned ml = wave_min_u32(a ? lo : 0xffffffffu); ma = __ballot(a && lo == ml); }
    mask = ma;
    return readlane_d(v, __builtin_amdgcn_readfirstlane(__ffsll((long long)ma) - 1));
}
// wave arg-min: the minimum value, a ballot of the lanes that hold it, the winner's record by v_readlane (wave_min_c's rules)
__device__ __forceinline__ RCand wave_min_rc(RCand m)
{
    const bool has = m.i >= 0;
    RCand r = rc_none();
    if (__ballot(has) == 0ull) return r;
    unsigned long long mm;
    const double vmin = wave_argmin_d(has ? m.v : (double)INFINITY, mm);
    const bool at = has && ((mm >> (threadIdx.x & 63)) & 1ull);
    const unsigned long long mask = __ballot(at);
    if (mask == 0) return r;
    unsigned long long wm = mask;
    int extra = 0;
    if (mask & (mask - 1)) {
        const int ii = wave_min_i(at ? m.i : 0x7fffffff);
        wm = __ballot(at && m.i == ii);
        if (wm != mask && vmin < (double)INFINITY) extra = CAND_TIE;
    }
    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)wm) - 1);
    r.v = vmin; r.i = __builtin_amdgcn_readlane(m.i, l); r.y = __builtin_amdgcn_readlane(m.y, l);
    r.fl = __builtin_amdgcn_readlane(m.fl, l) | extra;
    r.szi = __builtin_amdgcn_readlane(m.szi, l); r.szy = __builtin_amdgcn_readlane(m.szy, l);
    r.tyi = __builtin_amdgcn_readlane(m.tyi, l); r.tyy = __builtin_amdgcn_readlane(m.tyy, l);
    return r;
}
__device__ __forceinline__ void rq_acc(RQ& m, double v, int j, int sz, int ty)       // ascending j
{
    if (v < m.v) { m.v2 = m.v; m.v = v; m.i = j; m.sz = sz; m.ty = ty; }
    else if (v < m.v2) m.v2 = v;
}
__device__ __forceinline__ RQ rq_merge(RQ a, RQ b)
{
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    const bool bw = b.v < a.v || (b.v == a.v && b.i < a.i);
    RQ r = bw ? b : a;
    r.v2 = fmin(bw ? a.v : b.v, fmin(a.v2, b.v2));
    return r;
}
__device__ __forceinline__ RQ wave_min_rq(RQ m)
{
    const bool has = m.i >= 0;
    RQ r = rq_none();
    if (__ballot(has) == 0ull) return r;
    unsigned long long mm;
    const double vmin = wave_argmin_d(has ? m.v : (double)INFINITY, mm);
    unsigned long long wm = __ballot(has && ((mm >> (threadIdx.x & 63)) & 1ull));
    if (wm == 0) return r;
    if (wm & (wm - 1)) {           // the same minimum in several lanes: the lowest column, as a sequential scan would find it
        const bool at = has && ((wm >> (threadIdx.x & 63)) & 1ull);
        const int ii = wave_min_i(at ? m.i : 0x7fffffff);
        wm = __ballot(at && m.i == ii);
    }
    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)wm) - 1);
    r.v = vmin; r.i = __builtin_amdgcn_readlane(m.i, l);
    r.sz = __builtin_amdgcn_readlane(m.sz, l); r.ty = __builtin_amdgcn_readlane(m.ty, l);
    // every lane but the winner's contributes its own minimum, the winner's lane its second value
    const bool win = (int)(threadIdx.x & 63) == l;
    unsigned long long m2;
    r.v2 = wave_argmin_d(win ? m.v2 : (has ? m.v : (double)INFINITY), m2);
    return r;
}
__device__ __forceinline__ unsigned lo32(double v) { return (unsigned)(unsigned long long)__double_as_longlong(v); }
__device__ __forceinline__ unsigned hi32(double v) { return (unsigned)((unsigned long long)__double_as_longlong(v) >> 32); }
__device__ __forceinline__ unsigned rq_word(const RQ& q, int k)      // word k of a row partial
{
    return k == 0 ? lo32(q.v) : k == 1 ? hi32(q.v) : k == 2 ? (unsigned)q.i : k == 3 ? lo32(q.v2) : k == 4 ? hi32(q.v2) : k == 5 ? (unsigned)q.sz : (unsigned)q.ty;
}

// TB = launch bound (256 / 512 / 1024 threads): the register budget follows it -- 128 VGPRs at 1024 threads spill part of the column state
template <bool ONEX, int TB, int UU, int METHOD>
__global__ __launch_bounds__(TB) void k_linkage_rg(double* D, int n, int* cid, const int* nb0, const double* md0, const double* md20, double* Z,
                                                         MwGran* gran /*[2][G][RG_SLOT], zeroed*/, unsigned* sync, int cap /*columns per workgroup + 1*/, int G, int helper,
                                                         int k0 /*merges already done*/, const int* sz0, const int* ty0 /*cluster size (0 = gone) / last rewrite of every column after k0 merges; null: a fresh start*/)
{
    constexpr unsigned rg_xcc = 0;      // the one-XCD form runs on XCC 0
#include "linkage_rg_body.inc"
}

// The batched twin of k_linkage_rg<true, 256, RG_U, METHOD>: 8 G workgroups, up to 8 fresh jobs, job x on XCD x.  A workgroup reads the XCC it sits
// on; with a job of that number it runs k_linkage_rg's own body (linkage_rg_body.inc) on that job's matrix, slots and sync block: the ticket it takes there is
// the job's, and with one below G it is that rank, on the geometry (G, threads, cap) the job has alone, so its Z is the same bytes.  The plain-store exchange
// (STX<true>) needs every participant of a job on one XCD's L2: each of them has read that it sits on XCC x.  How the dispatcher deals the workgroups decides
// only whether G of them arrive; if not, the bounded poll ends that job alone (SYNC_TIMEOUT in its block) and the host runs it again by itself.  A raised error
// slot (a zero-norm row under the cosine metric): nobody touches the job.
// CONT = false starts every job fresh (k0 = 0, no sz0 / ty0: the first launches).  CONT = true is the continuation launch behind k_linkage_hx_jobs:
// a job goes on from the k0 merges the heap replay made at height 0, with the cluster sizes and last rewrites it left (sz0, ty0) and the bounds k_row_nn_mid_jobs
// recomputed -- what LinkageJob::continue_rg hands k_linkage_rg alone, on the same body, G, threads and cap.
template <int METHOD, bool CONT>
__global__ __launch_bounds__(256) void k_linkage_rg_jobs(const LinkageRgJob* __restrict__ jobs, int nj, int G, int helper, const int* __restrict__ errs)
{
    __shared__ int s_job;
    if (threadIdx.x == 0) {
        const int xcc = (int)__builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));       // HW_REG_XCC_ID[3:0]
        s_job = (xcc < nj && jobs[xcc].n >= 2 && !errs[jobs[xcc].err]) ? xcc : -1;
    }
    __syncthreads();
    if (s_job < 0) return;
    const LinkageRgJob jb = jobs[s_job];
    const unsigned rg_xcc = (unsigned)s_job;
    constexpr bool ONEX = true;
    constexpr int UU = RG_U;
    double* D = jb.D; const int n = jb.n; int* cid = jb.cid; const int* nb0 = jb.nb; const double* md0 = jb.md; const double* md20 = jb.md2; double* Z = jb.Z;
    MwGran* gran = jb.gran; unsigned* sync = jb.sync; const int cap = jb.cap;
    const int k0 = CONT ? jb.k0 : 0; const int* const sz0 = CONT ? jb.sz0 : nullptr; const int* const ty0 = CONT ? jb.ty0 : nullptr;
#include "linkage_rg_body.inc"
}

// launcher: false = the geometry does not fit this kernel (the caller takes k_linkage_mw)
static_assert(RG_GMAX == LINKAGE_RG_GMAX && RG_U == LINKAGE_RG_U && RG_T_MAX == LINKAGE_RG_T_MAX && RG_SLOT == LINKAGE_RG_SLOT, "linkage_batch_plan.h plans with these limits");
bool linkage_rg_fits(int64_t N, int G, int TH) { return linkage_rg_fits_geom(N, G, TH); }
// The kernel for a method and a geometry, and the threads it is launched with (the helper wave included); null: not built.  Every (threads, columns per
// thread) form exists for centroid, the default and the measured one; the other six methods are built for the 256-thread, 4-column form only (every
// automatic geometry up to 131 072 rows), to bound build time -- run_linkage sends any other job of theirs to the heap replay.
static const void* rg_kernel(int method, bool onex, int G, int TH, int cap, int& helper, int& TT)
{
    bool wide;                                               // more than 4 columns per thread: the 8-column form
    linkage_rg_form(G, TH, cap, helper, TT, wide);
    constexpr int CEN = LW_CENTROID;
    if (method == LW_CENTROID)
        return wide ? (TT <= 256 ? (onex ? (const void*)k_linkage_rg<true, 256, 8, CEN> : (const void*)k_linkage_rg<false, 256, 8, CEN>)
                                 : (onex ? (const void*)k_linkage_rg<true, 512, 8, CEN> : (const void*)k_linkage_rg<false, 512, 8, CEN>))
             : TT <= 256 ? (onex ? (const void*)k_linkage_rg<true, 256, RG_U, CEN> : (const void*)k_linkage_rg<false, 256, RG_U, CEN>)
             : TT <= 512 ? (onex ? (const void*)k_linkage_rg<true, 512, RG_U, CEN> : (const void*)k_linkage_rg<false, 512, RG_U, CEN>)
                         : (onex ? (const void*)k_linkage_rg<true, 1024, RG_U, CEN> : (const void*)k_linkage_rg<false, 1024, RG_U, CEN>);
    const void* f = nullptr;
    if (!wide && TT <= 256)
        lw_dispatch(method, [&](auto M) {
            f = onex ? (const void*)k_linkage_rg<true, 256, RG_U, M.value> : (const void*)k_linkage_rg<false, 256, RG_U, M.value>; });
    return f;
}
bool linkage_rg_has(int method, bool onex, int G, int TH, int cap, int helper)
{
    int TT;
    return rg_kernel(method, onex, G, TH, cap, helper, TT) != nullptr;
}
hipError_t linkage_rg_launch(sd_ctx* c, int method, bool onex, int G, int TH, double* D, int n, int* cid, const int* nb, const double* md, const double* md2,
                             double* Z, MwGran* gran, unsigned* sync, int cap, int helper, int k0, const int* sz0, const int* ty0)
{
    int TT;
    const void* f = rg_kernel(method, onex, G, TH, cap, helper, TT);
    const size_t dyn = (((size_t)cap * 9) + 15) & ~(size_t)15;
    if (!f) return hipErrorInvalidValue;          // (linkage_rg_has said so before)
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    (void)hipGetLastError();
    void* args[] = {&D, &n, &cid, &nb, &md, &md2, &Z, &gran, &sync, &cap, &G, &helper, &k0, &sz0, &ty0};
    // cooperative launch: all workgroups are resident together, or the launch is refused (they poll each other's slots)
    return hipLaunchCooperativeKernel(f, dim3(onex ? 8 * G : G), dim3(TT), args, dyn, c->stream);
}
// the caller (run_linkage_many) has planned the launch with linkage_job_xcd: the 256-thread, 4-column form, G <= 32, the helper wave counted in TH + 64 <= 256
hipError_t linkage_rg_jobs_launch(sd_ctx* c, int method, int G, int TH, int helper, const LinkageRgJob* d_jobs, int nj, int max_cap, const int* d_errs, bool cont)
{
    int TT; bool wide;
    linkage_rg_form(G, TH, max_cap, helper, TT, wide);
    const void* f = nullptr;
    if (!wide && TT <= 256 && G >= 2 && G <= 32 && nj >= 1 && nj <= LINKAGE_XCD_JOBS)
        lw_dispatch(method, [&](auto M) { f = cont ? (const void*)k_linkage_rg_jobs<M.value, true> : (const void*)k_linkage_rg_jobs<M.value, false>; });
    if (!f) return hipErrorInvalidValue;
    const size_t dyn = (((size_t)max_cap * 9) + 15) & ~(size_t)15;      // the largest job's; a job lays its own cap out in it
    (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    (void)hipGetLastError();
    void* args[] = {&d_jobs, &nj, &G, &helper, &d_errs};
    // cooperative launch: all workgroups are resident together, or the launch is refused (the workgroups of a job poll each other's slots)
    return hipLaunchCooperativeKernel(f, dim3(8 * G), dim3(TT), args, dyn, c->stream);
}
int linkage_rg_slot_granules() { return RG_SLOT; }
