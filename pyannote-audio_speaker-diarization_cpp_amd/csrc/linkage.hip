// linkage.hip -- Clustering::linkage (a12): pdist + scipy-generic linkage on the GPU           cl.cpp:289-440
// The driver: the preparation kernels (distance matrix, exact nearest neighbours, fills), the plan of one job and run_linkage, which takes the job through
// the four linkage kernels by their launchers (linkage_dev.h); each kernel lives in a file of its own (linkage_rg.hip, linkage_mw.hip, linkage_hx.hip,
// linkage_heap.hip).
//
// Design: the fp64 distance matrix -- the full N x N square while it fits (3.7 GB at N = 21 573), the condensed N(N-1)/2 form above -- stays resident in
// HBM.  k_pdist / k_pdist_sq build it from LDS tiles with the reference's sequential per-pair summation order.  The N-1 dependent merges run in one
// persistent kernel: from N = 1500 up a cooperative one (k_linkage_rg, k_linkage_mw) that replaces the reference's binary heap by a parallel arg-min over
// the per-row lower bounds on G co-resident workgroups and takes a merge only while the closest pair is unique; for small N and from the first exact tie
// on, one that replays the reference's heap operation by operation (k_linkage_hx, k_linkage_heap), so Z is bit-identical to the reference for every
// input, ties included.
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"
#include <cstring>

// ---------------------------------------------------------------- k_pdist (cl.cpp:408-431)
// The tile loop and the value of a pair are linkage_dev.h's pdist_tile and pdist_value (COS: the cosine metric); k_pdist_sq and k_pdist_jobs
// (linkage_batch.hip) call the same two.  A zero-norm row under the cosine metric raises *err (the reference throws, sd.cpp:493-495).
template <bool COS>
__global__ __launch_bounds__(256) void k_pdist(const double* __restrict__ X, int64_t N, int d, double* __restrict__ D, int* __restrict__ err)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;
    __shared__ double Xi[PT][33], Xj[PT][33];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4], ma[4], mb[4];
    pdist_tile<COS>(X, N, d, ti, tj, Xi, Xj, acc, ma, mb);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t i = (int64_t)ti * PT + ty + 16 * u, j = (int64_t)tj * PT + tx + 16 * v;
            if (i < j && j < N) {
                bool zero_norm = false;
                D[cidx(N, i, j)] = pdist_value<COS>(acc[u][v], ma[u], mb[v], &zero_norm);
                if (zero_norm) *err = 1;
            }
        }
}

// the same distances as the full N x N square (k_linkage_mw<*, true>, k_linkage_rg): linkage_dev.h's pdist_sq_tile, which k_pdist_sq_jobs (linkage_batch.hip) calls too
template <bool COS>
__global__ __launch_bounds__(256) void k_pdist_sq(const double* __restrict__ X, int64_t N, int d, double* __restrict__ D, int* __restrict__ err)
{
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj < ti) return;
    __shared__ double Xi[PT][33], Xj[PT][33];
    __shared__ double Tt[PT][PT + 1];
    pdist_sq_tile<COS>(X, N, d, ti, tj, D, err, Xi, Xj, Tt);
}

// exact nearest neighbour, bound and second bound above each row: a wave per row (row_min2, linkage_dev.h)
__global__ __launch_bounds__(256) void k_row_nn(const double* __restrict__ D, int64_t n, int* __restrict__ nb, double* __restrict__ md, double* __restrict__ md2, int square)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n - 1) return;
    const Min2 m = row_min2(D + (square ? x * n + x + 1 : cidx(n, x, x + 1)), n - 1 - x, x);
    if (lane == 0) { nb[x] = m.i; md[x] = (m.i < 0) ? INFINITY : m.v; if (md2) md2[x] = (m.i < 0) ? INFINITY : m.v2; }
}

// the same for a square matrix some merges into the job (run_linkage: k_linkage_hx merged the duplicates, k_linkage_rg continues): only clusters still there
// (size != 0), and entry {x, j} from the row that was written last
__global__ __launch_bounds__(256) void k_row_nn_mid(const double* __restrict__ D, int64_t n, const int* __restrict__ size, const int* __restrict__ ty,
                                                    int* __restrict__ nb, double* __restrict__ md, double* __restrict__ md2)
{
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n - 1) return;
    const Min2 m = row_min2_mid(D, n, size, ty, x);
    if (lane == 0) { nb[x] = m.i; md[x] = (m.i < 0) ? INFINITY : m.v; md2[x] = (m.i < 0) ? INFINITY : m.v2; }
}

__global__ void k_fill_i32(int* p, int v, int64_t n, int iota)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = iota ? (int)i : v;
}

// ---------------------------------------------------------------- run_linkage: the plan, then its steps
// X[N][d] (rows as given; Clustering::linkage does not normalise) -> Z[N-1][4] on the device
//   N < 1500 (or option linkage_wgs = 0): k_linkage_heap, the reference's algorithm heap included.
//   above: k_linkage_rg / k_linkage_mw on G co-resident workgroups (cooperative launch: the runtime guarantees residency or refuses).  They
//   take a merge from their parallel arg-min only while the closest pair is unique; at the first exact tie (duplicate embeddings), on a
//   refused launch or on a poll timeout the heap replay k_linkage_hx takes the job (a tie at height 0: only up to the first merge above 0,
//   then k_linkage_rg goes on), and k_linkage_heap where that cannot run.
//
// Geometry of one job, computed once from the size, the device and the linkage_* options.  The one input that is not arithmetic: whether the square
// matrix could be allocated (`square_ok` = false: the job takes the condensed form).  G <= 1: the one-workgroup heap kernel, the other fields unused.
struct LinkagePlan {
    int G, TH, cap, slot_gran;          // cooperative workgroups, threads of each, rows a workgroup owns + 1, granules of a slot
    bool square, use_rg, onex;          // full N x N matrix; k_linkage_rg (else k_linkage_mw); one XCD first
    bool replay, hx_onex; int workers;  // a tie can go to k_linkage_hx (square matrix, option linkage_tie_kernel, a geometry that fits): one XCD first, worker workgroups
};
static LinkagePlan linkage_plan(const sd_ctx* c, int64_t N, bool square_ok)
{
    LinkagePlan p = {};
    // the arithmetic is linkage_batch_plan.h's linkage_geometry, which run_linkage_many's planner shares
    const LinkageGeom g = linkage_geometry(linkage_opts(c), N, square_ok);
    p.G = g.G; p.TH = g.TH;
    if (g.G <= 1) return p;
    const bool square = g.square, use_rg = g.use_rg;
    p.cap = g.cap; p.square = g.square; p.use_rg = g.use_rg; p.onex = g.onex;
    p.slot_gran = use_rg ? linkage_rg_slot_granules() : linkage_mw_slot_granules();
    // (linkage_batch_plan.h too: run_linkage_many asks the same question of a job that ties inside an XCD launch)
    const LinkageTie t = linkage_tie_plan(c->linkage_tie_kernel, c->linkage_one_xcd, c->num_cu, N, square);
    p.replay = t.replay; p.workers = t.workers; p.hx_onex = t.hx_onex;
    return p;
}

// how the cooperative attempt ended
enum CoopEnd { COOP_DONE, COOP_TIE, COOP_TIMEOUT, COOP_REFUSED, COOP_ONEX_TIMEOUT };
struct CoopOutcome {
    CoopEnd end;
    bool onex;              // the form that ran: one XCD, or -- where that launch was refused -- all
    double tie_h;           // COOP_TIE of k_linkage_rg: the height of the tie
    bool untouched;         // matrix, bounds and ids are still as prepare() left them
};

// one job with its plan and its workspaces; the steps of run_linkage
struct LinkageJob {
    sd_ctx* c; const double* d_X; int64_t N; int d; double* d_Z;
    int method, metric;             // SD_LINKAGE_* (= LW_*), SD_METRIC_*
    LinkagePlan p;
    int* size; int* cid; int* nb; double* md; double* md2;
    double* D; MwGran* gran; unsigned* sync; int* size_all; int* tyv;

    // distance matrix (condensed or square) into Dm, sizes = 1, ids = iota, exact nearest neighbours above each row
    int prepare(double* Dm, bool square)
    {
        const int64_t m = N * (N - 1) / 2;
        const int tiles = (int)((N + PT - 1) / PT);
        {
            ProfScope ps(c, "pdist", (double)m * d * 3.0, (double)m * 8.0 * (square ? 2 : 1) + (double)N * d * 8.0);
            int* d_err = nullptr;
            if (metric == SD_METRIC_COSINE) {
                WS(c, int, e, "cl_err", 4);
                d_err = e;
                HIPCHK(c, hipMemsetAsync(d_err, 0, sizeof(int), c->stream));
                if (square) hipLaunchKernelGGL(k_pdist_sq<true>, dim3(tiles, tiles), dim3(256), 0, c->stream, d_X, N, d, Dm, d_err);
                else hipLaunchKernelGGL(k_pdist<true>, dim3(tiles, tiles), dim3(256), 0, c->stream, d_X, N, d, Dm, d_err);
            }
            else if (square) hipLaunchKernelGGL(k_pdist_sq<false>, dim3(tiles, tiles), dim3(256), 0, c->stream, d_X, N, d, Dm, d_err);
            else hipLaunchKernelGGL(k_pdist<false>, dim3(tiles, tiles), dim3(256), 0, c->stream, d_X, N, d, Dm, d_err);
            KCHECK(c);
            if (d_err) {            // no linkage kernel ever sees a NaN distance
                int herr = 0;
                HIPCHK(c, hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                if (herr) SD_FAIL(c, SD_ERR_NUMERIC, "linkage: zero-norm row under the cosine metric (reference throws, sd.cpp:493-495)");
            }
        }
        hipLaunchKernelGGL(k_fill_i32, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, size, 1, N, 0);
        hipLaunchKernelGGL(k_fill_i32, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, cid, 0, N, 1);
        KCHECK(c);
        ProfScope ps(c, "row_nn", 0, (double)m * 8.0);
        hipLaunchKernelGGL(k_row_nn, dim3((unsigned)((N - 1 + 3) / 4)), dim3(256), 0, c->stream, Dm, N, nb, md, md2, square ? 1 : 0);
        KCHECK(c);
        return SD_OK;
    }

    // k_linkage_rg or k_linkage_mw on the plan's geometry: one XCD first where the plan says so, then all.  `o` comes in as "refused, nothing touched".
    int coop(CoopOutcome& o)
    {
        {
            ProfScope ps(c, "linkage", 0, 24.0 * (double)N * (double)N);
            const int n_i = (int)N;
            // "has the kernel written anything?" is read from Z itself: row 0 is zeroed here and written (size field >= 2) right behind the first merge's
            // stores into D, before any later exit (linkage_rg.hip: write_Z follows the column pass, the row-tie check comes behind it).  Round 5 kept a
            // merge counter in a sync word of its own instead; those two stores in the kernel's exit paths changed its register allocation and cost 9 ms per hour
            // (profiles/r06_linkage_ab.txt: 76.2 -> 85.7 ms on one box, one process, interleaved).
            if (p.use_rg) HIPCHK(c, hipMemsetAsync(d_Z, 0, 4 * sizeof(double), c->stream));
            // cooperative launch: all workgroups are resident together, or the launch is refused (they poll each other's slots)
            auto launch = [&](bool onex) {
                return p.use_rg ? linkage_rg_launch(c, method, onex, p.G, p.TH, D, n_i, cid, nb, md, md2, d_Z, gran, sync, p.cap, (int)c->linkage_prefetch)
                                : linkage_mw_launch(c, onex, p.square, p.G, p.TH, D, n_i, size_all, cid, nb, md, md2, d_Z, gran, sync, p.cap);
            };
            hipError_t le = o.onex ? launch(true) : hipErrorUnknown;
            if (o.onex && le != hipSuccess) { (void)hipGetLastError(); o.onex = false; }
            if (!o.onex) le = launch(false);
            if (p.use_rg) c->stats["linkage_rg_launches"].launches += 1;
            if (le != hipSuccess) { (void)hipGetLastError(); return SD_OK; }
        }
        unsigned h[SYNC_HOST_WORDS] = {0};
        HIPCHK(c, hipMemcpyAsync(h, sync, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->stats["linkage_retry_rounds"].flops += (double)h[SYNC_ROUNDS];
        o.untouched = false;
        o.end = h[SYNC_TIMEOUT] ? (o.onex ? COOP_ONEX_TIMEOUT : COOP_TIMEOUT) : h[SYNC_TIE] ? COOP_TIE : COOP_DONE;
        if (o.end == COOP_TIE && p.use_rg) {      // stopped in front of its first merge (with two pairs of duplicates: always)?  Z's row 0, zeroed before the launch, is still zero
            double z03 = 1.0;
            HIPCHK(c, hipMemcpy(&z03, d_Z + 3, sizeof(double), hipMemcpyDeviceToHost));
            o.untouched = z03 == 0.0;
            const unsigned long long b = ((unsigned long long)h[SYNC_TIE_HI] << 32) | h[SYNC_TIE_LO];
            memcpy(&o.tie_h, &b, 8);
        }
        return SD_OK;
    }

    // The reference's heap replayed with the row work spread over worker workgroups (k_linkage_hx) on the square matrix, up to the first merge above
    // `stop_above`: one XCD first where the plan says so; refused there, or too few workgroups arrived: all XCDs, once.  *ran = false: stopped both times.
    // `untouched` (matrix, bounds and ids as prepare() left them: no second pdist) is consumed and kept up to date for the caller's next step.
    int replay(double stop_above, bool& untouched, bool* ran, int64_t* merges)
    {
        bool hx_onex = p.hx_onex; int workers = p.workers;
        *ran = false;
        for (int attempt = 0; attempt < 2; ++attempt) {
            if (int rc = untouched ? SD_OK : prepare(D, true)) return rc;
            untouched = false;
            hipLaunchKernelGGL(k_fill_i32, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, c->stream, tyv, -1, N, 0);
            KCHECK(c);
            bool stopped = false, launched = false;
            if (int rc = linkage_hx_run(c, method, hx_onex, workers, D, N, cid, size, tyv, nb, md, d_Z, &stopped, stop_above, merges, &launched)) return rc;
            if (!launched) { untouched = true; c->stats["linkage_hx_refused"].launches += 1; }      // a refused launch has not touched matrix, bounds or ids
            if (!stopped) { *ran = true; return SD_OK; }
            if (!hx_onex) break;
            hx_onex = false;                 // one XCD refused or too few workgroups arrived there: all XCDs
            workers = N >= 60000 ? 127 : 63;
            if (!linkage_hx_fits(N, workers)) break;
        }
        return SD_OK;
    }

    // after a zero phase of k_done merges: exact bounds of the rows still there (k_row_nn_mid), then k_linkage_rg continues from that state on the form the
    // first attempt ran on.  *done = false: refused, another tie or a poll timeout -- the whole replay takes the job.
    int continue_rg(bool onex, int64_t k_done, bool* done)
    {
        *done = false;
        {
            ProfScope ps(c, "row_nn", 0, (double)(N * (N - 1) / 2) * 8.0);
            hipLaunchKernelGGL(k_row_nn_mid, dim3((unsigned)((N - 1 + 3) / 4)), dim3(256), 0, c->stream, D, N, size, tyv, nb, md, md2);
            KCHECK(c);
        }
        HIPCHK(c, hipMemsetAsync(gran, 0, (size_t)2 * p.G * p.slot_gran * sizeof(MwGran), c->stream));
        HIPCHK(c, hipMemsetAsync(sync, 0, SYNC_WORDS * sizeof(unsigned), c->stream));
        hipError_t le;
        {
            ProfScope ps(c, "linkage", 0, 24.0 * (double)N * (double)N);
            le = linkage_rg_launch(c, method, onex, p.G, p.TH, D, (int)N, cid, nb, md, md2, d_Z, gran, sync, p.cap, (int)c->linkage_prefetch, (int)k_done, size, tyv);
            c->stats["linkage_rg_launches"].launches += 1;
        }
        if (le != hipSuccess) { (void)hipGetLastError(); return SD_OK; }
        unsigned h[SYNC_HOST_WORDS] = {0};
        HIPCHK(c, hipMemcpyAsync(h, sync, sizeof(h), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (!h[SYNC_TIMEOUT] && !h[SYNC_TIE]) { c->stats["linkage_zero_phase_jobs"].launches += 1; *done = true; return SD_OK; }
        if (c->profile_detail) fprintf(stderr, "linkage: zero phase (%lld merges), then %s -> whole replay\n", (long long)k_done, h[SYNC_TIE] ? "another tie" : "a poll timeout");
        return SD_OK;
    }

    // k_linkage_heap, the reference's algorithm on one workgroup, on the condensed matrix
    int one_workgroup()
    {
        WS(c, double, Dc, "cl_D", N * (N - 1) / 2);
        if (int rc = prepare(Dc, false)) return rc;
        return linkage_heap_run(c, method, Dc, N, size, cid, nb, md, d_Z);
    }
};

// (method and metric are validated where they enter: sd_linkage_ex / sd_cluster_ex and the option keys)
int run_linkage(sd_ctx* c, const double* d_X, int64_t N, int d, double* d_Z, int method, int metric)
{
    if (N < 2) return SD_OK;
    const int64_t m = N * (N - 1) / 2;
    if (N > 0x7fffffff / 4 || (double)m * 8.0 > 230e9) SD_FAIL(c, SD_ERR_ARG, "linkage: N=%lld needs a %.0f GB condensed matrix (limit 230 GB)", (long long)N, (double)m * 8e-9);
    WS(c, int, size, "cl_size", N);
    WS(c, int, cid, "cl_cid", N);
    WS(c, int, nb, "cl_nb", N);
    WS(c, double, md, "cl_md", N);
    WS(c, double, md2, "cl_md2", N);
    int rc;
    LinkageJob j = {c, d_X, N, d, d_Z, method, metric, linkage_plan(c, N, true), size, cid, nb, md, md2};
    LinkagePlan& p = j.p;
    if (p.G <= 1) return j.one_workgroup();
    if (p.square && !(j.D = ws_get<double>(c, "cl_Dsq", (size_t)N * N))) {      // no room for the square: the condensed form needs half
        (void)hipGetLastError(); c->stats["linkage_square_alloc_failed"].launches += 1;
        p = linkage_plan(c, N, false);
    }
    if (!p.square) { WS(c, double, Dc, "cl_D", m); j.D = Dc; }
    if (p.G > c->num_cu || p.G > linkage_mw_max_workgroups()) SD_FAIL(c, SD_ERR_ARG, "linkage: N=%lld needs %d cooperative workgroups", (long long)N, p.G);
    if ((rc = j.prepare(j.D, p.square))) return rc;
    // A method the cooperative kernel of this geometry is not built for counts as a refused launch: k_linkage_mw knows centroid only, k_linkage_rg the other
    // six on its 256-thread, 4-column form (linkage_rg_has) -- the replay kernels (k_linkage_hx, k_linkage_heap) know all seven on every geometry, so no
    // combination ever runs another method's formula.  Such a job needs none of the cooperative kernel's workspaces.
    const bool coop_has = p.use_rg ? linkage_rg_has(method, p.onex, p.G, p.TH, p.cap, (int)c->linkage_prefetch) : linkage_mw_has(method);
    if (!coop_has) c->stats["linkage_method_replays"].launches += 1;
    if (coop_has) {
        WS(c, MwGran, gran, "cl_gran", (int64_t)2 * p.G * p.slot_gran);
        HIPCHK(c, hipMemsetAsync(gran, 0, (size_t)2 * p.G * p.slot_gran * sizeof(MwGran), c->stream));
        j.gran = gran;
        if (!p.use_rg) {          // k_linkage_mw: per-workgroup private copies of sizes (and ty)
            if ((rc = linkage_mw_prepare(c, N, p.G, p.square, &j.size_all))) return rc;
        }
        WS(c, unsigned, sync, "cl_sync", SYNC_WORDS);
        HIPCHK(c, hipMemsetAsync(sync, 0, SYNC_WORDS * sizeof(unsigned), c->stream));
        j.sync = sync;
    }

    // 1. the cooperative kernel; a forced replay counts as a refused launch: nothing has run
    CoopOutcome o = {COOP_REFUSED, p.onex, 0.0, true};
    if (!c->linkage_force_heap && coop_has && (rc = j.coop(o))) return rc;
    if (o.end == COOP_DONE) return SD_OK;
    if (o.end == COOP_ONEX_TIMEOUT) {
        // too few workgroups found themselves on XCC 0 (dispatch not round-robin?): never again in this context; the
        // multi-XCD form does the job (the distance matrix is rebuilt by the recursive call)
        c->linkage_one_xcd = 0;
        c->stats["linkage_one_xcd_timeouts"].launches += 1;
        return run_linkage(c, d_X, N, d, d_Z, method, metric);
    }
    if (o.end == COOP_TIE) c->stats["linkage_tie_fallbacks"].launches += 1;
    c->stats["linkage_fallbacks"].launches += 1;
    const char* why = c->linkage_force_heap ? "forced (option linkage_force_heap)" : !coop_has ? "method not built into the cooperative kernel of this geometry" : o.end == COOP_REFUSED ? "cooperative launch refused" : o.end == COOP_TIMEOUT ? "slot poll timed out" : "exact tie";
    if (c->profile_detail) fprintf(stderr, "linkage: %s at N = %lld -> heap replay\n", why, (long long)N);

    if (p.replay) {
        WS(c, int, tyv, "cl_ty", N);
        j.tyv = tyv;
        bool untouched = o.untouched, ran = false;
        // 2. Ties at height 0 -- rows that occur twice, the usual reason for a tie -- end once the duplicates are merged.  The replay takes the merges at
        // height 0 only, and k_linkage_rg continues from that state (exact bounds of the rows still there from k_row_nn_mid); a later tie sends the whole
        // job through the replay, as before.  (Both kernels produce the reference's sequence: the replay always, k_linkage_rg while the closest pair is unique.)
        if (p.use_rg && o.end == COOP_TIE && o.tie_h == 0.0 && c->linkage_zero_phase != 0) {
            int64_t k_done = 0;
            if ((rc = j.replay(0.0, untouched, &ran, &k_done))) return rc;
            if (ran) {
                c->stats["linkage_zero_phase_merges"].flops += (double)k_done;
                if (k_done >= N - 1) { c->stats["linkage_hx_jobs"].launches += 1; return SD_OK; }
                bool done = false;
                if (k_done > 0 && (rc = j.continue_rg(o.onex, k_done, &done))) return rc;
                if (done) return SD_OK;
            }
        }
        // 3. the whole job through the replay
        if ((rc = j.replay((double)INFINITY, untouched, &ran, nullptr))) return rc;
        if (ran) { c->stats["linkage_hx_jobs"].launches += 1; return SD_OK; }
        c->stats["linkage_hx_failed"].launches += 1;
    }
    // 4. last resort.  The heap kernel works on the condensed matrix; the square one (up to 170 GB) is given back first, so that the fallback -- exact
    // ties are its designed trigger -- also fits right below the auto-square limit (the stream is idle: it was synchronised above)
    { auto it = c->ws.find("cl_Dsq"); if (it != c->ws.end()) it->second.release(); }
    return j.one_workgroup();
}
