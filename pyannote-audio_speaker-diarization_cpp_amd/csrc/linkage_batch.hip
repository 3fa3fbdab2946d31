// linkage_batch.hip -- run_linkage_many: the small linkage jobs of one call in shared launches, one workgroup per job.
// The jobs of a group call (sd_diarize_many*, sd_stream_turns_many) and of sd_linkage_many are independent; below N = 1500 run_linkage gives each of them
// to k_linkage_heap, one workgroup on one CU.  Here the jobs that would go there (linkage_batch_plan.h) are taken through the same three steps together:
//   k_pdist_jobs<COS>            the condensed distance matrices of all jobs, blockIdx.z = job; k_pdist's pdist_tile and pdist_value
//   k_prepare_jobs               sizes = 1, ids = iota, the exact nearest neighbour above each row by k_row_nn's rule
//   k_linkage_heap_jobs<M, T>    one workgroup of T threads per job: k_linkage_heap's heap_linkage, heap in LDS
// The distances and the merges of a job come from the same functions (linkage_dev.h) as on the single path, so its Z is the same bytes whatever else is in the launch.
// All three read a device table of LinkageDevJob; a job's error slot, raised by k_pdist_jobs for a zero-norm row under the cosine metric, stops the two
// kernels behind it for that job alone (no linkage kernel ever sees a NaN distance).
// Under option linkage_batch_xcd the jobs run_linkage would take to the one-XCD form of k_linkage_rg (1500 <= N < 16 000) share launches too:
//   k_pdist_sq_jobs<COS>         the square matrices of all jobs of a group, blockIdx.z = job; k_pdist_sq's pdist_sq_tile
//   k_prepare_sq_jobs            ids = iota, nearest neighbour, bound and second bound above each row by k_row_nn's row_min2
//   k_linkage_rg_jobs<M>         (linkage_rg.hip) up to eight jobs per cooperative launch, job x on the 32 CUs of XCD x: k_linkage_rg's own body
// A job that meets an exact tie there, or whose launch is refused or times out, goes through run_linkage alone afterwards.
// Under option linkage_batch_xcd_zero the jobs that tie at height 0 in front of their first merge (duplicate rows) stay in the batch instead:
//   k_prepare_zero_jobs          size = 1, ty = -1
//   k_linkage_hx_jobs<M>         (linkage_hx.hip) up to eight jobs per cooperative launch, job x on XCD x: k_linkage_hx's own body, the merges at height 0 only
//   k_row_nn_mid_jobs            the exact bounds of the rows still there, by k_row_nn_mid's row_min2_mid
//   k_linkage_rg_jobs<M, true>   k_linkage_rg's body from merge k0 on
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"
#include <algorithm>

struct LinkageDevJob {
    const double* X;        // [n][d] rows
    double* D;              // [n (n - 1) / 2] condensed matrix
    int* size; int* cid; int* nb;      // [n] each
    double* md;             // [n]
    double* Z;              // [n - 1][4]
    int n, err;             // rows; index of the job's error slot
};

// ---------------------------------------------------------------- k_pdist_jobs: k_pdist (linkage.hip) per job
template <bool COS>
__global__ __launch_bounds__(256) void k_pdist_jobs(const LinkageDevJob* __restrict__ jobs, int d, int* __restrict__ errs)
{
    const LinkageDevJob jb = jobs[blockIdx.z];
    const int64_t N = jb.n;
    const int tiles = (int)((N + PT - 1) / PT);
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti >= tiles || tj >= tiles || tj < ti) return;      // beyond this job's own tiles, or below the diagonal
    double* __restrict__ D = jb.D;
    __shared__ double Xi[PT][33], Xj[PT][33];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4], ma[4], mb[4];
    pdist_tile<COS>(jb.X, N, d, ti, tj, Xi, Xj, acc, ma, mb);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t i = (int64_t)ti * PT + ty + 16 * u, j = (int64_t)tj * PT + tx + 16 * v;
            if (i < j && j < N) {
                bool zero_norm = false;
                D[cidx(N, i, j)] = pdist_value<COS>(acc[u][v], ma[u], mb[v], &zero_norm);
                if (zero_norm) errs[jb.err] = 1;
            }
        }
}

// ---------------------------------------------------------------- k_prepare_jobs: the two k_fill_i32 launches and k_row_nn (linkage.hip) per job
// grid (row quads of the longest job, jobs), 256 threads: a wave per row.  A job has ceil((n - 1) / 4) * 256 >= n threads of its own for the fills.
// The nearest neighbour above row x: the minimum of D[x, x+1 ..] with the lowest column among equals -- what k_row_nn's min2 scan keeps in (v, i).
__global__ __launch_bounds__(256) void k_prepare_jobs(const LinkageDevJob* __restrict__ jobs, const int* __restrict__ errs)
{
    const LinkageDevJob jb = jobs[blockIdx.y];
    const int64_t n = jb.n;
    if ((int64_t)blockIdx.x * 4 >= n - 1 || errs[jb.err]) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) { jb.size[t] = 1; jb.cid[t] = (int)t; }
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n - 1) return;
    const double* row = jb.D + cidx(n, x, x + 1);
    const int64_t cnt = n - 1 - x;
    MinIdx m; m.v = INFINITY; m.i = -1;
    for (int64_t k = lane; k < cnt; k += 64) { const double v = row[k]; if (v < m.v) { m.v = v; m.i = (int)(x + 1 + k); } }
    m = wave_min(m);
    if (lane == 0) { jb.nb[x] = m.i; jb.md[x] = (m.i < 0) ? INFINITY : m.v; }
}

// ---------------------------------------------------------------- k_linkage_heap_jobs: k_linkage_heap (linkage_heap.hip) per job, T threads
// heap_linkage (linkage_dev.h) as k_linkage_heap calls it; what differs is where the arrays come from (the job table), that the heap is always in LDS (the
// planner batches n - 1 <= LINKAGE_HEAP_LDS only) and the thread count, on which nothing the function computes depends.
#define JOBS_CHANGED_WORDS ((LINKAGE_HEAP_LDS + 1 + 31) / 32)
template <int METHOD, int T>
__global__ __launch_bounds__(T) void k_linkage_heap_jobs(const LinkageDevJob* jobs, const int* errs)
{
    __shared__ unsigned changed[JOBS_CHANGED_WORDS];      // bitmap of the rows whose bound dropped in this merge
    __shared__ MinIdx sh[T / 64];
    __shared__ HeapShared s;
    __shared__ double s_hv[LINKAGE_HEAP_LDS];
    __shared__ int s_hk[LINKAGE_HEAP_LDS], s_hp[LINKAGE_HEAP_LDS];
    const LinkageDevJob jb = jobs[blockIdx.x];
    const int n = jb.n;
    if (n < 2 || n - 1 > LINKAGE_HEAP_LDS || errs[jb.err]) return;
    HeapRef h;
    h.val = s_hv; h.key = s_hk; h.pos = s_hp; h.size = n - 1;
    heap_linkage<METHOD, T>(jb.D, n, jb.size, jb.cid, jb.nb, jb.md, jb.Z, h, changed, sh, s);
}

// ---------------------------------------------------------------- the preparation of the jobs that run one per XCD (k_linkage_rg_jobs, linkage_rg.hip)
// k_pdist_sq_jobs<COS>: k_pdist_sq (linkage.hip) per job, blockIdx.z = job: pdist_sq_tile on the job's own N x N square
template <bool COS>
__global__ __launch_bounds__(256) void k_pdist_sq_jobs(const LinkageRgJob* __restrict__ jobs, int d, int* __restrict__ errs)
{
    const LinkageRgJob jb = jobs[blockIdx.z];
    const int64_t N = jb.n;
    const int tiles = (int)((N + PT - 1) / PT);
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti >= tiles || tj >= tiles || tj < ti) return;      // beyond this job's own tiles, or below the diagonal
    __shared__ double Xi[PT][33], Xj[PT][33];
    __shared__ double Tt[PT][PT + 1];
    pdist_sq_tile<COS>(jb.X, N, d, ti, tj, jb.D, errs + jb.err, Xi, Xj, Tt);
}

// k_prepare_sq_jobs: ids = iota and k_row_nn's scan (row_min2) on the square matrix per job: nb, md and md2 are the bits LinkageJob::prepare gives.  Grid as
// k_prepare_jobs.  (No size array: k_linkage_rg keeps the cluster sizes in registers, 1 each at a fresh start.)
__global__ __launch_bounds__(256) void k_prepare_sq_jobs(const LinkageRgJob* __restrict__ jobs, const int* __restrict__ errs)
{
    const LinkageRgJob jb = jobs[blockIdx.y];
    const int64_t n = jb.n;
    if ((int64_t)blockIdx.x * 4 >= n - 1 || errs[jb.err]) return;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < n) jb.cid[t] = (int)t;
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n - 1) return;
    const Min2 m = row_min2(jb.D + x * n + x + 1, n - 1 - x, x);
    if (lane == 0) { jb.nb[x] = m.i; jb.md[x] = (m.i < 0) ? INFINITY : m.v; jb.md2[x] = (m.i < 0) ? INFINITY : m.v2; }
}

// ---------------------------------------------------------------- the jobs that tie at height 0 inside an XCD launch (option linkage_batch_xcd_zero)
// k_prepare_zero_jobs: size = 1 and ty = -1 for the jobs of a zero launch (k_linkage_hx_jobs, linkage_hx.hip) -- what LinkageJob::prepare and ::replay fill for
// k_linkage_hx alone; the first launches keep neither array.  Grid (ceil(longest n / 256), jobs)
__global__ __launch_bounds__(256) void k_prepare_zero_jobs(const LinkageHxJob* __restrict__ jobs, const int* __restrict__ errs)
{
    const LinkageHxJob jb = jobs[blockIdx.y];
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < jb.n && !errs[jb.err]) { jb.size[t] = 1; jb.ty[t] = -1; }
}

// k_row_nn_mid_jobs: k_row_nn_mid (linkage.hip) per job, blockIdx.y = job, a wave per row: row_min2_mid over the clusters the zero launch left (sz0, ty0).
// nb, md and md2 are the bits LinkageJob::continue_rg gets.  Grid (row quads of the longest job, jobs)
__global__ __launch_bounds__(256) void k_row_nn_mid_jobs(const LinkageRgJob* __restrict__ jobs, const int* __restrict__ errs)
{
    const LinkageRgJob jb = jobs[blockIdx.y];
    const int64_t n = jb.n;
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= n - 1 || errs[jb.err]) return;
    const Min2 m = row_min2_mid(jb.D, n, jb.sz0, jb.ty0, x);
    if (lane == 0) { jb.nb[x] = m.i; jb.md[x] = (m.i < 0) ? INFINITY : m.v; jb.md2[x] = (m.i < 0) ? INFINITY : m.v2; }
}

// ---------------------------------------------------------------- the driver
// Threads per job: 256.  Measured (tools/linkage_many_times.py, profiles/linkage_many_times.txt; 64 jobs, one per CU): 2.24 ms at N = 100, 16.00 at 400 and
// 57.81 at 1000 with 256 threads against 2.20 / 16.66 / 58.12 with k_linkage_heap's 1024 -- no difference beyond the spread of the rounds: a merge is bound by
// the one thread that replays the heap and by the latency of a row's loads, not by the width of the scans.  256 it is, because a CU then holds four jobs
// (4 waves and 33 KB of LDS each) where it holds two of 1024 threads, which is what counts once a call has more jobs than the device has CUs.
static int linkage_batch_threads(const sd_ctx* c) { return c->linkage_batch_threads >= 1024 ? 1024 : 256; }

struct LinkageManyRun {
    sd_ctx* c; const LinkageManyJob* jobs; int d, method, metric; int32_t* status;
    bool xcd_off = false;       // a slot poll of k_linkage_rg_jobs timed out: no further launch of it in this call

    // the single route: run_linkage as it is, Z to the caller's rows.  SD_ERR_NUMERIC is the job's own status
    int single(int64_t j)
    {
        const LinkageManyJob& q = jobs[j];
        status[j] = SD_OK;
        if (q.N < 2) return SD_OK;
        WS(c, double, dZ, "cl_Z", (q.N - 1) * 4);
        const int rc = run_linkage(c, q.d_X, q.N, d, dZ, method, metric);
        if (rc == SD_ERR_NUMERIC) { status[j] = rc; return SD_OK; }
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(q.h_Z, dZ, (size_t)(q.N - 1) * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return SD_OK;
    }

    // jobs ord[0 .. G), longest first, in one set of launches.  Workspaces that cannot be allocated: the halves, down to single jobs
    int group(const int64_t* ord, int64_t G)
    {
        int64_t nD = 0, nI = 0, nM = 0, nZ = 0;
        for (int64_t k = 0; k < G; ++k) {
            const int64_t N = jobs[ord[k]].N;
            nD += N * (N - 1) / 2; nI += linkage_job_ints(N); nM += N; nZ += (N - 1) * 4;
        }
        double* D = ws_get<double>(c, "lb_D", (size_t)nD);
        int* I = D ? ws_get<int>(c, "lb_int", (size_t)nI) : nullptr;
        double* M = I ? ws_get<double>(c, "lb_md", (size_t)nM) : nullptr;
        double* Z = M ? ws_get<double>(c, "lb_Z", (size_t)nZ) : nullptr;
        LinkageDevJob* tab = Z ? ws_get<LinkageDevJob>(c, "lb_tab", (size_t)G) : nullptr;
        int* errs = tab ? ws_get<int>(c, "lb_err", (size_t)G) : nullptr;
        if (!errs) {
            (void)hipGetLastError();
            c->stats["linkage_batch_alloc_failed"].launches += 1;
            if (G == 1) return single(ord[0]);
            if (int rc = group(ord, G / 2)) return rc;
            return group(ord + G / 2, G - G / 2);
        }
        std::vector<LinkageDevJob> h((size_t)G);
        std::vector<double> hZ((size_t)nZ);
        std::vector<int> herr((size_t)G, 0);
        int64_t oD = 0, oI = 0, oM = 0, oZ = 0;
        for (int64_t k = 0; k < G; ++k) {
            const LinkageManyJob& q = jobs[ord[k]];
            const int64_t N = q.N, s = linkage_job_ints(N) / 3;
            h[(size_t)k] = LinkageDevJob{q.d_X, D + oD, I + oI, I + oI + s, I + oI + 2 * s, M + oM, Z + oZ, (int)N, (int)k};
            oD += N * (N - 1) / 2; oI += 3 * s; oM += N; oZ += (N - 1) * 4;
        }
        const int64_t longest = jobs[ord[0]].N;
        const int tiles = (int)((longest + PT - 1) / PT);
        HIPCHK(c, hipMemcpyAsync(tab, h.data(), (size_t)G * sizeof(LinkageDevJob), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(errs, 0, (size_t)G * sizeof(int), c->stream));
        {
            ProfScope ps(c, "pdist_jobs", (double)nD * d * 3.0, (double)nD * 8.0 + (double)nM * d * 8.0);
            if (metric == SD_METRIC_COSINE) hipLaunchKernelGGL(k_pdist_jobs<true>, dim3(tiles, tiles, (unsigned)G), dim3(256), 0, c->stream, tab, d, errs);
            else hipLaunchKernelGGL(k_pdist_jobs<false>, dim3(tiles, tiles, (unsigned)G), dim3(256), 0, c->stream, tab, d, errs);
            KCHECK(c);
        }
        {
            ProfScope ps(c, "row_nn_jobs", 0, (double)nD * 8.0);
            hipLaunchKernelGGL(k_prepare_jobs, dim3((unsigned)((longest - 1 + 3) / 4), (unsigned)G), dim3(256), 0, c->stream, tab, errs);
            KCHECK(c);
        }
        {
            ProfScope ps(c, "linkage_heap_jobs", 0, 24.0 * (double)nD * 2.0);
            const int T = linkage_batch_threads(c);
            const bool known = lw_dispatch(method, [&](auto Mth) {
                if (T == 1024) hipLaunchKernelGGL((k_linkage_heap_jobs<Mth.value, 1024>), dim3((unsigned)G), dim3(1024), 0, c->stream, tab, errs);
                else hipLaunchKernelGGL((k_linkage_heap_jobs<Mth.value, 256>), dim3((unsigned)G), dim3(256), 0, c->stream, tab, errs); });
            if (!known) SD_FAIL(c, SD_ERR_ARG, "k_linkage_heap_jobs: no linkage method %d", method);
            KCHECK(c);
        }
        HIPCHK(c, hipMemcpyAsync(hZ.data(), Z, (size_t)nZ * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(herr.data(), errs, (size_t)G * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        oZ = 0;
        for (int64_t k = 0; k < G; ++k) {
            const LinkageManyJob& q = jobs[ord[k]];
            const size_t nz = (size_t)(q.N - 1) * 4;
            if (herr[(size_t)k]) status[ord[k]] = SD_ERR_NUMERIC;      // zero-norm row under the cosine metric (the reference throws, sd.cpp:493-495): its Z stays as it was
            else { status[ord[k]] = SD_OK; memcpy(q.h_Z, hZ.data() + oZ, nz * sizeof(double)); }
            oZ += (int64_t)nz;
        }
        return SD_OK;
    }

    // Option linkage_batch_xcd_zero.  `open_k` / `open_j`: the jobs of an XCD group (numbers in the group, records `h`) that their first launch left
    // unfinished, and how it ended.  Those that stopped at a tie at height 0 in front of their first merge (linkage_xcd_zero_plan) go through run_linkage's three
    // steps for that case together, up to eight to a launch, one per XCD: k_linkage_hx_jobs takes the merges at height 0, k_row_nn_mid_jobs recomputes the exact
    // bounds of the rows still there, k_linkage_rg_jobs<M, true> continues.  finished[a] = 1: job open_k[a] is done and its Z is with the caller; every other is the
    // caller's to run again alone -- where LinkageJob::continue_rg falls through to the whole replay, and on a refused launch, a timeout or a refused allocation.
    int zero_launches(const int64_t* ord, const std::vector<LinkageRgJob>& h, const std::vector<int64_t>& open_k, const std::vector<LinkageXcdZeroJob>& open_j,
                      const int* errs, std::vector<char>& finished)
    {
        LinkageXcdZeroPlan zp;
        linkage_xcd_zero_plan(open_j.data(), (int64_t)open_j.size(),
                              LinkageXcdZeroOpts{c->linkage_batch_xcd_zero, c->linkage_zero_phase, c->linkage_tie_kernel, c->linkage_one_xcd, c->linkage_hx_wide, c->num_cu}, zp);
        auto finish = [&](size_t a) {            // Z to the caller's rows (the stream is synchronised by the caller of finish's last use)
            const LinkageManyJob& q = jobs[ord[open_k[a]]];
            status[ord[open_k[a]]] = SD_OK; finished[a] = 1;
            c->stats["linkage_xcd_zero_jobs"].launches += 1;
            return hipMemcpyAsync(q.h_Z, h[(size_t)open_k[a]].Z, (size_t)(q.N - 1) * 4 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        };
        int64_t za = 0;
        for (int64_t zb : zp.launch_end) {
            const int nj = (int)(zb - za);
            const int64_t first = za;
            za = zb;
            if (xcd_off) break;                  // a poll timed out in this call: what is left is redone alone
            const int workers = zp.workers[(size_t)first];
            const LinkageXcdKey key = open_j[(size_t)zp.order[(size_t)first]].key;
            int64_t nI = 0, nF = 0, maxN = 0;
            const int64_t nGr = linkage_xcd_zero_granules(workers);
            for (int i = 0; i < nj; ++i) {
                const int64_t N = open_j[(size_t)zp.order[(size_t)(first + i)]].N;
                nI += linkage_xcd_zero_ints(N, workers); nF += linkage_xcd_zero_doubles(N, workers); maxN = std::max(maxN, N);
            }
            int* I = ws_get<int>(c, "lx_zero_int", (size_t)nI);
            double* F = I ? ws_get<double>(c, "lx_zero_f64", (size_t)nF) : nullptr;
            MwGran* gr = F ? ws_get<MwGran>(c, "lx_zero_gran", (size_t)(nGr * LINKAGE_XCD_JOBS)) : nullptr;
            unsigned* zsync = gr ? ws_get<unsigned>(c, "lx_zero_sync", (size_t)LINKAGE_XCD_JOBS * SYNC_HOST_WORDS) : nullptr;
            LinkageHxJob* ztab = zsync ? ws_get<LinkageHxJob>(c, "lx_zero_tab", (size_t)LINKAGE_XCD_JOBS) : nullptr;
            LinkageRgJob* ctab = ztab ? ws_get<LinkageRgJob>(c, "lx_zero_cont", (size_t)LINKAGE_XCD_JOBS) : nullptr;
            if (!ctab) { (void)hipGetLastError(); c->stats["linkage_batch_alloc_failed"].launches += 1; continue; }
            // 1. the table
            std::vector<LinkageHxJob> zh((size_t)nj);
            size_t max_dyn = 0;
            int64_t oI = 0, oF = 0;
            for (int i = 0; i < nj; ++i) {
                const LinkageRgJob& r = h[(size_t)open_k[(size_t)zp.order[(size_t)(first + i)]]];
                const int64_t N = r.n, s = (N + 1) & ~(int64_t)1, cap = linkage_xcd_zero_cap(N, workers);
                bool s16; int lc; size_t dyn;
                linkage_hx_form(N, false, s16, lc, dyn);
                max_dyn = std::max(max_dyn, dyn);
                int* ip = I + oI; double* fp = F + oF;
                zh[(size_t)i] = LinkageHxJob{r.D, r.cid, ip, ip + s, r.nb, r.md, r.Z, fp, ip + 2 * s, ip + 3 * s, gr + i * nGr, gr + i * nGr + 16, ip + 4 * s, fp + N,
                                            zsync + i * SYNC_HOST_WORDS, (int)N, (int)cap, lc, r.err};
                oI += linkage_xcd_zero_ints(N, workers); oF += linkage_xcd_zero_doubles(N, workers);
            }
            HIPCHK(c, hipMemcpyAsync(ztab, zh.data(), (size_t)nj * sizeof(LinkageHxJob), hipMemcpyHostToDevice, c->stream));
            // 2. size = 1, ty = -1   3. granules and sync blocks
            hipLaunchKernelGGL(k_prepare_zero_jobs, dim3((unsigned)((maxN + 255) / 256), (unsigned)nj), dim3(256), 0, c->stream, ztab, errs);
            KCHECK(c);
            HIPCHK(c, hipMemsetAsync(gr, 0, (size_t)(nGr * nj) * sizeof(MwGran), c->stream));
            HIPCHK(c, hipMemsetAsync(zsync, 0, (size_t)nj * SYNC_HOST_WORDS * sizeof(unsigned), c->stream));
            // 4. the merges at height 0
            hipError_t le;
            {
                ProfScope ps(c, "linkage_hx_zero_jobs", 0, 24.0 * (double)maxN * (double)maxN * (double)nj);
                le = linkage_hx_jobs_launch(c, method, workers, ztab, nj, max_dyn, errs);
            }
            if (le != hipSuccess) { (void)hipGetLastError(); c->stats["linkage_hx_refused"].launches += 1; continue; }      // refused: nothing ran
            // 5. the sync words   6. who is done, who goes on
            unsigned hw[LINKAGE_XCD_JOBS * SYNC_HOST_WORDS] = {0};
            HIPCHK(c, hipMemcpyAsync(hw, zsync, (size_t)nj * SYNC_HOST_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            std::vector<LinkageRgJob> ch;        // the jobs of the continuation launch
            std::vector<size_t> ca;              // ... their places in open_k
            bool timeout = false;
            int cap_rg = 0;
            for (int i = 0; i < nj; ++i) {
                const size_t a = (size_t)zp.order[(size_t)(first + i)];
                const unsigned* w = hw + (size_t)i * SYNC_HOST_WORDS;
                c->stats["linkage_hx_stale_scans"].flops += (double)w[SYNC_ROUNDS];
                if (w[SYNC_TIMEOUT]) { timeout = true; continue; }
                const int64_t k_done = (int64_t)w[SYNC_MERGES], N = open_j[a].N;
                c->stats["linkage_xcd_zero_merges"].flops += (double)k_done;
                if (k_done >= N - 1) { HIPCHK(c, finish(a)); continue; }
                if (k_done <= 0) continue;
                LinkageRgJob r = h[(size_t)open_k[a]];
                r.sync = zsync + ch.size() * SYNC_HOST_WORDS; r.sz0 = zh[(size_t)i].size; r.ty0 = zh[(size_t)i].ty; r.k0 = (int)k_done;
                cap_rg = std::max(cap_rg, r.cap);
                ch.push_back(r); ca.push_back(a);
            }
            if (timeout) { xcd_off = true; c->stats["linkage_xcd_timeouts"].launches += 1; }
            // 7. exact bounds of the rows still there, then k_linkage_rg's body from merge k0 on
            if (!ch.empty() && !xcd_off) {
                const int nc = (int)ch.size();
                HIPCHK(c, hipMemcpyAsync(ctab, ch.data(), (size_t)nc * sizeof(LinkageRgJob), hipMemcpyHostToDevice, c->stream));
                {
                    ProfScope ps(c, "row_nn_mid_jobs", 0, (double)maxN * (double)maxN * 4.0 * (double)nc);
                    hipLaunchKernelGGL(k_row_nn_mid_jobs, dim3((unsigned)((maxN - 1 + 3) / 4), (unsigned)nc), dim3(256), 0, c->stream, ctab, errs);
                    KCHECK(c);
                }
                for (const LinkageRgJob& r : ch) HIPCHK(c, hipMemsetAsync(r.gran, 0, (size_t)2 * key.G * linkage_rg_slot_granules() * sizeof(MwGran), c->stream));
                HIPCHK(c, hipMemsetAsync(zsync, 0, (size_t)nc * SYNC_HOST_WORDS * sizeof(unsigned), c->stream));
                {
                    ProfScope ps(c, "linkage_rg_cont_jobs", 0, 24.0 * (double)maxN * (double)maxN * (double)nc);
                    le = linkage_rg_jobs_launch(c, method, key.G, key.TH, key.helper, ctab, nc, cap_rg, errs, true);
                }
                if (le != hipSuccess) (void)hipGetLastError();      // refused: redone alone
                else {
                    HIPCHK(c, hipMemcpyAsync(hw, zsync, (size_t)nc * SYNC_HOST_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    timeout = false;
                    for (int i = 0; i < nc; ++i) {
                        const unsigned* w = hw + (size_t)i * SYNC_HOST_WORDS;
                        c->stats["linkage_retry_rounds"].flops += (double)w[SYNC_ROUNDS];
                        if (w[SYNC_TIMEOUT]) timeout = true;
                        else if (!w[SYNC_TIE]) HIPCHK(c, finish(ca[(size_t)i]));
                    }
                    if (timeout) { xcd_off = true; c->stats["linkage_xcd_timeouts"].launches += 1; }
                }
            }
            HIPCHK(c, hipStreamSynchronize(c->stream));      // the finished jobs' Z has arrived; the workspaces are free for the next launch
        }
        return SD_OK;
    }

    // XCD-batched jobs xp.order[k0 .. k1) (of one group of the plan, or less), longest first: the preparation in shared launches, then k_linkage_rg_jobs on
    // every launch of the plan that lies in the range.  A job whose sync block shows neither a timeout nor a tie is done; any other -- an exact tie, a poll
    // timeout, a refused launch (all its jobs), a launch not made after a timeout -- is run again alone by run_linkage, from its rows, behind the group.
    // Workspaces that cannot be allocated: the halves, down to single jobs
    int xcd_group(const LinkageXcdPlan& xp, int64_t k0, int64_t k1)
    {
        const int64_t Gn = k1 - k0;
        const int64_t* ord = xp.order.data() + k0;
        int64_t nD = 0, nI = 0, nM = 0, nZ = 0, nG = 0;
        for (int64_t k = 0; k < Gn; ++k) {
            const int64_t N = jobs[ord[k]].N;
            nD += N * N; nI += linkage_xcd_ints(N); nM += 2 * N; nZ += (N - 1) * 4; nG += (int64_t)2 * xp.key[(size_t)(k0 + k)].G * linkage_rg_slot_granules();
        }
        double* D = ws_get<double>(c, "lx_D", (size_t)nD);
        int* I = D ? ws_get<int>(c, "lx_int", (size_t)nI) : nullptr;
        double* M = I ? ws_get<double>(c, "lx_md", (size_t)nM) : nullptr;
        double* Z = M ? ws_get<double>(c, "lx_Z", (size_t)nZ) : nullptr;
        MwGran* gran = Z ? ws_get<MwGran>(c, "lx_gran", (size_t)nG) : nullptr;
        unsigned* sync = gran ? ws_get<unsigned>(c, "lx_sync", (size_t)Gn * SYNC_HOST_WORDS) : nullptr;
        LinkageRgJob* tab = sync ? ws_get<LinkageRgJob>(c, "lx_tab", (size_t)Gn) : nullptr;
        int* errs = tab ? ws_get<int>(c, "lx_err", (size_t)Gn) : nullptr;
        if (!errs) {
            (void)hipGetLastError();
            c->stats["linkage_batch_alloc_failed"].launches += 1;
            if (Gn == 1) return single(ord[0]);
            if (int rc = xcd_group(xp, k0, k0 + Gn / 2)) return rc;
            return xcd_group(xp, k0 + Gn / 2, k1);
        }
        std::vector<LinkageRgJob> h((size_t)Gn);
        std::vector<double> hZ((size_t)nZ);
        std::vector<int> herr((size_t)Gn, 0);
        std::vector<unsigned> hs((size_t)Gn * SYNC_HOST_WORDS, 0u);
        std::vector<char> ran((size_t)Gn, 0);
        int64_t oD = 0, oI = 0, oM = 0, oZ = 0, oG = 0;
        for (int64_t k = 0; k < Gn; ++k) {
            const LinkageManyJob& q = jobs[ord[k]];
            const LinkageXcdKey& key = xp.key[(size_t)(k0 + k)];
            const int64_t N = q.N, s = linkage_xcd_ints(N) / 2;
            h[(size_t)k] = LinkageRgJob{q.d_X, D + oD, I + oI, I + oI + s, M + oM, M + oM + N, Z + oZ, gran + oG, sync + k * SYNC_HOST_WORDS, nullptr, nullptr,
                                        (int)N, (int)((N + key.G - 1) / key.G) + 1, (int)k, 0};
            oD += N * N; oI += 2 * s; oM += 2 * N; oZ += (N - 1) * 4; oG += (int64_t)2 * key.G * linkage_rg_slot_granules();
        }
        const int64_t longest = jobs[ord[0]].N;
        const int tiles = (int)((longest + PT - 1) / PT);
        HIPCHK(c, hipMemcpyAsync(tab, h.data(), (size_t)Gn * sizeof(LinkageRgJob), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(errs, 0, (size_t)Gn * sizeof(int), c->stream));
        HIPCHK(c, hipMemsetAsync(gran, 0, (size_t)nG * sizeof(MwGran), c->stream));
        HIPCHK(c, hipMemsetAsync(sync, 0, (size_t)Gn * SYNC_HOST_WORDS * sizeof(unsigned), c->stream));
        // option linkage_batch_xcd_zero: "has the kernel written anything?" is read from row 0 of a job's Z, as LinkageJob::coop reads it (size field >= 2 behind the first merge)
        const bool zero_on = c->linkage_batch_xcd_zero == 1;
        if (zero_on) HIPCHK(c, hipMemsetAsync(Z, 0, (size_t)nZ * sizeof(double), c->stream));
        {
            ProfScope ps(c, "pdist_sq_jobs", (double)(nD - nM / 2) / 2.0 * d * 3.0, (double)nD * 8.0 + (double)(nM / 2) * d * 8.0);
            if (metric == SD_METRIC_COSINE) hipLaunchKernelGGL(k_pdist_sq_jobs<true>, dim3(tiles, tiles, (unsigned)Gn), dim3(256), 0, c->stream, tab, d, errs);
            else hipLaunchKernelGGL(k_pdist_sq_jobs<false>, dim3(tiles, tiles, (unsigned)Gn), dim3(256), 0, c->stream, tab, d, errs);
            KCHECK(c);
        }
        {
            ProfScope ps(c, "row_nn_sq_jobs", 0, (double)nD * 4.0);
            hipLaunchKernelGGL(k_prepare_sq_jobs, dim3((unsigned)((longest - 1 + 3) / 4), (unsigned)Gn), dim3(256), 0, c->stream, tab, errs);
            KCHECK(c);
        }
        // the launches of the plan inside [k0, k1): the words the host reads of all sync blocks of a launch come back in one copy
        int64_t a = k0;
        for (int64_t end : xp.launch_end) {
            if (end <= k0) continue;
            const int64_t b = std::min(end, k1);
            if (a >= b || xcd_off) break;
            const LinkageXcdKey& key = xp.key[(size_t)a];
            int cap = 0;
            for (int64_t k = a; k < b; ++k) cap = std::max(cap, h[(size_t)(k - k0)].cap);
            hipError_t le;
            {
                ProfScope ps(c, "linkage_rg_jobs", 0, 24.0 * (double)jobs[ord[a - k0]].N * (double)jobs[ord[a - k0]].N * (double)(b - a));
                le = linkage_rg_jobs_launch(c, method, key.G, key.TH, key.helper, tab + (a - k0), (int)(b - a), cap, errs);
            }
            if (le != hipSuccess) (void)hipGetLastError();      // refused: nothing ran, every job of the launch goes the single route
            else {
                unsigned* hw = hs.data() + (size_t)(a - k0) * SYNC_HOST_WORDS;
                HIPCHK(c, hipMemcpyAsync(hw, sync + (a - k0) * SYNC_HOST_WORDS, (size_t)(b - a) * SYNC_HOST_WORDS * sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
                HIPCHK(c, hipStreamSynchronize(c->stream));
                bool timeout = false;
                for (int64_t k = a; k < b; ++k) {
                    ran[(size_t)(k - k0)] = 1;
                    c->stats["linkage_retry_rounds"].flops += (double)hw[(k - a) * SYNC_HOST_WORDS + SYNC_ROUNDS];
                    timeout = timeout || hw[(k - a) * SYNC_HOST_WORDS + SYNC_TIMEOUT] != 0;
                }
                if (timeout) { xcd_off = true; c->stats["linkage_xcd_timeouts"].launches += 1; }      // too few workgroups of some job found each other: not again in this call
            }
            a = b;
            if (b == k1) break;
        }
        HIPCHK(c, hipMemcpyAsync(hZ.data(), Z, (size_t)nZ * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(herr.data(), errs, (size_t)Gn * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<int64_t> redo;
        std::vector<int64_t> open_k;                 // jobs (numbers in the group) that neither failed nor finished, in plan order
        std::vector<LinkageXcdZeroJob> open_j;       // ... and how their first launch ended
        oZ = 0;
        for (int64_t k = 0; k < Gn; ++k) {
            const LinkageManyJob& q = jobs[ord[k]];
            const size_t nz = (size_t)(q.N - 1) * 4;
            const unsigned* hw = hs.data() + (size_t)k * SYNC_HOST_WORDS;
            if (herr[(size_t)k]) status[ord[k]] = SD_ERR_NUMERIC;      // zero-norm row under the cosine metric: its Z stays as it was (as in group())
            else if (ran[(size_t)k] && !hw[SYNC_TIMEOUT] && !hw[SYNC_TIE]) {
                status[ord[k]] = SD_OK; memcpy(q.h_Z, hZ.data() + oZ, nz * sizeof(double));
                c->stats["linkage_xcd_jobs"].launches += 1;
            }
            else if (!zero_on) redo.push_back(ord[k]);
            else {
                open_k.push_back(k);
                open_j.push_back(LinkageXcdZeroJob{q.N, xp.key[(size_t)(k0 + k)], ran[(size_t)k] != 0, hw[SYNC_TIMEOUT] != 0, hw[SYNC_TIE] != 0,
                                                   ((uint64_t)hw[SYNC_TIE_HI] << 32) | hw[SYNC_TIE_LO], hZ[(size_t)oZ + 3] == 0.0});
            }
            oZ += (int64_t)nz;
        }
        if (!open_k.empty()) {
            std::vector<char> finished(open_k.size(), 0);
            if (int rc = zero_launches(ord, h, open_k, open_j, errs, finished)) return rc;
            for (size_t a = 0; a < open_k.size(); ++a) if (!finished[a]) redo.push_back(ord[open_k[a]]);
        }
        for (int64_t j : redo) {
            c->stats["linkage_xcd_redone"].launches += 1;
            if (int rc = single(j)) return rc;
        }
        return SD_OK;
    }
};

bool linkage_job_shares_launches(const sd_ctx* c, int64_t N, int method)
{
    return linkage_job_batched(LinkageRoute{c->linkage_wgs, c->linkage_one_xcd, c->num_cu}, N) || linkage_job_xcd(linkage_xcd_opts(c, method), N);
}

// (method and metric are validated where they enter, as for run_linkage)
int run_linkage_many(sd_ctx* c, const LinkageManyJob* jobs, int64_t J, int d, int method, int metric, int32_t* status)
{
    std::vector<int64_t> N((size_t)J);
    for (int64_t j = 0; j < J; ++j) N[(size_t)j] = jobs[j].N;
    LinkageBatchPlan p;
    linkage_batch_plan(N.data(), J, LinkageRoute{c->linkage_wgs, c->linkage_one_xcd, c->num_cu}, c->linkage_batch_bytes, p);
    LinkageManyRun r = {c, jobs, d, method, metric, status, false};
    int64_t first = 0;
    for (int64_t end : p.group_end) {
        if (int rc = r.group(p.order.data() + first, end - first)) return rc;
        first = end;
    }
    // of the jobs left: those of the one-XCD cooperative class eight to a launch (option linkage_batch_xcd), the others as ever, in list order
    LinkageXcdPlan xp;
    linkage_xcd_plan(N.data(), p.single, linkage_xcd_opts(c, method), xp);
    first = 0;
    for (int64_t end : xp.group_end) {
        if (int rc = r.xcd_group(xp, first, end)) return rc;
        first = end;
    }
    for (int64_t j : xp.single) if (int rc = r.single(j)) return rc;
    return SD_OK;
}

extern "C" int sd_linkage_many(sd_ctx* c, const double* h_X, const int64_t* N, int64_t J, int d, int method, int metric, double* h_Z, int32_t* status)
{
    ENTER(c);
    if (!h_X || !N || !h_Z || !status || J < 1 || d <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_linkage_many: bad argument (J >= 1, d >= 1)");
    int64_t rows = 0;
    for (int64_t j = 0; j < J; ++j) {
        if (N[j] < 0 || N[j] > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "sd_linkage_many: job %lld has %lld rows", (long long)j, (long long)N[j]);
        rows += N[j];
        if (rows > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "sd_linkage_many: more than 2^31 - 1 rows in one call");
    }
    if (int rc = check_method_metric(c, method, metric)) return rc;
    DTMP(c, dx, (size_t)rows * d * sizeof(double));
    HIPCHK(c, hipMemcpyAsync(dx.p, h_X, (size_t)rows * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    std::vector<LinkageManyJob> jobs((size_t)J);
    int64_t r0 = 0, z0 = 0;
    for (int64_t j = 0; j < J; ++j) {
        jobs[(size_t)j] = LinkageManyJob{(const double*)dx.p + (size_t)r0 * d, N[j], h_Z + (size_t)z0 * 4};
        status[j] = SD_OK;
        r0 += N[j]; z0 += N[j] > 1 ? N[j] - 1 : 0;
    }
    const int rc = run_linkage_many(c, jobs.data(), J, d, method, metric, status);
    (void)hipStreamSynchronize(c->stream);      // dx goes away with this frame
    return rc;
}
