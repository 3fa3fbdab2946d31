// linkage_batch.hip -- run_linkage_many: the small linkage jobs of one call in shared launches, one workgroup per job.
// The jobs of a group call (sd_diarize_many*, sd_stream_turns_many) and of sd_linkage_many are independent; below N = 1500 run_linkage gives each of them
// to k_linkage_heap, one workgroup on one CU.  Here the jobs that would go there (linkage_batch_plan.h) are taken through the same three steps together:
//   k_pdist_jobs<COS>            the condensed distance matrices of all jobs, blockIdx.z = job; per pair the arithmetic of k_pdist
//   k_prepare_jobs               sizes = 1, ids = iota, the exact nearest neighbour above each row by k_row_nn's rule
//   k_linkage_heap_jobs<M, T>    one workgroup of T threads per job: the body of k_linkage_heap, heap in LDS
// The algorithm of a job is the one of the single path, statement for statement, so its Z is the same bytes whatever else is in the launch.
// All three read a device table of LinkageDevJob; a job's error slot, raised by k_pdist_jobs for a zero-norm row under the cosine metric, stops the two
// kernels behind it for that job alone (no linkage kernel ever sees a NaN distance).
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
#define PT 64
template <bool COS>
__global__ __launch_bounds__(256) void k_pdist_jobs(const LinkageDevJob* __restrict__ jobs, int d, int* __restrict__ errs)
{
    const LinkageDevJob jb = jobs[blockIdx.z];
    const int64_t N = jb.n;
    const int tiles = (int)((N + PT - 1) / PT);
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti >= tiles || tj >= tiles || tj < ti) return;      // beyond this job's own tiles, or below the diagonal
    const double* __restrict__ X = jb.X;
    double* __restrict__ D = jb.D;
    __shared__ double Xi[PT][33], Xj[PT][33];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4];
    double ma[4] = {0.0, 0.0, 0.0, 0.0}, mb[4] = {0.0, 0.0, 0.0, 0.0};      // COS: squared norms of the tile's rows
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    for (int q0 = 0; q0 < d; q0 += 32) {
        for (int e = tid; e < PT * 32; e += 256) {
            const int r = e >> 5, q = e & 31;
            int64_t gi = (int64_t)ti * PT + r; if (gi > N - 1) gi = N - 1;
            int64_t gj = (int64_t)tj * PT + r; if (gj > N - 1) gj = N - 1;
            const bool in = (q0 + q) < d;
            Xi[r][q] = in ? X[(size_t)gi * d + q0 + q] : 0.0;
            Xj[r][q] = in ? X[(size_t)gj * d + q0 + q] : 0.0;
        }
        __syncthreads();
        for (int q = 0; q < 32; ++q) {          // sequential in q: same summation order as the reference (and as k_pdist)
            double a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) { a[u] = Xi[ty + 16 * u][q]; b[u] = Xj[tx + 16 * u][q]; }
            if constexpr (COS) {
#pragma unroll
                for (int u = 0; u < 4; ++u) { ma[u] += a[u] * a[u]; mb[u] += b[u] * b[u]; }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) acc[u][v] += a[u] * b[v];
            } else {
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int v = 0; v < 4; ++v) { const double df = a[u] - b[v]; acc[u][v] += df * df; }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int64_t i = (int64_t)ti * PT + ty + 16 * u, j = (int64_t)tj * PT + tx + 16 * v;
            if (i < j && j < N) {
                if constexpr (COS) {
                    if (ma[u] == 0.0 || mb[v] == 0.0) { errs[jb.err] = 1; D[cidx(N, i, j)] = NAN; }
                    else D[cidx(N, i, j)] = 1.0 - (acc[u][v] / (sqrt(ma[u]) * sqrt(mb[v])));
                } else D[cidx(N, i, j)] = sqrt(acc[u][v]);
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
template <int T>
__device__ __forceinline__ MinIdx block_min_t(MinIdx m, MinIdx* sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    m = wave_min(m);
    __syncthreads();                 // sh may still be read from the previous use
    if (lane == 0) sh[w] = m;
    __syncthreads();
    MinIdx r = sh[0];
#pragma unroll
    for (int k = 1; k < T / 64; ++k) r = better(r, sh[k]);
    return r;
}

// fast_linkage (cl.cpp:289-406) with its heap replayed by thread 0, as k_linkage_heap does it (see there for the account of every step); what differs is
// where the arrays come from (the job table), that the heap is always in LDS (the planner batches n - 1 <= LINKAGE_HEAP_LDS only) and the thread count.
// Nothing the threads compute depends on T: the scans keep the lowest index among equal minima, the Lance-Williams update is per element, the rows whose
// bound dropped are drained in ascending order.
#define JOBS_CHANGED_WORDS ((LINKAGE_HEAP_LDS + 1 + 31) / 32)
template <int METHOD, int T>
__global__ __launch_bounds__(T) void k_linkage_heap_jobs(const LinkageDevJob* jobs, const int* errs)
{
    __shared__ unsigned changed[JOBS_CHANGED_WORDS];      // bitmap of the rows whose bound dropped in this merge
    __shared__ MinIdx sh[T / 64];
    __shared__ int s_ok, s_x, s_y;
    __shared__ double s_dist;
    __shared__ double s_hv[LINKAGE_HEAP_LDS];
    __shared__ int s_hk[LINKAGE_HEAP_LDS], s_hp[LINKAGE_HEAP_LDS];
    const LinkageDevJob jb = jobs[blockIdx.x];
    const int n = jb.n;
    if (n < 2 || n - 1 > LINKAGE_HEAP_LDS || errs[jb.err]) return;
    double* D = jb.D; int* size = jb.size; int* cid = jb.cid; int* nb = jb.nb; double* md = jb.md; double* Z = jb.Z;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t N = n;
    HeapRef h;
    h.val = s_hv; h.key = s_hk; h.pos = s_hp; h.size = n - 1;
    const int nwords = (n + 31) / 32;
    for (int i = tid; i < nwords; i += T) changed[i] = 0u;
    for (int i = tid; i < n - 1; i += T) { h.val[i] = md[i]; h.key[i] = i; h.pos[i] = i; }          // cl.cpp:80-91
    __syncthreads();
    if (tid == 0) for (int i = h.size / 2; i >= 0; --i) hp_down(h, i);                                // cl.cpp:94
    __syncthreads();
    for (int k = 0; k < n - 1; ++k) {
        int x = 0, y = 0; double dist = 0.0;
        for (int guard = 0; guard < n - k; ++guard) {                                                // cl.cpp:323
            if (tid == 0) {
                const int hx = h.key[0]; const double hd = h.val[0]; const int hy = nb[hx];          // get_min
                s_x = hx; s_y = hy; s_dist = hd;
                s_ok = (hy >= 0) && (hd == D[cidx(N, hx, hy)]);                                     // cl.cpp:329
            }
            __syncthreads();
            x = s_x; y = s_y; dist = s_dist;
            const int ok = s_ok;
            __syncthreads();
            if (ok) break;
            // stale candidate: row x's true nearest neighbour (cl.cpp:333-338)
            MinIdx q = scan_row_nn<4>(D, size, N, n, x, tid, T);
            q = block_min_t<T>(q, sh);
            y = q.i; dist = (q.i < 0) ? (double)INFINITY : q.v;
            if (tid == 0) { nb[x] = y; md[x] = dist; hp_change(h, x, dist); }
            __syncthreads();
        }
        if (tid == 0) { hp_swap(h, 0, h.size - 1); h.size -= 1; hp_down(h, 0); }                      // remove_min, cl.cpp:101-105
        if (y < 0) { if (tid == 0) Z[(size_t)k * 4 + 3] = NAN; return; }                             // cannot happen while two clusters are active
        const int nx = size[x], ny = size[y];
        __syncthreads();
        if (tid == 0) {
            int ix = cid[x], iy = cid[y];
            if (ix > iy) { const int t = ix; ix = iy; iy = t; }
            Z[(size_t)k * 4 + 0] = (double)ix; Z[(size_t)k * 4 + 1] = (double)iy;
            Z[(size_t)k * 4 + 2] = dist;       Z[(size_t)k * 4 + 3] = (double)(nx + ny);
            size[x] = 0; size[y] = nx + ny; cid[y] = n + k;
        }
        __syncthreads();
        for (int z0 = tid; z0 < n; z0 += T * 4) {                    // 4 rows per thread: all their loads issued together
            double dzx[4], dzy[4], mdz[4]; int sz[4], nbz[4]; int64_t izy[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int z = z0 + u * T;
                const int zc = (z < n && z != y) ? z : ((y > 0) ? 0 : 1);        // any valid row other than y
                izy[u] = cidx(N, zc, y);
                sz[u] = size[zc];
                dzx[u] = (zc == x) ? 0.0 : D[cidx(N, zc, x)];
                dzy[u] = D[izy[u]];
                const int zr = zc < n - 1 ? zc : n - 2;
                nbz[u] = nb[zr]; mdz[u] = md[zr];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int z = z0 + u * T;
                if (z >= n || z == y || sz[u] == 0) continue;
                const double nd = lw_update<METHOD>(dzx[u], dzy[u], dist, nx, ny, sz[u]);   // cl.cpp:367
                D[izy[u]] = nd;
                if (z < x && nbz[u] == x) nb[z] = y;                                    // cl.cpp:374-378
                if (z < y && nd < mdz[u]) { nb[z] = y; md[z] = nd; atomicOr(&changed[z >> 5], 1u << (z & 31)); }   // cl.cpp:381-392
            }
        }
        __syncthreads();
        // change_value(z, D[z,y]) for the rows whose bound dropped, ascending z (cl.cpp:381-392): wave 0 walks the bitmap
        if (tid < 64) {
            for (int w0 = 0; w0 < nwords; w0 += 64) {
                const int wi = w0 + lane;
                const unsigned wd = wi < nwords ? changed[wi] : 0u;
                unsigned long long live = __ballot(wd != 0u);
                if (wd != 0u) changed[wi] = 0u;
                while (live) {
                    const int l = __builtin_ctzll(live);
                    live &= live - 1;
                    unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)wd, l);
                    while (bits) {
                        const int z = (w0 + l) * 32 + __builtin_ctz(bits);
                        bits &= bits - 1;
                        if (lane == 0) hp_change(h, z, md[z]);
                    }
                }
            }
        }
        __syncthreads();
        if (y < n - 1) {                                                              // cl.cpp:395-404
            MinIdx q = scan_row_nn<4>(D, size, N, n, y, tid, T);
            q = block_min_t<T>(q, sh);
            if (tid == 0 && q.i >= 0) { nb[y] = q.i; md[y] = q.v; hp_change(h, y, q.v); }
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- the driver
// Threads per job: 256.  Measured (tools/linkage_many_times.py, profiles/linkage_many_times.txt; 64 jobs, one per CU): 2.24 ms at N = 100, 16.00 at 400 and
// 57.81 at 1000 with 256 threads against 2.20 / 16.66 / 58.12 with k_linkage_heap's 1024 -- no difference beyond the spread of the rounds: a merge is bound by
// the one thread that replays the heap and by the latency of a row's loads, not by the width of the scans.  256 it is, because a CU then holds four jobs
// (4 waves and 33 KB of LDS each) where it holds two of 1024 threads, which is what counts once a call has more jobs than the device has CUs.
static int linkage_batch_threads(const sd_ctx* c) { return c->linkage_batch_threads >= 1024 ? 1024 : 256; }

struct LinkageManyRun {
    sd_ctx* c; const LinkageManyJob* jobs; int d, method, metric; int32_t* status;

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
};

// (method and metric are validated where they enter, as for run_linkage)
int run_linkage_many(sd_ctx* c, const LinkageManyJob* jobs, int64_t J, int d, int method, int metric, int32_t* status)
{
    std::vector<int64_t> N((size_t)J);
    for (int64_t j = 0; j < J; ++j) N[(size_t)j] = jobs[j].N;
    LinkageBatchPlan p;
    linkage_batch_plan(N.data(), J, LinkageRoute{c->linkage_wgs, c->linkage_one_xcd, c->num_cu}, c->linkage_batch_bytes, p);
    LinkageManyRun r = {c, jobs, d, method, metric, status};
    int64_t first = 0;
    for (int64_t end : p.group_end) {
        if (int rc = r.group(p.order.data() + first, end - first)) return rc;
        first = end;
    }
    for (int64_t j : p.single) if (int rc = r.single(j)) return rc;
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
    if (method < SD_LINKAGE_SINGLE || method > SD_LINKAGE_WEIGHTED) SD_FAIL(c, SD_ERR_ARG, "unknown linkage method %d (SD_LINKAGE_SINGLE .. SD_LINKAGE_WEIGHTED)", method);
    if (metric != SD_METRIC_EUCLIDEAN && metric != SD_METRIC_COSINE) SD_FAIL(c, SD_ERR_ARG, "unknown metric %d (SD_METRIC_EUCLIDEAN, SD_METRIC_COSINE)", metric);
    if (metric == SD_METRIC_COSINE && (method == SD_LINKAGE_CENTROID || method == SD_LINKAGE_MEDIAN || method == SD_LINKAGE_WARD))
        SD_FAIL(c, SD_ERR_ARG, "centroid, median and ward linkage are defined for the euclidean metric only");
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
