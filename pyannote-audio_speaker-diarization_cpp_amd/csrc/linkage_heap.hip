// linkage_heap.hip -- k_linkage_heap: the reference's linkage (fast_linkage, cl.cpp:289-406) on ONE workgroup, its binary heap replayed operation by
// operation, on the condensed distance matrix; all seven methods.  run_linkage (linkage.hip) takes it for small N and as the last resort behind k_linkage_hx.
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"

// (scan_row_nn, the nearest-neighbour scan of a row, and the heap operations hp_* are linkage_dev.h's: k_linkage_heap_jobs shares them)
#define LT 1024
__device__ __forceinline__ MinIdx block_min(MinIdx m, MinIdx* sh)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    m = wave_min(m);
    __syncthreads();                 // sh may still be read from the previous use
    if (lane == 0) sh[w] = m;
    __syncthreads();
    MinIdx r = sh[0];
#pragma unroll
    for (int k = 1; k < LT / 64; ++k) r = better(r, sh[k]);
    return r;
}

// ---------------------------------------------------------------- k_linkage_heap : persistent single workgroup, the reference's heap included
// fast_linkage (cl.cpp:289-406) with its indexed binary min-heap (cl.cpp:28-119) kept bit for bit: thread 0 replays every
// Heap operation the reference performs, in the reference's order -- heapify (cl.cpp:94), get_min / change_value in the lazy
// validation loop (cl.cpp:323-339), remove_min (cl.cpp:340), change_value for the rows whose lower bound dropped IN ASCENDING z
// (cl.cpp:381-392), change_value for row y (cl.cpp:395-404) -- while the O(n) parts of a merge (Lance-Williams update, neighbour
// patches, nearest-neighbour scans) run on all threads.  Which of several rows with EXACTLY equal lower bounds the heap hands
// out first depends on the whole history of its array, so nothing short of replaying it reproduces the reference's merge
// order on data with ties (duplicate embeddings, lattice points); with it Z is bit-identical for any input.
// The heap (values / key_by_index / index_by_key) lives in LDS up to HEAP_LDS entries, in global memory above.
// The rows whose bound dropped are collected in an LDS bitmap and drained in ascending order by wave 0.
// (no __restrict__: every array here is written by one thread and re-read by others across barriers)
#define HEAP_LDS 2048
static_assert(HEAP_LDS == LINKAGE_HEAP_LDS, "linkage_batch_plan.h batches the jobs whose heap fits this kernel's LDS heap");
template <int METHOD>
__global__ __launch_bounds__(LT) void k_linkage_heap(double* D, int n, int* size, int* cid, int* nb, double* md, double* Z,
                                                      double* g_hval, int* g_hkey, int* g_hpos)
{
    extern __shared__ unsigned changed[];                 // bitmap of the rows whose bound dropped in this merge
    __shared__ MinIdx sh[LT / 64];
    __shared__ int s_ok, s_x, s_y;
    __shared__ double s_dist;
    __shared__ double s_hv[HEAP_LDS];
    __shared__ int s_hk[HEAP_LDS], s_hp[HEAP_LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t N = n;
    const bool in_lds = (n - 1) <= HEAP_LDS;
    HeapRef h;
    h.val = in_lds ? s_hv : g_hval; h.key = in_lds ? s_hk : g_hkey; h.pos = in_lds ? s_hp : g_hpos; h.size = n - 1;
    const int nwords = (n + 31) / 32;
    for (int i = tid; i < nwords; i += LT) changed[i] = 0u;
    for (int i = tid; i < n - 1; i += LT) { h.val[i] = md[i]; h.key[i] = i; h.pos[i] = i; }         // cl.cpp:80-91
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
            MinIdx q = scan_row_nn<4>(D, size, N, n, x, tid, LT);
            q = block_min(q, sh);
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
        for (int z0 = tid; z0 < n; z0 += LT * 4) {                   // 4 rows per thread: all their loads issued together
            double dzx[4], dzy[4], mdz[4]; int sz[4], nbz[4]; int64_t izy[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int z = z0 + u * LT;
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
                const int z = z0 + u * LT;
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
            MinIdx q = scan_row_nn<4>(D, size, N, n, y, tid, LT);
            q = block_min(q, sh);
            if (tid == 0 && q.i >= 0) { nb[y] = q.i; md[y] = q.v; hp_change(h, y, q.v); }
        }
        __syncthreads();
    }
}

// launcher (declared in linkage_dev.h): Dc = condensed matrix, nb / md = exact nearest neighbours above each row, size = 1, cid = iota (LinkageJob::prepare)
int linkage_heap_run(sd_ctx* c, int method, double* Dc, int64_t N, int* size, int* cid, int* nb, double* md, double* d_Z)
{
    double* hval = nullptr; int* hkey = nullptr; int* hpos = nullptr;
    if (N - 1 > HEAP_LDS) {
        WS(c, double, hv, "cl_hval", N);
        WS(c, int, hk, "cl_hkey", N);
        WS(c, int, hp, "cl_hpos", N);
        hval = hv; hkey = hk; hpos = hp;
    }
    ProfScope ps(c, "linkage_heap", 0, 24.0 * (double)N * (double)N);
    const bool known = lw_dispatch(method, [&](auto M) {
        hipLaunchKernelGGL(k_linkage_heap<M.value>, dim3(1), dim3(LT), (size_t)((N + 31) / 32) * sizeof(unsigned), c->stream, Dc, (int)N, size, cid, nb, md, d_Z, hval, hkey, hpos); });
    if (!known) SD_FAIL(c, SD_ERR_ARG, "k_linkage_heap: no linkage method %d", method);
    KCHECK(c);
    return SD_OK;
}
