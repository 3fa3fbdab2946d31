// linkage_dev.h -- device helpers shared by the linkage kernels (k_linkage_rg, k_linkage_mw, k_linkage_hx, k_linkage_heap: one file each, linkage_<name>.hip)
// and their batch forms (linkage_batch.hip), the preparation kernels (linkage.hip), the words of the `sync` block they and the host talk through, and the launchers run_linkage (linkage.hip) drives.
// Translation units that include this file are compiled with -ffp-contract=off (Makefile EXACT; exact_fp.h refuses any other build): fp64 results
// bit-identical to the reference's x86 build.
#pragma once
#include "common.h"
#include "exact_fp.h"
#include "cosine_rule.h"
#include "linkage_batch_plan.h"
#include <cfloat>
#include <cmath>
#include <type_traits>

__host__ __device__ __forceinline__ int64_t cidx(int64_t n, int64_t i, int64_t j)     // cl.cpp:236-242
{
    if (i < j) return n * i - (i * (i + 1) / 2) + (j - i - 1);
    return n * j - (j * (j + 1) / 2) + (i - j - 1);
}

// ---------------------------------------------------------------- one tile of pairwise distances (cl.cpp:408-431): k_pdist, k_pdist_sq, k_pdist_jobs
// 256 threads take the PT x PT tile (ti, tj) of rows of X[N][d]: thread (ty, tx) = (tid >> 4, tid & 15) accumulates the 4 x 4 pairs of rows
// ti * PT + ty + 16 u and tj * PT + tx + 16 v through the LDS stages Xi / Xj, sequential in q: the summation order of the reference.  COS: acc holds the
// dot products, ma / mb the squared norms of the thread's rows (one row each, kept once per row of the tile: the same sums a per-pair loop would form);
// else acc holds the sums of squared differences and ma / mb stay 0.  Rows past N - 1 are read as row N - 1; the caller stores only pairs inside N.
#define PT 64
template <bool COS>
__device__ __forceinline__ void pdist_tile(const double* __restrict__ X, int64_t N, int d, int ti, int tj, double (&Xi)[PT][33], double (&Xj)[PT][33],
                                           double (&acc)[4][4], double (&ma)[4], double (&mb)[4])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        ma[u] = 0.0; mb[u] = 0.0;
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[u][v] = 0.0;
    }
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
        for (int q = 0; q < 32; ++q) {          // sequential in q: same summation order as the reference
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
}
// the distance of one pair from its sums.  COS: the reference's own cosine rule (cosine_rule.h; Clustering.py:317-333 runs the single / complete / average /
// weighted linkages on it), *zero_norm raised for a zero-norm row (the reference throws, sd.cpp:493-495); else the euclidean distance, zero_norm unused
template <bool COS>
__device__ __forceinline__ double pdist_value(double acc, double ma, double mb, bool* zero_norm)
{
    if constexpr (COS) return cosine_distance(acc, ma, mb, zero_norm);
    else return sqrt(acc);
}

// the same distances as the full N x N square: k_pdist_sq, k_pdist_sq_jobs.  Tile (ti, tj), ti <= tj, is computed once and written twice, the
// mirror through the LDS transpose Tt so that both writes are row-contiguous.  D[i][j] and D[j][i] are the same bits; the diagonal is 0.
// The whole workgroup (256 threads) calls it; a zero-norm row under the cosine metric raises *err.
template <bool COS>
__device__ __forceinline__ void pdist_sq_tile(const double* __restrict__ X, int64_t N, int d, int ti, int tj, double* __restrict__ D, int* __restrict__ err,
                                              double (&Xi)[PT][33], double (&Xj)[PT][33], double (&Tt)[PT][PT + 1])
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    double acc[4][4], ma[4], mb[4];
    pdist_tile<COS>(X, N, d, ti, tj, Xi, Xj, acc, ma, mb);
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int li = ty + 16 * u, lj = tx + 16 * v;
            const int64_t i = (int64_t)ti * PT + li, j = (int64_t)tj * PT + lj;
            double dv;
            if constexpr (COS) {
                dv = 0.0;
                if (i != j && i < N && j < N) {
                    bool zero_norm = false;
                    dv = pdist_value<true>(acc[u][v], ma[u], mb[v], &zero_norm);
                    if (zero_norm) *err = 1;
                }
            } else dv = (i == j) ? 0.0 : pdist_value<false>(acc[u][v], ma[u], mb[v], nullptr);
            Tt[li][lj] = dv;
            if (i < N && j < N && (ti != tj || i <= j)) D[(size_t)i * N + j] = dv;
        }
    __syncthreads();
    for (int e = tid; e < PT * PT; e += 256) {
        const int lj = e >> 6, li = e & 63;                 // consecutive threads: consecutive i = consecutive addresses of row j
        const int64_t i = (int64_t)ti * PT + li, j = (int64_t)tj * PT + lj;
        if (i < N && j < N && i < j) D[(size_t)j * N + i] = Tt[li][lj];
    }
}

// ---------------------------------------------------------------- nearest active neighbour above a row (cl.cpp:259-276)
struct MinIdx { double v; int i; };
__device__ __forceinline__ MinIdx better(MinIdx a, MinIdx b)
{
    // smaller value wins; equal values -> lower index (== "first strictly smaller" of a sequential scan); -1 = none
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    if (b.v < a.v) return b;
    if (b.v == a.v && b.i < a.i) return b;
    return a;
}
// Wave-wide reductions with DPP lane moves (quad swaps, half-mirror, mirror, row broadcasts) instead of
// ds_bpermute shuffles: the dependent chain is ~10x shorter, and these reductions sit on the serial path of
// every merge.  All 64 lanes must be active.  The result (in lane 63 after the last step) is returned to all lanes.
template <int CTRL, int RM> __device__ __forceinline__ int dppi(int x) { return __builtin_amdgcn_update_dpp(x, x, CTRL, RM, 0xF, false); }
template <int CTRL, int RM> __device__ __forceinline__ double dppd(double v)
{
    const int lo = dppi<CTRL, RM>(__double2loint(v)), hi = dppi<CTRL, RM>(__double2hiint(v));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_d(double v, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
// Wave minimum in two moves instead of six (value, index) butterfly steps of ~12 dependent instructions each: the minimum VALUE
// first (v_min_f64 over DPP moves), then a ballot of the lanes that hold it.  One lane in the ballot (the rule on data without
// ties): its index is read with v_readlane.  Several: the lowest index among them, as `better` decides.  Same result as the
// butterfly for every input without NaN (distances are never NaN here).
__device__ __forceinline__ double wave_min_d(double v)
{
    v = fmin(v, dppd<0xB1, 0xF>(v)); v = fmin(v, dppd<0x4E, 0xF>(v)); v = fmin(v, dppd<0x141, 0xF>(v)); v = fmin(v, dppd<0x140, 0xF>(v));
    v = fmin(v, dppd<0x142, 0xA>(v)); v = fmin(v, dppd<0x143, 0xC>(v));
    return readlane_d(v, 63);
}
__device__ __forceinline__ int wave_min_i(int v)
{
    v = min(v, dppi<0xB1, 0xF>(v)); v = min(v, dppi<0x4E, 0xF>(v)); v = min(v, dppi<0x141, 0xF>(v)); v = min(v, dppi<0x140, 0xF>(v));
    v = min(v, dppi<0x142, 0xA>(v)); v = min(v, dppi<0x143, 0xC>(v));
    return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ MinIdx wave_min(MinIdx m)
{
    const bool has = m.i >= 0;
    const double vmin = wave_min_d(has ? m.v : (double)INFINITY);
    const bool at = has && m.v == vmin;
    const unsigned long long mask = __ballot(at);
    MinIdx r; r.v = INFINITY; r.i = -1;
    if (mask == 0) return r;
    r.v = vmin;
    if (mask & (mask - 1)) r.i = wave_min_i(at ? m.i : 0x7fffffff);
    else r.i = __builtin_amdgcn_readlane(m.i, __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1));
    return r;
}
// the same over a workgroup of T threads, all of them calling; sh: T / 64 entries of LDS.  Every thread returns the workgroup's minimum
template <int T>
__device__ __forceinline__ MinIdx block_min(MinIdx m, MinIdx* sh)
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

// Two smallest values of a set: the minimum with its index (same rules as MinIdx) and the smallest value among all OTHER elements
// (equal to the minimum when it occurs twice).  The second value is what makes a row's bound robust: when the distance to its
// neighbour grows but stays below every other entry of the row, the bound is still exact (see k_linkage_mw).
struct Min2 { double v; int i; double v2; };
__device__ __forceinline__ void min2_acc(Min2& m, double v, int j)       // sequential scan in ascending j
{
    if (v < m.v) { m.v2 = m.v; m.v = v; m.i = j; }
    else if (v < m.v2) m.v2 = v;
}
__device__ __forceinline__ Min2 min2_merge(Min2 a, Min2 b)
{
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    Min2 r;
    const bool bw = b.v < a.v || (b.v == a.v && b.i < a.i);
    r.v = bw ? b.v : a.v; r.i = bw ? b.i : a.i;
    r.v2 = fmin(bw ? a.v : b.v, fmin(a.v2, b.v2));
    return r;
}
__device__ __forceinline__ Min2 wave_min2(Min2 m)
{
    MinIdx q; q.v = m.v; q.i = m.i;
    const MinIdx w = wave_min(q);
    Min2 r; r.v = w.v; r.i = w.i; r.v2 = INFINITY;
    if (w.i < 0) return r;
    // every lane but the winner's contributes its own minimum, the winner's lane its second value
    const bool win = m.i == w.i && m.i >= 0;
    r.v2 = wave_min_d(win ? m.v2 : (m.i >= 0 ? m.v : (double)INFINITY));
    return r;
}

// the exact bounds of row x from its `cnt` entries above the diagonal, row[t] = D[x, x + 1 + t]: one wave scans (k_row_nn, k_prepare_sq_jobs)
__device__ __forceinline__ Min2 row_min2(const double* __restrict__ row, int64_t cnt, int64_t x)
{
    const int lane = threadIdx.x & 63;
    Min2 m; m.v = INFINITY; m.i = -1; m.v2 = INFINITY;
    for (int64_t t = lane; t < cnt; t += 64) min2_acc(m, row[t], (int)(x + 1 + t));
    return wave_min2(m);
}

// the same for row x of a square matrix some merges into the job: only clusters still there (size != 0), and entry {x, j} from the row that was written
// last (ty: the merge that rewrote a row last, -1 = never): one wave scans (k_row_nn_mid, k_row_nn_mid_jobs)
__device__ __forceinline__ Min2 row_min2_mid(const double* __restrict__ D, int64_t n, const int* __restrict__ size, const int* __restrict__ ty, int64_t x)
{
    const int lane = threadIdx.x & 63;
    Min2 m; m.v = INFINITY; m.i = -1; m.v2 = INFINITY;
    if (size[x] != 0) {
        const int tx = ty[x];
        for (int64_t j = x + 1 + lane; j < n; j += 64)
            if (size[j] != 0) min2_acc(m, tx >= ty[j] ? D[x * n + j] : D[j * n + x], (int)j);
    }
    return wave_min2(m);
}

// Lance-Williams update of the distance between cluster i and the merge of x and y, the linkage method a compile-time parameter
// (clustering/Clustering.py:251-276 declares the seven; the codes are scipy's, also SD_LINKAGE_* in sdhip.h).  Formulas and operation order are
// those of scipy's generic algorithm (_hierarchy_distance_update.pxi, one function per method behind fast_linkage); centroid is the
// reference's cl.cpp:250-256, which restates the same expression.  Cluster sizes are ints there and enter every product as int -> double.
constexpr int LW_SINGLE = 0, LW_COMPLETE = 1, LW_AVERAGE = 2, LW_CENTROID = 3, LW_MEDIAN = 4, LW_WARD = 5, LW_WEIGHTED = 6;
template <int METHOD>
__host__ __device__ __forceinline__ double lw_update(double d_xi, double d_yi, double d_xy, int sx, int sy, int si)
{
    static_assert(METHOD >= LW_SINGLE && METHOD <= LW_WEIGHTED, "unknown linkage method");
    if constexpr (METHOD == LW_SINGLE) return d_xi < d_yi ? d_xi : d_yi;               // fmin / fmax of two non-NaN distances
    else if constexpr (METHOD == LW_COMPLETE) return d_xi > d_yi ? d_xi : d_yi;
    else if constexpr (METHOD == LW_AVERAGE) return ((double)sx * d_xi + (double)sy * d_yi) / (double)(sx + sy);
    else if constexpr (METHOD == LW_CENTROID)
        return sqrt(((((double)sx * d_xi * d_xi) + ((double)sy * d_yi * d_yi)) -
                     ((double)(sx * sy) * d_xy * d_xy) / (double)(sx + sy)) / (double)(sx + sy));
    else if constexpr (METHOD == LW_MEDIAN) return sqrt(0.5 * (d_xi * d_xi + d_yi * d_yi) - 0.25 * d_xy * d_xy);
    else if constexpr (METHOD == LW_WARD) {
        const double t = 1.0 / (double)(sx + sy + si);
        return sqrt((double)(si + sx) * t * d_xi * d_xi + (double)(si + sy) * t * d_yi * d_yi - (double)si * t * d_xy * d_xy);
    }
    else return 0.5 * (d_xi + d_yi);
}

// a runtime method code -> the compile-time parameter: calls f(std::integral_constant<int, METHOD>) for the seven codes; false (f not called) for any other
template <class F> inline bool lw_dispatch(int method, F&& f)
{
    switch (method) {
    case LW_SINGLE: f(std::integral_constant<int, LW_SINGLE>()); return true;
    case LW_COMPLETE: f(std::integral_constant<int, LW_COMPLETE>()); return true;
    case LW_AVERAGE: f(std::integral_constant<int, LW_AVERAGE>()); return true;
    case LW_CENTROID: f(std::integral_constant<int, LW_CENTROID>()); return true;
    case LW_MEDIAN: f(std::integral_constant<int, LW_MEDIAN>()); return true;
    case LW_WARD: f(std::integral_constant<int, LW_WARD>()); return true;
    case LW_WEIGHTED: f(std::integral_constant<int, LW_WEIGHTED>()); return true;
    }
    return false;
}

// ---------------------------------------------------------------- shared by the one-workgroup heap kernels (k_linkage_heap, k_linkage_heap_jobs)
// nearest active neighbour above row x, scanned by `nthreads` threads with U loads in flight per thread
// (a plain strided loop keeps one load outstanding and is latency bound: ~1 us per element per thread)
template <int U>
__device__ __forceinline__ MinIdx scan_row_nn(const double* __restrict__ D, const int* __restrict__ size, int64_t N, int n, int x,
                                              int first, int stride)
{
    MinIdx q; q.v = INFINITY; q.i = -1;
    const double* row = D + cidx(N, x, (int64_t)x + 1) - (x + 1);       // row[j] = D[x, j]
    for (int j0 = x + 1 + first; j0 < n; j0 += stride * U) {
        double v[U]; int sz[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * stride;
            const int jc = j < n ? j : n - 1;
            v[u] = row[jc]; sz[u] = size[jc];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u * stride;
            if (j < n && sz[u] != 0 && v[u] < q.v) { q.v = v[u]; q.i = j; }
        }
    }
    return q;
}


// the reference's indexed binary min-heap (cl.cpp:28-119), operation for operation; one thread runs them
struct HeapRef { double* val; int* key; int* pos; int size; };
__device__ __forceinline__ void hp_swap(HeapRef& h, int a, int b)                          // cl.cpp:70-78
{
    const double va = h.val[a], vb = h.val[b];
    h.val[a] = vb; h.val[b] = va;
    const int ka = h.key[a], kb = h.key[b];
    h.key[a] = kb; h.key[b] = ka;
    h.pos[ka] = b; h.pos[kb] = a;
}
__device__ __forceinline__ void hp_down(HeapRef& h, int idx)                                // cl.cpp:53-68
{
    int ch = 2 * idx + 1;
    while (ch < h.size) {
        if (ch + 1 < h.size && h.val[ch + 1] < h.val[ch]) ch += 1;
        if (h.val[idx] > h.val[ch]) { hp_swap(h, idx, ch); idx = ch; ch = 2 * idx + 1; }
        else break;
    }
}
__device__ __forceinline__ void hp_up(HeapRef& h, int idx)                                  // cl.cpp:44-51
{
    int par = (idx - 1) >> 1;
    while (idx > 0 && h.val[par] > h.val[idx]) { hp_swap(h, idx, par); idx = par; par = (idx - 1) >> 1; }
}
__device__ __forceinline__ void hp_change(HeapRef& h, int key, double v)                    // cl.cpp:108-117
{
    const int idx = h.pos[key];
    const double old = h.val[idx];
    h.val[idx] = v;
    if (v < old) hp_up(h, idx); else hp_down(h, idx);
}

// ---------------------------------------------------------------- heap_linkage: one workgroup of T threads, the reference's heap included
// fast_linkage (cl.cpp:289-406) with its indexed binary min-heap (cl.cpp:28-119) kept bit for bit: thread 0 replays every
// Heap operation the reference performs, in the reference's order -- heapify (cl.cpp:94), get_min / change_value in the lazy
// validation loop (cl.cpp:323-339), remove_min (cl.cpp:340), change_value for the rows whose lower bound dropped IN ASCENDING z
// (cl.cpp:381-392), change_value for row y (cl.cpp:395-404) -- while the O(n) parts of a merge (Lance-Williams update, neighbour
// patches, nearest-neighbour scans) run on all threads.  Which of several rows with EXACTLY equal lower bounds the heap hands
// out first depends on the whole history of its array, so nothing short of replaying it reproduces the reference's merge
// order on data with ties (duplicate embeddings, lattice points); with it Z is bit-identical for any input.
// The rows whose bound dropped are collected in the LDS bitmap `changed` ((n + 31) / 32 words) and drained in ascending order by wave 0.
// Nothing the threads compute depends on T: the scans keep the lowest index among equal minima, the Lance-Williams update is per element, the rows whose
// bound dropped are drained in ascending order.
// The whole workgroup calls it with the same arguments: D the condensed matrix with exact nb / md, size = 1, cid = iota; h.val / key / pos with room for
// n - 1 entries (LDS or global memory), h.size = n - 1; sh: T / 64 entries and s in LDS.  It returns for all threads together.
// (no __restrict__: every array here is written by one thread and re-read by others across barriers)
struct HeapShared { int ok, x, y; double dist; };      // thread 0's candidate of the validation loop, for everyone
template <int METHOD, int T>
__device__ __forceinline__ void heap_linkage(double* D, int n, int* size, int* cid, int* nb, double* md, double* Z, HeapRef h, unsigned* changed,
                                             MinIdx* sh, HeapShared& s)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t N = n;
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
                s.x = hx; s.y = hy; s.dist = hd;
                s.ok = (hy >= 0) && (hd == D[cidx(N, hx, hy)]);                                     // cl.cpp:329
            }
            __syncthreads();
            x = s.x; y = s.y; dist = s.dist;
            const int ok = s.ok;
            __syncthreads();
            if (ok) break;
            // stale candidate: row x's true nearest neighbour (cl.cpp:333-338)
            MinIdx q = scan_row_nn<4>(D, size, N, n, x, tid, T);
            q = block_min<T>(q, sh);
            y = q.i; dist = (q.i < 0) ? (double)INFINITY : q.v;
            if (tid == 0) { nb[x] = y; md[x] = dist; hp_change(h, x, dist); }
            __syncthreads();
        }
        if (tid == 0) { hp_swap(h, 0, h.size - 1); h.size -= 1; hp_down(h, 0); }                      // remove_min, cl.cpp:101-105
        if (y < 0) { if (tid == 0) Z[(size_t)k * 4 + 3] = NAN; return; }                             // cannot happen while two clusters are active; y is the same in every thread
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
            q = block_min<T>(q, sh);
            if (tid == 0 && q.i >= 0) { nb[y] = q.i; md[y] = q.v; hp_change(h, y, q.v); }
        }
        __syncthreads();
    }
}


// A slot is a set of 8-byte granules {32-bit payload word, 32-bit round tag}: a reader that sees the tag of the round it waits for has the
// payload of that round (8-byte stores are single transactions), so publishing needs no separate "ready" flag and no counter.
typedef unsigned long long MwGran;
// The `sync` block (workspace cl_sync, zeroed before every cooperative launch): words the kernels raise and the host reads after the launch.
// (SYNC_ROUNDS counts retry rounds in k_linkage_mw / k_linkage_rg, stale scans in k_linkage_hx.)
constexpr int SYNC_TIMEOUT = 1;                  // a slot poll timed out (one XCD: too few workgroups found themselves on XCC 0)
constexpr int SYNC_ROUNDS = 2;                   // diagnostic counter: retry rounds / stale scans
constexpr int SYNC_MERGES = 3;                   // k_linkage_hx: merges done when it stopped
constexpr int SYNC_TIE = 5;                      // the closest pair was not unique: nothing more was merged
constexpr int SYNC_TICKET = 6;                   // one-XCD forms: next ticket of the workgroups that found themselves on XCC 0
constexpr int SYNC_TIE_LO = 26, SYNC_TIE_HI = 27;      // k_linkage_rg: the tie's height (bits of the double)
constexpr int SYNC_HOST_WORDS = LINKAGE_SYNC_HOST_WORDS;      // what the host copies back (32; a job of k_linkage_rg_jobs has a block of just these)
constexpr int SYNC_WORDS = 32 + 16 * 256;
// arg-min candidate flags: bit 0 = the bound is exact; bit 1 (CAND_TIE) = some OTHER row holds exactly the same bound -- the case in which the
// reference's heap, not the value, decides who comes first (k_linkage_heap)
#define CAND_TIE 2

// Cross-workgroup data of the cooperative kernel (distance matrix, bounds, neighbours, slots) is moved with agent-scope
// relaxed atomics only: on gfx950 these are `sc1` loads / stores (write-through past the per-XCD L2, loads that do not
// trust a non-coherent line).  Every wave drains its stores (`s_waitcnt vmcnt(0)`) before the workgroup publishes its
// slot, so no agent-scope release / acquire -- an L2 write-back and a full L2 invalidate per merge -- is needed, and
// each workgroup's private state (cluster sizes, freshness flags) stays cached.
template <class T> __device__ __forceinline__ T LDG(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// One-XCD form (k_linkage_mw<true>): every participating workgroup sits on the SAME XCD (checked in the kernel from
// HW_REG_XCC_ID, not assumed), so that XCD's L2 is the point of coherence: stores stay plain -- they write through the CU's L1
// and KEEP the line in the L2 (an sc1 store drops it, and even a same-XCD reader then pays the cross-XCD round trip) -- while
// loads stay sc1 (bypass the reader's L1, served by the L2).  MI355X_MICROARCH.md, table of store / load flavours.
template <bool ONEX, class T> __device__ __forceinline__ void STX(T* p, T v)
{
    if constexpr (ONEX) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the linkage_* options and the device, as linkage_batch_plan.h's arithmetic takes them
inline LinkageOpts linkage_opts(const sd_ctx* c)
{
    return LinkageOpts{c->linkage_wgs, c->linkage_one_xcd, c->linkage_threads, c->linkage_square, c->linkage_kernel, c->linkage_prefetch, c->num_cu};
}
inline LinkageXcdOpts linkage_xcd_opts(const sd_ctx* c, int method)
{
    return LinkageXcdOpts{c->linkage_batch_xcd, linkage_opts(c), method, c->linkage_force_heap, c->linkage_batch_bytes};
}

// ---------------------------------------------------------------- launchers run_linkage (linkage.hip) drives
// linkage_rg.hip
bool linkage_rg_fits(int64_t N, int G, int TH);
bool linkage_rg_has(int method, bool onex, int G, int TH, int cap, int helper);
hipError_t linkage_rg_launch(sd_ctx* c, int method, bool onex, int G, int TH, double* D, int n, int* cid, const int* nb, const double* md, const double* md2,
                             double* Z, MwGran* gran, unsigned* sync, int cap, int helper, int k0 = 0, const int* sz0 = nullptr, const int* ty0 = nullptr);
int linkage_rg_slot_granules();
// k_linkage_rg_jobs: up to 8 fresh jobs of the one-XCD, 256-thread, 4-column form in one cooperative launch, job x on XCD x.  G and helper are
// the launch's; the record holds what k_linkage_rg takes per job, the rows the two preparation kernels (linkage_batch.hip) build the matrix from, and the index
// of the job's error slot (raised: no kernel behind the distances touches the job)
struct LinkageRgJob {
    const double* X;        // [n][d] rows
    double* D;              // [n][n] square matrix
    int* cid; int* nb;      // [n] each
    double* md; double* md2;      // [n] each
    double* Z;              // [n - 1][4]
    MwGran* gran;           // [2][G][slot granules], zeroed
    unsigned* sync;         // [SYNC_HOST_WORDS], zeroed
    const int* sz0; const int* ty0;      // [n] each, read by the continuation launch only: cluster size (0 = gone) / last rewrite of every column after k0 merges
    int n, cap, err, k0;    // k0: merges already done (the continuation launch; a first launch starts every job fresh whatever stands here)
};
// cont: the continuation launch k_linkage_rg_jobs<M, true> behind a zero launch of k_linkage_hx_jobs: every job goes on from its k0, sz0, ty0
hipError_t linkage_rg_jobs_launch(sd_ctx* c, int method, int G, int TH, int helper, const LinkageRgJob* d_jobs, int nj, int max_cap, const int* d_errs, bool cont = false);
// linkage_mw.hip: centroid only; at most linkage_mw_max_workgroups() workgroups; size_all = what linkage_mw_prepare set up (workspace cl_size_all)
bool linkage_mw_has(int method);
int linkage_mw_max_workgroups();
int linkage_mw_slot_granules();
int linkage_mw_prepare(sd_ctx* c, int64_t N, int G, bool square, int** size_all);
hipError_t linkage_mw_launch(sd_ctx* c, bool onex, bool square, int G, int TH, double* D, int n, int* size_all, int* cid, int* nb, double* md, const double* md2,
                             double* Z, MwGran* gran, unsigned* sync, int cap);
// linkage_hx.hip
bool linkage_hx_fits(int64_t N, int workers);
int linkage_hx_run(sd_ctx* c, int method, bool onex, int workers, double* D, int64_t N, int* cid, int* size, int* tyv, int* nb, double* md, double* d_Z, bool* stopped,
                   double stop_above = (double)INFINITY, int64_t* merges_done = nullptr, bool* launched = nullptr);
// k_linkage_hx_jobs: up to 8 jobs of the one-XCD, 16-bit form in one cooperative launch of 8 (workers + 1) workgroups, job x on XCD x, each up to its first
// merge above height 0.  `workers` is the launch's; the record holds what k_linkage_hx takes per job -- every array the job's own -- and the index
// of its error slot.  The caller has set size = 1, ty = -1, zeroed the granules and the sync block, and left matrix, bounds and ids as the preparation made them.
struct LinkageHxJob {
    double* D;              // [n][n] square matrix
    int* cid; int* size; int* ty; int* nb;      // [n] each
    double* md;             // [n]
    double* Z;              // [n - 1][4]
    double* hval; int* hkey; int* hpos;         // [n] each: the heap's lower tier (keys and positions: the 32-bit form's, unused by the 16-bit one)
    MwGran* cmd; MwGran* rep;                   // [16], [workers][8], zeroed
    int* chg_z; double* chg_v;                  // [workers][cap] each
    unsigned* sync;         // [SYNC_HOST_WORDS], zeroed
    int n, cap, lc, err;    // rows; columns per worker; heap values in LDS (linkage_hx_form); error slot
};
hipError_t linkage_hx_jobs_launch(sd_ctx* c, int method, int workers, const LinkageHxJob* d_jobs, int nj, size_t max_dyn, const int* d_errs);
// linkage_heap.hip: the condensed matrix Dc with exact nb / md, size = 1, cid = iota; every method
int linkage_heap_run(sd_ctx* c, int method, double* Dc, int64_t N, int* size, int* cid, int* nb, double* md, double* d_Z);
