// linkage_mw.hip -- k_linkage_mw: the cooperative centroid linkage (Clustering::linkage's fast_linkage, cl.cpp:289-406) with the per-row state in LDS,
// on the condensed or the square distance matrix, and its launchers.  run_linkage (linkage.hip) takes it where k_linkage_rg does not run: the condensed
// form (no room for the square above 170 GB, option linkage_square = 0), a geometry k_linkage_rg does not fit, option linkage_kernel = 0.
#include "common.h"
#include "exact_fp.h"
#include "linkage_dev.h"

// ---------------------------------------------------------------- k_linkage_mw : the same algorithm on G co-resident workgroups
// Rows are owned round-robin (row z belongs to workgroup z % G).  Per merge every workgroup
//   1. applies the size bookkeeping of the merge to its own view (identical stores from all workgroups),
//   2. runs the Lance-Williams update for its rows, folding the nearest-neighbour search of row y into the
//      same pass (the new D[z,y], z > y, are in registers: row y is never re-read),
//   3. computes its local arg-min of the lower bounds and publishes {NN(y) partial, arg-min} in a slot,
//   4. exchanges slots with the others: the slot is a set of tagged 8-byte granules {payload word, round number} that
//      the readers poll directly -- no counter, no flag, no fence (everything the workgroups hand each other travels in
//      agent-scope `sc1` loads / stores, see LDG / STX in linkage_dev.h; placement independent); every workgroup reduces the G
//      slots itself, so all take the same decision without a broadcast.
// A stale candidate (cl.cpp:329-338) costs one extra round (see the kernel's own header below).
// Used from N = 1500 up, where one CU's memory pipeline is the bottleneck.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "k_linkage_mw's fence-free slot exchange (sc1 write-through stores, sc1 loads, 8-byte tagged granules) is written for gfx950 only"
#endif
#define MWT 256
#define MWT_MAX 1024
// arg-min candidate that carries its neighbour and its flags along through the reductions.
// fresh bit 0: the bound is exact (== D[i, y]); bit 1 (CAND_TIE): some OTHER row holds exactly the same bound -- the case in
// which the reference's heap, not the value, decides who comes first (see k_linkage_heap)
struct Cand { double v; int i; int y; int fresh; };

__device__ __forceinline__ Cand cbetter(Cand a, Cand b)
{
    if (b.i < 0) return a;
    if (a.i < 0) return b;
    if (b.v < a.v) return b;
    if (b.v == a.v) {
        Cand r = (b.i < a.i) ? b : a;
        if (a.i != b.i && a.v < INFINITY) r.fresh |= CAND_TIE | ((a.fresh | b.fresh) & CAND_TIE);
        return r;
    }
    return a;
}
// sequential accumulation of one row into a thread's running candidate (same rules as cbetter)
__device__ __forceinline__ void cand_acc(Cand& m, double v, int z, int y, int fresh)
{
    if (m.i < 0 || v < m.v) { m.v = v; m.i = z; m.y = y; m.fresh = fresh; }
    else if (v == m.v) {
        const int tie = (v < INFINITY) ? CAND_TIE : 0;
        if (z < m.i) { m.i = z; m.y = y; m.fresh = fresh | tie | (m.fresh & CAND_TIE); }
        else m.fresh |= tie;
    }
}
// same two moves for candidates.  cbetter's tie rule survives: the winner is the lowest row among the lanes at the minimum, and
// CAND_TIE is raised when a DIFFERENT row sits at the same finite bound (flags inherited from the losers add nothing to that)
__device__ __forceinline__ Cand wave_min_c(Cand m)
{
    const bool has = m.i >= 0;
    const double vmin = wave_min_d(has ? m.v : (double)INFINITY);
    const bool at = has && m.v == vmin;
    const unsigned long long mask = __ballot(at);
    Cand r; r.v = INFINITY; r.i = -1; r.y = -1; r.fresh = 0;
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
    r.fresh = __builtin_amdgcn_readlane(m.fresh, l) | extra;
    return r;
}
__device__ __forceinline__ Cand block_min_c(Cand m, Cand* sh, int nwaves)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    m = wave_min_c(m);
    __syncthreads();
    if (lane == 0) sh[w] = m;
    __syncthreads();
    Cand r; r.v = INFINITY; r.i = -1; r.y = -1; r.fresh = 0;
    if (lane < nwaves) r = sh[lane];
    return wave_min_c(r);                // every wave folds the per-wave winners itself
}
// the two reductions of a merge round (NN(y) partial and local arg-min) through ONE LDS exchange
__device__ __forceinline__ void block_min_qc(Min2& q, Cand& m, Min2* shq, Cand* shc, int nwaves)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    q = wave_min2(q);
    m = wave_min_c(m);
    __syncthreads();
    if (lane == 0) { shq[w] = q; shc[w] = m; }
    __syncthreads();
    Min2 rq; rq.v = INFINITY; rq.i = -1; rq.v2 = INFINITY;
    Cand r; r.v = INFINITY; r.i = -1; r.y = -1; r.fresh = 0;
    if (lane < nwaves) { rq = shq[lane]; r = shc[lane]; }
    q = wave_min2(rq);
    m = wave_min_c(r);
}

// ---------------------------------------------------------------- k_linkage_mw : the cooperative kernel
//  * every workgroup keeps its owned ACTIVE rows as a compact list in LDS (swap-with-last removal), so the
//    Lance-Williams pass and the arg-min touch N-k rows at merge k instead of N (half the random HBM accesses);
//  * a stale candidate (cl.cpp:329-338) is not rescanned by its owner alone (one CU pulling a 1.4 MB row at
//    N = 172 773 takes ~60 us): all workgroups see the same published candidates, pick the same KR best stale rows
//    and each scans its share of the columns of every such row; the partial minima travel in the slots of the
//    one barrier the round needs anyway.  Refreshing up to KR near-top stale rows per round needs ~5x fewer rounds
//    than refreshing only the top one (measured 9.3 k vs 49 k rounds at N = 21 573).
#define KR 4
// A slot is SLOT_WORDS 8-byte granules {32-bit payload word, 32-bit round tag}: a reader that sees the tag of the round it
// waits for has the payload of that round (8-byte stores are single transactions), so publishing needs no separate
// "ready" flag and no counter -- the readers poll the granules themselves.  Words: 0-1 arg-min bound (double), 2 its row,
// 3 its neighbour, 4 freshness, 5-6 NN(y) partial (double), 7 its row; merge rounds: 8 "row x had a second pair at the merge height",
// 9-10 second value of the NN(y) partial; retry rounds: 8+5r.. refreshed-row partial r (minimum double, its row, second value double).
#define SLOT_WORDS 32

// SQ form (k_linkage_mw<*, true>): the distance matrix is the full N x N square and a workgroup owns a contiguous range of COLUMNS.
// Only rows are ever read or written in bulk: a merge (x, y) reads rows x and y and writes row y, every workgroup its own column range,
// coalesced (the condensed form touches one 64-byte line per entry for the half of the entries that lie in a column: 150 000 scattered
// transactions per merge at N = 100 000, tools/tlb_probe2.hip).  Row y is NOT mirrored into column y.  Instead every cluster carries the
// index ty of the last merge that rewrote its row (-1: never), and the entry {a, b} is read from the row of the cluster with the larger
// ty -- the one written last, which holds the current value; with equal ty (two clusters that never were a merge's y) both rows still
// hold the pdist value.  A merge that involves a cluster older than a bystander z reads that one entry from row z (scattered); on
// clustered data (one growing cluster per speaker swallowing singletons) that is a handful of entries per merge.
template <bool ONEX, bool SQ>
__global__ __launch_bounds__(MWT_MAX) void k_linkage_mw(double* D, int n, int* size_all, int* cid, int* nb, double* md, const double* md2_init,
                                                         double* Z, MwGran* gran /*[2][G][SLOT_WORDS], zeroed*/,
                                                         unsigned* sync, int cap /*owned rows per workgroup, upper bound*/, int G)
{
    extern __shared__ __attribute__((aligned(16))) int dyn_lds[];
    // per owned row, 32 B of LDS: the active list and, beside every entry, the row's lower bound / neighbour / freshness.  The
    // owner is the only reader of these in the hot loops (local arg-min, Lance-Williams pass), so they never leave the CU; the
    // global md / nb copies are still written (row y's old bound is read by everybody) but not read back by the owner.
    // l_md2 is the second level of the bound: every active entry of the row OTHER than the neighbour's is >= l_md2.  While the
    // neighbour's distance stays <= l_md2 the bound is exact whatever the merge did to it, and a row only goes stale (and costs a
    // retry round when it reaches the top) after it has lost BOTH levels; with the reference's single lower bound (cl.cpp:323-339) a
    // row went stale every time the distance to its neighbour grew -- about half the rows per merge on clustered data, 0.46 retry
    // rounds per merge on the planted hour.  Same merges: the arg-min of exact values does not depend on how the bounds are kept.
    double* l_md = (double*)dyn_lds;                 // [cap] bound of act[p]
    double* l_md2 = l_md + cap;                      // [cap] lower bound of the row's entries other than the neighbour's
    int* act = (int*)(l_md2 + cap);                  // [cap] owned active rows, unordered.  SQ: l_ty[s] = ty of owned column z0 + s
    int* pos = act + cap;                            // [cap] pos[z / G] = index of owned row z in act
    int* l_nb = pos + cap;                           // [cap] neighbour of act[p]
    unsigned char* l_fr = (unsigned char*)(l_nb + cap);   // [cap] freshness of act[p]
    __shared__ Min2 sh[MWT_MAX / 64];
    __shared__ Cand shc[MWT_MAX / 64];
    __shared__ Min2 s_part[KR][MWT_MAX / 64];
    __shared__ unsigned s_words[MWT][SLOT_WORDS + 1];  // this round's slots of all workgroups, as received (+1: lane u reads word w of slot u -- a 128-byte row stride would put all lanes on two banks)
    __shared__ Cand s_cand[MWT + 1];        // published local bests of the G <= 256 workgroups (+ row y)
    __shared__ Min2 s_row[KR];
    __shared__ int s_L[2][KR];
    __shared__ int s_nL[2];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = blockDim.x, NW = T >> 6;
    int g = blockIdx.x;
    if constexpr (ONEX) {
        // 8 G workgroups were launched; the first G that find themselves on XCC 0 take part (rank = ticket), the others leave.
        // Under round-robin dispatch exactly the G workgroups with blockIdx % 8 == 0 qualify; under any other dispatch too few
        // may arrive and the participants run into the poll timeout -- run_linkage then repeats the job with the multi-XCD form.
        __shared__ int s_ticket;
        if (tid == 0) {
            const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));       // HW_REG_XCC_ID[3:0]
            s_ticket = (xcc == 0) ? (int)atomicAdd(&sync[SYNC_TICKET], 1u) : -1;
        }
        __syncthreads();
        g = s_ticket;
        if (g < 0 || g >= G) return;
    }
    const int64_t N = n;
    int* size = size_all + (size_t)g * n * (SQ ? 2 : 1);       // this workgroup's private copy of the cluster sizes (SQ: followed by its copy of ty)
    int* tyv = size + n;                                       // SQ only
    int* l_ty = act;                                           // SQ only
    const int colsB = cap - 1;                                 // SQ: columns per workgroup; z0 = first owned column, nown = how many exist
    const int z0 = SQ ? g * colsB : 0;
    const int nown = SQ ? (n - z0 < colsB ? (n - z0 > 0 ? n - z0 : 0) : colsB) : 0;
    auto own = [&](int z) -> bool { return SQ ? (z >= z0 && z < z0 + colsB) : ((z % G) == g); };
    auto slot = [&](int z) -> int { return SQ ? z - z0 : pos[z / G]; };
    unsigned bar = 0;
    int par = 0, lp = 0;             // slot parity, refresh-list parity
    // receive round `bar` of every workgroup's slot (nw words each) into s_words; returns false on timeout
    auto consume = [&](int nw) -> bool {
        const MwGran* base = gran + (size_t)par * G * SLOT_WORDS;
        bool ok = true;
        for (int idx = tid; idx < G * nw; idx += T) {
            const int sl = idx / nw, wd = idx - sl * nw;
            const MwGran* p = base + (size_t)sl * SLOT_WORDS + wd;
            MwGran v = LDG(p);
            unsigned spins = 0;
            while ((unsigned)(v >> 32) != bar) {
                __builtin_amdgcn_s_sleep(1);
                v = LDG(p);
                if (++spins > (1u << 24)) { sync[SYNC_TIMEOUT] = 1; ok = false; break; }     // ~seconds: never in a healthy run
            }
            s_words[sl][wd] = (unsigned)v;
        }
        return __syncthreads_and(ok ? 1 : 0) != 0;
    };
    MinIdx none; none.v = INFINITY; none.i = -1;

    // local arg-min over the owned active rows, skipping the rows being refreshed this round
    auto local_argmin = [&](int nL, const int* L) -> Cand {
        int ex[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) ex[r] = r < nL ? L[r] : -1;
        Cand m; m.v = INFINITY; m.i = -1; m.y = -1; m.fresh = 0;
        const int cnt = SQ ? nown : s_cnt;
        for (int p0 = tid; p0 < cnt; p0 += T * 4) {
            double v[4]; int zz[4], ny_[4]; unsigned char fr[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = p0 + u * T;
                const int pc = p < cnt ? p : 0;
                fr[u] = l_fr[pc];
                int z = p < cnt ? (SQ ? ((fr[u] & 2) ? -1 : z0 + pc) : act[pc]) : -1;
                if (z >= n - 1) z = -1;
                zz[u] = z;
                v[u] = l_md[pc]; ny_[u] = l_nb[pc];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int z = zz[u];
                bool skip = z < 0;
#pragma unroll
                for (int r = 0; r < KR; ++r) skip |= (z == ex[r]);
                if (!skip) cand_acc(m, v[u], z, ny_[u], fr[u] & 1);
            }
        }
        return block_min_c(m, shc, NW);
    };
    // this workgroup's share of the columns of the nL rows in L: wave tasks (row r, sub-slice s)
    auto scan_rows = [&](int nL, const int* L, Min2* outv /*LDS [KR]*/) {
        if (nL <= 0) return;
        const int S = NW >= nL ? NW / nL : 1;
        for (int t = wv; t < nL * S; t += NW) {
            const int r = t % nL, sidx = t / nL;
            const int x = L[r];
            Min2 q; q.v = INFINITY; q.i = -1; q.v2 = INFINITY;
            if constexpr (SQ) {
                // this workgroup's own columns above x: entry {x, j} from the row written last
                const int txr = tyv[x];
                const int64_t jend = (int64_t)z0 + nown, step = (int64_t)S * 64;
                for (int64_t j0 = (x + 1 > z0 ? x + 1 : z0) + (int64_t)sidx * 64 + lane; j0 < jend; j0 += step * 4) {
                    double v[4]; bool ok[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int64_t j = j0 + u * step; const int64_t jc = j < jend ? j : jend - 1;
                        const int sj = (int)(jc - z0);
                        ok[u] = j < jend && !(l_fr[sj] & 2);
                        v[u] = LDG(txr >= l_ty[sj] ? &D[(int64_t)x * N + jc] : &D[jc * N + x]);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (ok[u]) min2_acc(q, v[u], (int)(j0 + u * step));
                }
                q = wave_min2(q);
                if (lane == 0) s_part[r][sidx] = q;
                continue;
            }
            const double* row = D + cidx(N, x, (int64_t)x + 1) - (x + 1);
            const int64_t step = (int64_t)G * S * 64;
            for (int64_t j0 = (int64_t)x + 1 + ((int64_t)g * S + sidx) * 64 + lane; j0 < n; j0 += step * 4) {
                double v[4]; int sz[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t j = j0 + u * step; const int64_t jc = j < n ? j : n - 1;
                    v[u] = LDG(&row[jc]); sz[u] = size[jc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t j = j0 + u * step;
                    if (j < n && sz[u] != 0) min2_acc(q, v[u], (int)j);
                }
            }
            q = wave_min2(q);
            if (lane == 0) s_part[r][sidx] = q;
        }
        __syncthreads();
        if (tid < nL) {
            Min2 q = s_part[tid][0];
            for (int k2 = 1; k2 < S; ++k2) q = min2_merge(q, s_part[tid][k2]);
            outv[tid] = q;
        }
        __syncthreads();
    };
    // publish this workgroup's slot for the next round.  Every wave first drains its write-through stores (distance
    // matrix, bounds): whoever sees the slot may read them.
    auto publish = [&](Min2 q, Cand m, int nL, const Min2* rows, int row_tie = 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        ++bar;
        MwGran* sl = gran + ((size_t)par * G + g) * SLOT_WORDS;
        const MwGran tag = (MwGran)bar << 32;
        if (tid == 0) {
            const unsigned long long av = (unsigned long long)__double_as_longlong(m.v), nv = (unsigned long long)__double_as_longlong(q.v);
            STX<ONEX>(&sl[0], tag | (unsigned)av); STX<ONEX>(&sl[1], tag | (unsigned)(av >> 32)); STX<ONEX>(&sl[2], tag | (unsigned)m.i);
            STX<ONEX>(&sl[3], tag | (unsigned)m.y); STX<ONEX>(&sl[4], tag | (unsigned)m.fresh);
            STX<ONEX>(&sl[5], tag | (unsigned)nv); STX<ONEX>(&sl[6], tag | (unsigned)(nv >> 32)); STX<ONEX>(&sl[7], tag | (unsigned)q.i);
            if (nL == 0) {          // rounds without refreshed rows: word 8 = "row x had a second pair at the merge height", 9-10 = second value of the NN(y) partial
                const unsigned long long sv = (unsigned long long)__double_as_longlong(q.v2);
                STX<ONEX>(&sl[8], tag | (unsigned)row_tie); STX<ONEX>(&sl[9], tag | (unsigned)sv); STX<ONEX>(&sl[10], tag | (unsigned)(sv >> 32));
            }
        }
        if (tid < nL) {
            const unsigned long long pv = (unsigned long long)__double_as_longlong(rows[tid].v), sv = (unsigned long long)__double_as_longlong(rows[tid].v2);
            MwGran* rw = sl + 8 + 5 * tid;
            STX<ONEX>(&rw[0], tag | (unsigned)pv); STX<ONEX>(&rw[1], tag | (unsigned)(pv >> 32)); STX<ONEX>(&rw[2], tag | (unsigned)rows[tid].i);
            STX<ONEX>(&rw[3], tag | (unsigned)sv); STX<ONEX>(&rw[4], tag | (unsigned)(sv >> 32));
        }
    };
    auto word_d = [&](int sl, int wd) -> double {
        return __longlong_as_double((long long)(((unsigned long long)s_words[sl][wd + 1] << 32) | s_words[sl][wd]));
    };
    // after consume(): every WAVE folds the G slots itself -- global best, NN(y), "row x had a second pair" -- so a merge round
    // needs no LDS broadcast and no workgroup barrier here; only a retry round (refreshed rows are folded one per wave) has two
    Cand d_best; Min2 d_nn; int d_rowtie = 0;
    const Min2 none2 = {INFINITY, -1, INFINITY};
    d_best.v = INFINITY; d_best.i = -1; d_best.y = -1; d_best.fresh = 0; d_nn = none2;
    auto digest = [&](int nLprev, const int* Lprev, int yrow, bool with_nn) {
        if (tid < G) {          // kept for pick_stale (read there behind a barrier)
            Cand c; c.v = word_d(tid, 0); c.i = (int)s_words[tid][2]; c.y = (int)s_words[tid][3]; c.fresh = (int)s_words[tid][4]; s_cand[tid] = c;
        }
        if (nLprev > 0) {
            for (int r = wv; r < nLprev; r += NW) {          // refreshed rows: one wave folds the G partial minima of a row
                Min2 a = none2;
                for (int u = lane; u < G; u += 64) { Min2 pq; pq.v = word_d(u, 8 + 5 * r); pq.i = (int)s_words[u][10 + 5 * r]; pq.v2 = word_d(u, 11 + 5 * r); a = min2_merge(a, pq); }
                a = wave_min2(a);
                if (lane == 0) s_row[r] = a;
            }
            __syncthreads();
        }
        Cand b; b.v = INFINITY; b.i = -1; b.y = -1; b.fresh = 0;
        Min2 a = none2;
        int rt = 0;
        for (int u = lane; u < G; u += 64) {
            Cand c; c.v = word_d(u, 0); c.i = (int)s_words[u][2]; c.y = (int)s_words[u][3]; c.fresh = (int)s_words[u][4];
            b = cbetter(b, c);
            if (with_nn) { Min2 pq; pq.v = word_d(u, 5); pq.i = (int)s_words[u][7]; pq.v2 = word_d(u, 9); a = min2_merge(a, pq); }
            if (nLprev == 0) rt |= (int)s_words[u][8];
        }
        if (lane < nLprev) {           // the rows refreshed in this round are exact now
            Cand c; c.i = Lprev[lane]; c.y = s_row[lane].i; c.v = (c.y < 0) ? INFINITY : s_row[lane].v; c.fresh = 1;
            if (c.y >= 0) b = cbetter(b, c);
        }
        d_best = wave_min_c(b);
        if (with_nn) d_nn = wave_min2(a);
        d_rowtie = (nLprev == 0 && __ballot(rt != 0) != 0ull) ? 1 : 0;
        if (nLprev > 0) {
            // owners store the refreshed rows (read back only by the owner's later arg-mins)
            if (tid < nLprev && own(Lprev[tid])) {
                const int x = Lprev[tid]; const Min2 q = s_row[tid];
                const double qv = (q.i < 0) ? (double)INFINITY : q.v;
                const int px = slot(x);
                l_nb[px] = q.i; l_md[px] = qv; l_md2[px] = (q.i < 0) ? (double)INFINITY : q.v2; l_fr[px] = 1;
                STX<ONEX>(&nb[x], q.i); STX<ONEX>(&md[x], qv);
            }
            __syncthreads();
        }
    };
    // the next refresh list: the KR best stale candidates among s_cand[0..G) and `extra` (row y after a merge); wave 0
    // extracts them one by one from registers, every workgroup arrives at the same list
    auto pick_stale = [&](Cand extra, int slot) {
        __syncthreads();               // s_cand of this round complete
        if (wv == 0) {
            MinIdx c[5];
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const int idx = lane + 64 * u;
                c[u] = none;
                if (idx <= G) {
                    Cand o = extra;
                    if (idx < G) o = s_cand[idx];
                    if (o.i >= 0 && !(o.fresh & 1) && o.v != INFINITY) { c[u].v = o.v; c[u].i = o.i; }
                }
            }
            // common case: at most KR stale candidates -> take them all (their order is irrelevant), no reduction needed
            int nl = 0;
#pragma unroll
            for (int u = 0; u < 5; ++u) {
                const bool st = c[u].i >= 0;
                const unsigned long long mk = __ballot(st);
                const int at = nl + __popcll(mk & ((1ull << lane) - 1ull));
                if (st && at < KR) s_L[slot][at] = c[u].i;
                nl += __popcll(mk);
            }
            if (nl > KR) {                       // more than KR: the KR best by (bound, row)
                nl = 0;
                for (int r = 0; r < KR; ++r) {
                    MinIdx bq = none;
#pragma unroll
                    for (int u = 0; u < 5; ++u) bq = better(bq, c[u]);
                    bq = wave_min(bq);
                    if (bq.i < 0) break;
                    if (lane == 0) s_L[slot][r] = bq.i;
#pragma unroll
                    for (int u = 0; u < 5; ++u) if (c[u].i == bq.i) c[u].i = -1;
                    nl = r + 1;
                }
            }
            if (lane == 0) s_nL[slot] = nl;
        }
        __syncthreads();
    };
    Cand nocand; nocand.v = INFINITY; nocand.i = -1; nocand.y = -1; nocand.fresh = 1;

    // ---- initial state: exact bounds from k_row_nn; owned rows g, g+G, ...
    int cnt0 = 0;
    if constexpr (SQ) {
        for (int i2 = tid; i2 < nown; i2 += T) {
            const int z = z0 + i2;
            l_ty[i2] = -1;
            l_md[i2] = z < n - 1 ? md[z] : (double)INFINITY; l_md2[i2] = z < n - 1 ? md2_init[z] : (double)INFINITY; l_nb[i2] = z < n - 1 ? nb[z] : -1; l_fr[i2] = 1;
        }
    } else
    for (int z = g + G * tid, i2 = tid; z < n; z += G * T, i2 += T) {
        act[i2] = z; pos[i2] = i2;
        l_md[i2] = z < n - 1 ? md[z] : (double)INFINITY; l_md2[i2] = z < n - 1 ? md2_init[z] : (double)INFINITY; l_nb[i2] = z < n - 1 ? nb[z] : -1; l_fr[i2] = 1;
    }
    if (tid == 0) { cnt0 = (n - g + G - 1) / G; if (cnt0 < 0) cnt0 = 0; s_cnt = cnt0; s_nL[0] = 0; s_nL[1] = 0; }
    __syncthreads();
    {
        Cand m0 = local_argmin(0, s_L[0]);
        publish(none2, m0, 0, s_row);
    }
    if (!consume(11)) return;
    digest(0, s_L[0], -1, false);
    par ^= 1;
    Cand best = d_best;
    if (!((best.fresh & 1) && best.y >= 0)) pick_stale(nocand, lp);
    int x = best.i, y = best.y; double dist = best.v; bool fresh = (best.fresh & 1) != 0;
    // cluster sizes of the pair about to merge, requested as soon as the pair is known (an L2 round trip off the merge's serial path)
    int nx_pre = 0, ny_pre = 0, cx_pre = 0, cy_pre = 0;            // (workgroup 0's first thread also needs the pair's dendrogram ids)
    int tx_pre = -1, ty_pre = -1;                                  // SQ: last merge that rewrote row x / row y
    auto prefetch_pair = [&]() {
        if (fresh && y >= 0) {
            nx_pre = size[x]; ny_pre = size[y];
            if constexpr (SQ) { tx_pre = tyv[x]; ty_pre = tyv[y]; }
            if (g == 0 && tid == 0) { cx_pre = cid[x]; cy_pre = cid[y]; }
        }
    };
    prefetch_pair();
    // a merge is taken from the arg-min only when its pair is the UNIQUE closest pair; otherwise the kernel stops and
    // run_linkage repeats the job with k_linkage_heap, which owns the reference's tie order
    auto tie_stop = [&](int flags) -> bool {
        if (!(flags & CAND_TIE)) return false;
        if (g == 0 && tid == 0) sync[SYNC_TIE] = 1;
        return true;
    };

    for (int k = 0; k < n - 1; ++k) {
        // ---- lazy validation (cl.cpp:323-339): cooperative refresh of the KR best stale candidates per round
        for (int guard = 0; guard <= n - k; ++guard) {
            if (fresh && y >= 0) break;
            if (g == 0 && tid == 0) sync[SYNC_ROUNDS] += 1;            // diagnostic: retry rounds
            const int nL = s_nL[lp]; const int* L = s_L[lp];
            scan_rows(nL, L, s_row);
            Cand m = local_argmin(nL, L);
            publish(none2, m, nL, s_row);
            if (!consume(nL > 0 ? 8 + 5 * nL : 11)) return;
            digest(nL, L, -1, false);
            par ^= 1;
            best = d_best;
            lp ^= 1;
            if (!((best.fresh & 1) && best.y >= 0)) pick_stale(nocand, lp);
            x = best.i; dist = best.v; y = best.y; fresh = (best.fresh & 1) != 0;
            prefetch_pair();
        }
        if (tie_stop(best.fresh)) return;
        // ---- merge (x, y) at height dist
        const int nx = nx_pre, ny = ny_pre;
        // No workgroup barrier in front of the pass: the pair is in every thread's registers, the pass skips x and y by value, and x
        // leaves its owner's active list -- and the pair's sizes change in this workgroup's private size[] -- only behind the pass
        // (below): a slower wave may still be loading size[x] / size[y] in prefetch_pair when thread 0 gets here.
        auto write_Z = [&]() {                             // (behind the pass: thread 0 must not wait for the pair's ids before it issues its loads)
            if (tid == 0 && g == 0) {
                int ix = cx_pre, iy = cy_pre;
                if (ix > iy) { const int t = ix; ix = iy; iy = t; }
                Z[(size_t)k * 4 + 0] = (double)ix; Z[(size_t)k * 4 + 1] = (double)iy;
                Z[(size_t)k * 4 + 2] = dist;       Z[(size_t)k * 4 + 3] = (double)(nx + ny);
                cid[y] = n + k;
            }
        };
        if (k == n - 2) { write_Z(); break; }
        // ---- one pass over the owned active rows: Lance-Williams update + neighbour patches (cl.cpp:361-392),
        // NN(y) partial from the fresh distances (cl.cpp:395-404), next local arg-min
        Min2 q = none2;
        Cand m; m.v = INFINITY; m.i = -1; m.y = -1; m.fresh = 0;
        int row_tie = 0;
        const int cnt = SQ ? nown : s_cnt;
        const int txm = tx_pre, tym = ty_pre;             // SQ: ty of the pair before this merge
        int zdummy = 0;                                   // any valid row other than x and y (n >= 3 here)
        while (zdummy == x || zdummy == y) ++zdummy;
        if (SQ) { zdummy = z0; while ((zdummy == x || zdummy == y) && zdummy + 1 < z0 + (nown > 0 ? nown : 1)) ++zdummy; }   // (an own column: its l_ty slot exists)
        for (int p0 = tid; p0 < cnt; p0 += T * 4) {
            double dzx[4], dzy[4], mdz[4], md2z[4]; int zz[4], nbz[4], frz[4], pp[4]; int64_t izy[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = p0 + u * T;
                const int pc = p < cnt ? p : 0;
                pp[u] = pc;
                frz[u] = l_fr[pc];
                int z = p < cnt ? (SQ ? ((frz[u] & 2) ? -1 : z0 + pc) : act[pc]) : -1;
                if (z == y || z == x) z = -1;
                zz[u] = z;
                const int zc = z >= 0 ? z : zdummy;
                if constexpr (SQ) {
                    // the current value of {z, x} / {z, y} lives in the row of the cluster whose row was written last (row y is written
                    // below).  The row copies are requested at once, before the pair's ty have arrived (prefetch_pair's loads are still
                    // in flight): on clustered data they are the right ones for all but a handful of entries, fixed up below.
                    izy[u] = (int64_t)y * N + zc;
                    dzx[u] = LDG(&D[(int64_t)x * N + zc]);
                    dzy[u] = LDG(&D[izy[u]]);
                } else {
                    izy[u] = cidx(N, zc, y);
                    dzx[u] = LDG(&D[cidx(N, zc, x)]);
                    dzy[u] = LDG(&D[izy[u]]);
                }
                nbz[u] = l_nb[pc]; mdz[u] = l_md[pc]; md2z[u] = l_md2[pc];
            }
            if constexpr (SQ) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (zz[u] < 0) continue;
                    const int tz = l_ty[zz[u] - z0];
                    if (txm < tz) dzx[u] = LDG(&D[(int64_t)zz[u] * N + x]);        // z's row was written after x's: the current {z, x} is there
                    if (tym < tz) dzy[u] = LDG(&D[(int64_t)zz[u] * N + y]);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int z = zz[u];
                if (z < 0) continue;
                const double nd = lw_update<LW_CENTROID>(dzx[u], dzy[u], dist, nx, ny, 0);
                STX<ONEX>(&D[izy[u]], nd);
                if (z > x && dzx[u] == dist) row_tie = 1;         // row x had a second neighbour at exactly the merge height
                double mz = (z < n - 1) ? mdz[u] : INFINITY; int nz = nbz[u], fz = frz[u];
                if (z < y) {
                    // row z's entries above the diagonal: x's is gone (if z < x), y's is nd now.  Invariants: mz <= every active entry of
                    // the row (the reference's lower bound), m2 <= every active entry OTHER than the neighbour's.
                    const double m2 = fmax(md2z[u], mz);
                    if ((z < x && nz == x) || nz == y) {
                        // the neighbour's entry is the one that changed (or went away: y takes over).  Exact while nd is still the row minimum.
                        nz = y;
                        if (nd <= m2) { mz = nd; fz = 1; } else { mz = m2; fz = 0; }
                        l_md[pp[u]] = mz; l_md2[pp[u]] = m2; l_nb[pp[u]] = y; l_fr[pp[u]] = (unsigned char)fz; STX<ONEX>(&md[z], mz); STX<ONEX>(&nb[z], y);
                    } else if (nd < mz) {
                        // y becomes the neighbour; the old neighbour's entry (>= mz) joins the others, which are all >= mz
                        l_md2[pp[u]] = mz;
                        nz = y; mz = nd; fz = 1; l_md[pp[u]] = nd; l_nb[pp[u]] = y; l_fr[pp[u]] = 1; STX<ONEX>(&md[z], nd); STX<ONEX>(&nb[z], y);
                    } else if (nd < m2) l_md2[pp[u]] = nd;
                } else if (nd < q.v || (nd == q.v && z < q.i)) { q.v2 = q.v; q.v = nd; q.i = z; }
                else if (nd < q.v2) q.v2 = nd;
                if (z < n - 1) cand_acc(m, mz, z, nz, fz);
            }
        }
        block_min_qc(q, m, sh, shc, NW);
        row_tie = __syncthreads_or(row_tie);
        write_Z();
        if (tid == 0) { size[x] = 0; size[y] = nx + ny; }     // (every thread is past the pass and has used the old sizes)
        if constexpr (SQ) {
            if (tid == 0) {
                tyv[y] = k;                                   // row y is the current copy of every {y, z} from now on
                if (own(y)) l_ty[y - z0] = k;
                if (own(x)) l_fr[x - z0] = 2;                 // column x is gone
            }
        } else
        if (tid == 0 && (x % G) == g) {                       // owner drops x from its active list
            const int p = pos[x / G], c2 = s_cnt - 1, last = act[c2];
            act[p] = last; pos[last / G] = p; s_cnt = c2;
            l_md[p] = l_md[c2]; l_md2[p] = l_md2[c2]; l_nb[p] = l_nb[c2]; l_fr[p] = l_fr[c2];
        }
        publish(q, m, 0, s_row, row_tie);
        if (!consume(11)) return;
        digest(0, s_L[lp], y, true);
        par ^= 1;
        if (d_rowtie) { if (g == 0 && tid == 0) sync[SYNC_TIE] = 1; return; }
        best = d_best;
        const Min2 nn = d_nn;
        // row y: exact by construction when it has an active neighbour above (cl.cpp:395-404), else its old (stale) bound
        Cand cy; cy.i = -1; cy.v = INFINITY; cy.y = -1; cy.fresh = 0;
        if (y < n - 1) {
            if (nn.i >= 0) {
                cy.v = nn.v; cy.i = y; cy.y = nn.i; cy.fresh = 1;
                // The next pass starts without a workgroup barrier, and a wave reads LDS behind its own writes: the values are written by the ONE wave whose
                // thread reads slot py in the pass (slot p belongs to thread p % T).  (Until round 5 lane 0 of EVERY wave wrote them: a wave that fell a
                // whole pass behind then overwrote the update the next merge had already made to the slot -- a wrong late merge in ~4 % of the runs of a
                // 2 200-row job with 16 waves per workgroup, none seen with 8 or 4; found by tools/linkage_fuzz.py, profiles/r05_linkage_fuzz.txt.)
                if (own(y)) {
                    const int py = slot(y);
                    if (lane == 0 && wv == ((py % T) >> 6)) { l_nb[py] = nn.i; l_md[py] = nn.v; l_md2[py] = nn.v2; l_fr[py] = 1; }
                    if (tid == 0) { STX<ONEX>(&nb[y], nn.i); STX<ONEX>(&md[y], nn.v); }
                }
            } else {
                cy.v = LDG(&md[y]); cy.i = y; cy.y = LDG(&nb[y]); cy.fresh = 0;
                if (own(y)) { const int py = slot(y); if (lane == 0 && wv == ((py % T) >> 6)) l_fr[py] = 0; }
            }
            best = cbetter(best, cy);
            __builtin_amdgcn_wave_barrier();       // keep the LDS stores above in front of the next pass's LDS loads in the instruction stream
        }
        lp ^= 1;
        if (!((best.fresh & 1) && best.y >= 0)) pick_stale(cy, lp);
        x = best.i; dist = best.v; y = best.y; fresh = (best.fresh & 1) != 0;
        prefetch_pair();
    }
}

// per-workgroup private copies for k_linkage_mw: [G][n] sizes (all 1); square form: [G][2 n] = sizes (1) followed by ty (-1)
__global__ void k_fill_size_ty(int* p, int64_t n, int64_t total, int with_ty)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < total) p[i] = (with_ty && ((i / n) & 1)) ? -1 : 1;
}

// ---------------------------------------------------------------- launchers (declared in linkage_dev.h)
bool linkage_mw_has(int method) { return method == LW_CENTROID; }
int linkage_mw_max_workgroups() { return MWT; }         // s_words / s_cand hold one slot per workgroup
int linkage_mw_slot_granules() { return SLOT_WORDS; }
// workspace cl_size_all: every workgroup's private copy of the sizes (square form: and of ty), as a job starts
int linkage_mw_prepare(sd_ctx* c, int64_t N, int G, bool square, int** size_all)
{
    const int64_t priv = (int64_t)G * N * (square ? 2 : 1);
    WS(c, int, sa, "cl_size_all", priv);
    hipLaunchKernelGGL(k_fill_size_ty, dim3((unsigned)((priv + 255) / 256)), dim3(256), 0, c->stream, sa, N, priv, square ? 1 : 0);
    KCHECK(c);
    *size_all = sa;
    return SD_OK;
}
hipError_t linkage_mw_launch(sd_ctx* c, bool onex, bool square, int G, int TH, double* D, int n, int* size_all, int* cid, int* nb, double* md, const double* md2,
                             double* Z, MwGran* gran, unsigned* sync, int cap)
{
    const void* f = onex ? (square ? (const void*)k_linkage_mw<true, true> : (const void*)k_linkage_mw<true, false>)
                         : (square ? (const void*)k_linkage_mw<false, true> : (const void*)k_linkage_mw<false, false>);
    const size_t dyn = (size_t)cap * 32;
    if (dyn > 48 * 1024) {          // the row lists of a hand-set geometry may pass the default dynamic-LDS limit
        (void)hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        (void)hipGetLastError();
    }
    void* args[] = {&D, &n, &size_all, &cid, &nb, &md, &md2, &Z, &gran, &sync, &cap, &G};
    // cooperative launch: all workgroups are resident together, or the launch is refused (they poll each other's slots)
    return hipLaunchCooperativeKernel(f, dim3(onex ? 8 * G : G), dim3(TH), args, dyn, c->stream);
}
