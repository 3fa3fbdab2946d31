// linkage_rg_body.inc -- the body of k_linkage_rg, from its first declaration to the end of the merge loop, included by k_linkage_rg and by its batched twin
// k_linkage_rg_jobs (linkage_rg.hip) and by nothing else.  Not a header: it is the inside of a __global__ function, which must have in scope
//   ONEX, UU, METHOD                    compile-time: the one-XCD form, columns per thread, the linkage method
//   D, n, cid, nb0, md0, md20, Z, gran, sync, cap, G, helper, k0, sz0, ty0      what k_linkage_rg takes as arguments (see there)
//   rg_xcc                              ONEX: the XCC whose workgroups take part
// A function would be the plainer way to share it; it was tried and moved the register allocation of every existing instantiation (+4 VGPRs on the 256-thread
// forms, +20 bytes of scratch on the 1024-thread one; profiles/linkage_xcd_descriptors.txt), and this kernel's time follows its registers (DESIGN 4.1).  Included
// text compiles to what the kernel compiled to before.
    extern __shared__ __attribute__((aligned(16))) int dyn_lds[];
    // what the cooperative row scans of a retry round need of a column they do not own in registers: last rewrite, cluster size, "gone"
    int* l_ty = dyn_lds;                              // [cap]
    int* l_sz = l_ty + cap;                           // [cap]
    unsigned char* l_dead = (unsigned char*)(l_sz + cap);   // [cap]
    __shared__ RQ sh_q[RG_T_MAX / 64];
    __shared__ RCand sh_c[RG_T_MAX / 64];
    __shared__ int sh_tie[RG_T_MAX / 64];
    __shared__ RQ s_part[RG_KR][RG_T_MAX / 64];
    __shared__ RQ s_row[RG_KR];
    __shared__ unsigned s_words[RG_GMAX][RG_SLOT + 1];   // this round's slots as received (+1: lane u reads word w of slot u)
    __shared__ RCand s_cand[RG_GMAX + 1];
    __shared__ int s_L[2][RG_KR], s_Lty[2][RG_KR], s_Lsz[2][RG_KR];
    __shared__ int s_nL[2];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // helper = 1: the last wave owns no columns and takes no part in the hand-offs; after every merge it requests the rows of the runner-up
    // neighbours of the new cluster for this workgroup's columns, so that they sit in the XCD's L2 when one of them becomes the next merge's
    // partner (on clustered data the new cluster is in 97 % of the next merges, and its partner was the 2nd or 3rd nearest one or two merges
    // before in 85 % of them: profiles/r05_linkage_*.txt).  Results do not depend on it.
    const int T = (int)blockDim.x - (helper ? 64 : 0), NW = (int)blockDim.x >> 6;
    const bool is_helper = helper && wv == NW - 1;
    int g = blockIdx.x;
    if constexpr (ONEX) {
        // 8 G workgroups were launched; the first G that find themselves on XCC rg_xcc take part (rank = ticket), the others leave (k_linkage_mw)
        __shared__ int s_ticket;
        if (tid == 0) {
            const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));       // HW_REG_XCC_ID[3:0]
            s_ticket = (xcc == rg_xcc) ? (int)atomicAdd(&sync[SYNC_TICKET], 1u) : -1;
        }
        __syncthreads();
        g = s_ticket;
        if (g < 0 || g >= G) return;
    }
    const int64_t N = n;
    const int colsB = cap - 1;
    const int z0 = g * colsB;
    const int nown = n - z0 < colsB ? (n - z0 > 0 ? n - z0 : 0) : colsB;
    const int nu = (nown + T - 1) / T;                       // register slots in use (uniform over the workgroup), <= UU
    const int zsafe = z0 < n ? z0 : 0;                       // a valid column for the loads of idle register slots
    unsigned bar = 0;
    int par = 0, lp = 0;

    // ---- per-column state, registers
    int zc[UU], c_nb[UU], c_fl[UU], c_ty[UU], c_sz[UU], c_nbsz[UU], c_nbty[UU];
    double c_md[UU], c_md2[UU];
#pragma unroll
    for (int u = 0; u < UU; ++u) {
        const int p = tid + u * T;
        const int z = (!is_helper && p < nown) ? z0 + p : -1;
        zc[u] = z;
        const bool row = z >= 0 && z < n - 1;
        c_md[u] = row ? md0[z] : (double)INFINITY; c_md2[u] = row ? md20[z] : (double)INFINITY; c_nb[u] = row ? nb0[z] : -1;
        c_fl[u] = z >= 0 ? 1 : 2;                               // bit 0 fresh, bit 1 gone (or no column)
        c_ty[u] = -1; c_sz[u] = 1; c_nbsz[u] = 1; c_nbty[u] = -1;
        if (sz0 && z >= 0) {                                    // continuing behind k0 merges another kernel made (run_linkage: the heap replay took the duplicates)
            c_sz[u] = sz0[z]; c_ty[u] = ty0[z];
            if (c_sz[u] == 0) { c_fl[u] = 2; c_nb[u] = -1; c_md[u] = (double)INFINITY; c_md2[u] = (double)INFINITY; }
            if (c_nb[u] >= 0) { c_nbsz[u] = sz0[c_nb[u]]; c_nbty[u] = ty0[c_nb[u]]; }
        }
        if (z >= 0) { l_ty[p] = c_ty[u]; l_sz[p] = c_sz[u]; l_dead[p] = (c_fl[u] & 2) ? 1 : 0; }
    }
    if (tid == 0) { s_nL[0] = 0; s_nL[1] = 0; }
    __syncthreads();

    // receive round `bar` of every workgroup's slot (nw words each) into s_words; false on timeout
    auto consume = [&](int nw) -> bool {
        const MwGran* base = gran + (size_t)par * G * RG_SLOT;
        bool ok = true;
        const int total = G * nw;
        // a thread's granules are requested together and re-requested together until all of them carry this round's tag (one after the other each
        // would cost its own round trip to the L2: 3 in a row for some threads at 32 workgroups x 16 words and 256 threads)
        for (int i0 = is_helper ? total : tid; i0 < total; i0 += 4 * T) {
            const MwGran* p[4]; MwGran v[4]; int sl[4], wd[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int idx = i0 + j * T;
                const int ic = idx < total ? idx : i0;
                sl[j] = ic / nw; wd[j] = ic - sl[j] * nw;
                p[j] = base + (size_t)sl[j] * RG_SLOT + wd[j];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = LDG(p[j]);
            unsigned spins = 0;
            for (;;) {
                bool pend = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) pend |= (unsigned)(v[j] >> 32) != bar;
                if (!pend) break;
                __builtin_amdgcn_s_sleep(1);
#pragma unroll
                for (int j = 0; j < 4; ++j) if ((unsigned)(v[j] >> 32) != bar) v[j] = LDG(p[j]);
                if (++spins > (1u << 24)) { sync[SYNC_TIMEOUT] = 1; ok = false; break; }     // ~seconds: never in a healthy run
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) if (i0 + j * T < total) s_words[sl[j]][wd[j]] = (unsigned)v[j];
        }
        return __syncthreads_and(ok ? 1 : 0) != 0;
    };
    auto word_d = [&](int sl, int wd) -> double {
        return __longlong_as_double((long long)(((unsigned long long)s_words[sl][wd + 1] << 32) | s_words[sl][wd]));
    };
    auto slot_cand = [&](int u) -> RCand {
        RCand c; c.v = word_d(u, 0); c.i = (int)s_words[u][2]; c.y = (int)s_words[u][3]; c.fl = (int)s_words[u][4] & ~RG_ROWTIE;
        c.szi = (int)s_words[u][5]; c.szy = (int)s_words[u][6]; c.tyi = (int)s_words[u][7]; c.tyy = (int)s_words[u][8];
        return c;
    };
    auto slot_q = [&](int u, int base) -> RQ {
        RQ q; q.v = word_d(u, base); q.i = (int)s_words[u][base + 2]; q.v2 = word_d(u, base + 3); q.sz = (int)s_words[u][base + 5]; q.ty = (int)s_words[u][base + 6];
        return q;
    };
    // the workgroup's slot for the next round, one store instruction of wave 0 (lane w stores word w).  Every wave has drained its
    // stores to the distance matrix in front of the barrier that precedes this call: whoever sees the slot may read them.
    auto publish = [&](const RCand& m, const RQ& q, int row_tie, int nL, const RQ* rows /*LDS*/) {
        ++bar;
        if (wv == 0) {
            MwGran* sl = gran + ((size_t)par * G + g) * RG_SLOT;
            const MwGran tag = (MwGran)bar << 32;
            unsigned w = 0;
            bool on = false;
            if (lane < RG_CW) {
                on = true;
                w = lane == 0 ? lo32(m.v) : lane == 1 ? hi32(m.v) : lane == 2 ? (unsigned)m.i : lane == 3 ? (unsigned)m.y : lane == 4 ? (unsigned)(m.fl | (row_tie ? RG_ROWTIE : 0))
                  : lane == 5 ? (unsigned)m.szi : lane == 6 ? (unsigned)m.szy : lane == 7 ? (unsigned)m.tyi : (unsigned)m.tyy;
            } else if (nL == 0) {
                if (lane < RG_CW + RG_QW) { on = true; w = rq_word(q, lane - RG_CW); }
            } else if (lane < RG_CW + RG_QW * nL) {
                const int r = (lane - RG_CW) / RG_QW;
                const RQ t = rows[r];
                on = true; w = rq_word(t, lane - RG_CW - RG_QW * r);
            }
            if (on) STX<ONEX>(&sl[lane], tag | (MwGran)w);
        }
    };
    // after consume(): every WAVE folds the G slots itself -- global best, NN(y), "row x had a second pair"
    RCand d_best = rc_none(); RQ d_nn = rq_none(); int d_rowtie = 0;
    auto digest = [&](int nLprev, const int* Lprev, const int* Lprev_ty, const int* Lprev_sz, bool with_nn) {
        if (tid < G) s_cand[tid] = slot_cand(tid);          // kept for pick_stale (read there behind a barrier)
        if (nLprev > 0) {
            for (int r = wv; r < nLprev; r += NW) {          // refreshed rows: one wave folds the G partial minima of a row
                RQ a = rq_none();
                for (int u = lane; u < G; u += 64) a = rq_merge(a, slot_q(u, RG_CW + RG_QW * r));
                a = wave_min_rq(a);
                if (lane == 0) s_row[r] = a;
            }
            __syncthreads();
        }
        RCand b = rc_none();
        RQ a = rq_none();
        int rt = 0;
        for (int u = lane; u < G; u += 64) {
            b = rc_better(b, slot_cand(u));
            if (with_nn) a = rq_merge(a, slot_q(u, RG_CW));
            if (nLprev == 0) rt |= (int)s_words[u][4] & RG_ROWTIE;
        }
        if (lane < nLprev) {           // the rows refreshed in this round are exact now
            const RQ q = s_row[lane];
            RCand c; c.i = Lprev[lane]; c.y = q.i; c.v = (q.i < 0) ? (double)INFINITY : q.v; c.fl = 1;
            c.szi = Lprev_sz[lane]; c.tyi = Lprev_ty[lane]; c.szy = q.sz; c.tyy = q.ty;
            if (c.y >= 0) b = rc_better(b, c);
        }
        d_best = wave_min_rc(b);
        if (with_nn) d_nn = wave_min_rq(a);
        d_rowtie = (nLprev == 0 && __ballot(rt != 0) != 0ull) ? 1 : 0;
        if (nLprev > 0) {
            // the owner of a refreshed row takes it into its registers
            for (int r = 0; r < nLprev; ++r) {
                const int xr = Lprev[r];
                const RQ q = s_row[r];
#pragma unroll
                for (int u = 0; u < UU; ++u)
                    if (zc[u] == xr) {
                        c_nb[u] = q.i; c_md[u] = (q.i < 0) ? (double)INFINITY : q.v; c_md2[u] = (q.i < 0) ? (double)INFINITY : q.v2;
                        c_fl[u] = (c_fl[u] & 2) | 1; c_nbsz[u] = q.sz; c_nbty[u] = q.ty;
                    }
            }
        }
    };
    // local arg-min over the owned active rows, skipping the rows being refreshed this round
    auto local_argmin = [&](int nL, const int* L) -> RCand {
        int ex[RG_KR];
#pragma unroll
        for (int r = 0; r < RG_KR; ++r) ex[r] = r < nL ? L[r] : -1;
        RCand m = rc_none();
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            const int z = zc[u];
            bool skip = z < 0 || (c_fl[u] & 2) || z >= n - 1;
#pragma unroll
            for (int r = 0; r < RG_KR; ++r) skip |= (z == ex[r]);
            if (!skip) rc_acc(m, c_md[u], z, c_nb[u], c_fl[u] & 1, c_sz[u], c_nbsz[u], c_ty[u], c_nbty[u]);
        }
        m = wave_min_rc(m);
        __syncthreads();
        if (lane == 0) sh_c[wv] = m;
        __syncthreads();
        RCand r = rc_none();
        if (lane < NW) r = sh_c[lane];
        return wave_min_rc(r);
    };
    // this workgroup's share -- its own columns -- of the nL rows in L: wave tasks (row r, sub-slice s)
    auto scan_rows = [&](int nL, const int* L, const int* Lty, RQ* outv /*LDS [RG_KR]*/) {
        if (nL <= 0) return;
        const int S = NW >= nL ? NW / nL : 1;
        for (int t = wv; t < nL * S; t += NW) {
            const int r = t % nL, sidx = t / nL;
            const int x = L[r];
            const int txr = Lty[r];
            RQ q = rq_none();
            const int64_t jend = (int64_t)z0 + nown, step = (int64_t)S * 64;
            for (int64_t j0 = (x + 1 > z0 ? x + 1 : z0) + (int64_t)sidx * 64 + lane; j0 < jend; j0 += step * 4) {
                double v[4]; bool ok[4]; int sj[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int64_t j = j0 + u * step; const int64_t jc = j < jend ? j : jend - 1;
                    sj[u] = (int)(jc - z0);
                    ok[u] = j < jend && !l_dead[sj[u]];
                    v[u] = LDG(txr >= l_ty[sj[u]] ? &D[(int64_t)x * N + jc] : &D[jc * N + x]);      // entry {x, j} from the row written last
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) if (ok[u]) rq_acc(q, v[u], (int)(j0 + u * step), l_sz[sj[u]], l_ty[sj[u]]);
            }
            q = wave_min_rq(q);
            if (lane == 0) s_part[r][sidx] = q;
        }
        __syncthreads();
        if (tid < nL) {
            RQ q = s_part[tid][0];
            for (int k2 = 1; k2 < S; ++k2) q = rq_merge(q, s_part[tid][k2]);
            outv[tid] = q;
        }
        __syncthreads();
    };
    // the next refresh list: the RG_KR best stale candidates among s_cand[0..G) and `extra`; wave 0 extracts them, every
    // workgroup arrives at the same list (with the ty and the size of each listed row's cluster)
    MinIdx none; none.v = INFINITY; none.i = -1;
    auto pick_stale = [&](const RCand& extra, int slot) {
        __syncthreads();               // s_cand of this round complete
        if (wv == 0) {
            constexpr int CU = (RG_GMAX + 1 + 63) / 64;
            MinIdx c[CU]; int oty[CU], osz[CU];
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const int idx = lane + 64 * u;
                c[u] = none; oty[u] = -1; osz[u] = 0;
                if (idx <= G) {
                    RCand o = extra;
                    if (idx < G) o = s_cand[idx];
                    if (o.i >= 0 && !(o.fl & 1) && o.v != INFINITY) { c[u].v = o.v; c[u].i = o.i; oty[u] = o.tyi; osz[u] = o.szi; }
                }
            }
            int nl = 0;
#pragma unroll
            for (int u = 0; u < CU; ++u) {
                const bool st = c[u].i >= 0;
                const unsigned long long mk = __ballot(st);
                const int at = nl + __popcll(mk & ((1ull << lane) - 1ull));
                if (st && at < RG_KR) { s_L[slot][at] = c[u].i; s_Lty[slot][at] = oty[u]; s_Lsz[slot][at] = osz[u]; }
                nl += __popcll(mk);
            }
            if (nl > RG_KR) {                       // more than RG_KR: the best by (bound, row)
                nl = 0;
                for (int r = 0; r < RG_KR; ++r) {
                    MinIdx bq = none;
#pragma unroll
                    for (int u = 0; u < CU; ++u) bq = better(bq, c[u]);
                    bq = wave_min(bq);
                    if (bq.i < 0) break;
#pragma unroll
                    for (int u = 0; u < CU; ++u)
                        if (c[u].i == bq.i) { s_L[slot][r] = bq.i; s_Lty[slot][r] = oty[u]; s_Lsz[slot][r] = osz[u]; c[u].i = -1; }
                    nl = r + 1;
                }
            }
            if (lane == 0) s_nL[slot] = nl;
        }
        __syncthreads();
    };
    RCand nocand = rc_none(); nocand.fl = 1;

    // ---- initial state: exact bounds from k_row_nn
    {
        const RCand m0 = local_argmin(0, s_L[0]);
        publish(m0, rq_none(), 0, 0, s_row);
    }
    if (!consume(RG_MW)) return;
    digest(0, s_L[0], s_Lty[0], s_Lsz[0], false);
    par ^= 1;
    RCand best = d_best;
    if (!((best.fl & 1) && best.y >= 0)) pick_stale(nocand, lp);

    for (int k = k0; k < n - 1; ++k) {
        // ---- lazy validation (cl.cpp:323-339): cooperative refresh of the best stale candidates
        for (int guard = 0; guard <= n - k; ++guard) {
            if ((best.fl & 1) && best.y >= 0) break;
            if (g == 0 && tid == 0) sync[SYNC_ROUNDS] += 1;            // diagnostic: retry rounds
            const int nL = s_nL[lp]; const int* L = s_L[lp];
            scan_rows(nL, L, s_Lty[lp], s_row);
            const RCand m = local_argmin(nL, L);
            publish(m, rq_none(), 0, nL, s_row);
            if (!consume(nL > 0 ? RG_CW + RG_QW * nL : RG_MW)) return;
            digest(nL, L, s_Lty[lp], s_Lsz[lp], false);
            par ^= 1;
            best = d_best;
            lp ^= 1;
            if (!((best.fl & 1) && best.y >= 0)) pick_stale(nocand, lp);
        }
        if (best.fl & CAND_TIE) {      // the closest pair is not unique: the heap decides (run_linkage); the height of the tie goes along
            if (g == 0 && tid == 0) { sync[SYNC_TIE] = 1; sync[SYNC_TIE_LO] = lo32(best.v); sync[SYNC_TIE_HI] = hi32(best.v); }
            return;
        }
        // ---- merge (x, y) at height dist; everything about the pair came with the candidate
        const int x = best.i, y = best.y;
        const double dist = best.v;
        const int nx = best.szi, ny = best.szy, txm = best.tyi, tym = best.tyy;
        int cx_pre = 0, cy_pre = 0;
        if (g == 0 && tid == 0) { cx_pre = cid[x]; cy_pre = cid[y]; }      // dendrogram ids of the pair (this thread is their only reader and writer)
        auto write_Z = [&]() {
            if (tid == 0 && g == 0) {
                int ix = cx_pre, iy = cy_pre;
                if (ix > iy) { const int t = ix; ix = iy; iy = t; }
                Z[(size_t)k * 4 + 0] = (double)ix; Z[(size_t)k * 4 + 1] = (double)iy;
                Z[(size_t)k * 4 + 2] = dist;       Z[(size_t)k * 4 + 3] = (double)(nx + ny);
                cid[y] = n + k;
            }
        };
        if (k == n - 2) { write_Z(); break; }
        // ---- one pass over the owned active columns: Lance-Williams update + neighbour patches (cl.cpp:361-392), NN(y) partial
        // from the fresh distances (cl.cpp:395-404), next local arg-min
        RQ q = rq_none();
        RCand m = rc_none();
        int row_tie = 0;
        double dzx[UU], dzy[UU]; bool act[UU];
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            act[u] = false;
            if (u < nu && !is_helper) {
                const int z = zc[u];
                act[u] = z >= 0 && !(c_fl[u] & 2) && z != x && z != y;
                const int zl = act[u] ? z : zsafe;
                // the row copies are requested at once; where a bystander's row was written after the pair's, the entry is fetched from there below
                dzx[u] = LDG(&D[(int64_t)x * N + zl]);
                dzy[u] = LDG(&D[(int64_t)y * N + zl]);
            }
        }
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            if (u < nu && act[u]) {
                if (txm < c_ty[u]) dzx[u] = LDG(&D[(int64_t)zc[u] * N + x]);        // z's row was written after x's: the current {z, x} is there
                if (tym < c_ty[u]) dzy[u] = LDG(&D[(int64_t)zc[u] * N + y]);
            }
        }
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            if (!(u < nu && act[u])) continue;
            const int z = zc[u];
            const double nd = lw_update<METHOD>(dzx[u], dzy[u], dist, nx, ny, c_sz[u]);
            STX<ONEX>(&D[(int64_t)y * N + z], nd);
            if (z > x && dzx[u] == dist) row_tie = 1;         // row x had a second neighbour at exactly the merge height
            double mz = (z < n - 1) ? c_md[u] : (double)INFINITY;
            int nz = c_nb[u], fz = c_fl[u] & 1;
            if (z < y) {
                // row z's entries above the diagonal: x's is gone (if z < x), y's is nd now.  Invariants: mz <= every active entry of the row
                // (the reference's lower bound), m2 <= every active entry OTHER than the neighbour's (k_linkage_mw)
                const double m2 = fmax(c_md2[u], mz);
                if ((z < x && nz == x) || nz == y) {
                    nz = y;
                    if (nd <= m2) { mz = nd; fz = 1; } else { mz = m2; fz = 0; }
                    c_md[u] = mz; c_md2[u] = m2; c_nb[u] = y; c_fl[u] = fz; c_nbsz[u] = nx + ny; c_nbty[u] = k;
                } else if (nd < mz) {
                    c_md2[u] = mz;
                    nz = y; mz = nd; fz = 1; c_md[u] = nd; c_nb[u] = y; c_fl[u] = 1; c_nbsz[u] = nx + ny; c_nbty[u] = k;
                } else if (nd < m2) c_md2[u] = nd;
            } else rq_acc(q, nd, z, c_sz[u], c_ty[u]);
            if (z < n - 1) rc_acc(m, mz, z, nz, fz, c_sz[u], c_nbsz[u], c_ty[u], c_nbty[u]);
        }
        write_Z();
        // ---- the two reductions and the flag through ONE LDS exchange; the stores of this wave have landed before its record is visible
        q = wave_min_rq(q);
        m = wave_min_rc(m);
        const int tie_w = __ballot(row_tie != 0) != 0ull ? 1 : 0;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) { sh_q[wv] = q; sh_c[wv] = m; sh_tie[wv] = tie_w; }
        __syncthreads();
        if (NW <= 8) {            // few waves: every lane folds the records itself (LDS broadcast reads) -- shorter than two more DPP reductions
            q = sh_q[0]; m = sh_c[0]; row_tie = sh_tie[0];
            for (int w2 = 1; w2 < NW; ++w2) { q = rq_merge(q, sh_q[w2]); m = rc_better(m, sh_c[w2]); row_tie |= sh_tie[w2]; }
        } else {
            RQ rq = rq_none(); RCand rc = rc_none(); int rt = 0;
            if (lane < NW) { rq = sh_q[lane]; rc = sh_c[lane]; rt = sh_tie[lane]; }
            q = wave_min_rq(rq);
            m = wave_min_rc(rc);
            row_tie = __ballot(rt != 0) != 0ull ? 1 : 0;
        }
        // ---- the pair's own columns: x is gone, y is the merged cluster, rewritten in this merge
#pragma unroll
        for (int u = 0; u < UU; ++u) {
            if (zc[u] == x) { c_fl[u] |= 2; l_dead[tid + u * T] = 1; }
            if (zc[u] == y) { c_sz[u] = nx + ny; c_ty[u] = k; l_sz[tid + u * T] = nx + ny; l_ty[tid + u * T] = k; }
        }
        publish(m, q, row_tie, 0, s_row);
        if (!consume(RG_MW)) return;
        digest(0, s_L[lp], s_Lty[lp], s_Lsz[lp], true);
        par ^= 1;
        if (d_rowtie) { if (g == 0 && tid == 0) { sync[SYNC_TIE] = 1; sync[SYNC_TIE_LO] = lo32(dist); sync[SYNC_TIE_HI] = hi32(dist); } return; }     // (this merge's stores into row y are out, and so is row k of Z: run_linkage reads from Z's row 0 whether the matrix is still what linkage_prepare left)
        best = d_best;
        const RQ nn = d_nn;
        // row y: exact by construction (cl.cpp:395-404).  Without an active column above it the row has no pair left, now or later
        // (columns are only ever removed): exact bound +inf
        RCand cy = rc_none();
        if (y < n - 1) {
            if (nn.i >= 0) { cy.v = nn.v; cy.i = y; cy.y = nn.i; cy.fl = 1; cy.szi = nx + ny; cy.szy = nn.sz; cy.tyi = k; cy.tyy = nn.ty; }
#pragma unroll
            for (int u = 0; u < UU; ++u)
                if (zc[u] == y) {
                    c_nb[u] = nn.i; c_md[u] = nn.i >= 0 ? nn.v : (double)INFINITY; c_md2[u] = nn.i >= 0 ? nn.v2 : (double)INFINITY;
                    c_fl[u] = (c_fl[u] & 2) | 1; c_nbsz[u] = nn.sz; c_nbty[u] = nn.ty;
                }
            best = rc_better(best, cy);
        }
        if (is_helper) {
            // the two best local NN(y) candidates other than the winner (whose row the pass requests right now)
            double qv = INFINITY; int qi = -1;
            if (lane < G) { const RQ t = slot_q(lane, RG_CW); qv = t.v; qi = t.i; }
            if (qi == nn.i || qi < 0) qv = INFINITY;
            for (int e = 0; e < 2; ++e) {
                unsigned long long mm;
                const double v = wave_argmin_d(qv, mm);
                const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)mm) - 1);
                const int r = v < (double)INFINITY ? __builtin_amdgcn_readlane(qi, l) : -1;
                if (lane == l) qv = INFINITY;
                if (r >= 0) {
                    // requests whose data nobody waits for: the loads pull the lines into the L2, the register they land in is never read
                    const double* row = D + (int64_t)r * N + z0;
                    for (int j = lane; j < nown; j += 64) {
                        double dump;
                        asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(dump) : "v"(row + j) : "memory");
                    }
                }
            }
        }
        lp ^= 1;
        if (!((best.fl & 1) && best.y >= 0)) pick_stale(cy, lp);
    }
