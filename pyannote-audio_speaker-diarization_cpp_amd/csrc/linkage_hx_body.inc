// linkage_hx_body.inc -- the body of k_linkage_hx, from its first declaration to the end of the workers' loop, included by k_linkage_hx and by its batched twin
// k_linkage_hx_jobs (linkage_hx.hip) and by nothing else.  Not a header: it is the inside of a __global__ function, which must have in scope
//   ONEX, S16, METHOD                   compile-time: the one-XCD form, 16-bit heap keys / positions in LDS, the linkage method
//   D, n, cid, size, tyv, nb, md, Z, g_hval, g_hkey, g_hpos, cmd, rep, chg_z, chg_v, sync, cap, G, lc, stop_above      what k_linkage_hx takes as arguments (see there)
//   hx_xcc                              ONEX: the XCC whose workgroups take part
// Shared by inclusion and not by a function for the reason linkage_rg_body.inc gives (profiles/linkage_xcd_zero_descriptors.txt): included text compiles to what
// the kernel compiled to before.
    extern __shared__ __attribute__((aligned(16))) int dyn_lds[];     // master: heap tier [lc] doubles + [lc] ints
    __shared__ MinIdx sh[HX_T / 64];
    __shared__ int s_cnt[HX_U][HX_T / 64];
    __shared__ unsigned s_rep[HX_GMAX][HX_REPW];
    __shared__ int s_pre[HX_GMAX + 1];
    __shared__ int st_z[HX_STAGE];
    __shared__ double st_v[HX_STAGE];
    __shared__ int s_x, s_y, s_ok, s_tx, s_ty, s_nx, s_ny;
    __shared__ double s_d;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    constexpr int NW = HX_T / 64;
    int g = blockIdx.x;
    if constexpr (ONEX) {
        // 8 (G + 1) workgroups were launched; the first G + 1 that find themselves on XCC hx_xcc take part (rank = ticket), the others leave
        __shared__ int s_ticket;
        if (tid == 0) {
            const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (3 << 11));       // HW_REG_XCC_ID[3:0]
            s_ticket = (xcc == hx_xcc) ? (int)atomicAdd(&sync[SYNC_TICKET], 1u) : -1;
        }
        __syncthreads();
        g = s_ticket;
        if (g < 0 || g > G) return;
    }
    const int64_t N = n;
    unsigned seq = 0;                       // commands sent / received so far
    // one 8-byte granule = {payload word, tag}
    auto poll = [&](const MwGran* p, unsigned tag, bool& ok) -> unsigned {
        MwGran v = LDG(p);
        unsigned spins = 0;
        while ((unsigned)(v >> 32) != tag) {
            __builtin_amdgcn_s_sleep(1);
            v = LDG(p);
            if (++spins > (1u << 24)) { sync[SYNC_TIMEOUT] = 1; ok = false; break; }     // ~seconds: never in a healthy run
        }
        return (unsigned)v;
    };

    if (g == 0) {
        // =============================================================== master: the reference's loop, heap included
        HxHeap<S16> h;
        h.lv = (double*)dyn_lds; h.gv = g_hval; h.lk16 = (unsigned short*)(h.lv + lc); h.lp16 = h.lk16 + n; h.gk = g_hkey; h.gp = g_hpos; h.lc = lc; h.size = n - 1;
        for (int i = tid; i < n - 1; i += HX_T) { h.setV(i, md[i]); h.setK(i, i); h.setP(i, i); }          // cl.cpp:80-91
        __syncthreads();
        if (tid == 0) for (int i = h.size / 2; i >= 0; --i) hx_down(h, i);                                  // cl.cpp:94
        __syncthreads();
        // command record: every thread knows the words (LDS), wave 0 stores them; the caller has drained the master's own stores (nb / md of
        // the rows it decided) before
        auto send = [&](int op, int x, int y, double d, int nx, int ny, int tx, int ty, int k) {
            ++seq;
            if (wv == 0 && lane < HX_CMDW) {
                const unsigned w = lane == 0 ? (unsigned)op : lane == 1 ? (unsigned)x : lane == 2 ? (unsigned)y : lane == 3 ? (unsigned)__double2loint(d) : lane == 4 ? (unsigned)__double2hiint(d)
                                 : lane == 5 ? (unsigned)nx : lane == 6 ? (unsigned)ny : lane == 7 ? (unsigned)tx : lane == 8 ? (unsigned)ty : (unsigned)k;
                STX<ONEX>(&cmd[lane], ((MwGran)seq << 32) | (MwGran)w);
            }
        };
        auto recv = [&]() -> bool {            // the G replies to command `seq` -> s_rep
            bool ok = true;
            for (int idx = tid; idx < G * HX_REPW; idx += HX_T) {
                const int sl = idx / HX_REPW, wd = idx - sl * HX_REPW;
                s_rep[sl][wd] = poll(&rep[(size_t)sl * 8 + wd], seq, ok);
            }
            return __syncthreads_and(ok ? 1 : 0) != 0;
        };
        auto fold_nn = [&]() -> MinIdx {       // lowest value, lowest column among equals: what a sequential scan in ascending j finds first
            MinIdx q; q.v = INFINITY; q.i = -1;
            for (int u = tid; u < G; u += HX_T) {
                MinIdx c; c.i = (int)s_rep[u][1];
                c.v = __hiloint2double((int)s_rep[u][3], (int)s_rep[u][2]);
                q = better(q, c);
            }
            q = wave_min(q);
            __syncthreads();
            if (lane == 0) sh[wv] = q;
            __syncthreads();
            MinIdx r = sh[0];
#pragma unroll
            for (int w2 = 1; w2 < NW; ++w2) r = better(r, sh[w2]);
            return r;
        };
        for (int k = 0; k < n - 1; ++k) {
            int x = 0, y = 0; double dist = 0.0;
            for (int guard = 0; guard < n - k; ++guard) {                                                // cl.cpp:323
                if (tid == 0) {
                    const int hx = h.K(0); const double hd = h.V(0); const int hy = LDG(&nb[hx]);        // get_min
                    const int tx = tyv[hx], ty = hy >= 0 ? tyv[hy] : -1;
                    s_x = hx; s_y = hy; s_d = hd; s_tx = tx; s_ty = ty;
                    s_ok = (hy >= 0) && (hd == LDG(tx >= ty ? &D[(int64_t)hx * N + hy] : &D[(int64_t)hy * N + hx]));   // cl.cpp:329
                }
                __syncthreads();
                x = s_x; y = s_y; dist = s_d;
                const int ok = s_ok, tx = s_tx;
                __syncthreads();
                if (ok) break;
                // stale candidate: row x's true nearest neighbour (cl.cpp:333-338), every worker scans its own columns
                if (g == 0 && tid == 0) sync[SYNC_ROUNDS] += 1;
                send(HX_OP_SCAN, x, 0, 0.0, 0, 0, tx, 0, k);
                if (!recv()) return;
                const MinIdx q = fold_nn();
                y = q.i; dist = (q.i < 0) ? (double)INFINITY : q.v;
                if (tid == 0) {
                    STX<ONEX>(&nb[x], y); STX<ONEX>(&md[x], dist);
                    hx_change(h, x, dist);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                }
                __syncthreads();
            }
            if (y < 0) { if (tid == 0) { Z[(size_t)k * 4 + 3] = NAN; sync[SYNC_TIMEOUT] = 1; } send(HX_OP_QUIT, 0, 0, 0.0, 0, 0, 0, 0, 0); return; }   // cannot happen while two clusters are active
            if (dist > stop_above) {                 // the caller continues from here with the cooperative kernel (run_linkage: duplicates merged, the rest is tie-free)
                if (tid == 0) sync[SYNC_MERGES] = (unsigned)k;
                send(HX_OP_QUIT, 0, 0, 0.0, 0, 0, 0, 0, 0);
                return;
            }
            if (tid == 0) { s_nx = size[x]; s_ny = size[y]; s_tx = tyv[x]; s_ty = tyv[y]; }
            __syncthreads();
            const int nx = s_nx, ny = s_ny, txm = s_tx, tym = s_ty;
            const bool last = (k == n - 2);
            if (!last) send(HX_OP_MERGE, x, y, dist, nx, ny, txm, tym, k);
            if (tid == 0) {
                hx_swap(h, 0, h.size - 1); h.size -= 1; hx_down(h, 0);                                   // remove_min, cl.cpp:101-105 (while the workers run their pass)
                int ix = cid[x], iy = cid[y];
                if (ix > iy) { const int t = ix; ix = iy; iy = t; }
                Z[(size_t)k * 4 + 0] = (double)ix; Z[(size_t)k * 4 + 1] = (double)iy;
                Z[(size_t)k * 4 + 2] = dist;       Z[(size_t)k * 4 + 3] = (double)(nx + ny);
                size[x] = 0; size[y] = nx + ny; cid[y] = n + k; tyv[y] = k;
            }
            if (last) break;
            if (!recv()) return;
            // change_value(z, D[z,y]) for the rows whose bound dropped, ascending z (cl.cpp:381-392): the workers' lists in worker order
            if (tid == 0) { int a = 0; for (int u = 0; u < G; ++u) { s_pre[u] = a; a += (int)s_rep[u][0]; } s_pre[G] = a; }
            __syncthreads();
            const int total = s_pre[G];
            for (int b0 = 0; b0 < total; b0 += HX_STAGE) {
                const int cnt = total - b0 < HX_STAGE ? total - b0 : HX_STAGE;
                for (int e = tid; e < cnt; e += HX_T) {
                    const int ge = b0 + e;
                    int lo = 0, hi = G - 1;                       // worker whose list holds entry ge: the last u with s_pre[u] <= ge
                    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (s_pre[mid] <= ge) lo = mid; else hi = mid - 1; }
                    const size_t src = (size_t)lo * cap + (ge - s_pre[lo]);
                    st_z[e] = LDG(&chg_z[src]); st_v[e] = LDG(&chg_v[src]);
                }
                __syncthreads();
                // change_value for every staged row, in list order.  A decrease whose new value is still >= its parent's moves nothing (cl.cpp:44-51:
                // the sift-up loop ends at once); a parent's value only ever DROPS while the list is worked off, so an entry that passes that test against
                // the heap as it stands passes it whenever its turn comes, and a run of such entries can be written at once.  Wave 0 takes 64 entries at a
                // time: the lanes in front of the first entry that WOULD move write their values together, that entry is sifted by its lane alone,
                // and the rest of the chunk is looked at again (on clustered data most bounds drop by a little and stay where they are).
                if (wv == 0) {
                    int e0 = 0;
                    while (e0 < cnt) {
                        const int e = e0 + lane;
                        const bool valid = e < cnt;
                        int idx = 0; double v = 0.0; bool stay = false;
                        if (valid) {
                            idx = h.P(st_z[e]); v = st_v[e];
                            stay = idx == 0 || !(h.V((idx - 1) >> 1) > v);
                        }
                        const unsigned long long mv = __ballot(valid && !stay);
                        const int f = mv ? __builtin_ctzll(mv) : 64;               // first lane whose entry moves
                        if (valid && lane < f) h.setV(idx, v);
                        __builtin_amdgcn_wave_barrier();
                        if (f < 64) {
                            if (lane == f) hx_decrease(h, st_z[e], st_v[e]);
                            e0 += f + 1;
                        } else e0 += 64;
                        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");   // this pass's heap writes are done before the next pass reads the heap
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                __syncthreads();
            }
            if (y < n - 1) {                                                                             // cl.cpp:395-404
                const MinIdx q = fold_nn();
                if (tid == 0 && q.i >= 0) { STX<ONEX>(&nb[y], q.i); STX<ONEX>(&md[y], q.v); hx_change(h, y, q.v); }
            }
            if (tid == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // nb / md of row y have landed before the next command is visible
            __syncthreads();
        }
        if (tid == 0) sync[SYNC_MERGES] = (unsigned)(n - 1);
        send(HX_OP_QUIT, 0, 0, 0.0, 0, 0, 0, 0, 0);
        return;
    }

    // =================================================================== workers
    const int wk = g - 1;
    const int colsB = cap;
    const int z0 = wk * colsB;
    const int nown = n - z0 < colsB ? (n - z0 > 0 ? n - z0 : 0) : colsB;
    const int nu = (nown + HX_T - 1) / HX_T;
    const int zsafe = z0 < n ? z0 : 0;
    int zc[HX_U], c_ty[HX_U]; bool c_dead[HX_U];
    int c_sz[HX_U];                         // size of the column's cluster: the one method whose update needs it (ward) keeps it here, as k_linkage_rg does
#pragma unroll
    for (int u = 0; u < HX_U; ++u) { const int p = tid + u * HX_T; zc[u] = p < nown ? z0 + p : -1; c_ty[u] = -1; c_dead[u] = zc[u] < 0; c_sz[u] = 1; }
    auto reply = [&](unsigned w0, unsigned w1, double v) {
        if (wv == 0 && lane < HX_REPW) {
            const unsigned w = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? (unsigned)__double2loint(v) : (unsigned)__double2hiint(v);
            STX<ONEX>(&rep[(size_t)wk * 8 + lane], ((MwGran)seq << 32) | (MwGran)w);
        }
    };
    auto block_nn = [&](MinIdx q) -> MinIdx {
        q = wave_min(q);
        __syncthreads();
        if (lane == 0) sh[wv] = q;
        __syncthreads();
        MinIdx r = sh[0];
#pragma unroll
        for (int w2 = 1; w2 < NW; ++w2) r = better(r, sh[w2]);
        return r;
    };
    for (;;) {
        // ---- the next command: every wave polls the record itself (lane w takes word w)
        ++seq;
        bool ok = true;
        unsigned wdv = 0;
        if (lane < HX_CMDW) wdv = poll(&cmd[lane], seq, ok);
        if (__ballot(!ok) != 0ull) return;
        const int op = __builtin_amdgcn_readlane((int)wdv, 0), x = __builtin_amdgcn_readlane((int)wdv, 1), y = __builtin_amdgcn_readlane((int)wdv, 2);
        const double dist = __hiloint2double(__builtin_amdgcn_readlane((int)wdv, 4), __builtin_amdgcn_readlane((int)wdv, 3));
        const int nx = __builtin_amdgcn_readlane((int)wdv, 5), ny = __builtin_amdgcn_readlane((int)wdv, 6);
        const int txm = __builtin_amdgcn_readlane((int)wdv, 7), tym = __builtin_amdgcn_readlane((int)wdv, 8), k = __builtin_amdgcn_readlane((int)wdv, 9);
        if (op == HX_OP_QUIT) return;
        if (op == HX_OP_SCAN) {
            // find_min_dist (cl.cpp:259-276) over this worker's columns above x: first strictly smaller in ascending j
            MinIdx q; q.v = INFINITY; q.i = -1;
            double v[HX_U]; bool in[HX_U];
#pragma unroll
            for (int u = 0; u < HX_U; ++u) {
                in[u] = false; v[u] = 0.0;
                if (u < nu) {
                    const int j = zc[u];
                    in[u] = j > x && !c_dead[u];
                    const int jl = in[u] ? j : zsafe;
                    v[u] = LDG(txm >= c_ty[u] || !in[u] ? &D[(int64_t)x * N + jl] : &D[(int64_t)jl * N + x]);      // entry {x, j} from the row written last
                }
            }
#pragma unroll
            for (int u = 0; u < HX_U; ++u) if (u < nu && in[u] && v[u] < q.v) { q.v = v[u]; q.i = zc[u]; }
            q = block_nn(q);
            reply(0u, (unsigned)q.i, q.v);
            continue;
        }
        // ---- merge (x, y) at height dist: the z loop of cl.cpp:361-392 for this worker's columns
        MinIdx q; q.v = INFINITY; q.i = -1;
        double dzx[HX_U], dzy[HX_U], mdz[HX_U], ndv[HX_U]; int nbz[HX_U]; bool act[HX_U], chg[HX_U];
#pragma unroll
        for (int u = 0; u < HX_U; ++u) {
            act[u] = false; chg[u] = false; ndv[u] = 0.0;
            if (u < nu) {
                const int z = zc[u];
                act[u] = z >= 0 && !c_dead[u] && z != x && z != y;
                const int zl = act[u] ? z : zsafe;
                dzx[u] = LDG(&D[(int64_t)x * N + zl]);
                dzy[u] = LDG(&D[(int64_t)y * N + zl]);
                const int zr = zl < n - 1 ? zl : n - 2;
                nbz[u] = LDG(&nb[zr]); mdz[u] = LDG(&md[zr]);
            }
        }
#pragma unroll
        for (int u = 0; u < HX_U; ++u) {
            if (u < nu && act[u]) {
                if (txm < c_ty[u]) dzx[u] = LDG(&D[(int64_t)zc[u] * N + x]);        // z's row was written after x's: the current {z, x} is there
                if (tym < c_ty[u]) dzy[u] = LDG(&D[(int64_t)zc[u] * N + y]);
            }
        }
#pragma unroll
        for (int u = 0; u < HX_U; ++u) {
            if (!(u < nu && act[u])) continue;
            const int z = zc[u];
            const double nd = lw_update<METHOD>(dzx[u], dzy[u], dist, nx, ny, c_sz[u]);                  // cl.cpp:367
            STX<ONEX>(&D[(int64_t)y * N + z], nd);
            if (z < x && nbz[u] == x) STX<ONEX>(&nb[z], y);                                             // cl.cpp:374-378
            if (z < y && nd < mdz[u]) { STX<ONEX>(&nb[z], y); STX<ONEX>(&md[z], nd); chg[u] = true; ndv[u] = nd; }   // cl.cpp:381-392
            if (z > y && nd < q.v) { q.v = nd; q.i = z; }                                                // cl.cpp:395-404 (ascending z per thread)
        }
#pragma unroll
        for (int u = 0; u < HX_U; ++u) {
            if (zc[u] == x && zc[u] >= 0) c_dead[u] = true;
            if (zc[u] == y && zc[u] >= 0) { c_ty[u] = k; if constexpr (METHOD == LW_WARD) c_sz[u] = nx + ny; }
        }
        // the changed rows in ascending z: column p = tid + u * T, so the order is u-major, then wave, then lane
        unsigned long long bm[HX_U];
#pragma unroll
        for (int u = 0; u < HX_U; ++u) { bm[u] = __ballot(chg[u]); if (lane == 0) s_cnt[u][wv] = __popcll(bm[u]); }
        q = block_nn(q);                      // (its barriers also publish s_cnt)
        int base[HX_U], totalc = 0;
#pragma unroll
        for (int u = 0; u < HX_U; ++u)
#pragma unroll
            for (int w2 = 0; w2 < NW; ++w2) { if (w2 == wv) base[u] = totalc; totalc += s_cnt[u][w2]; }
#pragma unroll
        for (int u = 0; u < HX_U; ++u)
            if (chg[u]) {
                const size_t dst = (size_t)wk * cap + base[u] + __popcll(bm[u] & ((1ull << lane) - 1ull));
                STX<ONEX>(&chg_z[dst], zc[u]); STX<ONEX>(&chg_v[dst], ndv[u]);
            }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // distances, neighbours, bounds and the list have landed before the reply is visible
        __syncthreads();
        reply((unsigned)totalc, (unsigned)q.i, q.v);
    }
