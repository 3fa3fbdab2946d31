// conv_res2.hip -- the f32 Res2Net convolutions (Cin = Cout = 128, three dilated taps, "same" padding, compact row space with the input
// space equal to the output space, with or without the second input) with the WEIGHTS as the stationary operand.
//
// conv_gemm.hip's 128 x 128 kernel stages 48 KB per K-step for these layers -- the rows of t1_i, of r_(i-1) and a W tile -- twelve times per
// tile: the three taps read the same rows shifted by the dilation, and every workgroup fetches the same 196 KB of W again for every tile.
// Here
//   * a wave owns 32 output columns for the whole launch and loads its slice of W once: 3 taps x 128 k x 32 columns = 192 registers per
//     lane, held in the layout of the MFMA's weight operand (as k_lstm_rec holds W_hh).  Nothing of W passes through LDS;
//   * the workgroup is persistent, one per CU, and walks the row tiles m = wg + gridDim * j.  For a tile of 128 output rows it stages the
//     rows [m0 - d, m0 + 128 + d) of u = X + X2 (added in f32 as conv_gemm.hip's lstore adds them) ONCE into an LDS panel of 136 rows x 132
//     floats (528-byte rows: conflict-free ds_read_b128).  A tap is a panel row index: conv_src_frame moves a frame by at most d (a
//     reflection about 0 or Tin - 1 by at most d, the clamp to the last stored frame towards t, an item shorter than d stays inside itself),
//     so every source row of the tile lies in the panel;
//   * there are two panels: the rows of tile j + 1 are loaded and written to the other panel between the MFMAs of tile j, a whole tile of
//     lead, and one barrier per tile.
// Four waves, one per SIMD, each 128 rows x 32 columns: 192 weight + 64 accumulator registers + fragments + loads in flight need the
// unified 512-register file of a single wave per SIMD.
//
// Same bits as k_conv_gemm<*, 0>: for every output element the same v_mfma_f32_32x32x2_f32 sequence from a zero accumulator -- tap 0, 1, 2;
// inside a tap the 32-channel chunks in order; inside a chunk MFMA (qq, e) contracts channels 4 qq + e and 16 + 4 qq + e -- and the same
// epilogue (conv_store_rows).  No communication between workgroups; the only synchronisation is __syncthreads.
#include "conv_dev.h"
#include <type_traits>
#include <utility>

#define R2_BM 128
#define R2_C 128                            // Cin = Cout
#define R2_DMAX 4
#define R2_PROWS (R2_BM + 2 * R2_DMAX)      // panel rows
#define R2_PLD 132                          // floats per panel row
#define R2_PBYTES (R2_PROWS * R2_PLD * 4)   // 71 808
#define R2_PASSES (R2_PROWS / 8)            // a pass: 256 threads x 16 bytes = 8 panel rows
#define R2_LEAD 4                           // passes in flight between a pass's loads and its LDS write
#define R2_GROUPS 48                        // 3 taps x 4 chunks x 4 K-groups of 16 MFMAs

// f(integral_constant<0>) ... f(integral_constant<N - 1>): a loop whose index is a constant expression in the body (register arrays, sched_group_barrier counts)
template <class F, int... I>
__device__ __forceinline__ void r2_for_(F&& f, std::integer_sequence<int, I...>) { (f(std::integral_constant<int, I>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void r2_for(F&& f) { r2_for_(f, std::make_integer_sequence<int, N>{}); }

template <bool HAS_X2>
__global__ __launch_bounds__(256) void k_conv_res2ws(ConvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];       // two panels
    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int li = lane & 31, lh = lane >> 5;
    const int lc = tid & 31, lr = tid >> 5;         // panel loader: 16-byte chunk lc of panel rows lr + 8 p
    const int d = a.dil;
    const int G = gridDim.x;
    int tile = blockIdx.x;
    if (tile >= a.m_tiles) return;

    // ---- the wave's weights: column wid * 32 + li, channels kc * 32 + lh * 16 + qq * 4 .. + 3 of tap kk in w[(kk * 4 + kc) * 4 + qq]
    f32x4 w[R2_GROUPS];
    {
        const float* wp = a.W + (size_t)(wid * 32 + li) * a.w_ld + lh * 16;
#pragma unroll
        for (int g = 0; g < R2_GROUPS; ++g) w[g] = *(const f4u*)(wp + (size_t)(g >> 4) * a.Cout * a.w_ld + ((g >> 2) & 3) * 32 + (g & 3) * 4);
    }
    const int cc = wid * 32 + li;
    float cb, cs, ch;
    conv_col_params(a, cc, cb, cs, ch);
    const float slope = conv_act_slope(a.act1);
    const unsigned ybytes = (unsigned)a.y_ld * 4u;
    const unsigned xldb = (unsigned)a.x_ld * 4u, x2ldb = (unsigned)a.x2_ld * 4u;
    const int in_rows = a.M;

    // ---- panel loads of one tile.  The descriptors start at the first panel row that exists and end behind the last one: a lane whose
    // panel row lies outside [0, in_rows) or behind the halo asks for bytes outside the descriptor, gets zeros and touches no memory
    __amdgpu_buffer_rsrc_t rA = conv_rsrc(a.X, 0), rX = conv_rsrc(a.X, 0);
    unsigned voA = 0, voX = 0;
    auto set_loads = [&](int t, bool on) {
        const int m0 = __builtin_amdgcn_readfirstlane(t * R2_BM);
        const int p0 = m0 - d > 0 ? m0 - d : 0;
        const int hi = m0 + R2_BM + d < in_rows ? m0 + R2_BM + d : in_rows;
        const int rel = m0 - d - p0 + lr;                                // row of the descriptor that panel row lr is (negative: before row 0)
        const int n = on ? hi - p0 : 0;
        rA = conv_rsrc(a.X + (size_t)p0 * a.x_ld, n > 0 ? ((size_t)(n - 1) * a.x_ld + R2_C) * 4 : 0);
        voA = (unsigned)rel * xldb + (unsigned)lc * 16u;
        if (HAS_X2) {
            rX = conv_rsrc(a.X2 + (size_t)p0 * a.x2_ld, n > 0 ? ((size_t)(n - 1) * a.x2_ld + R2_C) * 4 : 0);
            voX = (unsigned)rel * x2ldb + (unsigned)lc * 16u;
        }
    };
    f4u ra[R2_LEAD + 1], rx[HAS_X2 ? R2_LEAD + 1 : 1];
    auto gload = [&](auto P) {
        constexpr int p = decltype(P)::value;
        ra[p % (R2_LEAD + 1)] = __builtin_bit_cast(f4u, __builtin_amdgcn_raw_buffer_load_b128(rA, voA + (unsigned)(8 * p) * xldb, 0, 0));
        if constexpr (HAS_X2) rx[p % (R2_LEAD + 1)] = __builtin_bit_cast(f4u, __builtin_amdgcn_raw_buffer_load_b128(rX, voX + (unsigned)(8 * p) * x2ldb, 0, 0));
    };
    auto lstore = [&](auto P, float* panel) {
        constexpr int p = decltype(P)::value, s = p % (R2_LEAD + 1);
        if constexpr (HAS_X2) ra[s] += rx[s];
        *(float4*)&panel[(lr + 8 * p) * R2_PLD + lc * 4] = make_float4(ra[s][0], ra[s][1], ra[s][2], ra[s][3]);
    };

    // ---- row table entries of the lane's four rows (row rb * 32 + li of the tile), fetched a tile ahead
    int2 tabn[4];
    auto prefetch_tab = [&](int t) {
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) { int g = t * R2_BM + rb * 32 + li; if (g > a.M - 1) g = a.M - 1; tabn[rb] = a.rowtab[g]; }
    };

    f32x16 acc[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[rb][r] = 0.0f;

    // ---- prologue: the first tile's panel
    prefetch_tab(tile);
    set_loads(tile, true);
    r2_for<R2_PASSES>([&](auto P) {
        gload(P);
        lstore(P, lds);
    });
    __syncthreads();

    int buf = 0;
    while (true) {
        const int m0 = __builtin_amdgcn_readfirstlane(tile * R2_BM);
        float* const pcur = lds + buf * (R2_PROWS * R2_PLD);
        float* const pnext = lds + (buf ^ 1) * (R2_PROWS * R2_PLD);
        // fragment addresses: the panel row of tap kk of the lane's row rb * 32 + li (clamped into the panel: a row table whose input
        // space is not the output space, which the launcher cannot see, must not send a read outside it)
        const float* fp[4][3];
#pragma unroll
        for (int rb = 0; rb < 4; ++rb) {
            const int tt = ROWTAB_T(tabn[rb].y), nd = ROWTAB_LAST(tabn[rb].y);
#pragma unroll
            for (int kk = 0; kk < 3; ++kk) {
                int pr = tabn[rb].x + conv_src_frame(tt, kk, 3, 1, d, a.Tin, nd) - (m0 - d);
                pr = pr < 0 ? 0 : (pr > R2_PROWS - 1 ? R2_PROWS - 1 : pr);
                fp[rb][kk] = pcur + pr * R2_PLD + lh * 16;
            }
        }
        const int tnext = tile + G;
        const bool more = tnext < a.m_tiles;
        prefetch_tab(more ? tnext : tile);
        set_loads(more ? tnext : tile, more);

        // ---- 48 K-groups of 16 MFMAs.  The fragments of group g + 1 are read while group g runs; group g < 17 also issues the loads of
        // pass g of the next tile's panel, and group g + R2_LEAD writes them
        float4 fa[2][4];
        auto lfrag = [&](auto Gi, int fb) {
            constexpr int g = decltype(Gi)::value, kk = g >> 4, ko = ((g >> 2) & 3) * 32 + (g & 3) * 4;
#pragma unroll
            for (int rb = 0; rb < 4; ++rb) fa[fb][rb] = *(const float4*)(fp[rb][kk] + ko);
        };
        lfrag(std::integral_constant<int, 0>{}, 0);
        r2_for<R2_GROUPS>([&](auto Gi) {
            constexpr int g = decltype(Gi)::value, fb = g & 1;
            if constexpr (g + 1 < R2_GROUPS) lfrag(std::integral_constant<int, g + 1>{}, fb ^ 1);
            if constexpr (g < R2_PASSES) gload(Gi);
            if constexpr (g >= R2_LEAD && g < R2_PASSES + R2_LEAD) lstore(std::integral_constant<int, g - R2_LEAD>{}, pnext);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    const float av = e == 0 ? fa[fb][rb].x : e == 1 ? fa[fb][rb].y : e == 2 ? fa[fb][rb].z : fa[fb][rb].w;
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, w[g][e], acc[rb], 0, 0, 0);
                }
            // one memory instruction behind each of the first MFMAs (CONV_MFMA_PAIR): fragment reads, then the loads, then the LDS write
            if constexpr (g + 1 < R2_GROUPS) CONV_MFMA_PAIR(0x100, 4);
            if constexpr (g < R2_PASSES) CONV_MFMA_PAIR(0x020, HAS_X2 ? 2 : 1);
            if constexpr (g >= R2_LEAD && g < R2_PASSES + R2_LEAD) CONV_MFMA_PAIR(0x200, 1);
            __builtin_amdgcn_sched_barrier(0);
        });

        // ---- epilogue: conv_gemm.hip's fast path (rows stored as they lie); leaves the accumulators zeroed
        const __amdgpu_buffer_rsrc_t rY = conv_out_rsrc(a.Y + (size_t)m0 * a.y_ld, a.M - m0, R2_BM, (size_t)a.y_ld * 4);
#pragma unroll
        for (int rb = 0; rb < 4; ++rb)
            conv_store_rows<false>(acc[rb], rY, (unsigned)(rb * 32 + 4 * lh) * ybytes + (unsigned)cc * 4u, ybytes, false, 1.0f, cb, slope, cs, ch);
        if (!more) break;
        __syncthreads();            // the next panel is complete; this tile's panel may be overwritten from here on
        tile = tnext;
        buf ^= 1;
    }
}

// The rule of the Res2Net shape (see the head of the file).  M >= 2 048 is the wide tile's own lower bound.
static bool res2ws_takes(const sd_ctx* c, const ConvArgs& a)
{
    return c->conv_res2_ws && a.prec == 0 && a.Cout == R2_C && a.Cin == R2_C && a.KT == 3 && (a.kt_real == 0 || a.kt_real == 3) && a.pad_mode == 0 && a.dil >= 1 && a.dil <= R2_DMAX &&
           a.rowtab && (a.in_rows == 0 || a.in_rows == a.M) && !a.item_bias && !a.R && a.act2 == 0 && a.M >= 2048 &&
           ((a.x_ld | a.y_ld | a.w_ld) & 3) == 0 && (!a.X2 || (a.x2_ld & 3) == 0);
}

// returns 1 when the case is not this kernel's (the caller then takes the 128 x 128 form); launches only, the caller bills it
int launch_conv_res2ws(sd_ctx* c, const ConvArgs& in)
{
    if (!res2ws_takes(c, in)) return 1;
    const size_t lds_bytes = (size_t)2 * R2_PBYTES;
    if (!conv_set_dyn_lds(c, g_attr_res2, {(const void*)k_conv_res2ws<true>, (const void*)k_conv_res2ws<false>}, lds_bytes)) return 1;
    ConvArgs a = in;
    a.m_tiles = (a.M + R2_BM - 1) / R2_BM;
    a.n_tiles = 1;
    int grid = c->conv_res2_wgs > 0 ? c->conv_res2_wgs : c->num_cu;       // one persistent workgroup per CU
    if (grid > a.m_tiles) grid = a.m_tiles;
    c->last_conv_kernel = a.X2 ? "res2ws_f32_x2" : "res2ws_f32";
    if (a.X2) hipLaunchKernelGGL(k_conv_res2ws<true>, dim3(grid), dim3(256), lds_bytes, c->stream, a);
    else hipLaunchKernelGGL(k_conv_res2ws<false>, dim3(grid), dim3(256), lds_bytes, c->stream, a);
    if (hipGetLastError() != hipSuccess) SD_FAIL(c, SD_ERR_HIP, "k_conv_res2ws launch failed");
    return SD_OK;
}
