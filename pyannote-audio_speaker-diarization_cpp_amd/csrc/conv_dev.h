// conv_dev.h -- device code shared by the four implicit-GEMM conv kernels (conv_gemm.hip, conv_gemm_h.hip, conv_gemm_g.hip,
// conv_gemm_p.hip): the persistent super-block schedule, the row map of a tap, the row-table cursor of the load stream, the lane-quad
// transpose, buffer resources and LDS-DMA, and the small epilogue pieces.  These rules have to be the same in every kernel -- the
// kernels are compared with each other bit for bit (tests/test_gpu_parity.py) -- so each of them is written once, here.
//
// Everything is __forceinline__ and takes scalars (or one vector) by reference: these kernels sit at 248 - 256 VGPRs, and a helper that
// takes a small ARRAY by reference made hipcc keep the array in memory form (k_conv_gemm_w256<1>: 3 379 -> 4 158 instructions).
#pragma once
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));   // 4-byte aligned float4 (x_ld may be 10)
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;

// n times "one MFMA, then one memory instruction of class `mask`" (sched_group_barrier masks: 0x008 MFMA, 0x020 VMEM read, 0x100 DS read,
// 0x200 DS write).  Left alone the scheduler bunches a region's memory instructions; a bunch of 4 - 8 back-to-back VMEM / DS issues takes
// longer than one MFMA keeps the pipe busy and leaves a bubble.
#define CONV_MFMA_PAIR(mask, n) do { _Pragma("unroll") for (int i_ = 0; i_ < (n); ++i_) { __builtin_amdgcn_sched_group_barrier(0x008, 1, 0); __builtin_amdgcn_sched_group_barrier(mask, 1, 0); } } while (0)

// ---------------------------------------------------------------- persistent super-block schedule
// The grid is a fixed number of workgroups per CU (a multiple of 8).  The wpx workgroups whose id is equal mod 8 -- one XCD under round-robin
// dispatch; a speed assumption only, the results do not depend on it -- own the row panels m = xcd + 8 j and walk them in PM x PN super-blocks
// of tiles: workgroup wl works on position (pm, pn) = (wl / PN, wl % PN) of every block.  They advance through K roughly in step, so each A
// and W K-slice is pulled into the XCD's L2 once per block and shared by PN resp. PM workgroups (measured before this order: 125 GB of fabric
// reads for the 3072 x 3072 layer against 4.9 GB algorithmic).  Why PM x PN and not one long row of tiles: with 32 workgroups per XCD,
// 4 column tiles x 8 row panels beats 8 x 4 by a third on that layer (each W K-slice is shared by 8 workgroups instead of 4; f32 137 vs 103 TF,
// fp16 962 vs 778 TF, profiles/r02_layer_profile.txt).  pnmax is the kernel's widest block (launcher option; 4 for the 256 x 256 tiles).
// [How it is written matters to hipcc: the methods take the kernel's ConvArgs instead of keeping a reference or a copy of n_tiles, and init() has no
// early return -- with either, k_conv_gemm_pp spills 1 to 8 more SGPRs.]
struct ConvSched {
    int xcd, wl, wpx, mx, PN, PM, pm, pn, n_groups, sb_end;
    // false: this workgroup has no tile at all (the kernel returns at once); else q0 = the first super-block in which it has one
    __device__ __forceinline__ bool init(const ConvArgs& a, int pnmax, int& q0)
    {
        const int w = blockIdx.x, G = gridDim.x;                 // G is a multiple of 8
        xcd = w & 7; wl = w >> 3; wpx = G >> 3;
        mx = (a.m_tiles - xcd + 7) >> 3;                         // row panels of this XCD
        PN = a.n_tiles < pnmax ? a.n_tiles : pnmax;
        PM = wpx / PN > 0 ? wpx / PN : 1;
        pm = wl / PN; pn = wl - pm * PN;
        n_groups = (a.n_tiles + PN - 1) / PN;
        sb_end = pm < PM ? n_groups * ((mx + PM - 1) / PM) : 0;      // wl beyond the PM x PN positions: no tiles
        q0 = next(a, -1);
        return q0 < sb_end;
    }
    // the tile of this workgroup in super-block sb: row panel index j (of this XCD), column tile nt; false when the block has none for it
    __device__ __forceinline__ bool valid(const ConvArgs& a, int sb, int& j, int& nt) const
    {
        const int mg = sb / n_groups, ng = sb - mg * n_groups;
        j = mg * PM + pm; nt = ng * PN + pn;
        return j < mx && nt < a.n_tiles;
    }
    // next super-block in which this workgroup has a tile, or sb_end
    __device__ __forceinline__ int next(const ConvArgs& a, int sb) const
    {
        int j, nt;
        for (++sb; sb < sb_end; ++sb) if (valid(a, sb, j, nt)) return sb;
        return sb_end;
    }
    // first row / column of that tile; wave-uniform (readfirstlane keeps what is derived from them, the descriptors above all, in SGPRs)
    __device__ __forceinline__ void origin(const ConvArgs& a, int sb, int tile_m, int tile_n, int& m0, int& n0) const
    {
        int j, nt;
        (void)valid(a, sb, j, nt);
        m0 = __builtin_amdgcn_readfirstlane((xcd + 8 * j) * tile_m);
        n0 = __builtin_amdgcn_readfirstlane(nt * tile_n);
    }
};

// ---------------------------------------------------------------- row map
// "same" padding: the input frame that tap kk of output frame t reads.  Taps kk >= ktr are the second weight plane of the split-weight
// mode and shift like tap kk - ktr.  Frames outside [0, Tin) are reflected; `last` is the last frame the compact row space STORES of that
// item (dead-row skipping, ROWTAB_LAST): a tap beyond it reads that frame.
__device__ __forceinline__ int conv_src_frame(int t, int kk, int ktr, int half, int dil, int Tin, int last)
{
    int qr = t + ((kk >= ktr ? kk - ktr : kk) - half) * dil;
    if (qr < 0) qr = -qr;
    if (qr >= Tin) qr = 2 * (Tin - 1) - qr;
    if (qr < 0) qr = 0;
    if (qr > last) qr = last;
    return qr;
}

// Row-table entries of the NP rows a lane stages (register / LDS-staged kernels): `pre` holds the entries of the tile the load stream
// visits NEXT -- fetched one tile ahead, so a tile switch never waits for them -- and enter() decodes them when the stream gets there.
template <int NP>
struct ConvRowTab {
    int2 pre[NP]; int pre_base = 0;
    int rrel[NP], tt[NP], nd[NP];       // per part: item offset (rows) relative to the tile's first item, frame, last stored frame
    // row(p) = the row of the tile that part p of this lane stages; m0 = the tile's first row (wave-uniform)
    template <class Row>
    __device__ __forceinline__ void prefetch(const ConvArgs& a, int m0, Row row)
    {
        pre_base = a.rowtab[m0 < a.M ? m0 : a.M - 1].x;
#pragma unroll
        for (int p = 0; p < NP; ++p) { int g = m0 + row(p); if (g > a.M - 1) g = a.M - 1; pre[p] = a.rowtab[g]; }
    }
    // returns the first input row of the tile's first item: the activation descriptor starts there
    __device__ __forceinline__ int enter()
    {
        const int base = __builtin_amdgcn_readfirstlane(pre_base);
#pragma unroll
        for (int p = 0; p < NP; ++p) { rrel[p] = pre[p].x - base; tt[p] = ROWTAB_T(pre[p].y); nd[p] = ROWTAB_LAST(pre[p].y); }
        return base;
    }
};

// Position of a load stream that runs ahead of the compute stream and straight across tile boundaries: super-block q, tap kk, K-step kc of
// the tap, and sK = the K position in bytes (128 per step, the buffer loads' scalar offset).  K always runs 0 .. Cin - 1 in the same order
// for every tile: a row's result does not depend on where its tile sits in the schedule.
struct ConvLoadPos {
    int q, kk = 0, kc = 0;
    unsigned sK = 0;
    // on_tile(sb): the stream enters the tile of super-block sb; on_tap(kk): per-lane offsets of tap kk.  Past the last tile the stream
    // stays on it (dummy loads, never multiplied).
    template <class OnTile, class OnTap>
    __device__ __forceinline__ void advance(const ConvArgs& a, const ConvSched& s, int kcs, OnTile on_tile, OnTap on_tap)
    {
        if (++kc < kcs) { sK += 128; return; }
        kc = 0; sK = 0;
        if (++kk == a.KT) {
            kk = 0;
            const int nq = s.next(a, q);
            if (nq < s.sb_end) { q = nq; on_tile(q); }
        }
        on_tap(kk);
    }
};

// ---------------------------------------------------------------- buffer resources, LDS-DMA
// {base, stride 0, bytes (clamped to 4 GB - 1), raw 32-bit data format}: reads beyond `bytes` return 0, stores there are dropped
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_rsrc(const void* base, size_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes > 0xffffffffull ? 0xffffffffu : (unsigned)bytes, 0x00020000);
}
// output tile of `tile_rows` rows of row_bytes bytes that starts at `tile` with rows_left rows to the end of the batch: the descriptor
// ends at the batch's last row, so rows >= M are dropped by the range check
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_out_rsrc(const void* tile, int rows_left, int tile_rows, size_t row_bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)tile, 0, (unsigned)((size_t)(rows_left < tile_rows ? rows_left : tile_rows) * row_bytes), 0x00020000);      // (at most 256 rows: far below 4 GB)
}
// the same four words for inline assembly, forced wave-uniform (an "s" operand has to be in SGPRs)
__device__ __forceinline__ v4i conv_rsrc_sgpr(const void* base, size_t bytes)
{
    const unsigned long long b = (unsigned long long)base;
    v4i r;
    r[0] = __builtin_amdgcn_readfirstlane((int)(unsigned)b);
    r[1] = __builtin_amdgcn_readfirstlane((int)(unsigned)((b >> 32) & 0xffffu));
    r[2] = __builtin_amdgcn_readfirstlane((int)(bytes > 0xffffffffull ? 0xffffffffu : (unsigned)bytes));
    r[3] = 0x00020000;
    return r;
}
// One LDS-DMA wave instruction: 64 x 16 (b32: 64 x 4) bytes from the buffer `rs` (per-lane byte offset `vo`, scalar byte offset `so`) to the
// 1 KB (256 bytes) of LDS at `ldsaddr`.  Inline assembly on purpose: hipcc's waitcnt pass treats an LDS-DMA it knows about as a pending LDS
// store that ANY later ds_read may alias and puts `s_waitcnt vmcnt(0)` in front of the next fragment read -- which would serialise exactly the
// overlap the LDS-DMA kernels exist for.  The waits that order the DMAs against the fragment reads are the explicit ones at their barriers.
// `s_nop 4`: the descriptor words often come straight from v_readfirstlane, and an SGPR written by the vector ALU needs five wait states before
// a vector-memory instruction reads it; hipcc counts them for its own instructions, not inside an asm string.  m0 (the LDS address) is
// reserved: the compiler does not keep values in it across statements.
__device__ __forceinline__ void lds_dma_b32(v4i rs, unsigned ldsaddr, unsigned vo)
{
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dword %1, %2, 0 offen lds" :: "s"(ldsaddr), "v"(vo), "s"(rs) : "memory");
}
__device__ __forceinline__ void lds_dma_b128(v4i rs, unsigned ldsaddr, unsigned vo)
{
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds" :: "s"(ldsaddr), "v"(vo), "s"(rs) : "memory");
}
__device__ __forceinline__ void lds_dma_b128(v4i rs, unsigned ldsaddr, unsigned vo, unsigned so)
{
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" :: "s"(ldsaddr), "v"(vo), "s"(rs), "s"(so) : "memory");
}

// ---------------------------------------------------------------- epilogue pieces
// first activation as a slope in [0, 1], applied as max(v, v * slope): ReLU (0), leaky ReLU (0.01), identity (1).  (Not max(v, 0): a NaN
// has to stay a NaN; v * 0 keeps it.)
__device__ __forceinline__ float conv_act_slope(int act1) { return (act1 == 1) ? 0.0f : ((act1 == 2) ? 0.01f : 1.0f); }

// bias, folded-BatchNorm scale and shift of output channel cc (absent arrays: 0, 1, 0)
__device__ __forceinline__ void conv_col_params(const ConvArgs& a, int cc, float& cb, float& cs, float& ch)
{
    cb = a.bias ? a.bias[cc] : 0.0f;
    cs = a.scale ? a.scale[cc] : 1.0f; ch = a.scale ? a.shift[cc] : 0.0f;
}

// 4 x 4 transpose across the lane quad (two butterfly stages on DPP quad_perm): in, lane lq of a quad holds x0..x3 = four consecutive
// rows of its column; out, four consecutive columns (the quad's) of row lq.
__device__ __forceinline__ void quad_transpose4(float& x0, float& x1, float& x2, float& x3, int lq)
{
    float s0 = (lq & 1) ? x0 : x1;
    float s1 = (lq & 1) ? x2 : x3;
    float r0 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s0), 0xB1, 0xF, 0xF, true));
    float r1 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s1), 0xB1, 0xF, 0xF, true));
    if (lq & 1) { x0 = r0; x2 = r1; } else { x1 = r0; x3 = r1; }
    s0 = (lq & 2) ? x0 : x2;
    s1 = (lq & 2) ? x1 : x3;
    r0 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s0), 0x4E, 0xF, 0xF, true));
    r1 = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(s1), 0x4E, 0xF, 0xF, true));
    if (lq & 2) { x0 = r0; x1 = r1; } else { x2 = r0; x3 = r1; }
}

// f32 epilogue "rows stored as they lie" (C layout of the 32 x 32 MFMA: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)): every
// accumulator register is one output row for 32 consecutive columns across a half-wave and goes out as it is, 128 (fp16: 64) contiguous bytes
// per row and instruction, the row term in the scalar offset: no lane transposes, no per-row index arithmetic.  `vo` = the lane's byte offset
// of row 4 (lane >> 5) of the 32 x 32 block in the descriptor rY, ybytes = bytes per output row.  X: v = acc * as + cb (x3: the weights were
// scaled by a power of two); h16: rounded to fp16 at the store.  The registers are left zeroed for the next tile.
template <bool X>
__device__ __forceinline__ void conv_store_rows(f32x16& acc, __amdgpu_buffer_rsrc_t rY, unsigned vo, unsigned ybytes, bool h16, float as, float cb, float slope, float cs, float ch)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float v = X ? acc[r] * as + cb : acc[r] + cb;
        acc[r] = 0.0f;
        v = fmaxf(v, v * slope);
        v = v * cs + ch;
        const unsigned so = (unsigned)((r & 3) + 8 * (r >> 2)) * ybytes;
        if (h16) __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (_Float16)v), rY, vo, so, 0);
        else __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), rY, vo, so, 0);
    }
}
