// conv_gemm_g.hip -- the fp16 mode's wide layers (Cout >= 256) with LDS-DMA staging (round 4).
//
// conv_gemm_h.hip's fp16 form stages its operands through registers (buffer_load -> VGPRs -> ds_write, one K-step ahead).  Here
// `buffer_load_dwordx4 ... lds` writes them straight into LDS: no staging registers, no ds_write instructions, no VALU, and the
// request for step s + 2 goes out the moment its stage is released (right behind the barrier inside step s) with a whole K-step to land.
// What that bought, measured (profiles/r04_g256_ablation.txt): nothing on the big layers (MFA 991 -> 1 000 TF), 5 - 10 % on block0 -- the
// loop is not bound by the issue -> land latency, as round 3 believed, but by the CU's vector-memory INGEST rate: 64 KB per K-step
// arrive at 16 - 17 bytes per clock and CU whichever way they are requested (the same loop without MFMAs takes the same 3 900 cycles
// per step; without the DMAs 2 257 = the matrix pipe 91 % busy).  With a 256 x 256 tile the fp16 pipe needs 32 B / clk / CU: the kernel
// runs at ~ 85 % of what its memory path allows.  It stays the default fp16 form (fewer registers and instructions, same bits).
//
// Geometry as before: 256 x 256 tile, K-step of 64 halves (128 bytes of every row), 8 waves of 64 x 128 (2 x 4 tiles of
// v_mfma_f32_32x32x16_f16, 128 accumulator registers), persistent super-blocks per XCD, the load stream runs across tile boundaries.
// LDS: 2 stages x (256 + 256) rows x 128 B = 128 KB (+ 32 KB of epilogue strips = the CU's 160 KB).  An LDS-DMA wave instruction
// writes 64 x 16 consecutive bytes = eight whole rows, so rows cannot be padded; bank conflicts of the fragment reads are removed by a
// swizzle instead: the 16-byte chunk c of row R lives at chunk position c ^ ((R >> 1) & 7).  Every 16-lane group of a ds_read_b128
// ({0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... MI355X_MICROARCH.md, LDS) then reads sixteen different (128-byte half, chunk) slots
// of the 256-byte bank row: conflict-free.  The swizzle is applied on the SOURCE side (the DMA's per-lane global address picks the
// logical chunk its LDS slot holds) and in the fragment address.
//
// Ordering (MI355X_MICROARCH.md item 7, cdna_hip_programming.md "Read a staged buffer one phase AFTER the wait that retires it"):
// a wave waits for its own DMAs (vmcnt) and for its outstanding fragment reads of the buffer about to be re-filled (lgkmcnt(0)),
// then joins a raw s_barrier; the next buffer is read, and the released one re-filled, only behind that barrier.
// Same arithmetic as the register-staged form: every output element sums the same products in the same order, so the two kernels
// give the same bits (tests/test_gpu_parity.py::test_ecapa_fp16_lds_dma_staged_kernel_gives_the_same_bits).
// Schedule, row map, row-table cursor, the LDS-DMA wrappers (and why they are inline assembly) and the epilogue pieces: conv_dev.h.
#include "conv_dev.h"

#define GM 256
#define GN 256
#define G_STAGE 65536          // bytes per stage: 256 A rows + 256 B rows of 128 B
#define G_BOFF 32768
#define G_STRIP 4096           // epilogue strip per wave: 16 rows x 128 channels of fp16 (128 + 32 KB = all of the CU's LDS)

// P = 1: fp16 tensors (v_mfma_f32_32x32x16_f16, a K-step is 64 halves).  P = 0: f32 tensors (v_mfma_f32_32x32x2_f32 over the k pairs (k, k + 16)
// of a 32-float K-step, conv_gemm.hip's order: same bits as the 128 x 128 kernel and as conv_gemm_h.hip's register-staged form).  Either way a
// K-step is 128 bytes of every row, so stages, swizzle, DMA pieces and the load stream are the same.
template <int P>
__global__ __launch_bounds__(512) void k_conv_gemm_g256(ConvArgs a)
{
    constexpr int ES = P == 0 ? 4 : 2;               // bytes per element of X, W, Y
    extern __shared__ __attribute__((aligned(1024))) char lds[];

    ConvSched sch;
    int q0;
    if (!sch.init(a, a.sched > 0 ? a.sched : 4, q0)) return;
    const int pm = sch.pm, pn = sch.pn;

    const int tid = threadIdx.x;
    const int lane = tid & 63, wid = tid >> 6;
    const int wr = wid >> 1, wc = wid & 1;           // wave tile: rows wr * 64, columns wc * 128
    const int li = lane & 31, lh = lane >> 5;

    const int kcs = a.Cin / (128 / ES);
    const int S = a.KT * kcs;
    const int ktr = a.kt_real > 0 ? a.kt_real : a.KT;      // taps that shift rows (split-weight mode: KT = 2 * ktr planes)
    const int half = ktr / 2;
    const size_t in_rows = (size_t)(a.in_rows > 0 ? a.in_rows : a.M);

    // loader: wave `wid` fills rows [32 wid, 32 wid + 32) of both operands, eight rows per DMA instruction; lane l writes LDS bytes
    // [16 l, 16 l + 16) of the instruction's 1 KB: row Rp = 32 wid + 8 p + (l >> 3), chunk POSITION l & 7, which holds the logical
    // chunk (l & 7) ^ ((Rp >> 1) & 7)
    const int lrow = lane >> 3, pc = lane & 7;
    auto l_row = [&](int p) { return wid * 32 + p * 8 + lrow; };
    auto l_chunk = [&](int p) { return pc ^ ((((p & 1) << 2) + (lane >> 4)) & 7); };          // ((Rp >> 1) & 7) = 4 (p & 1) + (lane >> 4)
    // Activation rows (option conv_rot, same LDS image): piece p of wave `wid` covers rows 64 ((rot + p) & 3) + 8 wid + (l >> 3), so the
    // eight waves' p-th pieces together are one 64-row quarter of the tile, and the PN workgroups that share a row panel (same XCD, same
    // K-step) start with DIFFERENT quarters: each line of the panel is first requested by one of them and is on its way (or in the L2)
    // when the others ask -- a CU keeps ~16 KB of requests in flight, so what a K-step costs is the latency its lines see.  Measured on the
    // planted hour (profiles/r04_g256_request_order.txt): tdnn 749 -> 812 TF on one box, 883 -> 922 on another; MFA + 1 %.  [Requesting the own
    // quarter of step s + 3 one step early on top of it (into the idle strip area, only to warm the L2): no further gain.]
    const int rot = (a.stagger & 1) ? pn : 0;
    // bit 1: a wave's pieces 0, 1 (and 2, 3) lie 32 rows apart in ONE quarter, waves 0-3 and 4-7 take different quarters.  With the DMAs alone in the
    // loop (no MFMA, no fragment reads) a K-step of the tdnn layers takes 3 390 cycles in this order against 4 180 (MFA 2 910 / 3 400); the whole
    // kernel gains 2 - 5 % on tdnn (profiles/r04_g256_request_order.txt, section 6)
    const bool pairmap = (a.stagger & 2) != 0;
    auto qidx = [&](int p) { return pairmap ? (wid >> 2) + 2 * (p >> 1) : p; };
    auto rinq = [&](int p) { return pairmap ? 8 * (wid & 3) + 32 * (p & 1) : 8 * wid; };
    auto a_quarter = [&](int p) { return (rot + qidx(p)) & 3; };
    auto l_rowA = [&](int p) { return (a.stagger & 1) ? a_quarter(p) * 64 + rinq(p) + lrow : l_row(p); };
    auto l_chunkA = [&](int p) { return (a.stagger & 1) ? pc ^ ((((wid & 1) << 2) + (lane >> 4)) & 7) : l_chunk(p); };
    // the same for the weight rows among the PM workgroups that share a column panel (MFA's 6 MB column panel does not stay in a 4 MB L2: + 1.5 - 2 % there)
    const bool rotB = (a.stagger & 1) != 0;
    auto b_quarter = [&](int p) { return (pm + qidx(p)) & 3; };
    auto l_rowB = [&](int p) { return rotB ? b_quarter(p) * 64 + rinq(p) + lrow : l_row(p); };
    auto l_chunkB = [&](int p) { return rotB ? pc ^ ((((wid & 1) << 2) + (lane >> 4)) & 7) : l_chunk(p); };
    auto b_lds = [&](int p) { return rotB ? (unsigned)(b_quarter(p) * 8192 + rinq(p) * 128) : (unsigned)(wid * 4096 + p * 1024); };
    auto a_lds = [&](int p) { return (a.stagger & 1) ? (unsigned)(a_quarter(p) * 8192 + rinq(p) * 128) : (unsigned)(wid * 4096 + p * 1024); };
    unsigned a_off[4], b_off[4];          // wave-uniform LDS offsets of the pieces inside a stage (SGPRs)
#pragma unroll
    for (int p = 0; p < 4; ++p) { a_off[p] = __builtin_amdgcn_readfirstlane(a_lds(p)); b_off[p] = __builtin_amdgcn_readfirstlane((unsigned)G_BOFF + b_lds(p)); }
    ConvRowTab<4> tab;
    unsigned voA[4], voB[4];
    auto prefetch_tab = [&](int sb) { int m0, n0; sch.origin(a, sb, GM, GN, m0, n0); tab.prefetch(a, m0, l_rowA); };
    v4i rA = conv_rsrc_sgpr(a.X, 0);
    const v4i rB = conv_rsrc_sgpr(P == 0 ? (const void*)a.W : a.W16, (size_t)a.KT * a.Cout * a.w_ld * ES);
#pragma unroll
    for (int p = 0; p < 4; ++p) voB[p] = (unsigned)(l_rowB(p) * a.w_ld * ES + l_chunkB(p) * 16);
    ConvLoadPos lp; lp.q = q0;
    int m0l = 0, n0l = 0;
    unsigned sB = 0;
    auto set_tile = [&](int sb) {              // the stream enters a tile (its table entries were fetched a tile ago); asks for the next tile's
        sch.origin(a, sb, GM, GN, m0l, n0l);
        const int base = tab.enter();
        rA = conv_rsrc_sgpr((const char*)a.X + (size_t)base * a.x_ld * ES, (in_rows - base) * a.x_ld * ES);
        const int nq2 = sch.next(a, sb);
        if (nq2 < sch.sb_end) prefetch_tab(nq2);
    };
    auto set_tap = [&](int kk) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int qr = conv_src_frame(tab.tt[p], kk, ktr, half, a.dil, a.Tin, tab.nd[p]);
            voA[p] = (unsigned)(tab.rrel[p] + qr) * (unsigned)a.x_ld * ES + (unsigned)l_chunkA(p) * 16;
        }
        sB = (unsigned)(((size_t)kk * a.Cout + n0l) * a.w_ld * ES);
    };
    auto advance = [&]() { lp.advance(a, sch, kcs, set_tile, set_tap); };
    // eight LDS-DMA instructions per wave and K-step: four 1 KB pieces of A, four of B
    const unsigned lds0 = (unsigned)(size_t)(lds_char*)lds;
    auto dma_piece = [&](int st, int p) {            // piece p of 8: A pieces 0..3, W pieces 4..7
        const unsigned stb = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(st * G_STAGE));
        if (p < 4) lds_dma_b128(rA, stb + a_off[p], voA[p], lp.sK);
        else lds_dma_b128(rB, stb + b_off[p - 4], voB[p - 4], sB + lp.sK);
    };
    auto dma = [&](int st) {
        const unsigned stb = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(st * G_STAGE));
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            lds_dma_b128(rA, stb + a_off[p], voA[p], lp.sK);
            lds_dma_b128(rB, stb + b_off[p], voB[p], sB + lp.sK);
        }
    };

    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // fragments.  fp16: lane (li, lh) reads k = 16 kb + 8 lh .. + 7 (logical chunk 2 kb + lh) of row li of every 32-row block;
    // f32: k = 16 lh + 4 kb .. + 3 (logical chunk 4 lh + kb), the two k of each v_mfma_f32_32x32x2_f32 sixteen apart
    const int swz = (li >> 1) & 7;
    const char* const Afr = lds + (wr * 64 + li) * 128;
    const char* const Bfr = lds + G_BOFF + (wc * 128 + li) * 128;
    float4 ha[2][2], hb[2][4];
    // P = 2: v_mfma_f32_16x16x32_f16 (the chip holds 2.09 GHz on it against 1.79 on the 32x32x16 shape, tools/mfma_shape_clock.hip).  The wave's
    // 64 x 128 tile is 4 x 8 blocks of 16 x 16 (acc16, 128 registers); a K-step is two k-groups of 32 halves, each walked in two phases of
    // 4 x 4 blocks: phase kb = 2 g + h reads the weight fragments of blocks 4 h .. 4 h + 3 (and, for h = 0, the four activation fragments
    // of group g, kept for both phases).  Lane l reads k = 32 g + 8 (l >> 4) .. + 7 (logical chunk 4 g + (l >> 4)) of row l & 15 of a block;
    // with the stage's swizzle every 16-lane group of the ds_read_b128 covers the sixteen (128-byte half, chunk) slots once.
    f32x4 acc16[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) acc16[i][j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int l15 = lane & 15, l4 = lane >> 4;
    const char* const Afr16 = lds + (wr * 64 + l15) * 128;
    const char* const Bfr16 = lds + G_BOFF + (wc * 128 + l15) * 128;
    float4 qa[2][4], qb[2][4];
    auto hfrag = [&](int st, int kb, int fbuf) {
        if constexpr (P == 2) {
            const int g = kb >> 1, h = kb & 1;
            const int co = ((4 * g + l4) ^ ((l15 >> 1) & 7)) * 16 + st * G_STAGE;
            if (h == 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i) qa[g][i] = *(const float4*)(Afr16 + co + i * 16 * 128);
            }
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) qb[fbuf][jj] = *(const float4*)(Bfr16 + co + (4 * h + jj) * 16 * 128);
            return;
        }
        const int co = ((P == 0 ? 4 * lh + kb : 2 * kb + lh) ^ swz) * 16 + st * G_STAGE;
        ha[fbuf][0] = *(const float4*)(Afr + co);
        ha[fbuf][1] = *(const float4*)(Afr + co + 32 * 128);
#pragma unroll
        for (int j = 0; j < 4; ++j) hb[fbuf][j] = *(const float4*)(Bfr + co + j * 32 * 128);
    };
    auto hmma = [&](int fbuf, int kb) {
        if constexpr (P == 2) {
            const int g = kb >> 1, h = kb & 1;
#pragma unroll
            for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    acc16[i][4 * h + jj] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, qa[g][i]), __builtin_bit_cast(half8, qb[fbuf][jj]), acc16[i][4 * h + jj], 0, 0, 0);
            return;
        }
        if constexpr (P == 0) {
            // f32: the WEIGHT fragment is the MFMA's first operand, so the accumulator tile comes out transposed -- register r of acc[i][j],
            // lane (li, lh) = activation row 32 i + li, output channel 32 j + 8 (r >> 2) + 4 lh + (r & 3): four registers are four
            // consecutive channels of one row = one 16-byte store.  Same products in the same order: same bits as the other operand order.
            const float a0[4] = {ha[fbuf][0].x, ha[fbuf][0].y, ha[fbuf][0].z, ha[fbuf][0].w}, a1[4] = {ha[fbuf][1].x, ha[fbuf][1].y, ha[fbuf][1].z, ha[fbuf][1].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float bv = e == 0 ? hb[fbuf][j].x : e == 1 ? hb[fbuf][j].y : e == 2 ? hb[fbuf][j].z : hb[fbuf][j].w;
                    acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv, a0[e], acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv, a1[e], acc[1][j], 0, 0, 0);
                }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, ha[fbuf][0]), __builtin_bit_cast(half8, hb[fbuf][j]), acc[0][j], 0, 0, 0);
                acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, ha[fbuf][1]), __builtin_bit_cast(half8, hb[fbuf][j]), acc[1][j], 0, 0, 0);
            }
        }
    };
    // f32: the tile's 256 bias / BN scale / BN shift values go to LDS by LDS-DMA during the tile's LAST K-step (waves 0-3, 64 channels each, no
    // registers); that step's vmcnt(0) + barrier make them visible to the epilogue.  The area lies behind the stages (the fp16 form's strips).
    const v4i rPb = conv_rsrc_sgpr(a.bias, (size_t)a.Cout * 4), rPs = conv_rsrc_sgpr(a.scale, (size_t)a.Cout * 4), rPh = conv_rsrc_sgpr(a.shift, (size_t)a.Cout * 4);
    const float* const Ps = (const float*)(lds + 2 * G_STAGE);

    // prologue: steps 0 and 1 of the first tile are requested; step 0 has to be there
    prefetch_tab(q0);
    set_tile(q0);
    set_tap(0);
    int m0c = m0l, n0c = n0l;
    dma(0);
    advance();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    dma(1);
    advance();
    hfrag(0, 0, 0);

    int q = q0, s = 0, buf = 0;
    while (true) {
        // K-groups 0..2 of step s from stage `buf`; each group's fragments were read while the group before ran
        // MFMAs of a phase: the first carry the next phase's fragment reads (P = 2: four reads when the next phase keeps its activation fragments, eight otherwise)
        constexpr int NM = P == 0 ? 32 : P == 1 ? 8 : 16, NR_ODD = P == 2 ? 4 : 6, NR_EVEN = P == 2 ? 8 : 6;
        if constexpr (P == 0) {
            if (s == S - 1 && wid < 4) {
                const unsigned dst = __builtin_amdgcn_readfirstlane(lds0 + (unsigned)(2 * G_STAGE + wid * 256));
                const unsigned vo = (unsigned)(n0c + wid * 64 + lane) * 4u;
                if (a.bias) lds_dma_b32(rPb, dst, vo);
                if (a.scale) { lds_dma_b32(rPs, dst + 1024, vo); lds_dma_b32(rPh, dst + 2048, vo); }
            }
        }
        hfrag(buf, 1, 1);
        hmma(0, 0);
        CONV_MFMA_PAIR(0x100, NR_ODD); __builtin_amdgcn_sched_group_barrier(0x008, NM - NR_ODD, 0);
        __builtin_amdgcn_sched_barrier(0);
        hfrag(buf, 2, 0);
        hmma(1, 1);
        CONV_MFMA_PAIR(0x100, NR_EVEN); __builtin_amdgcn_sched_group_barrier(0x008, NM - NR_EVEN, 0);
        __builtin_amdgcn_sched_barrier(0);
        hfrag(buf, 3, 1);
        hmma(0, 2);
        CONV_MFMA_PAIR(0x100, NR_ODD); __builtin_amdgcn_sched_group_barrier(0x008, NM - NR_ODD, 0);
        __builtin_amdgcn_sched_barrier(0);
        // stage `buf` has been read out (this wave's last fragments of it are in registers once lgkmcnt reaches 0) and this wave's
        // share of step s + 1 has landed in the other stage (vmcnt(0)): behind the barrier that holds for every wave
        // (the counter retires in issue order.  Right behind an epilogue the wave's 16 output stores are YOUNGER than the eight DMAs
        // this barrier needs: vmcnt(16) lets them drain under the new tile's first K-step instead of in front of its first barrier)
        // (f32: 32 stores of 16 bytes per lane)
        if (s == 0 && q != q0 && P == 0) asm volatile("s_waitcnt vmcnt(32) lgkmcnt(0)" ::: "memory");
        else if (s == 0 && q != q0 && !a.y_f32) asm volatile("s_waitcnt vmcnt(16) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (P == 0) {
            // f32: a K-group is 32 MFMAs of 64 cycles; the eight DMA pieces go out one per four MFMAs instead of in a burst in front of them
            hfrag(buf ^ 1, 0, 0);
            const float a0[4] = {ha[1][0].x, ha[1][0].y, ha[1][0].z, ha[1][0].w}, a1[4] = {ha[1][1].x, ha[1][1].y, ha[1][1].z, ha[1][1].w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float bv = e == 0 ? hb[1][j].x : e == 1 ? hb[1][j].y : e == 2 ? hb[1][j].z : hb[1][j].w;
                    acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv, a0[e], acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(bv, a1[e], acc[1][j], 0, 0, 0);
                    if ((j & 1) == 1) { __builtin_amdgcn_sched_barrier(0); dma_piece(buf, e * 2 + (j >> 1)); __builtin_amdgcn_sched_barrier(0); }
                }
        } else {
            dma(buf);            // step s + 2 into the stage just released
            hfrag(buf ^ 1, 0, 0);
            hmma(1, 3);
        }
        __builtin_amdgcn_sched_barrier(0);
        advance();

        if (s == S - 1) {
            if constexpr (P == 0) {
            // ---- epilogue, f32.  Accumulator layout (weights first, see hmma): register r of acc[i][j], lane (li, lh) = row 32 i + li,
            // channel 32 j + 8 (r >> 2) + 4 lh + (r & 3): four registers = four consecutive channels of a row = one 16-byte store, 32
            // stores per wave.  [conv_gemm_h.hip stores every register as a row of 32 columns across a half-wave: 128 dword stores per
            // wave, more than the 6-bit vmcnt can skip, so the next tile's first LDS restaging waits for all of them; here the stores stay
            // outstanding under the next tile's first K-step (vmcnt(32) at its barrier).]  Parameters come from LDS (Ps, filled by DMA).
            // The descriptor starts at the tile's first row and ends at the batch's last one: rows >= M are dropped by the range check.
            const float slope = conv_act_slope(a.act1);
            const __amdgpu_buffer_rsrc_t rY = conv_out_rsrc(a.Y + (size_t)m0c * a.y_ld, a.M - m0c, GM, (size_t)a.y_ld * 4);
            const unsigned ybytes = (unsigned)a.y_ld * 4u;
            const bool hb_ = a.bias != nullptr, hs_ = a.scale != nullptr;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int cl = wc * 128 + j * 32 + 8 * gq + 4 * lh;           // first of the lane's four channels, within the tile
                    const float4 cb = hb_ ? *(const float4*)(Ps + cl) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float4 cs = hs_ ? *(const float4*)(Ps + 256 + cl) : make_float4(1.f, 1.f, 1.f, 1.f);
                    const float4 ch = hs_ ? *(const float4*)(Ps + 512 + cl) : make_float4(0.f, 0.f, 0.f, 0.f);
                    const float cbv[4] = {cb.x, cb.y, cb.z, cb.w}, csv[4] = {cs.x, cs.y, cs.z, cs.w}, chv[4] = {ch.x, ch.y, ch.z, ch.w};
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        f32x4 o;
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float v = acc[i][j][4 * gq + e] + cbv[e];
                            acc[i][j][4 * gq + e] = 0.0f;
                            v = fmaxf(v, v * slope);
                            o[e] = v * csv[e] + chv[e];
                        }
                        const unsigned vo = (unsigned)(wr * 64 + i * 32 + li) * ybytes + (unsigned)(n0c + cl) * 4u;
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, o), rY, vo, 0, 0);
                    }
                }
            }
            } else if constexpr (P == 2) {
            // ---- epilogue, 16 x 16 blocks.  C layout: register r of acc16[i][j], lane l = row 16 i + 4 (l >> 4) + r, column 16 j + (l & 15).
            // Same passage as the 32 x 32 form below: bias / activation / BatchNorm per value, a 4 x 4 transpose across the lane quad (four
            // consecutive columns of one row per lane), the wave's 4 KB strip sixteen rows (one i) at a time, whole rows back, 16-byte stores.
            const float slope = conv_act_slope(a.act1);
            const int lq = lane & 3;
            _Float16* const Y = (_Float16*)a.Y;
            char* const strip = lds + 2 * G_STAGE + wid * G_STRIP;               // [16 rows][256 bytes], 16-byte chunk c of row r at c ^ r
            float cb[8], cs[8], ch[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int cc = n0c + wc * 128 + j * 16 + l15;
                conv_col_params(a, cc, cb[j], cs[j], ch[j]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    float x[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float v = acc16[i][j][e] + cb[j];
                        acc16[i][j][e] = 0.0f;
                        v = fmaxf(v, v * slope);
                        x[e] = v * cs[j] + ch[j];
                    }
                    quad_transpose4(x[0], x[1], x[2], x[3], lq);
                    // the lane now holds row 4 (l >> 4) + lq of the block, columns 16 j + (l15 & ~3) .. + 3
                    const int sr = 4 * l4 + lq;
                    if (a.y_f32) {
                        const int g = m0c + wr * 64 + i * 16 + sr;
                        const int co = n0c + wc * 128 + j * 16 + (l15 & ~3);
                        if (g < a.M) *(float4*)(a.Y + (size_t)g * a.y_ld + co) = make_float4(x[0], x[1], x[2], x[3]);
                    } else {
                        const half4 hv = {(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3]};
                        *(half4*)(strip + sr * 256 + (((2 * j + (l15 >> 3)) ^ sr) * 16) + ((l15 >> 2) & 1) * 8) = hv;
                    }
                }
                if (!a.y_f32) {
                    const int c16 = lane & 15, rr = lane >> 4;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const float4 v = *(const float4*)(strip + (4 * t + rr) * 256 + ((c16 ^ (4 * t + rr)) * 16));
                        const int g = m0c + wr * 64 + i * 16 + 4 * t + rr;
                        if (g < a.M) *(float4*)(Y + (size_t)g * a.y_ld + n0c + wc * 128 + c16 * 8) = v;
                    }
                }
            }
            } else {
            // ---- epilogue.  C layout: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
            // The wave's 64 x 128 outputs pass through a wave-private 4 KB LDS strip, sixteen rows at a time: written as the accumulators lie
            // after the 4 x 4 quad transpose (8 bytes per lane), read back as whole 256-byte rows and stored 16 bytes per lane -- 16 store
            // instructions per wave, each four complete rows (the register-staged kernel: 32 stores of eight 64-byte segments).
            // [Tried: the weight fragment as the MFMA's first operand, which hands every lane four consecutive channels of one row and
            // needs no cross-lane transposes -- but then a lane needs the bias / BatchNorm parameters of 64 channels instead of 4, and
            // fetching them inside the loop (3 dependent float4 loads per register group) cost more than the 3 VALU per value it saved.]
            const float slope = conv_act_slope(a.act1);
            const int lq = lane & 3;
            _Float16* const Y = (_Float16*)a.Y;
            char* const strip = lds + 2 * G_STAGE + wid * G_STRIP;               // [16 rows][256 bytes], 16-byte chunk c of row r at c ^ r
            float cb[4], cs[4], ch[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int cc = n0c + wc * 128 + j * 32 + li;
                conv_col_params(a, cc, cb[j], cs[j], ch[j]);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i) {
#pragma unroll
                for (int hq = 0; hq < 2; ++hq) {                                    // sixteen rows: gq = 2 hq, 2 hq + 1
#pragma unroll
                    for (int g2 = 0; g2 < 2; ++g2) {
                        const int gq = 2 * hq + g2;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            float x[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                float v = acc[i][j][4 * gq + e] + cb[j];
                                acc[i][j][4 * gq + e] = 0.0f;
                                v = fmaxf(v, v * slope);
                                x[e] = v * cs[j] + ch[j];
                            }
                            quad_transpose4(x[0], x[1], x[2], x[3], lq);
                            // the lane now holds row 8 g2 + 4 lh + lq of the strip, columns 32 j + (li & ~3) .. + 3
                            if (a.y_f32) {
                                const int g = m0c + wr * 64 + i * 32 + 8 * gq + 4 * lh + lq;
                                const int co = n0c + wc * 128 + j * 32 + (li & ~3);
                                if (g < a.M) *(float4*)(a.Y + (size_t)g * a.y_ld + co) = make_float4(x[0], x[1], x[2], x[3]);
                            } else {
                                const half4 hv = {(_Float16)x[0], (_Float16)x[1], (_Float16)x[2], (_Float16)x[3]};
                                const int sr = 8 * g2 + 4 * lh + lq;
                                *(half4*)(strip + sr * 256 + (((j * 4 + (li >> 3)) ^ sr) * 16) + ((li >> 2) & 1) * 8) = hv;
                            }
                        }
                    }
                    if (!a.y_f32) {
                        // whole rows back: lane reads 16 bytes of row 4 t + (lane >> 4); the wave's LDS operations execute in order, so these
                        // reads see the writes above and the next strip's writes come behind them
                        const int c16 = lane & 15, rr = lane >> 4;
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            const float4 v = *(const float4*)(strip + (4 * t + rr) * 256 + ((c16 ^ (4 * t + rr)) * 16));
                            const int g = m0c + wr * 64 + i * 32 + 16 * hq + 4 * t + rr;
                            if (g < a.M) *(float4*)(Y + (size_t)g * a.y_ld + n0c + wc * 128 + c16 * 8) = v;
                        }
                    }
                }
            }
            }
            q = sch.next(a, q);
            if (q >= sch.sb_end) break;
            sch.origin(a, q, GM, GN, m0c, n0c);
            s = 0;
        } else {
            ++s;
        }
        buf ^= 1;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the load stream runs past the last tile: nothing may be in flight when the LDS is given back
}

// returns 1 when the layer does not fit this kernel (the caller then uses the register-staged forms)
int launch_conv_gemm_g256(sd_ctx* c, const ConvArgs& in, const char* tag)
{
    ConvArgs a = in;
    const bool h = a.prec == 1;
    if ((a.prec != 1 && a.prec != 0) || !a.rowtab || (h && !a.W16) || (!h && !a.W) || a.X2 || a.item_bias || a.R || a.act2 || a.pad_mode != 0 || a.Cout < 256 || (a.Cout % GN) != 0 ||
        (a.y_ld & 3) || a.Cin % (h ? 64 : 32) != 0 || a.M < 8 * GM || (a.x_ld & (h ? 7 : 3)) || (!h && a.y_f32)) return 1;
    if ((int64_t)a.Cin * (a.kt_real > 0 ? a.kt_real : a.KT) < (c->conv_w256_kmin > 0 ? c->conv_w256_kmin : (h ? 256 : 128))) return 1;
    if (((size_t)a.X & 15) || ((size_t)(h ? a.W16 : (const void*)a.W) & 15)) return 1;
    const size_t lds_bytes = (size_t)2 * G_STAGE + 8 * G_STRIP;       // (f32: 3 KB of parameters where the fp16 form keeps its strips)
    if (!conv_set_dyn_lds(c, g_attr_g256, {(const void*)k_conv_gemm_g256<1>, (const void*)k_conv_gemm_g256<2>, (const void*)k_conv_gemm_g256<0>}, lds_bytes)) return 1;
    a.sched = c->conv_pn;
    a.stagger = c->conv_rot;
    const int grid = conv_tiles_grid(c, a, GM, GN, 1);
    {
        ConvProfWide prof(c, tag, h ? "f16" : "f32", conv_bill(a, (double)a.M, h));
        const bool m16 = h && c->conv_mfma16 && ((int64_t)a.Cin * a.KT >= 1024 || c->conv_mfma16 == 2);
        c->last_conv_kernel = m16 ? "g256_m16" : h ? "g256_m32" : "g256_f32";
        if (m16) hipLaunchKernelGGL(k_conv_gemm_g256<2>, dim3(grid), dim3(512), lds_bytes, c->stream, a);
        else if (h) hipLaunchKernelGGL(k_conv_gemm_g256<1>         /* short contractions (block0, K = 640): 523 TF on this form against 486 */, dim3(grid), dim3(512), lds_bytes, c->stream, a);
        else hipLaunchKernelGGL(k_conv_gemm_g256<0>, dim3(grid), dim3(512), lds_bytes, c->stream, a);
    }
    if (hipGetLastError() != hipSuccess) SD_FAIL(c, SD_ERR_HIP, "k_conv_gemm_g256 launch failed (%s)", tag);
    return SD_OK;
}
