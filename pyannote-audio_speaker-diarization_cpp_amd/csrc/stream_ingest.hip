// stream_ingest.hip -- k_group_ingest: the pieces that the streams of one call are handed in their own encoding (sd_stream_push_audio*,
// sd_stream_push_many_audio*) decoded to the ends of their tails -- or, for a stream with an input rate, behind the inputs it holds -- in ONE
// launch.  It is group_copy's geometry (stream.hip) with IngestLoad (ingest_dev.h) as the load: steps 1 and 2 of the rule of include/sdhip.h run the text
// k_many_ingest runs.
//
// A row (StreamIngestRow, stream_ingest_plan.h): dst[0, len) = frames [0, len) of src, `pad` zeros behind, nothing at or behind dst[room].  A row is cut
// into groups of four floats at the 16-byte boundaries of its DESTINATION: group 0 is the 0 .. 3 floats in front of the first boundary, group g the four
// from head + 4 (g - 1) on, stored as one float4.  The four frames of a whole group are 4 * channels * (element size) contiguous bytes of the source; for one
// and two channels that is 4, 8, 16 or 32 bytes, read as one dword, one dwordx2, or one or two dwordx4 where the source is aligned at frame `head` (the
// host pushes are staged so that it is) and decoded from the registers by IngestLoad::of_bits -- the same decode, so the same bytes as the element-wise
// path, which every other group takes: three and more channels, an unaligned source, group 0, the last partial group, and the last whole group of a row
// that picks a channel other than the last one: its wide load would end behind the last element the rule reads, where the upload ends.
// grid (x: a stride over the groups of a row, y: a stride over the table), 256 threads; 64-bit indices throughout.
#include "common.h"
#include "stream_book.h"
#include "stream_ingest_plan.h"
#include "ingest_dev.h"
#include <algorithm>

// element e (counted from p) of a group held in the dwords w: ES = the element size in bytes
template <int ES> __device__ __forceinline__ uint32_t group_bits(const uint32_t* w, int e)
{
    return ES == 1 ? (w[e >> 2] >> (8 * (e & 3))) & 0xffu : ES == 2 ? (w[e >> 1] >> (16 * (e & 1))) & 0xffffu : w[e];
}

// the four frames at p (aligned to min(16, 4 * CH * ES) bytes) of CH = 1 or 2 channels
template <int CH, int ES> __device__ __forceinline__ float4 ingest_wide(const IngestLoad& load, const void* p)
{
    constexpr int W = CH * ES;      // dwords of the group: 1, 2, 4 or 8
    uint32_t w[W];
    if constexpr (W == 1) w[0] = *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (W == 2) { const uint2 v = *reinterpret_cast<const uint2*>(p); w[0] = v.x; w[1] = v.y; }
    else {
#pragma unroll
        for (int k = 0; k < W / 4; ++k) {
            const uint4 v = reinterpret_cast<const uint4*>(p)[k];
            w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
        }
    }
    float f[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (load.channel >= 0) {
            uint32_t b = group_bits<ES>(w, q * CH);
            if (CH == 2 && load.channel == 1) b = group_bits<ES>(w, q * CH + CH - 1);
            f[q] = load.of_bits(b);
        } else {      // IngestLoad's mean: s = +0.0f, s += x_q in channel order, the correctly rounded division
            float s = 0.0f;
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) s += load.of_bits(group_bits<ES>(w, q * CH + ch));
            f[q] = __fdiv_rn(s, (float)CH);
        }
    }
    return make_float4(f[0], f[1], f[2], f[3]);
}

__global__ __launch_bounds__(256) void k_group_ingest(const StreamIngestRow* __restrict__ rows, int R, int64_t pad)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        const StreamIngestRow row = rows[r];
        const IngestLoad load{row.src, row.enc, row.channels, row.channel};
        const int es = row.enc == SD_ENC_S16 ? 2 : row.enc == SD_ENC_F32 ? 4 : 1;
        const int64_t end = row.len + pad < row.room ? row.len + pad : row.room;      // floats of dst this row may write
        const int64_t n = row.len < end ? row.len : end;                               // ... that come from src
        // elements of src the rule reads for these n frames: no load may end behind them
        const int64_t elems = n <= 0 ? 0 : row.channel < 0 ? n * row.channels : (n - 1) * row.channels + row.channel + 1;
        int64_t head = (int64_t)((16 - ((uintptr_t)row.dst & 15)) & 15) / 4;
        if (head > end) head = end;
        const int64_t bpf = (int64_t)es * row.channels;                                // bytes of a frame
        const uintptr_t src_at_head = (uintptr_t)row.src + (uintptr_t)(head * bpf);
        const bool wide = row.channels <= 2 && (src_at_head & (uintptr_t)(4 * bpf < 16 ? 4 * bpf - 1 : 15)) == 0;
        for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ; g += step) {
            const int64_t i = g == 0 ? 0 : head + 4 * (g - 1);
            const int64_t cnt = g == 0 ? head : 4;
            if (i >= end) break;
            if (g > 0 && i + 4 <= end) {      // a whole aligned group: one 16-byte store
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (i + 4 <= n && wide && (i + 4) * row.channels <= elems) {
                    const void* p = (const char*)row.src + i * bpf;
                    if (row.channels == 1) v = es == 1 ? ingest_wide<1, 1>(load, p) : es == 2 ? ingest_wide<1, 2>(load, p) : ingest_wide<1, 4>(load, p);
                    else v = es == 1 ? ingest_wide<2, 1>(load, p) : es == 2 ? ingest_wide<2, 2>(load, p) : ingest_wide<2, 4>(load, p);
                } else {
                    if (i < n) v.x = load(i);
                    if (i + 1 < n) v.y = load(i + 1);
                    if (i + 2 < n) v.z = load(i + 2);
                    if (i + 3 < n) v.w = load(i + 3);
                }
                *reinterpret_cast<float4*>(row.dst + i) = v;
                continue;
            }
            for (int64_t j = i; j < i + cnt && j < end; ++j) row.dst[j] = j < n ? load(j) : 0.0f;
        }
    }
}

// ONE launch for the table d_rows (rows: the same table on the host, for the grid and the bill); pad = the zeros behind every row (SD_TAIL_PAD: a row that
// lands behind a rated stream's inputs has room = len and gets none).  stream.hip and the hook of stream_ingest_test.hip call this
int launch_group_ingest(sd_ctx* c, const StreamIngestRow* d_rows, const std::vector<StreamIngestRow>& rows, int64_t pad)
{
    if (rows.empty()) return SD_OK;
    int64_t longest = 1;
    double bytes = 0.0;
    for (const StreamIngestRow& w : rows) {
        longest = std::max(longest, w.len + pad);
        bytes += 4.0 * (double)std::min(w.len + pad, w.room) + (double)ingest_elem_bytes(w.enc) * (double)w.len * (double)w.channels;
    }
    const dim3 grid = many_grid(longest / 4 + 2, (int64_t)rows.size());
    {
        ProfScope ps(c, "group_ingest", 0.0, bytes);
        hipLaunchKernelGGL(k_group_ingest, grid, dim3(256), 0, c->stream, d_rows, (int)rows.size(), pad);
    }
    KCHECK(c);
    return SD_OK;
}
