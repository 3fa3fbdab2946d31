// ingest.hip -- k_many_ingest: the packed waveform of sd_diarize_many_audio* (many.hip) filled in ONE launch straight from the recordings as
// they arrive -- int16, float, mu-law or A-law elements, any channel count, any sample rate -- by the rule of include/sdhip.h ("recordings in their own
// rate and encoding"): decode, channel, rate.  The decode is ingest_plan.h's text (the host entries run the same) behind ingest_dev.h's IngestLoad, the rate step is resample_dev.h's
// resample_point, the body of k_resample and k_resample_jobs, with the staging load as its parameter: no tap arithmetic is restated here.
//
// The table (IngestRow, ingest_plan.h) has one row per slot and one for the SD_WAV_PAD floats behind the last slot; row r has tile0[r + 1] - tile0[r]
// tiles of RS_BLOCK outputs counted from its base, a block finds its row in the prefix table as k_resample_jobs does.  A tile takes one of three forms:
//   16 kHz row      the tile's frames are decoded and stored (thread per output: neighbouring threads read neighbouring frames)
//   off-rate row    the decoded input span of the tile is staged in LDS -- decode and channel rule applied while staging, zero outside [0, n) -- and the
//                   taps run over it (resample_point)
//   behind len16    zeros
// All three put the tile's 256 floats into LDS first; a full tile whose place in the pack is 16-byte aligned leaves as 64 stores of 16 bytes, any other
// tile as one float per thread.  A slot base is a multiple of 8 000 floats and a slot a multiple of 256 000, so in sd_diarize_many_audio* every tile of a
// slot is full and aligned; the pad row and the rows of the test hook (sdhip_ingest_test.h) reach the other path.  64-bit indices throughout; every
// store is guarded by the row's own length and by the length of the destination.
#include "common.h"
#include "ingest_plan.h"
#include "resample_dev.h"
#include "ingest_dev.h"      // IngestLoad: the staging load, steps 1 and 2 of the rule
#include <algorithm>
#include <cstring>

// dynamic LDS: [RS_BLOCK] the tile's outputs, 16-byte aligned at the base of the region (no static LDS in front of it) | the staging span of the call's
// largest rate pair
__global__ __launch_bounds__(RS_BLOCK) void k_many_ingest(const IngestRow* __restrict__ rows, const int64_t* __restrict__ tile0 /*[R + 1]*/, int R,
                                                           float* __restrict__ dst, int64_t dst_len)
{
    extern __shared__ __align__(16) float lds[];
    float* ys = lds;
    float* xs = lds + RS_BLOCK;
    const int64_t tile = blockIdx.x;
    int lo = 0, hi = R;                                                  // the last row with tile0[row] <= tile
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tile0[mid] <= tile) lo = mid; else hi = mid; }
    const IngestRow row = rows[lo];
    const int64_t off = (tile - tile0[lo]) * RS_BLOCK;                   // this tile's outputs go to dst[row.base + off ...]
    const IngestLoad load{row.src, row.enc, row.channels, row.channel};
    ys[threadIdx.x] = 0.0f;                                              // behind len16, and for the threads resample_point gives no output
    if (off < row.len16) {                                               // (the same for the whole block)
        if (row.L == row.M) {
            const int64_t m = off + threadIdx.x;
            if (m < row.len16) ys[threadIdx.x] = load(m);
        } else {
            const int span = (int)(((int64_t)(RS_BLOCK - 1) * row.M) / row.L) + 2 * row.J + 3;
            resample_point(xs, load, 0, row.n, off, row.len16, row.taps, row.L, row.M, row.J, span, ys);
        }
    }
    __syncthreads();
    const int64_t at = row.base + off;
    float* d = dst + at;
    const int64_t left = std::min(row.len - off, dst_len - at);          // floats of this tile and of the tiles behind it that may be written
    if (left >= RS_BLOCK && ((uintptr_t)d & 15) == 0) {
        if (threadIdx.x < RS_BLOCK / 4) reinterpret_cast<float4*>(d)[threadIdx.x] = reinterpret_cast<const float4*>(ys)[threadIdx.x];
    } else if (threadIdx.x < left) d[threadIdx.x] = ys[threadIdx.x];
}

// ONE launch for the table d_tab = [tile0: rows + 1 int64][rows] (the same table on the host: rows, tile0, for the grid and the LDS).  max_span = the
// largest staging span of the rows in floats (0: none is off-rate); the span and the RS_BLOCK outputs must fit the LDS (ingest_rate_refusal)
int launch_many_ingest(sd_ctx* c, const char* d_tab, const std::vector<IngestRow>& rows, const std::vector<int64_t>& tile0, int64_t max_span, float* d_dst, int64_t dst_len)
{
    const size_t R = rows.size();
    if (R < 1 || tile0.size() != R + 1 || tile0[R] < 1 || tile0[R] > 0x7fffffff || max_span < 0 || (max_span + RS_BLOCK) * (int64_t)sizeof(float) > 160 * 1024)
        SD_FAIL(c, SD_ERR_ARG, "launch_many_ingest: bad table (%zu rows, %lld tiles, span %lld)", R, (long long)(tile0.empty() ? 0 : tile0.back()), (long long)max_span);
    const size_t lds = (size_t)(RS_BLOCK + max_span) * sizeof(float);
    if (lds > 64 * 1024) HIPCHK(c, hipFuncSetAttribute((const void*)k_many_ingest, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    double flops = 0.0, bytes = 0.0;
    for (const IngestRow& w : rows) {
        bytes += 4.0 * (double)w.len + (double)ingest_elem_bytes(w.enc) * (double)w.n * (double)w.channels;
        if (w.L != w.M) flops += 2.0 * (double)(2 * w.J + 1) * (double)w.len16;
    }
    const int64_t* d_tile0 = (const int64_t*)d_tab;
    const IngestRow* d_rows = (const IngestRow*)(d_tab + (R + 1) * sizeof(int64_t));
    {
        ProfScope ps(c, "many_ingest", flops, bytes);
        hipLaunchKernelGGL(k_many_ingest, dim3((unsigned)tile0[R]), dim3(RS_BLOCK), lds, c->stream, d_rows, d_tile0, (int)R, d_dst, dst_len);
    }
    KCHECK(c);
    return SD_OK;
}

// the table as one block of bytes for one upload
std::vector<char> many_ingest_table(const std::vector<IngestRow>& rows, const std::vector<int64_t>& tile0)
{
    static_assert(sizeof(IngestRow) % sizeof(int64_t) == 0 && alignof(IngestRow) <= alignof(int64_t), "the rows sit behind rows + 1 int64");
    const size_t head = tile0.size() * sizeof(int64_t);
    std::vector<char> tab(head + rows.size() * sizeof(IngestRow));
    memcpy(tab.data(), tile0.data(), head);
    memcpy(tab.data() + head, rows.data(), rows.size() * sizeof(IngestRow));
    return tab;
}

// ------------------------------------------------------------------ host-only entries
extern "C" int64_t sd_audio_len16(const sd_audio* a) { return a ? ingest_len16(*a) : -1; }

extern "C" int sd_g711_decode(int32_t encoding, const uint8_t* codes, int64_t n, int16_t* out)
{
    if ((encoding != SD_ENC_MULAW && encoding != SD_ENC_ALAW) || n < 0 || (n > 0 && (!codes || !out))) return SD_ERR_ARG;
    for (int64_t i = 0; i < n; ++i) out[i] = (int16_t)(encoding == SD_ENC_MULAW ? g711_mulaw(codes[i]) : g711_alaw(codes[i]));
    return SD_OK;
}
