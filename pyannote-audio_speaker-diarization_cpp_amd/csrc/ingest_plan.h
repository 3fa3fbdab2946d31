// ingest_plan.h -- the host arithmetic of sd_diarize_many_audio* (many.hip) and the one text of the decode rule of a recording (include/sdhip.h,
// "recordings in their own rate and encoding"): G.711 and the element of a frame, used by the host entries (sd_g711_decode) and, under hipcc, by
// k_many_ingest (ingest.hip).  From R descriptors the planner makes the slots (PackRange through pack_range on len16), the row table of the kernel with
// its tile prefix, the byte layout of the upload -- every source at a 16-byte aligned offset of one workspace, only the bytes the rule reads -- and the
// largest input span of a tile.  No HIP in here: tools/sanitize/ingest_plan_main.cpp builds the same text alone under AddressSanitizer and UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/sdhip.h"
#include "many_plan.h"
#include "stream_book.h"        // pack_range, pack_plan
#include "resample_book.h"      // make_plan, resample_len, RS_BLOCK

#ifdef __HIPCC__
#define INGEST_HD __host__ __device__ __forceinline__
#else
#define INGEST_HD inline
#endif

// ITU-T G.711: the 16-bit value of a code (sd_g711_decode returns it; the sample is pcm_to_float of it)
INGEST_HD int32_t g711_mulaw(uint32_t code)
{
    const uint32_t u = ~code & 0xffu;
    const int32_t t = (int32_t)((((u & 15u) << 3) + 132u) << ((u >> 4) & 7u));
    const int32_t s = t - 132;
    return (u & 0x80u) ? -s : s;
}
INGEST_HD int32_t g711_alaw(uint32_t code)
{
    const uint32_t a = (code ^ 0x55u) & 0xffu, e = (a >> 4) & 7u, m = a & 15u;
    const int32_t s = e ? (int32_t)(((m << 4) + 264u) << (e - 1u)) : (int32_t)((m << 4) + 8u);
    return (a & 0x80u) ? s : -s;
}

inline int ingest_elem_bytes(int32_t enc) { return enc == SD_ENC_S16 ? 2 : enc == SD_ENC_F32 ? 4 : (enc == SD_ENC_MULAW || enc == SD_ENC_ALAW) ? 1 : 0; }

#define SD_INGEST_MAX_BYTES ((int64_t)1 << 42)      /* per recording: R < 2^20 of them stay far inside int64 */

// sd_audio_len16: the 16 kHz samples a descriptor defines; -1 for a bad one (n < 0 or beyond SD_MANY_MAX_SAMPLES frames, a rate <= 0, an unknown
// encoding, channels < 1, a channel outside [-1, channels)).  A null data pointer is the call's business, not the length's.
inline int64_t ingest_len16(const sd_audio& a)
{
    if (a.n < 0 || a.n > SD_MANY_MAX_SAMPLES || a.sample_rate <= 0 || !ingest_elem_bytes(a.encoding) || a.channels < 1 || a.channel < -1 || a.channel >= a.channels) return -1;
    return a.sample_rate == SD_SAMPLE_RATE ? a.n : resample_len(a.n, a.sample_rate, SD_SAMPLE_RATE);
}

// One row of k_many_ingest's table: dst[base, base + len16) = the recording's 16 kHz samples, zeros in dst[base + len16, base + len).  L == M: the
// frames are the samples; else the rate pair L / M with its tap table.  src = the first element of frame 0 (null: a row of zeros, n = len16 = 0).
struct IngestRow {
    const void* src; int64_t n;
    int64_t len16, base, len;
    const float* taps;      // [2J+1][L]; null where L == M
    int32_t L, M, J, enc, channels, channel;
};

enum IngestRefusal { INGEST_OK = 0, INGEST_BAD_DESC, INGEST_NULL_DATA, INGEST_RATE_TABLE, INGEST_RATE_LDS, INGEST_BYTES, INGEST_PACK_LIMITS, INGEST_TILES };

struct IngestPlan {
    std::vector<PackRange> rec;        // [R]; chunks = 0: no slot, status SD_ERR_SHORT
    int64_t total = 0;                 // chunks of the pack
    std::vector<IngestRow> rows;       // the recordings with a slot in list order (src = null, taps = null: the caller places them), then the pad row
    std::vector<int64_t> owner;        // [rows - 1]: the recording of a row
    std::vector<int64_t> tile0;        // [rows + 1]: tiles of RS_BLOCK outputs in front of a row
    std::vector<int64_t> src_off, src_bytes;      // [rows - 1]: the upload
    int64_t upload_bytes = 0;
    int64_t max_span = 0;              // floats of LDS the largest staging span takes (0: no off-rate row)
    int64_t bad = -1;                  // the recording a refusal names
};

// the refusals of a rate pair: resample_check's (the tap table, a span beyond the LDS) and resample_jobs' (the span and RS_BLOCK outputs in LDS)
inline int ingest_rate_refusal(const ResamplePlan& p)
{
    if ((2 * (int64_t)p.J + 1) * p.L > ((int64_t)64 << 20) || p.L > 0x7fffffff || p.M > 0x7fffffff) return INGEST_RATE_TABLE;
    if ((p.span + RS_BLOCK) * (int64_t)sizeof(float) > 160 * 1024) return INGEST_RATE_LDS;
    return INGEST_OK;
}

// bytes of the source the rule reads: whole frames in front of the last one, and of the last frame what its channel rule takes
inline int64_t ingest_src_bytes(const sd_audio& a)
{
    if (a.n <= 0) return 0;
    const __int128 elems = a.channel < 0 ? (__int128)a.n * a.channels : (__int128)(a.n - 1) * a.channels + a.channel + 1;
    const __int128 bytes = elems * ingest_elem_bytes(a.encoding);
    return bytes > (__int128)SD_INGEST_MAX_BYTES ? -1 : (int64_t)bytes;
}

// 0, or the refusal with plan.bad set.  cb = seg_batch_chunks; check_data: a null data pointer with n > 0 is refused
inline int ingest_plan(const sd_audio* a, int64_t R, int64_t cb, bool check_data, IngestPlan& plan)
{
    plan = IngestPlan();
    if (!a || R < 1 || R > ((int64_t)1 << 20)) return INGEST_PACK_LIMITS;
    plan.rec.resize((size_t)R);
    std::vector<ResamplePlan> rp((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        plan.bad = r;
        const int64_t len16 = ingest_len16(a[r]);
        if (len16 < 0) return INGEST_BAD_DESC;
        if (check_data && a[r].n > 0 && !a[r].data) return INGEST_NULL_DATA;
        if (make_plan(a[r].sample_rate, SD_SAMPLE_RATE, rp[(size_t)r])) return INGEST_BAD_DESC;
        if (a[r].sample_rate != SD_SAMPLE_RATE) if (int e = ingest_rate_refusal(rp[(size_t)r])) return e;
        if (ingest_src_bytes(a[r]) < 0) return INGEST_BYTES;
        if (len16 > SD_MANY_MAX_SAMPLES) return INGEST_PACK_LIMITS;
        pack_range(len16, 0, cb, true, plan.rec[(size_t)r]);
        plan.rec[(size_t)r].owner = r;
    }
    plan.bad = -1;
    if (pack_plan(plan.rec.data(), R, &plan.total)) return INGEST_PACK_LIMITS;
    if (plan.total > SD_MANY_MAX_CHUNKS) return INGEST_PACK_LIMITS;
    plan.tile0.push_back(0);
    for (const PackRange& q : plan.rec) {
        if (q.chunks <= 0) continue;
        const sd_audio& d = a[q.owner];
        const ResamplePlan& p = rp[(size_t)q.owner];
        const bool direct = d.sample_rate == SD_SAMPLE_RATE;
        IngestRow w{nullptr, d.n, q.n, q.base * (int64_t)SD_HOP, q.slot() * (int64_t)SD_HOP, nullptr,
                    direct ? 1 : (int32_t)p.L, direct ? 1 : (int32_t)p.M, direct ? 0 : (int32_t)p.J, d.encoding, d.channels, d.channel};
        plan.rows.push_back(w);
        plan.owner.push_back(q.owner);
        plan.src_off.push_back(plan.upload_bytes);
        plan.src_bytes.push_back(ingest_src_bytes(d));
        plan.upload_bytes += (plan.src_bytes.back() + 15) / 16 * 16;
        if (!direct && p.span > plan.max_span) plan.max_span = p.span;
        plan.tile0.push_back(plan.tile0.back() + (w.len + RS_BLOCK - 1) / RS_BLOCK);
    }
    // the zeroed floats behind the last slot (DevWav::padded; SD_TAIL_PAD = SD_WAV_PAD: many.hip asserts the two agree)
    plan.rows.push_back(IngestRow{nullptr, 0, 0, plan.total * (int64_t)SD_HOP, SD_TAIL_PAD, nullptr, 1, 1, 0, SD_ENC_F32, 1, 0});
    plan.tile0.push_back(plan.tile0.back() + (SD_TAIL_PAD + RS_BLOCK - 1) / RS_BLOCK);
    if (plan.tile0.back() > 0x7fffffff) return INGEST_TILES;
    return INGEST_OK;
}
