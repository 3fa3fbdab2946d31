// stream_ingest_plan.h -- the host arithmetic of sd_stream_push_audio* and sd_stream_push_many_audio* (stream.hip): a stream with an input
// format (sd_stream_set_input_format) takes interleaved frames in its own encoding, and k_group_ingest (stream_ingest.hip) decodes the pieces of all
// streams of a call in one launch.  From S pieces (pointer, frames, format) this file makes the refusals with the stream they name; with the
// destinations, the row table of the kernel, and for the host form the uploads: rows whose pointer, frames, encoding and channel count are equal -- the
// legs of one stereo call, which differ in the channel only -- share ONE upload, only the bytes the rule reads go up (ingest_src_bytes; the largest among
// the rows that share), and every upload is placed so that its first row's source is 16-byte aligned where its destination is (frame `head`), which is
// what lets the kernel read it with wide loads.  No HIP in here: tools/sanitize/stream_ingest_main.cpp builds the same text alone under AddressSanitizer
// and UBSan.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>
#include "../../include/sdhip.h"
#include "ingest_plan.h"        // ingest_elem_bytes, ingest_src_bytes, SD_INGEST_MAX_BYTES

// the input format of a stream (sd_stream_set_input_format); set = false: a stream of the typed pushes
struct StreamFormat { int32_t enc = SD_ENC_S16, channels = 1, channel = 0; bool set = false; };

inline bool stream_format_ok(int32_t enc, int32_t channels, int32_t channel) { return ingest_elem_bytes(enc) != 0 && channels >= 1 && channel >= -1 && channel < channels; }

// One row of k_group_ingest's table: dst[0, len) = frames [0, len) of src by steps 1 and 2 of the rule, `pad` zeros behind (the kernel's argument), nothing
// at or behind dst[room].  src = the first element of frame 0.
struct StreamIngestRow { const void* src; float* dst; int64_t len, room; int32_t enc, channels, channel, reserved; };

// what one stream is handed in a call
struct StreamPiece { const void* data; int64_t frames; StreamFormat f; };

enum StreamIngestRefusal { SI_OK = 0, SI_NO_FORMAT, SI_FRAMES, SI_NULL_DATA, SI_BYTES, SI_ALIGN };

// bytes of the piece the rule reads (ingest_src_bytes); -1 beyond SD_INGEST_MAX_BYTES
inline int64_t stream_piece_bytes(const StreamPiece& p)
{
    const sd_audio a{p.data, p.frames, SD_SAMPLE_RATE, p.f.enc, p.f.channels, p.f.channel};
    return ingest_src_bytes(a);
}

// The refusals of the pieces themselves, in list order: 0, or the refusal with *bad = the stream it names.  A piece of no frames is legal with any
// pointer, on a stream without a format too (nothing is handed over).  dev: the pointers are device pointers and must be aligned to their element.
inline int stream_ingest_check(const StreamPiece* p, int64_t S, bool dev, int64_t* bad)
{
    for (int64_t i = 0; i < S; ++i) {
        *bad = i;
        if (p[i].frames < 0 || p[i].frames > SD_MANY_MAX_SAMPLES) return SI_FRAMES;
        if (p[i].frames == 0) continue;
        if (!p[i].f.set) return SI_NO_FORMAT;
        if (!p[i].data) return SI_NULL_DATA;
        if (stream_piece_bytes(p[i]) < 0) return SI_BYTES;
        if (dev && (uintptr_t)p[i].data % (uintptr_t)ingest_elem_bytes(p[i].f.enc) != 0) return SI_ALIGN;
    }
    *bad = -1;
    return SI_OK;
}

struct StreamIngestPlan {
    std::vector<StreamIngestRow> rows;      // the pieces with frames > 0 in list order; host form: src = null, the caller adds the stage to up_off[cls]
    std::vector<int64_t> cls;               // [rows]: the upload a row reads (host form)
    std::vector<const void*> up_src;        // [uploads]: the caller's pointer
    std::vector<int64_t> up_off, up_bytes;  // [uploads]: bytes into the stage, bytes that go up
    int64_t upload_bytes = 0;               // the stage
};

// floats in front of the first 16-byte boundary of a destination: the kernel's group 0
inline int64_t stream_ingest_head(const float* dst) { return (int64_t)((16 - ((uintptr_t)dst & 15)) & 15) / 4; }

// The table of checked pieces (stream_ingest_check) once the destinations are known: dst[i] / room[i] for stream i (unused where frames == 0).
// host: the sharing classes and the layout of the stage (a 16-byte aligned allocation); else the rows read the callers' device pointers.
inline void stream_ingest_plan(const StreamPiece* p, float* const* dst, const int64_t* room, int64_t S, bool host, StreamIngestPlan& plan)
{
    plan = StreamIngestPlan();
    std::map<std::tuple<const void*, int64_t, int32_t, int32_t>, int64_t> seen;
    for (int64_t i = 0; i < S; ++i) {
        if (p[i].frames <= 0) continue;
        const StreamFormat& f = p[i].f;
        plan.rows.push_back(StreamIngestRow{host ? nullptr : p[i].data, dst[i], p[i].frames, room[i], f.enc, f.channels, f.channel, 0});
        if (!host) { plan.cls.push_back(-1); continue; }
        const int64_t bytes = stream_piece_bytes(p[i]);
        const auto key = std::make_tuple(p[i].data, p[i].frames, f.enc, f.channels);
        const auto it = seen.find(key);
        if (it != seen.end()) {      // a leg of a call that is already going up: the same device bytes, the larger count
            plan.cls.push_back(it->second);
            if (bytes > plan.up_bytes[(size_t)it->second]) plan.up_bytes[(size_t)it->second] = bytes;
            continue;
        }
        seen.emplace(key, (int64_t)plan.up_src.size());
        plan.cls.push_back((int64_t)plan.up_src.size());
        plan.up_src.push_back(p[i].data);
        plan.up_bytes.push_back(bytes);
        plan.up_off.push_back(0);
    }
    // offsets once every upload has its bytes: upload u starts where frame `head` of its first row is 16-byte aligned.  head * bytes-per-frame is a
    // multiple of the element size, so the offset is one too
    std::vector<int64_t> first(plan.up_src.size(), -1);
    for (size_t q = 0; q < plan.rows.size(); ++q) if (host && first[(size_t)plan.cls[q]] < 0) first[(size_t)plan.cls[q]] = (int64_t)q;
    int64_t at = 0;
    for (size_t u = 0; u < plan.up_src.size(); ++u) {
        const StreamIngestRow& w = plan.rows[(size_t)first[u]];
        const int64_t lead = (stream_ingest_head(w.dst) * ingest_elem_bytes(w.enc) * w.channels) % 16;
        while ((at + lead) % 16 != 0) ++at;
        plan.up_off[u] = at;
        at += plan.up_bytes[u];
    }
    plan.upload_bytes = at;
}
