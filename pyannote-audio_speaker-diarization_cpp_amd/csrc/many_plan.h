// many_plan.h -- the host arithmetic of the packed layout of sd_diarize_many* (many.hip) and of the group calls of sd_stream (stream.hip): the slots,
// the one record of a slot (PackRange) and the one statement of the skinny / tile side rule (seg_tile_chunks) with its constant; and the list-file
// reader of `speakerDiarizer --many`.
// Plain C++ without a GPU header: the library, the command line and the stand-alone sanitizer programs (tools/many_plan_check.cpp, tools/sanitize/) include the same text.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>
#include "../../include/sdhip.h"

// chunk rule of SegmentModel::slide (sd.cpp:1419, 1457) = sd_num_chunks
inline int64_t sd_chunk_rule(int64_t n, int64_t* last_len)
{
    int64_t i = 0, cnt = 0;
    if (n > SD_CHUNK) { cnt = (n - SD_CHUNK + SD_HOP - 1) / SD_HOP; i = cnt * SD_HOP; }   // while (i + window < n), sd.cpp:1419
    int64_t ll = 0;
    if (i + 1 < n) { ll = n - i; cnt++; }                                                  // sd.cpp:1457
    if (last_len) *last_len = ll;
    return cnt;
}

// Recording r of n[r] samples has chunks_r = sd_chunk_rule(n[r]) chunks and gets a slot of roundup32(chunks_r + SD_MANY_GAP) chunks at chunk base
// chunk_base[r] = the sum of the earlier slots (sample base 8000 * chunk_base[r]); no chunk: an empty slot.  9 gap chunks = 72 000 samples: chunk
// chunks_r - 1 starts at sample 8000 (chunks_r - 1) and its 80 000-sample window ends at 8000 (chunks_r + 9), inside the slot.
// Returns 0, or 1 on a bad argument (a null pointer, R < 1, a length beyond SD_MANY_MAX_SAMPLES)
#define SD_MANY_GAP 9
#define SD_MANY_MAX_SAMPLES ((int64_t)1 << 40)      /* per recording: keeps every sum of this file far inside int64 for any R < 2^20 */
inline int64_t many_slot_chunks(int64_t n)
{
    const int64_t chunks = sd_chunk_rule(n, nullptr);
    return chunks <= 0 ? 0 : ((chunks + SD_MANY_GAP + 31) / 32) * 32;
}
inline int many_plan(const int64_t* n, int64_t R, int64_t* chunk_base, int64_t* total_chunks)
{
    if (!n || !chunk_base || !total_chunks || R < 1 || R > ((int64_t)1 << 20)) return 1;
    for (int64_t r = 0; r < R; ++r) if (n[r] > SD_MANY_MAX_SAMPLES) return 1;
    int64_t base = 0;
    for (int64_t r = 0; r < R; ++r) { chunk_base[r] = base; base += many_slot_chunks(n[r]); }
    *total_chunks = base;
    return 0;
}

// launch_conv_gemm (conv_gemm.hip): a plain f32 GEMM of at most SD_SKINNY_MAX_ROWS rows goes to k_skinny_gemm, a larger one to the 128 x 128 tile, whose K
// order differs in the last bits.  >= ROWTAB_MAX_ITEMS, so the per-utterance layers of an ECAPA batch always take the skinny kernel; PyanNet's dense
// layers have 293 rows per chunk, so a batch of up to SD_SKINNY_CHUNKS = 13 chunks takes it too, and a chunk's last bits say which side its batch was on
#define SD_SKINNY_MAX_ROWS 4096
#define SD_SKINNY_CHUNKS (SD_SKINNY_MAX_ROWS / SD_FRAMES)
#define SD_SEAL_CHUNKS 32      // a stream seals blocks of 32 chunks = 96 items = three whole reference embedding batches (sd.cpp:2429); the slots' unit too

// The side rule: how many of the `full` full chunks from chunk lo of a recording on, counted from lo, are on the tile side in the path their rows have to
// equal.  That path cuts them into batches of cb = seg_batch_chunks from lo on (run_segment); a batch of 13 chunks or fewer is on the skinny side.
// The exception is the pending range of a stream (stream.hip: segment_pending): 1 .. 13 pending full chunks whose batch in the whole path -- it starts
// at cb * (lo / cb) where cb is a multiple of 32 -- is past 13 chunks run in a batch padded to 14, on the tile side.  At lo = 0 it never fires: a
// recording of a pack is the pending range of a stream with nothing sealed.
inline int64_t seg_tile_chunks(int64_t lo, int64_t full, int64_t cb, bool pending)
{
    if (cb < 1) cb = 1;
    if (full <= 0) return 0;
    if (pending && full <= SD_SKINNY_CHUNKS) {
        const int64_t whole = (cb >= SD_SEAL_CHUNKS && cb % SD_SEAL_CHUNKS == 0) ? lo + full - cb * (lo / cb) : full;      // (a cb that cuts blocks: no promise)
        if (whole > SD_SKINNY_CHUNKS) return full;
    }
    if (cb <= SD_SKINNY_CHUNKS) return 0;
    const int64_t rem = full % cb;
    return (rem == 0 || rem > SD_SKINNY_CHUNKS) ? full : full - rem;
}

// One slot of a pack: a recording (lo = 0), or chunks [lo, lo + chunks) of a stream whose tail holds the audio from sample lo * 8000 on.  n, chunks,
// full and last_len describe the slot's samples as a recording of its own (sd_chunk_rule); stream_book.h: pack_range builds one, pack_plan sets base
struct PackRange {
    int64_t owner;                 // index in the call's list: the recording, or the stream
    int64_t lo, chunks;            // chunks of the owner
    int64_t n;                     // samples of the range as a recording of its own
    int64_t full, last_len;        // its full chunks; the length of its last chunk (80 000 unless short)
    int64_t tile;                  // seg_tile_chunks: chunks [lo, lo + tile) are on the tile side, the other full ones on the skinny side (many.hip: many_segment)
    int64_t base;                  // first chunk of the slot in the pack
    int64_t hi() const { return lo + chunks; }
    int64_t slot() const { return many_slot_chunks(n); }
};

// `speakerDiarizer --many LIST`: one wav path per line.  A trailing CR is dropped, an empty line and a line that starts with # are skipped; a NUL byte,
// a line of more than 4096 bytes, an unreadable file or a list without a path is an error (false, message in err)
inline bool many_read_list(const char* path, std::vector<std::string>& out, std::string& err)
{
    out.clear();
    FILE* f = path ? fopen(path, "rb") : nullptr;
    if (!f) { err = std::string("cannot open list file ") + (path ? path : "(null)"); return false; }
    std::string line;
    long long no = 1;
    bool ok = true;
    auto flush = [&]() {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (!line.empty() && line[0] != '#') out.push_back(line);
        line.clear(); ++no;
    };
    for (;;) {
        const int ch = fgetc(f);
        if (ch == EOF) { flush(); break; }
        if (ch == '\n') { flush(); continue; }
        if (ch == 0) { err = std::string(path) + ": line " + std::to_string(no) + " holds a NUL byte"; ok = false; break; }
        if (line.size() >= 4096) { err = std::string(path) + ": line " + std::to_string(no) + " is longer than 4096 bytes"; ok = false; break; }
        line.push_back((char)ch);
    }
    fclose(f);
    if (ok && out.empty()) { err = std::string(path) + ": no path in the list"; ok = false; }
    if (!ok) out.clear();
    return ok;
}
