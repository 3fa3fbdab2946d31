// many_plan.h -- the host arithmetic of the packed layout of sd_diarize_many* (many.hip) and the list-file reader of `speakerDiarizer --many`.
// Plain C++ without a GPU header: the library, the command line and the stand-alone sanitizer program (tools/many_plan_check.cpp) include the same text.
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
