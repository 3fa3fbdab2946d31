// stream_book.h -- host bookkeeping of an sd_stream (stream.hip): the sealing rule, the offsets of the device tail and the growth of the
// score / embedding cache.  No HIP in here: every device operation goes through the Dev parameter, so the same code runs against
// malloc'd memory under AddressSanitizer in tools/sanitize/stream_book_main.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/sdhip.h"

#define SD_TAIL_PAD 512                                    // zeroed floats behind the last sample: SD_WAV_PAD, what DevWav::padded promises (common.h; stream.hip asserts the two agree)
#define SD_SEAL_CHUNKS 32                                  // 96 items = three whole reference embedding batches (sd.cpp:2429)
#define SD_SEG_ROW ((int64_t)SD_FRAMES * SD_SPEAKERS)      // floats of one chunk in the score cache
#define SD_EMB_ROW ((int64_t)SD_SPEAKERS * SD_EMB_DIM)     // ... in the embedding cache
#define SD_TAIL_SPARE_MAX ((int64_t)1 << 22)               // a spare tail buffer above this many floats is given back after a compaction

// chunks k with k * 8000 + 80000 < n: the chunk that ends exactly at n goes through the reference's "last chunk" branch (sd.cpp:1457)
inline int64_t stream_full_chunks(int64_t n) { return n <= SD_CHUNK ? 0 : (n - SD_CHUNK - 1) / SD_HOP + 1; }
inline int64_t stream_sealed_chunks(int64_t n) { return SD_SEAL_CHUNKS * (stream_full_chunks(n) / SD_SEAL_CHUNKS); }

struct StreamBook {
    int64_t n = 0;                 // samples pushed so far
    int64_t sealed = 0;            // chunks [0, sealed): rows final, audio in front of sample sealed * 8000 dropped
    int64_t pending_n = -1;        // the n at which rows [sealed, total) were computed; valid while it equals n
    float* tail[2] = {nullptr, nullptr};      // tail[cur] holds samples [sealed * 8000, n) and SD_TAIL_PAD zeros; the other is the compaction target
    int64_t tail_cap[2] = {0, 0};  // floats
    int cur = 0;
    float* seg = nullptr;          // [cache_cap][293][3]
    float* emb = nullptr;          // [cache_cap * 3][192]
    int64_t cache_cap = 0;         // chunks
    int64_t tail_len() const { return n - sealed * SD_HOP; }
    float* tail_now() const { return tail[cur]; }
};

// Dev provides (every int: 0 or an SD_ERR_* code)
//   int alloc(void** p, size_t bytes);   void release(void* p);
//   int copy(void* dst, const void* src, size_t bytes);                 ranges of two different allocations
//   int move_tail(float* dst, const float* src, int64_t len);           dst[0, len) = src[0, len), dst[len, len + SD_TAIL_PAD) = 0; two different allocations

// room for `more` samples behind the tail, padding included; the samples held and their padding move along
template <class Dev> int book_reserve_tail(Dev& d, StreamBook& b, int64_t more)
{
    const int64_t need = b.tail_len() + more + SD_TAIL_PAD;
    if (need <= b.tail_cap[b.cur]) return 0;
    const int64_t cap = need > 2 * b.tail_cap[b.cur] ? need : 2 * b.tail_cap[b.cur];
    void* p = nullptr;
    if (int rc = d.alloc(&p, (size_t)cap * sizeof(float))) return rc;
    if (b.tail[b.cur]) {
        if (int rc = d.copy(p, b.tail[b.cur], (size_t)(b.tail_len() + SD_TAIL_PAD) * sizeof(float))) { d.release(p); return rc; }
        d.release(b.tail[b.cur]);
    }
    b.tail[b.cur] = (float*)p; b.tail_cap[b.cur] = cap;
    return 0;
}

// rows for `chunks` chunks in both caches; geometric growth, the rows held move along
template <class Dev> int book_reserve_cache(Dev& d, StreamBook& b, int64_t chunks)
{
    if (chunks <= b.cache_cap) return 0;
    int64_t cap = 2 * b.cache_cap > 64 ? 2 * b.cache_cap : 64;
    if (cap < chunks) cap = chunks;
    void *ps = nullptr, *pe = nullptr;
    if (int rc = d.alloc(&ps, (size_t)(cap * SD_SEG_ROW) * sizeof(float))) return rc;
    if (int rc = d.alloc(&pe, (size_t)(cap * SD_EMB_ROW) * sizeof(float))) { d.release(ps); return rc; }
    if (b.cache_cap > 0) {
        int rc = d.copy(ps, b.seg, (size_t)(b.cache_cap * SD_SEG_ROW) * sizeof(float));
        if (!rc) rc = d.copy(pe, b.emb, (size_t)(b.cache_cap * SD_EMB_ROW) * sizeof(float));
        if (rc) { d.release(ps); d.release(pe); return rc; }
        d.release(b.seg); d.release(b.emb);
    }
    b.seg = (float*)ps; b.emb = (float*)pe; b.cache_cap = cap;
    return 0;
}

// chunks [sealed, to) have their final rows: the audio in front of sample to * 8000 goes.  Source and destination of that move overlap
// inside one buffer, so it goes to the second one and the two change places.
template <class Dev> int book_seal(Dev& d, StreamBook& b, int64_t to)
{
    if (to <= b.sealed) return 0;
    const int64_t drop = (to - b.sealed) * SD_HOP, keep = b.tail_len() - drop;      // keep > 72 000: chunk to - 1 ends in front of n
    const int o = 1 - b.cur;
    if (b.tail_cap[o] < keep + SD_TAIL_PAD) {
        if (b.tail[o]) d.release(b.tail[o]);
        b.tail[o] = nullptr; b.tail_cap[o] = 0;
        const int64_t cap = 2 * (keep + SD_TAIL_PAD);
        void* p = nullptr;
        if (int rc = d.alloc(&p, (size_t)cap * sizeof(float))) return rc;
        b.tail[o] = (float*)p; b.tail_cap[o] = cap;
    }
    if (int rc = d.move_tail(b.tail[o], b.tail[b.cur] + drop, keep)) return rc;
    b.cur = o; b.sealed = to; b.pending_n = -1;
    if (b.tail_cap[1 - o] > SD_TAIL_SPARE_MAX) { d.release(b.tail[1 - o]); b.tail[1 - o] = nullptr; b.tail_cap[1 - o] = 0; }
    return 0;
}

template <class Dev> void book_release(Dev& d, StreamBook& b)
{
    for (int q = 0; q < 2; ++q) { if (b.tail[q]) d.release(b.tail[q]); b.tail[q] = nullptr; b.tail_cap[q] = 0; }
    if (b.seg) d.release(b.seg);
    if (b.emb) d.release(b.emb);
    b.seg = b.emb = nullptr; b.cache_cap = 0;
}
