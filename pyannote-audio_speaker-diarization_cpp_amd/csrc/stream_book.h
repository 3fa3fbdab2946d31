// stream_book.h -- host bookkeeping of an sd_stream (stream.hip): the sealing rule, the offsets of the device tail, the growth of the
// score / embedding cache, and the ranges of streams -- or recordings (many.hip) -- that share a pack: pack_range, pack_plan.  The record of a range
// (PackRange) and the side rule (seg_tile_chunks) are many_plan.h's.  No HIP in here: every device operation goes through the Dev parameter, so the
// same code runs against malloc'd memory under AddressSanitizer in tools/sanitize/stream_*_main.cpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/sdhip.h"
#include "many_plan.h"

#define SD_TAIL_PAD 512                                    // zeroed floats behind the last sample: SD_WAV_PAD, what DevWav::padded promises (common.h; stream.hip asserts the two agree)
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
    int64_t origin = 0;            // samples forgotten in front of sample 0 of this book (book_forget); n, sealed and pending_n count from there
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

// the second tail buffer, the compaction target, can take `keep` samples and their padding; what it held is nobody's
template <class Dev> int book_reserve_spare(Dev& d, StreamBook& b, int64_t keep)
{
    const int o = 1 - b.cur;
    if (b.tail_cap[o] >= keep + SD_TAIL_PAD) return 0;
    if (b.tail[o]) d.release(b.tail[o]);
    b.tail[o] = nullptr; b.tail_cap[o] = 0;
    const int64_t cap = 2 * (keep + SD_TAIL_PAD);
    void* p = nullptr;
    if (int rc = d.alloc(&p, (size_t)cap * sizeof(float))) return rc;
    b.tail[o] = (float*)p; b.tail_cap[o] = cap;
    return 0;
}

// A copy as a row of a table (stream.hip: group_copy): dst[0, len) = src[0, len), zeros behind as the kernel says, nothing at or behind dst[room]
struct GroupRow { const void* src; float* dst; int64_t len, room; };

// chunks [sealed, to) have their final rows: the audio in front of sample to * 8000 goes.  Source and destination of that move overlap inside one
// buffer, so it goes to the second one and the two change places.  In steps, so that a group call can make ONE launch of the moves of all its streams:
// the move as a row (SD_TAIL_PAD zeros behind) and the book after it -- the target has its room (book_reserve_spare) -- ...
inline bool book_seal_planned(StreamBook& b, int64_t to, GroupRow& mv)
{
    if (to <= b.sealed) return false;
    const int64_t drop = (to - b.sealed) * SD_HOP, keep = b.tail_len() - drop;      // keep > 72 000: chunk to - 1 ends in front of n
    const int o = 1 - b.cur;
    mv = GroupRow{b.tail[b.cur] + drop, b.tail[o], keep, b.tail_cap[o]};
    b.cur = o; b.sealed = to; b.pending_n = -1;
    return true;
}
// ... and once the move has been issued: a spare buffer above SD_TAIL_SPARE_MAX floats is given back (release waits for the device)
template <class Dev> void book_seal_trim(Dev& d, StreamBook& b)
{
    const int o = 1 - b.cur;
    if (b.tail_cap[o] > SD_TAIL_SPARE_MAX) { d.release(b.tail[o]); b.tail[o] = nullptr; b.tail_cap[o] = 0; }
}
// the single stream's seal.  A failed allocation leaves n, sealed, cur, the tail's samples and the caches as they were
template <class Dev> int book_seal(Dev& d, StreamBook& b, int64_t to)
{
    if (to <= b.sealed) return 0;
    if (int rc = book_reserve_spare(d, b, b.tail_len() - (to - b.sealed) * SD_HOP)) return rc;
    GroupRow mv;
    book_seal_planned(b, to, mv);
    if (int rc = d.move_tail(mv.dst, (const float*)mv.src, mv.len)) return rc;
    book_seal_trim(d, b);
    return 0;
}

// The sliding window: all but the last keep_blocks sealed blocks go.  D = sealed - 32 * keep_blocks chunks (nothing where D <= 0): the sealed rows
// behind them move to the front of fresh, smaller caches -- two different allocations, so a plain copy; the old ones are given back -- and the book
// counts from sample D * 8000 on: n and sealed drop, origin rises.  The tail starts at sample sealed * 8000 before and after and is not touched.
// D is a multiple of 32 chunks, so the blocks and the 96-item embedding batches lie where a book fed the kept samples alone has them.  The pending
// rows are NOT kept: the kernels behind a pending chunk's score row depend on how many chunks lie in front of it in its segmentation batch
// (stream.hip: segment_pending), which D changes; the next turns call infers them again, as it does after any push.
// A failed allocation or copy leaves the book what it was.  Returns 0 or the Dev's code; *dropped (may be null) = D or 0.
template <class Dev> int book_forget(Dev& d, StreamBook& b, int64_t keep_blocks, int64_t* dropped = nullptr)
{
    if (dropped) *dropped = 0;
    if (keep_blocks < 0) return SD_ERR_ARG;
    if (keep_blocks >= b.sealed / SD_SEAL_CHUNKS) return 0;
    const int64_t D = b.sealed - SD_SEAL_CHUNKS * keep_blocks, keep = b.sealed - D;
    const int64_t total = sd_chunk_rule(b.n - D * SD_HOP, nullptr);                  // the chunks of what stays: room for its pending rows too
    const int64_t cap = total > 64 ? total : 64;
    void *ps = nullptr, *pe = nullptr;
    if (int rc = d.alloc(&ps, (size_t)(cap * SD_SEG_ROW) * sizeof(float))) return rc;
    if (int rc = d.alloc(&pe, (size_t)(cap * SD_EMB_ROW) * sizeof(float))) { d.release(ps); return rc; }
    if (keep > 0) {
        int rc = d.copy(ps, b.seg + D * SD_SEG_ROW, (size_t)(keep * SD_SEG_ROW) * sizeof(float));
        if (!rc) rc = d.copy(pe, b.emb + D * SD_EMB_ROW, (size_t)(keep * SD_EMB_ROW) * sizeof(float));
        if (rc) { d.release(ps); d.release(pe); return rc; }
    }
    d.release(b.seg); d.release(b.emb);
    b.seg = (float*)ps; b.emb = (float*)pe; b.cache_cap = cap;
    b.n -= D * SD_HOP; b.sealed -= D; b.origin += D * SD_HOP; b.pending_n = -1;
    if (dropped) *dropped = D;
    return 0;
}

template <class Dev> void book_release(Dev& d, StreamBook& b)
{
    for (int q = 0; q < 2; ++q) { if (b.tail[q]) d.release(b.tail[q]); b.tail[q] = nullptr; b.tail_cap[q] = 0; }
    if (b.seg) d.release(b.seg);
    if (b.emb) d.release(b.emb);
    b.seg = b.emb = nullptr; b.cache_cap = 0;
}

// ------------------------------------------------------------------ ranges and their slots (sd_diarize_many*; sd_stream_push_many*, sd_stream_turns_many)
// What a group call infers for one stream is a RANGE: chunks [lo, hi) of the stream, lo = sealed (a multiple of 32), audio in the tail from sample
// lo * 8000 on.  A block that became sealed has full chunks only; the pending range ends at the stream's last chunk, which may be short.  A range
// is packed as a recording of r.n samples (many_plan.h): the samples behind lo * 8000 for the pending range, (hi - lo + 9) * 8000 -- the end of
// chunk hi - 1 -- for a sealed one, so sd_chunk_rule(r.n) is hi - lo with the stream's own last length and the slot is roundup32(hi - lo + 9).
// A recording of sd_diarize_many* is the pending range of a stream with nothing sealed.

// the range a stream of n samples with `sealed` sealed chunks contributes: pending = its chunks [sealed, total), else the blocks [sealed, sealed(n)).
// false, and r.chunks = 0: none (no chunk yet / nothing became sealed)
inline bool pack_range(int64_t n, int64_t sealed, int64_t cb, bool pending, PackRange& r)
{
    r = PackRange{};
    r.lo = sealed;
    if (pending) {
        r.n = n - sealed * SD_HOP;
        r.chunks = sd_chunk_rule(r.n, &r.last_len);
        r.full = (r.last_len > 0 && r.last_len < SD_CHUNK) ? r.chunks - 1 : r.chunks;
    } else {
        r.chunks = stream_sealed_chunks(n) - sealed;
        r.n = (r.chunks + SD_MANY_GAP) * SD_HOP;
        r.full = r.chunks; r.last_len = SD_CHUNK;
    }
    if (r.chunks <= 0) { r.chunks = 0; return false; }
    r.tile = seg_tile_chunks(r.lo, r.full, cb, pending);
    return true;
}

// slots for the ranges by many_plan's rule, base in place; 0, or 1 where many_plan refuses
inline int pack_plan(PackRange* r, int64_t count, int64_t* total_chunks)
{
    *total_chunks = 0;
    if (count < 1) return 0;
    std::vector<int64_t> n((size_t)count), base((size_t)count);
    for (int64_t i = 0; i < count; ++i) n[(size_t)i] = r[i].n;
    if (many_plan(n.data(), count, base.data(), total_chunks)) return 1;
    for (int64_t i = 0; i < count; ++i) r[i].base = base[(size_t)i];
    return 0;
}

// Growth before launch: everything a group call will need of one stream -- room for `more` samples behind the tail, cache rows for the chunks it
// has afterwards, and, where blocks become sealed, a compaction target that holds what stays -- so that no allocation can fail between the kernels.
// The samples and rows held move along; a failure leaves the stream what it was.
template <class Dev> int book_reserve_group(Dev& d, StreamBook& b, int64_t more)
{
    if (int rc = book_reserve_tail(d, b, more)) return rc;
    const int64_t n = b.n + more, to = stream_sealed_chunks(n);
    if (int rc = book_reserve_cache(d, b, sd_chunk_rule(n, nullptr))) return rc;
    return to <= b.sealed ? 0 : book_reserve_spare(d, b, n - to * SD_HOP);
}
