// The sliding window of sd_stream (csrc/stream_book.h: book_forget) against malloc'd memory, for AddressSanitizer + UBSan.  CPU only;
// tools/sanitize/build_stream_window.sh builds it.
//   stream_window [seed]   books through random sequences of reserve, push, seal, forget, the window's policy and the group variants of the same steps,
//                          the device work done by host loops.  After every step the book's samples and rows are those of a fresh book fed the kept
//                          samples in one push; allocation failures at every allocation of a forget, a reserve and a seal leave the book unchanged.
//                          -> "stream_window ok: ..." and exit 0, or the first mismatch
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "stream_book.h"

struct HostDev {
    long allocs = 0, live = 0;
    long fail_in = -1;                       // >= 0: the allocation that many allocations from now fails
    int alloc(void** p, size_t bytes) {
        if (fail_in == 0) { fail_in = -1; *p = nullptr; return SD_ERR_HIP; }
        if (fail_in > 0) --fail_in;
        *p = malloc(bytes ? bytes : 1); ++allocs; ++live; return *p ? 0 : SD_ERR_HIP;
    }
    void release(void* p) { free(p); --live; }
    int copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    int move_tail(float* dst, const float* src, int64_t len) {
        memcpy(dst, src, (size_t)len * sizeof(float));
        for (int q = 0; q < SD_TAIL_PAD; ++q) dst[len + q] = 0.0f;
        return 0;
    }
};

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// what the recording holds at absolute sample i, what the networks give for absolute chunk c (sealed rows), and for a pending chunk computed at n samples
static float sample_of(int64_t i) { return (float)(i % 65521) - 32760.0f; }
static float row_of(int64_t c) { return (float)(c * 7 + 3); }
static float pending_of(int64_t c, int64_t n_abs) { return -(float)(c * 5 + n_abs % 1000 + 1); }

static void fill_rows(StreamBook& b, int64_t lo, int64_t hi, bool pending)
{
    const int64_t c0 = b.origin / SD_HOP;
    for (int64_t c = lo; c < hi; ++c) {
        const float v = pending ? pending_of(c0 + c, b.origin + b.n) : row_of(c0 + c);
        for (int64_t q = 0; q < SD_SEG_ROW; ++q) b.seg[c * SD_SEG_ROW + q] = v;
        for (int64_t q = 0; q < SD_EMB_ROW; ++q) b.emb[c * SD_EMB_ROW + q] = -v;
    }
}

static void append(StreamBook& b, int64_t m)
{
    float* dst = b.tail_now() + b.tail_len();
    for (int64_t j = 0; j < m; ++j) dst[j] = sample_of(b.origin + b.n + j);
    for (int q = 0; q < SD_TAIL_PAD; ++q) dst[m + q] = 0.0f;
    b.n += m;
}

// sd_stream_push: the single-stream path of stream.hip around the book
static int push_single(HostDev& d, StreamBook& b, int64_t m, int64_t window)
{
    if (int rc = book_reserve_tail(d, b, m)) return rc;
    append(b, m);
    const int64_t to = stream_sealed_chunks(b.n);
    if (to <= b.sealed) return 0;
    if (int rc = book_reserve_cache(d, b, sd_chunk_rule(b.n, nullptr))) return rc;
    fill_rows(b, b.sealed, to, false);
    const StreamBook was = b;
    d.fail_in = 0;      // the seal's one allocation, where it needs one, fails first: the book, the tail in use and the caches stay (the spare buffer is nobody's)
    int rc = book_seal(d, b, to);
    if (d.fail_in == -1) {
        CHECK(rc == SD_ERR_HIP && b.n == was.n && b.sealed == was.sealed && b.pending_n == was.pending_n && b.cur == was.cur && b.tail_now() == was.tail_now() &&
              b.tail_cap[b.cur] == was.tail_cap[was.cur] && b.seg == was.seg && b.emb == was.emb && b.cache_cap == was.cache_cap, "a failed allocation in seal changed the book");
        rc = book_seal(d, b, to);
    }
    d.fail_in = -1;
    if (rc) return rc;
    return window >= 0 ? book_forget(d, b, window) : 0;
}

// sd_stream_push_many for one stream of the group: growth before launch, append, rows, the planned compaction, then the window
static int push_group(HostDev& d, StreamBook& b, int64_t m, int64_t window)
{
    if (int rc = book_reserve_group(d, b, m)) return rc;
    const long before = d.allocs;
    append(b, m);
    const int64_t to = stream_sealed_chunks(b.n);
    if (to > b.sealed) {
        fill_rows(b, b.sealed, to, false);
        GroupRow mv;
        if (book_seal_planned(b, to, mv)) {
            CHECK(mv.len + SD_TAIL_PAD <= mv.room, "compaction target: %lld floats for %lld", (long long)mv.room, (long long)mv.len);
            memcpy(mv.dst, mv.src, (size_t)mv.len * sizeof(float));
            for (int q = 0; q < SD_TAIL_PAD; ++q) mv.dst[mv.len + q] = 0.0f;
        }
        CHECK(d.allocs == before, "an allocation between the kernels of a group push");
        book_seal_trim(d, b);
        if (window >= 0) if (int rc = book_forget(d, b, window)) return rc;
    }
    return 0;
}

// sd_stream_turns: the pending rows
static int turns(HostDev& d, StreamBook& b)
{
    const int64_t total = sd_chunk_rule(b.n, nullptr);
    if (total <= 0 || b.pending_n == b.n) return 0;
    if (int rc = book_reserve_cache(d, b, total)) return rc;
    fill_rows(b, b.sealed, total, true);
    b.pending_n = b.n;
    return 0;
}

// the book against a fresh one fed samples [origin, origin + n) of the recording in one push
static int verify(const StreamBook& b, int64_t origin_want)
{
    CHECK(b.origin == origin_want && b.origin % (SD_SEAL_CHUNKS * SD_HOP) == 0, "origin %lld, expected %lld", (long long)b.origin, (long long)origin_want);
    HostDev d;
    StreamBook f;
    f.origin = b.origin;                      // (only so that the helpers above name the same absolute samples and chunks)
    if (b.n > 0) CHECK(push_single(d, f, b.n, -1) == 0, "the fresh book failed");
    CHECK(f.n == b.n && f.sealed == b.sealed && f.tail_len() == b.tail_len(), "book: n %lld sealed %lld, fresh n %lld sealed %lld", (long long)b.n, (long long)b.sealed, (long long)f.n, (long long)f.sealed);
    CHECK(b.sealed == stream_sealed_chunks(b.n), "sealed %lld at n = %lld", (long long)b.sealed, (long long)b.n);
    if (b.n > 0) {
        CHECK(b.tail_cap[b.cur] >= b.tail_len() + SD_TAIL_PAD, "tail capacity");
        CHECK(memcmp(b.tail_now(), f.tail_now(), (size_t)(b.tail_len() + SD_TAIL_PAD) * sizeof(float)) == 0, "tail samples at n = %lld, origin %lld", (long long)b.n, (long long)b.origin);
    }
    CHECK(b.cache_cap >= b.sealed, "cache of %lld chunks for %lld sealed", (long long)b.cache_cap, (long long)b.sealed);
    if (b.sealed > 0) {
        CHECK(memcmp(b.seg, f.seg, (size_t)(b.sealed * SD_SEG_ROW) * sizeof(float)) == 0, "sealed score rows at n = %lld, origin %lld", (long long)b.n, (long long)b.origin);
        CHECK(memcmp(b.emb, f.emb, (size_t)(b.sealed * SD_EMB_ROW) * sizeof(float)) == 0, "sealed embedding rows at n = %lld, origin %lld", (long long)b.n, (long long)b.origin);
    }
    if (b.pending_n == b.n && b.n > 0) {
        const int64_t total = sd_chunk_rule(b.n, nullptr), c0 = b.origin / SD_HOP;
        CHECK(b.cache_cap >= total, "cache of %lld chunks for %lld", (long long)b.cache_cap, (long long)total);
        for (int64_t c = b.sealed; c < total; ++c) {
            const float v = pending_of(c0 + c, b.origin + b.n);
            CHECK(b.seg[c * SD_SEG_ROW] == v && b.seg[(c + 1) * SD_SEG_ROW - 1] == v && b.emb[c * SD_EMB_ROW] == -v && b.emb[(c + 1) * SD_EMB_ROW - 1] == -v, "pending row %lld", (long long)c);
        }
    }
    book_release(d, f);
    CHECK(d.live == 0, "the fresh book leaked");
    return 0;
}

static bool same_book(const StreamBook& a, const StreamBook& b)
{
    return a.n == b.n && a.sealed == b.sealed && a.pending_n == b.pending_n && a.tail[0] == b.tail[0] && a.tail[1] == b.tail[1] && a.tail_cap[0] == b.tail_cap[0] &&
           a.tail_cap[1] == b.tail_cap[1] && a.cur == b.cur && a.seg == b.seg && a.emb == b.emb && a.cache_cap == b.cache_cap && a.origin == b.origin;
}

static int run_case(std::mt19937_64& rng, int steps, int64_t max_push, int64_t window, bool group, long* allocs, long* forgets, long* failures)
{
    HostDev d;
    StreamBook b;
    int64_t origin = 0;
    for (int step = 0; step < steps; ++step) {
        const uint64_t what = rng() % 10;
        if (what < 6) {                                   // a push
            int64_t m = 1 + (int64_t)(rng() % (uint64_t)max_push);
            const uint64_t how = rng() % 6;
            if (how == 0) m = 1;
            if (how == 1) {      // to an edge of the sealing rule
                const int64_t edge = (stream_sealed_chunks(b.n) + SD_SEAL_CHUNKS - 1) * SD_HOP + SD_CHUNK + (int64_t)(rng() % 2);
                m = edge > b.n ? edge - b.n : 1;
            }
            if (how == 2) m = 2 * SD_SEAL_CHUNKS * SD_HOP + 5;      // two blocks at once
            const int64_t sealed_before = b.sealed, n_before = b.n;
            CHECK((group ? push_group(d, b, m, window) : push_single(d, b, m, window)) == 0, "push failed");
            if (window >= 0 && stream_sealed_chunks(n_before + m) > sealed_before) {
                const int64_t blocks = stream_sealed_chunks(n_before + m) / SD_SEAL_CHUNKS;
                if (blocks > window) { origin += (blocks - window) * SD_SEAL_CHUNKS * SD_HOP; ++*forgets; }
            }
        } else if (what < 8) {                            // turns
            CHECK(turns(d, b) == 0, "turns failed");
        } else {                                          // a forget by hand, first with every allocation of it failing in turn
            const int64_t keep = (int64_t)(rng() % 4);
            CHECK(book_forget(d, b, -1) == SD_ERR_ARG, "a negative keep_blocks was taken");
            for (long q = 0; q < 2; ++q) {
                const StreamBook was = b;
                const long live = d.live;
                d.fail_in = q;
                const int rc = book_forget(d, b, keep);
                const bool fired = d.fail_in == -1;
                d.fail_in = -1;
                if (!fired) { CHECK(rc == 0, "forget failed without a failing allocation"); CHECK(same_book(was, b), "a forget with nothing to drop changed the book"); break; }
                CHECK(rc == SD_ERR_HIP && same_book(was, b) && d.live == live, "a failed allocation in forget changed the book");
                ++*failures;
                if (verify(b, origin)) return 1;
            }
            int64_t dropped = 0;
            CHECK(book_forget(d, b, keep, &dropped) == 0, "forget failed");
            CHECK(dropped % SD_SEAL_CHUNKS == 0 && dropped >= 0, "dropped %lld chunks", (long long)dropped);
            origin += dropped * SD_HOP;
            *forgets += dropped > 0;
        }
        if (verify(b, origin)) return 1;
        // a failed allocation in the growth of the next step leaves the book what it is (reserve and seal are the existing paths; the window adds origin to them)
        if (rng() % 4 == 0) {
            const StreamBook was = b;
            const long live = d.live;
            d.fail_in = 0;
            const int rc = group ? book_reserve_group(d, b, 3000000) : book_reserve_tail(d, b, 3000000);
            d.fail_in = -1;
            CHECK(rc == SD_ERR_HIP && same_book(was, b) && d.live == live, "a failed reserve changed the book");
            ++*failures;
            if (verify(b, origin)) return 1;
        }
    }
    book_release(d, b);
    CHECK(d.live == 0, "%ld allocations not released", d.live);
    *allocs += d.allocs;
    return 0;
}

int main(int argc, char** argv)
{
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 20241019ull);
    long allocs = 0, forgets = 0, failures = 0;
    for (int group = 0; group < 2; ++group) {
        if (run_case(rng, 60, 60000, -1, group != 0, &allocs, &forgets, &failures)) return 1;       // forgets by hand only, small pushes
        if (run_case(rng, 40, 400000, -1, group != 0, &allocs, &forgets, &failures)) return 1;      // ... pushes that seal
        if (run_case(rng, 40, 400000, 0, group != 0, &allocs, &forgets, &failures)) return 1;       // a window that keeps nothing sealed
        if (run_case(rng, 40, 400000, 1, group != 0, &allocs, &forgets, &failures)) return 1;       // one block
        if (run_case(rng, 40, 500000, 3, group != 0, &allocs, &forgets, &failures)) return 1;       // three, with forgets by hand below that
    }
    if (forgets < 20 || failures < 20) { printf("too little happened: %ld forgets, %ld failed allocations\n", forgets, failures); return 1; }
    printf("stream_window ok: %ld allocations, %ld forgets, %ld failed allocations\n", allocs, forgets, failures);
    return 0;
}
