// The host bookkeeping of sd_stream (csrc/stream_book.h) against malloc'd memory, for AddressSanitizer + UBSan: growth of the two caches,
// the offsets of the tail through appends and compactions, the sealing arithmetic.  The device operations are stubs of exactly the size
// asked for, so an offset that is off by one float is a heap overflow report.  CPU only; tools/sanitize/build_stream_book.sh builds it.
//   stream_book [seed]   -> "stream_book ok: ..." and exit 0, or the first mismatch and exit 1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "stream_book.h"

struct HostDev {
    long allocs = 0, live = 0;
    int alloc(void** p, size_t bytes) { *p = malloc(bytes ? bytes : 1); ++allocs; ++live; return *p ? 0 : SD_ERR_HIP; }
    void release(void* p) { free(p); --live; }
    int copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }      // (memcpy: ASan reports overlapping ranges)
    int move_tail(float* dst, const float* src, int64_t len) {
        memcpy(dst, src, (size_t)len * sizeof(float));
        for (int q = 0; q < SD_TAIL_PAD; ++q) dst[len + q] = 0.0f;
        return 0;
    }
};

static int64_t total_chunks(int64_t n) { return n >= 2 ? stream_full_chunks(n) + 1 : 0; }      // sd_num_chunks (sd.cpp:1419, 1457): the full chunks and the last one
static float sample_of(int64_t i) { return (float)(i % 65521) - 32760.0f; }        // sample i of the recording
static float seg_of(int64_t chunk, int64_t n_at) { return (float)(chunk * 7 + n_at % 1000); }

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// what stream.hip does around the book, with the inference replaced by rows that name their chunk and the n they were computed at
static int run_case(std::mt19937_64& rng, int pushes, int64_t max_push, long* allocs)
{
    HostDev dev;
    StreamBook b;
    std::vector<int64_t> row_n;                       // per chunk: the n its cache row was computed at
    auto infer = [&](int64_t lo, int64_t hi) {
        // the networks read samples [lo * 8000, min(n, (hi - 1) * 8000 + 80000)) of the tail: touch them all
        int64_t s1 = (hi - 1) * SD_HOP + SD_CHUNK; if (s1 > b.n) s1 = b.n;
        double sum = 0;
        for (int64_t i = lo * SD_HOP; i < s1 + 4; ++i) sum += b.tail_now()[i - b.sealed * SD_HOP];      // + 4: the shared conv0 reads into the padding
        (void)sum;
        if ((int64_t)row_n.size() < hi) row_n.resize((size_t)hi, -1);
        for (int64_t k = lo; k < hi; ++k) {
            for (int64_t q = 0; q < SD_SEG_ROW; ++q) b.seg[k * SD_SEG_ROW + q] = seg_of(k, b.n);
            for (int64_t q = 0; q < SD_EMB_ROW; ++q) b.emb[k * SD_EMB_ROW + q] = -seg_of(k, b.n);
            row_n[(size_t)k] = b.n;
        }
    };
    for (int p = 0; p < pushes; ++p) {
        int64_t m = 1 + (int64_t)(rng() % (uint64_t)max_push);
        if (p % 7 == 3) m = 1;
        if (p % 11 == 5) m = SD_HOP * SD_SEAL_CHUNKS;
        CHECK(book_reserve_tail(dev, b, m) == 0, "reserve_tail failed");
        float* dst = b.tail_now() + b.tail_len();
        for (int64_t i = 0; i < m; ++i) dst[i] = sample_of(b.n + i);
        for (int q = 0; q < SD_TAIL_PAD; ++q) dst[m + q] = 0.0f;
        b.n += m;
        const int64_t to = stream_sealed_chunks(b.n), total = total_chunks(b.n);
        CHECK(to % SD_SEAL_CHUNKS == 0 && to <= total && (to == 0 || (to - 1) * SD_HOP + SD_CHUNK < b.n), "sealed(%lld) = %lld", (long long)b.n, (long long)to);
        CHECK(total - to <= SD_SEAL_CHUNKS, "more than 32 pending chunks at n = %lld", (long long)b.n);
        if (to > b.sealed) {
            CHECK(book_reserve_cache(dev, b, total) == 0, "reserve_cache failed");
            infer(b.sealed, to);
            CHECK(book_seal(dev, b, to) == 0, "seal failed");
        }
        CHECK(b.sealed == to && b.tail_len() == b.n - to * SD_HOP && b.tail_cap[b.cur] >= b.tail_len() + SD_TAIL_PAD, "tail offsets at n = %lld", (long long)b.n);
        if (rng() % 3 == 0 && total > 0 && b.pending_n != b.n) {      // sd_stream_turns
            CHECK(book_reserve_cache(dev, b, total) == 0, "reserve_cache failed");
            infer(b.sealed, total);
            b.pending_n = b.n;
        }
        // the tail is the recording from sample sealed * 8000 on, with zeros behind it
        const float* t = b.tail_now();
        for (int64_t i = 0; i < b.tail_len(); ++i) CHECK(t[i] == sample_of(b.sealed * SD_HOP + i), "tail sample %lld at n = %lld", (long long)i, (long long)b.n);
        for (int q = 0; q < SD_TAIL_PAD; ++q) CHECK(t[b.tail_len() + q] == 0.0f, "padding float %d at n = %lld", q, (long long)b.n);
        // sealed rows are those computed when they sealed, through every growth of the cache; pending rows those of the last turns
        const int64_t upto = b.pending_n == b.n ? total : b.sealed;
        for (int64_t k = 0; k < upto; ++k) {
            const float want = seg_of(k, row_n[(size_t)k]);
            CHECK(b.seg[k * SD_SEG_ROW] == want && b.seg[(k + 1) * SD_SEG_ROW - 1] == want && b.emb[k * SD_EMB_ROW] == -want && b.emb[(k + 1) * SD_EMB_ROW - 1] == -want,
                  "cache row %lld at n = %lld", (long long)k, (long long)b.n);
            if (k < b.sealed) CHECK(stream_sealed_chunks(row_n[(size_t)k]) > k, "row %lld was written before it sealed", (long long)k);
        }
    }
    book_release(dev, b);
    CHECK(dev.live == 0, "%ld allocations not released", dev.live);
    *allocs += dev.allocs;
    return 0;
}

int main(int argc, char** argv)
{
    // the sealing rule against its definition, around every edge of the first blocks and at the top of the range
    for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)80000, (int64_t)80001, (int64_t)327999, (int64_t)328000, (int64_t)328001, (int64_t)583999, (int64_t)584000,
                      (int64_t)584001, (int64_t)2147483647, (int64_t)1 << 40, (int64_t)0x7fffffffffffffffLL}) {
        int64_t full = 0;
        if (n > SD_CHUNK) { full = (n - SD_CHUNK) / SD_HOP; if ((n - SD_CHUNK) % SD_HOP) ++full; }
        if (stream_full_chunks(n) != full || stream_sealed_chunks(n) != 32 * (full / 32)) { printf("sealing rule at n = %lld\n", (long long)n); return 1; }
    }
    if (stream_sealed_chunks(328000) != 0 || stream_sealed_chunks(328001) != 32 || stream_sealed_chunks(584001) != 64) { printf("sealing rule at the block edges\n"); return 1; }
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 20240607ull);
    long allocs = 0;
    if (run_case(rng, 400, 12000, &allocs)) return 1;            // many small pushes: steady state
    if (run_case(rng, 40, 700000, &allocs)) return 1;            // pushes that seal several blocks at once
    if (run_case(rng, 3, 6000000, &allocs)) return 1;            // minutes at a time
    printf("stream_book ok: %ld allocations\n", allocs);
    return 0;
}
