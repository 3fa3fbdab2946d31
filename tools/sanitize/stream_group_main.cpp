// The host planning of the group calls of sd_stream (csrc/many_plan.h: seg_tile_chunks, PackRange; csrc/stream_book.h: pack_range, pack_plan,
// book_reserve_group, book_seal_planned, book_seal_trim) against malloc'd memory, for AddressSanitizer + UBSan.  CPU only; tools/sanitize/build_stream_group.sh builds it.
//   stream_group plan <file>   every line of <file> is a case "cb pending S  n_0 sealed_0 ... n_{S-1} sealed_{S-1}"; prints per case
//                              "case <total> <ranges>" and per range "r <stream> <lo> <hi> <n_eq> <full> <last_len> <tile> <base> <slot>":
//                              tests/test_stream_group_cpu.py compares them with its own statement of the rules
//   stream_group tile <file>   every line of <file> is a case "lo full cb pending"; prints seg_tile_chunks of it, one line per case
//   stream_group run [seed]    groups of streams through random rounds of pushes, what stream.hip does around the books with the device work done by
//                              host loops that touch exactly the floats the table rows name -> "stream_group ok: ..." and exit 0, or the first mismatch
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
    int copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }
    int move_tail(float* dst, const float* src, int64_t len) {
        memcpy(dst, src, (size_t)len * sizeof(float));
        for (int q = 0; q < SD_TAIL_PAD; ++q) dst[len + q] = 0.0f;
        return 0;
    }
};

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

static float sample_of(int64_t stream, int64_t i) { return (float)((i + 977 * stream) % 65521) - 32760.0f; }
static float row_of(int64_t stream, int64_t chunk, int64_t n_at) { return (float)(stream * 100000 + chunk * 7 + n_at % 1000); }

static int plan_file(const char* path)
{
    FILE* f = fopen(path, "r");
    CHECK(f, "cannot open %s", path);
    long long cb, pending, S;
    while (fscanf(f, "%lld %lld %lld", &cb, &pending, &S) == 3) {
        std::vector<PackRange> ranges;
        for (long long i = 0; i < S; ++i) {
            long long n, sealed;
            CHECK(fscanf(f, "%lld %lld", &n, &sealed) == 2, "short case");
            PackRange r;
            if (!pack_range(n, sealed, cb, pending != 0, r)) continue;
            r.owner = i;
            ranges.push_back(r);
        }
        int64_t total = 0;
        CHECK(pack_plan(ranges.data(), (int64_t)ranges.size(), &total) == 0, "pack_plan refused a case");
        printf("case %lld %zu\n", (long long)total, ranges.size());
        for (const PackRange& r : ranges)
            printf("r %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (long long)r.owner, (long long)r.lo, (long long)r.hi(), (long long)r.n, (long long)r.full,
                   (long long)r.last_len, (long long)r.tile, (long long)r.base, (long long)r.slot());
    }
    fclose(f);
    return 0;
}

static int tile_file(const char* path)
{
    FILE* f = fopen(path, "r");
    CHECK(f, "cannot open %s", path);
    long long lo, full, cb, pending;
    while (fscanf(f, "%lld %lld %lld %lld", &lo, &full, &cb, &pending) == 4) printf("%lld\n", (long long)seg_tile_chunks(lo, full, cb, pending != 0));
    fclose(f);
    return 0;
}

// one group of S streams through `rounds` rounds of sd_stream_push_many and, now and then, sd_stream_turns_many
static int run_case(std::mt19937_64& rng, int S, int rounds, int64_t max_push, int64_t cb, long* allocs)
{
    HostDev dev;
    std::vector<StreamBook> b((size_t)S);
    std::vector<std::vector<int64_t>> row_n((size_t)S);      // per stream and chunk: the n its cache row was computed at

    // the packed inference of these ranges: reads what the pack kernel reads of the tails, writes what the scatter kernel writes of the caches
    auto infer = [&](std::vector<PackRange>& ranges, bool pending) -> int {
        int64_t total = 0;
        CHECK(pack_plan(ranges.data(), (int64_t)ranges.size(), &total) == 0, "pack_plan refused");
        int64_t next = 0;
        for (const PackRange& r : ranges) {
            StreamBook& k = b[(size_t)r.owner];
            CHECK(r.base == next && r.base % 32 == 0 && r.slot() == ((r.hi() - r.lo + SD_MANY_GAP + 31) / 32) * 32, "slot of stream %lld", (long long)r.owner);
            next = r.base + r.slot();
            CHECK(r.lo == k.sealed && r.lo % 32 == 0 && r.n <= k.tail_len() && r.n <= r.slot() * SD_HOP, "range of stream %lld", (long long)r.owner);
            CHECK((r.hi() - r.lo - 1) * SD_HOP + r.last_len <= r.n && r.tile >= 0 && r.tile <= r.full && r.full <= r.hi() - r.lo, "chunks of stream %lld", (long long)r.owner);
            double sum = 0;
            for (int64_t i = 0; i < r.n; ++i) {
                CHECK(k.tail_now()[i] == sample_of(r.owner, r.lo * SD_HOP + i), "sample %lld of the range of stream %lld", (long long)i, (long long)r.owner);
                sum += k.tail_now()[i];
            }
            (void)sum;
            const int64_t cnt = r.hi() - r.lo, room_seg = (k.cache_cap - r.lo) * SD_SEG_ROW, room_emb = (k.cache_cap - r.lo) * SD_EMB_ROW;
            CHECK(cnt * SD_SEG_ROW <= room_seg && cnt * SD_EMB_ROW <= room_emb, "cache room of stream %lld", (long long)r.owner);
            if ((int64_t)row_n[(size_t)r.owner].size() < r.hi()) row_n[(size_t)r.owner].resize((size_t)r.hi(), -1);
            for (int64_t c = r.lo; c < r.hi(); ++c) {
                for (int64_t q = 0; q < SD_SEG_ROW; ++q) k.seg[c * SD_SEG_ROW + q] = row_of(r.owner, c, k.n);
                for (int64_t q = 0; q < SD_EMB_ROW; ++q) k.emb[c * SD_EMB_ROW + q] = -row_of(r.owner, c, k.n);
                row_n[(size_t)r.owner][(size_t)c] = k.n;
            }
        }
        CHECK(next == total, "total of the pack");
        for (const PackRange& r : ranges) {
            StreamBook& k = b[(size_t)r.owner];
            if (pending) { k.pending_n = k.n; continue; }
            GroupRow mv;
            const long before = dev.allocs;
            CHECK(book_seal_planned(k, r.hi(), mv), "nothing to seal in stream %lld", (long long)r.owner);
            CHECK(mv.len + SD_TAIL_PAD <= mv.room, "compaction target of stream %lld: %lld floats for %lld", (long long)r.owner, (long long)mv.room, (long long)mv.len);
            memcpy(mv.dst, mv.src, (size_t)mv.len * sizeof(float));
            for (int q = 0; q < SD_TAIL_PAD; ++q) mv.dst[mv.len + q] = 0.0f;
            book_seal_trim(dev, k);
            CHECK(dev.allocs == before, "an allocation between the kernels");
        }
        return 0;
    };

    for (int round = 0; round < rounds; ++round) {
        // sd_stream_push_many: plan, growth, append, packed inference of what became sealed, compactions
        std::vector<int64_t> m((size_t)S);
        std::vector<PackRange> ranges;
        for (int i = 0; i < S; ++i) {
            int64_t v = 1 + (int64_t)(rng() % (uint64_t)max_push);
            const uint64_t how = rng() % 8;
            if (how == 0) v = 0;
            if (how == 1) v = 1;
            if (how == 2) {      // to an edge of the sealing rule: one sample short of the next block, or exactly at it
                const int64_t edge = (stream_sealed_chunks(b[(size_t)i].n) + SD_SEAL_CHUNKS - 1) * SD_HOP + SD_CHUNK + (int64_t)(rng() % 2);
                v = edge > b[(size_t)i].n ? edge - b[(size_t)i].n : 0;
            }
            if (how == 3) v = 2 * SD_SEAL_CHUNKS * SD_HOP + 5;      // two blocks at once
            m[(size_t)i] = v;
            PackRange r;
            if (pack_range(b[(size_t)i].n + v, b[(size_t)i].sealed, cb, false, r)) { r.owner = i; ranges.push_back(r); }
        }
        std::vector<char> busy((size_t)S, 0);
        for (const PackRange& r : ranges) busy[(size_t)r.owner] = 1;
        for (int i = 0; i < S; ++i)      // a stream with nothing to do in the call is not touched
            if (m[(size_t)i] > 0 || busy[(size_t)i]) CHECK(book_reserve_group(dev, b[(size_t)i], m[(size_t)i]) == 0, "reserve failed");
        const long before = dev.allocs;
        for (int i = 0; i < S; ++i) {
            StreamBook& k = b[(size_t)i];
            if (m[(size_t)i] == 0) continue;
            float* dst = k.tail_now() + k.tail_len();
            CHECK(m[(size_t)i] + SD_TAIL_PAD <= k.tail_cap[k.cur] - k.tail_len(), "tail room of stream %d", i);
            for (int64_t j = 0; j < m[(size_t)i]; ++j) dst[j] = sample_of(i, k.n + j);
            for (int q = 0; q < SD_TAIL_PAD; ++q) dst[m[(size_t)i] + q] = 0.0f;
            k.n += m[(size_t)i];
        }
        if (infer(ranges, false)) return 1;
        CHECK(dev.allocs == before, "an allocation behind the first kernel of a push");
        // sd_stream_turns_many, two rounds out of three
        if (rng() % 3) {
            std::vector<PackRange> pend;
            for (int i = 0; i < S; ++i) {
                PackRange r;
                if (b[(size_t)i].pending_n != b[(size_t)i].n && pack_range(b[(size_t)i].n, b[(size_t)i].sealed, cb, true, r)) { r.owner = i; pend.push_back(r); }
            }
            for (const PackRange& r : pend) CHECK(book_reserve_group(dev, b[(size_t)r.owner], 0) == 0, "reserve failed");
            const long at = dev.allocs;
            if (infer(pend, true)) return 1;
            CHECK(dev.allocs == at, "an allocation behind the first kernel of a turns call");
        }
        // every stream: the book, the tail and the rows are what the single-stream calls leave
        for (int i = 0; i < S; ++i) {
            const StreamBook& k = b[(size_t)i];
            const int64_t total = sd_chunk_rule(k.n, nullptr);
            CHECK(k.sealed == stream_sealed_chunks(k.n) && k.tail_len() == k.n - k.sealed * SD_HOP, "book of stream %d at n = %lld", i, (long long)k.n);
            if (!k.tail_now()) { CHECK(k.n == 0, "no tail at n = %lld", (long long)k.n); continue; }
            CHECK(k.tail_cap[k.cur] >= k.tail_len() + SD_TAIL_PAD, "tail capacity of stream %d", i);
            for (int64_t j = 0; j < k.tail_len(); ++j) CHECK(k.tail_now()[j] == sample_of(i, k.sealed * SD_HOP + j), "tail sample %lld of stream %d", (long long)j, i);
            for (int q = 0; q < SD_TAIL_PAD; ++q) CHECK(k.tail_now()[k.tail_len() + q] == 0.0f, "padding float %d of stream %d", q, i);
            const int64_t upto = k.pending_n == k.n ? total : k.sealed;
            for (int64_t c = 0; c < upto; ++c) {
                const float want = row_of(i, c, row_n[(size_t)i][(size_t)c]);
                CHECK(k.seg[c * SD_SEG_ROW] == want && k.seg[(c + 1) * SD_SEG_ROW - 1] == want && k.emb[c * SD_EMB_ROW] == -want && k.emb[(c + 1) * SD_EMB_ROW - 1] == -want,
                      "cache row %lld of stream %d", (long long)c, i);
                if (c < k.sealed) CHECK(stream_sealed_chunks(row_n[(size_t)i][(size_t)c]) > c, "row %lld of stream %d was written before it sealed", (long long)c, i);
            }
        }
    }
    for (int i = 0; i < S; ++i) book_release(dev, b[(size_t)i]);
    CHECK(dev.live == 0, "%ld allocations not released", dev.live);
    *allocs += dev.allocs;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 2 && !strcmp(argv[1], "plan")) return plan_file(argv[2]);
    if (argc > 2 && !strcmp(argv[1], "tile")) return tile_file(argv[2]);
    std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 20240911ull);
    long allocs = 0;
    if (run_case(rng, 5, 60, 40000, 4096, &allocs)) return 1;           // small pushes: steady state
    if (run_case(rng, 9, 12, 500000, 4096, &allocs)) return 1;          // pushes that seal, several blocks at once among them
    if (run_case(rng, 3, 12, 300000, 7, &allocs)) return 1;             // batches on the skinny side
    if (run_case(rng, 3, 12, 300000, 33, &allocs)) return 1;            // ... and batches that cut blocks
    printf("stream_group ok: %ld allocations\n", allocs);
    return 0;
}
