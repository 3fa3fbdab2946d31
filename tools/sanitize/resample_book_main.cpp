// The host bookkeeping of a stream with an input rate (csrc/resample_book.h) against malloc'd memory, for AddressSanitizer + UBSan: the rule F(n),
// the inputs a stream keeps from push to push, the rows it hands to k_resample_jobs.  The kernel is restated on the host, float only: per tile of 256
// outputs counted from the row's first output the input span is staged exactly as the device body stages it (so a window that is shorter than the
// row says is a heap overflow report), then the taps run over it with fmaf on two accumulators in the body's order.  Buffers are of exactly the size
// asked for.  CPU only; tools/sanitize/build_resample_book.sh builds it.
//   resample_book [seed]   -> "resample_book ok: ..." and exit 0, or the first mismatch and exit 1
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "resample_book.h"

#define PAD 512      // SD_TAIL_PAD: the zeros a row writes behind its last output

struct HostDev {
    long allocs = 0, live = 0, fail_at = -1;      // fail_at: the allocation (counted from 1) that fails, -1: none
    int alloc(void** p, size_t bytes) {
        if (++allocs == fail_at) { *p = nullptr; return SD_ERR_HIP; }
        *p = malloc(bytes ? bytes : 1); ++live;
        return *p ? 0 : SD_ERR_HIP;
    }
    void release(void* p) { free(p); --live; }
    int copy(void* dst, const void* src, size_t bytes) { memcpy(dst, src, bytes); return 0; }      // (memcpy: ASan reports overlapping ranges)
};

#define CHECK(cond, ...) do { if (!(cond)) { printf(__VA_ARGS__); printf("\n"); return 1; } } while (0)

// k_resample_jobs on one row: tiles from the row's first output, the staging and the fmaf chain of resample_point, the pad zeros of the last tile.
// Every read that is summed must lie in the window or outside [0, n_limit): *short_by = how far the window falls short of that (0: never)
static void run_row(const ResampleJob& j, int64_t* short_by)
{
    const int64_t span = ((int64_t)(RS_BLOCK - 1) * j.M) / j.L + 2 * (int64_t)j.J + 3;
    std::vector<float> xs((size_t)span);
    for (int64_t off = 0; off < j.count; off += RS_BLOCK) {
        const int64_t m0 = j.m_first + off, base = (m0 * j.M) / j.L - j.J - 1;
        for (int64_t i = 0; i < span; ++i) {
            const int64_t g = base + i;
            xs[(size_t)i] = (g >= j.first && g < j.n_limit) ? j.src[g - j.first] : 0.0f;
        }
        for (int64_t t = 0; t < RS_BLOCK && off + t < j.count; ++t) {
            const int64_t m = m0 + t, tt = m * j.M, i0 = tt / j.L;
            const int ph = (int)(tt - i0 * j.L);
            const int64_t lowest = i0 - j.J > 0 ? i0 - j.J : 0;      // the first input this output sums that is not silence in front of the recording
            if (lowest < j.n_limit && lowest < j.first && j.first - lowest > *short_by) *short_by = j.first - lowest;
            const float* xp = xs.data() + (i0 - base);
            const float* tp = j.taps + ph;
            float acc0 = 0.0f, acc1 = 0.0f;
            int q = -j.J;
            for (; q + 1 <= j.J; q += 2) {
                acc0 = fmaf(tp[(size_t)(q + j.J) * j.L], xp[-q], acc0);
                acc1 = fmaf(tp[(size_t)(q + j.J + 1) * j.L], xp[-q - 1], acc1);
            }
            if (q <= j.J) acc0 = fmaf(tp[(size_t)(q + j.J) * j.L], xp[-q], acc0);
            j.dst[off + t] = acc0 + acc1;
        }
    }
    for (int64_t i = j.count; i < j.count + j.pad; ++i) j.dst[i] = 0.0f;
}

struct Snapshot {
    RateBook r; std::vector<float> held;
    explicit Snapshot(const RateBook& b) : r(b), held(b.buf[b.cur] ? b.buf[b.cur] : nullptr, b.buf[b.cur] ? b.buf[b.cur] + b.held() : nullptr) {}
    bool same(const RateBook& b) const {
        return r.in_sr == b.in_sr && r.n_in == b.n_in && r.emitted == b.emitted && r.closed == b.closed && r.cur == b.cur && r.first == b.first &&
               r.buf[r.cur] == b.buf[b.cur] && r.cap[r.cur] == b.cap[b.cur] && (held.empty() || memcmp(held.data(), b.buf[b.cur], held.size() * sizeof(float)) == 0);
    }
};

// one stream at in_sr fed x in the given pieces, against the one-shot result of the same body; fail_at as in HostDev.  *allocs = allocations made
static int run_case(int32_t in_sr, const std::vector<float>& x, const std::vector<int64_t>& pieces, const std::vector<float>& taps, long fail_at, long* allocs, bool* failed)
{
    HostDev dev;
    dev.fail_at = fail_at;
    RateBook r;
    CHECK(make_plan(in_sr, SD_SAMPLE_RATE, r.p) == 0, "plan of %d", in_sr);
    r.in_sr = in_sr;
    const int64_t N = (int64_t)x.size(), len = resample_len(N, in_sr, SD_SAMPLE_RATE);
    int64_t short_by = 0;
    // the whole recording at once
    std::vector<float> want((size_t)len + PAD);
    { const ResampleJob all{x.data(), 0, N, want.data(), 0, len, taps.data(), (int32_t)r.p.L, (int32_t)r.p.M, r.p.J, PAD}; run_row(all, &short_by); }
    std::vector<float> got;
    auto emit = [&](const RatePush& q) -> int {      // the row into a buffer of exactly count + pad floats, then behind what was emitted
        float* dst = (float*)malloc((size_t)(q.count + PAD) * sizeof(float));
        const ResampleJob j = rate_job(r, q, dst, taps.data(), PAD);
        run_row(j, &short_by);
        got.insert(got.end(), dst, dst + q.count);
        free(dst);
        return 0;
    };
    int64_t at = 0;
    for (int64_t m : pieces) {
        const RatePush q = rate_plan_push(r, m);
        CHECK(q.n_after == at + m && q.f_after == resample_final_len(q.n_after, in_sr, SD_SAMPLE_RATE, r.p) && q.count >= 0, "plan of a push at n = %lld", (long long)at);
        const Snapshot before(r);
        int rc = rate_reserve(dev, r, m);
        if (rc) {      // the failing allocation: the book is what it was, and the same call goes through afterwards
            *failed = true;
            CHECK(before.same(r), "a failed allocation changed the book at n = %lld", (long long)at);
            rc = rate_reserve(dev, r, m);
        }
        CHECK(rc == 0, "reserve failed twice");
        CHECK(r.n_in == at && r.held() + m + RS_HIST_SLACK <= r.cap[r.cur] && r.first <= r.need_first(r.emitted), "room at n = %lld", (long long)at);
        float* in = r.buf[r.cur] + r.held();
        for (int64_t i = 0; i < m; ++i) in[i] = x[(size_t)(at + i)];
        for (int q2 = 0; q2 < RS_HIST_SLACK; ++q2) in[m + q2] = 0.0f;      // what k_pcm_to_f32 writes behind the samples it converts
        if (q.count > 0 && emit(q)) return 1;
        rate_commit(r, q);
        at += m;
        CHECK(r.emitted == (int64_t)got.size() && r.emitted <= resample_len(at, in_sr, SD_SAMPLE_RATE), "emitted at n = %lld", (long long)at);
        // the definition of F: every emitted output's last read lies in front of n, the next one's does not (or there is none)
        if (r.emitted > 0) CHECK(((r.emitted - 1) * r.p.M) / r.p.L + r.p.J <= at - 1, "output %lld is not final at n = %lld", (long long)r.emitted - 1, (long long)at);
        if (r.emitted < resample_len(at, in_sr, SD_SAMPLE_RATE)) CHECK((r.emitted * r.p.M) / r.p.L + r.p.J > at - 1, "output %lld is final at n = %lld", (long long)r.emitted, (long long)at);
        CHECK(got.empty() || memcmp(got.data(), want.data(), got.size() * sizeof(float)) == 0, "outputs differ from the one-shot result at n = %lld", (long long)at);
    }
    CHECK(at == N, "pieces do not add up");
    const RatePush q = rate_plan_flush(r);
    CHECK(q.f_after == len, "flush plan");
    if (q.count > 0 && emit(q)) return 1;
    rate_commit(r, q);
    r.closed = true;
    CHECK((int64_t)got.size() == len && memcmp(got.data(), want.data(), (size_t)len * sizeof(float)) == 0, "outputs differ from the one-shot result after the flush");
    CHECK(short_by == 0, "the inputs held fall %lld short of what an output reads", (long long)short_by);
    rate_release(dev, r);
    CHECK(dev.live == 0 && r.held() == 0, "%ld allocations not released", dev.live);
    *allocs = dev.allocs;
    return 0;
}

int main(int argc, char** argv)
{
    std::mt19937_64 rng(argc > 1 ? strtoull(argv[1], nullptr, 10) : 20240611ull);
    const int32_t rates[] = {8000, 11025, 22050, 32000, 44100, 48000, 12345};
    long total_allocs = 0, cases = 0, failures = 0;
    for (int32_t sr : rates) {
        ResamplePlan p;
        if (make_plan(sr, SD_SAMPLE_RATE, p)) return 1;
        // F against its definition by counting, and monotone
        int64_t prev = 0;
        for (int64_t n = 0; n < 1500; ++n) {
            const int64_t len = resample_len(n, sr, SD_SAMPLE_RATE);
            int64_t m = 0;
            while (m < len && (m * p.M) / p.L + p.J <= n - 1) ++m;
            const int64_t f = resample_final_len(n, sr, SD_SAMPLE_RATE, p);
            if (f != m || f < prev) { printf("F(%lld) at %d Hz: %lld, counted %lld\n", (long long)n, sr, (long long)f, (long long)m); return 1; }
            prev = f;
        }
        // every tap non-zero: the rule goes by the reads, not by which taps happen to be zero
        std::vector<float> taps((size_t)((2 * p.J + 1) * p.L));
        for (float& t : taps) t = (float)((int64_t)(rng() % 2001) - 1000) / 1024.0f + 0.0004f;
        const int64_t N = 2200 + (int64_t)(rng() % 900);
        std::vector<float> x((size_t)N);
        for (float& v : x) v = (float)((int64_t)(rng() % 65536) - 32768) / 32768.0f;
        std::vector<std::vector<int64_t>> schedules;
        schedules.push_back({N});
        { std::vector<int64_t> s; int64_t n = 0; while (n < N) { int64_t m = 1 + (int64_t)(rng() % 700); if (n + m > N) m = N - n; s.push_back(m); n += m; } schedules.push_back(s); }
        { std::vector<int64_t> s; int64_t n = 0; for (; n < 2 * p.J + 5 && n < N; ++n) s.push_back(1); while (n < N) { int64_t m = 1 + (int64_t)(rng() % 3); if (n + m > N) m = N - n; s.push_back(m); n += m; } schedules.push_back(s); }
        for (const auto& s : schedules) {
            long allocs = 0;
            bool failed = false;
            if (run_case(sr, x, s, taps, -1, &allocs, &failed)) { printf("  (%d Hz, %zu pieces)\n", sr, s.size()); return 1; }
            total_allocs += allocs; ++cases;
            for (long k = 1; k <= allocs; ++k) {      // every allocation fails in turn
                long a2 = 0;
                failed = false;
                if (run_case(sr, x, s, taps, k, &a2, &failed)) { printf("  (%d Hz, %zu pieces, allocation %ld fails)\n", sr, s.size(), k); return 1; }
                if (!failed) { printf("allocation %ld of %ld never failed at %d Hz\n", k, allocs, sr); return 1; }
                ++failures;
            }
        }
    }
    printf("resample_book ok: %ld cases, %ld allocations, %ld failed allocations survived\n", cases, total_allocs, failures);
    return 0;
}
