// resample_book.h -- host bookkeeping of a stream that takes its samples at another rate than 16 kHz (stream.hip: sd_stream_set_input_rate): the plan
// of a rate pair and the two length rules (resample.hip uses them too), the inputs a stream has to keep, and what one push and the closing flush
// ask of k_resample_jobs (resample.hip).  No HIP in here: every device operation goes through the Dev parameter (alloc / release / copy, as in
// stream_book.h), so the same code runs against malloc'd memory under AddressSanitizer in tools/sanitize/resample_book_main.cpp.
//
// Output m of the resampler reads the inputs x[i0 - J .. i0 + J], i0 = floor(m M / L), zero in front of sample 0 and behind the last one.  With n inputs
// pushed, output m is FINAL when all of those lie in front of n -- no later input can change it -- and it belongs to the output of every longer input:
//     F(n) = min(len(n), #{m >= 0 : floor(m M / L) + J <= n - 1}) = min(len(n), n - 1 - J < 0 ? 0 : ((n - J) L - 1) / M + 1)
// len(n) is the reference's float length rule (resampler.cc:21-22).  Both are non-decreasing in n.  The rule goes by the kernel's reads, not by which taps
// happen to be zero.  A stream has emitted outputs [0, emitted), emitted = F(n_in) until the input is closed and len(n_in) afterwards.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "../../include/sdhip.h"

#define RS_ZEROS 64
#define RS_CUTOFF 0.95
#define RS_BETA 10.056
#define RS_BLOCK 256
#define RS_HIST_SLACK 512      // floats of room behind the inputs held: k_pcm_to_f32 zeroes SD_WAV_PAD floats behind what it converts (stream.hip asserts the two agree)

struct ResamplePlan { int64_t L, M; int J; int64_t span; double half, fc; };

inline int64_t rs_gcd64(int64_t a, int64_t b) { while (b) { const int64_t t = a % b; a = b; b = t; } return a; }

inline int make_plan(int32_t in_sr, int32_t out_sr, ResamplePlan& p)
{
    if (in_sr <= 0 || out_sr <= 0) return 1;
    const int64_t g = rs_gcd64(in_sr, out_sr);
    p.L = out_sr / g; p.M = in_sr / g;
    const double fmax = (double)(p.L > p.M ? p.L : p.M);
    p.fc = RS_CUTOFF / (2.0 * fmax);
    p.half = (double)RS_ZEROS / (2.0 * p.fc);
    p.J = (int)std::floor(p.half / (double)p.L) + 1;
    p.span = ((RS_BLOCK - 1) * p.M) / p.L + 2 * (int64_t)p.J + 3;      // input samples a tile of RS_BLOCK outputs can touch, wherever the tile starts
    return 0;
}

// sd_resample_len
inline int64_t resample_len(int64_t n, int32_t in_sr, int32_t out_sr)
{
    if (n < 0 || in_sr <= 0 || out_sr <= 0) return -1;
    const float ratio = (float)(1.0 * out_sr / in_sr);                  // resampler.cc:21 (float ratio)
    return (int64_t)((float)(uint64_t)n * ratio);                       // resampler.cc:22: size_t * float -> float -> size_t
}

// F(n) above; -1 on bad arguments as resample_len
inline int64_t resample_final_len(int64_t n, int32_t in_sr, int32_t out_sr, const ResamplePlan& p)
{
    const int64_t len = resample_len(n, in_sr, out_sr);
    if (len < 0) return -1;
    if (n - 1 - p.J < 0) return 0;
    const __int128 by_reads = ((__int128)(n - p.J) * p.L - 1) / p.M + 1;
    return by_reads < (__int128)len ? (int64_t)by_reads : len;
}

// One row of k_resample_jobs' table: outputs [m_first, m_first + count) of the rate pair L / M into dst[0, count), `pad` zeros behind them.  src[0] is
// input sample `first`; reads at or behind input n_limit, and in front of input 0, are zero (the row's reads in front of `first` are never summed).
struct ResampleJob {
    const float* src; int64_t first, n_limit;
    float* dst; int64_t m_first, count;
    const float* taps;      // [2J+1][L]
    int32_t L, M, J, pad;
};

struct RateBook {
    int32_t in_sr = 0;             // 0: the stream has no resampler (none set, or 16 000)
    bool direct = false;           // a rate of 16 000 was set: no resampler, the samples are the inputs; sd_stream_end_input closes the input all the same
    ResamplePlan p{};
    int64_t n_in = 0;              // inputs pushed
    int64_t emitted = 0;           // outputs handed to the stream's tail
    bool closed = false;           // sd_stream_end_input
    float* buf[2] = {nullptr, nullptr};      // buf[cur] holds inputs [first, n_in) -- at least [need_first(emitted), n_in) -- and has RS_HIST_SLACK floats of room behind them
    int64_t cap[2] = {0, 0};       // floats
    int cur = 0;
    int64_t first = 0;
    int64_t held() const { return n_in - first; }
    // the first input that output m, and so every later one, reads
    int64_t need_first(int64_t m) const { const int64_t i = (int64_t)(((__int128)m * p.M) / p.L) - p.J; return i > 0 ? i : 0; }
};

// Room for `more` inputs behind those held.  Where the buffer is full, the inputs still needed -- about 2J of them; the float length rule lets emitted
// fall behind at very large n, so nothing assumes a bound -- move to the front of the other buffer (two allocations: a plain copy) and the two change
// places.  A failed allocation leaves the book as it was.
template <class Dev> int rate_reserve(Dev& d, RateBook& r, int64_t more)
{
    if (r.held() + more + RS_HIST_SLACK <= r.cap[r.cur]) return 0;
    int64_t from = r.need_first(r.emitted);
    if (from < r.first) from = r.first;
    if (from > r.n_in) from = r.n_in;
    const int64_t kept = r.n_in - from, need = kept + more + RS_HIST_SLACK;
    const int o = 1 - r.cur;
    if (r.cap[o] < need) {
        void* p = nullptr;
        if (int rc = d.alloc(&p, (size_t)(2 * need) * sizeof(float))) return rc;
        if (r.buf[o]) d.release(r.buf[o]);
        r.buf[o] = (float*)p; r.cap[o] = 2 * need;
    }
    if (kept > 0) if (int rc = d.copy(r.buf[o], r.buf[r.cur] + (from - r.first), (size_t)kept * sizeof(float))) return rc;
    r.cur = o; r.first = from;
    return 0;
}

// what a push of `more` inputs makes final: outputs [emitted, f_after)
struct RatePush { int64_t n_after, f_after, count; };
inline RatePush rate_plan_push(const RateBook& r, int64_t more)
{
    RatePush q;
    q.n_after = r.n_in + more;
    q.f_after = resample_final_len(q.n_after, r.in_sr, SD_SAMPLE_RATE, r.p);
    if (q.f_after < r.emitted) q.f_after = r.emitted;      // (F is non-decreasing: never taken)
    q.count = q.f_after - r.emitted;
    return q;
}
// ... and the closing flush: outputs [emitted, len(n_in)), silence behind the last input as for a whole recording
inline RatePush rate_plan_flush(const RateBook& r)
{
    RatePush q;
    q.n_after = r.n_in;
    q.f_after = resample_len(r.n_in, r.in_sr, SD_SAMPLE_RATE);
    if (q.f_after < r.emitted) q.f_after = r.emitted;
    q.count = q.f_after - r.emitted;
    return q;
}
// the row of either, once the new inputs have their place behind those held (rate_reserve): dst takes count outputs and `pad` zeros
inline ResampleJob rate_job(const RateBook& r, const RatePush& q, float* dst, const float* taps, int32_t pad)
{
    return ResampleJob{r.buf[r.cur], r.first, q.n_after, dst, r.emitted, q.count, taps, (int32_t)r.p.L, (int32_t)r.p.M, (int32_t)r.p.J, pad};
}
inline void rate_commit(RateBook& r, const RatePush& q) { r.n_in = q.n_after; r.emitted = q.f_after; }

template <class Dev> void rate_release(Dev& d, RateBook& r)
{
    for (int q = 0; q < 2; ++q) { if (r.buf[q]) d.release(r.buf[q]); r.buf[q] = nullptr; r.cap[q] = 0; }
    r.first = r.n_in;      // nothing is held
}
