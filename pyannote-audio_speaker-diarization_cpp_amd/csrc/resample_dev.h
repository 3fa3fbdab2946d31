// resample_dev.h -- the one device body of the resampler (resample.hip says what it computes): k_resample and k_resample_jobs (resample.hip) and the
// off-rate tiles of k_many_ingest (ingest.hip) run this text.  What differs between them is how an input sample is fetched while the tile's span is
// staged in LDS, and that is the body's Load parameter: a functor whose operator()(i) gives input sample first + i of the row.  The tap loop -- the FMA
// order, the two accumulators, the last add -- exists here only.
#pragma once
#include "resample_book.h"      // RS_BLOCK

// the staging load of k_resample / k_resample_jobs: mono floats
struct RsLoadF32 {
    const float* __restrict__ src;
    __device__ __forceinline__ float operator()(int64_t i) const { return src[i]; }
};

// The 256 outputs from m0 on, thread per output, of which those in front of m_end exist.  The tile's input span [base, base + span) is staged in LDS
// (coalesced; load(0) is input `first`, inputs outside [first, n_limit) read as zero), then the taps of the output's phase run over it in a fixed order
// on two accumulators, and the sum goes to out[threadIdx.x]: the tile's place in the recording for k_resample, LDS for k_resample_jobs and
// k_many_ingest.  A thread without an output stores nothing.
template <class Load>
__device__ __forceinline__ void resample_point(float* xs, const Load load, int64_t first, int64_t n_limit, int64_t m0, int64_t m_end,
                                               const float* __restrict__ taps /*[2J+1][L]*/, int L, int M, int J, int span, float* __restrict__ out)
{
    const int64_t base = (m0 * M) / L - J - 1;
    for (int i = threadIdx.x; i < span; i += RS_BLOCK) {
        const int64_t g = base + i;
        xs[i] = (g >= first && g < n_limit) ? load(g - first) : 0.0f;
    }
    __syncthreads();
    const int64_t m = m0 + threadIdx.x;
    if (m >= m_end) return;
    const int64_t t = m * M;
    const int64_t i0 = t / L;
    const int ph = (int)(t - i0 * L);
    const float* xp = xs + (i0 - base);                                 // xp[-j] = x[i0 - j]
    const float* tp = taps + ph;
    float acc0 = 0.0f, acc1 = 0.0f;
    int j = -J;
    for (; j + 1 <= J; j += 2) {
        acc0 = fmaf(tp[(size_t)(j + J) * L], xp[-j], acc0);
        acc1 = fmaf(tp[(size_t)(j + J + 1) * L], xp[-j - 1], acc1);
    }
    if (j <= J) acc0 = fmaf(tp[(size_t)(j + J) * L], xp[-j], acc0);
    out[threadIdx.x] = acc0 + acc1;
}
