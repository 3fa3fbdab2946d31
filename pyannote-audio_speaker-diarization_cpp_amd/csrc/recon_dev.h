// recon_dev.h -- the two per-element rules of a reconstruction (a15 / a16), stated once for reconstruct.hip (k_activations, k_topk: one job) and cut.hip
// (k_activations_cuts, k_topk_cuts: all cuts of a group).  A kernel decodes its index -- which cut, frame, cluster or row -- and calls these.
#pragma once
#include "common.h"
#include "exact_fp.h"
#include <cmath>

// the activation of cluster k in frame f: the sum over the chunks c covering f, ascending, of max_{s: hard[c][s] == k} seg[c][f - sfr[c]][s]; 0.0 if none
// (skip_average, missing = 0.0, sd.cpp:2651).  seg [chunks][293][3] raw f32 scores, hard [chunks][3], sfr [chunks] first frame of each chunk
__device__ __forceinline__ double activation_sum(const float* __restrict__ seg, const int* __restrict__ hard, const int* __restrict__ sfr, int64_t chunks,
                                                 int64_t f, int k)
{
    const double per_chunk = 0.5 / 0.016875;
    int64_t lo = (int64_t)((double)(f - (SD_FRAMES - 1)) / per_chunk) - 2; if (lo < 0) lo = 0;
    int64_t hi = (int64_t)((double)f / per_chunk) + 2; if (hi > chunks - 1) hi = chunks - 1;
    double sum = 0.0;
    for (int64_t c = lo; c <= hi; ++c) {
        const int64_t j = f - sfr[c];
        if (j < 0 || j >= SD_FRAMES) continue;
        const int* h = hard + c * SD_SPEAKERS;
        const float* s = seg + (c * SD_FRAMES + j) * SD_SPEAKERS;
        float mx = -INFINITY; bool any = false;
#pragma unroll
        for (int q = 0; q < SD_SPEAKERS; ++q)
            if (h[q] == k) { any = true; mx = (mx < s[q]) ? s[q] : mx; }      // std::max semantics, sd.cpp:2779
        if (any) sum += (double)mx;                                           // NaN entries are masked out, sd.cpp:1197-1201
    }
    return sum;
}

// b[k] = 1 for the `count` clusters (at most K, sd.cpp:2681) with the largest activation a[k], stable order on ties, 0 for the others (sd.cpp:2720-2759)
__device__ __forceinline__ void topk_row(const double* __restrict__ a, uint8_t* __restrict__ b, int K, int count)
{
    for (int k = 0; k < K; ++k) b[k] = 0;
    if (count > K) count = K;
    for (int j = 0; j < count; ++j) {
        int best = -1; double bv = 0.0;
        for (int k = 0; k < K; ++k) {
            if (b[k]) continue;
            const double v = -1.0 * a[k];                                     // argsort of negated values, sd.cpp:2727
            if (best < 0 || v < bv) { best = k; bv = v; }
        }
        if (best >= 0) b[best] = 1;
    }
}
