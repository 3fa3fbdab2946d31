// resample.hip -- SURVEY 8(f) row 2, the resample leg: Resampler::Resample (frontend/resampler.cc:19-36), i.e. libsamplerate 0.2.2's
// src_simple(SRC_SINC_BEST_QUALITY) with ratio out_sr / in_sr (pinned by pipeline/cmake/samplerate.cmake; the library itself is a
// FetchContent download and NOT in the reference checkout).
//
// What is kept of the reference: the call's contract -- mono float in, mono float out, ratio = out_sr / in_sr held in a FLOAT, output
// length (size_t)(in.size() * ratio) evaluated in float exactly as resampler.cc:21-22 does, output sample m taken at input time
// m * in_sr / out_sr with silence before the first and after the last input sample (src_simple: one-shot, end_of_input = 1).
// What cannot be kept: libsamplerate's arithmetic is a 340 239-entry coefficient table (src_sinc.c / high_qual_coeffs.h) that is
// third-party data absent here, so sample values are NOT comparable with it ("parity unpinned" for this leg).  The
// published algorithm is restated instead -- band-limited interpolation with a windowed sinc whose cutoff follows the LOWER of the
// two rates (J. O. Smith, "Digital Audio Resampling", the method libsamplerate's documentation names) -- in its exact polyphase
// form for the rational ratio L / M = out_sr / in_sr (no table interpolation error):
//     y[m] = sum_k x[k] * h(m * M - k * L),   h(u) = L * 2 fc * sinc(2 fc u) * kaiser_beta(u / half),  |u| <= half
//     fc = RS_CUTOFF / (2 * max(L, M))  (cycles per sample of the rate in_sr * L),  half = RS_ZEROS / (2 fc)
// with RS_ZEROS = 64 zero crossings per wing, RS_CUTOFF = 0.95 of the lower Nyquist frequency, Kaiser beta = 10.056 (100 dB).
// oracle/resample_oracle.py evaluates the same definition in float64 with numpy; scipy.signal.resample_poly applies the same taps
// independently.  One thread per output sample; the input span of a 256-output tile is staged in LDS (coalesced), the tap table
// [tap][phase] (built on the host in double, stored as float) stays in L2: a wave reads 64 phases of one tap row.
// That arithmetic is ONE device body, resample_point, under two kernels: k_resample (the whole recording) and k_resample_jobs (a table of windows of
// recordings that are still arriving: the streams with an input rate of stream.hip; the rule of what is final and the rows: resample_book.h).
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "resample_book.h"      // the plan of a rate pair, the two length rules, ResampleJob

static double bessel_i0(double x)
{
    double s = 1.0, t = 1.0;
    const double q = x * x / 4.0;
    for (int k = 1; k < 200; ++k) { t *= q / ((double)k * (double)k); s += t; if (t < 1e-17 * s) break; }
    return s;
}

extern "C" int64_t sd_resample_len(int64_t n, int32_t in_sr, int32_t out_sr) { return resample_len(n, in_sr, out_sr); }

extern "C" int64_t sd_resample_final_len(int64_t n, int32_t in_sr, int32_t out_sr)
{
    ResamplePlan p;
    if (n < 0 || make_plan(in_sr, out_sr, p)) return -1;
    return resample_final_len(n, in_sr, out_sr, p);
}

// The one device body of k_resample and k_resample_jobs (and of the off-rate tiles of k_many_ingest, ingest.hip): resample_point
#include "resample_dev.h"

// y[m], m in [0, n_out): thread per output; xs = input samples [base, base + span) of the tile, zero outside [0, n_in)
__global__ __launch_bounds__(RS_BLOCK) void k_resample(const float* __restrict__ x, int64_t n_in, float* __restrict__ y, int64_t n_out,
                                                        const float* __restrict__ taps /*[2J+1][L]*/, int L, int M, int J, int span)
{
    extern __shared__ float xs[];
    const int64_t m0 = (int64_t)blockIdx.x * RS_BLOCK;
    resample_point(xs, RsLoadF32{x}, 0, n_in, m0, n_out, taps, L, M, J, span, y + m0);
}

// Any number of windows in one launch: row r of the table (ResampleJob, resample_book.h) has tile0[r + 1] - tile0[r] tiles of RS_BLOCK outputs counted from
// ITS first output; a block finds its row in the prefix table (cut.hip: seg_of) and runs the body on it.  Rows of different rate pairs share the launch:
// dynamic LDS is the largest span of the call.  The tile's sums land in LDS; a full tile whose place in dst is 16-byte aligned leaves as 64 stores of
// 16 bytes, any other tile as one float per thread; the row's last tile writes the `pad` zeros behind the last output.  64-bit indices throughout.
__global__ __launch_bounds__(RS_BLOCK) void k_resample_jobs(const ResampleJob* __restrict__ rows, const int64_t* __restrict__ tile0 /*[R + 1]*/, int R)
{
    extern __shared__ float xs[];
    __shared__ __align__(16) float ys[RS_BLOCK];
    const int64_t tile = blockIdx.x;
    int lo = 0, hi = R;                                                  // the last row with tile0[row] <= tile
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (tile0[mid] <= tile) lo = mid; else hi = mid; }
    const ResampleJob row = rows[lo];
    const int64_t off = (tile - tile0[lo]) * RS_BLOCK;                   // this tile's outputs go to dst[off ...]
    const int span = (int)(((int64_t)(RS_BLOCK - 1) * row.M) / row.L) + 2 * row.J + 3;
    resample_point(xs, RsLoadF32{row.src}, row.first, row.n_limit, row.m_first + off, row.m_first + row.count, row.taps, row.L, row.M, row.J, span, ys);
    __syncthreads();
    float* d = row.dst + off;
    const int64_t left = row.count - off;                                // outputs of this tile and of the tiles behind it
    if (left >= RS_BLOCK && ((uintptr_t)d & 15) == 0) {
        if (threadIdx.x < RS_BLOCK / 4) reinterpret_cast<float4*>(d)[threadIdx.x] = reinterpret_cast<const float4*>(ys)[threadIdx.x];
    } else if (threadIdx.x < left) d[threadIdx.x] = ys[threadIdx.x];
    if (left <= RS_BLOCK) for (int64_t i = left + threadIdx.x; i < left + row.pad; i += RS_BLOCK) d[i] = 0.0f;
}

// the plan of a rate pair, or the refusals of sd_resample: a bad rate, a tap table or a tile's input span that is too large
int resample_check(sd_ctx* c, int32_t in_sr, int32_t out_sr, ResamplePlan& p)
{
    if (make_plan(in_sr, out_sr, p)) SD_FAIL(c, SD_ERR_ARG, "sd_resample: bad sample rate %d -> %d", in_sr, out_sr);
    const int64_t ntap = 2 * (int64_t)p.J + 1;
    if (ntap * p.L > (int64_t)64 << 20) SD_FAIL(c, SD_ERR_ARG, "sd_resample: %d -> %d Hz needs a %lld x %lld tap table (ratio %lld / %lld): unsupported rate pair",
                                                  in_sr, out_sr, (long long)ntap, (long long)p.L, (long long)p.L, (long long)p.M);
    if (p.span * (int64_t)sizeof(float) > 160 * 1024) SD_FAIL(c, SD_ERR_ARG, "sd_resample: %d -> %d Hz: a tile's input span (%lld samples) does not fit the LDS", in_sr, out_sr, (long long)p.span);
    return SD_OK;
}

// the tap table of a rate pair that resample_check accepted: double on the host, float on the device; cached per rate pair
int resample_taps(sd_ctx* c, int32_t in_sr, int32_t out_sr, const ResamplePlan& p, const float** taps)
{
    const int64_t ntap = 2 * (int64_t)p.J + 1;
    char key[64];
    snprintf(key, sizeof(key), "rs_taps_%d_%d", in_sr, out_sr);
    // "filled" is recorded only after the upload has completed: a failed allocation or copy leaves no entry behind that a later call would trust
    const bool have = c->rs_taps_filled.count(key) != 0;
    WS(c, float, d_taps, key, ntap * p.L);
    if (!have) {
        std::vector<float> h((size_t)(ntap * p.L));
        const double i0b = bessel_i0(RS_BETA);
        for (int64_t jj = 0; jj < ntap; ++jj)
            for (int64_t ph = 0; ph < p.L; ++ph) {
                const double u = (double)ph + (double)(jj - p.J) * (double)p.L;
                double v = 0.0;
                if (std::fabs(u) <= p.half) {
                    const double a = 2.0 * p.fc * u, r = u / p.half;
                    const double sinc = a == 0.0 ? 1.0 : std::sin(M_PI * a) / (M_PI * a);
                    v = (double)p.L * 2.0 * p.fc * sinc * bessel_i0(RS_BETA * std::sqrt(1.0 - r * r > 0 ? 1.0 - r * r : 0.0)) / i0b;
                }
                h[(size_t)(jj * p.L + ph)] = (float)v;
            }
        HIPCHK(c, hipMemcpyAsync(d_taps, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));                      // h goes out of scope
        c->rs_taps_filled.insert(key);
    }
    *taps = d_taps;
    return SD_OK;
}

// device-resident form used by sd_diarize_wav; d_out must hold sd_resample_len(n, in_sr, out_sr) floats
int resample_dev(sd_ctx* c, const float* d_in, int64_t n, int32_t in_sr, int32_t out_sr, float* d_out, int64_t n_out)
{
    ResamplePlan p;
    int rc;
    if ((rc = resample_check(c, in_sr, out_sr, p))) return rc;
    if (n_out <= 0) return SD_OK;
    const float* d_taps = nullptr;
    if ((rc = resample_taps(c, in_sr, out_sr, p, &d_taps))) return rc;
    const int64_t ntap = 2 * (int64_t)p.J + 1;
    const size_t lds = (size_t)p.span * sizeof(float);
    if (lds > 64 * 1024) HIPCHK(c, hipFuncSetAttribute((const void*)k_resample, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int64_t blocks = (n_out + RS_BLOCK - 1) / RS_BLOCK;
    {
        ProfScope ps(c, "resample", 2.0 * (double)ntap * (double)n_out, 4.0 * (double)(n + n_out));
        hipLaunchKernelGGL(k_resample, dim3((unsigned)blocks), dim3(RS_BLOCK), lds, c->stream, d_in, n, d_out, n_out, d_taps, (int)p.L, (int)p.M, p.J, (int)p.span);
    }
    KCHECK(c);
    return SD_OK;
}

// one k_resample_jobs launch for rows[0, R) (every count > 0; every rate pair accepted by resample_check); ordered on the context's stream.  A workgroup
// holds a row's input span AND the static ys[RS_BLOCK] in LDS: a row whose span plus RS_BLOCK floats exceed 160 KB is refused with SD_ERR_ARG before
// anything is uploaded or launched (the rule of sd_stream_set_input_rate; resample_check alone, which k_resample goes by, admits spans up to 160 KB)
int resample_jobs(sd_ctx* c, const ResampleJob* rows, int64_t R)
{
    if (R <= 0) return SD_OK;
    std::vector<int64_t> tile0((size_t)R + 1, 0);
    size_t lds = 0;
    double flops = 0.0, bytes = 0.0;
    for (int64_t r = 0; r < R; ++r) {
        const ResampleJob& j = rows[r];
        if (j.count <= 0 || j.L <= 0 || j.M <= 0 || j.J < 0 || j.pad < 0) SD_FAIL(c, SD_ERR_ARG, "resample_jobs: bad row %lld", (long long)r);
        const int64_t span = ((int64_t)(RS_BLOCK - 1) * j.M) / j.L + 2 * (int64_t)j.J + 3;
        if ((span + RS_BLOCK) * (int64_t)sizeof(float) > 160 * 1024)      // (the span and the kernel's static ys[RS_BLOCK]: sd_stream_set_input_rate's rule)
            SD_FAIL(c, SD_ERR_ARG, "resample_jobs: row %lld: a tile's input span (%lld samples) and its %d outputs do not fit the LDS", (long long)r, (long long)span, RS_BLOCK);
        lds = std::max(lds, (size_t)span * sizeof(float));
        tile0[(size_t)r + 1] = tile0[(size_t)r] + (j.count + RS_BLOCK - 1) / RS_BLOCK;
        flops += 2.0 * (double)(2 * j.J + 1) * (double)j.count;
        bytes += 4.0 * ((double)j.count * (double)j.M / (double)j.L + (double)j.count);
    }
    if (tile0[(size_t)R] > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "resample_jobs: %lld tiles in one launch", (long long)tile0[(size_t)R]);
    // the prefix table and the rows behind it: one workspace, one upload
    static_assert(sizeof(ResampleJob) % sizeof(int64_t) == 0 && alignof(ResampleJob) <= alignof(int64_t), "the rows sit behind R + 1 int64");
    const size_t head = ((size_t)R + 1) * sizeof(int64_t), tab_bytes = head + (size_t)R * sizeof(ResampleJob);
    std::vector<char> tab(tab_bytes);
    memcpy(tab.data(), tile0.data(), head);
    memcpy(tab.data() + head, rows, (size_t)R * sizeof(ResampleJob));
    WS(c, char, d_tab, "rs_jobs", tab_bytes);
    HIPCHK(c, hipMemcpy(d_tab, tab.data(), tab_bytes, hipMemcpyHostToDevice));
    const int64_t* d_tile0 = (const int64_t*)d_tab;
    const ResampleJob* d_rows = (const ResampleJob*)(d_tab + head);
    if (lds > 64 * 1024 - RS_BLOCK * sizeof(float)) HIPCHK(c, hipFuncSetAttribute((const void*)k_resample_jobs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        ProfScope ps(c, "resample_jobs", flops, bytes);
        hipLaunchKernelGGL(k_resample_jobs, dim3((unsigned)tile0[(size_t)R]), dim3(RS_BLOCK), lds, c->stream, d_rows, d_tile0, (int)R);
    }
    KCHECK(c);
    return SD_OK;
}

extern "C" int sd_resample(sd_ctx* c, const float* wav, int64_t n, int32_t in_sr, int32_t out_sr, float* out, int64_t cap, int64_t* n_out)
{
    if (!c) return SD_ERR_ARG;
    c->err.clear();
    if (hipSetDevice(c->device) != hipSuccess) SD_FAIL(c, SD_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    if (!wav || n <= 0 || !n_out) SD_FAIL(c, SD_ERR_ARG, "sd_resample: bad argument");
    const int64_t no = sd_resample_len(n, in_sr, out_sr);
    if (no < 0) SD_FAIL(c, SD_ERR_ARG, "sd_resample: bad sample rate %d -> %d", in_sr, out_sr);
    *n_out = no;
    if (!out) return SD_OK;                                              // length query
    if (cap < no) SD_FAIL(c, SD_ERR_ARG, "sd_resample: output buffer holds %lld samples, %lld needed", (long long)cap, (long long)no);
    WS(c, float, d_in, "rs_in", n);
    WS(c, float, d_out, "rs_out", no > 0 ? no : 1);
    HIPCHK(c, hipMemcpyAsync(d_in, wav, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    int rc;
    if ((rc = resample_dev(c, d_in, n, in_sr, out_sr, d_out, no))) return rc;
    if (no > 0) HIPCHK(c, hipMemcpyAsync(out, d_out, (size_t)no * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    sd_flush_profile(c);
    return SD_OK;
}
