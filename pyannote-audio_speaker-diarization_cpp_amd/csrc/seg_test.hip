// seg_test.hip -- sd_test_lstm_rec / sd_test_pool_norm / sd_test_chunk_norm / sd_test_classifier (sdhip_test.h): ONE launch of one of pyannet.hip's
// kernels, for tests/test_seg_kernels.py.  Host code only.  A hook lays the caller's operands out in guarded buffers, uploads them, calls the launcher
// seg_batch calls (common.h: launch_lstm_rec, launch_pool_norm, launch_chunk_norm / launch_chunk_stats, launch_classifier) and downloads the whole output
// buffer.  It holds no kernel and restates no kernel logic: grid, block and template choice are the launchers', the split planes of W_hh come from
// weights.cpp's lstm_whh_split.  What a hook does check is that every address the kernel is DEFINED to read lies inside the operand it was given.
#include "common.h"
#include <cmath>
#include <limits>

namespace {
const int64_t SLACK = 256;              // guard rows behind every buffer
// `n` operand floats, then `slack` NaNs
std::vector<float> with_nan(const float* src, size_t n, size_t slack)
{
    std::vector<float> v(n + slack, std::numeric_limits<float>::quiet_NaN());
    if (n) memcpy(v.data(), src, n * sizeof(float));
    return v;
}
int up(sd_ctx* c, const char* name, const std::vector<float>& h, float** d)
{
    WS(c, float, p, name, h.size());
    HIPCHK(c, hipMemcpyAsync(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // (the host image is the caller's temporary)
    *d = p;
    return SD_OK;
}
// a device buffer of n floats, all `canary`
int canary_buf(sd_ctx* c, const char* name, size_t n, float canary, float** d)
{
    return up(c, name, std::vector<float>(n, canary), d);
}
int down(sd_ctx* c, const float* d, size_t n, float* h)
{
    HIPCHK(c, hipMemcpyAsync(h, d, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}
}

extern "C" int sd_test_lstm_rec(sd_ctx* c, const float* G, const float* whh_f, const float* whh_b, int64_t B, int F, int prec, float canary, float* h_out)
{
    if (!c || !G || !whh_f || !whh_b || !h_out) return SD_ERR_ARG;
    ENTER(c);
    if (B < 1 || F < 1 || B * (int64_t)F > (1 << 20) || (prec != 0 && prec != 3)) SD_FAIL(c, SD_ERR_ARG, "sd_test_lstm_rec: B %lld, F %d, prec %d", (long long)B, F, prec);
    const size_t rows = (size_t)B * F, nw = (size_t)512 * 128;
    int rc;
    float *dG, *dWf, *dWb, *dH;
    if ((rc = up(c, "ts_G", with_nan(G, rows * 1024, SLACK * 1024), &dG))) return rc;
    if ((rc = up(c, "ts_whh_f", with_nan(whh_f, nw, SLACK), &dWf))) return rc;
    if ((rc = up(c, "ts_whh_b", with_nan(whh_b, nw, SLACK), &dWb))) return rc;
    if ((rc = canary_buf(c, "ts_H", (rows + SLACK) * 256, canary, &dH))) return rc;
    void *dXf = nullptr, *dXb = nullptr;
    float inv[2] = {0.0f, 0.0f};
    if (prec == 3) {
        std::vector<_Float16> hx(2 * nw);
        WS(c, _Float16, xf, "ts_whx_f", 2 * nw);
        WS(c, _Float16, xb, "ts_whx_b", 2 * nw);
        inv[0] = lstm_whh_split(whh_f, hx.data());
        HIPCHK(c, hipMemcpyAsync(xf, hx.data(), 2 * nw * sizeof(_Float16), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));             // (hx is reused)
        inv[1] = lstm_whh_split(whh_b, hx.data());
        HIPCHK(c, hipMemcpyAsync(xb, hx.data(), 2 * nw * sizeof(_Float16), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dXf = xf; dXb = xb;
    }
    if ((rc = launch_lstm_rec(c, dG, dWf, dWb, dXf, dXb, inv[0], inv[1], dH, B, F))) return rc;
    return down(c, dH, (rows + SLACK) * 256, h_out);
}

extern "C" int sd_test_pool_norm(sd_ctx* c, const float* in, int64_t in_rows, int64_t chunks, int Lc, int stage, const float* gw, const float* gb,
                                 const float* cst, const float* wsum, int chunk_rows, float canary, float* out)
{
    if (!c || !in || !gw || !gb || !out) return SD_ERR_ARG;
    ENTER(c);
    const bool shared = cst != nullptr;
    if (stage < 0 || stage > 2 || chunks < 1 || chunks > 4096 || Lc < 3 || Lc > (1 << 20) || (shared && (stage != 0 || !wsum || chunk_rows < 1)))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_pool_norm: stage %d, chunks %lld, Lc %d", stage, (long long)chunks, Lc);
    // rows the kernel is defined to read: chunk ck's rows [start, start + 3 (Lc / 3)), start = ck * chunk_rows (shared) or ck * Lc
    const int64_t need = shared ? (chunks - 1) * (int64_t)chunk_rows + Lc : chunks * (int64_t)Lc;
    if (in_rows != need) SD_FAIL(c, SD_ERR_ARG, "sd_test_pool_norm: %lld input rows, the case reads %lld", (long long)in_rows, (long long)need);
    const int C = stage == 0 ? 80 : 60, CPAD = stage == 0 ? 96 : 64, Lp = Lc / 3;
    int rc;
    float *dIn, *dGw, *dGb, *dOut, *dCst = nullptr, *dWs = nullptr;
    if ((rc = up(c, "ts_pn_in", with_nan(in, (size_t)in_rows * C, (size_t)SLACK * C), &dIn))) return rc;
    if ((rc = up(c, "ts_pn_gw", with_nan(gw, (size_t)C, SLACK), &dGw))) return rc;
    if ((rc = up(c, "ts_pn_gb", with_nan(gb, (size_t)C, SLACK), &dGb))) return rc;
    if (shared) {
        if ((rc = up(c, "ts_pn_cst", with_nan(cst, (size_t)chunks * 2, SLACK), &dCst))) return rc;
        if ((rc = up(c, "ts_pn_wsum", with_nan(wsum, 80, SLACK), &dWs))) return rc;
    }
    const size_t n_out = ((size_t)chunks * Lp + SLACK) * CPAD;
    if ((rc = canary_buf(c, "ts_pn_out", n_out, canary, &dOut))) return rc;
    if ((rc = launch_pool_norm(c, stage, dIn, chunks, Lc, dGw, dGb, dOut, (const float2*)dCst, dWs, shared ? chunk_rows : 0))) return rc;
    return down(c, dOut, n_out, out);
}

extern "C" int sd_test_chunk_norm(sd_ctx* c, const float* wav, int64_t n_wav, int64_t origin, int64_t first_chunk, int64_t hop, int L, int64_t chunks,
                                  float w, float b, int stats_only, float canary, float* out)
{
    if (!c || !wav || !out) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > 4096 || L < 1 || L > SD_CHUNK || hop < 1 || n_wav < 1 || (stats_only && hop != SD_HOP))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_chunk_norm: chunks %lld, L %d, hop %lld%s", (long long)chunks, L, (long long)hop, stats_only ? " (k_chunk_stats: hop is 8000)" : "");
    // samples the kernel is defined to read: chunk ck's [base, base + L), base = (first_chunk + ck) * hop - origin
    const int64_t lo = first_chunk * hop - origin, hi = (first_chunk + chunks - 1) * hop - origin + L;
    if (lo < 0 || hi > n_wav) SD_FAIL(c, SD_ERR_ARG, "sd_test_chunk_norm: the case reads samples [%lld, %lld) of %lld", (long long)lo, (long long)hi, (long long)n_wav);
    int rc;
    float *dW, *dOut;
    if ((rc = up(c, "ts_cn_wav", with_nan(wav, (size_t)n_wav, (size_t)SLACK * 4), &dW))) return rc;
    const size_t n_out = stats_only ? ((size_t)chunks + SLACK) * 2 : (size_t)chunks * SD_CHUNK + SLACK * 4;
    if ((rc = canary_buf(c, "ts_cn_out", n_out, canary, &dOut))) return rc;
    if (stats_only) rc = launch_chunk_stats(c, dW, origin, first_chunk, L, chunks, w, b, (float2*)dOut);
    else rc = launch_chunk_norm(c, dW, origin, first_chunk, hop, L, chunks, w, b, dOut);
    if (rc) return rc;
    return down(c, dOut, n_out, out);
}

extern "C" int sd_test_classifier(sd_ctx* c, const float* y, const float* W, const float* bias, int64_t chunks, int F, float canary, float* seg_out)
{
    if (!c || !y || !W || !bias || !seg_out) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > 4096 || F < 1 || F > SD_FRAMES) SD_FAIL(c, SD_ERR_ARG, "sd_test_classifier: chunks %lld, F %d", (long long)chunks, F);
    int rc;
    float *dY, *dW, *dB, *dS;
    if ((rc = up(c, "ts_cl_y", with_nan(y, (size_t)chunks * F * 128, (size_t)SLACK * 128), &dY))) return rc;
    if ((rc = up(c, "ts_cl_w", with_nan(W, 384, SLACK), &dW))) return rc;
    if ((rc = up(c, "ts_cl_b", with_nan(bias, 3, SLACK), &dB))) return rc;
    const size_t n_out = ((size_t)chunks * SD_FRAMES + SLACK) * 3;
    if ((rc = canary_buf(c, "ts_cl_seg", n_out, canary, &dS))) return rc;
    if ((rc = launch_classifier(c, dY, dW, dB, dS, chunks, F))) return rc;
    return down(c, dS, n_out, seg_out);
}
