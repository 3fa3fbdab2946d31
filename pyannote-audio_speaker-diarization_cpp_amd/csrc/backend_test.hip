// backend_test.hip -- the sd_test_* hooks of the kernels behind the two networks (sdhip_test.h): postseg.hip, cluster.hip, reconstruct.hip, cut.hip and the
// casts of pipeline.cpp, for tests/test_backend_kernels.py.  Host code only (compiled with the exact-arithmetic flags all the same: it sits with those files).
// A hook lays the caller's operands out in guarded device buffers, calls the function the product's stage calls for the launch (run_postseg, run_count,
// pcm_to_wav, or a launch_* of common.h) and downloads the whole outputs.  It holds no kernel and restates no kernel logic; what it does check is that
// every index a kernel is DEFINED to follow stays inside the operand it was given.
#include "common.h"
#include "exact_fp.h"
#include <cmath>
#include <limits>

namespace {
const int64_t SLACK = 256;
const size_t LIMIT = (size_t)1 << 28;      // elements of one buffer of a case: a test case is small

// n operand elements, then `guard` elements of value g, in the named workspace
template <class T> int up(sd_ctx* c, const char* name, const T* src, size_t n, size_t guard, T g, T** d)
{
    std::vector<T> h(n + guard, g);
    if (n) memcpy(h.data(), src, n * sizeof(T));
    WS(c, T, p, name, h.size());
    HIPCHK(c, hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d = p;
    return SD_OK;
}
// a workspace of n elements, all v
template <class T> int fill(sd_ctx* c, const char* name, size_t n, T v, T** d)
{
    return up<T>(c, name, nullptr, 0, n, v, d);
}
template <class T> int down(sd_ctx* c, const T* d, size_t n, T* h)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    return SD_OK;
}
const float FNAN = std::numeric_limits<float>::quiet_NaN();
const double DNAN = std::numeric_limits<double>::quiet_NaN();
bool ascending_from_zero(const int32_t* off, int n, bool strictly)
{
    if (off[0] != 0) return false;
    for (int i = 0; i < n; ++i) if (off[i + 1] < off[i] + (strictly ? 1 : 0)) return false;
    return true;
}
// the checks sd_test_topk and sd_test_recon_cuts share
bool crop_ok(int64_t act_rows, int64_t n_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow)
{
    return rows >= 1 && ar0 >= 0 && ar0 + rows <= act_rows && crow >= 0 && crow <= rows && cr0 >= 0 && cr0 + crow <= n_count && n_count >= 0;
}
}
#define RUN(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

extern "C" int sd_test_binarize(sd_ctx* c, const float* seg, int64_t chunks, float fcanary, int32_t icanary, uint8_t* bin_out, float* masks_out, int32_t* nact_out)
{
    if (!c || !seg) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > (1 << 16)) SD_FAIL(c, SD_ERR_ARG, "sd_test_binarize: chunks %lld", (long long)chunks);
    const size_t per = (size_t)SD_FRAMES * SD_SPEAKERS, n = (size_t)(chunks + SLACK);
    float* dS; uint8_t* dB = nullptr; float* dM = nullptr; int* dN = nullptr;
    RUN(up<float>(c, "tb_seg", seg, (size_t)chunks * per, (size_t)SLACK * per, FNAN, &dS));
    if (bin_out) RUN(fill<uint8_t>(c, "tb_bin", n * per, (uint8_t)SD_TEST_BCANARY, &dB));
    if (masks_out) RUN(fill<float>(c, "tb_masks", n * per, fcanary, &dM));
    if (nact_out) RUN(fill<int>(c, "tb_nact", n * SD_SPEAKERS, icanary, &dN));
    RUN(run_postseg(c, dS, chunks, dB, dM, dN));
    if (bin_out) RUN(down(c, dB, n * per, bin_out));
    if (masks_out) RUN(down(c, dM, n * per, masks_out));
    if (nact_out) RUN(down(c, dN, n * SD_SPEAKERS, nact_out));
    return SD_OK;
}

extern "C" int sd_test_count(sd_ctx* c, const uint8_t* bin, int64_t chunks, float fcanary, int32_t icanary, int32_t* count_out, double* avg_out)
{
    if (!c || !bin || !count_out) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > (1 << 16)) SD_FAIL(c, SD_ERR_ARG, "sd_test_count: chunks %lld", (long long)chunks);
    const size_t per = (size_t)SD_FRAMES * SD_SPEAKERS;
    const int64_t nf = count_frames_host(chunks);
    uint8_t* dB; int32_t* dC; double* dA = nullptr;
    RUN(up<uint8_t>(c, "tb_bin", bin, (size_t)chunks * per, (size_t)SLACK * per, (uint8_t)0x55, &dB));
    RUN(fill<int32_t>(c, "tb_count", (size_t)(nf + SLACK), icanary, &dC));
    if (avg_out) RUN(fill<double>(c, "tb_avg", (size_t)(nf + SLACK), (double)fcanary, &dA));
    RUN(run_count(c, dB, chunks, dC, nf, dA));
    RUN(down(c, dC, (size_t)(nf + SLACK), count_out));
    if (avg_out) RUN(down(c, dA, (size_t)(nf + SLACK), avg_out));
    return SD_OK;
}

extern "C" int sd_test_gather_normalize(sd_ctx* c, const double* X, int64_t rows, const int32_t* tidx, int64_t N, int d, float fcanary, double* xout, double* xn_out)
{
    if (!c || !X || !tidx || !xn_out) return SD_ERR_ARG;
    ENTER(c);
    if (rows < 1 || N < 1 || d < 1 || (size_t)(rows + SLACK) * d > LIMIT || (size_t)(N + SLACK) * d > LIMIT)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_gather_normalize: rows %lld, N %lld, d %d", (long long)rows, (long long)N, d);
    for (int64_t i = 0; i < N; ++i)
        if (tidx[i] < 0 || tidx[i] >= rows) SD_FAIL(c, SD_ERR_ARG, "sd_test_gather_normalize: tidx[%lld] = %d leaves the %lld rows", (long long)i, tidx[i], (long long)rows);
    double* dX; int* dT; double* dO = nullptr; double* dN;
    RUN(up<double>(c, "tb_X", X, (size_t)rows * d, (size_t)SLACK * d, DNAN, &dX));
    RUN(up<int>(c, "tb_tidx", tidx, (size_t)N, (size_t)SLACK, (int)rows, &dT));
    if (xout) RUN(fill<double>(c, "tb_Xout", (size_t)(N + SLACK) * d, (double)fcanary, &dO));
    RUN(fill<double>(c, "tb_Xn", (size_t)(N + SLACK) * d, (double)fcanary, &dN));
    RUN(launch_gather_normalize(c, dX, dT, N, d, dO, dN));
    if (xout) RUN(down(c, dO, (size_t)(N + SLACK) * d, xout));
    return down(c, dN, (size_t)(N + SLACK) * d, xn_out);
}

extern "C" int sd_test_cluster_means(sd_ctx* c, const double* X, int64_t rows, int d, const int32_t* order, const int32_t* off, int nl, float fcanary, double* cen_out)
{
    if (!c || !X || !order || !off || !cen_out) return SD_ERR_ARG;
    ENTER(c);
    if (rows < 1 || d < 1 || nl < 1 || nl > (1 << 20) || (size_t)(rows + SLACK) * d > LIMIT || (size_t)(nl + SLACK) * d > LIMIT || !ascending_from_zero(off, nl, false))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_cluster_means: rows %lld, d %d, nl %d, or off does not ascend from 0", (long long)rows, d, nl);
    const int n = off[nl];
    for (int i = 0; i < n; ++i)
        if (order[i] < 0 || order[i] >= rows) SD_FAIL(c, SD_ERR_ARG, "sd_test_cluster_means: order[%d] = %d leaves the %lld rows", i, order[i], (long long)rows);
    double* dX; int* dO; int* dF; double* dC;
    RUN(up<double>(c, "tb_X", X, (size_t)rows * d, (size_t)SLACK * d, DNAN, &dX));
    RUN(up<int>(c, "tb_order", order, (size_t)n, (size_t)SLACK, (int)rows, &dO));
    RUN(up<int>(c, "tb_off", off, (size_t)nl + 1, (size_t)SLACK, 0, &dF));
    RUN(fill<double>(c, "tb_cen", (size_t)(nl + SLACK) * d, (double)fcanary, &dC));
    RUN(launch_cluster_means(c, dX, d, dO, dF, nl, dC));
    return down(c, dC, (size_t)(nl + SLACK) * d, cen_out);
}

extern "C" int sd_test_assign(sd_ctx* c, const double* E, int64_t M, int d, const double* cen, int K, float fcanary, int32_t icanary, int32_t* hard_out,
                              int32_t* err_out, double* soft_out, double* best_out)
{
    if (!c || !E || !cen || !hard_out || !err_out) return SD_ERR_ARG;
    ENTER(c);
    if (M < 1 || d < 1 || K < 1 || (size_t)(M + SLACK) * d > LIMIT || (size_t)(K + SLACK) * d > LIMIT || (size_t)(M + SLACK) * K > LIMIT)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_assign: M %lld, d %d, K %d", (long long)M, d, K);
    double* dE; double* dC; int* dH; int* dR; double* dS = nullptr; double* dB = nullptr;
    RUN(up<double>(c, "tb_E", E, (size_t)M * d, (size_t)SLACK * d, DNAN, &dE));
    RUN(up<double>(c, "tb_cen", cen, (size_t)K * d, (size_t)SLACK * d, DNAN, &dC));
    RUN(fill<int>(c, "tb_hard", (size_t)(M + SLACK), icanary, &dH));
    RUN(fill<int>(c, "tb_err", (size_t)(1 + SLACK), icanary, &dR));
    if (soft_out) RUN(fill<double>(c, "tb_soft", (size_t)(M + SLACK) * K, (double)fcanary, &dS));
    if (best_out) RUN(fill<double>(c, "tb_best", (size_t)(M + SLACK), (double)fcanary, &dB));
    HIPCHK(c, hipMemsetAsync(dR, 0, sizeof(int), c->stream));      // as assign_all clears it
    RUN(launch_assign(c, dE, M, d, dC, K, dH, dR, dS, dB));
    RUN(down(c, dH, (size_t)(M + SLACK), hard_out));
    RUN(down(c, dR, (size_t)(1 + SLACK), err_out));
    if (soft_out) RUN(down(c, dS, (size_t)(M + SLACK) * K, soft_out));
    if (best_out) RUN(down(c, dB, (size_t)(M + SLACK), best_out));
    return SD_OK;
}

extern "C" int sd_test_constrained_argmax(sd_ctx* c, const double* soft, int64_t chunks, int K, double fill_value, int32_t icanary, int32_t* hard_out)
{
    if (!c || !soft || !hard_out) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > (1 << 20) || K < 1 || K > 64) SD_FAIL(c, SD_ERR_ARG, "sd_test_constrained_argmax: chunks %lld, K %d (1 .. 64)", (long long)chunks, K);
    const size_t per = (size_t)SD_SPEAKERS * K;
    double* dS; int* dH;
    RUN(up<double>(c, "tb_soft", soft, (size_t)chunks * per, (size_t)SLACK * per, DNAN, &dS));
    RUN(fill<int>(c, "tb_hard", (size_t)(chunks + SLACK) * SD_SPEAKERS, icanary, &dH));
    RUN(launch_constrained_argmax(c, dS, chunks, K, fill_value, dH));
    return down(c, dH, (size_t)(chunks + SLACK) * SD_SPEAKERS, hard_out);
}

extern "C" int sd_test_activations(sd_ctx* c, const float* seg, const int32_t* hard, int64_t chunks, int K, float fcanary, double* act_out, int64_t act_cap,
                                   int64_t* nact_out)
{
    if (!c || !seg || !hard || !act_out || !nact_out) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > (1 << 16) || K < 1 || K > (1 << 12)) SD_FAIL(c, SD_ERR_ARG, "sd_test_activations: chunks %lld, K %d", (long long)chunks, K);
    ReconFrames g;
    reconstruct_frames(chunks, count_frames_host(chunks), (chunks - 1) * (int64_t)SD_HOP + SD_CHUNK, g);
    *nact_out = g.nact;
    if (act_cap != (g.nact + SLACK) * K) SD_FAIL(c, SD_ERR_ARG, "sd_test_activations: %lld frames, the caller expects %lld", (long long)g.nact, (long long)(act_cap / K - SLACK));
    const size_t per = (size_t)SD_FRAMES * SD_SPEAKERS;
    float* dS; int* dH; int* dF; double* dA;
    RUN(up<float>(c, "tb_seg", seg, (size_t)chunks * per, (size_t)SLACK * per, FNAN, &dS));
    RUN(up<int>(c, "tb_hard", hard, (size_t)chunks * SD_SPEAKERS, (size_t)SLACK * SD_SPEAKERS, 0, &dH));
    RUN(up<int>(c, "tb_sfr", g.sfr.data(), (size_t)chunks, (size_t)SLACK, 0, &dF));
    RUN(fill<double>(c, "tb_act", (size_t)act_cap, (double)fcanary, &dA));
    RUN(launch_activations(c, dS, dH, dF, chunks, K, dA, g.nact));
    return down(c, dA, (size_t)act_cap, act_out);
}

extern "C" int sd_test_topk(sd_ctx* c, const double* act, int64_t act_rows, const int32_t* count, int64_t n_count, int64_t ar0, int64_t cr0, int64_t rows,
                            int64_t crow, int K, uint8_t* binary_out)
{
    if (!c || !act || !binary_out || (!count && n_count > 0)) return SD_ERR_ARG;
    ENTER(c);
    if (K < 1 || K > (1 << 12) || act_rows < 1 || (size_t)(act_rows + SLACK) * K > LIMIT || !crop_ok(act_rows, n_count, ar0, cr0, rows, crow))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_topk: rows [%lld, +%lld) of %lld, counts [%lld, +%lld) of %lld, K %d", (long long)ar0, (long long)rows, (long long)act_rows,
                (long long)cr0, (long long)crow, (long long)n_count, K);
    double* dA; int32_t* dC; uint8_t* dB;
    RUN(up<double>(c, "tb_act", act, (size_t)act_rows * K, (size_t)SLACK * K, DNAN, &dA));
    RUN(up<int32_t>(c, "tb_count", count, (size_t)n_count, (size_t)SLACK, 0x7fffffff, &dC));
    RUN(fill<uint8_t>(c, "tb_binary", (size_t)(rows + SLACK) * K, (uint8_t)SD_TEST_BCANARY, &dB));
    RUN(launch_topk(c, dA, dC, ar0, cr0, rows, crow, K, dB));
    return down(c, dB, (size_t)(rows + SLACK) * K, binary_out);
}

extern "C" int sd_test_assign_cuts(sd_ctx* c, const double* E, int64_t M, int d, const double* cen, const int32_t* coff, const int32_t* slot, int Tn, int n_slots,
                                   const int32_t* nact, float fcanary, int32_t icanary, double* m2_out, int32_t* hard_out, double* best_out, int32_t* err_out)
{
    if (!c || !E || !cen || !coff || !slot || !nact || !m2_out || !hard_out || !best_out || !err_out) return SD_ERR_ARG;
    ENTER(c);
    if (M < 1 || d < 1 || Tn < 1 || Tn > (1 << 16) || n_slots < Tn || n_slots > (1 << 16) || !ascending_from_zero(coff, Tn, true))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_assign_cuts: M %lld, d %d, Tn %d, n_slots %d, or coff does not ascend strictly from 0", (long long)M, d, Tn, n_slots);
    const int total = coff[Tn];
    if ((size_t)(M + SLACK) * d > LIMIT || (size_t)(total + SLACK) * d > LIMIT || (size_t)n_slots * M > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_assign_cuts: the case is too large");
    std::vector<char> seen((size_t)n_slots, 0);
    for (int q = 0; q < Tn; ++q) {
        if (slot[q] < 0 || slot[q] >= n_slots || seen[(size_t)slot[q]]) SD_FAIL(c, SD_ERR_ARG, "sd_test_assign_cuts: slot[%d] = %d (distinct, below %d)", q, slot[q], n_slots);
        seen[(size_t)slot[q]] = 1;
    }
    double* dE; double* dC; int* dF; int* dS; int* dN; double* dM; int* dH; double* dB; int* dR;
    RUN(up<double>(c, "tb_E", E, (size_t)M * d, (size_t)SLACK * d, DNAN, &dE));
    RUN(up<double>(c, "tb_cen", cen, (size_t)total * d, (size_t)SLACK * d, DNAN, &dC));
    RUN(up<int>(c, "tb_coff", coff, (size_t)Tn + 1, (size_t)SLACK, total, &dF));
    RUN(up<int>(c, "tb_slot", slot, (size_t)Tn, (size_t)SLACK, 0, &dS));
    RUN(up<int>(c, "tb_nact", nact, (size_t)M, (size_t)SLACK, 0, &dN));
    RUN(fill<double>(c, "tb_m2", (size_t)(total + SLACK), (double)fcanary, &dM));
    RUN(fill<int>(c, "tb_hard", (size_t)n_slots * M + SLACK, icanary, &dH));
    RUN(fill<double>(c, "tb_best", (size_t)Tn * M + SLACK, (double)fcanary, &dB));
    RUN(fill<int>(c, "tb_err", (size_t)(1 + SLACK), icanary, &dR));
    HIPCHK(c, hipMemsetAsync(dR, 0, sizeof(int), c->stream));      // as cut_group clears it
    RUN(launch_cut_cen_norms(c, dC, total, d, dM));
    RUN(launch_assign_cuts(c, dE, M, d, dC, dM, dF, dS, Tn, dN, dH, dB, dR));
    RUN(down(c, dM, (size_t)(total + SLACK), m2_out));
    RUN(down(c, dH, (size_t)n_slots * M + SLACK, hard_out));
    RUN(down(c, dB, (size_t)Tn * M + SLACK, best_out));
    return down(c, dR, (size_t)(1 + SLACK), err_out);
}

extern "C" int sd_test_recon_cuts(sd_ctx* c, const float* seg, const int32_t* hard, int64_t chunks, const int32_t* koff, int Tg, const double* act_in,
                                  const int32_t* count, int64_t n_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow, float fcanary, double* act_out,
                                  int64_t act_cap, uint8_t* binary_out, int64_t* nact_out)
{
    if (!c || !seg || !hard || !koff || !act_out || !binary_out || !nact_out || (!count && n_count > 0)) return SD_ERR_ARG;
    ENTER(c);
    if (chunks < 1 || chunks > (1 << 16) || Tg < 1 || Tg > (1 << 16) || !ascending_from_zero(koff, Tg, true))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_recon_cuts: chunks %lld, Tg %d, or koff does not ascend strictly from 0", (long long)chunks, Tg);
    ReconFrames g;
    reconstruct_frames(chunks, count_frames_host(chunks), (chunks - 1) * (int64_t)SD_HOP + SD_CHUNK, g);
    const int64_t nact = g.nact, sumK = koff[Tg];
    *nact_out = nact;
    if (act_cap != nact * sumK + SLACK || (size_t)act_cap > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_recon_cuts: %lld frames, the caller expects %lld elements", (long long)nact, (long long)act_cap);
    if (!crop_ok(nact, n_count, ar0, cr0, rows, crow))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_recon_cuts: rows [%lld, +%lld) of %lld, counts [%lld, +%lld) of %lld", (long long)ar0, (long long)rows, (long long)nact,
                (long long)cr0, (long long)crow, (long long)n_count);
    const size_t per = (size_t)SD_FRAMES * SD_SPEAKERS, hrow = (size_t)chunks * SD_SPEAKERS;
    float* dS; int* dH; int* dF; int* dK; double* dA; double* dI = nullptr; int32_t* dC; uint8_t* dB;
    RUN(up<float>(c, "tb_seg", seg, (size_t)chunks * per, (size_t)SLACK * per, FNAN, &dS));
    RUN(up<int>(c, "tb_hard", hard, (size_t)Tg * hrow, (size_t)SLACK * SD_SPEAKERS, 0, &dH));
    RUN(up<int>(c, "tb_sfr", g.sfr.data(), (size_t)chunks, (size_t)SLACK, 0, &dF));
    RUN(up<int>(c, "tb_koff", koff, (size_t)Tg + 1, (size_t)SLACK, (int)sumK, &dK));
    RUN(fill<double>(c, "tb_act", (size_t)act_cap, (double)fcanary, &dA));
    if (act_in) RUN(up<double>(c, "tb_act_in", act_in, (size_t)(nact * sumK), (size_t)SLACK, DNAN, &dI));
    RUN(up<int32_t>(c, "tb_count", count, (size_t)n_count, (size_t)SLACK, 0x7fffffff, &dC));
    RUN(fill<uint8_t>(c, "tb_binary", (size_t)(rows * sumK + SLACK), (uint8_t)SD_TEST_BCANARY, &dB));
    RUN(launch_activations_cuts(c, dS, dH, dF, chunks, dK, Tg, sumK, dA, nact));
    RUN(launch_topk_cuts(c, act_in ? dI : dA, dC, ar0, cr0, rows, crow, dK, Tg, nact, dB));
    RUN(down(c, dA, (size_t)act_cap, act_out));
    return down(c, dB, (size_t)(rows * sumK + SLACK), binary_out);
}

extern "C" int sd_test_pcm_to_f32(sd_ctx* c, const int16_t* pcm, int64_t n, float fcanary, float* wav_out)
{
    if (!c || !pcm || !wav_out) return SD_ERR_ARG;
    ENTER(c);
    if (n < 1 || (size_t)n > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_pcm_to_f32: n %lld", (long long)n);
    const size_t total = (size_t)n + SD_WAV_PAD + SLACK;
    int16_t* dP; float* dW;
    RUN(up<int16_t>(c, "tb_pcm", pcm, (size_t)n, (size_t)SLACK, (int16_t)0x7fff, &dP));
    RUN(fill<float>(c, "wav_f32", total, fcanary, &dW));      // pcm_to_wav's own workspace, reserved with its slack: the function finds it in place
    DevWav w{nullptr, 0};
    RUN(pcm_to_wav(c, dP, n, &w));
    if (w.p != dW) SD_FAIL(c, SD_ERR_ARG, "sd_test_pcm_to_f32: pcm_to_wav moved the workspace the hook had reserved");
    return down(c, dW, total, wav_out);
}

extern "C" int sd_test_f32_to_f64(sd_ctx* c, const float* a, int64_t n, float fcanary, double* b_out)
{
    if (!c || !a || !b_out) return SD_ERR_ARG;
    ENTER(c);
    if (n < 1 || (size_t)n > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_f32_to_f64: n %lld", (long long)n);
    float* dA; double* dB;
    RUN(up<float>(c, "tb_f32", a, (size_t)n, (size_t)SLACK, FNAN, &dA));
    RUN(fill<double>(c, "tb_f64", (size_t)(n + SLACK), (double)fcanary, &dB));
    RUN(launch_f32_to_f64(c, dA, dB, n));
    return down(c, dB, (size_t)(n + SLACK), b_out);
}

extern "C" int sd_test_mark_inactive(sd_ctx* c, const int32_t* hard, const int32_t* nact, int64_t n, int32_t icanary, int32_t* hard_out)
{
    if (!c || !hard || !nact || !hard_out) return SD_ERR_ARG;
    ENTER(c);
    if (n < 1 || (size_t)n > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_mark_inactive: n %lld", (long long)n);
    int* dH; int* dN;
    RUN(up<int>(c, "tb_hard", hard, (size_t)n, (size_t)SLACK, icanary, &dH));
    RUN(up<int>(c, "tb_nact", nact, (size_t)n, (size_t)SLACK, 0, &dN));
    RUN(launch_mark_inactive(c, dH, dN, n));
    return down(c, dH, (size_t)(n + SLACK), hard_out);
}
