// frontend_test.hip -- sd_test_frontend_prepare / sd_test_frontend_features / sd_test_frontend_signals (sdhip_test.h): the kernels of frontend.hip through
// the functions run_embed, sd_frontend and sd_embed_signals call, for tests/test_frontend_kernels.py.  Host code only.  A hook lays the caller's operands
// out in guarded buffers, uploads them, calls frontend_prepare / ecapa_row_plan / frontend_features (or embed_signals_frames / frontend_prepare_signals) in
// the product's order and downloads the whole outputs.  It holds no kernel and restates no kernel logic.  frontend_prepare keeps its tables in named
// workspaces of the context; a hook reserves those with 256 slack entries and fills them with the canary first, so the function finds them in place.
// What a hook does check is that every waveform address the kernel is DEFINED to read lies inside the slice it was given.
#include "common.h"
#include <cmath>
#include <limits>

namespace {
const int64_t SLACK = 256;
const float QNAN = std::numeric_limits<float>::quiet_NaN();
// a device workspace of n floats / ints, all `v`
int fill_f(sd_ctx* c, const char* name, size_t n, float v, float** d)
{
    const std::vector<float> h(n, v);
    WS(c, float, p, name, n);
    HIPCHK(c, hipMemcpyAsync(p, h.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d = p;
    return SD_OK;
}
int fill_i(sd_ctx* c, const char* name, size_t n, int32_t v, int** d)
{
    const std::vector<int32_t> h(n, v);
    WS(c, int, p, name, n);
    HIPCHK(c, hipMemcpyAsync(p, h.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d = p;
    return SD_OK;
}
// `front` NaNs, n operand floats, `back` NaNs; *d = the first operand float
int up_guarded(sd_ctx* c, const char* name, const float* src, size_t n, size_t front, size_t back, float** d)
{
    std::vector<float> h(front + n + back, QNAN);
    memcpy(h.data() + front, src, n * sizeof(float));
    WS(c, float, p, name, h.size());
    HIPCHK(c, hipMemcpyAsync(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d = p + front;
    return SD_OK;
}
int down(sd_ctx* c, const void* d, size_t bytes, void* h)
{
    if (!h) return SD_OK;
    HIPCHK(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

// the device side of one frontend_prepare call: every table it writes, each [.. + SLACK] and preset to a canary
struct Prep {
    int *prefix, *counts, *nnorm_all, *nvalid_all, *alist, *nact, *nnorm, *nvalid, *flags, *cidx;
    float* lens;
    int n_active;
    std::vector<int> h_nvalid;
};
int prepare(sd_ctx* c, const float* masks, int64_t items, int64_t first_item, bool compact, int32_t ic, float fc, Prep& P)
{
    int rc;
    float* dM;
    const size_t n = (size_t)items + SLACK;
    if ((rc = up_guarded(c, "tf_masks", masks, (size_t)items * SD_FRAMES, 0, (size_t)SLACK * SD_FRAMES, &dM))) return rc;
    // frontend_prepare's own workspaces
    if ((rc = fill_i(c, "fe_prefix", (size_t)items * 296 + SLACK, ic, &P.prefix))) return rc;
    if ((rc = fill_i(c, "fe_counts", n, ic, &P.counts))) return rc;
    if ((rc = fill_i(c, "fe_nnorm_all", n, ic, &P.nnorm_all))) return rc;
    if ((rc = fill_i(c, "fe_nvalid_all", n, ic, &P.nvalid_all))) return rc;
    if ((rc = fill_i(c, "fe_alist", n, ic, &P.alist))) return rc;
    if ((rc = fill_i(c, "fe_nact", 4, ic, &P.nact))) return rc;
    // its arguments
    if ((rc = fill_f(c, "tf_lens", n, fc, &P.lens))) return rc;
    if ((rc = fill_i(c, "tf_nnorm", n, ic, &P.nnorm))) return rc;
    if ((rc = fill_i(c, "tf_nvalid", n, ic, &P.nvalid))) return rc;
    if ((rc = fill_i(c, "tf_flags", n, ic, &P.flags))) return rc;
    if ((rc = fill_i(c, "tf_cidx", n, ic, &P.cidx))) return rc;
    P.n_active = 0;
    if ((rc = frontend_prepare(c, dM, items, first_item, P.lens, P.nnorm, P.nvalid, P.flags, compact, &P.n_active, compact ? P.cidx : nullptr,
                               compact ? &P.h_nvalid : nullptr))) return rc;
    // the function must have found the reserved tables in place (the kernels wrote where the canaries are)
    if (c->ws["fe_prefix"].as<int>() != P.prefix || c->ws["fe_counts"].as<int>() != P.counts || c->ws["fe_nnorm_all"].as<int>() != P.nnorm_all ||
        c->ws["fe_nvalid_all"].as<int>() != P.nvalid_all || c->ws["fe_alist"].as<int>() != P.alist || c->ws["fe_nact"].as<int>() != P.nact)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend: frontend_prepare moved a workspace the hook had reserved");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}
}

extern "C" int sd_test_frontend_prepare(sd_ctx* c, const float* masks, int64_t items, int64_t first_item, int compact, int32_t icanary, float fcanary,
                                        int32_t* prefix, int32_t* counts, float* wav_lens, int32_t* nnorm, int32_t* nvalid, int32_t* flags, int32_t* alist,
                                        int32_t* cidx, int32_t* nnorm_c, int32_t* nvalid_c, int32_t* n_active)
{
    if (!c || !masks || !prefix || !counts || !wav_lens || !nnorm || !nvalid || !flags) return SD_ERR_ARG;
    if (compact && (!alist || !cidx || !nnorm_c || !nvalid_c || !n_active)) return SD_ERR_ARG;
    ENTER(c);
    if (items < 1 || items > (1 << 20)) SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_prepare: items %lld", (long long)items);
    Prep P;
    int rc;
    if ((rc = prepare(c, masks, items, first_item, compact != 0, icanary, fcanary, P))) return rc;
    const size_t n = (size_t)items + SLACK, nb = n * sizeof(int32_t);
    if ((rc = down(c, P.prefix, ((size_t)items * 296 + SLACK) * sizeof(int32_t), prefix))) return rc;
    if ((rc = down(c, P.counts, nb, counts))) return rc;
    if ((rc = down(c, P.lens, n * sizeof(float), wav_lens))) return rc;
    if ((rc = down(c, P.flags, nb, flags))) return rc;
    // per item: the function's own arrays without compaction, its two workspaces with it
    if ((rc = down(c, compact ? P.nnorm_all : P.nnorm, nb, nnorm))) return rc;
    if ((rc = down(c, compact ? P.nvalid_all : P.nvalid, nb, nvalid))) return rc;
    if (compact) {
        if ((rc = down(c, P.alist, nb, alist))) return rc;
        if ((rc = down(c, P.cidx, nb, cidx))) return rc;
        if ((rc = down(c, P.nnorm, nb, nnorm_c))) return rc;
        if ((rc = down(c, P.nvalid, nb, nvalid_c))) return rc;
        if ((rc = down(c, P.nact, 4 * sizeof(int32_t), n_active))) return rc;
        if (n_active[0] != P.n_active) SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_prepare: the function reports %d live items, the device %d", P.n_active, n_active[0]);
    }
    return SD_OK;
}

namespace {
// ecapa_row_plan at option skip_dead_rows = skip for this call, the canary feature buffer, frontend_features, and everything back
int features(sd_ctx* c, const DevWav& w, int64_t first_item, int64_t run_items, bool compact, bool sig_mode, const std::vector<int>& h_nvalid, const int* d_nnorm,
             int skip, float canary, float* feats_out, int64_t feat_rows, int32_t* rowoff_out, int64_t* info_out)
{
    int rc;
    int* d_rowoff;
    if ((rc = fill_i(c, "tf_rowoff", EC_SPACES * ((size_t)run_items + 1) + SLACK, 0, &d_rowoff))) return rc;
    EcapaRowPlan plan;
    const bool keep = c->skip_dead_rows;
    c->skip_dead_rows = skip != 0;
    rc = ecapa_row_plan(c, h_nvalid.data(), run_items, plan, d_rowoff);
    c->skip_dead_rows = keep;
    if (rc) return rc;
    const int64_t rows_all = plan.off[0][(size_t)run_items];
    info_out[0] = run_items; info_out[1] = rows_all; info_out[2] = 0; info_out[3] = c->num_cu;
    if (feat_rows != rows_all + SLACK) SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend: the plan stores %lld rows, the caller expects %lld", (long long)rows_all, (long long)(feat_rows - SLACK));
    float* dF;
    if ((rc = fill_f(c, "tf_feats", (size_t)feat_rows * SD_FEAT_LD, canary, &dF))) return rc;
    c->fe_bill_samples = -1;
    c->fe_last_grid = 0;
    if ((rc = frontend_features(c, w, first_item, run_items, compact, d_nnorm, d_rowoff, dF, sig_mode))) return rc;
    info_out[2] = c->fe_last_grid;                          // what the launch used
    if ((rc = down(c, dF, (size_t)feat_rows * SD_FEAT_LD * sizeof(float), feats_out))) return rc;
    return down(c, d_rowoff, ((size_t)run_items + 1) * sizeof(int32_t), rowoff_out);
}
}

extern "C" int sd_test_frontend_features(sd_ctx* c, const float* wav, int64_t n_held, int64_t n_total, int64_t origin, int64_t first_item, const float* masks,
                                         int64_t items, int skip_dead_rows, float canary, float* feats_out, int64_t feat_rows, int32_t* rowoff_out,
                                         int32_t* cidx_out, int64_t* info_out)
{
    if (!c || !wav || !masks || !feats_out || !rowoff_out || !cidx_out || !info_out) return SD_ERR_ARG;
    ENTER(c);
    if (items < 1 || items > (1 << 16) || n_held < 1 || origin < 0 || origin + n_held > n_total || first_item < 0 || feat_rows < SLACK)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_features: items %lld, slice [%lld, +%lld) of %lld", (long long)items, (long long)origin, (long long)n_held, (long long)n_total);
    Prep P;
    int rc;
    if ((rc = prepare(c, masks, items, first_item, true, -7776, canary, P))) return rc;
    if ((rc = down(c, P.cidx, (size_t)items * sizeof(int32_t), cidx_out))) return rc;
    // samples the kernel is defined to read: of every live item, what its chunk holds of the recording
    int64_t lo = n_total, hi = 0;
    for (int64_t i = 0; i < items; ++i) {
        if (cidx_out[i] < 0) continue;
        const int64_t start = ((first_item + i) / SD_SPEAKERS) * (int64_t)SD_HOP;
        lo = std::min(lo, start);
        hi = std::max(hi, std::min(n_total, start + SD_CHUNK));
    }
    if (P.n_active > 0 && (lo < origin || hi > origin + n_held))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_features: the live items read samples [%lld, %lld), the slice holds [%lld, %lld)", (long long)lo, (long long)hi, (long long)origin, (long long)(origin + n_held));
    if (P.n_active == 0) {              // run_embed launches nothing more
        info_out[0] = 0; info_out[1] = 0; info_out[2] = 0; info_out[3] = c->num_cu;
        rowoff_out[0] = 0;
        if (feat_rows != SLACK) SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_features: no live item, the caller expects %lld rows", (long long)(feat_rows - SLACK));
        for (int64_t k = 0; k < feat_rows * SD_FEAT_LD; ++k) feats_out[k] = canary;
        return SD_OK;
    }
    float* dW;
    if ((rc = up_guarded(c, "tf_wav", wav, (size_t)n_held, SLACK, SLACK, &dW))) return rc;
    DevWav w{dW, n_total};
    w.origin = origin;
    return features(c, w, first_item, P.n_active, true, false, P.h_nvalid, P.nnorm, skip_dead_rows, canary, feats_out, feat_rows, rowoff_out, info_out);
}

extern "C" int sd_test_frontend_signals(sd_ctx* c, const float* signals, const float* wav_lens, int64_t B, int skip_dead_rows, int32_t icanary, float canary,
                                        int32_t* prefix_out, int32_t* counts_out, float* feats_out, int64_t feat_rows, int32_t* rowoff_out, int64_t* info_out)
{
    if (!c || !signals || !wav_lens || !prefix_out || !counts_out || !feats_out || !rowoff_out || !info_out) return SD_ERR_ARG;
    ENTER(c);
    if (B < 1 || B > (1 << 12) || feat_rows < SLACK) SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_signals: B %lld", (long long)B);
    if (!c->ew.loaded) SD_FAIL(c, SD_ERR_MODEL, "embedding model not loaded");
    int rc;
    std::vector<int> nv, nn;
    if ((rc = embed_signals_frames(c, wav_lens, B, nv, nn))) return rc;
    const int64_t ns = B * (int64_t)SD_CHUNK;
    float* dW;
    int* dn;
    if ((rc = up_guarded(c, "tf_wav", signals, (size_t)ns, SLACK, SLACK, &dW))) return rc;
    if ((rc = fill_i(c, "tf_nnorm", (size_t)B + SLACK, 0, &dn))) return rc;
    HIPCHK(c, hipMemcpyAsync(dn, nn.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the identity tables, in reserved workspaces as above
    int *dp, *dc;
    if ((rc = fill_i(c, "fe_prefix", (size_t)B * 296 + SLACK, icanary, &dp))) return rc;
    if ((rc = fill_i(c, "fe_counts", (size_t)B + SLACK, icanary, &dc))) return rc;
    if ((rc = frontend_prepare_signals(c, B))) return rc;
    if (c->ws["fe_prefix"].as<int>() != dp || c->ws["fe_counts"].as<int>() != dc)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_frontend_signals: frontend_prepare_signals moved a workspace the hook had reserved");
    if ((rc = down(c, dp, ((size_t)B * 296 + SLACK) * sizeof(int32_t), prefix_out))) return rc;
    if ((rc = down(c, dc, ((size_t)B + SLACK) * sizeof(int32_t), counts_out))) return rc;
    return features(c, DevWav{dW, ns}, 0, B, false, true, nv, dn, skip_dead_rows, canary, feats_out, feat_rows, rowoff_out, info_out);
}
