// api.cpp -- the C ABI of libsdhip.so (include/sdhip.h): context and options, host-buffer wrappers
// around the embedding stage, the wav reader's four entries (the reader itself: wav_file.h), output formats and the measurement hooks.
// (The other stage wrappers and the whole-path driver are in pipeline.cpp.)
#include "common.h"
#include "many_plan.h"
#include "wav_file.h"
#include "roster.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <fstream>
#include <tuple>

static std::string g_create_err;

int seg_prec(const sd_ctx* c) { return c->seg_precision >= 0 ? c->seg_precision : (c->ecapa_precision != 0 ? 3 : 0); }

extern "C" const char* sd_create_error(void) { return g_create_err.c_str(); }
extern "C" const char* sd_last_error(const sd_ctx* c) { return c ? c->err.c_str() : "null context"; }

extern "C" sd_ctx* sd_create(const char* seg_path, const char* emb_path, int device)
{
    g_create_err.clear();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_create_err = "no HIP device available (libsdhip has no CPU fallback)"; return nullptr; }
    if (device < 0 || device >= ndev) { g_create_err = "device id out of range"; return nullptr; }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return nullptr; }
    sd_ctx* c = new sd_ctx();
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->num_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { g_create_err = "hipStreamCreate failed"; delete c; return nullptr; }
    auto fail = [&](const std::string& m) { g_create_err = m; sd_destroy(c); return (sd_ctx*)nullptr; };
    const bool trace = getenv("SD_TRACE_CREATE") != nullptr;          // where the start-up time goes (tools/cold_start.py)
    double t0 = now_ms();
    if (seg_path && seg_path[0]) {
        Pack p; std::string e;
        if (load_model_any(seg_path, 0, p, e)) return fail(e);
        const double t1 = now_ms();
        if (build_seg_weights(c, p)) return fail(c->err);
        if (trace) fprintf(stderr, "sd_create: segmentation model read %.1f ms, layouts + upload %.1f ms\n", t1 - t0, now_ms() - t1);
    }
    t0 = now_ms();
    if (emb_path && emb_path[0]) {
        Pack p; std::string e;
        if (load_model_any(emb_path, 1, p, e)) return fail(e);
        const double t1 = now_ms();
        if (build_ecapa_weights(c, p)) return fail(c->err);
        if (trace) fprintf(stderr, "sd_create: embedding model read %.1f ms, layouts + upload %.1f ms\n", t1 - t0, now_ms() - t1);
    }
    c->err.clear();
    return c;
}

extern "C" void sd_destroy(sd_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    sd_flush_profile(c);
    (void)sd_comm_destroy(c);
    while (!c->streams.empty()) sd_stream_close(c->streams.back());      // streams still open own device memory of their own
    while (!c->cuts.empty()) sd_cut_close(c->cuts.back());               // ... and so do cuts
    for (void* p : c->owned) (void)hipFree(p);
    for (auto& kv : c->ws) kv.second.release();
    c->enr_gal.release(); c->enr_m2.release();
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

void sd_flush_profile(sd_ctx* c)
{
    for (auto& t : c->pending) {
        hipEvent_t e0 = std::get<1>(t), e1 = std::get<2>(t);
        float ms = 0;
        if (hipEventSynchronize(e1) == hipSuccess) (void)hipEventElapsedTime(&ms, e0, e1);
        KernelStat& s = c->stats[std::get<0>(t)];
        s.ms += ms; s.launches++; s.flops += std::get<3>(t); s.bytes += std::get<4>(t);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    c->pending.clear();
}

extern "C" int sd_kernel_stats(const sd_ctx* cc, const char* kernel, double* total_ms, int64_t* launches, double* flops, double* bytes)
{
    sd_ctx* c = const_cast<sd_ctx*>(cc);
    if (!c || !kernel) return SD_ERR_ARG;
    (void)hipStreamSynchronize(c->stream);
    sd_flush_profile(c);
    auto it = c->stats.find(kernel);
    KernelStat s; if (it != c->stats.end()) s = it->second;
    if (total_ms) *total_ms = s.ms; if (launches) *launches = s.launches; if (flops) *flops = s.flops; if (bytes) *bytes = s.bytes;
    return SD_OK;
}
// test hook: copy `bytes` of the named workspace (from `offset`) to the host -- intermediate activations for the precision diagnostics of tools/
extern "C" int sd_debug_read_ws(sd_ctx* c, const char* name, int64_t offset, void* h_out, int64_t bytes)
{
    if (!c || !name || !h_out || offset < 0 || bytes < 0) return SD_ERR_ARG;
    auto it = c->ws.find(name);
    if (it == c->ws.end() || !it->second.p) SD_FAIL(c, SD_ERR_ARG, "no workspace named %s", name);
    if ((size_t)(offset + bytes) > it->second.cap) SD_FAIL(c, SD_ERR_ARG, "workspace %s holds %zu bytes", name, it->second.cap);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_out, (const char*)it->second.p + offset, (size_t)bytes, hipMemcpyDeviceToHost));
    return SD_OK;
}
extern "C" void sd_reset_stats(sd_ctx* c) { if (!c) return; (void)hipStreamSynchronize(c->stream); sd_flush_profile(c); c->stats.clear(); }
extern "C" int sd_stage_ms(const sd_ctx* c, double* ms4) { if (!c || !ms4) return SD_ERR_ARG; for (int i = 0; i < 4; ++i) ms4[i] = c->stage_ms[i]; return SD_OK; }
extern "C" int sd_set_option(sd_ctx* c, const char* key, int64_t v)
{
    if (!c || !key) return SD_ERR_ARG;
    std::string k(key);
    if (k == "emb_batch_items") { c->emb_batch_items = v; c->emb_batch_explicit = true; }
    else if (k == "seg_batch_chunks") c->seg_batch_chunks = v;
    else if (k == "ws_limit_mb") g_ws_limit.store(v > 0 ? (size_t)v << 20 : 0);      // test hook, process-wide (sdhip_test.h)
    else if (k == "emb_batch_default") { c->emb_batch_items = 3072; c->emb_batch_explicit = false; c->embed_calls = v; }   // test hook: back to the implicit plan (v = calls already made)
    else if (k == "linkage_wgs") c->linkage_wgs = v;
    else if (k == "linkage_threads") c->linkage_threads = v;
    else if (k == "linkage_kernel") c->linkage_kernel = v;
    else if (k == "linkage_tie_kernel") c->linkage_tie_kernel = v;
    else if (k == "linkage_zero_phase") c->linkage_zero_phase = v;
    else if (k == "linkage_force_heap") c->linkage_force_heap = v != 0;
    else if (k == "linkage_hx_wide") c->linkage_hx_wide = v != 0;
    else if (k == "linkage_prefetch") c->linkage_prefetch = v != 0;
    else if (k == "linkage_one_xcd") c->linkage_one_xcd = v;
    else if (k == "linkage_square") c->linkage_square = v;
    else if (k == "linkage_batch") { if (v != 0 && v != 1) SD_FAIL(c, SD_ERR_ARG, "linkage_batch must be 0 or 1"); c->linkage_batch = v; }
    else if (k == "linkage_batch_xcd") { if (v != 0 && v != 1) SD_FAIL(c, SD_ERR_ARG, "linkage_batch_xcd must be 0 or 1"); c->linkage_batch_xcd = v; }
    else if (k == "linkage_batch_xcd_zero") { if (v != 0 && v != 1) SD_FAIL(c, SD_ERR_ARG, "linkage_batch_xcd_zero must be 0 or 1"); c->linkage_batch_xcd_zero = v; }
    else if (k == "linkage_batch_bytes") { if (v < 1) SD_FAIL(c, SD_ERR_ARG, "linkage_batch_bytes must be at least 1"); c->linkage_batch_bytes = v; }
    else if (k == "linkage_batch_threads") { if (v != 0 && v != 256 && v != 1024) SD_FAIL(c, SD_ERR_ARG, "linkage_batch_threads must be 0 (auto), 256 or 1024"); c->linkage_batch_threads = v; }
    else if (k == "skip_dead_rows") c->skip_dead_rows = v != 0;
    else if (k == "conv_h256") c->conv_h256 = v != 0;
    else if (k == "conv_glds") c->conv_glds = v != 0;
    else if (k == "conv_pp") c->conv_pp = v != 0;
    else if (k == "conv_glds_f32") c->conv_glds_f32 = v != 0;
    else if (k == "conv_mfma16") { if (v < 0 || v > 2) return SD_ERR_ARG; c->conv_mfma16 = (int)v; }      // 2: k_conv_gemm_g256 takes the 16x16x32 form on short contractions too (the reference the round-6 kernel is compared with bit for bit)
    else if (k == "conv_rot") { if (v < 0 || v > 3) return SD_ERR_ARG; c->conv_rot = (int)v; }
    else if (k == "conv_stagger") { if (v < 0 || v > 2) return SD_ERR_ARG; c->conv_stagger = (int)v; }
    else if (k == "conv_w256_f32") c->conv_w256_f32 = v != 0;
    else if (k == "conv_res2_ws") c->conv_res2_ws = v != 0;      // f32 Res2Net convs on the weight-stationary kernel (conv_res2.hip); 0 = the 128 x 128 kernel; same bits
    else if (k == "conv_res2_wgs") { if (v < 0 || v > 4096) return SD_ERR_ARG; c->conv_res2_wgs = (int)v; }
    else if (k == "conv_pn") c->conv_pn = (int)v;
    else if (k == "ecapa_ld_pad") { if (v < 0 || v > 1024 || ((int64_t)v & 7)) return SD_ERR_ARG; c->ecapa_ld_pad = (int)v; }
    else if (k == "seg_shared_conv0") c->seg_shared_conv0 = v != 0;
    else if (k == "seg_wide_ih") c->seg_wide_ih = v != 0;
    else if (k == "conv_w256_kmin") c->conv_w256_kmin = (int)v;
    else if (k == "conv_pn128") c->conv_pn128 = (int)v;
    else if (k == "seg_precision") { if (v != 0 && v != 3 && v != -1) SD_FAIL(c, SD_ERR_ARG, "seg_precision must be 0 (f32), 3 (split fp16 operands for the LSTM) or -1 (auto: 3 whenever ecapa_precision is not 0)"); c->seg_precision = (int)v; }
    else if (k == "ecapa_precision") { if (v < 0 || v > 3) SD_FAIL(c, SD_ERR_ARG, "ecapa_precision must be 0 (f32), 1 (fp16), 2 (fp16, hi + lo weight planes) or 3 (f32 tensors, split fp16 operands on the wide layers)");
                                        if (hipSetDevice(c->device) != hipSuccess) SD_FAIL(c, SD_ERR_HIP, "hipSetDevice failed");
                                        const int rcw = ensure_ecapa_mode_weights(c, (int)v); if (rcw) return rcw;      // fp16 weight forms: built on first use of the mode
                                        c->ecapa_precision = (int)v; }
    else if (k == "ecapa_f16_hp") { if (v != 0 && v != 1 && v != 3) SD_FAIL(c, SD_ERR_ARG, "ecapa_f16_hp must be 0, 1 (MFA output in f32) or 3 (+ the attention branch)"); c->ecapa_f16_hp = (int)v; }
    else if (k == "ecapa_keep_cat") c->ecapa_keep_cat = v != 0;
    else if (k == "rank0_permille") c->rank0_permille = (int)v;
    else if (k == "virtual_world") c->virtual_world = (int)v;
    else if (k == "comm_timeout_ms") c->comm_timeout_ms = v;
    else if (k == "inject_fail_rank") c->inject_fail_rank = (int)v;
    else if (k == "constrained_assignment") c->constrained_assignment = v != 0;
    else if (k == "clustering_method") { if (v < SD_LINKAGE_SINGLE || v > SD_LINKAGE_WEIGHTED) SD_FAIL(c, SD_ERR_ARG, "clustering_method must be one of SD_LINKAGE_SINGLE (0) .. SD_LINKAGE_WEIGHTED (6)"); c->clustering_method = (int)v; }
    else if (k == "min_cluster_size") { if (v < 1 || v > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "min_cluster_size must be at least 1"); c->min_cluster_size = (int)v; }
    else if (k == "max_num_embeddings") { if (v != -1 && v < 1) SD_FAIL(c, SD_ERR_ARG, "max_num_embeddings must be -1 (every train row) or at least 1"); c->max_num_embeddings = v; }
    else if (k == "clustering_seed") c->clustering_seed = v;
    else if (k == "num_clusters") c->num_clusters = (int)v;
    else if (k == "min_clusters") c->min_clusters = (int)v;
    else if (k == "max_clusters") c->max_clusters = (int)v;
    else if (k == "activity_hamming") { if (v != 0 && v != 1) SD_FAIL(c, SD_ERR_ARG, "activity_hamming must be 0 or 1"); c->activity_hamming = v != 0; }
    else if (k == "cut_group_bytes") { if (v < 1) SD_FAIL(c, SD_ERR_ARG, "cut_group_bytes must be at least 1"); c->cut_group_bytes = v; }      // test key (sdhip_test.h)
    else if (k == "profile") { c->profile = v != 0; c->profile_detail = v >= 2; }
    else SD_FAIL(c, SD_ERR_ARG, "unknown option %s", key);
    return SD_OK;
}

extern "C" int sd_set_option_f64(sd_ctx* c, const char* key, double v)
{
    if (!c || !key) return SD_ERR_ARG;
    std::string k(key);
    if (k == "clustering_threshold") { if (!(v >= 0.0 && v <= 2.0)) SD_FAIL(c, SD_ERR_ARG, "clustering_threshold must lie in [0, 2]"); c->clustering_threshold = v; }
    else if (k == "activity_onset") { if (!(v >= 0.0 && v <= 1.0)) SD_FAIL(c, SD_ERR_ARG, "activity_onset must lie in [0, 1]"); c->activity_onset = v; }
    else if (k == "activity_offset") { if (!(v >= 0.0 && v <= 1.0)) SD_FAIL(c, SD_ERR_ARG, "activity_offset must lie in [0, 1]"); c->activity_offset = v; }
    else if (k == "activity_min_duration_on") { if (!(v >= 0.0)) SD_FAIL(c, SD_ERR_ARG, "activity_min_duration_on must be >= 0"); c->activity_min_on = v; }
    else if (k == "activity_min_duration_off") { if (!(v >= 0.0)) SD_FAIL(c, SD_ERR_ARG, "activity_min_duration_off must be >= 0"); c->activity_min_off = v; }
    else if (k == "speaker_match_threshold") { if (!(v >= 0.0 && v <= 2.0)) SD_FAIL(c, SD_ERR_ARG, "speaker_match_threshold must lie in [0, 2]"); c->speaker_match_threshold = v; }
    else SD_FAIL(c, SD_ERR_ARG, "unknown real-valued option %s", key);
    return SD_OK;
}
extern "C" int sd_linkage_method_from_name(const char* name)
{
    static const char* const names[] = {"single", "complete", "average", "centroid", "median", "ward", "weighted"};      // scipy's codes = SD_LINKAGE_*
    if (!name) return -1;
    for (int i = 0; i < 7; ++i) if (std::string(name) == names[i]) return i;
    return -1;
}

// ------------------------------------------------------------------ helpers
extern "C" int64_t sd_num_chunks(int64_t n, int64_t* last_len) { return sd_chunk_rule(n, last_len); }      // many_plan.h: the one statement of the rule

// host-only: the rule of "max_num_embeddings" on a list of rows, through the function train_rows (cluster.hip) applies
extern "C" int64_t sd_sample_rows(const int32_t* rows, int64_t n, int64_t max_num, int64_t seed, int32_t* out)
{
    if (n < 0 || (n > 0 && (!rows || !out)) || (max_num != -1 && max_num < 1)) return -SD_ERR_ARG;
    for (int64_t q = 0; q < n; ++q) if (rows[q] < 0 || (q > 0 && rows[q] <= rows[q - 1])) return -SD_ERR_ARG;      // ascending and distinct: distinct keys
    std::vector<int32_t> kept;
    const int64_t m = sample_rows(rows, n, max_num, seed, kept);
    for (int64_t q = 0; q < m; ++q) out[q] = kept[(size_t)q];
    return m;
}

// ------------------------------------------------------------------ embedding path
extern "C" int sd_embed_dev(sd_ctx* c, const float* d_wav, int64_t n, const float* d_masks, int64_t items, int64_t first_item, float* d_emb)
{
    ENTER(c);
    if (!d_wav || !d_masks || !d_emb || n <= 0 || items < 0) SD_FAIL(c, SD_ERR_ARG, "sd_embed_dev: bad argument");
    int rc = run_embed(c, DevWav{d_wav, n}, d_masks, items, first_item, d_emb);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

extern "C" int sd_embed(sd_ctx* c, const float* h_wav, int64_t n, const float* h_masks, int64_t items, float* h_emb)
{
    ENTER(c);
    if (!h_wav || !h_masks || !h_emb || n <= 0 || items < 0) SD_FAIL(c, SD_ERR_ARG, "sd_embed: bad argument");
    DTMP(c, dw, n * sizeof(float)); DTMP(c, dm, items * SD_FRAMES * sizeof(float)); DTMP(c, de, items * SD_EMB_DIM * sizeof(float));
    HIPCHK(c, hipMemcpy(dw.p, h_wav, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dm.p, h_masks, items * SD_FRAMES * sizeof(float), hipMemcpyHostToDevice));
    int rc = run_embed(c, DevWav{(const float*)dw.p, n}, (const float*)dm.p, items, 0, (float*)de.p);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_emb, de.p, items * SD_EMB_DIM * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}

extern "C" int sd_frontend(sd_ctx* c, const float* h_wav, int64_t n, const float* h_masks, int64_t items, float* h_feats, float* h_lens)
{
    ENTER(c);
    if (!h_wav || !h_masks || n <= 0 || items <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_frontend: bad argument");
    DTMP(c, dw, n * sizeof(float)); DTMP(c, dm, items * SD_FRAMES * sizeof(float));
    DTMP(c, df, items * SD_TP * SD_FEAT_LD * sizeof(float)); DTMP(c, dl, items * sizeof(float));
    DTMP(c, dn, items * sizeof(int)); DTMP(c, dv, items * sizeof(int)); DTMP(c, dg, items * sizeof(int)); DTMP(c, dr, (items + 1) * sizeof(int));
    HIPCHK(c, hipMemcpy(dw.p, h_wav, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dm.p, h_masks, items * SD_FRAMES * sizeof(float), hipMemcpyHostToDevice));
    std::vector<int> ro((size_t)items + 1);
    for (int64_t i = 0; i <= items; ++i) ro[(size_t)i] = (int)(i * SD_TP);                  // every frame of every item (reference layout)
    HIPCHK(c, hipMemcpy(dr.p, ro.data(), ro.size() * sizeof(int), hipMemcpyHostToDevice));
    int rc = frontend_prepare(c, (const float*)dm.p, items, 0, (float*)dl.p, (int*)dn.p, (int*)dv.p, (int*)dg.p, false, nullptr, nullptr);
    if (rc) return rc;
    if ((rc = frontend_features(c, DevWav{(const float*)dw.p, n}, 0, items, false, (const int*)dn.p, (const int*)dr.p, (float*)df.p))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_feats) {
        std::vector<float> tmp((size_t)items * SD_TP * SD_FEAT_LD);
        HIPCHK(c, hipMemcpy(tmp.data(), df.p, tmp.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < items; ++i)
            for (int t = 0; t < SD_T; ++t)
                memcpy(h_feats + ((size_t)i * SD_T + t) * SD_NMELS, &tmp[((size_t)i * SD_TP + t) * SD_FEAT_LD], SD_NMELS * sizeof(float));
    }
    if (h_lens) HIPCHK(c, hipMemcpy(h_lens, dl.p, items * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}

extern "C" int sd_ecapa(sd_ctx* c, const float* h_feats, const float* h_lens, int64_t items, float* h_emb)
{
    ENTER(c);
    if (!h_feats || !h_lens || !h_emb || items <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_ecapa: bad argument");
    std::vector<int> nv((size_t)items);
    EcapaRowPlan plan;
    for (int64_t i = 0; i < items; ++i) {
        float lt = h_lens[i] * (float)SD_T;
        int v = (int)ceilf(lt); if (v > SD_T) v = SD_T; if (v < 1) v = 1;
        nv[(size_t)i] = v;
    }
    DTMP(c, dv, items * sizeof(int)); DTMP(c, dr, EC_SPACES * (items + 1) * sizeof(int)); DTMP(c, de, items * SD_EMB_DIM * sizeof(float));
    int rc = ecapa_row_plan(c, nv.data(), items, plan, (int*)dr.p);
    if (rc) return rc;
    const std::vector<int>& rowoff = plan.off[0];
    const int64_t rows = rowoff[(size_t)items];
    std::vector<float> tmp((size_t)rows * SD_FEAT_LD, 0.0f);                                 // compact rows: the frames each item needs
    for (int64_t i = 0; i < items; ++i)
        for (int t = 0; t < rowoff[(size_t)i + 1] - rowoff[(size_t)i]; ++t)
            memcpy(&tmp[((size_t)rowoff[(size_t)i] + t) * SD_FEAT_LD], h_feats + ((size_t)i * SD_T + t) * SD_NMELS, SD_NMELS * sizeof(float));
    DTMP(c, df, tmp.size() * sizeof(float));
    HIPCHK(c, hipMemcpy(df.p, tmp.data(), tmp.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dv.p, nv.data(), items * sizeof(int), hipMemcpyHostToDevice));
    if ((rc = ecapa_run_items(c, (const float*)df.p, (const int*)dv.p, plan, c->emb_batch_items, false, (float*)de.p))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_emb, de.p, items * SD_EMB_DIM * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}

// the frames wav_lens leaves an item of sd_embed_signals: nv = frames the network reads, nn = frames the mean runs over; refuses a length outside (0, 1]
// or one that rounds to no frame at all
int embed_signals_frames(sd_ctx* c, const float* h_wav_lens, int64_t B, std::vector<int>& nv, std::vector<int>& nn)
{
    nv.assign((size_t)B, 0); nn.assign((size_t)B, 0);
    for (int64_t i = 0; i < B; ++i) {
        if (!(h_wav_lens[i] > 0.0f) || h_wav_lens[i] > 1.0f) SD_FAIL(c, SD_ERR_ARG, "sd_embed_signals: wav_lens[%lld] = %g (relative length in (0, 1])", (long long)i, (double)h_wav_lens[i]);
        const float lt = h_wav_lens[i] * (float)SD_T;                       // float32 product as in torch (k_wav_lens)
        nn[(size_t)i] = (int)rintf(lt);                                      // torch.round, threeModel.py:358
        int v = (int)ceilf(lt); if (v > SD_T) v = SD_T; if (v < 1) v = 1;    // arange(L) < len * L
        nv[(size_t)i] = v;
        if (nn[(size_t)i] < 1) SD_FAIL(c, SD_ERR_ARG, "sd_embed_signals: wav_lens[%lld] = %g leaves no frame to normalise over", (long long)i, (double)h_wav_lens[i]);
    }
    return SD_OK;
}

// EmbeddingModel1::infer as the reference declares it (sd.cpp:1977-2040, calling _infer sd.cpp:1889-1970): B already compacted, zero-padded
// signals of 80000 samples and their relative lengths -> [B][192].  No NaN rule here (getEmbedding applies it to the result, sd.cpp:2479-2549);
// the STFT / fbank run over all 501 frames of every row as the reference's do, the network over the frames wav_lens leaves valid + its reach.
extern "C" int sd_embed_signals(sd_ctx* c, const float* h_signals, const float* h_wav_lens, int64_t B, float* h_emb)
{
    ENTER(c);
    if (!h_signals || !h_wav_lens || !h_emb || B <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_embed_signals: bad argument");
    if (!c->ew.loaded) SD_FAIL(c, SD_ERR_MODEL, "embedding model not loaded");
    std::vector<int> nv, nn;
    if (const int rc = embed_signals_frames(c, h_wav_lens, B, nv, nn)) return rc;
    const int64_t ns = B * (int64_t)SD_CHUNK;
    // persistent workspaces, not per-call allocations: the reference calls infer once per batch of 32 items (677 times per hour of audio)
    WS(c, float, dw, "sig_wav", ns + SD_WAV_PAD); WS(c, int, dv, "sig_nvalid", B); WS(c, int, dn, "sig_nnorm", B);
    WS(c, int, dr, "sig_rowoff", EC_SPACES * (B + 1)); WS(c, float, de, "sig_emb", B * SD_EMB_DIM);
    HIPCHK(c, hipMemcpyAsync(dw, h_signals, ns * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dw + ns, 0, SD_WAV_PAD * sizeof(float), c->stream));
    HIPCHK(c, hipMemcpyAsync(dv, nv.data(), B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dn, nn.data(), B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    EcapaRowPlan plan;
    int rc = ecapa_row_plan(c, nv.data(), B, plan, dr);          // (synchronises the stream: the host vectors above may go)
    if (rc) return rc;
    WS(c, float, df, "sig_feats", (size_t)plan.off[0][(size_t)B] * SD_FEAT_LD);
    if ((rc = frontend_prepare_signals(c, B))) return rc;
    c->fe_bill_samples = -1;
    if ((rc = frontend_features(c, DevWav{dw, ns, 0, true}, 0, B, false, dn, dr, df, true))) return rc;
    const int64_t nb = c->emb_batch_explicit ? c->emb_batch_items : std::min<int64_t>(c->emb_batch_items, 768);      // an operator-level call: the small arena
    if ((rc = ecapa_run_items(c, df, dv, plan, nb, false, de))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_emb, de, B * SD_EMB_DIM * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}

// ------------------------------------------------------------------ wav reader (a1): wav_file.h behind the C ABI
extern "C" int sd_read_wav(const char* path, int16_t** pcm, int64_t* n, int32_t* sample_rate, int32_t* channels)
{
    return wav_read_pcm16(path, pcm, n, sample_rate, channels);
}
extern "C" void sd_free_pcm(int16_t* p) { free(p); }
extern "C" void sd_free_turns(sd_turn* t) { free(t); }
extern "C" int sd_format_turn(const sd_turn* t, char* buf, int cap)
{
    if (!t || !buf) return SD_ERR_ARG;
    snprintf(buf, (size_t)cap, "[%g -- %g] --> Speaker_%d", t->start, t->end, t->label);   // sd.cpp:3439, iostream default precision
    return SD_OK;
}

extern "C" int sd_read_wav_f32(const char* path, float** wav, int64_t* n, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample)
{
    return wav_read_f32(path, wav, n, sample_rate, channels, bits_per_sample);
}
extern "C" void sd_free_wav(float* p) { free(p); }
extern "C" int sd_read_wav_audio(const char* path, sd_audio* desc, void** data) { return wav_read_audio(path, desc, data); }

// ------------------------------------------------------------------ output formats
// Relabelling.  The reference prints the raw cluster index (sd.cpp:3439).  pyannote.audio renames the clusters on the way
// out: SpeakerDiarization.apply maps `diarization.labels()` -- the labels that occur, sorted BY THEIR STRING -- onto
// SPEAKER_00, SPEAKER_01, ... (mode 1); mode 0 numbers the speakers in order of first appearance.
extern "C" int sd_relabel_turns_ex(sd_turn* turns, int64_t n, int mode)
{
    if (n < 0 || (n > 0 && !turns) || (mode != 0 && mode != 1)) return SD_ERR_ARG;
    std::vector<int> seen;
    for (int64_t i = 0; i < n; ++i) if (std::find(seen.begin(), seen.end(), turns[i].label) == seen.end()) seen.push_back(turns[i].label);
    if (mode == 1) std::sort(seen.begin(), seen.end(), [](int a, int b) { return std::to_string(a) < std::to_string(b); });
    for (int64_t i = 0; i < n; ++i) turns[i].label = (int32_t)(std::find(seen.begin(), seen.end(), turns[i].label) - seen.begin());
    return SD_OK;
}
extern "C" int sd_relabel_turns(sd_turn* turns, int64_t n) { return sd_relabel_turns_ex(turns, n, 1); }

extern "C" int sd_last_confidence(const sd_ctx* c, double* conf, int64_t cap, int64_t* n)
{
    if (!c) return SD_ERR_ARG;
    if (n) *n = (int64_t)c->last.conf.size();
    if (conf) for (int64_t i = 0; i < cap && i < (int64_t)c->last.conf.size(); ++i) conf[i] = c->last.conf[(size_t)i];
    return SD_OK;
}

extern "C" int sd_last_activity_scores(const sd_ctx* c, double* scores, int64_t cap, int64_t* n)
{
    if (!c) return SD_ERR_ARG;
    if (n) *n = (int64_t)c->last_activity.size();
    if (scores) for (int64_t i = 0; i < cap && i < (int64_t)c->last_activity.size(); ++i) scores[i] = c->last_activity[(size_t)i];
    return SD_OK;
}

// one "SPEAKER <uri> 1 <start> <duration> <NA> <NA> SPEAKER_<kk> <NA> <conf>" line per turn (pyannote's RTTM writer layout;
// the last field is RTTM's confidence column, <NA> without conf)
extern "C" int sd_write_rttm_ex(const char* path, const char* uri, const sd_turn* turns, int64_t n_turns, const double* conf)
{
    if (!path || (n_turns > 0 && !turns) || n_turns < 0) return SD_ERR_ARG;
    FILE* f = fopen(path, "w");
    if (!f) return SD_ERR_ARG;
    for (int64_t i = 0; i < n_turns; ++i) {
        fprintf(f, "SPEAKER %s 1 %.3f %.3f <NA> <NA> SPEAKER_%02d <NA> ", (uri && uri[0]) ? uri : "audio",
                turns[i].start, turns[i].end - turns[i].start, turns[i].label);
        if (conf && conf[i] == conf[i]) fprintf(f, "%.4f\n", conf[i]); else fprintf(f, "<NA>\n");
    }
    fclose(f);
    return SD_OK;
}
extern "C" int sd_write_rttm(const char* path, const char* uri, const sd_turn* turns, int64_t n_turns)
{
    return sd_write_rttm_ex(path, uri, turns, n_turns, nullptr);
}

// ------------------------------------------------------------------ known speakers: centroids out, gallery matching, voiceprint files
// the K final centroids of the last clustering call of this ctx and the train rows of each (run_clustering keeps them; sd.cpp:2149-2167)
extern "C" int sd_last_speakers(const sd_ctx* c, double* h_centroids, int64_t cap, int64_t* K, int64_t* h_counts)
{
    if (!c || cap < 0) return SD_ERR_ARG;
    const int64_t k = c->last.cen_K, d = c->last.cen_d;
    if (K) *K = k;
    for (int64_t i = 0; i < k && i < cap; ++i) {
        if (h_centroids) memcpy(h_centroids + i * d, &c->last.cen[(size_t)(i * d)], (size_t)d * sizeof(double));
        if (h_counts) h_counts[i] = c->last.cen_counts[(size_t)i];
    }
    return SD_OK;
}

// h_cen (NULL = the last job's centroids, K and d must be theirs) against the gallery -> dist [K][M] in `dist`
static int speaker_dist_host(sd_ctx* c, const double* h_cen, int64_t K, const double* h_gallery, int64_t M, int d, std::vector<double>& dist, const char* who)
{
    if (!h_gallery || K < 1 || M < 1 || d < 1) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument (K, M, d >= 1)", who);
    if (!h_cen) {
        if (c->last.cen_K < 1) SD_FAIL(c, SD_ERR_ARG, "%s: no clustering call on this context yet", who);
        if (K != c->last.cen_K || d != c->last.cen_d) SD_FAIL(c, SD_ERR_ARG, "%s: the last job has %d centroids of %d dimensions, not %lld of %d", who, c->last.cen_K, c->last.cen_d, (long long)K, d);
        h_cen = c->last.cen.data();
    }
    if ((double)K * (double)M > 4e9) SD_FAIL(c, SD_ERR_ARG, "%s: a %lld x %lld table is out of range", who, (long long)K, (long long)M);
    dist.resize((size_t)K * (size_t)M);
    WS(c, double, d_cen, "spk_cen", K * d); WS(c, double, d_gal, "spk_gallery", M * d); WS(c, double, d_dist, "spk_dist", K * M);
    HIPCHK(c, hipMemcpy(d_cen, h_cen, (size_t)K * d * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_gal, h_gallery, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice));
    return run_speaker_dist(c, d_cen, K, d_gal, M, d, d_dist, dist.data());
}

extern "C" int sd_speaker_distances(sd_ctx* c, const double* h_cen, int64_t K, const double* h_gallery, int64_t M, int d, double* h_dist)
{
    ENTER(c);
    if (!h_dist) SD_FAIL(c, SD_ERR_ARG, "sd_speaker_distances: bad argument");
    std::vector<double> dist;
    if (int rc = speaker_dist_host(c, h_cen, K, h_gallery, M, d, dist, "sd_speaker_distances")) return rc;
    memcpy(h_dist, dist.data(), dist.size() * sizeof(double));
    return SD_OK;
}

// greedy one-to-one matching: the pairs with dist <= threshold in (dist, k, m) order, a pair taken when both sides are still free
extern "C" int sd_match_speakers(sd_ctx* c, const double* h_cen, int64_t K, const double* h_gallery, int64_t M, int d, double threshold,
                                 int32_t* h_match, double* h_dist_best)
{
    ENTER(c);
    if (!h_match) SD_FAIL(c, SD_ERR_ARG, "sd_match_speakers: bad argument");
    if (threshold != threshold) threshold = c->speaker_match_threshold;
    else if (!(threshold >= 0.0 && threshold <= 2.0)) SD_FAIL(c, SD_ERR_ARG, "sd_match_speakers: threshold must lie in [0, 2] (NaN = option speaker_match_threshold)");
    if (M > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "sd_match_speakers: gallery too long");
    std::vector<double> dist;
    if (int rc = speaker_dist_host(c, h_cen, K, h_gallery, M, d, dist, "sd_match_speakers")) return rc;
    std::vector<std::tuple<double, int64_t, int64_t>> pairs;
    for (int64_t k = 0; k < K; ++k)
        for (int64_t m = 0; m < M; ++m) { const double v = dist[(size_t)(k * M + m)]; if (v <= threshold) pairs.emplace_back(v, k, m); }
    std::sort(pairs.begin(), pairs.end());
    std::vector<char> taken((size_t)M, 0);
    for (int64_t k = 0; k < K; ++k) { h_match[k] = -1; if (h_dist_best) h_dist_best[k] = NAN; }
    for (const auto& p : pairs) {
        const int64_t k = std::get<1>(p), m = std::get<2>(p);
        if (h_match[k] >= 0 || taken[(size_t)m]) continue;
        h_match[k] = (int32_t)m; taken[(size_t)m] = 1;
        if (h_dist_best) h_dist_best[k] = std::get<0>(p);
    }
    return SD_OK;
}

// ------------------------------------------------------------------ enrolled speakers: the gallery run_clustering consults (cluster.hip), and its first step alone
// every value a number (SD_ERR_ARG), every row with a non-zero sequential sum of squares (SD_ERR_NUMERIC; the reference throws, sd.cpp:493-495)
static int check_gallery(sd_ctx* c, const double* g, int64_t M, int d, const char* who)
{
    for (int64_t m = 0; m < M; ++m) {
        double s = 0.0;
        for (int i = 0; i < d; ++i) { const double v = g[m * d + i]; if (!std::isfinite(v)) SD_FAIL(c, SD_ERR_ARG, "%s: gallery row %lld holds a value that is not a finite number", who, (long long)m); s += v * v; }
        if (s == 0.0) SD_FAIL(c, SD_ERR_NUMERIC, "%s: gallery row %lld has zero magnitude (reference throws, sd.cpp:493-495)", who, (long long)m);
        if (!std::isfinite(s)) SD_FAIL(c, SD_ERR_ARG, "%s: the squared norm of gallery row %lld overflows", who, (long long)m);
    }
    return SD_OK;
}

extern "C" int sd_set_enrolled(sd_ctx* c, const double* h_gallery, int64_t M, int d)
{
    ENTER(c);
    if (!h_gallery || M == 0) {                                              // clear
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->enr_gal.release(); c->enr_m2.release(); c->enr_host.clear(); c->enr_host.shrink_to_fit();
        c->enr_M = 0; c->enr_d = 0;
        return SD_OK;
    }
    if (M < 0 || M > 0x7fffffff || d < 1) SD_FAIL(c, SD_ERR_ARG, "sd_set_enrolled: bad argument (1 <= M < 2^31, d >= 1)");
    if (int rc = check_gallery(c, h_gallery, M, d, "sd_set_enrolled")) return rc;
    DevBuf gal, m2;                                                          // the previous gallery stays until the new one is complete
    if (gal.reserve((size_t)M * d * sizeof(double)) || m2.reserve((size_t)M * sizeof(double))) { gal.release(); m2.release(); SD_FAIL(c, SD_ERR_HIP, "sd_set_enrolled: hipMalloc of the gallery failed"); }
    int rc = SD_OK;
    if (hipMemcpyAsync(gal.p, h_gallery, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) { c->err = "sd_set_enrolled: upload failed"; rc = SD_ERR_HIP; }
    if (!rc) rc = run_gallery_norms(c, gal.as<double>(), M, d, m2.as<double>());
    if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "sd_set_enrolled: hipStreamSynchronize failed"; rc = SD_ERR_HIP; }
    if (rc) { gal.release(); m2.release(); return rc; }
    c->enr_gal.release(); c->enr_m2.release();
    c->enr_gal = gal; c->enr_m2 = m2;
    c->enr_host.assign(h_gallery, h_gallery + (size_t)M * d);
    c->enr_M = M; c->enr_d = d;
    return SD_OK;
}

extern "C" int sd_enrolled_info(const sd_ctx* c, int64_t* M, int* d)
{
    if (!c) return SD_ERR_ARG;
    if (M) *M = c->enr_M;
    if (d) *d = c->enr_d;
    return SD_OK;
}

extern "C" int sd_nearest_speakers(sd_ctx* c, const double* h_X, int64_t N, const double* h_gallery, int64_t M, int d, int32_t* h_best, double* h_dist)
{
    ENTER(c);
    if (!h_X || N < 1 || d < 1) SD_FAIL(c, SD_ERR_ARG, "sd_nearest_speakers: bad argument (N, d >= 1)");
    const double* d_gal; const double* d_m2;
    if (!h_gallery) {
        if (c->enr_M < 1) SD_FAIL(c, SD_ERR_ARG, "sd_nearest_speakers: no gallery is enrolled on this context");
        if (M != c->enr_M || d != c->enr_d) SD_FAIL(c, SD_ERR_ARG, "sd_nearest_speakers: the enrolled gallery has %lld rows of %d dimensions, not %lld of %d", (long long)c->enr_M, c->enr_d, (long long)M, d);
        d_gal = c->enr_gal.as<double>(); d_m2 = c->enr_m2.as<double>();
    } else {
        if (M < 1 || M > 0x7fffffff) SD_FAIL(c, SD_ERR_ARG, "sd_nearest_speakers: bad argument (1 <= M < 2^31)");
        if (int rc = check_gallery(c, h_gallery, M, d, "sd_nearest_speakers")) return rc;
        WS(c, double, t_gal, "spk_gallery", M * d); WS(c, double, t_m2, "ng_m2", M);
        HIPCHK(c, hipMemcpyAsync(t_gal, h_gallery, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
        if (int rc = run_gallery_norms(c, t_gal, M, d, t_m2)) return rc;
        d_gal = t_gal; d_m2 = t_m2;
    }
    WS(c, double, d_X, "ng_X", N * d); WS(c, int, d_best, "ng_best", N); WS(c, double, d_dist, "ng_dist", N);
    HIPCHK(c, hipMemcpyAsync(d_X, h_X, (size_t)N * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = run_nearest_gallery(c, d_X, nullptr, N, d_gal, d_m2, M, d, d_best, d_dist)) return rc;
    static_assert(sizeof(int) == sizeof(int32_t), "labels are 32-bit");
    if (h_best) HIPCHK(c, hipMemcpy(h_best, d_best, (size_t)N * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (h_dist) HIPCHK(c, hipMemcpy(h_dist, d_dist, (size_t)N * sizeof(double), hipMemcpyDeviceToHost));
    return SD_OK;
}

extern "C" int sd_last_enrolled(const sd_ctx* c, int32_t* h_rows, int64_t cap, int64_t* K)
{
    if (!c || cap < 0) return SD_ERR_ARG;
    const int64_t k = c->last.cen_K;
    if (K) *K = k;
    for (int64_t i = 0; i < k && i < cap; ++i) if (h_rows) h_rows[i] = i < (int64_t)c->last.enrolled.size() ? c->last.enrolled[(size_t)i] : -1;
    return SD_OK;
}

// ------------------------------------------------------------------ the speaker roster on the last job (the rule and the host-only entries: roster.cpp)
// steps B - D on the centroids of the last job: no rows, the context's threshold.  Host arithmetic only: nothing is launched
extern "C" int sd_roster_update_last(sd_roster* r, sd_ctx* c, int32_t* h_ids, int64_t cap, int64_t* K)
{
    if (!c) return SD_ERR_ARG;
    c->err.clear();
    if (!r || cap < 0) SD_FAIL(c, SD_ERR_ARG, "sd_roster_update_last: bad argument");
    const JobResult& job = c->last;
    if (job.cen_K < 1) SD_FAIL(c, SD_ERR_ARG, "sd_roster_update_last: no clustering call on this context yet");
    if (job.cen_d != r->d) SD_FAIL(c, SD_ERR_ARG, "sd_roster_update_last: the last job has centroids of %d dimensions, the roster entries of %d", job.cen_d, r->d);
    std::vector<int32_t> ids((size_t)job.cen_K);
    const int rc = sd_roster_update(r, job.cen.data(), job.cen_counts.data(), job.cen_K, nullptr, 0, nullptr, 0, 0, c->speaker_match_threshold, ids.data());
    if (rc == SD_ERR_NUMERIC) SD_FAIL(c, rc, "sd_roster_update_last: zero-magnitude centroid (reference throws, sd.cpp:493-495)");
    if (rc) SD_FAIL(c, rc, "sd_roster_update_last: the roster update failed (%d)", rc);
    if (K) *K = job.cen_K;
    if (h_ids) for (int64_t k = 0; k < job.cen_K && k < cap; ++k) h_ids[k] = ids[(size_t)k];
    c->last.roster_ids = std::move(ids);
    return SD_OK;
}

extern "C" int sd_last_roster_ids(const sd_ctx* c, int32_t* h_ids, int64_t cap, int64_t* K)
{
    if (!c || cap < 0) return SD_ERR_ARG;
    const int64_t k = (int64_t)c->last.roster_ids.size();
    if (K) *K = k;
    if (h_ids) for (int64_t i = 0; i < k && i < cap; ++i) h_ids[i] = c->last.roster_ids[(size_t)i];
    return SD_OK;
}

// voiceprint file: text, one speaker per line -- a name without white space, then SD_EMB_DIM values (%.17g: the round trip is bit-exact); # starts a comment
static std::string g_vp_err;
extern "C" const char* sd_voiceprints_error(void) { return g_vp_err.c_str(); }
static bool vp_name_ok(const char* s)
{
    if (!s || !s[0]) return false;
    for (const char* p = s; *p; ++p) if (*p == '#' || *p == ' ' || (*p >= '\t' && *p <= '\r')) return false;
    return true;
}
extern "C" void sd_free_voiceprints(char** names, double* emb, int64_t M)
{
    if (names) for (int64_t i = 0; i < M; ++i) free(names[i]);
    free(names); free(emb);
}
extern "C" int sd_read_voiceprints(const char* path, char*** names, double** emb, int64_t* M)
{
    g_vp_err.clear();
    if (!path || !names || !emb || !M) { g_vp_err = "sd_read_voiceprints: bad argument"; return SD_ERR_ARG; }
    *names = nullptr; *emb = nullptr; *M = 0;
    std::ifstream in(path);
    if (!in) { g_vp_err = std::string("cannot open ") + path; return SD_ERR_ARG; }
    std::vector<std::string> nm;
    std::vector<double> val;
    std::string line;
    auto bad = [&](int64_t no, const std::string& why) { char b[64]; snprintf(b, sizeof(b), ": line %lld: ", (long long)no); g_vp_err = std::string(path) + b + why; return (int)SD_ERR_ARG; };
    for (int64_t no = 1; std::getline(in, line); ++no) {
        const size_t hash = line.find('#');
        if (hash != std::string::npos) line.resize(hash);
        std::vector<std::string> tok;
        for (size_t i = 0; i < line.size();) {
            while (i < line.size() && (line[i] == ' ' || (line[i] >= '\t' && line[i] <= '\r'))) ++i;
            size_t j = i;
            while (j < line.size() && !(line[j] == ' ' || (line[j] >= '\t' && line[j] <= '\r'))) ++j;
            if (j > i) tok.push_back(line.substr(i, j - i));
            i = j;
        }
        if (tok.empty()) continue;
        if (tok.size() != (size_t)SD_EMB_DIM + 1) return bad(no, "a name and " + std::to_string(SD_EMB_DIM) + " values expected, " + std::to_string(tok.size() - 1) + " values found");
        if (std::find(nm.begin(), nm.end(), tok[0]) != nm.end()) return bad(no, "name " + tok[0] + " occurs twice");
        nm.push_back(tok[0]);
        for (size_t q = 1; q < tok.size(); ++q) {
            char* end = nullptr;
            const double v = strtod(tok[q].c_str(), &end);
            if (end == tok[q].c_str() || *end || !std::isfinite(v)) return bad(no, "'" + tok[q] + "' is not a finite number");
            val.push_back(v);
        }
    }
    const size_t n = nm.size();
    char** pn = (char**)malloc(sizeof(char*) * (n ? n : 1));
    double* pe = (double*)malloc(sizeof(double) * SD_EMB_DIM * (n ? n : 1));
    if (!pn || !pe) { free(pn); free(pe); g_vp_err = "out of host memory"; return SD_ERR_ARG; }
    for (size_t i = 0; i < n; ++i) pn[i] = strdup(nm[i].c_str());
    if (n) memcpy(pe, val.data(), val.size() * sizeof(double));
    *names = pn; *emb = pe; *M = (int64_t)n;
    return SD_OK;
}
extern "C" int sd_write_voiceprints(const char* path, const char* const* names, const double* emb, int64_t M)
{
    g_vp_err.clear();
    if (!path || M < 0 || (M > 0 && (!names || !emb))) { g_vp_err = "sd_write_voiceprints: bad argument"; return SD_ERR_ARG; }
    for (int64_t i = 0; i < M; ++i) {
        if (!vp_name_ok(names[i])) { g_vp_err = "sd_write_voiceprints: a name must be non-empty, without white space or #"; return SD_ERR_ARG; }
        for (int64_t j = 0; j < i; ++j) if (strcmp(names[i], names[j]) == 0) { g_vp_err = std::string("sd_write_voiceprints: name ") + names[i] + " occurs twice"; return SD_ERR_ARG; }
        for (int q = 0; q < SD_EMB_DIM; ++q) if (!std::isfinite(emb[i * SD_EMB_DIM + q])) { g_vp_err = std::string("sd_write_voiceprints: the voiceprint of ") + names[i] + " is not finite"; return SD_ERR_ARG; }
    }
    FILE* f = fopen(path, "w");
    if (!f) { g_vp_err = std::string("cannot write ") + path; return SD_ERR_ARG; }
    for (int64_t i = 0; i < M; ++i) {
        fputs(names[i], f);
        for (int q = 0; q < SD_EMB_DIM; ++q) fprintf(f, " %.17g", emb[i * SD_EMB_DIM + q]);
        fputc('\n', f);
    }
    if (fclose(f) != 0) { g_vp_err = std::string("cannot write ") + path; return SD_ERR_ARG; }
    return SD_OK;
}

// sd_write_rttm_ex with names: the speaker field of a turn with label k is names[k] where 0 <= k < K and names[k] != NULL, SPEAKER_kk otherwise
extern "C" int sd_write_rttm_named(const char* path, const char* uri, const sd_turn* turns, int64_t n_turns, const double* conf, const char* const* names, int64_t K)
{
    if (!path || (n_turns > 0 && !turns) || n_turns < 0 || K < 0 || (K > 0 && !names)) return SD_ERR_ARG;
    for (int64_t k = 0; k < K; ++k) if (names[k] && !vp_name_ok(names[k])) return SD_ERR_ARG;
    FILE* f = fopen(path, "w");
    if (!f) return SD_ERR_ARG;
    for (int64_t i = 0; i < n_turns; ++i) {
        const int32_t k = turns[i].label;
        fprintf(f, "SPEAKER %s 1 %.3f %.3f <NA> <NA> ", (uri && uri[0]) ? uri : "audio", turns[i].start, turns[i].end - turns[i].start);
        if (k >= 0 && k < K && names[k]) fprintf(f, "%s <NA> ", names[k]); else fprintf(f, "SPEAKER_%02d <NA> ", k);
        if (conf && conf[i] == conf[i]) fprintf(f, "%.4f\n", conf[i]); else fprintf(f, "<NA>\n");
    }
    fclose(f);
    return SD_OK;
}
