// common.h -- internal declarations shared by the HIP translation units of libsdhip.so
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <functional>
#include <initializer_list>
#include <vector>
#include "../../include/sdhip_test.h"
#include "cluster_host.h"
#include "many_plan.h"

#define SD_T 501          // STFT frames per item (1 + 80000/160), sd.cpp:1980-2008
#define SD_TP 501         // rows per item in activation buffers (= T: no padding rows; a 128-row tile may span two items)
#define SD_NBINS 201
#define SD_NMELS 80
#define SD_FEAT_LD 96     // mel channels padded to a multiple of 32

// The waveform a stage reads, on the device.  It travels as a value from the entry that knows the buffer to the launches: nothing about it is kept in the context
#define SD_WAV_PAD 512      // zeroed floats the library leaves behind the last sample it holds: SincNet's 256-tap rows read 4 samples past the last window
struct DevWav {
    const float* p;         // p[0] = sample `origin` of the recording
    int64_t n;              // samples of the whole recording (not of the slice held)
    int64_t origin = 0;     // > 0: the sharded entries and a stream hold a slice
    bool padded = false;    // SD_WAV_PAD zeroed floats follow the last held sample (library-allocated buffers only); the shared-conv0 path of PyanNet needs them
};

struct KernelStat { double ms = 0; int64_t launches = 0; double flops = 0, bytes = 0; };

// SD_TRACE_WS=1 (diagnostic): what the workspace allocations of a job cost -- hipMalloc / hipFree time and bytes, printed by sd_diarize*
// (process-wide, touched by every context's allocations: atomics)
inline std::atomic<long long> g_ws_alloc_us{0}, g_ws_free_us{0};
inline std::atomic<size_t> g_ws_alloc_bytes{0}, g_ws_allocs{0};
inline std::atomic<size_t> g_ws_limit{0};          // test hook (option ws_limit_mb): a workspace request above this many bytes fails like an exhausted GPU; 0 = off
// per-device "dynamic-LDS attribute set" masks of the wide conv kernels (the attribute belongs to the device's code object, the launch to a context)
inline std::atomic<unsigned> g_attr_w256{0}, g_attr_g256{0}, g_attr_pp{0}, g_attr_res2{0};
struct DevBuf {
    void* p = nullptr; size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        const auto t0 = std::chrono::steady_clock::now();
        if (p) (void)hipFree(p);
        const auto t1 = std::chrono::steady_clock::now();
        p = nullptr; cap = 0;
        size_t want = bytes + (bytes >> 3) + 256;
        const size_t lim = g_ws_limit.load(std::memory_order_relaxed);
        if ((lim && bytes > lim) || hipMalloc(&p, want) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return 1; }      // (the failure must not surface again at the next kernel-launch check)
        const auto t2 = std::chrono::steady_clock::now();
        g_ws_free_us += (long long)std::chrono::duration<double, std::micro>(t1 - t0).count();
        g_ws_alloc_us += (long long)std::chrono::duration<double, std::micro>(t2 - t1).count();
        g_ws_alloc_bytes += want; ++g_ws_allocs;
        cap = want; return 0;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// a conv / linear layer in device layout
struct ConvLayer {
    float* W = nullptr;       // [KT][Cout][CinPad] (Cin contiguous)
    void* W16 = nullptr;      // the same weights rounded to fp16 (ECAPA conv layers only; option ecapa_precision = 1)
    float* bias = nullptr;    // [Cout] or null
    float* scale = nullptr;   // folded BatchNorm (applied after act1) or null
    float* shift = nullptr;
    int Cin = 0, CinPad = 0, Cout = 0, KT = 1, dil = 1;
    int CinPad16 = 0;         // row length of W16 (multiple of 64)
    void* W16x = nullptr;     // option ecapa_precision = 3: [KT][Cout][CinPad / 8][8 hi | 8 lo] fp16 halves of W * w16x_scale (a power of two)
    float w16x_inv = 1.0f;    // 1 / w16x_scale
};

struct ConvArgs {
    const float* X; const float* X2; const float* W; float* Y;
    const void* W16;       // optional fp16 copy of W (same layout)
    const float* bias; const float* scale; const float* shift; const float* item_bias; const float* R;
    int x_ld, x2_ld, y_ld, r_ld, ib_ld;
    int w_ld;              // floats between consecutive output-channel rows of W (0 = Cin)
    int M;                 // total output rows
    int TpIn, TpOut;       // rows per item in input / output buffers
    int Tin, T;            // valid rows per item in input / output
    int Cin, Cout, KT, dil;
    int cin_real;          // un-padded input channels (algorithmic FLOP accounting only; 0 = Cin)
    int pad_mode;          // 0 = "same" with reflect padding, 1 = "valid" (src row = t + kk*dil)
    int act1, act2;        // act1: 0 none 1 relu 2 leaky(0.01); act2 (after BN): 0 none 1 tanh 2 sigmoid
    int m_tiles, n_tiles;
    int sched;             // persistent-schedule variant (set by the launcher)
    // compact row space (ECAPA): the buffers hold, item after item, only the frames that can influence a valid output
    // (need_i = min(501, nvalid_i + receptive field) rows of item i).  rowtab[g] of compact row g:
    //   .x = first compact row of g's item,  .y = frame t | (need - 1) << 10 | item << 20
    // g enumerates the OUTPUT rows; .x and the "last stored frame" refer to the INPUT buffer, which may live in a wider row
    // space of `in_rows` rows (0 = the same space, M rows): the 1x1 MFA layer reads the rows with their receptive-field margin
    // and writes only the frames < nvalid.  TpIn / TpOut / T are unused; a tap that reaches beyond the item's last stored
    // frame reads that last frame instead (it can only feed frames that are themselves beyond nvalid).  null = dense mapping.
    const int2* rowtab;
    int in_rows;
    int y_f32;             // fp16 mode: Y is float all the same (the attention logits feed an exp)
    int kt_real;           // fp16 split-weight mode: KT counts 2 * kt_real weight planes (hi, then lo) and tap kk shifts the rows like tap kk % kt_real; 0 = KT
    int prec;              // 0 = f32 (X, X2, W, Y are float), 1 = fp16 end to end (X, X2, W16, Y are _Float16; option ecapa_precision),
                           // 3 = f32 tensors, split fp16 operands on the matrix pipe (W16x; wide layers only, conv_gemm_h.hip)
    const void* W16x;      // prec 3: split weights (ConvLayer::W16x)
    float acc_scale;       // prec 3: 1 / weight scale, applied to the accumulator in the epilogue
    int stagger;           // 128 x 128 f32 kernel, short contractions: 0 = all workgroups start together, 1 / 2 = half of them start half a tile late (conv_gemm.hip)
};
#define ROWTAB_T(y) ((y) & 1023)
#define ROWTAB_LAST(y) (((y) >> 10) & 1023)
#define ROWTAB_ITEM(y) ((int)((unsigned)(y) >> 20))
#define ROWTAB_MAX_ITEMS 4095
// SD_SKINNY_MAX_ROWS, the row count up to which launch_conv_gemm (conv_gemm.hip) takes k_skinny_gemm, is many_plan.h's, next to the side rule that rests on it

struct EcapaWeights {
    bool loaded = false;
    float* mel_w = nullptr; int* mel_lo = nullptr; int* mel_cnt = nullptr; int* mel_off = nullptr; int mel_nnz = 0;
    float* window = nullptr;          // [400] f32 periodic Hamming
    double* tw_cos = nullptr;         // [400] cos(2 pi k/400)
    double* tw_nsin = nullptr;        // [400] -sin(2 pi k/400)
    ConvLayer block0;
    struct SERes { ConvLayer tdnn1, res[7], tdnn2, se1, se2; int dil; } blk[3];
    ConvLayer mfa, asp_tdnn_x, asp_tdnn_ms, asp_conv, fc;
    int C = 1024;
    // the fp16 copies of the per-frame conv layers are built ON THE GPU from the f32 weights the first time a mode that reads them is
    // selected (weights.cpp: ensure_ecapa_mode_weights): the default f32 mode pays nothing for them at start-up
    std::vector<ConvLayer*> conv16;   // layers that have fp16 forms
    bool have16 = false, have16x = false;
};

struct SegWeights {
    bool loaded = false;
    float wn_w = 1, wn_b = 0;          // InstanceNorm1d(1) affine on the waveform
    ConvLayer conv0, conv1, conv2;     // sincnet convs (conv0: Cin = 256 padded taps, x_ld = 10)
    float* conv0_wsum = nullptr;       // [80] sum of conv0's taps per filter (the shared-conv0 path folds the chunk normalisation into an affine map)
    float* in_w[3] = {nullptr, nullptr, nullptr};   // InstanceNorm affine per stage
    float* in_b[3] = {nullptr, nullptr, nullptr};
    ConvLayer lstm_ih[4];              // [1024][in] both directions stacked, bias = b_ih + b_hh
    float* lstm_hh[4][2] = {};         // [512][128] per layer, direction (PyTorch gate order i,f,g,o)
    void* lstm_hh_x[4][2] = {};        // option seg_precision = 3: [hi | lo][512][128] fp16 halves of W_hh * 2^e; lstm_hh_inv = 2^-e
    float lstm_hh_inv[4][2] = {};
    ConvLayer lin0, lin1;
    float* cls_w = nullptr; float* cls_b = nullptr;   // [3][128], [3]
};

// results kept for the step dumps (stepdump.cpp); filled only while dump_dir is set
struct StepStash {
    bool clustered = false;                    // run_clustering went past the "fewer than two rows" exit
    int64_t N = 0; int K = 0;
    std::vector<int> clusters, cluster_res, hard_pre;   // fcluster labels - 1, labels after the small -> large pass, [M] assignment before the inactive rule
    std::vector<double> X, Xn, soft;           // [N][d] filtered rows, the same normalised, [M][K] scores 2 - cosine distance
    int64_t ar0 = 0, cr0 = 0, rows = 0, crow_all = 0, nact = 0;   // to_diarization's crop ranges
    int64_t infer_items = 0;                   // items of the last shard_infer call (masks / counts workspaces describe them)
};

// What the last job leaves for sd_last_confidence / sd_last_speakers / sd_last_enrolled, as one value (sd_ctx::last).  conf: per-turn confidence, written at
// the end of finalize / sd_cut_turns_many.  The last clustering call (run_clustering, or the last cut): its cen_K final centroids [cen_K][cen_d] -- row k = raw
// label k -- and the train rows of each; cen_K = 0 before any and after one that failed.  enrolled: their gallery rows, -1 (or absent) where nobody enrolled.
// hard: finalize's [chunks * 3] assignment behind the inactive rule (the rows of a roster update; empty for a job that is no finalize).  roster_ids: the
// roster id of every raw label, empty unless a roster took part (sd_last_roster_ids).
struct JobResult { std::vector<double> conf, cen; std::vector<int64_t> cen_counts; int cen_K = 0, cen_d = 0; std::vector<int32_t> enrolled, hard, roster_ids; };

// one recording of a sd_diarize_many* call (many.hip): what finalize left in the context for it; sd_many_select puts it back
struct ManyJob { int status = SD_OK; JobResult res; };

struct sd_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    EcapaWeights ew;
    SegWeights sw;
    std::vector<void*> owned;                  // device allocations freed in sd_destroy
    char* warena_cur = nullptr; size_t warena_left = 0;   // weights.cpp: bump allocator over 64 MB device blocks
    std::map<std::string, DevBuf> ws;          // named workspaces
    std::set<std::string> rs_taps_filled;      // resample.hip: tap tables whose upload has completed
    std::map<std::string, KernelStat> stats;
    bool profile = false;
    bool profile_detail = false;               // also bracket conv_gemm per layer tag (option profile=2)
    std::vector<std::tuple<std::string, hipEvent_t, hipEvent_t, double, double>> pending;
    double stage_ms[4] = {0, 0, 0, 0};
    int64_t emb_batch_items = 3072;            // multiple of 96; row budget of a batch = this many full-length items (a batch also holds at most 4 095 items): ~57 GB of activation workspaces at the 1-h size, 1 % faster than 768 (fewer partly filled tile rounds and launch tails)
    bool emb_batch_explicit = false;            // set through sd_set_option: then it holds from the first call on
    int64_t embed_calls = 0;                    // run_embed calls of this context: the FIRST one plans 768-item batches (16 GB) unless the option was set --
                                                // a one-shot CLI user does not pay ~0.5 s of first-touch hipMalloc for a 57 GB arena; a context that sees more work grows it
    int64_t seg_batch_chunks = 4096;           // 128 LSTM workgroups per direction: one full wave of CUs
    int num_clusters = -1, min_clusters = -1, max_clusters = -1;   // optional constraints for the whole-path entry points
    int ecapa_precision = 0;                    // 0 = f32 MFMA (default, the measured configuration), 1 = fp16 MFMA with f32 accumulation, 2 = the same with hi + lo fp16 weight planes, 3 = f32 tensors, hi + lo split of BOTH operands on the fp16 MFMA (wide layers; the others stay f32)
    int seg_precision = -1;                     // -1 = auto: 3 whenever ecapa_precision != 0 (an fp16-pipe mode was asked for), else 0 (round 6; seg_prec() below); 0 = f32 MFMA; 3 = PyanNet's LSTM (input projections of layers 1-3 and the recurrence) with both MFMA operands split into hi + lo fp16 halves
    bool ecapa_keep_cat = false;                // diagnostics: f32 mode keeps the block outputs (the logits get their own buffer)
    int ecapa_f16_hp = 0;                       // fp16 mode: bit 0 = MFA output / pooling inputs in f32, bit 1 = attention branch on the f32 MFMA
    bool conv_w256_f32 = true;                  // f32: the same 256 x 256 kernel for the wide, long-K ECAPA layers (TDNN, MFA)
    int conv_pn128 = 0;                         // 128 x 128 kernel: column tiles per super-block (0 = 8); tuning
    int ecapa_ld_pad = 0;                       // elements added to the leading dimensions of the ECAPA activation buffers (multiple of 8)
    bool seg_wide_ih = true;                    // LSTM input projections of layers 1-3 on the 256 x 256 tile (identity row table); tuning
    bool seg_shared_conv0 = true;               // SincNet conv0 once over the waveform instead of once per (90 % overlapping) chunk
    int conv_w256_kmin = 0;                     // 256 x 256 kernel: shortest contraction Cin * KT it takes (0 = built-in: 1024 f32, 256 fp16); tuning
    int conv_pn = 0;                            // 256 x 256 kernel: column tiles per super-block (0 = 8); tuning
    bool conv_h256 = true;                      // fp16 mode: 256 x 256 tile kernel for the wide layers (conv_gemm_h.hip)
    int conv_mfma16 = 1;                        // fp16 LDS-DMA wide kernel on v_mfma_f32_16x16x32_f16 (higher clock under load) instead of 32x32x16; conv_gemm_g.hip
    int conv_rot = 3;                           // LDS-DMA wide kernel: the workgroups that share a row panel request its quarters in rotated order (conv_gemm_g.hip); tuning
    int conv_stagger = 0;                       // 128 x 128 f32 kernel: start half of the workgroups half a tile late (0 off, 1 odd, 2 upper half); tuning
    bool conv_res2_ws = true;                   // f32 Res2Net convs (Cin = Cout = 128, 3 taps, M >= 2 048): the weight-stationary kernel (conv_res2.hip); 0 = the 128 x 128 kernel; same bits; A-B
    int conv_res2_wgs = 0;                      // ... its workgroups (0 = one per CU); tuning / test: the bits do not depend on it
    bool conv_glds_f32 = false;                 // f32: the LDS-DMA staged form of the wide tile (conv_gemm_g.hip, P = 0): bit-identical, measured slower; A-B only
    bool conv_pp = true;                        // fp16 mode: the never-drained kernel for the wide layers (conv_gemm_p.hip, round 6); 0 = conv_gemm_g.hip; A-B
    bool conv_glds = true;                      // fp16 mode: ... staged by LDS-DMA (conv_gemm_g.hip) instead of through registers; tuning / A-B
    bool skip_dead_rows = true;                 // ECAPA: skip row panels beyond nvalid + receptive field
    int64_t linkage_wgs = -1;                  // -1 auto, 0/1 single workgroup, else cooperative workgroups
    int64_t linkage_square = -1;               // -1 auto (full N x N distance matrix while it fits), 0 condensed, 1 square
    int64_t linkage_one_xcd = 1;               // 1 = the one-XCD forms (every workgroup on XCC 0) on a device with >= 256 CUs: the cooperative kernel where the plan has G <= 32 workgroups, k_linkage_hx where 31 workers fit; run_linkage clears it after a one-XCD poll timeout
    int64_t linkage_zero_phase = 1;            // a tie at height 0 (duplicate rows): the heap replay takes the merges at height 0, k_linkage_rg the rest (0 = whole replay)
    int64_t linkage_tie_kernel = 1;            // what finishes a job with exact ties: 1 = k_linkage_hx (heap replay, row work on worker workgroups; > 1 = that many workers), 0 = k_linkage_heap (one workgroup)
    int64_t linkage_prefetch = 0;              // k_linkage_rg: 1 = a helper wave per workgroup requests the rows of the runner-up neighbours ahead of time
    bool linkage_hx_wide = false;              // test: k_linkage_hx with 32-bit heap keys / positions in global memory (the form of N > 65 535) on any size
    bool linkage_force_heap = false;           // test / measurement: skip the cooperative kernel, go straight to the heap replay
    int64_t linkage_kernel = -1;               // -1 auto / 1: k_linkage_rg (linkage_rg.hip) for the square form where its geometry fits (1: with more threads than linkage_threads asks for where that makes it fit), else k_linkage_mw (linkage_mw.hip); 0: k_linkage_mw
    int64_t linkage_threads = 0;               // 0 auto (linkage_plan: k_linkage_rg 256, doubled until its geometry fits; k_linkage_mw 512 for N >= 8000 -- one XCD: N >= 16000 --, else 256), else rounded down to 128 / 256 / 512 / 1024 threads per cooperative workgroup
    int64_t linkage_batch = 0;                 // group calls (finalize_jobs, many.hip): 1 = the dendrograms of the jobs that fit run ahead of the per-job finalize in shared launches (run_linkage_many), 0 = one job after the other (the default: profiles/linkage_many_times.txt)
    int64_t linkage_batch_bytes = (int64_t)2 << 30;   // run_linkage_many: bytes the workspaces of one group of jobs may take
    int64_t linkage_batch_xcd = 0;             // run_linkage_many: 1 = the jobs of the one-XCD cooperative class run eight to a launch, one per XCD (k_linkage_rg_jobs); 0 = one after the other (the default until profiles/linkage_xcd_times.txt says otherwise)
    int64_t linkage_batch_xcd_zero = 0;        // run_linkage_many, read only under linkage_batch_xcd = 1: 1 = a job of an XCD launch that stops at a tie at height 0 before its first merge (duplicate rows) stays in the batch: k_linkage_hx_jobs takes the merges at height 0, k_linkage_rg_jobs<M, true> the rest; 0 = such a job is redone alone (the default: tests/test_linkage_xcd.py pins it, profiles/linkage_xcd_zero_times.txt)
    int64_t linkage_batch_threads = 0;         // run_linkage_many: threads of the workgroup of a job, 0 auto (256), else 256 or 1024; tuning
    std::vector<double> ahead_Z; int64_t ahead_N = -1;      // finalize_jobs -> cluster_rows: the dendrogram of the job being finalized, from the pass ahead (ahead_N = its train rows; -1 = none)
    int num_cu = 256;
    bool constrained_assignment = false;        // Clustering.py:81-94 (one cluster per local speaker of a chunk)
    // the three hyper-parameters of Clustering.py:251-276; defaults = what the reference hard-codes (sd.cpp:2049-2056)
    int clustering_method = SD_LINKAGE_CENTROID;
    double clustering_threshold = (double)0.7153814381597874f;      // the reference's float constant, widened
    int min_cluster_size = 15;
    int64_t max_num_embeddings = -1;            // Clustering.py:12, 69-76: cluster a sample of this many train rows, assign all (-1 = all of them, the port's "IS INF")
    bool stream_intact = false;                 // a stream call failed only in an allocation of a forget: its streams stay usable (stream.hip: forget_to, guard)
    int64_t clustering_seed = 0;                // ... chosen by sample_rows (cluster_host.h) under this seed
    JobResult last;                            // the last job (sd_last_confidence, sd_last_speakers, sd_last_enrolled)
    // the enrolled gallery (sd_set_enrolled): the context's own device copy [enr_M][enr_d], the squared norms of its rows (k_row_sqnorms), and a host copy
    // for the candidate loop and the centroid table of run_clustering; enr_M = 0: none, and nothing of the clustering stage changes
    DevBuf enr_gal, enr_m2;
    std::vector<double> enr_host;
    int64_t enr_M = 0;
    int enr_d = 0;
    double speaker_match_threshold = (double)0.7153814381597874f * (double)0.7153814381597874f / 2;      // sd_match_speakers: t * t / 2, the cosine distance at which the default clustering stops merging two unit vectors
    // the activity stage (activity.hip): pyannote's Binarize parameters for the speech / overlap timeline, and the timeline of the last whole-path call
    double activity_onset = 0.5, activity_offset = 0.5, activity_min_on = 0.0, activity_min_off = 0.0;
    bool activity_hamming = false;              // aggregate()'s Hamming-weighted branch (sd.cpp:1211-1215)
    std::vector<double> last_activity;           // cropped scores of the last sd_activity* call (sd_last_activity_scores)
    int64_t fe_bill_samples = -1, fe_bill_frames = 0;   // profiling: selected samples / stored frames of the next k_stft_fbank launch (-1 = unknown)
    void* comm = nullptr;                       // ncclComm_t (comm.cpp), null = single GPU
    int rank = 0, world = 1;
    int virtual_world = 0;                      // test mode of sd_diarize_sharded on one rank (comm.cpp)
    int64_t comm_timeout_ms = 600000;            // deadline of the exchange step of a sharded job (a peer that never arrives); then ncclCommAbort
    int64_t job_seq = 0;                        // sharded jobs since sd_comm_init (travels in the status record: ranks in different jobs are detected)
    int inject_fail_rank = -1;                  // test hook: this rank (a played rank under virtual_world) reports SD_ERR_ARG instead of inferring
    int rank0_permille = -1;                    // share of the chunks rank 0 infers itself (it also finalizes); -1 = equal shares
    std::string dump_dir;                       // sd_set_dump_dir: the next finalize writes the reference's WRITE_DATA items there
    int dump_level = 0;
    StepStash stash;
    std::string ws_failed;                      // ws_get: name of the workspace whose allocation failed last ("" = none); the embedding stage's retry reads it
    int fe_last_grid = 0;                       // test hook (sd_test_frontend_*): workgroups of the last k_stft_fbank launch; set by frontend_features, host code only
    const char* last_conv_kernel = nullptr;     // test hook (sd_test_conv): which kernel the conv dispatch launched last; set by every launch site, host code only
    const float* planted_scores = nullptr;      // sd_set_planted: measurement / test hook
    const float* planted_emb = nullptr;
    int64_t planted_lo = 0, planted_n = 0;
    std::vector<ManyJob> many_jobs;             // per recording of the last sd_diarize_many* call, or per stream of the last sd_stream_turns_many (sd_many_select)
    std::vector<sd_stream*> streams;            // open sd_stream objects of this context (stream.hip); sd_destroy closes what is left
    std::vector<sd_cut*> cuts;                  // open sd_cut objects of this context (cut.hip); sd_destroy closes what is left
    int64_t cut_group_bytes = (int64_t)1 << 30; // sd_cut_turns_many: bytes the activation tables of one group of cuts may take (test key)
};

#define SD_FAIL(ctx, code, ...) do { char _b[512]; snprintf(_b, sizeof(_b), __VA_ARGS__); (ctx)->err = _b; return (code); } while (0)
#define HIPCHK(ctx, expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { SD_FAIL(ctx, SD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); } } while (0)
#define KCHECK(ctx) HIPCHK(ctx, hipGetLastError())

// workspace helper
template <class T> inline T* ws_get(sd_ctx* c, const char* name, size_t count) {
    DevBuf& b = c->ws[name];
    if (b.reserve(count * sizeof(T))) { c->ws_failed = name; return nullptr; }
    return b.as<T>();
}
#define WS(ctx, T, var, name, count) T* var = ws_get<T>(ctx, name, (size_t)(count)); if (!var) SD_FAIL(ctx, SD_ERR_HIP, "hipMalloc of workspace %s (%zu bytes) failed", name, (size_t)(count) * sizeof(T))

// ---- helpers of the host wrappers (api.cpp, pipeline.cpp, comm.cpp) and of the one-dimensional launches
struct DevTmp {   // RAII device scratch for the host-pointer wrappers
    void* p = nullptr;
    ~DevTmp() { if (p) (void)hipFree(p); }
    int alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16) == hipSuccess ? 0 : 1; }
};
#define DTMP(ctx, var, bytes) DevTmp var; if (var.alloc(bytes)) SD_FAIL(ctx, SD_ERR_HIP, "hipMalloc(%zu) failed", (size_t)(bytes))
#define ENTER(ctx) do { if (!(ctx)) return SD_ERR_ARG; (ctx)->err.clear(); if (hipSetDevice((ctx)->device) != hipSuccess) SD_FAIL(ctx, SD_ERR_HIP, "hipSetDevice failed"); } while (0)
#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)
inline double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// profiling bracket: records events around one launch when ctx->profile is set
struct ProfScope {
    sd_ctx* c; std::string name; hipEvent_t e0 = nullptr, e1 = nullptr; double flops, bytes;
    ProfScope(sd_ctx* ctx, const std::string& n, double fl = 0, double by = 0) : c(ctx), name(n), flops(fl), bytes(by) {
        if (c->profile) { (void)hipEventCreate(&e0); (void)hipEventCreate(&e1); (void)hipEventRecord(e0, c->stream); }
    }
    ~ProfScope() {
        if (c->profile) { (void)hipEventRecord(e1, c->stream); c->pending.emplace_back(name, e0, e1, flops, bytes); }
        else { KernelStat& s = c->stats[name]; s.launches++; s.flops += flops; s.bytes += bytes; }
    }
};
void sd_flush_profile(sd_ctx* c);   // api.cpp: resolves pending event pairs into stats

// ---- the launch tail the conv_gemm*.hip launchers share (host only)
// Tile counts and the persistent grid: wgs_per_cu workgroups on every CU, a multiple of 8 (an equal share per XCD), and
// no more workgroups per XCD than the busiest XCD has tiles
inline int conv_tiles_grid(const sd_ctx* c, ConvArgs& a, int tile_m, int tile_n, int wgs_per_cu)
{
    a.m_tiles = (a.M + tile_m - 1) / tile_m;
    a.n_tiles = (a.Cout + tile_n - 1) / tile_n;
    int g = (wgs_per_cu * c->num_cu / 8) * 8;
    if (g < 8) g = 8;
    const int lx_max = ((a.m_tiles + 7) / 8) * a.n_tiles;
    if (g / 8 > lx_max) g = lx_max * 8;
    return g;
}
// The FLOP / byte bill of a layer (bench.py's roofline figures): un-padded input channels, algorithmic taps (the lo planes of the split-weight mode
// are overhead, not work); `rows` output rows that read `inputs` input tensors
struct ConvBill { double flops, bytes; };
inline ConvBill conv_bill(const ConvArgs& a, double rows, bool f16, int inputs = 1)
{
    const int cin = a.cin_real > 0 ? a.cin_real : a.Cin;
    const int kt_alg = a.kt_real > 0 ? a.kt_real : a.KT;
    return {2.0 * rows * a.Cout * cin * kt_alg, (f16 ? 2.0 : 4.0) * (rows * cin * inputs + rows * a.Cout + (double)a.Cout * cin * a.KT)};
}
// The dynamic-LDS attribute of a kernel family, set once per device (a second thread that gets here meanwhile sets the same values); false = refused
inline bool conv_set_dyn_lds(const sd_ctx* c, std::atomic<unsigned>& mask, std::initializer_list<const void*> kernels, size_t lds_bytes)
{
    const unsigned dev_bit = 1u << (c->device & 31);
    if (mask.load(std::memory_order_acquire) & dev_bit) return true;
    for (const void* k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
    mask.fetch_or(dev_bit, std::memory_order_release);
    return true;
}
// The stats one launch of a wide (256 x 256) kernel bills: all conv_gemm launches (per layer tag under profile_detail), per precision ("f16" | "x3" | "f32"),
// the wide tile alone (bench.py's roofline object), and that split by caller (PyanNet's K = 256 projections / the ECAPA layers)
struct ConvProfWide {
    ProfScope all, prec, wide, caller;
    ConvProfWide(sd_ctx* c, const char* tag, const char* p, const ConvBill& b)
        : all(c, c->profile_detail ? std::string("conv_gemm:") + tag : std::string("conv_gemm"), b.flops, b.bytes),
          prec(c, std::string("conv_gemm_") + p, b.flops, b.bytes), wide(c, std::string("conv_w256_") + p, b.flops, b.bytes),
          caller(c, strcmp(tag, "lstm_ih") == 0 ? "conv_w256_seg" : "conv_w256_ecapa", b.flops, b.bytes) {}
};
// ---- conv_gemm.hip: picks the kernel (pp -> g256 -> w256 -> skinny -> res2ws -> 128 x 128); the launchers below are its steps and get `a` with w_ld already defaulted
int launch_conv_gemm(sd_ctx* c, const ConvArgs& a, const char* tag);
// ---- conv_gemm_h.hip (fp16 mode, Cout >= 256: 256 x 256 tile; returns 1 = not applicable)
int launch_conv_gemm_h256(sd_ctx* c, const ConvArgs& a, const char* tag);
// ---- conv_gemm_g.hip (fp16 mode, Cout >= 256: the same tile with LDS-DMA staging; returns 1 = not applicable)
int launch_conv_gemm_g256(sd_ctx* c, const ConvArgs& a, const char* tag);
// ---- conv_gemm_p.hip (fp16 mode, Cout % 256 == 0, K >= 512, M >= 2 048: the never-drained form of round 6; returns 1 = not applicable)
int launch_conv_gemm_pp(sd_ctx* c, const ConvArgs& a, const char* tag);
// ---- conv_res2.hip (f32 Res2Net shape: weights in registers, row panel in LDS; launches only, launch_conv_gemm bills it; returns 1 = not applicable)
int launch_conv_res2ws(sd_ctx* c, const ConvArgs& a);
// ---- api.cpp: the precision PyanNet's LSTM runs in: the option, or -- left at auto -- the split-operand form whenever the caller selected an fp16-pipe
// mode for ECAPA (scores within 1e-6 of the f32 path's, identical turns: tests/test_gpu_parity.py, tests/test_planted.py; 86 -> 58 ms per hour)
int seg_prec(const sd_ctx* c);
// ---- conv_narrow.hip (f32, Cout <= 96, "valid" convs of SincNet: tile as wide as the layer; returns 1 = not applicable)
int launch_conv_narrow(sd_ctx* c, const ConvArgs& a, const char* tag);
// ---- weights.cpp
struct PackTensor { std::vector<int64_t> dims; std::vector<float> data; };
typedef std::map<std::string, PackTensor> Pack;
int load_pack(const char* path, Pack& out, std::string& err);
int load_model_any(const char* path, int kind, Pack& out, std::string& err);   // onnx_reader.cpp: .sdw pack or .onnx (kind 0 seg, 1 emb)
int build_ecapa_weights(sd_ctx* c, const Pack& p);
int build_seg_weights(sd_ctx* c, const Pack& p);
float lstm_whh_split(const float* whh /*[512][128]*/, _Float16* planes /*[hi | lo][512][128]*/);   // option seg_precision = 3: fp16 planes of W_hh * 2^e; returns 2^-e
void* weight_alloc(sd_ctx* c, size_t bytes);                      // weights.cpp: bump allocator over 64 MB device blocks (freed by sd_destroy)
int ensure_ecapa_mode_weights(sd_ctx* c, int ecapa_precision);   // weights_gpu.hip: builds W16 (modes 1, 2) / W16x (mode 3) on first use
// the two forms of ONE layer, into device memory the caller provides (conv_w16_bytes / conv_w16x_bytes; d_max: one unsigned of scratch); asynchronous on c->stream
inline size_t conv_w16_bytes(const ConvLayer& L) { return (size_t)2 * L.KT * L.Cout * L.CinPad16 * 2; }
inline size_t conv_w16x_bytes(const ConvLayer& L) { return (size_t)2 * L.KT * L.Cout * L.CinPad * 2; }
int build_conv_w16(sd_ctx* c, ConvLayer& L, void* d);                      // sets L.W16
int build_conv_w16x(sd_ctx* c, ConvLayer& L, void* d, unsigned* d_max);    // sets L.W16x, L.w16x_inv (synchronises the stream once: the exponent is chosen on the host)
// ---- frontend.hip
int frontend_prepare(sd_ctx* c, const float* d_masks, int64_t items, int64_t first_item, float* d_wav_lens, int* d_nnorm, int* d_nvalid,
                     int* d_flags, bool compact, int* h_n_active, int* d_cidx, std::vector<int>* h_nvalid = nullptr);
int frontend_features(sd_ctx* c, const DevWav& w, int64_t first_item, int64_t run_items, bool compact, const int* d_nnorm,
                      const int* d_rowoff, float* d_feats /*[rowoff[run_items]][96]*/, bool sig_mode = false);
int embed_signals_frames(sd_ctx* c, const float* h_wav_lens, int64_t B, std::vector<int>& nv, std::vector<int>& nn);      // api.cpp: sd_embed_signals' nvalid / nnorm from wav_lens
int frontend_prepare_signals(sd_ctx* c, int64_t items);     // sd_embed_signals: identity gather tables for [items][80000] signal rows
// ---- ecapa.hip
// Compact row spaces of the embedding network: space s stores the frames t < min(501, nvalid + EC_MARGIN[s]) of every item.
// A layer is only computed where a later valid frame can see it (ecapa.hip): block0 / block 1 run in space 0, block 2 in space 1,
// block 3 in space 2, MFA and the attentive pooling in space 3 (the valid frames alone).
#define EC_SPACES 4
struct EcapaRowPlan {
    int64_t n = 0;
    std::vector<int> off[EC_SPACES];      // host prefix sums [n + 1]
    const int* d_off = nullptr;           // device copy [EC_SPACES][n + 1]
};
int ecapa_need_rows(int nvalid, bool skip_dead_rows);             // rows of an item in space 0
// row table of `items` items (k_build_rowtab): d_off_out / d_off_in = device prefix sums [items + 1] of the rows per item in the output / input space
int ecapa_build_rowtab(sd_ctx* c, const int* d_off_out, int base_out, const int* d_off_in, int base_in, int64_t items, int2* d_rowtab);
int ecapa_rows_to_half(sd_ctx* c, const float* d_f32, void* d_f16, int64_t n4);      // k_rows_to_half: n4 groups of four floats -> fp16 (the fp16 mode's conversion)
int ecapa_feats_to_half(sd_ctx* c, const float* d_f32, void* d_f16, int64_t rows);   // k_feats_to_half: [rows][96] f32 -> [rows][128] fp16, columns 96 .. 127 zero
int ecapa_scatter_emb(sd_ctx* c, const float* d_emb_c, const int* d_cidx, float* d_emb, int64_t items);   // k_scatter_emb: emb[i] = emb_c[cidx[i]], NaN where cidx[i] < 0
// the launches of ecapa.hip's glue kernels, asynchronous on c->stream: grid, block and the instantiation (f16: the tensors marked void are _Float16, else
// float) are computed here; run_ecapa_t and the test hooks of ecapa_test.hip call the same ones.  Item i's first row in x is rowoff[i] - row_base; the
// statistics run over its frames < nvalid[i]; rows = the rows of the batch (the profile's bill).  masked_mean: out [items][C]; asp_stats / asp_pool:
// ms / pooled [items][2 C] = (mean | std); logit [rows][ld] f32.  se_apply: y = gate[item] * t2 + res over the `rows` rows of t2's space (rowtab: a table
// of that space); res_map / out_map: tables from t2's space into the residual's / the output's space, null = the same space; C % 4 == 0
int launch_masked_mean(sd_ctx* c, bool f16, const void* x, int ld, const int* nvalid, const int* rowoff, int row_base, int64_t items, int64_t rows, float* out, int C);
int launch_se_apply(sd_ctx* c, bool f16, const void* t2, int t2_ld, const float* gate, const void* res, int res_ld, void* y, int y_ld, int C, int64_t rows,
                    const int2* rowtab, const int2* res_map, const int2* out_map);
int launch_asp_stats(sd_ctx* c, bool f16, const void* x, int ld, const int* nvalid, const int* rowoff, int row_base, int64_t items, int64_t rows, float* ms, int C);
int launch_asp_pool(sd_ctx* c, bool f16, const void* x, const float* logit, int ld, const int* nvalid, const int* rowoff, int row_base, int64_t items, int64_t rows,
                    float* pooled, int C);
int ecapa_row_plan(sd_ctx* c, const int* h_nvalid, int64_t n, EcapaRowPlan& plan, int* d_off /*[EC_SPACES][n + 1]*/);
// items [a0, a1) of the plan; d_feats = space-0 rows of ALL the plan's items
int run_ecapa(sd_ctx* c, const float* d_feats, const int* d_nvalid /*[n]*/, const EcapaRowPlan& plan, int64_t a0, int64_t a1, float* d_emb /*[n][192]*/);
// end index of every batch of the plan's items: whole items, at most cap_rows space-0 rows and ROWTAB_MAX_ITEMS items each (a single item always
// fits); balance = boundaries moved to where the wide-tile launches waste the least (ecapa.hip).  Pure host arithmetic on the prefix sums
std::vector<int64_t> ecapa_plan_batches(const EcapaRowPlan& plan, int64_t cap_rows, bool balance);
int64_t ecapa_round_items(int64_t nb);      // the item budget of a batch as it is used: a multiple of 96, at least 96
// all the plan's items in planned batches of a row budget of nb full-length items (run_ecapa per batch); x3 mode: repeats the batches on the f32
// kernels if an embedding came out non-finite
int ecapa_run_items(sd_ctx* c, const float* d_feats, const int* d_nvalid, const EcapaRowPlan& plan, int64_t nb, bool balance, float* d_emb);
int run_embed(sd_ctx* c, const DevWav& w, const float* d_masks, int64_t items, int64_t first_item, float* d_emb);
// ---- pyannet.hip
int run_segment(sd_ctx* c, const DevWav& w, int64_t chunk_lo, int64_t chunk_hi, float* d_seg);
// SegmentModel::infer as declared (sd.cpp:1352): rows = {rows.n / T separate waveforms of T samples, back to back; origin 0}
int run_segment_rows(sd_ctx* c, const DevWav& rows, int T, float* d_seg, int* frames);
// the launches of pyannet.hip's kernels, asynchronous on c->stream: grid, block and k_pool_norm's template choice are computed here; seg_batch and the test
// hooks of seg_test.hip call the same ones.  chunk_norm: xn [chunks][80000]; chunk_stats: st [chunks] (a, c), hop = 8000;
// pool_norm: stage 0 (C 80, pad 96, abs; cst != null: the shared form, chunk ck starts at row ck * chunk_rows of `in`), 1 or 2 (C 60, pad 64), Lp = Lc / 3;
// lstm_rec: G [B][F][1024] -> H [B][F][256], whx_f and whx_b non-null: k_lstm_rec_x3 on the split planes of lstm_whh_split, else k_lstm_rec;
// classifier: y [chunks * F][128] -> seg [chunks][293][3]
int launch_chunk_norm(sd_ctx* c, const float* d_wav, int64_t origin, int64_t first_chunk, int64_t hop, int L, int64_t chunks, float w, float b, float* xn);
int launch_chunk_stats(sd_ctx* c, const float* d_wav, int64_t origin, int64_t first_chunk, int L, int64_t chunks, float w, float b, float2* st);
int launch_pool_norm(sd_ctx* c, int stage, const float* in, int64_t chunks, int Lc, const float* gw, const float* gb, float* out,
                     const float2* cst, const float* wsum, int chunk_rows);
int launch_lstm_rec(sd_ctx* c, const float* G, const float* whh_f, const float* whh_b, const void* whx_f, const void* whx_b, float inv_f, float inv_b,
                    float* H, int64_t B, int F);
int launch_classifier(sd_ctx* c, const float* y, const float* W, const float* bias, float* seg, int64_t chunks, int F);
// ---- pipeline.cpp
int check_method_metric(sd_ctx* c, int method, int metric);      // the refusals of an entry that takes a linkage method and a metric from its caller; SD_OK = fine
// a 16-bit sample as the float the reference makes of it: sample * 1.0f / 32768.0 (sd.cpp:2948-2951); the division by 2^15 is exact in f32
__host__ __device__ __forceinline__ float pcm_to_float(int16_t s) { return (float)s * (1.0f / 32768.0f); }
__global__ void k_pcm_to_f32(const int16_t* __restrict__ pcm, float* __restrict__ dst, int64_t n);   // dst[0, n) = pcm / 32768, dst[n, n + SD_WAV_PAD) = 0; grid GRID1(n + SD_WAV_PAD)
__global__ void k_f32_to_f64(const float* __restrict__ a, double* __restrict__ b, int64_t n);          // embeddings widened before clustering (sd.cpp:2555); grid GRID1(n)
// the two producers of workspace "wav_f32": *out = {n samples, origin 0, padded}; a caller that uploaded a slice of a longer recording sets n and origin itself
int pcm_to_wav(sd_ctx* c, const int16_t* d_pcm, int64_t n, DevWav* out);
int f32_to_wav(sd_ctx* c, const float* h_wav, int64_t n, DevWav* out);
inline void clear_stage_ms(sd_ctx* c) { for (double& ms : c->stage_ms) ms = 0; }
// both networks on chunks [lo, hi) -> d_seg [hi-lo][293][3], d_emb [(hi-lo)*3][192]; seg_done: d_seg already holds the scores (stream.hip)
int shard_infer(sd_ctx* c, const DevWav& w, int64_t lo, int64_t hi, float* d_seg, float* d_emb, bool seg_done = false);
// the front of finalize, into buffers the caller names: binarised scores, active frames per row, the speaker count (d_count_avg may be null) and the
// embeddings widened to f64 (sd.cpp:2555)
int finalize_front(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, uint8_t* d_bin, int* d_nact, int32_t* d_count, double* d_count_avg, double* d_e64);
int finalize(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, std::vector<sd_turn>& v);
// the per-turn confidence of finalize (sdhip.h: sd_last_confidence) from the [chunks * 3] assignment behind the inactive rule and the best scores
void turn_confidence(const std::vector<sd_turn>& v, const std::vector<int>& hard, const std::vector<double>& soft_best, int64_t chunks, std::vector<double>& conf);
int turns_out(sd_ctx* c, const std::vector<sd_turn>& v, sd_turn** turns, int64_t* n_turns);
// ---- many.hip: both networks once over a pack of slots (many_plan.h).  sd_diarize_many* packs recordings, stream.hip the ranges of a group of streams
struct ManyRow { const void* src; int64_t n, base, len; };      // src[0, n) -> dst[base, base + n), zeros in dst[base + n, base + len)
struct ManyGap { int64_t first, count; };                         // chunks [first, first + count) belong to nobody
dim3 many_grid(int64_t longest, int64_t table);      // x: a stride over the longest row of a table, y: a stride over the table; 256 threads
// the launches of k_many_pack / k_many_gap_masks (d_rows / d_gaps: the table on the device, rows / gaps: the same table on the host, for the grid) and, in
// stream.hip, of the copy kernels (which: 0 k_group_append, 1 k_group_scatter, 2 k_group_tail_move; k_tail_move: src 16-byte aligned, dst an allocation's
// start): pack_infer, the stream stages and the hooks of input_test.hip call these
int launch_many_pack(sd_ctx* c, const ManyRow* d_rows, const std::vector<ManyRow>& rows, int is_f32, float* d_dst, int64_t dst_len);
int launch_many_gap_masks(sd_ctx* c, const ManyGap* d_gaps, const std::vector<ManyGap>& gaps, float* d_masks, int64_t total_chunks);
struct GroupRow;
int group_launch(sd_ctx* c, int which, const GroupRow* d_rows, const std::vector<GroupRow>& rows, int is_f32);
int launch_tail_move(sd_ctx* c, float* dst, const float* src, int64_t len);
// rows: one per slot that has a chunk, src on the device (is_f32: float samples, else 16-bit); total = many_plan's.  Leaves the scores [total][293][3]
// and embeddings [total * 3][192] of the pack in workspaces; stage_ms[0] and [1] are counted from t0
int pack_infer(sd_ctx* c, std::vector<ManyRow>& rows, int is_f32, const std::vector<PackRange>& rec, int64_t total, double t0, float** seg_out, float** emb_out);
// ---- ingest.hip: the fill step of sd_diarize_many_audio* (rows and plan: ingest_plan.h): the table as one block of bytes, [tile0: rows + 1 int64][rows],
// and ONE launch of k_many_ingest over it; many.hip and the hook of ingest_test.hip call these
struct IngestRow;
std::vector<char> many_ingest_table(const std::vector<IngestRow>& rows, const std::vector<int64_t>& tile0);
int launch_many_ingest(sd_ctx* c, const char* d_tab, const std::vector<IngestRow>& rows, const std::vector<int64_t>& tile0, int64_t max_span, float* d_dst, int64_t dst_len);
// the form of the samples an entry was handed, for the entries that come in three (sd_diarize_many*, sd_stream_push*, sd_stream_push_many*); the two
// _AUDIO forms are the frames of a stream with an input format (sd_stream_push_audio*, sd_stream_push_many_audio*), on the host or on the device
enum SampleForm { SD_PCM_HOST, SD_PCM_DEV, SD_F32_HOST, SD_AUDIO_HOST, SD_AUDIO_DEV };
// ---- stream_ingest.hip: ONE launch of k_group_ingest over a table (rows: stream_ingest_plan.h) with `pad` zeros behind every row; stream.hip and the
// hook of stream_ingest_test.hip call this
struct StreamIngestRow;
int launch_group_ingest(sd_ctx* c, const StreamIngestRow* d_rows, const std::vector<StreamIngestRow>& rows, int64_t pad);
// finalize, one job after the other, of a call with J outputs (sd_diarize_many*: recordings; sd_stream_turns_many: streams).  Presets turns / n_turns /
// status / c->many_jobs to "no job" (SD_ERR_SHORT), lets `infer` run the networks and name the rows of every job (chunks <= 0: none), then finalizes in
// list order: SD_ERR_NUMERIC is that job's own status, any other failure gives every turn list back and is returned; c->last is kept per job.
// `named` (may be empty) sees every job that ended SD_OK, with its turns handed over and c->last describing it, before c->last is kept: the roster of a
// stream renames the labels there (stream.hip); what it returns other than SD_OK ends the call like any other failure
struct FinalJob { const float* seg; const float* emb; int64_t chunks, n; };
int finalize_jobs(sd_ctx* c, int64_t J, sd_turn** turns, int64_t* n_turns, int32_t* status, const std::function<int(std::vector<FinalJob>&)>& infer,
                  const std::function<int(int64_t, sd_turn*, int64_t)>& named = nullptr);
// ---- cut.hip: the tail of the sd_cut_open* entries (sdhip.h, "many cuts of one dendrogram"); refuses a gallery and a dump directory itself
int cut_refusal(sd_ctx* c, const char* who);
int cut_open_dev(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, sd_cut** out);
// ---- resample.hip
int resample_dev(sd_ctx* c, const float* d_in, int64_t n, int32_t in_sr, int32_t out_sr, float* d_out, int64_t n_out);
// the windowed form behind sd_stream_set_input_rate (stream.hip; rows and plan: resample_book.h): the refusals of a rate pair, its cached tap table, and
// ONE launch of k_resample_jobs for any number of rows
struct ResamplePlan;
struct ResampleJob;
int resample_check(sd_ctx* c, int32_t in_sr, int32_t out_sr, ResamplePlan& p);
int resample_taps(sd_ctx* c, int32_t in_sr, int32_t out_sr, const ResamplePlan& p, const float** taps);
int resample_jobs(sd_ctx* c, const ResampleJob* rows, int64_t R);
// ---- postseg.hip
int run_postseg(sd_ctx* c, const float* d_seg, int64_t chunks, uint8_t* d_bin, float* d_masks, int* d_nact);
int run_count(sd_ctx* c, const uint8_t* d_bin, int64_t chunks, int32_t* d_count, int64_t n_count, double* d_avg = nullptr);
// ---- stepdump.cpp
int write_step_dumps(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n_samples, const std::vector<int>& hard_post, int K);
int64_t count_frames_host(int64_t chunks);
int sd_np_rint_host(double v);
int64_t closest_frame_host(double w_start, double w_step, double w_dur, double t);
// ---- linkage.hip
int run_linkage(sd_ctx* c, const double* d_X, int64_t N, int d, double* d_Z, int method = SD_LINKAGE_CENTROID, int metric = SD_METRIC_EUCLIDEAN);
int run_linkage_host(sd_ctx* c, const double* d_X, int64_t N, int d, int method, int metric, std::vector<double>& Z);      // cluster.hip: run_linkage, Z on the host
// ---- linkage_batch.hip: J independent jobs, rows on the device, Z [N - 1][4] of each to the host.  The jobs run_linkage would give to its one-workgroup
// kernel share launches (one workgroup per job, linkage_batch_plan.h), under option linkage_batch_xcd those of its one-XCD cooperative kernel too (eight to a
// launch, one per XCD; under option linkage_batch_xcd_zero those of them that tie at height 0 stay there), the others go through run_linkage; every Z is the bytes run_linkage gives for the
// job alone.  status[j] = SD_OK, or SD_ERR_NUMERIC for a job with a zero-norm row under the cosine metric (its Z is left as it was); any other failure is returned
struct LinkageManyJob { const double* d_X; int64_t N; double* h_Z; };
int run_linkage_many(sd_ctx* c, const LinkageManyJob* jobs, int64_t J, int d, int method, int metric, int32_t* status);
bool linkage_job_shares_launches(const sd_ctx* c, int64_t N, int method);      // would run_linkage_many take a job of N rows into a shared launch (given company)?
int run_clustering(sd_ctx* c, const double* d_emb /*[M][d] f64*/, int64_t M, int d, std::vector<int>& hard, int* K,
                   int num_clusters = -1, int min_clusters = -1, int max_clusters = -1, std::vector<double>* soft_best = nullptr);
// ---- activity.hip
int64_t activity_frames_host(int64_t chunks);                     // frames aggregate() yields for `chunks` chunks (sd.cpp:1232-1234)
int64_t activity_rows_host(int64_t nf, int64_t n_samples);        // ... without those that lie wholly in the last chunk's zero padding
int run_activity_scores(sd_ctx* c, const float* d_seg, int64_t chunks, int kind, double* d_scores, int64_t nf);
int run_activity_regions(sd_ctx* c, const double* d_scores, int64_t rows, int label, std::vector<sd_turn>& turns);
// ---- speakers.hip
int check_spans(sd_ctx* c, const sd_turn* spans, int64_t n_spans, const char* who);      // 0 <= start <= end, numbers; touches nothing but c->err
void spans_to_samples(const sd_turn* spans, int64_t n_spans, int32_t label, int64_t n, std::vector<int64_t>& out);      // -> sorted, merged [first, end) sample pairs
int run_span_masks(sd_ctx* c, const std::vector<int64_t>& spans, int64_t chunks, int64_t n, float* d_masks /*[chunks * 3][293]*/);
int run_voiceprint_mean(sd_ctx* c, const float* d_emb /*[chunks * 3][192]*/, int64_t chunks, double* h_mean /*[192]*/, int64_t* n_live);      // synchronises
int run_speaker_dist(sd_ctx* c, const double* d_cen, int64_t K, const double* d_gal, int64_t M, int d, double* d_dist, double* h_dist /*[K][M]*/);      // synchronises
int run_gallery_norms(sd_ctx* c, const double* d_gal, int64_t M, int d, double* d_m2 /*[M]*/);      // asynchronous
int run_nearest_gallery(sd_ctx* c, const double* d_E, const int* d_tidx /*[N] or null*/, int64_t N, const double* d_gal, const double* d_m2, int64_t M, int d,
                        int* d_best /*[N]*/, double* d_dist /*[N]*/);      // synchronises
// ---- cluster.hip: the steps of run_clustering that cut.hip shares: the front (train rows, X / Xn / dendrogram), the one finish of a cut, the centroids
int train_rows(sd_ctx* c, const double* d_e64, int64_t M, int d, std::vector<int>& tidx);
int cluster_rows(sd_ctx* c, const double* d_emb, const std::vector<int>& idx, int d, double** Xout, double** Xnout, std::vector<double>& Z);
int linkage_rows(sd_ctx* c, const double* d_emb, const std::vector<int>& idx, int d, double* out /*[N][d], device*/);      // the rows cluster_rows gives the linkage (context's method); asynchronous
int cluster_cut(sd_ctx* c, const std::vector<double>& Z, int64_t N, const double* X, int d, const ClusterSpec& spec, ClusterPlan& p, std::vector<int>* first_cut);
int mean_of_rows(sd_ctx* c, const double* d_emb, int d, const std::vector<int>& tidx, std::vector<double>& h_cen);
int final_means(sd_ctx* c, const double* X, int d, const std::vector<int>& lab, int nl, int G, std::vector<int>& order, std::vector<int>& off, double** cen_out);
int assign_all(sd_ctx* c, const double* d_emb, int64_t M, int d, const double* d_cen2, int K, const std::vector<int64_t>& counts,
               std::vector<int>& hard, int* Kout, std::vector<double>* soft_best, double** soft_out, JobResult& res);
// ---- the launches of the back end's kernels, asynchronous on c->stream: grid, block and LDS are computed here, once; the stage functions above and
// the test hooks of backend_test.hip call the same ones.  cluster.hip: gather_normalize (Xout may be null), cluster_means (nl blocks of min(d rounded
// up to 64, 1 024) threads), assign (soft / best may be null), constrained_argmax (K <= 64)
int launch_gather_normalize(sd_ctx* c, const double* d_emb, const int* d_tidx, int64_t N, int d, double* Xout, double* Xn);
int launch_cluster_means(sd_ctx* c, const double* X, int d, const int* d_order, const int* d_off, int nl, double* d_cen);
int launch_assign(sd_ctx* c, const double* E, int64_t M, int d, const double* cen, int K, int* hard, int* err, double* soft, double* best);
int launch_constrained_argmax(sd_ctx* c, const double* soft, int64_t chunks, int K, double fill, int* hard);
// reconstruct.hip: act [nact][K]; binary [rows][K] from rows [ar0, ar0 + rows) of act and entries [cr0, cr0 + crow) of count
int launch_activations(sd_ctx* c, const float* d_seg, const int* d_hard, const int* d_sfr, int64_t chunks, int K, double* d_act, int64_t nact);
int launch_topk(sd_ctx* c, const double* d_act, const int32_t* d_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow, int K, uint8_t* d_binary);
// cut.hip: the batched twins; total = coff[Tn] rows of the centroid table, sumK = koff[Tg] label columns
int launch_cut_cen_norms(sd_ctx* c, const double* d_cen, int total, int d, double* d_m2);
int launch_assign_cuts(sd_ctx* c, const double* E, int64_t M, int d, const double* d_cen, const double* d_m2, const int* d_coff, const int* d_slot, int Tn,
                       const int* d_nact, int* d_hard, double* d_best, int* d_err);
int launch_activations_cuts(sd_ctx* c, const float* d_seg, const int* d_hard, const int* d_sfr, int64_t chunks, const int* d_koff, int Tg, int64_t sumK,
                            double* d_act, int64_t nact);
int launch_topk_cuts(sd_ctx* c, const double* d_act, const int32_t* d_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow, const int* d_koff, int Tg,
                     int64_t nact, uint8_t* d_binary);
// pipeline.cpp: the widening of the embeddings and the inactive rule (sd.cpp:2555, 3172-3191)
int launch_f32_to_f64(sd_ctx* c, const float* d_a, double* d_b, int64_t n);
int launch_mark_inactive(sd_ctx* c, int* d_hard, const int* d_nact, int64_t n);
// ---- cluster.hip: the three refusals of a call that clusters under an enrolled gallery (SD_ERR_ARG; nothing is touched); SD_OK without a gallery
int enrolled_refusal(sd_ctx* c, int d, int num_clusters, int min_clusters, int max_clusters);
// ---- reconstruct.hip
// what run_reconstruct derives from the sizes of a job alone: the activation frames, the first frame of every chunk, the crop of activations and
// counts to their common extent (sd.cpp:2691-2706) and the start of the cropped window
struct ReconFrames { int64_t nact = 0, ar0 = 0, cr0 = 0, rows = 0, crow_all = 0; float astart = 0; std::vector<int> sfr; };
void reconstruct_frames(int64_t chunks, int64_t n_count, int64_t n_samples, ReconFrames& g);
void to_annotation_host(const std::vector<uint8_t>& binary, int64_t rows, int K, double w_start, std::vector<sd_turn>& out);
int run_reconstruct(sd_ctx* c, const float* d_seg, const int* d_nact, const int* d_hard, const int32_t* d_count,
                    int64_t n_count, int64_t chunks, int64_t n_samples, int K, std::vector<sd_turn>& turns);
