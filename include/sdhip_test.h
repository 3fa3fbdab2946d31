/*
 * sdhip_test.h -- test, measurement and tuning hooks of libsdhip.so.
 *
 * Nothing in this header replaces a reference interface: these entry points exist for tests/, bench.py and tools/ only (the
 * drop-in boundary is sdhip.h, whose every entry cites the reference code it stands in for).  The symbols are exported by the
 * same library; a host program that only diarizes never needs this file.
 */
#ifndef SDHIP_TEST_H
#define SDHIP_TEST_H
#include "sdhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- planted workload (measurement / test hook, SURVEY 8d: "with synthetic weights force a deterministic activity
 * pattern for stage >= a4 (override sigmoid outputs from the schedule) so N is controlled").  With seeded random
 * weights PyanNet and ECAPA do not follow the talkers, so every stage after them would only ever see one degenerate
 * case (K = 1, one turn).  After this call sd_diarize* / sd_shard_infer_dev still run both networks at full cost, then
 * replace the segmentation scores of chunks [chunk_lo, chunk_lo + chunks) by d_scores [chunks][293][3] before
 * post-segmentation, and the embedding rows of those chunks that are not NaN by the reference's own rule
 * (sd.cpp:2479-2549) by d_emb [chunks*3][192] before the all-gather / clustering.  Either pointer may be NULL; the
 * buffers stay owned by the caller and must outlive the calls; chunks = 0 removes the hook.  Never set by the CLI. */
int sd_set_planted(sd_ctx*, const float* d_scores, const float* d_emb, int64_t chunk_lo, int64_t chunks);

/* ---- measurement hooks (bench.py): GPU time of named kernels measured with hipEvents on the library's own stream
 * (option "profile" = 1), with the algorithmic FLOPs / bytes the launcher bills them. */
int sd_kernel_stats(const sd_ctx*, const char* kernel, double* total_ms, int64_t* launches, double* flops, double* bytes);
void sd_reset_stats(sd_ctx*);
/* copy `bytes` of the library's named device workspace (from byte `offset`) to the host: intermediate activations for the precision
 * diagnostics under tools/ ("ec_x0", "ec_cat", "ec_mfa", "ec_pooled", ...) */
int sd_debug_read_ws(sd_ctx*, const char* name, int64_t offset, void* h_out, int64_t bytes);
/* host only: the split-weight packing of option ecapa_precision = 3 (weights.cpp) on host buffers.  w = [K][Cout][CinPad] floats (CinPad a
 * multiple of 32, channels >= cin ignored), out_halves = 2 * K * Cout * CinPad fp16 bit patterns: per 32-channel chunk of a row
 * [hi 0..7 | lo 0..7 | hi 8..15 | ...] of w * 2^e; *inv_scale = 2^-e */
int sd_test_pack_split_weights(const float* w, int K, int Cout, int CinPad, int cin, uint16_t* out_halves, float* inv_scale);
/* host only, no context: the batches the embedding stage forms for n items of nvalid[i] valid frames (1 .. 501) at option emb_batch_items =
 * batch_items (rounded as the stage rounds it: down to a multiple of 96, at least 96) and option skip_dead_rows.  balance = 0: the greedy
 * rule of sd_ecapa / sd_embed_signals (whole items while batch_items * 501 rows of the widest row space and 4 095 items hold them);
 * balance = 1: the rule of the whole path, boundaries moved to where the wide-tile launches waste the least (ecapa.hip).  Writes the end
 * index (exclusive) of every batch to bounds[0 .. cap) and returns the number of batches, or -SD_ERR_ARG (n < 0, cap < 0, a null pointer
 * with n > 0, more batches than cap, or a row space of more than 0x7fffffff / 4 rows, which the stage's int offsets refuse too). */
int64_t sd_test_emb_batches(const int32_t* nvalid, int64_t n, int64_t batch_items, int skip_dead_rows, int balance, int64_t* bounds, int64_t cap);
/* test / tuning keys of sd_set_option (defaults are the measured optimum; results do not depend on the tuning keys):
 * "profile", "emb_batch_items", "seg_batch_chunks", "linkage_wgs" (-1 auto, 0 one workgroup), "linkage_threads", "linkage_one_xcd",
 * "skip_dead_rows", "virtual_world" (test mode: a communicator of ONE rank plays all W ranks of the plan in turn, slot by slot, so plan +
 * slot assembly + status exchange of a W-GPU job run on a 1-GPU box), "inject_fail_rank" (test: that rank -- a played rank under
 * virtual_world -- reports SD_ERR_ARG instead of inferring; every rank must then return an error for the job),
 * "conv_h256" / "conv_w256_f32" (256 x 256 tile for the wide ECAPA layers in fp16 / f32), "conv_glds" (fp16: that tile staged by LDS-DMA,
 * conv_gemm_g.hip, instead of through registers; same bits; default 1), "conv_glds_f32" (the same for f32: same bits, measured 5 % slower, default 0), "conv_rot" (LDS-DMA kernel, bit 0: the workgroups that
 * share a row / column panel request its four quarters in rotated order; bit 1: a wave's DMA pieces pair up inside one quarter; same bits; default 3), "conv_mfma16" (that kernel on
 * v_mfma_f32_16x16x32_f16 instead of 32x32x16: the chip holds a higher clock on it; default 1; 2 = on short contractions (block0) too: the form the round-6
 * kernel is compared with bit for bit), "conv_pp" (fp16: the wide layers with K >= 512 and M >= 2 048 on the never-drained kernel of round 6, conv_gemm_p.hip;
 * same bits as "conv_glds"; default 1), "conv_stagger" (128 x 128 f32 kernel: half of
 * the workgroups start half a tile late; 0 off (default, no effect measured), 1 / 2), "conv_w256_kmin" (shortest contraction that tile
 * takes), "conv_pn" / "conv_pn128" (column tiles per super-block), "ecapa_ld_pad" (elements added to the activation rows, multiple of 8),
 * "conv_res2_ws" (f32 Res2Net convs -- Cin = Cout = 128, 3 taps, a row table over one row space, M >= 2 048 -- on the weight-stationary kernel,
 * conv_res2.hip; 0 = on the 128 x 128 kernel as before; same bits; default 1), "conv_res2_wgs" (that kernel's workgroups, 0 .. 4 096; 0 = one per CU (default); same bits),
 * "seg_shared_conv0" (1 = SincNet's first convolution once over the waveform instead of once per overlapping chunk), "seg_wide_ih" (1 = LSTM input
 * projections of layers 1-3 on the 256 x 256 tile), "linkage_square" (-1 auto, 0 condensed, 1 full N x N distance matrix), "ecapa_f16_hp" /
 * "ecapa_keep_cat" (precision diagnostics of tools/diag_fp16_layers.py), "linkage_kernel" (-1 auto / 1: k_linkage_rg for the square matrix where its geometry fits,
 * 0: k_linkage_mw), "linkage_tie_kernel" (what finishes a job with exact ties: 1 = k_linkage_hx, n > 1 = with n worker workgroups, 0 = k_linkage_heap),
 * "linkage_zero_phase" (1, default: after a tie at height 0 the replay takes the merges at height 0 only and k_linkage_rg the rest; 0: whole replay),
 * "linkage_force_heap" (1 = skip the cooperative kernel: the heap replay on tie-free data), "linkage_hx_wide" (1 = k_linkage_hx's 32-bit key / position form, which
 * jobs above 65 535 rows take, on any size), "linkage_prefetch" (1 = k_linkage_rg's helper wave; measured: no gain), "ws_limit_mb" (test: PROCESS-WIDE, a workspace request above this many
 * MB fails as on an exhausted GPU; 0 = off), "emb_batch_default" (test: forget an explicit "emb_batch_items"; value = embedding calls the
 * context pretends to have made, 0 = the next one plans the small first-job arena), "cut_group_bytes" (sd_cut_turns_many: the bytes the
 * activation tables of one group of cuts may take, default 1 GiB, at least 1; a cut that alone takes more is a group of one) and
 * "linkage_batch_threads" (k_linkage_heap_jobs: threads of the workgroup of a job; 0 auto (default: 256, the measured choice), 256 or 1024; same bits). */
/* environment (diagnostic): SD_TRACE_CREATE=1 prints where sd_create's time goes; SD_TRACE_WS=1 makes sd_diarize_dev print the job's stage times and what the
 * process's workspace hipMalloc / hipFree calls have cost so far (count, GB, ms) with every workspace of 256 MB or more. */
/* tuning hook (tools/): time one conv_gemm shape on scratch data (dbg = 100 * pad_units + 10 * (sched + 1); a non-zero last digit,
 * which chose an ablation build until those were retired, is SD_ERR_ARG) */
int sd_bench_conv(sd_ctx*, int64_t items, int Tp, int T, int Cin, int Cout, int KT, int dil, int has_x2, int dbg, int reps, double* ms_per_launch);

/* ---- test hook (tests/test_conv_kernels.py): ONE conv / linear case through the product's dispatch (launch_conv_narrow when asked, then
 * launch_conv_gemm), on operands the caller chooses, with guard regions round every buffer.  The hook uploads, launches and downloads; the
 * row table, the fp16 / split weight forms and the fp16 activations are made by the product's own kernels.
 * Row spaces.  dense = 0: compact spaces through a row table: item i stores n_in[i] input rows and n_out[i] output rows (1 .. 1024,
 * n_out[i] <= tin); M = sum n_out, in_rows = sum n_in.  dense = 1: no row table; every item has tp_in input rows (tin valid) and tp_out
 * output rows (t valid); M = items * tp_out, in_rows = items * tp_in; n_in / n_out are not read.
 * Buffers.  shared = 0: X, X2 and Y each live in a buffer of their own: X at column x_col0 of [in_rows + 256][x_ld], X2 at column x2_col0 of
 * a second buffer of that shape, Y at column y_col0 of [M + 256][y_ld].  shared = 1: all three are column slices of ONE [M + 256][y_ld]
 * buffer (x_ld == y_ld, in_rows == M: the Res2Net pattern).  An X slice is cin_pad columns wide: cin operands, then zeros.  Everything else
 * holds `canary`, except the 256 slack rows of the X / X2 slices, which hold NaN.  fp16 (prec 1): the buffers are built in f32 and rounded
 * to fp16 by the product's conversion kernel.
 * cin_pad = 0: the product's padding rule (a multiple of 32; of 64 for prec 1); else the padded channel count as given (contract tests).
 * prec: 0 f32, 1 fp16 end to end (y_f32 = 1: Y stays float), 3 split operands.  act1: 0 none, 1 relu, 2 leaky; act2: 0 none, 1 tanh, 2 sigmoid. */
typedef struct sd_conv_case {
    int32_t items, dense, tin, t, tp_in, tp_out;
    int32_t cin, cin_pad, cout, kt, dil, pad_mode;
    int32_t shared, x_ld, x_col0, has_x2, x2_col0, y_ld, y_col0, y_f32;
    int32_t act1, act2, prec, try_narrow;
    float canary;
} sd_conv_case;
/* w [kt][cout][cin], x / x2 [in_rows][cin], bias / scale / shift [cout] (scale and shift come together), item_bias [items][cout]: host
 * pointers, f32, each optional except w and x.  y_out [(M + 256) * y_ld] receives the WHOLE output buffer as f32, guards included;
 * kernel_name (name_cap bytes) the name of the kernel the dispatch launched last ("" = none): pp_relu, pp, g256_m16, g256_m32, g256_f32,
 * w256_f32, w256_f16, w256_x3, skinny, gemm128_{f32,f16,x3}[_x2], narrow2, narrow3. */
int sd_test_conv(sd_ctx*, const sd_conv_case*, const int32_t* n_in, const int32_t* n_out, const float* w, const float* x, const float* x2,
                 const float* bias, const float* scale, const float* shift, const float* item_bias, float* y_out, char* kernel_name, int name_cap);

/* ---- test hooks (tests/test_seg_kernels.py): ONE launch of one kernel of the segmentation network (csrc/pyannet.hip) on operands the caller chooses,
 * through the launcher the product's seg_batch calls (grid, block and template choice are the product's).  Host pointers, f32.  A hook uploads,
 * launches and downloads; it restates no kernel logic.  Guards: every input is followed by NaN (256 rows of the operand's row width behind an
 * activation, 256 floats behind a parameter vector); every output buffer is filled with `canary` and has 256 slack rows behind it, and comes back
 * WHOLE, slack included.  A case whose defined reads do not lie inside the operand given is refused with SD_ERR_ARG before anything is launched.
 *
 * sd_test_lstm_rec: k_lstm_rec (prec 0) / k_lstm_rec_x3 (prec 3: the split planes of W_hh are made by the loader's own function).  G [B][F][1024]:
 * per direction 512 = gates i, f, g, o x 128 units (the input projection plus both biases); whh_f / whh_b [512][128].  h_out [(B * F + 256)][256].
 * sd_test_pool_norm: k_pool_norm; stage 0 (C = 80 channels, rows of 96, |.| first), 1 or 2 (C = 60, rows of 64).  in [in_rows][C], in_rows =
 * chunks * Lc; gw / gb [C].  cst != NULL (stage 0 only) selects the shared form: cst [chunks][2] = (a, c) of k_chunk_stats, wsum [80], chunk ck
 * starts at row ck * chunk_rows, in_rows = (chunks - 1) * chunk_rows + Lc.  out [(chunks * (Lc / 3) + 256)][96 or 64].
 * sd_test_chunk_norm: k_chunk_norm (stats_only = 0): chunk ck = samples [(first_chunk + ck) * hop - origin, + L) of wav [n_wav];
 * out [chunks * 80000 + 1024].  stats_only = 1: k_chunk_stats (hop must be 8000); out [(chunks + 256)][2] = (a, c).
 * sd_test_classifier: k_classifier; y [chunks * F][128], W [3][128], bias [3], F <= 293; seg_out [(chunks * 293 + 256)][3]. */
int sd_test_lstm_rec(sd_ctx*, const float* G, const float* whh_f, const float* whh_b, int64_t B, int F, int prec, float canary, float* h_out);
int sd_test_pool_norm(sd_ctx*, const float* in, int64_t in_rows, int64_t chunks, int Lc, int stage, const float* gw, const float* gb,
                      const float* cst, const float* wsum, int chunk_rows, float canary, float* out);
int sd_test_chunk_norm(sd_ctx*, const float* wav, int64_t n_wav, int64_t origin, int64_t first_chunk, int64_t hop, int L, int64_t chunks,
                       float w, float b, int stats_only, float canary, float* out);
int sd_test_classifier(sd_ctx*, const float* y, const float* W, const float* bias, int64_t chunks, int F, float canary, float* seg_out);

/* ---- test hooks (tests/test_ecapa_glue.py): ONE launch of one glue kernel of the embedding network (csrc/ecapa.hip) through the launcher run_ecapa_t
 * calls, under the contract of the segmentation hooks above: host pointers, f32; every input followed by NaN (256 rows of the operand's row width, 256
 * elements behind a vector); every output filled with `canary`, 256 slack rows behind it, back WHOLE; a case whose defined reads leave its operands is
 * SD_ERR_ARG before any launch.  f16 = 1: the activations are _Float16: built in f32 as given, rounded by the product's own conversion kernel
 * (k_rows_to_half), and an fp16 output comes back widened to f32.  Leading dimensions are multiples of 4.
 *
 * sd_test_ecapa_stats: kind 0 = k_masked_mean -> out [items + 256][C]; 1 = k_asp_stats, 2 = k_asp_pool -> out [items + 256][2 C] = (mean | std).
 * x [rows][ld] (and logits [rows][ld], f32 in either mode, kind 2 only; else NULL), rows = rowoff[items] - row_base; item i's rows start at
 * rowoff[i] - row_base and its frames < nvalid[i] are read: 1 <= nvalid[i] <= rowoff[i + 1] - rowoff[i].  rowoff [items + 1] ascending, rowoff[0] =
 * row_base >= 0: the items of a larger plan in front of this batch.  C <= ld; the pad columns ld - C are the caller's (NaN in the tests).
 * sd_test_se_apply: y = gate[item] * t2 + residual (k_se_apply) over the rows of space `os`.  off [4][items + 1]: prefix sums (off[s][0] = 0) of the rows
 * each item stores in four row spaces; item i's frame t is row off[s][i] + t.  The row tables come from ecapa_build_rowtab on these sums.
 * t2 [Mo][t2_ld], gate [items][C], C % 4 == 0, Mo = off[os][items].
 * shared = 0 (the first block): res [off[rs][items]][res_ld] is a buffer of its own in space rs, mapped when rs != os; the output is column slice
 * [out_col0, + C) of a [off[ys][items] + 256][y_ld] canary buffer, mapped when ys != os.  shared = 1 (the later blocks): res [off[ys][items]][C] is
 * laid into column slice [res_col0, + C) of that same buffer (rs == ys, res_ld ignored; its 256 slack rows hold NaN), the output goes to slice
 * [out_col0, + C), disjoint from it.  Every item must store at least as many rows in spaces rs and ys as in os.  y_out = the whole
 * [off[ys][items] + 256][y_ld] buffer.
 * sd_test_rowtab: k_build_rowtab; off_out / off_in [items + 1] prefix sums with bases base_out = off_out[0], base_in = off_in[0]; items <= 4095, at
 * most 1024 rows per item.  tab_out [(off_out[items] - base_out + 128)][2] int32: the table and its 128 slack entries, preset to (canary, canary).
 * sd_test_scatter_emb: k_scatter_emb; emb_c [n_c][192], cidx [items] (-1 = dropped, else < n_c) -> emb_out [items + 256][192].
 * sd_test_to_half: kind 0 = k_feats_to_half: f [rows][96] -> h_out [rows + 256][128] fp16 bit patterns (the slack holds the bits of fp16(canary));
 * kind 1 = k_rows_to_half: f [rows][width], width % 4 == 0 -> h_out [rows + 256][width]. */
int sd_test_ecapa_stats(sd_ctx*, int kind, int f16, const float* x, const float* logits, const int32_t* nvalid, const int32_t* rowoff, int64_t items,
                        int row_base, int C, int ld, float canary, float* out);
int sd_test_se_apply(sd_ctx*, int f16, int shared, const float* t2, int t2_ld, const float* gate, const float* res, int res_ld, int res_col0, int out_col0,
                     int y_ld, int C, const int32_t* off, int64_t items, int os, int rs, int ys, float canary, float* y_out);
int sd_test_rowtab(sd_ctx*, const int32_t* off_out, const int32_t* off_in, int64_t items, int32_t canary, int32_t* tab_out);
int sd_test_scatter_emb(sd_ctx*, const float* emb_c, int64_t n_c, const int32_t* cidx, int64_t items, float canary, float* emb_out);
int sd_test_to_half(sd_ctx*, int kind, const float* f, int64_t rows, int width, float canary, uint16_t* h_out);

/* ---- test hooks (tests/test_frontend_kernels.py): the kernels of the embedding front end (csrc/frontend.hip) through the functions run_embed, sd_frontend
 * and sd_embed_signals call, under the contract of the hooks above: host pointers; every input followed by 256 guard units of NaN; every output preset to a
 * canary, 256 slack entries (rows) behind it, back WHOLE; a case whose defined reads leave its operands is SD_ERR_ARG before any launch.  The window, the
 * twiddles and the sparse mel bank are the context's (weights.cpp): a case that needs others loads another pack.
 *
 * sd_test_frontend_prepare: frontend_prepare as run_embed (compact = 1) or sd_frontend (compact = 0) calls it: k_mask_prefix, k_wav_lens and, under
 * compact, k_compact_active.  masks [items][293] (followed by 256 x 293 NaN), first_item a multiple of 32.  Out, each with 256 slack entries and preset to
 * icanary (the float array: fcanary): prefix [items * 296 + 256] (columns 294 / 295 of a row are never written), counts, wav_lens, nnorm, nvalid, flags
 * [items + 256] per ITEM; under compact also alist, cidx, nnorm_c, nvalid_c [items + 256] and n_active [4] (entry 0 written); with compact = 0 those five
 * may be NULL and are not touched.
 * sd_test_frontend_features: the first half of run_embed in its order: frontend_prepare(compact), ecapa_row_plan, frontend_features (k_stft_fbank),
 * with option skip_dead_rows as given for this call.  wav [n_held] is the slice of a recording of n_total samples that starts at sample `origin`; it is
 * uploaded with 256 NaN in front of it and 256 NaN behind it.  Refused: a live item whose chunk ((first_item + item) / 3) * 8000 starts before origin, or
 * a slice that ends before min(n_total, end of the last live item's chunk).  feats_out [feat_rows][96], feat_rows = rows of all live items + 256 exactly
 * (else SD_ERR_ARG: the caller knows the row plan it expects), preset to canary; rowoff_out [items + 1] (entries 0 .. n_active written), cidx_out [items];
 * info_out [4] = n_active, rows_all, the grid frontend_features gave the k_stft_fbank launch (it records it in the context), compute units.
 * sd_test_frontend_signals: the path of sd_embed_signals up to and including frontend_features (sig_mode): signals [B][80000] (256 NaN in front, 256 NaN
 * behind), wav_lens [B] under sd_embed_signals' own rule.  prefix_out [B * 296 + 256] and counts_out [B + 256]: the tables of k_identity_prefix, preset to
 * icanary.  The other outputs as above (cidx is the identity and is not returned). */
int sd_test_frontend_prepare(sd_ctx*, const float* masks, int64_t items, int64_t first_item, int compact, int32_t icanary, float fcanary, int32_t* prefix,
                             int32_t* counts, float* wav_lens, int32_t* nnorm, int32_t* nvalid, int32_t* flags, int32_t* alist, int32_t* cidx,
                             int32_t* nnorm_c, int32_t* nvalid_c, int32_t* n_active);
int sd_test_frontend_features(sd_ctx*, const float* wav, int64_t n_held, int64_t n_total, int64_t origin, int64_t first_item, const float* masks,
                              int64_t items, int skip_dead_rows, float canary, float* feats_out, int64_t feat_rows, int32_t* rowoff_out,
                              int32_t* cidx_out, int64_t* info_out);
int sd_test_frontend_signals(sd_ctx*, const float* signals, const float* wav_lens, int64_t B, int skip_dead_rows, int32_t icanary, float canary,
                             int32_t* prefix_out, int32_t* counts_out, float* feats_out, int64_t feat_rows, int32_t* rowoff_out, int64_t* info_out);

/* ---- test hooks (tests/test_backend_kernels.py): ONE launch of one kernel behind the two networks (csrc/postseg.hip, cluster.hip, reconstruct.hip, cut.hip and
 * the casts of pipeline.cpp) through the function the product's stage calls (grid, block and LDS are the product's), under the contract of the hooks above:
 * host pointers; every input is followed by 256 guard units -- NaN for floating-point operands, for integer and byte operands a value that would change
 * a result (named per hook) --, a unit being a row where the operand has rows and an element otherwise; every output is preset to a canary (fcanary for
 * float and double, icanary for int32, SD_TEST_BCANARY for bytes), has 256 slack units behind it and comes back WHOLE; a case whose defined reads leave
 * its operands is SD_ERR_ARG before any launch.  An output pointer documented as optional may be NULL: the kernel then gets a null pointer, as in the product.
 *
 * sd_test_binarize: k_binarize_masks (run_postseg).  seg [chunks][293][3] -> bin [(chunks + 256) * 879] bytes, masks [(chunks + 256) * 3][293],
 *   nact [(chunks + 256) * 3]; each optional.
 * sd_test_count: k_count with run_count's geometry.  bin [chunks][293][3] bytes (guard bytes 0x55) -> count [sd_count_frames(chunks) + 256] and, optional,
 *   avg of the same length.
 * sd_test_gather_normalize: k_gather_normalize.  X [rows][d], tidx [N] in [0, rows) (guard: `rows`, the first NaN row) -> xout (optional) and xn [N + 256][d].
 * sd_test_cluster_means: k_cluster_means.  X [rows][d], order [off[nl]] in [0, rows) (guard: `rows`), off [nl + 1] ascending from 0 (guard: 0)
 *   -> cen [nl + 256][d].
 * sd_test_assign: k_assign.  E [M][d], cen [K][d] -> hard [M + 256], err [1 + 256] (entry 0 cleared before the launch, as assign_all clears it), soft
 *   [(M + 256) * K] (optional), best [M + 256] (optional).
 * sd_test_constrained_argmax: k_constrained_argmax.  soft [chunks][3][K], 1 <= K <= 64, fill = the caller's (Clustering.py:83) -> hard [(chunks + 256) * 3].
 * sd_test_activations: k_activations with reconstruct_frames' first frames.  seg [chunks][293][3], hard [chunks][3] (guard: 0) -> act [nact + 256][K];
 *   *nact_out = the frames (rows of act that the kernel writes).
 * sd_test_topk: k_topk.  act [act_rows][K], count [n_count] (guard: 0x7fffffff); 0 <= ar0, ar0 + rows <= act_rows, 0 <= crow <= rows, 0 <= cr0,
 *   cr0 + crow <= n_count -> binary [(rows + 256) * K] bytes.
 * sd_test_assign_cuts: k_cut_cen_norms, then k_assign_cuts.  E [M][d], cen [coff[Tn]][d], coff [Tn + 1] strictly ascending from 0 (guard: coff[Tn]), slot
 *   [Tn] distinct in [0, n_slots) (guard: 0), nact [M] (guard: 0) -> m2 [coff[Tn] + 256], hard [n_slots * M + 256], best [Tn * M + 256], err [1 + 256].
 * sd_test_recon_cuts: k_activations_cuts, then k_topk_cuts.  seg [chunks][293][3], hard [Tg][chunks * 3] (guard: 0), koff [Tg + 1] strictly ascending from 0
 *   (guard: koff[Tg]), count [n_count] (guard: 0x7fffffff) -> act [nact * koff[Tg] + 256], binary [rows * koff[Tg] + 256] bytes.  act_in (optional,
 *   [nact * koff[Tg]]): k_topk_cuts reads this table (NaN behind it) instead of the one k_activations_cuts wrote.  ar0 + rows <= nact, the rest as sd_test_topk.
 * sd_test_pcm_to_f32: k_pcm_to_f32 (pcm_to_wav).  pcm [n] (guard: 0x7fff) -> wav [n + 512 + 256]: the samples, the 512 zeros, the canary.
 * sd_test_f32_to_f64: k_f32_to_f64.  a [n] -> b [n + 256].
 * sd_test_mark_inactive: k_mark_inactive.  hard [n] (in), nact [n] (guard: 0) -> hard_out [n + 256]: the table behind the rule, then icanary. */
#define SD_TEST_BCANARY 0xA5
int sd_test_binarize(sd_ctx*, const float* seg, int64_t chunks, float fcanary, int32_t icanary, uint8_t* bin_out, float* masks_out, int32_t* nact_out);
int sd_test_count(sd_ctx*, const uint8_t* bin, int64_t chunks, float fcanary, int32_t icanary, int32_t* count_out, double* avg_out);
int sd_test_gather_normalize(sd_ctx*, const double* X, int64_t rows, const int32_t* tidx, int64_t N, int d, float fcanary, double* xout, double* xn_out);
int sd_test_cluster_means(sd_ctx*, const double* X, int64_t rows, int d, const int32_t* order, const int32_t* off, int nl, float fcanary, double* cen_out);
int sd_test_assign(sd_ctx*, const double* E, int64_t M, int d, const double* cen, int K, float fcanary, int32_t icanary, int32_t* hard_out, int32_t* err_out,
                   double* soft_out, double* best_out);
int sd_test_constrained_argmax(sd_ctx*, const double* soft, int64_t chunks, int K, double fill, int32_t icanary, int32_t* hard_out);
int sd_test_activations(sd_ctx*, const float* seg, const int32_t* hard, int64_t chunks, int K, float fcanary, double* act_out, int64_t act_cap, int64_t* nact_out);
int sd_test_topk(sd_ctx*, const double* act, int64_t act_rows, const int32_t* count, int64_t n_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow,
                 int K, uint8_t* binary_out);
int sd_test_assign_cuts(sd_ctx*, const double* E, int64_t M, int d, const double* cen, const int32_t* coff, const int32_t* slot, int Tn, int n_slots,
                        const int32_t* nact, float fcanary, int32_t icanary, double* m2_out, int32_t* hard_out, double* best_out, int32_t* err_out);
int sd_test_recon_cuts(sd_ctx*, const float* seg, const int32_t* hard, int64_t chunks, const int32_t* koff, int Tg, const double* act_in, const int32_t* count,
                       int64_t n_count, int64_t ar0, int64_t cr0, int64_t rows, int64_t crow, float fcanary, double* act_out, int64_t act_cap,
                       uint8_t* binary_out, int64_t* nact_out);
int sd_test_pcm_to_f32(sd_ctx*, const int16_t* pcm, int64_t n, float fcanary, float* wav_out);
int sd_test_f32_to_f64(sd_ctx*, const float* a, int64_t n, float fcanary, double* b_out);
int sd_test_mark_inactive(sd_ctx*, const int32_t* hard, const int32_t* nact, int64_t n, int32_t icanary, int32_t* hard_out);

/* ---- test hooks (tests/test_input_kernels.py): the kernels IN FRONT of the two networks -- the resampler (csrc/resample.hip), the copy kernels of the streams
 * (csrc/stream.hip), the pack and gap-mask kernels (csrc/many.hip) and the fp16 weight forms (csrc/weights_gpu.hip) -- through the function the product calls
 * for the launch, under the contract of the hooks above: host pointers; every floating-point input is followed (for the resampler also preceded) by 256 NaN,
 * 16-bit samples by 256 times 0x7fff; every output is preset to a canary, has 256 slack units behind it and comes back WHOLE; a case whose defined reads or
 * writes leave its operands, or two of whose rows write the same place, is SD_ERR_ARG before any launch.
 *
 * sd_test_resample: k_resample through resample_dev.  x [n] at in_sr; n_out = -1 means sd_resample_len(n, in_sr, out_sr), else 0 .. that length ->
 *   y_out [n_out + 256].  taps_out (optional): the tap table the context built and cached for the pair, [2J + 1][L], read back from the device; taps_cap
 *   must be its size.
 * sd_test_resample_jobs: ONE k_resample_jobs launch through resample_jobs for R rows to 16 kHz.  Row r holds inputs [first, first + held) of its
 *   recording, given as x[x_off, x_off + held) of the shared host array x [x_len] and uploaded with 256 NaN on either side; inputs from n_limit
 *   (<= first + held) on read as zero; outputs [m_first, m_first + count), count >= 1, and `pad` zeros go to arena[dst_off ...] of ONE destination arena
 *   -> arena_out [arena + 256].  Tap tables come from resample_taps.  Refused: a row with first > 0 whose first summed input floor(m_first M / L) - J lies
 *   in front of `first` (outside the kernel's contract).  When resample_jobs itself refuses the table (SD_ERR_ARG), the arena is downloaded all the same.
 * sd_test_group_copy: which 0 = k_group_append (is_f32 = 0: src is int16), 1 = k_group_scatter, 2 = k_group_tail_move, all through group_launch; 3 =
 *   k_tail_move, one row, through the function the single stream's seal calls.  is_f32 is read for which = 0 only.  src [src_len] floats or int16,
 *   rows [R][4] = (src_off, dst_off, len, room) in elements, ONE destination arena -> dst_out [dst_len + 256].  Refused: src_off + len > src_len,
 *   dst_off + room > dst_len, rows whose [dst_off, dst_off + room) overlap; for which = 3 src_off % 4 != 0, dst_off != 0 (the kernel's stated alignment) or
 *   room < len + 512 (it has no room clamp).
 * sd_test_many_pack: k_many_pack.  rows [R][4] = (src_off or -1 for a null source, n, base, len); a null source must have nothing to read
 *   -> dst_out [dst_len + 256].
 * sd_test_many_gap_masks: k_many_gap_masks.  gaps [G][2] = (first, count) -> masks_out [(total_chunks + 256) * 3][293].
 * sd_test_weight_forms: form 0 = build_conv_w16 (k_w16_planes), 1 = build_conv_w16x (k_w_absmax, k_w16x) on a scratch layer of w [K][Cout][CinPad], CinPad a
 *   multiple of 32, channels >= cin ignored.  halves_out: the fp16 bit patterns -- form 0: [2][K][Cout][roundup64(cin)], form 1: 2 * K * Cout * CinPad in the
 *   layout of sd_test_pack_split_weights -- and 256 times `canary` behind them; halves_cap must be that size.  *inv_scale: 2^-e of form 1, 0 for form 0. */
typedef struct sd_resample_case_row {
    int32_t in_sr, pad;
    int64_t first, held, n_limit, m_first, count, x_off, dst_off;
} sd_resample_case_row;
int sd_test_resample(sd_ctx*, const float* x, int64_t n, int32_t in_sr, int32_t out_sr, int64_t n_out, float canary, float* y_out, float* taps_out,
                     int64_t taps_cap);
int sd_test_resample_jobs(sd_ctx*, const sd_resample_case_row* rows, int64_t R, const float* x, int64_t x_len, int64_t arena, float canary, float* arena_out);
int sd_test_group_copy(sd_ctx*, int which, int is_f32, const void* src, int64_t src_len, const int64_t* rows, int64_t R, int64_t dst_len, float canary,
                       float* dst_out);
int sd_test_many_pack(sd_ctx*, int is_f32, const void* src, int64_t src_len, const int64_t* rows, int64_t R, int64_t dst_len, float canary, float* dst_out);
int sd_test_many_gap_masks(sd_ctx*, const int64_t* gaps, int64_t G, int64_t total_chunks, float canary, float* masks_out);
int sd_test_weight_forms(sd_ctx*, const float* w, int K, int Cout, int CinPad, int cin, int form, uint16_t canary, uint16_t* halves_out, int64_t halves_cap,
                         float* inv_scale);

#ifdef __cplusplus
}
#endif
#endif
