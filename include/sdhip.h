/*
 * sdhip.h -- C ABI of libsdhip.so, the MI355X (gfx950) implementation of the
 * speaker-diarization hot path of leohuang2013/pyannote-audio_speaker-diarization_cpp.
 *
 * Every entry point names the reference interface it replaces ("sd.cpp" =
 * pipeline/src/speakerDiarizer.cpp, "cl.h/.cpp" = pipeline/src/clustering/).
 * Plain pointers and sizes only; no C++/torch types; no exceptions cross the
 * boundary.  All functions return SD_OK (0) or an SD_ERR_* code; the message is
 * available from sd_last_error().  A context is bound to one GPU and is not
 * thread-safe (same as the reference's static Ort::Env, onnx_model.cc:21-24).
 *
 * Pointer naming: h_* = host memory, d_* = device (HBM) memory of the ctx's GPU.
 */
#ifndef SDHIP_H
#define SDHIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct sd_ctx sd_ctx;

/* one speaker turn; replaces Annotation::Result (sd.cpp:866-876) */
typedef struct sd_turn { double start, end; int32_t label; int32_t _pad; } sd_turn;

enum {
    SD_OK = 0,
    SD_ERR_ARG = 1,      /* bad argument                                          */
    SD_ERR_HIP = 2,      /* HIP runtime failure / no GPU                          */
    SD_ERR_MODEL = 3,    /* weight file missing or malformed (reference: Ort::Exception) */
    SD_ERR_SHORT = 4,    /* audio too short for one segmentation frame (reference: UB, sd.cpp:2997) */
    SD_ERR_NUMERIC = 5,  /* zero-norm centroid (reference throws, sd.cpp:493-495) */
    SD_ERR_COMM = 6,     /* multi-GPU exchange failed or timed out; the communicator has been aborted */
    SD_ERR_NOMEM = 7     /* a host allocation of a roster call failed; the roster is what it was (sd_roster_*) */
};

/* fixed geometry of the reference */
#define SD_SAMPLE_RATE 16000
#define SD_CHUNK 80000      /* 5.0 s, sd.cpp:1335,1411 */
#define SD_HOP 8000         /* 0.5 s, sd.cpp:1336,1412 */
#define SD_FRAMES 293       /* sd.cpp:1415 */
#define SD_SPEAKERS 3       /* sd.cpp:1351 */
#define SD_EMB_DIM 192      /* sd.cpp:2484 */
#define SD_EMB_BATCH 32     /* sd.cpp:2429 */

/* ---- context ------------------------------------------------------------
 * replaces OnnxModel::OnnxModel(path) x2 (onnx_model.cc:41-105) + SegmentModel /
 * EmbeddingModel1 construction (sd.cpp:2958, 3043).  Model files are either the
 * reference's ONNX files (segment2.onnx / emd4.onnx as written by segment/export2.py
 * and embeddings/export3.py; weights are pulled out of the graph, no ONNX runtime)
 * or ".sdw" weight packs (tools/make_weights.py).  Either path may be NULL when only
 * the other network (or only clustering) is used. */
sd_ctx* sd_create(const char* seg_model_path, const char* emb_model_path, int device_id);
void sd_destroy(sd_ctx*);
/* host-only: parse an ONNX model (kind 0 = segmentation, 1 = embedding) and write the .sdw pack */
int sd_convert_onnx(const char* onnx_path, int kind, const char* out_sdw_path);
const char* sd_convert_error(void);
const char* sd_last_error(const sd_ctx*);     /* "" when no error */
const char* sd_create_error(void);            /* reason for the last NULL from sd_create */

/* ---- a2: chunk rule of SegmentModel::slide (sd.cpp:1419, 1457) ---------- */
int64_t sd_num_chunks(int64_t n_samples, int64_t* last_chunk_len);

/* ---- a2+a3: SegmentModel::slide + ::infer (sd.cpp:1352-1504) ------------
 * wav: n float samples already scaled to [-1,1).  out: [chunks][293][3] f32. */
int sd_segment(sd_ctx*, const float* h_wav, int64_t n, float* h_out, int64_t* chunks);
int sd_segment_dev(sd_ctx*, const float* d_wav, int64_t n, float* d_out, int64_t chunks);

/* ---- a3 alone: SegmentModel::infer exactly as the reference declares it (sd.cpp:1352-1404: "input: batch size x samples count,
 * output: batch size x 293 x 3") for a host that keeps the reference's own slide() (sd.cpp:1407-1504) and swaps only the model call.
 * h_chunks [rows][T] separate waveforms (T = 80000 in slide(); a shorter last chunk is what sd.cpp:1457-1480 passes), any number of rows
 * (the reference fills its fixed batch of 32, sd.cpp:1356-1364).  h_out [rows][293][3]; *frames (may be NULL) = the frames the network
 * yields for T samples, 293 for T = 80000; frames beyond it are zero (slide()'s padding, sd.cpp:1473-1479).  Bit-identical to sd_segment
 * on the same samples. */
int sd_segment_chunks(sd_ctx*, const float* h_chunks, int64_t rows, int64_t T, float* h_out, int32_t* frames);

/* ---- a4-a6: binarize_swf, speaker_count, cleanSegmentations + mask choice
 * (sd.cpp:1506-1639, 1665-1738, 710-743, 3047-3078).
 * seg [chunks][293][3] -> binarized u8 [chunks][293][3], masks f32 [chunks*3][293],
 * count i32 [*n_count] (capacity cap_count).  Any output pointer may be NULL. */
int sd_postseg(sd_ctx*, const float* h_seg, int64_t chunks, uint8_t* h_bin,
               float* h_masks, int32_t* h_count, int64_t cap_count, int64_t* n_count);
int64_t sd_count_frames(int64_t chunks);      /* frames speaker_count produces */

/* ---- a6-a9: crop + getEmbedding + EmbeddingModel1::infer (sd.cpp:1641-1662,
 * 2436-2561, 1977-2040, 1889-1970).  Item i = (chunk i/3, local speaker i%3)
 * reads wav[chunk*8000 .. +80000) (zero padded) with mask row i.  Batches of 32
 * consecutive items share max_len exactly as the reference's batches do.
 * out: [items][192] f32, NaN rows for too-short items. */
int sd_embed(sd_ctx*, const float* h_wav, int64_t n, const float* h_masks,
             int64_t items, float* h_emb);
int sd_embed_dev(sd_ctx*, const float* d_wav, int64_t n, const float* d_masks,
                 int64_t items, int64_t first_item, float* d_emb);

/* ---- a8+a9 alone: EmbeddingModel1::infer exactly as the reference declares it (sd.cpp:1977-2040 "input: batch size x waveform, wave
 * lens; output: embedding", with _infer sd.cpp:1889-1970) for a host that keeps the reference's own getEmbedding() (sd.cpp:2436-2561:
 * interpolate, padSequence, wav_lens, NaN rule) and swaps only the model call.  h_signals [B][80000] compacted zero-padded signals,
 * h_wav_lens [B] relative lengths in (0, 1] (sd.cpp:2499-2510), any B (the reference pads its batch to 32 with lens 1.0, sd.cpp:1898-1899).
 * h_emb [B][192]; no NaN rule here -- getEmbedding applies it to what infer returns (sd.cpp:2540-2556).  Rows that sd_embed computes
 * come out bit-identical. */
int sd_embed_signals(sd_ctx*, const float* h_signals, const float* h_wav_lens, int64_t B, float* h_emb);

/* ---- a8 + head of a9 alone (operator seam for parity tests): compaction +
 * STFT + power + mel + dB + mean-norm.  signals-level inputs as for sd_embed;
 * out feats [items][501][80] f32, wav_lens [items] f32 (reference layout). */
int sd_frontend(sd_ctx*, const float* h_wav, int64_t n, const float* h_masks,
                int64_t items, float* h_feats, float* h_wav_lens);
/* ECAPA-TDNN body alone: feats [items][501][80], wav_lens [items] -> [items][192] */
int sd_ecapa(sd_ctx*, const float* h_feats, const float* h_wav_lens, int64_t items, float* h_emb);

/* ---- a12: Clustering::linkage (cl.h:8, cl.cpp:417-440): X[N][d] f64 -> Z[N-1][4] */
int sd_linkage(sd_ctx*, const double* h_X, int64_t N, int d, double* h_Z);
/* ---- a12+a13: Clustering::cluster (cl.h:7, cl.cpp:459-468): 1-based labels */
int sd_cluster(sd_ctx*, const double* h_X, int64_t N, int d, double cutoff, int32_t* h_labels1);
/* ---- a12 / a12+a13 with the linkage method and the metric chosen by the caller: the `method` hyper-parameter of the clustering step
 * (clustering/Clustering.py:251-276 / 317-333) and the metric its two branches use.  Method codes are scipy's; centroid, median or ward
 * with the cosine metric returns SD_ERR_ARG (scipy refuses the combination; Clustering.py:317-321 normalises the rows and goes euclidean
 * instead).  Cosine distance is 1 - dot / (sqrt(m1) * sqrt(m2)) with sequential sums, the reference's own rule (sd.cpp:476-498); a
 * zero-norm row returns SD_ERR_NUMERIC.  Z is the dendrogram of scipy's generic algorithm (scipy.cluster._hierarchy.fast_linkage, the
 * ancestor of cl.cpp:289-406), ties included.  sd_linkage / sd_cluster are the centroid + euclidean case. */
enum {
    SD_LINKAGE_SINGLE = 0, SD_LINKAGE_COMPLETE = 1, SD_LINKAGE_AVERAGE = 2, SD_LINKAGE_CENTROID = 3,
    SD_LINKAGE_MEDIAN = 4, SD_LINKAGE_WARD = 5, SD_LINKAGE_WEIGHTED = 6
};
enum { SD_METRIC_EUCLIDEAN = 0, SD_METRIC_COSINE = 1 };
int sd_linkage_ex(sd_ctx*, const double* h_X, int64_t N, int d, int method, int metric, double* h_Z);     /* Clustering.py:251-276 / 317-333 */
int sd_cluster_ex(sd_ctx*, const double* h_X, int64_t N, int d, int method, int metric, double cutoff, int32_t* h_labels1);     /* Clustering.py:251-276 / 317-333 */
/* ---- a12 for J independent jobs in one call: the batch form of sd_linkage_ex.  h_X holds the rows of all jobs, job after job (N[j] rows of d each),
 * h_Z the dendrograms in the same order, max(N[j] - 1, 0) rows of 4 each.  Z of job j is, byte for byte, what sd_linkage_ex gives for job j alone,
 * whatever else is in the call and in whatever order, for every N: the jobs that sd_linkage_ex runs on one workgroup (N < 1500) share launches,
 * one workgroup per job and, under "linkage_batch_xcd", the jobs of the one-XCD cooperative class, eight to a launch; the others take sd_linkage_ex's
 * own route.  Under "linkage_batch_xcd_zero" a job of that class whose rows hold duplicates (a tie at height 0) stays in those launches too.  N[j] of 0 or 1 is legal: no rows, status SD_OK.  A job with a zero-norm row
 * under the cosine metric gets status[j] = SD_ERR_NUMERIC and its rows of h_Z are left as they were; the others finish and the call returns SD_OK.
 * SD_ERR_ARG before anything is written: a null pointer, J < 1, a negative N[j], d <= 0, more than 2^31 - 1 rows in all, an unknown method or
 * metric, centroid / median / ward with the cosine metric. */
int sd_linkage_many(sd_ctx*, const double* h_X /* rows of all jobs, job after job */, const int64_t* N /*[J]*/, int64_t J, int d, int method, int metric, double* h_Z /* sum(max(N[j]-1,0)) rows of 4 */, int32_t* status /*[J]*/);     /* cl.cpp:289-440; Clustering.py:251-276 / 317-333 */
/* host-only: "single", "complete", "average", "centroid", "median", "ward", "weighted" -> its code, anything else -> -1 (Clustering.py:251-276 / 317-333) */
int sd_linkage_method_from_name(const char* name);
/* ---- a13 alone: Clustering::fcluster (cl.h:9-10, cl.cpp:442-457; criterion "distance", cl.cpp:121-232): Z [N-1][4] of N observations
 * -> 1-based labels [N], numbered as the reference numbers them.  Host arithmetic only: no GPU work, the context may be NULL.  A Z that
 * is not a dendrogram of N observations (the reference indexes with its entries unchecked) returns SD_ERR_ARG. */
int sd_fcluster(sd_ctx*, const double* h_Z, int64_t N, double cutoff, int32_t* h_labels1);
/* ---- a10+a11+a14: Cluster::clustering (sd.cpp:2063-2116): emb [chunks][3][d]
 * f64 with NaN rows -> hard clusters i32 [chunks][3]; *n_clusters = K */
int sd_clustering(sd_ctx*, const double* h_emb, int64_t chunks, int d, int32_t* h_hard, int32_t* n_clusters);
/* same with the num_clusters / min_clusters / max_clusters constraints (-1 = unset) that the reference leaves
 * unimplemented (assert(false), sd.cpp:2368-2369); semantics of clustering/Clustering.py:21-43, 352-399 */
int sd_clustering_ex(sd_ctx*, const double* h_emb, int64_t chunks, int d, int num_clusters, int min_clusters,
                     int max_clusters, int32_t* h_hard, int32_t* n_clusters);

/* ---- a15-a17: inactive mask, reconstruct, to_diarization, to_annotation
 * (sd.cpp:3172-3191, 2789-2848, 2638-2764, 2852-2935).  Returns malloc'd turns
 * sorted by start (Annotation::finalResult, sd.cpp:962-978). */
int sd_reconstruct(sd_ctx*, const float* h_seg, const uint8_t* h_bin, const int32_t* h_hard,
                   const int32_t* h_count, int64_t n_count, int64_t chunks, int64_t n_samples,
                   sd_turn** turns, int64_t* n_turns);

/* ---- whole path: speakerDiarization() (sd.cpp:2937-3234) -----------------
 * pcm: 16-bit mono 16 kHz samples as WavReader yields them (wav.h:107-111);
 * scaling by 1/32768 (sd.cpp:2950) happens on the GPU. */
int sd_diarize(sd_ctx*, const int16_t* h_pcm, int64_t n, sd_turn** turns, int64_t* n_turns);
int sd_diarize_dev(sd_ctx*, const int16_t* d_pcm, int64_t n, sd_turn** turns, int64_t* n_turns);
void sd_free_turns(sd_turn*);

/* ---- the two halves of the multi-GPU path as separate calls (a host that brings its own collective): ranks run infer on
 * their contiguous chunk range (multiple of 32 chunks), exchange d_seg / d_emb, then any rank finalizes. */
/* d_pcm_shard holds samples [first_sample, first_sample + shard_samples) of the n_total-sample
 * recording and must cover [chunk_lo*8000, min(n_total, (chunk_hi-1)*8000 + 80000)). */
int sd_shard_infer_dev(sd_ctx*, const int16_t* d_pcm_shard, int64_t first_sample, int64_t shard_samples,
                       int64_t n_total, int64_t chunk_lo, int64_t chunk_hi,
                       float* d_seg /*[hi-lo][293][3]*/, float* d_emb /*[(hi-lo)*3][192]*/);
int sd_finalize_dev(sd_ctx*, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n,
                    sd_turn** turns, int64_t* n_turns);

/* ---- the same path on several GPUs under the boundary (comm.cpp): one process per GPU, RCCL all-gather of scores and
 * embeddings over xGMI on the library's stream, clustering on rank 0.  Replaces speakerDiarization() (sd.cpp:2937-3234)
 * for long recordings; the reference has no counterpart (single device, onnx_model.cc:21-71).
 * Bootstrap: rank 0 calls sd_comm_unique_id (needs a GPU) and the host program hands the SD_COMM_ID_BYTES bytes to every
 * rank; then every rank calls sd_comm_init with the same id (collective, like ncclCommInitRank).  */
#define SD_COMM_ID_BYTES 128
int sd_comm_unique_id(void* id /*[SD_COMM_ID_BYTES]*/);
int sd_comm_init(sd_ctx*, const void* id, int rank, int world);
int sd_comm_destroy(sd_ctx*);
int sd_comm_info(const sd_ctx*, int* rank, int* world /* 0 = no communicator */);
/* host-only: chunk range [ranges[2r], ranges[2r+1]) of every rank r for an n_total-sample recording -- contiguous, each
 * starting on a multiple of 32 chunks (= 3 reference embedding batches) -- and the slot size (chunks) of the padded
 * all-gather.  rank0_permille = share of the chunks rank 0 infers itself (it also finalizes), -1 = equal shares; the
 * library uses option "rank0_permille" for the same plan.  Rank r needs samples
 * [lo*8000, min(n_total, (hi-1)*8000 + 80000)). */
int sd_shard_plan(int64_t n_total, int world, int rank0_permille, int64_t* ranges /*[world][2]*/, int64_t* slot_chunks);
/* collective: every rank passes the samples of its range (h_/d_pcm_shard[0] is sample first_sample of the recording).
 * Rank 0 receives the turns; the other ranks return *n_turns = 0 once the exchange has completed (rank 0's clustering of this
 * job then overlaps their inference of the next one).  Failure is collective: a rank that fails in its part still joins the
 * exchange with a status record, and EVERY rank returns an error for that job; a rank that never arrives (crash) makes the
 * others return SD_ERR_COMM after "comm_timeout_ms" with the communicator aborted.  After any non-OK return the job group must be
 * torn down (sd_comm_destroy / exit) -- the ranks' job counters no longer agree. */
int sd_diarize_sharded(sd_ctx*, const int16_t* h_pcm_shard, int64_t first_sample, int64_t shard_samples, int64_t n_total,
                       sd_turn** turns, int64_t* n_turns);
int sd_diarize_sharded_dev(sd_ctx*, const int16_t* d_pcm_shard, int64_t first_sample, int64_t shard_samples, int64_t n_total,
                           sd_turn** turns, int64_t* n_turns);

/* ---- a1: wav::WavReader::Open (wav.h:62-126).  Returns malloc'd pcm (free with
 * sd_free_pcm); only 16-bit PCM is accepted (README.md:37), channels are read
 * interleaved-as-mono exactly like the reference (wav.h:95-97). */
int sd_read_wav(const char* path, int16_t** pcm, int64_t* n, int32_t* sample_rate, int32_t* channels);
void sd_free_pcm(int16_t*);
/* every bit depth WavReader reads (8 / 16 / 32, wav.h:99-122), as float samples already divided by 32768
 * (sd.cpp:2948-2951); free with sd_free_wav.  sd_diarize_f32 is sd_diarize for such samples. */
int sd_read_wav_f32(const char* path, float** wav, int64_t* n, int32_t* sample_rate, int32_t* channels, int32_t* bits_per_sample);
void sd_free_wav(float*);
int sd_diarize_f32(sd_ctx*, const float* h_wav, int64_t n, sd_turn** turns, int64_t* n_turns);
/* ---- the resample leg of SURVEY 8(f) row 2: Resampler::Resample (frontend/resampler.cc:19-36 = libsamplerate 0.2.2 src_simple,
 * SRC_SINC_BEST_QUALITY; dormant in the reference, which reads `sample_rate` and ignores it, sd.cpp:2940-2942).  Mono float samples at
 * in_sr -> out_sr on the GPU (k_resample: exact polyphase band-limited sinc interpolation, 64 zero crossings per wing, cutoff 0.95 of
 * the lower Nyquist frequency, Kaiser 100 dB; csrc/resample.hip states what is and is not comparable with libsamplerate).
 * sd_resample_len = the reference's output length, (size_t)(n * ratio) with both factors in float (resampler.cc:21-22).
 * out == NULL: only *n_out is set. */
int64_t sd_resample_len(int64_t n, int32_t in_sr, int32_t out_sr);
int sd_resample(sd_ctx*, const float* wav, int64_t n, int32_t in_sr, int32_t out_sr, float* out, int64_t cap, int64_t* n_out);
/* ---- the head of speakerDiarization() (sd.cpp:2937-2951: WavReader, / 32768) in one call, with the input checks the reference
 * lacks (README.md:37 asks for 16 kHz / mono / 16-bit and nothing validates it).  flags = 0: a file whose sample rate is not 16 000 is
 * REFUSED with SD_ERR_ARG (the reference would process it as if it were 16 kHz); channels are read interleaved as the reference
 * does (wav.h:95-97).  SD_WAV_RESAMPLE: other rates go through sd_resample first.  SD_WAV_DOWNMIX: channels are averaged first.
 * SD_WAV_ASSUME_16K: drop-in parity with the reference on off-rate files -- the rate in the header is ignored as the reference ignores it. */
/* ---- the reference's WRITE_DATA switch (debugWrite / debugWrite2d / debugWrite3d, sd.cpp:62-234 and their call sites): with a directory
 * set, every following whole-path call (sd_diarize*, sd_finalize_dev) writes DIR/cpp_<item>.txt for the items of
 * pipeline/script/verifyEveryStepResult.py:6-17 in the reference's text format -- DIR = "/tmp" is what that script reads.  level 1: all
 * items but the two 15 - 25 MB-per-batch ones; level 2: + imasks<n>, batch_waveform<n>; level 0 / dir NULL: off.  csrc/stepdump.cpp says
 * which files are GPU tensors written as they are and which are views derived from them. */
int sd_set_dump_dir(sd_ctx*, const char* dir, int level);
#define SD_WAV_RESAMPLE 1
#define SD_WAV_DOWNMIX 2
#define SD_WAV_ASSUME_16K 4   /* the reference's behaviour on a file whose rate is not 16 000: process the samples as if it were (sd.cpp:2940-2942) */
int sd_diarize_wav(sd_ctx*, const char* path, int flags, sd_turn** turns, int64_t* n_turns);
/* ---- output formats (the reference prints raw cluster ids to stdout only, sd.cpp:3433-3441) */
/* RTTM file of the turns ("SPEAKER <uri> 1 <start> <dur> <NA> <NA> SPEAKER_kk <NA> <conf|NA>") */
int sd_write_rttm(const char* path, const char* uri, const sd_turn* turns, int64_t n_turns);
int sd_write_rttm_ex(const char* path, const char* uri, const sd_turn* turns, int64_t n_turns, const double* conf /* or NULL */);
/* renumber the labels in place: mode 1 (sd_relabel_turns) = pyannote.audio's SPEAKER_00.. convention (the labels that occur,
 * sorted by their decimal string, pyannote.core Annotation.labels()); mode 0 = order of first appearance */
int sd_relabel_turns(sd_turn* turns, int64_t n_turns);
int sd_relabel_turns_ex(sd_turn* turns, int64_t n_turns, int mode);
/* per-turn confidence of the turns the last sd_diarize* / sd_finalize_dev of this ctx returned (same order): mean soft score
 * (2 - cosine distance to the cluster centroid, soft_clusters of sd.cpp:2191-2207; range 0..2) of the (chunk, local speaker)
 * items assigned to the turn's cluster whose chunk overlaps the turn; NaN when no such item has an embedding */
int sd_last_confidence(const sd_ctx*, double* conf, int64_t cap, int64_t* n);

/* ---- speech / overlapped-speech regions from the segmentation stage alone: what pyannote's VoiceActivityDetection and
 * OverlappedSpeechDetection pipelines compute, with the reference's own two building blocks -- PipelineHelper::aggregate (sd.cpp:1167-1311,
 * skip_average = false, missing = 0.0) over the per-chunk largest (SD_ACTIVITY_SPEECH) or second largest (SD_ACTIVITY_OVERLAP) of the three
 * scores, then to_annotation (sd.cpp:2852-2935) on that one-column timeline with window start 0.0.  A chunk frame with a NaN score is masked
 * out.  Results are bit-identical to those two functions, Track::support (collar = min_duration_off, when > 0) and Track::removeShort
 * (min_duration_on, when > 0; it never removes the first region, sd.cpp:943-953) included.  Options, through sd_set_option_f64:
 * "activity_onset", "activity_offset" (defaults 0.5, in [0, 1]; comparisons are strict, offset > onset is legal: a score strictly between
 * the two toggles the state), "activity_min_duration_on", "activity_min_duration_off" (defaults 0.0, >= 0); through sd_set_option:
 * "activity_hamming" (1 = every contribution and every count weighted by np.hamming(293): the branch sd.cpp:1211-1215 names and leaves
 * unimplemented; default 0).  Nothing of the embedding, clustering or reconstruction stages runs. */
enum { SD_ACTIVITY_SPEECH = 0, SD_ACTIVITY_OVERLAP = 1 };
/* the stage alone, sd.cpp:1167-1311: seg [chunks][293][3] f32 -> the aggregated timeline, all *n_frames frames of it (f64); h_scores == NULL: only the count */
int sd_activity_scores(sd_ctx*, const float* h_seg, int64_t chunks, int kind, double* h_scores, int64_t cap, int64_t* n_frames);
/* the stage alone, sd.cpp:2852-2935: a timeline -> malloc'd regions (sd_free_turns) by the context's four options; label 0 */
int sd_activity_regions(sd_ctx*, const double* h_scores, int64_t n_frames, sd_turn** turns, int64_t* n_turns);
/* whole path, sd.cpp:1167-1311 / 2852-2935 behind the head of speakerDiarization(): samples as for sd_diarize / _dev / _f32 / _wav (same SD_WAV_* flags,
 * same refusals, SD_ERR_SHORT where they return it) -> regions with label = kind.  The timeline keeps the frames up to the one closest to the end of
 * the audio: those that lie wholly in the zero padding of the last chunk are dropped. */
int sd_activity(sd_ctx*, const int16_t* h_pcm, int64_t n, int kind, sd_turn** turns, int64_t* n_turns);
int sd_activity_dev(sd_ctx*, const int16_t* d_pcm, int64_t n, int kind, sd_turn** turns, int64_t* n_turns);
int sd_activity_f32(sd_ctx*, const float* h_wav, int64_t n, int kind, sd_turn** turns, int64_t* n_turns);
int sd_activity_wav(sd_ctx*, const char* path, int flags, int kind, sd_turn** turns, int64_t* n_turns);
/* the timeline (sd.cpp:1167-1311, cropped as above) of the last whole-path sd_activity* call of this ctx */
int sd_last_activity_scores(const sd_ctx*, double* scores, int64_t cap, int64_t* n);

/* ---- a recording that is still growing: replaces calling speakerDiarization() (sd.cpp:2937-3234) again on everything heard so far.  After any
 * sequence of pushes sd_stream_turns returns what sd_diarize returns on the concatenation of what was pushed -- turns, order, labels and confidences,
 * bit for bit -- without running either network twice on a chunk that is complete.  With n samples pushed, chunk k is FULL when k * 8000 + 80000 < n
 * (the chunk that ends exactly at n goes through the reference's "last chunk" branch, sd.cpp:1457) and the first 32 * (full / 32) chunks are SEALED:
 * 96 items = three whole reference embedding batches (sd.cpp:2429), so their scores and embeddings can never change again, whatever is pushed later.
 * A push appends the samples to the stream's f32 tail on the device, runs both networks on the blocks that have just become sealed, into the
 * stream's own cache, and drops the audio in front of sample sealed * 8000; it computes no turns.  Any size is legal, 16-bit and float pushes may be
 * mixed.  sd_stream_turns infers the pending chunks [sealed, total) behind the sealed rows and finalizes all of them under the context's current
 * clustering options; it keeps the pending rows, so a second call with nothing pushed in between runs no inference.  sd_last_confidence and
 * sd_stage_ms describe it ([0], [1] = the pending inference, [2] = the finalize, [3] = the call; after a push [0], [1], [3] = the sealing);
 * SD_ERR_SHORT where sd_diarize returns it; SD_ERR_ARG while a dump directory is set (the step files describe one whole-path inference).
 * A stream owns its device memory and uses the context's workspaces only inside a call: other entry points and other streams of the context may be
 * called between its calls; sd_destroy closes the streams still open.  "ecapa_precision" and "seg_precision" are fixed when the stream is opened: a
 * push or turns call under other values returns SD_ERR_ARG.  An argument error leaves the stream as it was; after SD_ERR_HIP every further
 * call returns SD_ERR_ARG until the stream is closed.  One GPU: the sharded path has no streams. */
typedef struct sd_stream sd_stream;
int sd_stream_open(sd_ctx*, sd_stream** s);                                    /* sd.cpp:2937-3234, repeated */
int sd_stream_push(sd_stream*, const int16_t* h_pcm, int64_t n);               /* samples as for sd_diarize (wav.h:107-111, sd.cpp:2950) */
int sd_stream_push_dev(sd_stream*, const int16_t* d_pcm, int64_t n);
int sd_stream_push_f32(sd_stream*, const float* h_wav, int64_t n);             /* samples as for sd_diarize_f32 */
int sd_stream_turns(sd_stream*, sd_turn** turns, int64_t* n_turns);            /* == sd_diarize of everything pushed so far; free with sd_free_turns */
int sd_stream_info(const sd_stream*, int64_t* n_samples, int64_t* chunks_sealed, int64_t* chunks_total);      /* any pointer may be NULL */
/* cached rows of chunks [chunk_lo, chunk_hi) inside [0, total): h_seg [hi-lo][293][3] and / or h_emb [(hi-lo)*3][192] (either may be NULL).  Pending
 * rows are those the last sd_stream_turns computed; SD_ERR_ARG when samples were pushed since, or when the range leaves [0, total) */
int sd_stream_read(sd_stream*, int64_t chunk_lo, int64_t chunk_hi, float* h_seg, float* h_emb);
void sd_stream_close(sd_stream*);
/* host-only: the sealed chunks of an n_samples-sample recording, 32 * (full / 32) as above (slide()'s chunk rule, sd.cpp:1419, 1457) */
int64_t sd_stream_sealed_chunks(int64_t n_samples);
/* ---- a stream that runs all day: a sliding window.  After sd_stream_forget the stream is a new stream to which the kept samples were pushed, except
 * that it remembers how many samples it has forgotten.  sd_stream_forget drops D = sealed - 32 * keep_blocks chunks (nothing where D <= 0): the front
 * D rows of the score and the embedding cache go -- the kept sealed rows are copied into fresh, smaller allocations and the old ones are given back,
 * so device memory really shrinks --, n_samples drops by D * 8000, sealed by D, and the origin rises by D * 8000.  The tail already starts at
 * sample sealed * 8000 and is not touched.  D is a multiple of 32 chunks = 256 000 samples, so block boundaries and the 96-item embedding batches
 * stay where a new stream puts them, and a cached sealed row depends on its own chunk and on the kernel alone: sd_stream_turns, _read, _info and
 * every sd_last_* result are, bit for bit, those of sd_diarize of samples [origin, origin + n_samples) of what was pushed, with times counted from
 * the origin.  The pending rows are inferred again by the next sd_stream_turns, as after a push (which kernel a pending chunk's scores take depends
 * on the chunks in front of it in its batch).  A failed allocation inside a forget -- by hand, or by the window behind a push -- returns SD_ERR_HIP,
 * leaves the stream exactly what it was before that forget and leaves it usable; behind a push the samples are in and the blocks sealed
 * (sd_stream_info says so: do not push them again), in a group call the streams later in the list keep their blocks until their next push that seals.
 * Every other SD_ERR_HIP, a failed copy inside a forget included, makes the stream unusable as for the other calls.
 * sd_stream_set_window(W >= 0) is the policy: every push, single or through sd_stream_push_many*, that seals a block then forgets down to W blocks
 * (in a group call per stream, after the group's launches); -1 = off, the default.  sd_stream_origin: the samples forgotten so far.
 * SD_ERR_ARG: keep_blocks < 0 (set_window: < -1), a stream that is unusable or whose precision options changed, as for the other calls.
 * The window itself carries no speakers over: every update clusters anew, as for streams in general, and a raw label means the same person from one
 * update to the next only under an enrolled gallery -- or with a roster attached (sd_stream_set_roster, below), which renames the labels of every
 * update to ids that last, also for a talker who left the window and comes back. */
int sd_stream_forget(sd_stream*, int64_t keep_blocks);                         /* sd.cpp:2937-3234, repeated */
int sd_stream_set_window(sd_stream*, int64_t keep_blocks /* -1 = off, the default */);
int sd_stream_origin(const sd_stream*, int64_t* first_sample);
/* ---- many live recordings at once: S streams of ONE context in one call, for a caller with dozens of calls in progress on one card.  Every stream
 * keeps its contract: after any sequence of single and group calls its turns, labels, confidences, centroids and cached rows are the bytes it gives
 * when it is driven alone, which are those of sd_diarize of everything pushed to it.  The networks run once per call over a pack of the streams'
 * ranges -- a block that became sealed, or the pending chunks [sealed, total) -- laid out by sd_many_plan's rule (a range of c chunks gets a slot of
 * roundup32(c + 9) chunks), so the ranges share the segmentation batches and the embedding batches.
 * sd_stream_push_many*: n[i] samples for stream s[i], as for sd_stream_push / _dev / _f32; n[i] == 0 with any pointer is legal and gives that stream
 * nothing.  One upload, one conversion launch and one synchronisation for all of them; every block that became sealed in any stream (two or more
 * in one stream included) is inferred in one packed inference, and sd_stream_info of every stream says what it says after the single push.
 * sd_stream_turns_many: the pending range of every stream with samples pushed since its last turns is inferred in one packed inference, then
 * every stream is finalized in the order of the list under the context's current options, an enrolled gallery included.  status[i] = SD_OK,
 * SD_ERR_SHORT (no chunk yet; turns[i] = NULL) or SD_ERR_NUMERIC from that stream's clustering (turns[i] = NULL); the other streams go on and the
 * call returns SD_OK.  Any other failure ends the call and nothing stays allocated to the caller.  Afterwards sd_many_select(ctx, i) makes stream i
 * the job that sd_last_confidence, sd_last_speakers and sd_last_enrolled describe.
 * Refused with SD_ERR_ARG before anything is touched: a null array, S < 1, a null stream, a null sample pointer with n[i] > 0, a negative n[i], the
 * same stream twice, streams of different contexts, a stream that is unusable after SD_ERR_HIP, a stream opened under another precision than the
 * context has now, a planted workload (its chunk range means one recording), a pack of more than SD_MANY_MAX_CHUNKS chunks, and for
 * sd_stream_turns_many a dump directory and the refusals of an enrolled gallery.  SD_ERR_HIP in the middle of a call makes every stream of the
 * call unusable.  sd_stage_ms: as for sd_stream_push and sd_stream_turns, [2] = the sum of the finalizes. */
int sd_stream_push_many(sd_stream* const* s /*[S]*/, const int16_t* const* h_pcm /*[S]*/, const int64_t* n /*[S]*/, int64_t S);     /* sd.cpp:2937-3234, 2950 */
int sd_stream_push_many_dev(sd_stream* const* s /*[S]*/, const int16_t* const* d_pcm /*[S]*/, const int64_t* n /*[S]*/, int64_t S);     /* sd.cpp:2937-3234, 2950 */
int sd_stream_push_many_f32(sd_stream* const* s /*[S]*/, const float* const* h_wav /*[S]*/, const int64_t* n /*[S]*/, int64_t S);     /* sd.cpp:2937-3234, 2948-2951 */
int sd_stream_turns_many(sd_stream* const* s /*[S]*/, int64_t S, sd_turn** turns /*[S]*/, int64_t* n_turns /*[S]*/, int32_t* status /*[S]*/);     /* sd.cpp:2937-3234 */
/* ---- streams at any sample rate: call-centre audio arrives at 8 kHz, and sd_resample treats what it is given as a whole recording, with silence in
 * front of it and behind it, so it cannot be called piece by piece.  After sd_stream_set_input_rate(s, in_sr) every push -- sd_stream_push / _dev / _f32
 * and the stream's row of sd_stream_push_many* -- hands over samples at in_sr, and the stream resamples them itself (k_resample_jobs, csrc/resample.hip:
 * the arithmetic of sd_resample on a window of the inputs).  L / M = 16000 / in_sr reduced, J the taps per wing of that pair (about 67 * max(1, M / L)),
 * len(n) = sd_resample_len(n, in_sr, 16000).  Output m reads the inputs floor(m M / L) - J .. floor(m M / L) + J.  With n inputs pushed, output m is FINAL
 * when no later input can change it and it belongs to the output of every longer input:
 *     F(n) = min(len(n), #{m >= 0 : floor(m M / L) + J <= n - 1}) = min(len(n), n - 1 - J < 0 ? 0 : ((n - J) L - 1) / M + 1)      (integer division)
 * -- by the kernel's reads, not by which taps happen to be zero.  len and F are non-decreasing: an emitted output is never taken back.
 * sd_resample_final_len (host-only) computes F; -1 on bad arguments as sd_resample_len.
 * The contract: with y_n = sd_resample(all n inputs so far, in_sr, 16000), after any sequence of pushes the stream is, bit for bit, a plain stream to
 * which y_n[0 .. F(n)) was pushed with sd_stream_push_f32: sd_stream_info (which keeps counting 16 kHz samples), sd_stream_turns (turns, order, labels),
 * sd_last_confidence, sd_last_speakers, sd_stream_read, sealing, window / forget and roster.  The stream lags the audio by the filter wing, len(n) - F(n)
 * samples (at most 136 = 8.5 ms at 8 kHz, about 100 at the usual other rates): there are no provisional samples and the tail is never rewound.
 * sd_stream_end_input closes the input: it emits y_n[F(n) .. len(n)) with silence behind the last input exactly as sd_resample has it, and from then on
 * the stream is the plain stream to which all of sd_resample(x) was pushed -- sd_stream_turns is sd_diarize_f32(sd_resample(x)), what sd_diarize_wav
 * with SD_WAV_RESAMPLE gives for the file.  Afterwards a push returns SD_ERR_ARG (in a group call: a row with n[i] > 0), a second sd_stream_end_input is
 * SD_OK and does nothing, and sd_stream_turns, _read, _forget and the roster keep working.
 * sd_stream_set_input_rate is legal only before the first sample is pushed; SD_ERR_ARG otherwise, for in_sr <= 0 and for a rate pair sd_resample
 * refuses (tap table or a tile's input span too large; the stream's kernel keeps 1 KiB of the 160 KiB for its stores, so a span within 1 KiB of
 * sd_resample's limit -- 40 705 .. 40 960 inputs per tile, rates near 1.7 MHz -- is refused here and not there).  16000 means no resampler: every push
 * takes exactly the path of a stream without a rate, and sd_stream_end_input only closes the input -- SD_OK, pushes refused afterwards, closed = 1 -- so
 * that a host which sets the rate from a variable ends every call the same way.
 * A group call may hold streams with and without a rate and of different rates: still one upload, one conversion launch and one synchronisation, and
 * at most ONE resampling launch whatever S and the rates.  An argument error leaves the stream, the inputs it holds included, as it was; so does a
 * failed allocation of a single push before anything was launched (SD_ERR_HIP, the stream stays usable); any other SD_ERR_HIP makes the stream (in a
 * group call: the streams of the call) unusable; a group call keeps the group's rule for a failed allocation too.  sd_stream_end_input on a stream on
 * which no rate was ever set: SD_ERR_ARG.  Device memory per rated stream: the inputs since the buffer last turned over, in two buffers of up to
 * 2 x (largest piece + 2 J + 512) floats each -- 1.3 MB for 10 s pieces at 8 kHz.
 * sd_stream_input_info: the rate, the inputs pushed, the outputs final so far (F(n); len(n) once closed) and whether the input is closed; any pointer
 * may be NULL; a stream without a rate reports 16000, n, n, 0 with n the samples pushed. */
int sd_stream_set_input_rate(sd_stream*, int32_t in_sr);     /* frontend/resampler.cc:19-36 */
int sd_stream_end_input(sd_stream*);     /* frontend/resampler.cc:19-36 (src_simple: end_of_input = 1) */
int sd_stream_input_info(const sd_stream*, int32_t* in_sr, int64_t* n_in, int64_t* n_final, int32_t* closed);     /* frontend/resampler.cc:19-36 */
int64_t sd_resample_final_len(int64_t n, int32_t in_sr, int32_t out_sr);     /* frontend/resampler.cc:19-36, 21-22 */

/* ---- a speaker roster: labels that keep their meaning.  The label of a turn is a raw cluster number (sd.cpp:3433-3441) and every update of a stream
 * clusters anew, so "Speaker_1" of one update may be "Speaker_0" of the next.  A roster is a small host object that hands out persistent speaker ids.
 * Attached to a stream (sd_stream_set_roster) it makes the labels of sd_stream_turns / sd_stream_turns_many roster ids; applied to the last job of a
 * context (sd_roster_update_last) it links the speakers of separate recordings, the recordings of a sd_diarize_many pack for instance.  It only renames
 * labels: times, order, confidences and centroids are the bytes they are without it, and nothing is launched on the device that was not launched before
 * -- one update is K x P cosine distances of d doubles and a table over the job's rows, on the host.
 * State: P entries; entry p holds a centroid c_p [d] (f64), a row count n_p and u_p, the index of the last update that gave p out (-1 for a loaded entry
 * that never was); an update counter U.
 * Input of one update: K label columns with centroids C [K][d] and train-row counts m [K] -- what sd_last_speakers returns; a row whose first element is
 * NaN counts 0 --; optionally the job's hard labels rows [M] (the cluster of every (chunk, local speaker) row behind the inactive rule, < 0 = none) and the
 * ids prev [Mp] that the previous update of the same stream gave the rows of its table (< 0 = none), with shift >= 0: row i of this job is row i + shift of
 * the previous one (3 x the chunks forgotten in between); a threshold t.  Every k in [0, K) gets an id and two k never get the same one:
 *  A rows: cnt[k][p] = the number of i with i + shift < Mp, rows[i] = k >= 0 and prev[i + shift] = p >= 0.  The pairs with cnt > 0 are sorted by
 *    (-cnt, k, p); a pair is taken when both sides are still free.  Skipped when rows or prev is absent.  This is the hysteresis: a speaker keeps the id
 *    his rows had, whatever the clustering renumbered.
 *  B centroids: the k that are still free and whose centroid is not NaN against the entries p that this update has not given out and whose centroid is
 *    not NaN, by the cosine distance of sd_speaker_distances (three sequential f64 sums, sd.cpp:476-498); the pairs with distance <= t (inclusive) are
 *    sorted by (distance, k, p) and taken greedily: the rule of sd_match_speakers.  This brings back a speaker who was away from the window and names
 *    speakers across recordings.  A zero-norm centroid on either side of this step (it reads all of both sides, or nothing when one side is empty):
 *    SD_ERR_NUMERIC.
 *  C the k that are still free get the new ids P, P + 1, ... in ascending k.
 *  D refresh, for every k -> p: when p is new or m[k] >= n_p, c_p = C[k] and n_p = m[k] -- an entry keeps the estimate made from the most rows, a tie goes
 *    to the later one --; u_p = U.  Then U += 1.
 * Any error -- SD_ERR_ARG (a null pointer, a negative size, count or shift, rows[i] >= K, prev[i] >= P, a threshold outside [0, 2]), SD_ERR_NUMERIC,
 * SD_ERR_NOMEM -- leaves the roster exactly as it was.  What a roster does not do: it never merges or expires entries, so a person whom an early update
 * split into two ids stays two ids.
 * sd_roster_open: host only, no context and no GPU, as sd_fcluster.  sd_roster_close: SD_ERR_ARG while a stream is attached; NULL is a no-op.
 * sd_roster_load: entries 0 .. P - 1 into an EMPTY roster (SD_ERR_ARG otherwise), yesterday's roster or the rows of a voiceprint file for instance.
 * sd_roster_speakers: at most cap entries; any of the three arrays may be NULL.  sd_roster_update: the rule; h_rows and h_prev may be NULL; a NaN
 * threshold means the constant t * t / 2 of sd_match_speakers.  sd_roster_update_last: steps B - D on the last job of this context that clustered
 * (SD_ERR_ARG when there is none or when its rows do not have the roster's d), with the context's "speaker_match_threshold"; at most cap ids are written;
 * after sd_many_select(r) it names recording r of a pack.  sd_last_roster_ids: the id of every raw label k of the last job -- they name the rows of
 * sd_last_speakers --, *K = 0 when no roster took part in it.  sd_relabel_turns_map: label k becomes ids[k]; a label outside [0, K) returns SD_ERR_ARG and
 * nothing is written.
 * sd_stream_set_roster (NULL detaches; the roster's d must be 192): from then on sd_stream_turns, and sd_stream_turns_many for this stream, run one update
 * behind their successful finalize -- rows = that finalize's hard labels, prev = the ids the stream kept from its previous update, shift from the two
 * origins (sd_stream_forget needs no call of its own), t = the context's option -- and relabel the turns in place; sd_last_roster_ids, also behind
 * sd_many_select(i), gives the map.  A second call with nothing pushed gives the same ids.  A call that fails anywhere leaves the roster and what the stream
 * kept as they were; in a group call a failing update ends the call as SD_ERR_HIP does, and the rosters are put back.  Several streams of one context may
 * share a roster; detaching, or attaching another roster, drops what the stream kept.  An enrolled gallery and "max_num_embeddings" need no special case:
 * the roster names whatever label columns and table rows the job has. */
typedef struct sd_roster sd_roster;
int sd_roster_open(int d, sd_roster** r);     /* no counterpart: the reference keeps no speaker between calls (sd.cpp:3433-3441) */
int sd_roster_close(sd_roster*);     /* no counterpart (sd.cpp:3433-3441) */
int sd_roster_load(sd_roster*, const double* h_cen /*[P][d]*/, const int64_t* h_counts /*[P]*/, int64_t P);     /* no counterpart (sd.cpp:3433-3441) */
int sd_roster_info(const sd_roster*, int64_t* P, int64_t* updates, int* d);     /* any pointer may be NULL; no counterpart (sd.cpp:3433-3441) */
int sd_roster_speakers(const sd_roster*, double* h_cen /*[cap][d]*/, int64_t* h_counts /*[cap]*/, int64_t* h_seen /*[cap]*/, int64_t cap, int64_t* P);     /* no counterpart (sd.cpp:3433-3441) */
int sd_roster_update(sd_roster*, const double* h_cen /*[K][d]*/, const int64_t* h_counts /*[K]*/, int64_t K, const int32_t* h_rows /*[M] or NULL*/, int64_t M, const int32_t* h_prev /*[Mp] or NULL*/, int64_t Mp, int64_t shift, double threshold, int32_t* h_ids /*[K]*/);     /* sd.cpp:476-498, 3433-3441 */
int sd_roster_update_last(sd_roster*, sd_ctx*, int32_t* h_ids /*[cap]*/, int64_t cap, int64_t* K);     /* sd.cpp:476-498, 3433-3441 */
int sd_relabel_turns_map(sd_turn*, int64_t n_turns, const int32_t* ids /*[K]*/, int64_t K);     /* sd.cpp:3433-3441 */
int sd_stream_set_roster(sd_stream*, sd_roster*);     /* sd.cpp:476-498, 3433-3441 */
int sd_last_roster_ids(const sd_ctx*, int32_t* h_ids /*[cap]*/, int64_t cap, int64_t* K);     /* sd.cpp:3433-3441 */

/* ---- known speakers: cluster numbers mean nothing outside one call; these entries give the clusters an identity that lasts.  The centroids that
 * assign_embeddings builds (sd.cpp:2149-2167; what pyannote hands out with return_embeddings=True, Clustering.py:97-164) come out of the last job, a
 * voiceprint of a known person is computed from regions of a recording exactly as the diarizer computes its own embeddings, and centroids are matched
 * against a gallery of voiceprints by the reference's cosine distance (sd.cpp:476-498).
 * sd_last_speakers: the K final centroids of the last call of this ctx that clustered -- sd_clustering*, sd_diarize*, sd_finalize_dev, sd_stream_turns,
 * sd_diarize_sharded* on rank 0 -- and the number of train rows (sd.cpp:2224) of each: means of the un-normalised train rows, members in ascending row
 * order, sequential f64 sums.  Row k is the cluster whose turns carry raw label k (before any sd_relabel_turns).  Rows have the d of that call: 192 on every
 * whole path.  At most cap rows are written; either pointer may be NULL; *K = 0 before any clustering call.  Where the reference computes no centroid
 * (fewer than two train rows, or max_clusters < 2; sd.cpp:2081-2088) K = 1: the single train row or the mean of the train rows, with its count -- a NaN row
 * with count 0 when there is no train row at all, so "row index = label" always holds. */
int sd_last_speakers(const sd_ctx*, double* h_centroids /*[cap][192] or NULL*/, int64_t cap, int64_t* K, int64_t* h_counts /*[cap] or NULL*/);     /* sd.cpp:2149-2167 */
/* sd_voiceprint*: the embedding of the samples that lie in `spans` -- those with spans[i].label == label, all of them when label < 0; spans == NULL, or no
 * span at all with label < 0: the whole recording.  A span covers samples [llrint(start * 16000), llrint(end * 16000)) clamped to [0, n); overlapping spans
 * are merged.  Same chunks as the diarizer (sd_num_chunks), same item grid, same batches of 32 (sd.cpp:2429): item 3c carries the mask "mask frame f of
 * chunk c is 1.0 iff its first sample c * 8000 + ceil(80000 f / 293) lies in a span and before n", items 3c + 1 and 3c + 2 are empty.  h_emb = the f64 mean
 * of the rows 3c that are not NaN (a window with fewer than 640 selected samples is, sd.cpp:44), ascending c, sequential sums; *n_windows = their number.
 * One label per call: a voiceprint never depends on what else is in the list.  No window at all: SD_ERR_SHORT (*n_windows = 0).  A span with end < start, a
 * NaN or a negative time: SD_ERR_ARG before anything is touched.  No segmentation network runs: a caller who wants silence removed passes the regions of
 * sd_activity* as spans.  Samples as for sd_diarize / _dev / _f32 / _wav (same SD_WAV_* flags, same refusals).  sd_span_masks is the mask stage alone. */
int sd_span_masks(sd_ctx*, int64_t n_samples, const sd_turn* spans, int64_t n_spans, int32_t label, float* h_masks /*[chunks*3][293]*/);     /* sd.cpp:3047-3078, 1641-1662 */
int sd_voiceprint(sd_ctx*, const int16_t* h_pcm, int64_t n, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb /*[192]*/, int64_t* n_windows);     /* sd.cpp:2436-2561, 2149-2167 */
int sd_voiceprint_dev(sd_ctx*, const int16_t* d_pcm, int64_t n, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb /*[192]*/, int64_t* n_windows);     /* sd.cpp:2436-2561, 2149-2167 */
int sd_voiceprint_f32(sd_ctx*, const float* h_wav, int64_t n, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb /*[192]*/, int64_t* n_windows);     /* sd.cpp:2436-2561, 2149-2167 */
int sd_voiceprint_wav(sd_ctx*, const char* path, int flags, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb /*[192]*/, int64_t* n_windows);     /* sd.cpp:2937-2951, 2436-2561 */
/* sd_speaker_distances: h_dist[k][m] = 1 - dot / (sqrt(m1) * sqrt(m2)) of centroid k and gallery row m, dot, m1 and m2 each a sequential sum over the d
 * dimensions (sd.cpp:476-498: the bits of the assignment step).  h_cen == NULL: the last job's centroids (K and d must be theirs).  A centroid row whose
 * first element is NaN (count 0) is skipped: NaN distances.  A zero-norm row among the others or anywhere in the gallery: SD_ERR_NUMERIC (the reference
 * throws, sd.cpp:493-495).
 * sd_match_speakers: the pairs with distance <= threshold (NaN = option "speaker_match_threshold", sd_set_option_f64, in [0, 2]; default t * t / 2 with
 * t = (double)0.7153814381597874f, the cosine distance at which the default clustering stops merging two unit vectors; a constant, it does not follow
 * "clustering_threshold") sorted by (distance, k, m); a pair is taken when both sides are still free: greedy, deterministic, one-to-one.
 * h_match[k] = the gallery row of centroid k or -1, h_dist_best[k] (may be NULL) = its distance or NaN. */
int sd_speaker_distances(sd_ctx*, const double* h_cen /*[K][d] or NULL*/, int64_t K, const double* h_gallery /*[M][d]*/, int64_t M, int d, double* h_dist /*[K][M]*/);     /* sd.cpp:476-498 */
int sd_match_speakers(sd_ctx*, const double* h_cen, int64_t K, const double* h_gallery, int64_t M, int d, double threshold, int32_t* h_match /*[K]*/, double* h_dist_best /*[K] or NULL*/);     /* sd.cpp:476-498, 293-316 */
/* host-only: voiceprint files -- text, one speaker per line: a name without white space, then 192 values printed with %.17g (read -> write -> read is
 * bit-exact); # starts a comment.  A malformed line (wrong number of values, not a finite number, a name twice) returns SD_ERR_ARG with the line number in
 * sd_voiceprints_error().  sd_read_voiceprints returns malloc'd names [M] and emb [M][192]: free both with sd_free_voiceprints. */
int sd_read_voiceprints(const char* path, char*** names, double** emb, int64_t* M);     /* no counterpart: the reference keeps no speaker between calls (sd.cpp:3433-3441) */
int sd_write_voiceprints(const char* path, const char* const* names, const double* emb, int64_t M);     /* no counterpart (sd.cpp:3433-3441) */
void sd_free_voiceprints(char** names, double* emb, int64_t M);
const char* sd_voiceprints_error(void);     /* reason for the last non-OK return of the two calls above */
/* sd_write_rttm_ex with names: the speaker field of a turn with label k is names[k] where 0 <= k < K and names[k] != NULL, SPEAKER_kk otherwise */
int sd_write_rttm_named(const char* path, const char* uri, const sd_turn* turns, int64_t n_turns, const double* conf /* or NULL */, const char* const* names /*[K]*/, int64_t K);     /* sd.cpp:3433-3441 */

/* ---- enrolled speakers: the clustering itself knows the people the caller has enrolled.  With a gallery V [M][d] set, every following call of this
 * ctx that clusters -- sd_clustering (not with num_clusters / min_clusters / max_clusters), the whole path, sd_finalize_dev, sd_stream_turns, rank 0 of a
 * sharded job -- follows this rule; E = the [rows][d] embeddings, its N train rows those whose first element is not NaN (sd.cpp:2224), ascending;
 * t = option "speaker_match_threshold":
 *  1 nearest: dist(x, m) = 1 - dot / (sqrt(m1) * sqrt(m2)), three sequential f64 sums (sd.cpp:476-498); g(x) = the smallest m that attains the minimum.
 *    A zero-norm train row: SD_ERR_NUMERIC.
 *  2 claim: x is claimed by g(x) iff dist <= t (inclusive, as sd_match_speakers); t = 2 claims every row: closed-set operation.
 *  3 used speakers: U = the distinct g of the claimed rows, ascending; G = |U|.  G = 0: the plain job, bit for bit.
 *  4 size rule: R = the unclaimed train rows, N' = |R|; mcs = min(min_cluster_size, max(1, round(0.1 * N))) -- from N, not N'.
 *  5 the rows of R are clustered as the plain job clusters its rows (f32-rounded norm, "clustering_method" / "clustering_threshold"); N' = 1: one
 *    cluster of one row; N' = 0: none.
 *  6 size split with mcs: candidates = V[U[0]] .. V[U[G-1]], then the means (un-normalised rows, member order) of the large clusters in ascending id;
 *    every small cluster goes to the nearest candidate (float minVal, dd < minVal, sd.cpp:2396, in that order).  One that goes to an enrolled candidate
 *    contributes to no mean; one that goes to a large cluster joins it.
 *  7 the surviving new clusters are renumbered 0 .. L-1 in sorted-id order (sd.cpp:519-548), their means recomputed over the merged membership in
 *    ascending row order (sd.cpp:2149-2167).
 *  8 assignment: ALL rows of E over the table [V[U[0]], .., V[U[G-1]], mean_0, .., mean_{L-1}], K = G + L, first maximum wins (sd.cpp:293-316), or
 *    the constrained arg-max under "constrained_assignment".  A label is a row of this table: enrolled people first in gallery order, then strangers.
 *  9 sd_last_speakers returns this table; the count of an enrolled row = the train rows it claimed in step 2, of a new row = its members.
 *    sd_last_enrolled returns [U[0], .., U[G-1], -1 x L].  sd_last_confidence works unchanged.
 * Refused with SD_ERR_ARG before anything is touched: a gallery together with any of the three cluster-count constraints, a gallery while a dump
 * directory is set (the step files describe the reference's flow), a clustering call whose d is not the gallery's. */
/* enrol a gallery for every following call of this ctx that clusters; h_gallery == NULL or M == 0 clears it.  The ctx keeps its own device copy.
 * A non-finite value: SD_ERR_ARG; a zero-norm row: SD_ERR_NUMERIC; the previous gallery stays in both cases. */
int sd_set_enrolled(sd_ctx*, const double* h_gallery /*[M][d]*/, int64_t M, int d);     /* sd.cpp:476-498 / 2149-2212 */
int sd_enrolled_info(const sd_ctx*, int64_t* M, int* d);     /* 0, 0 when none; sd.cpp:476-498 / 2149-2212 */
/* step 1 alone: h_gallery == NULL = the enrolled one (M and d must be its).  h_best [N], h_dist [N] (either may be NULL): the bits of sd_speaker_distances for
 * the same pair, the first minimum.  No N x M table exists: device memory beyond the operands is O(N + M). */
int sd_nearest_speakers(sd_ctx*, const double* h_X /*[N][d], no NaN rows*/, int64_t N, const double* h_gallery, int64_t M, int d,
                        int32_t* h_best, double* h_dist);     /* sd.cpp:476-498 / 2149-2212 */
/* gallery row of every label of the last call that clustered, -1 for a speaker nobody enrolled; all -1 without a gallery */
int sd_last_enrolled(const sd_ctx*, int32_t* h_rows /*[cap]*/, int64_t cap, int64_t* K);     /* sd.cpp:476-498 / 2149-2212 */

/* ---- many recordings in one call: replaces a loop of speakerDiarization() calls (sd.cpp:2937-3234) over short files.  The two networks run once over
 * all recordings -- their chunks share the segmentation batches ("seg_batch_chunks") and their live items the embedding batches -- and everything
 * behind the networks runs per recording, one after the other, exactly as in sd_diarize: every clustering option, "constrained_assignment" and an
 * enrolled gallery apply to every recording.  turns[r] / n_turns[r] (free each with sd_free_turns) are what sd_diarize returns for recording r alone
 * on this context, bit for bit, in "ecapa_precision" 0, 1 and 2; mode 3 repeats ALL batches of an embedding call on the f32 kernels when any
 * embedding overflows, so there a packed call equals the loop only while no recording of the pack triggers that fallback.
 * status[r] = SD_OK, SD_ERR_SHORT (sd_num_chunks(n[r]) <= 0; turns[r] = NULL) or SD_ERR_NUMERIC from that recording's clustering (turns[r] = NULL);
 * the other recordings go on and the call returns SD_OK.  Any other failure (SD_ERR_HIP, SD_ERR_MODEL) is returned at once and nothing stays
 * allocated to the caller.  Refused with SD_ERR_ARG before anything is touched: R < 1, a null row, a dump directory set (the step files describe
 * one recording), a planted workload set (its chunk range means one recording), the refusals of an enrolled gallery (above), and a pack of more
 * than SD_MANY_MAX_CHUNKS chunks (sd_many_plan's total: 3 * 501 feature rows per chunk must stay within the int row counts of a launch, 2^31 / 4).
 * Host float rows must hold finite samples: the first convolution reads 4 samples past a recording's last window with zero weights, and in a
 * pack those can be the first samples of the next recording.
 * sd_stage_ms: [0], [1] = the shared inference, [2] = the sum of the finalizes, [3] = the call.
 * sd_many_plan (host-only): the packed layout.  Recording r has chunks_r = sd_num_chunks(n[r]) chunks and a slot of roundup32(chunks_r + 9) chunks
 * (none when chunks_r <= 0) at chunk_base[r] = the sum of the earlier slots; *total_chunks = the sum of all slots.  Its samples sit at sample
 * 8000 * chunk_base[r] of the packed waveform with zeros behind them up to the end of the slot, which lies at or behind the end of its last
 * chunk's 80 000-sample window; every base is a multiple of 32 chunks = 3 reference embedding batches (sd.cpp:2429).
 * sd_many_select: makes recording r of the last sd_diarize_many* call of this ctx -- or stream r of its last sd_stream_turns_many call, whichever
 * of the two came later -- "the last job" for sd_last_confidence, sd_last_speakers and sd_last_enrolled (after the call itself that is the last
 * recording that was finalized); SD_ERR_ARG for an r outside the call or one whose status is not SD_OK. */
#define SD_MANY_MAX_CHUNKS 357199
int sd_many_plan(const int64_t* n, int64_t R, int64_t* chunk_base /*[R]*/, int64_t* total_chunks);     /* sd.cpp:1419, 1457, 2429 */
int sd_diarize_many(sd_ctx*, const int16_t* const* h_pcm /*[R]*/, const int64_t* n /*[R]*/, int64_t R, sd_turn** turns /*[R]*/, int64_t* n_turns /*[R]*/, int32_t* status /*[R]*/);     /* sd.cpp:2937-3234 */
int sd_diarize_many_dev(sd_ctx*, const int16_t* const* d_pcm /*[R]*/, const int64_t* n /*[R]*/, int64_t R, sd_turn** turns /*[R]*/, int64_t* n_turns /*[R]*/, int32_t* status /*[R]*/);     /* sd.cpp:2937-3234 */
int sd_diarize_many_f32(sd_ctx*, const float* const* h_wav /*[R]*/, const int64_t* n /*[R]*/, int64_t R, sd_turn** turns /*[R]*/, int64_t* n_turns /*[R]*/, int32_t* status /*[R]*/);     /* sd.cpp:2937-3234, 2948-2951 */
int sd_many_select(sd_ctx*, int64_t r);     /* sd.cpp:2149-2167, 2191-2207 */

/* ---- recordings in their own rate and encoding: the head of speakerDiarization() (sd.cpp:2937-2951: WavReader, / 32768) and the dormant resample leg
 * (frontend/resampler.cc:19-36) for every recording of a pack, on the device.  Telephony files are 8 kHz, mostly G.711 at one byte per sample, often
 * stereo with one party per channel; sd_diarize_many_audio* takes them as they are and fills the packed waveform in one kernel launch (k_many_ingest,
 * csrc/ingest.hip) -- no per-recording sd_resample, no round trip.
 * THE RULE.  A recording a defines 16 kHz mono floats y in three steps.
 *   1. Decode.  SD_ENC_S16: v * 2^-15 (sd.cpp:2950).  SD_ENC_F32: the value itself.  SD_ENC_MULAW: with u = ~code, t = (((u & 15) << 3) + 132) <<
 *      ((u >> 4) & 7), s = t - 132, negative when u & 0x80; the sample is s * 2^-15.  SD_ENC_ALAW: with a = code ^ 0x55, e = (a >> 4) & 7, m = a & 15,
 *      s = e ? ((m << 4) + 264) << (e - 1) : (m << 4) + 8, positive when a & 0x80; the sample is s * 2^-15.  These are ITU-T G.711's tables;
 *      sd_g711_decode (host-only) returns s for n codes.
 *   2. Channel.  Channel c of frame i is element i * channels + c.  channel == -1 is SD_WAV_DOWNMIX's rule: s = +0.0f, s += x_q in channel order in
 *      float, then s / (float)channels correctly rounded.
 *   3. Rate.  At 16 000 Hz y is that sequence; at any other rate y = sd_resample(x, n, sample_rate, 16000), of length sd_resample_len(n, sample_rate,
 *      16000).  sd_audio_len16 (host-only) returns that length, or -1 for a bad descriptor (n < 0 or n > 2^40, sample_rate <= 0, an unknown encoding,
 *      channels < 1, channel outside [-1, channels)).
 * THE CONTRACT.  Recording r gets, byte for byte, what sd_diarize_f32(ctx, y_r, len_r) gives for it alone -- turns, order, labels, confidences,
 * sd_last_speakers and sd_last_enrolled after sd_many_select(r), status -- in any order of the pack and under every option sd_diarize_many_f32 honours.
 * A recording whose y has no chunk (n == 0 included) gets SD_ERR_SHORT and the others go on.  _dev: data are device pointers.
 * Refused with SD_ERR_ARG, nothing touched, the recording named: a null data with n > 0; a bad descriptor (above); a rate pair sd_resample refuses or
 * whose tile span does not fit the LDS next to the tile's outputs (sd_stream_set_input_rate's rule); for _dev a pointer not aligned to its element; and
 * everything sd_diarize_many refuses (a dump directory, a planted workload, the pack limits counted on sd_audio_len16, the enrolled refusals).
 * sd_read_wav_audio (host-only): a wav file as such a recording -- format tag 1 with 16 bits, tag 7 (mu-law) or tag 6 (A-law) with 8 bits, any channel
 * count and rate; *data = the raw data bytes, malloc'd (free), *desc filled with channel = 0.  Any other file is SD_ERR_ARG: the caller falls back to
 * sd_read_wav / sd_read_wav_f32, which are unchanged. */
enum { SD_ENC_S16 = 0, SD_ENC_F32 = 1, SD_ENC_MULAW = 2, SD_ENC_ALAW = 3 };
typedef struct sd_audio {
    const void* data;      /* n * channels interleaved elements: int16, float, or one G.711 code per byte */
    int64_t n;             /* sample frames */
    int32_t sample_rate;   /* > 0 */
    int32_t encoding;      /* SD_ENC_* */
    int32_t channels;      /* >= 1 */
    int32_t channel;       /* 0 .. channels-1: that channel; -1: the mean of all (SD_WAV_DOWNMIX's rule) */
} sd_audio;
int64_t sd_audio_len16(const sd_audio*);     /* resampler.cc:21-22 */
int sd_g711_decode(int32_t encoding, const uint8_t* codes, int64_t n, int16_t* out);     /* ITU-T G.711; the reference reads PCM only (wav.h:99-122) */
int sd_read_wav_audio(const char* path, sd_audio* desc, void** data);     /* wav.h:62-126 */
int sd_diarize_many_audio(sd_ctx*, const sd_audio* rec /*[R]*/, int64_t R, sd_turn** turns /*[R]*/, int64_t* n_turns /*[R]*/, int32_t* status /*[R]*/);     /* sd.cpp:2937-3234, 2948-2951; resampler.cc:19-36 */
int sd_diarize_many_audio_dev(sd_ctx*, const sd_audio* rec /*[R]*/, int64_t R, sd_turn** turns /*[R]*/, int64_t* n_turns /*[R]*/, int32_t* status /*[R]*/);     /* sd.cpp:2937-3234, 2948-2951; resampler.cc:19-36 */

/* ---- streams in their own encoding: a live call is 8 kHz G.711 at one byte per sample, often interleaved stereo with one party per channel.  After
 * sd_stream_set_input_format(s, encoding, channels, channel) the stream takes its audio as it arrives, through the four _audio pushes, and decodes it
 * on the device (k_group_ingest, csrc/stream_ingest.hip) -- no host decode, no de-interleaving, and both legs of a stereo call from one upload.
 * THE RULE.  A stream with a format receives interleaved frames of `channels` elements.  Frame i becomes one float by steps 1 (decode) and 2 (channel)
 * of the rule of sd_audio above, the same text on the device as sd_diarize_many_audio* runs.  Step 3 (rate) is the stream's own: it follows
 * sd_stream_set_input_rate, which may be called before or after the format; both are set before the first sample.
 * THE CONTRACT.  Let x be the mono float sequence that steps 1 and 2 define on all frames pushed so far.  After any sequence of single and group
 * pushes the stream is, bit for bit, the stream with the same input rate (or none) to which x was pushed with sd_stream_push_f32: sd_stream_info,
 * sd_stream_input_info (n_in counts frames), sd_stream_turns (turns, order, labels), sd_last_confidence, sd_last_speakers, sd_stream_read, sealing,
 * window / forget and the roster.  So after sd_stream_end_input the turns are those of sd_diarize_many_audio for the sd_audio that describes
 * everything pushed.
 * A stream without a format keeps every path it has: sd_stream_push / _dev / _f32 and sd_stream_push_many / _dev / _f32 launch what they launched.  A
 * stream with a format takes only the _audio pushes: a typed push on it is SD_ERR_ARG, and so is its row of a typed group call with n[i] > 0; an _audio
 * push on a stream without a format is SD_ERR_ARG (in a group call: its row with frames[i] > 0).  The format (SD_ENC_S16, 1, 0) is legal and gives the
 * bytes of sd_stream_push, so that a host which sets the format from a variable ends every call the same way.
 * sd_stream_push_many_audio*: S streams of one context, of any formats and rates; frames[i] == 0 with any pointer is legal.  Host form: one upload per
 * DISTINCT SOURCE -- rows whose data pointer, frames, encoding and channels are equal (the legs of one stereo call, which differ in `channel` only) share
 * one upload and read the same device bytes -- and only the bytes the rule reads go up (for channel c of the last frame nothing behind element c; for
 * rows that share, the largest count among them).  Then one table upload, ONE k_group_ingest launch, at most ONE k_resample_jobs launch and one
 * synchronisation whatever S, the formats and the rates, and the packed inference of sd_stream_push_many.  A single push is sd_stream_push with the same
 * kernel on a table of one row as its conversion launch.
 * Refused with SD_ERR_ARG before anything is touched (a group call names the stream): sd_stream_set_input_format after a sample was pushed or the input
 * was closed, for an unknown encoding, channels < 1 or a channel outside [-1, channels); a push of frames < 0 or frames > 2^40, of a null pointer with
 * frames > 0, of a piece whose bytes exceed 2^42, in the _dev forms of a pointer not aligned to its element, on a closed input, and everything
 * sd_stream_push and sd_stream_push_many refuse.  An argument error, or a failed allocation of the staging workspaces (before the first launch), leaves
 * the stream usable and exactly what it was, the inputs held by a rated stream included; any other SD_ERR_HIP makes the stream (in a group call: the
 * streams of the call) unusable, as for the typed pushes.
 * sd_stream_input_format: the format and whether one was set; any pointer may be NULL; a stream without one reports SD_ENC_S16, 1, 0, 0. */
int sd_stream_set_input_format(sd_stream*, int32_t encoding /*SD_ENC_**/, int32_t channels, int32_t channel /* -1: the mean */);     /* wav.h:99-122, sd.cpp:2948-2951 */
int sd_stream_input_format(const sd_stream*, int32_t* encoding, int32_t* channels, int32_t* channel, int32_t* is_set);     /* wav.h:99-122 */
int sd_stream_push_audio(sd_stream*, const void* h_data, int64_t frames);     /* wav.h:99-122, sd.cpp:2948-2951; resampler.cc:19-36 */
int sd_stream_push_audio_dev(sd_stream*, const void* d_data, int64_t frames);     /* wav.h:99-122, sd.cpp:2948-2951; resampler.cc:19-36 */
int sd_stream_push_many_audio(sd_stream* const* s /*[S]*/, const void* const* h_data /*[S]*/, const int64_t* frames /*[S]*/, int64_t S);     /* sd.cpp:2937-3234, 2948-2951; resampler.cc:19-36 */
int sd_stream_push_many_audio_dev(sd_stream* const* s /*[S]*/, const void* const* d_data /*[S]*/, const int64_t* frames /*[S]*/, int64_t S);     /* sd.cpp:2937-3234, 2948-2951; resampler.cc:19-36 */

/* ---- scoring against a ground truth (host-only, no context, no GPU).  The reference has no counterpart: it prints turns and measures nothing.
 * sd_der is the diarization error rate of pyannote.metrics' DiarizationErrorRate, restated:
 *  - the time line is cut at every start and end of a turn of ref and of hyp (and of a uem span and a collar zone, below).  In an elementary interval of
 *    length D, A = the distinct labels of the reference turns that cover it, B = those of the hypothesis turns;
 *      total += |A| D,  missed += max(0, |A| - |B|) D,  false_alarm += max(0, |B| - |A|) D,
 *      correct += |{a in A : map(a) in B}| D,  confusion += (min(|A|, |B|) - that count) D;
 *    der = (missed + false_alarm + confusion) / total, NaN when total == 0.
 *  - map is the one-to-one pairing of reference and hypothesis labels that maximises the summed co-occurrence duration (sum of D over the scored
 *    intervals with a in A and b in B), found by a rectangular assignment solver for any number of labels.  Every optimal pairing gives the same
 *    correct, so the components are defined where the pairing is not unique; a pair that never co-occurs is no pair.
 *  - uem (may be NULL): only time inside these spans is scored; their labels are not read.
 *  - collar (seconds, >= 0): around every start and end t of a reference turn the zone from the f64 value t - collar / 2 to the f64 value
 *    t + collar / 2 is not scored (pyannote's convention: half on each side).
 *  - skip_overlap != 0: intervals with |A| >= 2 are not scored.
 * Arithmetic is f64: intervals in ascending time, each length one subtraction of two boundaries, each component a sum that carries its rounding
 * errors (the result is the exact sum of those lengths rounded once).  Labels are any integers >= 0.  map[h] (h < cap; map may be NULL with
 * cap = 0) = the reference label paired with hypothesis label h, or -1; *n_map = the largest hypothesis label + 1.
 * SD_ERR_ARG: a negative or NaN time, end < start, a negative label, a negative or NaN collar.
 * sd_read_rttm: the SPEAKER lines of an RTTM file as sd_write_rttm* and pyannote write them: fields separated by white space, field 2 the uri
 * (uri != NULL keeps the lines of that uri only), 4 the start, 5 the duration (end = start + duration), 8 the speaker name.  Labels number the
 * names in order of first appearance; names [K] (may be NULL) returns them.  Lines of other record types and ;; comments are passed over; a
 * SPEAKER line with fewer than 8 fields or a start or duration that is not a number >= 0 returns SD_ERR_ARG.  Free the turns with sd_free_turns,
 * the names with sd_free_rttm_names.  sd_score_error = the reason for the last non-OK return of sd_der / sd_read_rttm, with the line number. */
typedef struct sd_der_result { double der, total, missed, false_alarm, confusion, correct; } sd_der_result;
int sd_der(const sd_turn* ref, int64_t n_ref, const sd_turn* hyp, int64_t n_hyp, const sd_turn* uem /* or NULL */, int64_t n_uem, double collar,
           int skip_overlap, sd_der_result* result, int32_t* map /*[cap] or NULL*/, int64_t cap, int64_t* n_map /* or NULL */);
int sd_read_rttm(const char* path, const char* uri /* or NULL */, sd_turn** turns, int64_t* n, char*** names /* or NULL */, int64_t* K /* or NULL */);
void sd_free_rttm_names(char** names, int64_t K);
const char* sd_score_error(void);

/* ---- many cuts of one dendrogram: for a caller who tries several clustering thresholds on one recording.  The linkage is most of a finalize and
 * depends on none of "clustering_threshold", "min_cluster_size" and "num_clusters"; a cut object runs it once.
 * sd_cut_open_dev (d_seg, d_emb as for sd_finalize_dev) and the whole-path forms sd_cut_open / _pcm_dev / _f32 / _wav (samples as for sd_diarize /
 * _dev / _f32 / _wav: same flags, same refusals; both networks run inside) do everything of a finalize that does not depend on the cut: binarisation,
 * speaker count, the f64 embeddings, the train rows (sd.cpp:2224), their gathered and normalised copies, and ONE linkage with the context's
 * "clustering_method" at that moment.  The cut owns copies of all of it, on the device and -- the dendrogram -- on the host: other calls on the
 * context may come between two calls on a cut.
 * sd_cut_turns_many evaluates T cuts: turns[t] / n_turns[t] (free each with sd_free_turns) and K[t] (may be NULL; the number of label columns, largest
 * label + 1) are what sd_finalize_dev returns on the same inputs with the three options of specs[t] set -- turns, order and labels, bit for bit.
 * In a spec a NaN threshold, min_cluster_size 0 and num_clusters 0 mean the context's current option; num_clusters -1 means unset.  "min_clusters",
 * "max_clusters" and "constrained_assignment" are read from the context at the call.  The context's options are never changed.  After the call
 * sd_last_confidence and sd_last_speakers describe cut T - 1 as after that sd_finalize_dev.  sd_cut_turns is the T = 1 case of the same code.
 * All cuts of a group share their device launches: one assignment of every embedding to the centroids of all cuts, one pass over the frames for
 * the activations of all cuts, one selection of the most active clusters, one copy back.  A group is the longest run of consecutive specs whose
 * activation tables fit a byte budget (1 GiB; test key "cut_group_bytes"); results do not depend on the grouping.  Under "constrained_assignment"
 * the assignment runs cut by cut.
 * sd_cut_dendrogram: the linkage matrix Z [N - 1][4] of the N train rows (*N; at most cap rows are written, Z may be NULL); its heights are the
 * only thresholds at which a cut can change.  N < 2: no row.
 * SD_ERR_ARG before anything is touched, at open and at every evaluation: an enrolled gallery (its flow clusters other rows), a dump directory
 * (the step files describe one finalize); at an evaluation also a threshold outside [0, 2], min_cluster_size < 0, num_clusters < -1.
 * sd_destroy closes the cuts still open.  Not for streams, sd_diarize_many or the sharded path; another linkage method needs another cut. */
typedef struct sd_cut sd_cut;
typedef struct sd_cut_spec { double threshold; int32_t min_cluster_size; int32_t num_clusters; } sd_cut_spec;
int sd_cut_open_dev(sd_ctx*, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, sd_cut** cut);
int sd_cut_open(sd_ctx*, const int16_t* h_pcm, int64_t n, sd_cut** cut);
int sd_cut_open_pcm_dev(sd_ctx*, const int16_t* d_pcm, int64_t n, sd_cut** cut);
int sd_cut_open_f32(sd_ctx*, const float* h_wav, int64_t n, sd_cut** cut);
int sd_cut_open_wav(sd_ctx*, const char* path, int flags, sd_cut** cut);
int sd_cut_turns(sd_cut*, const sd_cut_spec* spec, sd_turn** turns, int64_t* n_turns, int32_t* K /* or NULL */);
int sd_cut_turns_many(sd_cut*, const sd_cut_spec* specs /*[T]*/, int64_t T, sd_turn** turns /*[T]*/, int64_t* n_turns /*[T]*/, int32_t* K /*[T] or NULL*/);
int sd_cut_dendrogram(const sd_cut*, double* h_Z /*[cap][4] or NULL*/, int64_t cap, int64_t* N);
int sd_cut_info(const sd_cut*, int64_t* chunks, int64_t* n_samples, int64_t* train_rows);      /* any pointer may be NULL */
void sd_cut_close(sd_cut*);

/* ---- a18: the reference's output line (sd.cpp:3439) */
int sd_format_turn(const sd_turn* t, char* buf, int cap);

/* ---- the reference's four stage timers (sd.cpp:53-60; labels of sd.cpp:3028, 3110, 3231, 3434): wall ms of the last
 * sd_diarize* call, [0]=segmentation [1]=embedding [2]=clustering [3]=total; after a whole-path sd_activity* call [0] and [3], the others 0 */
int sd_stage_ms(const sd_ctx*, double* ms4);
/* ---- options.  Product keys (the knobs clustering/Clustering.py and the multi-GPU path expose; the reference hard-codes them):
 * "num_clusters", "min_clusters", "max_clusters" (-1 = unset; Clustering.py:21-43), "constrained_assignment" (1 = constrained_argmax of
 * Clustering.py:81-94: the local speakers of a chunk go to different clusters; applies to sd_clustering* and the whole path),
 * "clustering_method" (SD_LINKAGE_*, default SD_LINKAGE_CENTROID = 3), "min_cluster_size" (>= 1, default 15) and, through sd_set_option_f64,
 *   "clustering_threshold" (0 .. 2, default (double)0.7153814381597874f): the three hyper-parameters of Clustering.py:251-276 / 317-333, which the
 *   reference hard-codes (sd.cpp:2049-2056).  Centroid, median and ward run on the unit-normalised rows with euclidean distances, the other four on
 *   the rows as they are with the cosine metric.  They apply to sd_clustering*, the whole path, sd_finalize_dev and the sharded path,
 * "max_num_embeddings" (-1 = unset (default), or >= 1; anything else SD_ERR_ARG) and "clustering_seed" (any int64, default 0):
 *   BaseClustering.max_num_embeddings of Clustering.py:12, 69-76, which the port carries commented out (sd.cpp:2218, 2231-2249: "IS INF").  Let T be
 *   the train rows of a clustering call: the row indices i of emb [M][d] whose first element is not NaN (sd.cpp:2224), ascending.  With the option
 *   unset or |T| <= max_num_embeddings nothing changes.  Otherwise the max_num_embeddings rows of T with the smallest key(seed, i) stay, ascending
 *   by i, where in 64-bit wrap-around arithmetic
 *       G = 0x9E3779B97F4A7C15,  fin(x): x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31
 *       key(seed, i) = fin(fin((uint64)seed + G) + (uint64)i * G).
 *   fin is a bijection and G is odd: distinct i have distinct keys and there is no tie rule.  i is the row's index in the table the call was
 *   given (chunk * 3 + speaker), not its position among the train rows; the sample for m is a subset of the sample for m + 1; a row appended
 *   to a growing recording removes at most one row from the sample.  From there on the sample IS "the train rows", as in Clustering.py: N of the
 *   minimum-cluster-size rule and of the number-of-clusters rules is the sample size, the linkage, the cut and the small-cluster pass see the sample
 *   only, centroids are means of sampled rows, sd_last_speakers counts sampled rows, voiceprints of an enrolled gallery claim among the sampled
 *   rows -- and the final assignment labels ALL M rows as ever.  A deliberate deviation: the reference draws the sample with random.shuffle; the
 *   keyed choice is the deterministic form of the same uniform sample.  Read wherever train rows are taken: sd_clustering*, the whole path,
 *   sd_finalize_dev, rank 0 of a sharded job, streams, every recording of sd_diarize_many (i is local to the recording's own table) and, at
 *   open, cut objects (sd_cut_info's train_rows and sd_cut_dendrogram describe the sample).  sd_sample_rows below shows the rule.  While the
 *   option is set a call that clusters under a dump directory returns SD_ERR_ARG: the step files describe the reference's flow, which clusters
 *   every train row (the same refusal as for an enrolled gallery),
 * "ecapa_precision" (0 = f32 MFMA = the reference's ORT precision (default); 1 = fp16 weights and activations on the fp16 MFMA with f32
 *   accumulation; 2 = the same with hi + lo fp16 weight planes; 3 = f32 tensors, both MFMA operands split into hi + lo fp16 halves, three
 *   products per multiply-add: f32-grade embeddings (<= 1e-7 cosine distance to mode 0) at about half of mode 0's time; a batch whose activations
 *   leave fp16's range is detected and repeated on the f32 kernels),
 *   Mode 0 is f32 storage, f32 MFMA products and f32 accumulation; its transcendentals are the hardware forms, not libm: tanh / sigmoid of
 *   the LSTM gates through v_exp_f32 + v_rcp_f32, the softmax of the attentive pooling through v_exp_f32 / v_rcp_f32 (each <= 1 ulp of
 *   the f32 result, i.e. ~1e-7 relative -- three orders below the parity tolerance rtol 1e-3 / atol 1e-4, and below what a different
 *   summation order already moves); "f32 = the reference's precision" means that class of result, not libm-bit-identical.
 * "seg_precision" (-1 = auto (default): 3 whenever "ecapa_precision" is not 0 -- a caller who asked for an fp16-pipe mode gets it in both networks --
 *   else 0; 0 = f32 MFMA; 3 = the same operand split for PyanNet's LSTM: input projections of layers 1-3 and the recurrence; scores within 2e-6 of
 *   mode 0, identical turns on the planted hour and on the reference's 1-min wav),
 * "rank0_permille" (sd_diarize_sharded: share of the chunks rank 0 infers itself, -1 = equal),
 * "comm_timeout_ms" (deadline of the exchange step of a sharded job, default 600 000),
 * "activity_hamming" (0 / 1, see sd_activity* above),
 * "linkage_batch" (0 (default) / 1; anything else SD_ERR_ARG): 1 = the group calls (sd_diarize_many*, sd_stream_turns_many) run the dendrograms of
 *   their jobs ahead of the per-job finalize, in shared launches with one workgroup per job (what sd_linkage_many does), for every job that
 *   clusters 2 .. 1499 train rows without an enrolled gallery; 0 = one job after the other.  Results are the same bytes either way; single-job
 *   entries never look at it.  Worth setting where the jobs of a call are short (recordings or streams of a few minutes, or any length under
 *   "max_num_embeddings" <= 1499): 64 streams at 1 min update in 31 ms instead of 106.  Off by default because jobs of 1500 train rows and more
 *   -- a stream from about 10 minutes on -- take sd_linkage_ex's own route either way and gain nothing (README, "batched small-N linkage").  "linkage_batch_bytes" (>= 1, default 2 GiB): the device bytes the workspaces of one such group of jobs may take, here and
 *   in sd_linkage_many; more jobs than fit run in several groups, and results do not depend on the grouping.
 * "linkage_batch_xcd" (0 (default) / 1; anything else SD_ERR_ARG): 1 = sd_linkage_many -- and with it, under "linkage_batch" = 1, the group calls -- runs
 *   the jobs that sd_linkage_ex gives to its cooperative kernel on one XCD (1500 .. 15 999 rows on a device of 256 CUs; at least two in the call, each
 *   within "linkage_batch_bytes": 8 N^2 bytes and a little) eight to a launch, one job per XCD, after a shared preparation.  A job that meets an exact tie
 *   there, or whose launch is refused or times out, is run again alone; results are the same bytes either way.  0 = every call launches what it launched
 *   before the key existed.  Measured: 8 .. 64 jobs of 1 500 .. 8 000 rows 5.2 - 6.4 x the loop of sd_linkage_ex.  Off by default because jobs with duplicate rows
 *   -- every stream of the synthetic workload -- tie at height 0, are redone alone and gain nothing (README, "Mid-size linkage jobs, one per XCD").
 * "linkage_batch_xcd_zero" (0 (default) / 1; anything else SD_ERR_ARG; read only where "linkage_batch_xcd" = 1): 1 = a job of such a launch that stops at
 *   a tie at height 0 in front of its first merge -- duplicate rows: looped audio, digital silence, synthetic streams -- stays in the batch: the heap replay
 *   takes the merges at height 0 and the cooperative kernel the rest, the three steps sd_linkage_ex takes for such a job alone, up to eight jobs to a launch,
 *   one per XCD.  A tie above 0, a tie after a merge, a refused launch or a timeout still sends the job through sd_linkage_ex's route alone; results are
 *   the same bytes either way, for every method and both metrics.  0 = every call launches what it launched before the key existed (a job that ties is
 *   redone alone).  Measured: 8 .. 64 jobs of 1 500 .. 8 000 rows with 5 % copied rows 5.2 - 6.6 x the loop of sd_linkage_ex; 64 streams at 10 min update in
 *   191 ms instead of 986 with "linkage_batch", "linkage_batch_xcd" and this key at 1.  Off by default because that behaviour of "linkage_batch_xcd" = 1 is
 *   pinned by its tests and a default changes in a step of its own (README, "Ties at height 0 inside the XCD batch"; profiles/linkage_xcd_zero_times.txt).
 * Test and tuning keys are listed in sdhip_test.h.  An unknown key returns SD_ERR_ARG. */
int sd_set_option(sd_ctx*, const char* key, int64_t value);
/* the real-valued keys: "clustering_threshold" (Clustering.py:251-276 / 317-333; outside [0, 2] or NaN: SD_ERR_ARG) and the four "activity_*" keys of
 * sd_activity* above (NaN or out of range: SD_ERR_ARG), and "speaker_match_threshold" of sd_match_speakers above (outside [0, 2] or NaN: SD_ERR_ARG).
 * An unknown key returns SD_ERR_ARG. */
int sd_set_option_f64(sd_ctx*, const char* key, double value);
/* host-only: the rule of "max_num_embeddings" on a list of n distinct rows >= 0 in ascending order, through the function the clustering stage
 * applies.  max_num = -1 or >= 1.  Returns the number of rows written to out -- min(n, max_num), n under -1 -- or -SD_ERR_ARG. */
int64_t sd_sample_rows(const int32_t* rows /*[n] ascending*/, int64_t n, int64_t max_num, int64_t seed,
                       int32_t* out /*[min(n, max_num)]*/);     /* Clustering.py:69-76; sd.cpp:2231-2249 */

#ifdef __cplusplus
}
#endif
#endif
