// pipeline.cpp -- stage wrappers and the whole-path entries behind the C ABI: a source is brought to a DevWav (bring), then the family's tail runs.
// speakerDiarization() (sd.cpp:2937-3234) re-stated as: scale pcm -> segmentation -> post-seg ->
// embeddings -> [multi-GPU: all-gather here] -> count, clustering, reconstruction, annotation.
#include "common.h"
#include "wav_file.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>

// a1 tail: input_wav[i] = pcm_to_float(sample) (common.h)
__global__ void k_pcm_to_f32(const int16_t* __restrict__ pcm, float* __restrict__ dst, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = pcm_to_float(pcm[i]);
    else if (i < n + SD_WAV_PAD) dst[i] = 0.0f;   // padding: SincNet's 256-tap rows read 4 samples past the last window (zero weights, finite data)
}
// embeddings are widened to double before clustering (sd.cpp:2555)
__global__ void k_f32_to_f64(const float* __restrict__ a, double* __restrict__ b, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) b[i] = (double)a[i];
}
__global__ void k_mark_inactive(int* __restrict__ hard, const int* __restrict__ nact, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && nact[i] == 0) hard[i] = -2;                                  // sd.cpp:3172-3191
}

// the launches of the two kernels above (finalize_front / finalize, many.hip, the test hooks); asynchronous on c->stream
int launch_f32_to_f64(sd_ctx* c, const float* d_a, double* d_b, int64_t n)
{
    hipLaunchKernelGGL(k_f32_to_f64, GRID1(n), 0, c->stream, d_a, d_b, n);
    KCHECK(c);
    return SD_OK;
}
int launch_mark_inactive(sd_ctx* c, int* d_hard, const int* d_nact, int64_t n)
{
    hipLaunchKernelGGL(k_mark_inactive, GRID1(n), 0, c->stream, d_hard, d_nact, n);
    KCHECK(c);
    return SD_OK;
}

// planted workload (sd_set_planted): rows that are not NaN by the reference's rule take the planted embedding.
// One 192-thread block per row: every thread reads element 0 before anyone overwrites it.
__global__ void k_plant_emb(float* __restrict__ emb, const float* __restrict__ planted)
{
    const size_t i = (size_t)blockIdx.x * SD_EMB_DIM + threadIdx.x;
    const float first = emb[(size_t)blockIdx.x * SD_EMB_DIM];
    const float v = planted[i];
    __syncthreads();
    if (first == first) emb[i] = v;
}

// ------------------------------------------------------------------ a2+a3
extern "C" int sd_segment_dev(sd_ctx* c, const float* d_wav, int64_t n, float* d_out, int64_t chunks)
{
    ENTER(c);
    if (!d_wav || !d_out || n <= 1) SD_FAIL(c, SD_ERR_ARG, "sd_segment_dev: bad argument");
    if (chunks != sd_num_chunks(n, nullptr)) SD_FAIL(c, SD_ERR_ARG, "sd_segment_dev: chunks must equal sd_num_chunks(n)");
    int rc = run_segment(c, DevWav{d_wav, n, 0, false}, 0, chunks, d_out);      // the caller's buffer: nothing is known about the bytes behind sample n
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

extern "C" int sd_segment(sd_ctx* c, const float* h_wav, int64_t n, float* h_out, int64_t* chunks)
{
    ENTER(c);
    if (!h_wav || !h_out || !chunks) SD_FAIL(c, SD_ERR_ARG, "sd_segment: bad argument");
    const int64_t nc = sd_num_chunks(n, nullptr);
    *chunks = nc;
    if (nc <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)n);
    DTMP(c, dw, (n + SD_WAV_PAD) * sizeof(float)); DTMP(c, ds, nc * SD_FRAMES * 3 * sizeof(float));
    HIPCHK(c, hipMemcpy(dw.p, h_wav, n * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset((float*)dw.p + n, 0, SD_WAV_PAD * sizeof(float)));
    int rc = run_segment(c, DevWav{(const float*)dw.p, n, 0, true}, 0, nc, (float*)ds.p);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_out, ds.p, nc * SD_FRAMES * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}

// SegmentModel::infer as the reference declares it (sd.cpp:1352-1404): [rows][T] separate waveforms -> [rows][293][3]; *frames = the
// frames the network yields for T samples (293 for T = 80000), the rest of each row's 293 is zero (slide()'s padding, sd.cpp:1473-1479)
extern "C" int sd_segment_chunks(sd_ctx* c, const float* h_chunks, int64_t rows, int64_t T, float* h_out, int32_t* frames)
{
    ENTER(c);
    if (!h_chunks || !h_out || rows <= 0 || T < 1 || T > SD_CHUNK) SD_FAIL(c, SD_ERR_ARG, "sd_segment_chunks: bad argument (rows >= 1, 1 <= T <= %d)", SD_CHUNK);
    // persistent workspaces, not per-call allocations: slide() calls infer once per batch of 32 chunks (225 times per hour of audio)
    WS(c, float, dw, "rows_wav", rows * T + SD_WAV_PAD); WS(c, float, ds, "rows_seg", rows * SD_FRAMES * 3);
    HIPCHK(c, hipMemcpyAsync(dw, h_chunks, rows * T * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(dw + rows * T, 0, SD_WAV_PAD * sizeof(float), c->stream));
    int fr = 0;
    if (int rc = run_segment_rows(c, DevWav{dw, rows * T, 0, true}, (int)T, ds, &fr)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_out, ds, rows * SD_FRAMES * 3 * sizeof(float), hipMemcpyDeviceToHost));
    if (frames) *frames = fr;
    return SD_OK;
}

// ------------------------------------------------------------------ a4-a6
extern "C" int sd_postseg(sd_ctx* c, const float* h_seg, int64_t chunks, uint8_t* h_bin, float* h_masks,
                          int32_t* h_count, int64_t cap_count, int64_t* n_count)
{
    ENTER(c);
    if (!h_seg || chunks <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_postseg: bad argument");
    const int64_t ne = chunks * SD_FRAMES * 3;
    const int64_t nf = count_frames_host(chunks);
    if (n_count) *n_count = nf;
    if (h_count && cap_count < nf) SD_FAIL(c, SD_ERR_ARG, "sd_postseg: count capacity %lld < %lld", (long long)cap_count, (long long)nf);
    DTMP(c, ds, ne * sizeof(float)); DTMP(c, db, ne); DTMP(c, dm, ne * sizeof(float)); DTMP(c, dn, chunks * 3 * sizeof(int)); DTMP(c, dc, nf * sizeof(int32_t));
    HIPCHK(c, hipMemcpy(ds.p, h_seg, ne * sizeof(float), hipMemcpyHostToDevice));
    int rc = run_postseg(c, (const float*)ds.p, chunks, (uint8_t*)db.p, (float*)dm.p, (int*)dn.p);
    if (rc) return rc;
    if ((rc = run_count(c, (const uint8_t*)db.p, chunks, (int32_t*)dc.p, nf))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_bin) HIPCHK(c, hipMemcpy(h_bin, db.p, ne, hipMemcpyDeviceToHost));
    if (h_masks) HIPCHK(c, hipMemcpy(h_masks, dm.p, ne * sizeof(float), hipMemcpyDeviceToHost));
    if (h_count) HIPCHK(c, hipMemcpy(h_count, dc.p, nf * sizeof(int32_t), hipMemcpyDeviceToHost));
    return SD_OK;
}

// ------------------------------------------------------------------ a12-a14
// method / metric of the *_ex entries and sd_linkage_many (Clustering.py:251-276 / 317-333); 0 = fine
int check_method_metric(sd_ctx* c, int method, int metric)
{
    if (method < SD_LINKAGE_SINGLE || method > SD_LINKAGE_WEIGHTED) SD_FAIL(c, SD_ERR_ARG, "unknown linkage method %d (SD_LINKAGE_SINGLE .. SD_LINKAGE_WEIGHTED)", method);
    if (metric != SD_METRIC_EUCLIDEAN && metric != SD_METRIC_COSINE) SD_FAIL(c, SD_ERR_ARG, "unknown metric %d (SD_METRIC_EUCLIDEAN, SD_METRIC_COSINE)", metric);
    if (metric == SD_METRIC_COSINE && (method == SD_LINKAGE_CENTROID || method == SD_LINKAGE_MEDIAN || method == SD_LINKAGE_WARD))
        SD_FAIL(c, SD_ERR_ARG, "centroid, median and ward linkage are defined for the euclidean metric only");
    return SD_OK;
}

extern "C" int sd_linkage_ex(sd_ctx* c, const double* h_X, int64_t N, int d, int method, int metric, double* h_Z);
extern "C" int sd_linkage(sd_ctx* c, const double* h_X, int64_t N, int d, double* h_Z)
{
    return sd_linkage_ex(c, h_X, N, d, SD_LINKAGE_CENTROID, SD_METRIC_EUCLIDEAN, h_Z);
}
extern "C" int sd_linkage_ex(sd_ctx* c, const double* h_X, int64_t N, int d, int method, int metric, double* h_Z)
{
    ENTER(c);
    if (!h_X || !h_Z || N < 2 || d <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_linkage: need N >= 2");
    if (int rc = check_method_metric(c, method, metric)) return rc;
    DTMP(c, dx, N * d * sizeof(double)); DTMP(c, dz, (N - 1) * 4 * sizeof(double));
    HIPCHK(c, hipMemcpy(dx.p, h_X, N * d * sizeof(double), hipMemcpyHostToDevice));
    int rc = run_linkage(c, (const double*)dx.p, N, d, (double*)dz.p, method, metric);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_Z, dz.p, (N - 1) * 4 * sizeof(double), hipMemcpyDeviceToHost));
    return SD_OK;
}

extern "C" int sd_cluster_ex(sd_ctx* c, const double* h_X, int64_t N, int d, int method, int metric, double cutoff, int32_t* h_labels1);
extern "C" int sd_cluster(sd_ctx* c, const double* h_X, int64_t N, int d, double cutoff, int32_t* h_labels1)
{
    return sd_cluster_ex(c, h_X, N, d, SD_LINKAGE_CENTROID, SD_METRIC_EUCLIDEAN, cutoff, h_labels1);
}
extern "C" int sd_cluster_ex(sd_ctx* c, const double* h_X, int64_t N, int d, int method, int metric, double cutoff, int32_t* h_labels1)
{
    ENTER(c);
    if (!h_X || !h_labels1 || N < 1 || d <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_cluster: bad argument");
    if (int rc = check_method_metric(c, method, metric)) return rc;
    DTMP(c, dx, N * d * sizeof(double));
    HIPCHK(c, hipMemcpy(dx.p, h_X, N * d * sizeof(double), hipMemcpyHostToDevice));
    std::vector<double> Z; std::vector<int> lab;
    if (int rc = run_linkage_host(c, (const double*)dx.p, N, d, method, metric, Z)) return rc;
    fcluster_host(Z, N, cutoff, lab);
    for (int64_t i = 0; i < N; ++i) h_labels1[i] = lab[(size_t)i];
    return SD_OK;
}

// Clustering::fcluster (cl.h:9-10, cl.cpp:442-457; criterion "distance"): Z [N-1][4] of N observations -> 1-based labels [N].  Host
// arithmetic only (O(N) pointer chasing over a dendrogram the caller already holds): no GPU work, c may be NULL.
extern "C" int sd_fcluster(sd_ctx* c, const double* h_Z, int64_t N, double cutoff, int32_t* h_labels1)
{
    if (c) c->err.clear();
    auto fail = [&](const char* m) { if (c) c->err = m; return (int)SD_ERR_ARG; };
    if (!h_labels1 || N < 1 || (N > 1 && !h_Z)) return fail("sd_fcluster: bad argument");
    // a dendrogram of N leaves: merge k joins two DIFFERENT nodes < N + k, each node at most once (the reference indexes arrays with them unchecked)
    std::vector<char> used((size_t)(2 * N - 1), 0);
    for (int64_t k = 0; k + 1 < N; ++k)
        for (int q = 0; q < 2; ++q) {
            const double v = h_Z[k * 4 + q];
            if (!(v >= 0.0) || v >= (double)(N + k) || v != std::floor(v) || used[(size_t)v]) return fail("sd_fcluster: Z is not a dendrogram of N observations");
            used[(size_t)v] = 1;
        }
    std::vector<double> Z(h_Z, h_Z + (size_t)(N > 1 ? N - 1 : 0) * 4);
    std::vector<int> T;
    fcluster_host(Z, N, cutoff, T);
    for (int64_t i = 0; i < N; ++i) h_labels1[i] = T[(size_t)i];
    return SD_OK;
}

extern "C" int sd_clustering_ex(sd_ctx* c, const double* h_emb, int64_t chunks, int d, int num_clusters, int min_clusters, int max_clusters,
                                int32_t* h_hard, int32_t* n_clusters);
extern "C" int sd_clustering(sd_ctx* c, const double* h_emb, int64_t chunks, int d, int32_t* h_hard, int32_t* n_clusters)
{
    return sd_clustering_ex(c, h_emb, chunks, d, -1, -1, -1, h_hard, n_clusters);
}
extern "C" int sd_clustering_ex(sd_ctx* c, const double* h_emb, int64_t chunks, int d, int num_clusters, int min_clusters, int max_clusters,
                                int32_t* h_hard, int32_t* n_clusters)
{
    ENTER(c);
    if (!h_emb || !h_hard || chunks <= 0 || d <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_clustering: bad argument");
    const int64_t M = chunks * SD_SPEAKERS;
    DTMP(c, de, M * d * sizeof(double));
    HIPCHK(c, hipMemcpy(de.p, h_emb, M * d * sizeof(double), hipMemcpyHostToDevice));
    std::vector<int> hard; int K = 1;
    int rc = run_clustering(c, (const double*)de.p, M, d, hard, &K, num_clusters, min_clusters, max_clusters);
    if (rc) return rc;
    for (int64_t i = 0; i < M; ++i) h_hard[i] = hard[(size_t)i];
    if (n_clusters) *n_clusters = K;
    return SD_OK;
}

int turns_out(sd_ctx* c, const std::vector<sd_turn>& v, sd_turn** turns, int64_t* n_turns)
{
    sd_turn* t = (sd_turn*)malloc(sizeof(sd_turn) * (v.size() ? v.size() : 1));
    if (!t) SD_FAIL(c, SD_ERR_ARG, "out of host memory");
    for (size_t i = 0; i < v.size(); ++i) t[i] = v[i];
    *turns = t; *n_turns = (int64_t)v.size();
    return SD_OK;
}

// ------------------------------------------------------------------ a15-a17
extern "C" int sd_reconstruct(sd_ctx* c, const float* h_seg, const uint8_t* h_bin, const int32_t* h_hard, const int32_t* h_count,
                              int64_t n_count, int64_t chunks, int64_t n_samples, sd_turn** turns, int64_t* n_turns)
{
    ENTER(c);
    if (!h_seg || !h_bin || !h_hard || !h_count || !turns || !n_turns || chunks <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_reconstruct: bad argument");
    const int64_t ne = chunks * SD_FRAMES * 3;
    std::vector<int> hard((size_t)chunks * 3);
    int K = 0;
    for (int64_t i = 0; i < chunks; ++i)
        for (int k = 0; k < 3; ++k) {
            int s = 0;
            for (int f = 0; f < SD_FRAMES; ++f) s += h_bin[(i * SD_FRAMES + f) * 3 + k];
            int h = h_hard[i * 3 + k];
            if (s == 0) h = -2;
            hard[(size_t)(i * 3 + k)] = h;
            if (h > K) K = h;
        }
    K += 1;                                                                   // sd.cpp:2803-2812
    DTMP(c, ds, ne * sizeof(float)); DTMP(c, dh, chunks * 3 * sizeof(int)); DTMP(c, dc, (n_count > 0 ? n_count : 1) * sizeof(int32_t));
    HIPCHK(c, hipMemcpy(ds.p, h_seg, ne * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dh.p, hard.data(), chunks * 3 * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dc.p, h_count, n_count * sizeof(int32_t), hipMemcpyHostToDevice));
    std::vector<sd_turn> v;
    int rc = run_reconstruct(c, (const float*)ds.p, nullptr, (const int*)dh.p, (const int32_t*)dc.p, n_count, chunks, n_samples, K, v);
    if (rc) return rc;
    return turns_out(c, v, turns, n_turns);
}

// ------------------------------------------------------------------ sharded inference + finalize
int pcm_to_wav(sd_ctx* c, const int16_t* d_pcm, int64_t n, DevWav* out)
{
    WS(c, float, w, "wav_f32", n + SD_WAV_PAD);
    hipLaunchKernelGGL(k_pcm_to_f32, GRID1(n + SD_WAV_PAD), 0, c->stream, d_pcm, w, n);
    KCHECK(c);
    *out = DevWav{w, n, 0, true};
    return SD_OK;
}

// host floats already divided by 32768 (sd.cpp:2948-2951)
int f32_to_wav(sd_ctx* c, const float* h_wav, int64_t n, DevWav* out)
{
    WS(c, float, w, "wav_f32", n + SD_WAV_PAD);
    HIPCHK(c, hipMemcpyAsync(w, h_wav, (size_t)n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + n, 0, SD_WAV_PAD * sizeof(float), c->stream));
    *out = DevWav{w, n, 0, true};
    return SD_OK;
}

// planted workload (sd_set_planted): chunks [pa, pb) of the scores of chunks [lo, hi) are taken from the caller's buffer
static int plant_scores(sd_ctx* c, int64_t lo, int64_t hi, float* d_seg)
{
    const int64_t pa = std::max(lo, c->planted_lo), pb = std::min(hi, c->planted_lo + c->planted_n);
    if (pb > pa && c->planted_scores)
        HIPCHK(c, hipMemcpyAsync(d_seg + (size_t)(pa - lo) * SD_FRAMES * 3, c->planted_scores + (size_t)(pa - c->planted_lo) * SD_FRAMES * 3,
                                 (size_t)(pb - pa) * SD_FRAMES * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    return SD_OK;
}

// seg_done: d_seg already holds the scores of chunks [lo, hi) (stream.hip computes those of a small pending batch itself, on the kernels the whole
// path takes for them); everything behind the segmentation step is the same
int shard_infer(sd_ctx* c, const DevWav& w, int64_t lo, int64_t hi, float* d_seg, float* d_emb, bool seg_done)
{
    const int64_t nc = hi - lo;
    c->stash.infer_items = nc > 0 ? nc * SD_SPEAKERS : 0;
    if (nc <= 0) return SD_OK;
    if ((lo * SD_SPEAKERS) % SD_EMB_BATCH != 0) SD_FAIL(c, SD_ERR_ARG, "shard start %lld must be a multiple of 32 chunks", (long long)lo);
    int rc;
    const double t0 = now_ms();
    if (!seg_done && (rc = run_segment(c, w, lo, hi, d_seg))) return rc;
    if ((rc = plant_scores(c, lo, hi, d_seg))) return rc;
    const int64_t pa = std::max(lo, c->planted_lo), pb = std::min(hi, c->planted_lo + c->planted_n);
    WS(c, float, d_masks, "sh_masks", nc * 3 * SD_FRAMES);
    if ((rc = run_postseg(c, d_seg, nc, nullptr, d_masks, nullptr))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t1 = now_ms();
    c->stage_ms[0] += t1 - t0;
    if ((rc = run_embed(c, w, d_masks, nc * 3, lo * 3, d_emb))) return rc;
    if (pb > pa && c->planted_emb) {
        hipLaunchKernelGGL(k_plant_emb, dim3((unsigned)((pb - pa) * 3)), dim3(SD_EMB_DIM), 0, c->stream,
                           d_emb + (size_t)(pa - lo) * 3 * SD_EMB_DIM, c->planted_emb + (size_t)(pa - c->planted_lo) * 3 * SD_EMB_DIM);
        KCHECK(c);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[1] += now_ms() - t1;
    return SD_OK;
}

// per-turn confidence: mean soft score (2 - cosine distance to the centroid, sd.cpp:2191-2207) of the
// (chunk, local speaker) items assigned to the turn's cluster whose 5 s chunk [0.5 c, 0.5 c + 5) overlaps the turn
void turn_confidence(const std::vector<sd_turn>& v, const std::vector<int>& hard, const std::vector<double>& soft_best, int64_t chunks, std::vector<double>& conf)
{
    conf.assign(v.size(), NAN);
    for (size_t t = 0; t < v.size(); ++t) {
        int64_t c0 = (int64_t)std::floor((v[t].start - 5.0) / 0.5), c1 = (int64_t)std::ceil(v[t].end / 0.5);
        if (c0 < 0) c0 = 0;
        if (c1 > chunks - 1) c1 = chunks - 1;
        double sum = 0.0; int64_t cnt = 0;
        for (int64_t ck = c0; ck <= c1; ++ck) {
            if (!(0.5 * (double)ck < v[t].end && 0.5 * (double)ck + 5.0 > v[t].start)) continue;
            for (int s = 0; s < SD_SPEAKERS; ++s) {
                const size_t i = (size_t)(ck * SD_SPEAKERS + s);
                if (hard[i] == v[t].label && soft_best[i] == soft_best[i]) { sum += soft_best[i]; cnt++; }
            }
        }
        if (cnt > 0) conf[t] = sum / (double)cnt;
    }
}

int finalize_front(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, uint8_t* d_bin, int* d_nact, int32_t* d_count, double* d_count_avg, double* d_e64)
{
    const int64_t M = chunks * SD_SPEAKERS;
    int rc;
    if ((rc = run_postseg(c, d_seg, chunks, d_bin, nullptr, d_nact))) return rc;
    if ((rc = run_count(c, d_bin, chunks, d_count, count_frames_host(chunks), d_count_avg))) return rc;
    return launch_f32_to_f64(c, d_emb, d_e64, M * SD_EMB_DIM);
}

int finalize(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, std::vector<sd_turn>& v)
{
    int rc;
    if ((rc = enrolled_refusal(c, SD_EMB_DIM, c->num_clusters, c->min_clusters, c->max_clusters))) return rc;      // before anything is touched
    const double t0 = now_ms();
    const int64_t M = chunks * SD_SPEAKERS;
    const int64_t nf = count_frames_host(chunks);
    WS(c, uint8_t, d_bin, "fin_bin", chunks * SD_FRAMES * 3);
    WS(c, int, d_nact, "fin_nact", M);
    WS(c, int32_t, d_count, "fin_count", nf);
    WS(c, double, d_e64, "fin_e64", M * SD_EMB_DIM);
    WS(c, int, d_hard, "fin_hard", M);
    double* d_count_avg = nullptr;
    if (!c->dump_dir.empty()) { WS(c, double, t_avg, "fin_count_avg", nf); d_count_avg = t_avg; }
    if ((rc = finalize_front(c, d_seg, d_emb, chunks, d_bin, d_nact, d_count, d_count_avg, d_e64))) return rc;
    std::vector<int> hard; int K = 1;
    std::vector<double> soft_best;
    if ((rc = run_clustering(c, d_e64, M, SD_EMB_DIM, hard, &K, c->num_clusters, c->min_clusters, c->max_clusters, &soft_best))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_hard, hard.data(), (size_t)M * sizeof(int), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch_mark_inactive(c, d_hard, d_nact, M))) return rc;
    HIPCHK(c, hipMemcpyAsync(hard.data(), d_hard, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int Kr = 0;
    for (int h : hard) if (h > Kr) Kr = h;
    Kr += 1;                                                                  // sd.cpp:2803-2812
    if ((rc = run_reconstruct(c, d_seg, d_nact, d_hard, d_count, nf, chunks, n, Kr, v))) return rc;
    if (!c->dump_dir.empty()) {
        rc = write_step_dumps(c, d_seg, d_emb, chunks, n, hard, Kr);
        c->stash.infer_items = 0;            // the per-batch files describe the inference that led to THIS finalize only
        if (rc) return rc;
    }
    { KernelStat& ks = c->stats["clusters_K"]; ks.launches++; ks.flops += (double)Kr; ks.bytes += (double)v.size(); }       // bench: K and turns per job
    turn_confidence(v, hard, soft_best, chunks, c->last.conf);
    c->last.hard.assign(hard.begin(), hard.end());      // the rows of a roster update (roster.h)
    c->stage_ms[2] += now_ms() - t0;
    return SD_OK;
}

extern "C" int sd_shard_infer_dev(sd_ctx* c, const int16_t* d_pcm_shard, int64_t first_sample, int64_t shard_samples, int64_t n,
                                  int64_t chunk_lo, int64_t chunk_hi, float* d_seg, float* d_emb)
{
    ENTER(c);
    if (!d_pcm_shard || !d_seg || !d_emb || n <= 1 || shard_samples <= 0 || first_sample < 0) SD_FAIL(c, SD_ERR_ARG, "sd_shard_infer_dev: bad argument");
    const int64_t need_lo = chunk_lo * SD_HOP;
    int64_t need_hi = (chunk_hi - 1) * SD_HOP + SD_CHUNK; if (need_hi > n) need_hi = n;
    if (chunk_hi > chunk_lo && (first_sample > need_lo || first_sample + shard_samples < need_hi))
        SD_FAIL(c, SD_ERR_ARG, "shard samples [%lld,%lld) do not cover chunks [%lld,%lld)", (long long)first_sample, (long long)(first_sample + shard_samples), (long long)chunk_lo, (long long)chunk_hi);
    DevWav w;
    if (int rc = pcm_to_wav(c, d_pcm_shard, shard_samples, &w)) return rc;
    clear_stage_ms(c);
    w.n = n; w.origin = first_sample;             // a slice of the recording: kernels index it with absolute sample positions
    return shard_infer(c, w, chunk_lo, chunk_hi, d_seg, d_emb);
}

extern "C" int sd_finalize_dev(sd_ctx* c, const float* d_seg, const float* d_emb, int64_t chunks, int64_t n, sd_turn** turns, int64_t* n_turns)
{
    ENTER(c);
    if (!d_seg || !d_emb || !turns || !n_turns || chunks <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_finalize_dev: bad argument");
    std::vector<sd_turn> v;
    c->stage_ms[2] = 0;                      // per call: a rank that only finalizes never passes through sd_shard_infer_dev
    int rc = finalize(c, d_seg, d_emb, chunks, n, v);
    if (rc) return rc;
    return turns_out(c, v, turns, n_turns);
}

extern "C" int sd_set_planted(sd_ctx* c, const float* d_scores, const float* d_emb, int64_t chunk_lo, int64_t chunks)
{
    if (!c || chunk_lo < 0 || chunks < 0) return SD_ERR_ARG;
    c->planted_scores = chunks > 0 ? d_scores : nullptr;
    c->planted_emb = chunks > 0 ? d_emb : nullptr;
    c->planted_lo = chunk_lo; c->planted_n = (d_scores || d_emb) ? chunks : 0;
    return SD_OK;
}

// ------------------------------------------------------------------ the whole-path entries: sd_diarize*, sd_activity* and sd_voiceprint*
// Each family has one body for its four entries (device pcm, host pcm, host f32, wav file): ENTER, the argument checks, bring() -- the source becomes a
// padded DevWav and t0, the start of what stage_ms[3] covers -- and the family's tail, called directly: diarize_wav_dev and activity_wav_dev fill a turn
// vector that turns_out hands over, voiceprint_wav_dev has no turns.  No entry calls another entry.
struct Source {
    enum Form { DevPcm, HostPcm, HostF32, WavFile } form;
    const void* in;                  // d_pcm, h_pcm, h_wav or the path
    int64_t n; int flags;            // samples of the first three forms; SD_WAV_* of a file
};

// What bring() leaves: the device samples and t0, and the scratch that must live until the entry returns -- the upload of host pcm (a per-call hipMalloc
// and a synchronous hipMemcpy inside the call, freed behind the networks: no implicit synchronisation in front of them) and the samples of a wav file
// (f32_to_wav and the resampler's upload copy from them asynchronously)
struct Brought { DevWav w; double t0 = 0; DevTmp pcm; WavLoad file; };

// t0 and clear_stage_ms: device pcm and host pcm once the device samples exist (the upload of host pcm is outside stage_ms[3]), host f32 before the upload,
// a wav file as the form it resolves to -- the resampled one after the file is read, before the upload of the off-rate samples
static int bring(sd_ctx* c, const Source& s, const char* who, Brought& b)
{
    switch (s.form) {
    case Source::DevPcm:             // n <= 0 is this form's only guard on n: nothing is uploaded from a count that is not one
        if (s.n <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)s.n);
        b.t0 = now_ms();
        clear_stage_ms(c);
        return pcm_to_wav(c, (const int16_t*)s.in, s.n, &b.w);
    case Source::HostPcm:
        if (s.n <= 0) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
        if (b.pcm.alloc(s.n * sizeof(int16_t))) SD_FAIL(c, SD_ERR_HIP, "hipMalloc(%zu) failed", (size_t)s.n * sizeof(int16_t));
        HIPCHK(c, hipMemcpy(b.pcm.p, s.in, s.n * sizeof(int16_t), hipMemcpyHostToDevice));
        return bring(c, Source{Source::DevPcm, b.pcm.p, s.n, 0}, who, b);
    case Source::HostF32:            // 8 / 32-bit wavs: samples already divided by 32768 exactly as the reference's loop does for every bit depth (sd.cpp:2948-2951)
        if (s.n <= 0) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
        b.t0 = now_ms();
        clear_stage_ms(c);
        return f32_to_wav(c, (const float*)s.in, s.n, &b.w);
    case Source::WavFile: break;
    }
    // a wav file: wav_file.h reads it and applies the rate / channel rule; the resampling is done here, on the device
    const char* path = (const char*)s.in;
    WavLoad& f = b.file;
    wav_load(path, s.flags, f);
    if (f.refused()) SD_FAIL(c, f.kind == WavLoad::NO_SAMPLES ? SD_ERR_SHORT : SD_ERR_ARG, "%s", f.refusal(path).c_str());
    if (f.kind == WavLoad::PCM16) return bring(c, Source{Source::HostPcm, f.pcm, f.n, 0}, who, b);
    if (f.kind == WavLoad::F32) return bring(c, Source{Source::HostF32, f.f32, f.n, 0}, who, b);
    b.t0 = now_ms();
    const int64_t no = sd_resample_len(f.n, f.sr, 16000);
    if (no <= 0) SD_FAIL(c, SD_ERR_SHORT, "%s: %lld samples at %d Hz give no 16 kHz sample", path, (long long)f.n, f.sr);
    clear_stage_ms(c);
    WS(c, float, d_in, "rs_in", f.n);
    WS(c, float, d_wav, "wav_f32", no + SD_WAV_PAD);
    HIPCHK(c, hipMemcpyAsync(d_in, f.f32, (size_t)f.n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(d_wav + no, 0, SD_WAV_PAD * sizeof(float), c->stream));
    b.w = DevWav{d_wav, no, 0, true};
    return resample_dev(c, d_in, f.n, f.sr, 16000, d_wav, no);
}

// What every family refuses on the source, its other arguments and the flags of a file alone (SD_ERR_ARG), in the order and the words the forms have:
// rest_ok = the family's own arguments are fine, hint = its remark on them
static int check_args(sd_ctx* c, const Source& s, bool rest_ok, const char* who, const char* hint = "")
{
    if (s.form == Source::HostPcm && (!s.in || s.n <= 0)) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
    if (!s.in || !rest_ok) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument%s", who, hint);
    if (s.form == Source::WavFile && (s.flags & ~(SD_WAV_RESAMPLE | SD_WAV_DOWNMIX | SD_WAV_ASSUME_16K))) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
    return SD_OK;
}
// a wav entry that fails behind its argument checks leaves an empty list
static void no_turns_yet(const Source& s, sd_turn** turns, int64_t* n_turns) { if (s.form == Source::WavFile) { *turns = nullptr; *n_turns = 0; } }

// chunks, both networks, finalize -> turns
static int diarize_wav_dev(sd_ctx* c, const DevWav& w, double t0, std::vector<sd_turn>& v)
{
    const int64_t chunks = sd_num_chunks(w.n, nullptr);
    if (chunks <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)w.n);
    WS(c, float, d_seg, "dz_seg", chunks * SD_FRAMES * 3);
    WS(c, float, d_emb, "dz_emb", chunks * 3 * SD_EMB_DIM);
    int rc;
    if ((rc = shard_infer(c, w, 0, chunks, d_seg, d_emb))) return rc;
    if ((rc = finalize(c, d_seg, d_emb, chunks, w.n, v))) return rc;
    c->stage_ms[3] = now_ms() - t0;
    if (getenv("SD_TRACE_WS")) {
        fprintf(stderr, "[sdhip] job %.1f ms (segmentation %.1f, embedding %.1f, finalize %.1f); workspace allocations so far in this process: %zu hipMalloc, %.2f GB, %.1f ms (+ %.1f ms hipFree)\n",
                c->stage_ms[3], c->stage_ms[0], c->stage_ms[1], c->stage_ms[2], g_ws_allocs.load(), (double)g_ws_alloc_bytes.load() / 1e9, (double)g_ws_alloc_us.load() * 1e-3, (double)g_ws_free_us.load() * 1e-3);
        for (const auto& kv : c->ws) if (kv.second.cap >= ((size_t)256 << 20)) fprintf(stderr, "[sdhip]   %-16s %8.2f GB\n", kv.first.c_str(), (double)kv.second.cap / 1e9);
    }
    return SD_OK;
}

static int diarize_from(sd_ctx* c, const Source& s, const char* who, sd_turn** turns, int64_t* n_turns)
{
    ENTER(c);
    int rc;
    if ((rc = check_args(c, s, turns && n_turns, who))) return rc;
    no_turns_yet(s, turns, n_turns);
    Brought b;
    std::vector<sd_turn> v;
    if ((rc = bring(c, s, who, b)) || (rc = diarize_wav_dev(c, b.w, b.t0, v))) return rc;
    return turns_out(c, v, turns, n_turns);
}

extern "C" int sd_diarize_dev(sd_ctx* c, const int16_t* d_pcm, int64_t n, sd_turn** turns, int64_t* n_turns)
{
    return diarize_from(c, Source{Source::DevPcm, d_pcm, n, 0}, "sd_diarize_dev", turns, n_turns);
}
extern "C" int sd_diarize(sd_ctx* c, const int16_t* h_pcm, int64_t n, sd_turn** turns, int64_t* n_turns)
{
    return diarize_from(c, Source{Source::HostPcm, h_pcm, n, 0}, "sd_diarize", turns, n_turns);
}
extern "C" int sd_diarize_f32(sd_ctx* c, const float* h_wav, int64_t n, sd_turn** turns, int64_t* n_turns)
{
    return diarize_from(c, Source{Source::HostF32, h_wav, n, 0}, "sd_diarize_f32", turns, n_turns);
}
extern "C" int sd_diarize_wav(sd_ctx* c, const char* path, int flags, sd_turn** turns, int64_t* n_turns)
{
    return diarize_from(c, Source{Source::WavFile, path, 0, flags}, "sd_diarize_wav", turns, n_turns);
}

// ------------------------------------------------------------------ a cut object from samples (cut.hip): chunks, both networks, then everything of a
// finalize in front of the cut of the dendrogram.  stage_ms[0], [1] = the inference, [3] = the time since t0
static int cut_wav_dev(sd_ctx* c, const DevWav& w, double t0, sd_cut** cut)
{
    const int64_t chunks = sd_num_chunks(w.n, nullptr);
    if (chunks <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)w.n);
    WS(c, float, d_seg, "dz_seg", chunks * SD_FRAMES * 3);
    WS(c, float, d_emb, "dz_emb", chunks * 3 * SD_EMB_DIM);
    int rc;
    if ((rc = shard_infer(c, w, 0, chunks, d_seg, d_emb))) return rc;
    if ((rc = cut_open_dev(c, d_seg, d_emb, chunks, w.n, cut))) return rc;
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

static int cut_from(sd_ctx* c, const Source& s, const char* who, sd_cut** cut)
{
    ENTER(c);
    int rc;
    if ((rc = check_args(c, s, cut != nullptr, who))) return rc;
    *cut = nullptr;
    if ((rc = cut_refusal(c, who))) return rc;                   // before anything is touched
    Brought b;
    if ((rc = bring(c, s, who, b))) return rc;
    return cut_wav_dev(c, b.w, b.t0, cut);
}

extern "C" int sd_cut_open_pcm_dev(sd_ctx* c, const int16_t* d_pcm, int64_t n, sd_cut** cut)
{
    return cut_from(c, Source{Source::DevPcm, d_pcm, n, 0}, "sd_cut_open_pcm_dev", cut);
}
extern "C" int sd_cut_open(sd_ctx* c, const int16_t* h_pcm, int64_t n, sd_cut** cut)
{
    return cut_from(c, Source{Source::HostPcm, h_pcm, n, 0}, "sd_cut_open", cut);
}
extern "C" int sd_cut_open_f32(sd_ctx* c, const float* h_wav, int64_t n, sd_cut** cut)
{
    return cut_from(c, Source{Source::HostF32, h_wav, n, 0}, "sd_cut_open_f32", cut);
}
extern "C" int sd_cut_open_wav(sd_ctx* c, const char* path, int flags, sd_cut** cut)
{
    return cut_from(c, Source{Source::WavFile, path, 0, flags}, "sd_cut_open_wav", cut);
}

// ------------------------------------------------------------------ speech / overlapped-speech regions (activity.hip)
// the stage alone: scores [chunks][293][3] -> the aggregated timeline of all its frames (sd.cpp:1167-1311)
extern "C" int sd_activity_scores(sd_ctx* c, const float* h_seg, int64_t chunks, int kind, double* h_scores, int64_t cap, int64_t* n_frames)
{
    ENTER(c);
    if (chunks <= 0 || (kind != SD_ACTIVITY_SPEECH && kind != SD_ACTIVITY_OVERLAP)) SD_FAIL(c, SD_ERR_ARG, "sd_activity_scores: bad argument (kind = SD_ACTIVITY_SPEECH or SD_ACTIVITY_OVERLAP)");
    const int64_t nf = activity_frames_host(chunks);
    if (n_frames) *n_frames = nf;
    if (!h_scores) return SD_OK;
    if (!h_seg) SD_FAIL(c, SD_ERR_ARG, "sd_activity_scores: bad argument");
    if (cap < nf) SD_FAIL(c, SD_ERR_ARG, "sd_activity_scores: capacity %lld < %lld", (long long)cap, (long long)nf);
    const int64_t ne = chunks * SD_FRAMES * 3;
    DTMP(c, ds, ne * sizeof(float)); DTMP(c, dsc, nf * sizeof(double));
    HIPCHK(c, hipMemcpy(ds.p, h_seg, ne * sizeof(float), hipMemcpyHostToDevice));
    if (int rc = run_activity_scores(c, (const float*)ds.p, chunks, kind, (double*)dsc.p, nf)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_scores, dsc.p, nf * sizeof(double), hipMemcpyDeviceToHost));
    return SD_OK;
}

// the stage alone: a timeline -> regions by the context's activity_onset / _offset / _min_duration_on / _min_duration_off (sd.cpp:2852-2935); label 0
extern "C" int sd_activity_regions(sd_ctx* c, const double* h_scores, int64_t n_frames, sd_turn** turns, int64_t* n_turns)
{
    ENTER(c);
    if (!h_scores || n_frames <= 0 || !turns || !n_turns) SD_FAIL(c, SD_ERR_ARG, "sd_activity_regions: bad argument");
    *turns = nullptr; *n_turns = 0;
    DTMP(c, dsc, n_frames * sizeof(double));
    HIPCHK(c, hipMemcpy(dsc.p, h_scores, n_frames * sizeof(double), hipMemcpyHostToDevice));
    std::vector<sd_turn> v;
    if (int rc = run_activity_regions(c, (const double*)dsc.p, n_frames, 0, v)) return rc;
    return turns_out(c, v, turns, n_turns);
}

// The tail of the sd_activity* entries: chunks, PyanNet, the activity stage -> turns labelled `kind`.  Nothing of the embedding, clustering or
// reconstruction stages runs.  stage_ms[0] = segmentation, [3] = the time since t0
static int activity_wav_dev(sd_ctx* c, const DevWav& w, int kind, double t0, std::vector<sd_turn>& v)
{
    c->last_activity.clear();
    const int64_t chunks = sd_num_chunks(w.n, nullptr);
    if (chunks <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)w.n);
    WS(c, float, d_seg, "dz_seg", chunks * SD_FRAMES * 3);
    int rc;
    const double t1 = now_ms();
    if ((rc = run_segment(c, w, 0, chunks, d_seg))) return rc;
    if ((rc = plant_scores(c, 0, chunks, d_seg))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[0] += now_ms() - t1;
    const int64_t nf = activity_frames_host(chunks), rows = activity_rows_host(nf, w.n);
    WS(c, double, d_scores, "act_scores", nf);
    if ((rc = run_activity_scores(c, d_seg, chunks, kind, d_scores, nf))) return rc;
    c->last_activity.resize((size_t)rows);
    HIPCHK(c, hipMemcpyAsync(c->last_activity.data(), d_scores, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if ((rc = run_activity_regions(c, d_scores, rows, kind, v))) return rc;      // (synchronises the stream)
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

static int activity_from(sd_ctx* c, const Source& s, int kind, const char* who, sd_turn** turns, int64_t* n_turns)
{
    ENTER(c);
    int rc;
    if ((rc = check_args(c, s, turns && n_turns && (kind == SD_ACTIVITY_SPEECH || kind == SD_ACTIVITY_OVERLAP), who, " (kind = SD_ACTIVITY_SPEECH or SD_ACTIVITY_OVERLAP)"))) return rc;
    no_turns_yet(s, turns, n_turns);
    Brought b;
    std::vector<sd_turn> v;
    if ((rc = bring(c, s, who, b)) || (rc = activity_wav_dev(c, b.w, kind, b.t0, v))) return rc;
    return turns_out(c, v, turns, n_turns);
}

extern "C" int sd_activity_dev(sd_ctx* c, const int16_t* d_pcm, int64_t n, int kind, sd_turn** turns, int64_t* n_turns)
{
    return activity_from(c, Source{Source::DevPcm, d_pcm, n, 0}, kind, "sd_activity_dev", turns, n_turns);
}
extern "C" int sd_activity(sd_ctx* c, const int16_t* h_pcm, int64_t n, int kind, sd_turn** turns, int64_t* n_turns)
{
    return activity_from(c, Source{Source::HostPcm, h_pcm, n, 0}, kind, "sd_activity", turns, n_turns);
}
extern "C" int sd_activity_f32(sd_ctx* c, const float* h_wav, int64_t n, int kind, sd_turn** turns, int64_t* n_turns)
{
    return activity_from(c, Source{Source::HostF32, h_wav, n, 0}, kind, "sd_activity_f32", turns, n_turns);
}
extern "C" int sd_activity_wav(sd_ctx* c, const char* path, int flags, int kind, sd_turn** turns, int64_t* n_turns)
{
    return activity_from(c, Source{Source::WavFile, path, 0, flags}, kind, "sd_activity_wav", turns, n_turns);
}

// ------------------------------------------------------------------ voiceprint of a speaker from regions of a recording (speakers.hip)
// the stage alone: spans -> the mask rows sd_voiceprint* hands to the embedding stage, [chunks * 3][293] with chunks = sd_num_chunks(n_samples)
extern "C" int sd_span_masks(sd_ctx* c, int64_t n_samples, const sd_turn* spans, int64_t n_spans, int32_t label, float* h_masks)
{
    ENTER(c);
    if (!h_masks || n_samples <= 0) SD_FAIL(c, SD_ERR_ARG, "sd_span_masks: bad argument");
    if (int rc = check_spans(c, spans, n_spans, "sd_span_masks")) return rc;
    const int64_t chunks = sd_num_chunks(n_samples, nullptr);
    if (chunks <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)n_samples);
    std::vector<int64_t> ss;
    spans_to_samples(spans, n_spans, label, n_samples, ss);
    const size_t bytes = (size_t)chunks * SD_SPEAKERS * SD_FRAMES * sizeof(float);
    DTMP(c, dm, bytes);
    if (int rc = run_span_masks(c, ss, chunks, n_samples, (float*)dm.p)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h_masks, dm.p, bytes, hipMemcpyDeviceToHost));
    return SD_OK;
}

// The tail of the sd_voiceprint* entries: chunks, span masks, the embedding stage over all items, the mean of the live rows 3c.  No segmentation
// network runs and nothing is clustered.  stage_ms[1] = the embedding stage, [3] = the time since t0
struct VoiceprintArgs { const sd_turn* spans; int64_t n_spans; int32_t label; double* h_emb; int64_t* n_windows; };
static int voiceprint_wav_dev(sd_ctx* c, const DevWav& w, const VoiceprintArgs& a, double t0)
{
    if (!c->ew.loaded) SD_FAIL(c, SD_ERR_MODEL, "embedding model not loaded");
    const int64_t chunks = sd_num_chunks(w.n, nullptr);
    if (chunks <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)w.n);
    std::vector<int64_t> ss;
    spans_to_samples(a.spans, a.n_spans, a.label, w.n, ss);
    const int64_t items = chunks * SD_SPEAKERS;
    WS(c, float, d_masks, "vp_masks", items * SD_FRAMES);
    WS(c, float, d_emb, "vp_emb", items * SD_EMB_DIM);
    int rc;
    const double t1 = now_ms();
    if ((rc = run_span_masks(c, ss, chunks, w.n, d_masks))) return rc;
    if ((rc = run_embed(c, w, d_masks, items, 0, d_emb))) return rc;
    double mean[SD_EMB_DIM];
    int64_t live = 0;
    if ((rc = run_voiceprint_mean(c, d_emb, chunks, mean, &live))) return rc;      // (synchronises the stream)
    c->stage_ms[1] += now_ms() - t1;
    c->stage_ms[3] = now_ms() - t0;
    if (a.n_windows) *a.n_windows = live;
    if (live <= 0) SD_FAIL(c, SD_ERR_SHORT, "no window of the recording holds 640 selected samples (sd.cpp:44): no voiceprint");
    memcpy(a.h_emb, mean, sizeof(mean));
    return SD_OK;
}

static int voiceprint_from(sd_ctx* c, const Source& s, const VoiceprintArgs& a, const char* who)
{
    ENTER(c);
    int rc;
    if ((rc = check_args(c, s, a.h_emb != nullptr, who)) || (rc = check_spans(c, a.spans, a.n_spans, who))) return rc;
    Brought b;
    if ((rc = bring(c, s, who, b))) return rc;
    return voiceprint_wav_dev(c, b.w, a, b.t0);
}

extern "C" int sd_voiceprint_dev(sd_ctx* c, const int16_t* d_pcm, int64_t n, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb, int64_t* n_windows)
{
    return voiceprint_from(c, Source{Source::DevPcm, d_pcm, n, 0}, VoiceprintArgs{spans, n_spans, label, h_emb, n_windows}, "sd_voiceprint_dev");
}
extern "C" int sd_voiceprint(sd_ctx* c, const int16_t* h_pcm, int64_t n, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb, int64_t* n_windows)
{
    return voiceprint_from(c, Source{Source::HostPcm, h_pcm, n, 0}, VoiceprintArgs{spans, n_spans, label, h_emb, n_windows}, "sd_voiceprint");
}
extern "C" int sd_voiceprint_f32(sd_ctx* c, const float* h_wav, int64_t n, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb, int64_t* n_windows)
{
    return voiceprint_from(c, Source{Source::HostF32, h_wav, n, 0}, VoiceprintArgs{spans, n_spans, label, h_emb, n_windows}, "sd_voiceprint_f32");
}
extern "C" int sd_voiceprint_wav(sd_ctx* c, const char* path, int flags, const sd_turn* spans, int64_t n_spans, int32_t label, double* h_emb, int64_t* n_windows)
{
    return voiceprint_from(c, Source{Source::WavFile, path, 0, flags}, VoiceprintArgs{spans, n_spans, label, h_emb, n_windows}, "sd_voiceprint_wav");
}
