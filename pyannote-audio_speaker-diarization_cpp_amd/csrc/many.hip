// many.hip -- sd_diarize_many*: many recordings in one call, both networks over one packed waveform, finalize per recording.
//
// Layout (many_plan.h): recording r gets a slot of roundup32(chunks_r + 9) chunks at chunk base B_r, sample base 8000 B_r, zeros behind its n_r
// samples.  Packed chunk B_r + k starts at the sample where chunk k of the recording alone starts, B_r * 3 is a multiple of 96 items, so the
// reference's embedding batches of 32 items (sd.cpp:2429) fall where they fall in the recording alone, and the 9+ chunks behind chunks_r are
// nobody's: their masks are zeroed, frontend_prepare drops their items as dead, finalize never sees their rows.
//   k_many_pack       one launch: the samples of every recording into its slot (16-bit: x 1/32768 as k_pcm_to_f32; f32: copied), zeros behind them
//   k_many_gap_masks  one launch: zero mask rows for the gap chunks of every slot
//   (sd_diarize_many_audio*: k_many_ingest, ingest.hip, fills the pack instead -- recordings in their own rate and encoding)
// Both walk a table indexed by recording; every store is guarded by the row's own slot length and by the length of the destination.
// pack_infer, the inference over a filled table, and finalize_jobs, the finalize per output, are shared with the group calls of stream.hip, whose slots
// hold ranges of streams.  A slot is a PackRange (many_plan.h) built by pack_range (stream_book.h): a recording is the pending range of a
// stream with nothing sealed.  Which side of PyanNet's skinny limit a chunk is on is seg_tile_chunks' word (many_plan.h), here and in stream.hip.
#include "common.h"
#include "stream_book.h"
#include "linkage_batch_plan.h"
#include "ingest_plan.h"
#include "resample_book.h"
#include <algorithm>
#include <utility>

// grid (x: a stride over the samples of a slot, y: a stride over the table), 256 threads
__global__ void k_many_pack(const ManyRow* __restrict__ rows, int R, int is_f32, float* __restrict__ dst, int64_t dst_len)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        const ManyRow row = rows[r];
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < row.len && row.base + i < dst_len; i += step) {
            float v = 0.0f;
            if (i < row.n) v = is_f32 ? ((const float*)row.src)[i] : pcm_to_float(((const int16_t*)row.src)[i]);
            dst[row.base + i] = v;
        }
    }
}

// masks [total_chunks * 3][293]; same grid shape
__global__ void k_many_gap_masks(const ManyGap* __restrict__ gaps, int G, float* __restrict__ masks, int64_t total_chunks)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x, per = (int64_t)SD_SPEAKERS * SD_FRAMES, all = total_chunks * per;
    for (int g = blockIdx.y; g < G; g += gridDim.y) {
        const ManyGap gap = gaps[g];
        const int64_t first = gap.first * per, cnt = gap.count * per;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt && first + i < all; i += step) masks[first + i] = 0.0f;
    }
}

dim3 many_grid(int64_t longest, int64_t table)
{
    const int64_t gx = std::min<int64_t>(std::max<int64_t>((longest + 255) / 256, 1), 2048), gy = std::min<int64_t>(std::max<int64_t>(table, 1), 1024);
    return dim3((unsigned)gx, (unsigned)gy);
}

// the two launches, for pack_infer and for the hooks of input_test.hip: the x stride covers the longest row (gap) of the table, the y stride the table
int launch_many_pack(sd_ctx* c, const ManyRow* d_rows, const std::vector<ManyRow>& rows, int is_f32, float* d_dst, int64_t dst_len)
{
    int64_t longest = 0;
    for (const ManyRow& r : rows) longest = std::max(longest, r.len);
    hipLaunchKernelGGL(k_many_pack, many_grid(longest, (int64_t)rows.size()), dim3(256), 0, c->stream, d_rows, (int)rows.size(), is_f32, d_dst, dst_len);
    KCHECK(c);
    return SD_OK;
}
int launch_many_gap_masks(sd_ctx* c, const ManyGap* d_gaps, const std::vector<ManyGap>& gaps, float* d_masks, int64_t total_chunks)
{
    int64_t longest_gap = 0;
    for (const ManyGap& g : gaps) longest_gap = std::max(longest_gap, g.count);
    hipLaunchKernelGGL(k_many_gap_masks, many_grid(longest_gap * SD_SPEAKERS * SD_FRAMES, (int64_t)gaps.size()), dim3(256), 0, c->stream, d_gaps, (int)gaps.size(),
                       d_masks, total_chunks);
    KCHECK(c);
    return SD_OK;
}

extern "C" int sd_many_plan(const int64_t* n, int64_t R, int64_t* chunk_base, int64_t* total_chunks)
{
    return many_plan(n, R, chunk_base, total_chunks) ? SD_ERR_ARG : SD_OK;
}

// ------------------------------------------------------------------ segmentation over the pack
// A full chunk of a recording reads samples of that recording only, and packed chunk B_r + k starts where chunk k starts: run_segment on the pack
// "as one recording" computes it from the same samples with the same kernels -- provided its batch is on the same side of the one threshold at
// which PyanNet's kernels change with the batch size: up to SD_SKINNY_CHUNKS = 13 chunks the dense layers take k_skinny_gemm, above that the
// 128 x 128 tile, and the two differ in the last bits (many_plan.h).  So the plan keeps, for every chunk, the side its batch has in the loop of
// single calls (batches of seg_batch_chunks from chunk 0 of the recording; q.tile = seg_tile_chunks):
//   tile side    chunks [0, T_r): ranges of neighbouring recordings are joined across the gap chunks between them (rows that nobody reads) and
//                run in shared batches of seg_batch_chunks, each of 14 chunks or more;
//   skinny side  chunks [T_r, full_r): the batches of the single path, one recording at a time (a batch of at most 13 chunks has no room for more);
//   short last chunk (sd.cpp:1457-1480): the single path's own call on a view of the slot -- its frame count depends on its length, and the shared
//                first convolution the single path takes for it is not the per-row form of run_segment_rows bit for bit (tests/test_next_rows.py)
#define MANY_JOIN_CHUNKS 256      /* tile ranges at most this far apart are one range: up to 4096 chunks are one wave of LSTM workgroups, a launch sequence more costs more */

// A slot of a stream's range (q.lo > 0, stream.hip) differs in two things.  Its tile side is what the caller says, and can be shorter than 14 chunks
// (1 .. 13 pending chunks behind sealed ones): such a range reaches FORWARD into the zero chunks of its own slot -- at least 19 of them -- and the
// rows it computes there are the slot's gap rows, or the row the short last chunk's own call writes afterwards.  And its short last chunk is chunk
// lo + chunks - 1 of a recording that holds samples from lo * 8000 on: the view says so, as the stream's own tail does.
static int many_segment(sd_ctx* c, const float* d_pack, int64_t total, const std::vector<PackRange>& rec, float* d_seg)
{
    const size_t row = (size_t)SD_FRAMES * 3;
    const int64_t cb = c->seg_batch_chunks < 1 ? 1 : c->seg_batch_chunks;
    const DevWav pack{d_pack, total * (int64_t)SD_HOP, 0, true};      // sd_num_chunks of it = total - 9 full chunks and no short one: every real chunk is among them
    std::vector<std::pair<int64_t, int64_t>> tile, skinny;
    for (const PackRange& q : rec) {
        if (q.chunks <= 0) continue;
        const int64_t T = q.tile;
        if (T > 0) {
            if (!tile.empty() && q.base - tile.back().second <= MANY_JOIN_CHUNKS) tile.back().second = q.base + T;
            else tile.emplace_back(q.base, q.base + T);
        }
        for (int64_t k = T; k < q.full; k += cb) skinny.emplace_back(q.base + k, q.base + std::min(q.full, k + cb));
    }
    int rc;
    for (const auto& t : tile)
        for (int64_t k = t.first; k < t.second; k += cb) {
            int64_t lo = k, hi = std::min(t.second, k + cb);
            if (hi - lo <= SD_SKINNY_CHUNKS) {
                if (hi - (SD_SKINNY_CHUNKS + 1) >= t.first) lo = hi - (SD_SKINNY_CHUNKS + 1);      // the rest of a range: reaches back into chunks already computed (same bits) to stay on the tile side
                else hi = lo + SD_SKINNY_CHUNKS + 1;                                                   // a range shorter than that: forward, into its slot's zero chunks
            }
            if (lo < 0 || hi > total - SD_MANY_GAP) SD_FAIL(c, SD_ERR_ARG, "packed segmentation batch [%lld,%lld) leaves the pack's %lld full chunks", (long long)lo, (long long)hi, (long long)(total - SD_MANY_GAP));
            if ((rc = run_segment(c, pack, lo, hi, d_seg + (size_t)lo * row))) return rc;
        }
    for (const auto& s : skinny)
        if ((rc = run_segment(c, pack, s.first, s.second, d_seg + (size_t)s.first * row))) return rc;
    for (const PackRange& q : rec) {
        if (q.chunks <= 0 || q.full == q.chunks) continue;
        const DevWav view{d_pack + q.base * (int64_t)SD_HOP, q.n + q.lo * (int64_t)SD_HOP, q.lo * (int64_t)SD_HOP, true};      // zeros up to the end of the slot, at least 8000 of them behind a short last chunk
        if ((rc = run_segment(c, view, q.hi() - 1, q.hi(), d_seg + (size_t)(q.base + q.chunks - 1) * row))) return rc;
    }
    return SD_OK;
}

// ------------------------------------------------------------------ both networks once over the pack (shard_infer's steps; the segmentation step is many_segment)
// The fill step is the caller's: it is handed `fill_bytes` of table workspace on the device (the gaps' table sits behind them), the pack and its length,
// uploads its table and launches the kernel that writes every slot and the SD_WAV_PAD floats behind the last one -- launch_many_pack for
// sd_diarize_many* and the stream group calls, launch_many_ingest for sd_diarize_many_audio*.  Everything behind it is the same code.
static int pack_infer_fill(sd_ctx* c, size_t fill_bytes, const std::function<int(char*, float*, int64_t)>& fill, const std::vector<PackRange>& rec, int64_t total, double t0,
                           float** seg_out, float** emb_out)
{
    std::vector<ManyGap> gaps;
    for (const PackRange& q : rec) {
        if (q.chunks <= 0) continue;
        gaps.push_back(ManyGap{q.base + q.chunks, q.slot() - q.chunks});
    }
    const int64_t pack_len = total * (int64_t)SD_HOP + SD_WAV_PAD;
    const size_t row_bytes = (fill_bytes + 15) / 16 * 16, gap_bytes = gaps.size() * sizeof(ManyGap);
    WS(c, float, d_pack, "many_wav", pack_len);
    WS(c, char, d_tab, "many_tab", row_bytes + gap_bytes);
    WS(c, float, d_seg, "many_seg", total * SD_FRAMES * 3);
    WS(c, float, d_masks, "many_masks", total * 3 * SD_FRAMES);
    WS(c, float, d_emb, "many_emb", total * 3 * SD_EMB_DIM);
    HIPCHK(c, hipMemcpy(d_tab + row_bytes, gaps.data(), gap_bytes, hipMemcpyHostToDevice));
    int rc;
    if ((rc = fill(d_tab, d_pack, pack_len))) return rc;

    HIPCHK(c, hipMemsetAsync(d_seg, 0, (size_t)total * SD_FRAMES * 3 * sizeof(float), c->stream));      // gap rows: defined values for run_postseg
    if ((rc = many_segment(c, d_pack, total, rec, d_seg))) return rc;
    if ((rc = run_postseg(c, d_seg, total, nullptr, d_masks, nullptr))) return rc;
    if ((rc = launch_many_gap_masks(c, (const ManyGap*)(d_tab + row_bytes), gaps, d_masks, total))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const double t1 = now_ms();
    c->stage_ms[0] = t1 - t0;
    // w.n is the packed length here.  The one place below run_embed that reads it, k_stft_fbank, clips a VALUE with it (a sample at or behind n reads
    // as 0.0f): behind n_r the pack holds the same +0.0f.  The sample COUNTS of an item come from its mask row alone (k_mask_prefix) in both paths
    if ((rc = run_embed(c, DevWav{d_pack, total * (int64_t)SD_HOP, 0, true}, d_masks, total * 3, 0, d_emb))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[1] = now_ms() - t1;
    *seg_out = d_seg; *emb_out = d_emb;
    return SD_OK;
}

int pack_infer(sd_ctx* c, std::vector<ManyRow>& rows, int is_f32, const std::vector<PackRange>& rec, int64_t total, double t0, float** seg_out, float** emb_out)
{
    rows.push_back(ManyRow{nullptr, 0, total * (int64_t)SD_HOP, SD_WAV_PAD});      // the zeroed floats behind the last slot (DevWav::padded)
    const size_t row_bytes = rows.size() * sizeof(ManyRow);
    return pack_infer_fill(c, row_bytes, [&](char* d_tab, float* d_pack, int64_t pack_len) -> int {
        HIPCHK(c, hipMemcpy(d_tab, rows.data(), row_bytes, hipMemcpyHostToDevice));
        return launch_many_pack(c, (const ManyRow*)d_tab, rows, is_f32, d_pack, pack_len);      // (a row is a slot, or the SD_WAV_PAD floats behind the last one)
    }, rec, total, t0, seg_out, emb_out);
}

// ------------------------------------------------------------------ the dendrograms of a group call, ahead of the per-job finalize
// The per-job finalize spends most of its time in a one-workgroup linkage (N < 1500 train rows) while the rest of the device waits; the jobs of one call are
// independent.  This pass forms, for every job, the rows cluster_rows would hand to the linkage -- with the kernels the finalize uses: k_f32_to_f64,
// train_rows (the "max_num_embeddings" sample included), k_gather_normalize -- and runs all dendrograms in shared launches (run_linkage_many).  Z[j] /
// ZN[j] (the train rows it belongs to; -1 = none) wait on the host for cluster_rows, which takes a Z only where it finds the same row count itself.
// Jobs that skip the pass and run their linkage where they always did: under an enrolled gallery (the linkage is over the unclaimed rows), a trivial
// number-of-clusters rule, fewer than two train rows, a job run_linkage_many would run alone -- neither the one-workgroup kernel's nor, under option
// linkage_batch_xcd, of the one-XCD cooperative class (linkage_job_shares_launches): nothing to gain, and its Z would be held for longer.  A job whose dendrogram fails with SD_ERR_NUMERIC keeps no Z: its finalize runs the linkage itself and reports what the sequential path reports.
static int dendrograms_ahead(sd_ctx* c, const std::vector<FinalJob>& jobs, std::vector<std::vector<double>>& Z, std::vector<int64_t>& ZN)
{
    const size_t J = jobs.size();
    Z.assign(J, std::vector<double>()); ZN.assign(J, -1);
    if (c->linkage_batch == 0 || c->enr_M > 0 || J < 2) return SD_OK;
    const double t0 = now_ms();
    const int d = SD_EMB_DIM;
    int64_t maxM = 0, pool = 0, live = 0;
    for (const FinalJob& q : jobs) {
        if (q.chunks <= 0) continue;
        const int64_t M = q.chunks * SD_SPEAKERS;
        maxM = std::max(maxM, M); pool += c->linkage_batch_xcd ? M : std::min<int64_t>(M, LINKAGE_HEAP_LDS + 1); live += 1;      // (a job of the one-XCD class has up to M train rows)
    }
    if (live < 2) return SD_OK;
    WS(c, double, d_e64, "lb_e64", maxM * d);
    WS(c, double, d_X, "lb_X", pool * d);
    const ClusterSpec spec = {c->clustering_threshold, c->min_cluster_size, c->num_clusters, c->min_clusters, c->max_clusters};
    std::vector<std::vector<int>> tidx(J);
    std::vector<LinkageManyJob> lj;
    std::vector<size_t> owner;
    int64_t off = 0;
    int rc;
    for (size_t j = 0; j < J; ++j) {
        const FinalJob& q = jobs[j];
        if (q.chunks <= 0) continue;
        const int64_t M = q.chunks * SD_SPEAKERS;
        if ((rc = launch_f32_to_f64(c, q.emb, d_e64, M * d))) return rc;
        if ((rc = train_rows(c, d_e64, M, d, tidx[j]))) return rc;
        const int64_t N = (int64_t)tidx[j].size();
        if (!linkage_job_shares_launches(c, N, c->clustering_method) || resolve_num_clusters(spec, N).trivial) continue;
        if ((rc = linkage_rows(c, d_e64, tidx[j], d, d_X + (size_t)off * d))) return rc;
        Z[j].resize((size_t)(N - 1) * 4);
        lj.push_back(LinkageManyJob{d_X + (size_t)off * d, N, Z[j].data()});
        owner.push_back(j);
        off += N;
    }
    if (lj.size() >= 2) {
        const int method = c->clustering_method;
        std::vector<int32_t> st(lj.size(), SD_OK);
        if ((rc = run_linkage_many(c, lj.data(), (int64_t)lj.size(), d, method, linkage_metric_of(method), st.data()))) return rc;
        for (size_t k = 0; k < lj.size(); ++k) if (st[k] == SD_OK) ZN[owner[k]] = lj[k].N;
    } else HIPCHK(c, hipStreamSynchronize(c->stream));      // one job alone gains nothing: its finalize runs the linkage (tidx of the last gather must outlive its upload)
    c->stage_ms[2] += now_ms() - t0;
    return SD_OK;
}

// ------------------------------------------------------------------ finalize per output (common.h)
int finalize_jobs(sd_ctx* c, int64_t J, sd_turn** turns, int64_t* n_turns, int32_t* status, const std::function<int(std::vector<FinalJob>&)>& infer,
                  const std::function<int(int64_t, sd_turn*, int64_t)>& named)
{
    c->many_jobs.assign((size_t)J, ManyJob());
    for (int64_t j = 0; j < J; ++j) { turns[j] = nullptr; n_turns[j] = 0; status[j] = SD_ERR_SHORT; c->many_jobs[(size_t)j].status = SD_ERR_SHORT; }
    std::vector<FinalJob> jobs((size_t)J, FinalJob{nullptr, nullptr, 0, 0});
    int rc;
    if ((rc = infer(jobs))) return rc;
    std::vector<std::vector<double>> Zs;
    std::vector<int64_t> ZN;
    if ((rc = dendrograms_ahead(c, jobs, Zs, ZN))) return rc;
    // one job after the other; what finalize leaves in the context is kept per job (sd_many_select)
    for (int64_t j = 0; j < J; ++j) {
        const FinalJob& q = jobs[(size_t)j];
        if (q.chunks <= 0) continue;
        std::vector<sd_turn> v;
        c->ahead_N = ZN[(size_t)j]; c->ahead_Z.swap(Zs[(size_t)j]);      // cluster_rows takes it where it finds the same train rows
        rc = finalize(c, q.seg, q.emb, q.chunks, q.n, v);
        c->ahead_N = -1; c->ahead_Z.clear();
        ManyJob& job = c->many_jobs[(size_t)j];
        status[j] = job.status = rc;
        if (rc == SD_ERR_NUMERIC) continue;                    // this job's clustering; the others go on
        if (rc == SD_OK) rc = turns_out(c, v, &turns[j], &n_turns[j]);
        if (rc == SD_OK && named) rc = named(j, turns[j], n_turns[j]);
        if (rc) {
            for (int64_t k = 0; k < J; ++k) { sd_free_turns(turns[k]); turns[k] = nullptr; n_turns[k] = 0; }
            return rc;
        }
        job.res = c->last;
    }
    return SD_OK;
}

// ------------------------------------------------------------------ the call
static int many_run(sd_ctx* c, const void* const* src, int form, const int64_t* n, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status, const char* who)
{
    // refusals: nothing is touched
    if (!src || !n || !turns || !n_turns || !status || R < 1) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument (R >= 1)", who);
    for (int64_t r = 0; r < R; ++r) if (!src[r]) SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld is a null pointer", who, (long long)r);
    if (!c->dump_dir.empty()) SD_FAIL(c, SD_ERR_ARG, "%s: a dump directory is set (the step files describe one recording)", who);
    if (c->planted_n > 0) SD_FAIL(c, SD_ERR_ARG, "%s: a planted workload is set (its chunk range means one recording)", who);
    std::vector<PackRange> rec((size_t)R);      // a recording without a chunk: chunks = 0, no slot, status SD_ERR_SHORT
    for (int64_t r = 0; r < R; ++r) { pack_range(n[r], 0, c->seg_batch_chunks, true, rec[(size_t)r]); rec[(size_t)r].owner = r; }
    int64_t total = 0;
    if (pack_plan(rec.data(), R, &total)) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument (at most 2^20 recordings of at most 2^40 samples)", who);
    if (total > SD_MANY_MAX_CHUNKS) SD_FAIL(c, SD_ERR_ARG, "%s: %lld packed chunks (limit %d: the rows of one call are counted in int)", who, (long long)total, SD_MANY_MAX_CHUNKS);
    int rc;
    if ((rc = enrolled_refusal(c, SD_EMB_DIM, c->num_clusters, c->min_clusters, c->max_clusters))) return rc;

    const double t0 = now_ms();
    clear_stage_ms(c);
    rc = finalize_jobs(c, R, turns, n_turns, status, [&](std::vector<FinalJob>& jobs) -> int {
        if (total <= 0) return SD_OK;
        std::vector<ManyRow> rows;
        int64_t src_samples = 0;
        for (const PackRange& q : rec) {
            if (q.chunks <= 0) continue;
            rows.push_back(ManyRow{src[q.owner], q.n, q.base * (int64_t)SD_HOP, q.slot() * (int64_t)SD_HOP});
            src_samples += q.n;
        }
        if (form != SD_PCM_DEV) {      // host rows: uploaded back to back, then packed like device rows
            const size_t es = form == SD_F32_HOST ? sizeof(float) : sizeof(int16_t);
            WS(c, char, d_src, "many_src", (size_t)src_samples * es);
            size_t off = 0;
            for (ManyRow& w : rows) {
                HIPCHK(c, hipMemcpyAsync(d_src + off, w.src, (size_t)w.n * es, hipMemcpyHostToDevice, c->stream));
                w.src = d_src + off;
                off += (size_t)w.n * es;
            }
        }
        float *d_seg = nullptr, *d_emb = nullptr;
        if (int e = pack_infer(c, rows, form == SD_F32_HOST ? 1 : 0, rec, total, t0, &d_seg, &d_emb)) return e;
        for (const PackRange& q : rec) jobs[(size_t)q.owner] = FinalJob{d_seg + (size_t)q.base * SD_FRAMES * 3, d_emb + (size_t)q.base * 3 * SD_EMB_DIM, q.chunks, q.n};
        return SD_OK;
    });
    if (rc) return rc;
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

extern "C" int sd_diarize_many(sd_ctx* c, const int16_t* const* h_pcm, const int64_t* n, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    ENTER(c);
    return many_run(c, (const void* const*)h_pcm, SD_PCM_HOST, n, R, turns, n_turns, status, "sd_diarize_many");
}

extern "C" int sd_diarize_many_dev(sd_ctx* c, const int16_t* const* d_pcm, const int64_t* n, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    ENTER(c);
    return many_run(c, (const void* const*)d_pcm, SD_PCM_DEV, n, R, turns, n_turns, status, "sd_diarize_many_dev");
}

extern "C" int sd_diarize_many_f32(sd_ctx* c, const float* const* h_wav, const int64_t* n, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    ENTER(c);
    return many_run(c, (const void* const*)h_wav, SD_F32_HOST, n, R, turns, n_turns, status, "sd_diarize_many_f32");
}

// ------------------------------------------------------------------ recordings in their own rate and encoding
// The second front of the pack: the slots are planned on len16 (ingest_plan.h), the sources go up as they are -- every one at a 16-byte aligned offset of
// one workspace, only the bytes the rule reads -- and ONE k_many_ingest launch (ingest.hip) decodes, picks or averages the channels, resamples and pads
// them into the pack.  The tap tables come from resample_taps, once per distinct rate of the call and before the launch; no k_resample* launch and no
// synchronisation stands in front of the pack.  Behind the fill it is pack_infer_fill and finalize_jobs, as for sd_diarize_many*.
static_assert(SD_TAIL_PAD == SD_WAV_PAD, "ingest_plan.h sizes the pad row by SD_TAIL_PAD");
static int many_audio_run(sd_ctx* c, const sd_audio* a, bool dev, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status, const char* who)
{
    // refusals: nothing is touched
    if (!a || !turns || !n_turns || !status || R < 1) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument (R >= 1)", who);
    if (!c->dump_dir.empty()) SD_FAIL(c, SD_ERR_ARG, "%s: a dump directory is set (the step files describe one recording)", who);
    if (c->planted_n > 0) SD_FAIL(c, SD_ERR_ARG, "%s: a planted workload is set (its chunk range means one recording)", who);
    IngestPlan plan;
    const int why = ingest_plan(a, R, c->seg_batch_chunks, true, plan);
    const long long bad = (long long)plan.bad;
    switch (why) {
    case INGEST_OK: break;
    case INGEST_BAD_DESC: SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld: bad descriptor (n >= 0, sample_rate > 0, an SD_ENC_* encoding, channels >= 1, channel in [-1, channels))", who, bad);
    case INGEST_NULL_DATA: SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld is a null pointer", who, bad);
    case INGEST_RATE_TABLE: {
        ResamplePlan p;
        const int rc = resample_check(c, a[plan.bad].sample_rate, SD_SAMPLE_RATE, p);      // its own message, the recording in front of it
        const std::string msg = c->err;
        SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld: %s", who, bad, rc ? msg.c_str() : "unsupported rate pair");
    }
    case INGEST_RATE_LDS: SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld: %d -> %d Hz: a tile's input span and its %d outputs do not fit the LDS", who, bad, a[plan.bad].sample_rate, SD_SAMPLE_RATE, RS_BLOCK);
    case INGEST_BYTES: SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld holds more than 2^42 bytes", who, bad);
    case INGEST_PACK_LIMITS:
        if (plan.bad >= 0) SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld: more than 2^40 samples at 16 kHz", who, bad);
        if (plan.total > SD_MANY_MAX_CHUNKS) SD_FAIL(c, SD_ERR_ARG, "%s: %lld packed chunks (limit %d: the rows of one call are counted in int)", who, (long long)plan.total, SD_MANY_MAX_CHUNKS);
        SD_FAIL(c, SD_ERR_ARG, "%s: bad argument (at most 2^20 recordings of at most 2^40 samples)", who);
    default: SD_FAIL(c, SD_ERR_ARG, "%s: the pack has too many tiles for one launch", who);
    }
    if (dev)
        for (int64_t r = 0; r < R; ++r)
            if (a[r].n > 0 && ((uintptr_t)a[r].data % (uintptr_t)ingest_elem_bytes(a[r].encoding)) != 0)
                SD_FAIL(c, SD_ERR_ARG, "%s: recording %lld: the device pointer is not aligned to its %d-byte elements", who, (long long)r, ingest_elem_bytes(a[r].encoding));
    int rc;
    if ((rc = enrolled_refusal(c, SD_EMB_DIM, c->num_clusters, c->min_clusters, c->max_clusters))) return rc;

    const double t0 = now_ms();
    clear_stage_ms(c);
    const std::vector<PackRange>& rec = plan.rec;
    const int64_t total = plan.total;
    rc = finalize_jobs(c, R, turns, n_turns, status, [&](std::vector<FinalJob>& jobs) -> int {
        if (total <= 0) return SD_OK;
        const size_t S = plan.owner.size();      // rows with a source; the pad row is behind them
        // tap tables first: building one synchronises, a cached one costs nothing
        for (size_t k = 0; k < S; ++k) {
            IngestRow& w = plan.rows[k];
            if (w.L == w.M) continue;
            const int32_t sr = a[plan.owner[k]].sample_rate;
            ResamplePlan p;
            if (int e = resample_check(c, sr, SD_SAMPLE_RATE, p)) return e;
            if (int e = resample_taps(c, sr, SD_SAMPLE_RATE, p, &w.taps)) return e;
        }
        if (dev) for (size_t k = 0; k < S; ++k) plan.rows[k].src = a[plan.owner[k]].data;
        else {
            WS(c, char, d_src, "many_src", (size_t)plan.upload_bytes);
            for (size_t k = 0; k < S; ++k) {
                HIPCHK(c, hipMemcpyAsync(d_src + plan.src_off[k], a[plan.owner[k]].data, (size_t)plan.src_bytes[k], hipMemcpyHostToDevice, c->stream));
                plan.rows[k].src = d_src + plan.src_off[k];
            }
        }
        const std::vector<char> tab = many_ingest_table(plan.rows, plan.tile0);
        float *d_seg = nullptr, *d_emb = nullptr;
        if (int e = pack_infer_fill(c, tab.size(), [&](char* d_tab, float* d_pack, int64_t pack_len) -> int {
                HIPCHK(c, hipMemcpy(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
                return launch_many_ingest(c, d_tab, plan.rows, plan.tile0, plan.max_span, d_pack, pack_len);
            }, rec, total, t0, &d_seg, &d_emb)) return e;
        for (const PackRange& q : rec) jobs[(size_t)q.owner] = FinalJob{d_seg + (size_t)q.base * SD_FRAMES * 3, d_emb + (size_t)q.base * 3 * SD_EMB_DIM, q.chunks, q.n};
        return SD_OK;
    });
    if (rc) return rc;
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

extern "C" int sd_diarize_many_audio(sd_ctx* c, const sd_audio* rec, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    ENTER(c);
    return many_audio_run(c, rec, false, R, turns, n_turns, status, "sd_diarize_many_audio");
}

extern "C" int sd_diarize_many_audio_dev(sd_ctx* c, const sd_audio* rec, int64_t R, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    ENTER(c);
    return many_audio_run(c, rec, true, R, turns, n_turns, status, "sd_diarize_many_audio_dev");
}

extern "C" int sd_many_select(sd_ctx* c, int64_t r)
{
    if (!c) return SD_ERR_ARG;
    c->err.clear();
    if (r < 0 || r >= (int64_t)c->many_jobs.size()) SD_FAIL(c, SD_ERR_ARG, "sd_many_select: the last sd_diarize_many* / sd_stream_turns_many call of this context had %zu recordings", c->many_jobs.size());
    const ManyJob& job = c->many_jobs[(size_t)r];
    if (job.status != SD_OK) SD_FAIL(c, SD_ERR_ARG, "sd_many_select: recording %lld ended with status %d and left no job", (long long)r, job.status);
    c->last = job.res;
    return SD_OK;
}
