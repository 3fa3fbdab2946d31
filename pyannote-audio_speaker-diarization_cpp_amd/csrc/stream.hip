// stream.hip -- sd_stream_*: incremental diarization of a recording that is still growing.  Replaces calling speakerDiarization()
// (sd.cpp:2937-3234) again on everything heard so far: a stream keeps the scores and embeddings of the chunks that can never change
// again (stream_book.h: blocks of 32 chunks whose every chunk ends in front of the last sample), the audio behind them as f32 on the
// device, and at sd_stream_turns infers only the chunks behind the sealed part before the usual finalize.  The networks run through
// shard_infer on sub-ranges (pipeline.cpp); the device code here is the tail's compaction (16-bit pushes are appended by k_pcm_to_f32).
// sd_stream_push_many* / sd_stream_turns_many serve many streams of one context in one call: the networks run over a pack of the streams' blocks and
// pending ranges (many.hip: pack_infer), three table-driven copy kernels replace the per-stream launches; the single-stream entries keep their paths.
// A range is a PackRange (many_plan.h) built by pack_range (stream_book.h), a copy a GroupRow (stream_book.h); which side of PyanNet's skinny limit a
// chunk is on is seg_tile_chunks' word (many_plan.h) for the pack and for segment_pending alike; the finalize per stream is many.hip's finalize_jobs.
// A roster attached to a stream (sd_stream_set_roster; the rule: roster.cpp) renames the labels behind a successful finalize: host arithmetic on what the
// finalize left in the context, no launch of its own.
// A stream with an input rate (sd_stream_set_input_rate) takes its samples at that rate: a push puts them behind the inputs the stream keeps
// (resample_book.h) and one k_resample_jobs launch (resample.hip) writes the 16 kHz samples they made final straight behind the tail -- in a group call
// one launch for all such streams, whatever their rates; everything behind the tail sees 16 kHz samples and is what it was.
// A stream with an input format (sd_stream_set_input_format) takes interleaved frames in its own encoding through the _audio pushes: k_group_ingest
// (stream_ingest.hip) on the table stream_ingest_plan.h makes of them is the conversion launch, of one row in a single call and of all streams' rows in a
// group call, where the legs of one stereo call share one upload; behind it the push is the typed push of the floats it decoded.
#include "common.h"
#include "stream_book.h"
#include "resample_book.h"
#include "stream_ingest_plan.h"
#include "roster.h"
#include "../../include/sdhip_stream_test.h"
#include <algorithm>

static_assert(SD_TAIL_PAD == SD_WAV_PAD, "the tail's padding is what DevWav::padded promises");
static_assert(RS_HIST_SLACK >= SD_WAV_PAD, "k_pcm_to_f32 zeroes SD_WAV_PAD floats behind the inputs it converts into a stream's history");

// compaction into the second buffer: dst[0, len) = src[0, len), zeros behind; four floats per thread (src sits a multiple of 8000 floats
// behind its allocation's start, dst at the start of its own: both 16-byte aligned)
__global__ void k_tail_move(const float* __restrict__ src, float* __restrict__ dst, int64_t len)
{
    const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 4 <= len) { *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i); return; }
    for (int q = 0; q < 4; ++q) {
        const int64_t j = i + q;
        if (j < len) dst[j] = src[j];
        else if (j < len + SD_TAIL_PAD) dst[j] = 0.0f;
    }
}

// ------------------------------------------------------------------ device code of the group calls (sd_stream_push_many*, sd_stream_turns_many)
// Three copy kernels, each ONE launch per call for all streams, walking a table of rows: dst[0, len) = src[0, len) and `pad` zeros behind, nothing at
// or behind dst[room].  A row is cut into groups of four floats at the 16-byte boundaries of its DESTINATION (a tail ends anywhere): group 0 is the
// 0 .. 3 floats in front of the first boundary, group g the four from head + 4 (g - 1) on, stored as one float4; the source is read 16 bytes (8 for
// 16-bit samples) at a time where it is aligned at `head` too -- the host pushes are staged so that it is -- and element by element where not.
//   k_group_append     the pushes of all streams to the ends of their tails, SD_TAIL_PAD zeros behind each (16-bit: x 1/32768 as k_pcm_to_f32; f32: copied)
//   k_group_scatter    rows of the pack's scores / embeddings into the caches of the streams that own them
//   k_group_tail_move  the compactions of all streams that sealed: k_tail_move per row
// grid (x: a stride over the groups of a row, y: a stride over the table), 256 threads; 64-bit indices throughout.  GroupRow: stream_book.h

template <bool PCM> __device__ __forceinline__ float group_load(const void* src, int64_t j)
{
    return PCM ? pcm_to_float(((const int16_t*)src)[j]) : ((const float*)src)[j];
}

template <bool PCM> __device__ __forceinline__ void group_copy(const GroupRow* __restrict__ rows, int R, int64_t pad)
{
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int r = blockIdx.y; r < R; r += gridDim.y) {
        const GroupRow row = rows[r];
        const int64_t end = row.len + pad < row.room ? row.len + pad : row.room;      // floats of dst this row may write
        const int64_t n = row.len < end ? row.len : end;                               // ... that come from src
        int64_t head = (int64_t)((16 - ((uintptr_t)row.dst & 15)) & 15) / 4;
        if (head > end) head = end;
        const uintptr_t src_at_head = (uintptr_t)row.src + (uintptr_t)head * (PCM ? sizeof(int16_t) : sizeof(float));
        const bool wide = (src_at_head & (PCM ? 7 : 15)) == 0;
        for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; ; g += step) {
            const int64_t i = g == 0 ? 0 : head + 4 * (g - 1);
            const int64_t cnt = g == 0 ? head : 4;
            if (i >= end) break;
            if (g > 0 && i + 4 <= end) {      // a whole aligned group: one 16-byte store
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (i + 4 <= n && wide) {
                    if (PCM) {
                        const short4 p = *reinterpret_cast<const short4*>((const int16_t*)row.src + i);
                        v = make_float4(pcm_to_float(p.x), pcm_to_float(p.y), pcm_to_float(p.z), pcm_to_float(p.w));
                    } else v = *reinterpret_cast<const float4*>((const float*)row.src + i);
                } else {
                    if (i < n) v.x = group_load<PCM>(row.src, i);
                    if (i + 1 < n) v.y = group_load<PCM>(row.src, i + 1);
                    if (i + 2 < n) v.z = group_load<PCM>(row.src, i + 2);
                    if (i + 3 < n) v.w = group_load<PCM>(row.src, i + 3);
                }
                *reinterpret_cast<float4*>(row.dst + i) = v;
                continue;
            }
            for (int64_t j = i; j < i + cnt && j < end; ++j) row.dst[j] = j < n ? group_load<PCM>(row.src, j) : 0.0f;
        }
    }
}

__global__ void k_group_append(const GroupRow* __restrict__ rows, int R, int is_f32)
{
    if (is_f32) group_copy<false>(rows, R, SD_TAIL_PAD);
    else group_copy<true>(rows, R, SD_TAIL_PAD);
}
__global__ void k_group_scatter(const GroupRow* __restrict__ rows, int R) { group_copy<false>(rows, R, 0); }
__global__ void k_group_tail_move(const GroupRow* __restrict__ rows, int R) { group_copy<false>(rows, R, SD_TAIL_PAD); }

// the launches of the four copy kernels, for the stages below and for the hooks of input_test.hip (common.h)
int launch_tail_move(sd_ctx* c, float* dst, const float* src, int64_t len)
{
    hipLaunchKernelGGL(k_tail_move, GRID1((len + SD_TAIL_PAD + 3) / 4), 0, c->stream, src, dst, len);
    KCHECK(c);
    return SD_OK;
}

int group_launch(sd_ctx* c, int which, const GroupRow* d_rows, const std::vector<GroupRow>& rows, int is_f32)
{
    if (rows.empty()) return SD_OK;
    int64_t longest = 1;
    for (const GroupRow& r : rows) longest = std::max(longest, r.len + SD_TAIL_PAD);
    const dim3 grid = many_grid(longest / 4 + 2, (int64_t)rows.size());
    if (which == 0) { ProfScope ps(c, "group_append"); hipLaunchKernelGGL(k_group_append, grid, dim3(256), 0, c->stream, d_rows, (int)rows.size(), is_f32); }
    else if (which == 1) hipLaunchKernelGGL(k_group_scatter, grid, dim3(256), 0, c->stream, d_rows, (int)rows.size());
    else hipLaunchKernelGGL(k_group_tail_move, grid, dim3(256), 0, c->stream, d_rows, (int)rows.size());
    KCHECK(c);
    return SD_OK;
}

struct sd_stream {
    sd_ctx* c = nullptr;
    StreamBook b;
    int ecapa_precision = 0, seg_precision = 0;      // fixed at sd_stream_open: a cache of mixed precision is nobody's answer
    bool dead = false;                               // after SD_ERR_HIP: every call but sd_stream_close is refused
    int64_t window = -1;                             // sd_stream_set_window: sealed blocks kept after a push that seals one (-1: all of them)
    sd_roster* roster = nullptr;                     // sd_stream_set_roster: names the labels of every turns call (null: raw cluster numbers)
    std::vector<int32_t> kept;                       // ... the roster id of every table row at the last update, -1 where the row had no label
    int64_t kept_origin = 0;                         // ... and the origin then: row i of the table now was row i + 3 (origin - kept_origin) / 8000
    bool has_kept = false;
    RateBook r;                                      // sd_stream_set_input_rate: the inputs held and the outputs emitted (resample_book.h); in_sr 0 = a plain stream
    StreamFormat f;                                  // sd_stream_set_input_format: the frames the _audio pushes hand over (stream_ingest_plan.h); not set = the typed pushes
};

namespace {
// the device operations of stream_book.h on the stream's context; copies are ordered on the context's stream
struct HipDev {
    sd_ctx* c;
    bool alloc_failed = false;      // the failure this Dev reported was an allocation's: nothing has been launched or moved for it
    int alloc(void** p, size_t bytes) {
        if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; alloc_failed = true; SD_FAIL(c, SD_ERR_HIP, "hipMalloc of %zu bytes for a stream failed", bytes); }
        return SD_OK;
    }
    void release(void* p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); }
    int copy(void* dst, const void* src, size_t bytes) {
        HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
        return SD_OK;
    }
    int move_tail(float* dst, const float* src, int64_t len) { return launch_tail_move(c, dst, src, len); }
};

// The segmentation step of the pending range [lo, hi), lo = sealed.  PyanNet's dense layers (LSTM layer 0's input projection, the two linear layers)
// take k_skinny_gemm up to SD_SKINNY_CHUNKS = 13 chunks in a batch and the 128 x 128 tile above that; the two sum K in different orders.  The whole path
// computes these chunks in a batch that starts at a multiple of seg_batch_chunks; where seg_tile_chunks (many_plan.h) says that batch is on the tile
// side and the pending one alone is not, the pending chunks run in a batch padded to 14 chunks:
// a scratch waveform with the pending full chunks' audio and zeros behind it, as a recording just long enough for 14 full chunks from lo on.  A row's
// bits depend on its own chunk and on the kernels alone, so the real rows are the whole path's; the padding rows are thrown away.  The short last
// chunk is a batch of one in both paths.
int segment_pending(sd_stream* s, const DevWav& tail, int64_t lo, int64_t hi)
{
    sd_ctx* c = s->c;
    const StreamBook& b = s->b;
    float* d_seg = b.seg + lo * SD_SEG_ROW;
    int64_t last_len = 0;
    const int64_t total = sd_num_chunks(b.n, &last_len);
    const bool short_tail = hi == total && last_len > 0 && last_len < SD_CHUNK;
    const int64_t full_hi = short_tail ? hi - 1 : hi, mine = full_hi - lo;
    if (mine <= 0 || mine > SD_SKINNY_CHUNKS || seg_tile_chunks(lo, mine, c->seg_batch_chunks, true) != mine) return run_segment(c, tail, lo, hi, d_seg);
    const int64_t pad_hi = lo + SD_SKINNY_CHUNKS + 1;
    const int64_t n_pad = (pad_hi - 1) * SD_HOP + SD_CHUNK + 1;                      // the shortest recording whose chunks [lo, pad_hi) are all full
    const int64_t have = (full_hi - 1) * SD_HOP + SD_CHUNK - lo * SD_HOP;            // samples of the pending full chunks: all in the tail
    const int64_t len = n_pad - lo * SD_HOP;
    WS(c, float, w, "st_pad_wav", len + SD_TAIL_PAD);
    WS(c, float, sg, "st_pad_seg", (pad_hi - lo) * SD_SEG_ROW);
    HIPCHK(c, hipMemcpyAsync(w, b.tail_now(), (size_t)have * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(w + have, 0, (size_t)(len + SD_TAIL_PAD - have) * sizeof(float), c->stream));
    int rc;
    if ((rc = run_segment(c, DevWav{w, n_pad, lo * SD_HOP, true}, lo, pad_hi, sg))) return rc;
    HIPCHK(c, hipMemcpyAsync(d_seg, sg, (size_t)(mine * SD_SEG_ROW) * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (short_tail) return run_segment(c, tail, hi - 1, hi, d_seg + mine * SD_SEG_ROW);
    return SD_OK;
}

// book_forget on the stream's context, by hand or as the window's policy behind a push.  A failed allocation leaves the book what it was before the
// forget (stream_book.h) with nothing launched: the call returns SD_ERR_HIP, but guard / group_guard leave the streams usable (c->stream_intact)
int forget_to(sd_stream* s, int64_t keep_blocks)
{
    HipDev dev{s->c};
    const int rc = book_forget(dev, s->b, keep_blocks);
    if (rc && dev.alloc_failed) s->c->stream_intact = true;
    return rc;
}

// both networks on chunks [lo, hi) of the recording, read from the tail, into the cache rows of those chunks
int infer_rows(sd_stream* s, int64_t lo, int64_t hi, bool pending)
{
    sd_ctx* c = s->c;
    StreamBook& b = s->b;
    // kernels index the recording with absolute sample positions; every append and every compaction leaves SD_TAIL_PAD zeros behind sample n
    const DevWav tail{b.tail_now(), b.n, b.sealed * SD_HOP, true};
    if (pending) {      // its launches are timed with the segmentation stage: shard_infer synchronises behind the masks
        const double t0 = now_ms();
        const int rc = segment_pending(s, tail, lo, hi);
        c->stage_ms[0] += now_ms() - t0;
        if (rc) return rc;
    }
    return shard_infer(c, tail, lo, hi, b.seg + lo * SD_SEG_ROW, b.emb + lo * SD_EMB_ROW, pending);
}

// the blocks that have become sealed: inferred once, then their audio is dropped
int seal_blocks(sd_stream* s, bool window)
{
    StreamBook& b = s->b;
    const int64_t to = stream_sealed_chunks(b.n);
    if (to <= b.sealed) return SD_OK;
    HipDev dev{s->c};
    int rc;
    if ((rc = book_reserve_cache(dev, b, sd_num_chunks(b.n, nullptr)))) return rc;
    if ((rc = infer_rows(s, b.sealed, to, false))) return rc;
    if ((rc = book_seal(dev, b, to))) return rc;
    return window && s->window >= 0 ? forget_to(s, s->window) : SD_OK;      // the window's policy: a push that sealed a block forgets down to it
}

int check_call(sd_stream* s, const char* who)
{
    sd_ctx* c = s->c;
    if (s->dead) SD_FAIL(c, SD_ERR_ARG, "%s: the stream is unusable after a HIP failure; close it", who);
    if (c->ecapa_precision != s->ecapa_precision || seg_prec(c) != s->seg_precision)
        SD_FAIL(c, SD_ERR_ARG, "%s: the stream was opened with ecapa_precision %d / seg_precision %d, the context now has %d / %d", who,
                s->ecapa_precision, s->seg_precision, c->ecapa_precision, seg_prec(c));
    return SD_OK;
}

inline bool audio_kind(int kind) { return kind == SD_AUDIO_HOST || kind == SD_AUDIO_DEV; }

const char* ingest_refusal_text(int e)
{
    switch (e) {
    case SI_NO_FORMAT: return "the stream has no input format (sd_stream_set_input_format)";
    case SI_FRAMES: return "a bad number of frames";
    case SI_NULL_DATA: return "a null pointer with frames to read";
    case SI_BYTES: return "a piece beyond SD_INGEST_MAX_BYTES";
    default: return "a device pointer that is not aligned to its element";
    }
}

// The conversion launch of the _audio pushes: the table of a plan on the device -- for the host form behind the uploads, one per distinct source, into one
// workspace -- and ONE k_group_ingest launch.  A failed allocation comes before the first launch and leaves every stream what it was.
int ingest_rows(sd_ctx* c, StreamIngestPlan& plan, bool host)
{
    if (plan.rows.empty()) return SD_OK;
    StreamIngestRow* d_tab = ws_get<StreamIngestRow>(c, "stg_itab", plan.rows.size());
    char* stage = host ? ws_get<char>(c, "stg_src", (size_t)plan.upload_bytes + 16) : nullptr;
    if (!d_tab || (host && !stage)) { c->stream_intact = true; SD_FAIL(c, SD_ERR_HIP, "hipMalloc of the staging workspaces of %zu rows (%lld bytes) failed", plan.rows.size(), (long long)plan.upload_bytes); }
    if (host) {
        for (size_t u = 0; u < plan.up_src.size(); ++u)
            HIPCHK(c, hipMemcpyAsync(stage + plan.up_off[u], plan.up_src[u], (size_t)plan.up_bytes[u], hipMemcpyHostToDevice, c->stream));
        for (size_t q = 0; q < plan.rows.size(); ++q) plan.rows[q].src = stage + plan.up_off[(size_t)plan.cls[q]];
    }
    HIPCHK(c, hipMemcpy(d_tab, plan.rows.data(), plan.rows.size() * sizeof(StreamIngestRow), hipMemcpyHostToDevice));
    return launch_group_ingest(c, d_tab, plan.rows, SD_TAIL_PAD);
}

// ... of a single push: a table of one row
int ingest_one(sd_stream* s, const void* src, int64_t m, int kind, float* dst, int64_t room)
{
    const StreamPiece p{src, m, s->f};
    StreamIngestPlan plan;
    stream_ingest_plan(&p, &dst, &room, 1, kind == SD_AUDIO_HOST, plan);
    return ingest_rows(s->c, plan, kind == SD_AUDIO_HOST);
}

// A push to a stream with an input rate (sd_stream_set_input_rate): the piece goes behind the inputs the stream holds, ONE k_resample_jobs launch of one
// row writes the outputs that piece made final -- [F(n), F(n')), resample_book.h -- straight behind the tail with their padding, and from there on it is
// a push of those 16 kHz samples.  A push that makes no output final only extends the inputs held.  Growth comes first: a failed allocation leaves the
// stream as it was, and usable.
int push_rated(sd_stream* s, const void* src, int64_t m, int kind, const char* who)
{
    sd_ctx* c = s->c;
    StreamBook& b = s->b;
    RateBook& r = s->r;
    if (r.closed) SD_FAIL(c, SD_ERR_ARG, "%s: the stream's input was closed by sd_stream_end_input", who);
    if (m == 0) return SD_OK;
    const double t0 = now_ms();
    clear_stage_ms(c);
    HipDev dev{c};
    const RatePush q = rate_plan_push(r, m);
    const float* taps = nullptr;
    int rc;
    if ((rc = resample_taps(c, r.in_sr, SD_SAMPLE_RATE, r.p, &taps))) return rc;      // (cached since sd_stream_set_input_rate)
    if (!(rc = rate_reserve(dev, r, m)) && q.count > 0) rc = book_reserve_tail(dev, b, q.count);
    if (rc) { if (dev.alloc_failed) c->stream_intact = true; return rc; }
    float* in = r.buf[r.cur] + r.held();
    if (audio_kind(kind)) { if ((rc = ingest_one(s, src, m, kind, in, m))) return rc; }      // (room = m: nothing behind the inputs)
    else if (kind == SD_F32_HOST) HIPCHK(c, hipMemcpyAsync(in, src, (size_t)m * sizeof(float), hipMemcpyHostToDevice, c->stream));
    else {
        const int16_t* d_pcm = (const int16_t*)src;
        if (kind == SD_PCM_HOST) {
            WS(c, int16_t, stage, "st_pcm", m);
            HIPCHK(c, hipMemcpyAsync(stage, src, (size_t)m * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            d_pcm = stage;
        }
        {
            ProfScope ps(c, "pcm_to_f32");
            hipLaunchKernelGGL(k_pcm_to_f32, GRID1(m + SD_WAV_PAD), 0, c->stream, d_pcm, in, m);      // (its zeros land in the slack behind the inputs)
        }
        KCHECK(c);
    }
    if (q.count > 0) {
        const ResampleJob job = rate_job(r, q, b.tail_now() + b.tail_len(), taps, SD_TAIL_PAD);
        if ((rc = resample_jobs(c, &job, 1))) return rc;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's buffer may go
    rate_commit(r, q);
    b.n += q.count;
    if ((rc = seal_blocks(s, true))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

// sd_stream_end_input: the outputs behind the last final one, [F(n), len(n)), with silence behind the last input as sd_resample has it; afterwards the
// stream is a plain stream to which sd_resample of all its inputs was pushed, and takes no more
int end_input_impl(sd_stream* s)
{
    sd_ctx* c = s->c;
    const char* who = "sd_stream_end_input";
    if (int rc = check_call(s, who)) return rc;
    StreamBook& b = s->b;
    RateBook& r = s->r;
    if (!r.in_sr && !r.direct) SD_FAIL(c, SD_ERR_ARG, "%s: the stream has no input rate (sd_stream_set_input_rate)", who);
    if (r.closed) return SD_OK;
    if (r.direct) { r.closed = true; return SD_OK; }      // a rate of 16 000: nothing is held back, the input is just closed
    const double t0 = now_ms();
    clear_stage_ms(c);
    HipDev dev{c};
    const RatePush q = rate_plan_flush(r);
    int rc;
    if (q.count > 0) {
        const float* taps = nullptr;
        if ((rc = resample_taps(c, r.in_sr, SD_SAMPLE_RATE, r.p, &taps))) return rc;
        if ((rc = book_reserve_tail(dev, b, q.count))) { if (dev.alloc_failed) c->stream_intact = true; return rc; }
        const ResampleJob job = rate_job(r, q, b.tail_now() + b.tail_len(), taps, SD_TAIL_PAD);
        if ((rc = resample_jobs(c, &job, 1))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    rate_commit(r, q);
    r.closed = true;
    rate_release(dev, r);
    b.n += q.count;
    if ((rc = seal_blocks(s, true))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

// sd_stream_set_input_rate: before the first sample only; 16 000 = no resampler (the stream only remembers that a rate was set, so that
// sd_stream_end_input can close its input).  Nothing of the stream is touched by a refusal or a failure
int set_rate_impl(sd_stream* s, int32_t in_sr)
{
    sd_ctx* c = s->c;
    const char* who = "sd_stream_set_input_rate";
    if (int rc = check_call(s, who)) return rc;
    c->stream_intact = true;
    if (in_sr <= 0) SD_FAIL(c, SD_ERR_ARG, "%s: bad sample rate %d", who, in_sr);
    if (s->b.n > 0 || s->b.origin > 0 || s->r.n_in > 0 || s->r.closed) SD_FAIL(c, SD_ERR_ARG, "%s: samples have been pushed; the rate is set before the first one", who);
    RateBook nb;
    if (in_sr != SD_SAMPLE_RATE) {
        int rc;
        if ((rc = resample_check(c, in_sr, SD_SAMPLE_RATE, nb.p))) return rc;
        if ((nb.p.span + RS_BLOCK) * (int64_t)sizeof(float) > 160 * 1024) SD_FAIL(c, SD_ERR_ARG, "%s: %d Hz: a tile's input span (%lld samples) does not fit the LDS", who, in_sr, (long long)nb.p.span);
        const float* taps = nullptr;
        if ((rc = resample_taps(c, in_sr, SD_SAMPLE_RATE, nb.p, &taps))) return rc;      // built here: no push pays for it
        nb.in_sr = in_sr;
    } else nb.direct = true;
    HipDev dev{c};
    rate_release(dev, s->r);
    s->r = nb;
    return SD_OK;
}

// sd_stream_set_input_format: before the first sample only, like the rate, and in either order with it.  Nothing of the stream is touched by a refusal
int set_format_impl(sd_stream* s, int32_t enc, int32_t channels, int32_t channel)
{
    sd_ctx* c = s->c;
    const char* who = "sd_stream_set_input_format";
    if (int rc = check_call(s, who)) return rc;
    c->stream_intact = true;
    if (!stream_format_ok(enc, channels, channel)) SD_FAIL(c, SD_ERR_ARG, "%s: bad format (encoding %d, %d channels, channel %d)", who, enc, channels, channel);
    if (s->b.n > 0 || s->b.origin > 0 || s->r.n_in > 0 || s->r.closed) SD_FAIL(c, SD_ERR_ARG, "%s: samples have been pushed or the input is closed; the format is set before the first sample", who);
    s->f.enc = enc; s->f.channels = channels; s->f.channel = channel; s->f.set = true;
    return SD_OK;
}

int push_impl(sd_stream* s, const void* src, int64_t m, int kind, const char* who)
{
    sd_ctx* c = s->c;
    if (m < 0 || (m > 0 && !src)) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
    if (int rc = check_call(s, who)) return rc;
    if (audio_kind(kind) != s->f.set)
        SD_FAIL(c, SD_ERR_ARG, s->f.set ? "%s: the stream has an input format (sd_stream_set_input_format) and takes the _audio pushes only" : "%s: the stream has no input format (sd_stream_set_input_format)", who);
    if (audio_kind(kind)) {
        const StreamPiece p{src, m, s->f};
        int64_t bad = -1;
        if (const int e = stream_ingest_check(&p, 1, kind == SD_AUDIO_DEV, &bad)) SD_FAIL(c, SD_ERR_ARG, "%s: %s", who, ingest_refusal_text(e));
    }
    if (s->r.in_sr) return push_rated(s, src, m, kind, who);
    if (s->r.closed) SD_FAIL(c, SD_ERR_ARG, "%s: the stream's input was closed by sd_stream_end_input", who);
    if (m == 0) return SD_OK;
    const double t0 = now_ms();
    clear_stage_ms(c);
    StreamBook& b = s->b;
    HipDev dev{c};
    int rc;
    if ((rc = book_reserve_tail(dev, b, m))) return rc;
    float* dst = b.tail_now() + b.tail_len();
    if (audio_kind(kind)) { if ((rc = ingest_one(s, src, m, kind, dst, b.tail_cap[b.cur] - b.tail_len()))) return rc; }
    else if (kind == SD_F32_HOST) {
        HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)m * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(dst + m, 0, SD_TAIL_PAD * sizeof(float), c->stream));
    } else {
        const int16_t* d_pcm = (const int16_t*)src;
        if (kind == SD_PCM_HOST) {
            WS(c, int16_t, stage, "st_pcm", m);
            HIPCHK(c, hipMemcpyAsync(stage, src, (size_t)m * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            d_pcm = stage;
        }
        {
            ProfScope ps(c, "pcm_to_f32");
            hipLaunchKernelGGL(k_pcm_to_f32, GRID1(m + SD_TAIL_PAD), 0, c->stream, d_pcm, dst, m);
        }
        KCHECK(c);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's buffer may go
    b.n += m;
    if ((rc = seal_blocks(s, true))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

// The roster's update behind a finalize that succeeded: c->last describes that job, t[0, nt) are its turns with raw labels.  The rule runs on the
// centroids and counts of the job, its hard labels, and the ids this stream kept from its previous update; then the labels of t become roster ids and
// c->last carries the map.  `kept` receives ids[hard[i]] per row for the caller to commit.  Any failure leaves the roster, the stream and t untouched.
int name_turns(sd_stream* s, sd_turn* t, int64_t nt, std::vector<int32_t>& kept)
{
    sd_ctx* c = s->c;
    JobResult& job = c->last;
    const int64_t K = job.cen_K, M = (int64_t)job.hard.size();
    if (job.cen_d != s->roster->d) SD_FAIL(c, SD_ERR_ARG, "the roster's entries have %d dimensions, the job's centroids %d", s->roster->d, job.cen_d);
    for (int64_t i = 0; i < nt; ++i) if (t[i].label < 0 || t[i].label >= K) SD_FAIL(c, SD_ERR_ARG, "turn label %d outside the job's %lld label columns", t[i].label, (long long)K);
    const int64_t shift = SD_SPEAKERS * ((s->b.origin - s->kept_origin) / SD_HOP);
    std::vector<int32_t> ids((size_t)K);
    kept.resize((size_t)M);
    const int rc = sd_roster_update(s->roster, job.cen.data(), job.cen_counts.data(), K, job.hard.data(), M, s->has_kept ? s->kept.data() : nullptr,
                                    s->has_kept ? (int64_t)s->kept.size() : 0, s->has_kept ? shift : 0, c->speaker_match_threshold, ids.data());
    if (rc == SD_ERR_NUMERIC) SD_FAIL(c, rc, "roster update: zero-magnitude centroid (reference throws, sd.cpp:493-495)");
    if (rc) SD_FAIL(c, rc, "roster update failed (%d)", rc);
    for (int64_t i = 0; i < M; ++i) kept[(size_t)i] = job.hard[(size_t)i] >= 0 ? ids[(size_t)job.hard[(size_t)i]] : -1;
    (void)sd_relabel_turns_map(t, nt, ids.data(), K);      // (the labels were checked above)
    job.roster_ids = std::move(ids);
    return SD_OK;
}

int turns_impl(sd_stream* s, sd_turn** turns, int64_t* n_turns)
{
    sd_ctx* c = s->c;
    if (!turns || !n_turns) SD_FAIL(c, SD_ERR_ARG, "sd_stream_turns: bad argument");
    if (int rc = check_call(s, "sd_stream_turns")) return rc;
    if (!c->dump_dir.empty()) SD_FAIL(c, SD_ERR_ARG, "sd_stream_turns: the step files describe one whole-path inference; clear the dump directory");
    StreamBook& b = s->b;
    const int64_t total = sd_num_chunks(b.n, nullptr);
    if (total <= 0) SD_FAIL(c, SD_ERR_SHORT, "audio of %lld samples yields no chunk", (long long)b.n);
    const double t0 = now_ms();
    clear_stage_ms(c);
    int rc;
    if ((rc = seal_blocks(s, false))) return rc;     // (nothing to do unless an earlier push failed half way; the window waits for the next push that seals)
    if (b.pending_n != b.n) {
        HipDev dev{c};
        if ((rc = book_reserve_cache(dev, b, total))) return rc;
        if ((rc = infer_rows(s, b.sealed, total, true))) return rc;
        b.pending_n = b.n;
    }
    std::vector<sd_turn> v;
    if ((rc = finalize(c, b.seg, b.emb, total, b.n, v))) return rc;
    c->stage_ms[3] = now_ms() - t0;
    if (!s->roster) return turns_out(c, v, turns, n_turns);
    // the turns are handed over first: the update is the last thing that can fail, and it changes nothing when it does
    sd_turn* t = nullptr; int64_t nt = 0;
    std::vector<int32_t> kept;
    if ((rc = turns_out(c, v, &t, &nt))) return rc;
    if ((rc = name_turns(s, t, nt, kept))) { sd_free_turns(t); return rc; }
    s->kept.swap(kept); s->kept_origin = b.origin; s->has_kept = true;
    c->stage_ms[3] = now_ms() - t0;
    *turns = t; *n_turns = nt;
    return SD_OK;
}

int read_impl(sd_stream* s, int64_t lo, int64_t hi, float* h_seg, float* h_emb)
{
    sd_ctx* c = s->c;
    if (s->dead) SD_FAIL(c, SD_ERR_ARG, "sd_stream_read: the stream is unusable after a HIP failure; close it");
    const StreamBook& b = s->b;
    const int64_t total = sd_num_chunks(b.n, nullptr);
    if (lo < 0 || lo > hi || hi > total) SD_FAIL(c, SD_ERR_ARG, "sd_stream_read: chunks [%lld,%lld) outside [0,%lld)", (long long)lo, (long long)hi, (long long)total);
    if (hi > b.sealed && b.pending_n != b.n)
        SD_FAIL(c, SD_ERR_ARG, "sd_stream_read: chunks from %lld on are pending and stale; call sd_stream_turns first", (long long)b.sealed);
    if (hi == lo) return SD_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h_seg) HIPCHK(c, hipMemcpy(h_seg, b.seg + lo * SD_SEG_ROW, (size_t)((hi - lo) * SD_SEG_ROW) * sizeof(float), hipMemcpyDeviceToHost));
    if (h_emb) HIPCHK(c, hipMemcpy(h_emb, b.emb + lo * SD_EMB_ROW, (size_t)((hi - lo) * SD_EMB_ROW) * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}

// sd_stream_forget: all but the last keep_blocks sealed blocks go (stream_book.h: book_forget)
int forget_impl(sd_stream* s, int64_t keep_blocks, const char* who)
{
    sd_ctx* c = s->c;
    if (keep_blocks < 0) SD_FAIL(c, SD_ERR_ARG, "%s: keep_blocks must be >= 0", who);
    if (int rc = check_call(s, who)) return rc;
    if (int rc = forget_to(s, keep_blocks)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

// a HIP failure in the middle of a call leaves a tail or a cache nobody can vouch for
// (unless the only failure was an allocation of a forget: forget_to)
int guard(sd_stream* s, int rc) { if (rc == SD_ERR_HIP && !s->c->stream_intact) s->dead = true; s->c->stream_intact = false; return rc; }

// ------------------------------------------------------------------ groups of streams
// the refusals both group calls share; the caller has checked the list itself and every entry against null
int group_check(sd_ctx* c, sd_stream* const* s, int64_t S, const char* who)
{
    std::vector<const sd_stream*> seen(s, s + S);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) SD_FAIL(c, SD_ERR_ARG, "%s: the same stream twice in the list", who);
    for (int64_t i = 0; i < S; ++i) if (s[i]->c != c) SD_FAIL(c, SD_ERR_ARG, "%s: stream %lld belongs to another context", who, (long long)i);
    for (int64_t i = 0; i < S; ++i) if (int rc = check_call(s[i], who)) return rc;
    if (c->planted_n > 0) SD_FAIL(c, SD_ERR_ARG, "%s: a planted workload is set (its chunk range means one recording)", who);
    return SD_OK;
}

// the ranges the streams contribute once stream i holds n_after[i] samples and `sealed[i]` sealed chunks, with their slots
int group_ranges(sd_ctx* c, int64_t S, const int64_t* n_after, const int64_t* sealed, const char* wanted, bool pending, std::vector<PackRange>& out, int64_t* total, const char* who)
{
    out.clear();
    for (int64_t i = 0; i < S; ++i) {
        PackRange r;
        if (!wanted[i] || !pack_range(n_after[i], sealed[i], c->seg_batch_chunks, pending, r)) continue;
        r.owner = i;
        out.push_back(r);
    }
    if (pack_plan(out.data(), (int64_t)out.size(), total)) SD_FAIL(c, SD_ERR_ARG, "%s: a range of more than 2^40 samples", who);
    if (*total > SD_MANY_MAX_CHUNKS) SD_FAIL(c, SD_ERR_ARG, "%s: %lld packed chunks (limit %d: the rows of one call are counted in int)", who, (long long)*total, SD_MANY_MAX_CHUNKS);
    return SD_OK;
}

// Both networks over the pack of these ranges, read from the tails; their rows into the owners' caches; and, for blocks that became sealed, the
// compactions.  Tails, caches and compaction targets have their room (book_reserve_group).
int group_infer(sd_ctx* c, sd_stream* const* s, const std::vector<PackRange>& ranges, int64_t total, bool pending, bool window = false)
{
    if (ranges.empty()) return SD_OK;
    const double t0 = now_ms();
    std::vector<ManyRow> rows;
    for (const PackRange& r : ranges) rows.push_back(ManyRow{s[r.owner]->b.tail_now(), r.n, r.base * (int64_t)SD_HOP, r.slot() * (int64_t)SD_HOP});
    float *d_seg = nullptr, *d_emb = nullptr;
    int rc;
    if ((rc = pack_infer(c, rows, 1, ranges, total, t0, &d_seg, &d_emb))) return rc;
    std::vector<GroupRow> seg, emb, mov;
    for (const PackRange& r : ranges) {
        StreamBook& b = s[r.owner]->b;
        seg.push_back(GroupRow{d_seg + r.base * SD_SEG_ROW, b.seg + r.lo * SD_SEG_ROW, r.chunks * SD_SEG_ROW, (b.cache_cap - r.lo) * SD_SEG_ROW});
        emb.push_back(GroupRow{d_emb + r.base * SD_EMB_ROW, b.emb + r.lo * SD_EMB_ROW, r.chunks * SD_EMB_ROW, (b.cache_cap - r.lo) * SD_EMB_ROW});
        GroupRow mv;
        if (pending) b.pending_n = b.n;
        else if (book_seal_planned(b, r.hi(), mv)) mov.push_back(mv);
    }
    const size_t R = ranges.size();
    WS(c, GroupRow, d_tab, "stg_tab", 3 * R);
    HIPCHK(c, hipMemcpy(d_tab, seg.data(), R * sizeof(GroupRow), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_tab + R, emb.data(), R * sizeof(GroupRow), hipMemcpyHostToDevice));
    if (!mov.empty()) HIPCHK(c, hipMemcpy(d_tab + 2 * R, mov.data(), mov.size() * sizeof(GroupRow), hipMemcpyHostToDevice));
    if ((rc = group_launch(c, 1, d_tab, seg, 0))) return rc;
    if ((rc = group_launch(c, 1, d_tab + R, emb, 0))) return rc;
    if ((rc = group_launch(c, 2, d_tab + 2 * R, mov, 0))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!pending) {
        HipDev dev{c};
        for (const PackRange& r : ranges) book_seal_trim(dev, s[r.owner]->b);
        for (const PackRange& r : ranges)      // the window's policy, per stream, behind the group's launches
            if (window && s[r.owner]->window >= 0 && (rc = forget_to(s[r.owner], s[r.owner]->window))) return rc;
    }
    return SD_OK;
}

// what a group push does behind its conversion launch, whatever the form of the samples: the one k_resample_jobs launch, the one synchronisation, the
// books, and the packed inference of the blocks that became sealed
int push_many_tail(sd_ctx* c, sd_stream* const* s, int64_t S, const std::vector<ResampleJob>& jobs, const std::vector<RatePush>& rated,
                   const std::vector<int64_t>& add, const std::vector<PackRange>& ranges, int64_t total, double t0)
{
    int rc;
    if ((rc = resample_jobs(c, jobs.data(), (int64_t)jobs.size()))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the callers' buffers may go: once for all streams
    for (int64_t i = 0; i < S; ++i) {
        if (s[i]->r.in_sr) rate_commit(s[i]->r, rated[(size_t)i]);
        s[i]->b.n += add[(size_t)i];
    }

    if ((rc = group_infer(c, s, ranges, total, false, true))) return rc;
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

int push_many_impl(sd_ctx* c, sd_stream* const* s, const void* const* src, const int64_t* n, int64_t S, int kind, const char* who)
{
    // refusals: nothing is touched
    if (!src || !n) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
    int64_t pushed = 0;
    for (int64_t i = 0; i < S; ++i) {
        if (n[i] < 0 || n[i] > SD_MANY_MAX_SAMPLES || (n[i] > 0 && !src[i])) SD_FAIL(c, SD_ERR_ARG, "%s: bad samples for stream %lld", who, (long long)i);
        pushed += n[i];
    }
    int rc;
    if ((rc = group_check(c, s, S, who))) return rc;
    // a stream with an input format takes the _audio calls only, a stream without one the typed calls; a row that hands nothing over is legal in both
    const bool audio = audio_kind(kind);
    std::vector<StreamPiece> pieces;
    if (audio) {
        for (int64_t i = 0; i < S; ++i) pieces.push_back(StreamPiece{src[i], n[i], s[i]->f});
        int64_t bad = -1;
        if (const int e = stream_ingest_check(pieces.data(), S, kind == SD_AUDIO_DEV, &bad)) SD_FAIL(c, SD_ERR_ARG, "%s: stream %lld: %s", who, (long long)bad, ingest_refusal_text(e));
    } else
        for (int64_t i = 0; i < S; ++i) if (n[i] > 0 && s[i]->f.set) SD_FAIL(c, SD_ERR_ARG, "%s: stream %lld has an input format (sd_stream_set_input_format) and takes the _audio pushes only", who, (long long)i);
    // a stream with an input rate gains the outputs its piece makes final (push_rated), a plain one its piece: add[i] samples at 16 kHz
    std::vector<RatePush> rated((size_t)S);
    std::vector<int64_t> add(n, n + S);
    for (int64_t i = 0; i < S; ++i) {
        if (s[i]->r.closed && n[i] > 0) SD_FAIL(c, SD_ERR_ARG, "%s: the input of stream %lld was closed by sd_stream_end_input", who, (long long)i);
        if (!s[i]->r.in_sr) continue;
        rated[(size_t)i] = rate_plan_push(s[i]->r, n[i]);
        add[(size_t)i] = rated[(size_t)i].count;
    }
    std::vector<int64_t> n_after((size_t)S), sealed((size_t)S);
    std::vector<char> wanted((size_t)S, 1);
    for (int64_t i = 0; i < S; ++i) { n_after[(size_t)i] = s[i]->b.n + add[(size_t)i]; sealed[(size_t)i] = s[i]->b.sealed; }
    std::vector<PackRange> ranges;
    int64_t total = 0;
    if ((rc = group_ranges(c, S, n_after.data(), sealed.data(), wanted.data(), false, ranges, &total, who))) return rc;
    if (pushed == 0) return SD_OK;

    const double t0 = now_ms();
    clear_stage_ms(c);
    // growth before the first kernel: a failed allocation leaves every stream what it was
    HipDev dev{c};
    std::vector<char> busy((size_t)S, 0);
    for (const PackRange& r : ranges) busy[(size_t)r.owner] = 1;
    for (int64_t i = 0; i < S; ++i) {
        if ((add[(size_t)i] > 0 || busy[(size_t)i]) && (rc = book_reserve_group(dev, s[i]->b, add[(size_t)i]))) return rc;
        if (s[i]->r.in_sr && n[i] > 0 && (rc = rate_reserve(dev, s[i]->r, n[i]))) return rc;
    }
    // the rows of the one k_resample_jobs launch: every stream whose piece makes an output final, whatever its rate (the tap tables are cached)
    std::vector<ResampleJob> jobs;
    for (int64_t i = 0; i < S; ++i) {
        if (!s[i]->r.in_sr || add[(size_t)i] <= 0) continue;
        const float* taps = nullptr;
        if ((rc = resample_taps(c, s[i]->r.in_sr, SD_SAMPLE_RATE, s[i]->r.p, &taps))) return rc;
        jobs.push_back(rate_job(s[i]->r, rated[(size_t)i], s[i]->b.tail_now() + s[i]->b.tail_len(), taps, SD_TAIL_PAD));
    }

    // the samples of all streams: host ones uploaded back to back (each placed so that it is as aligned as its place in the tail), one conversion launch;
    // the piece of a stream with an input rate goes behind the inputs it holds, with no padding
    if (audio) {      // the frames of all streams: one upload per distinct source, one table, ONE k_group_ingest launch
        std::vector<float*> dst((size_t)S, nullptr);
        std::vector<int64_t> room((size_t)S, 0);
        for (int64_t i = 0; i < S; ++i) {
            if (n[i] <= 0) continue;
            StreamBook& b = s[i]->b;
            const RateBook& r = s[i]->r;
            dst[(size_t)i] = r.in_sr ? r.buf[r.cur] + r.held() : b.tail_now() + b.tail_len();
            room[(size_t)i] = r.in_sr ? n[i] : b.tail_cap[b.cur] - b.tail_len();
        }
        StreamIngestPlan plan;
        stream_ingest_plan(pieces.data(), dst.data(), room.data(), S, kind == SD_AUDIO_HOST, plan);
        if ((rc = ingest_rows(c, plan, kind == SD_AUDIO_HOST))) return rc;
        return push_many_tail(c, s, S, jobs, rated, add, ranges, total, t0);
    }
    const size_t es = kind == SD_F32_HOST ? sizeof(float) : sizeof(int16_t);
    std::vector<GroupRow> rows;
    std::vector<size_t> off;
    size_t stage_len = 0;
    for (int64_t i = 0; i < S; ++i) {
        if (n[i] <= 0) continue;
        StreamBook& b = s[i]->b;
        const RateBook& r = s[i]->r;
        float* dst = r.in_sr ? r.buf[r.cur] + r.held() : b.tail_now() + b.tail_len();
        rows.push_back(GroupRow{src[i], dst, n[i], r.in_sr ? n[i] : b.tail_cap[b.cur] - b.tail_len()});
        const size_t head = (size_t)((16 - ((uintptr_t)dst & 15)) & 15) / 4;
        while ((stage_len + head) % 4 != 0) ++stage_len;
        off.push_back(stage_len);
        stage_len += (size_t)n[i];
    }
    WS(c, GroupRow, d_tab, "stg_tab", rows.size());
    if (kind != SD_PCM_DEV) {
        WS(c, char, stage, "stg_src", stage_len * es);
        for (size_t q = 0; q < rows.size(); ++q) {
            HIPCHK(c, hipMemcpyAsync(stage + off[q] * es, rows[q].src, (size_t)rows[q].len * es, hipMemcpyHostToDevice, c->stream));
            rows[q].src = stage + off[q] * es;
        }
    }
    HIPCHK(c, hipMemcpy(d_tab, rows.data(), rows.size() * sizeof(GroupRow), hipMemcpyHostToDevice));
    if ((rc = group_launch(c, 0, d_tab, rows, kind == SD_F32_HOST ? 1 : 0))) return rc;
    return push_many_tail(c, s, S, jobs, rated, add, ranges, total, t0);
}

int turns_many_impl(sd_ctx* c, sd_stream* const* s, int64_t S, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    const char* who = "sd_stream_turns_many";
    // refusals: nothing is touched
    if (!turns || !n_turns || !status) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
    int rc;
    if ((rc = group_check(c, s, S, who))) return rc;
    if (!c->dump_dir.empty()) SD_FAIL(c, SD_ERR_ARG, "%s: the step files describe one whole-path inference; clear the dump directory", who);
    if ((rc = enrolled_refusal(c, SD_EMB_DIM, c->num_clusters, c->min_clusters, c->max_clusters))) return rc;
    std::vector<int64_t> n_now((size_t)S), sealed((size_t)S);
    std::vector<char> all((size_t)S, 1), stale((size_t)S, 0);
    for (int64_t i = 0; i < S; ++i) { n_now[(size_t)i] = s[i]->b.n; sealed[(size_t)i] = s[i]->b.sealed; }
    std::vector<PackRange> to_seal, to_infer;      // (to_seal: nothing unless an earlier push failed half way)
    int64_t seal_total = 0, total = 0;
    if ((rc = group_ranges(c, S, n_now.data(), sealed.data(), all.data(), false, to_seal, &seal_total, who))) return rc;
    for (int64_t i = 0; i < S; ++i) {
        const int64_t to = stream_sealed_chunks(s[i]->b.n);
        stale[(size_t)i] = (s[i]->b.pending_n != s[i]->b.n || to > s[i]->b.sealed) ? 1 : 0;
        sealed[(size_t)i] = std::max(to, s[i]->b.sealed);
    }
    if ((rc = group_ranges(c, S, n_now.data(), sealed.data(), stale.data(), true, to_infer, &total, who))) return rc;

    // rosters: a copy of each before the first update, put back if the call fails behind it; what the streams keep is committed at the end
    std::vector<sd_roster*> rosters, saved;
    for (int64_t i = 0; i < S; ++i) if (s[i]->roster && std::find(rosters.begin(), rosters.end(), s[i]->roster) == rosters.end()) rosters.push_back(s[i]->roster);
    auto drop_saved = [&]() { for (sd_roster* q : saved) roster_free(q); saved.clear(); };
    for (sd_roster* q : rosters) {
        sd_roster* copy = nullptr;
        if (roster_copy(q, &copy)) { drop_saved(); SD_FAIL(c, SD_ERR_NOMEM, "%s: out of host memory for the copy of a roster", who); }
        saved.push_back(copy);
    }
    std::vector<std::vector<int32_t>> kept((size_t)S);
    std::vector<char> named((size_t)S, 0);

    const double t0 = now_ms();
    clear_stage_ms(c);
    rc = finalize_jobs(c, S, turns, n_turns, status, [&](std::vector<FinalJob>& jobs) -> int {
        HipDev dev{c};
        for (const PackRange& r : to_seal) if (int e = book_reserve_group(dev, s[r.owner]->b, 0)) return e;
        for (const PackRange& r : to_infer) if (int e = book_reserve_group(dev, s[r.owner]->b, 0)) return e;
        if (int e = group_infer(c, s, to_seal, seal_total, false)) return e;
        if (int e = group_infer(c, s, to_infer, total, true)) return e;
        for (int64_t i = 0; i < S; ++i) jobs[(size_t)i] = FinalJob{s[i]->b.seg, s[i]->b.emb, sd_num_chunks(s[i]->b.n, nullptr), s[i]->b.n};
        return SD_OK;
    }, [&](int64_t i, sd_turn* t, int64_t nt) -> int {
        if (!s[i]->roster) return SD_OK;
        named[(size_t)i] = 1;
        return name_turns(s[i], t, nt, kept[(size_t)i]);
    });
    if (rc) {
        for (size_t q = 0; q < rosters.size(); ++q) roster_swap_tables(rosters[q], saved[q]);
        drop_saved();
        return rc;
    }
    drop_saved();
    for (int64_t i = 0; i < S; ++i) if (named[(size_t)i]) { s[i]->kept.swap(kept[(size_t)i]); s[i]->kept_origin = s[i]->b.origin; s[i]->has_kept = true; }
    c->stage_ms[3] = now_ms() - t0;
    return SD_OK;
}

// SD_ERR_HIP in the middle of a group call: nobody can vouch for any tail or cache of the call
int group_guard(sd_stream* const* s, int64_t S, int rc)
{
    if (rc == SD_ERR_HIP && !s[0]->c->stream_intact) for (int64_t i = 0; i < S; ++i) s[i]->dead = true;
    s[0]->c->stream_intact = false;
    return rc;
}
bool group_list_ok(sd_stream* const* s, int64_t S)
{
    if (!s || S < 1) return false;
    for (int64_t i = 0; i < S; ++i) if (!s[i]) return false;
    return true;
}
}

extern "C" int sd_stream_push_many(sd_stream* const* s, const int16_t* const* h_pcm, const int64_t* n, int64_t S)
{
    if (!group_list_ok(s, S)) return SD_ERR_ARG;
    ENTER(s[0]->c);
    return group_guard(s, S, push_many_impl(s[0]->c, s, (const void* const*)h_pcm, n, S, SD_PCM_HOST, "sd_stream_push_many"));
}
extern "C" int sd_stream_push_many_dev(sd_stream* const* s, const int16_t* const* d_pcm, const int64_t* n, int64_t S)
{
    if (!group_list_ok(s, S)) return SD_ERR_ARG;
    ENTER(s[0]->c);
    return group_guard(s, S, push_many_impl(s[0]->c, s, (const void* const*)d_pcm, n, S, SD_PCM_DEV, "sd_stream_push_many_dev"));
}
extern "C" int sd_stream_push_many_f32(sd_stream* const* s, const float* const* h_wav, const int64_t* n, int64_t S)
{
    if (!group_list_ok(s, S)) return SD_ERR_ARG;
    ENTER(s[0]->c);
    return group_guard(s, S, push_many_impl(s[0]->c, s, (const void* const*)h_wav, n, S, SD_F32_HOST, "sd_stream_push_many_f32"));
}
extern "C" int sd_stream_turns_many(sd_stream* const* s, int64_t S, sd_turn** turns, int64_t* n_turns, int32_t* status)
{
    if (!group_list_ok(s, S)) return SD_ERR_ARG;
    ENTER(s[0]->c);
    return group_guard(s, S, turns_many_impl(s[0]->c, s, S, turns, n_turns, status));
}

extern "C" int64_t sd_stream_sealed_chunks(int64_t n_samples) { return stream_sealed_chunks(n_samples); }

extern "C" int sd_stream_open(sd_ctx* c, sd_stream** out)
{
    ENTER(c);
    if (!out) SD_FAIL(c, SD_ERR_ARG, "sd_stream_open: bad argument");
    sd_stream* s = new sd_stream();
    s->c = c;
    s->ecapa_precision = c->ecapa_precision;
    s->seg_precision = seg_prec(c);
    c->streams.push_back(s);
    *out = s;
    return SD_OK;
}

extern "C" void sd_stream_close(sd_stream* s)
{
    if (!s) return;
    sd_ctx* c = s->c;
    (void)hipSetDevice(c->device);
    HipDev dev{c};
    book_release(dev, s->b);
    rate_release(dev, s->r);
    if (s->roster) s->roster->attached -= 1;
    c->streams.erase(std::remove(c->streams.begin(), c->streams.end(), s), c->streams.end());
    delete s;
}

extern "C" int sd_stream_push(sd_stream* s, const int16_t* h_pcm, int64_t n)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, h_pcm, n, SD_PCM_HOST, "sd_stream_push"));
}
extern "C" int sd_stream_push_dev(sd_stream* s, const int16_t* d_pcm, int64_t n)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, d_pcm, n, SD_PCM_DEV, "sd_stream_push_dev"));
}
extern "C" int sd_stream_push_f32(sd_stream* s, const float* h_wav, int64_t n)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, h_wav, n, SD_F32_HOST, "sd_stream_push_f32"));
}
extern "C" int sd_stream_turns(sd_stream* s, sd_turn** turns, int64_t* n_turns)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, turns_impl(s, turns, n_turns));
}
extern "C" int sd_stream_info(const sd_stream* s, int64_t* n_samples, int64_t* chunks_sealed, int64_t* chunks_total)
{
    if (!s) return SD_ERR_ARG;
    if (n_samples) *n_samples = s->b.n;
    if (chunks_sealed) *chunks_sealed = s->b.sealed;
    if (chunks_total) *chunks_total = sd_num_chunks(s->b.n, nullptr);
    return SD_OK;
}
extern "C" int sd_stream_forget(sd_stream* s, int64_t keep_blocks)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, forget_impl(s, keep_blocks, "sd_stream_forget"));
}
extern "C" int sd_stream_set_window(sd_stream* s, int64_t keep_blocks)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    sd_ctx* c = s->c;
    if (keep_blocks < -1) SD_FAIL(c, SD_ERR_ARG, "sd_stream_set_window: keep_blocks must be -1 (no window) or >= 0");
    if (int rc = check_call(s, "sd_stream_set_window")) return rc;
    s->window = keep_blocks;
    return SD_OK;
}
extern "C" int sd_stream_set_roster(sd_stream* s, sd_roster* r)
{
    if (!s) return SD_ERR_ARG;
    sd_ctx* c = s->c;
    c->err.clear();
    if (r && r->d != SD_EMB_DIM) SD_FAIL(c, SD_ERR_ARG, "sd_stream_set_roster: the roster's entries have %d dimensions, a stream's centroids %d", r->d, SD_EMB_DIM);
    if (r == s->roster) return SD_OK;
    if (s->roster) s->roster->attached -= 1;
    if (r) r->attached += 1;
    s->roster = r;
    s->kept.clear(); s->kept_origin = 0; s->has_kept = false;      // what the stream kept were ids of the other roster
    return SD_OK;
}
extern "C" int sd_stream_origin(const sd_stream* s, int64_t* first_sample)
{
    if (!s || !first_sample) return SD_ERR_ARG;
    *first_sample = s->b.origin;
    return SD_OK;
}
extern "C" int sd_stream_read(sd_stream* s, int64_t chunk_lo, int64_t chunk_hi, float* h_seg, float* h_emb)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, read_impl(s, chunk_lo, chunk_hi, h_seg, h_emb));
}

// ---- a stream in its own encoding (sdhip.h, "streams in their own encoding"; stream_ingest_plan.h; stream_ingest.hip: k_group_ingest)
extern "C" int sd_stream_set_input_format(sd_stream* s, int32_t encoding, int32_t channels, int32_t channel)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, set_format_impl(s, encoding, channels, channel));
}
extern "C" int sd_stream_input_format(const sd_stream* s, int32_t* encoding, int32_t* channels, int32_t* channel, int32_t* is_set)
{
    if (!s) return SD_ERR_ARG;
    if (encoding) *encoding = s->f.enc;
    if (channels) *channels = s->f.channels;
    if (channel) *channel = s->f.channel;
    if (is_set) *is_set = s->f.set ? 1 : 0;
    return SD_OK;
}
extern "C" int sd_stream_push_audio(sd_stream* s, const void* h_data, int64_t frames)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, h_data, frames, SD_AUDIO_HOST, "sd_stream_push_audio"));
}
extern "C" int sd_stream_push_audio_dev(sd_stream* s, const void* d_data, int64_t frames)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, d_data, frames, SD_AUDIO_DEV, "sd_stream_push_audio_dev"));
}
extern "C" int sd_stream_push_many_audio(sd_stream* const* s, const void* const* h_data, const int64_t* frames, int64_t S)
{
    if (!group_list_ok(s, S)) return SD_ERR_ARG;
    ENTER(s[0]->c);
    return group_guard(s, S, push_many_impl(s[0]->c, s, h_data, frames, S, SD_AUDIO_HOST, "sd_stream_push_many_audio"));
}
extern "C" int sd_stream_push_many_audio_dev(sd_stream* const* s, const void* const* d_data, const int64_t* frames, int64_t S)
{
    if (!group_list_ok(s, S)) return SD_ERR_ARG;
    ENTER(s[0]->c);
    return group_guard(s, S, push_many_impl(s[0]->c, s, d_data, frames, S, SD_AUDIO_DEV, "sd_stream_push_many_audio_dev"));
}

// ---- a stream at another sample rate (sdhip.h, "streams at any sample rate"; resample_book.h; resample.hip: k_resample_jobs)
extern "C" int sd_stream_set_input_rate(sd_stream* s, int32_t in_sr)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, set_rate_impl(s, in_sr));
}
extern "C" int sd_stream_end_input(sd_stream* s)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, end_input_impl(s));
}
extern "C" int sd_stream_input_info(const sd_stream* s, int32_t* in_sr, int64_t* n_in, int64_t* n_final, int32_t* closed)
{
    if (!s) return SD_ERR_ARG;
    const bool plain = s->r.in_sr == 0;      // its inputs are its samples: all of them final at once, those in front of the window's origin included
    if (in_sr) *in_sr = plain ? SD_SAMPLE_RATE : s->r.in_sr;
    if (n_in) *n_in = plain ? s->b.origin + s->b.n : s->r.n_in;
    if (n_final) *n_final = plain ? s->b.origin + s->b.n : s->r.emitted;
    if (closed) *closed = s->r.closed ? 1 : 0;
    return SD_OK;
}
// test hook (sdhip_stream_test.h): the f32 samples the stream holds, from sample sealed * 8000 (counted from the origin) on
extern "C" int sd_test_stream_tail(sd_stream* s, float* h_out, int64_t cap, int64_t* n, int64_t* first_sample)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    sd_ctx* c = s->c;
    if (s->dead) SD_FAIL(c, SD_ERR_ARG, "sd_test_stream_tail: the stream is unusable after a HIP failure; close it");
    const int64_t len = s->b.tail_len();
    if (n) *n = len;
    if (first_sample) *first_sample = s->b.origin + s->b.sealed * SD_HOP;
    if (!h_out) return SD_OK;
    if (cap < len) SD_FAIL(c, SD_ERR_ARG, "sd_test_stream_tail: the buffer holds %lld samples, %lld needed", (long long)cap, (long long)len);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (len > 0) HIPCHK(c, hipMemcpy(h_out, s->b.tail_now(), (size_t)len * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}
