// stream.hip -- sd_stream_*: incremental diarization of a recording that is still growing.  Replaces calling speakerDiarization()
// (sd.cpp:2937-3234) again on everything heard so far: a stream keeps the scores and embeddings of the chunks that can never change
// again (stream_book.h: blocks of 32 chunks whose every chunk ends in front of the last sample), the audio behind them as f32 on the
// device, and at sd_stream_turns infers only the chunks behind the sealed part before the usual finalize.  The networks run through
// shard_infer on sub-ranges (pipeline.cpp); the device code here is the tail's compaction (16-bit pushes are appended by k_pcm_to_f32).
#include "common.h"
#include "stream_book.h"
#include <algorithm>

static_assert(SD_TAIL_PAD == SD_WAV_PAD, "the tail's padding is what DevWav::padded promises");

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

struct sd_stream {
    sd_ctx* c = nullptr;
    StreamBook b;
    int ecapa_precision = 0, seg_precision = 0;      // fixed at sd_stream_open: a cache of mixed precision is nobody's answer
    bool dead = false;                               // after SD_ERR_HIP: every call but sd_stream_close is refused
};

namespace {
// the device operations of stream_book.h on the stream's context; copies are ordered on the context's stream
struct HipDev {
    sd_ctx* c;
    int alloc(void** p, size_t bytes) {
        if (hipMalloc(p, bytes ? bytes : 16) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; SD_FAIL(c, SD_ERR_HIP, "hipMalloc of %zu bytes for a stream failed", bytes); }
        return SD_OK;
    }
    void release(void* p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(p); }
    int copy(void* dst, const void* src, size_t bytes) {
        HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
        return SD_OK;
    }
    int move_tail(float* dst, const float* src, int64_t len) {
        hipLaunchKernelGGL(k_tail_move, GRID1((len + SD_TAIL_PAD + 3) / 4), 0, c->stream, src, dst, len);
        KCHECK(c);
        return SD_OK;
    }
};

enum { PUSH_PCM_HOST, PUSH_PCM_DEV, PUSH_F32_HOST };

// chunks of a PyanNet batch up to which its dense layers (LSTM layer 0's input projection, the two linear layers) take k_skinny_gemm, not the
// 128 x 128 tile (common.h: SD_SKINNY_MAX_ROWS; 13); the two sum K in different orders, so a chunk's last bits say which one its batch took
#define SD_SEG_SKINNY_CHUNKS (SD_SKINNY_MAX_ROWS / SD_FRAMES)

// The segmentation step of the pending range [lo, hi), lo = sealed.  The whole path computes these chunks in a batch that starts at a multiple of
// seg_batch_chunks; where that batch is past the skinny limit and the pending one alone is not, the pending chunks run in a batch padded to 14 chunks:
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
    const int64_t cb = c->seg_batch_chunks;
    const int64_t whole = (cb >= SD_SEAL_CHUNKS && cb % SD_SEAL_CHUNKS == 0) ? full_hi - cb * (lo / cb) : mine;      // (a tuning value of seg_batch_chunks that cuts blocks: no promise)
    if (mine <= 0 || mine > SD_SEG_SKINNY_CHUNKS || whole <= SD_SEG_SKINNY_CHUNKS) return run_segment(c, tail, lo, hi, d_seg);
    const int64_t pad_hi = lo + SD_SEG_SKINNY_CHUNKS + 1;
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
int seal_blocks(sd_stream* s)
{
    StreamBook& b = s->b;
    const int64_t to = stream_sealed_chunks(b.n);
    if (to <= b.sealed) return SD_OK;
    HipDev dev{s->c};
    int rc;
    if ((rc = book_reserve_cache(dev, b, sd_num_chunks(b.n, nullptr)))) return rc;
    if ((rc = infer_rows(s, b.sealed, to, false))) return rc;
    return book_seal(dev, b, to);
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

int push_impl(sd_stream* s, const void* src, int64_t m, int kind, const char* who)
{
    sd_ctx* c = s->c;
    if (m < 0 || (m > 0 && !src)) SD_FAIL(c, SD_ERR_ARG, "%s: bad argument", who);
    if (int rc = check_call(s, who)) return rc;
    if (m == 0) return SD_OK;
    const double t0 = now_ms();
    clear_stage_ms(c);
    StreamBook& b = s->b;
    HipDev dev{c};
    int rc;
    if ((rc = book_reserve_tail(dev, b, m))) return rc;
    float* dst = b.tail_now() + b.tail_len();
    if (kind == PUSH_F32_HOST) {
        HIPCHK(c, hipMemcpyAsync(dst, src, (size_t)m * sizeof(float), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemsetAsync(dst + m, 0, SD_TAIL_PAD * sizeof(float), c->stream));
    } else {
        const int16_t* d_pcm = (const int16_t*)src;
        if (kind == PUSH_PCM_HOST) {
            WS(c, int16_t, stage, "st_pcm", m);
            HIPCHK(c, hipMemcpyAsync(stage, src, (size_t)m * sizeof(int16_t), hipMemcpyHostToDevice, c->stream));
            d_pcm = stage;
        }
        hipLaunchKernelGGL(k_pcm_to_f32, GRID1(m + SD_TAIL_PAD), 0, c->stream, d_pcm, dst, m);
        KCHECK(c);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));      // the caller's buffer may go
    b.n += m;
    if ((rc = seal_blocks(s))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_ms[3] = now_ms() - t0;
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
    if ((rc = seal_blocks(s))) return rc;            // (nothing to do unless an earlier push failed half way)
    if (b.pending_n != b.n) {
        HipDev dev{c};
        if ((rc = book_reserve_cache(dev, b, total))) return rc;
        if ((rc = infer_rows(s, b.sealed, total, true))) return rc;
        b.pending_n = b.n;
    }
    std::vector<sd_turn> v;
    if ((rc = finalize(c, b.seg, b.emb, total, b.n, v))) return rc;
    c->stage_ms[3] = now_ms() - t0;
    return turns_out(c, v, turns, n_turns);
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

// a HIP failure in the middle of a call leaves a tail or a cache nobody can vouch for
int guard(sd_stream* s, int rc) { if (rc == SD_ERR_HIP) s->dead = true; return rc; }
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
    c->streams.erase(std::remove(c->streams.begin(), c->streams.end(), s), c->streams.end());
    delete s;
}

extern "C" int sd_stream_push(sd_stream* s, const int16_t* h_pcm, int64_t n)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, h_pcm, n, PUSH_PCM_HOST, "sd_stream_push"));
}
extern "C" int sd_stream_push_dev(sd_stream* s, const int16_t* d_pcm, int64_t n)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, d_pcm, n, PUSH_PCM_DEV, "sd_stream_push_dev"));
}
extern "C" int sd_stream_push_f32(sd_stream* s, const float* h_wav, int64_t n)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, push_impl(s, h_wav, n, PUSH_F32_HOST, "sd_stream_push_f32"));
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
extern "C" int sd_stream_read(sd_stream* s, int64_t chunk_lo, int64_t chunk_hi, float* h_seg, float* h_emb)
{
    if (!s) return SD_ERR_ARG;
    ENTER(s->c);
    return guard(s, read_impl(s, chunk_lo, chunk_hi, h_seg, h_emb));
}
