// stream_ingest_main.cpp -- the planner of sd_stream_push_audio* / sd_stream_push_many_audio* (csrc/stream_ingest_plan.h) alone, as a stand-alone
// program under AddressSanitizer + UBSan (build_stream_ingest.sh); tests/test_stream_audio_cpu.py reads its lines.  Named cases print what the planner
// made of them; 300 random tables are compared against a naive second implementation in this file (the bytes of a piece by walking its frames, the
// classes by a linear search, the offsets by stepping a byte at a time); any disagreement prints a line with BAD.  Ends with "stream ingest ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include "stream_ingest_plan.h"

alignas(64) static float g_dst[1 << 12];
alignas(64) static unsigned char g_src[1 << 12];

static StreamFormat fmt(int32_t enc, int32_t channels, int32_t channel) { StreamFormat f; f.enc = enc; f.channels = channels; f.channel = channel; f.set = true; return f; }

static void show(const char* name, const std::vector<StreamPiece>& p, const std::vector<float*>& dst, const std::vector<int64_t>& room, bool host)
{
    StreamIngestPlan plan;
    stream_ingest_plan(p.data(), dst.data(), room.data(), (int64_t)p.size(), host, plan);
    printf("case %s -> rows=%zu uploads=%zu total=%lld", name, plan.rows.size(), plan.up_src.size(), (long long)plan.upload_bytes);
    for (size_t q = 0; q < plan.rows.size(); ++q) printf(" | cls=%lld len=%lld room=%lld ch=%d", (long long)plan.cls[q], (long long)plan.rows[q].len, (long long)plan.rows[q].room, plan.rows[q].channel);
    for (size_t u = 0; u < plan.up_src.size(); ++u) printf(" | off=%lld bytes=%lld", (long long)plan.up_off[u], (long long)plan.up_bytes[u]);
    printf("\n");
}

static void refusal(const char* name, const std::vector<StreamPiece>& p, bool dev)
{
    int64_t bad = -7;
    const int e = stream_ingest_check(p.data(), (int64_t)p.size(), dev, &bad);
    printf("refusal %s -> %d bad=%lld\n", name, e, (long long)bad);
}

// ---- the naive second implementation
static int64_t naive_bytes(const StreamPiece& p)
{
    int64_t last = -1;      // the largest element index a frame reads
    for (int64_t i = 0; i < p.frames; ++i)
        for (int q = 0; q < p.f.channels; ++q)
            if (p.f.channel < 0 || p.f.channel == q) { const int64_t e = i * p.f.channels + q; if (e > last) last = e; }
    const int es = p.f.enc == SD_ENC_S16 ? 2 : p.f.enc == SD_ENC_F32 ? 4 : 1;
    return (last + 1) * es;
}

static bool random_round(std::mt19937_64& rng, int round)
{
    const int S = 1 + (int)(rng() % 12);
    std::vector<StreamPiece> p;
    std::vector<float*> dst;
    std::vector<int64_t> room;
    for (int i = 0; i < S; ++i) {
        const int32_t enc = (int32_t)(rng() % 4), channels = 1 + (int32_t)(rng() % 4);
        const int32_t channel = (int32_t)(rng() % (uint64_t)(channels + 1)) - 1;
        const int64_t frames = rng() % 4 == 0 ? 0 : 1 + (int64_t)(rng() % 40);
        const void* data = g_src + 4 * (rng() % 3);      // few pointers: rows meet
        StreamPiece q{data, frames, fmt(enc, channels, channel)};
        if (i > 0 && rng() % 3 == 0) { q = p[(size_t)(rng() % (uint64_t)i)]; q.f.channel = (int32_t)(rng() % (uint64_t)(q.f.channels + 1)) - 1; }      // another leg of an earlier row
        p.push_back(q);
        dst.push_back(g_dst + 64 * i + (int)(rng() % 4));
        room.push_back(frames + (int64_t)(rng() % 600));
    }
    StreamIngestPlan plan;
    stream_ingest_plan(p.data(), dst.data(), room.data(), S, true, plan);
    // naive: rows, classes by linear search, bytes as the largest among the rows of a class, offsets a byte at a time
    struct Up { const void* d; int64_t n; int32_t enc, ch; int64_t bytes; size_t first_row; };
    std::vector<Up> ups;
    std::vector<int64_t> cls, owner;
    for (int i = 0; i < S; ++i) {
        if (p[(size_t)i].frames <= 0) continue;
        const StreamPiece& q = p[(size_t)i];
        size_t u = 0;
        for (; u < ups.size(); ++u) if (ups[u].d == q.data && ups[u].n == q.frames && ups[u].enc == q.f.enc && ups[u].ch == q.f.channels) break;
        if (u == ups.size()) ups.push_back(Up{q.data, q.frames, q.f.enc, q.f.channels, 0, owner.size()});
        if (naive_bytes(q) > ups[u].bytes) ups[u].bytes = naive_bytes(q);
        cls.push_back((int64_t)u);
        owner.push_back(i);
    }
    bool ok = plan.rows.size() == owner.size() && plan.cls == cls && plan.up_src.size() == ups.size();
    int64_t at = 0;
    for (size_t u = 0; ok && u < ups.size(); ++u) {
        const StreamPiece& q = p[(size_t)owner[ups[u].first_row]];
        const int es = q.f.enc == SD_ENC_S16 ? 2 : q.f.enc == SD_ENC_F32 ? 4 : 1;
        int64_t head = 0;
        while (((uintptr_t)(dst[(size_t)owner[ups[u].first_row]] + head) & 15) != 0) ++head;
        while ((at + head * es * q.f.channels) % 16 != 0) ++at;
        ok = plan.up_off[u] == at && plan.up_bytes[u] == ups[u].bytes && plan.up_src[u] == ups[u].d && at % es == 0;
        at += ups[u].bytes;
    }
    ok = ok && plan.upload_bytes == at;
    for (size_t q = 0; ok && q < plan.rows.size(); ++q) {
        const StreamIngestRow& w = plan.rows[q];
        const StreamPiece& s = p[(size_t)owner[q]];
        ok = w.src == nullptr && w.dst == dst[(size_t)owner[q]] && w.len == s.frames && w.room == room[(size_t)owner[q]] && w.enc == s.f.enc && w.channels == s.f.channels && w.channel == s.f.channel;
    }
    // no two uploads overlap
    for (size_t u = 1; ok && u < plan.up_off.size(); ++u) ok = plan.up_off[u] >= plan.up_off[u - 1] + plan.up_bytes[u - 1];
    printf("round %d: %d streams, %zu rows, %zu uploads, %lld bytes%s\n", round, S, plan.rows.size(), plan.up_src.size(), (long long)plan.upload_bytes, ok ? "" : " BAD");
    return ok;
}

int main()
{
    const void* A = g_src;
    const void* B = g_src + 64;
    // the two legs of one stereo call: one upload, counted once
    show("two legs", {{A, 1000, fmt(SD_ENC_MULAW, 2, 0)}, {A, 1000, fmt(SD_ENC_MULAW, 2, 1)}}, {g_dst, g_dst + 2048}, {1512, 1512}, true);
    show("two legs, the later one first", {{A, 1000, fmt(SD_ENC_MULAW, 2, 1)}, {A, 1000, fmt(SD_ENC_MULAW, 2, 0)}}, {g_dst, g_dst + 2048}, {1512, 1512}, true);
    show("same pointer, other frames", {{A, 1000, fmt(SD_ENC_MULAW, 2, 0)}, {A, 999, fmt(SD_ENC_MULAW, 2, 1)}}, {g_dst, g_dst + 2048}, {1512, 1511}, true);
    show("same pointer, other channels", {{A, 1000, fmt(SD_ENC_MULAW, 2, 0)}, {A, 1000, fmt(SD_ENC_MULAW, 1, 0)}}, {g_dst, g_dst + 2048}, {1512, 1512}, true);
    show("same pointer, other encoding", {{A, 1000, fmt(SD_ENC_MULAW, 2, 0)}, {A, 1000, fmt(SD_ENC_ALAW, 2, 0)}}, {g_dst, g_dst + 2048}, {1512, 1512}, true);
    show("other pointer", {{A, 1000, fmt(SD_ENC_MULAW, 2, 0)}, {B, 1000, fmt(SD_ENC_MULAW, 2, 1)}}, {g_dst, g_dst + 2048}, {1512, 1512}, true);
    // only the bytes the rule reads: channel 0 of 3 stops two elements early; legs 0 and 1 of 3 take the larger count; the mean takes all
    show("channel 0 of 3, int16", {{A, 10, fmt(SD_ENC_S16, 3, 0)}}, {g_dst}, {522}, true);
    show("channels 0 and 1 of 3, int16", {{A, 10, fmt(SD_ENC_S16, 3, 0)}, {A, 10, fmt(SD_ENC_S16, 3, 1)}}, {g_dst, g_dst + 1024}, {522, 522}, true);
    show("mean of 3, float", {{A, 10, fmt(SD_ENC_F32, 3, -1)}}, {g_dst}, {522}, true);
    // offsets congruent to the destination's head: a tail that ends 1, 2, 3 floats behind a boundary has 3, 2, 1 floats in front of the next
    show("heads 0 3 2 1, mono mu-law", {{A, 5, fmt(SD_ENC_MULAW, 1, 0)}, {g_src + 1, 5, fmt(SD_ENC_MULAW, 1, 0)}, {g_src + 2, 5, fmt(SD_ENC_MULAW, 1, 0)}, {g_src + 3, 5, fmt(SD_ENC_MULAW, 1, 0)}},
         {g_dst, g_dst + 65, g_dst + 130, g_dst + 195}, {517, 517, 517, 517}, true);
    show("heads 3 1, stereo int16", {{A, 5, fmt(SD_ENC_S16, 2, 1)}, {B, 7, fmt(SD_ENC_S16, 2, -1)}}, {g_dst + 1, g_dst + 67}, {517, 519}, true);
    // frames == 0: no row and no upload, with any pointer, on a stream without a format too
    show("frames 0", {{nullptr, 0, fmt(SD_ENC_S16, 1, 0)}, {A, 8, fmt(SD_ENC_ALAW, 1, 0)}, {A, 0, StreamFormat()}}, {nullptr, g_dst, nullptr}, {0, 8, 0}, true);
    show("nothing at all", {{nullptr, 0, fmt(SD_ENC_S16, 1, 0)}}, {nullptr}, {0}, true);
    // the device form: the rows read the callers' pointers, nothing goes up
    show("device form", {{A, 1000, fmt(SD_ENC_MULAW, 2, 0)}, {A, 1000, fmt(SD_ENC_MULAW, 2, 1)}}, {g_dst, g_dst + 2048}, {1512, 1512}, false);

    refusal("fine", {{A, 10, fmt(SD_ENC_S16, 1, 0)}, {nullptr, 0, StreamFormat()}}, false);
    refusal("frames < 0", {{A, 10, fmt(SD_ENC_S16, 1, 0)}, {A, -1, fmt(SD_ENC_S16, 1, 0)}}, false);
    refusal("frames = 2^40", {{A, (int64_t)1 << 40, fmt(SD_ENC_MULAW, 1, 0)}}, false);
    refusal("frames = 2^40 + 1", {{A, 10, fmt(SD_ENC_S16, 1, 0)}, {A, 10, fmt(SD_ENC_S16, 1, 0)}, {A, ((int64_t)1 << 40) + 1, fmt(SD_ENC_MULAW, 1, 0)}}, false);
    refusal("no format", {{A, 10, fmt(SD_ENC_S16, 1, 0)}, {A, 1, StreamFormat()}}, false);
    refusal("null data", {{nullptr, 3, fmt(SD_ENC_F32, 1, 0)}}, false);
    refusal("bytes = 2^42", {{A, (int64_t)1 << 40, fmt(SD_ENC_F32, 1, 0)}}, false);
    refusal("bytes = 2^42 + 4", {{A, 10, fmt(SD_ENC_S16, 1, 0)}, {A, ((int64_t)1 << 39) + 1, fmt(SD_ENC_S16, 4, -1)}}, false);
    refusal("bytes of channel 0 of 4 = 2^42 - 6", {{A, (int64_t)1 << 39, fmt(SD_ENC_S16, 4, 0)}}, false);
    refusal("2^40 frames of 2^31 - 1 float channels", {{A, (int64_t)1 << 40, fmt(SD_ENC_F32, 0x7fffffff, -1)}}, false);
    refusal("odd int16 pointer, host form", {{g_src + 1, 10, fmt(SD_ENC_S16, 1, 0)}}, false);
    refusal("odd int16 pointer, device form", {{A, 10, fmt(SD_ENC_S16, 1, 0)}, {g_src + 1, 10, fmt(SD_ENC_S16, 1, 0)}}, true);
    refusal("float pointer + 2, device form", {{g_src + 2, 10, fmt(SD_ENC_F32, 2, -1)}}, true);
    refusal("odd G.711 pointer, device form", {{g_src + 1, 10, fmt(SD_ENC_ALAW, 2, 1)}}, true);

    std::mt19937_64 rng(20240607);
    bool ok = true;
    for (int k = 0; k < 300; ++k) ok = random_round(rng, k) && ok;
    if (!ok) { printf("BAD: a random round disagrees\n"); return 1; }
    printf("stream ingest ok\n");
    return 0;
}
