// The planner of sd_diarize_many_audio* (csrc/ingest_plan.h) and the reader sd_read_wav_audio (csrc/wav_file.h: wav_read_audio) for AddressSanitizer +
// UBSan.  CPU only; tools/sanitize/build_ingest.sh builds it.
//   ingest FILE...   -> per file "<file> audio rc=<code> n=<frames> sr=<rate> enc=<SD_ENC_*> ch=<channels> channel=<c> <hex of the data bytes>", then the
//   planner on seeded random descriptor lists -- every invariant of a plan is checked here, a violation prints "BAD ..." and exits 1 -- and on the
//   size limits of many_plan.h, one line each "limit <name> -> <refusal code> bad=<recording>", then "ingest ok" and exit 0
#include <cstdio>
#include <cstdlib>
#include "ingest_plan.h"
#include "wav_file.h"

static uint64_t lcg_state = 88172645463325252ull;
static uint64_t lcg() { lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull; return lcg_state >> 17; }
#define CHECK(cond, ...) do { if (!(cond)) { printf("BAD " __VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void check_plan(const std::vector<sd_audio>& a, int64_t cb, int round)
{
    IngestPlan p;
    const int rc = ingest_plan(a.data(), (int64_t)a.size(), cb, false, p);
    if (rc != INGEST_OK) { printf("round %d: refusal %d bad=%lld\n", round, rc, (long long)p.bad); return; }
    const size_t S = p.owner.size();
    CHECK(p.rows.size() == S + 1 && p.tile0.size() == S + 2 && p.src_off.size() == S && p.src_bytes.size() == S && p.rec.size() == a.size(), "sizes, round %d", round);
    int64_t end = 0, up = 0, span = 0, slots = 0;
    for (size_t k = 0; k < S; ++k) {
        const IngestRow& w = p.rows[k];
        const sd_audio& d = a[(size_t)p.owner[k]];
        const PackRange& q = p.rec[(size_t)p.owner[k]];
        CHECK(k == 0 || p.owner[k] > p.owner[k - 1], "list order, round %d", round);
        CHECK(w.len16 == ingest_len16(d) && w.len16 <= w.len && w.base == end && w.base % SD_HOP == 0 && w.len == q.slot() * (int64_t)SD_HOP && q.chunks > 0, "row %zu, round %d", k, round);
        CHECK(w.n == d.n && w.enc == d.encoding && w.channels == d.channels && w.channel == d.channel, "descriptor of row %zu, round %d", k, round);
        CHECK((d.sample_rate == SD_SAMPLE_RATE) == (w.L == w.M), "rate pair of row %zu, round %d", k, round);
        CHECK(p.tile0[k + 1] - p.tile0[k] == (w.len + RS_BLOCK - 1) / RS_BLOCK, "tiles of row %zu, round %d", k, round);
        CHECK(p.src_off[k] % 16 == 0 && p.src_off[k] == up && p.src_bytes[k] == ingest_src_bytes(d) && p.src_bytes[k] <= d.n * d.channels * ingest_elem_bytes(d.encoding), "upload of row %zu, round %d", k, round);
        up += (p.src_bytes[k] + 15) / 16 * 16;
        end = w.base + w.len; slots += q.slot();
        if (w.L != w.M) { const int64_t s = ((int64_t)(RS_BLOCK - 1) * w.M) / w.L + 2 * (int64_t)w.J + 3; if (s > span) span = s; CHECK((s + RS_BLOCK) * 4 <= 160 * 1024, "span of row %zu, round %d", k, round); }
    }
    size_t live = 0;
    for (const PackRange& q : p.rec) live += q.chunks > 0;
    const IngestRow& pad = p.rows[S];
    CHECK(live == S && up == p.upload_bytes && span == p.max_span && slots == p.total && end == p.total * (int64_t)SD_HOP, "totals, round %d", round);
    CHECK(pad.base == end && pad.len == SD_TAIL_PAD && pad.n == 0 && pad.len16 == 0 && !pad.src && p.tile0[S + 1] - p.tile0[S] == 2, "pad row, round %d", round);
    printf("round %d: %zu recordings, %zu rows, %lld chunks, %lld tiles, %lld bytes up, span %lld\n", round, a.size(), S, (long long)p.total, (long long)p.tile0.back(), (long long)p.upload_bytes, (long long)p.max_span);
}

static void limit(const char* name, std::vector<sd_audio> a, int64_t R = -1)
{
    IngestPlan p;
    const int rc = ingest_plan(a.empty() ? nullptr : a.data(), R < 0 ? (int64_t)a.size() : R, 4096, true, p);
    printf("limit %s -> %d bad=%lld\n", name, rc, (long long)p.bad);
}

int main(int argc, char** argv)
{
    for (int k = 1; k < argc; ++k) {
        sd_audio d{}; void* data = nullptr;
        const int rc = wav_read_audio(argv[k], &d, &data);
        printf("%s audio rc=%d n=%lld sr=%d enc=%d ch=%d channel=%d ", argv[k], rc, (long long)d.n, d.sample_rate, d.encoding, d.channels, d.channel);
        const size_t bytes = rc == SD_OK ? (size_t)d.n * d.channels * ingest_elem_bytes(d.encoding) : 0;
        for (size_t i = 0; i < bytes; ++i) printf("%02x", ((const unsigned char*)data)[i]);
        printf(bytes ? "\n" : "-\n");
        free(data);
    }
    const int32_t rates[] = {8000, 16000, 11025, 44100, 48000, 22050, 32000, 16001, 24000, 1, 7, 672000, 1680000, 2147483647};      // the last five: every fourth round
    static char byte;
    for (int round = 0; round < 200; ++round) {
        std::vector<sd_audio> a((size_t)(1 + lcg() % 40));
        for (sd_audio& d : a) {
            d.data = &byte;
            d.n = lcg() % 5 == 0 ? (int64_t)(lcg() % 3) : (int64_t)(lcg() % 3000000);
            d.sample_rate = rates[lcg() % (round % 4 == 0 ? 14 : 9)];
            d.encoding = (int32_t)(lcg() % 4);
            d.channels = 1 + (int32_t)(lcg() % 4);
            d.channel = (int32_t)(lcg() % (uint64_t)(d.channels + 1)) - 1;
            if (round % 17 == 16 && lcg() % 8 == 0) d.channel = d.channels;      // a bad descriptor now and then
        }
        check_plan(a, round % 3 == 0 ? 7 : 4096, round);
    }
    const int64_t big = SD_MANY_MAX_SAMPLES;
    static char b2;
    limit("null list", {});
    limit("R = 0", {sd_audio{&b2, 10, 16000, 0, 1, 0}}, 0);
    limit("R = 2^20 + 1", {sd_audio{&b2, 10, 16000, 0, 1, 0}}, ((int64_t)1 << 20) + 1);
    limit("n = 2^40 at 16 kHz", {sd_audio{&b2, big, 16000, SD_ENC_MULAW, 1, 0}});
    limit("n = 2^40 + 1", {sd_audio{&b2, big + 1, 16000, SD_ENC_MULAW, 1, 0}});
    limit("n = 2^40 at 1 Hz", {sd_audio{&b2, big, 1, SD_ENC_MULAW, 1, 0}});
    limit("n = 2^40 at 2^31 - 1 Hz", {sd_audio{&b2, big, 2147483647, SD_ENC_MULAW, 1, 0}});
    limit("n = 2^40 of 2^31 - 1 float channels", {sd_audio{&b2, big, 16000, SD_ENC_F32, 2147483647, -1}});
    limit("n = 2^40 int16 stereo", {sd_audio{&b2, big, 16000, SD_ENC_S16, 2, 1}});
    limit("null data", {sd_audio{&b2, 10, 16000, 0, 1, 0}, sd_audio{nullptr, 10, 16000, 0, 1, 0}});
    limit("null data, n = 0", {sd_audio{nullptr, 0, 8000, 2, 1, 0}});
    limit("SD_MANY_MAX_CHUNKS", {sd_audio{&b2, (int64_t)SD_HOP * (SD_MANY_MAX_CHUNKS - 40), 16000, 2, 1, 0}});
    limit("SD_MANY_MAX_CHUNKS + 1 slot", {sd_audio{&b2, (int64_t)SD_HOP * (SD_MANY_MAX_CHUNKS - 40), 16000, 2, 1, 0}, sd_audio{&b2, 100000, 16000, 2, 1, 0}});
    {
        std::vector<sd_audio> many((size_t)1 << 20, sd_audio{&b2, big, 16000, SD_ENC_MULAW, 1, 0});      // 2^20 recordings of 2^40 samples: every sum stays inside int64
        limit("2^20 recordings of 2^40 samples", many);
    }
    printf("ingest ok\n");
    return 0;
}
