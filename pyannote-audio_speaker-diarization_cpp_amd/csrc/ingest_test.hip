// ingest_test.hip -- the sd_test_many_ingest hook of k_many_ingest (sdhip_ingest_test.h), for tests/test_ingest_kernel.py.  Host code only, under the
// contract of input_test.hip's hooks: the caller's operands are laid out in guarded device buffers, the launch goes through the function the product
// calls (launch_many_ingest), the whole destination comes back.  It holds no kernel, restates no kernel logic and picks no grid; it checks that every
// index the kernel is DEFINED to follow stays inside the operand it was given, and that no two rows write the same place.
#include "common.h"
#include "ingest_plan.h"
#include "../../include/sdhip_ingest_test.h"
#include <algorithm>
#include <cstring>
#include <limits>

namespace {
const int64_t SLACK = 256;
const int64_t LIMIT = (int64_t)1 << 28;
}

extern "C" int sd_test_many_ingest(sd_ctx* c, const int64_t* rows, int64_t R, const void* src, int64_t src_bytes, int64_t dst_len, float canary, float* dst_out)
{
    if (!c || !rows || !dst_out) return SD_ERR_ARG;
    ENTER(c);
    if (R < 1 || R > (1 << 16) || src_bytes < 0 || src_bytes > LIMIT || (src_bytes > 0 && !src) || dst_len < 1 || dst_len > LIMIT)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_many_ingest: R %lld, src_bytes %lld, dst_len %lld", (long long)R, (long long)src_bytes, (long long)dst_len);
    std::vector<IngestRow> tab((size_t)R);
    std::vector<int64_t> tile0((size_t)R + 1, 0), at((size_t)R, 0), bytes((size_t)R, 0);
    std::vector<std::pair<int64_t, int64_t>> dst;
    std::vector<ResamplePlan> plans((size_t)R);
    int64_t max_span = 0, held = 0;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t* q = rows + 8 * r;
        const sd_audio a{nullptr, q[4], (int32_t)q[3], (int32_t)q[0], (int32_t)q[1], (int32_t)q[2]};
        const int64_t so = q[5], base = q[6], len = q[7];
        const int64_t len16 = (q[3] > 0x7fffffff || q[0] != a.encoding || q[1] != a.channels || q[2] != a.channel) ? -1 : ingest_len16(a);
        if (len16 < 0 || a.n > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_ingest: row %lld: bad descriptor", (long long)r);
        const int es = ingest_elem_bytes(a.encoding);
        const int64_t need = ingest_src_bytes(a);
        if (need < 0 || base < 0 || len < 1 || len > LIMIT || base + len > dst_len || len16 > len || so < -1 || (so < 0 && need > 0) || (so >= 0 && (so % es != 0 || so + need > src_bytes)))
            SD_FAIL(c, SD_ERR_ARG, "sd_test_many_ingest: row %lld leaves its operands", (long long)r);
        ResamplePlan& p = plans[(size_t)r];
        const bool direct = a.sample_rate == SD_SAMPLE_RATE;
        if (!direct) {
            int rc = resample_check(c, a.sample_rate, SD_SAMPLE_RATE, p);
            if (rc) return rc;
            if (ingest_rate_refusal(p)) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_ingest: row %lld: the rate pair's span does not fit the LDS", (long long)r);
            max_span = std::max(max_span, p.span);
        }
        tab[(size_t)r] = IngestRow{nullptr, a.n, len16, base, len, nullptr, direct ? 1 : (int32_t)p.L, direct ? 1 : (int32_t)p.M, direct ? 0 : p.J, a.encoding, a.channels, a.channel};
        tile0[(size_t)r + 1] = tile0[(size_t)r] + (len + RS_BLOCK - 1) / RS_BLOCK;
        dst.emplace_back(base, base + len);
        at[(size_t)r] = held; bytes[(size_t)r] = need;
        held += (need + SLACK * es + 15) / 16 * 16;
    }
    std::sort(dst.begin(), dst.end());
    for (size_t k = 1; k < dst.size(); ++k) if (dst[k].first < dst[k - 1].second) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_ingest: two rows share a destination");
    // every row's source with 256 guard elements behind it
    std::vector<unsigned char> h((size_t)std::max<int64_t>(held, 16), 0);
    for (int64_t r = 0; r < R; ++r) {
        unsigned char* p = h.data() + at[(size_t)r];
        if (bytes[(size_t)r]) memcpy(p, (const unsigned char*)src + rows[8 * r + 5], (size_t)bytes[(size_t)r]);
        unsigned char* g = p + bytes[(size_t)r];
        const int32_t enc = tab[(size_t)r].enc;
        for (int64_t i = 0; i < SLACK; ++i) {
            if (enc == SD_ENC_S16) { const int16_t v = 0x7fff; memcpy(g + 2 * i, &v, 2); }
            else if (enc == SD_ENC_F32) { const float v = std::numeric_limits<float>::quiet_NaN(); memcpy(g + 4 * i, &v, 4); }
            else g[i] = enc == SD_ENC_MULAW ? 0x80 : 0xaa;      // 32124 and 32256: the largest of each law
        }
    }
    WS(c, unsigned char, dS, "ti_src", h.size());
    HIPCHK(c, hipMemcpy(dS, h.data(), h.size(), hipMemcpyHostToDevice));
    std::vector<float> fillv((size_t)(dst_len + SLACK), canary);
    WS(c, float, dD, "ti_y", fillv.size());
    HIPCHK(c, hipMemcpy(dD, fillv.data(), fillv.size() * sizeof(float), hipMemcpyHostToDevice));
    for (int64_t r = 0; r < R; ++r) {
        IngestRow& w = tab[(size_t)r];
        if (bytes[(size_t)r]) w.src = dS + at[(size_t)r];
        if (w.L != w.M) { int rc = resample_taps(c, (int32_t)rows[8 * r + 3], SD_SAMPLE_RATE, plans[(size_t)r], &w.taps); if (rc) return rc; }
    }
    const std::vector<char> bytes_tab = many_ingest_table(tab, tile0);
    WS(c, char, d_tab, "ti_tab", bytes_tab.size());
    HIPCHK(c, hipMemcpy(d_tab, bytes_tab.data(), bytes_tab.size(), hipMemcpyHostToDevice));
    int rc = launch_many_ingest(c, d_tab, tab, tile0, max_span, dD, dst_len);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst_out, dD, fillv.size() * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}
