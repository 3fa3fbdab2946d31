// stream_ingest_test.hip -- the sd_test_group_ingest hook of k_group_ingest (sdhip_stream_ingest_test.h), for tests/test_stream_ingest_kernel.py.  Host
// code only, under the contract of input_test.hip's hooks: the caller's operands are laid out in guarded device buffers, the launch goes through the
// function the product calls (launch_group_ingest), the whole destination comes back.  It holds no kernel, restates no kernel logic and picks no grid;
// it checks that every index the kernel is DEFINED to follow stays inside the operand it was given, and that no two rows write the same place.
#include "common.h"
#include "stream_book.h"
#include "stream_ingest_plan.h"
#include "../../include/sdhip_stream_ingest_test.h"
#include <algorithm>
#include <cstring>
#include <limits>
#include <map>
#include <tuple>

namespace {
const int64_t SLACK = 256;
const int64_t LIMIT = (int64_t)1 << 28;
}

extern "C" int sd_test_group_ingest(sd_ctx* c, const int64_t* rows, int64_t R, const void* src, int64_t src_bytes, int64_t dst_len, float canary, float* dst_out)
{
    if (!c || !rows || !dst_out) return SD_ERR_ARG;
    ENTER(c);
    if (R < 1 || R > (1 << 16) || src_bytes < 0 || src_bytes > LIMIT || (src_bytes > 0 && !src) || dst_len < 1 || dst_len > LIMIT)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_group_ingest: R %lld, src_bytes %lld, dst_len %lld", (long long)R, (long long)src_bytes, (long long)dst_len);
    struct Source { int64_t so, bytes, at; int32_t enc; };
    std::vector<Source> sources;
    std::map<std::tuple<int64_t, int64_t, int64_t, int64_t>, size_t> seen;      // (src_off, n, encoding, channels) -> its source
    std::vector<size_t> of((size_t)R);
    std::vector<StreamIngestRow> tab((size_t)R);
    std::vector<std::pair<int64_t, int64_t>> dst;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t* q = rows + 7 * r;
        const int64_t n = q[3], so = q[4], dof = q[5], room = q[6];
        if (q[0] < 0 || q[0] > 3 || q[1] < 1 || q[1] > 0x7fffffff || q[2] < -1 || q[2] >= q[1] || !stream_format_ok((int32_t)q[0], (int32_t)q[1], (int32_t)q[2]) || n < 0 || n > LIMIT)
            SD_FAIL(c, SD_ERR_ARG, "sd_test_group_ingest: row %lld: bad format or length", (long long)r);
        StreamPiece p{nullptr, n, StreamFormat{(int32_t)q[0], (int32_t)q[1], (int32_t)q[2], true}};
        const int es = ingest_elem_bytes(p.f.enc);
        const int64_t need = stream_piece_bytes(p);
        if (need < 0 || so < 0 || so % es != 0 || so + need > src_bytes || dof < 0 || room < 0 || dof + room > dst_len)
            SD_FAIL(c, SD_ERR_ARG, "sd_test_group_ingest: row %lld leaves its operands", (long long)r);
        dst.emplace_back(dof, dof + room);
        const auto key = std::make_tuple(so, n, q[0], q[1]);
        auto it = seen.find(key);
        if (it == seen.end()) { it = seen.emplace(key, sources.size()).first; sources.push_back(Source{so, 0, 0, p.f.enc}); }
        Source& s = sources[it->second];
        s.bytes = std::max(s.bytes, need);
        of[(size_t)r] = it->second;
        tab[(size_t)r] = StreamIngestRow{nullptr, nullptr, n, room, p.f.enc, p.f.channels, p.f.channel, 0};
    }
    std::sort(dst.begin(), dst.end());
    for (size_t k = 1; k < dst.size(); ++k) if (dst[k].first < dst[k - 1].second) SD_FAIL(c, SD_ERR_ARG, "sd_test_group_ingest: two rows share a destination");
    // every distinct source on its own, as aligned as the caller's offset says, with 256 guard elements behind the last element the rule reads
    int64_t held = 0;
    for (Source& s : sources) {
        s.at = held + s.so % 16;
        held = (s.at + s.bytes + SLACK * ingest_elem_bytes(s.enc) + 15) / 16 * 16;
    }
    std::vector<unsigned char> h((size_t)std::max<int64_t>(held, 16), 0);
    for (const Source& s : sources) {
        unsigned char* g = h.data() + s.at;
        if (s.bytes) memcpy(g, (const unsigned char*)src + s.so, (size_t)s.bytes);
        g += s.bytes;
        for (int64_t i = 0; i < SLACK; ++i) {
            if (s.enc == SD_ENC_S16) { const int16_t v = 0x7fff; memcpy(g + 2 * i, &v, 2); }
            else if (s.enc == SD_ENC_F32) { const float v = std::numeric_limits<float>::quiet_NaN(); memcpy(g + 4 * i, &v, 4); }
            else g[i] = s.enc == SD_ENC_MULAW ? 0x80 : 0xaa;      // 32124 and 32256: the largest of each law
        }
    }
    WS(c, unsigned char, dS, "ti_src", h.size());
    HIPCHK(c, hipMemcpy(dS, h.data(), h.size(), hipMemcpyHostToDevice));
    std::vector<float> fillv((size_t)(dst_len + SLACK), canary);
    WS(c, float, dD, "ti_y", fillv.size());
    HIPCHK(c, hipMemcpy(dD, fillv.data(), fillv.size() * sizeof(float), hipMemcpyHostToDevice));
    for (int64_t r = 0; r < R; ++r) {
        tab[(size_t)r].src = dS + sources[of[(size_t)r]].at;
        tab[(size_t)r].dst = dD + rows[7 * r + 5];
    }
    WS(c, StreamIngestRow, d_tab, "ti_tab", R);
    HIPCHK(c, hipMemcpy(d_tab, tab.data(), (size_t)R * sizeof(StreamIngestRow), hipMemcpyHostToDevice));
    int rc = launch_group_ingest(c, d_tab, tab, SD_TAIL_PAD);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(dst_out, dD, fillv.size() * sizeof(float), hipMemcpyDeviceToHost));
    return SD_OK;
}
