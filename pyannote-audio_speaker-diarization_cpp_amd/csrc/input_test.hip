// input_test.hip -- the sd_test_* hooks of the kernels in front of the two networks (sdhip_test.h): resample.hip, the copy kernels of stream.hip, the two
// table kernels of many.hip and the weight forms of weights_gpu.hip, for tests/test_input_kernels.py.  Host code only.  A hook lays the caller's operands out
// in guarded device buffers, calls the function the product calls for the launch (resample_dev, resample_jobs, group_launch, launch_tail_move,
// launch_many_pack, launch_many_gap_masks, build_conv_w16 / build_conv_w16x) and downloads the whole outputs.  It holds no kernel, restates no kernel logic
// and picks no grid; what it does check is that every index a kernel is DEFINED to follow stays inside the operand it was given, and that no two rows of a
// table write the same place.
#include "common.h"
#include "stream_book.h"
#include "resample_book.h"
#include <algorithm>
#include <cstring>
#include <limits>

namespace {
const int64_t SLACK = 256;
const int64_t LIMIT = (int64_t)1 << 28;      // elements of one buffer of a case: a test case is small
const float FNAN = std::numeric_limits<float>::quiet_NaN();

// `front` elements of value g, n operand elements, `guard` elements of value g, in the named workspace; *d = the first operand element
template <class T> int up(sd_ctx* c, const char* name, const T* src, size_t n, size_t front, size_t guard, T g, T** d)
{
    std::vector<T> h(front + n + guard, g);
    if (n) memcpy(h.data() + front, src, n * sizeof(T));
    WS(c, T, p, name, h.size());
    HIPCHK(c, hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d = p + front;
    return SD_OK;
}
template <class T> int fill(sd_ctx* c, const char* name, size_t n, T v, T** d) { return up<T>(c, name, nullptr, 0, 0, n, v, d); }
template <class T> int down(sd_ctx* c, const T* d, size_t n, T* h)
{
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
    return SD_OK;
}
// do the intervals [lo, hi) of a table overlap?  (empty ones overlap nothing)
bool overlap(std::vector<std::pair<int64_t, int64_t>> iv)
{
    std::sort(iv.begin(), iv.end());
    int64_t end = std::numeric_limits<int64_t>::min();
    for (const auto& q : iv) {
        if (q.second <= q.first) continue;
        if (q.first < end) return true;
        end = q.second;
    }
    return false;
}
}
#define RUN(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)

extern "C" int sd_test_resample(sd_ctx* c, const float* x, int64_t n, int32_t in_sr, int32_t out_sr, int64_t n_out, float canary, float* y_out,
                                float* taps_out, int64_t taps_cap)
{
    if (!c || !x || !y_out) return SD_ERR_ARG;
    ENTER(c);
    const int64_t len = sd_resample_len(n, in_sr, out_sr);
    if (n_out < 0) n_out = len;
    if (n < 1 || n > LIMIT || len < 0 || n_out > len || n_out > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_resample: n %lld, %d -> %d Hz, n_out %lld of %lld", (long long)n, in_sr, out_sr, (long long)n_out, (long long)len);
    ResamplePlan p;
    RUN(resample_check(c, in_sr, out_sr, p));
    const int64_t ntap = (2 * (int64_t)p.J + 1) * p.L;
    if (taps_out && taps_cap != ntap) SD_FAIL(c, SD_ERR_ARG, "sd_test_resample: the tap table has %lld entries, the caller expects %lld", (long long)ntap, (long long)taps_cap);
    float* dX; float* dY;
    RUN(up<float>(c, "ti_x", x, (size_t)n, (size_t)SLACK, (size_t)SLACK, FNAN, &dX));
    RUN(fill<float>(c, "ti_y", (size_t)(n_out + SLACK), canary, &dY));
    RUN(resample_dev(c, dX, n, in_sr, out_sr, dY, n_out));
    RUN(down(c, dY, (size_t)(n_out + SLACK), y_out));
    if (taps_out) {
        const float* d_taps = nullptr;
        RUN(resample_taps(c, in_sr, out_sr, p, &d_taps));      // (cached by the launch above; built here where n_out = 0)
        RUN(down(c, d_taps, (size_t)ntap, taps_out));
    }
    return SD_OK;
}

extern "C" int sd_test_resample_jobs(sd_ctx* c, const sd_resample_case_row* rows, int64_t R, const float* x, int64_t x_len, int64_t arena, float canary,
                                     float* arena_out)
{
    if (!c || !rows || !x || !arena_out) return SD_ERR_ARG;
    ENTER(c);
    if (R < 1 || R > (1 << 16) || x_len < 0 || x_len > LIMIT || arena < 1 || arena > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_resample_jobs: R %lld, x_len %lld, arena %lld", (long long)R, (long long)x_len, (long long)arena);
    std::vector<ResamplePlan> plans((size_t)R);
    std::vector<std::pair<int64_t, int64_t>> dst;
    int64_t held_all = 0;
    for (int64_t r = 0; r < R; ++r) {
        const sd_resample_case_row& q = rows[r];
        RUN(resample_check(c, q.in_sr, SD_SAMPLE_RATE, plans[(size_t)r]));
        const ResamplePlan& p = plans[(size_t)r];
        const bool ok = q.first >= 0 && q.held >= 0 && q.n_limit >= 0 && q.n_limit <= q.first + q.held && q.m_first >= 0 && q.count >= 1 && q.pad >= 0 &&
                        q.x_off >= 0 && q.x_off + q.held <= x_len && q.dst_off >= 0 && q.dst_off + q.count + q.pad <= arena && q.m_first + q.count < ((int64_t)1 << 40);
        if (!ok) SD_FAIL(c, SD_ERR_ARG, "sd_test_resample_jobs: row %lld leaves its operands", (long long)r);
        // the first input that is summed lies in front of the inputs held: outside the kernel's contract (resample_book.h: need_first)
        if (q.first > 0 && (q.m_first * p.M) / p.L - p.J < q.first) SD_FAIL(c, SD_ERR_ARG, "sd_test_resample_jobs: row %lld reads in front of input %lld", (long long)r, (long long)q.first);
        dst.emplace_back(q.dst_off, q.dst_off + q.count + q.pad);
        held_all += q.held + 2 * SLACK;
    }
    if (overlap(dst)) SD_FAIL(c, SD_ERR_ARG, "sd_test_resample_jobs: two rows share a destination");
    // every row's inputs with 256 NaN in front of and behind them
    std::vector<float> h((size_t)held_all, FNAN);
    std::vector<int64_t> at((size_t)R);
    int64_t o = 0;
    for (int64_t r = 0; r < R; ++r) {
        at[(size_t)r] = o + SLACK;
        if (rows[r].held) memcpy(h.data() + o + SLACK, x + rows[r].x_off, (size_t)rows[r].held * sizeof(float));
        o += rows[r].held + 2 * SLACK;
    }
    float* dX; float* dA;
    RUN(up<float>(c, "ti_x", h.data(), h.size(), 0, 0, FNAN, &dX));
    RUN(fill<float>(c, "ti_y", (size_t)(arena + SLACK), canary, &dA));
    std::vector<ResampleJob> jobs((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        const sd_resample_case_row& q = rows[r];
        const ResamplePlan& p = plans[(size_t)r];
        const float* taps = nullptr;
        RUN(resample_taps(c, q.in_sr, SD_SAMPLE_RATE, p, &taps));
        jobs[(size_t)r] = ResampleJob{dX + at[(size_t)r], q.first, q.n_limit, dA + q.dst_off, q.m_first, q.count, taps, (int32_t)p.L, (int32_t)p.M, (int32_t)p.J, q.pad};
    }
    const int rc = resample_jobs(c, jobs.data(), R);
    if (rc && rc != SD_ERR_ARG) return rc;
    RUN(down(c, dA, (size_t)(arena + SLACK), arena_out));      // after a refusal too: the caller sees that nothing was written
    return rc;
}

extern "C" int sd_test_group_copy(sd_ctx* c, int which, int is_f32, const void* src, int64_t src_len, const int64_t* rows, int64_t R, int64_t dst_len,
                                  float canary, float* dst_out)
{
    if (!c || !src || !rows || !dst_out) return SD_ERR_ARG;
    ENTER(c);
    if (which < 0 || which > 3 || R < 1 || R > (1 << 16) || (which == 3 && R != 1) || src_len < 0 || src_len > LIMIT || dst_len < 1 || dst_len > LIMIT)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_group_copy: which %d, R %lld, src_len %lld, dst_len %lld", which, (long long)R, (long long)src_len, (long long)dst_len);
    const bool pcm = which == 0 && !is_f32;
    std::vector<std::pair<int64_t, int64_t>> dst;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t so = rows[4 * r], dof = rows[4 * r + 1], len = rows[4 * r + 2], room = rows[4 * r + 3];
        if (so < 0 || len < 0 || so + len > src_len || dof < 0 || room < 0 || dof + room > dst_len) SD_FAIL(c, SD_ERR_ARG, "sd_test_group_copy: row %lld leaves its operands", (long long)r);
        // k_tail_move: four floats per thread from 16-byte aligned places, and no `room`: len + SD_TAIL_PAD floats are written
        if (which == 3 && (so % 4 != 0 || dof != 0 || room < len + SD_TAIL_PAD)) SD_FAIL(c, SD_ERR_ARG, "sd_test_group_copy: k_tail_move takes src_off %% 4 == 0, dst_off 0, room >= len + %d", SD_TAIL_PAD);
        dst.emplace_back(dof, dof + room);
    }
    if (overlap(dst)) SD_FAIL(c, SD_ERR_ARG, "sd_test_group_copy: two rows share a destination");
    void* dS; float* dD;
    if (pcm) { int16_t* p; RUN(up<int16_t>(c, "ti_src", (const int16_t*)src, (size_t)src_len, 0, (size_t)SLACK, (int16_t)0x7fff, &p)); dS = p; }
    else { float* p; RUN(up<float>(c, "ti_src", (const float*)src, (size_t)src_len, 0, (size_t)SLACK, FNAN, &p)); dS = p; }
    RUN(fill<float>(c, "ti_y", (size_t)(dst_len + SLACK), canary, &dD));
    std::vector<GroupRow> tab((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        const void* s = pcm ? (const void*)((const int16_t*)dS + rows[4 * r]) : (const void*)((const float*)dS + rows[4 * r]);
        tab[(size_t)r] = GroupRow{s, dD + rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3]};
    }
    if (which == 3) RUN(launch_tail_move(c, tab[0].dst, (const float*)tab[0].src, tab[0].len));
    else {
        WS(c, GroupRow, d_tab, "ti_tab", R);
        HIPCHK(c, hipMemcpy(d_tab, tab.data(), (size_t)R * sizeof(GroupRow), hipMemcpyHostToDevice));
        RUN(group_launch(c, which, d_tab, tab, pcm ? 0 : 1));
    }
    return down(c, dD, (size_t)(dst_len + SLACK), dst_out);
}

extern "C" int sd_test_many_pack(sd_ctx* c, int is_f32, const void* src, int64_t src_len, const int64_t* rows, int64_t R, int64_t dst_len, float canary,
                                 float* dst_out)
{
    if (!c || !src || !rows || !dst_out) return SD_ERR_ARG;
    ENTER(c);
    if (R < 1 || R > (1 << 16) || src_len < 0 || src_len > LIMIT || dst_len < 1 || dst_len > LIMIT) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_pack: R %lld, src_len %lld, dst_len %lld", (long long)R, (long long)src_len, (long long)dst_len);
    std::vector<std::pair<int64_t, int64_t>> dst;
    for (int64_t r = 0; r < R; ++r) {
        const int64_t so = rows[4 * r], n = rows[4 * r + 1], base = rows[4 * r + 2], len = rows[4 * r + 3];
        const int64_t reads = std::min(n, std::min(len, std::max<int64_t>(dst_len - base, 0)));      // i < n, i < len, base + i < dst_len
        if (n < 0 || base < 0 || len < 0 || len > LIMIT || so < -1 || (so < 0 && reads > 0) || (so >= 0 && so + reads > src_len)) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_pack: row %lld leaves its operands", (long long)r);
        dst.emplace_back(base, std::min(base + len, dst_len));
    }
    if (overlap(dst)) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_pack: two rows share a destination");
    void* dS; float* dD;
    if (is_f32) { float* p; RUN(up<float>(c, "ti_src", (const float*)src, (size_t)src_len, 0, (size_t)SLACK, FNAN, &p)); dS = p; }
    else { int16_t* p; RUN(up<int16_t>(c, "ti_src", (const int16_t*)src, (size_t)src_len, 0, (size_t)SLACK, (int16_t)0x7fff, &p)); dS = p; }
    RUN(fill<float>(c, "ti_y", (size_t)(dst_len + SLACK), canary, &dD));
    std::vector<ManyRow> tab((size_t)R);
    for (int64_t r = 0; r < R; ++r) {
        const int64_t so = rows[4 * r];
        const void* s = so < 0 ? nullptr : is_f32 ? (const void*)((const float*)dS + so) : (const void*)((const int16_t*)dS + so);
        tab[(size_t)r] = ManyRow{s, rows[4 * r + 1], rows[4 * r + 2], rows[4 * r + 3]};
    }
    WS(c, ManyRow, d_tab, "ti_tab", R);
    HIPCHK(c, hipMemcpy(d_tab, tab.data(), (size_t)R * sizeof(ManyRow), hipMemcpyHostToDevice));
    RUN(launch_many_pack(c, d_tab, tab, is_f32, dD, dst_len));
    return down(c, dD, (size_t)(dst_len + SLACK), dst_out);
}

extern "C" int sd_test_many_gap_masks(sd_ctx* c, const int64_t* gaps, int64_t G, int64_t total_chunks, float canary, float* masks_out)
{
    if (!c || !gaps || !masks_out) return SD_ERR_ARG;
    ENTER(c);
    if (G < 1 || G > (1 << 16) || total_chunks < 1 || total_chunks > (1 << 16)) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_gap_masks: G %lld, total_chunks %lld", (long long)G, (long long)total_chunks);
    std::vector<ManyGap> tab((size_t)G);
    for (int64_t g = 0; g < G; ++g) {
        tab[(size_t)g] = ManyGap{gaps[2 * g], gaps[2 * g + 1]};
        if (tab[(size_t)g].first < 0 || tab[(size_t)g].count < 0 || tab[(size_t)g].count > (1 << 16)) SD_FAIL(c, SD_ERR_ARG, "sd_test_many_gap_masks: gap %lld", (long long)g);
    }
    const size_t n = (size_t)(total_chunks + SLACK) * SD_SPEAKERS * SD_FRAMES;
    float* dM;
    RUN(fill<float>(c, "ti_y", n, canary, &dM));
    WS(c, ManyGap, d_tab, "ti_tab", G);
    HIPCHK(c, hipMemcpy(d_tab, tab.data(), (size_t)G * sizeof(ManyGap), hipMemcpyHostToDevice));
    RUN(launch_many_gap_masks(c, d_tab, tab, dM, total_chunks));
    return down(c, dM, n, masks_out);
}

extern "C" int sd_test_weight_forms(sd_ctx* c, const float* w, int K, int Cout, int CinPad, int cin, int form, uint16_t canary, uint16_t* halves_out,
                                    int64_t halves_cap, float* inv_scale)
{
    if (!c || !w || !halves_out || !inv_scale) return SD_ERR_ARG;
    ENTER(c);
    if (K < 1 || Cout < 1 || cin < 1 || cin > CinPad || CinPad % 32 != 0 || (form != 0 && form != 1) || (int64_t)K * Cout * CinPad > LIMIT / 4)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_weight_forms: K %d, Cout %d, CinPad %d (a multiple of 32), cin %d, form %d", K, Cout, CinPad, cin, form);
    // a scratch layer, padded as weights.cpp pads it
    ConvLayer L;
    L.Cin = cin; L.Cout = Cout; L.KT = K; L.dil = 1;
    L.CinPad = CinPad;
    L.CinPad16 = (cin + 63) / 64 * 64;
    const size_t halves = (form ? conv_w16x_bytes(L) : conv_w16_bytes(L)) / 2;
    if (halves_cap != (int64_t)halves + SLACK) SD_FAIL(c, SD_ERR_ARG, "sd_test_weight_forms: the form has %zu halves, the caller expects %lld", halves, (long long)(halves_cap - SLACK));
    float* dW; uint16_t* dH;
    RUN(up<float>(c, "ti_src", w, (size_t)K * Cout * CinPad, 0, (size_t)SLACK, FNAN, &dW));
    RUN(fill<uint16_t>(c, "ti_h", halves + SLACK, canary, &dH));
    L.W = dW;
    *inv_scale = 0.0f;
    if (form) {
        WS(c, unsigned, d_max, "ti_wmax", 1);
        RUN(build_conv_w16x(c, L, dH, d_max));
        *inv_scale = L.w16x_inv;
    } else RUN(build_conv_w16(c, L, dH));
    return down(c, dH, halves + SLACK, halves_out);
}
