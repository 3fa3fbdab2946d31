// ecapa_test.hip -- sd_test_ecapa_stats / sd_test_se_apply / sd_test_rowtab / sd_test_scatter_emb / sd_test_to_half (sdhip_test.h): ONE launch of one of
// ecapa.hip's glue kernels, for tests/test_ecapa_glue.py.  Host code only.  A hook lays the caller's operands out in guarded buffers, uploads them, calls
// the launcher run_ecapa_t / run_embed call (common.h: launch_masked_mean, launch_asp_stats, launch_asp_pool, launch_se_apply, ecapa_build_rowtab,
// ecapa_scatter_emb, ecapa_feats_to_half, ecapa_rows_to_half) and downloads the whole output buffer.  It holds no kernel and restates no kernel logic:
// grid, block and template choice are the launchers', the row tables come from k_build_rowtab and the fp16 operands from k_rows_to_half.  What a hook
// does check is that every address the kernel is DEFINED to read lies inside the operand it was given.
#include "common.h"
#include <cmath>
#include <limits>

namespace {
const int64_t SLACK = 256;              // guard rows behind every buffer
const int64_t TAB_SLACK = 128;          // slack entries of a row table (run_ecapa_t allocates as many)
const float QNAN = std::numeric_limits<float>::quiet_NaN();
// `n` operand floats, then `slack` NaNs
std::vector<float> with_nan(const float* src, size_t n, size_t slack)
{
    std::vector<float> v(n + slack, QNAN);
    if (n) memcpy(v.data(), src, n * sizeof(float));
    return v;
}
// a host image to the device; half: through the product's conversion kernel into a second workspace (img.size() % 4 == 0)
int up(sd_ctx* c, const char* name, const std::vector<float>& h, bool half, void** d)
{
    WS(c, float, p, name, h.size());
    HIPCHK(c, hipMemcpyAsync(p, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    *d = p;
    if (half) {
        const std::string n16 = std::string(name) + "_h";
        WS(c, uint16_t, p16, n16.c_str(), h.size());
        if (const int rc = ecapa_rows_to_half(c, p, p16, (int64_t)(h.size() / 4))) return rc;
        *d = p16;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));                 // (the host image is the caller's temporary)
    return SD_OK;
}
// `n` ints, then SLACK times `guard`
int up_int(sd_ctx* c, const char* name, const int32_t* src, size_t n, int32_t guard, int** d)
{
    std::vector<int32_t> h(n + SLACK, guard);
    memcpy(h.data(), src, n * sizeof(int32_t));
    WS(c, int, p, name, h.size());
    HIPCHK(c, hipMemcpyAsync(p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *d = p;
    return SD_OK;
}
// n elements of a device buffer back as f32
int down(sd_ctx* c, const void* d, size_t n, bool half, float* h)
{
    if (half) {
        std::vector<_Float16> h16(n);
        HIPCHK(c, hipMemcpyAsync(h16.data(), d, n * 2, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < n; ++i) h[i] = (float)h16[i];
        return SD_OK;
    }
    HIPCHK(c, hipMemcpyAsync(h, d, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}
// prefix sums [items + 1] of one row space: ascending from off[0], 1 .. 1024 rows per item (a row table numbers frames 0 .. 1023)
bool space_ok(const int32_t* off, int64_t items)
{
    for (int64_t i = 0; i < items; ++i) { const int64_t n = (int64_t)off[i + 1] - off[i]; if (n < 1 || n > 1024) return false; }
    return off[0] >= 0 && off[items] - off[0] <= (1 << 22);
}
}

extern "C" int sd_test_ecapa_stats(sd_ctx* c, int kind, int f16, const float* x, const float* logits, const int32_t* nvalid, const int32_t* rowoff, int64_t items,
                                   int row_base, int C, int ld, float canary, float* out)
{
    if (!c || !x || !nvalid || !rowoff || !out) return SD_ERR_ARG;
    ENTER(c);
    if (kind < 0 || kind > 2 || items < 1 || items > ROWTAB_MAX_ITEMS || C < 1 || C > (1 << 16) || ld < C || (ld & 3) || (kind == 2) != (logits != nullptr) ||
        rowoff[0] != row_base || !space_ok(rowoff, items))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_ecapa_stats: kind %d, items %lld, C %d, ld %d, row_base %d", kind, (long long)items, C, ld, row_base);
    // rows the kernel is defined to read: item i's [rowoff[i] - row_base, + nvalid[i])
    for (int64_t i = 0; i < items; ++i)
        if (nvalid[i] < 1 || nvalid[i] > rowoff[i + 1] - rowoff[i]) SD_FAIL(c, SD_ERR_ARG, "sd_test_ecapa_stats: item %lld reads %d frames of %d stored", (long long)i, nvalid[i], rowoff[i + 1] - rowoff[i]);
    const size_t rows = (size_t)(rowoff[items] - row_base);
    int rc;
    void *dX = nullptr, *dL = nullptr, *dOut = nullptr;
    int *dNv, *dOff;
    if ((rc = up(c, "te_st_x", with_nan(x, rows * ld, (size_t)SLACK * ld), f16 != 0, &dX))) return rc;
    if (logits && (rc = up(c, "te_st_l", with_nan(logits, rows * ld, (size_t)SLACK * ld), false, &dL))) return rc;
    // (behind the int vectors: values with which a kernel that read them would give NaN without leaving the buffers)
    if ((rc = up_int(c, "te_st_nv", nvalid, (size_t)items, 0, &dNv))) return rc;
    if ((rc = up_int(c, "te_st_off", rowoff, (size_t)items + 1, row_base, &dOff))) return rc;
    const size_t W = kind == 0 ? (size_t)C : (size_t)2 * C, n_out = ((size_t)items + SLACK) * W;
    if ((rc = up(c, "te_st_out", std::vector<float>(n_out, canary), false, &dOut))) return rc;
    if (kind == 0) rc = launch_masked_mean(c, f16 != 0, dX, ld, dNv, dOff, row_base, items, (int64_t)rows, (float*)dOut, C);
    else if (kind == 1) rc = launch_asp_stats(c, f16 != 0, dX, ld, dNv, dOff, row_base, items, (int64_t)rows, (float*)dOut, C);
    else rc = launch_asp_pool(c, f16 != 0, dX, (const float*)dL, ld, dNv, dOff, row_base, items, (int64_t)rows, (float*)dOut, C);
    if (rc) return rc;
    return down(c, dOut, n_out, false, out);
}

extern "C" int sd_test_se_apply(sd_ctx* c, int f16, int shared, const float* t2, int t2_ld, const float* gate, const float* res, int res_ld, int res_col0, int out_col0,
                                int y_ld, int C, const int32_t* off, int64_t items, int os, int rs, int ys, float canary, float* y_out)
{
    if (!c || !t2 || !gate || !res || !off || !y_out) return SD_ERR_ARG;
    ENTER(c);
    auto space = [](int s) { return s >= 0 && s < EC_SPACES; };
    if (items < 1 || items > ROWTAB_MAX_ITEMS || C < 4 || (C & 3) || !space(os) || !space(rs) || !space(ys) || t2_ld < C || ((t2_ld | y_ld | out_col0) & 3) ||
        out_col0 < 0 || out_col0 + C > y_ld)
        SD_FAIL(c, SD_ERR_ARG, "sd_test_se_apply: items %lld, C %d, spaces %d / %d / %d, t2_ld %d, y_ld %d, out_col0 %d", (long long)items, C, os, rs, ys, t2_ld, y_ld, out_col0);
    if (shared ? (rs != ys || res_col0 < 0 || (res_col0 & 3) || res_col0 + C > y_ld || (res_col0 < out_col0 + C && out_col0 < res_col0 + C)) : (res_ld < C || (res_ld & 3)))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_se_apply: %s", shared ? "shared buffer: one space, two disjoint slices inside the row" : "residual rows shorter than C");
    const size_t n1 = (size_t)items + 1;
    const int32_t *o_os = off + os * n1, *o_rs = off + rs * n1, *o_ys = off + ys * n1;
    if (o_os[0] || o_rs[0] || o_ys[0] || !space_ok(o_os, items) || !space_ok(o_rs, items) || !space_ok(o_ys, items)) SD_FAIL(c, SD_ERR_ARG, "sd_test_se_apply: bad row space");
    // rows the kernel is defined to touch: frame t of item i for every t the space `os` stores, in the residual's and in the output's space
    for (int64_t i = 0; i < items; ++i) {
        const int n = o_os[i + 1] - o_os[i];
        if (o_rs[i + 1] - o_rs[i] < n || o_ys[i + 1] - o_ys[i] < n) SD_FAIL(c, SD_ERR_ARG, "sd_test_se_apply: item %lld stores %d frames in space %d, fewer in space %d or %d", (long long)i, n, os, rs, ys);
    }
    const size_t Mo = (size_t)o_os[items], Rr = (size_t)o_rs[items], Ry = (size_t)o_ys[items];
    const bool half = f16 != 0;
    std::vector<float> hy((Ry + SLACK) * y_ld, canary);
    if (shared)
        for (size_t r = 0; r < Ry + SLACK; ++r)
            for (int k = 0; k < C; ++k) hy[r * y_ld + res_col0 + k] = r < Ry ? res[r * C + k] : QNAN;
    int rc;
    void *dY = nullptr, *dRes = nullptr, *dT2 = nullptr, *dG = nullptr;
    int* dOff;
    if ((rc = up(c, "te_se_y", hy, half, &dY))) return rc;
    if (!shared && (rc = up(c, "te_se_res", with_nan(res, Rr * res_ld, (size_t)SLACK * res_ld), half, &dRes))) return rc;
    if ((rc = up(c, "te_se_t2", with_nan(t2, Mo * t2_ld, (size_t)SLACK * t2_ld), half, &dT2))) return rc;
    if ((rc = up(c, "te_se_gate", with_nan(gate, (size_t)items * C, SLACK), false, &dG))) return rc;
    if ((rc = up_int(c, "te_se_off", off, EC_SPACES * n1, 0, &dOff))) return rc;
    // the tables, as run_ecapa_t's tab(so, si) builds them: t2's own space (the item of a row), os -> rs, os -> ys
    auto tab = [&](const char* name, int si, int2** out) -> int {
        WS(c, int2, p, name, Mo + TAB_SLACK);
        *out = p;
        return ecapa_build_rowtab(c, dOff + os * n1, 0, dOff + si * n1, 0, items, p);
    };
    int2 *t_self = nullptr, *res_map = nullptr, *out_map = nullptr;
    if ((rc = tab("te_se_tab", os, &t_self))) return rc;
    if (rs != os && (rc = tab("te_se_rmap", rs, &res_map))) return rc;
    if (ys != os && (rc = tab("te_se_omap", ys, &out_map))) return rc;
    const size_t es = half ? 2 : 4;
    const void* pres = shared ? (const void*)((const char*)dY + (size_t)res_col0 * es) : dRes;
    if ((rc = launch_se_apply(c, half, dT2, t2_ld, (const float*)dG, pres, shared ? y_ld : res_ld, (char*)dY + (size_t)out_col0 * es, y_ld, C, (int64_t)Mo,
                              t_self, res_map, out_map))) return rc;
    return down(c, dY, hy.size(), half, y_out);
}

extern "C" int sd_test_rowtab(sd_ctx* c, const int32_t* off_out, const int32_t* off_in, int64_t items, int32_t canary, int32_t* tab_out)
{
    if (!c || !off_out || !off_in || !tab_out) return SD_ERR_ARG;
    ENTER(c);
    if (items < 1 || items > ROWTAB_MAX_ITEMS || !space_ok(off_out, items) || !space_ok(off_in, items)) SD_FAIL(c, SD_ERR_ARG, "sd_test_rowtab: items %lld or a bad row space", (long long)items);
    const size_t n = (size_t)(off_out[items] - off_out[0]) + TAB_SLACK;
    int rc;
    int *dOut, *dIn;
    if ((rc = up_int(c, "te_rt_out", off_out, (size_t)items + 1, off_out[items], &dOut))) return rc;
    if ((rc = up_int(c, "te_rt_in", off_in, (size_t)items + 1, off_in[items], &dIn))) return rc;
    const std::vector<int32_t> h(2 * n, canary);
    WS(c, int2, tab, "te_rt_tab", n);
    HIPCHK(c, hipMemcpyAsync(tab, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = ecapa_build_rowtab(c, dOut, off_out[0], dIn, off_in[0], items, tab))) return rc;
    HIPCHK(c, hipMemcpyAsync(tab_out, tab, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}

extern "C" int sd_test_scatter_emb(sd_ctx* c, const float* emb_c, int64_t n_c, const int32_t* cidx, int64_t items, float canary, float* emb_out)
{
    if (!c || !cidx || !emb_out || (n_c > 0 && !emb_c)) return SD_ERR_ARG;
    ENTER(c);
    if (items < 1 || items > (1 << 20) || n_c < 0) SD_FAIL(c, SD_ERR_ARG, "sd_test_scatter_emb: items %lld, %lld compact rows", (long long)items, (long long)n_c);
    for (int64_t i = 0; i < items; ++i) if (cidx[i] >= n_c) SD_FAIL(c, SD_ERR_ARG, "sd_test_scatter_emb: item %lld reads compact row %d of %lld", (long long)i, cidx[i], (long long)n_c);
    int rc;
    void *dC = nullptr, *dE = nullptr;
    int* dIdx;
    if ((rc = up(c, "te_sc_c", with_nan(emb_c, (size_t)n_c * SD_EMB_DIM, (size_t)SLACK * SD_EMB_DIM), false, &dC))) return rc;
    if ((rc = up_int(c, "te_sc_idx", cidx, (size_t)items, -1, &dIdx))) return rc;
    const size_t n_out = ((size_t)items + SLACK) * SD_EMB_DIM;
    if ((rc = up(c, "te_sc_e", std::vector<float>(n_out, canary), false, &dE))) return rc;
    if ((rc = ecapa_scatter_emb(c, (const float*)dC, dIdx, (float*)dE, items))) return rc;
    return down(c, dE, n_out, false, emb_out);
}

extern "C" int sd_test_to_half(sd_ctx* c, int kind, const float* f, int64_t rows, int width, float canary, uint16_t* h_out)
{
    if (!c || !f || !h_out) return SD_ERR_ARG;
    ENTER(c);
    if ((kind != 0 && kind != 1) || rows < 1 || rows > (1 << 20) || (kind == 0 ? width != SD_FEAT_LD : (width < 4 || (width & 3) || width > (1 << 16))))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_to_half: kind %d, rows %lld, width %d", kind, (long long)rows, width);
    const int w_out = kind == 0 ? 128 : width;
    int rc;
    void* dF = nullptr;
    if ((rc = up(c, "te_th_f", with_nan(f, (size_t)rows * width, (size_t)SLACK * width), false, &dF))) return rc;
    const size_t n_out = ((size_t)rows + SLACK) * w_out;
    const std::vector<_Float16> hc(n_out, (_Float16)canary);
    WS(c, _Float16, dH, "te_th_h", n_out);
    HIPCHK(c, hipMemcpyAsync(dH, hc.data(), n_out * 2, hipMemcpyHostToDevice, c->stream));
    if (kind == 0) rc = ecapa_feats_to_half(c, (const float*)dF, dH, rows);
    else rc = ecapa_rows_to_half(c, (const float*)dF, dH, rows * width / 4);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(h_out, dH, n_out * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return SD_OK;
}
