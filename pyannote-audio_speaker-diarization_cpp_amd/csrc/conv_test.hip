// conv_test.hip -- sd_test_conv (sdhip_test.h): one conv / linear case through the product's dispatch, for tests/test_conv_kernels.py.
// Host code only.  The hook lays the caller's operands out in guarded buffers, uploads them, calls launch_conv_narrow (when asked) and
// launch_conv_gemm exactly as pyannet.hip / ecapa.hip do, and downloads the whole output buffer.  It holds no kernel and restates no
// kernel logic: the row table (k_build_rowtab), the fp16 / split weight forms (build_conv_w16 / build_conv_w16x) and the fp16 activations
// (k_rows_to_half) come from the product's own code.
#include "common.h"
#include <cmath>
#include <limits>

namespace {
struct Slice { int col0, width; };      // a column range of a buffer row
// [rows + slack][ld] f32 image: `fill` everywhere
std::vector<float> image(int64_t rows, int64_t slack, int ld, float fill) { return std::vector<float>((size_t)((rows + slack) * ld), fill); }
// src [rows][cin] into columns [s.col0, s.col0 + s.width) of the image: cin operands, zeros up to the slice's width; NaN in the slack rows
void put_x(std::vector<float>& img, int ld, int64_t rows, int64_t slack, Slice s, const float* src, int cin)
{
    for (int64_t r = 0; r < rows + slack; ++r)
        for (int k = 0; k < s.width; ++k)
            img[(size_t)(r * ld + s.col0 + k)] = r >= rows ? std::numeric_limits<float>::quiet_NaN() : (k < cin ? src[(size_t)(r * cin + k)] : 0.0f);
}
bool overlap(Slice a, Slice b) { return a.col0 < b.col0 + b.width && b.col0 < a.col0 + a.width; }
const int64_t SLACK = 256;              // guard rows behind every buffer: one tile of the widest kernel
}

extern "C" int sd_test_conv(sd_ctx* c, const sd_conv_case* k, const int32_t* n_in, const int32_t* n_out, const float* w, const float* x, const float* x2,
                            const float* bias, const float* scale, const float* shift, const float* item_bias, float* y_out, char* kernel_name, int name_cap)
{
    if (!c || !k || !w || !x || !y_out || !kernel_name || name_cap < 1) return SD_ERR_ARG;
    kernel_name[0] = 0;
    c->err.clear();
    if (hipSetDevice(c->device) != hipSuccess) return SD_ERR_HIP;
    const bool f16 = k->prec == 1, x3 = k->prec == 3;
    if (k->prec != 0 && !f16 && !x3) SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: prec %d", k->prec);
    if (k->items < 1 || k->items > ROWTAB_MAX_ITEMS || k->cin < 1 || k->cout < 1 || k->kt < 1 || k->dil < 1 || (k->has_x2 && !x2) || (!scale != !shift) ||
        (k->cin_pad != 0 && k->cin_pad < k->cin))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: bad case");
    // ---- row spaces
    int64_t M = 0, in_rows = 0;
    std::vector<int> off((size_t)2 * (k->items + 1), 0);      // prefix sums: [0] output space, [1] input space
    if (k->dense) {
        if (k->tp_in < 1 || k->tp_out < 1 || k->tin < 1 || k->tin > k->tp_in || k->t < 1 || k->t > k->tp_out) SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: bad dense row space");
        M = (int64_t)k->items * k->tp_out; in_rows = (int64_t)k->items * k->tp_in;
    } else {
        if (!n_in || !n_out || k->tin < 1 || k->tin > 1023) SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: bad compact row space");
        for (int i = 0; i < k->items; ++i) {
            if (n_in[i] < 1 || n_in[i] > 1024 || n_out[i] < 1 || n_out[i] > k->tin) SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: item %d: %d input rows, %d output rows", i, n_in[i], n_out[i]);
            off[(size_t)i + 1] = off[(size_t)i] + n_out[i];
            off[(size_t)(k->items + 1) + i + 1] = off[(size_t)(k->items + 1) + i] + n_in[i];
        }
        M = off[(size_t)k->items]; in_rows = off[(size_t)2 * k->items + 1];
    }
    // ---- the layer, padded as weights.cpp pads it
    ConvLayer L;
    L.Cin = k->cin; L.Cout = k->cout; L.KT = k->kt; L.dil = k->dil;
    L.CinPad = k->cin_pad ? k->cin_pad : (k->cin + 31) / 32 * 32;
    L.CinPad16 = k->cin_pad ? k->cin_pad : (k->cin + 63) / 64 * 64;
    const int Cin = f16 ? L.CinPad16 : L.CinPad;
    // ---- placement
    const Slice sx = {k->x_col0, Cin}, sx2 = {k->x2_col0, Cin}, sy = {k->y_col0, k->cout};
    const int x_ld = k->x_ld, y_ld = k->y_ld;
    if (sx.col0 < 0 || sy.col0 < 0 || sx.col0 + sx.width > x_ld || sy.col0 + sy.width > y_ld || (k->has_x2 && (sx2.col0 < 0 || sx2.col0 + sx2.width > x_ld)) || ((x_ld | y_ld) & 3))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: a slice does not fit its row (or a leading dimension is not a multiple of 4)");
    if (k->shared && (x_ld != y_ld || in_rows != M || overlap(sx, sy) || (k->has_x2 && (overlap(sx2, sy) || overlap(sx, sx2))) || (f16 && k->y_f32)))
        SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: shared buffer: x_ld == y_ld, one row space, disjoint slices, one element type");
    const bool y_half = f16 && !k->y_f32;
    // host images
    std::vector<float> hy = image(M, SLACK, y_ld, k->canary), hx, hx2;
    if (k->shared) {
        put_x(hy, y_ld, M, SLACK, sx, x, k->cin);
        if (k->has_x2) put_x(hy, y_ld, M, SLACK, sx2, x2, k->cin);
    } else {
        hx = image(in_rows, SLACK, x_ld, k->canary);
        put_x(hx, x_ld, in_rows, SLACK, sx, x, k->cin);
        if (k->has_x2) { hx2 = image(in_rows, SLACK, x_ld, k->canary); put_x(hx2, x_ld, in_rows, SLACK, sx2, x2, k->cin); }
    }
    std::vector<float> hw((size_t)k->kt * k->cout * L.CinPad, 0.0f);
    for (size_t r = 0; r < (size_t)k->kt * k->cout; ++r)
        for (int i = 0; i < k->cin; ++i) hw[r * L.CinPad + i] = w[r * k->cin + i];
    // ---- device buffers (workspaces of their own); an image goes up as f32 and, for an fp16 buffer, through the product's conversion
    hipStream_t st = c->stream;
    int rc;
    auto upload = [&](const std::vector<float>& img, bool half, const char* name32, const char* name16, void** out) -> int {
        WS(c, float, d32, name32, img.size());
        HIPCHK(c, hipMemcpyAsync(d32, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice, st));
        *out = d32;
        if (half) {
            WS(c, uint16_t, d16, name16, img.size());
            if ((rc = ecapa_rows_to_half(c, d32, d16, (int64_t)(img.size() / 4)))) return rc;
            *out = d16;
        }
        return SD_OK;
    };
    void *dY = nullptr, *dX = nullptr, *dX2 = nullptr;
    if ((rc = upload(hy, y_half, "tc_Y32", "tc_Y16", &dY))) return rc;
    if (k->shared) { dX = dY; dX2 = dY; }
    else {
        if ((rc = upload(hx, f16, "tc_X32", "tc_X16", &dX))) return rc;
        if (k->has_x2 && (rc = upload(hx2, f16, "tc_X232", "tc_X216", &dX2))) return rc;
    }
    WS(c, float, dW, "tc_W", hw.size());
    HIPCHK(c, hipMemcpyAsync(dW, hw.data(), hw.size() * sizeof(float), hipMemcpyHostToDevice, st));
    L.W = dW;
    WS(c, float, dP, "tc_params", (size_t)3 * k->cout + (size_t)k->items * k->cout + 16);
    float* dIB = dP + (size_t)3 * k->cout;
    if (bias) { HIPCHK(c, hipMemcpyAsync(dP, bias, (size_t)k->cout * 4, hipMemcpyHostToDevice, st)); L.bias = dP; }
    if (scale) {
        HIPCHK(c, hipMemcpyAsync(dP + k->cout, scale, (size_t)k->cout * 4, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(dP + 2 * (size_t)k->cout, shift, (size_t)k->cout * 4, hipMemcpyHostToDevice, st));
        L.scale = dP + k->cout; L.shift = dP + 2 * (size_t)k->cout;
    }
    if (item_bias) HIPCHK(c, hipMemcpyAsync(dIB, item_bias, (size_t)k->items * k->cout * 4, hipMemcpyHostToDevice, st));
    if (f16) {
        if (L.CinPad16 % 4) SD_FAIL(c, SD_ERR_ARG, "sd_test_conv: cin_pad %d", L.CinPad16);
        WS(c, char, d, "tc_W16", conv_w16_bytes(L));
        if ((rc = build_conv_w16(c, L, d))) return rc;
    }
    if (x3) {
        WS(c, char, d, "tc_W16x", conv_w16x_bytes(L));
        WS(c, unsigned, d_max, "tc_wmax", 1);
        if ((rc = build_conv_w16x(c, L, d, d_max))) return rc;
    }
    int2* d_tab = nullptr;
    if (!k->dense) {
        WS(c, int, d_off, "tc_rowoff", off.size());
        HIPCHK(c, hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(int), hipMemcpyHostToDevice, st));
        WS(c, int2, tab, "tc_rowtab", (size_t)M + 512);
        HIPCHK(c, hipMemsetAsync(tab, 0, ((size_t)M + 512) * sizeof(int2), st));
        if ((rc = ecapa_build_rowtab(c, d_off, 0, d_off + (k->items + 1), 0, k->items, tab))) return rc;
        d_tab = tab;
    }
    // ---- the call, as ecapa.hip's conv_args / pyannet.hip's call sites fill it
    const size_t es = f16 ? 2 : 4;
    ConvArgs a; memset(&a, 0, sizeof(a));
    a.X = (const float*)((const char*)dX + (size_t)sx.col0 * es); a.x_ld = x_ld;
    if (k->has_x2) { a.X2 = (const float*)((const char*)dX2 + (size_t)sx2.col0 * es); a.x2_ld = x_ld; }
    a.Y = (float*)((char*)dY + (size_t)sy.col0 * (y_half ? 2 : 4)); a.y_ld = y_ld;
    a.W = L.W; a.W16 = L.W16; a.bias = L.bias; a.scale = L.scale; a.shift = L.shift;
    if (item_bias) { a.item_bias = dIB; a.ib_ld = k->cout; }
    a.M = (int)M; a.Tin = k->tin;
    if (k->dense) { a.TpIn = k->tp_in; a.TpOut = k->tp_out; a.T = k->t; }
    else { a.TpIn = a.TpOut = SD_TP; a.T = k->tin; a.rowtab = d_tab; a.in_rows = (int)in_rows; }
    a.Cin = Cin; a.cin_real = k->cin; a.Cout = k->cout; a.KT = k->kt; a.dil = k->dil; a.w_ld = Cin;
    a.pad_mode = k->pad_mode; a.act1 = k->act1; a.act2 = k->act2; a.y_f32 = k->y_f32; a.prec = f16 ? 1 : 0;
    if (x3) { a.prec = 3; a.W16x = L.W16x; a.acc_scale = L.w16x_inv; }
    c->last_conv_kernel = nullptr;
    rc = 1;
    if (k->try_narrow) rc = launch_conv_narrow(c, a, "test");
    if (rc == 1) rc = launch_conv_gemm(c, a, "test");
    if (c->last_conv_kernel) snprintf(kernel_name, (size_t)name_cap, "%s", c->last_conv_kernel);
    if (rc) return rc;
    // ---- the whole output buffer back, as f32
    const size_t ny = hy.size();
    if (y_half) {
        std::vector<_Float16> h16(ny);
        HIPCHK(c, hipMemcpyAsync(h16.data(), dY, ny * 2, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (size_t i = 0; i < ny; ++i) y_out[i] = (float)h16[i];
    } else {
        HIPCHK(c, hipMemcpyAsync(y_out, dY, ny * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return SD_OK;
}
