// Test hooks for the GAN side (not in the header): each runs ONE launch of disc_engine.hip's forward / backward or of
// perceptual_engine.hip's on the caller's buffers, through the WideCtx member (wide_recipes.h) or the vsr_launch_* function the engines
// call, with the weight image the engines' pack step makes.  Argument checks and launches only: no kernel lives here.
// tests/test_wide_gpu.py compares every hook with an fp64 restatement.  (vsr_debug_disc_plan sits beside the plan it reads, in
// disc_engine.hip; vsr_debug_wide2_set_max_wg beside the launcher, in conv_wide.hip.)
//   *_pm: blocked pixel-major of the element type of `dtype`; w: fp32 OIHW.  bf16 runs on conv_wide2_kernel, fp32 on the generic
//   conv_wide_kernel: the dtype alone picks the weight image and the kernel (vsr_launch_conv_wide refuses the generic image in bf16).
#include "wide_recipes.h"
#include "debug_hooks.h"

namespace {
bool bad_ch(int c) { return c < 64 || (c & 63); }
}  // namespace

extern "C" {

// WideCtx::wide on vsr_launch_pack_wide2 (bf16) / vsr_launch_pack_wide (fp32) of w (cout, cin, 3, 3) or (cout, cin, 4, 4):
//   mode 0  y (N, H, W, cout)    = epi(conv3x3(x (N, H, W, cin)))                  mode 2  y (N, H, W, cin)    = epi(its data gradient(x (N, H, W, cout)))
//   mode 1  y (N, H, W, cout)    = epi(conv4x4 stride 2(x (N, 2H, 2W, cin)))       mode 3  y (N, 2H, 2W, cin) = epi(its data gradient(x (N, H, W, cout)))
// epi: + bias, act (ACT_NONE / ACT_RELU / ACT_LEAKY with `slope`), -> y_act, + res, * (aux > 0 ? 1 : slope), -> y; y_act, res, aux: y's
// layout, or NULL.  wpack: wpack_elems elements of scratch for the weight image (refused if too few).  max_wg: bf16 only, at most so
// many workgroups per output column (0: none).  The value before the mask (VsrWideConv::y_pre) is stored by no engine launch and has
// no argument here; nor can a mode read parity views and write phases at once.
int vsr_debug_wide_conv(int dtype, int mode, int cout, int cin, const void* x_pm, const float* w, const float* bias, void* wpack, long long wpack_elems,
                        void* y_pm, int act, float slope, void* y_act_pm, const void* res_pm, const void* aux_pm, int max_wg, int N, int H, int W,
                        void* stream) {
    if (bad_dtype(dtype) || mode < 0 || mode > 3 || bad_ch(cout) || bad_ch(cin) || !x_pm || !w || !wpack || !y_pm || bad_dims(N, H, W) || max_wg < 0 ||
        (act != ACT_NONE && act != ACT_RELU && act != ACT_LEAKY))
        return VSR_ERR_BADARG;
    const bool bf16 = dtype == VSR_BF16, dgrad = mode >= 2;
    const int xC = dgrad ? cout : cin, yC = dgrad ? cin : cout, in_step = mode == 1 ? 2 : 1, out_step = mode == 3 ? 2 : 1;
    if (wpack_elems < (bf16 ? vsr_wide2_pack_elems(cout, cin, mode) : vsr_wide_pack_elems(cout, cin, mode))) return VSR_ERR_WORKSPACE;
    if (!bf16 && (max_wg || (long long)N * (out_step == 2 ? 4 : 1) * (yC / 64) > 65535)) return VSR_ERR_UNSUPPORTED;
    const WideCtx c{(hipStream_t)stream, dtype, N, nullptr};
    if (bf16) CK(vsr_launch_pack_wide2(w, wpack, cout, cin, mode, c.st)); else CK(vsr_launch_pack_wide(dtype, w, wpack, cout, cin, mode, c.st));
    return c.wide(x_pm, xC, H * in_step, W * in_step, in_step, H, W, wpack, bias, y_pm, yC, out_step, act, slope, y_act_pm, res_pm, nullptr, aux_pm, max_wg);
}

// WideCtx::wgrad_layer: gw (dyC, xC, 3, 3) (views 1) or (dyC, xC, 4, 4) (views 4) += the weight gradient from dy (N, H, W, dyC) and the
// layer's input x (views 1: (N, H, W, xC); views 4: (N, 2H, 2W, xC), read as its four parity views).  slab: slab_floats floats of
// scratch, at least twice vsr_conv3x3_c64_wgrad_slab_floats() (a pair-batched launch writes up to VSR_WGRAD_MAX_PAIR_SLABS partials).
int vsr_debug_wide_wgrad(int dtype, int views, int xC, int dyC, const void* x_pm, const void* dy_pm, float* gw, float* slab, long long slab_floats,
                         int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || (views != 1 && views != 4) || bad_ch(xC) || bad_ch(dyC) || !x_pm || !dy_pm || !gw || !slab || bad_dims(N, H, W)) return VSR_ERR_BADARG;
    if (slab_floats < (long long)wide_slab_floats()) return VSR_ERR_WORKSPACE;
    const int npairs = (xC / 64) * (dyC / 64) * views;
    if (dtype == VSR_BF16 && npairs > 1 && (long long)npairs * WideCtx::pair_ksplit(npairs, N * cdiv(H, 8) * cdiv(W, 32)) > VSR_WGRAD_MAX_PAIR_SLABS)
        return VSR_ERR_UNSUPPORTED;
    const int step = views == 4 ? 2 : 1;
    const WideCtx c{(hipStream_t)stream, dtype, N, slab};
    return c.wgrad_layer(x_pm, xC, H * step, W * step, views, dy_pm, dyC, H, W, gw);
}

// vsr_launch_up2_fwd: out (N, 2H, 2W, C) = bilinear x2 (align_corners=False) of a (+ b, or NULL)
int vsr_debug_wide_up2_fwd(int dtype, const void* a_pm, const void* b_pm, void* out_pm, int N, int H, int W, int C, void* stream) {
    if (bad_dtype(dtype) || !a_pm || !out_pm || bad_dims(N, H, W) || C < 8 || (C & 7)) return VSR_ERR_BADARG;
    if (N > 65535 || H > 65535) return VSR_ERR_UNSUPPORTED;
    return vsr_launch_up2_fwd(dtype, a_pm, b_pm, out_pm, N, H, W, C, (hipStream_t)stream);
}

// vsr_launch_up2_bwd in the engine's two forms: din (N, H, W, C) = up2^T(dout (N, 2H, 2W, C)) and dmask = din * (m > 0 ? 1 : slope), or
// dmask alone (din NULL).  din without dmask is launched by no engine and refused here.
int vsr_debug_wide_up2_bwd(int dtype, const void* dout_pm, void* din_pm, void* dmask_pm, const void* m_pm, float slope, int N, int H, int W, int C,
                           void* stream) {
    if (bad_dtype(dtype) || !dout_pm || !dmask_pm || !m_pm || bad_dims(N, H, W) || C < 8 || (C & 7)) return VSR_ERR_BADARG;
    if (N > 65535 || H > 65535) return VSR_ERR_UNSUPPORTED;
    return vsr_launch_up2_bwd(dtype, dout_pm, din_pm, dmask_pm, m_pm, slope, N, H, W, C, (hipStream_t)stream);
}

// vsr_launch_mask_pm: out = g * (m > 0 ? 1 : slope) over `elems` elements (whole blocked images: a multiple of 8)
int vsr_debug_wide_mask(int dtype, const void* g_pm, const void* m_pm, void* out_pm, float slope, long long elems, void* stream) {
    if (bad_dtype(dtype) || !g_pm || !m_pm || !out_pm || elems < 8 || (elems & 7)) return VSR_ERR_BADARG;
    return vsr_launch_mask_pm(dtype, g_pm, m_pm, out_pm, slope, elems, (hipStream_t)stream);
}

// WideCtx::pool_fwd / pool_bwd on a (N, Hi, Wi, C):
//   op 0  g (N, Hi/2, Wi/2, C) = MaxPool2d(2, 2)(a); dp NULL
//   op 1  g (N, Hi, Wi, C)    <- (g + route(dp (N, Hi/2, Wi/2, C))) * (a > 0), in place
int vsr_debug_vgg_pool(int dtype, int op, const void* a_pm, const void* dp_pm, void* g_pm, int N, int Hi, int Wi, int C, void* stream) {
    if (bad_dtype(dtype) || (op & ~1) || !a_pm || !g_pm || (op == 1) != (dp_pm != nullptr) || N < 1 || Hi < 2 || Wi < 2 || C < 8 || (C & 7)) return VSR_ERR_BADARG;
    if (N > 65535 || Hi > 65535 || Wi > 65535) return VSR_ERR_UNSUPPORTED;
    const WideCtx c{(hipStream_t)stream, dtype, N, nullptr};
    return op == 0 ? c.pool_fwd(a_pm, g_pm, Hi, Wi, C) : c.pool_bwd(a_pm, dp_pm, g_pm, Hi, Wi, C);
}

// WideCtx::tap + vsr_launch_tap_sum: sums[img * 5] = sum |s - h| over image img of (N, H, W, C) (sums[img * 5 + 1..4] = 0: one tap of the
// loss's five); grad: h <- scale * sign(s - h), sign(0) = 0.  partial: N * 512 doubles of scratch; sums: N * 5 doubles.
int vsr_debug_vgg_tap(int dtype, const void* s_pm, void* h_pm, int grad, float scale, double* partial, double* sums, int N, int H, int W, int C, void* stream) {
    if (bad_dtype(dtype) || !s_pm || !h_pm || (grad & ~1) || !partial || !sums || bad_dims(N, H, W) || C < 8 || (C & 7)) return VSR_ERR_BADARG;
    if (N > 65535) return VSR_ERR_UNSUPPORTED;
    const WideCtx c{(hipStream_t)stream, dtype, N, nullptr};
    CK(c.tap(s_pm, h_pm, grad != 0, scale, H, W, C, partial));
    const int nb[VSR_TAP_N] = {vsr_tap_blocks(H, W, C), 0, 0, 0, 0};
    return vsr_launch_tap_sum(partial, sums, N, nb, c.st);
}

// vsr_wide2_grid (host only, launches nothing): out[0..2] = workgroups per output column, output columns, tiles of the conv_wide2 launch
// with `ncob` 64-channel output blocks over the domain (N, H, W).  num_cus 0: the current device's.
int vsr_debug_wide_grid(int ncob, int out_step, int N, int H, int W, int max_wg, int num_cus, int* out) {
    if (ncob < 1 || (out_step != 1 && out_step != 2) || bad_dims(N, H, W) || max_wg < 0 || num_cus < 0 || !out) return VSR_ERR_BADARG;
    vsr_wide2_grid(ncob, out_step, N, H, W, max_wg, num_cus ? num_cus : vsr_num_cus(), &out[0], &out[1], &out[2]);
    return VSR_OK;
}

}  // extern "C"
