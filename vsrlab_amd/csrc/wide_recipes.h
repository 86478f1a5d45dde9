// Launch recipes of the GAN side, shared by the engines that run them (disc_engine.hip, perceptual_engine.hip) and the test hooks
// (wide_hooks.hip): one wide convolution, one 64 x 64 block of a wide layer's weight gradient, the whole weight gradient of a wide
// layer, and the grid / block count of VGG's own kernels (perceptual_engine.hip).  Like host.h and recipes.h: no kernel and no state
// live here.  The engines hand in pointers into their arena, the hooks the caller's buffers; both run this code.
#pragma once
#include "host.h"

// partials per (image, tap) of the perceptual loss: the tap kernel's block count is a pure function of the level geometry
// (>= 8 chunks per thread, <= VSR_TAP_PMAX), so an image's sum has the same bits whatever the batch it is computed in
#define VSR_TAP_PMAX 512
#define VSR_TAP_NT 256
#define VSR_TAP_N 5
inline int vsr_tap_blocks(int H, int W, int C) {
    const long long chunks = (long long)H * pm_ws(W) * (C / 8) * 32;
    long long nb = (chunks + VSR_TAP_NT * 8 - 1) / (VSR_TAP_NT * 8);
    return (int)(nb < 1 ? 1 : (nb > VSR_TAP_PMAX ? VSR_TAP_PMAX : nb));
}

// floats of a slab buffer that holds the partials of every launch below: one per workgroup (wgrad_slab_floats()) or per pair and pixel
// part of a pair-batched launch
inline size_t wide_slab_floats() {
    return (size_t)(VSR_WGRAD_NWG > VSR_WGRAD_MAX_PAIR_SLABS ? VSR_WGRAD_NWG : VSR_WGRAD_MAX_PAIR_SLABS) * wgrad_slab_stride3();
}

struct WideCtx {
    hipStream_t st; int dtype; int n;      // n: images per launch
    float* slab;                           // wide_slab_floats() (null: no weight gradients)

    // y (n, H out_step, W out_step, yC) = epilogue(conv(x (n, Hx, Wx, xC))) over the conv domain (n, H, W): 3x3 stride 1, or the parity
    // views of a 4x4 stride-2 conv (in_step 2), or the four output phases of its data gradient (out_step 2).  wpack: the image of
    // vsr_launch_pack_wide2 (bf16) or vsr_launch_pack_wide (fp32).  Epilogue: + bias, act, -> y_act, + res, -> y_pre, * mask(aux), -> y.
    // max_wg: at most so many conv_wide2 workgroups per output column (0: none; the engines leave it 0)
    int wide(const void* x, int xC, int Hx, int Wx, int in_step, int H, int W, const void* wpack, const float* bias, void* y, int yC,
             int out_step, int act, float slope, void* y_act = nullptr, const void* res = nullptr, void* y_pre = nullptr, const void* aux = nullptr,
             int max_wg = 0) const {
        VsrWideConv c = {};
        c.x = x; c.xC = xC; c.Hx = Hx; c.Wx = Wx; c.in_step = in_step; c.nsl = xC / 64;
        c.N = n; c.H = H; c.W = W; c.bias = bias;
        if (dtype == VSR_BF16) c.wpack2 = wpack; else c.wpack = wpack;
        c.y = y; c.yC = yC; c.Hy = H * out_step; c.Wy = W * out_step; c.out_step = out_step; c.ncob = yC / 64;
        c.act = act; c.slope = slope; c.y_act = y_act; c.res = res; c.y_pre = y_pre; c.aux = aux; c.max_wg = max_wg;
        return vsr_launch_conv_wide(dtype, c, st);
    }
    // one 64 x 64 block of a weight gradient: slabs -> reduce.  view < 0: 3x3 layer (OIHW with 9 taps); else parity view of a 4x4 layer
    int wgrad_block(const void* x, int xC, int x_slice, int Hx, int Wx, int x_step, int view, const void* dy, int dyC, int dy_slice,
                    int H, int W, float* gw, int cin_total, int co0, int ci0) const {
        WgradArgs a = {};
        a.N = n; a.H = H; a.W = W; a.nseg = 1;
        a.x[0] = x; a.x_step = x_step; a.x_oy = view >= 0 ? (view >> 1) : 0; a.x_ox = view >= 0 ? (view & 1) : 0;
        a.Hx = Hx; a.Wx = Wx; a.x_nstride = pm_image_elems(Hx, Wx, xC); a.x_ctotal = xC; a.x_coff = x_slice * 8;
        a.dy[0] = dy; a.dy_step = 1; a.Hy = H; a.Wy = W; a.dy_nstride = pm_image_elems(H, W, dyC); a.dy_ctotal = dyC; a.dy_coff = dy_slice * 8;
        const WgradShape shape = {3, 64, false, 64, false};
        if (view < 0) return wgrad_run(st, dtype, slab, a, shape, {64, 64, gw + (size_t)co0 * cin_total * 9, cin_total, ci0, 1, 0, nullptr, 1});
        int nslabs = 0;
        CK(wgrad_launch(st, dtype, slab, a, shape, true, &nslabs));
        return vsr_launch_wgrad_reduce_s2(slab, nslabs, a.slab_stride, gw, cin_total, co0, ci0, view, st);
    }
    // pixel parts of a pair-batched launch: ~512 workgroups per launch, a multiple of 8, no more than the tiles rounded up to one
    static int pair_ksplit(int npairs, int tiles) {
        int ksplit = ((512 / npairs) + 7) & ~7;
        if (ksplit < 8) ksplit = 8;
        const int cap = (tiles + 7) & ~7;
        if (ksplit > cap) ksplit = cap;
        return ksplit;
    }
    // the whole weight gradient of a wide layer: x (xC channels; views == 4: the four parity views of a 4x4 stride-2 conv's input),
    // dy (dyC channels).  bf16: every (view, cout block, cin slice) pair in one launch + one reduction; fp32: pair by pair.  gw is added to.
    int wgrad_layer(const void* x, int xC, int Hx, int Wx, int views, const void* dy, int dyC, int H, int W, float* gw) const {
        const int nsl = xC / 64, ncob = dyC / 64, npairs = nsl * ncob * views, x_step = views == 4 ? 2 : 1;
        if (dtype == VSR_BF16 && npairs > 1) {
            WgradArgs a = {};
            a.N = n; a.H = H; a.W = W; a.nseg = 1;
            a.x[0] = x; a.x_step = x_step; a.Hx = Hx; a.Wx = Wx; a.x_nstride = pm_image_elems(Hx, Wx, xC); a.x_ctotal = xC;
            a.dy[0] = dy; a.dy_step = 1; a.Hy = H; a.Wy = W; a.dy_nstride = pm_image_elems(H, W, dyC); a.dy_ctotal = dyC;
            a.slab = slab; a.slab_stride = wgrad_slab_stride3();
            return vsr_launch_wgrad_pairs(dtype, a, nsl, ncob, views, pair_ksplit(npairs, n * cdiv(H, 8) * cdiv(W, 32)), gw, xC, st);
        }
        for (int v = 0; v < views; ++v) for (int o = 0; o < ncob; ++o) for (int s = 0; s < nsl; ++s)
            CK(wgrad_block(x, xC, s, Hx, Wx, x_step, views == 4 ? v : -1, dy, dyC, o, H, W, gw, xC, 64 * o, 64 * s));
        return VSR_OK;
    }

    // ---- VGG's own launches (kernels: perceptual_engine.hip) on (n, Hi, Wi, C) ----
    int pool_fwd(const void* in, void* out, int Hi, int Wi, int C) const { return vsr_launch_maxpool2_fwd(dtype, in, out, n, Hi, Wi, C, st); }
    // g <- (g + route(dp)) * (a > 0): a the pool's stored input, dp the gradient of its output
    int pool_bwd(const void* a, const void* dp, void* g, int Hi, int Wi, int C) const { return vsr_launch_maxpool2_bwd(dtype, a, dp, g, n, Hi, Wi, C, st); }
    // partial[img * VSR_TAP_PMAX + b], b < vsr_tap_blocks(H, W, C): sums of |s - h|; grad: h <- scale * sign(s - h)
    int tap(const void* s, void* h, bool grad, float scale, int H, int W, int C, double* partial) const {
        return vsr_launch_tap_l1(dtype, s, h, grad ? h : nullptr, scale, n, H, W, C, partial, vsr_tap_blocks(H, W, C), st);
    }
};
