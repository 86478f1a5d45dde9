// Test hooks for the reconstruction tail (not in the header): each runs ONE tail launch on the caller's buffers through the recipe
// (Ctx member) or launcher the engines use, with the weight packs engine.hip / cleaner_engine.hip / disc_engine.hip make for that layer.
// Argument checks and launches only: no kernel lives here.  tests/test_hr_tail_gpu.py compares every hook with an fp64 restatement.
//   w: fp32 OIHW; *_pm: blocked pixel-major, 64 channels, element type of `dtype`; wpack / bias_pack / sign_scratch / slab: caller scratch.
#include "recipes.h"
#include "debug_hooks.h"

extern "C" {

// conv_last.2 (engine.hip recon_forward), the pre-clean out conv, the discriminator's conv_9: 64 -> cout_real (1..4) 3x3, planar fp32
// destination (images y_nstride floats apart) + bias + planar residual `pres` (destination layout) + bilinear x base_scale of the planar
// frames base_lr (base_h x base_w, images base_nstride floats apart).  bf16: c64_to_planar_kernel; fp32: the generic kernel.
// wpack: 9 * 32 * 64 elements; bias_pack: 64 floats.
int vsr_debug_tail_last2_fwd(int dtype, const void* x_pm, const float* w, const float* bias, void* wpack, float* bias_pack, float* y, long long y_nstride,
                             const float* pres, const float* base_lr, long long base_nstride, int base_h, int base_w, int base_scale, int cout_real,
                             int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !x_pm || !w || !wpack || !y || bad_dims(N, H, W) || cout_real < 1 || cout_real > 4 || (bias && !bias_pack) ||
        y_nstride < (long long)cout_real * H * W)
        return VSR_ERR_BADARG;
    if (base_lr && ((base_scale != 2 && base_scale != 4) || base_h < 1 || base_w < 1 || (long long)base_h * base_scale != H ||
                    (long long)base_w * base_scale != W || base_nstride < (long long)cout_real * base_h * base_w))
        return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack(w, wpack, 9, 32, 64, cout_real, 64, 64, 0, 1, 0, 0));
    if (bias) CK(c.pack_bias(bias, bias_pack, cout_real));
    ConvArgs a = conv_args(N, H, W, 64);
    a.src[0] = x_pm; a.wpack = wpack; a.bias = bias ? bias_pack : nullptr; a.cout_real = cout_real;
    a.dst[0] = y; a.dst_nstride = y_nstride; a.pres = pres;
    if (base_lr) { a.base_lr = base_lr; a.base_nstride = base_nstride; a.base_h = base_h; a.base_w = base_w; a.base_scale = base_scale; }
    return vsr_launch_conv(dtype, 3, 1, 64, 64, 0, 32, EPI_PLANAR, a, c.st);
}

// conv_last.2's data gradient (engine.hip recon_backward; bf16 only): dx_pm = mask(aux) * dgrad(dsr), dsr planar fp32 (3 planes, images
// dsr_nstride floats apart), w (3,64,3,3).  mask_src: 0 none, 1 the activation aux_pm, 2 its sign bits, which this hook makes with
// vsr_launch_sign_bits_c64 into sign_scratch (N * ceil(H/8) * ceil(W/32) * 2048 bytes).
int vsr_debug_tail_last2_dgrad(const float* dsr, long long dsr_nstride, const float* w, const void* aux_pm, int mask_src, void* sign_scratch,
                               int mask_mode, float slope, void* dx_pm, int N, int H, int W, void* stream) {
    if (!dsr || !w || !dx_pm || bad_dims(N, H, W) || dsr_nstride < (long long)3 * H * W || mask_src < 0 || mask_src > 2) return VSR_ERR_BADARG;
    if (mask_src != 0 && (!aux_pm || (mask_mode != MASK_RELU && mask_mode != MASK_LEAKY))) return VSR_ERR_BADARG;
    if (mask_src == 2 && !sign_scratch) return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    if (mask_src == 2) CK(vsr_launch_sign_bits_c64(aux_pm, sign_scratch, N, H, W, st));
    return vsr_launch_last2_dgrad(dsr, dsr_nstride, w, mask_src ? aux_pm : nullptr, dx_pm, N, H, W, mask_src ? mask_mode : MASK_NONE, st,
                                  mask_src == 2 ? sign_scratch : nullptr, slope);
}

// Planar fp32 (pc = 1 or 3 planes, images src_nstride floats apart) -> 64 channels, 3x3, + bias, LeakyReLU(slope) (act = ACT_LEAKY), * mask(aux):
// the pre-clean stem (Ctx::stem on Ctx::pack_stem's weights) and the discriminator's conv_0.  w (64,pc,3,3); wpack: 9 * 64 * 16 elements.
// bf16: last2_dgrad_kernel<., PACKED>; fp32: the generic kernel.
int vsr_debug_tail_planar_c64(int dtype, const float* src, long long src_nstride, int pc, const float* w, const float* bias, void* wpack, void* y_pm,
                              int act, float slope, const void* aux_pm, int mask_mode, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !src || !w || !wpack || !y_pm || bad_dims(N, H, W) || (pc != 1 && pc != 3) || src_nstride < (long long)pc * H * W ||
        (act != ACT_NONE && act != ACT_LEAKY))
        return VSR_ERR_BADARG;
    if (aux_pm ? (mask_mode != MASK_RELU && mask_mode != MASK_LEAKY) : mask_mode != MASK_NONE) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack(w, wpack, 9, 64, 16, 64, pc, pc, 0, 1, 0, 0));
    ConvArgs a = conv_args(N, H, W, 64);
    a.src[0] = src; a.src_nstride[0] = src_nstride; a.planar_c = pc; a.wpack = wpack; a.bias = bias; a.dst[0] = y_pm;
    a.act = act; a.leaky_slope = slope; a.aux[0] = aux_pm; a.mask_mode = mask_mode;
    return vsr_launch_conv(dtype, 3, 1, 16, 16, 1, 64, EPI_NHWC, a, c.st);
}

// Weight and bias gradient of a 64 -> pc (1..3) 3x3 conv with a planar fp32 cotangent (images dy_nstride floats apart): conv_last.2, the
// pre-clean out conv, conv_9 -- wgrad_run() with the engines' shape + the fixed-order reduction.  gw (pc,64,3,3) and gb (pc) are overwritten.
// slab: vsr_conv3x3_c64_wgrad_slab_floats() floats.  bf16: last2_wgrad_ring_kernel (W % 4 == 0, dy and dy_nstride 16-byte aligned) or
// last2_wgrad_kernel; fp32: the generic kernel.
int vsr_debug_tail_last2_wgrad(int dtype, const void* x_pm, const float* dy, long long dy_nstride, int pc, float* gw, float* gb, float* slab,
                               int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !x_pm || !dy || !gw || !slab || bad_dims(N, H, W) || pc < 1 || pc > 3 || dy_nstride < (long long)pc * H * W)
        return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, 64, slab);
    WgradArgs a = wg_base(N, H, W, 64, 64);
    a.x[0] = x_pm; a.dy[0] = dy; a.dy_nstride = dy_nstride; a.dy_planar_c = pc;
    return c.wgrad(a, {3, 64, false, 16, true}, {pc, 64, gw, 64, 0, 1, 0, gb, 0});
}

// Ctx::conv(..., unshuffle = true) (bf16 only: the persistent kernel): y = conv3x3 64 -> 64 of x_pm (N x H x W, H and W even) + bias, written
// as four phase planes of N x H/2 x W/2.  mode: Ctx::pack_cc's (0 forward weights, 1 data-gradient weights: conv_last.0's data gradient).
// wpack: 9 * 64 * 64 elements; y_planes: 4 * N * pm_image_elems(H/2, W/2, 64) elements.
int vsr_debug_tail_conv_unshuffle(int dtype, const void* x_pm, const float* w, const float* bias, int mode, void* wpack, void* y_planes,
                                  int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !x_pm || !w || !wpack || !y_planes || bad_dims(N, H, W) || (H & 1) || (W & 1) || (mode & ~1)) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack_cc(3, w, wpack, mode));
    return c.conv(3, x_pm, wpack, bias, y_planes, ACT_NONE, nullptr, nullptr, 0, N, H, W, nullptr, nullptr, true);
}

// Ctx::conv_ps_dgrad on Ctx::pack_ps's data-gradient weights: dy (N,2H,2W,64) -> dx (N,H,W,64) * mask(aux).  w (256,64,3,3); wpack: 4 * 9 * 64 * 64
// elements.  dy_planes / dx_planes: that tensor is phase-separated (bf16 only; dx_planes needs H, W even).  mask_src as above (sign bits: bf16).
int vsr_debug_tail_ps_dgrad(int dtype, const void* dy_pm, const float* w, void* wpack, void* dx_pm, const void* aux_pm, int mask_mode, int mask_src,
                            void* sign_scratch, int dy_planes, int dx_planes, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !dy_pm || !w || !wpack || !dx_pm || bad_dims(N, H, W) || mask_src < 0 || mask_src > 2 || (dy_planes & ~1) || (dx_planes & ~1))
        return VSR_ERR_BADARG;
    if (mask_src != 0 && (!aux_pm || (mask_mode != MASK_RELU && mask_mode != MASK_LEAKY))) return VSR_ERR_BADARG;
    if (mask_src == 2 && !sign_scratch) return VSR_ERR_BADARG;
    if (dtype != VSR_BF16 && (dy_planes || dx_planes || mask_src == 2)) return VSR_ERR_UNSUPPORTED;      // the fp32 recipe has the strided form only
    if (dx_planes && ((H & 1) || (W & 1))) return VSR_ERR_BADARG;
    if (dx_planes && mask_src) return VSR_ERR_UNSUPPORTED;                                              // no kernel masks a phase-separated destination
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack_ps(w, wpack, 1));
    if (mask_src == 2) CK(vsr_launch_sign_bits_c64(aux_pm, sign_scratch, N, H, W, c.st));
    return c.conv_ps_dgrad(dy_pm, wpack, dx_pm, mask_src ? aux_pm : nullptr, mask_src ? mask_mode : MASK_NONE, N, H, W,
                           mask_src == 2 ? sign_scratch : nullptr, dy_planes != 0, dx_planes != 0);
}

// Ctx::ps_wgrads, one segment: x (N,H,W,64), dy (N,2H,2W,64) strided or phase-separated; gw (256,64,3,3) and gb (256) are overwritten.
int vsr_debug_tail_ps_wgrads(int dtype, const void* x_pm, const void* dy_pm, int dy_planes, float* gw, float* gb, float* slab, int N, int H, int W,
                             void* stream) {
    if (bad_dtype(dtype) || !x_pm || !dy_pm || !gw || !slab || bad_dims(N, H, W) || (dy_planes & ~1)) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, 64, slab);
    return c.ps_wgrads(&x_pm, &dy_pm, 1, dy_planes != 0, N, H, W, gw, gb, 0);
}

}  // extern "C"
