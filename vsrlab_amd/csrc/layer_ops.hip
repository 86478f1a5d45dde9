// The per-op C ABI: one layer (or one elementwise step) per call on the caller's buffers, through the same launch recipes as the
// engines.  Argument checks and launches only.
#include "recipes.h"
#include "debug_hooks.h"

constexpr int C64 = 64;         // the fixed width of the vsr_conv3x3_c64_* entries and of vsr_conv_layer_bwd's scratch layout

extern "C" {

// ---- per-op entry points -------------------------------------------------------------------------
static bool layer_width_ok(int c) { return c == 16 || c == 32 || c == 64; }      // the widths of the per-op trunk / stem / shuffle layers

int vsr_flow_warp_fwd(int dtype, const void* in_pm, const float* flow, void* out_pm, int N, int H, int W, int Cc, void* stream) {
    return vsr_flow_warp_fwd_ex(dtype, in_pm, flow, out_pm, N, H, W, Cc, 0, stream);
}
int vsr_flow_warp_bwd(int dtype, const void* dout_pm, const float* flow, float* dacc, int N, int H, int W, int Cc, void* stream) {
    return vsr_flow_warp_bwd_ex(dtype, dout_pm, flow, dacc, N, H, W, Cc, 0, stream);
}
int vsr_flow_warp_bwd_flow(int dtype, const void* in_pm, const void* dout_pm, const float* flow, float* dflow, int N, int H, int W,
                           int Cc, void* stream) {
    return vsr_flow_warp_bwd_flow_ex(dtype, in_pm, dout_pm, flow, dflow, N, H, W, Cc, 0, stream);
}
/* padding_mode: 0 = 'zeros' (the propagation warps), 1 = 'border' (the warps inside SPyNet, spynet.py:60) */
int vsr_flow_warp_fwd_ex(int dtype, const void* in_pm, const float* flow, void* out_pm, int N, int H, int W, int Cc, int padding_mode,
                         void* stream) {
    if (bad_dtype(dtype) || !in_pm || !flow || !out_pm || bad_dims(N, H, W) || Cc < 16 || (Cc & 15) || (padding_mode & ~1)) return VSR_ERR_BADARG;
    return vsr_launch_warp_fwd(dtype, in_pm, flow, out_pm, N, H, W, Cc, (long long)2 * H * W, (hipStream_t)stream, padding_mode);
}
int vsr_flow_warp_bwd_ex(int dtype, const void* dout_pm, const float* flow, float* dacc, int N, int H, int W, int Cc, int padding_mode,
                         void* stream) {
    if (bad_dtype(dtype) || !dout_pm || !flow || !dacc || bad_dims(N, H, W) || Cc < 16 || (Cc & 15) || (padding_mode & ~1)) return VSR_ERR_BADARG;
    return vsr_launch_warp_bwd(dtype, dout_pm, flow, dacc, N, H, W, Cc, (long long)2 * H * W, (hipStream_t)stream, padding_mode);
}
// Test hook (not in the header): the engine's GATHER form of the 64-channel zeros-padding warp adjoint on its own -- out = T(dtop + adjoint(dout)),
// near sources gathered, far ones through the 64-bit fixed-point accumulator S (N*H*W*64 long longs, all zero on entry and exit;
// far_count: one zeroed int).  tests: against the scatter form above, and that a non-finite far contribution stays non-finite.
// Both are vsr_debug_warp_gather (warp_hooks.hip) at flow_nstride = 2HW.
extern "C" int vsr_debug_warp_bwd_gather(int dtype, const void* dout_pm, const float* flow, const void* dtop_pm, long long* S, int* far_count,
                                         void* out_pm, int N, int H, int W, void* stream) {
    return vsr_debug_warp_gather(dtype, 64, dout_pm, flow, (long long)2 * H * W, dtop_pm, S, far_count, out_pm, N, H, W, stream);
}
// ... the same at Cc = 16, 32 or 64 channels (S: N*H*W*Cc long longs): the narrow engine's propagation warps
extern "C" int vsr_debug_warp_bwd_gather_c(int dtype, const void* dout_pm, const float* flow, const void* dtop_pm, long long* S, int* far_count,
                                           void* out_pm, int N, int H, int W, int Cc, void* stream) {
    return vsr_debug_warp_gather(dtype, Cc, dout_pm, flow, (long long)2 * H * W, dtop_pm, S, far_count, out_pm, N, H, W, stream);
}
int vsr_flow_warp_bwd_flow_ex(int dtype, const void* in_pm, const void* dout_pm, const float* flow, float* dflow, int N, int H, int W,
                              int Cc, int padding_mode, void* stream) {
    if (bad_dtype(dtype) || !in_pm || !dout_pm || !flow || !dflow || bad_dims(N, H, W) || Cc < 16 || (Cc & 15) || (padding_mode & ~1)) return VSR_ERR_BADARG;
    return vsr_launch_warp_bwd_flow(dtype, in_pm, dout_pm, flow, dflow, N, H, W, Cc, (long long)2 * H * W, (hipStream_t)stream, padding_mode);
}
int vsr_planar_to_pm(int dtype, const float* in, void* out_pm, int N, int Cin, int H, int W, int Cc, void* stream) {
    if (bad_dtype(dtype) || !in || !out_pm || bad_dims(N, H, W) || Cin < 1 || Cc < Cin || (Cc & 15)) return VSR_ERR_BADARG;
    return vsr_launch_planar_to_pm(dtype, in, out_pm, N, Cin, H, W, Cc, (hipStream_t)stream);
}
int vsr_pm_to_planar(int dtype, const void* in_pm, float* out, int N, int Cout, int H, int W, int Cc, void* stream) {
    if (bad_dtype(dtype) || !in_pm || !out || bad_dims(N, H, W) || Cout < 1 || Cc < Cout || (Cc & 15)) return VSR_ERR_BADARG;
    return vsr_launch_pm_to_planar(dtype, in_pm, out, N, Cout, H, W, Cc, (hipStream_t)stream);
}

int vsr_conv3x3_c64_fwd(int dtype, const void* x_pm, const float* w, const float* b, void* wpack, void* y_pm, const void* res_pm,
                        int act, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !x_pm || !wpack || !y_pm || bad_dims(N, H, W) || act < ACT_NONE || act > ACT_LEAKY) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    if (w) CK(c.pack_cc(3, w, wpack, 0));   // w == NULL: wpack already packed
    return c.conv(3, x_pm, wpack, b, y_pm, act, res_pm, nullptr, 0, N, H, W);
}

size_t vsr_conv3x3_c64_chain_sync_bytes(int nlayers, int N, int H, int W) {
    if (nlayers < 1 || nlayers > VSR_CHAIN_MAX_LAYERS || bad_dims(N, H, W)) return 0;
    return vsr_chain_sync_bytes(nlayers, N, H, W);
}

int vsr_conv3x3_c64_chain_fwd(const void* images, const void* wpack, const float* bias, int nlayers, int N, int H, int W, void* sync,
                              void* stream) {
    if (!images || !wpack || !bias || !sync || nlayers < 1 || nlayers > VSR_CHAIN_MAX_LAYERS || bad_dims(N, H, W)) return VSR_ERR_BADARG;
    const size_t img = (size_t)N * pm_image_elems(H, W, C64) * 2, wset = (size_t)9 * C64 * C64 * 2;
    // the kernel addresses every operand as a 32-bit offset (x 256 B) from one base
    uintptr_t lo = (uintptr_t)images;
    if ((uintptr_t)wpack < lo) lo = (uintptr_t)wpack;
    if ((uintptr_t)bias < lo) lo = (uintptr_t)bias;
    lo &= ~(uintptr_t)255;
    auto off = [&](const void* p, size_t add, unsigned* out) {
        const uintptr_t d = (uintptr_t)p + add - lo;
        if ((d & 255) || (d >> 8) >= 0xffffffffull) return false;
        *out = (unsigned)(d >> 8);
        return true;
    };
    ChainArgs a = {};
    a.base = (char*)lo; a.sync = (unsigned*)sync; a.N = N; a.H = H; a.W = W; a.nlayers = nlayers;
    for (int l = 0; l < nlayers; ++l) {
        ChainLayer& L = a.layer[l];
        L = {0, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0, 0, (l & 1) ? CHAIN_SKIP : CHAIN_RELU};
        bool ok = off(images, (size_t)l * img, &L.src) && off(images, (size_t)(l + 1) * img, &L.dst) && off(wpack, (size_t)l * wset, &L.w) &&
                  off(bias, (size_t)l * C64 * 4, &L.bias);
        if (l & 1) ok = ok && off(images, (size_t)(l - 1) * img, &L.res);
        if (!ok) return VSR_ERR_UNSUPPORTED;
    }
    return vsr_launch_conv3x3_chain(a, vsr_num_cus(), (hipStream_t)stream);
}

int vsr_conv3x3_c64_dgrad(int dtype, const void* dy_pm, const float* w, void* wpack, void* dx_pm, const void* res_pm,
                          const void* aux_pm, int mask_mode, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !dy_pm || !w || !wpack || !dx_pm || bad_dims(N, H, W) || mask_mode < MASK_NONE || mask_mode > MASK_LEAKY ||
        (mask_mode != MASK_NONE && !aux_pm))
        return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack_cc(3, w, wpack, 1));
    return c.conv(3, dy_pm, wpack, nullptr, dx_pm, ACT_NONE, res_pm, aux_pm, mask_mode, N, H, W);
}

/* Backward of ONE conv layer of vsr_conv_layer_fwd (same shapes, same argument meaning): the reference's building blocks are ordinary
 * autograd modules (core/modules/conv.py:15-22,94-103, upsampling.py:4-12, spynet.py:13-21), so each layer needs its data gradient,
 * weight gradient and bias gradient on its own.  Every piece is a kernel the engines already run:
 *   dyM = dy * act'(y)           (mask_pm / spynet_dres; act'(y) from the layer's stored OUTPUT y: ReLU / LeakyReLU keep the sign)
 *   dx  = conv(dyM, flipped W)   (the forward kernels on weights packed with mode 1; pixel-shuffle: four phase launches)
 *   dlr = the stems' 3 planar LR channels (64 -> 3 planar kernel)
 *   gw, gb = wgrad(x, dyM)       (producer/consumer kernel for 3x3 64->64, generic kernel otherwise; reduced in a fixed order)
 * x_pm / lr_planar / y_* as given to / returned by the forward; dy_* has y's layout.  dx_pm, dlr_planar, gw, gb may be NULL (not
 * needed); gw / gb are OVERWRITTEN.  scratch: vsr_conv_layer_bwd_scratch_bytes(...) bytes.                                         */
size_t vsr_conv_layer_bwd_scratch_bytes(int dtype, int N, int H, int W, int pixel_shuffle) {
    if (bad_dtype(dtype) || bad_dims(N, H, W)) return 0;
    const size_t es = esize(dtype);
    const int s = pixel_shuffle ? 2 : 1;
    return (size_t)49 * 64 * 64 * 4 * es + (size_t)N * pm_image_elems(s * H, s * W, C64) * es + wgrad_slab_bytes() + 1024;
}

int vsr_conv_layer_bwd(int dtype, int ks, const void* x_pm, int cin_pm, const float* lr_planar, const float* w, int cin_real, int cout_real,
                       const void* y_pm, const float* y_planar, const void* dy_pm, const float* dy_planar, int cd, int act, float slope,
                       int pixel_shuffle, void* dx_pm, float* dlr_planar, float* gw, float* gb, void* scratch, size_t scratch_bytes,
                       int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !w || !scratch || bad_dims(N, H, W) || (!x_pm && !lr_planar) || (!dy_pm && !dy_planar) || act < ACT_NONE || act > ACT_LEAKY)
        return VSR_ERR_BADARG;
    if (act != ACT_NONE && !(dy_pm ? y_pm != nullptr : y_planar != nullptr)) return VSR_ERR_BADARG;     // the mask needs the layer's output
    if (scratch_bytes < vsr_conv_layer_bwd_scratch_bytes(dtype, N, H, W, pixel_shuffle)) return VSR_ERR_WORKSPACE;
    if (pixel_shuffle && !layer_width_ok(cin_pm)) return VSR_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const size_t es = esize(dtype);
    char* wp = (char*)scratch;
    char* dym = wp + (size_t)49 * 64 * 64 * 4 * es;
    const int sps = pixel_shuffle ? 2 : 1;
    float* slab = reinterpret_cast<float*>(dym + (((size_t)N * pm_image_elems(sps * H, sps * W, C64) * es + 255) & ~(size_t)255));
    const float mslope = act == ACT_LEAKY ? vsr_slope(slope) : 0.f;

    if (!dy_pm) {   // planar output: the 16 -> 2 SPyNet layer.  dyM as a 16-channel pixel-major tensor
        if (ks != 7 || cout_real != 2 || cin_pm != 16 || cin_real != 16 || !x_pm || pixel_shuffle) return VSR_ERR_UNSUPPORTED;
        if (act == ACT_RELU) CK(vsr_launch_spynet_dres(dtype, dy_planar, y_planar, dym, N, H, W, st));
        else if (act == ACT_NONE) CK(vsr_launch_planar_to_pm(dtype, dy_planar, dym, N, 2, H, W, 16, st));
        else return VSR_ERR_UNSUPPORTED;
    } else if (act != ACT_NONE) {
        const int cdy = pixel_shuffle ? cin_pm : cd;
        CK(vsr_launch_mask_pm(dtype, dy_pm, y_pm, dym, mslope, (long long)N * pm_image_elems(sps * H, sps * W, cdy), st));
    }
    const void* dyM = (!dy_pm || act != ACT_NONE) ? (const void*)dym : dy_pm;

    // (gw / gb are overwritten: every reduction below writes its own part of them)
    if (lr_planar) {                                       // stems: cat([lr(3), feat(C)]) or lr alone  (conv.py:97), C = 16, 32 or 64
        const int C = cout_real;
        if (ks != 3 || !layer_width_ok(C) || cd != C || pixel_shuffle) return VSR_ERR_UNSUPPORTED;
        const bool cat = x_pm != nullptr;
        if ((cat && (cin_pm != C || cin_real != C + 3)) || (!cat && cin_real != 3)) return VSR_ERR_UNSUPPORTED;
        const Ctx c(nullptr, st, dtype, C, slab);
        if (cat && dx_pm) {
            CK(c.pack_stem_dgrad(w, wp));
            CK(c.conv(3, dyM, wp, nullptr, dx_pm, ACT_NONE, nullptr, nullptr, 0, N, H, W));
        }
        if (dlr_planar) {
            CK(c.pack_stem_dlr(w, wp, cat));
            CK(c.conv_planar3(dyM, wp, nullptr, dlr_planar, (long long)3 * H * W, nullptr, N, H, W));
        }
        if (gw) {
            WgradArgs a = wg_base(N, H, W, C, C), af = a;
            a.x[0] = lr_planar; a.x_nstride = (long long)3 * H * W; a.dy[0] = dyM;
            af.x[0] = x_pm; af.dy[0] = dyM;
            CK(c.stem_wgrads(cat, a, af, gw, gb, 0));
        }
        return VSR_OK;
    }
    if (ks == 3 || ks == 1) {
        const int C = cin_pm;
        if (!layer_width_ok(C) || cin_real != C || !x_pm) return VSR_ERR_UNSUPPORTED;
        const Ctx c(nullptr, st, dtype, C, slab);
        if (pixel_shuffle) {                               // conv3x3 C -> 4C + PixelShuffle(2)  (upsampling.py:10-12)
            if (ks != 3 || cout_real != 4 * C || cd != C || act != ACT_NONE) return VSR_ERR_UNSUPPORTED;
            if (dx_pm) {
                CK(c.pack_ps(w, wp, 1));
                CK(c.conv_ps_dgrad(dyM, wp, dx_pm, nullptr, 0, N, H, W));
            }
            if (gw) CK(c.ps_wgrads(&x_pm, &dyM, 1, false, N, H, W, gw, gb, 0));
            return VSR_OK;
        }
        if (cout_real != C || cd != C) return VSR_ERR_UNSUPPORTED;
        if (dx_pm) {
            CK(c.pack_cc(ks, w, wp, 1));
            CK(c.conv(ks, dyM, wp, nullptr, dx_pm, ACT_NONE, nullptr, nullptr, 0, N, H, W));
        }
        if (gw) {
            WgradArgs a = wg_base(N, H, W, C, C);
            a.x[0] = x_pm; a.dy[0] = dyM;
            CK(c.wgrad_cc(ks, a, gw, C, 0, gb, 0));
        }
        return VSR_OK;
    }
    if (ks != 7 || pixel_shuffle || !x_pm) return VSR_ERR_UNSUPPORTED;
    for (int j = 0; j < NSPY; ++j) {                       // the SPyNet layer shapes (spynet.py:16-18), as spynet_backward runs them
        if (cin_pm != SPY_CIP[j] || cout_real != SPY_CO[j] || cin_real != SPY_CI[j]) continue;
        if (j < NSPY - 1 && cd != SPY_CD[j]) return VSR_ERR_BADARG;
        const Ctx c(nullptr, st, dtype, 64, slab);
        if (gw) CK(c.spy_wgrad(j, x_pm, dyM, N, H, W, gw, gb, 0));
        if (dx_pm) {
            CK(c.pack_spy(j, w, wp, 1));
            CK(c.spy_dgrad(j, dyM, wp, dx_pm, nullptr, N, H, W));
        }
        return VSR_OK;
    }
    return VSR_ERR_UNSUPPORTED;
}

/* One convolution layer on blocked pixel-major tensors, forward only: the building blocks the reference's modules expose
 * on their own (ConvReLU core/modules/conv.py:15-22, SpynetModule spynet.py:13-21, PixelShufflePack upsampling.py:4-12,
 * the stem of ResidualBlock conv.py:97).  w: fp32 OIHW (cout_real, cin_real [+3 for lr_planar], ks, ks); b: cout_real or NULL.
 *   ks 3 or 1: x_pm has 64 channels, 64 outputs (pixel_shuffle: 256 outputs written as (N,2H,2W,64), upsampling.py:10-12);
 *   ks 7: (cin_pm, cout) in {(16,32), (32,64), (64,32), (32,16), (16,2 -> y_planar)} (the SPyNet layers);
 *   lr_planar (N,3,H,W) fp32, ks 3: the conv reads cat([lr, x]) (x_pm may be NULL = lr only): the trunk / pre-clean stems.
 * y_pm has cd channels per pixel (16 / 32 / 64); y_planar (N,cout_real,H,W) fp32 instead when cout_real <= 4.
 * wpack: scratch of 49 * 64 * 64 * 4 elements of `dtype` (packed weights of this call).                               */
int vsr_conv_layer_fwd(int dtype, int ks, const void* x_pm, int cin_pm, const float* lr_planar, const float* w, const float* b,
                       int cin_real, int cout_real, void* wpack, void* y_pm, int cd, float* y_planar, int act, float slope,
                       int pixel_shuffle, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !w || !wpack || bad_dims(N, H, W) || (!x_pm && !lr_planar) || (!y_pm && !y_planar) || act < ACT_NONE || act > ACT_LEAKY)
        return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    char* wp = (char*)wpack;
    // (the kernels read the bias as fp32 from device memory: the caller's tensor is used as is -- cout_real values, padded reads are masked by cout_real)
    if (lr_planar) {                                       // stems: cat([lr(3), feat(C)]) or lr alone, C = 16, 32 or 64
        const int C = cout_real;
        if (ks != 3 || !layer_width_ok(C) || !y_pm || cd != C || pixel_shuffle) return VSR_ERR_UNSUPPORTED;
        const bool cat = x_pm != nullptr;
        if (cat ? (cin_pm != C || cin_real != C + 3) : cin_real != 3) return VSR_ERR_UNSUPPORTED;
        const Ctx c(nullptr, st, dtype, C);
        CK(c.pack_stem(w, wp, cat));
        return c.stem(cat, x_pm, lr_planar, (long long)3 * H * W, wp, b, y_pm, act, slope, N, H, W);
    }
    if (ks == 3 || ks == 1) {
        const int C = cin_pm;
        if (!layer_width_ok(C) || cin_real != C) return VSR_ERR_UNSUPPORTED;
        const Ctx c(nullptr, st, dtype, C);
        if (pixel_shuffle) {
            if (ks != 3 || cout_real != 4 * C || !y_pm || cd != C) return VSR_ERR_UNSUPPORTED;
            CK(c.pack_ps(w, wp, 0));
            float* b4 = reinterpret_cast<float*>(wp + (size_t)4 * 9 * c.CO * C * c.es);
            if (b) CK(c.pack_ps_bias(b, b4));
            return c.conv_ps(x_pm, wp, b ? b4 : nullptr, y_pm, N, H, W, act, slope);
        }
        if (cout_real != C || !y_pm || cd != C) return VSR_ERR_UNSUPPORTED;
        CK(c.pack_cc(ks, w, wp, 0));
        return c.conv(ks, x_pm, wp, b, y_pm, act, nullptr, nullptr, 0, N, H, W, nullptr, nullptr, false, slope);
    }
    if (ks != 7 || pixel_shuffle) return VSR_ERR_UNSUPPORTED;
    for (int j = 0; j < NSPY; ++j) {
        if (cin_pm != SPY_CIP[j] || cout_real != SPY_CO[j] || cin_real != SPY_CI[j]) continue;
        const Ctx c(nullptr, st, dtype);
        CK(c.pack_spy(j, w, wp, 0));
        if (j < NSPY - 1 ? (!y_pm || cd != SPY_CD[j]) : !y_planar) return VSR_ERR_BADARG;
        return c.spy_conv(j, x_pm, wp, b, j < NSPY - 1 ? y_pm : (void*)y_planar, act, slope, nullptr, N, H, W);
    }
    return VSR_ERR_UNSUPPORTED;
}

size_t vsr_conv3x3_c64_wgrad_slab_floats(void) { return wgrad_slab_floats(); }

int vsr_conv3x3_c64_wgrad(int dtype, const void* x_pm, const void* dy_pm, float* gw, float* gb, float* slab, int N, int H, int W,
                          void* stream) {
    if (bad_dtype(dtype) || !x_pm || !dy_pm || !gw || !slab || bad_dims(N, H, W)) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, 64, slab);
    WgradArgs a = wg_base(N, H, W);
    a.x[0] = x_pm; a.dy[0] = dy_pm;
    return c.wgrad(a, {3, 64, false, 64, false}, {C64, C64, gw, C64, 0, 1, 0, gb, 0}, false);      // an odd tile count stays odd: wgrad_run()
}

size_t vsr_charbonnier_scratch_floats(void) { return (size_t)vsr_charbonnier_scratch_floats_impl(); }
int vsr_charbonnier_fwd_bwd(const float* sr, const float* hr, float* dsr, float* loss, float* scratch, long long numel, float eps, void* stream) {
    if (!sr || !hr || !dsr || !loss || !scratch || numel < 1) return VSR_ERR_BADARG;
    return vsr_launch_charbonnier_grad(sr, hr, dsr, loss, scratch, numel, eps, (hipStream_t)stream);
}

}  // extern "C"
