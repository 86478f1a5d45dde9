// Test hooks for SPyNet (not in the header): each runs ONE launch of spynet_engine.hip's spynet_run / spynet_backward on the caller's
// buffers, through the Ctx member (recipes.h) or the vsr_launch_* function the engine calls, with the weight packs spynet_pack makes for
// layer j.  Argument checks and launches only: no kernel lives here.  tests/test_spynet_gpu.py compares every hook with an fp64
// restatement.
//   j: the layer of a level, 0..4 (SPY_CI[j] -> SPY_CO[j] channels, 7x7); w: fp32 OIHW (SPY_CO[j], SPY_CI[j], 7, 7); *_pm: blocked
//   pixel-major of the element type of `dtype`, with SPY_CIP[j] channels (a layer's input), SPY_CD[j] (its output, j < 4) or
//   SPY_DK[j] (the gradient of its output); planar tensors are fp32.  wpack: 49 * 64 * 64 elements; slab:
//   vsr_conv3x3_c64_wgrad_slab_floats() floats.
#include "recipes.h"
#include "debug_hooks.h"

namespace {
bool bad_layer(int j) { return j < 0 || j >= NSPY; }
}  // namespace

extern "C" {

// Ctx::spy_conv(j) on Ctx::pack_spy(j, w, ., 0): y = act(conv7x7(x) + bias), act ReLU or none.  j < 4: y_pm pixel-major; j = 4: y planar
// fp32 (N, 2, H, W) (+ pres, planar fp32, which no other layer takes).
int vsr_debug_spy_conv(int dtype, int j, const void* x_pm, const float* w, const float* bias, void* wpack, void* y, int act, const float* pres,
                       int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_layer(j) || !x_pm || !w || !wpack || !y || bad_dims(N, H, W) || (act != ACT_NONE && act != ACT_RELU)) return VSR_ERR_BADARG;
    if (pres && j != NSPY - 1) return VSR_ERR_UNSUPPORTED;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack_spy(j, w, wpack, 0));
    return c.spy_conv(j, x_pm, wpack, bias, y, act, 0.f, pres, N, H, W);
}

// Ctx::spy_dgrad(j) on Ctx::pack_spy(j, w, ., 1): dx = dgrad(conv_j)(dy) (* (aux > 0)); aux_pm: the layer's stored input (SPY_CIP[j] channels)
// or NULL.  Layer 0's input is no activation: no kernel masks its 8 real channels.
int vsr_debug_spy_dgrad(int dtype, int j, const void* dy_pm, const float* w, void* wpack, void* dx_pm, const void* aux_pm, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_layer(j) || !dy_pm || !w || !wpack || !dx_pm || bad_dims(N, H, W)) return VSR_ERR_BADARG;
    if (aux_pm && j == 0) return VSR_ERR_UNSUPPORTED;
    const Ctx c(nullptr, (hipStream_t)stream, dtype);
    CK(c.pack_spy(j, w, wpack, 1));
    return c.spy_dgrad(j, dy_pm, wpack, dx_pm, aux_pm, N, H, W);
}

// Ctx::spy_wgrad(j): gw (SPY_CO[j], SPY_CI[j], 7, 7) and gb (SPY_CO[j]) or NULL from x (the layer's input) and dy (the gradient of its
// output); accumulate: add to what gw / gb hold, else overwrite.
int vsr_debug_spy_wgrad(int dtype, int j, const void* x_pm, const void* dy_pm, float* gw, float* gb, int accumulate, float* slab, int N, int H, int W,
                        void* stream) {
    if (bad_dtype(dtype) || bad_layer(j) || !x_pm || !dy_pm || !gw || !slab || bad_dims(N, H, W) || (accumulate & ~1)) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, 64, slab);
    return c.spy_wgrad(j, x_pm, dy_pm, N, H, W, gw, gb, accumulate);
}

// vsr_launch_spynet_prepare: frames (F, 3, h, w) planar; level0: flow_prev NULL, flow_up = 0; else flow_prev (P, 2, h/2, w/2), h and w
// even.  pair_mode 0: P = 2 n (t - 1), F = n t; pair_mode 1: F = 2 P (n, t unused).  Writes flow_up (P, 2, h, w) and x16_pm.
int vsr_debug_spy_prepare(int dtype, const float* frames, const float* flow_prev, float* flow_up, void* x16_pm, int n, int t, int P, int pair_mode,
                          int h, int w, int level0, void* stream) {
    if (bad_dtype(dtype) || !frames || !flow_up || !x16_pm || bad_dims(P, h, w) || (pair_mode & ~1) || (level0 & ~1) || (level0 != 0) != (flow_prev == nullptr))
        return VSR_ERR_BADARG;
    if (!pair_mode && (n < 1 || t < 2 || P != 2 * n * (t - 1))) return VSR_ERR_BADARG;
    if (!level0 && ((h | w) & 1)) return VSR_ERR_BADARG;
    return vsr_launch_spynet_prepare(dtype, frames, flow_prev, flow_up, x16_pm, n, t, P, pair_mode, h, w, level0, (hipStream_t)stream);
}

// vsr_launch_spynet_prepare_bwd in the engine's three forms: level 0 (flow_up, dflow_l, dflow_prev NULL; dframes given) and level > 0
// (flow_up, dflow_l, dflow_prev given; dframes given or NULL); neither destination is never launched and refused here.  dflow_prev
// (P, 2, h/2, w/2) and dframes (F, 3, h, w) are ADDED to.
int vsr_debug_spy_prepare_bwd(int dtype, const void* dx16_pm, const float* dflow_l, const float* frames, const float* flow_up, float* dflow_prev,
                              float* dframes, int n, int t, int P, int pair_mode, int h, int w, void* stream) {
    if (bad_dtype(dtype) || !dx16_pm || !frames || bad_dims(P, h, w) || (pair_mode & ~1) || (!dflow_prev && !dframes)) return VSR_ERR_BADARG;
    if (!pair_mode && (n < 1 || t < 2 || P != 2 * n * (t - 1))) return VSR_ERR_BADARG;
    if (dflow_prev ? (!flow_up || !dflow_l || ((h | w) & 1)) : (flow_up || dflow_l)) return VSR_ERR_BADARG;
    return vsr_launch_spynet_prepare_bwd(dtype, dx16_pm, dflow_l, frames, flow_up, dflow_prev, dframes, n, t, P, pair_mode, h, w, (hipStream_t)stream);
}

// vsr_launch_spynet_dres: out_pm (16 channels) = dflow (P, 2, h, w) * (res > 0) in channels 0 and 1, zeros behind; res NULL: no mask.
int vsr_debug_spy_dres(int dtype, const float* dflow, const float* res, void* out_pm, int P, int h, int w, void* stream) {
    if (bad_dtype(dtype) || !dflow || !out_pm || bad_dims(P, h, w)) return VSR_ERR_BADARG;
    return vsr_launch_spynet_dres(dtype, dflow, res, out_pm, P, h, w, (hipStream_t)stream);
}

// The planar fp32 launches of the pyramid, one per `op`; `planes` images of (h, w), resized to / from (hu, wu) where the op resizes:
//   0 resize_norm      out (planes, 3, hu, wu) = (resize(in (planes, 3, h, w)) - mean) / std
//   1 resize_norm_bwd  out (planes, 3, h, w)  += resize^T(in (planes, 3, hu, wu)) / std
//   2 avgpool2         out (planes, h/2, w/2)  = 2x2 means of in (planes, h, w), h and w even
//   3 avgpool2_bwd_add out (planes, h, w)     += in (planes, h/2, w/2) / 4
//   4 flow_out         out (planes, 2, h, w)   = resize(in (planes, 2, hu, wu)) * (w / wu, h / hu)
//   5 flow_out_bwd     out (planes, 2, hu, wu) += resize^T(in (planes, 2, h, w)) * (w / wu, h / hu)
//   6 add_f32          out = in + in2, planes * h * w elements
int vsr_debug_spy_planar(int op, const float* in, const float* in2, float* out, const float* mean, const float* std, long long planes, int h, int w,
                         int hu, int wu, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (op < 0 || op > 6 || !in || !out || planes < 1 || planes > 0x7fffffff || h < 1 || w < 1) return VSR_ERR_BADARG;
    const bool resizes = op == 0 || op == 1 || op == 4 || op == 5;
    if (resizes && (hu < 1 || wu < 1)) return VSR_ERR_BADARG;
    if ((op == 0 && !mean) || (op <= 1 && !std) || (op == 6 && !in2)) return VSR_ERR_BADARG;
    if ((op == 2 || op == 3) && ((h | w) & 1)) return VSR_ERR_BADARG;
    switch (op) {
        case 0: return vsr_launch_resize_norm(in, out, mean, std, (int)planes, h, w, hu, wu, st);
        case 1: return vsr_launch_resize_norm_bwd(in, out, std, (int)planes, h, w, hu, wu, st);
        case 2: return vsr_launch_avgpool2(in, out, planes, h, w, st);
        case 3: return vsr_launch_avgpool2_bwd_add(in, out, planes, h, w, st);
        case 4: return vsr_launch_flow_out(in, out, (int)planes, hu, wu, h, w, st);
        case 5: return vsr_launch_flow_out_bwd(in, out, (int)planes, hu, wu, h, w, st);
        default: return vsr_launch_add_f32(in, in2, out, planes * h * w, st);
    }
}

}  // extern "C"
