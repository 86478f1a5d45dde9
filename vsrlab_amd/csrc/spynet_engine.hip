// SPyNet on the HIP path: weight packing, forward and backward for P frame pairs (shared with the BasicVSR engine through
// spynet_engine.h) and the stand-alone vsr_spynet_* entries.  No allocation, no synchronisation, no global state.
#include "spynet_engine.h"

namespace vsr {

// ---- SPyNet (spynet.py:38-93) for P frame pairs ------------------------------------------------
// frames: planar fp32 (F,3,h,w).  pair_mode 0: BasicVSR pairing over (n,t) (basicvsr.py:32-35);
// pair_mode 1: frames = [ref_0..ref_{P-1}, supp_0..supp_{P-1}].
int spynet_pack(const Ctx& c, const SpyPlan& sp, const float* const* params, int base_idx) {
    for (int l = 0; l < 6; ++l)
        for (int j = 0; j < NSPY; ++j) {
            const float* w = params[base_idx + (l * NSPY + j) * 2];
            const float* b = params[base_idx + (l * NSPY + j) * 2 + 1];
            CK(c.pack_spy(j, w, c.at(sp.wpack[l][j]), 0));
            CK(c.pack_bias(b, c.at(sp.bias[l][j]), SPY_CO[j]));
            if (sp.save) CK(c.pack_spy(j, w, c.at(sp.wpackd[l][j]), 1));
        }
    return VSR_OK;
}

// last_relu: the reference's RealBasicVSR Spynet ends every level in a ReLU (spynet.py:16-18); the canonical SPyNet of
// vsr/models/VRT/modules/spynet.py:76 does not.  level_out[l] (optional, l = 0..5): the level's flow resized to
// (h >> (5-l), w >> (5-l)) like VRT's return_levels (VRT/modules/spynet.py:134-141).
int spynet_run(const Ctx& c, const SpyPlan& sp, const float* frames, const float* mean, const float* std, int n, int t,
               int pair_mode, float* flows_out, bool last_relu, float* const* level_out) {
    const int P = sp.P, F = sp.F, hu = sp.hu, wu = sp.wu;
    CK(vsr_launch_resize_norm(frames, (float*)c.at(sp.pyr[5]), mean, std, F, sp.h, sp.w, hu, wu, c.st));
    for (int l = 5; l > 0; --l)
        CK(vsr_launch_avgpool2(c.fat(sp.pyr[l]), (float*)c.at(sp.pyr[l - 1]), (long long)F * 3, hu >> (5 - l), wu >> (5 - l), c.st));
    size_t fprev = sp.flow_a, fcur = sp.flow_b;
    for (int l = 0; l < 6; ++l) {
        const int hl = hu >> (5 - l), wl = wu >> (5 - l);
        const size_t fup = sp.save ? sp.sfup[l] : sp.flow_up;
        const size_t bufs[NSPY + 1] = {sp.save ? sp.sx[l][0] : sp.x16, sp.save ? sp.sx[l][1] : sp.b32a, sp.save ? sp.sx[l][2] : sp.b64,
                                       sp.save ? sp.sx[l][3] : sp.b32b, sp.save ? sp.sx[l][4] : sp.b16, 0};
        CK(vsr_launch_spynet_prepare(c.dtype, c.fat(sp.pyr[l]), l == 0 ? nullptr : c.fat(fprev), (float*)c.at(fup), c.at(bufs[0]),
                                     n, t, P, pair_mode, hl, wl, l == 0, c.st));
        for (int j = 0; j < NSPY; ++j) {
            const int act = (j < NSPY - 1 || last_relu) ? ACT_RELU : ACT_NONE;     // RealBasicVSR's Spynet: ReLU after the LAST conv too (spynet.py:16-18)
            // the last layer: flow = flow_up + residue (spynet.py:65); save: keep the residue, its sign is the last ReLU's mask
            void* y = j < NSPY - 1 ? c.at(bufs[j + 1]) : c.at(sp.save ? sp.sres[l] : fcur);
            const float* pres = (j == NSPY - 1 && !sp.save) ? c.fat(fup) : nullptr;
            CK(c.spy_conv(j, c.at(bufs[j]), c.at(sp.wpack[l][j]), c.fat(sp.bias[l][j]), y, act, 0.f, pres, P, hl, wl));
            if (j == NSPY - 1 && sp.save)
                CK(vsr_launch_add_f32(c.fat(fup), c.fat(sp.sres[l]), (float*)c.at(fcur), (long long)P * 2 * hl * wl, c.st));
        }
        if (level_out && level_out[l])
            CK(vsr_launch_flow_out(c.fat(fcur), level_out[l], P, hl, wl, sp.h >> (5 - l), sp.w >> (5 - l), c.st));
        size_t tmp = fprev; fprev = fcur; fcur = tmp;
    }
    if (!flows_out) return VSR_OK;
    return vsr_launch_flow_out(c.fat(fprev), flows_out, P, hu, wu, sp.h, sp.w, c.st);
}

// Backward of spynet_run for train_flow (spynet.py:38-93): dflows_out = d loss / d flows (P,2,h,w) ->
// weight / bias gradients of the 6 x 5 convs (g[base_idx ...], OIHW fp32).  The frames are not differentiated.
// dframes (optional): (F,3,h,w) fp32, ACCUMULATED into: the gradient w.r.t. the input frames (through the pyramid).
// last_relu = false: the canonical SPyNet (no ReLU behind a level's last conv); dlevel (optional, 6 entries, NULL = none):
// cotangents of the per-level outputs of spynet_run's level_out (VRT's return_levels); dflows_out may then be NULL.
int spynet_backward(const Ctx& c, const SpyPlan& sp, const float* dflows_out, int n, int t, int pair_mode, float* const* g,
                    int base_idx, float* dframes, const float* std, bool last_relu, const float* const* dlevel) {
    const int P = sp.P, hu = sp.hu, wu = sp.wu;
    size_t dcur = sp.dfa, dprev = sp.dfb;
    HIP_CHECK_RET(hipMemsetAsync(c.at(dcur), 0, (size_t)P * 2 * hu * wu * 4, c.st));
    if (dflows_out) CK(vsr_launch_flow_out_bwd(dflows_out, (float*)c.at(dcur), P, hu, wu, sp.h, sp.w, c.st));
    if (dframes)
        for (int l = 0; l < 6; ++l)
            HIP_CHECK_RET(hipMemsetAsync(c.at(sp.dpyr[l]), 0, (size_t)sp.F * 3 * (hu >> (5 - l)) * (wu >> (5 - l)) * 4, c.st));
    for (int l = 5; l >= 0; --l) {
        const int hl = hu >> (5 - l), wl = wu >> (5 - l);
        if (dlevel && dlevel[l])   // this level's flow was also an output (resized to the frame's own pyramid size): add its cotangent
            CK(vsr_launch_flow_out_bwd(dlevel[l], (float*)c.at(dcur), P, hl, wl, sp.h >> (5 - l), sp.w >> (5 - l), c.st));
        // flow_l = flow_up + ReLU(conv5): dY of the last conv, as a 16-channel pixel-major tensor
        CK(vsr_launch_spynet_dres(c.dtype, c.fat(dcur), last_relu ? c.fat(sp.sres[l]) : nullptr, c.at(sp.dres), P, hl, wl, c.st));
        size_t dy = sp.dres;
        for (int j = NSPY - 1; j >= 0; --j) {
            float* gw = g ? g[base_idx + (l * NSPY + j) * 2] : nullptr;
            float* gb = g ? g[base_idx + (l * NSPY + j) * 2 + 1] : nullptr;
            CK(c.spy_wgrad(j, c.at(sp.sx[l][j]), c.at(dy), P, hl, wl, gw, gb, 1));
            if (j == 0 && l == 0 && !dframes) break;       // level 0's input depends on the frames only
            // dX_j = dgrad(conv_j)(dY_j) (* ReLU'(X_j) for j > 0: X_j is the previous conv's ReLU output)
            const size_t dx = (dy == sp.gA) ? sp.gB : sp.gA;
            CK(c.spy_dgrad(j, c.at(dy), c.at(sp.wpackd[l][j]), c.at(dx), j > 0 ? c.at(sp.sx[l][j]) : nullptr, P, hl, wl));
            dy = dx;
        }
        float* dfr = dframes ? (float*)c.at(sp.dpyr[l]) : nullptr;
        if (l == 0) {
            if (dfr) CK(vsr_launch_spynet_prepare_bwd(c.dtype, c.at(dy), nullptr, c.fat(sp.pyr[0]), nullptr, nullptr, dfr, n, t, P, pair_mode, hl, wl, c.st));
            break;
        }
        // x16 = [ref | warp(supp, flow_up) | flow_up], flow_up = 2 * up(flow_{l-1}): everything that reaches flow_{l-1}
        HIP_CHECK_RET(hipMemsetAsync(c.at(dprev), 0, (size_t)P * 2 * (hl / 2) * (wl / 2) * 4, c.st));
        CK(vsr_launch_spynet_prepare_bwd(c.dtype, c.at(dy), c.fat(dcur), c.fat(sp.pyr[l]), c.fat(sp.sfup[l]), (float*)c.at(dprev), dfr,
                                         n, t, P, pair_mode, hl, wl, c.st));
        const size_t tmp = dcur; dcur = dprev; dprev = tmp;
    }
    if (dframes) {   // pyramid adjoint: avg_pool2d from fine to coarse (spynet.py:44-45), then the /32 resize + normalisation
        for (int l = 1; l < 6; ++l)
            CK(vsr_launch_avgpool2_bwd_add(c.fat(sp.dpyr[l - 1]), (float*)c.at(sp.dpyr[l]), (long long)sp.F * 3, hu >> (5 - l), wu >> (5 - l), c.st));
        CK(vsr_launch_resize_norm_bwd(c.fat(sp.dpyr[5]), dframes, std, sp.F, sp.h, sp.w, hu, wu, c.st));
    }
    return VSR_OK;
}

}  // namespace vsr

extern "C" {

// ---- SPyNet alone ---------------------------------------------------------------------------------
struct SpyAlone { SpyPlan sp; size_t frames = 0, slab = 0, dframes = 0, total = 0; };
static SpyAlone spy_alone_plan(int N, int h, int w, int dtype, bool save) {
    SpyAlone s; Bump b;
    s.frames = b.take((size_t)2 * N * 3 * h * w * 4);
    s.sp.plan(b, N, 2 * N, h, w, dtype);
    if (save) {                                  // appended: the forward-only offsets do not move
        s.sp.plan_save(b, dtype);
        s.slab = b.take(wgrad_slab_bytes());
        s.dframes = b.take((size_t)2 * N * 3 * h * w * 4);
    }
    s.total = b.off;
    return s;
}
// the stand-alone forward / backward behind the four entries below (each entry checks its own arguments first)
static int spy_alone_forward(int N, int h, int w, int dtype, const float* const* params, const float* ref, const float* supp, float* flow,
                             bool last_relu, float* const* level_out, void* workspace, size_t workspace_bytes, int need_backward, void* stream) {
    if (bad_dtype(dtype)) return VSR_ERR_BADARG;
    const SpyAlone s = spy_alone_plan(N, h, w, dtype, need_backward != 0);
    if (workspace_bytes < s.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Ctx c((char*)workspace, st, dtype);
    const size_t fb = (size_t)N * 3 * h * w * 4;
    HIP_CHECK_RET(hipMemcpyAsync(c.at(s.frames), ref, fb, hipMemcpyDeviceToDevice, st));
    HIP_CHECK_RET(hipMemcpyAsync((char*)c.at(s.frames) + fb, supp, fb, hipMemcpyDeviceToDevice, st));
    CK(vsr::spynet_pack(c, s.sp, params, 0));
    return vsr::spynet_run(c, s.sp, c.fat(s.frames), params[60], params[61], N, 2, 1, flow, last_relu, level_out);
}
static int spy_alone_backward(int N, int h, int w, int dtype, float* const* grads, const float* dflow, const float* std, bool last_relu,
                              const float* const* dlevel, float* dref, float* dsupp, void* workspace, size_t workspace_bytes, void* stream) {
    if (bad_dtype(dtype)) return VSR_ERR_BADARG;
    if (grads) for (int k = 0; k < 60; k += 2) if (!grads[k] && grads[k + 1]) return VSR_ERR_BADARG;   // a bias gradient comes with its weight's
    const SpyAlone s = spy_alone_plan(N, h, w, dtype, true);
    if (workspace_bytes < s.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Ctx c((char*)workspace, st, dtype, 64, (float*)((char*)workspace + s.slab));
    const bool want = dref || dsupp;
    const size_t fb = (size_t)N * 3 * h * w * 4;
    if (want) HIP_CHECK_RET(hipMemsetAsync(c.at(s.dframes), 0, 2 * fb, st));
    CK(vsr::spynet_backward(c, s.sp, dflow, N, 2, 1, grads, 0, want ? (float*)c.at(s.dframes) : nullptr, std, last_relu, dlevel));
    if (dref) HIP_CHECK_RET(hipMemcpyAsync(dref, c.at(s.dframes), fb, hipMemcpyDeviceToDevice, st));
    if (dsupp) HIP_CHECK_RET(hipMemcpyAsync(dsupp, (char*)c.at(s.dframes) + fb, fb, hipMemcpyDeviceToDevice, st));
    return VSR_OK;
}

size_t vsr_spynet_workspace_bytes(int N, int h, int w, int dtype, int need_backward) {
    if (bad_dims(N, h, w)) return 0;
    return spy_alone_plan(N, h, w, dtype, need_backward != 0).total;
}

int vsr_spynet_forward(int N, int h, int w, int dtype, const float* const* params, int nparams, const float* ref,
                       const float* supp, float* flow, void* workspace, size_t workspace_bytes, int need_backward, void* stream) {
    if (N < 1 || h < 1 || w < 1 || !params || nparams != 62 || !ref || !supp || !flow || !workspace) return VSR_ERR_BADARG;
    return spy_alone_forward(N, h, w, dtype, params, ref, supp, flow, true, nullptr, workspace, workspace_bytes, need_backward, stream);
}

/* SPyNet with the options of the reference's OTHER SpyNet classes: last_relu = 0 is the canonical network
 * (vsr/models/VRT/modules/spynet.py:68-157); level_out: HOST array of 6 device pointers (NULL entries = not wanted), level l
 * receives the flow of pyramid level l resized to (h >> (5-l), w >> (5-l)) (its `return_levels`).  Forward only.       */
int vsr_spynet_forward_ex(int N, int h, int w, int dtype, const float* const* params, int nparams, const float* ref,
                          const float* supp, int last_relu, float* const* level_out, void* workspace, size_t workspace_bytes,
                          int need_backward, void* stream) {
    if (N < 1 || h < 32 || w < 32 || !params || nparams != 62 || !ref || !supp || !level_out || !workspace) return VSR_ERR_BADARG;
    return spy_alone_forward(N, h, w, dtype, params, ref, supp, nullptr, last_relu != 0, level_out, workspace, workspace_bytes, need_backward, stream);
}

int vsr_spynet_backward(int N, int h, int w, int dtype, float* const* grads, int nparams, const float* dflow, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (N < 1 || h < 1 || w < 1 || !grads || nparams != 62 || !dflow || !workspace) return VSR_ERR_BADARG;
    return spy_alone_backward(N, h, w, dtype, grads, dflow, nullptr, true, nullptr, nullptr, nullptr, workspace, workspace_bytes, stream);
}

/* the same, plus the gradient w.r.t. the two input frames: dref, dsupp (N,3,h,w) fp32 are WRITTEN (either may be NULL).
 * params: the 62 tensors of the forward (std is needed for the normalisation's adjoint); grads may be NULL (frozen net). */
int vsr_spynet_backward_ex(int N, int h, int w, int dtype, const float* const* params, float* const* grads, int nparams, const float* dflow,
                           int last_relu, const float* const* dlevel, float* dref, float* dsupp, void* workspace, size_t workspace_bytes,
                           void* stream) {
    if (N < 1 || h < 1 || w < 1 || !params || nparams != 62 || !workspace || !params[61]) return VSR_ERR_BADARG;
    bool any = dflow != nullptr;
    if (dlevel) for (int l = 0; l < 6; ++l) any = any || dlevel[l];
    if (!any) return VSR_ERR_BADARG;
    return spy_alone_backward(N, h, w, dtype, grads, dflow, params[61], last_relu != 0, dlevel, dref, dsupp, workspace, workspace_bytes, stream);
}

}  // extern "C"
