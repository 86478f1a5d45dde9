// Test hooks for the flow warp (not in the header): each runs ONE launch of csrc/elementwise.hip's warp kernels on the caller's buffers, through
// the launcher the engines and the per-op entries call, with the image stride of the flow (`flow_nstride`, floats between the flows of
// consecutive images; the engines pass (t - 1) * 2HW) and the padding mode as arguments.  Argument checks and launches only: no kernel lives
// here.  tests/test_flow_warp_gpu.py compares every hook with an fp64 restatement.
//   C: the channel width (16, 32 or 64; another width: VSR_ERR_UNSUPPORTED); *_pm: blocked pixel-major, C channels, element type of `dtype`;
//   flow / dflow: planar fp32, 2 planes (x, y) per image; border: 0 = 'zeros' padding, 1 = 'border'.
#include "host.h"
#include "debug_hooks.h"

namespace {
bool bad_width(int C) { return C != 16 && C != 32 && C != 64; }
bool bad_flow(const float* flow, long long nstride, int H, int W) { return !flow || nstride < (long long)2 * H * W; }
}  // namespace

extern "C" {

// vsr_launch_warp_fwd: out = bilinear(in, (x + flow_x, y + flow_y)).
int vsr_debug_warp_fwd(int dtype, int C, const void* in_pm, const float* flow, long long flow_nstride, void* out_pm, int border,
                       int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !in_pm || !out_pm || bad_dims(N, H, W) || bad_flow(flow, flow_nstride, H, W) || (border & ~1)) return VSR_ERR_BADARG;
    if (bad_width(C)) return VSR_ERR_UNSUPPORTED;
    return vsr_launch_warp_fwd(dtype, in_pm, flow, out_pm, N, H, W, C, flow_nstride, (hipStream_t)stream, border);
}

// The scatter form of the adjoint: vsr_launch_warp_bwd adds warp^T(dout) into dacc (plain [N][H][W][C] fp32, zeroed by the caller), then
// vsr_launch_add_cast writes out = T(a + dacc); a_pm may be NULL.
int vsr_debug_warp_scatter(int dtype, int C, const void* dout_pm, const float* flow, long long flow_nstride, float* dacc, const void* a_pm,
                           void* out_pm, int border, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !dout_pm || !dacc || !out_pm || bad_dims(N, H, W) || bad_flow(flow, flow_nstride, H, W) || (border & ~1)) return VSR_ERR_BADARG;
    if (bad_width(C)) return VSR_ERR_UNSUPPORTED;
    CK(vsr_launch_warp_bwd(dtype, dout_pm, flow, dacc, N, H, W, C, flow_nstride, (hipStream_t)stream, border));
    return vsr_launch_add_cast(dtype, a_pm, dacc, out_pm, N, H, W, C, (hipStream_t)stream);
}

// The gather form (zeros padding): vsr_launch_warp_bwd_gather writes out = T(dtop + warp^T(dout)); dtop_pm may be NULL.  S: N*H*W*C long
// longs, all zero on entry and on exit; far_count: one zeroed int, the number of far sources afterwards.
int vsr_debug_warp_gather(int dtype, int C, const void* dout_pm, const float* flow, long long flow_nstride, const void* dtop_pm, long long* S,
                          int* far_count, void* out_pm, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !dout_pm || !S || !far_count || !out_pm || bad_dims(N, H, W) || bad_flow(flow, flow_nstride, H, W)) return VSR_ERR_BADARG;
    if (bad_width(C)) return VSR_ERR_UNSUPPORTED;
    return vsr_launch_warp_bwd_gather(dtype, dout_pm, flow, dtop_pm, S, far_count, out_pm, N, H, W, C, flow_nstride, (hipStream_t)stream);
}

// vsr_launch_warp_bwd_flow: dflow (images flow_nstride floats apart, like the flow) = d/d flow of <dout, warp(in, flow)>.
int vsr_debug_warp_flowgrad(int dtype, int C, const void* in_pm, const void* dout_pm, const float* flow, long long flow_nstride, float* dflow,
                            int border, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || !in_pm || !dout_pm || !dflow || bad_dims(N, H, W) || bad_flow(flow, flow_nstride, H, W) || (border & ~1)) return VSR_ERR_BADARG;
    if (bad_width(C)) return VSR_ERR_UNSUPPORTED;
    return vsr_launch_warp_bwd_flow(dtype, in_pm, dout_pm, flow, dflow, N, H, W, C, flow_nstride, (hipStream_t)stream, border);
}

// vsr_launch_add_cast alone: out = T(a + s); a_pm (pixel-major) or s (plain [N][H][W][C] fp32) may be NULL, not both.
int vsr_debug_warp_add_cast(int dtype, int C, const void* a_pm, const float* s, void* out_pm, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || (!a_pm && !s) || !out_pm || bad_dims(N, H, W)) return VSR_ERR_BADARG;
    if (bad_width(C)) return VSR_ERR_UNSUPPORTED;
    return vsr_launch_add_cast(dtype, a_pm, s, out_pm, N, H, W, C, (hipStream_t)stream);
}

}  // extern "C"
