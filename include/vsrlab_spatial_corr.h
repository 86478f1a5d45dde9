/* vsrlab_spatial_corr.h -- C ABI of libvsrlab_spatial_corr.so: the local correlation (SpatialCorrelationSampler, PWC cost volume).
 *
 * A library of its own beside libvsrlab_hip.so, whose set of exported symbols is pinned (ABI 4) and stays as it is.  The
 * conventions are those of include/vsrlab_hip.h: device pointers, a hipStream_t passed as void*, 0 (VSR_STATUS_OK) or a negative
 * VSR_STATUS_* code returned, nothing thrown; the status-string call of libvsrlab_hip.so names the codes.  Neither library needs
 * the other to be loaded.                                                                                                      */
#ifndef VSRLAB_SPATIAL_CORR_H
#define VSRLAB_SPATIAL_CORR_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- Local correlation: SpatialCorrelationSampler and PWC's cost volume (csrc/spatial_corr.hip) ---------
 * core/modules/correlation.py iter_spatial_correlation_sample (kernel_size 1, dilation 1) and
 * optical_flow/models/irr/pwc_modules.py compute_cost_volume, in one launch instead of one pass per displacement:
 *   out[n][i][j][y][x] = scale * sum_c in1[n][c][y s_h][x s_w] * in2[n][c][y s_h + i d_h - m_h][x s_w + j d_w - m_w]
 * in the frame zero-padded by (pad_h, pad_w), H' = H + 2 pad_h, in2 zero outside it, m = dil (patch - 1) / 2; i (slow) is the
 * vertical displacement index.  scale: 1 for the sampler, 1 / C for the cost volume (channel i * patch_w + j).
 *   in1, in2, din1, din2 (N, C, H, W); out, dout (N, patch_h, patch_w, ceil(H' / s_h), ceil(W' / s_w)): fp32 planar.
 *   ws: workspace_bytes(d) bytes, owned by the call until it finished (the two maps re-laid pixel-major in `dtype`, channels
 *       padded to 8); the backward re-lays what it needs itself, nothing is carried over from the forward.
 *   bwd: din1 / din2 may each be NULL (not computed, nothing written).  Both are gathers with one owner per element: no
 *       atomics, bit-identical across runs.  d in1 is 0 at positions a stride of 2 skips.
 * Supported: C >= 1; patch odd and <= 9, stride 1 or 2, dil 1 or 2, 0 <= pad <= m, each per axis; H' W' <= 2^24,
 * N H' W' <= 2^28, N <= 65535, C <= 65536.  Anything else is VSR_STATUS_UNSUPPORTED (workspace_bytes: 0) before any launch. */
typedef struct VsrSpatialCorrDesc {
    int N, C, H, W;
    int patch_h, patch_w, stride_h, stride_w, pad_h, pad_w, dil_h, dil_w;
    int dtype;
    float scale;
} VsrSpatialCorrDesc;
size_t vsr_spatial_corr_workspace_bytes(const VsrSpatialCorrDesc* d);                   /* 0: unsupported descriptor */
int vsr_spatial_corr_fwd(const VsrSpatialCorrDesc* d, const float* in1, const float* in2, float* out, void* ws, size_t ws_bytes,
                         void* stream);
int vsr_spatial_corr_bwd(const VsrSpatialCorrDesc* d, const float* in1, const float* in2, const float* dout, float* din1, float* din2,
                         void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRLAB_SPATIAL_CORR_H */
