/* vsrlab_conv3d.h -- C ABI of libvsrlab_conv3d.so: the spatio-temporal convolutions of the reference's core/modules (conv.py: ConvST /
 * ConvSTBlock; upsampling.py: PixelShufflePack3D) and of VRT's reconstruction tail (vrt.py: Upsample and the (1,3,3) nn.Conv3d layers)
 * -- one stride-1 'same' Conv3d over three tap sets, on planar operands read through strides.  DESIGN section 11k.
 *
 * A library of its own beside libvsrlab_hip.so, whose set of exported symbols is pinned (ABI 4) and stays as it is.  The
 * conventions are those of include/vsrlab_mixer.h: device pointers, a hipStream_t passed as void*, 0 (VSR_STATUS_OK) or a negative
 * VSR_STATUS_* code returned, nothing thrown; the status-string call of libvsrlab_hip.so names the codes.  Neither library needs
 * the other to be loaded.  Activations are fp32 or bf16 (dtype 0 / 1) and read where they lie; weights and biases are fp32; all
 * arithmetic is fp32.  No entry uses a float atomic: every output, weight gradients included, is bit-identical from run to run.
 * Every entry checks its arguments before it touches the GPU: a null pointer, a non-positive extent, an unknown dtype, an unknown
 * tap set, activation or shuffle factor is VSR_STATUS_BADARG; a shape outside the stated bounds, or one whose element offsets or
 * workgroup count overflow, is VSR_STATUS_UNSUPPORTED; a workspace that is too small is VSR_STATUS_WORKSPACE.                      */
#ifndef VSRLAB_CONV3D_H
#define VSRLAB_CONV3D_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* tap sets (kt, kh, kw), all stride 1 with zero padding k / 2 on every axis that has taps */
#define VSR_CONV3D_133 0
#define VSR_CONV3D_311 1
#define VSR_CONV3D_333 2
#define VSR_CONV3D_ACT_NONE 0
#define VSR_CONV3D_ACT_LEAKY 1
#define VSR_CONV3D_MAX_C 256

/* x: B x Cin x T x H x W and y: B x Cout x T x H x W as LOGICAL extents; where element (b, c, t, h, w) of x lies is
 *   x + b x_stride[0] + c x_stride[1] + t x_stride[2] + h W + w        (elements; an H x W plane is always contiguous)
 * so (b,t,c,h,w), (b,c,t,h,w) and a transposed view of either are all just strides; no alignment beyond the element's own.
 * pixel_shuffle = 2 (needs Cout % 4 == 0): y is B x Cout/4 x T x 2H x 2W, its planes 2H x 2W contiguous, and output channel
 * 4c + 2i + j of pixel (h, w) is stored at channel c, pixel (2h + i, 2w + j) of the same frame -- nn.PixelShuffle(2) on the last three
 * axes.  act: VSR_CONV3D_ACT_LEAKY applies LeakyReLU(slope), which commutes with the shuffle.
 * Bounds: 1 <= Cin, Cout <= VSR_CONV3D_MAX_C (any value: the padding to the MFMA granule happens in the weight packing); any
 * T, H, W >= 1; strides >= 0; every element offset of x and y below 2^62 and the workgroup count below 2^31.                      */
typedef struct VsrConv3dDesc {
    int B, Cin, Cout, T, H, W;
    int taps, dtype, act;
    float slope;
    int pixel_shuffle;
    long long x_stride[3];      /* batch, channel, frame */
    long long y_stride[3];
} VsrConv3dDesc;

/* bytes of `workspace` (256-byte aligned) for fwd (need_backward = 0) or bwd (1); 0 for a descriptor fwd would refuse */
size_t vsr_conv3d_workspace_bytes(const VsrConv3dDesc* desc, int need_backward);

/* y = act(conv3d(x, w) + b).  w: (Cout, Cin, kt, kh, kw) fp32, nn.Conv3d's layout; b: (Cout) fp32 or NULL. */
int vsr_conv3d_fwd(const VsrConv3dDesc* desc, const void* x, const float* w, const float* b, void* y, void* workspace,
                   size_t workspace_bytes, void* stream);

/* dy has y's extents and strides, dx has x's.  dx, dw, db: each may be NULL (skipped); dw (w's layout) and db are OVERWRITTEN with
 * sums formed as per-workgroup partials in the workspace and added in workgroup order by a second launch.  y: the forward's result,
 * read only when act is not none (its sign) and then required.                                                                    */
int vsr_conv3d_bwd(const VsrConv3dDesc* desc, const void* x, const float* w, const void* y, const void* dy, void* dx, float* dw,
                   float* db, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRLAB_CONV3D_H */
