/* vsrlab_mixer.h -- C ABI of libvsrlab_mixer.so: the DCT-token MLP-Mixer of the reference's core/modules (dct_transforms.py:
 * EncoderDCT / DecoderIDCT; mlp.py: Mlp / MixerBlock / MlpMixer) -- a block transform between planar frames and tokens, and a
 * residual two-layer GELU MLP along one axis of a dense tensor.  DESIGN section 11j.
 *
 * A library of its own beside libvsrlab_hip.so, whose set of exported symbols is pinned (ABI 4) and stays as it is.  The
 * conventions are those of include/vsrlab_hip.h: device pointers, a hipStream_t passed as void*, 0 (VSR_STATUS_OK) or a negative
 * VSR_STATUS_* code returned, nothing thrown; the status-string call of libvsrlab_hip.so names the codes.  Neither library needs
 * the other to be loaded.  Activations are fp32 or bf16 (dtype 0 / 1) and read where they lie; weights and biases are fp32; all
 * arithmetic is fp32.  No entry uses a float atomic: every output, weight gradients included, is bit-identical from run to run.
 * Every entry checks its arguments before it touches the GPU: a null pointer, a non-positive extent, an unknown dtype or a pointer
 * that lacks the alignment of its element type is VSR_STATUS_BADARG; a shape outside the stated bounds, or one whose element or
 * workgroup count overflows, is VSR_STATUS_UNSUPPORTED.                                                                          */
#ifndef VSRLAB_MIXER_H
#define VSRLAB_MIXER_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- block transform (csrc/token_mixer.hip) -------------------------------------------------------------------------------------
 * x: (N, C, H, W) planar; w: (C ps^2, ps, ps) fp32, the weight of nn.Conv2d(C, C ps^2, ps, ps, groups=C) as the module holds it
 * (any values: a loaded checkpoint is honoured); y: (N, P, C ps^2) tokens, P = (H / ps)(W / ps), token p = bi (W / ps) + bj.
 *   fwd:   y[n, p, c ps^2 + k] = sum_{i,j} w[c ps^2 + k, i, j] x[n, c, bi ps + i, bj ps + j];   rows and columns of x at or past
 *          (H / ps) ps and (W / ps) ps are not read
 *   idct:  x[n, c, bi ps + i, bj ps + j] = sum_k y[n, p, c ps^2 + k] w[c ps^2 + k, i, j]   (ConvTranspose2d(.., groups=C)); every
 *          element of x is written, the remainder rows and columns with zeros
 * Each is the other's adjoint for the same w, so each is the other's backward.  ps in {2, 4, 8}, C ps^2 <= 256, H >= ps, W >= ps. */
typedef struct VsrBlockDctDesc {
    int N, C, H, W, ps, dtype;
} VsrBlockDctDesc;

int vsr_block_dct_fwd(const VsrBlockDctDesc* desc, const void* x, const float* w, void* y, void* stream);
int vsr_block_idct_fwd(const VsrBlockDctDesc* desc, const void* y, const float* w, void* x, void* stream);

/* ---- residual MLP along one axis ------------------------------------------------------------------------------------------------
 * The dense tensor is viewed as (outer, D, inner); for every (o, i)
 *   y[o, :, i] = r x[o, :, i] + W2 gelu(W1 x[o, :, i] + b1) + b2,   r = 1 (residual != 0) or 0
 * W1: (hidden, D), b1: (hidden), W2: (D, hidden), b2: (D), nn.Linear's layout; gelu is the exact erf form.
 * The fused path: 1 <= D <= VSR_AXIS_MLP_MAX_D (a lane holds its position's D inputs and D accumulators in registers) and
 * 1 <= hidden <= VSR_AXIS_MLP_MAX_HIDDEN (the weights pass through LDS in chunks of 32 hidden units, so LDS does not bound hidden;
 * the bound is where a GEMM is the better tool), any outer >= 1 and inner >= 1.  vsr_axis_mlp_supported(): 1 inside it, else 0.
 *
 * bwd recomputes the hidden vector from x (the forward saves nothing).  dx = r dy + W1^T (gelu'(h) * W2^T dy); null dx: skipped.
 * dw1, db1, dw2, db2: all four or none (null: skipped); they are OVERWRITTEN with the sums over all (o, i), which are formed as one
 * partial per workgroup in `scratch` (vsr_axis_mlp_scratch_bytes(), 4-byte aligned; too small: VSR_STATUS_WORKSPACE) and added in
 * workgroup order by a second launch.                                                                                             */
#define VSR_AXIS_MLP_MAX_D 48
#define VSR_AXIS_MLP_MAX_HIDDEN 1024

typedef struct VsrAxisMlpDesc {
    long long outer;
    int D;
    long long inner;
    int hidden, dtype, residual;
} VsrAxisMlpDesc;

int vsr_axis_mlp_supported(const VsrAxisMlpDesc* desc);
size_t vsr_axis_mlp_scratch_bytes(const VsrAxisMlpDesc* desc);
int vsr_axis_mlp_fwd(const VsrAxisMlpDesc* desc, const void* x, const float* w1, const float* b1, const float* w2, const float* b2,
                     void* y, void* stream);
int vsr_axis_mlp_bwd(const VsrAxisMlpDesc* desc, const void* x, const void* dy, const float* w1, const float* b1, const float* w2,
                     const float* b2, void* dx, float* dw1, float* db1, float* dw2, float* db2, void* scratch, size_t scratch_bytes,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRLAB_MIXER_H */
