/* vsrlab_losses.h -- C ABI of libvsrlab_losses.so: the pixel losses that the reference's LossPipeline combines (src/core/losses.py:
 * WL1Loss :20-27, rmse_loss :76-77) and the adjoint of the bilinear resize of its `match_` keys (:169-173).
 *
 * A library of its own beside libvsrlab_hip.so, whose set of exported symbols is pinned (ABI 4) and stays as it is.  The
 * conventions are those of include/vsrlab_hip.h: device pointers, a hipStream_t passed as void*, 0 (VSR_STATUS_OK) or a negative
 * VSR_STATUS_* code returned, nothing thrown; the status-string call of libvsrlab_hip.so names the codes.  Neither library needs
 * the other to be loaded.                                                                                                      */
#ifndef VSRLAB_LOSSES_H
#define VSRLAB_LOSSES_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- mean reduction of a pair, fused with its gradient (csrc/pixel_losses.hip) ---------------------------
 * kind VSR_LOSS_L1:   loss[0] = mean |x - y|,    dx = sign(x - y) * fp32(1 / numel), sign(0) = 0
 * kind VSR_LOSS_MSE:  loss[0] = mean (x - y)^2,  dx = (x - y) * fp32(1 / numel)   -- HALF the derivative of the mean: the factor
 *                     1 / (2 sqrt(mean)) of a root taken by the caller cancels the 2, so d sqrt(mean) / dx = dx / sqrt(mean)
 * x and y: `numel` dense elements each, of x_dtype and y_dtype (0: fp32, 1: bf16) independently, read as they lie; differences,
 * sums and the gradient are fp32, dx is stored in x's dtype.  dx may be null: only the value is computed (the same bits).
 * Two launches: one pass over x and y that leaves one partial per workgroup in `scratch` (vsr_pixel_loss_scratch_floats() floats),
 * and one workgroup that adds the partials in index order: the value is bit-identical from run to run.
 * Pointers need the alignment of their element type only; with x, y and dx all 16-byte aligned a lane moves 16 bytes per access.
 * Null x, y, loss or scratch, numel < 1, an unknown kind or dtype and a misaligned pointer are VSR_STATUS_BADARG.              */
#define VSR_LOSS_L1 0
#define VSR_LOSS_MSE 1

size_t vsr_pixel_loss_scratch_floats(void);
int vsr_pixel_loss_fwd_bwd(int kind, const void* x, int x_dtype, const void* y, int y_dtype, void* dx, float* loss, float* scratch,
                           long long numel, void* stream);

/* ---- adjoint of the bilinear resize, vsr_resize_bilinear of include/vsrlab_hip.h ------------------------------------------------
 * dout: (planes, h, w), the cotangent of the resized images; din: (planes, H, W), the gradient w.r.t. the images that were resized,
 * written everywhere (0 where no output pixel samples the input, as happens when down-scaling without antialiasing).  Both fp32 and
 * dense.  A gather with one owner per element of din and the forward's own fp32 tap expressions: no atomics, bit-identical from run
 * to run.  Extents of 1 are valid.  Null pointers and non-positive planes or extents are VSR_STATUS_BADARG; an extent above 2^22
 * or an element count that overflows 64 bits is VSR_STATUS_UNSUPPORTED.                                                          */
int vsr_resize_bilinear_bwd(const float* dout, float* din, long long planes, int H, int W, int h, int w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRLAB_LOSSES_H */
