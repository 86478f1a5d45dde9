/* vsrlab_warp_taps.h -- C ABI of libvsrlab_warp_taps.so: the 'nearest' and 'nearest4' modes of VRT's flow_warp and the aligned
 * 27-channel input of VRT.forward (reference vsr/models/VRT/modules/spynet.py:11-63, vrt.py:145-150, :211-228).
 *
 * A library of its own beside libvsrlab_hip.so, whose set of exported symbols is pinned (ABI 4) and stays as it is.  The
 * conventions are those of include/vsrlab_hip.h: device pointers, a hipStream_t passed as void*, 0 (VSR_STATUS_OK) or a negative
 * VSR_STATUS_* code returned, nothing thrown; the status-string call of libvsrlab_hip.so names the codes.  Neither library needs
 * the other to be loaded.                                                                                                      */
#ifndef VSRLAB_WARP_TAPS_H
#define VSRLAB_WARP_TAPS_H
#ifdef __cplusplus
extern "C" {
#endif

/* ---- integer-tap gathers along an optical flow (csrc/warp_taps.hip) --------------------------------------
 * For the output pixel (row r, column c) of image n:  px = float(c) + flow[n, 0, r, c],  py = float(r) + flow[n, 1, r, c], one
 * fp32 add each.
 *   taps = 4 ('nearest4'): the taps (floor px, floor py), (floor px, ceil py), (ceil px, floor py), (ceil px, ceil py) in this
 *                          order; tap k fills the output channels k C .. k C + C - 1.
 *   taps = 1 ('nearest'):  the tap (rint px, rint py), ties to even; C output channels.
 * A tap (ix, iy) is x[n, :, iy, ix] when 0 <= ix <= W - 1 and 0 <= iy <= H - 1 and 0 otherwise; the range test is made on the
 * float value, so a non-finite or huge flow gives zeros and never forms an address.  border = 1 clamps the tap into the image
 * instead (padding_mode 'border'; a NaN position reads index 0).  A pure gather: every output value is an input value or 0.
 *
 * Tensors are planar and dense: x (N, C, H, W) and out (N, taps C, H, W) of `dtype` (0: fp32, 1: bf16), flow (N, 2, H, W) fp32.
 * x alone may have an ELEMENT stride x_nstride between its images (0: dense, C H W), so that a frame x[:, i] of a clip is passed
 * as it lies.
 *
 * The clip entries build what VRT.forward feeds conv_first:  x (B, D, C, H, W), flows_backward and flows_forward (B, D - 1, 2, H, W)
 *   out (B, D, 9 C, H, W) = cat([x, x_backward, x_forward], 2)
 *   x_backward[:, i - 1] = nearest4(x[:, i], flows_backward[:, i - 1]), i = 1 .. D - 1;  x_backward[:, D - 1] = 0
 *   x_forward[:, i + 1]  = nearest4(x[:, i], flows_forward[:, i]),      i = 0 .. D - 2;  x_forward[:, 0] = 0
 * in ONE launch that also writes the copy of x and the two zero blocks.  They use N as B, need D >= 2 and taps = 4, and every
 * tensor dense (x_nstride = 0).
 *
 * The backward entries give the gradient w.r.t. x (the flow has none: the taps are piecewise constant): every in-frame tap adds
 * its cotangent to its source pixel -- at an integer position the four taps add to the SAME pixel -- with atomicAdd on fp32.
 *   acc: fp32, as many elements as x, dense; it need not be initialised (the first launch does that: zeros, or for the clip the
 *        cotangent of the copy of x).  gx: dense, of `dtype`, rounded once from acc.  With dtype fp32 acc may BE gx.
 *
 * Supported: N, C >= 1, H, W >= 2 (at extent 1 the reference's max(w - 1, 1) normalisation reads index 0 for every tap:
 * VSR_STATUS_UNSUPPORTED), at most 2^31 - 1 workgroups of 256 lanes.  taps not in {1, 4}, D < 2 or taps != 4 for a clip entry,
 * a negative x_nstride and null pointers are VSR_STATUS_BADARG; an unknown dtype is VSR_STATUS_UNSUPPORTED.  All of it is
 * decided before anything is launched.  Element offsets are 64-bit.                                                             */
typedef struct VsrWarpTapsDesc {
    int N, D, C, H, W;               /* D: clip entries only */
    int taps, border, dtype;
    long long x_nstride;             /* pair forward only */
} VsrWarpTapsDesc;

int vsr_warp_taps_fwd(const VsrWarpTapsDesc* d, const void* x, const float* flow, void* out, void* stream);
int vsr_warp_taps_bwd(const VsrWarpTapsDesc* d, const void* gout, const float* flow, float* acc, void* gx, void* stream);
int vsr_warp_taps_clip_fwd(const VsrWarpTapsDesc* d, const void* x, const float* flows_backward, const float* flows_forward, void* out,
                           void* stream);
int vsr_warp_taps_clip_bwd(const VsrWarpTapsDesc* d, const void* gout, const float* flows_backward, const float* flows_forward, float* acc,
                           void* gx, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VSRLAB_WARP_TAPS_H */
