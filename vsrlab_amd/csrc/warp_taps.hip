// The 'nearest' and 'nearest4' modes of VRT's flow_warp (reference vsr/models/VRT/modules/spynet.py:11-63) and the aligned input of
// VRT.forward (vrt.py:145-150: cat([x, x_backward, x_forward], 2), the two halves from get_aligned_image, :211-228).  DESIGN
// section 11h is the specification: integer taps found with one fp32 add, one floor / ceil / rint and a range test ON THE FLOAT, so
// that a non-finite or huge flow gives zeros and never forms an address.  Every output value is an input value or 0: the result is
// bit-identical to the reference's four grid_sample(mode='nearest') calls and their cat.
// Built into a library of its own, libvsrlab_warp_taps.so (include/vsrlab_warp_taps.h): libvsrlab_hip.so's exports stay as they are.
//
// A streaming gather, no LDS: everything is planar and a lane owns one pixel of one image.  It reads its two flow values once,
// derives the plane offsets of its taps (-1: outside), and then per channel and tap gathers one value -- adjacent lanes' taps are
// adjacent addresses unless the flow tears -- and stores it, a wave writing 64 consecutive values of a row.  Nearly all traffic is
// those stores: per pixel C values read, 2 flow values read, taps C values written.  (A form in which a lane owned 16 bytes of
// consecutive columns and stored them at once was measured and was never faster, DESIGN section 11h: it is not here.)
//   wt_fwd_kernel:      one frame pair, taps 1 or 4
//   wt_clip_fwd_kernel: the whole clip in one launch.  The lane of (b, d, row, columns) writes all 9 C channels of its pixels: the
//                       copy of x, the four taps of frame d + 1 along flows_backward[d] (zeros for d = D - 1) and the four taps of
//                       frame d - 1 along flows_forward[d - 1] (zeros for d = 0).  No memset, no copy, no cat.
// The gradient w.r.t. x is the scatter of the same taps: wt_init_kernel writes the fp32 accumulator (zeros; for the clip the cotangent
// of the copy of x), wt_bwd_kernel / wt_clip_bwd_kernel add every in-frame tap's cotangent to its source pixel with atomicAdd
// (global_atomic_add_f32: at an integer position the four taps add to the same pixel, like the reference's four grid_sample
// backwards), and wt_round_kernel rounds the accumulator to the tensor's dtype once.  The flow has no gradient.
#include <limits.h>
#include "elt.h"
#include "host.h"
#include "../../include/vsrlab_warp_taps.h"

namespace {

constexpr int WT_BLOCK = 256;
constexpr int WT_MAXDIM = 1 << 24;              // (float)(extent - 1) is exact up to here

struct WtArgs {
    const void* x; const void* g; void* out;
    const float *flow_b, *flow_f;               // pair: flow_b alone
    float* acc;
    long long items;                            // lanes with work: one per pixel of every image
    long long x_nstride;                        // elements between the images of x (pair forward)
    int D, C, H, W, border;
};

// one coordinate's tap as an index, or -1 outside [0, n - 1]: the range test is made on the float (NaN fails it)
static __device__ __forceinline__ int wt_index(float t, int n, int border) {
    const float hi = (float)(n - 1);
    if (border) t = fminf(fmaxf(t, 0.f), hi);   // padding_mode 'border'; a NaN becomes 0
    return (t >= 0.f && t <= hi) ? (int)t : -1;
}

// the plane offsets iy W + ix of the taps of the output pixel (r, c), -1 for a tap outside the image.
// TAPS = 4: (floor x, floor y), (floor x, ceil y), (ceil x, floor y), (ceil x, ceil y); TAPS = 1: (rint x, rint y), ties to even
template <int TAPS>
static __device__ __forceinline__ void wt_taps(float fx, float fy, int r, int c, int H, int W, int border, int* off) {
    const float px = (float)c + fx, py = (float)r + fy;
    if (TAPS == 4) {
        const int ix[2] = {wt_index(floorf(px), W, border), wt_index(ceilf(px), W, border)};
        const int iy[2] = {wt_index(floorf(py), H, border), wt_index(ceilf(py), H, border)};
#pragma unroll
        for (int k = 0; k < 4; ++k) off[k] = (ix[k >> 1] < 0 || iy[k & 1] < 0) ? -1 : iy[k & 1] * W + ix[k >> 1];
    } else {
        const int ix = wt_index(rintf(px), W, border), iy = wt_index(rintf(py), H, border);
        off[0] = (ix < 0 || iy < 0) ? -1 : iy * W + ix;
    }
}

// TAPS C output planes from o on, at the pixel with plane offset p = (r, c): the taps of the image xs along the flow fl
template <typename T, int TAPS>
static __device__ __forceinline__ void wt_gather(const T* __restrict__ xs, const float* __restrict__ fl, T* __restrict__ o, int C, int H, int W,
                                                 long long hw, int r, int c, long long p, int border) {
    int off[TAPS];
    wt_taps<TAPS>(fl[p], fl[hw + p], r, c, H, W, border, off);
    for (int ch = 0; ch < C; ++ch) {
        const T* xc = xs + ch * hw;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) o[((long long)k * C + ch) * hw + p] = off[k] >= 0 ? xc[off[k]] : (T)0.f;
    }
}

template <typename T>
static __device__ __forceinline__ void wt_zero(T* __restrict__ o, int planes, long long hw, long long p) {
    for (int ch = 0; ch < planes; ++ch) o[ch * hw + p] = (T)0.f;
}

// lane -> (image, row, column)
static __device__ __forceinline__ bool wt_lane(const WtArgs& a, long long& img, int& r, int& c) {
    const long long i = (long long)blockIdx.x * WT_BLOCK + threadIdx.x;
    if (i >= a.items) return false;
    const long long t = i / a.W;
    c = (int)(i - t * a.W);
    img = t / a.H;
    r = (int)(t - img * a.H);
    return true;
}

template <typename T, int TAPS>
__global__ __launch_bounds__(WT_BLOCK) void wt_fwd_kernel(WtArgs a) {
    long long n; int r, c0;
    if (!wt_lane(a, n, r, c0)) return;
    const long long hw = (long long)a.H * a.W;
    wt_gather<T, TAPS>(static_cast<const T*>(a.x) + n * a.x_nstride, a.flow_b + n * 2 * hw, static_cast<T*>(a.out) + n * TAPS * a.C * hw,
                       a.C, a.H, a.W, hw, r, c0, (long long)r * a.W + c0, a.border);
}

template <typename T>
__global__ __launch_bounds__(WT_BLOCK) void wt_clip_fwd_kernel(WtArgs a) {
    long long n; int r, c0;
    if (!wt_lane(a, n, r, c0)) return;
    const long long hw = (long long)a.H * a.W, chw = a.C * hw, p = (long long)r * a.W + c0;
    const long long b = n / a.D;
    const int d = (int)(n - b * a.D);
    const T* xf = static_cast<const T*>(a.x) + n * chw;                         // frame d
    T* o = static_cast<T*>(a.out) + n * 9 * chw;
    for (int c = 0; c < a.C; ++c) o[c * hw + p] = xf[c * hw + p];
    const long long fl = (b * (a.D - 1) + d) * 2 * hw;                          // flow d of clip b
    if (d < a.D - 1) wt_gather<T, 4>(xf + chw, a.flow_b + fl, o + chw, a.C, a.H, a.W, hw, r, c0, p, a.border);
    else wt_zero<T>(o + chw, 4 * a.C, hw, p);
    if (d > 0) wt_gather<T, 4>(xf - chw, a.flow_f + fl - 2 * hw, o + 5 * chw, a.C, a.H, a.W, hw, r, c0, p, a.border);
    else wt_zero<T>(o + 5 * chw, 4 * a.C, hw, p);
}

// the cotangents of the TAPS C planes from g on, at pixel p = (r, c), added to their source pixels in the fp32 image `acc`
template <typename T, int TAPS>
static __device__ __forceinline__ void wt_scatter(const T* __restrict__ g, const float* __restrict__ fl, float* __restrict__ acc, int C, int H,
                                                  int W, long long hw, int r, int c0, long long p, int border) {
    int off[TAPS];
    wt_taps<TAPS>(fl[p], fl[hw + p], r, c0, H, W, border, off);
    for (int ch = 0; ch < C; ++ch)
#pragma unroll
        for (int k = 0; k < TAPS; ++k)
            if (off[k] >= 0) atomicAdd(acc + ch * hw + off[k], to_f(g[((long long)k * C + ch) * hw + p]));
}

template <typename T, int TAPS>
__global__ __launch_bounds__(WT_BLOCK) void wt_bwd_kernel(WtArgs a) {
    long long n; int r, c0;
    if (!wt_lane(a, n, r, c0)) return;
    const long long hw = (long long)a.H * a.W;
    wt_scatter<T, TAPS>(static_cast<const T*>(a.g) + n * TAPS * a.C * hw, a.flow_b + n * 2 * hw, a.acc + n * a.C * hw, a.C, a.H, a.W, hw, r, c0,
                        (long long)r * a.W + c0, a.border);
}

template <typename T>
__global__ __launch_bounds__(WT_BLOCK) void wt_clip_bwd_kernel(WtArgs a) {
    long long n; int r, c0;
    if (!wt_lane(a, n, r, c0)) return;
    const long long hw = (long long)a.H * a.W, chw = a.C * hw, p = (long long)r * a.W + c0;
    const long long b = n / a.D;
    const int d = (int)(n - b * a.D);
    const T* g = static_cast<const T*>(a.g) + n * 9 * chw;
    float* acc = a.acc + n * chw;                                               // frame d
    const long long fl = (b * (a.D - 1) + d) * 2 * hw;
    if (d < a.D - 1) wt_scatter<T, 4>(g + chw, a.flow_b + fl, acc + chw, a.C, a.H, a.W, hw, r, c0, p, a.border);
    if (d > 0) wt_scatter<T, 4>(g + 5 * chw, a.flow_f + fl - 2 * hw, acc - chw, a.C, a.H, a.W, hw, r, c0, p, a.border);
}

// acc[n][e] = g ? g[n][e] (images g_nstride apart) : 0, e < chw
template <typename T>
__global__ __launch_bounds__(WT_BLOCK) void wt_init_kernel(float* __restrict__ acc, const T* __restrict__ g, long long total, long long chw,
                                                           long long g_nstride) {
    const long long i = (long long)blockIdx.x * WT_BLOCK + threadIdx.x;
    if (i >= total) return;
    float v = 0.f;
    if (g) { const long long n = i / chw; v = to_f(g[n * g_nstride + (i - n * chw)]); }
    acc[i] = v;
}

template <typename T>
__global__ __launch_bounds__(WT_BLOCK) void wt_round_kernel(const float* __restrict__ acc, T* __restrict__ gx, long long total) {
    const long long i = (long long)blockIdx.x * WT_BLOCK + threadIdx.x;
    if (i < total) gx[i] = (T)acc[i];
}

struct WtPlan { long long imgs, hw, total; int blocks_px, blocks_el; };   // images, pixels per plane, elements of x; workgroups per pixel / element

bool wt_blocks(long long items, int& blocks) {
    const long long b = (items + WT_BLOCK - 1) / WT_BLOCK;
    if (b > INT_MAX) return false;
    blocks = (int)b;
    return true;
}

int wt_plan(const VsrWarpTapsDesc* d, bool clip, WtPlan& pl) {
    if (!d) return VSR_ERR_BADARG;
    if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1) return VSR_ERR_BADARG;
    if (d->taps != 1 && d->taps != 4) return VSR_ERR_BADARG;
    if (clip && (d->D < 2 || d->taps != 4 || d->x_nstride != 0)) return VSR_ERR_BADARG;
    if (d->x_nstride < 0) return VSR_ERR_BADARG;
    if (bad_dtype(d->dtype)) return VSR_ERR_UNSUPPORTED;
    if (d->H < 2 || d->W < 2 || d->H > WT_MAXDIM || d->W > WT_MAXDIM) return VSR_ERR_UNSUPPORTED;
    pl.hw = (long long)d->H * d->W;
    if (pl.hw > INT_MAX) return VSR_ERR_UNSUPPORTED;                            // plane offsets are ints
    pl.imgs = (long long)d->N * (clip ? d->D : 1);
    long long px, out;
    if (__builtin_mul_overflow(pl.imgs, pl.hw, &px) || __builtin_mul_overflow(px, (long long)d->C, &pl.total) ||
        __builtin_mul_overflow(pl.total, 9LL * 4, &out))
        return VSR_ERR_UNSUPPORTED;
    if (!wt_blocks(px, pl.blocks_px) || !wt_blocks(pl.total, pl.blocks_el)) return VSR_ERR_UNSUPPORTED;
    return VSR_OK;
}

WtArgs wt_args(const VsrWarpTapsDesc* d) {
    WtArgs a = {};
    a.D = d->D; a.C = d->C; a.H = d->H; a.W = d->W; a.border = d->border ? 1 : 0;
    a.x_nstride = d->x_nstride ? d->x_nstride : (long long)d->C * d->H * d->W;
    return a;
}

template <typename T>
void wt_finish(hipStream_t st, const WtPlan& pl, const float* acc, void* gx) {
    if (static_cast<const void*>(acc) != gx)
        hipLaunchKernelGGL(wt_round_kernel<T>, dim3(pl.blocks_el), dim3(WT_BLOCK), 0, st, acc, static_cast<T*>(gx), pl.total);
}

}  // namespace

#define WT_BY_DTYPE(d, ...) do { if ((d)->dtype == VSR_BF16) { typedef bf16_t T; __VA_ARGS__; } else { typedef float T; __VA_ARGS__; } } while (0)

extern "C" {

int vsr_warp_taps_fwd(const VsrWarpTapsDesc* d, const void* x, const float* flow, void* out, void* stream) {
    WtPlan pl;
    CK(wt_plan(d, false, pl));
    if (!x || !flow || !out) return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    WtArgs a = wt_args(d);
    a.x = x; a.flow_b = flow; a.out = out; a.items = pl.imgs * pl.hw;
    WT_BY_DTYPE(d, {
        if (d->taps == 4) hipLaunchKernelGGL((wt_fwd_kernel<T, 4>), dim3(pl.blocks_px), dim3(WT_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((wt_fwd_kernel<T, 1>), dim3(pl.blocks_px), dim3(WT_BLOCK), 0, st, a);
    });
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_warp_taps_bwd(const VsrWarpTapsDesc* d, const void* gout, const float* flow, float* acc, void* gx, void* stream) {
    WtPlan pl;
    CK(wt_plan(d, false, pl));
    if (!gout || !flow || !acc || !gx) return VSR_ERR_BADARG;
    if (d->dtype != VSR_F32 && static_cast<void*>(acc) == gx) return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    WtArgs a = wt_args(d);
    a.g = gout; a.flow_b = flow; a.acc = acc; a.items = pl.imgs * pl.hw;
    hipLaunchKernelGGL(wt_init_kernel<float>, dim3(pl.blocks_el), dim3(WT_BLOCK), 0, st, acc, (const float*)nullptr, pl.total, pl.total, 0LL);
    WT_BY_DTYPE(d, {
        if (d->taps == 4) hipLaunchKernelGGL((wt_bwd_kernel<T, 4>), dim3(pl.blocks_px), dim3(WT_BLOCK), 0, st, a);
        else hipLaunchKernelGGL((wt_bwd_kernel<T, 1>), dim3(pl.blocks_px), dim3(WT_BLOCK), 0, st, a);
        wt_finish<T>(st, pl, acc, gx);
    });
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_warp_taps_clip_fwd(const VsrWarpTapsDesc* d, const void* x, const float* flows_backward, const float* flows_forward, void* out,
                           void* stream) {
    WtPlan pl;
    CK(wt_plan(d, true, pl));
    if (!x || !flows_backward || !flows_forward || !out) return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    WtArgs a = wt_args(d);
    a.x = x; a.flow_b = flows_backward; a.flow_f = flows_forward; a.out = out; a.items = pl.imgs * pl.hw;
    WT_BY_DTYPE(d, hipLaunchKernelGGL(wt_clip_fwd_kernel<T>, dim3(pl.blocks_px), dim3(WT_BLOCK), 0, st, a));
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_warp_taps_clip_bwd(const VsrWarpTapsDesc* d, const void* gout, const float* flows_backward, const float* flows_forward, float* acc,
                           void* gx, void* stream) {
    WtPlan pl;
    CK(wt_plan(d, true, pl));
    if (!gout || !flows_backward || !flows_forward || !acc || !gx) return VSR_ERR_BADARG;
    if (d->dtype != VSR_F32 && static_cast<void*>(acc) == gx) return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
    WtArgs a = wt_args(d);
    a.g = gout; a.flow_b = flows_backward; a.flow_f = flows_forward; a.acc = acc; a.items = pl.imgs * pl.hw;
    const long long chw = (long long)d->C * pl.hw;
    WT_BY_DTYPE(d, {
        // the identity part: the cotangent of the copy of x, the first C of every frame's 9 C planes
        hipLaunchKernelGGL(wt_init_kernel<T>, dim3(pl.blocks_el), dim3(WT_BLOCK), 0, st, acc, static_cast<const T*>(gout), pl.total, chw, 9 * chw);
        hipLaunchKernelGGL(wt_clip_bwd_kernel<T>, dim3(pl.blocks_px), dim3(WT_BLOCK), 0, st, a);
        wt_finish<T>(st, pl, acc, gx);
    });
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
