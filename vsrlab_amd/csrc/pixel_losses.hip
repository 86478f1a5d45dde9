// The pixel losses that LossPipeline combines (reference src/core/losses.py: WL1Loss :20-27, rmse_loss :76-77) and the adjoint of the
// bilinear resize that its `match_` keys put in front of them (:169-173; the forward is resize_bilinear_kernel, train_step.hip).
// DESIGN section 11i is the specification.  Built into a library of its own, libvsrlab_losses.so (include/vsrlab_losses.h):
// libvsrlab_hip.so's exports stay as they are.
//
//   pair_loss_kernel:  one pass over x and y, each fp32 or bf16 and read as it lies: the gradient w.r.t. x, in x's dtype, and one
//                      fp32 partial per workgroup.  HBM streaming: a lane moves 8 consecutive elements per trip, in 16-byte accesses.
//   pair_sum_kernel:   ONE workgroup adds the partials: the fixed order of reduce.h (pairwise combiner), as for Charbonnier
//                      (elementwise.hip).  Bit-identical from run to run, no atomics.
//   resize_bilinear_bwd_kernel:  the adjoint as a GATHER: a lane owns one element of d in, finds by arithmetic the output rows and
//                      columns whose taps can include it, and decides which do with the forward's own fp32 expressions.  One owner
//                      per element, no atomics, bit-identical from run to run; an input pixel that no output samples gets 0.
#include "elt.h"
#include "host.h"
#include "reduce.h"
#include "../../include/vsrlab_losses.h"

namespace {

constexpr int PL_BLOCK = 256;
constexpr int PL_BLOCKS = 1024;                 // at most this many workgroups and partials (vsr_pixel_loss_scratch_floats)
constexpr int PL_VEC = 8;                       // elements per lane and trip: 16 bytes of bf16, two 16-byte accesses of fp32
constexpr int RS_MAXDIM = 1 << 22;              // the forward's fp32 source coordinate is within 1 of the exact one up to here

// one element's term of the sum and its gradient factor; d = x - y in fp32
//   L1:  |d| and sign(d) scale with sign(0) = 0 (torch's l1_loss backward; a NaN stays one)
//   MSE: d d and d scale (the 2 of the derivative belongs to the caller's square root: d sqrt(m) = dm / (2 sqrt(m)))
template <int KIND>
static __device__ __forceinline__ float pl_term(float d, float scale, float& g) {
    if (KIND == VSR_LOSS_L1) {
        g = d > 0.f ? scale : (d < 0.f ? -scale : d * 0.f);
        return fabsf(d);
    }
    g = d * scale;
    return d * d;
}

template <typename TX, typename TY, int KIND>
__global__ __launch_bounds__(PL_BLOCK) void pair_loss_kernel(const TX* __restrict__ x, const TY* __restrict__ y, TX* __restrict__ dx,
                                                             float* __restrict__ partial, long long n, float scale, int vec) {
    __shared__ float red[PL_BLOCK / 64];
    float local = 0.f;
    const long long first = (long long)blockIdx.x * PL_BLOCK + threadIdx.x, step = (long long)gridDim.x * PL_BLOCK;
    if (vec) {
        const long long nv = n / PL_VEC;
        for (long long i = first; i < nv; i += step) {
            float a[PL_VEC], b[PL_VEC], g[PL_VEC];
            ld8<TX>(x + i * PL_VEC, a);
            ld8<TY>(y + i * PL_VEC, b);
#pragma unroll
            for (int j = 0; j < PL_VEC; ++j) local += pl_term<KIND>(a[j] - b[j], scale, g[j]);
            if (dx) st8<TX>(dx + i * PL_VEC, g);
        }
        if (blockIdx.x == 0 && threadIdx.x < (int)(n % PL_VEC)) {     // tail of a length that is not a multiple of 8
            const long long i = nv * PL_VEC + threadIdx.x;
            float g;
            local += pl_term<KIND>(to_f(x[i]) - to_f(y[i]), scale, g);
            if (dx) dx[i] = (TX)g;
        }
    } else {                                                          // a pointer that is not 16-byte aligned (a view at an odd storage offset): scalar
        for (long long i = first; i < n; i += step) {
            float g;
            local += pl_term<KIND>(to_f(x[i]) - to_f(y[i]), scale, g);
            if (dx) dx[i] = (TX)g;
        }
    }
    wave_sums_to_lds(local, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum4_pairwise(red) * scale;
}

static_assert(PL_BLOCK == 256, "partials_sum256");
__global__ __launch_bounds__(PL_BLOCK) void pair_sum_kernel(const float* __restrict__ partial, int nblocks, float* __restrict__ loss) {
    partials_sum256(partial, nblocks, loss);
}

// The output indices whose taps can include input index i: the source coordinate f(o) = scale (o + 0.5) - 0.5 is monotone in o and
// i is a tap iff i - 1 < f < i + 1 (or the clamps put it there), so they are the contiguous range (i - 0.5) / scale - 0.5 < o <
// (i + 1.5) / scale - 0.5.  Found in fp64 and widened by one on each side: the fp32 f differs from the exact one by less than 1 output
// step's worth only below RS_MAXDIM, and membership is decided by bil_src (elt.h: the fp32 expressions that resize_bilinear_kernel of
// train_step.hip spells out, so forward and adjoint agree on every tap and weight bit for bit), never by this range.
static __device__ __forceinline__ void rs_range(int i, float scale, int out, int& lo, int& hi) {
    const double s = (double)scale;
    const double a = floor(((double)i - 0.5) / s - 0.5) - 1.0, b = ceil(((double)i + 1.5) / s - 0.5) + 1.0;
    lo = a < 0.0 ? 0 : (a > (double)(out - 1) ? out - 1 : (int)a);
    hi = b > (double)(out - 1) ? out - 1 : (b < 0.0 ? 0 : (int)b);
}

__global__ __launch_bounds__(PL_BLOCK) void resize_bilinear_bwd_kernel(const float* __restrict__ dout, float* __restrict__ din, long long planes,
                                                                       int H, int W, int h, int w) {
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;
    const long long total = planes * H * W;
    for (long long idx = (long long)blockIdx.x * PL_BLOCK + threadIdx.x; idx < total; idx += (long long)gridDim.x * PL_BLOCK) {
        const int X = (int)(idx % W);
        const int Y = (int)((idx / W) % H);
        const long long pl = idx / ((long long)W * H);
        int ylo, yhi, xlo, xhi;
        rs_range(Y, sy, h, ylo, yhi);
        rs_range(X, sx, w, xlo, xhi);
        const float* g = dout + pl * h * w;
        float acc = 0.f;
        for (int y = ylo; y <= yhi; ++y) {
            int y0, y1; float ly;
            bil_src(y, H, y0, y1, ly, sy);
            if (y0 != Y && y1 != Y) continue;
            // on the last row y1 = y0: both weights land on the same input pixel and both are added
            const float wy = (y0 == Y ? 1.f - ly : 0.f) + (y1 == Y ? ly : 0.f);
            const float* row = g + (long long)y * w;
            float racc = 0.f;
            for (int x = xlo; x <= xhi; ++x) {
                int x0, x1; float lx;
                bil_src(x, W, x0, x1, lx, sx);
                if (x0 != X && x1 != X) continue;
                racc += row[x] * ((x0 == X ? 1.f - lx : 0.f) + (x1 == X ? lx : 0.f));
            }
            acc += racc * wy;
        }
        din[idx] = acc;
    }
}

template <typename TX, typename TY>
void pl_launch(int kind, int blocks, hipStream_t st, const void* x, const void* y, void* dx, float* scratch, long long n, float scale, int vec) {
    if (kind == VSR_LOSS_L1)
        hipLaunchKernelGGL((pair_loss_kernel<TX, TY, VSR_LOSS_L1>), dim3(blocks), dim3(PL_BLOCK), 0, st, static_cast<const TX*>(x),
                           static_cast<const TY*>(y), static_cast<TX*>(dx), scratch, n, scale, vec);
    else
        hipLaunchKernelGGL((pair_loss_kernel<TX, TY, VSR_LOSS_MSE>), dim3(blocks), dim3(PL_BLOCK), 0, st, static_cast<const TX*>(x),
                           static_cast<const TY*>(y), static_cast<TX*>(dx), scratch, n, scale, vec);
}

}  // namespace

extern "C" {

size_t vsr_pixel_loss_scratch_floats(void) { return PL_BLOCKS; }

int vsr_pixel_loss_fwd_bwd(int kind, const void* x, int x_dtype, const void* y, int y_dtype, void* dx, float* loss, float* scratch,
                           long long numel, void* stream) {
    if (!x || !y || !loss || !scratch || numel < 1) return VSR_ERR_BADARG;
    if (kind != VSR_LOSS_L1 && kind != VSR_LOSS_MSE) return VSR_ERR_BADARG;
    if (bad_dtype(x_dtype) || bad_dtype(y_dtype)) return VSR_ERR_BADARG;
    const uintptr_t px = reinterpret_cast<uintptr_t>(x), py = reinterpret_cast<uintptr_t>(y), pd = reinterpret_cast<uintptr_t>(dx);
    if ((px & (esize(x_dtype) - 1)) || (pd & (esize(x_dtype) - 1)) || (py & (esize(y_dtype) - 1))) return VSR_ERR_BADARG;
    if ((reinterpret_cast<uintptr_t>(loss) | reinterpret_cast<uintptr_t>(scratch)) & 3) return VSR_ERR_BADARG;
    const int vec = ((px | py | pd) & 15) == 0;            // 16-byte accesses need the alignment; otherwise the scalar loop (same values, another fixed order)
    const long long want = ((vec ? numel / PL_VEC : numel) + PL_BLOCK - 1) / PL_BLOCK;
    const int blocks = (int)(want < 1 ? 1 : (want > PL_BLOCKS ? PL_BLOCKS : want));
    const float scale = 1.0f / (float)numel;
    hipStream_t st = (hipStream_t)stream;
    if (x_dtype == VSR_BF16 && y_dtype == VSR_BF16) pl_launch<bf16_t, bf16_t>(kind, blocks, st, x, y, dx, scratch, numel, scale, vec);
    else if (x_dtype == VSR_BF16) pl_launch<bf16_t, float>(kind, blocks, st, x, y, dx, scratch, numel, scale, vec);
    else if (y_dtype == VSR_BF16) pl_launch<float, bf16_t>(kind, blocks, st, x, y, dx, scratch, numel, scale, vec);
    else pl_launch<float, float>(kind, blocks, st, x, y, dx, scratch, numel, scale, vec);
    hipLaunchKernelGGL(pair_sum_kernel, dim3(1), dim3(PL_BLOCK), 0, st, scratch, blocks, loss);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_resize_bilinear_bwd(const float* dout, float* din, long long planes, int H, int W, int h, int w, void* stream) {
    if (!dout || !din || planes < 1 || H < 1 || W < 1 || h < 1 || w < 1) return VSR_ERR_BADARG;
    if ((reinterpret_cast<uintptr_t>(dout) | reinterpret_cast<uintptr_t>(din)) & 3) return VSR_ERR_BADARG;
    if (H > RS_MAXDIM || W > RS_MAXDIM || h > RS_MAXDIM || w > RS_MAXDIM) return VSR_ERR_UNSUPPORTED;
    long long in_px, out_px, t;
    if (__builtin_mul_overflow((long long)H, (long long)W, &in_px) || __builtin_mul_overflow((long long)h, (long long)w, &out_px) ||
        __builtin_mul_overflow(planes, in_px, &t) || __builtin_mul_overflow(planes, out_px, &t))
        return VSR_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(resize_bilinear_bwd_kernel, dim3(grid_for(planes * in_px, PL_BLOCK)), dim3(PL_BLOCK), 0, (hipStream_t)stream, dout, din,
                       planes, H, W, h, w);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
