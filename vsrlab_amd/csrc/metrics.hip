// PSNR and SSIM of an image pair in one pass over both images (piqa.PSNR / piqa.SSIM with their defaults: the reference's `metric:`
// blocks, conf/train/default.yaml:8-14; core/utils.py:242-252).  DESIGN section 11d.
//
// One workgroup of 256 threads owns one 64 x 256 tile of SSIM outputs of one plane and walks it top to bottom:
//   * the haloed input rows come in chunks of WS rows (WS = window size), 16 bytes per load where the rows allow it, the clamp of x
//     applied on the way in.  What goes to LDS is the pair (u, v) = (x + y, x - y) minus the tile's own first pixel (sx + sy, sx - sy):
//     SSIM needs G(x), G(y), G(x^2 + y^2) and G(xy) only, which are linear in G(u), G(v), G(u^2), G(v^2), and variances do not move
//     with a shift, so the fp32 cancellation in G(u^2) - G(u)^2 is taken on values near zero (constant and identical images come out
//     exact);
//   * thread c filters row r horizontally for output column c (WS 8-byte LDS reads, packed fp32 math on the pairs) and adds the result
//     into the WS running vertical sums it keeps in registers, one per output row that row r belongs to; the sum that row r completes
//     is evaluated to ss and added to the thread's total.  The chunk loop is unrolled by WS so the ring of sums has static indices;
//   * (x - y)^2 is summed where a pixel is staged, over the tile's own 64 x 256 input pixels (the last tile row / column also owns
//     the WS - 1 border rows / columns), so every input pixel counts once.
// The next chunk's global loads are in flight while the current one is filtered (two LDS buffers, one barrier per chunk).
// Per-tile sums go to scratch as fp64; a second launch adds them per image in a fixed order.  No atomics.
#include "host.h"
#include <climits>
#include <cmath>

namespace {

constexpr int MT_TW = 256, MT_TH = 64, MT_THREADS = 256, MT_MAX_WS = 15;

typedef __attribute__((ext_vector_type(2))) float f32x2_t;

struct MetricsArgs {
    const float* x; const float* y;
    double* partial;                       // [planes * tiles_y * tiles_x][2]: sum of ss, sum of (x - y)^2
    int H, W, Ho, Wo, tiles_x, tiles_y;
    int vec;                               // every row segment of a tile starts 16-byte aligned and W is a multiple of 4
    int clamp_x; float lo, hi, c1, c2;
    float g[MT_MAX_WS];
};

__device__ inline f32x2_t pk_fma(f32x2_t a, f32x2_t b, f32x2_t c) { return __builtin_elementwise_fma(a, b, c); }

template <int WS>
__global__ __launch_bounds__(MT_THREADS) void metrics_tile_kernel(MetricsArgs a) {
    constexpr int RW = (MT_TW + WS - 1 + 3) & ~3, QW = RW / 4, ITEMS = WS * QW, NIT = (ITEMS + MT_THREADS - 1) / MT_THREADS;
    __shared__ __attribute__((aligned(16))) f32x2_t rows[2][WS][RW];
    __shared__ double red[2][MT_THREADS / 64];
    const int tid = threadIdx.x;
    const int tiles_pp = a.tiles_x * a.tiles_y;
    const long long plane = blockIdx.x / (unsigned)tiles_pp;
    const int tile = blockIdx.x % (unsigned)tiles_pp, ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const int y0 = ty * MT_TH, x0 = tx * MT_TW;
    const int rows_out = min(MT_TH, a.Ho - y0), cols_out = min(MT_TW, a.Wo - x0);
    const int rows_in = rows_out + WS - 1, cols_in = cols_out + WS - 1;              // x0 + cols_in <= W, y0 + rows_in <= H
    const int own_rows = ty == a.tiles_y - 1 ? rows_in : MT_TH, own_cols = tx == a.tiles_x - 1 ? cols_in : MT_TW;
    const long long base = plane * a.H * a.W + (long long)y0 * a.W + x0;
    const float* xp = a.x + base;
    const float* yp = a.y + base;
    float sx = xp[0];
    const float sy = yp[0];
    if (a.clamp_x) sx = fminf(fmaxf(sx, a.lo), a.hi);

    float4 xr[NIT], yr[NIT];
    float msum = 0.f, ssum = 0.f;

    // global -> registers: chunk `k` = tile rows [k WS, (k+1) WS); what lies outside the tile's input stays (0, 0)
    auto fetch = [&](int k) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * MT_THREADS, row = i / QW, c = 4 * (i - row * QW), r = k * WS + row;
            float4 vx = make_float4(0.f, 0.f, 0.f, 0.f), vy = vx;
            if (i < ITEMS && r < rows_in && c < cols_in) {
                const long long o = (long long)r * a.W + c;
                if (a.vec) {
                    vx = *reinterpret_cast<const float4*>(xp + o);
                    vy = *reinterpret_cast<const float4*>(yp + o);
                } else {
                    vx.x = xp[o]; vy.x = yp[o];
                    if (c + 1 < cols_in) { vx.y = xp[o + 1]; vy.y = yp[o + 1]; }
                    if (c + 2 < cols_in) { vx.z = xp[o + 2]; vy.z = yp[o + 2]; }
                    if (c + 3 < cols_in) { vx.w = xp[o + 3]; vy.w = yp[o + 3]; }
                }
                if (a.clamp_x) {
                    vx.x = fminf(fmaxf(vx.x, a.lo), a.hi); vx.y = fminf(fmaxf(vx.y, a.lo), a.hi);
                    vx.z = fminf(fmaxf(vx.z, a.lo), a.hi); vx.w = fminf(fmaxf(vx.w, a.lo), a.hi);
                    if (!a.vec) {                                                   // the clamp must not lift a pixel that is not there
                        if (c + 1 >= cols_in) vx.y = 0.f;
                        if (c + 2 >= cols_in) vx.z = 0.f;
                        if (c + 3 >= cols_in) vx.w = 0.f;
                    }
                }
            }
            xr[it] = vx; yr[it] = vy;
        }
    };
    // registers -> LDS as shifted (u, v) pairs, and the squared error of the pixels this tile owns
    auto commit = [&](int k, int buf) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int i = tid + it * MT_THREADS, row = i / QW, c = 4 * (i - row * QW), r = k * WS + row;
            if (i < ITEMS) {
                const float4 vx = xr[it], vy = yr[it];
                if (r < own_rows) {
                    const float d0 = vx.x - vy.x, d1 = vx.y - vy.y, d2 = vx.z - vy.z, d3 = vx.w - vy.w;
                    if (c < own_cols) msum = fmaf(d0, d0, msum);
                    if (c + 1 < own_cols) msum = fmaf(d1, d1, msum);
                    if (c + 2 < own_cols) msum = fmaf(d2, d2, msum);
                    if (c + 3 < own_cols) msum = fmaf(d3, d3, msum);
                }
                const float ax = vx.x - sx, bx = vx.y - sx, cx = vx.z - sx, dx = vx.w - sx;
                const float ay = vy.x - sy, by = vy.y - sy, cy = vy.z - sy, dy = vy.w - sy;
                float4* dst = reinterpret_cast<float4*>(&rows[buf][row][c]);
                dst[0] = make_float4(ax + ay, ax - ay, bx + by, bx - by);
                dst[1] = make_float4(cx + cy, cx - cy, dx + dy, dx - dy);
            }
        }
    };

    const f32x2_t shift = {sx + sy, sx - sy};
    f32x2_t acc1[WS], acc2[WS];                  // running vertical sums of G_h(u, v) and G_h(u^2, v^2); slot = output row mod WS
#pragma unroll
    for (int s = 0; s < WS; ++s) { acc1[s] = f32x2_t{0.f, 0.f}; acc2[s] = f32x2_t{0.f, 0.f}; }

    const int nchunks = (rows_in + WS - 1) / WS;
    fetch(0);
    commit(0, 0);
    __syncthreads();
    for (int k = 0; k < nchunks; ++k) {
        const bool more = k + 1 < nchunks;
        if (more) fetch(k + 1);
        const f32x2_t(*buf)[RW] = rows[k & 1];
#pragma unroll
        for (int j = 0; j < WS; ++j) {
            const int r = k * WS + j;
            if (r < rows_in) {
                const f32x2_t* rp = &buf[j][tid];
                // horizontal pass; the taps are symmetric, so the two samples at equal distance from the centre share one multiply
                const f32x2_t mid = rp[WS / 2], gm = {a.g[WS / 2], a.g[WS / 2]};
                f32x2_t h1 = gm * mid, h2 = gm * (mid * mid);
#pragma unroll
                for (int t = 0; t < WS / 2; ++t) {
                    const f32x2_t l = rp[t], rr = rp[WS - 1 - t], gt = {a.g[t], a.g[t]};
                    h1 = pk_fma(gt, l + rr, h1);
                    h2 = pk_fma(gt, pk_fma(rr, rr, l * l), h2);
                }
                // vertical pass: row r is tap t of output row r - t, whose slot is (j - t) mod WS because chunks start at multiples of WS
                acc1[j] = f32x2_t{a.g[0], a.g[0]} * h1;
                acc2[j] = f32x2_t{a.g[0], a.g[0]} * h2;
#pragma unroll
                for (int t = 1; t < WS; ++t) {
                    const int s = (j - t + WS) % WS;
                    const f32x2_t gt = {a.g[t], a.g[t]};
                    acc1[s] = pk_fma(gt, h1, acc1[s]);
                    acc2[s] = pk_fma(gt, h2, acc2[s]);
                }
                if (r >= WS - 1) {                                                  // output row r - (WS - 1) is complete
                    const f32x2_t m = acc1[(j + 1) % WS];
                    const f32x2_t var = pk_fma(-m, m, acc2[(j + 1) % WS]);          // (s_uu, s_vv)
                    const f32x2_t mf = m + shift, mm = mf * mf;                     // (mu_u^2, mu_v^2): mu_x = (mu_u + mu_v) / 2
                    const float num = ((mm.x - mm.y) * 0.5f + a.c1) * ((var.x - var.y) * 0.5f + a.c2);
                    const float den = ((mm.x + mm.y) * 0.5f + a.c1) * ((var.x + var.y) * 0.5f + a.c2);
                    if (tid < cols_out) ssum += num / den;
                }
            }
        }
        if (more) commit(k + 1, (k + 1) & 1);
        __syncthreads();
    }

    // the order of reduce.h (wave sum, then the wave sums in index order), on two values in lock-step: one barrier serves both
    double ds = ssum, dm = msum;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { ds += __shfl_down(ds, off); dm += __shfl_down(dm, off); }
    if ((tid & 63) == 0) { red[0][tid >> 6] = ds; red[1][tid >> 6] = dm; }
    __syncthreads();
    if (tid == 0) {
        double s = red[0][0], m = red[1][0];
        for (int w = 1; w < MT_THREADS / 64; ++w) { s += red[0][w]; m += red[1][w]; }
        a.partial[2 * (long long)blockIdx.x] = s;
        a.partial[2 * (long long)blockIdx.x + 1] = m;
    }
}

// sums[n] = the `per_image` tile partials of image n, added in an order that depends on per_image alone: per thread at stride
// MT_THREADS, then the halving tree of reduce.h (tree_sum256) on two values in lock-step
__global__ __launch_bounds__(MT_THREADS) void metrics_reduce_kernel(const double* partial, double* sums, long long per_image) {
    __shared__ double red[2][MT_THREADS];
    const int tid = threadIdx.x;
    const double* p = partial + 2 * per_image * blockIdx.x;
    double s = 0.0, m = 0.0;
    for (long long i = tid; i < per_image; i += MT_THREADS) { s += p[2 * i]; m += p[2 * i + 1]; }
    red[0][tid] = s; red[1][tid] = m;
    __syncthreads();
    for (int half = MT_THREADS / 2; half >= 1; half >>= 1) {
        if (tid < half) { red[0][tid] += red[0][tid + half]; red[1][tid] += red[1][tid + half]; }
        __syncthreads();
    }
    if (tid == 0) { sums[2 * (long long)blockIdx.x] = red[0][0]; sums[2 * (long long)blockIdx.x + 1] = red[1][0]; }
}

struct MetricsPlan { int Ho, Wo, tiles_x, tiles_y; long long tiles, images; };

int metrics_plan(const VsrMetricsDesc* d, MetricsPlan& p) {
    if (!d || d->planes < 1 || d->C < 1 || d->planes % d->C || bad_dims(1, d->H, d->W)) return VSR_ERR_BADARG;
    if (!(d->sigma > 0.f) || (d->clamp_x && !(d->clamp_lo <= d->clamp_hi))) return VSR_ERR_BADARG;
    const int ws = d->window_size;
    if (ws < 3 || ws > MT_MAX_WS || !(ws & 1) || d->H < ws || d->W < ws) return VSR_ERR_UNSUPPORTED;
    p.Ho = d->H - ws + 1; p.Wo = d->W - ws + 1;
    p.tiles_x = cdiv(p.Wo, MT_TW); p.tiles_y = cdiv(p.Ho, MT_TH);
    p.tiles = d->planes * p.tiles_x * p.tiles_y;
    p.images = d->planes / d->C;
    if (p.tiles > INT_MAX || p.images > INT_MAX) return VSR_ERR_UNSUPPORTED;        // both are a grid's x dimension
    return VSR_OK;
}

}  // namespace

extern "C" {

size_t vsr_metrics_scratch_bytes(const VsrMetricsDesc* d) {
    MetricsPlan p;
    return metrics_plan(d, p) == VSR_OK ? (size_t)p.tiles * 2 * sizeof(double) : 0;
}

int vsr_psnr_ssim(const VsrMetricsDesc* d, const float* x, const float* y, double* sums, void* scratch, size_t scratch_bytes,
                  void* stream) {
    MetricsPlan p;
    CK(metrics_plan(d, p));
    if (!x || !y || !sums || !scratch) return VSR_ERR_BADARG;
    if (scratch_bytes < (size_t)p.tiles * 2 * sizeof(double)) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    MetricsArgs a = {};
    a.x = x; a.y = y; a.partial = reinterpret_cast<double*>(scratch);
    a.H = d->H; a.W = d->W; a.Ho = p.Ho; a.Wo = p.Wo; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y;
    a.vec = d->W % 4 == 0 && (reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) % 16 == 0;
    a.clamp_x = d->clamp_x != 0; a.lo = d->clamp_lo; a.hi = d->clamp_hi; a.c1 = d->c1; a.c2 = d->c2;
    const int ws = d->window_size;
    float total = 0.f;
    for (int i = 0; i < ws; ++i) {
        const float t = (float)i - 0.5f * (float)(ws - 1);
        a.g[i] = expf(-(t * t) / (2.f * d->sigma * d->sigma));
        total += a.g[i];
    }
    for (int i = 0; i < ws; ++i) a.g[i] /= total;
    const dim3 grid((unsigned)p.tiles), block(MT_THREADS);
    switch (ws) {
        case 3: hipLaunchKernelGGL(metrics_tile_kernel<3>, grid, block, 0, st, a); break;
        case 5: hipLaunchKernelGGL(metrics_tile_kernel<5>, grid, block, 0, st, a); break;
        case 7: hipLaunchKernelGGL(metrics_tile_kernel<7>, grid, block, 0, st, a); break;
        case 9: hipLaunchKernelGGL(metrics_tile_kernel<9>, grid, block, 0, st, a); break;
        case 11: hipLaunchKernelGGL(metrics_tile_kernel<11>, grid, block, 0, st, a); break;
        case 13: hipLaunchKernelGGL(metrics_tile_kernel<13>, grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL(metrics_tile_kernel<15>, grid, block, 0, st, a); break;
    }
    HIP_CHECK_RET(hipGetLastError());
    hipLaunchKernelGGL(metrics_reduce_kernel, dim3((unsigned)p.images), block, 0, st, a.partial, sums,
                       (long long)d->C * p.tiles_x * p.tiles_y);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
