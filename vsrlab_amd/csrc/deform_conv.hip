// Deformable 3x3 convolution (torchvision deform_conv2d semantics: stride 1, padding 1, dilation 1, groups 1) and VRT's
// flow-guided alignment (vsr/models/VRT/modules/deform_conv.py:133-145) fused into it, forward and backward.  DESIGN section 11c.
//
// Layout.  x is staged once per call from planar fp32 into channels-last [N][H*W][XC] of T (bf16 or fp32): a gather wants one
// pixel's channels contiguous (cl_stage.h, one tile of width XC with the group map; d x comes back the same way).  Every deformable
// group is padded to cpgp = 8 (cpg <= 8) or a multiple of 16 channels and XC is a multiple of 32, so a 8-channel piece never
// straddles two groups and one bilinear set-up serves a whole piece.  Padding channels are zero in x and in the packed weights.
//
// Forward / data backward: one wave owns 32 consecutive pixels of one image; the pixel is the MFMA column (lane & 31), so each
// lane gathers its own pixel's operand fragment straight from HBM/L2 and no column tile ever exists in memory.
//   forward : Y[cout][pixel]  += Wf[tap][cout][cin] * col[tap][cin][pixel]      (A = packed weights, B = gathered columns)
//   backward: dcol[cin][pixel] = Wb[tap][cin][cout] * dY[cout][pixel]           (A = packed weights, B = dY held in registers)
//             and the accumulator rows (4 consecutive channels per lane) meet the same 4 corners again for d x (fp32 vector
//             atomics), d offset and d mask (per-pixel sums, one owner each: bit-identical across runs).
// Weight gradient: workgroup = (tap, pixel part); it gathers a 64-pixel column tile and the dY tile to LDS (pixels contiguous:
// the K index of this product) and keeps all Cout x Cin accumulator blocks of its tap in registers; partial slabs + a reduction
// launch in a fixed order (bit-identical across runs), as wgrad_mfma.hip does.
#include "elt.h"
#include "cl_stage.h"
#include "reduce.h"
#include "host.h"

namespace {

constexpr int DC_MAXC = CL_MAXW;        // Cin, Cout and the padded channel count XC, which is one cl_stage.h tile: 192
constexpr int DC_MAXOB = DC_MAXC / 32;  // 32-row accumulator blocks
constexpr int DC_MAXOC = DC_MAXC / 16;  // 16-deep K steps over Cout
constexpr int DC_WPIX = 64;             // pixels per weight-gradient tile
constexpr int DC_WROW = DC_WPIX + 8;    // LDS row (elements): 16-byte aligned rows, skewed banks
constexpr int DC_WPARTS = 56;           // pixel parts of the weight gradient: 9 taps x 56 = 504 workgroups
constexpr int DC_WMAXB = 9;             // accumulator blocks per wave: 36 / 4

__device__ __forceinline__ void put(bf16x8_t& f, int i, float v) { f[i] = (bf16_t)v; }
__device__ __forceinline__ void put(f32x8_t& f, int i, float v) { f.v[i] = v; }
__device__ __forceinline__ float get(const bf16x8_t& f, int i) { return (float)f[i]; }
__device__ __forceinline__ float get(const f32x8_t& f, int i) { return f.v[i]; }
__device__ __forceinline__ bf16_t elem(const bf16x8_t& f, int i) { return f[i]; }
__device__ __forceinline__ float elem(const f32x8_t& f, int i) { return f.v[i]; }
template <typename T> __device__ __forceinline__ typename Elt<T>::frag_t load8(const T* p) {
    return *reinterpret_cast<const typename Elt<T>::frag_t*>(p);
}
__device__ __forceinline__ void load4(const float* p, float* v) {
    const f32x4_t t = *reinterpret_cast<const f32x4_t*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
__device__ __forceinline__ void load4(const bf16_t* p, float* v) {
    const bf16x4_t t = *reinterpret_cast<const bf16x4_t*>(p);
    v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
}

struct DeformArgs {
    const void* xs;                       // staged x
    const float *off, *mask;              // plain mode: offset (N, 18 dg, H, W), mask (N, 9 dg, H, W) or null
    const float *raw, *flow;              // flow-guided: conv_offset output (N, 27 dg, H, W), flow (N, 2, H, W), channel 0 = x
    float mrm;
    const void* wpack;
    const float* bias;
    float* y;
    const float* dy;
    float *dxacc, *doff, *dmask, *draw, *dflow;
    float* slab;
    int N, Cin, Cout, H, W, dg, cpg, cpgp, XC, CoutP;
    int flow_guided, parts;
};

// the flow-guided epilogue of the offset convolution (deform_conv.py:134-142); the stand-alone kernel below and the fused
// kernels share these two functions, so a fused call and a plain call on the formed tensors see the same bits
__device__ __forceinline__ float fg_offset(float mrm, float t, float f) { return mrm * t + f; }
__device__ __forceinline__ float fg_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

struct Samp {
    int o00, o01, o10, o11;               // pixel indices of the four corners (clamped into the image)
    float w00, w01, w10, w11;             // bilinear weights, 0 where the corner lies outside
    float ly, lx, m, ty, tx;
    bool v00, v01, v10, v11;
};

// sample position of tap k, group g at pixel (y, x) = index p of image n
__device__ __forceinline__ void setup(const DeformArgs& a, int n, int g, int k, int p, int y, int x, float fy, float fx, Samp& s) {
    const long long HW = (long long)a.H * a.W;
    const int ch = 2 * (g * 9 + k);
    float dy, dx;
    s.ty = s.tx = 0.f; s.m = 1.f;
    if (a.flow_guided) {
        const float* r = a.raw + (long long)n * 27 * a.dg * HW + p;
        s.ty = tanhf(r[ch * HW]); s.tx = tanhf(r[(ch + 1) * HW]);
        dy = fg_offset(a.mrm, s.ty, fy); dx = fg_offset(a.mrm, s.tx, fx);
        s.m = fg_sigmoid(r[(18 * a.dg + g * 9 + k) * HW]);
    } else {
        const float* o = a.off + (long long)n * 18 * a.dg * HW + p;
        dy = o[ch * HW]; dx = o[(ch + 1) * HW];
        if (a.mask) s.m = a.mask[((long long)n * 9 * a.dg + g * 9 + k) * HW + p];
    }
    const float py = (float)(y - 1 + k / 3) + dy, px = (float)(x - 1 + k % 3) + dx;
    const float fy0 = floorf(py), fx0 = floorf(px);
    s.ly = py - fy0; s.lx = px - fx0;
    // far outside (or not a number): every corner invalid; the clamp keeps the int conversion defined
    const bool in = py > -1.f && py < (float)a.H && px > -1.f && px < (float)a.W;
    const int y0 = in ? (int)fy0 : -2, x0 = in ? (int)fx0 : -2;
    const bool vy0 = y0 >= 0 && y0 < a.H, vy1 = y0 + 1 >= 0 && y0 + 1 < a.H;
    const bool vx0 = x0 >= 0 && x0 < a.W, vx1 = x0 + 1 >= 0 && x0 + 1 < a.W;
    s.v00 = vy0 && vx0; s.v01 = vy0 && vx1; s.v10 = vy1 && vx0; s.v11 = vy1 && vx1;
    const int cy0 = vy0 ? y0 : 0, cy1 = vy1 ? y0 + 1 : 0, cx0 = vx0 ? x0 : 0, cx1 = vx1 ? x0 + 1 : 0;
    s.o00 = cy0 * a.W + cx0; s.o01 = cy0 * a.W + cx1; s.o10 = cy1 * a.W + cx0; s.o11 = cy1 * a.W + cx1;
    if (!in) { s.ly = 0.f; s.lx = 0.f; }
    s.w00 = s.v00 ? (1.f - s.ly) * (1.f - s.lx) : 0.f;
    s.w01 = s.v01 ? (1.f - s.ly) * s.lx : 0.f;
    s.w10 = s.v10 ? s.ly * (1.f - s.lx) : 0.f;
    s.w11 = s.v11 ? s.ly * s.lx : 0.f;
}

// 8 channels of the column of one pixel: (bilinear sample) * mask, rounded to T
template <typename T>
__device__ __forceinline__ typename Elt<T>::frag_t gather8(const T* img, int XC, int c, const Samp& s) {
    const auto a = load8<T>(img + (long long)s.o00 * XC + c), b = load8<T>(img + (long long)s.o01 * XC + c);
    const auto d = load8<T>(img + (long long)s.o10 * XC + c), e = load8<T>(img + (long long)s.o11 * XC + c);
    typename Elt<T>::frag_t f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        put(f, i, (s.w00 * get(a, i) + s.w01 * get(b, i) + s.w10 * get(d, i) + s.w11 * get(e, i)) * s.m);
    return f;
}

template <typename T> __device__ __forceinline__ typename Elt<T>::frag_t zero_frag() {
    typename Elt<T>::frag_t f;
#pragma unroll
    for (int i = 0; i < 8; ++i) put(f, i, 0.f);
    return f;
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void deform_fwd_kernel(DeformArgs a) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int HW = a.H * a.W, tpi = cdiv(HW, 32);
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= (long long)a.N * tpi) return;
    const int n = (int)(tile / tpi), p0 = (int)(tile % tpi) * 32 + j;
    const bool pv = p0 < HW;
    const int p = pv ? p0 : HW - 1, y = p / a.W, x = p % a.W;
    const T* img = reinterpret_cast<const T*>(a.xs) + (long long)n * HW * a.XC;
    const T* wp = reinterpret_cast<const T*>(a.wpack);
    float fy = 0.f, fx = 0.f;
    if (a.flow_guided) { fx = a.flow[((long long)n * 2) * HW + p]; fy = a.flow[((long long)n * 2 + 1) * HW + p]; }
    const int nob = a.CoutP / 32, nkc = a.XC / 16;
    f32x16_t acc[DC_MAXOB];
#pragma unroll
    for (int ob = 0; ob < DC_MAXOB; ++ob)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[ob][r] = 0.f;
    for (int k = 0; k < 9; ++k) {
        int curg = -1;
        Samp s;
        for (int kc = 0; kc < nkc; ++kc) {
            const int c = kc * 16 + 8 * h, g = c / a.cpgp;      // this lane's 8 channels and their group
            typename Elt<T>::frag_t b = zero_frag<T>();
            if (g < a.dg) {
                if (g != curg) { curg = g; setup(a, n, g, k, p, y, x, fy, fx, s); }
                b = gather8<T>(img, a.XC, c, s);
            }
            const T* wk = wp + ((long long)(k * nkc + kc) * nob) * 512 + lane * 8;
#pragma unroll
            for (int ob = 0; ob < DC_MAXOB; ++ob)
                if (ob < nob) mma(acc[ob], load8<T>(wk + ob * 512), b);
        }
    }
    if (!pv) return;
#pragma unroll
    for (int ob = 0; ob < DC_MAXOB; ++ob)
        if (ob < nob)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = 32 * ob + 8 * (r >> 2) + 4 * h + (r & 3);
                if (o < a.Cout) a.y[((long long)n * a.Cout + o) * HW + p] = acc[ob][r] + (a.bias ? a.bias[o] : 0.f);
            }
}

// ---- backward: d x (scatter), d offset / d mask or d out / d flow -----------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void deform_bwd_kernel(DeformArgs a) {
    const int lane = threadIdx.x & 63, j = lane & 31, h = lane >> 5;
    const int HW = a.H * a.W, tpi = cdiv(HW, 32);
    const long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= (long long)a.N * tpi) return;
    const int n = (int)(tile / tpi), p0 = (int)(tile % tpi) * 32 + j;
    const bool pv = p0 < HW;
    const int p = pv ? p0 : HW - 1, y = p / a.W, x = p % a.W;
    const T* img = reinterpret_cast<const T*>(a.xs) + (long long)n * HW * a.XC;
    const T* wp = reinterpret_cast<const T*>(a.wpack);
    float* dxi = a.dxacc ? a.dxacc + (long long)n * HW * a.XC : nullptr;
    float fy = 0.f, fx = 0.f;
    if (a.flow_guided) { fx = a.flow[((long long)n * 2) * HW + p]; fy = a.flow[((long long)n * 2 + 1) * HW + p]; }
    const int noc = a.CoutP / 16, ncb = a.XC / 32;
    typename Elt<T>::frag_t dyf[DC_MAXOC];                    // B[k = cout 16 oc + 8 h + e][pixel]
#pragma unroll
    for (int oc = 0; oc < DC_MAXOC; ++oc)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int o = 16 * oc + 8 * h + e;
            put(dyf[oc], e, (pv && o < a.Cout) ? a.dy[((long long)n * a.Cout + o) * HW + p] : 0.f);
        }
    float dfy = 0.f, dfx = 0.f;
    for (int k = 0; k < 9; ++k) {
        int curg = -1;
        Samp s;
        float apy = 0.f, apx = 0.f, am = 0.f;              // this lane's share of the current group's sums
        // the group's sums are complete: add the two lane halves (4 channels of every 8 each) and store once per pixel
        auto flush = [&](int g) {
            const float sy = (apy + __shfl_xor(apy, 32)) * s.m, sx = (apx + __shfl_xor(apx, 32)) * s.m, sm = am + __shfl_xor(am, 32);
            if (h == 0 && pv) {
                const int ch = 2 * (g * 9 + k);
                if (a.flow_guided) {
                    if (a.draw) {
                        float* r = a.draw + (long long)n * 27 * a.dg * HW + p;
                        r[(long long)ch * HW] = sy * a.mrm * (1.f - s.ty * s.ty);
                        r[(long long)(ch + 1) * HW] = sx * a.mrm * (1.f - s.tx * s.tx);
                        r[(long long)(18 * a.dg + g * 9 + k) * HW] = sm * s.m * (1.f - s.m);
                    }
                    dfy += sy; dfx += sx;
                } else {
                    if (a.doff) {
                        float* o = a.doff + (long long)n * 18 * a.dg * HW + p;
                        o[(long long)ch * HW] = sy; o[(long long)(ch + 1) * HW] = sx;
                    }
                    if (a.dmask) a.dmask[((long long)n * 9 * a.dg + g * 9 + k) * HW + p] = sm;
                }
            }
            apy = apx = am = 0.f;
        };
        for (int cb = 0; cb < ncb; ++cb) {
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const T* wk = wp + ((long long)(k * ncb + cb) * noc) * 512 + lane * 8;
#pragma unroll
            for (int oc = 0; oc < DC_MAXOC; ++oc)
                if (oc < noc) mma(acc, load8<T>(wk + oc * 512), dyf[oc]);
            // acc[4 q + i] = d col of channel 32 cb + 8 q + 4 h + i at this lane's pixel
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c0 = 32 * cb + 8 * q, g = c0 / a.cpgp;      // wave-uniform
                if (g < a.dg) {
                    if (g != curg) {
                        if (curg >= 0) flush(curg);
                        curg = g;
                        setup(a, n, g, k, p, y, x, fy, fx, s);
                    }
                    const int c = c0 + 4 * h;
                    float v00[4], v01[4], v10[4], v11[4];
                    load4(img + (long long)s.o00 * a.XC + c, v00); load4(img + (long long)s.o01 * a.XC + c, v01);
                    load4(img + (long long)s.o10 * a.XC + c, v10); load4(img + (long long)s.o11 * a.XC + c, v11);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float gc = acc[4 * q + i];
                        const float a00 = s.v00 ? v00[i] : 0.f, a01 = s.v01 ? v01[i] : 0.f, a10 = s.v10 ? v10[i] : 0.f, a11 = s.v11 ? v11[i] : 0.f;
                        if (dxi && pv) {
                            const float gm = gc * s.m;
                            if (s.v00) unsafeAtomicAdd(dxi + (long long)s.o00 * a.XC + c + i, s.w00 * gm);
                            if (s.v01) unsafeAtomicAdd(dxi + (long long)s.o01 * a.XC + c + i, s.w01 * gm);
                            if (s.v10) unsafeAtomicAdd(dxi + (long long)s.o10 * a.XC + c + i, s.w10 * gm);
                            if (s.v11) unsafeAtomicAdd(dxi + (long long)s.o11 * a.XC + c + i, s.w11 * gm);
                        }
                        am += gc * (s.w00 * a00 + s.w01 * a01 + s.w10 * a10 + s.w11 * a11);
                        apy += gc * ((1.f - s.lx) * (a10 - a00) + s.lx * (a11 - a01));
                        apx += gc * ((1.f - s.ly) * (a01 - a00) + s.ly * (a11 - a10));
                    }
                }
            }
        }
        if (curg >= 0) flush(curg);
    }
    if (a.flow_guided && a.dflow && h == 0 && pv) {
        a.dflow[((long long)n * 2) * HW + p] = dfx;
        a.dflow[((long long)n * 2 + 1) * HW + p] = dfy;
    }
}

// ---- weight gradient --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void deform_wgrad_kernel(DeformArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T* col = reinterpret_cast<T*>(smem);                   // [XC][DC_WROW]
    T* dyt = col + a.XC * DC_WROW;                         // [CoutP][DC_WROW]
    const int k = blockIdx.x % 9, part = blockIdx.x / 9;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, j = lane & 31, h = lane >> 5;
    const int HW = a.H * a.W, tpi = cdiv(HW, DC_WPIX), ntiles = a.N * tpi;
    const int nob = a.CoutP / 32, ncb = a.XC / 32, nb = nob * ncb;
    f32x16_t acc[DC_WMAXB];
#pragma unroll
    for (int b = 0; b < DC_WMAXB; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[b][r] = 0.f;
    for (int tile = part; tile < ntiles; tile += a.parts) {
        const int n = tile / tpi, pbase = (tile % tpi) * DC_WPIX;
        __syncthreads();                                   // the previous tile's MFMAs have read their operands
        {   // column tile: lane = pixel, wave w takes the 8-channel pieces w, w + 4, ...
            const int p0 = pbase + lane;
            const bool pv = p0 < HW;
            const int p = pv ? p0 : HW - 1, y = p / a.W, x = p % a.W;
            const T* img = reinterpret_cast<const T*>(a.xs) + (long long)n * HW * a.XC;
            float fy = 0.f, fx = 0.f;
            if (a.flow_guided) { fx = a.flow[((long long)n * 2) * HW + p]; fy = a.flow[((long long)n * 2 + 1) * HW + p]; }
            int curg = -1;
            Samp s;
            for (int c8 = wave; c8 < a.XC / 8; c8 += 4) {
                const int c = 8 * c8, g = c / a.cpgp;
                typename Elt<T>::frag_t f = zero_frag<T>();
                if (g < a.dg && pv) {
                    if (g != curg) { curg = g; setup(a, n, g, k, p, y, x, fy, fx, s); }
                    f = gather8<T>(img, a.XC, c, s);
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) col[(c + e) * DC_WROW + lane] = elem(f, e);
            }
            for (int idx = t; idx < a.CoutP * DC_WPIX; idx += 256) {
                const int o = idx / DC_WPIX, px = idx % DC_WPIX;
                const float v = (o < a.Cout && pbase + px < HW) ? a.dy[((long long)n * a.Cout + o) * HW + pbase + px] : 0.f;
                dyt[o * DC_WROW + px] = (T)v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < DC_WMAXB; ++b) {
            const int blk = wave + 4 * b;
            if (blk < nb) {
                const int ob = blk / ncb, cb = blk % ncb;
                const T* pa = dyt + (32 * ob + j) * DC_WROW + 8 * h;       // A[cout][pixel 16 s + 8 h + e]
                const T* pb = col + (32 * cb + j) * DC_WROW + 8 * h;       // B[pixel][cin]
#pragma unroll
                for (int s = 0; s < DC_WPIX / 16; ++s) mma(acc[b], load8<T>(pa + 16 * s), load8<T>(pb + 16 * s));
            }
        }
    }
    // slab[part][tap][cout][XC]
    float* sl = a.slab + ((long long)part * 9 + k) * a.CoutP * a.XC;
#pragma unroll
    for (int b = 0; b < DC_WMAXB; ++b) {
        const int blk = wave + 4 * b;
        if (blk < nb) {
            const int ob = blk / ncb, cb = blk % ncb;
#pragma unroll
            for (int r = 0; r < 16; ++r) sl[(long long)(32 * ob + 8 * (r >> 2) + 4 * h + (r & 3)) * a.XC + 32 * cb + j] = acc[b][r];
        }
    }
}

__global__ void deform_wgrad_reduce_kernel(const float* slab, int parts, int Cout, int Cin, int cpg, int cpgp, int XC, int CoutP, float* gw) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Cout * Cin * 9) return;
    const int k = idx % 9, ci = (idx / 9) % Cin, o = idx / (9 * Cin);
    const int cp = (ci / cpg) * cpgp + ci % cpg;
    float s = 0.f;
    for (int part = 0; part < parts; ++part) s += slab[(((long long)part * 9 + k) * CoutP + o) * XC + cp];
    gw[idx] = s;
}

// d bias[o] = sum of dY[:, o]: one workgroup per channel, fixed order (reduce.h)
__global__ __launch_bounds__(256) void deform_bgrad_kernel(const float* dy, float* gb, int N, int Cout, int HW) {
    __shared__ float red[256];
    const int o = blockIdx.x, t = threadIdx.x;
    float s = 0.f;
    for (int n = 0; n < N; ++n) {
        const float* r = dy + ((long long)n * Cout + o) * HW;
        for (int p = t; p < HW; p += 256) s += r[p];
    }
    tree_sum256(s, red);
    if (t == 0) gb[o] = red[0];
}

// ---- packing ----------------------------------------------------------------------------------------------------------
// weights (Cout, Cin, 3, 3) fp32 -> MFMA A fragments, 512 elements (64 lanes x 8) per (tap, K step, row block):
//   mode 0 (forward):  [tap][XC/16][CoutP/32]: lane (i, h), e -> W[cout 32 ob + i][channel 16 kc + 8 h + e]
//   mode 1 (backward): [tap][XC/32][CoutP/16]: lane (i, h), e -> W[cout 16 oc + 8 h + e][channel 32 cb + i]
template <typename T>
__global__ void deform_pack_kernel(const float* w, T* dst, int mode, int Cout, int Cin, int cpg, int cpgp, int dg, int XC, int CoutP) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 9 * XC * CoutP) return;
    const int e = idx & 7, lane = (idx >> 3) & 63, i = lane & 31, h = lane >> 5;
    int rest = idx >> 9, o, cp;
    if (mode == 0) {
        const int nob = CoutP / 32, ob = rest % nob, kc = (rest / nob) % (XC / 16);
        rest /= nob * (XC / 16);
        o = 32 * ob + i; cp = 16 * kc + 8 * h + e;
    } else {
        const int noc = CoutP / 16, oc = rest % noc, cb = (rest / noc) % (XC / 32);
        rest /= noc * (XC / 32);
        o = 16 * oc + 8 * h + e; cp = 32 * cb + i;
    }
    const int k = rest, g = cp / cpgp, cl = cp % cpgp;
    const bool ok = g < dg && cl < cpg && o < Cout;
    dst[idx] = (T)(ok ? w[((long long)o * Cin + g * cpg + cl) * 9 + k] : 0.f);
}

__global__ void deform_offset_mask_kernel(const float* raw, const float* flow, float mrm, int dg, long long HW, long long total,
                                          float* off, float* mask) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const long long p = idx % HW;
    const int c = (int)((idx / HW) % (27 * dg));
    const long long n = idx / (HW * 27 * dg);
    const float v = raw[idx];
    if (c < 18 * dg) off[(n * 18 * dg + c) * HW + p] = fg_offset(mrm, tanhf(v), flow[(n * 2 + ((c & 1) ? 0 : 1)) * HW + p]);
    else mask[(n * 9 * dg + (c - 18 * dg)) * HW + p] = fg_sigmoid(v);
}

// ---- host -------------------------------------------------------------------------------------------------------------
struct DeformPlan {
    int cpg, cpgp, XC, CoutP, parts;
    size_t xs, wpack, dxacc, slab, total;
};

int deform_plan(const VsrDeformDesc* d, int backward, DeformPlan& pl) {
    if (!d || bad_dims(d->N, d->H, d->W) || d->Cin < 1 || d->Cout < 1 || d->deform_groups < 1 || bad_dtype(d->dtype)) return VSR_ERR_BADARG;
    if (d->flow_guided && !d->modulated) return VSR_ERR_BADARG;
    if (d->Cin % d->deform_groups) return VSR_ERR_UNSUPPORTED;
    if (d->Cin > DC_MAXC || d->Cout > DC_MAXC) return VSR_ERR_UNSUPPORTED;
    if ((long long)d->H * d->W > (1ll << 24) || (long long)d->N * d->H * d->W > (1ll << 30)) return VSR_ERR_UNSUPPORTED;
    pl.cpg = d->Cin / d->deform_groups;
    pl.cpgp = pl.cpg <= 8 ? 8 : (pl.cpg + 15) & ~15;
    pl.XC = (d->deform_groups * pl.cpgp + 31) & ~31;
    if (pl.XC > DC_MAXC) return VSR_ERR_UNSUPPORTED;      // e.g. 180 channels in 18 groups of 10
    pl.CoutP = (d->Cout + 31) & ~31;
    const long long pix = (long long)d->N * d->H * d->W;
    const int ntiles = d->N * cdiv(d->H * d->W, DC_WPIX);
    pl.parts = ntiles < DC_WPARTS ? ntiles : DC_WPARTS;
    Bump b;
    pl.xs = b.take((size_t)pix * pl.XC * esize(d->dtype));
    pl.wpack = b.take((size_t)9 * pl.XC * pl.CoutP * esize(d->dtype));
    pl.dxacc = pl.slab = 0;
    if (backward) {
        pl.dxacc = b.take((size_t)pix * pl.XC * 4);
        pl.slab = b.take((size_t)pl.parts * 9 * pl.CoutP * pl.XC * 4);
    }
    pl.total = b.off;
    return VSR_OK;
}

template <typename T>
int deform_prepare(const VsrDeformDesc* d, const DeformPlan& pl, const float* x, const float* weight, int mode, char* ws, hipStream_t st) {
    cl_pack<0>(st, d->N, d->Cin, d->H * d->W, pl.XC, ClGroups{pl.cpg, pl.cpgp}, x, reinterpret_cast<T*>(ws + pl.xs));
    hipLaunchKernelGGL(deform_pack_kernel<T>, dim3(cdiv(9 * pl.XC * pl.CoutP, 256)), dim3(256), 0, st, weight, reinterpret_cast<T*>(ws + pl.wpack),
                       mode, d->Cout, d->Cin, pl.cpg, pl.cpgp, d->deform_groups, pl.XC, pl.CoutP);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

DeformArgs deform_args(const VsrDeformDesc* d, const DeformPlan& pl, const float* om, const float* mask, const float* flow, char* ws) {
    DeformArgs a = {};
    a.xs = ws + pl.xs; a.wpack = ws + pl.wpack;
    if (d->flow_guided) { a.raw = om; a.flow = flow; a.mrm = d->max_residue; }
    else { a.off = om; a.mask = d->modulated ? mask : nullptr; }
    a.N = d->N; a.Cin = d->Cin; a.Cout = d->Cout; a.H = d->H; a.W = d->W; a.dg = d->deform_groups;
    a.cpg = pl.cpg; a.cpgp = pl.cpgp; a.XC = pl.XC; a.CoutP = pl.CoutP; a.flow_guided = d->flow_guided; a.parts = pl.parts;
    return a;
}

bool deform_bad_inputs(const VsrDeformDesc* d, const float* x, const float* om, const float* mask, const float* flow, const float* weight) {
    if (!x || !om || !weight) return true;
    if (d->flow_guided) return !flow || mask;
    return d->modulated ? !mask : mask != nullptr;
}

}  // namespace

extern "C" {

size_t vsr_deform_conv_workspace_bytes(const VsrDeformDesc* d, int need_backward) {
    DeformPlan pl;
    return deform_plan(d, need_backward, pl) == VSR_OK ? pl.total : 0;
}

int vsr_deform_conv_fwd(const VsrDeformDesc* d, const float* x, const float* offset, const float* mask, const float* flow,
                        const float* weight, const float* bias, float* y, void* workspace, size_t workspace_bytes, void* stream) {
    DeformPlan pl;
    CK(deform_plan(d, 0, pl));
    if (deform_bad_inputs(d, x, offset, mask, flow, weight) || !y || !workspace) return VSR_ERR_BADARG;
    if (workspace_bytes < pl.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    DeformArgs a = deform_args(d, pl, offset, mask, flow, ws);
    a.bias = bias; a.y = y;
    const int grid = (int)(((long long)d->N * cdiv(d->H * d->W, 32) + 3) / 4);
    if (d->dtype == VSR_BF16) {
        CK(deform_prepare<bf16_t>(d, pl, x, weight, 0, ws, st));
        hipLaunchKernelGGL(deform_fwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
    } else {
        CK(deform_prepare<float>(d, pl, x, weight, 0, ws, st));
        hipLaunchKernelGGL(deform_fwd_kernel<float>, dim3(grid), dim3(256), 0, st, a);
    }
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_deform_conv_bwd(const VsrDeformDesc* d, const float* x, const float* offset, const float* mask, const float* flow,
                        const float* weight, const float* dy, float* dx, float* doffset, float* dmask, float* dflow,
                        float* dweight, float* dbias, void* workspace, size_t workspace_bytes, void* stream) {
    DeformPlan pl;
    CK(deform_plan(d, 1, pl));
    if (deform_bad_inputs(d, x, offset, mask, flow, weight) || !dy || !workspace) return VSR_ERR_BADARG;
    if ((dmask && (d->flow_guided || !d->modulated)) || (dflow && !d->flow_guided)) return VSR_ERR_BADARG;
    if (workspace_bytes < pl.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* ws = reinterpret_cast<char*>(workspace);
    const int HW = d->H * d->W;
    const bool bf = d->dtype == VSR_BF16;
    DeformArgs a = deform_args(d, pl, offset, mask, flow, ws);
    a.dy = dy;
    CK(bf ? deform_prepare<bf16_t>(d, pl, x, weight, 1, ws, st) : deform_prepare<float>(d, pl, x, weight, 1, ws, st));
    if (dx || doffset || dmask || dflow) {
        if (dx) {
            a.dxacc = reinterpret_cast<float*>(ws + pl.dxacc);
            HIP_CHECK_RET(hipMemsetAsync(a.dxacc, 0, (size_t)d->N * HW * pl.XC * 4, st));
        }
        if (d->flow_guided) { a.draw = doffset; a.dflow = dflow; }
        else { a.doff = doffset; a.dmask = dmask; }
        const int grid = (int)(((long long)d->N * cdiv(HW, 32) + 3) / 4);
        if (bf) hipLaunchKernelGGL(deform_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, st, a);
        else hipLaunchKernelGGL(deform_bwd_kernel<float>, dim3(grid), dim3(256), 0, st, a);
        HIP_CHECK_RET(hipGetLastError());
        if (dx) cl_unpack<0>(st, d->N, d->Cin, HW, pl.XC, ClGroups{pl.cpg, pl.cpgp}, a.dxacc, dx);
    }
    if (dweight) {
        a.slab = reinterpret_cast<float*>(ws + pl.slab);
        const size_t lds = (size_t)(pl.XC + pl.CoutP) * DC_WROW * esize(d->dtype);
        static VsrDevOnce once_b, once_f;
        if (bf) {
            CK(vsr_set_max_dynamic_lds(once_b, reinterpret_cast<const void*>(&deform_wgrad_kernel<bf16_t>), 160 * 1024));
            hipLaunchKernelGGL(deform_wgrad_kernel<bf16_t>, dim3(9 * pl.parts), dim3(256), lds, st, a);
        } else {
            CK(vsr_set_max_dynamic_lds(once_f, reinterpret_cast<const void*>(&deform_wgrad_kernel<float>), 160 * 1024));
            hipLaunchKernelGGL(deform_wgrad_kernel<float>, dim3(9 * pl.parts), dim3(256), lds, st, a);
        }
        hipLaunchKernelGGL(deform_wgrad_reduce_kernel, dim3(cdiv(d->Cout * d->Cin * 9, 256)), dim3(256), 0, st, a.slab, pl.parts, d->Cout, d->Cin,
                           pl.cpg, pl.cpgp, pl.XC, pl.CoutP, dweight);
    }
    if (dbias) hipLaunchKernelGGL(deform_bgrad_kernel, dim3(d->Cout), dim3(256), 0, st, dy, dbias, d->N, d->Cout, HW);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_deform_offset_mask(const VsrDeformDesc* d, const float* out, const float* flow, float* offset, float* mask, void* stream) {
    DeformPlan pl;
    CK(deform_plan(d, 0, pl));
    if (!d->flow_guided || !out || !flow || !offset || !mask) return VSR_ERR_BADARG;
    const long long HW = (long long)d->H * d->W, total = (long long)d->N * 27 * d->deform_groups * HW;
    hipLaunchKernelGGL(deform_offset_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, flow,
                       d->max_residue, d->deform_groups, HW, total, offset, mask);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
