// The spatio-temporal convolution of the reference's core/modules (conv.py: ConvST / ConvSTBlock; upsampling.py: PixelShufflePack3D) and
// of VRT's reconstruction tail (vrt.py: Upsample, conv_first, conv_before_upsample, conv_last): one stride-1 'same' Conv3d over the tap
// sets (1,3,3), (3,1,1) and (3,3,3), on planar operands read through batch / channel / frame strides.  DESIGN section 11k is the
// specification.  Built into a library of its own, libvsrlab_conv3d.so (include/vsrlab_conv3d.h): libvsrlab_hip.so's exports stay as
// they are.
//
//   conv3d_pack_kernel:  the fp32 (Cout, Cin, kt, kh, kw) weight -> MFMA A fragments of type T, [cout block of 64][cin chunk of 16]
//       [tap][part][32-row block][lane]: a fragment is one 16-byte (bf16) / 32-byte (fp32) load.  Channel counts are padded to the
//       granule HERE, with zeros, never in the caller's tensors.  `transposed`: the flipped, transposed weight of the data gradient.
//       The weights are fp32 by the ABI, and stay so in effect: in bf16 a weight is packed as TWO parts, hi = bf16(w) and
//       lo = bf16(w - hi), and the kernel issues one MFMA per part (w x to 2^-17, where a single rounding of w would put the result
//       at sqrt 2 x the error of its own storage rounding).
//   conv3d_kernel:  implicit GEMM, M = Cout, N = 32 pixels along W, K = Cin per tap.  A workgroup owns an 8-row x 32-pixel tile of one
//       frame and 64 output channels; per chunk of 16 input channels it stages the (kt) x (8 + 2) x (32 + 2) patch from the planar
//       operand into LDS as [frame][row][pixel][16 channels] -- the global side reads whole pixel rows of one channel plane, the LDS
//       side writes and reads 8 channels of a pixel as one 16- / 32-byte piece, so a B fragment is one ds_read_b128 (two in fp32).
//       A wave owns two rows of the tile and both 32-channel blocks (4 accumulator sets).  The epilogue adds the bias, applies the
//       LeakyReLU and stores planar through the output strides, or through the PixelShuffle(2) pattern.  The data gradient is this
//       kernel on the transposed pack.
//   conv3d_dz_kernel:  dz = lrelu'(y) * unshuffle(dy), once, into the workspace (only with an activation or a shuffle).
//   conv3d_wgrad_kernel + conv3d_reduce_kernel:  M = Cout, N = Cin, K = pixels.  A workgroup owns a 64 x 64 block of (cout, cin) pairs
//       (a wave one 32 x 32 block, all kh x kw taps of one frame tap in accumulators) and walks every grid-th 2-row x 32-pixel tile;
//       one partial set per workgroup, added in workgroup order by the second launch.  conv3d_dbias_kernel: the same for db.
//       No atomics: bit-identical from run to run.
#include "elt.h"
#include "host.h"
#include "../../include/vsrlab_conv3d.h"

namespace {

typedef long long i64;
constexpr int TILE_H = 8;                      // rows of a forward tile: 4 waves x 2 rows
constexpr int WG_TH = 2;                       // rows of a weight-gradient tile
constexpr int WG_MAX_PARTS = 512;              // partial sets of a weight gradient at most ...
constexpr i64 WG_MAX_BYTES = 64ll << 20;       // ... and their bytes
constexpr int DB_PARTS = 64;

template <typename T> constexpr int wparts() { return sizeof(T) == 2 ? 2 : 1; }       // parts of a packed weight: hi (+ lo in bf16)
template <typename T> static __device__ __forceinline__ typename Elt<T>::frag_t ldfrag(const T* p);
template <> __device__ __forceinline__ bf16x8_t ldfrag<bf16_t>(const bf16_t* p) { return *reinterpret_cast<const bf16x8_t*>(p); }
template <> __device__ __forceinline__ f32x8_t ldfrag<float>(const float* p) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    f32x8_t f;
    f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
    return f;
}
static __device__ __forceinline__ void put(bf16x8_t& f, int j, bf16_t v) { f[j] = v; }
static __device__ __forceinline__ void put(f32x8_t& f, int j, float v) { f.v[j] = v; }
static __device__ __forceinline__ void zero16(f32x16_t& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = 0.f;
}

// ---- weight packing ---------------------------------------------------------------------------------------------------------------------
// M x K x NT (rows, reduction, taps) from w: (M, K, NT), or (transposed) from w: (K, M, NT) with the taps reversed
template <typename T>
__global__ __launch_bounds__(256) void conv3d_pack_kernel(const float* __restrict__ w, T* __restrict__ out, int M, int K, int NT, int nkc,
                                                          int transposed, int total) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    int q = idx;
    const int lane = q & 63; q >>= 6;
    const int mb = q & 1; q >>= 1;
    const int tap = q % NT; q /= NT;
    const int kc = q % nkc, cb = q / nkc;
    const int m = cb * 64 + mb * 32 + (lane & 31), k0 = kc * 16 + (lane >> 5) * 8;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = k0 + j;
        v[j] = 0.f;
        if (m < M && k < K) v[j] = transposed ? w[((i64)k * M + m) * NT + (NT - 1 - tap)] : w[((i64)m * K + k) * NT + tap];
    }
    constexpr int NP = wparts<T>();
    T* o = out + ((i64)((idx >> 7) * NP) * 128 + (idx & 127)) * 8;                       // part 0 of this (.., tap)'s [part][block][lane]
    st8<T>(o, v);
    if (NP == 2) {
        float hi[8];
        ld8<T>(o, hi);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] -= hi[j];
        st8<T>(o + 128 * 8, v);
    }
}

// ---- forward / data gradient --------------------------------------------------------------------------------------------------------------
struct CArgs {
    const void* in; void* out; const void* wpack; const float* bias;
    i64 isb, isc, ist, osb, osc, ost;
    int Cin, Cout, T, H, W, tiles_h, tiles_w, nkc, act, shuffle;
    float slope;
};

template <typename T, int KT, int KS>
__global__ __launch_bounds__(256) void conv3d_kernel(const CArgs a) {
    typedef typename Elt<T>::frag_t frag_t;
    constexpr int PH = TILE_H + KS - 1, PW = 32 + KS - 1, NT = KT * KS * KS, PS = KS / 2, PT = KT / 2, NP = wparts<T>();
    __shared__ __attribute__((aligned(16))) T patch[KT * PH * PW * 16];                   // [frame][row][pixel][16 channels]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
    int q = blockIdx.x;
    const int tw = q % a.tiles_w; q /= a.tiles_w;
    const int th = q % a.tiles_h; q /= a.tiles_h;
    const int t = q % a.T, b = q / a.T;
    const int h0 = th * TILE_H, w0 = tw * 32, cb = blockIdx.y, row0 = 2 * wave;
    const T* in = static_cast<const T*>(a.in) + (i64)b * a.isb;
    const bool active = h0 + row0 < a.H, two = a.Cout - cb * 64 > 32;
    const T* wp = static_cast<const T*>(a.wpack) + ((i64)cb * a.nkc * NT * NP * 2 * 64 + lane) * 8;
    f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) zero16(acc[i >> 1][i & 1]);

    for (int kc = 0; kc < a.nkc; ++kc) {
        __syncthreads();                                                                 // the previous chunk's reads are done
        for (int idx = tid; idx < KT * PH * PW * 2; idx += 256) {                        // lanes along the pixel row
            int r = idx / PW;
            const int p = idx - r * PW;
            int f = r / PH;
            r -= f * PH;
            const int half = f / KT;
            f -= half * KT;
            const int tt = t + f - PT, row = h0 + r - PS, col = w0 + p - PS;
            const bool ok = tt >= 0 && tt < a.T && row >= 0 && row < a.H && col >= 0 && col < a.W;
            const i64 off = (i64)tt * a.ist + (i64)row * a.W + col;
            const int c0 = kc * 16 + half * 8;
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (ok && c0 + j < a.Cin) ? to_f(in[off + (i64)(c0 + j) * a.isc]) : 0.f;
            st8<T>(&patch[((f * PH + r) * PW + p) * 16 + half * 8], v);
        }
        __syncthreads();
        if (active) {
            const T* wk = wp + (i64)kc * NT * NP * 2 * 64 * 8;
#pragma unroll
            for (int f = 0; f < KT; ++f)
#pragma unroll
                for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        const int tap = (f * KS + ky) * KS + kx;
                        const frag_t b0 = ldfrag<T>(&patch[((f * PH + row0 + ky) * PW + l32 + kx) * 16 + kg * 8]);
                        const frag_t b1 = ldfrag<T>(&patch[((f * PH + row0 + 1 + ky) * PW + l32 + kx) * 16 + kg * 8]);
#pragma unroll
                        for (int part = 0; part < NP; ++part) {
                            const frag_t a0 = ldfrag<T>(wk + ((tap * NP + part) * 2 + 0) * 64 * 8);
                            mma(acc[0][0], a0, b0);
                            mma(acc[0][1], a0, b1);
                            if (two) {
                                const frag_t a1 = ldfrag<T>(wk + ((tap * NP + part) * 2 + 1) * 64 * 8);
                                mma(acc[1][0], a1, b0);
                                mma(acc[1][1], a1, b1);
                            }
                        }
                    }
        }
    }
    if (!active) return;
    T* out = static_cast<T*>(a.out) + (i64)b * a.osb + (i64)t * a.ost;
    const int col = w0 + l32;
#pragma unroll
    for (int mb = 0; mb < 2; ++mb)
#pragma unroll
        for (int r2 = 0; r2 < 2; ++r2) {
            const int row = h0 + row0 + r2;
            if (row >= a.H || col >= a.W) continue;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int co = cb * 64 + mb * 32 + 8 * (i >> 2) + 4 * kg + (i & 3);
                if (co >= a.Cout) continue;
                float v = acc[mb][r2][i];
                if (a.bias) v += a.bias[co];
                if (a.act == VSR_CONV3D_ACT_LEAKY) v = v > 0.f ? v : v * a.slope;
                if (a.shuffle)
                    out[(i64)(co >> 2) * a.osc + (i64)(2 * row + ((co >> 1) & 1)) * (2 * a.W) + 2 * col + (co & 1)] = (T)v;
                else
                    out[(i64)co * a.osc + (i64)row * a.W + col] = (T)v;
            }
        }
}

// ---- dz = lrelu'(y) * unshuffle(dy), (B, Cout, T, H, W) contiguous ------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void conv3d_dz_kernel(const T* __restrict__ y, const T* __restrict__ dy, T* __restrict__ dz, i64 total, int Cout,
                                                        int Tn, int H, int W, i64 sb, i64 sc, i64 st, int act, float slope, int shuffle) {
    for (i64 idx = (i64)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (i64)gridDim.x * 256) {
        i64 q = idx;
        const int w = (int)(q % W); q /= W;
        const int h = (int)(q % H); q /= H;
        const int t = (int)(q % Tn); q /= Tn;
        const int co = (int)(q % Cout);
        const i64 b = q / Cout;
        const i64 off = shuffle ? b * sb + (i64)(co >> 2) * sc + (i64)t * st + (i64)(2 * h + ((co >> 1) & 1)) * (2 * W) + 2 * w + (co & 1)
                                : b * sb + (i64)co * sc + (i64)t * st + (i64)h * W + w;
        float g = to_f(dy[off]);
        if (act == VSR_CONV3D_ACT_LEAKY && !(to_f(y[off]) > 0.f)) g *= slope;
        dz[idx] = (T)g;
    }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
struct WArgs {
    const void* x; const void* dz; float* partial;
    i64 xsb, xsc, xst, zsb, zsc, zst, tiles, E;
    int Cin, Cout, T, H, W, KT, tiles_h, tiles_w, ncib;
};

// an LDS row stride (elements) of an odd number of dwords, at least `base`: lanes a row apart fall into different banks
template <typename T> constexpr int odd_stride(int base) { return sizeof(T) == 2 ? ((base + 3) / 4) * 4 + 2 : (base | 1); }

template <typename T, int KS>
__global__ __launch_bounds__(256) void conv3d_wgrad_kernel(const WArgs a) {
    typedef typename Elt<T>::frag_t frag_t;
    constexpr int XR = WG_TH + KS - 1, XW = 32 + KS - 1, XWP = XW + (KS > 1 ? 2 : 0), PS = KS / 2;
    constexpr int XCS = odd_stride<T>(XR * XWP), ZCS = odd_stride<T>(WG_TH * 32);
    __shared__ T xl[64 * XCS];                                                           // [cin][row][pixel]
    __shared__ T zl[64 * ZCS];                                                           // [cout][row][pixel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, kg = lane >> 5;
    const int cob = blockIdx.y / a.ncib, cib = blockIdx.y - cob * a.ncib, mb = wave >> 1, nb = wave & 1;
    const bool wave_on = cob * 64 + mb * 32 < a.Cout && cib * 64 + nb * 32 < a.Cin;
    const T* xg = static_cast<const T*>(a.x);
    const T* zg = static_cast<const T*>(a.dz);
    const int NT = a.KT * KS * KS;
    float* mine = a.partial + (i64)blockIdx.x * a.E;

    for (int f = 0; f < a.KT; ++f) {
        f32x16_t acc[KS][KS];
#pragma unroll
        for (int i = 0; i < KS * KS; ++i) zero16(acc[i / KS][i % KS]);
        for (i64 tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {                 // tiles in index order
            i64 q = tile;
            const int tw = (int)(q % a.tiles_w); q /= a.tiles_w;
            const int th = (int)(q % a.tiles_h); q /= a.tiles_h;
            const int t = (int)(q % a.T);
            const i64 b = q / a.T;
            const int tt = t + f - a.KT / 2, h0 = th * WG_TH, w0 = tw * 32;
            if (tt < 0 || tt >= a.T) continue;                                           // the tap reads padding only (uniform)
            __syncthreads();
            for (int idx = tid; idx < 64 * WG_TH * 32; idx += 256) {
                const int p = idx & 31, r = (idx >> 5) % WG_TH, c = idx / (32 * WG_TH);
                const int co = cob * 64 + c, row = h0 + r, col = w0 + p;
                T v = (T)0.f;
                if (co < a.Cout && row < a.H && col < a.W) v = zg[b * a.zsb + (i64)co * a.zsc + (i64)t * a.zst + (i64)row * a.W + col];
                zl[c * ZCS + r * 32 + p] = v;
            }
            for (int idx = tid; idx < 64 * XR * XWP; idx += 256) {
                const int p = idx % XWP, r = (idx / XWP) % XR, c = idx / (XWP * XR);
                const int ci = cib * 64 + c, row = h0 + r - PS, col = w0 + p - PS;
                T v = (T)0.f;
                if (p < XW && ci < a.Cin && row >= 0 && row < a.H && col >= 0 && col < a.W)
                    v = xg[b * a.xsb + (i64)ci * a.xsc + (i64)tt * a.xst + (i64)row * a.W + col];
                xl[c * XCS + r * XWP + p] = v;
            }
            __syncthreads();
            if (!wave_on) continue;
#pragma unroll
            for (int s = 0; s < WG_TH * 2; ++s) {                                        // 16 pixels per MFMA step
                const int r = s >> 1, pb = 16 * (s & 1) + 8 * kg;
                frag_t af;
                const T* zp = &zl[(mb * 32 + l32) * ZCS + r * 32 + pb];
#pragma unroll
                for (int j = 0; j < 8; ++j) put(af, j, zp[j]);
#pragma unroll
                for (int ky = 0; ky < KS; ++ky) {
                    const T* xp = &xl[(nb * 32 + l32) * XCS + (r + ky) * XWP + pb];
                    T v[8 + KS - 1];
#pragma unroll
                    for (int j = 0; j < 8 + KS - 1; ++j) v[j] = xp[j];
#pragma unroll
                    for (int kx = 0; kx < KS; ++kx) {
                        frag_t bf;
#pragma unroll
                        for (int j = 0; j < 8; ++j) put(bf, j, v[kx + j]);
                        mma(acc[ky][kx], af, bf);
                    }
                }
            }
        }
        if (wave_on) {
            const int ci = cib * 64 + nb * 32 + l32;
#pragma unroll
            for (int ky = 0; ky < KS; ++ky)
#pragma unroll
                for (int kx = 0; kx < KS; ++kx)
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int co = cob * 64 + mb * 32 + 8 * (i >> 2) + 4 * kg + (i & 3);
                        if (co < a.Cout && ci < a.Cin) mine[((i64)co * a.Cin + ci) * NT + (f * KS + ky) * KS + kx] = acc[ky][kx][i];
                    }
        }
    }
}

// db partials: workgroup (co, part) adds the planes part, part + parts, ... of channel co; the fixed tree of reduce.h (tree_sum256) inside the workgroup
template <typename T>
__global__ __launch_bounds__(256) void conv3d_dbias_kernel(const T* __restrict__ dz, float* __restrict__ partial, int Cout, int Tn, i64 planes,
                                                           i64 HW, i64 zsb, i64 zsc, i64 zst) {
    __shared__ float red[256];
    const int co = blockIdx.x, part = blockIdx.y;
    float s = 0.f;
    for (i64 pl = part; pl < planes; pl += gridDim.y) {
        const T* p = dz + (pl / Tn) * zsb + (i64)co * zsc + (pl % Tn) * zst;
        for (i64 i = threadIdx.x; i < HW; i += 256) s += to_f(p[i]);
    }
    red[threadIdx.x] = s;                                           // spelled out: profiles/reduce_header_isa.md
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(i64)part * Cout + co] = red[0];
}

// the partial sets added in workgroup order; a thread per entry
__global__ __launch_bounds__(256) void conv3d_reduce_kernel(const float* __restrict__ partial, int parts, i64 E, float* __restrict__ out) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    float s = 0.f;
    for (int g = 0; g < parts; ++g) s += partial[(i64)g * E + e];
    out[e] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
inline bool misaligned(const void* p, size_t al) { return (reinterpret_cast<uintptr_t>(p) & (al - 1)) != 0; }
inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }
inline void taps_of(int taps, int* kt, int* ks) {
    *kt = taps == VSR_CONV3D_133 ? 1 : 3;
    *ks = taps == VSR_CONV3D_311 ? 1 : 3;
}

// one past the largest element offset of a (B, C, T, plane) operand, or -1 where it passes 2^62
inline i64 span(int B, int C, int T, i64 plane, const long long* s) {
    i64 tot = plane, v;
    const i64 n[3] = {B - 1, C - 1, T - 1};
    for (int i = 0; i < 3; ++i)
        if (__builtin_mul_overflow(n[i], (i64)s[i], &v) || __builtin_add_overflow(tot, v, &tot)) return -1;
    return tot > (1ll << 62) ? -1 : tot;
}

struct Plan {
    int kt, ks, nt, cy;                 // cy: channels of y as stored (Cout, or Cout / 4 with the shuffle)
    i64 fwd_tiles, wg_tiles, E;
    int wg_parts, db_parts;
    bool need_dz;
    size_t pack_fwd, pack_bwd, dz_bytes, wg_bytes, db_bytes;
};

int plan_of(const VsrConv3dDesc* d, Plan* p) {
    if (!d) return VSR_ERR_BADARG;
    if (d->B < 1 || d->Cin < 1 || d->Cout < 1 || d->T < 1 || d->H < 1 || d->W < 1 || bad_dtype(d->dtype)) return VSR_ERR_BADARG;
    if (d->taps != VSR_CONV3D_133 && d->taps != VSR_CONV3D_311 && d->taps != VSR_CONV3D_333) return VSR_ERR_BADARG;
    if (d->act != VSR_CONV3D_ACT_NONE && d->act != VSR_CONV3D_ACT_LEAKY) return VSR_ERR_BADARG;
    if (d->pixel_shuffle != 0 && d->pixel_shuffle != 2) return VSR_ERR_BADARG;
    for (int i = 0; i < 3; ++i)
        if (d->x_stride[i] < 0 || d->y_stride[i] < 0) return VSR_ERR_BADARG;
    if (d->Cin > VSR_CONV3D_MAX_C || d->Cout > VSR_CONV3D_MAX_C) return VSR_ERR_UNSUPPORTED;
    if (d->pixel_shuffle && (d->Cout & 3)) return VSR_ERR_UNSUPPORTED;
    if (d->act == VSR_CONV3D_ACT_LEAKY && !(d->slope > 0.f)) return VSR_ERR_UNSUPPORTED;      // the backward reads the sign off y
    taps_of(d->taps, &p->kt, &p->ks);
    p->nt = p->kt * p->ks * p->ks;
    p->cy = d->pixel_shuffle ? d->Cout / 4 : d->Cout;
    const i64 plane = (i64)d->H * d->W;
    if (span(d->B, d->Cin, d->T, plane, d->x_stride) < 0 || span(d->B, p->cy, d->T, d->pixel_shuffle ? 4 * plane : plane, d->y_stride) < 0)
        return VSR_ERR_UNSUPPORTED;
    i64 bt, el;
    if (__builtin_mul_overflow((i64)d->B, (i64)d->T, &bt) || __builtin_mul_overflow(bt, plane, &el) ||
        __builtin_mul_overflow(el, (i64)VSR_CONV3D_MAX_C * 4, &el))
        return VSR_ERR_UNSUPPORTED;
    p->fwd_tiles = bt * cdiv(d->H, TILE_H) * cdiv(d->W, 32);
    p->wg_tiles = bt * cdiv(d->H, WG_TH) * cdiv(d->W, 32);
    if (p->fwd_tiles > 0x7fffffffLL || p->wg_tiles > (1ll << 40)) return VSR_ERR_UNSUPPORTED;
    p->E = (i64)d->Cout * d->Cin * p->nt;
    i64 parts = WG_MAX_BYTES / (p->E * 4);
    parts = parts < 1 ? 1 : (parts > WG_MAX_PARTS ? WG_MAX_PARTS : parts);
    p->wg_parts = (int)(p->wg_tiles < parts ? p->wg_tiles : parts);
    p->db_parts = (int)(bt < DB_PARTS ? bt : DB_PARTS);
    p->need_dz = d->act != VSR_CONV3D_ACT_NONE || d->pixel_shuffle != 0;
    const size_t es = esize(d->dtype);
    const size_t np = d->dtype == VSR_BF16 ? 2 : 1;                                       // hi + lo
    p->pack_fwd = up256((size_t)cdiv(d->Cout, 64) * cdiv(d->Cin, 16) * p->nt * np * 2 * 64 * 8 * es);
    p->pack_bwd = up256((size_t)cdiv(d->Cin, 64) * cdiv(d->Cout, 16) * p->nt * np * 2 * 64 * 8 * es);
    p->dz_bytes = p->need_dz ? up256((size_t)bt * plane * d->Cout * es) : 0;
    p->wg_bytes = up256((size_t)p->wg_parts * p->E * 4);
    p->db_bytes = up256((size_t)p->db_parts * d->Cout * 4);
    return VSR_OK;
}

template <typename T>
void pack_launch(const float* w, void* out, int M, int K, int nt, bool transposed, hipStream_t st) {
    const int nkc = cdiv(K, 16), total = cdiv(M, 64) * nkc * nt * 2 * 64;
    hipLaunchKernelGGL((conv3d_pack_kernel<T>), dim3(cdiv(total, 256)), dim3(256), 0, st, w, static_cast<T*>(out), M, K, nt, nkc,
                       transposed ? 1 : 0, total);
}

template <typename T>
void conv_launch(int taps, const CArgs& a, i64 tiles, hipStream_t st) {
    const dim3 grid((unsigned)tiles, (unsigned)cdiv(a.Cout, 64)), block(256);
    if (taps == VSR_CONV3D_133) hipLaunchKernelGGL((conv3d_kernel<T, 1, 3>), grid, block, 0, st, a);
    else if (taps == VSR_CONV3D_311) hipLaunchKernelGGL((conv3d_kernel<T, 3, 1>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((conv3d_kernel<T, 3, 3>), grid, block, 0, st, a);
}

template <typename T>
void fwd_run(const VsrConv3dDesc* d, const Plan& p, const void* x, const float* w, const float* b, void* y, void* ws, hipStream_t st) {
    pack_launch<T>(w, ws, d->Cout, d->Cin, p.nt, false, st);
    CArgs a = {};
    a.in = x; a.out = y; a.wpack = ws; a.bias = b;
    a.isb = d->x_stride[0]; a.isc = d->x_stride[1]; a.ist = d->x_stride[2];
    a.osb = d->y_stride[0]; a.osc = d->y_stride[1]; a.ost = d->y_stride[2];
    a.Cin = d->Cin; a.Cout = d->Cout; a.T = d->T; a.H = d->H; a.W = d->W;
    a.tiles_h = cdiv(d->H, TILE_H); a.tiles_w = cdiv(d->W, 32); a.nkc = cdiv(d->Cin, 16);
    a.act = d->act; a.slope = d->slope; a.shuffle = d->pixel_shuffle;
    conv_launch<T>(d->taps, a, p.fwd_tiles, st);
}

template <typename T>
void bwd_run(const VsrConv3dDesc* d, const Plan& p, const void* x, const float* w, const void* y, const void* dy, void* dx, float* dw, float* db,
             char* ws, hipStream_t st) {
    char* pack = ws;
    char* dzbuf = pack + p.pack_bwd;
    float* wg_part = reinterpret_cast<float*>(dzbuf + p.dz_bytes);
    float* db_part = reinterpret_cast<float*>(reinterpret_cast<char*>(wg_part) + p.wg_bytes);
    const i64 plane = (i64)d->H * d->W;
    const void* dz = dy;
    i64 zsb = d->y_stride[0], zsc = d->y_stride[1], zst = d->y_stride[2];
    if (p.need_dz) {
        zsc = (i64)d->T * plane; zst = plane; zsb = zsc * d->Cout;
        const i64 total = zsb * d->B;
        hipLaunchKernelGGL((conv3d_dz_kernel<T>), dim3(grid_for(total)), dim3(256), 0, st, static_cast<const T*>(y), static_cast<const T*>(dy),
                           reinterpret_cast<T*>(dzbuf), total, d->Cout, d->T, d->H, d->W, (i64)d->y_stride[0], (i64)d->y_stride[1],
                           (i64)d->y_stride[2], d->act, d->slope, d->pixel_shuffle);
        dz = dzbuf;
    }
    if (dx) {                                                                            // the forward kernel on flipped, transposed weights
        pack_launch<T>(w, pack, d->Cin, d->Cout, p.nt, true, st);
        CArgs a = {};
        a.in = dz; a.out = dx; a.wpack = pack;
        a.isb = zsb; a.isc = zsc; a.ist = zst;
        a.osb = d->x_stride[0]; a.osc = d->x_stride[1]; a.ost = d->x_stride[2];
        a.Cin = d->Cout; a.Cout = d->Cin; a.T = d->T; a.H = d->H; a.W = d->W;
        a.tiles_h = cdiv(d->H, TILE_H); a.tiles_w = cdiv(d->W, 32); a.nkc = cdiv(d->Cout, 16);
        conv_launch<T>(d->taps, a, p.fwd_tiles, st);
    }
    if (dw) {
        WArgs a = {};
        a.x = x; a.dz = dz; a.partial = wg_part;
        a.xsb = d->x_stride[0]; a.xsc = d->x_stride[1]; a.xst = d->x_stride[2];
        a.zsb = zsb; a.zsc = zsc; a.zst = zst;
        a.tiles = p.wg_tiles; a.E = p.E;
        a.Cin = d->Cin; a.Cout = d->Cout; a.T = d->T; a.H = d->H; a.W = d->W; a.KT = p.kt;
        a.tiles_h = cdiv(d->H, WG_TH); a.tiles_w = cdiv(d->W, 32); a.ncib = cdiv(d->Cin, 64);
        const dim3 grid((unsigned)p.wg_parts, (unsigned)(cdiv(d->Cout, 64) * a.ncib)), block(256);
        if (p.ks == 3) hipLaunchKernelGGL((conv3d_wgrad_kernel<T, 3>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((conv3d_wgrad_kernel<T, 1>), grid, block, 0, st, a);
        hipLaunchKernelGGL(conv3d_reduce_kernel, dim3((unsigned)((p.E + 255) / 256)), dim3(256), 0, st, wg_part, p.wg_parts, p.E, dw);
    }
    if (db) {
        hipLaunchKernelGGL((conv3d_dbias_kernel<T>), dim3(d->Cout, p.db_parts), dim3(256), 0, st, static_cast<const T*>(dz), db_part, d->Cout,
                           d->T, (i64)d->B * d->T, plane, zsb, zsc, zst);
        hipLaunchKernelGGL(conv3d_reduce_kernel, dim3(cdiv(d->Cout, 256)), dim3(256), 0, st, db_part, p.db_parts, (i64)d->Cout, db);
    }
}

inline size_t bwd_bytes(const Plan& p) { return p.pack_bwd + p.dz_bytes + p.wg_bytes + p.db_bytes; }

}  // namespace

extern "C" {

size_t vsr_conv3d_workspace_bytes(const VsrConv3dDesc* desc, int need_backward) {
    Plan p;
    if (plan_of(desc, &p) != VSR_OK) return 0;
    return need_backward ? bwd_bytes(p) : p.pack_fwd;
}

int vsr_conv3d_fwd(const VsrConv3dDesc* d, const void* x, const float* w, const float* b, void* y, void* workspace, size_t workspace_bytes,
                   void* stream) {
    if (!d || !x || !w || !y || !workspace) return VSR_ERR_BADARG;
    Plan p;
    CK(plan_of(d, &p));
    if (misaligned(x, esize(d->dtype)) || misaligned(y, esize(d->dtype)) || misaligned(w, 4) || misaligned(b, 4) || misaligned(workspace, 256))
        return VSR_ERR_BADARG;
    if (workspace_bytes < p.pack_fwd) return VSR_ERR_WORKSPACE;
    if (d->dtype == VSR_BF16) fwd_run<bf16_t>(d, p, x, w, b, y, workspace, (hipStream_t)stream);
    else fwd_run<float>(d, p, x, w, b, y, workspace, (hipStream_t)stream);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_conv3d_bwd(const VsrConv3dDesc* d, const void* x, const float* w, const void* y, const void* dy, void* dx, float* dw, float* db,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !x || !w || !dy || !workspace) return VSR_ERR_BADARG;
    Plan p;
    CK(plan_of(d, &p));
    if (d->act != VSR_CONV3D_ACT_NONE && !y) return VSR_ERR_BADARG;
    const size_t es = esize(d->dtype);
    if (misaligned(x, es) || misaligned(y, es) || misaligned(dy, es) || misaligned(dx, es) || misaligned(w, 4) || misaligned(dw, 4) ||
        misaligned(db, 4) || misaligned(workspace, 256))
        return VSR_ERR_BADARG;
    if (workspace_bytes < bwd_bytes(p)) return VSR_ERR_WORKSPACE;
    if (d->dtype == VSR_BF16) bwd_run<bf16_t>(d, p, x, w, y, dy, dx, dw, db, static_cast<char*>(workspace), (hipStream_t)stream);
    else bwd_run<float>(d, p, x, w, y, dy, dx, dw, db, static_cast<char*>(workspace), (hipStream_t)stream);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
