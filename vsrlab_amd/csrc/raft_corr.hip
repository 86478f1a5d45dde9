// RAFT's correlation lookup (optical_flow/models/raft/corr.py) without the all-pairs volume, forward and backward.  DESIGN
// section 11e.
//
// The reference forms corr[p][q] = <fmap1[p], fmap2[q]> / sqrt(D) for every pixel pair, pools it three times over q with
// avg_pool2d(2, 2) and reads 7 x 7 bilinear windows out of the four volumes.  Pooling is linear and acts on q alone, so level l
// of the volume is <fmap1[p], avgpool^l(fmap2)[q]> / sqrt(D): the same numbers come from pooling fmap2 and taking the dot
// products a window needs when it is read.
//
// Layout.  fmap1 and every level of fmap2 are packed pixel-major, [N][H_l * W_l][D] of T (bf16 or fp32), D = 128 values of a
// pixel contiguous; level l is the 2 x 2 mean (floor sizes) of the stored level l - 1, summed in fp32.
//
// Lookup forward: the 49 taps of a window share one fractional part, so a window is 64 dot products on the 8 x 8 integer grid
// around floor(c) - 3 and a 4-tap combine.  One wave per query, lane = grid point; the query's fmap1 vector comes from LDS
// (one broadcast read per 8 channels serves all levels) and each lane streams its own pixel of every level in 8-channel
// chunks.  A workgroup takes 32 consecutive queries: their windows overlap in cache, and the (channel, pixel) tile of results
// goes through LDS so that the planar output is written in 128-byte runs.
// Lookup backward: the same wave first turns the 49 window cotangents of a level into the 64 grid cotangents dG (lane = grid
// point), then switches to lane = channel (c and c + 64): d fmap1[p] += dG[g] * level[q_g] is a gather with one owner per
// element (bit-identical across runs), d level[q_g] += dG[g] * fmap1[p] is a scatter of 256-byte fp32 atomic rows.
// Both go into pixel-major fp32 accumulators that every lookup of one pyramid adds to; the pyramid backward un-pools the
// level accumulators into level 0 and unpacks to planar once.
//
// Coordinates are clamped in float to [-8, size + 7] before floor(): a window that far out has no tap inside either way, and
// no huge or non-finite coordinate reaches an integer conversion or an address.
#include "elt.h"
#include "cl_stage.h"
#include "host.h"

namespace {

constexpr int RC_D = 128;               // feature channels
constexpr int RC_R = 3;                 // window radius
constexpr int RC_TAPS = 49;
constexpr int RC_MAXL = 4;
constexpr int RC_QT = 32;               // queries per workgroup

struct RaftArgs {
    const void* f1;                     // packed fmap1
    const void* lev[RC_MAXL];           // packed levels of fmap2
    int Hl[RC_MAXL], Wl[RC_MAXL];
    const float* coords;                // (N, 2, H, W), channel 0 = x
    float* out;                         // (N, L * 49, H, W)
    const float* dout;
    float* g1;                          // fp32 accumulators, pixel-major
    float* glev[RC_MAXL];
    int N, H, W, L;
    float scale;
};

struct Win { int x0, y0; float ax, ay; };

// the window of centre c / 2^l at a level of size (Hl, Wl): grid origin floor(c) - 3 and the fractional part
__device__ __forceinline__ Win window(float cx, float cy, int l, int Hl, int Wl) {
    const float s = 1.f / (float)(1 << l);
    cx *= s; cy *= s;
    if (!(cx >= -8.f)) cx = -8.f;                          // also what a NaN becomes
    if (!(cx <= (float)Wl + 7.f)) cx = (float)Wl + 7.f;
    if (!(cy >= -8.f)) cy = -8.f;
    if (!(cy <= (float)Hl + 7.f)) cy = (float)Hl + 7.f;
    const float fx = floorf(cx), fy = floorf(cy);
    Win w;
    w.x0 = (int)fx - RC_R; w.y0 = (int)fy - RC_R;
    w.ax = cx - fx; w.ay = cy - fy;
    return w;
}

// ---- lookup forward ---------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void raft_lookup_fwd_kernel(RaftArgs a) {
    __shared__ __attribute__((aligned(16))) float f1s[RC_QT][RC_D];
    __shared__ float outs[RC_MAXL * RC_TAPS][RC_QT + 1];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long HW = (long long)a.H * a.W, total = (long long)a.N * HW;
    const long long p0 = (long long)blockIdx.x * RC_QT;
    const T* f1 = reinterpret_cast<const T*>(a.f1);
    for (int i = t; i < RC_QT * RC_D / 8; i += 256) {
        const long long p = p0 + i / (RC_D / 8);
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (p < total) ld8<T>(f1 + p * RC_D + (i % (RC_D / 8)) * 8, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) f1s[i / (RC_D / 8)][(i % (RC_D / 8)) * 8 + e] = v[e];
    }
    __syncthreads();
    const int gx = lane & 7, gy = lane >> 3;
    for (int qi = wave; qi < RC_QT; qi += 4) {
        const long long p = p0 + qi;
        if (p >= total) break;
        const long long n = p / HW, pix = p % HW;
        const float cx = a.coords[(n * 2) * HW + pix], cy = a.coords[(n * 2 + 1) * HW + pix];
        Win w[RC_MAXL];
        const T* src[RC_MAXL];
        bool ok[RC_MAXL];
        float acc[RC_MAXL];
#pragma unroll
        for (int l = 0; l < RC_MAXL; ++l) {
            acc[l] = 0.f; ok[l] = false; src[l] = nullptr;
            if (l < a.L) {
                const int Hl = a.Hl[l], Wl = a.Wl[l];
                w[l] = window(cx, cy, l, Hl, Wl);
                const int x = w[l].x0 + gx, y = w[l].y0 + gy;
                ok[l] = x >= 0 && x < Wl && y >= 0 && y < Hl;
                // a grid point outside reads pixel 0 of its image and is dropped below
                src[l] = reinterpret_cast<const T*>(a.lev[l]) + (n * Hl * Wl + (ok[l] ? y * Wl + x : 0)) * RC_D;
            }
        }
        for (int c = 0; c < RC_D; c += 8) {
            const float4 fa = *reinterpret_cast<const float4*>(&f1s[qi][c]), fb = *reinterpret_cast<const float4*>(&f1s[qi][c + 4]);
#pragma unroll
            for (int l = 0; l < RC_MAXL; ++l)
                if (l < a.L) {
                    float v[8];
                    ld8<T>(src[l] + c, v);
                    float s = acc[l];
                    s = fmaf(fa.x, v[0], s); s = fmaf(fa.y, v[1], s); s = fmaf(fa.z, v[2], s); s = fmaf(fa.w, v[3], s);
                    s = fmaf(fb.x, v[4], s); s = fmaf(fb.y, v[5], s); s = fmaf(fb.z, v[6], s); s = fmaf(fb.w, v[7], s);
                    acc[l] = s;
                }
        }
#pragma unroll
        for (int l = 0; l < RC_MAXL; ++l)
            if (l < a.L) {
                const float g = ok[l] ? acc[l] : 0.f;
                const float g01 = __shfl_down(g, 1), g10 = __shfl_down(g, 8), g11 = __shfl_down(g, 9);
                if (gx < 7 && gy < 7) {         // tap i = gx offsets x, tap j = gy offsets y: channel l * 49 + i * 7 + j
                    const float ax = w[l].ax, ay = w[l].ay;
                    const float v = (1.f - ay) * ((1.f - ax) * g + ax * g01) + ay * ((1.f - ax) * g10 + ax * g11);
                    outs[l * RC_TAPS + gx * 7 + gy][qi] = v * a.scale;
                }
            }
    }
    __syncthreads();
    const int C = a.L * RC_TAPS;
    for (int i = t; i < C * RC_QT; i += 256) {
        const int ch = i / RC_QT, qi = i % RC_QT;
        const long long p = p0 + qi;
        if (p < total) a.out[((p / HW) * C + ch) * HW + p % HW] = outs[ch][qi];
    }
}

// ---- lookup backward --------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void raft_lookup_bwd_kernel(RaftArgs a) {
    __shared__ float douts[RC_MAXL * RC_TAPS][RC_QT + 1];
    __shared__ float dgs[4][RC_MAXL][64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const long long HW = (long long)a.H * a.W, total = (long long)a.N * HW;
    const long long p0 = (long long)blockIdx.x * RC_QT;
    const int C = a.L * RC_TAPS;
    for (int i = t; i < C * RC_QT; i += 256) {
        const int ch = i / RC_QT, qi = i % RC_QT;
        const long long p = p0 + qi;
        douts[ch][qi] = p < total ? a.dout[((p / HW) * C + ch) * HW + p % HW] * a.scale : 0.f;
    }
    __syncthreads();
    const int gx = lane & 7, gy = lane >> 3;
    const T* f1 = reinterpret_cast<const T*>(a.f1);
    for (int it = 0; it < RC_QT / 4; ++it) {                // the same trip count in every wave: barriers inside
        const int qi = it * 4 + wave;
        const long long p = p0 + qi;
        const bool live = p < total;                        // wave-uniform
        const long long n = live ? p / HW : 0, pix = live ? p % HW : 0;
        Win w[RC_MAXL];
        if (live) {
            const float cx = a.coords[(n * 2) * HW + pix], cy = a.coords[(n * 2 + 1) * HW + pix];
#pragma unroll
            for (int l = 0; l < RC_MAXL; ++l)
                if (l < a.L) {
                    const int Hl = a.Hl[l], Wl = a.Wl[l];
                    w[l] = window(cx, cy, l, Hl, Wl);
                    const int x = w[l].x0 + gx, y = w[l].y0 + gy;
                    const bool ok = x >= 0 && x < Wl && y >= 0 && y < Hl;
                    const float ax = w[l].ax, ay = w[l].ay;
                    const float d = (gx < 7 && gy < 7) ? douts[l * RC_TAPS + gx * 7 + gy][qi] : 0.f;
                    const float d01 = __shfl_up(d, 1), d10 = __shfl_up(d, 8), d11 = __shfl_up(d, 9);
                    float g = (1.f - ay) * (1.f - ax) * d;
                    if (gx > 0) g += (1.f - ay) * ax * d01;
                    if (gy > 0) g += ay * (1.f - ax) * d10;
                    if (gx > 0 && gy > 0) g += ay * ax * d11;
                    dgs[wave][l][lane] = ok ? g : 0.f;      // 0 marks "skip": no address is formed from a point outside
                }
        }
        __syncthreads();
        if (live) {
            const float fa = to_f(f1[p * RC_D + lane]), fb = to_f(f1[p * RC_D + 64 + lane]);
            float sa = 0.f, sb = 0.f;
#pragma unroll
            for (int l = 0; l < RC_MAXL; ++l)
                if (l < a.L) {
                    const int Hl = a.Hl[l], Wl = a.Wl[l];
                    const int x0 = __builtin_amdgcn_readfirstlane(w[l].x0), y0 = __builtin_amdgcn_readfirstlane(w[l].y0);
                    const long long base = n * Hl * Wl;
                    const T* lv = reinterpret_cast<const T*>(a.lev[l]);
                    for (int g = 0; g < 64; ++g) {
                        const float dg = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(dgs[wave][l][g])));
                        if (dg != 0.f) {
                            const long long q = (base + (long long)(y0 + (g >> 3)) * Wl + (x0 + (g & 7))) * RC_D;
                            sa = fmaf(dg, to_f(lv[q + lane]), sa);
                            sb = fmaf(dg, to_f(lv[q + 64 + lane]), sb);
                            unsafeAtomicAdd(a.glev[l] + q + lane, dg * fa);
                            unsafeAtomicAdd(a.glev[l] + q + 64 + lane, dg * fb);
                        }
                    }
                }
            a.g1[p * RC_D + lane] += sa;                    // one owner per element and launch
            a.g1[p * RC_D + 64 + lane] += sb;
        }
        __syncthreads();
    }
}

// ---- pool and its adjoint (pack and unpack: cl_stage.h in full RC_D-channel rows) ------------------------------------
// level (N, Hf, Wf) -> its 2 x 2 mean (N, Hc, Wc), Hc = Hf / 2, Wc = Wf / 2: one thread per pixel and 8-channel chunk
template <typename T>
__global__ __launch_bounds__(256) void raft_pool_kernel(const T* fine, T* coarse, int Hf, int Wf, int Hc, int Wc, long long chunks) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= chunks) return;
    const int c = (int)(idx % (RC_D / 8)) * 8;
    const long long pc = idx / (RC_D / 8), n = pc / ((long long)Hc * Wc);
    const int r = (int)(pc % ((long long)Hc * Wc)), y = r / Wc, x = r % Wc;
    const T* s = fine + ((n * Hf + 2 * y) * Wf + 2 * x) * RC_D + c;
    float v00[8], v01[8], v10[8], v11[8], o[8];
    ld8<T>(s, v00); ld8<T>(s + RC_D, v01); ld8<T>(s + (long long)Wf * RC_D, v10); ld8<T>(s + (long long)(Wf + 1) * RC_D, v11);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = ((v00[e] + v01[e]) + (v10[e] + v11[e])) * 0.25f;
    st8<T>(coarse + pc * RC_D + c, o);
}
// its adjoint, accumulated: fine += coarse[y / 2][x / 2] / 4 where that pixel exists (fp32 accumulators)
__global__ __launch_bounds__(256) void raft_unpool_kernel(float* fine, const float* coarse, int Hf, int Wf, int Hc, int Wc, long long quads) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= quads) return;
    const int c = (int)(idx % (RC_D / 4)) * 4;
    const long long pf = idx / (RC_D / 4), n = pf / ((long long)Hf * Wf);
    const int r = (int)(pf % ((long long)Hf * Wf)), y = r / Wf, x = r % Wf;
    if ((y >> 1) >= Hc || (x >> 1) >= Wc) return;
    const float4 g = *reinterpret_cast<const float4*>(coarse + ((n * Hc + (y >> 1)) * Wc + (x >> 1)) * RC_D + c);
    float4* d = reinterpret_cast<float4*>(fine + pf * RC_D + c);
    float4 v = *d;
    v.x += 0.25f * g.x; v.y += 0.25f * g.y; v.z += 0.25f * g.z; v.w += 0.25f * g.w;
    *d = v;
}

// ---- host -------------------------------------------------------------------------------------------------------------
struct RaftPlan {
    int Hl[RC_MAXL], Wl[RC_MAXL];
    size_t f1, lev[RC_MAXL], total;     // offsets into the packed maps (es = element size) or the accumulators (es = 4)
};

int raft_plan(const VsrRaftCorrDesc* d, size_t es, RaftPlan& pl) {
    if (!d || bad_dims(d->N, d->H, d->W) || d->D < 1 || d->levels < 1 || d->radius < 0 || bad_dtype(d->dtype)) return VSR_ERR_BADARG;
    if (d->D != RC_D || d->radius != RC_R || d->levels > RC_MAXL) return VSR_ERR_UNSUPPORTED;
    if ((d->H >> (d->levels - 1)) < 2 || (d->W >> (d->levels - 1)) < 2) return VSR_ERR_UNSUPPORTED;   // a 1-wide level: 0 / 0 in the reference
    if ((long long)d->H * d->W > (1ll << 24) || (long long)d->N * d->H * d->W > (1ll << 28) || d->N > 65535) return VSR_ERR_UNSUPPORTED;
    Bump b;
    pl.f1 = b.take((size_t)d->N * d->H * d->W * RC_D * es);
    for (int l = 0; l < RC_MAXL; ++l) {
        pl.Hl[l] = d->H >> l; pl.Wl[l] = d->W >> l; pl.lev[l] = 0;
        if (l < d->levels) pl.lev[l] = b.take((size_t)d->N * pl.Hl[l] * pl.Wl[l] * RC_D * es);
    }
    pl.total = b.off;
    return VSR_OK;
}

RaftArgs raft_args(const VsrRaftCorrDesc* d, const RaftPlan& pk, const void* packed, const RaftPlan* ga, void* gacc) {
    RaftArgs a = {};
    const char* pb = reinterpret_cast<const char*>(packed);
    char* gb = reinterpret_cast<char*>(gacc);
    a.f1 = pb + pk.f1;
    if (ga) a.g1 = reinterpret_cast<float*>(gb + ga->f1);
    for (int l = 0; l < d->levels; ++l) {
        a.lev[l] = pb + pk.lev[l]; a.Hl[l] = pk.Hl[l]; a.Wl[l] = pk.Wl[l];
        if (ga) a.glev[l] = reinterpret_cast<float*>(gb + ga->lev[l]);
    }
    a.N = d->N; a.H = d->H; a.W = d->W; a.L = d->levels;
    a.scale = 1.f / sqrtf((float)d->D);
    return a;
}

template <typename T>
void raft_build(const VsrRaftCorrDesc* d, const RaftPlan& pl, const float* fmap1, const float* fmap2, char* pk, hipStream_t st) {
    cl_pack<RC_D>(st, d->N, RC_D, d->H * d->W, RC_D, ClIdentity{}, fmap1, reinterpret_cast<T*>(pk + pl.f1));
    cl_pack<RC_D>(st, d->N, RC_D, d->H * d->W, RC_D, ClIdentity{}, fmap2, reinterpret_cast<T*>(pk + pl.lev[0]));
    for (int l = 1; l < d->levels; ++l) {
        const long long chunks = (long long)d->N * pl.Hl[l] * pl.Wl[l] * (RC_D / 8);
        hipLaunchKernelGGL(raft_pool_kernel<T>, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, st,
                           reinterpret_cast<const T*>(pk + pl.lev[l - 1]), reinterpret_cast<T*>(pk + pl.lev[l]), pl.Hl[l - 1], pl.Wl[l - 1],
                           pl.Hl[l], pl.Wl[l], chunks);
    }
}

}  // namespace

extern "C" {

size_t vsr_raft_corr_workspace_bytes(const VsrRaftCorrDesc* d, int gradients) {
    RaftPlan pl;
    if (!d) return 0;
    return raft_plan(d, gradients ? 4 : esize(d->dtype), pl) == VSR_OK ? pl.total : 0;
}

int vsr_raft_corr_pyramid_fwd(const VsrRaftCorrDesc* d, const float* fmap1, const float* fmap2, void* packed, size_t packed_bytes,
                              void* stream) {
    RaftPlan pl;
    if (!d) return VSR_ERR_BADARG;
    CK(raft_plan(d, esize(d->dtype), pl));
    if (!fmap1 || !fmap2 || !packed) return VSR_ERR_BADARG;
    if (packed_bytes < pl.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (d->dtype == VSR_BF16) raft_build<bf16_t>(d, pl, fmap1, fmap2, reinterpret_cast<char*>(packed), st);
    else raft_build<float>(d, pl, fmap1, fmap2, reinterpret_cast<char*>(packed), st);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_raft_corr_pyramid_bwd(const VsrRaftCorrDesc* d, void* gacc, size_t gacc_bytes, float* dfmap1, float* dfmap2, void* stream) {
    RaftPlan ga;
    if (!d) return VSR_ERR_BADARG;
    CK(raft_plan(d, 4, ga));
    if (!gacc) return VSR_ERR_BADARG;
    if (gacc_bytes < ga.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* gb = reinterpret_cast<char*>(gacc);
    if (dfmap1) cl_unpack<RC_D>(st, d->N, RC_D, d->H * d->W, RC_D, ClIdentity{}, reinterpret_cast<const float*>(gb + ga.f1), dfmap1);
    if (dfmap2) {
        for (int l = d->levels - 1; l >= 1; --l) {
            const long long quads = (long long)d->N * ga.Hl[l - 1] * ga.Wl[l - 1] * (RC_D / 4);
            hipLaunchKernelGGL(raft_unpool_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st,
                               reinterpret_cast<float*>(gb + ga.lev[l - 1]), reinterpret_cast<const float*>(gb + ga.lev[l]), ga.Hl[l - 1],
                               ga.Wl[l - 1], ga.Hl[l], ga.Wl[l], quads);
        }
        cl_unpack<RC_D>(st, d->N, RC_D, d->H * d->W, RC_D, ClIdentity{}, reinterpret_cast<const float*>(gb + ga.lev[0]), dfmap2);
    }
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_raft_corr_lookup_fwd(const VsrRaftCorrDesc* d, const void* packed, size_t packed_bytes, const float* coords, float* out,
                             void* stream) {
    RaftPlan pl;
    if (!d) return VSR_ERR_BADARG;
    CK(raft_plan(d, esize(d->dtype), pl));
    if (!packed || !coords || !out) return VSR_ERR_BADARG;
    if (packed_bytes < pl.total) return VSR_ERR_WORKSPACE;
    RaftArgs a = raft_args(d, pl, packed, nullptr, nullptr);
    a.coords = coords; a.out = out;
    const unsigned grid = (unsigned)(((long long)d->N * d->H * d->W + RC_QT - 1) / RC_QT);
    if (d->dtype == VSR_BF16) hipLaunchKernelGGL(raft_lookup_fwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(raft_lookup_fwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_raft_corr_lookup_bwd(const VsrRaftCorrDesc* d, const void* packed, size_t packed_bytes, const float* coords, const float* dout,
                             void* gacc, size_t gacc_bytes, void* stream) {
    RaftPlan pl, ga;
    if (!d) return VSR_ERR_BADARG;
    CK(raft_plan(d, esize(d->dtype), pl));
    CK(raft_plan(d, 4, ga));
    if (!packed || !coords || !dout || !gacc) return VSR_ERR_BADARG;
    if (packed_bytes < pl.total || gacc_bytes < ga.total) return VSR_ERR_WORKSPACE;
    RaftArgs a = raft_args(d, pl, packed, &ga, gacc);
    a.coords = coords; a.dout = dout;
    const unsigned grid = (unsigned)(((long long)d->N * d->H * d->W + RC_QT - 1) / RC_QT);
    if (d->dtype == VSR_BF16) hipLaunchKernelGGL(raft_lookup_bwd_kernel<bf16_t>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(raft_lookup_bwd_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
