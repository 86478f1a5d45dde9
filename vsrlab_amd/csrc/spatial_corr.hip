// The local correlation of core/modules/correlation.py (SpatialCorrelationSampler) and PWC's cost volume
// (optical_flow/models/irr/pwc_modules.py compute_cost_volume), forward and both gradients.  DESIGN section 11f.
// Built into a library of its own, libvsrlab_spatial_corr.so (include/vsrlab_spatial_corr.h): libvsrlab_hip.so's exports stay as they are.
//
//   out[n][i][j][y][x] = scale * sum_c in1[n][c][y s_h][x s_w] * in2[n][c][y s_h + i d_h - m_h][x s_w + j d_w - m_w]
//
// in the frame padded by `padding` (H' x W'), in2 zero outside it, m = d (P - 1) / 2.  The reference evaluates one displacement
// per pass over both maps; here one launch reads each map once.
//
// Layout.  Both maps are re-laid pixel-major, [N][H][W][Cp] of T (bf16 or fp32), Cp = C rounded up to 8 with zeros, in the
// UNPADDED frame: the padding zeros and the displacement halo are bounds tests when a tile is staged, never memory.  A staged
// pixel is one 16-byte chunk (4 fp32 or 8 bf16 channels), so every LDS access is a ds_read_b128 / ds_write_b128.
//
// Forward: a workgroup owns 8 x 32 output pixels, one lane each.  Per channel chunk it stages the haloed tile of in2 those pixels
// reach ((7 s_h + (P_h - 1) d_h + 1) rows) in LDS; a lane keeps its own in1 chunk in registers and all P_h P_w sums in
// accumulators, and the next chunk is fetched while this one's taps run.  Plane (i, j) of the output is then written by a wave
// as two 128-byte runs.
// d in1 is the same walk with the roles turned: the lane's P_h P_w cotangents sit in registers, the sum runs over the patch
// and the chunk's channels leave as planar 128-byte runs.  d in2 tiles in2's own pixels: pixel (v, u) gathers, for every (i, j)
// whose (v - i d + m, u - j d + m) is a sampled position, that position's cotangent (registers) times in1 there (staged in LDS).
// All three are gathers: one owner per element, no atomics, bit-identical across runs.
//
// What bounds it: every FMA group takes one ds_read_b128 operand, so fp32 runs at the LDS rate (about half the vector rate) and
// bf16 at the VALU's (FMAs plus the unpack).  DESIGN section 11f has the measurements and what was not built.
//
// No address is formed from a coordinate outside its image: a staged pixel outside carries the index -1 and becomes zeros, a
// lane without an output pixel reads the staged tile only (every staged index is inside the tile by construction) and stores
// nothing.
#include "elt.h"
#include "cl_stage.h"
#include "host.h"
#include "../../include/vsrlab_spatial_corr.h"

namespace {

constexpr int SC_TY = 8, SC_TX = 32;    // pixels per workgroup: outputs (forward, d in1), in2 pixels (d in2)
constexpr int SC_PMAX = 9;              // patch size per axis
constexpr int SC_SMAX = 2, SC_DMAX = 2; // stride, dilation_patch
// the largest staged tiles (stride 2, dilation 2, patch 9), the fixed LDS row pitch and the 256-thread staging slots of each
// tiling: _O by output pixel (forward, d in1), _I by in2 pixel (d in2)
constexpr int SC_RH_O = (SC_TY - 1) * SC_SMAX + (SC_PMAX - 1) * SC_DMAX + 1, SC_PITCH_O = (SC_TX - 1) * SC_SMAX + (SC_PMAX - 1) * SC_DMAX + 1;
constexpr int SC_RH_I = SC_TY + (SC_PMAX - 1) * SC_DMAX, SC_PITCH_I = SC_TX + (SC_PMAX - 1) * SC_DMAX;
constexpr int SC_SLOTS_O = (SC_RH_O * SC_PITCH_O + 255) / 256, SC_SLOTS_I = (SC_RH_I * SC_PITCH_I + 255) / 256;
static_assert(SC_RH_O < 256 && SC_PITCH_O < 256 && SC_RH_I < 256 && SC_PITCH_I < 256, "a staging slot packs (ry, rx) into 8 bits each");

// channels per 16-byte chunk, and the chunk as floats
template <typename T> struct ScChunk;
template <> struct ScChunk<float> { static constexpr int CK = 4; };
template <> struct ScChunk<bf16_t> { static constexpr int CK = 8; };
static __device__ __forceinline__ void chunk_f(const uint4& v, float* f, float*) {
    f[0] = __uint_as_float(v.x); f[1] = __uint_as_float(v.y); f[2] = __uint_as_float(v.z); f[3] = __uint_as_float(v.w);
}
static __device__ __forceinline__ void chunk_f(const uint4& v, float* f, bf16_t*) { unpack8(v, f); }

// The backward kernels multiply a chunk's channels by one cotangent per tap.  The compiler pairs the channels into packed FMAs
// and would keep every cotangent splatted into a register pair across the channel loop (162 registers for 81 taps, and spills
// in the bf16 build); passing the value through here inside the loop keeps one register per cotangent.
static __device__ __forceinline__ float keep_scalar(float v) {
    asm volatile("" : "+v"(v));
    return v;
}

struct ScArgs {
    const void* p1;                     // packed in1, in2
    const void* p2;
    float* out;                         // (N, Ph, Pw, Ho, Wo)
    const float* dout;
    float* din1;                        // (N, C, H, W)
    float* din2;
    int N, C, Cp, H, W;                 // the unpadded frame
    int Ph, Pw, sh, sw, ph, pw, dh, dw, mh, mw;
    int Ho, Wo;
    int tiles_x;
    int RH, RW;                         // the staged tile
    int zsplit;                         // patch rows (forward) or channel chunks (backward) per blockIdx.z
    float scale;
};

// A thread's staging slots: tile pixel (ry, rx) = slot k * 256 + t of the RH x RW tile whose pixel (0, 0) is (ry0, rx0) of the
// unpadded frame, as ry << 8 | rx, bit 16 set where that pixel is inside the image (outside: staged as zeros); -1: no such slot.
template <int SLOTS>
static __device__ __forceinline__ void stage_plan(const ScArgs& a, int ry0, int rx0, int t, int* code) {
    const int total = a.RH * a.RW;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const int i = k * 256 + t;
        code[k] = -1;
        if (i < total) {
            const int ry = i / a.RW, rx = i - ry * a.RW, yy = ry0 + ry, xx = rx0 + rx;
            code[k] = ((yy >= 0 && yy < a.H && xx >= 0 && xx < a.W) ? 1 << 16 : 0) | ry << 8 | rx;
        }
    }
}
// Channels [c, c + CK) of the thread's slots, global memory -> registers -> the tile (rows PITCH pixels apart).  img: image n
// of the packed map.  Two steps, so that the forward can fetch the next chunk while it computes on this one.
template <typename T, int SLOTS>
static __device__ __forceinline__ void stage_load(const ScArgs& a, const T* img, int ry0, int rx0, int c, const int* code, uint4* v) {
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        v[k] = make_uint4(0, 0, 0, 0);
        if (code[k] >= 0 && (code[k] >> 16)) {
            const int ry = (code[k] >> 8) & 0xff, rx = code[k] & 0xff;
            v[k] = *reinterpret_cast<const uint4*>(img + (long long)((ry0 + ry) * a.W + rx0 + rx) * a.Cp + c);
        }
    }
}
template <int SLOTS, int PITCH>
static __device__ __forceinline__ void stage_store(const int* code, const uint4* v, uint4* tile) {
#pragma unroll
    for (int k = 0; k < SLOTS; ++k)
        if (code[k] >= 0) tile[((code[k] >> 8) & 0xff) * PITCH + (code[k] & 0xff)] = v[k];
}

// The kernels are instantiated per patch width and horizontal dilation (PW, DW) and stage their tiles at a fixed pitch: the taps of
// one patch row are the row's LDS address plus compile-time offsets, read back to back in one basic block (a uniform test per tap
// would end the block and leave every ds_read waiting alone).  Patch rows are skipped by a uniform test, P_h and d_h are run-time.

// ---- forward ------------------------------------------------------------------------------------------------------------
template <typename T, int PW, int DW>
__global__ __launch_bounds__(256) void sc_fwd_kernel(ScArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint4 sc_tile[];
    constexpr int CK = ScChunk<T>::CK;
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5, n = blockIdx.y;
    const int y0 = (int)(blockIdx.x / a.tiles_x) * SC_TY, x0 = (int)(blockIdx.x % a.tiles_x) * SC_TX;
    const int y = y0 + ty, x = x0 + tx;
    const bool live = y < a.Ho && x < a.Wo;
    const int y1 = y * a.sh - a.ph, x1 = x * a.sw - a.pw;               // the lane's in1 pixel in the unpadded frame
    const bool has1 = live && y1 >= 0 && y1 < a.H && x1 >= 0 && x1 < a.W;
    const long long img = (long long)n * a.H * a.W;
    const T* p1 = reinterpret_cast<const T*>(a.p1) + (img + (has1 ? y1 * a.W + x1 : 0)) * a.Cp;
    const T* p2 = reinterpret_cast<const T*>(a.p2) + img * a.Cp;
    const int ry0 = y0 * a.sh - a.mh - a.ph, rx0 = x0 * a.sw - a.mw - a.pw;
    int code[SC_SLOTS_O];
    stage_plan<SC_SLOTS_O>(a, ry0, rx0, t, code);
    const uint4* mine = sc_tile + ty * a.sh * SC_PITCH_O + tx * a.sw;
    float acc[SC_PMAX][PW];
#pragma unroll
    for (int i = 0; i < SC_PMAX; ++i)
#pragma unroll
        for (int j = 0; j < PW; ++j) acc[i][j] = 0.f;
    // this workgroup's patch rows (blockIdx.z: a small map is spread over more workgroups, each with the whole tile)
    const int i0 = blockIdx.z * a.zsplit, i1 = min(a.Ph, i0 + a.zsplit);
    uint4 nxt[SC_SLOTS_O], v1n = make_uint4(0, 0, 0, 0);
    stage_load<T, SC_SLOTS_O>(a, p2, ry0, rx0, 0, code, nxt);
    if (has1) v1n = *reinterpret_cast<const uint4*>(p1);
    for (int c = 0; c < a.Cp; c += CK) {
        __syncthreads();
        stage_store<SC_SLOTS_O, SC_PITCH_O>(code, nxt, sc_tile);
        __syncthreads();
        float f1[CK];
        chunk_f(v1n, f1, (T*)nullptr);
        if (c + CK < a.Cp) {                                               // the next chunk is in flight during this one's taps
            stage_load<T, SC_SLOTS_O>(a, p2, ry0, rx0, c + CK, code, nxt);
            if (has1) v1n = *reinterpret_cast<const uint4*>(p1 + c + CK);
        }
#pragma unroll
        for (int i = 0; i < SC_PMAX; ++i)
            if (i >= i0 && i < i1) {
                const uint4* row = mine + i * a.dh * SC_PITCH_O;
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    float f2[CK];
                    chunk_f(row[j * DW], f2, (T*)nullptr);
                    float s = acc[i][j];
#pragma unroll
                    for (int e = 0; e < CK; ++e) s = fmaf(f1[e], f2[e], s);
                    acc[i][j] = s;
                }
            }
    }
    if (!live) return;
    const long long plane = (long long)a.Ho * a.Wo;
    float* o = a.out + (long long)n * a.Ph * a.Pw * plane + (long long)y * a.Wo + x;
#pragma unroll
    for (int i = 0; i < SC_PMAX; ++i)
        if (i >= i0 && i < i1) {
#pragma unroll
            for (int j = 0; j < PW; ++j) o[(long long)(i * PW + j) * plane] = acc[i][j] * a.scale;
        }
}

// ---- d in1 ----------------------------------------------------------------------------------------------------------------
template <typename T, int PW, int DW>
__global__ __launch_bounds__(256) void sc_bwd1_kernel(ScArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint4 sc_tile[];
    constexpr int CK = ScChunk<T>::CK;
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5, n = blockIdx.y;
    const int y0 = (int)(blockIdx.x / a.tiles_x) * SC_TY, x0 = (int)(blockIdx.x % a.tiles_x) * SC_TX;
    const int y = y0 + ty, x = x0 + tx;
    const bool live = y < a.Ho && x < a.Wo;
    const int y1 = y * a.sh - a.ph, x1 = x * a.sw - a.pw;
    const bool has1 = live && y1 >= 0 && y1 < a.H && x1 >= 0 && x1 < a.W;  // a sampled position inside the padding is cropped
    const long long img = (long long)n * a.H * a.W;
    const T* p2 = reinterpret_cast<const T*>(a.p2) + img * a.Cp;
    const int ry0 = y0 * a.sh - a.mh - a.ph, rx0 = x0 * a.sw - a.mw - a.pw;
    int code[SC_SLOTS_O];
    stage_plan<SC_SLOTS_O>(a, ry0, rx0, t, code);
    const uint4* mine = sc_tile + ty * a.sh * SC_PITCH_O + tx * a.sw;
    const long long plane = (long long)a.Ho * a.Wo;
    const float* dp = a.dout + (long long)n * a.Ph * a.Pw * plane + (live ? (long long)y * a.Wo + x : 0);
    float d[SC_PMAX][PW];
#pragma unroll
    for (int i = 0; i < SC_PMAX; ++i)
#pragma unroll
        for (int j = 0; j < PW; ++j) d[i][j] = (has1 && i < a.Ph) ? dp[(long long)(i * PW + j) * plane] * a.scale : 0.f;
    float* g = a.din1 + img * a.C + (has1 ? y1 * a.W + x1 : 0);
    // this workgroup's channel chunks (blockIdx.z: a small map is spread over more workgroups; channels are independent)
    const int c0 = blockIdx.z * a.zsplit * CK, c1 = min(a.Cp, c0 + a.zsplit * CK);
    for (int c = c0; c < c1; c += CK) {
        uint4 cur[SC_SLOTS_O];
        stage_load<T, SC_SLOTS_O>(a, p2, ry0, rx0, c, code, cur);
        __syncthreads();
        stage_store<SC_SLOTS_O, SC_PITCH_O>(code, cur, sc_tile);
        __syncthreads();
        float s[CK];
#pragma unroll
        for (int e = 0; e < CK; ++e) s[e] = 0.f;
#pragma unroll
        for (int i = 0; i < SC_PMAX; ++i)
            if (i < a.Ph) {
                const uint4* row = mine + i * a.dh * SC_PITCH_O;
#pragma unroll
                for (int j = 0; j < PW; ++j) {
                    float f2[CK];
                    chunk_f(row[j * DW], f2, (T*)nullptr);
                    const float dij = keep_scalar(d[i][j]);
#pragma unroll
                    for (int e = 0; e < CK; ++e) s[e] = fmaf(dij, f2[e], s[e]);
                }
            }
        if (has1) {
#pragma unroll
            for (int e = 0; e < CK; ++e)
                if (c + e < a.C) g[(long long)(c + e) * a.H * a.W] = s[e];
        }
    }
}

// ---- d in2 ----------------------------------------------------------------------------------------------------------------
// tiles_x, RH, RW: of this kernel's own tiling (in2's pixels; the staged map is in1 with a halo of m on every side).  The taps
// are walked from the far end, (i, j) = (P_h - 1 - ir, P_w - 1 - jr): in2 pixel (v, u) is displacement (i, j) of the padded
// position (v + pad - m + ir d, ...), so that tile offsets grow with (ir, jr) and stay compile-time.
template <typename T, int PW, int DW>
__global__ __launch_bounds__(256) void sc_bwd2_kernel(ScArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint4 sc_tile[];
    constexpr int CK = ScChunk<T>::CK;
    const int t = threadIdx.x, tx = t & 31, ty = t >> 5, n = blockIdx.y;
    const int v0 = (int)(blockIdx.x / a.tiles_x) * SC_TY, u0 = (int)(blockIdx.x % a.tiles_x) * SC_TX;
    const int v = v0 + ty, u = u0 + tx;                                     // unpadded frame
    const bool live = v < a.H && u < a.W;
    const long long img = (long long)n * a.H * a.W;
    const T* p1 = reinterpret_cast<const T*>(a.p1) + img * a.Cp;
    const int ry0 = v0 - a.mh, rx0 = u0 - a.mw;
    int code[SC_SLOTS_I];
    stage_plan<SC_SLOTS_I>(a, ry0, rx0, t, code);
    const uint4* mine = sc_tile + ty * SC_PITCH_I + tx;
    const long long plane = (long long)a.Ho * a.Wo;
    const float* dp = a.dout + (long long)n * a.Ph * a.Pw * plane;
    float d[SC_PMAX][PW];
#pragma unroll
    for (int ir = 0; ir < SC_PMAX; ++ir)
#pragma unroll
        for (int jr = 0; jr < PW; ++jr) {
            d[ir][jr] = 0.f;
            if (live && ir < a.Ph) {
                const int yp = v + a.ph - a.mh + ir * a.dh, xp = u + a.pw - a.mw + jr * DW;    // sampled if on the stride grid
                if (yp >= 0 && xp >= 0 && yp % a.sh == 0 && xp % a.sw == 0) {
                    const int y = yp / a.sh, x = xp / a.sw;
                    if (y < a.Ho && x < a.Wo)
                        d[ir][jr] = dp[(long long)((a.Ph - 1 - ir) * PW + PW - 1 - jr) * plane + (long long)y * a.Wo + x] * a.scale;
                }
            }
        }
    float* g = a.din2 + img * a.C + (live ? v * a.W + u : 0);
    // this workgroup's channel chunks (blockIdx.z: a small map is spread over more workgroups; channels are independent)
    const int c0 = blockIdx.z * a.zsplit * CK, c1 = min(a.Cp, c0 + a.zsplit * CK);
    for (int c = c0; c < c1; c += CK) {
        uint4 cur[SC_SLOTS_I];
        stage_load<T, SC_SLOTS_I>(a, p1, ry0, rx0, c, code, cur);
        __syncthreads();
        stage_store<SC_SLOTS_I, SC_PITCH_I>(code, cur, sc_tile);
        __syncthreads();
        float s[CK];
#pragma unroll
        for (int e = 0; e < CK; ++e) s[e] = 0.f;
#pragma unroll
        for (int ir = 0; ir < SC_PMAX; ++ir)
            if (ir < a.Ph) {
                const uint4* row = mine + ir * a.dh * SC_PITCH_I;
#pragma unroll
                for (int jr = 0; jr < PW; ++jr) {
                    float f1[CK];
                    chunk_f(row[jr * DW], f1, (T*)nullptr);
                    const float dij = keep_scalar(d[ir][jr]);
#pragma unroll
                    for (int e = 0; e < CK; ++e) s[e] = fmaf(dij, f1[e], s[e]);
                }
            }
        if (live) {
#pragma unroll
            for (int e = 0; e < CK; ++e)
                if (c + e < a.C) g[(long long)(c + e) * a.H * a.W] = s[e];
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------------
struct ScPlan {
    int Cp, Ho, Wo, mh, mw;
    size_t p1, p2, total;
};

int sc_plan(const VsrSpatialCorrDesc* d, ScPlan& pl) {
    if (!d || bad_dims(d->N, d->H, d->W) || d->C < 1 || bad_dtype(d->dtype)) return VSR_ERR_BADARG;
    if (d->patch_h < 1 || d->patch_w < 1 || d->stride_h < 1 || d->stride_w < 1 || d->pad_h < 0 || d->pad_w < 0 || d->dil_h < 1 || d->dil_w < 1)
        return VSR_ERR_BADARG;
    if (d->patch_h % 2 == 0 || d->patch_w % 2 == 0 || d->patch_h > SC_PMAX || d->patch_w > SC_PMAX) return VSR_ERR_UNSUPPORTED;
    if (d->stride_h > SC_SMAX || d->stride_w > SC_SMAX || d->dil_h > SC_DMAX || d->dil_w > SC_DMAX) return VSR_ERR_UNSUPPORTED;
    pl.mh = d->dil_h * (d->patch_h - 1) / 2; pl.mw = d->dil_w * (d->patch_w - 1) / 2;
    if (d->pad_h > pl.mh || d->pad_w > pl.mw) return VSR_ERR_UNSUPPORTED;
    // every in-image pixel index is an int and every tile count fits a grid dimension; offsets into the tensors are 64-bit
    if (d->H > (1 << 20) || d->W > (1 << 20) || d->C > (1 << 16) || d->N > 65535) return VSR_ERR_UNSUPPORTED;
    const long long Hp = d->H + 2 * d->pad_h, Wp = d->W + 2 * d->pad_w;
    if (Hp * Wp > (1ll << 24) || (long long)d->N * Hp * Wp > (1ll << 28)) return VSR_ERR_UNSUPPORTED;
    pl.Ho = (int)((Hp + d->stride_h - 1) / d->stride_h); pl.Wo = (int)((Wp + d->stride_w - 1) / d->stride_w);
    pl.Cp = (d->C + 7) & ~7;
    Bump b;
    const size_t bytes = (size_t)d->N * d->H * d->W * pl.Cp * esize(d->dtype);
    pl.p1 = b.take(bytes); pl.p2 = b.take(bytes);
    pl.total = b.off;
    return VSR_OK;
}

ScArgs sc_args(const VsrSpatialCorrDesc* d, const ScPlan& pl, void* ws) {
    ScArgs a = {};
    a.p1 = reinterpret_cast<char*>(ws) + pl.p1; a.p2 = reinterpret_cast<char*>(ws) + pl.p2;
    a.N = d->N; a.C = d->C; a.Cp = pl.Cp; a.H = d->H; a.W = d->W;
    a.Ph = d->patch_h; a.Pw = d->patch_w; a.sh = d->stride_h; a.sw = d->stride_w; a.ph = d->pad_h; a.pw = d->pad_w;
    a.dh = d->dil_h; a.dw = d->dil_w; a.mh = pl.mh; a.mw = pl.mw;
    a.Ho = pl.Ho; a.Wo = pl.Wo;
    a.scale = d->scale;
    return a;
}
// the two tilings: by output pixel (forward, d in1; the staged map is in2) and by in2 pixel (d in2; the staged map is in1)
unsigned sc_tile_by_output(ScArgs& a) {
    a.tiles_x = cdiv(a.Wo, SC_TX);
    a.RH = (SC_TY - 1) * a.sh + (a.Ph - 1) * a.dh + 1; a.RW = (SC_TX - 1) * a.sw + (a.Pw - 1) * a.dw + 1;
    return (unsigned)(a.tiles_x * cdiv(a.Ho, SC_TY));
}
unsigned sc_tile_by_in2(ScArgs& a) {
    a.tiles_x = cdiv(a.W, SC_TX);
    a.RH = SC_TY + 2 * a.mh; a.RW = SC_TX + 2 * a.mw;
    return (unsigned)(a.tiles_x * cdiv(a.H, SC_TY));
}

template <typename T>   // cl_stage.h in 32-channel tiles: C reaches 65536
void sc_pack(const VsrSpatialCorrDesc* d, const ScPlan& pl, const float* x, const void* dst, hipStream_t st) {
    cl_pack<32>(st, d->N, d->C, d->H * d->W, pl.Cp, ClIdentity{}, x, reinterpret_cast<T*>(const_cast<void*>(dst)));
}

// A grid of `wgs` workgroups that leaves compute units idle is multiplied by blockIdx.z: `parts` independent units of work (patch
// rows of the forward, channel chunks of a backward) go `a.zsplit` to a group.  Every sum is formed by one thread in one order
// whatever the split, so the results do not depend on it.
unsigned sc_split(ScArgs& a, long long wgs, int parts) {
    const int cus = vsr_num_cus();
    long long want = wgs >= cus ? 1 : cus / wgs;
    if (want > parts) want = parts;
    a.zsplit = cdiv(parts, (int)want);
    return (unsigned)cdiv(parts, a.zsplit);
}

// the kernel of one (patch_w, dil_w); ROWS x PITCH of 16-byte pixels of LDS
#define SC_LAUNCH_PW(kernel, PITCH, PW)                                                                                          \
    case PW:                                                                                                                     \
        if (a.dw == 1) hipLaunchKernelGGL((kernel<T, PW, 1>), dim3(tiles, d->N, groups), dim3(256), (size_t)a.RH * (PITCH) * sizeof(uint4), st, a); \
        else hipLaunchKernelGGL((kernel<T, PW, 2>), dim3(tiles, d->N, groups), dim3(256), (size_t)a.RH * (PITCH) * sizeof(uint4), st, a); \
        break;
#define SC_LAUNCH(kernel, PITCH)                                                                                                 \
    switch (a.Pw) {                                                                                                              \
        SC_LAUNCH_PW(kernel, PITCH, 1) SC_LAUNCH_PW(kernel, PITCH, 3) SC_LAUNCH_PW(kernel, PITCH, 5) SC_LAUNCH_PW(kernel, PITCH, 7) \
        SC_LAUNCH_PW(kernel, PITCH, 9)                                                                                           \
    }

template <typename T>
void sc_fwd(const VsrSpatialCorrDesc* d, const ScPlan& pl, ScArgs a, const float* in1, const float* in2, hipStream_t st) {
    sc_pack<T>(d, pl, in1, a.p1, st);
    sc_pack<T>(d, pl, in2, a.p2, st);
    const unsigned tiles = sc_tile_by_output(a), groups = sc_split(a, (long long)tiles * d->N, a.Ph);
    SC_LAUNCH(sc_fwd_kernel, SC_PITCH_O);
}

template <typename T>
void sc_bwd(const VsrSpatialCorrDesc* d, const ScPlan& pl, ScArgs a, const float* in1, const float* in2, hipStream_t st) {
    if (a.din1) {
        sc_pack<T>(d, pl, in2, a.p2, st);
        const unsigned tiles = sc_tile_by_output(a), groups = sc_split(a, (long long)tiles * d->N, pl.Cp / ScChunk<T>::CK);
        SC_LAUNCH(sc_bwd1_kernel, SC_PITCH_O);
    }
    if (a.din2) {
        sc_pack<T>(d, pl, in1, a.p1, st);
        const unsigned tiles = sc_tile_by_in2(a), groups = sc_split(a, (long long)tiles * d->N, pl.Cp / ScChunk<T>::CK);
        SC_LAUNCH(sc_bwd2_kernel, SC_PITCH_I);
    }
}
#undef SC_LAUNCH
#undef SC_LAUNCH_PW

}  // namespace

extern "C" {

size_t vsr_spatial_corr_workspace_bytes(const VsrSpatialCorrDesc* d) {
    ScPlan pl;
    if (!d) return 0;
    return sc_plan(d, pl) == VSR_OK ? pl.total : 0;
}

int vsr_spatial_corr_fwd(const VsrSpatialCorrDesc* d, const float* in1, const float* in2, float* out, void* ws, size_t ws_bytes,
                         void* stream) {
    ScPlan pl;
    if (!d) return VSR_ERR_BADARG;
    CK(sc_plan(d, pl));
    if (!in1 || !in2 || !out || !ws) return VSR_ERR_BADARG;
    if (ws_bytes < pl.total) return VSR_ERR_WORKSPACE;
    ScArgs a = sc_args(d, pl, ws);
    a.out = out;
    if (d->dtype == VSR_BF16) sc_fwd<bf16_t>(d, pl, a, in1, in2, (hipStream_t)stream);
    else sc_fwd<float>(d, pl, a, in1, in2, (hipStream_t)stream);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_spatial_corr_bwd(const VsrSpatialCorrDesc* d, const float* in1, const float* in2, const float* dout, float* din1, float* din2,
                         void* ws, size_t ws_bytes, void* stream) {
    ScPlan pl;
    if (!d) return VSR_ERR_BADARG;
    CK(sc_plan(d, pl));
    if (!in1 || !in2 || !dout || !ws) return VSR_ERR_BADARG;
    if (ws_bytes < pl.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    ScArgs a = sc_args(d, pl, ws);
    a.dout = dout; a.din1 = din1; a.din2 = din2;
    // d in1 is written at the sampled positions only: the ones a stride > 1 skips are zero
    if (din1 && (d->stride_h > 1 || d->stride_w > 1))
        HIP_CHECK_RET(hipMemsetAsync(din1, 0, (size_t)d->N * d->C * d->H * d->W * sizeof(float), st));
    if (d->dtype == VSR_BF16) sc_bwd<bf16_t>(d, pl, a, in1, in2, st);
    else sc_bwd<float>(d, pl, a, in1, in2, st);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
