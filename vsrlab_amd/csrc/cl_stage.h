// The staging layer of the gather ops (deform_conv.hip, raft_corr.hip, spatial_corr.hip): planar fp32 (N, C, HW) re-laid into a plain
// channels-last image [N][HW][Cp] of T (bf16 or fp32) with the pad channels zero, so that a gather finds one pixel's channels
// contiguous, and the way back for an fp32 accumulator of that shape.  Device code plus its launchers, every function static: the
// header is included by the files that use it and serves both shared libraries.  DESIGN section 3, "Staging layer".
// A workgroup of 256 threads transposes 32 pixels x one channel tile through a [32][width + 1] fp32 LDS tile: on the planar side lane
// px = t & 31 owns a pixel and 8 channels go per pass (128-byte runs), on the channels-last side the tile is walked linearly (whole
// pixel rows).  blockIdx = (pixel tile, channel tile, n).  TW > 0: gridDim.y channel tiles of TW packed channels (one may end past
// Cp: nothing is stored there); TW = 0: one tile of the run-time width Cp <= CL_MAXW.  Map::src(cp) is the source channel that packed
// channel cp holds; cp is a pad (zero in the packed image, never read on the way back) when that is not in [0, C).  Map::dst is the
// inverse on the real channels.  The images are sized exactly: no pixel at or past HW is stored and no address is formed for one.
#pragma once
#include "common.h"

constexpr int CL_PT = 32, CL_MAXW = 192;        // pixels per tile; the widest run-time tile (TW = 0)

struct ClIdentity {                     // channel cp is channel cp; C .. Cp - 1 are pads
    static constexpr bool tiles = true; // a channel tile of the packed image holds a range of source channels: TW > 0 is allowed
    __device__ int src(int cp) const { return cp; }
    __device__ int dst(int c) const { return c; }
};
struct ClGroups {                       // groups of cpg channels in slots of cpgp; whatever follows the last group is a pad
    static constexpr bool tiles = false;
    int cpg, cpgp, icpg, icpgp;         // i<x> = 2^16 / x + 1: n * i<x> >> 16 = n / x for x <= CL_MAXW, n < 452; no division delays a load
    ClGroups(int cpg, int cpgp) : cpg(cpg), cpgp(cpgp), icpg(65536 / cpg + 1), icpgp(65536 / cpgp + 1) {}
    __device__ int src(int cp) const { const int g = cp * icpgp >> 16, cl = cp - g * cpgp; return cl < cpg ? g * cpg + cl : -1; }
    __device__ int dst(int c) const { const int g = c * icpg >> 16; return g * cpgp + c - g * cpg; }
};

template <typename T, int TW, typename Map>
static __global__ __launch_bounds__(256) void cl_pack_kernel(const float* x, T* dst, int C, int HW, int Cp, Map map) {
    __shared__ float tile[CL_PT * ((TW ? TW : CL_MAXW) + 1)];
    const int w = TW ? TW : Cp, ld = w + 1;
    const int n = blockIdx.z, p0 = blockIdx.x * CL_PT, c0 = blockIdx.y * w, t = threadIdx.x, px = t & 31;
    if (p0 + px < HW) {
#pragma unroll 4
        for (int c = t >> 5; c < w; c += 8) {
            // a pad reads channel 0 of its pixel and drops it: the loads stay unconditional, four passes' loads in flight at once
            const int s = map.src(c0 + c);
            const float v = x[((long long)n * C + ((unsigned)s < (unsigned)C ? s : 0)) * HW + p0 + px];
            tile[px * ld + c] = (unsigned)s < (unsigned)C ? v : 0.f;
        }
    }
    __syncthreads();
    for (int i = t; i < CL_PT * w; i += 256) {
        const int q = i / w, c = i % w;
        if (p0 + q < HW && c0 + c < Cp) dst[((long long)n * HW + p0 + q) * Cp + c0 + c] = (T)tile[q * ld + c];
    }
}

// the adjoint, for an fp32 accumulator: [N][HW][Cp] -> planar; what the pads hold is dropped.  Each direction walks the channels of
// its destination, so every store is unconditional: here the tile's source channels c0 .. cend - 1, found at Map::dst(c).
template <int TW, typename Map>
static __global__ __launch_bounds__(256) void cl_unpack_kernel(const float* src, float* x, int C, int HW, int Cp, Map map) {
    static_assert(TW == 0 || Map::tiles, "a channel tile must hold the source channels c0 .. c0 + TW - 1");
    __shared__ float tile[CL_PT * ((TW ? TW : CL_MAXW) + 1)];
    const int w = TW ? TW : Cp, ld = w + 1;
    const int n = blockIdx.z, p0 = blockIdx.x * CL_PT, c0 = blockIdx.y * w, t = threadIdx.x, px = t & 31, cend = min(c0 + w, C);
    for (int i = t; i < CL_PT * w; i += 256) {
        const int q = i / w, c = i % w;
        tile[q * ld + c] = (p0 + q < HW && c0 + c < Cp) ? src[((long long)n * HW + p0 + q) * Cp + c0 + c] : 0.f;
    }
    __syncthreads();
    if (p0 + px < HW)
        for (int c = c0 + (t >> 5); c < cend; c += 8) x[((long long)n * C + c) * HW + p0 + px] = tile[px * ld + map.dst(c) - c0];
}

template <int TW>
static dim3 cl_grid(int N, int HW, int Cp) { return dim3(cdiv(HW, CL_PT), cdiv(Cp, TW ? TW : Cp), N); }
template <int TW, typename T, typename Map>
static void cl_pack(hipStream_t st, int N, int C, int HW, int Cp, Map map, const float* x, T* dst) {
    hipLaunchKernelGGL((cl_pack_kernel<T, TW, Map>), cl_grid<TW>(N, HW, Cp), dim3(256), 0, st, x, dst, C, HW, Cp, map);
}
template <int TW, typename Map>
static void cl_unpack(hipStream_t st, int N, int C, int HW, int Cp, Map map, const float* src, float* x) {
    hipLaunchKernelGGL((cl_unpack_kernel<TW, Map>), cl_grid<TW>(N, HW, Cp), dim3(256), 0, st, src, x, C, HW, Cp, map);
}
