// The element layer of the kernels: every kernel is written once and instantiated for T = bf16 (the perf build) and T = float
// (the exact parity build); what differs between the two -- fragment and chunk types, the MFMA step, the conversions of an
// 8-channel chunk of the blocked pixel-major layout (common.h) -- is defined here, once.  Device code only: included by the
// files that define kernels, never by the host-side headers.
//
// A "chunk" is 8 consecutive channels of one pixel as it lies in memory (16 bytes of bf16, 32 bytes of fp32); a "fragment" is
// the same 8 values as an MFMA operand.  conv_mfma.hip alone keeps its chunk REGISTERS as native vectors (see there).
#pragma once
#include "common.h"

struct f32x8_t { float v[8]; };
struct chunk32_t { uint4 a, b; };
template <typename T> struct Elt;
template <> struct Elt<bf16_t> {
    static constexpr int CHB = 16;                 // bytes per 8-channel chunk
    typedef bf16x8_t frag_t;
    typedef uint4 chunk_t;
};
template <> struct Elt<float> {
    static constexpr int CHB = 32;
    typedef f32x8_t frag_t;
    typedef chunk32_t chunk_t;
};

// D[32 x 32] += A[32 x 16] B[16 x 32]: each lane holds 8 consecutive channels (k) of its row of A and its column of B
static __device__ __forceinline__ void mma(f32x16_t& acc, const bf16x8_t& a, const bf16x8_t& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
static __device__ __forceinline__ void mma(f32x16_t& acc, const f32x8_t& a, const f32x8_t& b) {
    // k-slot j of the 32x32x2 step = channel {j (lanes 0-31), 8+j (lanes 32-63)} of the 16-group:
    // any consistent k order is a valid reduction order.
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[j], b.v[j], acc, 0, 0, 0);
}

static __device__ __forceinline__ float to_f(bf16_t v) { return (float)v; }
static __device__ __forceinline__ float to_f(float v) { return v; }

// 4 consecutive channels, loaded and stored as one 8- or 16-byte access
template <typename T> struct Vec4;
template <> struct __attribute__((aligned(8))) Vec4<bf16_t> { bf16_t v[4]; };
template <> struct __attribute__((aligned(16))) Vec4<float> { float v[4]; };

template <typename T> static __device__ __forceinline__ typename Elt<T>::chunk_t zero_chunk();
template <> __device__ __forceinline__ uint4 zero_chunk<bf16_t>() { return make_uint4(0, 0, 0, 0); }
template <> __device__ __forceinline__ chunk32_t zero_chunk<float>() { chunk32_t z; z.a = make_uint4(0, 0, 0, 0); z.b = z.a; return z; }

// channels (a, b, c, 0, 0, 0, 0, 0): a planar 3-channel pixel on its way into a padded 16-channel LDS image
static __device__ __forceinline__ uint4 make_chunk3(float a, float b, float c, bf16_t*) {
    union { bf16_t h[8]; uint4 u; } t; t.u = make_uint4(0, 0, 0, 0);
    t.h[0] = (bf16_t)a; t.h[1] = (bf16_t)b; t.h[2] = (bf16_t)c; return t.u;
}
static __device__ __forceinline__ chunk32_t make_chunk3(float a, float b, float c, float*) {
    chunk32_t t; t.a = make_uint4(__float_as_uint(a), __float_as_uint(b), __float_as_uint(c), 0); t.b = make_uint4(0, 0, 0, 0); return t;
}

// a loaded chunk -> 8 floats, and back (rounding to T)
static __device__ __forceinline__ void unpack8(const uint4& v, float* f) {
    union { uint4 u; bf16_t h[8]; } t; t.u = v;
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)t.h[j];
}
static __device__ __forceinline__ void unpack8(const chunk32_t& v, float* f) {
    f[0] = __uint_as_float(v.a.x); f[1] = __uint_as_float(v.a.y); f[2] = __uint_as_float(v.a.z); f[3] = __uint_as_float(v.a.w);
    f[4] = __uint_as_float(v.b.x); f[5] = __uint_as_float(v.b.y); f[6] = __uint_as_float(v.b.z); f[7] = __uint_as_float(v.b.w);
}
static __device__ __forceinline__ void pack8(const float* f, uint4& v) {
    union { uint4 u; bf16_t h[8]; } t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t.h[j] = (bf16_t)f[j];
    v = t.u;
}
static __device__ __forceinline__ void pack8(const float* f, chunk32_t& v) {
    v.a = make_uint4(__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]), __float_as_uint(f[3]));
    v.b = make_uint4(__float_as_uint(f[4]), __float_as_uint(f[5]), __float_as_uint(f[6]), __float_as_uint(f[7]));
}

// the same on the chunk at p (16- / 32-byte aligned)
template <typename T> static __device__ __forceinline__ void ld8(const T* p, float* f);
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float* f) {
    union { uint4 u; bf16_t h[8]; } t; t.u = *reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = (float)t.h[j];
}
template <> __device__ __forceinline__ void ld8<float>(const float* p, float* f) {
    const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
template <typename T> static __device__ __forceinline__ void st8(T* p, const float* f);
template <> __device__ __forceinline__ void st8<bf16_t>(bf16_t* p, const float* f) {
    union { uint4 u; bf16_t h[8]; } t;
#pragma unroll
    for (int j = 0; j < 8; ++j) t.h[j] = (bf16_t)f[j];
    *reinterpret_cast<uint4*>(p) = t.u;
}
template <> __device__ __forceinline__ void st8<float>(float* p, const float* f) {
    reinterpret_cast<float4*>(p)[0] = make_float4(f[0], f[1], f[2], f[3]);
    reinterpret_cast<float4*>(p)[1] = make_float4(f[4], f[5], f[6], f[7]);
}

// PyTorch upsample_bilinear2d(align_corners=False): the two source taps and the weight of the second for output index d;
// `inv` = in_size / out_size, any ratio (1/4 and 1/2 in basicvsr.py:22, the resize of compute_loss and its adjoint)
static __device__ __forceinline__ void bil_src(int d, int in_size, int& i0, int& i1, float& l1, float inv) {
    float s = (d + 0.5f) * inv - 0.5f;
    s = s < 0.f ? 0.f : s;
    i0 = (int)s;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
}

// ds_read_b64_tr_b16: the transposing LDS read that fetches a K-strided bf16 MFMA fragment from a [pixel][channel] image
static __device__ __forceinline__ s16x4_t lds_tr_read(const char* p) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4_t*)p);
}
