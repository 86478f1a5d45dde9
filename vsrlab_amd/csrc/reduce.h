// The deterministic block reductions of the kernels, stated once.  Device code only: included by the files that define kernels.
//
// The contract: every loss value, norm, metric and bias gradient has the same bits from run to run, because every sum is taken in a
// fixed order and no atomic touches the value path:
//   1. each thread adds its own elements in a fixed strided order (the kernel's loop);
//   2. wave_sum: the 64-lane __shfl_down tree, offsets 32, 16, ... 1, result in lane 0;
//   3. wave_heads: lane 0 of each wave puts its sum into LDS, then one NAMED combiner adds the wave sums, either pairwise over four
//      waves, (r0 + r1) + (r2 + r3), or in index order, ((0 + r0) + r1) + ...;
//   4. where a launch has many workgroups, each writes one partial and ONE workgroup adds the partials in index order: per thread
//      at stride 256, then tree_sum256, the LDS halving tree from 128 down (partials_sum256 is that whole step).
// The two combiners round differently: the same inputs give different fp32 bits.  Which one a call site takes is part of its ABI,
// like its grid and block size -- recorded values, and the order test of vsr_pixel_loss_fwd_bwd (tests/test_losses_gpu.py), depend on it.
//
// The machine code of every caller was compared with its spelled-out form (profiles/reduce_header_isa.md: the sites left spelled
// out are listed there).  That is why wave_sum works in place, and why a reduction whose LDS words are reused calls wave_sum and
// wave_heads itself while one that writes them once takes wave_sums_to_lds: otherwise the same instructions come out in another order.
#pragma once
#include <hip/hip_runtime.h>

// v <- the sum of v over the 64 lanes of a wave; valid in lane 0
template <typename T> static __device__ __forceinline__ void wave_sum(T& v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
}

// red[w] = s of wave w's lane 0 (after wave_sum: the wave's sum), visible to the whole workgroup on return.  red: blockDim.x / 64 words of LDS;
// `guard`: a barrier in front of the store, for a red that other threads may still be reading from an earlier reduction.
template <typename T> static __device__ __forceinline__ void wave_heads(T s, T* red, bool guard) {
    if (guard) __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
}
// the two in one for a red that is written once
template <typename T> static __device__ __forceinline__ void wave_sums_to_lds(T v, T* red) { wave_sum(v); wave_heads(v, red, false); }

// the two combiners of the wave sums in red; in index order over `nwaves` waves, or over the workgroup's blockDim.x / 64
template <typename T> static __device__ __forceinline__ T sum4_pairwise(const T* red) { return (red[0] + red[1]) + (red[2] + red[3]); }
template <typename T> static __device__ __forceinline__ T sum_inorder(const T* red, int nwaves = 0) {
    T s = 0;
    for (int i = 0; i < (nwaves ? nwaves : (int)(blockDim.x >> 6)); ++i) s += red[i];
    return s;
}

// a 256-thread workgroup's sum of s, left in red[0] (256 words of LDS): red[tid] = s, then halves 128, 64, ... 1
template <typename T> static __device__ __forceinline__ void tree_sum256(T s, T* red) {
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
}

// step 4 as a kernel body: ONE workgroup of 256 threads, out[0] = the n partials added per thread at stride 256, then the tree
static __device__ __forceinline__ void partials_sum256(const float* __restrict__ partial, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    tree_sum256(s, red);
    if (threadIdx.x == 0) out[0] = red[0];
}
