// The hot kernel of the path: 3x3, 64 -> 64 channels, bf16 in / fp32 accumulate.
//   core/modules/conv.py:85-86 (ResidualConv conv1/conv2), basicvsr.py:20 (conv_last.0),
//   upsampling.py:7 (as 4 pixel-shuffle phases), and all their data gradients: > 70 % of the FLOPs.
//
// At 540p one launch moves 133-200 MB for 38 GFLOP: 21-32 us at the 6.3 TB/s a CU-side stream reaches,
// 15 us on the matrix cores -- the kernel is HBM-bound, and a CU needs ~75 KB in flight to cover ~3 us of
// loaded HBM latency.  Design for one MI355X CU (160 KiB LDS, 4 SIMDs):
//   * ONE 512-thread workgroup per CU, grid = #CUs, persistent over 8x32-pixel tiles: 4 MFMA waves + 4 LDS-DMA producer waves, one of
//     each per SIMD.  The packed weights (72 KiB) are loaded into LDS once and stay; the haloed input tile is double-buffered and
//     filled one whole tile ahead; the residual / mask operands of the epilogue are requested into registers before the K loop.
//     Nothing the tile needs is waited for at first use.
//   * the LDS images, the weight staging, the producers' DMA, the K loop and the packed-word epilogue arms are the tile core this kernel
//     shares with the chain kernel (conv3x3_chain.hip): conv3x3_c64_tile.h, described there.  Here: the tile walk, the launch's
//     arguments, and the epilogue arms only a single layer needs (LeakyReLU(0.1), masks read from `aux`, pixel-shuffle placement).
#include "conv3x3_c64_tile.h"
#include <type_traits>

namespace {

constexpr int P_LDS = BIAS_OFF + 256;                                     // 161,024 <= 163,840

__device__ uint4 g_conv_zero_chunk[2];

template <int ACT> __device__ __forceinline__ float p_act(float v, float slope) {
    if (ACT == ACT_RELU) return v > 0.f ? v : 0.f;
    if (ACT == ACT_LEAKY) return v > 0.f ? v : slope * v;
    return v;
}

// What a restructuring could buy was bounded with ablated builds of this file: DESIGN 4.1.  Clock build only (make CLOCK=1):
// s_memtime / s_memrealtime around the whole kernel, lane 0 of wave 0, to a buffer of their own.
#ifdef VSR_CLOCK
__device__ unsigned long long g_clk[256 * 4];
#endif

__device__ __forceinline__ void tile_coords(int tile, int ntx, int nty, int& n, int& ty0, int& tx0) {
    const int per = ntx * nty;
    n = tile / per;
    const int r = tile - n * per;
    const int ty = r / ntx;
    ty0 = ty * PTH;
    tx0 = (r - ty * ntx) * PTW;
}

// Walks a workgroup's tiles first, first + stride, ... keeping (image, tile row, tile column): two divisions once, then a handful of
// scalar adds and compares per tile (tile_coords per tile = two runtime divisions through v_rcp_iflag_f32, ~60 instructions).
struct TileIter {
    int tile, n, ty, tx;          // tile index; image, tile row, tile column
    int sn, sty, stx;             // the stride in those units
    __device__ __forceinline__ void init(int first, int stride, int ntx, int nty) {
        const int per = ntx * nty;
        tile = first; n = first / per; int r = first - n * per; ty = r / ntx; tx = r - ty * ntx;
        sn = stride / per; r = stride - sn * per; sty = r / ntx; stx = r - sty * ntx;
    }
    __device__ __forceinline__ void advance(int stride, int ntx, int nty) {
        tile += stride;
        tx += stx; if (tx >= ntx) { tx -= ntx; ++ty; }
        ty += sty; if (ty >= nty) { ty -= nty; ++n; }
        n += sn;
    }
};

__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

// Plain (not nt) tile DMA and output stores.  tools/bw_probe.hip streams reads at 6.4-7.0 TB/s with nt against 5.7-6.2 without, and
// out of cache (tools/ab_conv.py, 8 rotating buffer sets) nt STORES took 7 % off a bias+ReLU launch (36.7 -> 34.0 us; bias+skip 42.3 ->
// 41.5; nt loads: 36.2 / 44.3) -- but inside a step, applied to the outputs of >= 512 MB (the 16P tensors of the reconstruction), the
// step was 0.2-0.7 ms SLOWER (124.6-124.9 -> 125.1-125.6 ms, three interleaved pairs): their consumers do find the tail of such a
// tensor in the Infinity Cache (r04).
constexpr int DMA_PLAIN = 0;

// Epilogue variants are compile-time: a runtime-selected epilogue serialises 16 load->use->store
// chains per tile (measured: 14 us of a 71 us launch).
template <int ACT, bool HAS_RES, int MASK>
__global__ __launch_bounds__(PNT, 1) void conv3x3_c64_persist_kernel(const ConvArgs ka) {
    extern __shared__ __attribute__((aligned(16))) char smem[];

    // Every kernel argument the kernel uses, requested in ONE batch at the top and pinned in scalar registers: hipcc otherwise
    // loads arguments lazily, next to their first use, and the producers' way to the first DMA piece went through three
    // dependent s_load + lgkmcnt(0) rounds on the (cold) kernarg segment (r03 stamps: 3.0 k cycles from the start of the
    // launch to the first piece; the first tile is the critical path of the prologue).
    const int z = blockIdx.y;
    struct {
        int N, H, W, Ws, Wd, in_step, out_step, src_ox0, src_oy0, out_oxz, out_oyz, bias_zstride, unshuffle;
        long long src_nstride0, dst_nstride, w_zstride, plane;
        unsigned long long src0, wpack, resz, auxz, sign_bitsz, dstz, sign_outz, bias; float leaky_slope;   // pointers as integers: GP() below
    } a = {ka.N, ka.H, ka.W, ka.Ws, ka.Wd, ka.in_step, ka.out_step, ka.src_ox[0], ka.src_oy[0], ka.out_ox[z], ka.out_oy[z], ka.bias_zstride, ka.unshuffle,
           ka.src_nstride[0], ka.dst_nstride, ka.w_zstride, ka.unshuffle_plane,
           (unsigned long long)ka.src[0], (unsigned long long)ka.wpack, (unsigned long long)ka.res[z], (unsigned long long)ka.aux[z],
           (unsigned long long)ka.sign_bits[z], (unsigned long long)ka.dst[z], (unsigned long long)ka.sign_out[z], (unsigned long long)ka.bias, ka.leaky_slope};
    asm volatile("" : "+s"(a.N), "+s"(a.H), "+s"(a.W), "+s"(a.Ws), "+s"(a.Wd), "+s"(a.in_step), "+s"(a.out_step), "+s"(a.src_ox0), "+s"(a.src_oy0),
                 "+s"(a.out_oxz), "+s"(a.out_oyz), "+s"(a.bias_zstride), "+s"(a.unshuffle), "+s"(a.src_nstride0), "+s"(a.dst_nstride), "+s"(a.w_zstride), "+s"(a.plane));
    asm volatile("" : "+s"(a.src0), "+s"(a.wpack), "+s"(a.resz), "+s"(a.auxz), "+s"(a.sign_bitsz), "+s"(a.dstz), "+s"(a.sign_outz), "+s"(a.bias), "+s"(a.leaky_slope));
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int role = __builtin_amdgcn_readfirstlane(wave >> 2);            // 0: MFMA + epilogue, 1: LDS-DMA producer
    const int w4 = wave & 3;                                               // index within the role
    const int l15 = lane & 15, q = lane >> 4;                              // 16x16x32 operand / accumulator coordinates
    const int pxl = PM_LANE_PIXEL(l15);
    char* lds_w = smem;
    char* lds_t = smem + W_BYTES;                                         // two tile buffers
#ifdef VSR_CLOCK
    unsigned long long clk_t0 = 0, clk_r0 = 0;
    if (tid == 0) { clk_t0 = __builtin_amdgcn_s_memtime(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
#endif

    const int ntx = cdiv(a.W, PTW), nty = cdiv(a.H, PTH);
    const int total = a.N * ntx * nty;
    const int WSs = pm_ws(a.Ws), WSd = pm_ws(a.Wd);           // source / destination images may be larger than the view
    const TileWalk walk = xcd_tile_walk(total, blockIdx.x, gridDim.x);

    // bias of this z as fp32 in LDS: the accumulators of every tile start from it (32 fewer live registers
    // than carrying it, which is what lets two waves share a SIMD)
    // (slot r = the channel MFMA row r of the 64 computes: paired-block order, see the epilogue)
    if (tid < 64) reinterpret_cast<float*>(smem + BIAS_OFF)[tid] = a.bias ? GP(const float, a.bias)[(long long)z * a.bias_zstride + pm_acc_chan(tid >> 4, tid & 15)] : 0.f;

    // ---- weights of this z -> LDS (C64_W_LOAD / C64_W_STORE) ----
    // The four MFMA waves stage all 4608 chunks (18 per thread; the loads are issued first, the waves' own set-up arithmetic runs
    // under their latency, then the LDS writes); the producer waves meanwhile do nothing but get the first tile's DMA out: at
    // the start of a launch the tile is the critical path (r03 stamps: the producers took 2.7 k cycles of set-up + 2.2 k of
    // issue + 3.2 k for their half of the weights before the first barrier; 8.4 k cycles of a 63 k-cycle launch).
    const auto* wg = GP(const u32x4_t, a.wpack + (unsigned long long)((long long)z * a.w_zstride) * 2);

    if (role == 1) {
        // =================== producer waves: LDS-DMA of the haloed tiles, one tile ahead ===================
        // Their VMEM issue slots (an LDS-DMA instruction does not finish issuing until the memory pipe takes it) run
        // beside the MFMA waves' matrix-core time on the same SIMDs.
        const auto* src = GP(const char, a.src0);
        const auto* zsrc = GP(const char, g_conv_zero_chunk);
        int rel[NPIECE_W];
        C64_DMA_REL(rel, w4, lane, a.in_step, a.src_oy0, a.src_ox0, WSs)
        auto issue = [&](const TileIter& it, int buf) {
            const int n = it.n, ty0 = it.ty * PTH, tx0 = it.tx * PTW;
            const auto* org = src + ((long long)n * a.src_nstride0 + pm_off(ty0 * a.in_step, tx0 * a.in_step, 0, a.Ws, 64)) * 2;
            char* dstb = lds_t + buf * IN_BYTES;
            C64_DMA_TILE(DMA_PLAIN, rel, org, zsrc, dstb, w4, lane, ty0, tx0, a.H, a.W)
        };
        int cur = 0;
        TileIter it;
        it.init(walk.first, walk.stride, ntx, nty);
        if (it.tile < walk.end) issue(it, 0);              // first tile in flight while the MFMA waves stage the weights
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // weights and the first tile are in LDS
        while (it.tile < walk.end) {
            it.advance(walk.stride, ntx, nty);
            if (it.tile < walk.end) issue(it, cur ^ 1);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            cur ^= 1;
        }
    } else {
        // =================== MFMA waves: K loop + epilogue of tile rows 2 w4, 2 w4 + 1 ===================
        u32x4_t wv[WCH];
        C64_W_LOAD(wv, wg, tid)
        C64_MFMA_LANE(w4, l15, q, pxl)
        // epilogue: accumulator blocks (2k, nb) and (2k+1, nb), registers j = channels 8 (4k + q) + j and + 4 + j of pixel
        // (row nb >> 1, 16 (nb & 1) + i): chunk 4k + q of the blocked layout, whole.  loff[nb] = lane-constant part of the
        // destination element offset relative to the tile's origin pm_off(ty0*os + ooy, tx0*os) (tx0*os: multiple of 32)
        int loff[4];
#pragma unroll
        for (int nb = 0; nb < 4; ++nb) {
            const int dx = ((nb & 1) * 16 + pxl) * a.out_step + a.out_oxz;
            loff[nb] = ((((w4 * 2 + (nb >> 1)) * a.out_step) * WSd + (dx >> 5)) * 8 + q) * 256 + (dx & 31) * 8;
            if (a.unshuffle) {      // phase-separated destination (ConvArgs::unshuffle): plane 2 (row & 1) + (px & 1), position (row >> 1, px >> 1)
                const int row = w4 * 2 + (nb >> 1), px = (nb & 1) * 16 + pxl;
                loff[nb] = (int)(((row & 1) * 2 + (px & 1)) * a.plane) + (((row >> 1) * pm_ws(a.Wd >> 1)) * 8 + q) * 256 + (px >> 1) * 8;
            }
        }
        C64_W_STORE(wv, lds_w, tid)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                   // weights and the first tile are in LDS
        auto* const dst_z = GP(bf16_t, a.dstz);
        const auto* const res_z = GP(const bf16_t, a.resz);
        const auto* const aux_z = GP(const bf16_t, a.auxz);
        const auto* const sbits_z = GP(const u32x2_t, a.sign_bitsz);
        auto* const sout_z = GP(u32x2_t, a.sign_outz);
        const float slope = vsr_slope(a.leaky_slope);      // LeakyReLU slope (0.1 on the BasicVSR path, 0.2 in the discriminator)

        f32x4_t bvec[4];
#pragma unroll
        for (int mb = 0; mb < 4; ++mb) bvec[mb] = c64_bias_rows(smem, q, mb);
        C64_RES_IDENTITY(idA, l15, q)
        static_assert(!HAS_RES || ACT == ACT_NONE, "the residual goes in on the matrix cores, ahead of any activation");

        int cur = 0;
        TileIter it;
        for (it.init(walk.first, walk.stride, ntx, nty); it.tile < walk.end; it.advance(walk.stride, ntx, nty)) {
            // epilogue operands, requested now, used after the K loop
            const int tile = it.tile, n = it.n, ty0 = it.ty * PTH, tx0 = it.tx * PTW;
            const long long tbase = a.unshuffle ? (long long)n * a.dst_nstride + pm_off(ty0 >> 1, tx0 >> 1, 0, a.Wd >> 1, 64)      // (tx0 >> 1: a multiple of 16)
                                                : (long long)n * a.dst_nstride + pm_off(ty0 * a.out_step + a.out_oyz, tx0 * a.out_step, 0, a.Wd, 64);
            // a tile inside the image (all but the last tile row / column of a ragged size) needs no per-lane bounds: straight-line
            // operand loads and epilogue (wave-uniform choice)
            const bool full = ty0 + PTH <= a.H && tx0 + PTW <= a.W;
            bool ok[4];
            constexpr bool BITS = MASK == MASK_RELU_BITS || MASK == MASK_LEAKY_BITS;
            constexpr bool LATE_MASK = HAS_RES && MASK != MASK_NONE && !BITS;   // both bf16 operands early would not fit 2 waves / SIMD
            u32x4_t rr[2][4], mm[2][4];                                // [k][nb]: 8 channels of one pixel
            u32x2_t sbits = {0u, 0u};                         // 64 sign bits of this lane's 64 outputs of the tile
            if (BITS) sbits = sbits_z[c64_sign_word(tile, w4, lane)];
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) ok[nb] = (tx0 + (nb & 1) * 16 + pxl < a.W) && (ty0 + w4 * 2 + (nb >> 1) < a.H);
#define CV_OPERANDS(OKN)                                                                                               \
            _Pragma("unroll") for (int nb = 0; nb < 4; ++nb) {                                                         \
                if (OKN) {                                                                                             \
                    _Pragma("unroll") for (int k = 0; k < 2; ++k) {                                                    \
                        const long long o = tbase + loff[nb] + k * 1024;                                               \
                        if (HAS_RES) rr[k][nb] = *GP(const u32x4_t, res_z + o);                                        \
                        if (MASK != MASK_NONE && !LATE_MASK && !BITS) mm[k][nb] = *GP(const u32x4_t, aux_z + o);       \
                    }                                                                                                  \
                }                                                                                                      \
            }
            if (HAS_RES || (MASK != MASK_NONE && !LATE_MASK && !BITS)) {
                if (full) { CV_OPERANDS(true) } else { CV_OPERANDS(ok[nb]) }
            }
#undef CV_OPERANDS

            f32x4_t acc[4][4];                                      // first written by step 0's MFMAs, whose C operand is the bias

            C64_K_LOOP(acc, bvec, cur)

            // ---- epilogue, entirely in registers; a store covers two 256-byte runs (two chunks x 16 pixels) per wave ----
            // The residual / mask operands were requested before the K loop and have long returned, but vmcnt counts loads and
            // stores together in issue order: hipcc's per-use waits (vmcnt(3) in every ok[nb] branch) made each store wait for
            // the write acknowledgement of the store three before it -- ~5 exposed store latencies per tile (r03: 48 -> ~42 us
            // per bias+skip launch).  One explicit wait here (the builtin: hipcc's scoreboard then knows the queue is empty)
            // covers the operands; the stores after it are never waited for inside the tile.
            if (HAS_RES || MASK != MASK_NONE) __builtin_amdgcn_s_waitcnt(0x0F70);        // vmcnt(0) alone
            if constexpr (HAS_RES) { C64_ADD_RESIDUAL(acc, idA, rr) }
            unsigned sout[2] = {0u, 0u};                    // the lane's sign words (c64_tile.h)
            auto epilogue = [&](auto FULL) {
#pragma unroll
            for (int nb = 0; nb < 4; ++nb) {
                if (decltype(FULL)::value || ok[nb]) {
                    auto* dst = dst_z + tbase + loff[nb];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        float v[8];
#pragma unroll
                        for (int j = 0; j < 4; ++j) { v[j] = acc[2 * k][nb][j]; v[4 + j] = acc[2 * k + 1][nb][j]; }
                        const unsigned wbits = k ? sbits.y : sbits.x;            // words wd = 16 k + 4 nb + jj
                        unsigned ow[4];
                        if (ACT == ACT_RELU && !HAS_RES && MASK == MASK_NONE) {
                            C64_ARM_RELU(ow, v, nb, sout[k])       // conv1 of a ResidualConv
                        } else if (ACT == ACT_LEAKY && !HAS_RES && MASK == MASK_NONE) {
                            // conv_last.0: LeakyReLU = max(v, slope v) (0 < slope < 1), sign bits from the packed words as in the ReLU case
                            // (bit = "the stored half is positive", what sign_bits_c64_kernel computes from a stored activation)
#pragma unroll
                            for (int jj = 0; jj < 4; ++jj) {
                                ow[jj] = pk_bf16(fmaxf(v[2 * jj], v[2 * jj] * slope), fmaxf(v[2 * jj + 1], v[2 * jj + 1] * slope));
                                sout[k] |= pk_min_u16(pk_max_i16(ow[jj], 0u), C64_K11) << (4 * nb + jj);
                            }
                        } else if (ACT == ACT_NONE && !HAS_RES && MASK == MASK_RELU_BITS) {
                            C64_ARM_MASKED(ow, v, nb, wbits)       // dgrad(conv2) * ReLU'
                        } else {
#pragma unroll
                            for (int j = 0; j < 8; ++j) v[j] = p_act<ACT>(v[j], slope);
                            if (ACT != ACT_NONE && !HAS_RES) {      // sign of the activation = sign of its argument (ReLU and LeakyReLU alike)
#pragma unroll
                                for (int j = 0; j < 8; ++j) sout[k] |= (v[j] > 0.f ? 1u : 0u) << (4 * nb + (j >> 1) + 16 * (j & 1));
                            }
                            if (BITS) {
                                const float neg = MASK == MASK_LEAKY_BITS ? slope : 0.f;
#pragma unroll
                                for (int j = 0; j < 8; ++j) v[j] *= ((wbits >> (4 * nb + (j >> 1) + 16 * (j & 1))) & 1u) ? 1.f : neg;
                            } else if (MASK != MASK_NONE) {
                                const float neg = MASK == MASK_LEAKY ? slope : 0.f;
                                u32x4_t mq = mm[k][nb];
                                if (LATE_MASK) mq = *GP(const u32x4_t, aux_z + tbase + loff[nb] + k * 1024);
                                const unsigned mw[4] = {mq.x, mq.y, mq.z, mq.w};
#pragma unroll
                                for (int jj = 0; jj < 4; ++jj) {
                                    if (MASK == MASK_RELU) {    // +0 where masked, as the sign-bit arm stores (a product with 0 keeps v's sign: -0)
                                        v[2 * jj] = bf_lo(mw[jj]) > 0.f ? v[2 * jj] : 0.f;
                                        v[2 * jj + 1] = bf_hi(mw[jj]) > 0.f ? v[2 * jj + 1] : 0.f;
                                    } else {
                                        v[2 * jj] *= (bf_lo(mw[jj]) > 0.f ? 1.f : neg);
                                        v[2 * jj + 1] *= (bf_hi(mw[jj]) > 0.f ? 1.f : neg);
                                    }
                                }
                            }
                            C64_ARM_PLAIN(ow, v)
                        }
                        const u32x4_t o = {ow[0], ow[1], ow[2], ow[3]};
                        *GP(u32x4_t, dst + k * 1024) = o;
                    }
                }
            }
            };
            if (full) epilogue(std::true_type{}); else epilogue(std::false_type{});
            if (ACT != ACT_NONE && !HAS_RES && sout_z) sout_z[c64_sign_word(tile, w4, lane)] = u32x2_t{sout[0], sout[1]};
            __syncthreads();                               // the producers' next tile has landed; everybody has finished reading `cur`
            cur ^= 1;
        }
    }
#ifdef VSR_CLOCK
    if (tid == 0 && blockIdx.y == 0 && blockIdx.x < 256) {
        g_clk[blockIdx.x * 4 + 0] = __builtin_amdgcn_s_memtime() - clk_t0;
        g_clk[blockIdx.x * 4 + 1] = __builtin_amdgcn_s_memrealtime() - clk_r0;
    }
#endif
}

// Sign bits of a stored bf16 activation in THIS kernel's tile order ([tile][MFMA wave][lane] x 64 bits; the lane's piece (k, nb) =
// chunk 4k + q of pixel (row 2 w4 + (nb >> 1), column 16 (nb & 1) + pxl), its packed word jj = channels 2jj, 2jj+1: bits
// 4 nb + jj and 16 + 4 nb + jj of word k): for activations produced by another kernel (the trunk stem runs on the generic
// two-source kernel) whose mask a persistent data-gradient launch needs.  66 MB read, 4 MB written at 540p.
__global__ void sign_bits_c64_kernel(const bf16_t* __restrict__ x, uint2* __restrict__ bits, int N, int H, int W) {
    const int ntx = cdiv(W, PTW), nty = cdiv(H, PTH);
    const long long total = (long long)N * ntx * nty * 256;
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int lane = (int)(gid & 63), w4 = (int)((gid >> 6) & 3);
    const int tile = (int)(gid >> 8);
    const int l15 = lane & 15, q = lane >> 4;
    const int pxl = PM_LANE_PIXEL(l15);
    int n, ty0, tx0;
    tile_coords(tile, ntx, nty, n, ty0, tx0);
    unsigned out[2] = {0u, 0u};
#pragma unroll
    for (int nb = 0; nb < 4; ++nb) {
        const int yy = ty0 + 2 * w4 + (nb >> 1), xx = tx0 + (nb & 1) * 16 + pxl;
        if (yy < H && xx < W) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const uint4 v = *reinterpret_cast<const uint4*>(x + (long long)n * pm_image_elems(H, W, 64) + pm_off(yy, xx, 4 * k + q, W, 64));
                const unsigned vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int jj = 0; jj < 4; ++jj)
                    out[k] |= ((bf_lo(vw[jj]) > 0.f ? 1u : 0u) | (bf_hi(vw[jj]) > 0.f ? 0x10000u : 0u)) << (4 * nb + jj);
            }
        }
    }
    bits[gid] = make_uint2(out[0], out[1]);
}

template <int ACT, bool HAS_RES, int MASK>
static int launch_persist(const ConvArgs& a, int num_cus, hipStream_t st) {
    auto kern = conv3x3_c64_persist_kernel<ACT, HAS_RES, MASK>;
    static VsrDevOnce once;                                 // one per instantiation, remembered per device
    { const int rc = vsr_set_max_dynamic_lds(once, reinterpret_cast<const void*>(kern), P_LDS); if (rc != VSR_OK) return rc; }
    const int tiles = a.N * cdiv(a.W, PTW) * cdiv(a.H, PTH);
    int gx = num_cus / a.nz;
    gx &= ~7;                                               // whole XCD groups (xcd_tile_walk)
    if (gx < 8) gx = num_cus / a.nz;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    hipLaunchKernelGGL(kern, dim3(gx, a.nz), dim3(PNT), P_LDS, st, a);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // namespace

#ifdef VSR_CLOCK
extern "C" int vsr_debug_read_clk(unsigned long long* host_out) {      // [256 workgroups][cycles, 100 MHz ticks, -, -] of the last launch
    return hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_clk), sizeof(unsigned long long) * 256 * 4) == hipSuccess ? 0 : -3;
}
#endif

// Eligibility is decided by the dispatcher in conv_mfma.hip (bf16, 3x3, one 64-channel source at unit
// step, 64 output channels, blocked pixel-major destination).  Returns VSR_ERR_UNSUPPORTED for an epilogue
// combination that has no instantiation; the caller then uses the generic kernel.
int vsr_launch_conv3x3_c64_persist(const ConvArgs& a, int num_cus, hipStream_t st) {
    bool res = false, aux = false;
    for (int z = 0; z < a.nz; ++z) { res = res || a.res[z]; aux = aux || a.aux[z]; }
    for (int z = 0; z < a.nz; ++z) if ((res && !a.res[z]) || (aux && !a.aux[z])) return VSR_ERR_UNSUPPORTED;
    int mask = aux ? a.mask_mode : MASK_NONE;
    if (mask == MASK_RELU && !res) {                       // sign bits instead of the activation, if every z has them
        bool bits = true;
        for (int z = 0; z < a.nz; ++z) bits = bits && a.sign_bits[z];
        if (bits) mask = MASK_RELU_BITS;
    }
    if (mask == MASK_LEAKY && res) {                       // (dgrad + dX) * LeakyReLU': the mask from sign bits keeps the residual prefetch
        bool bits = true;
        for (int z = 0; z < a.nz; ++z) bits = bits && a.sign_bits[z];
        if (bits) mask = MASK_LEAKY_BITS;
    }
    if (pm_image_elems((PTHH + 2) * a.in_step, a.Ws, 64) * 2 > 0x7fffffffLL || pm_image_elems(2 * PTH + 2, a.Wd, 64) > 0x7fffffffLL)
        return VSR_ERR_UNSUPPORTED;                                                  // in-tile offsets are 32-bit
    if (a.unshuffle) {                                         // phase-separated destination: plain stride-1 launches without an activation-mask operand
        if (a.nz != 1 || a.out_step != 1 || a.out_ox[0] || a.out_oy[0] || (a.Hd & 1) || (a.Wd & 1) || a.Hd != a.H || a.Wd != a.W || aux ||
            a.unshuffle_plane < (long long)a.N * pm_image_elems(a.Hd / 2, a.Wd / 2, 64) || a.dst_nstride != pm_image_elems(a.Hd / 2, a.Wd / 2, 64) ||
            3 * a.unshuffle_plane + pm_image_elems(PTH + 2, a.Wd / 2, 64) > 0x7fffffffLL)
            return VSR_ERR_UNSUPPORTED;
    }
#define PERSIST_CASE(ACT, RES, MASK) if (a.act == ACT && res == RES && mask == MASK) return launch_persist<ACT, RES, MASK>(a, num_cus, st);
    PERSIST_CASE(ACT_RELU, false, MASK_NONE)     // conv1 of a ResidualConv
    PERSIST_CASE(ACT_NONE, true, MASK_NONE)      // conv2 + skip ; dgrad(conv1) + dX
    PERSIST_CASE(ACT_LEAKY, false, MASK_NONE)    // conv_last.0
    PERSIST_CASE(ACT_NONE, false, MASK_NONE)     // upsample phases, plain dgrads
    PERSIST_CASE(ACT_NONE, false, MASK_RELU)     // dgrad(conv2) * ReLU'
    PERSIST_CASE(ACT_NONE, false, MASK_RELU_BITS)   // the same, from the sign bits the bias+ReLU launch left (4 MB instead of 66 MB)
    PERSIST_CASE(ACT_NONE, true, MASK_LEAKY)     // (dgrad(conv1 of block 0) + dX) * LeakyReLU' of the stem
    PERSIST_CASE(ACT_NONE, true, MASK_LEAKY_BITS)   // the same with the stem's sign bits (vsr_launch_sign_bits_c64): no late 66 MB mask read
    PERSIST_CASE(ACT_NONE, false, MASK_LEAKY)    // dgrad * LeakyReLU' (discriminator conv_7 / conv_8)
#undef PERSIST_CASE
    return VSR_ERR_UNSUPPORTED;
}

// bits: N * ceil(H/8) * ceil(W/32) * 256 uint2 (the size the engine reserves for a persistent launch's sign_out)
int vsr_launch_sign_bits_c64(const void* x_pm, void* bits, int N, int H, int W, hipStream_t st) {
    if (!x_pm || !bits || N < 1 || H < 1 || W < 1) return VSR_ERR_BADARG;
    const long long total = (long long)N * cdiv(W, PTW) * cdiv(H, PTH) * 256;
    hipLaunchKernelGGL(sign_bits_c64_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const bf16_t*)x_pm, (uint2*)bits, N, H, W);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}
