// The tile core of the 3x3, 64 -> 64 channel bf16 convolution: everything that conv3x3_persist.hip (one layer per launch) and
// conv3x3_chain.hip (a chain of layers per launch) do the same way, defined once.  Device code only.  Both kernels run ONE 512-thread
// workgroup per CU, persistent over 8x32-pixel tiles (one 32-pixel segment of the blocked layout wide, see common.h): 4 MFMA waves + 4
// LDS-DMA producer waves, one of each per SIMD.  What differs between them -- how a tile is chosen, the cache policy of the DMA, the
// output / residual memory operations, the extra epilogue arms of the one-layer kernel, the chain's publish logic -- is in their files.
//
// LDS image (160 KiB per CU):
//   * the packed weights [9 taps][64 cout][64 cin] bf16 (72 KiB) stay in LDS: [tap][cout row][8 chunks of 16 B], XOR-swizzled on the
//     chunk (C64_W_SWIZZLED_BYTE).
//   * the haloed 10x34-pixel input tile is DOUBLE-BUFFERED (2 x 42.5 KiB) and filled by the producer waves' LDS-DMA
//     (global_load_lds_dwordx4) one whole tile ahead.  The pixel image mirrors the blocked global layout, [tile row][chunk][34 pixels]
//     [16 B]: 16 consecutive lanes read 16 consecutive 16-byte slots (conflict-free without a swizzle), a ky shift is an immediate, and
//     a DMA piece reads runs of up to 512 contiguous bytes (a [pixel][chunk] image made every lane of a piece hit a different line:
//     +40 % DMA issue time measured).
//   * 64 fp32 bias values behind the tiles (BIAS_OFF); what a kernel keeps behind them is its own.
//   * K loop: 288 v_mfma_f32_16x16x32_bf16 per MFMA wave and tile, no barrier inside; A (weights) and B (pixels) fragments are
//     ds_read_b128 at register base + immediate, issued by hand one k-step ahead of their MFMAs (inline asm + counted s_waitcnt: hipcc
//     sinks builtin LDS reads back in front of their consumers).
//   * epilogue: the accumulator layout (lane = pixel of the segment, registers = 4 consecutive rows of a 16-row block) IS the blocked
//     global layout once the 64 output channels are dealt to the MFMA rows in "paired-block order" (pm_acc_chan, common.h): lane
//     (pixel i, quarter q) then holds the 8 consecutive channels of chunk 4k + q in the accumulators of blocks 2k and 2k+1, i.e. one
//     whole 16-byte piece of the blocked layout.  Bias / ReLU / residual add / activation-gradient mask are applied in registers and
//     every store (and residual / mask load) is a 16-byte-per-lane wave instruction over four 256-byte runs: 8 stores + 8 loads per
//     wave and tile.  (r03: with 4 channels per lane = 16 + 16 eight-byte instructions, the vector-memory issue path, shared with the
//     producers' 44 DMA pieces per tile, cost 1.2 k cycles per tile for the operand loads alone; with plain [pixel][64 ch] rows the
//     stores hit 32 lines per instruction; an LDS transposition cost 2.7 k cycles per tile.)  ReLU and the sign bits are computed on
//     the PACKED bf16 words (v_pk_max_i16, v_pk_min_u16, v_lshl_or_b32: 1.5 instructions per element instead of 4).
//
// Why so much of this is macros: a register array must not go through a pointer or a reference (it would live in scratch memory), the
// fragment reads need literal immediates, and the machine code of both kernels is sensitive to the order of every address
// computation -- a helper function is optimised on its own before it is inlined, which changed the schedule and the register
// allocation of the kernels wherever it was tried.  The macros keep the statements the two kernels were tuned with.
#pragma once
#include "common.h"

constexpr int PTW = 32, PTH = 8, PNT = 512;                              // tile; 4 MFMA waves + 4 DMA waves
constexpr int PTWH = PTW + 2, PTHH = PTH + 2, PNPIX = PTHH * PTWH;       // 34 x 10 = 340 haloed pixels
constexpr int W_BYTES = 9 * 64 * 64 * 2;                                  // 73,728
constexpr int IN_BYTES = PNPIX * 128;                                     // 43,520 per buffer
constexpr int BIAS_OFF = W_BYTES + 2 * IN_BYTES;                          // 64 fp32 bias values behind the tiles
constexpr int IN_CHUNKS = PNPIX * 8;                                      // 2,720 16-byte chunks
constexpr int NPIECE_T = (IN_CHUNKS + 63) / 64;                           // 43 DMA pieces of 1 KiB (last half full)
constexpr int NPIECE_W = (NPIECE_T + 3) / 4;                              // 11 per wave; wave w4 = 0 always issues exactly 11
constexpr int WCH = 9 * 64 * 8 / 256;                                     // 18 weight chunks per thread of the 256 that stage a set

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;     // a 16-byte piece (native vector: usable behind address-space pointers)
typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
// a pointer kept as an integer comes back with its address space named, or hipcc addresses it with flat_ instructions
#define GP(T, x) ((__attribute__((address_space(1))) T*)(x))

// two fp32 -> one dword of two bf16 (v_cvt_pk_bf16_f32), low half = a
static __device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    bf16x2_t p = {(bf16_t)a, (bf16_t)b};
    return __builtin_bit_cast(unsigned, p);
}
static __device__ __forceinline__ unsigned pk_max_i16(unsigned a, unsigned b) { unsigned r; asm("v_pk_max_i16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
static __device__ __forceinline__ unsigned pk_min_u16(unsigned a, unsigned b) { unsigned r; asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
static __device__ __forceinline__ unsigned pk_mul_lo_u16(unsigned a, unsigned b) { unsigned r; asm("v_pk_mul_lo_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }

// ---- weights: global [tap][cout][cin] -> LDS.  Row r = MFMA row (block r >> 4, row r & 15) holds output channel pm_acc_chan(r >> 4,
// r & 15); chunk c of row r at (r*8 + (c ^ ((r>>1)&7))): the 16 rows a ds_read_b128 pass touches (same chunk, rows 16 mb .. 16 mb + 15)
// then fall on 16 distinct 16-byte bank groups.  256 threads stage a set, 18 chunks each: the loads are issued first, the LDS writes
// when they have returned.
#define C64_W_SWIZZLED_BYTE(r, c) (((r) * 8 + ((c) ^ (((r) >> 1) & 7))) * 16)
// t = the thread's index among the 256 that stage the set, u32x4_t wv[WCH]
#define C64_W_LOAD(wv, wg, t)                                                                                            \
    _Pragma("unroll") for (int i = 0; i < WCH; ++i) {                                                                    \
        const int idx = (t) + i * 256;                                                                                   \
        const int tap = idx >> 9, r = (idx >> 3) & 63, c = idx & 7;                                                      \
        wv[i] = (wg)[(tap * 64 + pm_acc_chan(r >> 4, r & 15)) * 8 + c];                                                  \
    }
#define C64_W_STORE(wv, lds_w, t)                                                                                        \
    _Pragma("unroll") for (int i = 0; i < WCH; ++i) {                                                                    \
        const int idx = (t) + i * 256;                                                                                   \
        const int tap = idx >> 9, r = (idx >> 3) & 63, c = idx & 7;                                                      \
        *reinterpret_cast<u32x4_t*>((lds_w) + tap * 8192 + C64_W_SWIZZLED_BYTE(r, c)) = wv[i];                           \
    }

// ---- producer waves: LDS-DMA of a haloed tile.  DMA pieces of wave w4: piece = w4 + 4 i (64 consecutive 16-byte LDS slots).
// rel[i] = the source BYTE offset of this lane's slot (row ty, chunk c, pixel tx) from the tile origin in the blocked layout (tx0 is a
// multiple of 32: the 32 inner pixels of a row are one global segment, i.e. 512 contiguous bytes per chunk; the halo columns are the
// last / first pixel of the neighbouring segments).  View pixel (ty-1, tx-1) is source pixel (v*in_step + src_o) of an image of WSs
// segments per row: in_step 2 = one pixel-shuffle phase of a twice-as-large tensor (the data gradient of conv3x3 + PixelShuffle).
// C64_DMA_REL fills int rel[NPIECE_W]; the chain kernel's sources are whole images: in_step 1, offsets 0.
#define C64_DMA_REL(rel, w4, lane, in_step, src_oy, src_ox, WSs)                                                         \
    _Pragma("unroll") for (int i = 0; i < NPIECE_W; ++i) {                                                               \
        const int idx = ((w4) + 4 * i) * 64 + (lane);           /* LDS slot = [row ty][chunk c][34 pixels tx] x 16 B */  \
        const int ty = idx / (8 * PTWH), rem = idx - ty * (8 * PTWH);                                                    \
        const int c = rem / PTWH, tx = rem - c * PTWH;                                                                   \
        const int dx = (tx - 1) * (in_step) + (src_ox);                                                                  \
        rel[i] = (((((ty - 1) * (in_step) + (src_oy)) * (WSs) + (dx >> 5)) * 8 + c) * 256 + (dx & 31) * 8) * 2;          \
    }
// AUX: the cache policy bits of the DMA (0 plain, 16 = sc1)
#define C64_GLDS16(src, dst, AUX)                                                                     \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src),            \
                                     (__attribute__((address_space(3))) void*)(dst), 16, 0, AUX)
// The tile at view pixel (ty0, tx0) of an H x W view -> the tile buffer dstb; org = the source address of its origin, zsrc = 16
// zero bytes in global memory (what a pixel outside the view reads).
#define C64_DMA_TILE(AUX, rel, org, zsrc, dstb, w4, lane, ty0, tx0, H, W)                                                \
    if (ty0 >= 1 && ty0 + PTH < (H) && tx0 >= 1 && tx0 + PTW < (W)) {          /* interior tile (wave-uniform) */         \
        _Pragma("unroll") for (int i = 0; i < NPIECE_W; ++i) {                                                           \
            const int piece = (w4) + 4 * i;                                                                              \
            if (piece < NPIECE_T && piece * 64 + (lane) < IN_CHUNKS) C64_GLDS16((org) + rel[i], (dstb) + piece * 1024, AUX); \
        }                                                                                                                \
    } else {                                                                    /* border: bounds per lane, zero source */ \
        _Pragma("unroll") for (int i = 0; i < NPIECE_W; ++i) {                                                           \
            const int piece = (w4) + 4 * i;                                                                              \
            const int idx = piece * 64 + (lane);                                                                         \
            const int ty = idx / (8 * PTWH), rem = idx - ty * (8 * PTWH);                                                \
            const int tx = rem % PTWH;                                                                                   \
            const int vy = ty0 + ty - 1, vx = tx0 + tx - 1;                                                              \
            const auto* s = (vy >= 0 && vy < (H) && vx >= 0 && vx < (W)) ? (org) + rel[i] : (zsrc);                      \
            if (piece < NPIECE_T && idx < IN_CHUNKS) C64_GLDS16(s, (dstb) + piece * 1024, AUX);                          \
        }                                                                                                                \
    }

// ---- MFMA waves: wave w4 computes tile rows 2 w4, 2 w4 + 1.  v_mfma_f32_16x16x32_bf16 (under MFMA load on random data the chip holds
// a higher clock on this shape than on 32x32x16, MI355X_MICROARCH "DVFS give-back" item 7): wave tile = 4 cout blocks x 4 pixel blocks
// (row, half) of 16; a step = one tap x 32 channels = 8 fragment reads (4 A + 4 B, ds_read_b128) + 16 MFMAs.
// Operand lane l = (i = l & 15, q = l >> 4): A[cout 16 mb + i][8 channels 8q..8q+7], B[same 8 channels][pixel pxl = PM_LANE_PIXEL(i)].
// Fragment addresses: A two lane bases per channel half (taps 0-5 / 6-8: the immediate is 16 bits) + immediates (tap, mb); B ONE lane
// base + immediates (row, ky, kx, half, channel half) of the [row][chunk][34 px][16 B] image.
// C64_MFMA_LANE declares them under the names the K loop uses: unsigned a_lo[2], a_hi[2]; int b_lane.
#define C64_MFMA_LANE(w4, l15, q, pxl)                                                                                   \
    unsigned a_lo[2], a_hi[2];                                                                                           \
    _Pragma("unroll") for (int kk = 0; kk < 2; ++kk) {                                                                   \
        a_lo[kk] = (unsigned)C64_W_SWIZZLED_BYTE(l15, 4 * kk + (q));                                                     \
        a_hi[kk] = a_lo[kk] + 6 * 8192;                                                                                  \
    }                                                                                                                    \
    const int b_lane = (w4) * 2 * (PTWH * 128) + (q) * (PTWH * 16) + (pxl) * 16;
// The bias of the wave's 16 rows of block mb (couts pm_acc_chan(mb, 4q + j)), from the LDS slots BIAS_OFF (slot r = the channel MFMA
// row r of the 64 computes).  It stays in registers and is the C operand of every accumulator's first MFMA: no per-tile
// initialisation (64 moves + 4 LDS reads per tile before), and 32 fewer live registers than carrying it per accumulator.
static __device__ __forceinline__ f32x4_t c64_bias_rows(const char* smem, int q, int mb) {
    return *reinterpret_cast<const f32x4_t*>(smem + BIAS_OFF + (mb * 16 + 4 * q) * 4);
}
// The residual is added ON THE MATRIX CORES (r03): the 16-byte residual piece a lane prefetches (chunk 4k + q of its pixel) is exactly
// a B fragment of a K step over the 32 channels of pieces k, and "+ residual" is one more MFMA per accumulator with a 0 / 1 selection
// matrix as A: row r of block mb is channel pm_acc_chan(mb, r) = k group r >> 2, element 4 (mb & 1) + (r & 3) of that step.  16 MFMAs
// (256 cycles) replace 64 unpacks + 64 adds per tile and wave (512 issue cycles); fp32 accumulation of 1.0 x bf16 is the same single
// rounding as the v_add_f32 it replaces.  rr[k][nb] = residual piece k of pixel block nb.
#define C64_RES_IDENTITY(idA, l15, q)                                                                                    \
    bf16x8_t idA[2];                                                                                                     \
    _Pragma("unroll") for (int hb = 0; hb < 2; ++hb)                                                                     \
        _Pragma("unroll") for (int j = 0; j < 8; ++j) idA[hb][j] = (bf16_t)(((q) == ((l15) >> 2) && j == 4 * hb + ((l15) & 3)) ? 1.f : 0.f);
#define C64_ADD_RESIDUAL(acc, idA, rr)                                                                                 \
    _Pragma("unroll") for (int nb = 0; nb < 4; ++nb)                                                                   \
        _Pragma("unroll") for (int mb = 0; mb < 4; ++mb)                                                               \
            acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(idA[mb & 1], __builtin_bit_cast(bf16x8_t, rr[mb >> 1][nb]), acc[mb][nb], 0, 0, 0);

// ---- K loop of one tile: C64_K_LOOP(acc, bvec, cur) with f32x4_t acc[4][4] (first written by step 0's MFMAs, whose C operand is
// the bias bvec[mb]), the lane bases of C64_MFMA_LANE, cur = the tile buffer.  18 steps s = (tap, channel half) of 16 MFMAs.  The 8 fragment
// reads of step s+1 are issued before the MFMAs of step s, by hand (hipcc sinks builtin LDS reads back in front of their consumers):
// one read behind each of the first 8 MFMAs of step s, so that the wave's LDS issue slots sit in the shadow of its own MFMAs and the
// last read has 8 MFMAs (128 cycles) to return before step s+1 starts.  Every offset is an immediate: s is a literal.
#define C64_DSR(dst, addr, imm) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "i"(imm))
#define C64_LOADA(tap_, kk_, slot, mb)                                                                                 \
    C64_DSR(fa_[slot][mb], (tap_ < 6 ? a_lo[kk_] : a_hi[kk_]), (tap_ < 6 ? tap_ : tap_ - 6) * 8192 + (mb) * 2048);
#define C64_LOADB(ky_, kx_, kk_, slot, nb)                                                                             \
    C64_DSR(fb_[slot][nb], bb_, (((nb) >> 1) + ky_) * (PTWH * 128) + kk_ * (4 * PTWH * 16) + (((nb) & 1) * 16 + kx_) * 16);
#define C64_LOAD(s, slot)                                                                                              \
    {                                                                                                                  \
        constexpr int tap_ = (s) / 2, kk_ = (s) % 2, ky_ = tap_ / 3, kx_ = tap_ % 3;                                   \
        C64_LOADA(tap_, kk_, slot, 0) C64_LOADA(tap_, kk_, slot, 1) C64_LOADA(tap_, kk_, slot, 2) C64_LOADA(tap_, kk_, slot, 3) \
        C64_LOADB(ky_, kx_, kk_, slot, 0) C64_LOADB(ky_, kx_, kk_, slot, 1) C64_LOADB(ky_, kx_, kk_, slot, 2) C64_LOADB(ky_, kx_, kk_, slot, 3) \
    }
#define C64_MFMA(acc, bvec, s, mb, nb) acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa_[(s) % 2][mb], fb_[(s) % 2][nb], (s) == 0 ? bvec[mb] : acc[mb][nb], 0, 0, 0);
#define C64_ML_A(acc, bvec, s, mb, nb, lmb)                                                                            \
    C64_MFMA(acc, bvec, s, mb, nb)                                                                                     \
    __builtin_amdgcn_sched_barrier(0);        /* hipcc would otherwise bunch the reads behind the MFMAs */               \
    if ((s) + 1 < 18) { constexpr int t1_ = ((s) + 1) / 2, k1_ = ((s) + 1) % 2; C64_LOADA(t1_, k1_, ((s) + 1) % 2, lmb) } \
    __builtin_amdgcn_sched_barrier(0);
#define C64_ML_B(acc, bvec, s, mb, nb, lnb)                                                                            \
    C64_MFMA(acc, bvec, s, mb, nb)                                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                                                                 \
    if ((s) + 1 < 18) { constexpr int t1_ = ((s) + 1) / 2, k1_ = ((s) + 1) % 2; C64_LOADB(t1_ / 3, t1_ % 3, k1_, ((s) + 1) % 2, lnb) } \
    __builtin_amdgcn_sched_barrier(0);
#define C64_STEP(acc, bvec, s)                                                                                         \
    {                                                                                                                  \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      /* step s is in registers */                           \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        C64_ML_A(acc, bvec, s, 0, 0, 0) C64_ML_A(acc, bvec, s, 0, 1, 1) C64_ML_A(acc, bvec, s, 0, 2, 2) C64_ML_A(acc, bvec, s, 0, 3, 3) \
        C64_ML_B(acc, bvec, s, 1, 0, 0) C64_ML_B(acc, bvec, s, 1, 1, 1) C64_ML_B(acc, bvec, s, 1, 2, 2) C64_ML_B(acc, bvec, s, 1, 3, 3) \
        C64_MFMA(acc, bvec, s, 2, 0) C64_MFMA(acc, bvec, s, 2, 1) C64_MFMA(acc, bvec, s, 2, 2) C64_MFMA(acc, bvec, s, 2, 3)  \
        C64_MFMA(acc, bvec, s, 3, 0) C64_MFMA(acc, bvec, s, 3, 1) C64_MFMA(acc, bvec, s, 3, 2) C64_MFMA(acc, bvec, s, 3, 3)  \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
    }
#define C64_K_LOOP(acc, bvec, cur)                                                                                                    \
    {                                                                                                                  \
        bf16x8_t fa_[2][4], fb_[2][4];                                                                                 \
        const unsigned bb_ = (unsigned)(W_BYTES + (cur) * IN_BYTES + (b_lane));   /* B base of this tile's buffer */   \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      /* nothing of ours is outstanding */                   \
        __builtin_amdgcn_sched_barrier(0);                                                                             \
        C64_LOAD(0, 0)                                                                                                 \
        C64_STEP(acc, bvec, 0) C64_STEP(acc, bvec, 1) C64_STEP(acc, bvec, 2) C64_STEP(acc, bvec, 3) C64_STEP(acc, bvec, 4) C64_STEP(acc, bvec, 5) \
        C64_STEP(acc, bvec, 6) C64_STEP(acc, bvec, 7) C64_STEP(acc, bvec, 8) C64_STEP(acc, bvec, 9) C64_STEP(acc, bvec, 10) C64_STEP(acc, bvec, 11) \
        C64_STEP(acc, bvec, 12) C64_STEP(acc, bvec, 13) C64_STEP(acc, bvec, 14) C64_STEP(acc, bvec, 15) C64_STEP(acc, bvec, 16) C64_STEP(acc, bvec, 17) \
    }

// ---- epilogue arms on the packed words.  A lane's piece (k, nb) = float v[8] = the accumulators acc[2k][nb], acc[2k+1][nb] = channels
// 8 (4k + q) + 0..7 of pixel (row 2 w4 + (nb >> 1), column 16 (nb & 1) + pxl): chunk 4k + q of the blocked layout, whole; its packed
// word ow[jj] = channels 2jj, 2jj+1.  Sign bits of the tile: the lane's 64 outputs are 32 packed words wd = (4k + nb) * 4 + jj; word
// wd owns bits (wd & 15) [even channel] and 16 + (wd & 15) [odd channel] of the lane's sign word k.
constexpr unsigned C64_K11 = 0x00010001u;
#define C64_ARM_PLAIN(ow, v)                                                                                             \
    _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) ow[jj] = pk_bf16(v[2 * jj], v[2 * jj + 1]);
// conv1 of a ResidualConv: round, then ReLU on the packed words (bf16 bit patterns order like int16 for this purpose: negative and
// -0 -> +0); sign bit = "the stored half is non-zero", OR-ed into sign_k = the lane's sign word k
#define C64_ARM_RELU(ow, v, nb, sign_k)                                                                                  \
    _Pragma("unroll") for (int jj = 0; jj < 4; ++jj) {                                                                   \
        ow[jj] = pk_max_i16(pk_bf16(v[2 * jj], v[2 * jj + 1]), 0u);                                                      \
        sign_k |= pk_min_u16(ow[jj], C64_K11) << (4 * (nb) + jj);                                                        \
    }
// dgrad(conv2) * ReLU': multiply the packed halves by their 0 / 1 bits of the lane's sign word k
#define C64_ARM_MASKED(ow, v, nb, wbits)                                                                                 \
    _Pragma("unroll") for (int jj = 0; jj < 4; ++jj)                                                                     \
        ow[jj] = pk_mul_lo_u16(pk_bf16(v[2 * jj], v[2 * jj + 1]), ((wbits) >> (4 * (nb) + jj)) & C64_K11);
// The 8 bytes of sign bits of (tile, MFMA wave w4, lane): [tile][wave][lane] x 64 bits.  Every kernel that writes or reads them uses
// this tile decomposition, the paired-block channel order and PM_LANE_PIXEL.
static __device__ __forceinline__ long long c64_sign_word(int tile, int w4, int lane) { return (long long)tile * 256 + w4 * 64 + lane; }
