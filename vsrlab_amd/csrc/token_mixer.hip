// The DCT-token MLP-Mixer of the reference's core/modules (dct_transforms.py: EncoderDCT / DecoderIDCT; mlp.py: Mlp / MixerBlock /
// MlpMixer).  DESIGN section 11j is the specification.  Built into a library of its own, libvsrlab_mixer.so
// (include/vsrlab_mixer.h): libvsrlab_hip.so's exports stay as they are.
//
//   block_dct_kernel / block_idct_kernel:  the grouped stride-ps convolution and its transpose, between planar frames (N, C, H, W)
//       and tokens (N, P, C ps^2).  A workgroup owns one block row of one image and a run of `tw` pixels of it, all C channels.  The
//       planar side moves as row segments of tw pixels (lanes along the row), the token side as ONE contiguous span of (tw / ps) C ps^2
//       values (lanes along the span); LDS lies between them, as in cl_stage.h, whose [pixel][channel] tile this replaces by
//       [channel row][pixel] because a token mixes ps x ps pixels.  A thread owns one coefficient (forward) or one pixel position of
//       the block (inverse) of one channel, keeps its ps^2 weights in registers and walks the tile's blocks.
//   axis_mlp_kernel:  y = x + W2 gelu(W1 x + b1) + b2 along the middle axis of an (outer, D, inner) view, and (BWD) the gradient
//       w.r.t. x from a recomputed hidden vector.  A lane works on one (o, i) position: its D inputs and D accumulators are registers;
//       the weights pass through LDS in chunks of 32 hidden units and are read as broadcasts (every lane the same 16 bytes).
//       inner == 1 (STAGED): the workgroup's tokens are one contiguous span, moved to and from LDS by whole-line accesses and read
//       by each lane at the odd stride DMAX + 1.  Otherwise lanes run along inner.  Four lanes share a position and take every
//       fourth hidden unit each, so that a channel axis of a few thousand tokens still fills the chip.
//   axis_mlp_wgrad_kernel + axis_mlp_wreduce_kernel:  the weight gradients.  64 positions at a time are staged transposed in LDS (x,
//       dy, recomputed gelu(h) and dh, 32 hidden units per chunk); a thread owns a fixed 4 x 4 tile of (d, j) entries of dW1 and of
//       dW2 and adds the positions to it in index order over every tile its workgroup walks; one partial set per workgroup, added
//       in workgroup order by the second launch.  No atomics: bit-identical from run to run.
#include "elt.h"
#include "host.h"
#include "../../include/vsrlab_mixer.h"

namespace {

// ---- block transform ---------------------------------------------------------------------------------------------------------------
constexpr int BD_BLOCK = 256;
constexpr int BD_LDS = 6144;                    // floats of one tile: (C ps) channel rows x tw pixels = (tw / ps) tokens x C ps^2
constexpr int BD_MAXCK = 256;                   // C ps^2 at most: one thread per coefficient of a token

// the run of pixels a workgroup owns: a multiple of 32 (so of ps), as long as the tile fits, 32 at least (C ps <= 128: 4096 floats)
inline int bd_tile_width(int C, int ps) {
    int tw = (BD_LDS / (C * ps)) & ~31;
    return tw > 256 ? 256 : (tw < 32 ? 32 : tw);
}

struct BdTile { int n, bi, col0, wv; bool last; };
// workgroup -> (image, block row, first pixel column, valid pixels of the run: a multiple of ps)
static __device__ __forceinline__ BdTile bd_tile(int rows_y, int tiles_x, int tw, int BW, int ps) {
    BdTile t;
    int b = blockIdx.x;
    const int tx = b % tiles_x;
    b /= tiles_x;
    t.bi = b % rows_y;
    t.n = b / rows_y;
    t.col0 = tx * tw;
    t.wv = min(tw, BW * ps - t.col0);
    t.last = tx == tiles_x - 1;
    return t;
}

template <typename T, int PS>
__global__ __launch_bounds__(BD_BLOCK) void block_dct_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y, int C,
                                                             int H, int W, int BH, int BW, int tw, int tiles_x) {
    constexpr int K = PS * PS;
    __shared__ float in[BD_LDS];                                      // [c PS + i][tw]
    const int t = threadIdx.x, CK = C * K, rows = C * PS;
    const BdTile tl = bd_tile(BH, tiles_x, tw, BW, PS);
    for (int idx = t; idx < rows * tl.wv; idx += BD_BLOCK) {          // lanes along the pixel row
        const int r = idx / tl.wv, col = idx - r * tl.wv, c = r / PS, i = r - c * PS;
        in[r * tw + col] = to_f(x[(((long long)tl.n * C + c) * H + tl.bi * PS + i) * W + tl.col0 + col]);
    }
    __syncthreads();
    const int per = BD_BLOCK / CK, nb = tl.wv / PS;                   // blocks in flight; blocks of the tile
    if (t >= per * CK) return;
    const int ck = t % CK, c = ck / K;
    float wr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wr[k] = w[ck * K + k];
    T* out = y + (((long long)tl.n * BH + tl.bi) * BW + tl.col0 / PS) * CK;       // the tile's tokens: one contiguous span
    for (int bl = t / CK; bl < nb; bl += per) {
        const float* src = in + c * PS * tw + bl * PS;
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < PS; ++i)
#pragma unroll
            for (int j = 0; j < PS; ++j) acc = fmaf(wr[i * PS + j], src[i * tw + j], acc);
        out[bl * CK + ck] = (T)acc;                                   // lanes along the span: bl CK + ck = t + (trip) per CK
    }
}

template <typename T, int PS>
__global__ __launch_bounds__(BD_BLOCK) void block_idct_kernel(const T* __restrict__ y, const float* __restrict__ w, T* __restrict__ x, int C,
                                                              int H, int W, int BH, int BW, int tw, int tiles_x) {
    constexpr int K = PS * PS;
    __shared__ float tok[BD_LDS];                                     // [block][C K]
    __shared__ float out[BD_LDS + BD_MAXCK];                          // [c PS + i][tw + PS]: lanes (i, j) of one block on PS^2 distinct banks
    const int t = threadIdx.x, CK = C * K, ld = tw + PS;
    const int rows_y = BH + (H > BH * PS ? 1 : 0);                    // one more row of workgroups zero-fills the remainder rows
    const BdTile tl = bd_tile(rows_y, tiles_x, tw, BW, PS);
    const bool real = tl.bi < BH;                                     // uniform over the workgroup
    if (real) {
        const int nb = tl.wv / PS;
        const T* src = y + (((long long)tl.n * BH + tl.bi) * BW + tl.col0 / PS) * CK;
        for (int idx = t; idx < nb * CK; idx += BD_BLOCK) tok[idx] = to_f(src[idx]);
        __syncthreads();
        const int per = BD_BLOCK / CK;
        if (t < per * CK) {
            const int pk = t % CK, c = pk / K, ij = pk - c * K, i = ij / PS, j = ij - i * PS;
            float wr[K];
#pragma unroll
            for (int k = 0; k < K; ++k) wr[k] = w[(c * K + k) * K + ij];
            for (int bl = t / CK; bl < nb; bl += per) {
                const float* s = tok + bl * CK + c * K;
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) acc = fmaf(s[k], wr[k], acc);
                out[(c * PS + i) * ld + bl * PS + j] = acc;
            }
        }
        __syncthreads();
    }
    // the planar side, lanes along the pixel row; the last run of a row also writes the remainder columns (zeros)
    const int nri = real ? PS : H - BH * PS, wext = tl.last ? W - tl.col0 : tl.wv;
    for (int idx = t; idx < C * nri * wext; idx += BD_BLOCK) {
        const int r = idx / wext, col = idx - r * wext, c = r / nri, i = r - c * nri;
        const float v = (real && col < tl.wv) ? out[(c * PS + i) * ld + col] : 0.f;
        x[(((long long)tl.n * C + c) * H + tl.bi * PS + i) * W + tl.col0 + col] = (T)v;
    }
}

// ---- residual MLP along one axis -----------------------------------------------------------------------------------------------------
constexpr int AM_BLOCK = 128;                   // lanes of a workgroup of axis_mlp_kernel: AM_BLOCK / AM_SPLIT positions
constexpr int AM_JC = 32;                       // hidden units per LDS weight chunk
constexpr int AM_SPLIT = 4;                     // lanes per position (the shuffles of axis_mlp_kernel are written for 4)
constexpr int WG_BLOCK = 256, WG_POS = 64;      // axis_mlp_wgrad_kernel: threads, positions per staged tile
constexpr int WG_MAX = 256;                     // at most this many workgroups and partial sets

static __device__ __forceinline__ float gelu_f(float h) { return 0.5f * h * (1.f + erff(h * 0.70710678118654752f)); }
static __device__ __forceinline__ float gelu_grad_f(float h) {
    return 0.5f * (1.f + erff(h * 0.70710678118654752f)) + h * 0.39894228040143268f * expf(-0.5f * h * h);
}

// hidden units j0 .. j0 + AM_JC - 1 into LDS: w1s[jl][d] = W1[j][d], w2s[jl][d] = W2[d][j], zero where j >= hidden or d >= D, so that
// the padded lanes of a dot product add nothing and a hidden unit past the end has h = 0, gelu(h) = 0 and dh = 0
template <int DMAX, int NT>
static __device__ __forceinline__ void am_load_chunk(float* w1s, float* w2s, float* b1s, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, int j0, int D, int hidden) {
    for (int e = threadIdx.x; e < AM_JC * DMAX; e += NT) {
        const int jl = e / DMAX, d = e - jl * DMAX, j = j0 + jl;
        const bool ok = j < hidden && d < D;
        w1s[e] = ok ? w1[j * D + d] : 0.f;
        w2s[e] = ok ? w2[d * hidden + j] : 0.f;
    }
    if (threadIdx.x < AM_JC) b1s[threadIdx.x] = j0 + (int)threadIdx.x < hidden ? b1[j0 + threadIdx.x] : 0.f;
}

// row . v over DMAX entries, the row read as 16-byte LDS broadcasts; four partial sums keep four FMA chains in flight
template <int DMAX>
static __device__ __forceinline__ float am_dot(const float* row, const float* v) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d4 = 0; d4 < DMAX / 4; ++d4) {
        const float4 r = reinterpret_cast<const float4*>(row)[d4];
        s[d4 & 3] = fmaf(r.x, v[4 * d4], s[d4 & 3]);
        s[d4 & 3] = fmaf(r.y, v[4 * d4 + 1], s[d4 & 3]);
        s[d4 & 3] = fmaf(r.z, v[4 * d4 + 2], s[d4 & 3]);
        s[d4 & 3] = fmaf(r.w, v[4 * d4 + 3], s[d4 & 3]);
    }
    return (s[0] + s[1]) + (s[2] + s[3]);
}
// acc += row * a
template <int DMAX>
static __device__ __forceinline__ void am_axpy(const float* row, float a, float* acc) {
#pragma unroll
    for (int d4 = 0; d4 < DMAX / 4; ++d4) {
        const float4 r = reinterpret_cast<const float4*>(row)[d4];
        acc[4 * d4] = fmaf(r.x, a, acc[4 * d4]);
        acc[4 * d4 + 1] = fmaf(r.y, a, acc[4 * d4 + 1]);
        acc[4 * d4 + 2] = fmaf(r.z, a, acc[4 * d4 + 2]);
        acc[4 * d4 + 3] = fmaf(r.w, a, acc[4 * d4 + 3]);
    }
}

// forward: out = (sum_j W2[:, j] gelu(h_j)) + (b2 + r x);  BWD: out = r dy + sum_j W1[j, :] (gelu'(h_j) W2[:, j] . dy)
// AM_SPLIT = 4 lanes share a position: lane `part` of them takes the hidden units part, part + 4, ... of every chunk, and the partial
// accumulators are added across the lanes (xor 1, then xor 2: every lane the same sum in the same order).  Few positions (a channel
// axis has numel / D of them) then still fill the chip; with many, the shuffles are 2 D adds beside 2 D hidden / 4 FMAs.
template <typename T, int DMAX, bool BWD, bool STAGED>
__global__ __launch_bounds__(AM_BLOCK) void axis_mlp_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ w1,
                                                            const float* __restrict__ b1, const float* __restrict__ w2,
                                                            const float* __restrict__ b2, T* __restrict__ out, long long Q, int D,
                                                            long long inner, int hidden, int residual) {
    constexpr int S = DMAX + 1;                                       // odd: lanes of a wave read their tokens from distinct banks
    __shared__ __attribute__((aligned(16))) float w1s[AM_JC * DMAX];
    __shared__ __attribute__((aligned(16))) float w2s[AM_JC * DMAX];
    __shared__ float b1s[AM_JC];
    constexpr int SPLIT = AM_SPLIT, TPW = AM_BLOCK / SPLIT;           // positions of a workgroup
    __shared__ float stage[STAGED ? (BWD ? 2 : 1) * TPW * S : 1];
    const int t = threadIdx.x, tp = t / SPLIT, part = t % SPLIT;
    const long long q0 = (long long)blockIdx.x * TPW, q = q0 + tp;
    const bool live = q < Q;
    const long long left = Q - q0;
    const int span = (int)(left < TPW ? left : TPW) * D;              // STAGED: the workgroup's tokens are elements q0 D .. q0 D + span - 1
    float xr[DMAX], gr[BWD ? DMAX : 1], acc[DMAX];
    long long base = 0;
    if (STAGED) {
        for (int e = t; e < span; e += AM_BLOCK) {
            const int tk = e / D, d = e - tk * D;
            stage[tk * S + d] = to_f(x[q0 * D + e]);
            if (BWD) stage[TPW * S + tk * S + d] = to_f(dy[q0 * D + e]);
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
            xr[d] = d < D ? stage[tp * S + d] : 0.f;                  // a lane past Q reads what nobody wrote and stores nothing
            if (BWD) gr[d] = d < D ? stage[TPW * S + tp * S + d] : 0.f;
        }
    } else {
        const long long o = live ? q / inner : 0;
        base = live ? o * D * inner + (q - o * inner) : 0;
#pragma unroll
        for (int d = 0; d < DMAX; ++d) {
            const bool ok = live && d < D;
            xr[d] = ok ? to_f(x[base + d * inner]) : 0.f;
            if (BWD) gr[d] = ok ? to_f(dy[base + d * inner]) : 0.f;
        }
    }
#pragma unroll
    for (int d = 0; d < DMAX; ++d) acc[d] = 0.f;

    for (int j0 = 0; j0 < hidden; j0 += AM_JC) {
        __syncthreads();                                              // the previous chunk has been read
        am_load_chunk<DMAX, AM_BLOCK>(w1s, w2s, b1s, w1, b1, w2, j0, D, hidden);
        __syncthreads();
        const int jn = min(AM_JC, hidden - j0);
        for (int jl = part; jl < jn; jl += SPLIT) {
            const float h = b1s[jl] + am_dot<DMAX>(w1s + jl * DMAX, xr);
            if (BWD) {
                const float dh = am_dot<DMAX>(w2s + jl * DMAX, gr) * gelu_grad_f(h);
                am_axpy<DMAX>(w1s + jl * DMAX, dh, acc);
            } else {
                am_axpy<DMAX>(w2s + jl * DMAX, gelu_f(h), acc);
            }
        }
    }

    const float* res = BWD ? gr : xr;
#pragma unroll
    for (int d = 0; d < DMAX; ++d) {
        acc[d] += __shfl_xor(acc[d], 1, 64);
        acc[d] += __shfl_xor(acc[d], 2, 64);
        if (d < D) acc[d] += (BWD ? 0.f : b2[d]) + (residual ? res[d] : 0.f);
    }
    if (STAGED) {
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
            if (d < D && part == 0) stage[tp * S + d] = acc[d];       // the position's own slot
        __syncthreads();
        for (int e = t; e < span; e += AM_BLOCK) {
            const int tk = e / D, d = e - tk * D;
            out[q0 * D + e] = (T)stage[tk * S + d];
        }
    } else if (live && part == 0) {
#pragma unroll
        for (int d = 0; d < DMAX; ++d)
            if (d < D) out[base + d * inner] = (T)acc[d];
    }
}

// One partial set per workgroup: [dW1 (hidden, D)][db1 (hidden)][dW2 (D, hidden)][db2 (D)].
template <typename T, int DMAX>
__global__ __launch_bounds__(WG_BLOCK) void axis_mlp_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, const float* __restrict__ w1,
                                                                  const float* __restrict__ b1, const float* __restrict__ w2,
                                                                  float* __restrict__ partial, long long Q, int D, long long inner, int hidden,
                                                                  long long ntiles, int E) {
    constexpr int DT = DMAX / 4, JT = AM_JC / 4, NOWN = DT * JT;      // 4 x 4 tiles of (d, j); NOWN <= 96 owner threads
    __shared__ __attribute__((aligned(16))) float w1s[AM_JC * DMAX];
    __shared__ __attribute__((aligned(16))) float w2s[AM_JC * DMAX];
    __shared__ float b1s[AM_JC];
    __shared__ __attribute__((aligned(16))) float xt[DMAX * WG_POS];  // [d][position]: staged, computed and accumulated without a bank conflict
    __shared__ __attribute__((aligned(16))) float dyt[DMAX * WG_POS];
    __shared__ __attribute__((aligned(16))) float gt[AM_JC * WG_POS];  // gelu(h_j)
    __shared__ __attribute__((aligned(16))) float dht[AM_JC * WG_POS]; // dh_j
    const int t = threadIdx.x, pl = t & (WG_POS - 1), jg = t / WG_POS;            // compute phase: position, group of 8 hidden units
    const bool owner = t < NOWN;
    const int dt = t % DT, jt = t / DT;                               // accumulate phase: the thread's tile
    float* mine = partial + (long long)blockIdx.x * E;
    const int DH = D * hidden;

    for (int j0 = 0; j0 < hidden; j0 += AM_JC) {
        // (the last reader of the previous chunk's weights was the compute phase, two barriers back)
        am_load_chunk<DMAX, WG_BLOCK>(w1s, w2s, b1s, w1, b1, w2, j0, D, hidden);
        float a1[4][4], a2[4][4], ab1[4], ab2[4];                     // a1[b][a]: dW1[j0 + 4 jt + b][4 dt + a]; a2[a][b]: dW2[4 dt + a][j0 + 4 jt + b]
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            ab1[a] = 0.f; ab2[a] = 0.f;
#pragma unroll
            for (int b = 0; b < 4; ++b) { a1[a][b] = 0.f; a2[a][b] = 0.f; }
        }
        for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
            __syncthreads();                                          // the previous tile has been accumulated; the weights are there
            const long long q0 = tile * WG_POS;
            for (int idx = t; idx < DMAX * WG_POS; idx += WG_BLOCK) {
                const int d = idx / WG_POS, p = idx - d * WG_POS;
                const long long q = q0 + p;
                const bool ok = q < Q && d < D;
                const long long o = ok ? q / inner : 0, at = ok ? o * D * inner + d * inner + (q - o * inner) : 0;
                xt[idx] = ok ? to_f(x[at]) : 0.f;                     // a position past Q: x = dy = 0, so dh = 0 and every term it adds is 0
                dyt[idx] = ok ? to_f(dy[at]) : 0.f;
            }
            __syncthreads();
            {
                float xr[DMAX], gr[DMAX];
#pragma unroll
                for (int d = 0; d < DMAX; ++d) { xr[d] = xt[d * WG_POS + pl]; gr[d] = dyt[d * WG_POS + pl]; }
#pragma unroll 2
                for (int u = 0; u < AM_JC / 4; ++u) {
                    const int jl = jg * (AM_JC / 4) + u;
                    const float h = b1s[jl] + am_dot<DMAX>(w1s + jl * DMAX, xr);
                    gt[jl * WG_POS + pl] = gelu_f(h);
                    dht[jl * WG_POS + pl] = am_dot<DMAX>(w2s + jl * DMAX, gr) * gelu_grad_f(h);
                }
            }
            __syncthreads();
            if (owner) {
                for (int p = 0; p < WG_POS; p += 4) {
                    float xv[4][4], dv[4][4], gv[4][4], hv[4][4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const float4 v0 = *reinterpret_cast<const float4*>(xt + (4 * dt + a) * WG_POS + p);
                        const float4 v1 = *reinterpret_cast<const float4*>(dyt + (4 * dt + a) * WG_POS + p);
                        const float4 v2 = *reinterpret_cast<const float4*>(gt + (4 * jt + a) * WG_POS + p);
                        const float4 v3 = *reinterpret_cast<const float4*>(dht + (4 * jt + a) * WG_POS + p);
                        xv[a][0] = v0.x; xv[a][1] = v0.y; xv[a][2] = v0.z; xv[a][3] = v0.w;
                        dv[a][0] = v1.x; dv[a][1] = v1.y; dv[a][2] = v1.z; dv[a][3] = v1.w;
                        gv[a][0] = v2.x; gv[a][1] = v2.y; gv[a][2] = v2.z; gv[a][3] = v2.w;
                        hv[a][0] = v3.x; hv[a][1] = v3.y; hv[a][2] = v3.z; hv[a][3] = v3.w;
                    }
#pragma unroll
                    for (int pp = 0; pp < 4; ++pp)                    // positions in index order
#pragma unroll
                        for (int a = 0; a < 4; ++a) {
                            ab1[a] += hv[a][pp];
                            ab2[a] += dv[a][pp];
#pragma unroll
                            for (int b = 0; b < 4; ++b) {
                                a1[b][a] = fmaf(hv[b][pp], xv[a][pp], a1[b][a]);
                                a2[a][b] = fmaf(dv[a][pp], gv[b][pp], a2[a][b]);
                            }
                        }
                }
            }
        }
        if (owner) {
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const int d = 4 * dt + a, ja = j0 + 4 * jt + a;
                if (dt == 0 && ja < hidden) mine[DH + ja] = ab1[a];
                if (jt == 0 && j0 == 0 && d < D) mine[2 * DH + hidden + d] = ab2[a];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int j = j0 + 4 * jt + b;
                    if (d < D && j < hidden) {
                        mine[j * D + d] = a1[b][a];
                        mine[DH + hidden + d * hidden + j] = a2[a][b];
                    }
                }
            }
        }
    }
}

// the partial sets added in workgroup order; a thread per entry
__global__ __launch_bounds__(256) void axis_mlp_wreduce_kernel(const float* __restrict__ partial, int nwg, int E, int D, int hidden,
                                                               float* __restrict__ dw1, float* __restrict__ db1, float* __restrict__ dw2,
                                                               float* __restrict__ db2) {
    const int e = blockIdx.x * 256 + threadIdx.x, DH = D * hidden;
    if (e >= E) return;
    float s = 0.f;
    for (int g = 0; g < nwg; ++g) s += partial[(long long)g * E + e];
    if (e < DH) dw1[e] = s;
    else if (e < DH + hidden) db1[e - DH] = s;
    else if (e < 2 * DH + hidden) dw2[e - DH - hidden] = s;
    else db2[e - 2 * DH - hidden] = s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

// the checks of both block-transform entries; *grid: the workgroups of the launch (rows_extra: the inverse's zero-fill row)
int bd_check(const VsrBlockDctDesc* d, const void* planar, const float* w, const void* tokens, bool rows_extra, int* tw, int* tiles_x, int* grid) {
    if (!d || !planar || !w || !tokens) return VSR_ERR_BADARG;
    if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1 || d->ps < 1 || bad_dtype(d->dtype)) return VSR_ERR_BADARG;
    if (misaligned(planar, esize(d->dtype)) || misaligned(tokens, esize(d->dtype)) || misaligned(w, 4)) return VSR_ERR_BADARG;
    if (d->ps != 2 && d->ps != 4 && d->ps != 8) return VSR_ERR_UNSUPPORTED;
    if (d->C > BD_MAXCK / (d->ps * d->ps)) return VSR_ERR_UNSUPPORTED;
    const int BH = d->H / d->ps, BW = d->W / d->ps;
    if (BH < 1 || BW < 1) return VSR_ERR_UNSUPPORTED;
    long long px, el;
    if (__builtin_mul_overflow((long long)d->H, (long long)d->W, &px) || __builtin_mul_overflow(px, (long long)d->C, &el) ||
        __builtin_mul_overflow(el, (long long)d->N, &el))
        return VSR_ERR_UNSUPPORTED;
    *tw = bd_tile_width(d->C, d->ps);
    *tiles_x = cdiv(BW * d->ps, *tw);
    const long long wgs = (long long)d->N * (BH + (rows_extra && d->H > BH * d->ps ? 1 : 0)) * *tiles_x;
    if (wgs > 0x7fffffffLL) return VSR_ERR_UNSUPPORTED;
    *grid = (int)wgs;
    return VSR_OK;
}

template <typename T>
void bd_launch(bool inverse, const VsrBlockDctDesc* d, const void* src, const float* w, void* dst, int tw, int tiles_x, int grid, hipStream_t st) {
    const int BH = d->H / d->ps, BW = d->W / d->ps;
#define BD_GO(PS)                                                                                                                             \
    if (inverse)                                                                                                                              \
        hipLaunchKernelGGL((block_idct_kernel<T, PS>), dim3(grid), dim3(BD_BLOCK), 0, st, static_cast<const T*>(src), w, static_cast<T*>(dst), \
                           d->C, d->H, d->W, BH, BW, tw, tiles_x);                                                                            \
    else                                                                                                                                      \
        hipLaunchKernelGGL((block_dct_kernel<T, PS>), dim3(grid), dim3(BD_BLOCK), 0, st, static_cast<const T*>(src), w, static_cast<T*>(dst),  \
                           d->C, d->H, d->W, BH, BW, tw, tiles_x)
    if (d->ps == 2) { BD_GO(2); }
    else if (d->ps == 4) { BD_GO(4); }
    else { BD_GO(8); }
#undef BD_GO
}

int bd_run(bool inverse, const VsrBlockDctDesc* d, const void* src, const float* w, void* dst, void* stream) {
    int tw = 0, tiles_x = 0, grid = 0;
    CK(inverse ? bd_check(d, dst, w, src, true, &tw, &tiles_x, &grid) : bd_check(d, src, w, dst, false, &tw, &tiles_x, &grid));
    if (d->dtype == VSR_BF16) bd_launch<bf16_t>(inverse, d, src, w, dst, tw, tiles_x, grid, (hipStream_t)stream);
    else bd_launch<float>(inverse, d, src, w, dst, tw, tiles_x, grid, (hipStream_t)stream);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

// what makes a desc malformed (BADARG) and what puts it outside the fused path (UNSUPPORTED); *Q: the positions outer * inner
int am_check_desc(const VsrAxisMlpDesc* d, long long* Q) {
    if (!d) return VSR_ERR_BADARG;
    if (d->outer < 1 || d->D < 1 || d->inner < 1 || d->hidden < 1 || bad_dtype(d->dtype)) return VSR_ERR_BADARG;
    if (d->D > VSR_AXIS_MLP_MAX_D || d->hidden > VSR_AXIS_MLP_MAX_HIDDEN) return VSR_ERR_UNSUPPORTED;
    long long el;
    if (__builtin_mul_overflow(d->outer, d->inner, Q) || __builtin_mul_overflow(*Q, (long long)d->D, &el)) return VSR_ERR_UNSUPPORTED;
    if ((*Q + AM_BLOCK / AM_SPLIT - 1) / (AM_BLOCK / AM_SPLIT) > 0x7fffffffLL) return VSR_ERR_UNSUPPORTED;
    return VSR_OK;
}

inline int am_entries(const VsrAxisMlpDesc* d) { return 2 * d->D * d->hidden + d->hidden + d->D; }
inline int am_wgrad_wgs(long long Q) {
    const long long tiles = (Q + WG_POS - 1) / WG_POS;
    return (int)(tiles < WG_MAX ? tiles : WG_MAX);
}

template <typename T, int DMAX>
void am_launch(bool bwd, const VsrAxisMlpDesc* d, long long Q, const void* x, const void* dy, const float* w1, const float* b1, const float* w2,
               const float* b2, void* out, hipStream_t st) {
    const int tpw = AM_BLOCK / AM_SPLIT;
    const dim3 grid((unsigned)((Q + tpw - 1) / tpw)), block(AM_BLOCK);
    const T *xp = static_cast<const T*>(x), *gp = static_cast<const T*>(dy);
    T* op = static_cast<T*>(out);
#define AM_GO(BWD, STAGED) \
    hipLaunchKernelGGL((axis_mlp_kernel<T, DMAX, BWD, STAGED>), grid, block, 0, st, xp, gp, w1, b1, w2, b2, op, Q, d->D, d->inner, d->hidden, d->residual)
    if (d->inner == 1) { if (bwd) AM_GO(true, true); else AM_GO(false, true); }
    else { if (bwd) AM_GO(true, false); else AM_GO(false, false); }
#undef AM_GO
}

template <typename T, int DMAX>
void am_launch_wgrad(const VsrAxisMlpDesc* d, long long Q, const void* x, const void* dy, const float* w1, const float* b1, const float* w2,
                     float* partial, hipStream_t st) {
    hipLaunchKernelGGL((axis_mlp_wgrad_kernel<T, DMAX>), dim3(am_wgrad_wgs(Q)), dim3(WG_BLOCK), 0, st, static_cast<const T*>(x),
                       static_cast<const T*>(dy), w1, b1, w2, partial, Q, d->D, d->inner, d->hidden, (Q + WG_POS - 1) / WG_POS, am_entries(d));
}

// the register width of a lane: D rounded up to one of the instantiated sizes
#define AM_DISPATCH(T, CALL)                         \
    do {                                             \
        if (d->D <= 8) CALL(T, 8);                   \
        else if (d->D <= 16) CALL(T, 16);            \
        else if (d->D <= 32) CALL(T, 32);            \
        else CALL(T, 48);                            \
    } while (0)

}  // namespace

extern "C" {

int vsr_block_dct_fwd(const VsrBlockDctDesc* desc, const void* x, const float* w, void* y, void* stream) {
    return bd_run(false, desc, x, w, y, stream);
}

int vsr_block_idct_fwd(const VsrBlockDctDesc* desc, const void* y, const float* w, void* x, void* stream) {
    return bd_run(true, desc, y, w, x, stream);
}

int vsr_axis_mlp_supported(const VsrAxisMlpDesc* desc) {
    long long Q;
    return am_check_desc(desc, &Q) == VSR_OK ? 1 : 0;
}

size_t vsr_axis_mlp_scratch_bytes(const VsrAxisMlpDesc* desc) {
    long long Q;
    if (am_check_desc(desc, &Q) != VSR_OK) return 0;
    return (size_t)am_wgrad_wgs(Q) * am_entries(desc) * sizeof(float);
}

int vsr_axis_mlp_fwd(const VsrAxisMlpDesc* d, const void* x, const float* w1, const float* b1, const float* w2, const float* b2, void* y,
                     void* stream) {
    if (!d || !x || !w1 || !b1 || !w2 || !b2 || !y) return VSR_ERR_BADARG;
    long long Q;
    CK(am_check_desc(d, &Q));
    if (misaligned(x, esize(d->dtype)) || misaligned(y, esize(d->dtype)) || misaligned(w1, 4) || misaligned(b1, 4) || misaligned(w2, 4) ||
        misaligned(b2, 4))
        return VSR_ERR_BADARG;
    hipStream_t st = (hipStream_t)stream;
#define AM_FWD(T, DMAX) am_launch<T, DMAX>(false, d, Q, x, nullptr, w1, b1, w2, b2, y, st)
    if (d->dtype == VSR_BF16) AM_DISPATCH(bf16_t, AM_FWD);
    else AM_DISPATCH(float, AM_FWD);
#undef AM_FWD
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_axis_mlp_bwd(const VsrAxisMlpDesc* d, const void* x, const void* dy, const float* w1, const float* b1, const float* w2, const float* b2,
                     void* dx, float* dw1, float* db1, float* dw2, float* db2, void* scratch, size_t scratch_bytes, void* stream) {
    if (!d || !x || !dy || !w1 || !b1 || !w2 || !b2) return VSR_ERR_BADARG;
    long long Q;
    CK(am_check_desc(d, &Q));
    const bool wg = dw1 || db1 || dw2 || db2;
    if (wg && !(dw1 && db1 && dw2 && db2 && scratch)) return VSR_ERR_BADARG;
    if (misaligned(x, esize(d->dtype)) || misaligned(dy, esize(d->dtype)) || misaligned(dx, esize(d->dtype)) || misaligned(w1, 4) ||
        misaligned(b1, 4) || misaligned(w2, 4) || misaligned(b2, 4) || misaligned(dw1, 4) || misaligned(db1, 4) || misaligned(dw2, 4) ||
        misaligned(db2, 4) || misaligned(scratch, 4))
        return VSR_ERR_BADARG;
    if (wg && scratch_bytes < vsr_axis_mlp_scratch_bytes(d)) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (dx) {
#define AM_BWD(T, DMAX) am_launch<T, DMAX>(true, d, Q, x, dy, w1, b1, w2, b2, dx, st)
        if (d->dtype == VSR_BF16) AM_DISPATCH(bf16_t, AM_BWD);
        else AM_DISPATCH(float, AM_BWD);
#undef AM_BWD
    }
    if (wg) {
        float* partial = static_cast<float*>(scratch);
#define AM_WG(T, DMAX) am_launch_wgrad<T, DMAX>(d, Q, x, dy, w1, b1, w2, partial, st)
        if (d->dtype == VSR_BF16) AM_DISPATCH(bf16_t, AM_WG);
        else AM_DISPATCH(float, AM_WG);
#undef AM_WG
        const int E = am_entries(d);
        hipLaunchKernelGGL(axis_mlp_wreduce_kernel, dim3(cdiv(E, 256)), dim3(256), 0, st, partial, am_wgrad_wgs(Q), E, d->D, d->hidden, dw1, db1,
                           dw2, db2);
    }
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
