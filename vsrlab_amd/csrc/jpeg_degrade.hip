// The JPEG round trip of core/augmentations.py RandomJPEGCompression: what libjpeg does to a frame at a given quality with 4:2:0
// chroma, without the entropy coder (lossless, so it changes no pixel).  DESIGN section 11g is the specification; every step is
// int32 and the result is bit-identical to the numpy oracle of tests/jpeg_common.py, which is bit-identical to libjpeg-turbo.
// Built into a library of its own, libvsrlab_jpeg.so (include/vsrlab_jpeg.h): libvsrlab_hip.so's exports stay as they are.
//
// Two launches, because the chroma upsampler reads one chroma sample across every block border:
//   1. jp_codec_kernel: a workgroup owns 64 x 16 pixels = four macroblocks = 24 blocks of 8 x 8 (16 Y, 4 Cb, 4 Cr).  A lane reads the
//      2 x 2 pixels of one chroma sample (planar input, any strides, coordinates clamped to the image: the clamp IS the edge
//      replication of step 2, and no load is conditional; below the image the chroma plane's last row is repeated), quantises to
//      8 bits, converts, downsamples, and writes samples - 128 into an LDS image of the blocks.  Then 192 lanes run the 1-D passes,
//      one lane per row or column: FDCT rows | FDCT columns, quantise, dequantise, IDCT columns (the lane keeps its column in
//      registers across the three) | IDCT rows, whose 8 results leave as one 8-byte store into the byte planes of the workspace.
//      The LDS image has a row pitch of 9 dwords: a wave's 8-dword row reads (lane stride 9) and its column reads (lane stride 1
//      inside a block, 72 between blocks) both touch every bank once.
//   2. jp_recon_kernel: a lane owns one chroma sample: it reads the 3 x 3 Cb and Cr neighbourhood (clamped to the CROPPED planes:
//      the replication of step 9; a plane at most 2 columns wide is upsampled by replication instead) and its four Y bytes, and
//      writes up to 2 x 2 pixels x 3 channels as k / 255.
// The only intermediates in memory are the byte planes: 1.5 bytes per padded pixel written once and read once (the 3 x 3
// neighbourhoods overlap in cache).  No coefficient and no fp32 plane goes through memory.  No MFMA: the 13-bit constants and the
// exact rounding rule it out.
//
// The quantiser divides by 8 Q through a reciprocal: floor(n / d) = umulhi(n, floor(2^32 / d) + 1) for n < 2^21 and d <= 2040
// (n e < 2^32 with e = M d - 2^32 <= d); n = |c| + 4 Q stays below 2^16.  tests/test_jpeg_host.py proves the identity over every Q and
// every n the oracle can reach.
#include "elt.h"
#include "host.h"
#include "../../include/vsrlab_jpeg.h"

namespace {

constexpr int JP_TW = 64, JP_TH = 16;           // pixels per workgroup of the codec launch
constexpr int JP_NB = 24, JP_LD = 9, JP_BS = 8 * JP_LD;   // its blocks, the LDS row pitch and block pitch in dwords
constexpr int JP_MAXDIM = 32768;

struct JpTables { int q[2][64]; unsigned m[2][64]; };       // Q and floor(2^32 / (8 Q)) + 1; [0] luminance, [1] chrominance
struct JpArgs {
    const void* x; void* y;
    unsigned char *py, *pcb, *pcr;
    int H, W, Hp, Wp;
    long long xs[4], ys[4];
};

#define JP_FIX(v) ((int)((v) * 65536 + 0.5))
#define JP_D(x, n) (((x) + (1 << ((n) - 1))) >> (n))

// the odd half that FDCT and IDCT share: (t4, t5, t6, t7) -> the four sums before the descale
static __device__ __forceinline__ void jp_odd(int& t4, int& t5, int& t6, int& t7) {
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    t4 *= 2446; t5 *= 16819; t6 *= 25172; t7 *= 12299;
    z1 *= -7373; z2 *= -20995;
    z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    t4 += z1 + z3; t5 += z2 + z4; t6 += z2 + z3; t7 += z1 + z4;
}

template <bool FIRST>
static __device__ __forceinline__ void jp_fdct(int* d) {
    constexpr int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
    int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : JP_D(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : JP_D(t10 - t11, 2);
    const int z = (t12 + t13) * 4433;
    d[2] = JP_D(z + t13 * 6270, n);
    d[6] = JP_D(z - t12 * 15137, n);
    jp_odd(t4, t5, t6, t7);
    d[7] = JP_D(t4, n); d[5] = JP_D(t5, n); d[3] = JP_D(t6, n); d[1] = JP_D(t7, n);
}

template <int n>
static __device__ __forceinline__ void jp_idct(int* x) {
    const int z1 = (x[2] + x[6]) * 4433;
    const int e2 = z1 - x[6] * 15137, e3 = z1 + x[2] * 6270;
    const int e0 = (x[0] + x[4]) << 13, e1 = (x[0] - x[4]) << 13;
    const int t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    int t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    jp_odd(t0, t1, t2, t3);
    x[0] = JP_D(t10 + t3, n); x[7] = JP_D(t10 - t3, n);
    x[1] = JP_D(t11 + t2, n); x[6] = JP_D(t11 - t2, n);
    x[2] = JP_D(t12 + t1, n); x[5] = JP_D(t12 - t1, n);
    x[3] = JP_D(t13 + t0, n); x[4] = JP_D(t13 - t0, n);
}

static __device__ __forceinline__ int jp_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// step 1: trunc(clamp(x, 0, 1) * 255), the product formed (and rounded) in T
template <typename T>
static __device__ __forceinline__ int jp_to_u8(T v) {
    const float f = fminf(fmaxf(to_f(v), 0.f), 1.f);
    return (int)to_f((T)(f * 255.f));
}

template <typename T>
__global__ __launch_bounds__(256) void jp_codec_kernel(JpArgs a, JpTables tb) {
    __shared__ int blk[JP_NB * JP_BS];
    __shared__ int sq[128];
    __shared__ unsigned sm[128];
    const int t = threadIdx.x, n = blockIdx.z, x0 = blockIdx.x * JP_TW, y0 = blockIdx.y * JP_TH;
    if (t < 128) { sq[t] = tb.q[t >> 6][t & 63]; sm[t] = tb.m[t >> 6][t & 63]; }
    {
        // chroma sample (cy, cx) of the tile and its 2 x 2 pixels; a coordinate past the image reads the last row / column.  Below
        // the image libjpeg replicates the last row of the downsampled chroma PLANE, not the pixels under it (for an even H the two
        // differ): such a lane reads the pixels of the last chroma row, and its Y samples are their second row, which is row H - 1
        const int cx = t & 31, cy = t >> 5, ch = (a.H + 1) >> 1;
        const bool below = (y0 >> 1) + cy >= ch;
        const int cyc = min((y0 >> 1) + cy, ch - 1);
        const T* xp = static_cast<const T*>(a.x) + n * a.xs[0];
        T v[12];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int gx = min(x0 + 2 * cx + (i & 1), a.W - 1), gy = min(2 * cyc + (i >> 1), a.H - 1);
            const long long off = gy * a.xs[2] + gx * a.xs[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[i * 3 + c] = xp[off + c * a.xs[1]];
        }
        int cb = 0, cr = 0, yv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = jp_to_u8(v[i * 3]), g = jp_to_u8(v[i * 3 + 1]), b = jp_to_u8(v[i * 3 + 2]);
            yv[i] = (JP_FIX(.299) * r + JP_FIX(.587) * g + JP_FIX(.114) * b + (1 << 15)) >> 16;
            cb += (-JP_FIX(.16874) * r - JP_FIX(.33126) * g + JP_FIX(.5) * b + (128 << 16) + (1 << 15) - 1) >> 16;
            cr += (JP_FIX(.5) * r - JP_FIX(.41869) * g - JP_FIX(.08131) * b + (128 << 16) + (1 << 15) - 1) >> 16;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int px = 2 * cx + (i & 1), py = 2 * cy + (i >> 1);
            blk[((py >> 3) * 8 + (px >> 3)) * JP_BS + (py & 7) * JP_LD + (px & 7)] = (below ? yv[2 + (i & 1)] : yv[i]) - 128;
        }
        const int bias = 1 + (cx & 1);          // the tile starts at an even chroma column: local parity is the plane's
        blk[(16 + (cx >> 3)) * JP_BS + cy * JP_LD + (cx & 7)] = ((cb + bias) >> 2) - 128;
        blk[(20 + (cx >> 3)) * JP_BS + cy * JP_LD + (cx & 7)] = ((cr + bias) >> 2) - 128;
    }
    __syncthreads();
    const int b = t >> 3, l = t & 7;            // block and the row or column of it this lane transforms (t < 192)
    int d[8];
    if (t < JP_NB * 8) {
        int* p = blk + b * JP_BS + l * JP_LD;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        jp_fdct<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = d[k];
    }
    __syncthreads();
    if (t < JP_NB * 8) {
        int* p = blk + b * JP_BS + l;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k * JP_LD];
        jp_fdct<false>(d);
        const int tab = b >= 16 ? 64 : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = sq[tab + k * 8 + l];
            const int c = d[k], m = c < 0 ? -c : c;
            const int r = (int)__umulhi((unsigned)(m + 4 * q), sm[tab + k * 8 + l]) * q;
            d[k] = c < 0 ? -r : r;
        }
        jp_idct<11>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k * JP_LD] = d[k];
    }
    __syncthreads();
    if (t < JP_NB * 8) {
        const int* p = blk + b * JP_BS + l * JP_LD;
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        jp_idct<18>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = jp_clamp255(d[k] + 128);
        uint2 o;
        o.x = d[0] | d[1] << 8 | d[2] << 16 | d[3] << 24;
        o.y = d[4] | d[5] << 8 | d[6] << 16 | d[7] << 24;
        // Hp is a multiple of the tile's height; a macroblock of the tile may lie past Wp: it stores nothing
        if (b < 16) {
            const int col = x0 + (b & 7) * 8, row = y0 + (b >> 3) * 8 + l;
            if (col < a.Wp) *reinterpret_cast<uint2*>(a.py + ((size_t)n * a.Hp + row) * a.Wp + col) = o;
        } else {
            const int Wc = a.Wp >> 1, col = (x0 >> 1) + (b & 3) * 8, row = (y0 >> 1) + l;
            unsigned char* pl = b < 20 ? a.pcb : a.pcr;
            if (col < Wc) *reinterpret_cast<uint2*>(pl + ((size_t)n * (a.Hp >> 1) + row) * Wc + col) = o;
        }
    }
}

// steps 9 and 10 for one chroma plane: c[row][col] is the 3 x 3 neighbourhood, o[2 dy + dx] the four upsampled samples - 128
static __device__ __forceinline__ void jp_upsample(const int (*c)[3], int* o) {
    int up[3], dn[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) { up[j] = 3 * c[1][j] + c[0][j]; dn[j] = 3 * c[1][j] + c[2][j]; }
    o[0] = ((3 * up[1] + up[0] + 8) >> 4) - 128; o[1] = ((3 * up[1] + up[2] + 7) >> 4) - 128;
    o[2] = ((3 * dn[1] + dn[0] + 8) >> 4) - 128; o[3] = ((3 * dn[1] + dn[2] + 7) >> 4) - 128;
}

template <typename T>
__global__ __launch_bounds__(256) void jp_recon_kernel(JpArgs a) {
    const int t = threadIdx.x, n = blockIdx.z;
    const int ch = (a.H + 1) >> 1, cw = (a.W + 1) >> 1, Wc = a.Wp >> 1, Hc = a.Hp >> 1;
    const int cx0 = blockIdx.x * 32 + (t & 31), cy0 = blockIdx.y * 8 + (t >> 5);
    // a lane past the cropped chroma plane works on its last sample and stores nothing: every load is unconditional and in bounds
    const int cx = min(cx0, cw - 1), cy = min(cy0, ch - 1);
    const int xi[3] = {max(cx - 1, 0), cx, min(cx + 1, cw - 1)}, yi[3] = {max(cy - 1, 0), cy, min(cy + 1, ch - 1)};
    const unsigned char* pb = a.pcb + (size_t)n * Hc * Wc;
    const unsigned char* pr = a.pcr + (size_t)n * Hc * Wc;
    int cb[3][3], cr[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) { cb[i][j] = pb[(size_t)yi[i] * Wc + xi[j]]; cr[i][j] = pr[(size_t)yi[i] * Wc + xi[j]]; }
    // 2 cy + 1 < Hp and 2 cx + 1 < Wp: the Y plane is padded, and 2 cx is even
    const unsigned char* pyr = a.py + ((size_t)n * a.Hp + 2 * cy) * a.Wp + 2 * cx;
    const unsigned y01 = *reinterpret_cast<const unsigned short*>(pyr), y23 = *reinterpret_cast<const unsigned short*>(pyr + a.Wp);
    const int yv[4] = {(int)(y01 & 255), (int)(y01 >> 8), (int)(y23 & 255), (int)(y23 >> 8)};
    int ub[4], ur[4];
    jp_upsample(cb, ub);
    jp_upsample(cr, ur);
    if (cw <= 2) {                              // libjpeg upsamples a chroma plane this narrow by replication
#pragma unroll
        for (int i = 0; i < 4; ++i) { ub[i] = cb[1][1] - 128; ur[i] = cr[1][1] - 128; }
    }
    if (cx0 >= cw || cy0 >= ch) return;
    T* yp = static_cast<T*>(a.y) + n * a.ys[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int px = 2 * cx + (i & 1), py = 2 * cy + (i >> 1);
        if (px >= a.W || py >= a.H) continue;
        const int r = jp_clamp255(yv[i] + ((JP_FIX(1.402) * ur[i] + (1 << 15)) >> 16));
        const int bl = jp_clamp255(yv[i] + ((JP_FIX(1.772) * ub[i] + (1 << 15)) >> 16));
        const int g = jp_clamp255(yv[i] + ((-JP_FIX(.34414) * ub[i] - JP_FIX(.71414) * ur[i] + (1 << 15)) >> 16));
        const long long off = py * a.ys[2] + px * a.ys[3];
        yp[off] = (T)((float)r / 255.f);
        yp[off + a.ys[1]] = (T)((float)g / 255.f);
        yp[off + 2 * a.ys[1]] = (T)((float)bl / 255.f);
    }
}

// Annex K of the JPEG standard, natural order
const unsigned char JP_BASE[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

void jp_tables(int quality, JpTables& tb) {
    const int q = quality < 1 ? 1 : (quality > 100 ? 100 : quality);
    const int s = q < 50 ? 5000 / q : 200 - 2 * q;
    for (int i = 0; i < 2; ++i)
        for (int k = 0; k < 64; ++k) {
            int v = (JP_BASE[i][k] * s + 50) / 100;
            v = v < 1 ? 1 : (v > 255 ? 255 : v);
            tb.q[i][k] = v;
            tb.m[i][k] = (unsigned)((1ull << 32) / (unsigned)(8 * v)) + 1u;
        }
}

struct JpPlan { int Hp, Wp; size_t y_bytes, c_bytes, total; };

int jp_plan(const VsrJpegDesc* d, JpPlan& pl) {
    if (bad_dims(d->N, d->H, d->W)) return VSR_ERR_BADARG;
    if (bad_dtype(d->x_dtype) || bad_dtype(d->y_dtype)) return VSR_ERR_UNSUPPORTED;
    if (d->N > 65535 || d->H > JP_MAXDIM || d->W > JP_MAXDIM) return VSR_ERR_UNSUPPORTED;
    pl.Hp = cdiv(d->H, 16) * 16; pl.Wp = cdiv(d->W, 16) * 16;
    Bump b;
    pl.y_bytes = (size_t)d->N * pl.Hp * pl.Wp;
    pl.c_bytes = pl.y_bytes / 4;
    b.take(pl.y_bytes); b.take(pl.c_bytes); b.take(pl.c_bytes);
    pl.total = b.off;
    return VSR_OK;
}

}  // namespace

extern "C" {

size_t vsr_jpeg_workspace_bytes(const VsrJpegDesc* d) {
    JpPlan pl;
    if (!d) return 0;
    return jp_plan(d, pl) == VSR_OK ? pl.total : 0;
}

int vsr_jpeg_fwd(const VsrJpegDesc* d, const void* x, void* y, void* ws, size_t ws_bytes, void* stream) {
    JpPlan pl;
    if (!d) return VSR_ERR_BADARG;
    CK(jp_plan(d, pl));
    if (!x || !y || !ws || ((size_t)ws & 255)) return VSR_ERR_BADARG;
    if (ws_bytes < pl.total) return VSR_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    JpArgs a = {};
    a.x = x; a.y = y; a.H = d->H; a.W = d->W; a.Hp = pl.Hp; a.Wp = pl.Wp;
    Bump b;
    a.py = static_cast<unsigned char*>(ws) + b.take(pl.y_bytes);
    a.pcb = static_cast<unsigned char*>(ws) + b.take(pl.c_bytes);
    a.pcr = static_cast<unsigned char*>(ws) + b.take(pl.c_bytes);
    for (int i = 0; i < 4; ++i) { a.xs[i] = d->x_stride[i]; a.ys[i] = d->y_stride[i]; }
    JpTables tb;
    jp_tables(d->quality, tb);
    const dim3 gc(cdiv(pl.Wp, JP_TW), pl.Hp / JP_TH, d->N), gr(cdiv((d->W + 1) / 2, 32), cdiv((d->H + 1) / 2, 8), d->N);
    if (d->x_dtype == VSR_BF16) hipLaunchKernelGGL(jp_codec_kernel<bf16_t>, gc, dim3(256), 0, st, a, tb);
    else hipLaunchKernelGGL(jp_codec_kernel<float>, gc, dim3(256), 0, st, a, tb);
    if (d->y_dtype == VSR_BF16) hipLaunchKernelGGL(jp_recon_kernel<bf16_t>, gr, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(jp_recon_kernel<float>, gr, dim3(256), 0, st, a);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

}  // extern "C"
