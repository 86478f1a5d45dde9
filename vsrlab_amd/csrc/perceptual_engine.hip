// VGG19 perceptual loss: value and data gradient (reference: core/losses.py:8,29-64, PerceptualLoss / PerceptualVGG on
// torchvision vgg19().features[:35]).  Like disc_engine.hip: one caller-provided workspace, a plan that is a pure function of
// the descriptor, work only enqueued on the given stream.
//
//   level 1 (H,    W   ):  a0 = relu(conv_0(img))  3 -> 64          conv_mfma (planar source)
//                          a2 = relu(conv_2(a0))   64 -> 64          conv3x3_persist          TAP '2'  (post-ReLU)
//   level 2 (H/2,  W/2 ):  p4 = pool(a2); a5, a7   64 -> 128 -> 128  conv_wide / conv_wide2   TAP '7'  (post-ReLU)
//   level 3 (H/4,  W/4 ):  p9 = pool(a7); a10 .. a16  -> 256                                    TAP '16' (post-ReLU)
//   level 4 (H/8,  W/8 ):  p18; a19 .. a25            -> 512                                    TAP '25' (post-ReLU)
//   level 5 (H/16, W/16):  p27; a28, a30, a32, t34    -> 512                                    TAP '34' (PRE-ReLU: conv5_4 is the
//                          last module of [:35]; torchvision's ReLU(inplace=True) overwrites the stored taps 2..25, not 34)
// MaxPool2d(2, 2) floors odd sizes.  No ImageNet normalisation (the reference has none).
//
// One call = one chunk of images: the hr forward keeps its five taps only (its other activations go to the sr buffers, which
// the sr forward then overwrites), the sr forward keeps every post-ReLU activation (ReLU masks and pool inputs of the
// backward), the tap kernel turns (f_k(sr), f_k(hr)) into per-image sums of |d| and the cotangent scale_k sign(d) (written over
// the hr tap), and the data-gradient chain runs from conv5_4 down to the planar fp32 d sr.  Each backward layer writes into the
// buffer of an activation that is no longer needed, so the backward needs no scratch of its own.
#include <vector>
#include "elt.h"
#include "reduce.h"
#include "wide_recipes.h"

namespace {

constexpr int NCONV = 16;
constexpr int NTAP = VSR_TAP_N;
constexpr int PMAX = VSR_TAP_PMAX;        // block partials per (image, tap)
// features index, output channels, input channels, level (0 = full resolution) of the 16 convolutions of features[:35]
constexpr int L_IDX[NCONV] = {0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34};
constexpr int L_CO[NCONV] = {64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512, 512};
constexpr int L_CI[NCONV] = {3, 64, 64, 128, 128, 256, 256, 256, 256, 512, 512, 512, 512, 512, 512, 512};
constexpr int L_LV[NCONV] = {0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4};
constexpr int TAP_CONV[NTAP] = {1, 3, 7, 11, 15};      // conv (by position) whose output is tap '2', '7', '16', '25', '34'

// ============================================== kernels =============================================================
// out (N, Hi/2, Wi/2, C) = MaxPool2d(2, 2)(in (N, Hi, Wi, C)), floor sizes.  One thread = one output pixel x 8 channels;
// consecutive lanes = consecutive pixels of a 32-pixel output segment (the store is one 512-byte run).
template <typename T>
__global__ void maxpool2_fwd_kernel(const T* __restrict__ in, T* __restrict__ out, int Hi, int Wi, int C) {
    const int Ho = Hi >> 1, Wo = Wi >> 1, CP = C >> 3;
    const int y = blockIdx.y, n = blockIdx.z;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pm_ws(Wo) * CP * 32) return;
    const int px = idx & 31, r = idx >> 5;
    const int c = r % CP, x = (r / CP) * 32 + px;
    if (x >= Wo) return;
    const T* ib = in + (long long)n * pm_image_elems(Hi, Wi, C);
    float m[8], v[8];
    ld8<T>(ib + pm_off(2 * y, 2 * x, c, Wi, C), m);
    ld8<T>(ib + pm_off(2 * y, 2 * x + 1, c, Wi, C), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
    ld8<T>(ib + pm_off(2 * y + 1, 2 * x, c, Wi, C), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
    ld8<T>(ib + pm_off(2 * y + 1, 2 * x + 1, c, Wi, C), v);
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = v[j] > m[j] ? v[j] : m[j];
    st8<T>(out + (long long)n * pm_image_elems(Ho, Wo, C) + pm_off(y, x, c, Wo, C), m);
}

// Backward of MaxPool2d(2, 2) fused with the tap cotangent and the ReLU in front of the pool:
//     g (N, Hi, Wi, C) <- (g + route(dp)) * (a > 0)
// a = the stored pool input (post-ReLU activation), dp = d pool output (N, Hi/2, Wi/2, C).  route() recomputes the argmax
// from a: the FIRST maximum of the window in row-major order, as max_pool2d's index does.  Rows / columns that the floor
// drops get no routed gradient but their mask all the same.  One thread = one 2 x 2 input block x 8 channels.
template <typename T>
__global__ void maxpool2_bwd_kernel(const T* __restrict__ a, const T* __restrict__ dp, T* __restrict__ g, int Hi, int Wi, int C) {
    const int Ho = Hi >> 1, Wo = Wi >> 1, Wb = (Wi + 1) >> 1, CP = C >> 3;
    const int by = blockIdx.y, n = blockIdx.z;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= pm_ws(Wb) * CP * 32) return;
    const int px = idx & 31, r = idx >> 5;
    const int c = r % CP, bx = (r / CP) * 32 + px;
    if (bx >= Wb) return;
    const long long img = (long long)n * pm_image_elems(Hi, Wi, C);
    const T* ab = a + img;
    T* gb = g + img;
    const bool inside = by < Ho && bx < Wo;
    float av[4][8], route[4][8];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 8; ++j) route[q][j] = 0.f;
    if (inside) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ld8<T>(ab + pm_off(2 * by + (q >> 1), 2 * bx + (q & 1), c, Wi, C), av[q]);
        float d[8];
        ld8<T>(dp + (long long)n * pm_image_elems(Ho, Wo, C) + pm_off(by, bx, c, Wo, C), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int arg = 0;
            float m = av[0][j];
#pragma unroll
            for (int q = 1; q < 4; ++q) if (av[q][j] > m) { m = av[q][j]; arg = q; }
#pragma unroll
            for (int q = 0; q < 4; ++q) route[q][j] = q == arg ? d[j] : 0.f;
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int y = 2 * by + (q >> 1), x = 2 * bx + (q & 1);
        if (y >= Hi || x >= Wi) continue;
        const long long o = pm_off(y, x, c, Wi, C);
        float gv[8], m[8];
        ld8<T>(gb + o, gv);
        if (inside) {
#pragma unroll
            for (int j = 0; j < 8; ++j) m[j] = av[q][j];
        } else {
            ld8<T>(ab + o, m);
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) gv[j] = m[j] > 0.f ? gv[j] + route[q][j] : 0.f;
        st8<T>(gb + o, gv);
    }
}

// The L1 term of one tap: s = f_k(sr), h = f_k(hr) (N, H, W, C).  Block b of image n sums |s - h| over a fixed strided share of
// the image's real pixels (fp32 within an 8-channel chunk, fp64 across chunks and lanes) into partial[n * PMAX + b]; g (may alias
// h: every element is read before it is written by the same thread) = scale * sign(s - h), sign(0) = 0.  The grid depends on the
// image geometry only, so an image's sum has the same bits whatever the batch it is computed in.
constexpr int TAP_NT = VSR_TAP_NT;
template <typename T>
__global__ __launch_bounds__(TAP_NT) void tap_l1_kernel(const T* __restrict__ s, const T* h, T* g, float scale, int H, int W, int C,
                                                        double* __restrict__ partial) {
    const int n = blockIdx.y, CP = C >> 3, WS = pm_ws(W);
    const long long img = (long long)n * pm_image_elems(H, W, C);
    const long long total = (long long)H * WS * CP * 32;                  // 8-channel chunks, padding pixels included
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * TAP_NT + threadIdx.x; i < total; i += (long long)gridDim.x * TAP_NT) {
        const int px = (int)(i & 31);
        const int seg = (int)((i >> 5) / CP % WS);
        if (seg * 32 + px >= W) continue;                                  // padding pixels are never written: skip them
        float a[8], b[8];
        ld8<T>(s + img + i * 8, a);
        ld8<T>(h + img + i * 8, b);
        float part = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = a[j] - b[j];
            part += fabsf(d);
            b[j] = d > 0.f ? scale : (d < 0.f ? -scale : 0.f);
        }
        acc += (double)part;
        if (g) st8<T>(g + img + i * 8, b);
    }
    __shared__ double red[TAP_NT / 64];
    wave_sums_to_lds(acc, red);
    if (threadIdx.x == 0) partial[(long long)n * PMAX + blockIdx.x] = sum_inorder(red, TAP_NT / 64);      // reduce.h: index order
}

struct TapSumArgs { int nb[NTAP]; };
// sums[n][k] = sum_b partial[k][n][b], b in increasing order
__global__ void tap_sum_kernel(const double* __restrict__ partial, double* __restrict__ sums, int N, TapSumArgs a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * NTAP) return;
    const int n = i / NTAP, k = i - n * NTAP;
    const double* p = partial + ((long long)k * N + n) * PMAX;
    double t = 0.0;
    for (int b = 0; b < a.nb[k]; ++b) t += p[b];
    sums[i] = t;
}

// =============================================== plan ===============================================================
struct PPlan {
    int n, h, w, dtype, need_grad; size_t es;
    int Hl[5], Wl[5];
    size_t wf[NCONV], wd[NCONV], bias[NCONV];
    size_t act[NCONV];          // sr: relu(conv_k) (the last: conv5_4 pre-ReLU); hr: the same buffers, except its taps
    size_t pool[4];             // p4, p9, p18, p27
    size_t htap[NTAP];          // hr taps, then the tap cotangents
    size_t partial;
    size_t total;

    size_t pm(int lv, int C) const { return (size_t)n * pm_image_elems(Hl[lv], Wl[lv], C) * es; }
    int build(const VsrPerceptualDesc& d) {
        n = d.n; h = d.h; w = d.w; dtype = d.dtype; need_grad = d.need_grad;
        if (dtype != VSR_F32 && dtype != VSR_BF16) return VSR_ERR_BADARG;
        if (n < 1 || h < 16 || w < 16 || n > 65535 || h > 65535 || w > 65535) return VSR_ERR_UNSUPPORTED;
        es = esize(dtype);
        Hl[0] = h; Wl[0] = w;
        for (int l = 1; l < 5; ++l) { Hl[l] = Hl[l - 1] / 2; Wl[l] = Wl[l - 1] / 2; }
        Bump b;
        for (int k = 0; k < NCONV; ++k) {
            const int co = L_CO[k], ci = L_CI[k];
            bias[k] = b.take((size_t)co * 4);
            if (k == 0) {                     // planar 3 -> 64 (16-channel padded source); its data gradient 64 -> 3 planar
                wf[k] = b.take((size_t)9 * 64 * 16 * es);
                wd[k] = need_grad ? b.take((size_t)9 * 32 * 64 * es) : 0;
            } else if (k == 1) {              // 64 -> 64: conv_mfma / conv3x3_persist image
                wf[k] = b.take((size_t)9 * 64 * 64 * es);
                wd[k] = need_grad ? b.take((size_t)9 * 64 * 64 * es) : 0;
            } else {
                const bool w2 = dtype == VSR_BF16;
                wf[k] = b.take((size_t)(w2 ? vsr_wide2_pack_elems(co, ci, 0) : vsr_wide_pack_elems(co, ci, 0)) * es);
                wd[k] = need_grad ? b.take((size_t)(w2 ? vsr_wide2_pack_elems(co, ci, 2) : vsr_wide_pack_elems(co, ci, 2)) * es) : 0;
            }
        }
        for (int k = 0; k < NCONV; ++k) act[k] = b.take(pm(L_LV[k], L_CO[k]));
        const int pc[4] = {64, 128, 256, 512};
        for (int l = 0; l < 4; ++l) pool[l] = b.take(pm(l + 1, pc[l]));
        for (int t = 0; t < NTAP; ++t) htap[t] = b.take(pm(L_LV[TAP_CONV[t]], L_CO[TAP_CONV[t]]));
        partial = b.take((size_t)NTAP * n * PMAX * sizeof(double));
        total = b.off;
        return VSR_OK;
    }
    // blocks of the tap kernel per image: a pure function of the level geometry (vsr_tap_blocks)
    int tap_blocks(int t) const {
        const int lv = L_LV[TAP_CONV[t]];
        return vsr_tap_blocks(Hl[lv], Wl[lv], L_CO[TAP_CONV[t]]);
    }
};

struct PCtx {
    const PPlan& p; char* ws; hipStream_t st; int dtype;
    void* at(size_t o) const { return ws + o; }
    const float* fat(size_t o) const { return reinterpret_cast<const float*>(ws + o); }

    ConvArgs base(int H, int W) const {
        ConvArgs a = {};
        a.in_step = 1; a.Hs = H; a.Ws = W; a.N = p.n; a.H = H; a.W = W; a.nz = 1;
        a.out_step = 1; a.Hd = H; a.Wd = W; a.CD = 64; a.cout_real = 64; a.dst_nstride = pm_image_elems(H, W, 64);
        a.src_nstride[0] = pm_image_elems(H, W, 64);
        return a;
    }
    // the wide and VGG launches: the shared recipes (wide_recipes.h) on this plan's batch
    WideCtx wc() const { return WideCtx{st, dtype, p.n, nullptr}; }
    // 3x3 stride-1 conv at >= 64 channels on conv_wide (fp32) / conv_wide2 (bf16).  aux: ReLU mask source (slope 0)
    int wide(int k, bool dgrad, const void* x, void* y, int act, const void* aux) const {
        const int lv = L_LV[k], xC = dgrad ? L_CO[k] : L_CI[k], yC = dgrad ? L_CI[k] : L_CO[k];
        return wc().wide(x, xC, p.Hl[lv], p.Wl[lv], 1, p.Hl[lv], p.Wl[lv], at(dgrad ? p.wd[k] : p.wf[k]), dgrad ? nullptr : fat(p.bias[k]),
                         y, yC, 1, act, 0.f, nullptr, nullptr, nullptr, aux);
    }
    int pool_fwd(int lv, int C, const void* in, void* out) const { return wc().pool_fwd(in, out, p.Hl[lv], p.Wl[lv], C); }
    int pool_bwd(int lv, int C, const void* a, const void* dp, void* g) const { return wc().pool_bwd(a, dp, g, p.Hl[lv], p.Wl[lv], C); }
    int tap(int t, const void* s, void* h, bool grad, float scale) const {
        const int lv = L_LV[TAP_CONV[t]], C = L_CO[TAP_CONV[t]];
        return wc().tap(s, h, grad, scale, p.Hl[lv], p.Wl[lv], C, reinterpret_cast<double*>(at(p.partial)) + (size_t)t * p.n * PMAX);
    }
};

int perc_pack(const PCtx& c, const float* const* prm) {
    const PPlan& p = c.p;
    const int dt = c.dtype;
    for (int k = 0; k < NCONV; ++k) {
        const float* wgt = prm[2 * k];
        HIP_CHECK_RET(hipMemcpyAsync(c.at(p.bias[k]), prm[2 * k + 1], (size_t)L_CO[k] * 4, hipMemcpyDeviceToDevice, c.st));
        if (k == 0) {
            CK(vsr_launch_pack_weights(dt, wgt, c.at(p.wf[0]), 9, 64, 16, 64, 3, 3, 0, 1, 0, 0, c.st));
            if (p.need_grad) CK(vsr_launch_pack_weights(dt, wgt, c.at(p.wd[0]), 9, 32, 64, 3, 64, 3, 0, 1, 0, 1, c.st));
        } else if (k == 1) {
            CK(vsr_launch_pack_weights(dt, wgt, c.at(p.wf[1]), 9, 64, 64, 64, 64, 64, 0, 1, 0, 0, c.st));
            if (p.need_grad) CK(vsr_launch_pack_weights(dt, wgt, c.at(p.wd[1]), 9, 64, 64, 64, 64, 64, 0, 1, 0, 1, c.st));
        } else if (dt == VSR_BF16) {
            CK(vsr_launch_pack_wide2(wgt, c.at(p.wf[k]), L_CO[k], L_CI[k], 0, c.st));
            if (p.need_grad) CK(vsr_launch_pack_wide2(wgt, c.at(p.wd[k]), L_CO[k], L_CI[k], 2, c.st));
        } else {
            CK(vsr_launch_pack_wide(dt, wgt, c.at(p.wf[k]), L_CO[k], L_CI[k], 0, c.st));
            if (p.need_grad) CK(vsr_launch_pack_wide(dt, wgt, c.at(p.wd[k]), L_CO[k], L_CI[k], 2, c.st));
        }
    }
    return VSR_OK;
}

// features[:35] on img (n,3,h,w) planar fp32.  hr: the tap outputs go to the hr tap buffers (the rest to the sr buffers).
int perc_forward(const PCtx& c, const float* img, bool hr) {
    const PPlan& p = c.p;
    const int dt = c.dtype;
    int t = 0;
    auto out = [&](int k) -> void* { return (hr && t < NTAP && TAP_CONV[t] == k) ? c.at(p.htap[t]) : c.at(p.act[k]); };
    {   // conv_0 + ReLU: planar 3-channel source
        ConvArgs a = c.base(p.h, p.w);
        a.src[0] = img; a.src_nstride[0] = (long long)3 * p.h * p.w; a.wpack = c.at(p.wf[0]); a.bias = c.fat(p.bias[0]);
        a.dst[0] = out(0); a.act = ACT_RELU;
        CK(vsr_launch_conv(dt, 3, 1, 16, 16, 1, 64, EPI_NHWC, a, c.st));
    }
    const void* x = out(0);
    for (int k = 1; k < NCONV; ++k) {
        if (L_LV[k] != L_LV[k - 1]) {            // MaxPool2d(2, 2) between the levels
            const int lv = L_LV[k - 1];
            CK(c.pool_fwd(lv, L_CO[k - 1], x, c.at(p.pool[lv])));
            x = c.at(p.pool[lv]);
        }
        void* y = out(k);
        const int act = k == NCONV - 1 ? ACT_NONE : ACT_RELU;
        if (k == 1) {
            ConvArgs a = c.base(p.h, p.w);
            a.src[0] = x; a.wpack = c.at(p.wf[1]); a.bias = c.fat(p.bias[1]); a.dst[0] = y; a.act = act;
            CK(vsr_launch_conv(dt, 3, 1, 64, 64, 0, 64, EPI_NHWC, a, c.st));
        } else {
            CK(c.wide(k, false, x, y, act, nullptr));
        }
        if (t < NTAP && TAP_CONV[t] == k) ++t;
        x = y;
    }
    return VSR_OK;
}

// d sr from the tap cotangents (in the hr tap buffers): conv5_4 .. conv_0, each layer's output into a dead activation buffer
int perc_backward(const PCtx& c, float* dsr) {
    const PPlan& p = c.p;
    const int dt = c.dtype;
    // g: the cotangent of conv k's (pre-ReLU) output; walk k = 15 .. 1, dgrad(conv k) * ReLU'(act[k-1]) -> buffer of act[k]
    const void* g = c.at(p.htap[NTAP - 1]);
    int t = NTAP - 1;
    for (int k = NCONV - 1; k >= 1; --k) {
        const bool pool_below = L_LV[k] != L_LV[k - 1];
        void* y = pool_below ? c.at(p.pool[L_LV[k - 1]]) : c.at(p.act[k]);
        const void* mask = pool_below ? nullptr : c.at(p.act[k - 1]);
        if (k == 1) {
            ConvArgs a = c.base(p.h, p.w);
            a.src[0] = g; a.wpack = c.at(p.wd[1]); a.dst[0] = y; a.act = ACT_NONE; a.aux[0] = mask; a.mask_mode = MASK_RELU;
            CK(vsr_launch_conv(dt, 3, 1, 64, 64, 0, 64, EPI_NHWC, a, c.st));
        } else {
            CK(c.wide(k, true, g, y, ACT_NONE, mask));
        }
        g = y;
        if (pool_below) {                         // d p -> the tap cotangent of conv k-1 (+ routed, * ReLU')
            --t;
            const int lv = L_LV[k - 1];
            CK(c.pool_bwd(lv, L_CO[k - 1], c.at(p.act[k - 1]), g, c.at(p.htap[t])));
            g = c.at(p.htap[t]);
        }
    }
    {   // conv_0's data gradient: 64 -> 3, planar fp32
        ConvArgs a = c.base(p.h, p.w);
        a.src[0] = g; a.wpack = c.at(p.wd[0]); a.cout_real = 3;
        a.dst[0] = dsr; a.dst_nstride = (long long)3 * p.h * p.w;
        CK(vsr_launch_conv(dt, 3, 1, 64, 64, 0, 32, EPI_PLANAR, a, c.st));
    }
    return VSR_OK;
}

}  // namespace

// ===================== the launchers of the kernels above (C++ linkage: wide_recipes.h, wide_hooks.hip) ==========================
int vsr_launch_maxpool2_fwd(int dtype, const void* in, void* out, int N, int Hi, int Wi, int C, hipStream_t st) {
    const int Ho = Hi / 2, Wo = Wi / 2;
    const dim3 grid(cdiv(pm_ws(Wo) * 32 * (C / 8), 256), Ho, N);
    if (dtype == VSR_BF16) hipLaunchKernelGGL(maxpool2_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)in, (bf16_t*)out, Hi, Wi, C);
    else hipLaunchKernelGGL(maxpool2_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)in, (float*)out, Hi, Wi, C);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_launch_maxpool2_bwd(int dtype, const void* a, const void* dp, void* g, int N, int Hi, int Wi, int C, hipStream_t st) {
    const int Wb = (Wi + 1) / 2, Hb = (Hi + 1) / 2;
    const dim3 grid(cdiv(pm_ws(Wb) * 32 * (C / 8), 256), Hb, N);
    if (dtype == VSR_BF16) hipLaunchKernelGGL(maxpool2_bwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)a, (const bf16_t*)dp, (bf16_t*)g, Hi, Wi, C);
    else hipLaunchKernelGGL(maxpool2_bwd_kernel<float>, grid, dim3(256), 0, st, (const float*)a, (const float*)dp, (float*)g, Hi, Wi, C);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_launch_tap_l1(int dtype, const void* s, const void* h, void* g, float scale, int N, int H, int W, int C, double* partial, int nblocks,
                      hipStream_t st) {
    const dim3 grid(nblocks, N);
    if (dtype == VSR_BF16)
        hipLaunchKernelGGL(tap_l1_kernel<bf16_t>, grid, dim3(TAP_NT), 0, st, (const bf16_t*)s, (const bf16_t*)h, (bf16_t*)g, scale, H, W, C, partial);
    else
        hipLaunchKernelGGL(tap_l1_kernel<float>, grid, dim3(TAP_NT), 0, st, (const float*)s, (const float*)h, (float*)g, scale, H, W, C, partial);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

int vsr_launch_tap_sum(const double* partial, double* sums, int N, const int* nblocks5, hipStream_t st) {
    TapSumArgs ta;
    for (int t = 0; t < NTAP; ++t) ta.nb[t] = nblocks5[t];
    hipLaunchKernelGGL(tap_sum_kernel, dim3(cdiv(N * NTAP, 256)), dim3(256), 0, st, partial, sums, N, ta);
    HIP_CHECK_RET(hipGetLastError());
    return VSR_OK;
}

extern "C" {

size_t vsr_perceptual_workspace_bytes(const VsrPerceptualDesc* d) {
    if (!d) return 0;
    PPlan p;
    if (p.build(*d) != VSR_OK) return 0;
    return p.total;
}

int vsr_perceptual_loss(const VsrPerceptualDesc* d, const float* const* params, int nparams, const float* sr, const float* hr,
                        const float* scales, double* sums, float* dsr, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d || !params || nparams != 2 * NCONV || !sr || !hr || !sums || !workspace) return VSR_ERR_BADARG;
    for (int k = 0; k < 2 * NCONV; ++k) if (!params[k]) return VSR_ERR_BADARG;
    if (d->need_grad && (!dsr || !scales)) return VSR_ERR_BADARG;
    if (!d->need_grad && dsr) return VSR_ERR_BADARG;
    PPlan p;
    CK(p.build(*d));
    if (workspace_bytes < p.total) return VSR_ERR_WORKSPACE;
    const PCtx c{p, (char*)workspace, (hipStream_t)stream, p.dtype};
    CK(perc_pack(c, params));
    CK(perc_forward(c, hr, true));
    CK(perc_forward(c, sr, false));
    int nb[NTAP];
    for (int t = 0; t < NTAP; ++t) {
        const int k = TAP_CONV[t];
        CK(c.tap(t, c.at(p.act[k]), c.at(p.htap[t]), p.need_grad != 0, p.need_grad ? scales[t] : 0.f));
        nb[t] = p.tap_blocks(t);
    }
    CK(vsr_launch_tap_sum((const double*)c.at(p.partial), sums, p.n, nb, c.st));
    if (p.need_grad) CK(perc_backward(c, dsr));
    return VSR_OK;
}

}  // extern "C"
