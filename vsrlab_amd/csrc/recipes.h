// Launch recipes shared by the BasicVSR-side host files (engine.hip, spynet_engine.hip, cleaner_engine.hip, layer_ops.hip): the
// SPyNet layer shapes and Ctx, one member function per kind of layer.  Like host.h: no kernel and no state live here.
#pragma once
#include <vector>
#include "host.h"

inline constexpr int NSPY = 5;         // convs per SPyNet level
inline constexpr int SPY_CI[NSPY] = {8, 32, 64, 32, 16};
inline constexpr int SPY_CO[NSPY] = {32, 64, 32, 16, 2};
inline constexpr int SPY_CIP[NSPY] = {16, 32, 64, 32, 16};
inline constexpr int SPY_COP[NSPY] = {32, 64, 32, 32, 32};   // padded (template) sizes
inline constexpr int SPY_CD[NSPY] = {32, 64, 32, 16, 0};     // channels per pixel of each layer's pixel-major output
// backward (train_flow): pixel-major channels of each layer's dY, and the dgrad launch's template rows (COUT)
inline constexpr int SPY_DK[NSPY] = {32, 64, 32, 16, 16};
inline constexpr int SPY_DROWS[NSPY] = {32, 32, 64, 32, 32};

// What every launch recipe needs: the stream, the compute dtype, the mid-channel width and (backward) this stream's weight-gradient
// slab buffer.  The engines address their arena through at() / fat(); the per-op entries (ws = null) run the same recipes on the
// caller's buffers.
struct Ctx {
    char* ws;
    hipStream_t st;
    int dtype;
    // mid channels: 64 (persistent kernels, sign bits, phase planes) or 16 / 32 (one generic-kernel launch per layer); CO: the conv
    // template's output rows for C outputs (C = 16 runs on the 32-row template with cout_real = 16)
    int C, CO;
    size_t es;
    float* slab;                // wgrad_slab_bytes() for the weight-gradient partials of this stream (null: no backward)
    mutable std::vector<VsrPackDesc>* batch = nullptr;      // while set, pack() collects descriptors for ONE multi-tensor launch
    Ctx(char* ws_, hipStream_t st_, int dtype_, int C_ = 64, float* slab_ = nullptr)
        : ws(ws_), st(st_), dtype(dtype_), C(C_), CO(C_ < 32 ? 32 : C_), es(esize(dtype_)), slab(slab_) {}
    void* at(size_t off) const { return ws + off; }
    const float* fat(size_t off) const { return reinterpret_cast<const float*>(ws + off); }

    // the destination of `a` (an N x H x W x 64 image, H and W even) as four phase planes of N x H/2 x W/2 x 64 (ConvArgs::unshuffle)
    static long long plane_elems(int N, int H, int W) { return (long long)N * pm_image_elems(H / 2, W / 2, 64); }
    static void set_unshuffle(ConvArgs& a, int N, int H, int W) {
        a.unshuffle = 1; a.unshuffle_plane = plane_elems(N, H, W); a.dst_nstride = pm_image_elems(H / 2, W / 2, 64);
    }
    // y = act(conv(x) + bias) (+res) (*mask(aux)) -- C -> C, 3x3 or 1x1, at one resolution (bf16 3x3 at C = 64: the persistent
    // kernel; sign bits and phase-separated outputs exist there only)
    int conv(int ks, const void* x, const void* wpack, const float* bias, void* y, int act, const void* res, const void* aux, int mask,
             int N, int H, int W, void* sign_out = nullptr, const void* sign_bits = nullptr, bool unshuffle = false, float slope = 0.f) const {
        ConvArgs a = conv_args(N, H, W, C);
        a.src[0] = x; a.wpack = wpack; a.bias = bias; a.dst[0] = y; a.act = act; a.leaky_slope = slope; a.res[0] = res; a.aux[0] = aux; a.mask_mode = mask;
        a.sign_out[0] = sign_out; a.sign_bits[0] = sign_bits;
        if (unshuffle) set_unshuffle(a, N, H, W);
        const int rc = vsr_launch_conv(dtype, ks, 1, C, C, 0, CO, EPI_NHWC, a, st);
        // VSRLAB_AMD_GENERIC_CONV=1 (A/B switch): the generic kernel does not write sign bits, but later launches (hr_tail.hip's
        // conv_last.2 data gradient, the masked data gradients) read them -- r04: the switch gave wrong gradients since round 2
        if (rc == VSR_OK && sign_out && dtype == VSR_BF16 && vsr_env().generic_conv) return vsr_launch_sign_bits_c64(y, sign_out, N, H, W, st);
        return rc;
    }
    // C -> 3 planar fp32 (+ pres): the stems' LR-channel gradient, the pre-clean out conv
    int conv_planar3(const void* x, const void* wpack, const float* bias, float* y, long long y_nstride, const float* pres, int N, int H, int W) const {
        ConvArgs a = conv_args(N, H, W, C);
        a.src[0] = x; a.wpack = wpack; a.bias = bias; a.cout_real = 3; a.dst[0] = y; a.dst_nstride = y_nstride; a.pres = pres;
        return vsr_launch_conv(dtype, 3, 1, C, C, 0, 32, EPI_PLANAR, a, st);
    }

    // ---- PixelShufflePack (upsampling.py:4-12) ----
    // PixelShuffle(2): out[c, 2y+i, 2x+j] = conv[4c+2i+j, y, x]  => sub-conv z uses rows 4c+z and bias entries 4c+z
    int pack_ps(const float* w, void* dst, int mode) const {
        for (int z = 0; z < 4; ++z) CK(pack(w, (char*)dst + (size_t)z * 9 * CO * C * es, 9, CO, C, C, C, C, 0, 4, z, mode));
        return VSR_OK;
    }
    int pack_ps_bias(const float* b, float* dst) const {
        for (int z = 0; z < 4; ++z) CK(pack_bias(b, dst + z * C, C, 4, z));
        return VSR_OK;
    }
    // conv3x3 C->4C + PixelShuffle(2): x (N,H,W,C) -> y (N,2H,2W,C)   (upsampling.py:10-12)
    int conv_ps(const void* x, const void* wpack, const float* bias4, void* y, int N, int H, int W, int act = ACT_NONE, float slope = 0.f) const {
        ConvArgs a = conv_args(N, H, W, C);
        a.src[0] = x; a.wpack = wpack; a.w_zstride = 9 * CO * C; a.bias = bias4; a.bias_zstride = C; a.nz = 4; a.act = act; a.leaky_slope = slope;
        a.out_step = 2; a.Hd = 2 * H; a.Wd = 2 * W; a.dst_nstride = pm_image_elems(2 * H, 2 * W, C);
        for (int z = 0; z < 4; ++z) { a.dst[z] = y; a.out_oy[z] = z >> 1; a.out_ox[z] = z & 1; }
        return vsr_launch_conv(dtype, 3, 1, C, C, 0, CO, EPI_NHWC, a, st);
    }
    // data gradient of the above: dy (N,2H,2W,64) -> dx (N,H,W,64) (* mask(aux)) = sum over the 4 pixel-shuffle
    // phases z of a transposed 3x3 64->64 conv of dy's phase z.  bf16: four launches of the persistent kernel (the
    // four weight sets do not fit LDS together), phase z reading phase z-1's partial sum as its residual in place --
    // the partial sums pass through bf16 three times (~1.6x the rounding error of the final store alone), for
    // 560 us instead of 1470 us at 1080x1920.  fp32: one generic 4-source launch, accumulated in registers.
    // dy_planes: dy is stored phase-separated (four N x H x W planes, written by a launch with ConvArgs::unshuffle): phase z is then a
    // contiguous tensor instead of every second pixel of every second row of the 2H x 2W image (r04: the strided form fetched every
    // line of dy twice per data gradient and again twice per weight gradient); dx_planes: write dx phase-separated in turn.
    // C < 64: the one 4-source launch in both dtypes (the persistent kernel is 64-channel).
    int conv_ps_dgrad(const void* dy, const void* wpackd, void* dx, const void* aux, int mask, int N, int H, int W, const void* sign_bits = nullptr,
                      bool dy_planes = false, bool dx_planes = false) const {
        if (dtype == VSR_BF16 && C == 64) {
            for (int z = 0; z < 4; ++z) {
                ConvArgs a = conv_args(N, H, W, C);
                if (dy_planes) {
                    a.src[0] = (const char*)dy + (size_t)z * plane_elems(N, 2 * H, 2 * W) * es;      // plane z: N x H x W, stride 1 (conv_args() set it up)
                } else {
                    a.in_step = 2; a.Hs = 2 * H; a.Ws = 2 * W;
                    a.src[0] = dy; a.src_oy[0] = z >> 1; a.src_ox[0] = z & 1; a.src_nstride[0] = pm_image_elems(2 * H, 2 * W, C);
                }
                a.wpack = (const char*)wpackd + (size_t)z * 9 * C * C * es; a.dst[0] = dx;
                a.res[0] = z > 0 ? dx : nullptr;
                if (dx_planes) set_unshuffle(a, N, H, W);
                if (z == 3) { a.aux[0] = aux; a.mask_mode = mask; a.sign_bits[0] = aux ? sign_bits : nullptr; }
                int rc = vsr_launch_conv(dtype, 3, 1, 64, 64, 0, 64, EPI_NHWC, a, st);
                if (rc != VSR_OK) return rc;
            }
            return VSR_OK;
        }
        ConvArgs a = conv_args(N, H, W, C);
        a.nz = 1; a.in_step = 2; a.Hs = 2 * H; a.Ws = 2 * W;
        for (int s = 0; s < 4; ++s) { a.src[s] = dy; a.src_oy[s] = s >> 1; a.src_ox[s] = s & 1; a.src_nstride[s] = pm_image_elems(2 * H, 2 * W, C); }
        a.wpack = wpackd; a.dst[0] = dx; a.aux[0] = aux; a.mask_mode = mask;
        return vsr_launch_conv(dtype, 3, 4, C, C, 0, CO, EPI_NHWC, a, st);
    }
    // weight gradients: one launch per pixel-shuffle phase z over the nseg (X, dY) pairs, X = the layer's input (N,H,W,C), dY = phase z
    // of the gradient into it (a contiguous plane when dy_planes, else every second pixel of every second row of the 2H x 2W image)
    int ps_wgrads(const void* const* x, const void* const* dy, int nseg, bool dy_planes, int N, int H, int W, float* gw, float* gb, int accumulate) const {
        for (int z = 0; z < 4; ++z) {
            WgradArgs a = wg_base(N, H, W, C, C);
            a.nseg = nseg;
            for (int i = 0; i < nseg; ++i) {
                a.x[i] = x[i];
                a.dy[i] = dy_planes ? (const char*)dy[i] + (size_t)z * plane_elems(N, 2 * H, 2 * W) * es : dy[i];      // plane z: N x H x W, contiguous
            }
            if (!dy_planes) { a.dy_step = 2; a.dy_oy = z >> 1; a.dy_ox = z & 1; a.Hy = 2 * H; a.Wy = 2 * W; a.dy_nstride = pm_image_elems(2 * H, 2 * W, C); }
            CK(wgrad(a, {3, C, false, C, false}, {C, C, gw, C, 0, 4, z, gb, accumulate}));
        }
        return VSR_OK;
    }

    // ---- the ResidualBlock stem (conv.py:97): conv3x3 on cat([lr(3), feat(C)]) (cat) or on lr alone ----
    // cat: source 0 = feat = input channels 3..C+2, source 1 = LR = 0..2 (basicvsr.py:56,71): two weight sets, feat's first
    int pack_stem(const float* w, void* dst, bool cat) const {
        const int I_total = cat ? C + 3 : 3;
        if (cat) CK(pack(w, dst, 9, CO, C, C, C, I_total, 3, 1, 0, 0));
        return pack(w, (char*)dst + (cat ? (size_t)9 * CO * C * es : 0), 9, CO, 16, C, 3, I_total, 0, 1, 0, 0);
    }
    // data-gradient weights: towards feat (conv(3, ...) runs them), towards the 3 LR channels (conv_planar3)
    int pack_stem_dgrad(const float* w, void* dst) const { return pack(w, dst, 9, CO, C, C, C, C + 3, 3, 1, 0, 1); }
    int pack_stem_dlr(const float* w, void* dst, bool cat) const { return pack(w, dst, 9, 32, C, 3, C, cat ? C + 3 : 3, 0, 1, 0, 1); }
    // feat: null => zeros (first frame of a direction); lr: planar fp32, lr_nstride floats between images
    int stem(bool cat, const void* feat, const float* lr, long long lr_nstride, const void* wpack, const float* bias, void* y, int act, float slope,
             int N, int H, int W) const {
        ConvArgs a = conv_args(N, H, W, C);
        a.wpack = wpack; a.bias = bias; a.dst[0] = y; a.act = act; a.leaky_slope = slope;
        a.src[cat ? 1 : 0] = lr; a.src_nstride[cat ? 1 : 0] = lr_nstride;
        if (!cat) return vsr_launch_conv(dtype, 3, 1, 16, 16, 1, CO, EPI_NHWC, a, st);
        a.src[0] = feat;
        return vsr_launch_conv(dtype, 3, 2, C, 16, 1, CO, EPI_NHWC, a, st);
    }
    // a_lr: X = the planar LR frames (+ the bias gradient); a_feat (cat, skipped without segments): X = feat
    int stem_wgrads(bool cat, WgradArgs& a_lr, WgradArgs& a_feat, float* gw, float* gb, int accumulate) const {
        const int I_total = cat ? C + 3 : 3;
        CK(wgrad(a_lr, {3, 16, true, C, false}, {C, 3, gw, I_total, 0, 1, 0, gb, accumulate}));
        if (cat && a_feat.nseg) CK(wgrad_cc(3, a_feat, gw, I_total, 3, nullptr, accumulate));
        return VSR_OK;
    }

    // ---- the 1x1 fusion conv on cat([outputs[i], feat_prop]) (basicvsr.py:18,75-77) ----
    // two weight sets, one per C-channel half of its 2C inputs; mode 0 forward, 1 data gradient
    int pack_point(const float* w, void* dst, int mode) const {
        for (int s = 0; s < 2; ++s) CK(pack(w, (char*)dst + (size_t)s * CO * C * es, 1, CO, C, C, C, 2 * C, s * C, 1, 0, mode));
        return VSR_OK;
    }
    // y = LeakyReLU(conv1x1(cat([xa, xb])) + bias)
    int point_conv(const void* xa, const void* xb, const void* wpack, const float* bias, void* y, int N, int H, int W) const {
        ConvArgs a = conv_args(N, H, W, C);
        a.src[0] = xa; a.src[1] = xb;
        a.wpack = wpack; a.bias = bias; a.dst[0] = y; a.act = ACT_LEAKY;
        return vsr_launch_conv(dtype, 1, 2, C, C, 0, CO, EPI_NHWC, a, st);
    }
    // its data gradient: two C-channel outputs (towards xa, towards xb) of one launch
    int point_dgrad(const void* dy, const void* wpackd, void* da, void* db, int N, int H, int W) const {
        ConvArgs a = conv_args(N, H, W, C);
        a.src[0] = dy; a.wpack = wpackd; a.w_zstride = CO * C; a.nz = 2;
        a.dst[0] = da; a.dst[1] = db;
        return vsr_launch_conv(dtype, 1, 1, C, C, 0, CO, EPI_NHWC, a, st);
    }

    // ---- SPyNet layer j (spynet.py:16-18) ----
    // mode 0: forward weights; mode 1: data-gradient weights, rows = the conv's input channels (template COUT of the dgrad launch), K = its outputs
    int pack_spy(int j, const float* w, void* dst, int mode) const {
        if (mode == 0) return pack(w, dst, 49, SPY_COP[j], SPY_CIP[j], SPY_CO[j], SPY_CI[j], SPY_CI[j], 0, 1, 0, 0);
        return pack(w, dst, 49, SPY_DROWS[j], SPY_DK[j], SPY_CI[j], SPY_CO[j], SPY_CI[j], 0, 1, 0, 1);
    }
    // y: pixel-major with SPY_CD[j] channels (j < 4) or planar fp32 (N,2,H,W) (+ pres) for the last layer
    int spy_conv(int j, const void* x, const void* wpack, const float* bias, void* y, int act, float slope, const float* pres, int N, int H, int W) const {
        ConvArgs a = conv_args(N, H, W, SPY_CD[j]);
        a.src[0] = x; a.src_nstride[0] = pm_image_elems(H, W, SPY_CIP[j]);
        a.wpack = wpack; a.bias = bias; a.act = act; a.leaky_slope = slope; a.cout_real = SPY_CO[j]; a.dst[0] = y;
        if (j < NSPY - 1) return vsr_launch_conv(dtype, 7, 1, SPY_CIP[j], SPY_CIP[j], 0, SPY_COP[j], EPI_NHWC, a, st);
        a.dst_nstride = (long long)2 * H * W; a.pres = pres;
        return vsr_launch_conv(dtype, 7, 1, 16, 16, 0, 32, EPI_PLANAR, a, st);
    }
    // dX_j = dgrad(conv_j)(dY_j) (* ReLU'(aux)); dy: pixel-major with SPY_DK[j] channels
    int spy_dgrad(int j, const void* dy, const void* wpackd, void* dx, const void* aux, int N, int H, int W) const {
        const int CI = SPY_CIP[j], DK = SPY_DK[j];
        ConvArgs a = conv_args(N, H, W, CI);
        a.src[0] = dy; a.src_nstride[0] = pm_image_elems(H, W, DK);
        a.wpack = wpackd; a.dst[0] = dx; a.cout_real = j == 0 ? 8 : CI;
        if (aux) { a.aux[0] = aux; a.mask_mode = MASK_RELU; }
        return vsr_launch_conv(dtype, 7, 1, DK, DK, 0, SPY_DROWS[j], EPI_NHWC, a, st);
    }
    int spy_wgrad(int j, const void* x, const void* dy, int N, int H, int W, float* gw, float* gb, int accumulate) const {
        const int CI = SPY_CIP[j], DK = SPY_DK[j];
        // fp32, 64 input channels: two 32-channel halves (the 14x38-pixel fp32 tile of 64 channels exceeds LDS)
        const int nhalf = (dtype == VSR_F32 && CI == 64) ? 2 : 1;
        for (int hf = 0; hf < nhalf; ++hf) {
            WgradArgs a = wg_base(N, H, W, CI, DK);
            a.x[0] = x; a.dy[0] = dy;
            const int cx = CI / nhalf;
            if (nhalf == 2) { a.x_ctotal = CI; a.x_coff = hf * (cx / 8); }
            const int cin_real = nhalf == 2 ? cx : SPY_CI[j];
            CK(wgrad(a, {7, cx, false, DK, false}, {SPY_CO[j], cin_real, gw, SPY_CI[j], hf * cx, 1, 0, hf == 0 ? gb : nullptr, accumulate}));
        }
        return VSR_OK;
    }

    // ---- weight gradients: one launch into this stream's slab buffer + its reduction (host.h) ----
    int wgrad(WgradArgs& a, const WgradShape& s, const WgradDst& d, bool even = true) const { return wgrad_run(st, dtype, slab, a, s, d, even); }
    // C -> C (3x3 / 1x1) into input channels [i_off, i_off + C) of gw's I_total
    int wgrad_cc(int ks, WgradArgs& a, float* gw, int I_total, int i_off, float* gb, int accumulate) const {
        return wgrad(a, {ks, C, false, C, false}, {C, C, gw, I_total, i_off, 1, 0, gb, accumulate});
    }

    // C -> C (3x3 / 1x1): mode 0 forward, 1 data gradient (flipped, transposed)
    int pack_cc(int ks, const float* w, void* dst, int mode) const { return pack(w, dst, ks * ks, CO, C, C, C, C, 0, 1, 0, mode); }
    int pack(const float* w, void* dst, int KK, int RP, int CPd, int r_real, int c_real, int I_total, int i_off, int o_mul,
             int o_add, int mode) const {
        return pack_any(dtype, w, dst, KK, RP, CPd, r_real, c_real, I_total, i_off, o_mul, o_add, mode);
    }
    int pack_bias(const float* b, void* dst, int nreal, int o_mul = 1, int o_add = 0) const {
        return pack_any(VSR_F32, b, dst, 1, nreal, 1, nreal, 1, 1, 0, o_mul, o_add, 0);
    }
    int pack_any(int dt, const float* w, void* dst, int KK, int RP, int CPd, int r_real, int c_real, int I_total, int i_off, int o_mul,
                 int o_add, int mode) const {
        if (!batch) return vsr_launch_pack_weights(dt, w, dst, KK, RP, CPd, r_real, c_real, I_total, i_off, o_mul, o_add, mode, st);
        VsrPackDesc d = {};
        d.w = w; d.dst = dst; d.total = KK * RP * CPd;
        d.KK = (short)KK; d.RP = (short)RP; d.CPd = (short)CPd; d.r_real = (short)r_real; d.c_real = (short)c_real;
        d.I_total = (short)I_total; d.i_off = (short)i_off; d.o_mul = (short)o_mul; d.o_add = (short)o_add;
        d.mode = (unsigned char)mode; d.dtype = (unsigned char)dt;
        batch->push_back(d);
        return VSR_OK;
    }
};
