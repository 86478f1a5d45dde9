// RealBasicVSR's pre-clean stack (realbasicvsr.py:17-30) as one engine call each way: a plan that is a pure function of the
// arguments, work only enqueued on the given stream.
#include "recipes.h"

extern "C" {

// ---- RealBasicVSR pre-clean stack, forward (realbasicvsr.py:17-30) ------------------------------------
// x <- x + conv(ResidualBlock(x)), `steps` times, on the F = n*t frames of the clip.
// params: resblock.conv.0.{weight,bias}, resblock.res_block.{i}.conv{1,2}.{weight,bias} ..., conv.{weight,bias}
struct CleanPlan {
    size_t stem_w = 0, stem_b = 0, out_w = 0, out_b = 0, feat = 0, act = 0, xa = 0, xb = 0, total = 0;
    std::vector<size_t> blk_w, blk_b;
    // need_backward: data-gradient weights, per-step saved tensors, backward scratch
    bool save = false;
    size_t stem_wd = 0, out_wd = 0, slab = 0, dXa = 0, dXb = 0, dA = 0, G0 = 0, dxa = 0, dxb = 0;
    std::vector<size_t> blk_wd;
    std::vector<size_t> xs;             // [steps]: planar fp32 input of each step (xs[0] unused: the caller's lr)
    std::vector<size_t> X, A;           // [steps][blocks+1] / [steps][blocks]
};
// C: mid channels (64, or 16 / 32 through vsr_cleaner_narrow_workspace_bytes); CO: packed rows of a C-output weight set
static CleanPlan clean_plan(int F, int h, int w, int blocks, int dtype, int steps, bool save, int C = 64) {
    CleanPlan p; Bump b;
    const int CO = C < 32 ? 32 : C;
    const size_t es = esize(dtype), w64 = (size_t)9 * CO * C * es;
    p.stem_w = b.take((size_t)9 * CO * 16 * es); p.stem_b = b.take(C * 4);
    p.blk_w.resize(2 * blocks); p.blk_b.resize(2 * blocks);
    for (int k = 0; k < 2 * blocks; ++k) { p.blk_w[k] = b.take(w64); p.blk_b[k] = b.take(C * 4); }
    p.out_w = b.take((size_t)9 * 32 * C * es); p.out_b = b.take(64 * 4);
    const size_t a1 = (size_t)F * pm_image_elems(h, w, C) * es;
    const size_t x1 = (size_t)F * 3 * h * w * 4;
    p.feat = b.take(a1); p.act = b.take(a1);
    p.xa = b.take(x1); p.xb = b.take(x1);
    p.save = save;
    if (save) {                                   // appended: the forward-only offsets do not move
        p.stem_wd = b.take((size_t)9 * 32 * C * es); p.out_wd = b.take((size_t)9 * CO * 16 * es);
        p.blk_wd.resize(2 * blocks);
        for (int k = 0; k < 2 * blocks; ++k) p.blk_wd[k] = b.take(w64);
        p.slab = b.take(wgrad_slab_bytes());
        p.dXa = b.take(a1); p.dXb = b.take(a1); p.dA = b.take(a1); p.G0 = b.take(a1);
        p.dxa = b.take(x1); p.dxb = b.take(x1);
        p.xs.assign(steps, 0); p.X.assign((size_t)steps * (blocks + 1), 0); p.A.assign((size_t)steps * blocks, 0);
        for (int s = 0; s < steps; ++s) {
            if (s > 0) p.xs[s] = b.take(x1);
            for (int k = 0; k <= blocks; ++k) p.X[(size_t)s * (blocks + 1) + k] = b.take(a1);
            for (int k = 0; k < blocks; ++k) p.A[(size_t)s * blocks + k] = b.take(a1);
        }
    }
    p.total = b.off;
    return p;
}

size_t vsr_cleaner_workspace_bytes(int F, int h, int w, int blocks, int steps, int dtype, int need_backward) {
    if (F < 1 || h < 1 || w < 1 || blocks < 0 || steps < 1) return 0;
    return clean_plan(F, h, w, blocks, dtype, steps, need_backward != 0).total;
}

size_t vsr_cleaner_narrow_workspace_bytes(int F, int h, int w, int mid_channels, int blocks, int steps, int dtype, int need_backward) {
    if (F < 1 || h < 1 || w < 1 || blocks < 0 || steps < 1 || (mid_channels != 16 && mid_channels != 32)) return 0;
    if (dtype != VSR_F32 && dtype != VSR_BF16) return 0;
    return clean_plan(F, h, w, blocks, dtype, steps, need_backward != 0, mid_channels).total;
}
static bool cleaner_width_ok(int mid_channels) { return mid_channels == 64 || mid_channels == 32 || mid_channels == 16; }

int vsr_cleaner_forward(int F, int h, int w, int mid_channels, int blocks, int steps, int dtype, const float* const* params,
                        int nparams, const float* lr, float* lq, void* workspace, size_t workspace_bytes, int need_backward,
                        void* stream) {
    if (F < 1 || h < 1 || w < 1 || blocks < 0 || steps < 1 || !params || !lr || !lq || !workspace) return VSR_ERR_BADARG;
    if (!cleaner_width_ok(mid_channels)) return VSR_ERR_UNSUPPORTED;
    if (bad_dtype(dtype) || nparams != 4 + 4 * blocks) return VSR_ERR_BADARG;
    const bool save = need_backward != 0;
    const int C = mid_channels;
    const CleanPlan p = clean_plan(F, h, w, blocks, dtype, steps, save, C);
    if (workspace_bytes < p.total) return VSR_ERR_WORKSPACE;
    const Ctx c((char*)workspace, (hipStream_t)stream, dtype, C);
    const int CO = c.CO;
    CK(c.pack_stem(params[0], c.at(p.stem_w), false));
    CK(c.pack_bias(params[1], c.at(p.stem_b), C));
    for (int k = 0; k < 2 * blocks; ++k) {
        CK(c.pack_cc(3, params[2 + 2 * k], c.at(p.blk_w[k]), 0));
        CK(c.pack_bias(params[3 + 2 * k], c.at(p.blk_b[k]), C));
        if (save) CK(c.pack_cc(3, params[2 + 2 * k], c.at(p.blk_wd[k]), 1));
    }
    CK(c.pack(params[2 + 4 * blocks], c.at(p.out_w), 9, 32, C, 3, C, C, 0, 1, 0, 0));
    CK(c.pack_bias(params[3 + 4 * blocks], c.at(p.out_b), 3));
    if (save) {
        CK(c.pack_stem_dlr(params[0], c.at(p.stem_wd), false));                            // C -> 3 (planar epilogue)
        CK(c.pack(params[2 + 4 * blocks], c.at(p.out_wd), 9, CO, 16, C, 3, C, 0, 1, 0, 1));     // 3 (planar source) -> C
    }
    const float* xin = lr;
    for (int s = 0; s < steps; ++s) {
        float* xout = (s == steps - 1) ? lq : (float*)c.at(save ? p.xs[s + 1] : ((s & 1) ? p.xb : p.xa));
        auto Xs = [&](int k) { return save ? c.at(p.X[(size_t)s * (blocks + 1) + k]) : c.at(p.feat); };
        // ResidualBlock stem: conv3x3 3->64 + LeakyReLU(0.1) on the planar frames (conv.py:97)
        CK(c.stem(false, nullptr, xin, (long long)3 * h * w, c.at(p.stem_w), c.fat(p.stem_b), Xs(0), ACT_LEAKY, 0.f, F, h, w));
        for (int b = 0; b < blocks; ++b) {
            void* act = save ? c.at(p.A[(size_t)s * blocks + b]) : c.at(p.act);
            CK(c.conv(3, Xs(b), c.at(p.blk_w[2 * b]), c.fat(p.blk_b[2 * b]), act, ACT_RELU, nullptr, nullptr, 0, F, h, w));
            CK(c.conv(3, act, c.at(p.blk_w[2 * b + 1]), c.fat(p.blk_b[2 * b + 1]), Xs(b + 1), ACT_NONE, Xs(b), nullptr, 0, F, h, w));
        }
        // x + conv3x3 64->3 (realbasicvsr.py:28-29; a fresh tensor instead of the reference's in-place +=)
        CK(c.conv_planar3(Xs(blocks), c.at(p.out_w), c.fat(p.out_b), xout, (long long)3 * h * w, xin, F, h, w));
        xin = xout;
    }
    return VSR_OK;
}

// Backward of the above for the cotangent dlq (F,3,h,w): grads[k] (the 4 + 4*blocks tensors; NULL = not wanted, a bias
// needs its weight's entry) are ACCUMULATED into; dlr (F,3,h,w, optional) is written.  The parameters are shared by the
// `steps` iterations, so each iteration adds its weight gradients.
int vsr_cleaner_backward(int F, int h, int w, int mid_channels, int blocks, int steps, int dtype, float* const* grads, int nparams,
                         const float* lr, const float* dlq, float* dlr, void* workspace, size_t workspace_bytes, void* stream) {
    if (F < 1 || h < 1 || w < 1 || blocks < 0 || steps < 1 || !grads || !lr || !dlq || !workspace) return VSR_ERR_BADARG;
    if (!cleaner_width_ok(mid_channels) || blocks < 1) return VSR_ERR_UNSUPPORTED;      // the stem's LeakyReLU mask is fused into block 0's dgrad
    if (bad_dtype(dtype) || nparams != 4 + 4 * blocks) return VSR_ERR_BADARG;
    const int C = mid_channels;
    const CleanPlan p = clean_plan(F, h, w, blocks, dtype, steps, true, C);
    if (workspace_bytes < p.total) return VSR_ERR_WORKSPACE;
    const Ctx c((char*)workspace, (hipStream_t)stream, dtype, C, (float*)((char*)workspace + p.slab));
    const float* dx = dlq;                                   // gradient w.r.t. x_{s+1}
    for (int s = steps - 1; s >= 0; --s) {
        const float* xs = s == 0 ? lr : c.fat(p.xs[s]);
        auto Xs = [&](int k) { return c.at(p.X[(size_t)s * (blocks + 1) + k]); };
        auto As = [&](int k) { return c.at(p.A[(size_t)s * blocks + k]); };
        float* gow = grads[2 + 4 * blocks]; float* gob = grads[3 + 4 * blocks];
        {   // out conv C->3: X = X_blocks, dY = dx (planar)
            WgradArgs a = wg_base(F, h, w, C, C);
            a.x[0] = Xs(blocks); a.dy[0] = dx; a.dy_nstride = (long long)3 * h * w;
            CK(c.wgrad(a, {3, C, false, 16, true}, {3, C, gow, C, 0, 1, 0, gob, 1}));
        }
        size_t dcur = p.dXa, dnext = p.dXb;
        // d X_blocks = dgrad(out conv)(dx): planar 3 -> C, the stem's launch on the flipped weights
        CK(c.stem(false, nullptr, dx, (long long)3 * h * w, c.at(p.out_wd), nullptr, c.at(dcur), ACT_NONE, 0.f, F, h, w));
        for (int b = blocks - 1; b >= 0; --b) {   // x + conv2(relu(conv1(x)))   (conv.py:89-92)
            CK(c.conv(3, c.at(dcur), c.at(p.blk_wd[2 * b + 1]), nullptr, c.at(p.dA), ACT_NONE, nullptr, As(b), MASK_RELU, F, h, w));
            {
                WgradArgs a = wg_base(F, h, w, C, C);
                a.x[0] = As(b); a.dy[0] = c.at(dcur);
                CK(c.wgrad_cc(3, a, grads[2 + 2 * (2 * b + 1)], C, 0, grads[3 + 2 * (2 * b + 1)], 1));
            }
            void* out = b > 0 ? c.at(dnext) : c.at(p.G0);      // b == 0: also through the stem's LeakyReLU
            CK(c.conv(3, c.at(p.dA), c.at(p.blk_wd[2 * b]), nullptr, out, ACT_NONE, c.at(dcur), b == 0 ? Xs(0) : nullptr,
                        b == 0 ? MASK_LEAKY : 0, F, h, w));
            {
                WgradArgs a = wg_base(F, h, w, C, C);
                a.x[0] = Xs(b); a.dy[0] = c.at(p.dA);
                CK(c.wgrad_cc(3, a, grads[2 + 2 * (2 * b)], C, 0, grads[3 + 2 * (2 * b)], 1));
            }
            const size_t tmp = dcur; dcur = dnext; dnext = tmp;
        }
        const void* g0 = c.at(p.G0);
        {   // stem 3->C: X = x_s (planar), dY = G0
            WgradArgs a = wg_base(F, h, w, C, C);
            a.x[0] = xs; a.x_nstride = (long long)3 * h * w; a.dy[0] = g0;
            CK(c.stem_wgrads(false, a, a, grads[0], grads[1], 1));
        }
        const bool last = s == 0;
        if (!last || dlr) {   // d x_s = d x_{s+1} + dgrad(stem)(G0)
            float* dxs = last ? dlr : (float*)c.at((s & 1) ? p.dxa : p.dxb);
            CK(c.conv_planar3(g0, c.at(p.stem_wd), nullptr, dxs, (long long)3 * h * w, dx, F, h, w));
            dx = dxs;
        }
    }
    return VSR_OK;
}

}  // extern "C"
