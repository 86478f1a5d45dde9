// Test hooks for the propagation trunk (not in the header): each runs ONE launch, or one recipe, of the trunk on the caller's buffers
// through the Ctx member (recipes.h) or launcher the engines call, with the weight packs engine.hip / cleaner_engine.hip make for that
// layer.  Argument checks and launches only: no kernel lives here.  tests/test_trunk_gpu.py compares every hook with an fp64 restatement.
//   C: the mid-channel width (16, 32 or 64); w: fp32 OIHW; *_pm: blocked pixel-major, C channels, element type of `dtype`;
//   wpack / slab: caller scratch; x[] / dy[] of the weight gradients: HOST arrays of device pointers, one per segment.
// Sign bits and chains exist on the persistent 64-channel bf16 kernels only: VSR_ERR_UNSUPPORTED at another width or in fp32.
#include "recipes.h"
#include "debug_hooks.h"

namespace {
bool bad_width(int C) { return C != 16 && C != 32 && C != 64; }
bool bits_ok(int dtype, int C) { return dtype == VSR_BF16 && C == 64; }
bool bad_mask(int mask, const void* aux) { return aux ? (mask != MASK_RELU && mask != MASK_LEAKY) : mask != MASK_NONE; }
bool bad_segs(const void* const* p, int n) {
    for (int i = 0; i < n; ++i) if (!p[i]) return true;
    return false;
}
}  // namespace

extern "C" {

// Ctx::conv on Ctx::pack_cc(ks, mode)'s weights: y = act(conv(x) + bias) (+ res) (* mask(aux)), C -> C, ks 3 or 1; mode 0 forward
// weights, 1 data-gradient weights.  res may be y (in place).  sign_out: the launch writes the sign bits of y there; sign_bits: the
// launch masks from them instead of aux; make_bits: vsr_launch_sign_bits_c64(aux) fills sign_bits first (what the engine does for the
// stem's output).  unshuffle: y as four phase planes (ks 3, H and W even).  wpack: ks * ks * max(C, 32) * C elements;
// sign words: N * ceil(H/8) * ceil(W/32) * 2048 bytes.
int vsr_debug_trunk_conv(int dtype, int C, int ks, int mode, const void* x_pm, const float* w, const float* bias, void* wpack, void* y_pm, int act,
                         float slope, const void* res_pm, const void* aux_pm, int mask, void* sign_out, void* sign_bits, int make_bits, int unshuffle,
                         int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || (ks != 1 && ks != 3) || (mode & ~1) || !x_pm || !w || !wpack || !y_pm || bad_dims(N, H, W) ||
        act < ACT_NONE || act > ACT_LEAKY || bad_mask(mask, aux_pm) || (make_bits & ~1) || (unshuffle & ~1))
        return VSR_ERR_BADARG;
    if ((sign_bits && !aux_pm) || (make_bits && !sign_bits)) return VSR_ERR_BADARG;
    if (unshuffle && (ks != 3 || (H & 1) || (W & 1))) return VSR_ERR_BADARG;
    if ((sign_out || sign_bits || unshuffle) && (!bits_ok(dtype, C) || ks != 3)) return VSR_ERR_UNSUPPORTED;
    if (sign_out && (act == ACT_NONE || res_pm || aux_pm)) return VSR_ERR_UNSUPPORTED;                // the bits are an activation's, written by the plain arms
    if (unshuffle && mask != MASK_NONE) return VSR_ERR_UNSUPPORTED;                                   // no kernel masks a phase-separated destination
    const Ctx c(nullptr, (hipStream_t)stream, dtype, C);
    CK(c.pack_cc(ks, w, wpack, mode));
    if (make_bits) CK(vsr_launch_sign_bits_c64(aux_pm, sign_bits, N, H, W, c.st));
    return c.conv(ks, x_pm, wpack, bias, y_pm, act, res_pm, aux_pm, mask, N, H, W, sign_out, sign_bits, unshuffle != 0, slope);
}

// Ctx::stem on Ctx::pack_stem's weights: y = act(conv3x3(cat([lr, feat])) + bias) (cat) or act(conv3x3(lr) + bias).  lr: planar fp32, 3 planes,
// images lr_nstride floats apart; feat_pm NULL with cat: the zero state of a direction's first frame.  w (C, cat ? C + 3 : 3, 3, 3);
// wpack: 9 * max(C, 32) * (cat ? C + 16 : 16) elements.
int vsr_debug_trunk_stem(int dtype, int C, int cat, const void* feat_pm, const float* lr, long long lr_nstride, const float* w, const float* bias,
                         void* wpack, void* y_pm, int act, float slope, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || (cat & ~1) || !lr || !w || !wpack || !y_pm || bad_dims(N, H, W) || lr_nstride < (long long)3 * H * W ||
        (act != ACT_NONE && act != ACT_LEAKY) || (!cat && feat_pm))
        return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, C);
    CK(c.pack_stem(w, wpack, cat != 0));
    return c.stem(cat != 0, feat_pm, lr, lr_nstride, wpack, bias, y_pm, act, slope, N, H, W);
}

// The stem's two data gradients of g0 (N, H, W, C): towards feat (dfeat_pm; cat only) -- Ctx::conv on Ctx::pack_stem_dgrad's weights -- and
// towards the 3 LR channels (dlr: planar fp32, images dlr_nstride floats apart) -- Ctx::conv_planar3 on Ctx::pack_stem_dlr's, with
// pres == dlr when `accumulate` (the engine adds both directions' gradients into dlrs in place).  Either destination may be NULL.
// wpack: 9 * max(C, 32) * C + 9 * 32 * C elements.
int vsr_debug_trunk_stem_dgrad(int dtype, int C, int cat, const void* g0_pm, const float* w, void* wpack, void* dfeat_pm, float* dlr,
                               long long dlr_nstride, int accumulate, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || (cat & ~1) || !g0_pm || !w || !wpack || (!dfeat_pm && !dlr) || bad_dims(N, H, W) || (accumulate & ~1) ||
        (dfeat_pm && !cat) || (dlr && dlr_nstride < (long long)3 * H * W))
        return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, C);
    void* wpack_lr = (char*)wpack + (size_t)9 * c.CO * C * c.es;
    if (dfeat_pm) {
        CK(c.pack_stem_dgrad(w, wpack));
        CK(c.conv(3, g0_pm, wpack, nullptr, dfeat_pm, ACT_NONE, nullptr, nullptr, 0, N, H, W));
    }
    if (dlr) {
        CK(c.pack_stem_dlr(w, wpack_lr, cat != 0));
        CK(c.conv_planar3(g0_pm, wpack_lr, nullptr, dlr, dlr_nstride, accumulate ? dlr : nullptr, N, H, W));
    }
    return VSR_OK;
}

// The 1x1 fusion conv on Ctx::pack_point's weights.  backward = 0: Ctx::point_conv, y0 = LeakyReLU(conv1x1(cat([a, b])) + bias);
// backward = 1: Ctx::point_dgrad of a_pm, y0 = the gradient towards the first C inputs, y1 towards the second.  w (C, 2C, 1, 1);
// wpack: 2 * max(C, 32) * C elements.
int vsr_debug_trunk_point(int dtype, int C, int backward, const void* a_pm, const void* b_pm, const float* w, const float* bias, void* wpack,
                          void* y0_pm, void* y1_pm, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || (backward & ~1) || !a_pm || !w || !wpack || !y0_pm || bad_dims(N, H, W)) return VSR_ERR_BADARG;
    if (backward ? (!y1_pm || b_pm || bias) : (!b_pm || y1_pm)) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, C);
    CK(c.pack_point(w, wpack, backward));
    if (backward) return c.point_dgrad(a_pm, wpack, y0_pm, y1_pm, N, H, W);
    return c.point_conv(a_pm, b_pm, wpack, bias, y0_pm, N, H, W);
}

// Ctx::wgrad_cc(ks, ...) over nseg (1..VSR_WG_MAXSEG) pairs (x[i], dy[i]), each N x H x W x C: gw (C, I_total, ks, ks) receives input channels
// [i_off, i_off + C); gb (C) or NULL; accumulate: add to what gw / gb hold, else overwrite (the rest of gw is left alone either way).
// slab: vsr_conv3x3_c64_wgrad_slab_floats() floats.
int vsr_debug_trunk_wgrad_cc(int dtype, int C, int ks, const void* const* x, const void* const* dy, int nseg, float* gw, int I_total, int i_off,
                             float* gb, int accumulate, float* slab, int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || (ks != 1 && ks != 3) || !x || !dy || !gw || !slab || bad_dims(N, H, W) || (accumulate & ~1) ||
        nseg < 1 || nseg > VSR_WG_MAXSEG || i_off < 0 || I_total < i_off + C)
        return VSR_ERR_BADARG;
    if (bad_segs(x, nseg) || bad_segs(dy, nseg)) return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, C, slab);
    WgradArgs a = wg_base(N, H, W, C, C);
    a.nseg = nseg;
    for (int i = 0; i < nseg; ++i) { a.x[i] = x[i]; a.dy[i] = dy[i]; }
    return c.wgrad_cc(ks, a, gw, I_total, i_off, gb, accumulate);
}

// Ctx::stem_wgrads: gw (C, cat ? C + 3 : 3, 3, 3) and gb (C) from nseg (1..VSR_WG_MAXSEG) LR segments (lr[i]: planar fp32, 3 planes, images
// x_nstride floats apart; g0[i]: N x H x W x C) and -- cat -- nseg_feat (0..nseg: a direction's first frame has no state) feat
// segments (feat[i], g0_feat[i]).
int vsr_debug_trunk_stem_wgrads(int dtype, int C, int cat, const float* const* lr, long long x_nstride, const void* const* g0, int nseg,
                                const void* const* feat, const void* const* g0_feat, int nseg_feat, float* gw, float* gb, int accumulate, float* slab,
                                int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || (cat & ~1) || !lr || !g0 || !gw || !slab || bad_dims(N, H, W) || (accumulate & ~1) ||
        nseg < 1 || nseg > VSR_WG_MAXSEG || nseg_feat < 0 || nseg_feat > nseg || (!cat && nseg_feat) || (nseg_feat && (!feat || !g0_feat)) ||
        x_nstride < (long long)3 * H * W)
        return VSR_ERR_BADARG;
    if (bad_segs(reinterpret_cast<const void* const*>(lr), nseg) || bad_segs(g0, nseg) || (nseg_feat && (bad_segs(feat, nseg_feat) || bad_segs(g0_feat, nseg_feat))))
        return VSR_ERR_BADARG;
    const Ctx c(nullptr, (hipStream_t)stream, dtype, C, slab);
    WgradArgs a = wg_base(N, H, W, C, C), af = a;
    a.nseg = nseg; af.nseg = nseg_feat;
    a.x_nstride = x_nstride;
    for (int i = 0; i < nseg; ++i) { a.x[i] = lr[i]; a.dy[i] = g0[i]; }
    for (int i = 0; i < nseg_feat; ++i) { af.x[i] = feat[i]; af.dy[i] = g0_feat[i]; }
    return c.stem_wgrads(cat != 0, a, af, gw, gb, accumulate);
}

// vsr_launch_conv3x3_chain on an explicit layer list: layers[8 l .. 8 l + 7] = ChainLayer's src, dst, res, sbits, sout, w, bias, variant, the
// first seven as offsets in units of 256 bytes from `base` (0xffffffff: none).  w[l] (host array; an entry may be NULL: the slot is
// packed already): fp32 OIHW weights of layer l, packed into its slot by Ctx::pack_cc(3, ., mode) (0 forward chain, 1 backward chain)
// before the launch.  sync: vsr_conv3x3_c64_chain_sync_bytes(nlayers, N, H, W) bytes.  bf16, 64 channels.
int vsr_debug_trunk_chain(int dtype, int C, void* base, void* sync, const unsigned* layers, int nlayers, const float* const* w, int mode,
                          int N, int H, int W, void* stream) {
    if (bad_dtype(dtype) || bad_width(C) || !base || !sync || !layers || nlayers < 1 || nlayers > VSR_CHAIN_MAX_LAYERS || (mode & ~1) ||
        bad_dims(N, H, W) || ((uintptr_t)base & 255))
        return VSR_ERR_BADARG;
    if (!bits_ok(dtype, C)) return VSR_ERR_UNSUPPORTED;
    const Ctx c((char*)base, (hipStream_t)stream, dtype, C);
    ChainArgs a = {};
    a.base = c.ws; a.sync = (unsigned*)sync; a.N = N; a.H = H; a.W = W; a.nlayers = nlayers;
    for (int l = 0; l < nlayers; ++l) {
        const unsigned* v = layers + 8 * l;
        a.layer[l] = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], (int)v[7]};
        if (v[5] == 0xffffffffu) return VSR_ERR_BADARG;
    }
    if (w)
        for (int l = 0; l < nlayers; ++l)
            if (w[l]) CK(c.pack_cc(3, w[l], c.at((size_t)a.layer[l].w << 8), mode));
    return vsr_launch_conv3x3_chain(a, vsr_num_cus(), c.st);
}

}  // extern "C"
