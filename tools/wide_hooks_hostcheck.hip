// Stand-alone host check of csrc/wide_hooks.hip: the hooks' argument checks and what they hand to the launch layer, with every device
// launch stubbed, for a run under ASan / UBSan on a machine without a GPU (the launch layer below the hooks is hostcheck_launch_layer.h's
// recorders).
//   make -C vsrlab_amd/csrc hooks_hostcheck        (or the target wide_hostcheck alone)
// Exit status 0 and "wide hostcheck OK": every refusal came back before any pack or launch; every accepted vsr_debug_wide_conv reached the
// pack of its mode and vsr_launch_conv_wide with the slices, output blocks, steps, image sizes, epilogue operands and max_wg of its mode;
// vsr_debug_wide_wgrad reached vsr_launch_wgrad_pairs with the ksplit of WideCtx::pair_ksplit for every layer geometry at 1, 8 and 200
// tiles (bf16), or the pair-by-pair path with each pair's parity view, channel slices and destination block (fp32).
#define HOSTCHECK_NAME "wide hostcheck"
#include "hostcheck_launch_layer.h"

int main() {
    float* f = hostcheck_buffer();
    void* v = f;
    char* cb = reinterpret_cast<char*>(f);
    double* dd = reinterpret_cast<double*>(cb + 16384);
    const int BF = VSR_BF16, FP = VSR_F32, n = 2, h = 13, w = 37;
    const long long BIG = 1LL << 40;

    // ---- the wide conv ----
    REFUSED(vsr_debug_wide_conv(2, 0, 128, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 4, 128, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 96, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);      // channels: multiples of 64
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 32, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 0, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, nullptr, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, nullptr, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, nullptr, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, v, BIG, nullptr, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, v, BIG, v, 3, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, -1, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, 0, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_conv(BF, 0, 128, 64, v, f, f, v, vsr_wide2_pack_elems(128, 64, 0) - 1, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_WORKSPACE);
    REFUSED(vsr_debug_wide_conv(FP, 3, 128, 64, v, f, f, v, vsr_wide_pack_elems(128, 64, 3) - 1, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, n, h, w, nullptr), VSR_ERR_WORKSPACE);
    REFUSED(vsr_debug_wide_conv(FP, 0, 128, 64, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 3, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);          // the cap is conv_wide2's
    REFUSED(vsr_debug_wide_conv(FP, 3, 64, 512, v, f, f, v, BIG, v, 0, 0.2f, nullptr, nullptr, nullptr, 0, 2048, h, w, nullptr), VSR_ERR_UNSUPPORTED);      // grid.z over 65535
    for (int dt = 0; dt < 2; ++dt)
        for (int mode = 0; mode < 4; ++mode)
            for (int geo = 0; geo < 2; ++geo) {
                const int cout = geo ? 128 : 256, cin = geo ? (mode >= 2 ? 64 : 128) : 512;                // geo 1: 64 output rows for modes 2, 3 (K-split)
                const bool epi = mode == 0 || mode == 3;
                reset();
                EXPECT(vsr_debug_wide_conv(dt ? BF : FP, mode, cout, cin, v, f, mode < 2 ? f + 64 : nullptr, cb + 4096, BIG, cb + 8192, mode < 2 ? ACT_LEAKY : ACT_NONE, 0.2f,
                                           epi ? cb + 12288 : nullptr, epi ? cb + 2048 : nullptr, mode >= 2 ? cb + 6144 : nullptr, dt ? 3 : 0, n, h, w, nullptr) == VSR_OK);
                EXPECT(g_pack.size() == 1 && g_pack[0].w2 == dt && g_pack[0].dtype == (dt ? BF : FP) && g_pack[0].cout == cout && g_pack[0].cin == cin && g_pack[0].mode == mode &&
                       g_pack[0].dst == cb + 4096);
                EXPECT(g_wide.size() == 1 && launches() == 1);
                if (g_wide.size() != 1) continue;
                const VsrWideConv& c = g_wide[0].c;
                const int xC = mode >= 2 ? cout : cin, yC = mode >= 2 ? cin : cout, is_ = mode == 1 ? 2 : 1, os = mode == 3 ? 2 : 1;
                EXPECT(g_wide[0].dtype == (dt ? BF : FP) && c.x == v && c.xC == xC && c.nsl == xC / 64 && c.Hx == h * is_ && c.Wx == w * is_ && c.in_step == is_);
                EXPECT(c.N == n && c.H == h && c.W == w && c.y == cb + 8192 && c.yC == yC && c.ncob == yC / 64 && c.Hy == h * os && c.Wy == w * os && c.out_step == os);
                EXPECT(dt ? (c.wpack2 == cb + 4096 && !c.wpack) : (c.wpack == cb + 4096 && !c.wpack2));
                EXPECT(c.bias == (mode < 2 ? f + 64 : nullptr) && c.act == (mode < 2 ? ACT_LEAKY : ACT_NONE) && c.slope == 0.2f && !c.y_pre && c.max_wg == (dt ? 3 : 0));
                EXPECT(c.y_act == (epi ? cb + 12288 : nullptr) && c.res == (epi ? cb + 2048 : nullptr) && c.aux == (mode >= 2 ? cb + 6144 : nullptr));
                EXPECT(!(c.in_step == 2 && c.out_step == 2));
            }

    // ---- the weight gradient of a wide layer ----
    const long long NF = (long long)wide_slab_floats();
    REFUSED(vsr_debug_wide_wgrad(3, 1, 128, 64, v, v, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 2, 128, 64, v, v, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);                  // views: 1 or 4
    REFUSED(vsr_debug_wide_wgrad(BF, 0, 128, 64, v, v, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 100, 64, v, v, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 8, v, v, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 64, nullptr, v, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 64, v, nullptr, f, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 64, v, v, nullptr, f, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 64, v, v, f, nullptr, NF, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 64, v, v, f, f, NF, n, 0, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_wgrad(BF, 1, 128, 64, v, v, f, f, NF - 1, n, h, w, nullptr), VSR_ERR_WORKSPACE);
    REFUSED(vsr_debug_wide_wgrad(BF, 4, 512, 512, v, v, f, f, NF, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);            // 256 pairs x 8 parts > VSR_WGRAD_MAX_PAIR_SLABS
    const int GEO[6][3] = {{1, 128, 64}, {1, 256, 128}, {1, 512, 256}, {4, 64, 128}, {4, 128, 256}, {4, 256, 512}};      // views, xC, dyC: conv_6, 5, 4, 1, 2, 3
    const int DOM[3][3] = {{1, 1, 1}, {1, 16, 128}, {1, 80, 640}};                                                      // 1, 8 and 200 tiles
    for (const auto& g : GEO)
        for (const auto& d : DOM) {
            const int views = g[0], xC = g[1], dyC = g[2], st = views == 4 ? 2 : 1, npairs = (xC / 64) * (dyC / 64) * views;
            const int tiles = d[0] * ((d[1] + 7) / 8) * ((d[2] + 31) / 32);
            reset();
            EXPECT(vsr_debug_wide_wgrad(BF, views, xC, dyC, v, cb + 4096, f + 256, f + 1024, NF, d[0], d[1], d[2], nullptr) == VSR_OK);
            EXPECT(g_pairs.size() == 1 && launches() == 1);
            if (g_pairs.size() != 1) continue;
            const PairsCall& p = g_pairs[0];
            int want = ((512 / npairs) + 7) & ~7;
            if (want < 8) want = 8;
            if (want > ((tiles + 7) & ~7)) want = (tiles + 7) & ~7;
            EXPECT(p.ksplit == want && p.ksplit >= 8 && (p.ksplit & 7) == 0 && (long long)npairs * p.ksplit <= VSR_WGRAD_MAX_PAIR_SLABS);
            EXPECT(tiles != 1 || p.ksplit == 8);                                                                        // one tile: seven of eight parts are empty
            EXPECT(p.nsl == xC / 64 && p.ncob == dyC / 64 && p.views == views && p.cin_total == xC && p.gw == f + 256);
            EXPECT(p.a.x[0] == v && p.a.dy[0] == cb + 4096 && p.a.slab == f + 1024 && p.a.slab_stride == wgrad_slab_stride3() && p.a.nseg == 1);
            EXPECT(p.a.N == d[0] && p.a.H == d[1] && p.a.W == d[2] && p.a.x_step == st && p.a.Hx == d[1] * st && p.a.Wx == d[2] * st && p.a.dy_step == 1 &&
                   p.a.Hy == d[1] && p.a.Wy == d[2] && p.a.x_ctotal == xC && p.a.dy_ctotal == dyC &&
                   p.a.x_nstride == pm_image_elems(d[1] * st, d[2] * st, xC) && p.a.dy_nstride == pm_image_elems(d[1], d[2], dyC));
        }
    // fp32: pair by pair, views outermost, then cout blocks, then cin slices
    for (int views = 1; views <= 4; views += 3) {
        const int xC = 128, dyC = 192, st = views == 4 ? 2 : 1;
        reset();
        EXPECT(vsr_debug_wide_wgrad(FP, views, xC, dyC, v, cb + 4096, f + 256, f + 1024, NF, n, h, w, nullptr) == VSR_OK);
        const int npairs = 2 * 3 * views;
        EXPECT((int)g_wgrad.size() == npairs && (int)g_reduce.size() == npairs && g_pairs.empty());
        for (int i = 0; i < npairs && i < (int)g_wgrad.size() && i < (int)g_reduce.size(); ++i) {
            const int s = i % 2, o = (i / 2) % 3, vw = i / 6;
            const WgradCall& c = g_wgrad[i];
            const ReduceCall& r = g_reduce[i];
            EXPECT(c.ks == 3 && c.cx == 64 && c.cout == 64 && !c.x_planar && !c.dy_planar && c.a.x[0] == v && c.a.dy[0] == cb + 4096 && c.a.slab == f + 1024);
            EXPECT(c.a.x_step == st && c.a.x_oy == (views == 4 ? vw >> 1 : 0) && c.a.x_ox == (views == 4 ? vw & 1 : 0) && c.a.Hx == h * st && c.a.Wx == w * st);
            EXPECT(c.a.x_ctotal == xC && c.a.x_coff == s * 8 && c.a.dy_ctotal == dyC && c.a.dy_coff == o * 8 && c.a.N == n && c.a.H == h && c.a.W == w);
            if (views == 4) EXPECT(r.s2 == 1 && r.view == vw && r.co0 == 64 * o && r.ci0 == 64 * s && r.cin_total == xC && r.gw == f + 256 && r.nwg == c.nwg);
            else EXPECT(r.s2 == 0 && r.gw == f + 256 + (size_t)64 * o * xC * 9 && r.I_total == xC && r.i_off == 64 * s && r.accumulate == 1 && r.nwg == c.nwg);
        }
    }

    // ---- up2, its adjoint, the mask ----
    REFUSED(vsr_debug_wide_up2_fwd(2, v, v, v, n, h, w, 128, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_fwd(BF, nullptr, v, v, n, h, w, 128, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_fwd(BF, v, v, nullptr, n, h, w, 128, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_fwd(BF, v, v, v, n, h, w, 12, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_fwd(BF, v, v, v, n, 0, w, 128, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_fwd(BF, v, v, v, 65536, h, w, 128, nullptr), VSR_ERR_UNSUPPORTED);
    for (int with = 0; with < 2; ++with) {
        reset();
        EXPECT(vsr_debug_wide_up2_fwd(with ? BF : FP, v, with ? cb + 2048 : nullptr, cb + 4096, n, 1, 5, 256, nullptr) == VSR_OK);
        EXPECT(g_elt.size() == 1 && is(g_elt[0], "up2_fwd") && g_elt[0].p[0] == v && g_elt[0].p[1] == (with ? cb + 2048 : nullptr) && g_elt[0].p[2] == cb + 4096 &&
               g_elt[0].v[0] == (with ? BF : FP) && g_elt[0].v[1] == n && g_elt[0].v[2] == 1 && g_elt[0].v[3] == 5 && g_elt[0].v[4] == 256);
    }
    REFUSED(vsr_debug_wide_up2_bwd(BF, nullptr, v, v, v, 0.2f, n, h, w, 128, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_bwd(BF, v, v, nullptr, v, 0.2f, n, h, w, 128, nullptr), VSR_ERR_BADARG);               // din alone: no engine form
    REFUSED(vsr_debug_wide_up2_bwd(BF, v, v, v, nullptr, 0.2f, n, h, w, 128, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_bwd(BF, v, v, v, v, 0.2f, n, h, w, 4, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_up2_bwd(BF, v, v, v, v, 0.2f, n, 65536, w, 128, nullptr), VSR_ERR_UNSUPPORTED);
    for (int both = 0; both < 2; ++both) {
        reset();
        EXPECT(vsr_debug_wide_up2_bwd(both ? BF : FP, v, both ? cb + 2048 : nullptr, cb + 4096, cb + 6144, 0.2f, n, h, w, 512, nullptr) == VSR_OK);
        EXPECT(g_elt.size() == 1 && is(g_elt[0], "up2_bwd") && g_elt[0].p[0] == v && g_elt[0].p[1] == (both ? cb + 2048 : nullptr) && g_elt[0].p[2] == cb + 4096 &&
               g_elt[0].p[3] == cb + 6144 && g_elt[0].f == 0.2f && g_elt[0].v[1] == n && g_elt[0].v[2] == h && g_elt[0].v[3] == w && g_elt[0].v[4] == 512);
    }
    REFUSED(vsr_debug_wide_mask(2, v, v, v, 0.f, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_mask(BF, nullptr, v, v, 0.f, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_mask(BF, v, nullptr, v, 0.f, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_mask(BF, v, v, nullptr, 0.f, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_mask(BF, v, v, v, 0.f, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_mask(BF, v, v, v, 0.f, 12, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_wide_mask(FP, v, cb + 2048, cb + 4096, 0.f, 1LL << 33, nullptr) == VSR_OK);
    EXPECT(g_elt.size() == 1 && is(g_elt[0], "mask") && g_elt[0].p[1] == cb + 2048 && g_elt[0].p[2] == cb + 4096 && g_elt[0].v[1] == 1LL << 33 && g_elt[0].f == 0.f);

    // ---- VGG's pool and tap ----
    REFUSED(vsr_debug_vgg_pool(2, 0, v, nullptr, v, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_pool(BF, 2, v, nullptr, v, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_pool(BF, 0, v, v, v, n, h, w, 64, nullptr), VSR_ERR_BADARG);                                  // the forward has no dp
    REFUSED(vsr_debug_vgg_pool(BF, 1, v, nullptr, v, n, h, w, 64, nullptr), VSR_ERR_BADARG);                            // the backward needs one
    REFUSED(vsr_debug_vgg_pool(BF, 0, nullptr, nullptr, v, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_pool(BF, 0, v, nullptr, nullptr, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_pool(BF, 0, v, nullptr, v, n, 1, w, 64, nullptr), VSR_ERR_BADARG);                            // an empty output
    REFUSED(vsr_debug_vgg_pool(BF, 1, v, v, v, n, h, 1, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_pool(BF, 0, v, nullptr, v, n, h, w, 60, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_pool(BF, 0, v, nullptr, v, 65536, h, w, 64, nullptr), VSR_ERR_UNSUPPORTED);
    for (int op = 0; op < 2; ++op) {
        reset();
        EXPECT(vsr_debug_vgg_pool(op ? BF : FP, op, v, op ? cb + 2048 : nullptr, cb + 4096, n, h, w, 512, nullptr) == VSR_OK);
        EXPECT(g_elt.size() == 1 && is(g_elt[0], op ? "pool_bwd" : "pool_fwd") && g_elt[0].p[0] == v && g_elt[0].p[op ? 2 : 1] == cb + 4096 &&
               g_elt[0].v[0] == (op ? BF : FP) && g_elt[0].v[1] == n && g_elt[0].v[2] == h && g_elt[0].v[3] == w && g_elt[0].v[4] == 512);
        if (op) EXPECT(g_elt[0].p[1] == cb + 2048);
    }
    REFUSED(vsr_debug_vgg_tap(2, v, v, 1, 0.5f, dd, dd + 1024, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, nullptr, v, 1, 0.5f, dd, dd + 1024, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, v, nullptr, 1, 0.5f, dd, dd + 1024, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, v, v, 2, 0.5f, dd, dd + 1024, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, v, v, 1, 0.5f, nullptr, dd + 1024, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, v, v, 1, 0.5f, dd, nullptr, n, h, w, 64, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, v, v, 1, 0.5f, dd, dd + 1024, n, h, w, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_vgg_tap(BF, v, v, 1, 0.5f, dd, dd + 1024, 65536, h, w, 64, nullptr), VSR_ERR_UNSUPPORTED);
    for (int grad = 0; grad < 2; ++grad) {
        reset();
        EXPECT(vsr_debug_vgg_tap(grad ? BF : FP, v, cb + 2048, grad, 0.5f, dd, dd + 1024, n, 135, 240, 128, nullptr) == VSR_OK);
        const int nb = vsr_tap_blocks(135, 240, 128);      // 135 rows x 8 segments x 16 chunks x 32 pixels over 2048 per block
        EXPECT(nb == (135 * 8 * 16 * 32 + 2047) / 2048 && vsr_tap_blocks(1, 1, 64) == 1 && vsr_tap_blocks(2160, 3840, 64) == VSR_TAP_PMAX);
        EXPECT(g_elt.size() == 2 && is(g_elt[0], "tap_l1") && is(g_elt[1], "tap_sum"));
        if (g_elt.size() != 2) continue;
        EXPECT(g_elt[0].p[0] == v && g_elt[0].p[1] == cb + 2048 && g_elt[0].p[2] == (grad ? cb + 2048 : nullptr) && g_elt[0].p[3] == dd && g_elt[0].f == 0.5f &&
               g_elt[0].v[1] == n && g_elt[0].v[2] == 135 && g_elt[0].v[3] == 240 && g_elt[0].v[4] == 128 && g_elt[0].v[5] == nb);
        EXPECT(g_elt[1].p[0] == dd && g_elt[1].p[1] == dd + 1024 && g_elt[1].v[0] == n && g_elt[1].v[1] == nb && g_elt[1].v[2] == 0 && g_elt[1].v[5] == 0);
    }

    // ---- the grid entry hands its arguments on ----
    int out[3] = {0, 0, 0};
    REFUSED(vsr_debug_wide_grid(0, 1, n, h, w, 0, 256, out), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_grid(2, 3, n, h, w, 0, 256, out), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_grid(2, 1, n, h, w, -1, 256, out), VSR_ERR_BADARG);
    REFUSED(vsr_debug_wide_grid(2, 1, n, h, w, 0, 256, nullptr), VSR_ERR_BADARG);
    EXPECT(vsr_debug_wide_grid(4, 2, n, h, w, 3, 256, out) == VSR_OK && out[0] == 3 && out[1] == 8 && out[2] == n * h * w + 256);

    // no wide hook reaches the BasicVSR side's conv, pack, sign-bit, streaming conv_last.2, chain or SPyNet launchers
    EXPECT(never({"conv", "pack_weights", "sign_bits_c64", "last2_wgrad", "last2_dgrad", "conv3x3_chain", "resize_norm", "resize_norm_bwd", "avgpool2",
                  "avgpool2_bwd_add", "flow_out", "flow_out_bwd", "add_f32", "prepare", "prepare_bwd", "dres"}));
    return hostcheck_finish(f);
}
