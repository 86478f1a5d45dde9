// Stand-alone host check of csrc/spynet_hooks.hip: the hooks' argument checks and what they hand to the launch layer, with every device
// launch stubbed, for a run under ASan / UBSan on a machine without a GPU (the launch layer below the hooks is hostcheck_launch_layer.h's
// recorders).
//   make -C vsrlab_amd/csrc hooks_hostcheck
// Exit status 0 and "spynet hostcheck OK": every refusal came back before any pack or launch, and every accepted call reached
// vsr_launch_conv / vsr_launch_wgrad / vsr_launch_wgrad_reduce / the elementwise launchers with the template sizes of its layer j, cout_real,
// the mask mode, the strides, the fp32 64-channel split (x_coff / x_ctotal) and the sizes it was given.
#define HOSTCHECK_NAME "spynet hostcheck"
#include "hostcheck_launch_layer.h"

int main() {
    float* f = hostcheck_buffer();
    void* v = f;
    char* cb = reinterpret_cast<char*>(f);
    const int n = 2, h = 8, w = 12, BF = VSR_BF16, FP = VSR_F32;
    const int CIP[5] = {16, 32, 64, 32, 16}, COP[5] = {32, 64, 32, 32, 32}, CO[5] = {32, 64, 32, 16, 2}, CI[5] = {8, 32, 64, 32, 16}, CD[5] = {32, 64, 32, 16, 0};
    const int DK[5] = {32, 64, 32, 16, 16}, DROWS[5] = {32, 32, 64, 32, 32};

    // ---- the forward conv ----
    REFUSED(vsr_debug_spy_conv(2, 0, v, f, f, v, v, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, -1, v, f, f, v, v, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 5, v, f, f, v, v, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 0, nullptr, f, f, v, v, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 0, v, nullptr, f, v, v, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 0, v, f, f, nullptr, v, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 0, v, f, f, v, nullptr, 1, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 0, v, f, f, v, v, 2, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);                      // LeakyReLU: no SPyNet layer
    REFUSED(vsr_debug_spy_conv(BF, 0, v, f, f, v, v, 1, nullptr, 0, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 0, v, f, f, v, v, 1, nullptr, n, h, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_conv(BF, 3, v, f, f, v, v, 1, f, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);                       // pres: the planar last layer only
    for (int dt = 0; dt < 2; ++dt)
        for (int j = 0; j < 5; ++j) {
            reset();
            const float* pres = j == 4 ? f + 512 : nullptr;
            EXPECT(vsr_debug_spy_conv(dt ? BF : FP, j, v, f, f + 64, cb + 4096, cb + 8192, j == 4 ? 0 : 1, pres, n, h, w, nullptr) == VSR_OK);
            EXPECT(g_pack.size() == 1 && g_pack[0].KK == 49 && g_pack[0].RP == COP[j] && g_pack[0].CPd == CIP[j] && g_pack[0].r_real == CO[j] &&
                   g_pack[0].c_real == CI[j] && g_pack[0].I_total == CI[j] && g_pack[0].i_off == 0 && g_pack[0].mode == 0 && g_pack[0].dst == cb + 4096);
            EXPECT(g_conv.size() == 1 && g_conv[0].dtype == (dt ? BF : FP) && g_conv[0].ks == 7 && g_conv[0].nsrc == 1 && g_conv[0].ca == CIP[j] && g_conv[0].last_planar == 0 &&
                   g_conv[0].cout_t == COP[j] && g_conv[0].epi == (j == 4 ? EPI_PLANAR : EPI_NHWC));
            const ConvArgs& a = g_conv[0].a;
            EXPECT(a.src[0] == v && a.wpack == cb + 4096 && a.bias == f + 64 && a.dst[0] == cb + 8192 && a.cout_real == CO[j] && a.CD == CD[j] &&
                   a.src_nstride[0] == pm_image_elems(h, w, CIP[j]) && a.act == (j == 4 ? ACT_NONE : ACT_RELU) && a.mask_mode == MASK_NONE && !a.aux[0] &&
                   a.pres == pres && a.N == n && a.H == h && a.W == w);
            EXPECT(a.dst_nstride == (j == 4 ? 2LL * h * w : pm_image_elems(h, w, CD[j])));
        }

    // ---- the data gradient ----
    REFUSED(vsr_debug_spy_dgrad(3, 1, v, f, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 5, v, f, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 1, nullptr, f, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 1, v, nullptr, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 1, v, f, nullptr, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 1, v, f, v, nullptr, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 1, v, f, v, v, nullptr, n, 0, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dgrad(BF, 0, v, f, v, v, v, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);                              // layer 0's input is no activation
    for (int dt = 0; dt < 2; ++dt)
        for (int j = 0; j < 5; ++j)
            for (int masked = 0; masked < (j ? 2 : 1); ++masked) {
                reset();
                EXPECT(vsr_debug_spy_dgrad(dt ? BF : FP, j, v, f, cb + 4096, cb + 8192, masked ? cb + 12288 : nullptr, n, h, w, nullptr) == VSR_OK);
                EXPECT(g_pack.size() == 1 && g_pack[0].KK == 49 && g_pack[0].RP == DROWS[j] && g_pack[0].CPd == DK[j] && g_pack[0].r_real == CI[j] &&
                       g_pack[0].c_real == CO[j] && g_pack[0].I_total == CI[j] && g_pack[0].mode == 1);
                EXPECT(g_conv.size() == 1 && g_conv[0].ks == 7 && g_conv[0].ca == DK[j] && g_conv[0].cout_t == DROWS[j] && g_conv[0].epi == EPI_NHWC);
                const ConvArgs& a = g_conv[0].a;
                EXPECT(a.src[0] == v && a.dst[0] == cb + 8192 && a.cout_real == (j == 0 ? 8 : CIP[j]) && a.CD == CIP[j] && a.src_nstride[0] == pm_image_elems(h, w, DK[j]) &&
                       a.dst_nstride == pm_image_elems(h, w, CIP[j]) && a.act == ACT_NONE && !a.bias && !a.pres);
                EXPECT(masked ? (a.aux[0] == cb + 12288 && a.mask_mode == MASK_RELU) : (!a.aux[0] && a.mask_mode == MASK_NONE));
            }

    // ---- the weight gradient ----
    REFUSED(vsr_debug_spy_wgrad(2, 0, v, v, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 7, v, v, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 0, nullptr, v, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 0, v, nullptr, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 0, v, v, nullptr, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 0, v, v, f, f, 0, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 0, v, v, f, f, 2, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_wgrad(BF, 0, v, v, f, f, 0, f, n, h, -1, nullptr), VSR_ERR_BADARG);
    for (int dt = 0; dt < 2; ++dt)
        for (int j = 0; j < 5; ++j) {
            reset();
            float* gb = j & 1 ? nullptr : f + 9216;
            EXPECT(vsr_debug_spy_wgrad(dt ? BF : FP, j, v, cb + 4096, f + 256, gb, j & 1, f + 1024, 3, 80, 352, nullptr) == VSR_OK);
            const int nhalf = (!dt && j == 2) ? 2 : 1;      // fp32, 64 input channels: two 32-channel halves
            EXPECT((int)g_wgrad.size() == nhalf && (int)g_reduce.size() == nhalf);
            for (int hf = 0; hf < nhalf && hf < (int)g_wgrad.size(); ++hf) {
                const WgradCall& c = g_wgrad[hf];
                const ReduceCall& r = g_reduce[hf];
                EXPECT(c.ks == 7 && c.cx == CIP[j] / nhalf && c.cout == DK[j] && !c.x_planar && !c.dy_planar && c.a.nseg == 1 && c.a.x[0] == v && c.a.dy[0] == cb + 4096 &&
                       c.a.slab == f + 1024 && c.a.x_nstride == pm_image_elems(80, 352, CIP[j]) && c.a.dy_nstride == pm_image_elems(80, 352, DK[j]) &&
                       c.a.N == 3 && c.a.H == 80 && c.a.W == 352);
                EXPECT(nhalf == 2 ? (c.a.x_ctotal == 64 && c.a.x_coff == hf * 4) : (c.a.x_ctotal == 0 && c.a.x_coff == 0));
                EXPECT(r.ks == 7 && r.cx == CIP[j] / nhalf && r.cout == DK[j] && r.cout_real == CO[j] && r.cin_real == (nhalf == 2 ? 32 : CI[j]) && r.I_total == CI[j] &&
                       r.i_off == hf * 32 && r.accumulate == (j & 1) && r.gw == f + 256 && r.gb == (hf == 0 ? gb : nullptr) && r.nwg == c.nwg);
            }
        }

    // ---- spynet_prepare and its adjoint ----
    REFUSED(vsr_debug_spy_prepare(2, f, nullptr, f, v, 1, 2, 2, 0, h, w, 1, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare(BF, nullptr, nullptr, f, v, 1, 2, 2, 0, h, w, 1, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare(BF, f, nullptr, nullptr, v, 1, 2, 2, 0, h, w, 1, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare(BF, f, nullptr, f, nullptr, 1, 2, 2, 0, h, w, 1, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare(BF, f, nullptr, f, v, 1, 2, 2, 0, h, w, 0, nullptr), VSR_ERR_BADARG);                   // a level > 0 without the flow below
    REFUSED(vsr_debug_spy_prepare(BF, f, f, f, v, 1, 2, 2, 0, h, w, 1, nullptr), VSR_ERR_BADARG);                         // level 0 with one
    REFUSED(vsr_debug_spy_prepare(BF, f, f, f, v, 1, 2, 3, 0, h, w, 0, nullptr), VSR_ERR_BADARG);                         // P is 2 n (t - 1)
    REFUSED(vsr_debug_spy_prepare(BF, f, f, f, v, 1, 1, 0, 0, h, w, 0, nullptr), VSR_ERR_BADARG);                         // one frame has no pair
    REFUSED(vsr_debug_spy_prepare(BF, f, f, f, v, 0, 0, 3, 2, h, w, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare(BF, f, f, f, v, 0, 0, 3, 1, 7, w, 0, nullptr), VSR_ERR_BADARG);                         // a level > 0 is twice the one below
    REFUSED(vsr_debug_spy_prepare(BF, f, f, f, v, 0, 0, 3, 1, h, 11, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare(BF, f, nullptr, f, v, 0, 0, 0, 1, h, w, 1, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_spy_prepare(BF, f, f + 64, f + 128, cb + 4096, 2, 3, 8, 0, h, w, 0, nullptr) == VSR_OK);
    EXPECT(g_elt.size() == 1 && is(g_elt[0], "prepare") && g_elt[0].p[0] == f && g_elt[0].p[1] == f + 64 && g_elt[0].p[2] == f + 128 && g_elt[0].p[3] == cb + 4096 &&
           g_elt[0].v[0] == BF && g_elt[0].v[1] == 2 && g_elt[0].v[2] == 3 && g_elt[0].v[3] == 8 && g_elt[0].v[4] == 0 && g_elt[0].v[5] == h && g_elt[0].v[6] == w && g_elt[0].v[7] == 0);
    reset();
    EXPECT(vsr_debug_spy_prepare(FP, f, nullptr, f + 128, cb + 4096, 0, 0, 3, 1, 1, 1, 1, nullptr) == VSR_OK);
    EXPECT(g_elt.size() == 1 && !g_elt[0].p[1] && g_elt[0].v[0] == FP && g_elt[0].v[3] == 3 && g_elt[0].v[4] == 1 && g_elt[0].v[5] == 1 && g_elt[0].v[7] == 1);

    REFUSED(vsr_debug_spy_prepare_bwd(BF, nullptr, f, f, f, f, f, 0, 0, 1, 1, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, f, nullptr, f, f, f, 0, 0, 1, 1, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, f, f, f, nullptr, nullptr, 0, 0, 1, 1, h, w, nullptr), VSR_ERR_BADARG);      // nothing to write
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, nullptr, f, f, f, f, 0, 0, 1, 1, h, w, nullptr), VSR_ERR_BADARG);            // a level > 0 has its flow gradient
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, f, f, nullptr, f, f, 0, 0, 1, 1, h, w, nullptr), VSR_ERR_BADARG);            // ... and its flow_up
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, nullptr, f, f, nullptr, f, 0, 0, 1, 1, h, w, nullptr), VSR_ERR_BADARG);      // level 0 has neither
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, f, f, f, f, f, 0, 0, 1, 1, 7, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_prepare_bwd(BF, v, f, f, f, f, f, 1, 3, 3, 0, h, w, nullptr), VSR_ERR_BADARG);
    const float* none = nullptr;
    float* nonew = nullptr;
    // the engine's three forms: level 0 into the frames; level > 0 with and without the frames
    struct Form { const float* dl; const float* fu; float* dprev; float* dfr; int hh; } forms[3] = {{none, none, nonew, f + 512, 3}, {f + 64, f + 128, f + 256, f + 512, h}, {f + 64, f + 128, f + 256, nonew, h}};
    for (const Form& fm : forms)
        for (int pm = 0; pm < 2; ++pm) {
            reset();
            EXPECT(vsr_debug_spy_prepare_bwd(pm ? FP : BF, v, fm.dl, f + 32, fm.fu, fm.dprev, fm.dfr, pm ? 0 : 1, pm ? 0 : 2, pm ? 3 : 2, pm, fm.hh, w, nullptr) == VSR_OK);
            EXPECT(g_elt.size() == 1 && is(g_elt[0], "prepare_bwd") && g_elt[0].p[0] == v && g_elt[0].p[1] == fm.dl && g_elt[0].p[2] == f + 32 && g_elt[0].p[3] == fm.fu &&
                   g_elt[0].p[4] == fm.dprev && g_elt[0].p[5] == fm.dfr && g_elt[0].v[0] == (pm ? FP : BF) && g_elt[0].v[3] == (pm ? 3 : 2) && g_elt[0].v[4] == pm &&
                   g_elt[0].v[5] == fm.hh && g_elt[0].v[6] == w);
        }

    // ---- spynet_dres ----
    REFUSED(vsr_debug_spy_dres(2, f, f, v, 1, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dres(BF, nullptr, f, v, 1, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dres(BF, f, f, nullptr, 1, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_dres(BF, f, f, v, 0, h, w, nullptr), VSR_ERR_BADARG);
    for (int with = 0; with < 2; ++with) {
        reset();
        EXPECT(vsr_debug_spy_dres(with ? BF : FP, f, with ? f + 64 : nullptr, cb + 4096, 3, h, w, nullptr) == VSR_OK);
        EXPECT(g_elt.size() == 1 && is(g_elt[0], "dres") && g_elt[0].p[0] == f && g_elt[0].p[1] == (with ? f + 64 : nullptr) && g_elt[0].p[2] == cb + 4096 &&
               g_elt[0].v[0] == (with ? BF : FP) && g_elt[0].v[1] == 3 && g_elt[0].v[2] == h && g_elt[0].v[3] == w);
    }

    // ---- the planar launches of the pyramid ----
    REFUSED(vsr_debug_spy_planar(-1, f, f, f, f, f, 2, h, w, 32, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(7, f, f, f, f, f, 2, h, w, 32, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(0, nullptr, f, f, f, f, 2, h, w, 32, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(0, f, f, nullptr, f, f, 2, h, w, 32, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(0, f, f, f, nullptr, f, 2, h, w, 32, 32, nullptr), VSR_ERR_BADARG);                      // resize_norm without a mean
    REFUSED(vsr_debug_spy_planar(1, f, f, f, f, nullptr, 2, h, w, 32, 32, nullptr), VSR_ERR_BADARG);                      // its adjoint without a std
    REFUSED(vsr_debug_spy_planar(0, f, f, f, f, f, 0, h, w, 32, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(0, f, f, f, f, f, 1LL << 31, h, w, 32, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(4, f, f, f, f, f, 2, h, w, 0, 32, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(5, f, f, f, f, f, 2, h, w, 32, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(2, f, f, f, f, f, 2, 7, w, 0, 0, nullptr), VSR_ERR_BADARG);                              // the pool halves both sizes
    REFUSED(vsr_debug_spy_planar(3, f, f, f, f, f, 2, h, 11, 0, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_spy_planar(6, f, nullptr, f, f, f, 2, h, w, 0, 0, nullptr), VSR_ERR_BADARG);
    const char* names[7] = {"resize_norm", "resize_norm_bwd", "avgpool2", "avgpool2_bwd_add", "flow_out", "flow_out_bwd", "add_f32"};
    for (int op = 0; op < 7; ++op) {
        reset();
        EXPECT(vsr_debug_spy_planar(op, f, f + 64, f + 128, f + 192, f + 224, 5, h, w, 32, 64, nullptr) == VSR_OK);
        EXPECT(g_elt.size() == 1 && is(g_elt[0], names[op]) && g_elt[0].p[0] == f);
        const EltCall& e = g_elt[0];
        if (op == 0) EXPECT(e.p[1] == f + 128 && e.p[2] == f + 192 && e.p[3] == f + 224 && e.v[0] == 5 && e.v[1] == h && e.v[2] == w && e.v[3] == 32 && e.v[4] == 64);
        if (op == 1) EXPECT(e.p[1] == f + 128 && e.p[2] == f + 224 && e.v[0] == 5 && e.v[1] == h && e.v[2] == w && e.v[3] == 32 && e.v[4] == 64);
        if (op == 2 || op == 3) EXPECT(e.p[1] == f + 128 && e.v[0] == 5 && e.v[1] == h && e.v[2] == w);
        if (op == 4 || op == 5) EXPECT(e.p[1] == f + 128 && e.v[0] == 5 && e.v[1] == 32 && e.v[2] == 64 && e.v[3] == h && e.v[4] == w);      // (P, hu, wu, h, w)
        if (op == 6) EXPECT(e.p[1] == f + 64 && e.p[2] == f + 128 && e.v[0] == 5LL * h * w);
    }

    // no SPyNet hook reaches the sign bits, the streaming conv_last.2 launchers, the chain or the wide launchers
    EXPECT(never({"sign_bits_c64", "last2_wgrad", "last2_dgrad", "conv3x3_chain", "conv_wide", "pack_wide", "pack_wide2", "wgrad_pairs", "wgrad_reduce_s2",
                  "up2_fwd", "up2_bwd", "mask", "pool_fwd", "pool_bwd", "tap_l1", "tap_sum"}));
    return hostcheck_finish(f);
}
