// Stand-alone host check of csrc/trunk_hooks.hip: the hooks' argument checks and what they hand to the launch layer, with every device
// launch stubbed, for a run under ASan / UBSan on a machine without a GPU (the launch layer below the hooks is hostcheck_launch_layer.h's
// recorders).
//   make -C vsrlab_amd/csrc hooks_hostcheck
// Exit status 0 and "trunk hostcheck OK": every refusal came back before any pack or launch, and every accepted call reached
// vsr_launch_conv / vsr_launch_wgrad / vsr_launch_wgrad_reduce / vsr_launch_conv3x3_chain with the segment counts, strides, i_off,
// accumulate flag and layer offsets it was given.
#define HOSTCHECK_NAME "trunk hostcheck"
#include "hostcheck_launch_layer.h"

int main() {
    float* f = hostcheck_buffer();
    void* v = f;
    char* cb = reinterpret_cast<char*>(f);
    const int n = 2, h = 8, w = 12, BF = VSR_BF16, FP = VSR_F32;
    const long long hw3 = 3LL * h * w;
    const void* seg[9] = {cb, cb + 256, cb + 512, cb + 768, cb + 1024, cb + 1280, cb + 1536, cb + 1792, cb + 2048};
    const void* segn[3] = {cb, nullptr, cb + 512};
    const float* const* fseg = reinterpret_cast<const float* const*>(seg);

    // ---- conv ----
    REFUSED(vsr_debug_trunk_conv(2, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 48, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 5, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 2, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, nullptr, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 3, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 1, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);      // a mask without aux
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, v, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);            // aux without a mask
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, v, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);            // bits without aux
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, v, 1, nullptr, nullptr, 1, 0, n, h, w, nullptr), VSR_ERR_BADARG);            // make_bits without a place
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 1, n, 7, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, 0, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_conv(FP, 64, 3, 0, v, f, f, v, v, 1, 0.f, nullptr, nullptr, 0, v, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);       // sign bits in fp32
    REFUSED(vsr_debug_trunk_conv(BF, 32, 3, 0, v, f, f, v, v, 1, 0.f, nullptr, nullptr, 0, v, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);       // ... at C < 64
    REFUSED(vsr_debug_trunk_conv(BF, 16, 3, 1, v, f, f, v, v, 0, 0.f, nullptr, v, 1, nullptr, v, 0, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_trunk_conv(BF, 64, 1, 0, v, f, f, v, v, 1, 0.f, nullptr, nullptr, 0, v, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);       // ... of a 1x1
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, v, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);       // ... of no activation
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 1, 0.f, v, nullptr, 0, v, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);             // ... behind a residual
    REFUSED(vsr_debug_trunk_conv(BF, 64, 3, 1, v, f, f, v, v, 0, 0.f, nullptr, v, 1, nullptr, nullptr, 0, 1, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);       // a masked phase-separated destination
    REFUSED(vsr_debug_trunk_conv(FP, 64, 3, 0, v, f, f, v, v, 0, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 1, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    reset();
    EXPECT(vsr_debug_trunk_conv(BF, 64, 3, 1, v, f, nullptr, v, cb + 4096, 0, 0.2f, cb + 4096, cb + 8192, 2, nullptr, cb + 12288, 1, 0, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 1 && g_pack[0].KK == 9 && g_pack[0].mode == 1 && g_pack[0].RP == 64 && g_sign == 1 && g_conv.size() == 1);
    EXPECT(g_conv[0].ks == 3 && g_conv[0].nsrc == 1 && g_conv[0].cout_t == 64 && g_conv[0].a.res[0] == g_conv[0].a.dst[0] && g_conv[0].a.aux[0] == cb + 8192 &&
           g_conv[0].a.sign_bits[0] == cb + 12288 && g_conv[0].a.mask_mode == MASK_LEAKY && g_conv[0].a.leaky_slope == 0.2f && !g_conv[0].a.sign_out[0] &&
           g_conv[0].a.src_nstride[0] == pm_image_elems(h, w, 64));
    reset();
    EXPECT(vsr_debug_trunk_conv(FP, 16, 1, 0, v, f, f, v, v, 1, 0.f, nullptr, nullptr, 0, nullptr, nullptr, 0, 0, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 1 && g_pack[0].KK == 1 && g_pack[0].RP == 32 && g_pack[0].CPd == 16 && g_conv.size() == 1 && g_conv[0].ks == 1 && g_conv[0].ca == 16 &&
           g_conv[0].cout_t == 32 && g_conv[0].a.cout_real == 16 && g_conv[0].a.CD == 16 && g_conv[0].a.act == ACT_RELU);
    reset();
    EXPECT(vsr_debug_trunk_conv(BF, 64, 3, 0, v, f, f, v, v, 1, 0.f, nullptr, nullptr, 0, cb + 256, nullptr, 0, 0, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_conv.size() == 1 && g_conv[0].a.sign_out[0] == cb + 256 && g_sign == 0);

    // ---- stem ----
    REFUSED(vsr_debug_trunk_stem(BF, 64, 1, v, f, hw3 - 1, f, f, v, v, 2, 0.f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem(BF, 64, 0, v, f, hw3, f, f, v, v, 2, 0.f, n, h, w, nullptr), VSR_ERR_BADARG);            // a state without cat
    REFUSED(vsr_debug_trunk_stem(BF, 64, 1, v, nullptr, hw3, f, f, v, v, 2, 0.f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem(BF, 64, 1, v, f, hw3, f, f, v, v, 1, 0.f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem(BF, 64, 2, v, f, hw3, f, f, v, v, 2, 0.f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem(BF, 24, 1, v, f, hw3, f, f, v, v, 2, 0.f, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_trunk_stem(BF, 32, 1, nullptr, f + 64, 5 * hw3, f, f, v, v, 2, 0.f, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 2 && g_pack[0].i_off == 3 && g_pack[0].I_total == 35 && g_pack[0].CPd == 32 && g_pack[1].i_off == 0 && g_pack[1].CPd == 16 &&
           g_pack[1].c_real == 3 && g_pack[1].dst == cb + 9 * 32 * 32 * 2);
    EXPECT(g_conv.size() == 1 && g_conv[0].nsrc == 2 && g_conv[0].ca == 32 && g_conv[0].cb == 16 && g_conv[0].last_planar == 1 && !g_conv[0].a.src[0] &&
           g_conv[0].a.src[1] == f + 64 && g_conv[0].a.src_nstride[1] == 5 * hw3 && g_conv[0].a.act == ACT_LEAKY);
    reset();
    EXPECT(vsr_debug_trunk_stem(FP, 64, 0, nullptr, f, hw3, f, nullptr, v, v, 0, 0.f, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 1 && g_pack[0].I_total == 3 && g_conv.size() == 1 && g_conv[0].nsrc == 1 && g_conv[0].a.src[0] == f && g_conv[0].a.src_nstride[0] == hw3);

    // ---- the stem's data gradients ----
    REFUSED(vsr_debug_trunk_stem_dgrad(BF, 64, 1, v, f, v, nullptr, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem_dgrad(BF, 64, 0, v, f, v, v, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);          // no state to differentiate towards
    REFUSED(vsr_debug_trunk_stem_dgrad(BF, 64, 1, v, f, v, nullptr, f, hw3 - 1, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem_dgrad(BF, 64, 1, v, f, v, v, f, hw3, 2, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_trunk_stem_dgrad(BF, 64, 1, v, f, v, cb + 4096, f + 2048, 2 * hw3, 1, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 2 && g_pack[0].mode == 1 && g_pack[0].i_off == 3 && g_pack[1].mode == 1 && g_pack[1].RP == 32 && g_pack[1].r_real == 3 &&
           g_pack[1].I_total == 67 && g_pack[1].dst == cb + 9 * 64 * 64 * 2);
    EXPECT(g_conv.size() == 2 && g_conv[0].epi == EPI_NHWC && g_conv[0].a.dst[0] == cb + 4096 && g_conv[1].epi == EPI_PLANAR && g_conv[1].a.dst[0] == f + 2048 &&
           g_conv[1].a.pres == f + 2048 && g_conv[1].a.dst_nstride == 2 * hw3 && g_conv[1].a.cout_real == 3);
    reset();
    EXPECT(vsr_debug_trunk_stem_dgrad(FP, 16, 0, v, f, v, nullptr, f + 2048, hw3, 0, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 1 && g_pack[0].I_total == 3 && g_conv.size() == 1 && !g_conv[0].a.pres);

    // ---- the fusion conv ----
    REFUSED(vsr_debug_trunk_point(BF, 64, 0, v, nullptr, f, f, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_point(BF, 64, 0, v, v, f, f, v, v, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_point(BF, 64, 1, v, nullptr, f, nullptr, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_point(BF, 64, 1, v, v, f, nullptr, v, v, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_point(BF, 64, 2, v, v, f, f, v, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_trunk_point(BF, 64, 0, v, cb + 256, f, f, v, cb + 512, nullptr, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 2 && g_pack[0].KK == 1 && g_pack[0].I_total == 128 && g_pack[0].i_off == 0 && g_pack[1].i_off == 64 && g_pack[1].dst == cb + 64 * 64 * 2 &&
           g_pack[1].mode == 0);
    EXPECT(g_conv.size() == 1 && g_conv[0].ks == 1 && g_conv[0].nsrc == 2 && g_conv[0].a.src[1] == cb + 256 && g_conv[0].a.act == ACT_LEAKY && g_conv[0].a.nz == 1);
    reset();
    EXPECT(vsr_debug_trunk_point(FP, 16, 1, v, nullptr, f, nullptr, v, cb + 512, cb + 768, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 2 && g_pack[1].mode == 1 && g_pack[1].i_off == 16 && g_pack[1].dst == cb + 32 * 16 * 4);
    EXPECT(g_conv.size() == 1 && g_conv[0].nsrc == 1 && g_conv[0].a.nz == 2 && g_conv[0].a.w_zstride == 32 * 16 && g_conv[0].a.dst[0] == cb + 512 && g_conv[0].a.dst[1] == cb + 768);

    // ---- C -> C weight gradients ----
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 0, f, 64, 0, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 9, f, 64, 0, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, segn, 3, f, 64, 0, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 1, seg, seg, 2, f, 127, 64, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 1, seg, seg, 2, f, 128, -1, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 2, seg, seg, 2, f, 128, 0, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 2, f, 64, 0, f, 2, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 2, nullptr, 64, 0, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 2, f, 64, 0, f, 0, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    for (int nseg = 1; nseg <= 8; ++nseg) {
        reset();
        EXPECT(vsr_debug_trunk_wgrad_cc(BF, 64, 1, seg, seg + 1, nseg, f + 64, 128, 64, nullptr, 1, f, 3, 80, 352, nullptr) == VSR_OK);
        EXPECT(g_wgrad.size() == 1 && g_reduce.size() == 1 && g_wgrad[0].a.nseg == nseg && g_wgrad[0].ks == 1 && g_wgrad[0].cx == 64 && g_wgrad[0].cout == 64 &&
               g_wgrad[0].nwg == 330 && g_wgrad[0].a.slab == f && g_wgrad[0].a.x_nstride == pm_image_elems(80, 352, 64));
        for (int i = 0; i < nseg; ++i) EXPECT(g_wgrad[0].a.x[i] == seg[i] && g_wgrad[0].a.dy[i] == seg[i + 1]);
        EXPECT(g_reduce[0].I_total == 128 && g_reduce[0].i_off == 64 && g_reduce[0].accumulate == 1 && g_reduce[0].gw == f + 64 && !g_reduce[0].gb &&
               g_reduce[0].nwg == 330 && g_reduce[0].ks == 1);
    }
    reset();
    EXPECT(vsr_debug_trunk_wgrad_cc(FP, 32, 3, seg, seg, 3, f, 32, 0, f + 9216, 0, f, 1, 17, 100, nullptr) == VSR_OK);      // 12 tiles; an odd count is rounded down to even
    EXPECT(g_wgrad.size() == 1 && g_wgrad[0].nwg == 12 && g_wgrad[0].cx == 32 && g_reduce.size() == 1 && g_reduce[0].accumulate == 0 && g_reduce[0].gb == f + 9216 &&
           g_reduce[0].cin_real == 32);
    reset();
    EXPECT(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 1, f, 64, 0, nullptr, 0, f, 1, 9, 66, nullptr) == VSR_OK && g_wgrad.size() == 1 && g_wgrad[0].nwg == 6);
    reset();
    EXPECT(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 1, f, 64, 0, nullptr, 0, f, 1, 17, 31, nullptr) == VSR_OK && g_wgrad.size() == 1 && g_wgrad[0].nwg == 2);      // 3 tiles
    reset();
    EXPECT(vsr_debug_trunk_wgrad_cc(BF, 64, 3, seg, seg, 1, f, 64, 0, nullptr, 0, f, 1, 1, 1, nullptr) == VSR_OK && g_wgrad.size() == 1 && g_wgrad[0].nwg == 1);

    // ---- the stem's weight gradients ----
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, hw3, seg, 0, seg, seg, 0, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, hw3, seg, 9, seg, seg, 8, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, hw3, seg, 2, seg, seg, 3, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);      // more states than frames
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 0, fseg, hw3, seg, 2, seg, seg, 1, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);      // states without cat
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, hw3, seg, 2, nullptr, seg, 1, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, hw3 - 1, seg, 2, seg, seg, 1, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, hw3, segn, 3, seg, seg, 1, f, f, 0, f, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_trunk_stem_wgrads(BF, 64, 1, fseg, 3 * hw3, seg + 1, 3, seg + 2, seg + 3, 2, f, f + 64, 1, f + 128, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_wgrad.size() == 2 && g_reduce.size() == 2);
    EXPECT(g_wgrad[0].x_planar == 1 && g_wgrad[0].cx == 16 && g_wgrad[0].a.nseg == 3 && g_wgrad[0].a.x_nstride == 3 * hw3 && g_wgrad[0].a.x[2] == seg[2] &&
           g_wgrad[0].a.dy[2] == seg[3] && g_wgrad[0].a.dy_nstride == pm_image_elems(h, w, 64));
    EXPECT(g_reduce[0].I_total == 67 && g_reduce[0].i_off == 0 && g_reduce[0].cin_real == 3 && g_reduce[0].gb == f + 64 && g_reduce[0].accumulate == 1);
    EXPECT(g_wgrad[1].x_planar == 0 && g_wgrad[1].cx == 64 && g_wgrad[1].a.nseg == 2 && g_wgrad[1].a.x[1] == seg[3] && g_wgrad[1].a.dy[1] == seg[4] &&
           g_wgrad[1].a.x_nstride == pm_image_elems(h, w, 64));
    EXPECT(g_reduce[1].I_total == 67 && g_reduce[1].i_off == 3 && g_reduce[1].cin_real == 64 && !g_reduce[1].gb && g_reduce[1].accumulate == 1 && g_reduce[1].gw == f);
    reset();
    EXPECT(vsr_debug_trunk_stem_wgrads(FP, 16, 1, fseg, hw3, seg, 1, nullptr, nullptr, 0, f, f, 0, f, n, h, w, nullptr) == VSR_OK);       // the first frame alone: no state
    EXPECT(g_wgrad.size() == 1 && g_reduce.size() == 1 && g_reduce[0].I_total == 19 && g_reduce[0].accumulate == 0);
    reset();
    EXPECT(vsr_debug_trunk_stem_wgrads(BF, 64, 0, fseg, hw3, seg, 8, nullptr, nullptr, 0, f, f, 0, f, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_wgrad.size() == 1 && g_wgrad[0].a.nseg == 8 && g_reduce[0].I_total == 3);

    // ---- chains ----
    const unsigned NONE = 0xffffffffu;
    unsigned fwd[16] = {1, 2, NONE, NONE, 7, 20, 30, CHAIN_RELU, 2, 3, 1, NONE, NONE, 21, 31, CHAIN_SKIP};
    unsigned bwd[24] = {9, 10, NONE, 7, NONE, 22, NONE, CHAIN_MASK, 10, 11, 9, NONE, NONE, 23, NONE, CHAIN_SKIP, 11, 12, NONE, 8, NONE, 24, NONE, CHAIN_MASK};
    unsigned now[8] = {1, 2, NONE, NONE, NONE, NONE, NONE, CHAIN_RELU};
    const float* wl[3] = {f, nullptr, f + 64};
    REFUSED(vsr_debug_trunk_chain(FP, 64, v, v, fwd, 2, wl, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_trunk_chain(BF, 32, v, v, fwd, 2, wl, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_trunk_chain(BF, 64, v, v, fwd, 0, wl, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_chain(BF, 64, v, v, fwd, VSR_CHAIN_MAX_LAYERS + 1, wl, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_chain(BF, 64, v, nullptr, fwd, 2, wl, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_chain(BF, 64, cb + 16, v, fwd, 2, wl, 0, n, h, w, nullptr), VSR_ERR_BADARG);                  // the base is 256-byte aligned
    REFUSED(vsr_debug_trunk_chain(BF, 64, v, v, fwd, 2, wl, 2, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_trunk_chain(BF, 64, v, v, now, 1, wl, 0, n, h, w, nullptr), VSR_ERR_BADARG);                        // a layer without weights
    reset();
    EXPECT(vsr_debug_trunk_chain(BF, 64, v, cb + 256, fwd, 2, wl, 0, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 1 && g_pack[0].dst == cb + 20 * 256 && g_pack[0].mode == 0 && g_chain.size() == 1);
    EXPECT(g_chain[0].base == cb && g_chain[0].sync == (unsigned*)(cb + 256) && g_chain[0].nlayers == 2 && g_chain[0].N == n && g_chain[0].H == h && g_chain[0].W == w);
    EXPECT(g_chain[0].layer[0].src == 1 && g_chain[0].layer[0].dst == 2 && g_chain[0].layer[0].sout == 7 && g_chain[0].layer[0].w == 20 && g_chain[0].layer[0].bias == 30 &&
           g_chain[0].layer[0].variant == CHAIN_RELU && g_chain[0].layer[1].res == 1 && g_chain[0].layer[1].sout == NONE && g_chain[0].layer[1].variant == CHAIN_SKIP);
    reset();
    EXPECT(vsr_debug_trunk_chain(BF, 64, v, cb + 256, bwd, 3, wl, 1, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 2 && g_pack[0].mode == 1 && g_pack[1].dst == cb + 24 * 256 && g_chain.size() == 1 && g_chain[0].nlayers == 3);
    EXPECT(g_chain[0].layer[0].sbits == 7 && g_chain[0].layer[0].bias == NONE && g_chain[0].layer[0].variant == CHAIN_MASK && g_chain[0].layer[1].res == 9 &&
           g_chain[0].layer[2].sbits == 8 && g_chain[0].layer[2].src == 11 && g_chain[0].layer[2].dst == 12);

    // no trunk hook reaches the streaming conv_last.2 launchers, the elementwise or the wide ones
    EXPECT(never({"last2_wgrad", "last2_dgrad", "conv_wide", "pack_wide", "pack_wide2", "wgrad_pairs", "wgrad_reduce_s2"}) && g_elt.empty());
    return hostcheck_finish(f);
}
