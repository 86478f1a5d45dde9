// Stand-alone host check of csrc/hr_tail_hooks.hip: the hooks' argument checks with every device launch stubbed, for a run under
// ASan / UBSan on a machine without a GPU (the launch layer below the hooks is hostcheck_launch_layer.h's recorders; no HIP call is made).
//   make -C vsrlab_amd/csrc hooks_hostcheck
// Exit status 0 and "hostcheck OK": every refusal came back before any launch, and every accepted call reached its launches
// with the sizes it was given.
#define HOSTCHECK_NAME "hostcheck"
#include "hostcheck_launch_layer.h"

// the ConvArgs of the latest vsr_launch_conv (all zero if there was none)
static const ConvArgs& last_conv() { static const ConvArgs none = {}; return g_conv.empty() ? none : g_conv.back().a; }

int main() {
    float* f = hostcheck_buffer();
    void* v = f;
    const int n = 2, h = 8, w = 12;
    const long long hw3 = 3LL * h * w;

    // ---- conv_last.2 forward ----
    REFUSED(vsr_debug_tail_last2_fwd(2, v, f, f, v, f, f, hw3, nullptr, nullptr, 0, 0, 0, 0, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, nullptr, f, f, v, f, f, hw3, nullptr, nullptr, 0, 0, 0, 0, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, nullptr, f, hw3, nullptr, nullptr, 0, 0, 0, 0, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3 - 1, nullptr, nullptr, 0, 0, 0, 0, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3, nullptr, nullptr, 0, 0, 0, 0, 5, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3, nullptr, f, 18, 2, 3, 3, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3, nullptr, f, 17, 2, 3, 4, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3, nullptr, f, 72, 4, 6, 4, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3, nullptr, nullptr, 0, 0, 0, 0, 3, 0x7fffffff, -1, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3 + 8, f, f, 18, 2, 3, 4, 3, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 2 && launches() == 1 && last_conv().cout_real == 3 && last_conv().dst_nstride == hw3 + 8 && last_conv().base_h == 2 && last_conv().base_w == 3 &&
           last_conv().base_scale == 4 && last_conv().base_nstride == 18 && last_conv().pres == f && last_conv().src_nstride[0] == pm_image_elems(h, w, 64));

    // ---- conv_last.2 data gradient ----
    REFUSED(vsr_debug_tail_last2_dgrad(nullptr, hw3, f, v, 1, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3 - 1, f, v, 1, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, nullptr, 1, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 2, nullptr, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 3, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 1, v, 0, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 1, v, 2, 0.1f, v, n, 0, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 2, v, 2, 0.1f, v, n, h, w, nullptr) == VSR_OK && launches() == 2);
    reset();
    EXPECT(vsr_debug_tail_last2_dgrad(f, 2 * hw3, f, nullptr, 0, nullptr, 0, 0.f, v, n, h, w, nullptr) == VSR_OK && launches() == 1);

    // ---- planar -> 64 ----
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 2, f, f, v, v, 2, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3 - 1, 3, f, f, v, v, 2, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, v, v, 1, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, v, v, 2, 0.1f, nullptr, 2, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, v, v, 2, 0.1f, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, nullptr, v, 2, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_tail_planar_c64(0, f, (long long)h * w, 1, f, nullptr, v, v, 0, 0.2f, v, 2, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_pack.size() == 1 && launches() == 1 && last_conv().planar_c == 1 && last_conv().src_nstride[0] == h * w && last_conv().mask_mode == MASK_LEAKY && last_conv().leaky_slope == 0.2f);

    // ---- 64 -> pc weight gradient ----
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 0, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 4, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, (long long)h * w - 1, 1, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 3, nullptr, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 3, f, f, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(3, v, f, hw3, 3, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    for (int pc = 1; pc <= 3; ++pc) {      // bf16: the streaming launcher gets the plane count (it used to get 3 whatever the cotangent had)
        reset();
        EXPECT(vsr_debug_tail_last2_wgrad(1, v, f, hw3, pc, f, f, f, n, h, w, nullptr) == VSR_OK && launches() == 2 && g_last2_wgrad.size() == 1 && g_last2_wgrad[0] == pc);
    }
    reset();
    EXPECT(vsr_debug_tail_last2_wgrad(0, v, f, hw3, 2, f, nullptr, f, n, h, w, nullptr) == VSR_OK && launches() == 2 && g_last2_wgrad.empty());

    // ---- phase planes ----
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 0, v, v, n, 7, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 0, v, v, n, h, 11, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 2, v, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 0, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_tail_conv_unshuffle(1, v, f, f, 1, v, v, n, h, w, nullptr) == VSR_OK && g_pack.size() == 1 && launches() == 1);
    EXPECT(last_conv().unshuffle == 1 && last_conv().unshuffle_plane == n * pm_image_elems(h / 2, w / 2, 64) && last_conv().dst_nstride == pm_image_elems(h / 2, w / 2, 64));

    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 2, 1, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, v, 2, 2, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 0, 0, nullptr, 2, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 0, 0, nullptr, 0, 1, n, 7, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(0, v, f, v, v, nullptr, 0, 0, nullptr, 1, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_tail_ps_dgrad(0, v, f, v, v, nullptr, 0, 0, nullptr, 0, 1, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, v, 2, 1, nullptr, 0, 1, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    reset();
    EXPECT(vsr_debug_tail_ps_dgrad(1, v, f, v, v, v, 2, 2, v, 1, 0, n, h, w, nullptr) == VSR_OK && g_pack.size() == 4 && launches() == 5);      // sign bits + 4 phases
    EXPECT(last_conv().sign_bits[0] == v && last_conv().aux[0] == v && last_conv().res[0] == v && last_conv().in_step == 1);
    reset();
    EXPECT(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 0, 0, nullptr, 0, 1, n, h, w, nullptr) == VSR_OK && launches() == 4 && last_conv().unshuffle == 1 && last_conv().in_step == 2);
    reset();
    EXPECT(vsr_debug_tail_ps_dgrad(0, v, f, v, v, v, 2, 1, nullptr, 0, 0, n, h, w, nullptr) == VSR_OK && launches() == 1 && g_pack.size() == 4);    // fp32: one 4-source launch

    REFUSED(vsr_debug_tail_ps_wgrads(1, nullptr, v, 0, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_wgrads(1, v, v, 2, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_wgrads(1, v, v, 0, f, f, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_wgrads(1, v, v, 0, nullptr, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    reset();
    EXPECT(vsr_debug_tail_ps_wgrads(1, v, v, 1, f, f, f, n, h, w, nullptr) == VSR_OK && launches() == 8);      // 4 phases x (launch + reduction)

    // no tail hook reaches the chain, the elementwise or the wide launchers
    EXPECT(never({"conv3x3_chain", "conv_wide", "pack_wide", "pack_wide2", "wgrad_pairs", "wgrad_reduce_s2"}) && g_elt.empty());
    return hostcheck_finish(f);
}
