// Stand-alone host check of csrc/warp_hooks.hip: the hooks' argument checks and what they hand to the launch layer, with every device
// launch stubbed, for a run under ASan / UBSan on a machine without a GPU (the launch layer below the hooks is hostcheck_launch_layer.h's
// recorders).
//   make -C vsrlab_amd/csrc hooks_hostcheck        (or the target warp_hostcheck alone)
// Exit status 0 and "warp hostcheck OK": every refusal came back before any launch, and every accepted call reached vsr_launch_warp_fwd /
// vsr_launch_warp_bwd + vsr_launch_add_cast / vsr_launch_warp_bwd_gather / vsr_launch_warp_bwd_flow with the pointers, the width, the
// flow's image stride and the padding mode it was given.
#define HOSTCHECK_NAME "warp hostcheck"
#include "hostcheck_launch_layer.h"

static bool dims(const EltCall& e, int dt, int n, int h, int w, int C) { return e.v[0] == dt && e.v[1] == n && e.v[2] == h && e.v[3] == w && e.v[4] == C; }

int main() {
    float* f = hostcheck_buffer();
    void* v = f;
    char* cb = reinterpret_cast<char*>(f);
    long long* S = reinterpret_cast<long long*>(cb + 16384);
    int* fc = reinterpret_cast<int*>(cb + 32768);
    const int n = 2, h = 8, w = 12, BF = VSR_BF16, FP = VSR_F32;
    const long long ns = 2LL * h * w;

    // ---- forward ----
    REFUSED(vsr_debug_warp_fwd(2, 64, v, f, ns, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, nullptr, f, ns, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, nullptr, ns, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns - 1, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);                  // the flows of two images overlap
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns, v, 2, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns, v, -1, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns, v, 0, 0, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns, v, 0, n, 0, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_fwd(BF, 64, v, f, ns, v, 0, n, h, -3, nullptr), VSR_ERR_BADARG);
    for (int C : {0, 8, 24, 48, 128}) REFUSED(vsr_debug_warp_fwd(BF, C, v, f, ns, v, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    for (int C : {16, 32, 64})
        for (int border = 0; border < 2; ++border) {
            reset();
            const int dt = border ? FP : BF;
            EXPECT(vsr_debug_warp_fwd(dt, C, v, f + 64, 3 * ns, cb + 4096, border, n, h, w, nullptr) == VSR_OK);
            EXPECT(launches() == 1 && g_elt.size() == 1 && is(g_elt[0], "warp_fwd") && g_elt[0].p[0] == v && g_elt[0].p[1] == f + 64 && g_elt[0].p[2] == cb + 4096 &&
                   dims(g_elt[0], dt, n, h, w, C) && g_elt[0].v[5] == 3 * ns && g_elt[0].v[6] == border);
        }

    // ---- the scatter adjoint: warp_bwd, then add_cast ----
    REFUSED(vsr_debug_warp_scatter(3, 64, v, f, ns, f, v, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, nullptr, f, ns, f, v, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, v, nullptr, ns, f, v, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, v, f, ns, nullptr, v, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, v, f, ns, f, v, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, v, f, 0, f, v, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, v, f, ns, f, v, v, 3, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 64, v, f, ns, f, v, v, 0, n, h, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_scatter(BF, 40, v, f, ns, f, v, v, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    for (int C : {16, 32, 64})
        for (int with = 0; with < 2; ++with) {
            reset();
            const void* a = with ? cb + 8192 : nullptr;
            EXPECT(vsr_debug_warp_scatter(with ? BF : FP, C, v, f + 64, 3 * ns, f + 1024, a, cb + 12288, with, n, h, w, nullptr) == VSR_OK);
            EXPECT(launches() == 2 && g_elt.size() == 2);
            if (g_elt.size() == 2) {
                const EltCall& b = g_elt[0];
                const EltCall& c = g_elt[1];
                EXPECT(is(b, "warp_bwd") && b.p[0] == v && b.p[1] == f + 64 && b.p[2] == f + 1024 && dims(b, with ? BF : FP, n, h, w, C) && b.v[5] == 3 * ns && b.v[6] == with);
                EXPECT(is(c, "add_cast") && c.p[0] == a && c.p[1] == f + 1024 && c.p[2] == cb + 12288 && dims(c, with ? BF : FP, n, h, w, C));
            }
        }

    // ---- the gather adjoint ----
    REFUSED(vsr_debug_warp_gather(2, 64, v, f, ns, nullptr, S, fc, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, nullptr, f, ns, nullptr, S, fc, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, v, nullptr, ns, nullptr, S, fc, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, v, f, ns, nullptr, nullptr, fc, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, v, f, ns, nullptr, S, nullptr, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, v, f, ns, nullptr, S, fc, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, v, f, ns - 1, nullptr, S, fc, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_gather(BF, 64, v, f, ns, nullptr, S, fc, v, n, -1, w, nullptr), VSR_ERR_BADARG);
    for (int C : {8, 24, 48, 96}) REFUSED(vsr_debug_warp_gather(BF, C, v, f, ns, nullptr, S, fc, v, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    for (int C : {16, 32, 64})
        for (int with = 0; with < 2; ++with) {
            reset();
            const void* dtop = with ? cb + 8192 : nullptr;
            const long long st = with ? 3 * ns : ns;
            EXPECT(vsr_debug_warp_gather(with ? BF : FP, C, v, f + 64, st, dtop, S, fc, cb + 12288, n, h, w, nullptr) == VSR_OK);
            EXPECT(launches() == 1 && g_elt.size() == 1 && is(g_elt[0], "warp_bwd_gather") && g_elt[0].p[0] == v && g_elt[0].p[1] == f + 64 && g_elt[0].p[2] == dtop &&
                   g_elt[0].p[3] == S && g_elt[0].p[4] == fc && g_elt[0].p[5] == cb + 12288 && dims(g_elt[0], with ? BF : FP, n, h, w, C) && g_elt[0].v[5] == st);
        }

    // ---- the flow gradient ----
    REFUSED(vsr_debug_warp_flowgrad(-1, 64, v, v, f, ns, f, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, nullptr, v, f, ns, f, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, v, nullptr, f, ns, f, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, v, v, nullptr, ns, f, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, v, v, f, ns, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, v, v, f, ns - 1, f, 0, n, h, w, nullptr), VSR_ERR_BADARG);          // dflow's images would overlap too
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, v, v, f, ns, f, 2, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 64, v, v, f, ns, f, 0, 0, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_flowgrad(BF, 20, v, v, f, ns, f, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    for (int C : {16, 32, 64})
        for (int border = 0; border < 2; ++border) {
            reset();
            EXPECT(vsr_debug_warp_flowgrad(border ? BF : FP, C, v, cb + 4096, f + 64, 3 * ns, f + 2048, border, n, h, w, nullptr) == VSR_OK);
            EXPECT(launches() == 1 && g_elt.size() == 1 && is(g_elt[0], "warp_bwd_flow") && g_elt[0].p[0] == v && g_elt[0].p[1] == cb + 4096 && g_elt[0].p[2] == f + 64 &&
                   g_elt[0].p[3] == f + 2048 && dims(g_elt[0], border ? BF : FP, n, h, w, C) && g_elt[0].v[5] == 3 * ns && g_elt[0].v[6] == border);
        }

    // ---- add_cast alone ----
    REFUSED(vsr_debug_warp_add_cast(2, 64, v, f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_add_cast(BF, 64, nullptr, nullptr, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_add_cast(BF, 64, v, f, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_add_cast(BF, 64, v, f, v, n, h, 0, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_warp_add_cast(BF, 72, v, f, v, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    for (int form = 0; form < 3; ++form) {
        reset();
        const void* a = form == 0 ? nullptr : v;
        const float* s = form == 1 ? nullptr : f + 1024;
        EXPECT(vsr_debug_warp_add_cast(form ? BF : FP, 32, a, s, cb + 12288, n, h, w, nullptr) == VSR_OK);
        EXPECT(launches() == 1 && g_elt.size() == 1 && is(g_elt[0], "add_cast") && g_elt[0].p[0] == a && g_elt[0].p[1] == s && g_elt[0].p[2] == cb + 12288 &&
               dims(g_elt[0], form ? BF : FP, n, h, w, 32));
    }

    // no warp hook packs a weight or reaches a convolution, a weight gradient, the chain or SPyNet's launches
    EXPECT(g_pack.empty());
    EXPECT(never({"conv", "sign_bits_c64", "last2_dgrad", "last2_wgrad", "wgrad", "wgrad_reduce", "pack_weights", "conv3x3_chain", "prepare", "prepare_bwd", "dres",
                  "conv_wide", "pack_wide", "pack_wide2", "wgrad_pairs", "wgrad_reduce_s2", "up2_fwd", "up2_bwd", "mask", "pool_fwd", "pool_bwd", "tap_l1", "tap_sum"}));
    return hostcheck_finish(f);
}
