// Stand-alone host check of csrc/hr_tail_hooks.hip: the hooks' argument checks with every device launch stubbed, for a run under
// ASan / UBSan on a machine without a GPU (the launch layer below the hooks is replaced by counters; no HIP call is made).
//   make -C vsrlab_amd/csrc hooks_hostcheck
// Exit status 0 and "hostcheck OK": every refusal came back before any launch, and every accepted call reached its launches
// with the sizes it was given.
#include <cstdio>
#include <cstdlib>
#include "../vsrlab_amd/csrc/recipes.h"

static int g_launches = 0, g_packs = 0;
static ConvArgs g_conv;
static int g_last2_pc = 0;

int vsr_launch_conv(int, int, int, int, int, int, int, int, const ConvArgs& a, hipStream_t) { ++g_launches; g_conv = a; return VSR_OK; }
int vsr_launch_sign_bits_c64(const void* x, void* bits, int, int, int, hipStream_t) { ++g_launches; return x && bits ? VSR_OK : VSR_ERR_BADARG; }
int vsr_launch_last2_dgrad(const float*, long long, const float*, const void*, void*, int, int, int, int, hipStream_t, const void*, float) { ++g_launches; return VSR_OK; }
int vsr_launch_last2_wgrad(const void*, const float*, long long, float*, int, int, int, int, int* nslabs, hipStream_t, int pc) {
    ++g_launches; g_last2_pc = pc; *nslabs = 1; return VSR_OK;
}
int vsr_launch_wgrad(int, int, int, int, int, int, const WgradArgs&, int nwg, int* nslabs, hipStream_t) { ++g_launches; *nslabs = nwg; return VSR_OK; }
int vsr_launch_wgrad_reduce(const float*, int, int, int, int, int, int, float*, int, int, int, int, float*, int, hipStream_t) { ++g_launches; return VSR_OK; }
void vsr_wgrad_slab_dims(int ks, int cx, int cout, int* coutp, int* cxp, int* stride) {
    const int ncb = cout >= 32 ? cout / 32 : 1, nib = cx >= 32 ? cx / 32 : 1;
    *coutp = ncb * 32; *cxp = nib * 32; *stride = ks * ks * (*coutp) * (*cxp) + (*coutp);
}
int vsr_launch_pack_weights(int, const float* w, void* dst, int, int, int, int, int, int, int, int, int, int, hipStream_t) { ++g_packs; return w && dst ? VSR_OK : VSR_ERR_BADARG; }

extern "C" {
int vsr_debug_tail_last2_fwd(int, const void*, const float*, const float*, void*, float*, float*, long long, const float*, const float*, long long, int, int, int,
                             int, int, int, int, void*);
int vsr_debug_tail_last2_dgrad(const float*, long long, const float*, const void*, int, void*, int, float, void*, int, int, int, void*);
int vsr_debug_tail_planar_c64(int, const float*, long long, int, const float*, const float*, void*, void*, int, float, const void*, int, int, int, int, void*);
int vsr_debug_tail_last2_wgrad(int, const void*, const float*, long long, int, float*, float*, float*, int, int, int, void*);
int vsr_debug_tail_conv_unshuffle(int, const void*, const float*, const float*, int, void*, void*, int, int, int, void*);
int vsr_debug_tail_ps_dgrad(int, const void*, const float*, void*, void*, const void*, int, int, void*, int, int, int, int, int, void*);
int vsr_debug_tail_ps_wgrads(int, const void*, const void*, int, float*, float*, float*, int, int, int, void*);
}

static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, "hostcheck: line %d: %s\n", __LINE__, #cond); ++g_fail; } } while (0)
// a refusal: the status, and neither a pack nor a launch happened
#define REFUSED(call, status) do { const int l0 = g_launches, p0 = g_packs; EXPECT((call) == (status)); EXPECT(g_launches == l0 && g_packs == p0); } while (0)

int main() {
    // real, small buffers: an accepted call hands them to the (stubbed) launch layer only
    float* f = static_cast<float*>(std::calloc(4096, 4));
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
    g_launches = g_packs = 0;
    EXPECT(vsr_debug_tail_last2_fwd(1, v, f, f, v, f, f, hw3 + 8, f, f, 18, 2, 3, 4, 3, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_packs == 2 && g_launches == 1 && g_conv.cout_real == 3 && g_conv.dst_nstride == hw3 + 8 && g_conv.base_h == 2 && g_conv.base_w == 3 &&
           g_conv.base_scale == 4 && g_conv.base_nstride == 18 && g_conv.pres == f && g_conv.src_nstride[0] == pm_image_elems(h, w, 64));

    // ---- conv_last.2 data gradient ----
    REFUSED(vsr_debug_tail_last2_dgrad(nullptr, hw3, f, v, 1, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3 - 1, f, v, 1, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, nullptr, 1, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 2, nullptr, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 3, v, 2, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 1, v, 0, 0.1f, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 1, v, 2, 0.1f, v, n, 0, w, nullptr), VSR_ERR_BADARG);
    g_launches = 0;
    EXPECT(vsr_debug_tail_last2_dgrad(f, hw3, f, v, 2, v, 2, 0.1f, v, n, h, w, nullptr) == VSR_OK && g_launches == 2);
    g_launches = 0;
    EXPECT(vsr_debug_tail_last2_dgrad(f, 2 * hw3, f, nullptr, 0, nullptr, 0, 0.f, v, n, h, w, nullptr) == VSR_OK && g_launches == 1);

    // ---- planar -> 64 ----
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 2, f, f, v, v, 2, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3 - 1, 3, f, f, v, v, 2, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, v, v, 1, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, v, v, 2, 0.1f, nullptr, 2, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, v, v, 2, 0.1f, v, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_planar_c64(1, f, hw3, 3, f, f, nullptr, v, 2, 0.1f, nullptr, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    g_launches = g_packs = 0;
    EXPECT(vsr_debug_tail_planar_c64(0, f, (long long)h * w, 1, f, nullptr, v, v, 0, 0.2f, v, 2, n, h, w, nullptr) == VSR_OK);
    EXPECT(g_packs == 1 && g_launches == 1 && g_conv.planar_c == 1 && g_conv.src_nstride[0] == h * w && g_conv.mask_mode == MASK_LEAKY && g_conv.leaky_slope == 0.2f);

    // ---- 64 -> pc weight gradient ----
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 0, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 4, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, (long long)h * w - 1, 1, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 3, nullptr, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(1, v, f, hw3, 3, f, f, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_last2_wgrad(3, v, f, hw3, 3, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    for (int pc = 1; pc <= 3; ++pc) {      // bf16: the streaming launcher gets the plane count (it used to get 3 whatever the cotangent had)
        g_launches = 0; g_last2_pc = 0;
        EXPECT(vsr_debug_tail_last2_wgrad(1, v, f, hw3, pc, f, f, f, n, h, w, nullptr) == VSR_OK && g_launches == 2 && g_last2_pc == pc);
    }
    g_launches = 0; g_last2_pc = 0;
    EXPECT(vsr_debug_tail_last2_wgrad(0, v, f, hw3, 2, f, nullptr, f, n, h, w, nullptr) == VSR_OK && g_launches == 2 && g_last2_pc == 0);

    // ---- phase planes ----
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 0, v, v, n, 7, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 0, v, v, n, h, 11, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 2, v, v, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_conv_unshuffle(1, v, f, f, 0, v, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    g_launches = g_packs = 0;
    EXPECT(vsr_debug_tail_conv_unshuffle(1, v, f, f, 1, v, v, n, h, w, nullptr) == VSR_OK && g_packs == 1 && g_launches == 1);
    EXPECT(g_conv.unshuffle == 1 && g_conv.unshuffle_plane == n * pm_image_elems(h / 2, w / 2, 64) && g_conv.dst_nstride == pm_image_elems(h / 2, w / 2, 64));

    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 2, 1, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, v, 2, 2, nullptr, 0, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 0, 0, nullptr, 2, 0, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 0, 0, nullptr, 0, 1, n, 7, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_dgrad(0, v, f, v, v, nullptr, 0, 0, nullptr, 1, 0, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_tail_ps_dgrad(0, v, f, v, v, nullptr, 0, 0, nullptr, 0, 1, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    REFUSED(vsr_debug_tail_ps_dgrad(1, v, f, v, v, v, 2, 1, nullptr, 0, 1, n, h, w, nullptr), VSR_ERR_UNSUPPORTED);
    g_launches = g_packs = 0;
    EXPECT(vsr_debug_tail_ps_dgrad(1, v, f, v, v, v, 2, 2, v, 1, 0, n, h, w, nullptr) == VSR_OK && g_packs == 4 && g_launches == 5);      // sign bits + 4 phases
    EXPECT(g_conv.sign_bits[0] == v && g_conv.aux[0] == v && g_conv.res[0] == v && g_conv.in_step == 1);
    g_launches = g_packs = 0;
    EXPECT(vsr_debug_tail_ps_dgrad(1, v, f, v, v, nullptr, 0, 0, nullptr, 0, 1, n, h, w, nullptr) == VSR_OK && g_launches == 4 && g_conv.unshuffle == 1 && g_conv.in_step == 2);
    g_launches = g_packs = 0;
    EXPECT(vsr_debug_tail_ps_dgrad(0, v, f, v, v, v, 2, 1, nullptr, 0, 0, n, h, w, nullptr) == VSR_OK && g_launches == 1 && g_packs == 4);    // fp32: one 4-source launch

    REFUSED(vsr_debug_tail_ps_wgrads(1, nullptr, v, 0, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_wgrads(1, v, v, 2, f, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_wgrads(1, v, v, 0, f, f, nullptr, n, h, w, nullptr), VSR_ERR_BADARG);
    REFUSED(vsr_debug_tail_ps_wgrads(1, v, v, 0, nullptr, f, f, n, h, w, nullptr), VSR_ERR_BADARG);
    g_launches = 0;
    EXPECT(vsr_debug_tail_ps_wgrads(1, v, v, 1, f, f, f, n, h, w, nullptr) == VSR_OK && g_launches == 8);      // 4 phases x (launch + reduction)

    std::free(f);
    if (g_fail) { std::fprintf(stderr, "hostcheck: %d check(s) failed\n", g_fail); return 1; }
    std::puts("hostcheck OK");
    return 0;
}
