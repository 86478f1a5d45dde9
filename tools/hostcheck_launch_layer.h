// The recording launch layer of the five stand-alone host checks (tools/*_hooks_hostcheck.hip): every vsr_launch_* function that
// csrc/hr_tail_hooks.hip, trunk_hooks.hip, spynet_hooks.hip, wide_hooks.hip or warp_hooks.hip reaches, directly or through recipes.h / wide_recipes.h,
// is replaced by a stub that records what it was handed and launches nothing.  No HIP call is made, so the programs run under
// ASan / UBSan on a machine without a GPU.  The hooks are called through csrc/debug_hooks.h, and the size formulas
// (vsr_wgrad_slab_dims, vsr_wide_pack_elems, vsr_wide2_pack_elems) are the library's own, inline in kernels.h.
// A program defines HOSTCHECK_NAME (the prefix of its messages) before it includes this header, and has its own main().
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <set>
#include <string>
#include <vector>
#include "../vsrlab_amd/csrc/recipes.h"
#include "../vsrlab_amd/csrc/wide_recipes.h"
#include "../vsrlab_amd/csrc/debug_hooks.h"

// ---- one record per launcher family ----
struct ConvCall { int dtype, ks, nsrc, ca, cb, last_planar, cout_t, epi; ConvArgs a; };
struct WgradCall { int ks, cx, x_planar, cout, dy_planar, nwg; WgradArgs a; };
// s2 0: vsr_launch_wgrad_reduce (ks .. accumulate, gb); s2 1: vsr_launch_wgrad_reduce_s2 (cin_total .. view; it always accumulates)
struct ReduceCall { int s2, nwg, ks, cx, cout, cout_real, cin_real, I_total, i_off, accumulate, cin_total, co0, ci0, view; float* gw; float* gb; };
// w2 -1: vsr_launch_pack_weights (KK .. i_off); 0: vsr_launch_pack_wide, 1: vsr_launch_pack_wide2 (cout, cin)
struct PackCall { int w2, dtype, KK, RP, CPd, r_real, c_real, I_total, i_off, cout, cin, mode; void* dst; };
struct PairsCall { int nsl, ncob, views, ksplit, cin_total; float* gw; WgradArgs a; };
struct WideCall { int dtype; VsrWideConv c; };
// an elementwise launch: which one, its pointers, its integers and its float, each in the launcher's own order
struct EltCall { const char* name; const void* p[6]; long long v[8]; float f; };
static std::vector<ConvCall> g_conv;
static std::vector<WgradCall> g_wgrad;
static std::vector<ReduceCall> g_reduce;
static std::vector<PackCall> g_pack;
static std::vector<PairsCall> g_pairs;
static std::vector<WideCall> g_wide;
static std::vector<EltCall> g_elt;
static std::vector<ChainArgs> g_chain;
static std::vector<int> g_last2_wgrad;      // the plane count each vsr_launch_last2_wgrad was handed
static int g_sign = 0, g_last2_dgrad = 0;
static int launches() {
    return (int)(g_conv.size() + g_wgrad.size() + g_reduce.size() + g_pairs.size() + g_wide.size() + g_elt.size() + g_chain.size() + g_last2_wgrad.size()) +
           g_sign + g_last2_dgrad;
}
static void reset() {
    g_conv.clear(); g_wgrad.clear(); g_reduce.clear(); g_pack.clear(); g_pairs.clear(); g_wide.clear(); g_elt.clear(); g_chain.clear(); g_last2_wgrad.clear();
    g_sign = g_last2_dgrad = 0;
}
// every launcher reached since the program started (reset() leaves it alone): a program ends on never({...}) of the launchers that no
// hook of its family may reach
static std::set<std::string> g_ever;
static const std::set<std::string> g_launchers = {      // the stubs' names: hit() and never() refuse any other (a misspelt one)
    "conv", "sign_bits_c64", "last2_dgrad", "last2_wgrad", "wgrad", "wgrad_reduce", "pack_weights", "conv3x3_chain", "resize_norm", "resize_norm_bwd",
    "avgpool2", "avgpool2_bwd_add", "flow_out", "flow_out_bwd", "add_f32", "prepare", "prepare_bwd", "dres", "conv_wide", "pack_wide2", "pack_wide",
    "wgrad_pairs", "wgrad_reduce_s2", "up2_fwd", "up2_bwd", "mask", "pool_fwd", "pool_bwd", "tap_l1", "tap_sum", "warp_fwd", "warp_bwd",
    "warp_bwd_gather", "warp_bwd_flow", "add_cast"};
static const char* hit(const char* launcher) {
    if (!g_launchers.count(launcher)) { std::fprintf(stderr, "hostcheck_launch_layer.h: unlisted launcher %s\n", launcher); std::abort(); }
    g_ever.insert(launcher);
    return launcher;
}
static bool never(std::initializer_list<const char*> launchers) {
    for (const char* l : launchers) if (!g_launchers.count(l) || g_ever.count(l)) return false;
    return true;
}

// ---- recipes.h's launchers ----
int vsr_launch_conv(int dtype, int ks, int nsrc, int ca, int cb, int last_planar, int cout_t, int epi, const ConvArgs& a, hipStream_t) {
    hit("conv"); g_conv.push_back({dtype, ks, nsrc, ca, cb, last_planar, cout_t, epi, a}); return VSR_OK;
}
int vsr_launch_sign_bits_c64(const void* x, void* bits, int, int, int, hipStream_t) { hit("sign_bits_c64"); ++g_sign; return x && bits ? VSR_OK : VSR_ERR_BADARG; }
int vsr_launch_last2_dgrad(const float*, long long, const float*, const void*, void*, int, int, int, int, hipStream_t, const void*, float) {
    hit("last2_dgrad"); ++g_last2_dgrad; return VSR_OK;
}
int vsr_launch_last2_wgrad(const void*, const float*, long long, float*, int, int, int, int, int* nslabs, hipStream_t, int pc) {
    hit("last2_wgrad"); g_last2_wgrad.push_back(pc); *nslabs = 1; return VSR_OK;
}
int vsr_launch_wgrad(int, int ks, int cx, int x_planar, int cout, int dy_planar, const WgradArgs& a, int nwg, int* nslabs, hipStream_t) {
    hit("wgrad"); g_wgrad.push_back({ks, cx, x_planar, cout, dy_planar, nwg, a}); *nslabs = nwg; return VSR_OK;
}
int vsr_launch_wgrad_reduce(const float*, int nwg, int ks, int cx, int cout, int cout_real, int cin_real, float* gw, int I_total, int i_off, int, int,
                            float* gb, int accumulate, hipStream_t) {
    hit("wgrad_reduce"); g_reduce.push_back({0, nwg, ks, cx, cout, cout_real, cin_real, I_total, i_off, accumulate, 0, 0, 0, -1, gw, gb}); return VSR_OK;
}
int vsr_launch_pack_weights(int dtype, const float* w, void* dst, int KK, int RP, int CPd, int r_real, int c_real, int I_total, int i_off, int, int, int mode, hipStream_t) {
    hit("pack_weights"); g_pack.push_back({-1, dtype, KK, RP, CPd, r_real, c_real, I_total, i_off, 0, 0, mode, dst}); return w && dst ? VSR_OK : VSR_ERR_BADARG;
}
int vsr_launch_conv3x3_chain(const ChainArgs& a, int num_cus, hipStream_t) { hit("conv3x3_chain"); g_chain.push_back(a); return num_cus >= 1 ? VSR_OK : VSR_ERR_BADARG; }

// ---- SPyNet's elementwise launchers ----
int vsr_launch_resize_norm(const float* in, float* out, const float* mean, const float* std, int F, int h, int w, int hu, int wu, hipStream_t) {
    g_elt.push_back({hit("resize_norm"), {in, out, mean, std}, {F, h, w, hu, wu}}); return VSR_OK;
}
int vsr_launch_resize_norm_bwd(const float* dnorm, float* dframes, const float* std, int F, int h, int w, int hu, int wu, hipStream_t) {
    g_elt.push_back({hit("resize_norm_bwd"), {dnorm, dframes, std}, {F, h, w, hu, wu}}); return VSR_OK;
}
int vsr_launch_avgpool2(const float* in, float* out, long long planes, int h, int w, hipStream_t) {
    g_elt.push_back({hit("avgpool2"), {in, out}, {planes, h, w}}); return VSR_OK;
}
int vsr_launch_avgpool2_bwd_add(const float* dcoarse, float* dfine, long long planes, int h, int w, hipStream_t) {
    g_elt.push_back({hit("avgpool2_bwd_add"), {dcoarse, dfine}, {planes, h, w}}); return VSR_OK;
}
int vsr_launch_flow_out(const float* in, float* out, int P, int hu, int wu, int h, int w, hipStream_t) {
    g_elt.push_back({hit("flow_out"), {in, out}, {P, hu, wu, h, w}}); return VSR_OK;
}
int vsr_launch_flow_out_bwd(const float* dout, float* din, int P, int hu, int wu, int h, int w, hipStream_t) {
    g_elt.push_back({hit("flow_out_bwd"), {dout, din}, {P, hu, wu, h, w}}); return VSR_OK;
}
int vsr_launch_add_f32(const float* a, const float* b, float* out, long long n, hipStream_t) {
    g_elt.push_back({hit("add_f32"), {a, b, out}, {n}}); return VSR_OK;
}
int vsr_launch_spynet_prepare(int dtype, const float* frames, const float* flow_prev, float* flow_up, void* x16, int n, int t, int P, int pair_mode, int h, int w,
                              int level0, hipStream_t) {
    g_elt.push_back({hit("prepare"), {frames, flow_prev, flow_up, x16}, {dtype, n, t, P, pair_mode, h, w, level0}}); return VSR_OK;
}
int vsr_launch_spynet_prepare_bwd(int dtype, const void* dx16, const float* dflow_l, const float* frames, const float* flow_up, float* dflow_prev, float* dframes,
                                  int n, int t, int P, int pair_mode, int h, int w, hipStream_t) {
    g_elt.push_back({hit("prepare_bwd"), {dx16, dflow_l, frames, flow_up, dflow_prev, dframes}, {dtype, n, t, P, pair_mode, h, w}}); return VSR_OK;
}
int vsr_launch_spynet_dres(int dtype, const float* dflow, const float* res, void* out, int P, int h, int w, hipStream_t) {
    g_elt.push_back({hit("dres"), {dflow, res, out}, {dtype, P, h, w}}); return VSR_OK;
}

// ---- wide_recipes.h's launchers ----
int vsr_launch_conv_wide(int dtype, const VsrWideConv& c, hipStream_t) { hit("conv_wide"); g_wide.push_back({dtype, c}); return VSR_OK; }
int vsr_launch_pack_wide2(const float*, void* dst, int cout, int cin, int mode, hipStream_t) {
    hit("pack_wide2"); g_pack.push_back({1, VSR_BF16, 0, 0, 0, 0, 0, 0, 0, cout, cin, mode, dst}); return VSR_OK;
}
int vsr_launch_pack_wide(int dtype, const float*, void* dst, int cout, int cin, int mode, hipStream_t) {
    hit("pack_wide"); g_pack.push_back({0, dtype, 0, 0, 0, 0, 0, 0, 0, cout, cin, mode, dst}); return VSR_OK;
}
void vsr_wide2_grid(int ncob, int out_step, int N, int H, int W, int max_wg, int num_cus, int* nwx, int* cols, int* tiles) {
    *nwx = max_wg; *cols = ncob * out_step; *tiles = N * H * W + num_cus;      // a recorder: the real one is conv_wide.hip's
}
int vsr_launch_wgrad_pairs(int, const WgradArgs& a, int nsl, int ncob, int views, int ksplit, float* gw, int cin_total, hipStream_t) {
    hit("wgrad_pairs"); g_pairs.push_back({nsl, ncob, views, ksplit, cin_total, gw, a}); return VSR_OK;
}
int vsr_launch_wgrad_reduce_s2(const float*, int nwg, int, float* gw, int cin_total, int co0, int ci0, int view, hipStream_t) {
    hit("wgrad_reduce_s2"); g_reduce.push_back({1, nwg, 0, 0, 0, 0, 0, 0, 0, 1, cin_total, co0, ci0, view, gw, nullptr}); return VSR_OK;
}
int vsr_launch_up2_fwd(int dtype, const void* a, const void* b, void* out, int N, int H, int W, int C, hipStream_t) {
    g_elt.push_back({hit("up2_fwd"), {a, b, out}, {dtype, N, H, W, C}, 0.f}); return VSR_OK;
}
int vsr_launch_up2_bwd(int dtype, const void* dout, void* din, void* dmask, const void* m, float slope, int N, int H, int W, int C, hipStream_t) {
    g_elt.push_back({hit("up2_bwd"), {dout, din, dmask, m}, {dtype, N, H, W, C}, slope}); return VSR_OK;
}
int vsr_launch_mask_pm(int dtype, const void* g, const void* m, void* out, float slope, long long elems, hipStream_t) {
    g_elt.push_back({hit("mask"), {g, m, out}, {dtype, elems}, slope}); return VSR_OK;
}
int vsr_launch_maxpool2_fwd(int dtype, const void* in, void* out, int N, int Hi, int Wi, int C, hipStream_t) {
    g_elt.push_back({hit("pool_fwd"), {in, out}, {dtype, N, Hi, Wi, C}, 0.f}); return VSR_OK;
}
int vsr_launch_maxpool2_bwd(int dtype, const void* a, const void* dp, void* g, int N, int Hi, int Wi, int C, hipStream_t) {
    g_elt.push_back({hit("pool_bwd"), {a, dp, g}, {dtype, N, Hi, Wi, C}, 0.f}); return VSR_OK;
}
int vsr_launch_tap_l1(int dtype, const void* s, const void* h, void* g, float scale, int N, int H, int W, int C, double* partial, int nblocks, hipStream_t) {
    g_elt.push_back({hit("tap_l1"), {s, h, g, partial}, {dtype, N, H, W, C, nblocks}, scale}); return VSR_OK;
}
int vsr_launch_tap_sum(const double* partial, double* sums, int N, const int* nb, hipStream_t) {
    g_elt.push_back({hit("tap_sum"), {partial, sums}, {N, nb[0], nb[1], nb[2], nb[3], nb[4]}, 0.f}); return VSR_OK;
}

// ---- the flow warp's launchers (v: dtype, N, H, W, C, then flow_nstride and border where the launcher has them) ----
int vsr_launch_warp_fwd(int dtype, const void* in, const float* flow, void* out, int N, int H, int W, int C, long long flow_nstride, hipStream_t, int border) {
    g_elt.push_back({hit("warp_fwd"), {in, flow, out}, {dtype, N, H, W, C, flow_nstride, border}, 0.f}); return VSR_OK;
}
int vsr_launch_warp_bwd(int dtype, const void* dout, const float* flow, float* dacc, int N, int H, int W, int C, long long flow_nstride, hipStream_t, int border) {
    g_elt.push_back({hit("warp_bwd"), {dout, flow, dacc}, {dtype, N, H, W, C, flow_nstride, border}, 0.f}); return VSR_OK;
}
int vsr_launch_warp_bwd_gather(int dtype, const void* dout, const float* flow, const void* dtop, long long* S, int* far_count, void* out, int N, int H, int W, int C,
                               long long flow_nstride, hipStream_t) {
    g_elt.push_back({hit("warp_bwd_gather"), {dout, flow, dtop, S, far_count, out}, {dtype, N, H, W, C, flow_nstride}, 0.f}); return VSR_OK;
}
int vsr_launch_warp_bwd_flow(int dtype, const void* in, const void* dout, const float* flow, float* dflow, int N, int H, int W, int C, long long flow_nstride,
                             hipStream_t, int border) {
    g_elt.push_back({hit("warp_bwd_flow"), {in, dout, flow, dflow}, {dtype, N, H, W, C, flow_nstride, border}, 0.f}); return VSR_OK;
}
int vsr_launch_add_cast(int dtype, const void* a, const float* s, void* out, int N, int H, int W, int C, hipStream_t) {
    g_elt.push_back({hit("add_cast"), {a, s, out}, {dtype, N, H, W, C}, 0.f}); return VSR_OK;
}

// ---- the checks ----
static int g_fail = 0;
#define EXPECT(cond) do { if (!(cond)) { std::fprintf(stderr, HOSTCHECK_NAME ": line %d: %s\n", __LINE__, #cond); ++g_fail; } } while (0)
// a refusal: the status, and neither a pack nor a launch happened
#define REFUSED(call, status) do { reset(); EXPECT((call) == (status)); EXPECT(launches() == 0 && g_pack.empty()); } while (0)
static bool is(const EltCall& e, const char* name) { return std::strcmp(e.name, name) == 0; }

// real, small buffers (64 KiB, 256-byte aligned, zeroed): an accepted call hands them to the stubbed launch layer only
static float* hostcheck_buffer() {
    float* f = static_cast<float*>(std::aligned_alloc(256, 1 << 16));
    for (int i = 0; i < (1 << 14); ++i) f[i] = 0.f;
    return f;
}
// the end of a main(): the exit status, and HOSTCHECK_NAME " OK" on stdout when every check held
static int hostcheck_finish(float* f) {
    std::free(f);
    if (g_fail) { std::fprintf(stderr, HOSTCHECK_NAME ": %d check(s) failed\n", g_fail); return 1; }
    std::puts(HOSTCHECK_NAME " OK");
    return 0;
}
