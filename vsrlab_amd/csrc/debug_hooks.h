// The one declaration of every vsr_debug_* test hook the product library exports.  Every file that defines a hook includes this header,
// so a definition that disagrees with it does not compile; tools/hostcheck_launch_layer.h calls the hooks through it, and
// tests/test_host_logic.py holds the ctypes rows of _lib.DEBUG_SIGNATURES against it.  Not installed under include/: the hooks are not
// part of the ABI.  What each hook does is described at its definition.  (The vsr_debug_read_clk* entries exist in the VSR_CLOCK build
// only and are not listed.)
#pragma once

struct VsrDiscDesc;      // include/vsrlab_hip.h

extern "C" {

// hr_tail_hooks.hip
int vsr_debug_tail_last2_fwd(int dtype, const void* x_pm, const float* w, const float* bias, void* wpack, float* bias_pack, float* y, long long y_nstride,
                             const float* pres, const float* base_lr, long long base_nstride, int base_h, int base_w, int base_scale, int cout_real,
                             int N, int H, int W, void* stream);
int vsr_debug_tail_last2_dgrad(const float* dsr, long long dsr_nstride, const float* w, const void* aux_pm, int mask_src, void* sign_scratch,
                               int mask_mode, float slope, void* dx_pm, int N, int H, int W, void* stream);
int vsr_debug_tail_planar_c64(int dtype, const float* src, long long src_nstride, int pc, const float* w, const float* bias, void* wpack, void* y_pm,
                              int act, float slope, const void* aux_pm, int mask_mode, int N, int H, int W, void* stream);
int vsr_debug_tail_last2_wgrad(int dtype, const void* x_pm, const float* dy, long long dy_nstride, int pc, float* gw, float* gb, float* slab,
                               int N, int H, int W, void* stream);
int vsr_debug_tail_conv_unshuffle(int dtype, const void* x_pm, const float* w, const float* bias, int mode, void* wpack, void* y_planes,
                                  int N, int H, int W, void* stream);
int vsr_debug_tail_ps_dgrad(int dtype, const void* dy_pm, const float* w, void* wpack, void* dx_pm, const void* aux_pm, int mask_mode, int mask_src,
                            void* sign_scratch, int dy_planes, int dx_planes, int N, int H, int W, void* stream);
int vsr_debug_tail_ps_wgrads(int dtype, const void* x_pm, const void* dy_pm, int dy_planes, float* gw, float* gb, float* slab, int N, int H, int W,
                             void* stream);

// trunk_hooks.hip
int vsr_debug_trunk_conv(int dtype, int C, int ks, int mode, const void* x_pm, const float* w, const float* bias, void* wpack, void* y_pm, int act,
                         float slope, const void* res_pm, const void* aux_pm, int mask, void* sign_out, void* sign_bits, int make_bits, int unshuffle,
                         int N, int H, int W, void* stream);
int vsr_debug_trunk_stem(int dtype, int C, int cat, const void* feat_pm, const float* lr, long long lr_nstride, const float* w, const float* bias,
                         void* wpack, void* y_pm, int act, float slope, int N, int H, int W, void* stream);
int vsr_debug_trunk_stem_dgrad(int dtype, int C, int cat, const void* g0_pm, const float* w, void* wpack, void* dfeat_pm, float* dlr,
                               long long dlr_nstride, int accumulate, int N, int H, int W, void* stream);
int vsr_debug_trunk_point(int dtype, int C, int backward, const void* a_pm, const void* b_pm, const float* w, const float* bias, void* wpack,
                          void* y0_pm, void* y1_pm, int N, int H, int W, void* stream);
int vsr_debug_trunk_wgrad_cc(int dtype, int C, int ks, const void* const* x, const void* const* dy, int nseg, float* gw, int I_total, int i_off,
                             float* gb, int accumulate, float* slab, int N, int H, int W, void* stream);
int vsr_debug_trunk_stem_wgrads(int dtype, int C, int cat, const float* const* lr, long long x_nstride, const void* const* g0, int nseg,
                                const void* const* feat, const void* const* g0_feat, int nseg_feat, float* gw, float* gb, int accumulate, float* slab,
                                int N, int H, int W, void* stream);
int vsr_debug_trunk_chain(int dtype, int C, void* base, void* sync, const unsigned* layers, int nlayers, const float* const* w, int mode,
                          int N, int H, int W, void* stream);

// spynet_hooks.hip
int vsr_debug_spy_conv(int dtype, int j, const void* x_pm, const float* w, const float* bias, void* wpack, void* y, int act, const float* pres,
                       int N, int H, int W, void* stream);
int vsr_debug_spy_dgrad(int dtype, int j, const void* dy_pm, const float* w, void* wpack, void* dx_pm, const void* aux_pm, int N, int H, int W, void* stream);
int vsr_debug_spy_wgrad(int dtype, int j, const void* x_pm, const void* dy_pm, float* gw, float* gb, int accumulate, float* slab, int N, int H, int W,
                        void* stream);
int vsr_debug_spy_prepare(int dtype, const float* frames, const float* flow_prev, float* flow_up, void* x16_pm, int n, int t, int P, int pair_mode,
                          int h, int w, int level0, void* stream);
int vsr_debug_spy_prepare_bwd(int dtype, const void* dx16_pm, const float* dflow_l, const float* frames, const float* flow_up, float* dflow_prev,
                              float* dframes, int n, int t, int P, int pair_mode, int h, int w, void* stream);
int vsr_debug_spy_dres(int dtype, const float* dflow, const float* res, void* out_pm, int P, int h, int w, void* stream);
int vsr_debug_spy_planar(int op, const float* in, const float* in2, float* out, const float* mean, const float* std, long long planes, int h, int w,
                         int hu, int wu, void* stream);

// wide_hooks.hip
int vsr_debug_wide_conv(int dtype, int mode, int cout, int cin, const void* x_pm, const float* w, const float* bias, void* wpack, long long wpack_elems,
                        void* y_pm, int act, float slope, void* y_act_pm, const void* res_pm, const void* aux_pm, int max_wg, int N, int H, int W,
                        void* stream);
int vsr_debug_wide_wgrad(int dtype, int views, int xC, int dyC, const void* x_pm, const void* dy_pm, float* gw, float* slab, long long slab_floats,
                         int N, int H, int W, void* stream);
int vsr_debug_wide_up2_fwd(int dtype, const void* a_pm, const void* b_pm, void* out_pm, int N, int H, int W, int C, void* stream);
int vsr_debug_wide_up2_bwd(int dtype, const void* dout_pm, void* din_pm, void* dmask_pm, const void* m_pm, float slope, int N, int H, int W, int C,
                           void* stream);
int vsr_debug_wide_mask(int dtype, const void* g_pm, const void* m_pm, void* out_pm, float slope, long long elems, void* stream);
int vsr_debug_vgg_pool(int dtype, int op, const void* a_pm, const void* dp_pm, void* g_pm, int N, int Hi, int Wi, int C, void* stream);
int vsr_debug_vgg_tap(int dtype, const void* s_pm, void* h_pm, int grad, float scale, double* partial, double* sums, int N, int H, int W, int C, void* stream);
int vsr_debug_wide_grid(int ncob, int out_step, int N, int H, int W, int max_wg, int num_cus, int* out);

// warp_hooks.hip
int vsr_debug_warp_fwd(int dtype, int C, const void* in_pm, const float* flow, long long flow_nstride, void* out_pm, int border,
                       int N, int H, int W, void* stream);
int vsr_debug_warp_scatter(int dtype, int C, const void* dout_pm, const float* flow, long long flow_nstride, float* dacc, const void* a_pm,
                           void* out_pm, int border, int N, int H, int W, void* stream);
int vsr_debug_warp_gather(int dtype, int C, const void* dout_pm, const float* flow, long long flow_nstride, const void* dtop_pm, long long* S,
                          int* far_count, void* out_pm, int N, int H, int W, void* stream);
int vsr_debug_warp_flowgrad(int dtype, int C, const void* in_pm, const void* dout_pm, const float* flow, long long flow_nstride, float* dflow,
                            int border, int N, int H, int W, void* stream);
int vsr_debug_warp_add_cast(int dtype, int C, const void* a_pm, const float* s, void* out_pm, int N, int H, int W, void* stream);

// disc_engine.hip (beside the plan it reads), conv_wide.hip (beside the launcher whose grid it caps)
int vsr_debug_disc_plan(const VsrDiscDesc* d, int need_backward, long long* offsets, int count);
int vsr_debug_wide2_set_max_wg(int max_wg);

// conv3x3_chain.hip
int vsr_debug_chain_item(unsigned P, int own, int R, int tiles, int ntx, int nlayers);
int vsr_debug_chain_timeouts(unsigned* host_out);
int vsr_debug_chain_inject_error(int launches);
int vsr_debug_chain_timing_begin(void);
int vsr_debug_chain_timing_read(float* us, int* layers, int* variant, long long* pixels, int max);

// layer_ops.hip
int vsr_debug_warp_bwd_gather(int dtype, const void* dout_pm, const float* flow, const void* dtop_pm, long long* S, int* far_count,
                              void* out_pm, int N, int H, int W, void* stream);
int vsr_debug_warp_bwd_gather_c(int dtype, const void* dout_pm, const float* flow, const void* dtop_pm, long long* S, int* far_count,
                                void* out_pm, int N, int H, int W, int Cc, void* stream);

}  // extern "C"
