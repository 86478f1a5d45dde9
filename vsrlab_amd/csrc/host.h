// Host-side launch layer shared by the engines (engine.hip, spynet_engine.hip, cleaner_engine.hip, disc_engine.hip,
// perceptual_engine.hip) and the per-op entries (layer_ops.hip): arena bump allocator, argument checks, the ConvArgs / WgradArgs
// initialisers and the weight-gradient "launch + reduce" recipe.  No kernel lives here.  recipes.h builds the BasicVSR side's Ctx on it.
#pragma once
#include "kernels.h"
#include "../../include/vsrlab_hip.h"

#define CK(expr) do { int _s = (expr); if (_s != VSR_OK) return _s; } while (0)

struct Bump {
    size_t off = 0;
    size_t take(size_t bytes) {
        size_t o = off;
        off += (bytes + 255) & ~size_t(255);
        return o;
    }
};

inline size_t esize(int dtype) { return dtype == VSR_BF16 ? 2 : 4; }
inline bool bad_dtype(int dtype) { return dtype != VSR_F32 && dtype != VSR_BF16; }
inline bool bad_dims(int N, int H, int W) { return N < 1 || H < 1 || W < 1; }

// One blocked C-channel image in, one out, at one resolution (N x H x W): what every caller then specialises.
inline ConvArgs conv_args(int N, int H, int W, int C) {
    ConvArgs a = {};
    a.in_step = 1; a.Hs = H; a.Ws = W; a.N = N; a.H = H; a.W = W; a.nz = 1;
    a.out_step = 1; a.Hd = H; a.Wd = W; a.CD = C; a.cout_real = C; a.dst_nstride = pm_image_elems(H, W, C);
    for (int s = 0; s < VSR_MAX_SRC; ++s) a.src_nstride[s] = pm_image_elems(H, W, C);
    return a;
}

inline WgradArgs wg_base(int N, int H, int W, int Cx = 64, int Cy = 64) {       // Cx / Cy: channels of the pixel-major X / dY
    WgradArgs a = {};
    a.N = N; a.H = H; a.W = W; a.nseg = 1;
    a.x_step = 1; a.Hx = H; a.Wx = W; a.x_nstride = pm_image_elems(H, W, Cx);
    a.dy_step = 1; a.Hy = H; a.Wy = W; a.dy_nstride = pm_image_elems(H, W, Cy);
    return a;
}

// A weight-gradient slab buffer holds VSR_WGRAD_NWG partials of the largest shape, 3x3 64 -> 64: every plan takes this many floats
// and wgrad_run() caps the workgroups of the other shapes by it.
inline int wgrad_slab_stride3() { int cp, xp, stride; vsr_wgrad_slab_dims(3, 64, 64, &cp, &xp, &stride); return stride; }
inline size_t wgrad_slab_floats() { return (size_t)VSR_WGRAD_NWG * wgrad_slab_stride3(); }
inline size_t wgrad_slab_bytes() { return wgrad_slab_floats() * 4; }

struct WgradShape { int ks, cx; bool x_planar; int cout; bool dy_planar; };      // the template shape of vsr_launch_wgrad
struct WgradDst {                                                                // where vsr_launch_wgrad_reduce puts the sums
    int cout_real, cin_real; float* gw; int I_total, i_off, o_mul, o_add; float* gb; int accumulate;
};

// One weight-gradient launch into `slab` (wgrad_slab_bytes()); *nslabs: the partials it wrote.
// The workgroup count decides how the pixels are partitioned and so the last bits of the fp32 sums: min(tiles, VSR_WGRAD_NWG), capped
// by what the slab buffer holds of this shape's partials (never binding for 3x3 64 -> 64), rounded down to even (the bf16 64 -> 64
// kernel runs two row-halves per workgroup).  even = false: vsr_conv3x3_c64_wgrad has always launched an odd tile count as it is --
// the bf16 kernel halves it to the same slab count either way, but the fp32 kernel (and VSRLAB_AMD_GENERIC_WGRAD) partitions
// e.g. 3 tiles over 3 workgroups instead of 2, and its callers' results are kept bit for bit.
inline int wgrad_launch(hipStream_t st, int dtype, float* slab, WgradArgs& a, const WgradShape& s, bool even, int* nslabs) {
    int cp, xpd, stride;
    vsr_wgrad_slab_dims(s.ks, s.cx, s.cout, &cp, &xpd, &stride);
    a.slab = slab; a.slab_stride = stride;
    const int tiles = a.N * cdiv(a.H, 8) * cdiv(a.W, 32);
    const long long cap = (long long)wgrad_slab_floats() / stride;
    int nwg = tiles < VSR_WGRAD_NWG ? tiles : VSR_WGRAD_NWG;
    if (nwg > cap) nwg = (int)cap;
    if (even && nwg > 1) nwg &= ~1;
    if (dtype == VSR_BF16 && s.ks == 3 && s.cx == 64 && !s.x_planar && s.cout == 16 && s.dy_planar && a.nseg == 1 && a.x_step == 1 &&
        a.dy_step == 1 && a.Hx == a.H && a.Wx == a.W && a.Hy == a.H && a.Wy == a.W)
        // 64 -> 3 conv with a planar cotangent (conv_last.2, the pre-clean out conv): streaming kernel of hr_tail.hip
        // (pc: a cotangent of 1 or 2 planes has no plane 2 to read -- the launcher's default of 3 read past it)
        return vsr_launch_last2_wgrad(a.x[0], reinterpret_cast<const float*>(a.dy[0]), a.dy_nstride, slab, stride, a.N, a.H, a.W, nslabs, st,
                                      a.dy_planar_c ? a.dy_planar_c : 3);
    return vsr_launch_wgrad(dtype, s.ks, s.cx, s.x_planar, s.cout, s.dy_planar, a, nwg, nslabs, st);
}
// ... + its reduction into d.gw / d.gb (neither wanted: nothing is launched; a bias gradient needs its weight's)
inline int wgrad_run(hipStream_t st, int dtype, float* slab, WgradArgs& a, const WgradShape& s, const WgradDst& d, bool even = true) {
    if (!d.gw && !d.gb) return VSR_OK;
    int nslabs = 0;
    CK(wgrad_launch(st, dtype, slab, a, s, even, &nslabs));
    if (!d.gw) return VSR_ERR_BADARG;
    return vsr_launch_wgrad_reduce(slab, nslabs, s.ks, s.cx, s.cout, d.cout_real, d.cin_real, d.gw, d.I_total, d.i_off, d.o_mul, d.o_add, d.gb,
                                   d.accumulate, st);
}
