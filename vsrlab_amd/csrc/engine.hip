// Whole-clip scheduler for the BasicVSR path: plans one workspace arena, then enqueues every
// kernel of BasicVSR.forward (basicvsr.py:39-83) and of its backward on one HIP
// stream.  No allocation, no synchronisation, no global state: the plan is a pure function of the
// descriptor, so forward and backward recompute identical offsets.
//
// Memory-rich by design (288 GB HBM3E): every trunk activation AND every trunk activation-gradient
// of the clip is retained, so each layer's weight gradient is ONE split-K launch over all t frames
// (see wgrad_mfma.hip) instead of t launches + t reductions.
#include <vector>
#include "recipes.h"
#include "spynet_engine.h"

namespace {

struct Plan {
    VsrBasicVSRDesc d = {};
    // mid channels: 64 (the whole-path entries: chains, persistent kernels, sign bits, phase planes) or 16 / 32 (the narrow entries:
    // one generic-kernel launch per layer, ReLU / LeakyReLU masks of the data gradients from the stored activations); CO: the conv
    // template's output rows for C outputs (C = 16 runs on the 32-row template with cout_real = 16)
    int C = 64, CO = 64;
    bool sb = false;             // sign bits of the masked data gradients are kept (bf16 training at C = 64)
    bool bwd = false, flowgrad = false;          // flowgrad: train_flow (basicvsr.py:25-28), SPyNet is differentiated too
    bool diet = false;           // VsrBasicVSRDesc.arena_mode = 1 (training only): see vsrlab_hip.h
    int rb = 0, n = 0, t = 0, h = 0, w = 0, dtype = VSR_F32;
    int scale = 4, ups = 2;      // upscale (2 or 4, basicvsr.py:12-23) and its PixelShufflePack count scale / 2
    bool unsh = false;           // the gradients INTO the pixel-shuffle layers (G_U1, G_U0) are kept phase-separated (ConvArgs::unshuffle)
    size_t es = 4;
    size_t px1 = 0;             // elements of one blocked (n,h,w,64) tensor
    size_t s_elems = 0;         // elements of the plain 64-bit fixed-point warp-scatter accumulator (n,h,w,64)
    // packed weights / biases
    size_t stem_w[2] = {}, stem_wd[2] = {}, stem_b[2] = {};
    std::vector<size_t> blk_w[2], blk_wd[2], blk_b[2];     // [2*rb]: conv1, conv2 alternating
    size_t point_w = 0, point_wd = 0, point_b = 0;
    size_t up_w[2] = {}, up_wd[2] = {}, up_b[2] = {};
    size_t last0_w = 0, last0_wd = 0, last0_b = 0, last2_w = 0, last2_wd = 0, last2_b = 0;
    SpyPlan spy;
    size_t flows = 0;               // fp32 planar [2*n*(t-1)][2][h][w]: first half backward, second half forward
    // trunk activations: [dir][frame]
    std::vector<size_t> Wp[2], X[2], A[2];      // X: (rb+1) per frame, A: rb per frame (saved mode)
    std::vector<size_t> SB[2];                  // sign bits of A (bf16 build): rb per frame, 8 bytes per lane and 8x32 tile
    std::vector<size_t> feat[2];                // = X[rb]
    size_t scratchA[2] = {}, scratchW[2] = {};            // inference mode, per direction (the directions run concurrently)
    // reconstruction
    std::vector<size_t> Pt, U0, U1, C0;
    std::vector<size_t> SBC0;                   // sign bits of C0 = LeakyReLU(conv_last.0) per frame (bf16 build, training)
    std::vector<size_t> SBPt;                   // sign bits of Pt = LeakyReLU(point_conv) per frame (bf16 build, training)
    std::vector<size_t> SBX0[2];                // sign bits of the stem outputs X_0 (bf16 build, training): mask of the block-0 data gradient
    // backward
    std::vector<size_t> G0[2], G1[2], DX[2];    // G1: rb per frame, DX: (rb+1) per frame (DX[0] unused -> G0)
    std::vector<size_t> dFeatB, dFF;            // per frame: d outputs[i], d feat_prop(i) from the reconstruction
    size_t S[2] = {}, dWp[2] = {}, slab[2] = {};               // per direction / stream
    size_t far_cnt = 0;                             // [2][t] ints: far-source counters of the gather-form warp backward
    size_t chain_sync[2] = {0, 0};              // counters of the trunk chain launches (0: chains not planned)
    bool chains = true;                         // VSRLAB_AMD_CHAIN, read ONCE per engine call (build()): 0 one launch per layer, else chains
    size_t G_C0 = 0, G_U1 = 0, G_U0 = 0, G_P = 0;
    // r04 (full arena, bf16): the gradients into the two pixel-shuffle layers and into the 1x1 fuse conv are kept PER FRAME (+9.8 GB per
    // clip at config 2), so that those layers' weight gradients are all-frames launches like the trunks' (28 + 28 + 14 one-frame launches
    // of 50-140 us each per step before: a one-frame launch at LR size is mostly prologue, slab write and first-tile latency)
    bool hrdef = false;
    std::vector<size_t> GU1f, GU0f, GPf;
    size_t dflows = 0;              // fp32 planar, layout of `flows`: gradient w.r.t. the flows (train_flow / input gradient)
    size_t stem_wd_lr[2] = {};       // data-gradient weights of the stems' 3 LR input channels (input gradient)
    size_t total = 0;

    size_t xoff(int dir, int i, int b) const { return X[dir][(size_t)i * (rb + 1) + b]; }
    size_t aoff(int dir, int i, int b) const { return A[dir][(size_t)i * rb + b]; }
    size_t sboff(int dir, int i, int b) const { return SB[dir][(size_t)i * rb + b]; }
    // diet: the trunk's activation gradients live in a ring of two buffers per kind and direction (block parity): a block's weight
    // gradients are launched right behind its data gradients, on the same stream, so its buffers are free two blocks later
    size_t g1off(int dir, int i, int b) const { return diet ? G1[dir][b & 1] : G1[dir][(size_t)i * rb + b]; }
    size_t dxoff(int dir, int i, int b) const { return diet ? DX[dir][b & 1] : DX[dir][(size_t)i * (rb + 1) + b]; }

    int build(const VsrBasicVSRDesc& desc, int mode, bool narrow = false) {     // mode: 0 inference, 1 training (frozen flow), 2 training incl. SPyNet
        d = desc; bwd = mode >= 1; flowgrad = mode >= 2;
        { const char* e = getenv("VSRLAB_AMD_CHAIN"); chains = !(e && e[0] == '0'); }
        if (d.arena_mode != 0 && d.arena_mode != 1) return VSR_ERR_BADARG;
        diet = bwd && d.arena_mode == 1;
        rb = d.res_blocks; n = d.n; t = d.t; h = d.h; w = d.w; dtype = d.dtype;
        scale = d.upscale; ups = scale / 2; unsh = false;
        const bool width_ok = narrow ? (d.mid_channels == 16 || d.mid_channels == 32) : d.mid_channels == 64;
        if (!width_ok || (scale != 4 && scale != 2) || rb < 1 || n < 1 || t < 1 || t > 32 || h < 1 || w < 1) return VSR_ERR_UNSUPPORTED;
        if (dtype != VSR_F32 && dtype != VSR_BF16) return VSR_ERR_BADARG;
        const int C = d.mid_channels;
        this->C = C; CO = C < 32 ? 32 : C;
        sb = bwd && dtype == VSR_BF16 && C == 64;
        es = esize(dtype);
        px1 = (size_t)n * pm_image_elems(h, w, C);
        s_elems = (size_t)n * h * w * C;
        // a2: a blocked C-channel tensor at 2h x 2w; a4: at the output size scale h x scale w (= a2 for upscale 2, which has no U1);
        // a4h: conv_last.0's 64-channel output (and its gradient) at the output size (= a4 at C = 64)
        const size_t a2 = (size_t)n * pm_image_elems(2 * h, 2 * w, C) * es, a4 = (size_t)n * pm_image_elems(scale * h, scale * w, C) * es;
        const size_t a4h = (size_t)n * pm_image_elems(scale * h, scale * w, 64) * es;
        Bump b;
        const size_t w64 = (size_t)9 * CO * C * es;
        for (int dir = 0; dir < 2; ++dir) {
            stem_w[dir] = b.take(w64 + (size_t)9 * CO * 16 * es);
            stem_wd[dir] = b.take(w64);
            stem_b[dir] = b.take(C * 4);
            blk_w[dir].resize(2 * rb); blk_wd[dir].resize(2 * rb); blk_b[dir].resize(2 * rb);
            for (int k = 0; k < 2 * rb; ++k) { blk_w[dir][k] = b.take(w64); blk_wd[dir][k] = b.take(w64); blk_b[dir][k] = b.take(C * 4); }
        }
        point_w = b.take((size_t)2 * CO * C * es); point_wd = b.take((size_t)2 * CO * C * es); point_b = b.take(C * 4);
        for (int k = 0; k < 2; ++k) { up_w[k] = b.take(4 * w64); up_wd[k] = b.take(4 * w64); up_b[k] = b.take(4 * C * 4); }
        last0_w = b.take((size_t)9 * 64 * C * es); last0_wd = b.take((size_t)9 * CO * 64 * es); last0_b = b.take(64 * 4);
        last2_w = b.take((size_t)9 * 32 * 64 * es); last2_wd = b.take((size_t)9 * 64 * 16 * es); last2_b = b.take(64 * 4);
        if (t > 1) spy.plan(b, 2 * n * (t - 1), n * t, h, w, dtype);
        flows = b.take((size_t)2 * n * (t > 1 ? t - 1 : 1) * 2 * h * w * 4);
        const size_t a1 = px1 * es;
        for (int dir = 0; dir < 2; ++dir) {
            Wp[dir].assign(t, 0); feat[dir].assign(t, 0);
            if (bwd) {
                X[dir].assign((size_t)t * (rb + 1), 0); A[dir].assign((size_t)t * rb, 0); SB[dir].assign((size_t)t * rb, 0);
                SBX0[dir].assign(t, 0);
                const size_t sbytes = sb ? (size_t)n * cdiv(h, 8) * cdiv(w, 32) * 2048 : 256;
                for (int i = 0; i < t; ++i) {
                    SBX0[dir][i] = b.take(sbytes);
                    Wp[dir][i] = b.take(a1);
                    for (int k = 0; k <= rb; ++k) X[dir][(size_t)i * (rb + 1) + k] = b.take(a1);
                    for (int k = 0; k < rb; ++k) A[dir][(size_t)i * rb + k] = b.take(a1);
                    for (int k = 0; k < rb; ++k) SB[dir][(size_t)i * rb + k] = b.take(sbytes);
                    feat[dir][i] = xoff(dir, i, rb);
                }
            } else {
                for (int i = 0; i < t; ++i) feat[dir][i] = b.take(a1);
            }
        }
        for (int dir = 0; dir < 2; ++dir) { scratchA[dir] = b.take(a1); scratchW[dir] = b.take(a1); }
        const int nrec = bwd ? t : 1;
        Pt.assign(t, 0); U0.assign(t, 0); U1.assign(t, 0); C0.assign(t, 0);
        // diet: the upsampled tensors of a frame (U0, U1 = the upsample layers' outputs, C0 = conv_last.0's) are not kept: one shared
        // buffer each, recomputed from Pt[i] at the top of the frame's reconstruction backward (2.4 GB per frame at 540p x4)
        for (int i = 0; i < nrec; ++i) {
            Pt[i] = b.take(a1);
            if (diet && i > 0) { U0[i] = U0[0]; U1[i] = U1[0]; C0[i] = C0[0]; } else { U0[i] = b.take(a2); U1[i] = ups == 2 ? b.take(a4) : U0[i]; C0[i] = b.take(a4h); }
        }
        for (int i = nrec; i < t; ++i) { Pt[i] = Pt[0]; U0[i] = U0[0]; U1[i] = U1[0]; C0[i] = C0[0]; }
        SBC0.assign(t, 0); SBPt.assign(t, 0);
        if (sb)
            for (int i = 0; i < t; ++i) {
                SBC0[i] = b.take((size_t)n * cdiv(scale * h, 8) * cdiv(scale * w, 32) * 2048);
                SBPt[i] = b.take((size_t)n * cdiv(h, 8) * cdiv(w, 32) * 2048);
            }
        if (bwd) {
            for (int dir = 0; dir < 2; ++dir) {
                G0[dir].assign(t, 0);
                for (int i = 0; i < t; ++i) G0[dir][i] = b.take(a1);
                if (diet) {
                    G1[dir].assign(2, 0); DX[dir].assign(2, 0);
                    for (int k = 0; k < 2; ++k) { G1[dir][k] = b.take(a1); DX[dir][k] = b.take(a1); }
                } else if (dir == 0) {
                    G1[dir].assign((size_t)t * rb, 0); DX[dir].assign((size_t)t * (rb + 1), 0);
                    for (int i = 0; i < t; ++i) {
                        for (int k = 0; k < rb; ++k) G1[dir][(size_t)i * rb + k] = b.take(a1);
                        for (int k = 1; k <= rb; ++k) DX[dir][(size_t)i * (rb + 1) + k] = b.take(a1);
                    }
                } else {
                    // ONE set of trunk activation gradients for both directions (r04: 2 x 7 x 60 x 66.8 MB = 56 GB at config 2 before):
                    // a direction's gradients are dead once its all-frames weight-gradient launches have read them, and
                    // backward_impl runs direction 1 (data gradients, then weight gradients) and then direction 0 on ONE stream
                    G1[dir] = G1[0]; DX[dir] = DX[0];
                }
            }
            dFeatB.assign(t, 0); dFF.assign(t, 0);
            for (int i = 0; i < t; ++i) { dFeatB[i] = b.take(a1); dFF[i] = b.take(a1); }
            for (int dir = 0; dir < 2; ++dir) { S[dir] = b.take(s_elems * 8); dWp[dir] = b.take(a1); }
            far_cnt = b.take((size_t)2 * 32 * 4);
            G_C0 = b.take(a4h); G_P = b.take(a1);
            // diet: dU1 is written after C0's last use and dU0 after U1's (recon_backward): they take those buffers
            // (upscale 2: there is no U1 / dU1; dU0 is conv_last.0's data gradient and takes C0's buffer in the diet arena)
            // r04 (full arena, bf16, persistent kernels): both are stored as four phase planes, whose 32-pixel row padding can exceed the
            // whole image's (2 ceil(x) >= ceil(2 x)): four planes of the next lower resolution each
            unsh = !diet && dtype == VSR_BF16 && !vsr_env().generic_conv && C == 64;
            const size_t gu1 = unsh && 4 * a2 > a4 ? 4 * a2 : a4, gu0 = unsh && 4 * a1 > a2 ? 4 * a1 : a2;
            if (ups == 2) { if (diet) { G_U1 = C0[0]; G_U0 = U1[0]; } else { G_U1 = b.take(gu1); G_U0 = b.take(gu0); } }
            else { G_U0 = diet ? C0[0] : b.take(gu0); G_U1 = G_U0; }
            hrdef = unsh;
            GU1f.assign(t, G_U1); GU0f.assign(t, G_U0); GPf.assign(t, G_P);
            if (hrdef)
                for (int i = 1; i < t; ++i) {             // frame 0 keeps the buffers above
                    GU0f[i] = b.take(gu0);
                    GU1f[i] = ups == 2 ? b.take(gu1) : GU0f[i];
                    GPf[i] = b.take(a1);
                }
            for (int k = 0; k < 2; ++k) slab[k] = b.take(wgrad_slab_bytes());
        }
        // the trunk chains' work / row counters (conv3x3_chain.hip), one block per direction (= per stream)
        for (int dir = 0; dir < 2; ++dir) chain_sync[dir] = sb ? b.take(vsr_chain_sync_bytes(VSR_CHAIN_MAX_LAYERS, n, h, w)) : 0;
        // appended last, so that every other offset is the same in modes 1 and 2
        dflows = 0;
        if (flowgrad && t > 1) {
            dflows = b.take((size_t)2 * n * (t - 1) * 2 * h * w * 4);
            spy.plan_save(b, dtype);
        }
        if (flowgrad) {
            for (int dir = 0; dir < 2; ++dir) stem_wd_lr[dir] = b.take((size_t)9 * 32 * C * es);
        }
        total = b.off;
        return VSR_OK;
    }
};

// lane 0: the caller's stream, 1: the helper stream (selects the per-stream weight-gradient slab buffer)
Ctx engine_ctx(const Plan& p, char* ws, hipStream_t st, int lane) {
    return Ctx(ws, st, p.dtype, p.C, p.bwd ? reinterpret_cast<float*>(ws + p.slab[lane]) : nullptr);
}

// parameter index helpers (order documented in vsrlab_hip.h)
struct PIdx {
    int rb;
    int ups = 2;                 // PixelShufflePack count = upscale // 2 (basicvsr.py:19)
    int trunk_base(int dir) const { return dir * (2 + 4 * rb); }
    int stem_w(int dir) const { return trunk_base(dir); }
    int stem_b(int dir) const { return trunk_base(dir) + 1; }
    int blk_w(int dir, int k) const { return trunk_base(dir) + 2 + 2 * k; }      // k = 2*block + (conv2 ? 1 : 0)
    int blk_b(int dir, int k) const { return trunk_base(dir) + 3 + 2 * k; }
    int point_w() const { return 2 * (2 + 4 * rb); }
    int point_b() const { return point_w() + 1; }
    int up_w(int k) const { return point_w() + 2 + 2 * k; }
    int up_b(int k) const { return up_w(k) + 1; }
    int last0_w() const { return point_w() + 2 + 2 * ups; }
    int last0_b() const { return last0_w() + 1; }
    int last2_w() const { return last0_w() + 2; }
    int last2_b() const { return last0_w() + 3; }
    int spy_base() const { return last0_w() + 4; }
    int spy_w(int lvl, int j) const { return spy_base() + (lvl * NSPY + j) * 2; }
    int spy_b(int lvl, int j) const { return spy_w(lvl, j) + 1; }
    int spy_mean() const { return spy_base() + 60; }
    int spy_std() const { return spy_base() + 61; }
    int count() const { return spy_base() + 62; }
};

int pack_all_collect(const Ctx& c, const Plan& p, const float* const* prm);
// every weight / bias pack of a forward (~465 tensors) in a handful of multi-tensor launches
int pack_all(const Ctx& c, const Plan& p, const float* const* prm) {
    std::vector<VsrPackDesc> descs;
    descs.reserve(512);
    c.batch = &descs;
    const int rc = pack_all_collect(c, p, prm);
    c.batch = nullptr;
    if (rc != VSR_OK) return rc;
    return vsr_launch_pack_multi(descs.data(), (int)descs.size(), c.st);
}

int pack_all_collect(const Ctx& c, const Plan& p, const float* const* prm) {
    const PIdx ix{p.rb, p.ups};
    const int C = p.C, CO = p.CO;           // (CO: packed rows of a C-output weight set)
    for (int dir = 0; dir < 2; ++dir) {
        const float* sw = prm[ix.stem_w(dir)];
        CK(c.pack_stem(sw, c.at(p.stem_w[dir]), true));
        CK(c.pack_bias(prm[ix.stem_b(dir)], c.at(p.stem_b[dir]), C));
        if (p.bwd) CK(c.pack_stem_dgrad(sw, c.at(p.stem_wd[dir])));
        if (p.flowgrad) CK(c.pack_stem_dlr(sw, c.at(p.stem_wd_lr[dir]), true));
        for (int k = 0; k < 2 * p.rb; ++k) {
            CK(c.pack_cc(3, prm[ix.blk_w(dir, k)], c.at(p.blk_w[dir][k]), 0));
            if (p.bwd) CK(c.pack_cc(3, prm[ix.blk_w(dir, k)], c.at(p.blk_wd[dir][k]), 1));
            CK(c.pack_bias(prm[ix.blk_b(dir, k)], c.at(p.blk_b[dir][k]), C));
        }
    }
    CK(c.pack_point(prm[ix.point_w()], c.at(p.point_w), 0));
    if (p.bwd) CK(c.pack_point(prm[ix.point_w()], c.at(p.point_wd), 1));
    CK(c.pack_bias(prm[ix.point_b()], c.at(p.point_b), C));
    for (int k = 0; k < p.ups; ++k) {
        CK(c.pack_ps(prm[ix.up_w(k)], c.at(p.up_w[k]), 0));
        if (p.bwd) CK(c.pack_ps(prm[ix.up_w(k)], c.at(p.up_wd[k]), 1));
        CK(c.pack_ps_bias(prm[ix.up_b(k)], (float*)c.at(p.up_b[k])));
    }
    // conv_last.0: C -> 64 (basicvsr.py:20); its data gradient 64 -> C
    CK(c.pack(prm[ix.last0_w()], c.at(p.last0_w), 9, 64, C, 64, C, C, 0, 1, 0, 0));
    if (p.bwd) CK(c.pack(prm[ix.last0_w()], c.at(p.last0_wd), 9, CO, 64, C, 64, C, 0, 1, 0, 1));
    CK(c.pack_bias(prm[ix.last0_b()], c.at(p.last0_b), 64));
    CK(c.pack(prm[ix.last2_w()], c.at(p.last2_w), 9, 32, 64, 3, 64, 64, 0, 1, 0, 0));
    if (p.bwd) CK(c.pack(prm[ix.last2_w()], c.at(p.last2_wd), 9, 64, 16, 64, 3, 64, 0, 1, 0, 1));
    CK(c.pack_bias(prm[ix.last2_b()], c.at(p.last2_b), 3));
    if (p.t > 1) CK(vsr::spynet_pack(c, p.spy, prm, ix.spy_base()));
    return VSR_OK;
}

// The 2 rb convolutions of a frame's residual blocks (and their data gradients) as ONE launch (conv3x3_chain.hip): training
// arena only (every layer has a buffer of its own there), bf16.  VSRLAB_AMD_CHAIN=0 (read once per engine call, Plan::build) = one launch per layer.
bool chain_on(const Plan& p) { return p.chains && p.chain_sync[0] && p.chain_sync[1] && 2 * p.rb <= VSR_CHAIN_MAX_LAYERS; }
unsigned chain_off(size_t o) { return (unsigned)(o >> 8); }
int chain_launch(const ChainArgs& a, hipStream_t st) {
    // A batch of clips, image by image (r04).  Layer l + 1 reads what layer l has just written and what layer l - 1 wrote (the
    // identity): with one 540p image in flight those ~200 MB live in the 256 MiB Infinity Cache, with two they do not -- measured on
    // `bench.py --clips 2`: 37.0 us per image and layer in one launch of both against 34.6 us with one clip.  Large images only:
    // small ones need both images' tiles to fill the chip.
    const size_t img_bytes = (size_t)pm_image_elems(a.H, a.W, 64) * 2, sb_bytes = (size_t)cdiv(a.H, 8) * cdiv(a.W, 32) * 2048;
    if (a.N > 1 && img_bytes * 3 * a.N > ((size_t)192 << 20) && cdiv(a.H, 8) * cdiv(a.W, 32) >= 2 * vsr_num_cus()) {
        for (int m = 0; m < a.N; ++m) {
            ChainArgs b = a;
            b.N = 1;
            const unsigned di = (unsigned)((m * img_bytes) >> 8), ds = (unsigned)((m * sb_bytes) >> 8);
            for (int l = 0; l < a.nlayers; ++l) {
                ChainLayer& L = b.layer[l];
                L.src += di; L.dst += di;
                if (L.res != 0xffffffffu) L.res += di;
                if (L.sbits != 0xffffffffu) L.sbits += ds;
                if (L.sout != 0xffffffffu) L.sout += ds;
            }
            CK(chain_launch(b, st));
        }
        return VSR_OK;
    }
    return vsr_launch_conv3x3_chain(a, vsr_num_cus(), st);
}
int trunk_chain_forward(const Ctx& c, const Plan& p, int dir, int i) {
    ChainArgs a = {};
    a.base = c.ws; a.sync = (unsigned*)c.at(p.chain_sync[dir]); a.N = p.n; a.H = p.h; a.W = p.w; a.nlayers = 2 * p.rb;
    for (int b = 0; b < p.rb; ++b) {
        ChainLayer& l1 = a.layer[2 * b];
        l1 = {chain_off(p.xoff(dir, i, b)), chain_off(p.aoff(dir, i, b)), 0xffffffffu, 0xffffffffu, chain_off(p.sboff(dir, i, b)),
              chain_off(p.blk_w[dir][2 * b]), chain_off(p.blk_b[dir][2 * b]), CHAIN_RELU};
        ChainLayer& l2 = a.layer[2 * b + 1];
        l2 = {chain_off(p.aoff(dir, i, b)), chain_off(p.xoff(dir, i, b + 1)), chain_off(p.xoff(dir, i, b)), 0xffffffffu, 0xffffffffu,
              chain_off(p.blk_w[dir][2 * b + 1]), chain_off(p.blk_b[dir][2 * b + 1]), CHAIN_SKIP};
    }
    return chain_launch(a, c.st);
}
// dA_b = dgrad(conv2)(dX_{b+1}) * ReLU'(A_b), dX_b = dX_{b+1} + dgrad(conv1)(dA_b) for b = rb-1 .. 1, and dA_0: 2 rb - 1 layers
int trunk_chain_backward(const Ctx& c, const Plan& p, int dir, int i) {
    ChainArgs a = {};
    a.base = c.ws; a.sync = (unsigned*)c.at(p.chain_sync[dir]); a.N = p.n; a.H = p.h; a.W = p.w;
    int L = 0;
    for (int b = p.rb - 1; b >= 0; --b) {
        a.layer[L++] = {chain_off(p.dxoff(dir, i, b + 1)), chain_off(p.g1off(dir, i, b)), 0xffffffffu, chain_off(p.sboff(dir, i, b)), 0xffffffffu,
                        chain_off(p.blk_wd[dir][2 * b + 1]), 0xffffffffu, CHAIN_MASK};
        if (b > 0)
            a.layer[L++] = {chain_off(p.g1off(dir, i, b)), chain_off(p.dxoff(dir, i, b)), chain_off(p.dxoff(dir, i, b + 1)), 0xffffffffu, 0xffffffffu,
                            chain_off(p.blk_wd[dir][2 * b]), 0xffffffffu, CHAIN_SKIP};
    }
    a.nlayers = L;
    return chain_launch(a, c.st);
}

// one call of ResidualBlock (conv.py:94-103) on cat([lr_i, warped feat])
int trunk_forward(const Ctx& c, const Plan& p, int dir, int i, const void* warped, const float* lrs) {
    const int n = p.n, h = p.h, w = p.w, rb = p.rb;
    void* x = p.bwd ? c.at(p.xoff(dir, i, 0)) : c.at(p.feat[dir][i]);
    {   // warped: null => zeros (first frame of the direction)
        CK(c.stem(true, warped, lrs + (size_t)i * 3 * h * w, (long long)p.t * 3 * h * w, c.at(p.stem_w[dir]), c.fat(p.stem_b[dir]), x, ACT_LEAKY, 0.f, n, h, w));
        // the stem runs on the generic two-source kernel: its LeakyReLU sign bits for the block-0 data gradient come from a 66 MB pass
        if (p.sb) CK(vsr_launch_sign_bits_c64(x, c.at(p.SBX0[dir][i]), n, h, w, c.st));
    }
    if (chain_on(p)) return trunk_chain_forward(c, p, dir, i);
    for (int b = 0; b < rb; ++b) {      // x + conv2(relu(conv1(x)))   (conv.py:89-92)
        void* act = p.bwd ? c.at(p.aoff(dir, i, b)) : c.at(p.scratchA[dir]);
        void* xn = p.bwd ? c.at(p.xoff(dir, i, b + 1)) : x;   // inference: in place (residual read = own pixel)
        CK(c.conv(3, x, c.at(p.blk_w[dir][2 * b]), c.fat(p.blk_b[dir][2 * b]), act, ACT_RELU, nullptr, nullptr, 0, n, h, w,
                    p.sb ? c.at(p.sboff(dir, i, b)) : nullptr));
        CK(c.conv(3, act, c.at(p.blk_w[dir][2 * b + 1]), c.fat(p.blk_b[dir][2 * b + 1]), xn, ACT_NONE, x, nullptr, 0, n, h, w));
        x = xn;
    }
    return VSR_OK;
}

// conv_last.0 + LeakyReLU (basicvsr.py:20-21): U1[i] (C channels) -> C0[i] (64 channels) at the output size
int last0_forward(const Ctx& c, const Plan& p, int i, void* sign_out) {
    const int S = p.scale;
    if (p.C == 64)
        return c.conv(3, c.at(p.U1[i]), c.at(p.last0_w), c.fat(p.last0_b), c.at(p.C0[i]), ACT_LEAKY, nullptr, nullptr, 0, p.n, S * p.h, S * p.w, sign_out);
    ConvArgs a = conv_args(p.n, S * p.h, S * p.w, c.C);
    a.src[0] = c.at(p.U1[i]); a.wpack = c.at(p.last0_w); a.bias = c.fat(p.last0_b); a.dst[0] = c.at(p.C0[i]); a.act = ACT_LEAKY;
    a.CD = 64; a.cout_real = 64; a.dst_nstride = pm_image_elems(S * p.h, S * p.w, 64);
    return vsr_launch_conv(c.dtype, 3, 1, p.C, p.C, 0, 64, EPI_NHWC, a, c.st);
}

int recon_forward(const Ctx& c, const Plan& p, int i, const float* lrs, float* sr) {
    const int n = p.n, h = p.h, w = p.w;
    // point_conv on cat([outputs[i], feat_prop]) (basicvsr.py:75-77)
    CK(c.point_conv(c.at(p.feat[0][i]), c.at(p.feat[1][i]), c.at(p.point_w), c.fat(p.point_b), c.at(p.Pt[i]), n, h, w));
    if (p.sb) CK(vsr_launch_sign_bits_c64(c.at(p.Pt[i]), c.at(p.SBPt[i]), n, h, w, c.st));   // mask of upsample.0's data gradient
    const int S = p.scale;                     // upscale: S / 2 PixelShufflePacks (basicvsr.py:19); U1 = U0 for S = 2 (Plan::build)
    CK(c.conv_ps(c.at(p.Pt[i]), c.at(p.up_w[0]), c.fat(p.up_b[0]), c.at(p.U0[i]), n, h, w));
    if (p.ups == 2) CK(c.conv_ps(c.at(p.U0[i]), c.at(p.up_w[1]), c.fat(p.up_b[1]), c.at(p.U1[i]), n, 2 * h, 2 * w));
    CK(last0_forward(c, p, i, p.sb ? c.at(p.SBC0[i]) : nullptr));
    {
        ConvArgs a = conv_args(n, S * h, S * w, c.C);   // conv_last.2 + bilinear xS skip (basicvsr.py:21-22,82)
        a.src_nstride[0] = pm_image_elems(S * h, S * w, 64);
        a.src[0] = c.at(p.C0[i]); a.wpack = c.at(p.last2_w); a.bias = c.fat(p.last2_b); a.cout_real = 3;
        a.dst[0] = sr + (size_t)i * 3 * S * S * h * w; a.dst_nstride = (long long)p.t * 3 * S * S * h * w;
        a.base_lr = lrs + (size_t)i * 3 * h * w; a.base_nstride = (long long)p.t * 3 * h * w; a.base_h = h; a.base_w = w; a.base_scale = S;
        CK(vsr_launch_conv(c.dtype, 3, 1, 64, 64, 0, 32, EPI_PLANAR, a, c.st));
    }
    return VSR_OK;
}

const float* flow_ptr(const Ctx& c, const Plan& p, int forward, int i) {   // flow of pair i, batch stride (t-1)*2*h*w
    return c.fat(p.flows) + ((size_t)forward * p.n * (p.t - 1) + i) * 2 * p.h * p.w;
}

// The two propagation directions are independent until the fusion conv (basicvsr.py:46-77), so their
// chains of 61 dependent launches per frame run on two streams: each stream's launch gap and pipeline
// fill is covered by the other's kernels.  The helper stream is forked from and joined to the caller's
// stream with events, so for the caller all work is still ordered in the stream it passed.
struct Helper { hipStream_t s = nullptr; hipEvent_t fork = nullptr, join = nullptr; int dev = -1; };
int get_helper(Helper** out) {
    thread_local Helper hp[16];
    int dev = 0;
    HIP_CHECK_RET(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return VSR_ERR_UNSUPPORTED;
    Helper& x = hp[dev];
    if (!x.s) {
        HIP_CHECK_RET(hipStreamCreateWithFlags(&x.s, hipStreamNonBlocking));
        HIP_CHECK_RET(hipEventCreateWithFlags(&x.fork, hipEventDisableTiming));
        HIP_CHECK_RET(hipEventCreateWithFlags(&x.join, hipEventDisableTiming));
        x.dev = dev;
    }
    *out = &x;
    return VSR_OK;
}
bool single_stream() { return vsr_env().single_stream; }
struct Fork {   // RAII: the join is enqueued on every exit path
    hipStream_t main; Helper* h; bool active = false;
    int begin(bool fork = true) {
        if (single_stream() || !fork) return VSR_OK;
        CK(get_helper(&h));
        HIP_CHECK_RET(hipEventRecord(h->fork, main));
        HIP_CHECK_RET(hipStreamWaitEvent(h->s, h->fork, 0));
        active = true;
        return VSR_OK;
    }
    hipStream_t side() const { return active ? h->s : main; }
    int end() {
        if (!active) return VSR_OK;
        active = false;
        HIP_CHECK_RET(hipEventRecord(h->join, h->s));
        HIP_CHECK_RET(hipStreamWaitEvent(main, h->join, 0));
        return VSR_OK;
    }
    ~Fork() { (void)end(); }
};

int forward_chain(const Ctx& c, const Plan& p, int dir, const float* lrs) {
    const int n = p.n, t = p.t, h = p.h, w = p.w;
    const long long fstride = (long long)(t - 1) * 2 * h * w;
    for (int k = 0; k < t; ++k) {
        // dir 0: backward-time propagation, frames t-1 .. 0 (basicvsr.py:46-60); dir 1: forward-time (basicvsr.py:62-73)
        const int i = dir == 0 ? t - 1 - k : k;
        void* warped = nullptr;
        if (k > 0) {
            const int prev = dir == 0 ? i + 1 : i - 1;
            warped = p.bwd ? c.at(p.Wp[dir][i]) : c.at(p.scratchW[dir]);
            CK(vsr_launch_warp_fwd(c.dtype, c.at(p.feat[dir][prev]), flow_ptr(c, p, dir, dir == 0 ? i : i - 1), warped, n, h, w, p.C, fstride, c.st));
        }
        CK(trunk_forward(c, p, dir, i, warped, lrs));
    }
    return VSR_OK;
}

int forward_impl(const Plan& p, const float* const* prm, const float* lrs, float* sr, char* ws, hipStream_t st) {
    const Ctx c = engine_ctx(p, ws, st, 0);
    const PIdx ix{p.rb, p.ups};
    const int n = p.n, t = p.t;
    CK(pack_all(c, p, prm));
    if (t > 1) CK(vsr::spynet_run(c, p.spy, lrs, prm[ix.spy_mean()], prm[ix.spy_std()], n, t, 0, (float*)c.at(p.flows)));
    {
        Fork f{st, nullptr};
        // (chain launches spin on each other's tiles: two of them side by side could each hold the CUs the other's unstarted
        // workgroups need -- conv3x3_chain.hip, "Work distribution" -- so with the chains on, both directions share the caller's stream)
        CK(f.begin(!chain_on(p)));
        const Ctx c0 = engine_ctx(p, ws, st, 0), c1 = engine_ctx(p, ws, f.side(), 1);
        CK(forward_chain(c0, p, 0, lrs));
        CK(forward_chain(c1, p, 1, lrs));
        CK(f.end());
    }
    for (int i = 0; i < t; ++i) CK(recon_forward(c, p, i, lrs, sr));      // fusion + upsampling (basicvsr.py:75-82)
    return VSR_OK;
}

// ---- backward ------------------------------------------------------------------------------------
// Weight gradients of PixelShufflePack k (upsample.k, upsampling.py:7) for the frames [f0, f1): one launch per pixel-shuffle phase z,
// X = the layer's input, dY = phase z of the gradient into it (a contiguous plane when p.unsh, else every second pixel of every second row)
int recon_ps_wgrads(const Ctx& c, const Plan& p, int k, int f0, int f1, float* const* g) {
    const PIdx ix{p.rb, p.ups};
    const int H = (k + 1) * p.h, W = (k + 1) * p.w;              // the layer's input size: h x w (k = 0), 2h x 2w (k = 1)
    for (int i0 = f0; i0 < f1; i0 += VSR_WG_MAXSEG) {
        const int i1 = i0 + VSR_WG_MAXSEG < f1 ? i0 + VSR_WG_MAXSEG : f1;
        const void* x[VSR_WG_MAXSEG];
        const void* dy[VSR_WG_MAXSEG];
        for (int i = i0; i < i1; ++i) { x[i - i0] = c.at(k == 1 ? p.U0[i] : p.Pt[i]); dy[i - i0] = c.at(k == 1 ? p.GU1f[i] : p.GU0f[i]); }
        CK(c.ps_wgrads(x, dy, i1 - i0, p.unsh, p.n, H, W, g[ix.up_w(k)], g[ix.up_b(k)], 1));
    }
    return VSR_OK;
}
// ... and of the 1x1 fuse conv on cat([outputs[i], feat_prop]) (basicvsr.py:18,75-77): one launch per 64-channel half of its input
int recon_point_wgrads(const Ctx& c, const Plan& p, int f0, int f1, float* const* g) {
    const PIdx ix{p.rb, p.ups};
    const int C = p.C;
    for (int i0 = f0; i0 < f1; i0 += VSR_WG_MAXSEG) {
        const int i1 = i0 + VSR_WG_MAXSEG < f1 ? i0 + VSR_WG_MAXSEG : f1;
        for (int s = 0; s < 2; ++s) {
            WgradArgs a = wg_base(p.n, p.h, p.w, C, C);
            a.nseg = 0;
            for (int i = i0; i < i1; ++i) { a.x[a.nseg] = c.at(p.feat[s][i]); a.dy[a.nseg] = c.at(p.GPf[i]); ++a.nseg; }
            CK(c.wgrad_cc(1, a, g[ix.point_w()], 2 * C, s * C, s == 0 ? g[ix.point_b()] : nullptr, 1));
        }
    }
    return VSR_OK;
}

int recon_backward(const Ctx& c, const Plan& p, int i, const float* lrs, const float* dsr, float* const* g, const float* last2_w) {
    const PIdx ix{p.rb, p.ups};
    if (p.diet) {   // U0, U1 and C0 of this frame were not kept: the forward's three launches again (the sign bits of C0 were)
        CK(c.conv_ps(c.at(p.Pt[i]), c.at(p.up_w[0]), c.fat(p.up_b[0]), c.at(p.U0[i]), p.n, p.h, p.w));
        if (p.ups == 2) CK(c.conv_ps(c.at(p.U0[i]), c.at(p.up_w[1]), c.fat(p.up_b[1]), c.at(p.U1[i]), p.n, 2 * p.h, 2 * p.w));
        CK(last0_forward(c, p, i, nullptr));
    }
    const int C = p.C;
    const int n = p.n, h = p.h, w = p.w, H4 = p.scale * h, W4 = p.scale * w;      // (the output size: 4h x 4w, or 2h x 2w for upscale 2)
    const float* dsr_i = dsr + (size_t)i * 3 * H4 * W4;
    const long long dsr_ns = (long long)p.t * 3 * H4 * W4;
    if (c.dtype == VSR_BF16 && last2_w) {   // d(conv_last.0 pre-activation) = dgrad(conv_last.2)(dsr) * LeakyReLU'(C0): hr_tail.hip
        CK(vsr_launch_last2_dgrad(dsr_i, dsr_ns, last2_w, c.at(p.C0[i]), c.at(p.G_C0), n, H4, W4, MASK_LEAKY, c.st, p.sb ? c.at(p.SBC0[i]) : nullptr));
    } else {
        ConvArgs a = conv_args(n, H4, W4, c.C);
        a.src[0] = dsr_i; a.src_nstride[0] = dsr_ns; a.wpack = c.at(p.last2_wd); a.dst[0] = c.at(p.G_C0);
        a.aux[0] = c.at(p.C0[i]); a.mask_mode = MASK_LEAKY;
        a.CD = 64; a.cout_real = 64; a.dst_nstride = pm_image_elems(H4, W4, 64);
        CK(vsr_launch_conv(c.dtype, 3, 1, 16, 16, 1, 64, EPI_NHWC, a, c.st));
    }
    {   // conv_last.2: X = C0, dY = dsr (planar)
        WgradArgs a = wg_base(n, H4, W4, 64, 64);
        a.x[0] = c.at(p.C0[i]); a.dy[0] = dsr_i; a.dy_nstride = dsr_ns;
        CK(c.wgrad(a, {3, 64, false, 16, true}, {3, 64, g[ix.last2_w()], 64, 0, 1, 0, g[ix.last2_b()], 1}));
    }
    // (r04: G_U1 / G_U0, the gradients into the pixel-shuffle layers, are written phase-separated when p.unsh)
    const size_t gu1 = p.GU1f[i], gu0 = p.GU0f[i], gp = p.GPf[i];     // (per frame when p.hrdef: their weight gradients run later, all frames per launch)
    if (C == 64) {
        CK(c.conv(3, c.at(p.G_C0), c.at(p.last0_wd), nullptr, c.at(gu1), ACT_NONE, nullptr, nullptr, 0, n, H4, W4, nullptr, nullptr, p.unsh));
    } else {    // conv_last.0's data gradient 64 -> C
        ConvArgs a = conv_args(n, H4, W4, c.C);
        a.src[0] = c.at(p.G_C0); a.src_nstride[0] = pm_image_elems(H4, W4, 64); a.wpack = c.at(p.last0_wd); a.dst[0] = c.at(gu1);
        CK(vsr_launch_conv(c.dtype, 3, 1, 64, 64, 0, p.CO, EPI_NHWC, a, c.st));
    }
    {   // conv_last.0: X = U1, dY = G_C0
        WgradArgs a = wg_base(n, H4, W4, C, 64);
        a.x[0] = c.at(p.U1[i]); a.dy[0] = c.at(p.G_C0);
        CK(c.wgrad(a, {3, C, false, 64, false}, {64, C, g[ix.last0_w()], C, 0, 1, 0, g[ix.last0_b()], 1}));
    }
    // upsample.1 (at 2h x 2w; upscale 4 only -- for upscale 2 G_U1 IS G_U0): dgrad, then wgrad per pixel-shuffle phase z
    if (p.ups == 2) {
        CK(c.conv_ps_dgrad(c.at(gu1), c.at(p.up_wd[1]), c.at(gu0), nullptr, 0, n, 2 * h, 2 * w, nullptr, p.unsh, p.unsh));
        if (!p.hrdef) CK(recon_ps_wgrads(c, p, 1, i, i + 1, g));
    }
    // upsample.0 (at h x w): its input is LeakyReLU(point_conv) => mask with P
    CK(c.conv_ps_dgrad(c.at(gu0), c.at(p.up_wd[0]), c.at(gp), c.at(p.Pt[i]), MASK_LEAKY, n, h, w, p.sb ? c.at(p.SBPt[i]) : nullptr, p.unsh, false));
    if (!p.hrdef) CK(recon_ps_wgrads(c, p, 0, i, i + 1, g));
    // point_conv dgrad: two C-channel outputs (d outputs[i], d feat_prop)
    CK(c.point_dgrad(c.at(gp), c.at(p.point_wd), c.at(p.dFeatB[i]), c.at(p.dFF[i]), n, h, w));
    if (!p.hrdef) CK(recon_point_wgrads(c, p, i, i + 1, g));
    return VSR_OK;
}

// BPTT through one ResidualBlock call; top gradient = dtop (T) + S (fp32 scatter, optional)
// pending_flow: the flow of the warp whose output gradient sits in dWp[dir] (from the previous frame of the chain), or null:
// the top gradient of this frame is dtop + warp^T(dWp) -- gather form, fused with the cast (elementwise.hip)
int stem_wgrads(const Ctx& c, const Plan& p, int dir, int f0, int f1, const float* lrs, float* const* g);
int block_wgrads(const Ctx& c, const Plan& p, int dir, int b, int f0, int f1, float* const* g);
// diet (Plan::diet): the frame's weight gradients are launched here, block by block behind the data gradients (one frame per
// launch, accumulated into g), because the activation gradients are not kept for backward_chain's all-frames launches
int trunk_backward(const Ctx& c, const Plan& p, int dir, int i, const void* dtop, const float* pending_flow, int pending_k, bool has_warp,
                   const float* lrs, float* const* g) {
    const int n = p.n, h = p.h, w = p.w, rb = p.rb;
    if (pending_flow) {
        const long long fstride = (long long)(p.t - 1) * 2 * h * w;
        CK(vsr_launch_warp_bwd_gather(c.dtype, c.at(p.dWp[dir]), pending_flow, dtop, (long long*)c.at(p.S[dir]),
                                      (int*)c.at(p.far_cnt) + dir * 32 + pending_k, c.at(p.dxoff(dir, i, rb)), n, h, w, p.C, fstride, c.st));
    } else {
        CK(vsr_launch_add_cast(c.dtype, dtop, nullptr, c.at(p.dxoff(dir, i, rb)), n, h, w, p.C, c.st));
    }
    const bool chain = chain_on(p) && !p.diet;            // diet: the activation gradients live in a two-block ring, the frame's weight
    if (chain) CK(trunk_chain_backward(c, p, dir, i));     // gradients are launched block by block behind them (the forward chain stays)
    for (int b = chain ? 0 : rb - 1; b >= 0; --b) {
        const void* dxn = c.at(p.dxoff(dir, i, b + 1));
        // dA = dgrad(conv2)(dX_{b+1}) * ReLU'(A_b)
        if (!chain) CK(c.conv(3, dxn, c.at(p.blk_wd[dir][2 * b + 1]), nullptr, c.at(p.g1off(dir, i, b)), ACT_NONE, nullptr, c.at(p.aoff(dir, i, b)), MASK_RELU, n, h, w,
                    nullptr, p.sb ? c.at(p.sboff(dir, i, b)) : nullptr));
        // dX_b = dX_{b+1} + dgrad(conv1)(dA); for b == 0 also through the stem's LeakyReLU
        void* out = b > 0 ? c.at(p.dxoff(dir, i, b)) : c.at(p.G0[dir][i]);
        CK(c.conv(3, c.at(p.g1off(dir, i, b)), c.at(p.blk_wd[dir][2 * b]), nullptr, out, ACT_NONE, dxn, b == 0 ? c.at(p.xoff(dir, i, 0)) : nullptr,
                    b == 0 ? MASK_LEAKY : 0, n, h, w, nullptr, (b == 0 && p.sb) ? c.at(p.SBX0[dir][i]) : nullptr));
        if (p.diet) CK(block_wgrads(c, p, dir, b, i, i + 1, g));
    }
    if (has_warp)   // gradient w.r.t. the warped state (feat part of the stem's input)
        CK(c.conv(3, c.at(p.G0[dir][i]), c.at(p.stem_wd[dir]), nullptr, c.at(p.dWp[dir]), ACT_NONE, nullptr, nullptr, 0, n, h, w));
    if (p.diet) CK(stem_wgrads(c, p, dir, i, i + 1, lrs, g));
    return VSR_OK;
}

// Weight gradients of one direction's trunk for the frames [f0, f1) (at most VSR_WG_MAXSEG per launch): the stem ...
int stem_wgrads(const Ctx& c, const Plan& p, int dir, int f0, int f1, const float* lrs, float* const* g) {
    const PIdx ix{p.rb, p.ups};
    const int n = p.n, t = p.t, h = p.h, w = p.w, C = p.C;
    WgradArgs a = wg_base(n, h, w, C, C), af = a;      // LR part (+ bias); feat part: only frames that had a warped state
    a.nseg = af.nseg = 0;
    a.x_nstride = (long long)t * 3 * h * w;
    for (int i = f0; i < f1; ++i) {
        a.x[a.nseg] = lrs + (size_t)i * 3 * h * w; a.dy[a.nseg] = c.at(p.G0[dir][i]); ++a.nseg;
        const bool has = dir == 0 ? (i < t - 1) : (i > 0);
        if (has) { af.x[af.nseg] = c.at(p.Wp[dir][i]); af.dy[af.nseg] = c.at(p.G0[dir][i]); ++af.nseg; }
    }
    return c.stem_wgrads(true, a, af, g[ix.stem_w(dir)], g[ix.stem_b(dir)], 1);
}
// ... and the two convs of ResidualConv block b
int block_wgrads(const Ctx& c, const Plan& p, int dir, int b, int f0, int f1, float* const* g) {
    const PIdx ix{p.rb, p.ups};
    const int C = p.C;
    WgradArgs a1 = wg_base(p.n, p.h, p.w, C, C), a2 = wg_base(p.n, p.h, p.w, C, C);
    a1.nseg = a2.nseg = 0;
    for (int i = f0; i < f1; ++i) {
        a1.x[a1.nseg] = c.at(p.xoff(dir, i, b)); a1.dy[a1.nseg] = c.at(p.g1off(dir, i, b)); ++a1.nseg;
        a2.x[a2.nseg] = c.at(p.aoff(dir, i, b)); a2.dy[a2.nseg] = c.at(p.dxoff(dir, i, b + 1)); ++a2.nseg;
    }
    CK(c.wgrad_cc(3, a1, g[ix.blk_w(dir, 2 * b)], C, 0, g[ix.blk_b(dir, 2 * b)], 1));
    CK(c.wgrad_cc(3, a2, g[ix.blk_w(dir, 2 * b + 1)], C, 0, g[ix.blk_b(dir, 2 * b + 1)], 1));
    return VSR_OK;
}
int trunk_wgrads(const Ctx& c, const Plan& p, int dir, const float* lrs, float* const* g) {
    for (int i0 = 0; i0 < p.t; i0 += VSR_WG_MAXSEG) {
        const int i1 = i0 + VSR_WG_MAXSEG < p.t ? i0 + VSR_WG_MAXSEG : p.t;
        CK(stem_wgrads(c, p, dir, i0, i1, lrs, g));
        for (int b = 0; b < p.rb; ++b) CK(block_wgrads(c, p, dir, b, i0, i1, g));
    }
    return VSR_OK;
}

// BPTT through one direction's chain, then that direction's weight gradients (all frames per launch)
int backward_chain(const Ctx& c, const Plan& p, int dir, const float* lrs, float* const* g) {
    const int n = p.n, t = p.t, h = p.h, w = p.w;
    const long long fstride = (long long)(t - 1) * 2 * h * w;
    // the gather-form warp backward keeps S all-zero between uses: ONE memset per chain (was one per frame)
    HIP_CHECK_RET(hipMemsetAsync(c.at(p.S[dir]), 0, p.s_elems * 8, c.st));
    HIP_CHECK_RET(hipMemsetAsync((int*)c.at(p.far_cnt) + dir * 32, 0, 32 * 4, c.st));
    const float* pending = nullptr;
    for (int k = 0; k < t; ++k) {
        // the state of dir 1 flows 0 -> t-1, so its gradient flows t-1 -> 0; dir 0 the other way round
        const int i = dir == 1 ? t - 1 - k : k;
        const void* dtop = dir == 1 ? c.at(p.dFF[i]) : c.at(p.dFeatB[i]);
        const bool last = k == t - 1;                     // the chain's first frame had no warped state
        CK(trunk_backward(c, p, dir, i, dtop, pending, k, !last, lrs, g));
        pending = nullptr;
        if (!last) {   // feat(i) = trunk(warp(feat(prev), flow)): the gradient of the warped state goes back through the warp
            pending = flow_ptr(c, p, dir, dir == 1 ? i - 1 : i);     // ... at the top of the next frame's trunk_backward
            if (p.flowgrad) {   // the same warp's gradient w.r.t. its flow (each flow is used by exactly one warp)
                const int prev = dir == 1 ? i - 1 : i + 1, fi = dir == 1 ? i - 1 : i;
                float* df = (float*)c.at(p.dflows) + ((size_t)dir * p.n * (p.t - 1) + fi) * 2 * p.h * p.w;
                CK(vsr_launch_warp_bwd_flow(c.dtype, c.at(p.feat[dir][prev]), c.at(p.dWp[dir]), flow_ptr(c, p, dir, fi), df, n, h, w, p.C, fstride, c.st));
            }
        }
    }
    return p.diet ? VSR_OK : trunk_wgrads(c, p, dir, lrs, g);
}

int backward_impl(const Plan& p, const float* const* prm, float* const* g, const float* lrs, const float* dsr, float* dlrs,
                  char* ws, hipStream_t st) {
    const Ctx c = engine_ctx(p, ws, st, 0);
    // input gradient, part 1: the bilinear x4 skip (basicvsr.py:22,82) -- overwrites dlrs, everything else accumulates
    if (dlrs) CK(vsr_launch_bilinear4_bwd(dsr, dlrs, (long long)p.n * p.t * 3, p.h, p.w, st, p.scale));
    for (int i = p.t - 1; i >= 0; --i) CK(recon_backward(c, p, i, lrs, dsr, g, prm ? prm[PIdx{p.rb, p.ups}.last2_w()] : nullptr));   // -> dFeatB[i], dFF[i]
    if (p.hrdef) {            // the weight gradients recon_backward left out: all frames per launch
        if (p.ups == 2) CK(recon_ps_wgrads(c, p, 1, 0, p.t, g));
        CK(recon_ps_wgrads(c, p, 0, 0, p.t, g));
        CK(recon_point_wgrads(c, p, 0, p.t, g));
    }
    Fork f{st, nullptr};
    // One stream: the two directions share their activation-gradient buffers (Plan::build), and chain launches of two streams could
    // each hold the CUs the other's unstarted workgroups need (conv3x3_chain.hip).  diet: rings per direction, no chains: two streams.
    CK(f.begin(p.diet));
    const Ctx c0 = engine_ctx(p, ws, st, 0), c1 = engine_ctx(p, ws, f.side(), 1);
    CK(backward_chain(c0, p, 1, lrs, g));
    CK(backward_chain(c1, p, 0, lrs, g));
    CK(f.end());
    if (dlrs) {   // part 2: the stems' LR channels (conv.py:97 on cat([lr_i, feat])), both directions, every frame
        for (int dir = 0; dir < 2; ++dir)
            for (int i = 0; i < p.t; ++i) {
                float* d = dlrs + (size_t)i * 3 * p.h * p.w;
                CK(c.conv_planar3(c.at(p.G0[dir][i]), c.at(p.stem_wd_lr[dir]), nullptr, d, (long long)p.t * 3 * p.h * p.w, d, p.n, p.h, p.w));
            }
    }
    if (p.flowgrad && p.t > 1)   // part 3 (and train_flow): through the flows into SPyNet's parameters / image pyramid
        CK(vsr::spynet_backward(c, p.spy, c.fat(p.dflows), p.n, p.t, 0, g, PIdx{p.rb, p.ups}.spy_base(), dlrs, prm[PIdx{p.rb, p.ups}.spy_std()]));
    return VSR_OK;
}

}  // namespace

// ================================ C ABI =========================================================
extern "C" {

int vsr_abi_version(void) { return 4; }

const char* vsr_status_string(int s) {
    switch (s) {
        case VSR_OK: return "ok";
        case VSR_ERR_BADARG: return "bad argument";
        case VSR_ERR_UNSUPPORTED: return "unsupported shape/configuration for the HIP path";
        case VSR_ERR_HIP: return "HIP runtime error";
        case VSR_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown status";
    }
}

int vsr_basicvsr_num_params(const VsrBasicVSRDesc* d) {
    if (!d || d->res_blocks < 0) return VSR_ERR_BADARG;
    return PIdx{d->res_blocks, d->upscale == 2 ? 1 : 2}.count();
}

}  // extern "C"

// The whole-path entries (mid_channels 64) and the narrow ones (16 / 32) differ only in the widths their Plan accepts.
namespace {
size_t basicvsr_workspace_bytes(const VsrBasicVSRDesc* d, int need_backward, bool narrow) {
    if (!d) return 0;
    Plan p;
    if (p.build(*d, need_backward, narrow) != VSR_OK) return 0;
    return p.total;
}

int basicvsr_forward(const VsrBasicVSRDesc* d, const float* const* params, int nparams, const float* lrs, float* sr,
                     void* workspace, size_t workspace_bytes, int need_backward, void* stream, bool narrow) {
    if (!d || !params || !lrs || !sr || !workspace) return VSR_ERR_BADARG;
    Plan p;
    CK(p.build(*d, need_backward, narrow));
    if (nparams != PIdx{p.rb, p.ups}.count()) return VSR_ERR_BADARG;
    for (int k = 0; k < nparams; ++k) if (!params[k]) return VSR_ERR_BADARG;
    if (workspace_bytes < p.total) return VSR_ERR_WORKSPACE;
    return forward_impl(p, params, lrs, sr, (char*)workspace, (hipStream_t)stream);
}

int basicvsr_backward(const VsrBasicVSRDesc* d, const float* const* params, float* const* grads, int nparams,
                      const float* lrs, const float* dsr, float* dlrs, void* workspace, size_t workspace_bytes, void* stream, bool narrow) {
    if (!d || !params || !grads || !lrs || !dsr || !workspace) return VSR_ERR_BADARG;
    if (d->res_blocks < 1) return VSR_ERR_UNSUPPORTED;
    const PIdx ix{d->res_blocks, d->upscale == 2 ? 1 : 2};
    if (nparams != ix.count()) return VSR_ERR_BADARG;
    bool flow = dlrs != nullptr;                           // input or SPyNet gradient wanted => the forward ran with need_backward = 2
    for (int k = ix.spy_base(); k < ix.spy_mean(); ++k) flow = flow || grads[k];
    Plan p;
    CK(p.build(*d, flow ? 2 : 1, narrow));
    if (workspace_bytes < p.total) return VSR_ERR_WORKSPACE;
    return backward_impl(p, params, grads, lrs, dsr, dlrs, (char*)workspace, (hipStream_t)stream);
}

int basicvsr_get_flows(const VsrBasicVSRDesc* d, const void* workspace, float* flow_forward, float* flow_backward, void* stream, bool narrow) {
    if (!d || !workspace) return VSR_ERR_BADARG;
    Plan p;
    CK(p.build(*d, 0, narrow));         // weight/flow offsets do not depend on need_backward
    if (p.t < 2) return VSR_OK;
    const size_t half = (size_t)p.n * (p.t - 1) * 2 * p.h * p.w * 4;
    const char* f = (const char*)workspace + p.flows;
    if (flow_backward) HIP_CHECK_RET(hipMemcpyAsync(flow_backward, f, half, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (flow_forward) HIP_CHECK_RET(hipMemcpyAsync(flow_forward, f + half, half, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return VSR_OK;
}
}  // namespace

extern "C" {
size_t vsr_basicvsr_workspace_bytes(const VsrBasicVSRDesc* d, int need_backward) { return basicvsr_workspace_bytes(d, need_backward, false); }
int vsr_basicvsr_forward(const VsrBasicVSRDesc* d, const float* const* params, int nparams, const float* lrs, float* sr,
                         void* workspace, size_t workspace_bytes, int need_backward, void* stream) {
    return basicvsr_forward(d, params, nparams, lrs, sr, workspace, workspace_bytes, need_backward, stream, false);
}
int vsr_basicvsr_backward(const VsrBasicVSRDesc* d, const float* const* params, float* const* grads, int nparams,
                          const float* lrs, const float* dsr, float* dlrs, void* workspace, size_t workspace_bytes, void* stream) {
    return basicvsr_backward(d, params, grads, nparams, lrs, dsr, dlrs, workspace, workspace_bytes, stream, false);
}
int vsr_basicvsr_get_flows(const VsrBasicVSRDesc* d, const void* workspace, float* flow_forward, float* flow_backward, void* stream) {
    return basicvsr_get_flows(d, workspace, flow_forward, flow_backward, stream, false);
}
size_t vsr_basicvsr_narrow_workspace_bytes(const VsrBasicVSRDesc* d, int need_backward) { return basicvsr_workspace_bytes(d, need_backward, true); }
int vsr_basicvsr_narrow_forward(const VsrBasicVSRDesc* d, const float* const* params, int nparams, const float* lrs, float* sr,
                                void* workspace, size_t workspace_bytes, int need_backward, void* stream) {
    return basicvsr_forward(d, params, nparams, lrs, sr, workspace, workspace_bytes, need_backward, stream, true);
}
int vsr_basicvsr_narrow_backward(const VsrBasicVSRDesc* d, const float* const* params, float* const* grads, int nparams,
                                 const float* lrs, const float* dsr, float* dlrs, void* workspace, size_t workspace_bytes, void* stream) {
    return basicvsr_backward(d, params, grads, nparams, lrs, dsr, dlrs, workspace, workspace_bytes, stream, true);
}
int vsr_basicvsr_narrow_get_flows(const VsrBasicVSRDesc* d, const void* workspace, float* flow_forward, float* flow_backward, void* stream) {
    return basicvsr_get_flows(d, workspace, flow_forward, flow_backward, stream, true);
}

}  // extern "C"
