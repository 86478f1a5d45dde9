// SPyNet (spynet.py:38-93) as the BasicVSR engine and the stand-alone entries share it: the arena plan and the three host functions
// of spynet_engine.hip.
#pragma once
#include "recipes.h"

struct SpyPlan {
    int P = 0, F = 0, h = 0, w = 0, hu = 0, wu = 0;
    size_t pyr[6] = {};          // planar fp32 normalised frames, level 0 = coarsest
    size_t x16 = 0, b32a = 0, b64 = 0, b32b = 0, b16 = 0;   // pixel-major T at the finest level size
    size_t flow_a = 0, flow_b = 0, flow_up = 0;     // planar fp32 [P][2][hu][wu]
    size_t wpack[6][NSPY] = {}, bias[6][NSPY] = {};
    // train_flow (need_backward = 2): per-level saved activations, dgrad weights and backward scratch
    bool save = false;
    size_t sx[6][NSPY] = {};                 // inputs of the 5 convs of each level: x16, b32a, b64, b32b, b16
    size_t sfup[6] = {}, sres[6] = {};            // planar fp32 flow_up and residue (= ReLU(conv5)) per level
    size_t wpackd[6][NSPY] = {};
    size_t gA = 0, gB = 0, dres = 0, dfa = 0, dfb = 0;
    size_t dpyr[6] = {};                     // gradient of the normalised pyramid (input-frame gradient)
    void plan_save(Bump& b, int dtype) {
        save = true;
        const size_t es = esize(dtype);
        for (int l = 0; l < 6; ++l) {
            const int hl = hu >> (5 - l), wl = wu >> (5 - l);
            for (int j = 0; j < NSPY; ++j) sx[l][j] = b.take((size_t)P * pm_image_elems(hl, wl, SPY_CIP[j]) * es);
            sfup[l] = b.take((size_t)P * 2 * hl * wl * 4);
            sres[l] = b.take((size_t)P * 2 * hl * wl * 4);
            for (int j = 0; j < NSPY; ++j) wpackd[l][j] = b.take((size_t)49 * 64 * 64 * es);
        }
        gA = b.take((size_t)P * pm_image_elems(hu, wu, 64) * es);
        gB = b.take((size_t)P * pm_image_elems(hu, wu, 64) * es);
        dres = b.take((size_t)P * pm_image_elems(hu, wu, 16) * es);
        dfa = b.take((size_t)P * 2 * hu * wu * 4);
        dfb = b.take((size_t)P * 2 * hu * wu * 4);
        for (int l = 0; l < 6; ++l) dpyr[l] = b.take((size_t)F * 3 * (hu >> (5 - l)) * (wu >> (5 - l)) * 4);
    }
    void plan(Bump& b, int P_, int F_, int h_, int w_, int dtype) {
        P = P_; F = F_; h = h_; w = w_;
        wu = (w % 32) == 0 ? w : 32 * (w / 32 + 1);      // spynet.py:72-73
        hu = (h % 32) == 0 ? h : 32 * (h / 32 + 1);
        const size_t es = esize(dtype);
        for (int l = 0; l < 6; ++l) {
            const int s = 5 - l;
            pyr[l] = b.take((size_t)F * 3 * (hu >> s) * (wu >> s) * 4);
        }
        const size_t px = (size_t)P * hu * wu;
        auto pm = [&](int Cc) { return (size_t)P * pm_image_elems(hu, wu, Cc) * es; };     // blocked pixel-major tensors
        x16 = b.take(pm(16)); b32a = b.take(pm(32)); b64 = b.take(pm(64));
        b32b = b.take(pm(32)); b16 = b.take(pm(16));
        flow_a = b.take(px * 2 * 4); flow_b = b.take(px * 2 * 4); flow_up = b.take(px * 2 * 4);
        for (int l = 0; l < 6; ++l)
            for (int j = 0; j < NSPY; ++j) {
                wpack[l][j] = b.take((size_t)49 * SPY_COP[j] * SPY_CIP[j] * es);
                bias[l][j] = b.take(64 * 4);
            }
    }
};

namespace vsr {
// (documented at their definitions, spynet_engine.hip)
int spynet_pack(const Ctx& c, const SpyPlan& sp, const float* const* params, int base_idx);
int spynet_run(const Ctx& c, const SpyPlan& sp, const float* frames, const float* mean, const float* std, int n, int t,
               int pair_mode, float* flows_out, bool last_relu = true, float* const* level_out = nullptr);
int spynet_backward(const Ctx& c, const SpyPlan& sp, const float* dflows_out, int n, int t, int pair_mode, float* const* g,
                    int base_idx, float* dframes = nullptr, const float* std = nullptr, bool last_relu = true,
                    const float* const* dlevel = nullptr);
}  // namespace vsr
