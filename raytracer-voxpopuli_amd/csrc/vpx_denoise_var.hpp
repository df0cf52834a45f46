// vpx_denoise_var.hpp — the variance-guided a-trous filter (vpx_denoise_var, vpx_denoise_var_host):
// host + device.
//
// vpx_denoise_ids' filter with one change: the luminance weight's tolerance is local.  The edge
// test stays the integer plane key (vpx_denoise.hpp); the soft weight h / (1 + dd * dd) divides the
// luminance difference by sigma_v standard deviations of the pixel's own luminance, estimated from
// the moments vpx_reproject_moments carries (or, where the history is short, from the 5x5
// neighbourhood on the pixel's plane) and filtered along with the colour.  The variance rides in
// the image's fourth channel through the passes: one 16-byte load per tap, as vpx_denoise_ids.
// A tap that does not match is never read into the arithmetic.  Every operation rounds once to
// float32, products before sums, nothing contracted, so the host loops and the kernels
// (k_var_estimate, k_atrous_var_lds, k_atrous_var_gather in vpx_kernels.hip) give the same bits.
// include/vpx.h holds the definition.
#pragma once

#include <stdint.h>
#if !defined(__HIPCC__)
#include <cmath>
#endif

#include "../../include/vpx.h"
#include "vpx_denoise.hpp"

// No fused multiply-add in this file whatever the command line says (as vpx_denoise.hpp).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vpx {
namespace denoise_var {

using denoise::Key;

struct Mom {  // one float2 of a moments image: the history's mean luminance and mean squared luminance
    float x, y;
};

VPX_DENOISE_HD float sqrt_exact(float v) {  // correctly rounded on both sides
#if defined(__HIPCC__)
    return sqrtf(v);
#else
    return std::sqrt(v);
#endif
}

// ---- step V
// The moments of a pixel without a moments image: its own luminance.
VPX_DENOISE_HD Mom self_moments(float cx, float cy, float cz) {
    const float l = denoise::lum(cx, cy, cz);
    return Mom{l, l * l};
}
VPX_DENOISE_HD float clamp_var(float v) { return v > 0.0f ? v : 0.0f; }  // a NaN gives 0
VPX_DENOISE_HD float temporal_var(Mom m) { return clamp_var(m.y - m.x * m.x); }
struct Spatial {
    float s1 = 0.f, s2 = 0.f, cnt = 0.f;
};
VPX_DENOISE_HD void spatial_tap(Spatial& s, Mom m) {
    s.s1 = s.s1 + m.x;
    s.s2 = s.s2 + m.y;
    s.cnt = s.cnt + 1.0f;
}
VPX_DENOISE_HD float spatial_var(const Spatial& s) {  // cnt >= 1: the centre matches
    const float mean = s.s1 / s.cnt;
    return clamp_var(s.s2 / s.cnt - mean * mean);
}

// ---- a pass
// G[|j|] * G[|i|], G = {0.5, 0.25}: the 3x3 prefilter of the variance (weight only).
VPX_DENOISE_HD float pre_weight(int j, int i) { return ((j == 0) ? 0.5f : 0.25f) * ((i == 0) ? 0.5f : 0.25f); }
struct Pre {
    float gs = 0.f, gw = 0.f;
};
VPX_DENOISE_HD void pre_tap(Pre& p, float g, float var) {
    p.gs = p.gs + g * var;
    p.gw = p.gw + g;
}
// 1 / tolerance: gw >= 1/4 (the centre matches).
VPX_DENOISE_HD float inv_tolerance(const Pre& p, float sigma_v, float epsilon) {
    const float gv = p.gs / p.gw;
    const float tol = sigma_v * sqrt_exact(gv) + epsilon;
    return 1.0f / tol;
}

struct Sum {
    float r = 0.f, g = 0.f, b = 0.f, w = 0.f, v = 0.f;
};
// One matching tap of colour (cx, cy, cz), variance cv and base weight h; lq: the centre's luminance.
VPX_DENOISE_HD void tap(Sum& s, float h, float cx, float cy, float cz, float cv, float lq, float inv) {
    const float dd = (denoise::lum(cx, cy, cz) - lq) * inv;
    const float w = h / (1.0f + dd * dd);
    s.r = s.r + w * cx;
    s.g = s.g + w * cy;
    s.b = s.b + w * cz;
    s.w = s.w + w;
    s.v = s.v + (w * w) * cv;
}
VPX_DENOISE_HD float out_var(const Sum& s) { return s.v / (s.w * s.w); }

// NULL, or why the call is refused (vpx.h: VPX_E_INVALID).
inline const char* check_call(uint32_t width, uint32_t height, const void* ids, const void* in, const void* mom,
                              const void* out, const vpx_denoise_var_params* d) {
    if (!ids || !in || !out || !d) return "null argument";
    if (width == 0 || height == 0 || width > denoise::kMaxSide || height > denoise::kMaxSide) return "frame size out of range";
    if ((uint64_t)((width + 15u) / 16u) * ((height + 15u) / 16u) * 256u > denoise::kMaxTilePixels)
        return "frame larger than 2^27 tile-padded pixels";
    if (d->passes < 1u || d->passes > denoise::kMaxPasses) return "vpx_denoise_var_params.passes outside 1..5";
    if (!(d->sigma_v > 0.0f) || d->sigma_v > 3.402823466e38f) return "vpx_denoise_var_params.sigma_v must be finite and positive";
    if (!(d->epsilon > 0.0f) || d->epsilon > 3.402823466e38f) return "vpx_denoise_var_params.epsilon must be finite and positive";
    if (!(d->min_history >= 1.0f && d->min_history <= 65536.0f) || d->min_history != (float)(uint32_t)d->min_history)
        return "vpx_denoise_var_params.min_history must be an integer in 1..65536";
    if (d->flags != 0u || d->reserved[0] != 0u || d->reserved[1] != 0u || d->reserved[2] != 0u)
        return "vpx_denoise_var_params.flags and reserved must be 0";
    if (out == in || out == ids || out == mom) return "out must not be in, ids or mom";
    return nullptr;
}

// ---------------------------------------------------------------------------- host path
// Step V: V0 = (in.rgb, var0).  mom: float2[W*H] or NULL.
inline void estimate_host(uint32_t W, uint32_t H, const Key* keys, const float* in, const float* mom, float min_history,
                          float* V0) {
    auto moments = [=](uint64_t r) {
        return mom ? Mom{mom[2 * r], mom[2 * r + 1]} : self_moments(in[4 * r], in[4 * r + 1], in[4 * r + 2]);
    };
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint64_t q = (uint64_t)y * W + x;
            const Key kq = keys[q];
            float var = 0.0f;
            if (denoise::valid(kq)) {
                if (mom && in[4 * q + 3] >= min_history) {
                    var = temporal_var(moments(q));
                } else {
                    Spatial s;
                    for (int j = -2; j <= 2; ++j)
                        for (int i = -2; i <= 2; ++i) {
                            const int64_t rx = (int64_t)x + i, ry = (int64_t)y + j;
                            if (rx < 0 || ry < 0 || rx >= (int64_t)W || ry >= (int64_t)H) continue;
                            const uint64_t r = (uint64_t)ry * W + (uint64_t)rx;
                            if (!denoise::same(keys[r], kq)) continue;
                            spatial_tap(s, moments(r));
                        }
                    var = spatial_var(s);
                }
            }
            V0[4 * q] = in[4 * q], V0[4 * q + 1] = in[4 * q + 1], V0[4 * q + 2] = in[4 * q + 2], V0[4 * q + 3] = var;
        }
}

// One pass over S (.w: the variance) into D; restore: NULL, or the image whose .w the last pass puts back.
inline void pass_host(uint32_t W, uint32_t H, const Key* keys, const float* S, float* D, int step, float sigma_v,
                      float epsilon, const float* restore) {
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint64_t q = (uint64_t)y * W + x;
            const Key kq = keys[q];
            const float* c = S + 4 * q;
            float* o = D + 4 * q;
            if (!denoise::valid(kq)) {
                o[0] = c[0], o[1] = c[1], o[2] = c[2], o[3] = restore ? restore[4 * q + 3] : c[3];
                continue;
            }
            Pre pre;
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i) {
                    const int64_t rx = (int64_t)x + i, ry = (int64_t)y + j;
                    if (rx < 0 || ry < 0 || rx >= (int64_t)W || ry >= (int64_t)H) continue;
                    const uint64_t r = (uint64_t)ry * W + (uint64_t)rx;
                    if (!denoise::same(keys[r], kq)) continue;
                    pre_tap(pre, pre_weight(j, i), S[4 * r + 3]);
                }
            const float inv = inv_tolerance(pre, sigma_v, epsilon);
            const float lq = denoise::lum(c[0], c[1], c[2]);
            Sum s;
            for (int j = -2; j <= 2; ++j)
                for (int i = -2; i <= 2; ++i) {
                    const int64_t rx = (int64_t)x + i * step, ry = (int64_t)y + j * step;
                    if (rx < 0 || ry < 0 || rx >= (int64_t)W || ry >= (int64_t)H) continue;
                    const uint64_t r = (uint64_t)ry * W + (uint64_t)rx;
                    if (!denoise::same(keys[r], kq)) continue;
                    tap(s, denoise::base_weight(j, i), S[4 * r], S[4 * r + 1], S[4 * r + 2], S[4 * r + 3], lq, inv);
                }
            o[0] = s.r / s.w, o[1] = s.g / s.w, o[2] = s.b / s.w;
            o[3] = restore ? restore[4 * q + 3] : out_var(s);
        }
}

// The whole call on host memory: a, b: float4[W*H] scratch images (b unused with one pass).
inline void run_host(uint32_t W, uint32_t H, const uint32_t* ids, const float* in, const float* mom, float* out,
                     uint32_t* rgb8, const vpx_denoise_var_params& d, Key* keys, float* a, float* b) {
    const uint64_t pixels = (uint64_t)W * H;
    denoise::keys_host(pixels, ids, keys);
    estimate_host(W, H, keys, in, mom, d.min_history, a);
    float* img[2] = {a, b};
    for (uint32_t p = 0; p < d.passes; ++p) {
        const bool last = p + 1 == d.passes;
        pass_host(W, H, keys, img[p & 1u], last ? out : img[(p + 1u) & 1u], 1 << p, d.sigma_v, d.epsilon,
                  last ? in : nullptr);
    }
    if (rgb8)
        for (uint64_t p = 0; p < pixels; ++p) rgb8[p] = denoise::tonemap_pack_host(out + 4 * p);
}

}  // namespace denoise_var
}  // namespace vpx
