// vpx_denoise.hpp — the plane-keyed a-trous filter (vpx_denoise_ids, vpx_denoise_host): host + device.
//
// A pixel's key is read from its vpx_render_ids record: the word that names volume, material and
// entry face, and the hit cell's coordinate along the face's axis.  Two pixels with equal keys lie
// on one flat surface of one material, so the filter's edge test is an integer equality and its
// base weights are dyadic.  One pass p (step s = 1 << p) averages, per valid pixel, the taps
// (x + i*s, y + j*s), j = -2..2 outer, i = -2..2 inner, that lie inside the image and carry the
// pixel's key, with weights H[|j|] * H[|i|], H = {3/8, 1/4, 1/16}, optionally divided by
// 1 + ((lum(tap) - lum(centre)) / sigma_l)^2.  A tap that does not match is never read into the
// arithmetic (no multiplication by a zero weight: a NaN on another surface stays there).  Every
// operation rounds once to float32, products before sums, nothing contracted, so the host loop
// and the kernels (k_plane_key, k_atrous_lds, k_atrous_gather in vpx_kernels.hip) give the same bits.
#pragma once

#include <stdint.h>

#include "../../include/vpx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VPX_DENOISE_HD __host__ __device__ __forceinline__
#else
#define VPX_DENOISE_HD inline
#endif

// No fused multiply-add in this file whatever the command line says (build() passes
// -ffp-contract=off as well; gcc on x86-64 has no fma to contract into without -mfma).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vpx {
namespace denoise {

constexpr uint32_t kMaxPasses = 5;   // steps 1, 2, 4, 8, 16
constexpr uint32_t kMaxSide = 32768; // vpx_frame_params' limit on width and height
constexpr uint64_t kMaxTilePixels = 1ull << 27;  // ... and on the 16x16-tile-padded pixel count

struct Key {
    uint32_t a, b;  // a: the ids' .y word; b: 0x80000000 | coord.  (0, 0): no plane
};

// The key of one vpx_render_ids record (.y, .z, .w; .x, the bits of t, is not read).  Nothing of
// the record is used as an index: any bit pattern has a key.
VPX_DENOISE_HD Key plane_key(uint32_t y, uint32_t z, uint32_t w) {
    const uint32_t v = y & 0xffffu, face = y >> 24;
    if (v < 2u || face < 1u || face > 6u) return Key{0u, 0u};
    const uint32_t axis = (face - 1u) >> 1;
    const uint32_t coord = axis == 0u ? (z & 0xffffu) : axis == 1u ? (z >> 16) : w;
    return Key{y, 0x80000000u | coord};
}
VPX_DENOISE_HD bool valid(Key k) { return k.b != 0u; }
VPX_DENOISE_HD bool same(Key p, Key q) { return p.a == q.a && p.b == q.b; }

// H[|j|] * H[|i|]: the nine products are exact.
VPX_DENOISE_HD float kernel_1d(int o) {
    const int a = o < 0 ? -o : o;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}
VPX_DENOISE_HD float base_weight(int j, int i) { return kernel_1d(j) * kernel_1d(i); }

// GetLuminance in the order tonemap_pack adds it.
VPX_DENOISE_HD float lum(float x, float y, float z) { return (x * 0.2126f + y * 0.7152f) + z * 0.0722f; }

struct Sum {
    float r = 0.f, g = 0.f, b = 0.f, w = 0.f;
};

// One matching tap of colour (cx, cy, cz) and base weight h; lq: the centre's luminance.
template <bool LUM>
VPX_DENOISE_HD void tap(Sum& s, float h, float cx, float cy, float cz, float lq, float inv_sigma) {
    float w = h;
    if (LUM) {
        const float d = (lum(cx, cy, cz) - lq) * inv_sigma;
        w = h / (1.0f + d * d);
    }
    s.r = s.r + w * cx;
    s.g = s.g + w * cy;
    s.b = s.b + w * cz;
    s.w = s.w + w;
}

// NULL, or why the call is refused (vpx.h: VPX_E_INVALID).
inline const char* check_call(uint32_t width, uint32_t height, const void* ids, const void* in, const void* out,
                              const vpx_denoise* d) {
    if (!ids || !in || !out || !d) return "null argument";
    if (width == 0 || height == 0 || width > kMaxSide || height > kMaxSide) return "frame size out of range";
    if ((uint64_t)((width + 15u) / 16u) * ((height + 15u) / 16u) * 256u > kMaxTilePixels)
        return "frame larger than 2^27 tile-padded pixels";
    if (d->passes < 1u || d->passes > kMaxPasses) return "vpx_denoise.passes outside 1..5";
    if (!(d->sigma_l >= 0.0f) || d->sigma_l > 3.402823466e38f) return "vpx_denoise.sigma_l must be 0 or finite and positive";
    if (d->flags != 0u || d->reserved != 0u) return "vpx_denoise.flags and reserved must be 0";
    if (out == in || out == ids) return "out must not be in or ids";
    return nullptr;
}

// ---------------------------------------------------------------------------- host path
inline void keys_host(uint64_t pixels, const uint32_t* ids, Key* keys) {
    for (uint64_t p = 0; p < pixels; ++p) keys[p] = plane_key(ids[4 * p + 1], ids[4 * p + 2], ids[4 * p + 3]);
}

template <bool LUM>
inline void pass_host(uint32_t W, uint32_t H, const Key* keys, const float* S, float* D, int step, float inv_sigma) {
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint64_t q = (uint64_t)y * W + x;
            const Key kq = keys[q];
            const float* c = S + 4 * q;
            float* o = D + 4 * q;
            if (!valid(kq)) {
                o[0] = c[0], o[1] = c[1], o[2] = c[2], o[3] = c[3];
                continue;
            }
            const float lq = LUM ? lum(c[0], c[1], c[2]) : 0.f;
            Sum s;
            for (int j = -2; j <= 2; ++j)
                for (int i = -2; i <= 2; ++i) {
                    const int64_t rx = (int64_t)x + i * step, ry = (int64_t)y + j * step;
                    if (rx < 0 || ry < 0 || rx >= (int64_t)W || ry >= (int64_t)H) continue;
                    const uint64_t r = (uint64_t)ry * W + (uint64_t)rx;
                    if (!same(keys[r], kq)) continue;
                    tap<LUM>(s, base_weight(j, i), S[4 * r], S[4 * r + 1], S[4 * r + 2], lq, inv_sigma);
                }
            o[0] = s.r / s.w, o[1] = s.g / s.w, o[2] = s.b / s.w, o[3] = c[3];
        }
}

// GetLuminance / ApplyReinhardJodie / RGBF32_to_RGB8 as the device's tonemap_pack
// (vpx_wavefront.hpp) computes them, for the host path's rgb8.
inline uint32_t tonemap_pack_host(const float* a) {
    const float l = lum(a[0], a[1], a[2]);
    uint32_t ch[3];
    for (int k = 0; k < 3; ++k) {
        const float rh = a[k] / (1.0f + a[k]);
        const float la = a[k] / (1.0f + l);
        const float o = la + rh * (rh - la);
        ch[k] = (uint32_t)(int64_t)(255.0f * (o < 1.0f ? o : 1.0f));
    }
    return (ch[0] << 16) + (ch[1] << 8) + ch[2];
}

// The whole call on host memory: a, b: float4[W*H] scratch images (unused with one pass).
inline void run_host(uint32_t W, uint32_t H, const uint32_t* ids, const float* in, float* out, uint32_t* rgb8,
                     const vpx_denoise& d, Key* keys, float* a, float* b) {
    const uint64_t pixels = (uint64_t)W * H;
    keys_host(pixels, ids, keys);
    const float inv_sigma = d.sigma_l > 0.0f ? 1.0f / d.sigma_l : 0.0f;
    const float* src = in;
    for (uint32_t p = 0; p < d.passes; ++p) {
        float* dst = p + 1 == d.passes ? out : (p & 1u) ? b : a;
        if (d.sigma_l > 0.0f)
            pass_host<true>(W, H, keys, src, dst, 1 << p, inv_sigma);
        else
            pass_host<false>(W, H, keys, src, dst, 1 << p, inv_sigma);
        src = dst;
    }
    if (rgb8)
        for (uint64_t p = 0; p < pixels; ++p) rgb8[p] = tonemap_pack_host(out + 4 * p);
}

}  // namespace denoise
}  // namespace vpx
