// vpx_reproject.hpp — the plane-keyed temporal reprojection (vpx_reproject_ids, vpx_reproject_ids_host):
// host + device.
//
// A moving camera's frame is one sample per pixel.  This pass carries the previous frame's history
// image over to the current camera: a pixel's hit point (its un-jittered ray at the ids' t) is
// projected into the previous camera, and the four history pixels around that position are blended
// in where their vpx_render_ids record names the same plane (vpx_denoise.hpp's key: volume,
// material, entry face, hit-cell coordinate along the face's axis).  The rejection test is that
// integer equality; there is no depth, normal or albedo threshold.  A tap that is not usable is
// never read into the arithmetic.  Every operation rounds once to float32, products before sums,
// nothing contracted, so the host loop and the kernel (k_reproject_ids in vpx_kernels.hip) give
// the same bits.  include/vpx.h holds the definition; pixel() below is it, for both.
#pragma once

#include <stdint.h>
// In a HIP translation unit the runtime header has declared the C library already; naming
// <string.h> here as well changes which memcpy an unrelated kernel of that unit compiles against.
#if !defined(__HIPCC__)
#include <string.h>

#include <cmath>
#endif

#include "../../include/vpx.h"
#include "vpx_denoise.hpp"

#if defined(__HIPCC__)
#define VPX_REPROJECT_HD __host__ __device__ __forceinline__
#else
#define VPX_REPROJECT_HD inline
#endif

// No fused multiply-add in this file whatever the command line says (as vpx_denoise.hpp).
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace vpx {
namespace reproject {

constexpr float kMaxHistory = 65536.0f;
constexpr uint32_t kMaxVolumes = 65534u;  // v = (.y & 0xffff) - 2 never reaches more
constexpr uint32_t kTabFloats = 24u;      // per volume: rows 0-2 of cur.inv_matrix, then of prev.matrix

struct V3 {
    float x, y, z;
};
struct Rgbw {  // one float4 of an image: a colour and, in a history image, the history length
    float r, g, b, w;
};
struct Id {  // one vpx_render_ids record
    uint32_t x, y, z, w;
};

// The call without its buffers, as the kernel takes it.
struct Args {
    vpx_camera cur;
    vpx_prev_camera prev;
    uint32_t width, height;
    float cap;  // max_history - 1: the longest history a tap may bring along
    uint32_t nohist_lo, nohist_hi;
    uint32_t n_volumes;
    uint32_t have_prev;  // ids_prev and hist_in are there
};

VPX_REPROJECT_HD V3 ld(const float* p) { return V3{p[0], p[1], p[2]}; }
VPX_REPROJECT_HD V3 sub(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
VPX_REPROJECT_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }  // left to right
VPX_REPROJECT_HD float rsqrt_exact(float v) {  // rsqrtf = 1 / sqrtf, both correctly rounded
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(1.0f, sqrtf(v));
#else
    return 1.0f / std::sqrt(v);
#endif
}

// Pixel (x, y)'s hit point: Camera::GetPrimaryRayNoDOF through Ray::Ray (camera.h:103-110,
// scene.cpp:83-93) in exact arithmetic, the bits of primary_ray() with kFlagReproject and
// make_ray() (vpx_wavefront.hpp, vpx_trace.hpp), then O + t * D.
VPX_REPROJECT_HD V3 hit_point(const vpx_camera& c, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float t) {
    const float u = (float)x * (1.0f / (float)W);
    const float v = (float)y * (1.0f / (float)H);
    const V3 tl = ld(c.top_left), tr = ld(c.top_right), bl = ld(c.bottom_left), o = ld(c.cam_pos);
    const V3 ex = sub(tr, tl), ey = sub(bl, tl);
    const V3 p = V3{(tl.x + ex.x * u) + ey.x * v, (tl.y + ex.y * u) + ey.y * v, (tl.z + ex.z * u) + ey.z * v};
    const V3 d = sub(p, o);
    const float inv = rsqrt_exact(dot(d, d));
    const V3 dn = V3{d.x * inv, d.y * inv, d.z * inv};
    return V3{o.x + t * dn.x, o.y + t * dn.y, o.z + t * dn.z};
}

// TransformPosition (tmpl8math.cpp:345-353) with rows 0-2 of a matrix: left-to-right sums.
VPX_REPROJECT_HD V3 transform_position(V3 a, const float* m) {
    return V3{m[0] * a.x + m[1] * a.y + m[2] * a.z + m[3] * 1.0f, m[4] * a.x + m[5] * a.y + m[6] * a.z + m[7] * 1.0f,
              m[8] * a.x + m[9] * a.y + m[10] * a.z + m[11] * 1.0f};
}

// Camera::PointToUV (camera.h:34-49) into the previous camera, then the bilinear footprint.
// false: no history (the point is not strictly inside the previous frustum: the reference has no
// such test; or a NaN position).  tlx, tly >= 0; tap k is (tlx + (k & 1), tly + (k >> 1)).
VPX_REPROJECT_HD bool footprint(const vpx_prev_camera& pc, V3 P, uint32_t W, uint32_t H, int& tlx, int& tly, float w[4]) {
    const V3 delta = sub(P, ld(pc.cam_pos));
    const float ldist = dot(ld(pc.left_normal), delta), rdist = dot(ld(pc.right_normal), delta);
    const float tdist = dot(ld(pc.top_normal), delta), bdist = dot(ld(pc.bottom_normal), delta);
    if (!(ldist > 0.0f && rdist > 0.0f && tdist > 0.0f && bdist > 0.0f)) return false;
    const float px = (ldist / (ldist + rdist)) * (float)W;
    const float py = (tdist / (tdist + bdist)) * (float)H;
    if (!(px >= 0.0f && px <= (float)W && py >= 0.0f && py <= (float)H)) return false;  // inf / inf only
    tlx = (int)px, tly = (int)py;
    const float fx = px - (float)tlx, fy = py - (float)tly;
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    w[0] = gx * gy, w[1] = fx * gy, w[2] = gx * fy, w[3] = fx * fy;
    return true;
}

struct Sum {
    float r = 0.f, g = 0.f, b = 0.f, w = 0.f, n = 0.f;
    bool any = false;
};
// One usable tap: weight w, history pixel h (h.w >= 1).
VPX_REPROJECT_HD void tap(Sum& s, float w, Rgbw h) {
    s.r = s.r + w * h.r;
    s.g = s.g + w * h.g;
    s.b = s.b + w * h.b;
    s.w = s.w + w;
    s.n = s.any ? (h.w < s.n ? h.w : s.n) : h.w;
    s.any = true;
}
VPX_REPROJECT_HD float blend_length(const Sum& s, float cap) { return (s.n < cap ? s.n : cap) + 1.0f; }
VPX_REPROJECT_HD Rgbw blend(const Sum& s, Rgbw cur, float cap) {
    const float hr = s.r / s.w, hg = s.g / s.w, hb = s.b / s.w;
    const float n = blend_length(s, cap);
    const float a = 1.0f / n;
    return Rgbw{hr + (cur.r - hr) * a, hg + (cur.g - hg) * a, hb + (cur.b - hb) * a, n};
}

// The moments payload (vpx_reproject_moments): the first two moments of the luminance ride along
// the colour, over the same usable taps with the same weights and the same blend factor.
struct Mom {  // one float2 of a moments image
    float x, y;
};
struct NoMoments {  // vpx_reproject_ids: no payload, nothing of it is compiled in
    static constexpr bool on = false;
    VPX_REPROJECT_HD Mom operator()(uint64_t) const { return Mom{0.f, 0.f}; }
};
VPX_REPROJECT_HD Mom blend_moments(Mom s, const Sum& sum, float l, float l2, float cap) {
    const float h1 = s.x / sum.w, h2 = s.y / sum.w;
    const float a = 1.0f / blend_length(sum, cap);
    return Mom{h1 + (l - h1) * a, h2 + (l2 - h2) * a};
}

// One pixel.  prev_key(i) -> denoise::Key of previous pixel i; hist(i) -> Rgbw of hist_in[i]; both
// are called with in-image indices only, prev_key for all four taps (clamped into the image, so
// that the loads need no branch and go out together) before any hist; hist only under a tap that
// is in the image, has a positive weight and q's key.  tab / moved: the volume table (MOVING).
// mom_in(i) -> Mom of mom_in[i], under a usable tap only; mo: the pixel's moments (MomIn::on).
template <bool MOVING, class PrevKey, class Hist, class MomIn>
VPX_REPROJECT_HD Rgbw pixel(const Args& a, uint32_t x, uint32_t y, Id id, Rgbw cur, PrevKey prev_key, Hist hist,
                            const float* tab, const uint32_t* moved, MomIn mom_in, Mom& mo) {
    float l = 0.f, l2 = 0.f;
    if (MomIn::on) {
        l = denoise::lum(cur.r, cur.g, cur.b);
        l2 = l * l;
        mo = Mom{l, l2};  // the no-history arm's
    }
    const Rgbw none{cur.r, cur.g, cur.b, 1.0f};
    const denoise::Key kq = denoise::plane_key(id.y, id.z, id.w);
    if (!a.have_prev || !denoise::valid(kq) || !(a.cap >= 1.0f)) return none;
    const uint32_t mat = (id.y >> 16) & 255u;
    if (mat >= a.nohist_lo && mat <= a.nohist_hi) return none;
    float t;
    __builtin_memcpy(&t, &id.x, 4);
    V3 P = hit_point(a.cur, a.width, a.height, x, y, t);
    if (MOVING) {
        const uint32_t v = (id.y & 0xffffu) - 2u;  // a valid key has .y & 0xffff >= 2
        if (v >= a.n_volumes) return none;
        if (moved[v]) P = transform_position(transform_position(P, tab + kTabFloats * v), tab + kTabFloats * v + 12u);
    }
    int tlx, tly;
    float w[4];
    if (!footprint(a.prev, P, a.width, a.height, tlx, tly, w)) return none;
    const int W = (int)a.width, H = (int)a.height;
    uint64_t at[4];
    bool use[4];
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const int tx = tlx + (k & 1), ty = tly + (k >> 1);
        const bool in = tx < W && ty < H;  // tlx, tly >= 0
        at[k] = (uint64_t)(ty < H ? ty : H - 1) * a.width + (uint32_t)(tx < W ? tx : W - 1);
        const denoise::Key kr = prev_key(at[k]);
        use[k] = in && w[k] > 0.0f && denoise::same(kr, kq);
    }
    Sum s;
    Mom ms{0.f, 0.f};
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k)
        if (use[k]) {
            const Rgbw h = hist(at[k]);
            if (h.w >= 1.0f) {  // a NaN length fails
                tap(s, w[k], h);
                if (MomIn::on) {
                    const Mom m = mom_in(at[k]);
                    ms.x = ms.x + w[k] * m.x;
                    ms.y = ms.y + w[k] * m.y;
                }
            }
        }
    if (!s.any) return none;
    if (MomIn::on) mo = blend_moments(ms, s, l, l2, a.cap);
    return blend(s, cur, a.cap);
}
template <bool MOVING, class PrevKey, class Hist>
VPX_REPROJECT_HD Rgbw pixel(const Args& a, uint32_t x, uint32_t y, Id id, Rgbw cur, PrevKey prev_key, Hist hist,
                            const float* tab, const uint32_t* moved) {
    Mom mo{0.f, 0.f};
    return pixel<MOVING>(a, x, y, id, cur, prev_key, hist, tab, moved, NoMoments{}, mo);
}

// NULL, or why the call is refused (vpx.h: VPX_E_INVALID).
inline const char* check_call(uint32_t width, uint32_t height, const void* ids_cur, const void* ids_prev, const void* cur,
                              const void* hist_in, const void* hist_out, const vpx_reproject* r, const void* cur_volumes,
                              const void* prev_volumes) {
    if (!ids_cur || !cur || !hist_out || !r) return "null argument";
    if (!ids_prev != !hist_in) return "ids_prev and hist_in come together or not at all";
    if (width == 0 || height == 0 || width > denoise::kMaxSide || height > denoise::kMaxSide) return "frame size out of range";
    if ((uint64_t)((width + 15u) / 16u) * ((height + 15u) / 16u) * 256u > denoise::kMaxTilePixels)
        return "frame larger than 2^27 tile-padded pixels";
    if (!(r->max_history >= 1.0f && r->max_history <= kMaxHistory) || r->max_history != std::floor(r->max_history))
        return "vpx_reproject.max_history must be an integer in 1..65536";
    if (r->nohist_lo <= r->nohist_hi && r->nohist_hi > 255u) return "vpx_reproject.nohist_hi beyond 255";
    if (r->flags != 0u || r->reserved != 0u) return "vpx_reproject.flags and reserved must be 0";
    if (r->n_volumes > kMaxVolumes) return "vpx_reproject.n_volumes beyond 65534";
    if (r->n_volumes > 0u && (!cur_volumes || !prev_volumes)) return "n_volumes without the volume arrays";
    if (hist_out == ids_cur || hist_out == ids_prev || hist_out == cur || hist_out == hist_in)
        return "hist_out must not be an input";
    return nullptr;
}
// vpx_reproject_moments: vpx_reproject_ids' refusals, then the moments buffers'.
inline const char* check_call_moments(uint32_t width, uint32_t height, const void* ids_cur, const void* ids_prev,
                                      const void* cur, const void* hist_in, const void* mom_in, const void* hist_out,
                                      const void* mom_out, const vpx_reproject* r, const void* cur_volumes,
                                      const void* prev_volumes) {
    if (const char* why = check_call(width, height, ids_cur, ids_prev, cur, hist_in, hist_out, r, cur_volumes, prev_volumes))
        return why;
    if (!mom_out) return "null argument";
    if (!mom_in != !hist_in) return "mom_in and hist_in come together or not at all";
    if (mom_in && hist_out == mom_in) return "hist_out must not be an input";
    if (mom_out == ids_cur || mom_out == ids_prev || mom_out == cur || mom_out == hist_in || mom_out == mom_in ||
        mom_out == hist_out)
        return "mom_out must not be an input or hist_out";
    return nullptr;
}

inline Args make_args(uint32_t width, uint32_t height, const vpx_reproject& r, bool have_prev) {
    Args a;
    a.cur = r.cur, a.prev = r.prev;
    a.width = width, a.height = height;
    a.cap = r.max_history - 1.0f;
    a.nohist_lo = r.nohist_lo, a.nohist_hi = r.nohist_hi;
    a.n_volumes = r.n_volumes;
    a.have_prev = have_prev ? 1u : 0u;
    return a;
}

// The volume table: per volume rows 0-2 of cur.inv_matrix and of prev.matrix, and whether the
// volume moved at all (matrix or inv_matrix differ in a byte).
inline void build_table(uint32_t n, const vpx_volume* cur, const vpx_volume* prev, float* tab, uint32_t* moved) {
    for (uint32_t v = 0; v < n; ++v) {
        memcpy(tab + kTabFloats * v, cur[v].inv_matrix, 12 * sizeof(float));
        memcpy(tab + kTabFloats * v + 12u, prev[v].matrix, 12 * sizeof(float));
        moved[v] = (memcmp(cur[v].matrix, prev[v].matrix, sizeof(cur[v].matrix)) != 0 ||
                    memcmp(cur[v].inv_matrix, prev[v].inv_matrix, sizeof(cur[v].inv_matrix)) != 0)
                       ? 1u
                       : 0u;
    }
}

// ---------------------------------------------------------------------------- host path
// The whole call on host memory (check_call has passed); tab / moved: build_table's, n_volumes > 0.
inline void run_host(uint32_t W, uint32_t H, const uint32_t* ids_cur, const uint32_t* ids_prev, const float* cur,
                     const float* hist_in, float* hist_out, uint32_t* rgb8, const vpx_reproject& r, const float* tab,
                     const uint32_t* moved) {
    const Args a = make_args(W, H, r, ids_prev && hist_in);
    auto prev_key = [=](uint64_t i) { return denoise::plane_key(ids_prev[4 * i + 1], ids_prev[4 * i + 2], ids_prev[4 * i + 3]); };
    auto hist = [=](uint64_t i) { return Rgbw{hist_in[4 * i], hist_in[4 * i + 1], hist_in[4 * i + 2], hist_in[4 * i + 3]}; };
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint64_t q = (uint64_t)y * W + x;
            const Id id{ids_cur[4 * q], ids_cur[4 * q + 1], ids_cur[4 * q + 2], ids_cur[4 * q + 3]};
            const Rgbw c{cur[4 * q], cur[4 * q + 1], cur[4 * q + 2], cur[4 * q + 3]};
            const Rgbw o = r.n_volumes ? pixel<true>(a, x, y, id, c, prev_key, hist, tab, moved)
                                       : pixel<false>(a, x, y, id, c, prev_key, hist, tab, moved);
            hist_out[4 * q] = o.r, hist_out[4 * q + 1] = o.g, hist_out[4 * q + 2] = o.b, hist_out[4 * q + 3] = o.w;
            if (rgb8) rgb8[q] = denoise::tonemap_pack_host(hist_out + 4 * q);
        }
}

// vpx_reproject_moments on host memory: the same pixel function with the moments payload.
struct HostMoments {
    static constexpr bool on = true;
    const float* m;
    Mom operator()(uint64_t i) const { return Mom{m[2 * i], m[2 * i + 1]}; }
};
inline void run_host_moments(uint32_t W, uint32_t H, const uint32_t* ids_cur, const uint32_t* ids_prev, const float* cur,
                             const float* hist_in, const float* mom_in, float* hist_out, float* mom_out, uint32_t* rgb8,
                             const vpx_reproject& r, const float* tab, const uint32_t* moved) {
    const Args a = make_args(W, H, r, ids_prev && hist_in);
    auto prev_key = [=](uint64_t i) { return denoise::plane_key(ids_prev[4 * i + 1], ids_prev[4 * i + 2], ids_prev[4 * i + 3]); };
    auto hist = [=](uint64_t i) { return Rgbw{hist_in[4 * i], hist_in[4 * i + 1], hist_in[4 * i + 2], hist_in[4 * i + 3]}; };
    const HostMoments mi{mom_in};
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            const uint64_t q = (uint64_t)y * W + x;
            const Id id{ids_cur[4 * q], ids_cur[4 * q + 1], ids_cur[4 * q + 2], ids_cur[4 * q + 3]};
            const Rgbw c{cur[4 * q], cur[4 * q + 1], cur[4 * q + 2], cur[4 * q + 3]};
            Mom mo{0.f, 0.f};
            const Rgbw o = r.n_volumes ? pixel<true>(a, x, y, id, c, prev_key, hist, tab, moved, mi, mo)
                                       : pixel<false>(a, x, y, id, c, prev_key, hist, tab, moved, mi, mo);
            hist_out[4 * q] = o.r, hist_out[4 * q + 1] = o.g, hist_out[4 * q + 2] = o.b, hist_out[4 * q + 3] = o.w;
            mom_out[2 * q] = mo.x, mom_out[2 * q + 1] = mo.y;
            if (rgb8) rgb8[q] = denoise::tonemap_pack_host(hist_out + 4 * q);
        }
}

}  // namespace reproject
}  // namespace vpx
