// vpx_noise.hpp — Scene::GenerateSomeNoise / GenerateSomeSmoke (host + device).
//
// Both generators (template/scene.cpp:226-282, 285-356) reset the grid, draw one RandomUInt()
// as the noise seed, fill a float field with FastNoise2's Perlin node (GenUniformGrid3D, start
// 0, index x + y*n + z*n*n, cell (x, y, z) sampled at (x*f, y*f, z*f)) and then loop over the
// cells, z outer, y, x inner, turning each value into a material.  FastNoise2 ships as a binary:
// its bits are not reproduced here.  `perlin3` below is this project's definition of the field
// (parity decision 9); everything around it — positions, thresholds with their
// float/double compares and the dead branch, the smoke ellipsoid, the order in which the loops
// consume the xorshift32 stream — is the reference's text.
//
// The loops draw from the caller's xorshift32 state in cell order, so a cell's state depends on
// how many draws came before it:
//   noise  only the cells of one band draw (scene.cpp:254-257): the k-th of them, 0-based, uses
//          the state after 2 + k steps.  The grid is cut into blocks of kBlockCells consecutive
//          cells; a block counts its drawers, an exclusive prefix over the counts gives every
//          block its first rank, and a drawer's rank is that plus its rank inside the block.
//   smoke  every cell draws twice (scene.cpp:314-317): cell i uses the states after 2 + 2i and
//          3 + 2i steps.
// The state after k steps comes from the GF(2) jump of vpx_model.hpp (T^k as a product of the
// T^(2^j)), so blocks are independent of each other: the host loops below and the kernels walk
// them in any order and give the grid of the sequential loop, bit for bit.
//
// All arithmetic is float32 with every product rounded before it is added: build with
// -ffp-contract=off.  The device build flushes float32 subnormals; a value that small (or the
// zero it becomes) changes no sum it enters and stays far below the smallest threshold, so the
// materials do not depend on it.
#pragma once

#include <math.h>
#include <stdint.h>

#include "vpx_model.hpp"

#if defined(__clang__)
#define VPX_NOISE_UNROLL _Pragma("unroll")  // spans stay in registers: every index a constant
#else
#define VPX_NOISE_UNROLL
#endif

namespace vpx {
namespace noise {

constexpr uint32_t kSpan = 16;           // consecutive cells of one thread (one 16-byte store)
constexpr uint32_t kBlockThreads = 256;  // threads of a workgroup
constexpr uint32_t kBlockCells = kSpan * kBlockThreads;  // cells whose drawers are counted together
constexpr uint32_t kScanPass = 256;      // block counts the prefix workgroup takes per pass
constexpr uint8_t kNone = 255;           // MaterialType::NONE
constexpr uint8_t kDrawMark = 254;       // "this cell draws": between the passes only, never left behind

// MaterialType (template/scene.h:38-57)
constexpr uint8_t kNonMetalRed = 1, kMetalHigh = 5, kMetalMid = 6, kMetalLow = 7, kEmissive = 15;
constexpr uint8_t kSmokeLow = 9, kSmokeLow2 = 10, kSmokeMid = 11, kSmokeMid2 = 12, kSmokeHigh = 13;

// ------------------------------------------------------------------------ the field
constexpr uint32_t kPrimeX = 501125321u, kPrimeY = 1136930381u, kPrimeZ = 1720413743u;

VPX_MODEL_HD int32_t lattice(float floored, uint32_t prime) { return (int32_t)((uint32_t)(int32_t)floored * prime); }
VPX_MODEL_HD int32_t next_lattice(int32_t c, uint32_t prime) { return (int32_t)((uint32_t)c + prime); }

VPX_MODEL_HD int32_t mix(int32_t h) {  // the end of hash(): the multiply wraps, the shift is arithmetic
    h = (int32_t)((uint32_t)h * 0x27d4eb2du);
    return (h >> 15) ^ h;
}
VPX_MODEL_HD int32_t hash(int32_t seed, int32_t a, int32_t b, int32_t c) { return mix(seed ^ a ^ b ^ c); }

VPX_MODEL_HD float grad(int32_t h, float fx, float fy, float fz) {
    const int32_t m = h & 13;
    const float u = m < 8 ? fx : fy;
    float v = m == 12 ? fx : fz;
    v = m < 2 ? fy : v;
    return ((h & 1) ? -u : u) + ((h & 2) ? -v : v);
}

VPX_MODEL_HD float fade(float t) { return t * t * t * (t * (t * 6.0f - 15.0f) + 10.0f); }
VPX_MODEL_HD float lerp(float a, float b, float t) { return a + t * (b - a); }

constexpr float kPerlinScale = 0.964921414852142333984375f;

// The definition, one sample at a time.
VPX_MODEL_HD float perlin3(int32_t seed, float x, float y, float z) {
    const float xs = floorf(x), ys = floorf(y), zs = floorf(z);
    const int32_t x0 = lattice(xs, kPrimeX), y0 = lattice(ys, kPrimeY), z0 = lattice(zs, kPrimeZ);
    const int32_t x1 = next_lattice(x0, kPrimeX), y1 = next_lattice(y0, kPrimeY), z1 = next_lattice(z0, kPrimeZ);
    const float xf0 = x - xs, yf0 = y - ys, zf0 = z - zs;
    const float xf1 = xf0 - 1.0f, yf1 = yf0 - 1.0f, zf1 = zf0 - 1.0f;
    const float u = fade(xf0), v = fade(yf0), w = fade(zf0);
    const float g000 = grad(hash(seed, x0, y0, z0), xf0, yf0, zf0), g100 = grad(hash(seed, x1, y0, z0), xf1, yf0, zf0);
    const float g010 = grad(hash(seed, x0, y1, z0), xf0, yf1, zf0), g110 = grad(hash(seed, x1, y1, z0), xf1, yf1, zf0);
    const float g001 = grad(hash(seed, x0, y0, z1), xf0, yf0, zf1), g101 = grad(hash(seed, x1, y0, z1), xf1, yf0, zf1);
    const float g011 = grad(hash(seed, x0, y1, z1), xf0, yf1, zf1), g111 = grad(hash(seed, x1, y1, z1), xf1, yf1, zf1);
    return kPerlinScale * lerp(lerp(lerp(g000, g100, u), lerp(g010, g110, u), v),
                               lerp(lerp(g001, g101, u), lerp(g011, g111, u), v), w);
}

// The same sample with what a grid row shares taken out: the y and z lattice terms, offsets and
// fades, and seed ^ y_j ^ z_k of the four (j, k) — xor is associative, every float operation is
// the one perlin3 does.
struct Row {
    int32_t h00, h10, h01, h11;  // seed ^ y_j ^ z_k as h<j><k>
    float yf0, yf1, zf0, zf1, v, w;
};
VPX_MODEL_HD Row row_terms(int32_t seed, float y, float z) {
    const float ys = floorf(y), zs = floorf(z);
    const int32_t y0 = lattice(ys, kPrimeY), z0 = lattice(zs, kPrimeZ);
    const int32_t y1 = next_lattice(y0, kPrimeY), z1 = next_lattice(z0, kPrimeZ);
    Row r;
    r.h00 = seed ^ y0 ^ z0, r.h10 = seed ^ y1 ^ z0, r.h01 = seed ^ y0 ^ z1, r.h11 = seed ^ y1 ^ z1;
    r.yf0 = y - ys, r.zf0 = z - zs;
    r.yf1 = r.yf0 - 1.0f, r.zf1 = r.zf0 - 1.0f;
    r.v = fade(r.yf0), r.w = fade(r.zf0);
    return r;
}
VPX_MODEL_HD float perlin_row(const Row& r, float x) {
    const float xs = floorf(x);
    const int32_t x0 = lattice(xs, kPrimeX), x1 = next_lattice(x0, kPrimeX);
    const float xf0 = x - xs, xf1 = xf0 - 1.0f, u = fade(xf0);
    const float g000 = grad(mix(r.h00 ^ x0), xf0, r.yf0, r.zf0), g100 = grad(mix(r.h00 ^ x1), xf1, r.yf0, r.zf0);
    const float g010 = grad(mix(r.h10 ^ x0), xf0, r.yf1, r.zf0), g110 = grad(mix(r.h10 ^ x1), xf1, r.yf1, r.zf0);
    const float g001 = grad(mix(r.h01 ^ x0), xf0, r.yf0, r.zf1), g101 = grad(mix(r.h01 ^ x1), xf1, r.yf0, r.zf1);
    const float g011 = grad(mix(r.h11 ^ x0), xf0, r.yf1, r.zf1), g111 = grad(mix(r.h11 ^ x1), xf1, r.yf1, r.zf1);
    return kPerlinScale * lerp(lerp(lerp(g000, g100, u), lerp(g010, g110, u), r.v),
                               lerp(lerp(g001, g101, u), lerp(g011, g111, u), r.v), r.w);
}

// ------------------------------------------------------------------- the two loops' bodies
// RandomFloat() of the draw u (tmpl8math.cpp:130-133)
VPX_MODEL_HD float random_float(uint32_t u) { return (float)u * 2.3283064365387e-10f; }

// GenerateSomeNoise's chain (scene.cpp:250-275) up to the draw: the cell's material, or
// kDrawMark for the band that calls Rand.  `n < 0.08`, `n < 0.2` and `n < 0.3` compare in double:
// 0.08f lies below 0.08 and still draws, 0.2f and 0.3f lie above their literals and fall
// through to EMISSIVE and METAL_HIGH.  `n < 0.17f` (:262) can never hold after `n < 0.2`
// failed.  A NaN fails every compare and keeps NONE.
VPX_MODEL_HD uint8_t noise_class(float n) {
    if (n <= 0.04f) return kNone;
    if ((double)n < 0.08) return kDrawMark;
    if ((double)n < 0.2) return kNonMetalRed;
    if (n < 0.17f) return 0;  // NON_METAL_WHITE: dead
    if ((double)n < 0.3) return kEmissive;
    if (n < 0.5f) return kMetalHigh;
    if (n < 0.7f) return kMetalMid;
    if (n < 0.9f) return kMetalLow;
    return kNone;
}
// static_cast<MatType>(Rand(static_cast<float>(GLASS))) (scene.cpp:256, tmpl8math.cpp:149-152):
// 0..7, and 8 when RandomFloat() rounds to 1.0f
VPX_MODEL_HD uint8_t noise_draw(uint32_t u) { return (uint8_t)(random_float(u) * 8.0f); }

// GenerateSomeSmoke's body (scene.cpp:304-349) for the cell (x, y, z) of an n^3 grid with the
// noise value nv; ux and uz are the draws of randomX and randomZ.  Rand(min, max) is
// min + RandomFloat() * (max - min) (tmpl8math.cpp:154-157), float3 - and / are per component
// (tmpl8math.h:1361, 1950) and dot is a.x*b.x + a.y*b.y + a.z*b.z, summed left to right
// (tmpl8math.h:2259-2262).
VPX_MODEL_HD uint8_t smoke_cell(float nv, uint32_t x, uint32_t y, uint32_t z, uint32_t n, uint32_t ux, uint32_t uz) {
    const float ws = (float)n;
    const float center = ws / 2.0f;            // :308-311, all three components
    const float lo = -ws / 4.0f, hi = ws / 2.0f;  // :314-317
    const float randomX = ws / 2.0f + (lo + random_float(ux) * (hi - lo));
    const float randomZ = ws / 2.0f + (lo + random_float(uz) * (hi - lo));
    const float dimy = ws / 3.0f;              // :318-321
    const float dx = ((float)x - center) / randomX, dy = ((float)y - center) / dimy, dz = ((float)z - center) / randomZ;  // :323
    const float d2 = dx * dx + dy * dy + dz * dz;  // :324
    if (nv - d2 < 0.04f || d2 > 1.5f) return kNone;  // :326
    if (nv < 0.3f) return kSmokeHigh;
    if (nv < 0.4f) return kSmokeMid2;
    if (nv < 0.6f) return kSmokeMid;
    if (nv < 0.7f) return kSmokeLow2;
    if (nv < 1.0f) return kSmokeLow;
    return kNone;
}

// ------------------------------------------------------------------------- spans of cells
// The noise values of `count` cells from the linear index `first` on.  ROW: the cells lie in one
// grid row (n % kSpan == 0 and first % kSpan == 0), the row's terms are computed once; otherwise
// every cell is taken apart and sampled on its own.
struct Cell {
    uint32_t x, y, z;
};
VPX_MODEL_HD Cell cell_of(uint64_t i, uint32_t n) {
    const uint64_t row = i / n;
    return Cell{(uint32_t)(i % n), (uint32_t)(row % n), (uint32_t)(row / n)};
}
VPX_MODEL_HD void next_cell(Cell& p, uint32_t n) {  // loop order: x inner, then y, then z
    if (++p.x == n) {
        p.x = 0;
        if (++p.y == n) p.y = 0, ++p.z;
    }
}

template <bool ROW>
VPX_MODEL_HD void field_span(int32_t nseed, uint32_t n, float f, uint64_t first, uint32_t count, float* out) {
    Cell p = cell_of(first, n);
    if (ROW) {
        const Row r = row_terms(nseed, (float)p.y * f, (float)p.z * f);
        VPX_NOISE_UNROLL
        for (uint32_t c = 0; c < kSpan; ++c)
            if (c < count) out[c] = perlin_row(r, (float)(p.x + c) * f);
    } else {
        VPX_NOISE_UNROLL
        for (uint32_t c = 0; c < kSpan; ++c) {
            if (c >= count) continue;
            out[c] = perlin3(nseed, (float)p.x * f, (float)p.y * f, (float)p.z * f);
            next_cell(p, n);
        }
    }
}

// Pass 1 of the noise generator on a span: the bytes (kDrawMark where a cell draws) and the
// mask of the drawers, bit c = cell first + c.
template <bool ROW>
VPX_MODEL_HD uint32_t noise_span(int32_t nseed, uint32_t n, float f, uint64_t first, uint32_t count, uint8_t* vals) {
    float nv[kSpan];
    field_span<ROW>(nseed, n, f, first, count, nv);
    uint32_t mask = 0;
    VPX_NOISE_UNROLL
    for (uint32_t c = 0; c < kSpan; ++c) {
        if (c >= count) continue;
        vals[c] = noise_class(nv[c]);
        mask |= (uint32_t)(vals[c] == kDrawMark) << c;
    }
    return mask;
}

// Pass 3 on a span: the marked cells take their draws, the first from the state after `s`.
VPX_MODEL_HD void noise_fill_span(uint32_t s, uint32_t mask, uint8_t* vals) {
    VPX_NOISE_UNROLL
    for (uint32_t c = 0; c < kSpan; ++c)
        if (mask >> c & 1u) {
            s = model::xs32_step(s);
            vals[c] = noise_draw(s);
        }
}

// The smoke generator on a span; s: the state before the span's first draw (after 1 + 2*first
// steps).  Returns the state after the span's last draw.
template <bool ROW>
VPX_MODEL_HD uint32_t smoke_span(int32_t nseed, uint32_t n, float f, uint64_t first, uint32_t count, uint32_t s, uint8_t* vals) {
    float nv[kSpan];
    field_span<ROW>(nseed, n, f, first, count, nv);
    Cell p = cell_of(first, n);
    VPX_NOISE_UNROLL
    for (uint32_t c = 0; c < kSpan; ++c) {
        if (c >= count) continue;
        const uint32_t ux = model::xs32_step(s);
        s = model::xs32_step(ux);
        vals[c] = smoke_cell(nv[c], p.x, p.y, p.z, n, ux, s);
        next_cell(p, n);
    }
    return s;
}

// ---------------------------------------------------------------------------- the call
#ifdef VPX_H_
// The argument rules of vpx_grid_generate_noise / vpx_noise_generate_host: nullptr, or what is
// wrong.  (n - 1) * |frequency| < 2^30 keeps every floored coordinate inside int32.
inline const char* check_gen(const vpx_noise_gen* in, uint32_t n) {
    if (!in) return "null vpx_noise_gen";
    if (in->reserved != 0) return "vpx_noise_gen.reserved must be 0";
    if (in->mode > VPX_GEN_SMOKE) return "unknown generator mode";
    if (n == 0 || n > 4096) return "grid size must be in [1, 4096]";
    if (!isfinite(in->frequency)) return "frequency must be finite";
    if (!((double)(n - 1) * fabs((double)in->frequency) < 1073741824.0)) return "(n - 1) * |frequency| must stay below 2^30";
    return nullptr;
}

// The whole grid on the host, block by block the way the kernels do it: t holds the jump
// matrices T^(2^j), at least the 38 that 1 + 2 * 4096^3 steps need; cells: n^3 bytes.
inline void generate_host(const uint32_t* t, uint32_t n, const vpx_noise_gen* in, uint8_t* cells, vpx_noise_result* out) {
    const uint64_t total = (uint64_t)n * n * n, blocks = (total + kBlockCells - 1) / kBlockCells;
    const bool row = n % kSpan == 0;
    const float f = in->frequency;
    const uint32_t us = model::xs32_step(in->seed);
    const int32_t nseed = (int32_t)us;
    uint64_t draws = 1;
    auto span_count = [&](uint64_t first) { return (uint32_t)(total - first < kSpan ? total - first : kSpan); };
    if (in->mode == VPX_GEN_SMOKE) {
        for (uint64_t b = 0; b < blocks; ++b) {
            uint32_t s = model::xs32_jump(t, in->seed, 1 + 2 * b * kBlockCells);
            for (uint64_t first = b * kBlockCells; first < total && first < (b + 1) * kBlockCells; first += kSpan)
                s = row ? smoke_span<true>(nseed, n, f, first, kSpan, s, cells + first)
                        : smoke_span<false>(nseed, n, f, first, span_count(first), s, cells + first);
        }
        draws += 2 * total;
    } else {
        uint64_t rank = 0;  // the exclusive prefix over the blocks' counts, as it goes
        for (uint64_t b = 0; b < blocks; ++b) {
            uint32_t masks[kBlockThreads];
            uint32_t cnt = 0;
            for (uint32_t th = 0; th < kBlockThreads; ++th) {
                const uint64_t first = b * kBlockCells + (uint64_t)th * kSpan;
                masks[th] = 0;
                if (first >= total) continue;
                masks[th] = row ? noise_span<true>(nseed, n, f, first, kSpan, cells + first)
                                : noise_span<false>(nseed, n, f, first, span_count(first), cells + first);
                cnt += (uint32_t)__builtin_popcount(masks[th]);
            }
            if (cnt) {
                const uint32_t base = model::xs32_jump(t, in->seed, 1 + rank);  // block-wide part of the jump
                uint32_t inblock = 0;
                for (uint32_t th = 0; th < kBlockThreads; ++th) {
                    if (!masks[th]) continue;
                    const uint64_t first = b * kBlockCells + (uint64_t)th * kSpan;
                    uint8_t v[kSpan];
                    const uint32_t cnt_span = span_count(first);
                    for (uint32_t c = 0; c < cnt_span; ++c) v[c] = cells[first + c];
                    noise_fill_span(model::xs32_jump(t, base, inblock), masks[th], v);
                    for (uint32_t c = 0; c < cnt_span; ++c) cells[first + c] = v[c];
                    inblock += (uint32_t)__builtin_popcount(masks[th]);
                }
            }
            rank += cnt;
        }
        draws += rank;
    }
    if (out) {
        out->noise_seed = us;
        out->draws = draws;
        out->seed = model::xs32_jump(t, in->seed, draws);
    }
}
#endif

}  // namespace noise
}  // namespace vpx
