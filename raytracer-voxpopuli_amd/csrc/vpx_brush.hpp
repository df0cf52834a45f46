// vpx_brush.hpp — brush edits (vpx_grid_brush, vpx_brush_apply_host): host + device.
//
// A brush writes one byte into the cells of a sphere or a box that pass its filter.  All
// arithmetic is integer (the sphere test in int64), so the host loop and brush_k give the same
// bytes; brushes apply in order, a later one's filter reading what an earlier one left.
#pragma once

#include <stdint.h>

#include "../../include/vpx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VPX_BRUSH_HD __host__ __device__ __forceinline__
#else
#define VPX_BRUSH_HD inline
#endif

namespace vpx {
namespace brush {

constexpr uint32_t kMaxBrushes = 256;

// NULL, or why the brush list is not valid (vpx.h: VPX_E_INVALID).
inline const char* check_brushes(const vpx_brush* b, uint32_t count) {
    if (!b) return "null brushes";
    if (count < 1 || count > kMaxBrushes) return "brush count outside 1..256";
    for (uint32_t i = 0; i < count; ++i) {
        if (b[i].shape != VPX_BRUSH_SPHERE && b[i].shape != VPX_BRUSH_BOX) return "unknown brush shape";
        if (b[i].reserved != 0) return "vpx_brush.reserved must be 0";
        if (b[i].match_lo > b[i].match_hi) return "match_lo > match_hi";
    }
    return nullptr;
}

// floor(sqrt(v)), exact
inline uint32_t isqrt(uint32_t v) {
    uint32_t r = 0;
    for (uint32_t bit = 1u << 15; bit; bit >>= 1) {
        const uint32_t t = r | bit;
        if ((uint64_t)t * t <= v) r = t;
    }
    return r;
}

// The brush's bounding box clipped to the grid (inclusive cells); false: it holds no cell.
inline bool clipped_box(const vpx_brush& b, uint32_t n, uint32_t lo[3], uint32_t hi[3]) {
    const int64_t r = b.shape == VPX_BRUSH_SPHERE ? (int64_t)isqrt(b.r2) : 0;
    for (int q = 0; q < 3; ++q) {
        int64_t l = b.shape == VPX_BRUSH_SPHERE ? (int64_t)b.center[q] - r : (int64_t)b.lo[q];
        int64_t h = b.shape == VPX_BRUSH_SPHERE ? (int64_t)b.center[q] + r : (int64_t)b.hi[q];
        if (l < 0) l = 0;
        if (h > (int64_t)n - 1) h = (int64_t)n - 1;
        if (l > h) return false;
        lo[q] = (uint32_t)l, hi[q] = (uint32_t)h;
    }
    return true;
}

// Cell (x, y, z) lies in the brush's shape (the box is the clipped one: the caller's loop).
VPX_BRUSH_HD bool in_shape(const vpx_brush& b, uint32_t x, uint32_t y, uint32_t z) {
    if (b.shape != VPX_BRUSH_SPHERE) return true;
    const int64_t dx = (int64_t)x - b.center[0], dy = (int64_t)y - b.center[1], dz = (int64_t)z - b.center[2];
    return dx * dx + dy * dy + dz * dz <= (int64_t)b.r2;
}

// The byte the brush leaves in a cell of its shape that holds m, and whether it changed.
VPX_BRUSH_HD bool writes(const vpx_brush& b, uint8_t m) { return m >= b.match_lo && m <= b.match_hi && m != b.value; }

// One brush over a host grid; returns the cells whose byte changed.
inline uint64_t apply_host(uint8_t* cells, uint32_t n, const vpx_brush& b) {
    uint32_t lo[3], hi[3];
    if (!clipped_box(b, n, lo, hi)) return 0;
    uint64_t changed = 0;
    for (uint32_t z = lo[2]; z <= hi[2]; ++z)
        for (uint32_t y = lo[1]; y <= hi[1]; ++y)
            for (uint32_t x = lo[0]; x <= hi[0]; ++x) {
                uint8_t& c = cells[x + (uint64_t)y * n + (uint64_t)z * n * n];
                if (in_shape(b, x, y, z) && writes(b, c)) c = b.value, ++changed;
            }
    return changed;
}

}  // namespace brush
}  // namespace vpx
