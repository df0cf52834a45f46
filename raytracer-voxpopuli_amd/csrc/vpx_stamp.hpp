// vpx_stamp.hpp — model stamps (vpx_grid_stamp, vpx_stamp_apply_host): host + device.
//
// A stamp gathers an oriented resident model into a box of an existing grid: every cell of the
// box reads ONE voxel, a non-empty voxel writes its byte (or the stamp's constant) where the
// cell's byte passes the filter.  All arithmetic is integer, so the host loop and stamp_k give
// the same bytes; stamps apply in order, a later one's filter reading what an earlier one left.
#pragma once

#include <stdint.h>

#include "../../include/vpx.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VPX_STAMP_HD __host__ __device__ __forceinline__
#else
#define VPX_STAMP_HD inline
#endif

namespace vpx {
namespace stamp {

constexpr uint32_t kMaxStamps = 256;
constexpr uint32_t kMaxDim = 256;  // a resident model's dimensions (vpx_model_upload)
constexpr uint32_t kKnownFlags = VPX_STAMP_GRID_BYTES | VPX_STAMP_CONSTANT;
constexpr uint32_t kOrientBits = 0x3Fu | 0x700u;

// vpx_stamp.orient decoded: axis[q] the model axis that feeds grid axis q, flip[q] whether grid
// q runs against it.  False: the axes are no permutation, or a stray bit is set.
VPX_STAMP_HD bool decode_orient(uint32_t orient, uint32_t axis[3], bool flip[3]) {
    if (orient & ~kOrientBits) return false;
    uint32_t seen = 0;
    for (int q = 0; q < 3; ++q) {
        axis[q] = (orient >> (2 * q)) & 3u;
        flip[q] = ((orient >> (8 + q)) & 1u) != 0;
        if (axis[q] > 2) return false;
        seen |= 1u << axis[q];
    }
    return seen == 7u;
}

// NULL, or why the stamp list is not valid (vpx.h: VPX_E_INVALID); the models are the caller's
// to look up.
inline const char* check_stamps(const vpx_stamp* s, uint32_t count) {
    if (!s) return "null stamps";
    if (count < 1 || count > kMaxStamps) return "stamp count outside 1..256";
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t axis[3];
        bool flip[3];
        if (!decode_orient(s[i].orient, axis, flip)) return "orient is not a permutation with mirror bits";
        if (s[i].flags & ~kKnownFlags) return "unknown stamp flags";
        if (s[i].reserved != 0 || s[i].reserved2 != 0) return "vpx_stamp.reserved must be 0";
        if (s[i].match_lo > s[i].match_hi) return "match_lo > match_hi";
    }
    return nullptr;
}

// One stamp of one model, ready for the cells: the clipped box, and the model index of a cell
// as base + sum(step[q] * (g[q] - origin[q])).
struct Plan {
    int32_t origin[3];
    uint32_t lo[3], hi[3];  // the stamp's box clipped to the grid, inclusive
    int32_t base, step[3];
    uint32_t flags;
    uint8_t value, match_lo, match_hi, pad;
};

// The plan of a valid stamp (check_stamps) of a model sx * sy * sz in an n^3 grid; false: its
// box holds no cell of the grid.
inline bool plan(const vpx_stamp& s, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n, Plan& p) {
    const uint32_t size[3] = {sx, sy, sz};
    const int32_t stride[3] = {1, (int32_t)sx, (int32_t)(sx * sy)};
    uint32_t axis[3];
    bool flip[3];
    if (!decode_orient(s.orient, axis, flip)) return false;
    p.base = 0;
    p.flags = s.flags, p.value = s.value, p.match_lo = s.match_lo, p.match_hi = s.match_hi, p.pad = 0;
    for (int q = 0; q < 3; ++q) {
        const int64_t e = size[axis[q]];
        int64_t l = (int64_t)s.origin[q], h = l + e - 1;
        if (l < 0) l = 0;
        if (h > (int64_t)n - 1) h = (int64_t)n - 1;
        if (l > h) return false;
        p.origin[q] = s.origin[q];
        p.lo[q] = (uint32_t)l, p.hi[q] = (uint32_t)h;
        p.step[q] = flip[q] ? -stride[axis[q]] : stride[axis[q]];
        if (flip[q]) p.base += (int32_t)(e - 1) * stride[axis[q]];
    }
    return true;
}

// The model index of the first cell (x = origin[0]) of the box's row (y, z); along grid x it
// moves by step[0].
VPX_STAMP_HD int32_t row_base(const Plan& p, uint32_t y, uint32_t z) {
    return p.base + p.step[1] * ((int32_t)y - p.origin[1]) + p.step[2] * ((int32_t)z - p.origin[2]);
}

// An empty voxel leaves its cell alone.
VPX_STAMP_HD bool empty(uint32_t flags, uint8_t v) { return (flags & VPX_STAMP_GRID_BYTES) ? v == 255 : v == 0; }

// The byte voxel v leaves in a cell that holds c; true: it differs from c.
VPX_STAMP_HD bool writes(const Plan& p, uint8_t v, uint8_t c, uint8_t& w) {
    w = (p.flags & VPX_STAMP_CONSTANT) ? p.value : v;
    return !empty(p.flags, v) && c >= p.match_lo && c <= p.match_hi && c != w;
}

// One planned stamp over a host grid; returns the cells whose byte changed.
inline uint64_t apply_host(uint8_t* cells, uint32_t n, const Plan& p, const uint8_t* vox) {
    uint64_t changed = 0;
    for (uint32_t z = p.lo[2]; z <= p.hi[2]; ++z)
        for (uint32_t y = p.lo[1]; y <= p.hi[1]; ++y) {
            const int32_t row = row_base(p, y, z);
            for (uint32_t x = p.lo[0]; x <= p.hi[0]; ++x) {
                uint8_t& c = cells[x + (uint64_t)y * n + (uint64_t)z * n * n];
                uint8_t w;
                if (writes(p, vox[row + p.step[0] * ((int32_t)x - p.origin[0])], c, w)) c = w, ++changed;
            }
        }
    return changed;
}

}  // namespace stamp
}  // namespace vpx
