// vpx_model.hpp — placing a .vox model into a grid (host + device).
//
// The reference's three loaders (Scene::LoadModel, LoadModelPartial, LoadModelRandomMaterials,
// template/scene.cpp:449-683) reset the grid to NONE and then loop over the model's voxels,
// z outer, y, x inner, writing voxel (x, y, z) to the cell
//     (trunc(x * s.x), trunc(z * s.y), trunc(y * s.z))          (y and z swapped)
// so where several voxels land in one cell the last one of the loop stays.  The target is a
// product of three per-axis maps, so the voxels that land in cell (gx, gy, gz) are the box
// X(gx) x Y(gz) x Z(gy) of the maps' preimages, and the last writer is the non-empty voxel
// of that box with the largest z, then y, then x.  A Plan holds the three preimage tables
// ("sources of destination coordinate g, ascending"); place_cell scans a cell's box from its
// last voxel backwards.  The maps are computed once, on the host, with the reference's float
// arithmetic; whoever gathers (host loop or kernel) does integer work only, so both give the
// same grid whatever the order they visit the cells in.  Writes the reference's unchecked
// Set would make outside the grid have no preimage entry: they are dropped.
//
// LoadModelPartial keeps the model columns x in [columns - thickness, columns + thickness]
// (uint32 arithmetic): the x table simply lists those columns only.
//
// LoadModelRandomMaterials draws Rand(lo, hi) once per voxel in loop order, empty voxels
// included, from a xorshift32 state (tmpl8math.cpp:119-133, 154-157).  The step is linear
// over GF(2), state' = T state, so voxel i's draw is T^(i+1) seed: with the matrices
// T^(2^j) a chunk of voxels jumps to its first state and steps from there.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define VPX_MODEL_HD __host__ __device__ __forceinline__
#else
#define VPX_MODEL_HD inline
#endif

namespace vpx {
namespace model {

constexpr uint32_t kMaxDim = 256;     // a .vox model is at most 256 voxels a side
constexpr uint8_t kNoneMat = 255;     // MaterialType::NONE
constexpr uint32_t kJumpDevice = 40;  // T^(2^j), j < 40: every voxel index of a 256^3 model, and the
                                      // 1 + 2 * 4096^3 draws of a smoke grid (vpx_noise.hpp)
constexpr uint32_t kJumpHost = 64;
constexpr uint32_t kChunk = 64;       // voxels per thread of the random-material pass

// ---------------------------------------------------------------------- xorshift32
VPX_MODEL_HD uint32_t xs32_step(uint32_t s) {  // RandomUInt, tmpl8math.cpp:119-125
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return s;
}

// m: 32 words, word b = the image of bit b
VPX_MODEL_HD uint32_t xs32_apply(const uint32_t* m, uint32_t s) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < 32; ++b) r ^= m[b] & (0u - ((s >> b) & 1u));
    return r;
}

// t: `levels` matrices of 32 words, matrix j = T^(2^j)
inline void xs32_build_tables(uint32_t* t, uint32_t levels) {
    for (uint32_t b = 0; b < 32; ++b) t[b] = xs32_step(1u << b);
    for (uint32_t j = 1; j < levels; ++j)
        for (uint32_t b = 0; b < 32; ++b) t[32 * j + b] = xs32_apply(t + 32 * (j - 1), t[32 * (j - 1) + b]);
}

// the state after k steps (k < 2^levels)
VPX_MODEL_HD uint32_t xs32_jump(const uint32_t* t, uint32_t s, uint64_t k) {
    for (uint32_t j = 0; k; ++j, k >>= 1)
        if (k & 1u) s = xs32_apply(t + 32 * j, s);
    return s;
}

// static_cast<MatType>(Rand(lo, hi)) of the draw u: lo + RandomFloat() * (hi - lo), the
// product rounded before the sum (build with -ffp-contract=off); 0 <= lo <= hi <= 255
VPX_MODEL_HD uint8_t xs32_material(uint32_t u, float lo, float hi) {
    const float r = (float)u * 2.3283064365387e-10f;
    const float p = r * (hi - lo);
    return (uint8_t)(lo + p);
}

// Materials of the voxels [first, first + kChunk) into mat (whole chunks: mat holds a
// multiple of kChunk bytes, the draws past the model's end are not read by anyone).
VPX_MODEL_HD void random_chunk(const uint32_t* t, uint32_t seed, uint64_t first, float lo, float hi, uint8_t* mat) {
    uint32_t s = xs32_jump(t, seed, first);
    for (uint32_t k = 0; k < kChunk; k += 16) {
        uint8_t v[16];
        for (uint32_t c = 0; c < 16; ++c) {
            s = xs32_step(s);
            v[c] = xs32_material(s, lo, hi);
        }
        uint32_t w[4];
        for (uint32_t q = 0; q < 4; ++q)
            w[q] = (uint32_t)v[4 * q] | (uint32_t)v[4 * q + 1] << 8 | (uint32_t)v[4 * q + 2] << 16 | (uint32_t)v[4 * q + 3] << 24;
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<uint4*>(mat + first + k) = make_uint4(w[0], w[1], w[2], w[3]);
#else
        for (uint32_t q = 0; q < 4; ++q)
            for (uint32_t c = 0; c < 4; ++c) mat[first + k + 4 * q + c] = (uint8_t)(w[q] >> (8 * c));
#endif
    }
}

// ------------------------------------------------------------------------- the plan
// Axis 0: grid x from model x (sx entries, scale s.x, column filter); axis 1: grid y from
// model z (sz, s.y); axis 2: grid z from model y (sy, s.z).  Bytes: src[3][256], the model
// coordinates of each axis sorted by (destination, coordinate); then start[3][n + 1] of
// uint16: the sources of destination g on axis a are src[a][start[a][g] .. start[a][g + 1]).
constexpr uint32_t kSrcBytes = 3 * kMaxDim;
inline uint64_t plan_bytes(uint32_t n) { return (kSrcBytes + 6ull * (n + 1ull) + 15ull) & ~15ull; }

struct PlanView {
    const uint8_t* src;
    const uint16_t* start;
    uint32_t n;
};
inline PlanView plan_view(const uint8_t* plan, uint32_t n) {
    return PlanView{plan, reinterpret_cast<const uint16_t*>(plan + kSrcBytes), n};
}

// static_cast<int>(float) as the x86 reference computes it: NaN and overflow give INT_MIN
inline int32_t f2i_trunc(float f) {
    if (!(f > -2147483904.0f && f < 2147483648.0f)) return INT32_MIN;
    return (int32_t)f;
}

// Scene::scaleModel as the loaders leave it: multiplied when size_x > gridsize, per call
inline void scale_rule(const float in[3], uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n, float out[3]) {
    out[0] = in[0], out[1] = in[1], out[2] = in[2];
    if (sx > n) {
        out[0] *= (float)n / (float)sx;
        out[1] *= (float)n / (float)sy;
        out[2] *= (float)n / (float)sz;
    }
}

// plan: plan_bytes(n) bytes, 2-byte aligned.  scl: the scale already multiplied (scale_rule).
// Model columns outside [col_lo, col_hi] get no entry (FULL: 0, 0xffffffff).
inline void build_plan(uint8_t* plan, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n, const float scl[3],
                       uint32_t col_lo, uint32_t col_hi) {
    uint16_t* start = reinterpret_cast<uint16_t*>(plan + kSrcBytes);
    const uint32_t dim[3] = {sx, sz, sy};
    for (uint32_t a = 0; a < 3; ++a) {
        uint8_t* src = plan + a * kMaxDim;
        uint16_t* st = start + (uint64_t)a * (n + 1);
        int32_t g[kMaxDim];
        for (uint32_t g0 = 0; g0 <= n; ++g0) st[g0] = 0;
        for (uint32_t v = 0; v < dim[a]; ++v) {
            g[v] = f2i_trunc((float)v * scl[a]);
            if (g[v] < 0 || (uint32_t)g[v] >= n || (a == 0 && !(v >= col_lo && v <= col_hi))) g[v] = -1;
            if (g[v] >= 0) ++st[g[v] + 1];
        }
        for (uint32_t g0 = 0; g0 < n; ++g0) st[g0 + 1] = (uint16_t)(st[g0 + 1] + st[g0]);
        for (uint32_t v = 0; v < kMaxDim; ++v) src[v] = 0;
        // sources in ascending order take their destination's next slot: st[g] walks up to the
        // old st[g + 1], so shifting the table by one entry afterwards restores it
        for (uint32_t v = 0; v < dim[a]; ++v)
            if (g[v] >= 0) src[st[g[v]]++] = (uint8_t)v;
        for (uint32_t g0 = n; g0 > 0; --g0) st[g0] = st[g0 - 1];
        st[0] = 0;
    }
}

#ifdef VPX_H_
// The argument rules of vpx_grid_load_model / vpx_model_place_host: nullptr, or what is wrong
inline const char* check_load(const vpx_model_load* in, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n) {
    if (!in) return "null vpx_model_load";
    if (in->reserved != 0) return "vpx_model_load.reserved must be 0";
    if (in->mode > VPX_LOAD_RANDOM) return "unknown load mode";
    if (!sx || !sy || !sz || sx > kMaxDim || sy > kMaxDim || sz > kMaxDim) return "model dimension outside 1..256";
    if (n == 0 || n > 4096) return "grid size must be in [1, 4096]";
    if (in->mode == VPX_LOAD_RANDOM && !(0.0f <= in->rand_lo && in->rand_lo <= in->rand_hi && in->rand_hi <= 255.0f))
        return "random material range must satisfy 0 <= rand_lo <= rand_hi <= 255";
    return nullptr;
}

// The plan of one load and the scale it leaves behind
inline void plan_load(uint8_t* plan, const vpx_model_load* in, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n,
                      float scale_out[3]) {
    scale_rule(in->scale_model, sx, sy, sz, n, scale_out);
    const bool part = in->mode == VPX_LOAD_PARTIAL;
    build_plan(plan, sx, sy, sz, n, scale_out, part ? in->columns - in->thickness : 0u,
               part ? in->columns + in->thickness : 0xffffffffu);
}
#endif

// The cell whose sources are xs x ys x zs (model coordinates, ascending): the last non-empty
// voxel in loop order, its byte of `mat` (the model itself, or the random materials).
VPX_MODEL_HD uint8_t place_cell(const uint8_t* xs, uint32_t nx, const uint8_t* ys, uint32_t ny, const uint8_t* zs,
                                uint32_t nz, const uint8_t* vox, const uint8_t* mat, uint32_t sx, uint32_t sxy) {
    for (uint32_t zi = nz; zi-- > 0;)
        for (uint32_t yi = ny; yi-- > 0;) {
            const uint32_t row = (uint32_t)ys[yi] * sx + (uint32_t)zs[zi] * sxy;
            for (uint32_t xi = nx; xi-- > 0;) {
                const uint32_t i = row + xs[xi];
                if (vox[i]) return mat[i];
            }
        }
    return kNoneMat;
}

// CNT consecutive cells of the grid row (gy, gz) from gx0 on (gx0 + CNT <= n)
template <int CNT>
VPX_MODEL_HD void place_span(const PlanView& p, const uint8_t* vox, const uint8_t* mat, uint32_t sx, uint32_t sy,
                             uint32_t gx0, uint32_t gy, uint32_t gz, uint8_t* vals) {
    const uint16_t* stx = p.start;
    const uint16_t* sty = p.start + (p.n + 1);
    const uint16_t* stz = p.start + 2 * (p.n + 1);
    const uint32_t z0 = sty[gy], nz = sty[gy + 1] - z0;  // grid y <- model z
    const uint32_t y0 = stz[gz], ny = stz[gz + 1] - y0;  // grid z <- model y
    if (!nz || !ny) {
        for (int c = 0; c < CNT; ++c) vals[c] = kNoneMat;
        return;
    }
    const uint8_t* zs = p.src + kMaxDim + z0;
    const uint8_t* ys = p.src + 2 * kMaxDim + y0;
    for (int c = 0; c < CNT; ++c) {
        const uint32_t x0 = stx[gx0 + c], nx = stx[gx0 + c + 1] - x0;
        vals[c] = place_cell(p.src + x0, nx, ys, ny, zs, nz, vox, mat, sx, sx * sy);
    }
}

// The whole grid on the host: cells = n^3 bytes
inline void place_grid(const PlanView& p, const uint8_t* vox, const uint8_t* mat, uint32_t sx, uint32_t sy,
                       uint8_t* cells) {
    const uint64_t n = p.n;
    for (uint32_t gz = 0; gz < p.n; ++gz)
        for (uint32_t gy = 0; gy < p.n; ++gy) {
            uint8_t* row = cells + gy * n + gz * n * n;
            for (uint32_t gx = 0; gx < p.n; ++gx) place_span<1>(p, vox, mat, sx, sy, gx, gy, gz, row + gx);
        }
}

}  // namespace model
}  // namespace vpx
