// vpx_kernels.hip — gfx950 kernels and the C-ABI of libvpx_hip.so (include/vpx.h).
//
// Kernels:
//   k_nearest / k_shade / k_shadow / k_finish   the frame as a wavefront of small kernels
//                                 per bounce level (vpx_wavefront.hpp); one lane per pixel,
//                                 16x16-pixel tiles per 256-thread workgroup (8x8 pixels per wave)
//   composite_tiles               rank-0 unpack + accumulate + tonemap of gathered tiles.
//   composite_rgb8                rank-0 unpack of gathered RGB8 tiles (sharded accumulator).
//   find_nearest_k / is_occluded_k / trace_k   per-ray unit entries.
//   k_cast_lane / k_cast_occluded_lane / k_cast_pool / k_cast_occluded_pool   ray batches in device
//                                 memory (vpx_cast_*): one thread per ray, or persistent waves that refill.
//   tiled_world_k / checksum_k    world generator and grid checksum.
//   model_gather_k / model_random_k   the model loaders' placement (vpx_model.hpp).
//   smoke_gen_k / noise_mark_k / noise_scan_k / noise_draw_k   the noise generators (vpx_noise.hpp).
//   brush_k                       one brush edit (vpx_brush.hpp).
//   stamp_k / capture_k           one model stamp (vpx_stamp.hpp); a box of a grid into a model.
//   k_plane_key / k_atrous_lds / k_atrous_gather   the plane-keyed denoise (vpx_denoise.hpp).
//   k_reproject_ids               the plane-keyed temporal reprojection (vpx_reproject.hpp).
//   k_reproject_moments / k_var_estimate / k_atrous_var_lds / k_atrous_var_gather   the variance-guided
//                                 denoise: moments through the reprojection (vpx_denoise_var.hpp).
//   refresh_l1_k / df_mark_k / df_diag_k / df_planes_box_k / axis_box_k / wide_box_k   the
//                                 region-local level refresh after an edit (refresh_levels).
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <array>
#include <atomic>
#include <initializer_list>
#include <utility>
#include <vector>

#include "vpx_wavefront.hpp"
#include "vpx_model.hpp"
#include "vpx_noise.hpp"
#include "vpx_brush.hpp"
#include "vpx_stamp.hpp"
#include "vpx_denoise.hpp"
#include "vpx_denoise_var.hpp"
#include "vpx_reproject.hpp"

using namespace vpx;

namespace {

constexpr int kTile = 16;  // 16x16 pixels per tile / 256-thread workgroup
#ifndef VPX_SPLIT_PRIMARY
#define VPX_SPLIT_PRIMARY 1  // multi-volume primary rays: lean world walk + instance pass (k_instances)
#endif
#ifndef VPX_DEFER_INSTANCES
#define VPX_DEFER_INSTANCES 1  // depth 0: the world head shades the paths no instance can change (DEFER)
#endif
#ifndef VPX_LANE_TAIL
#define VPX_LANE_TAIL 1  // frames in flight blend in their own tail launch where they have one (lane_tail_ok)
#endif
#ifndef VPX_LEVEL_FORK
#define VPX_LEVEL_FORK 1  // launch_render: a level's bounce walks beside its shadow walks
#endif
// k_tail: frames of at least VPX_TAIL_MIN_DEPTH bounces run their levels from VPX_TAIL_LEVEL on
// in one launch (0: off).
#ifndef VPX_LANE_DOUBLE
#define VPX_LANE_DOUBLE 1  // frames in flight: two sample buffers per lane (lane_render)
#endif
#ifndef VPX_TAIL_LEVEL
#define VPX_TAIL_LEVEL 7
#endif
#ifndef VPX_TAIL_MIN_DEPTH
#define VPX_TAIL_MIN_DEPTH 8
#endif
constexpr int kThreads = 256;
#ifndef VPX_REPROJECT_PREKEY
#define VPX_REPROJECT_PREKEY 0  // vpx_reproject_ids reads the previous ids themselves (1: k_plane_key's keys)
#endif
#ifndef VPX_DENOISE_LDS
#define VPX_DENOISE_LDS 1  // denoise steps 1 and 2 stage tile + halo in LDS (0: every step gathers from global memory)
#endif

// One tile per workgroup.  Several tiles per workgroup with their loads issued together
// measured within noise (round 3, four interleaved runs, ms per step: C1 0.5829-0.5888 with 1,
// 0.5808-0.5907 with 2, 0.5780-0.5849 with 4, 0.5847-0.6010 with 8; C3 3.689-3.699 with 1,
// 3.674-3.711 with 4): the blend is not what a frame in flight waits for.
__global__ __launch_bounds__(kThreads) void composite_tiles(FrameArgs f, const float4* __restrict__ gathered,
                                                            float4* __restrict__ accum, uint32_t* __restrict__ rgb8) {
    const uint32_t tile = blockIdx.x;
    uint32_t lx, ly;
    tile_lane_xy(threadIdx.x, lx, ly);
    const uint32_t x = (tile % f.tiles_x) * kTile + lx;
    const uint32_t y = (tile / f.tiles_x) * kTile + ly;
    if (x >= f.width || y >= f.height) return;
    const uint32_t r = tile % f.n_ranks, j = tile / f.n_ranks;
    const float4 s = gathered[((uint64_t)r * f.tiles_per_rank + j) * (kTile * kTile) + threadIdx.x];
    const uint64_t p = (uint64_t)y * f.width + x;
    const float4 a = blend(accum[p], mk(s.x, s.y, s.z), f.weight, f.inv_weight);
    accum[p] = a;
    if (rgb8) rgb8[p] = tonemap_pack(a);
}

// A rank's packed frame folded into its packed accumulator + RGB8 (the frames-in-flight form
// of k_finish<kFinishPackedAccum>: the same blend and tonemap of the same sample, in frame order).
__global__ __launch_bounds__(kThreads) void blend_packed(FrameArgs f, const float4* __restrict__ sample,
                                                         float4* __restrict__ accum, uint32_t* __restrict__ rgb8, uint32_t P) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    uint32_t x, y;
    if (path_pixel(f, p, x, y)) {
        const float4 s = sample[p];
        const float4 a = blend(accum[p], mk(s.x, s.y, s.z), f.weight, f.inv_weight);
        accum[p] = a;
        rgb8[p] = tonemap_pack(a);
    } else {
        accum[p] = make_float4(0.f, 0.f, 0.f, 0.f);
        rgb8[p] = 0u;
    }
}

// An accumulation window's samples (frame b of the chain at [b*T*256, (b+1)*T*256)) folded
// into the accumulator in frame order: per pixel the same blend of the same samples as B
// calls of k_finish / composite_tiles / blend_packed, and the tonemap of the last.  image:
// the one-GPU image (accum/rgb8 indexed by pixel); else a rank's packed accumulator.
__global__ __launch_bounds__(kThreads) void blend_window(FrameArgs f, const float4* __restrict__ sample, uint32_t B,
                                                         WindowWeights ww, int image, float4* __restrict__ accum,
                                                         uint32_t* __restrict__ rgb8) {
    const uint32_t T = f.batch_tiles;
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    uint32_t x, y;
    const bool valid = path_pixel(f, p, x, y);
    if (image && !valid) return;
    const uint64_t a_at = image ? (uint64_t)y * f.width + x : p;
    if (!valid) {
        accum[a_at] = make_float4(0.f, 0.f, 0.f, 0.f);
        rgb8[a_at] = 0u;
        return;
    }
    float4 a = accum[a_at];
    for (uint32_t b = 0; b < B; ++b) {
        const float4 s = sample[((uint64_t)b * T << 8) + p];
        a = blend(a, mk(s.x, s.y, s.z), ww.w[b], ww.iw[b]);
    }
    accum[a_at] = a;
    if (rgb8) rgb8[a_at] = tonemap_pack(a);
}

// Rank-0 scatter of the gathered packed RGB8 tiles (sharded-accumulator flow).
__global__ __launch_bounds__(kThreads) void composite_rgb8(FrameArgs f, const uint32_t* __restrict__ gathered,
                                                           uint32_t* __restrict__ rgb8) {
    const uint32_t tile = blockIdx.x;
    uint32_t lx, ly;
    tile_lane_xy(threadIdx.x, lx, ly);
    const uint32_t x = (tile % f.tiles_x) * kTile + lx;
    const uint32_t y = (tile / f.tiles_x) * kTile + ly;
    if (x >= f.width || y >= f.height) return;
    const uint32_t r = tile % f.n_ranks, j = tile / f.n_ranks;
    rgb8[(uint64_t)y * f.width + x] = gathered[((uint64_t)r * f.tiles_per_rank + j) * (kTile * kTile) + threadIdx.x];
}

// ------------------------------------------------------------------ unit entries
__device__ __forceinline__ Ray ray_from(const vpx_ray& in) {
    Ray r = make_ray(ld3(in.origin), ld3(in.direction));
    r.t = in.tmax;
    r.inside = in.inside_glass != 0;
    return r;
}

__global__ void find_nearest_k(SceneView sv, const vpx_ray* rays, uint32_t n, vpx_hit* hits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r = ray_from(rays[i]);
    Counters k{0u, 0u, 0u};
    const int32_t vox = find_nearest(sv, r, k);
    vpx_hit h;
    h.t = r.t;
    h.normal[0] = r.N.x, h.normal[1] = r.N.y, h.normal[2] = r.N.z;
    h.vox_index = vox;
    h.material = r.mat;
    h.cells = k.cells;
    h.inside_glass = r.inside ? 1u : 0u;
    hits[i] = h;
}

__global__ void is_occluded_k(SceneView sv, const vpx_ray* rays, uint32_t n, uint8_t* occ) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Ray r = ray_from(rays[i]);
    Counters k{0u, 0u, 0u};
    occ[i] = is_occluded(sv, r, k) ? 1 : 0;
}

// The filtered unit entries (vpx_find_nearest_filtered / vpx_is_occluded_filtered).
// VPX_QUERY_RAW_DIRECTION: Ray(O, D, rD, Dsign, len) (scene.cpp:29-37) takes D as given; rD and
// Dsign are formed per volume here, from the object-space D.
__device__ __forceinline__ Ray ray_from(const vpx_ray& in, uint32_t flags) {
    Ray r = ray_from(in);
    if (flags & VPX_QUERY_RAW_DIRECTION) r.D = ld3(in.direction);
    return r;
}

__global__ void find_nearest_filtered_k(SceneView sv, const vpx_ray* rays, uint32_t n, vpx_ray_filter f, vpx_hit* hits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r = ray_from(rays[i], f.flags);
    Counters k{0u, 0u, 0u};
    const int32_t vox = find_nearest_filtered(sv, r, k, f.first_volume, f.mat_lo, f.mat_hi, !(f.flags & VPX_QUERY_NO_SHAPES));
    vpx_hit h;
    h.t = r.t;
    h.normal[0] = r.N.x, h.normal[1] = r.N.y, h.normal[2] = r.N.z;
    h.vox_index = vox;
    h.material = r.mat;
    h.cells = k.cells;
    h.inside_glass = r.inside ? 1u : 0u;
    hits[i] = h;
}

__global__ void is_occluded_filtered_k(SceneView sv, const vpx_ray* rays, uint32_t n, vpx_ray_filter f, uint8_t* occ) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const Ray r = ray_from(rays[i], f.flags);
    Counters k{0u, 0u, 0u};
    occ[i] = is_occluded(sv, r, k, f.first_volume, !(f.flags & VPX_QUERY_NO_SHAPES)) ? 1 : 0;
}

// The hit-cell entries (vpx_find_nearest_cells / vpx_pick_pixel / vpx_render_ids): the filtered
// FindNearest in its CELLS form, one walk for the hit record and the cell record.
__device__ __forceinline__ vpx_hit cells_query(const SceneView& sv, Ray& r, const vpx_ray_filter& f, vpx_hit_cell& cell) {
    Counters k{0u, 0u, 0u};
    HitCell hc;
    const int32_t vox = find_nearest_filtered<NearestWalk, true>(
        sv, r, k, f.first_volume, f.mat_lo, f.mat_hi, !(f.flags & VPX_QUERY_NO_SHAPES), &hc);
    cell = hit_cell_record(sv, vox, hc);
    vpx_hit h;
    h.t = r.t;
    h.normal[0] = r.N.x, h.normal[1] = r.N.y, h.normal[2] = r.N.z;
    h.vox_index = vox;
    h.material = r.mat;
    h.cells = k.cells;
    h.inside_glass = r.inside ? 1u : 0u;
    return h;
}

__global__ void find_nearest_cells_k(SceneView sv, const vpx_ray* rays, uint32_t n, vpx_ray_filter f, vpx_hit* hits,
                                     vpx_hit_cell* cells) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r = ray_from(rays[i], f.flags);
    vpx_hit_cell c;
    hits[i] = cells_query(sv, r, f, c);
    cells[i] = c;
}

// Pixel (x, y)'s ray: Camera::GetPrimaryRayNoDOF, exact in both arithmetic modes (f.flags holds
// kFlagReproject and neither AA nor DOF, so the generator is never drawn from).
__device__ __forceinline__ vpx_hit pixel_query(const SceneView& sv, const FrameArgs& f, const vpx_ray_filter& flt, uint32_t x,
                                               uint32_t y, vpx_hit_cell& cell) {
    Rng g{0u};
    Ray r = primary_ray(f, x, y, g, sv.x86);
    return cells_query(sv, r, flt, cell);
}

__global__ void pick_pixel_k(SceneView sv, FrameArgs f, vpx_ray_filter flt, uint32_t x, uint32_t y, vpx_hit* hit,
                             vpx_hit_cell* cell) {
    vpx_hit_cell c;
    *hit = pixel_query(sv, f, flt, x, y, c);
    *cell = c;
}

// The ID pass: one lane per pixel, a 16x16 tile per workgroup in the frame kernels' 8x8-quadrant
// lane order (tile_lane_xy: a wave's rays leave from one 8x8 block, so its lanes stay in the same
// bricks and its walk phases stay full); lanes outside the image leave before the walk, whose
// ballots count active lanes only; one 16-byte store per pixel.
__global__ __launch_bounds__(kThreads) void k_ids(SceneView sv, FrameArgs f, vpx_ray_filter flt, uint4* __restrict__ ids) {
    uint32_t lx, ly;
    tile_lane_xy(threadIdx.x, lx, ly);
    const uint32_t x = (blockIdx.x % f.tiles_x) * kTile + lx;
    const uint32_t y = (blockIdx.x / f.tiles_x) * kTile + ly;
    if (x >= f.width || y >= f.height) return;
    vpx_hit_cell c;
    const vpx_hit h = pixel_query(sv, f, flt, x, y, c);
    const uint32_t face = (c.flags & VPX_CELL_FACE) ? 1u + 2u * ((c.flags >> 8) & 3u) + ((c.flags >> 10) & 1u) : 0u;
    uint4 o;
    o.x = __float_as_uint(h.t);
    o.y = ((uint32_t)(h.vox_index + 2) & 0xffffu) | (h.material & 255u) << 16 | face << 24;
    o.z = (uint32_t)c.cell[0] | (uint32_t)c.cell[1] << 16;
    o.w = (uint32_t)c.cell[2];
    ids[(uint64_t)y * f.width + x] = o;
}

// ------------------------------------------------------------------ ray batches in device memory
// vpx_cast_nearest / vpx_cast_occluded: the filtered queries on rays and records that already
// live on the device, queued on the context's stream like k_ids.
// Per-lane form: the unit kernels' bodies (find_nearest_filtered_k / find_nearest_cells_k /
// is_occluded_filtered_k) on device pointers, one thread per ray, every scene and filter.
template <bool CELLS>
__global__ __launch_bounds__(kThreads) void k_cast_lane(SceneView sv, const vpx_ray* __restrict__ rays, uint32_t n,
                                                        vpx_ray_filter f, vpx_hit* __restrict__ hits,
                                                        vpx_hit_cell* __restrict__ cells) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    Ray r = ray_from(rays[i], f.flags);
    if (CELLS) {
        vpx_hit_cell c;
        hits[i] = cells_query(sv, r, f, c);
        cells[i] = c;
    } else {
        Counters k{0u, 0u, 0u};
        const int32_t vox = find_nearest_filtered(sv, r, k, f.first_volume, f.mat_lo, f.mat_hi, !(f.flags & VPX_QUERY_NO_SHAPES));
        vpx_hit h;
        h.t = r.t;
        h.normal[0] = r.N.x, h.normal[1] = r.N.y, h.normal[2] = r.N.z;
        h.vox_index = vox;
        h.material = r.mat;
        h.cells = k.cells;
        h.inside_glass = r.inside ? 1u : 0u;
        hits[i] = h;
    }
}

__global__ __launch_bounds__(kThreads) void k_cast_occluded_lane(SceneView sv, const vpx_ray* __restrict__ rays, uint32_t n,
                                                                 vpx_ray_filter f, uint8_t* __restrict__ occ) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const Ray r = ray_from(rays[i], f.flags);
    Counters k{0u, 0u, 0u};
    occ[i] = is_occluded(sv, r, k, f.first_volume, !(f.flags & VPX_QUERY_NO_SHAPES)) ? 1 : 0;
}

// Pool form (batches that visit exactly one volume, the scene's last: first_volume == count - 1).
// The halves of find_nearest_filtered's visit of that volume around the walk: the walk state of
// ray `in` (false: the cull or Setup3DDDA refuses it, no cell is read), and the records from the
// finished walk.  The end re-reads the ray (as nearest_end_v does), so only the walk state, the
// bound and the cell counter live across the walk.
__device__ __forceinline__ bool cast_nearest_begin(const SceneView& sv, const vpx_volume& vol, uint32_t vi, uint32_t gn,
                                                   const vpx_ray& in, uint32_t flags, skip::Walk& wk, float& bound) {
    const Ray r = ray_from(in, flags);
    bound = r.t;
    ORay o;
    o.D = xform_vec_ssem(r.D, vol.inv_matrix);
    if (!(sv.x86.tab && (rcp_nan(o.D.x) || rcp_nan(o.D.y) || rcp_nan(o.D.z))) &&
        misses_volume_u(sv.vbounds, vi, r.O, world_inv(r.D), r.t))
        return false;
    o.O = xform_pos_ssem(r.O, vol.inv_matrix);
    o.rD = nearest_rd(o.D, sv.x86);
    Dda s;
    if (!dda_setup(vol, gn, o, s)) return false;
    wk = to_walk(s);
    return true;
}
template <bool CELLS>
__device__ __forceinline__ void cast_nearest_end(const SceneView& sv, const vpx_volume& vol, uint32_t vi, uint32_t gn,
                                                 const vpx_ray& in, const vpx_ray_filter& f, const skip::Walk& wk, bool hit,
                                                 uint32_t mat, int last, uint32_t ncells, vpx_hit* hit_out,
                                                 vpx_hit_cell* cell_out) {
    Ray r = ray_from(in, f.flags);
    int32_t vox = -2;
    if (hit) {
        r.t = wk.t;
        ORay o;
        o.O = xform_pos_ssem(r.O, vol.inv_matrix);
        o.D = xform_vec_ssem(r.D, vol.inv_matrix);
        r.N = normal_voxel(o, r.t, gn, vol.matrix);
        r.mat = mat;
        vox = (int32_t)vi;
    }
    if (!(f.flags & VPX_QUERY_NO_SHAPES) && (sv.num_spheres | sv.num_triangles)) {
        Ray sh = make_ray(r.O, r.D);
        for (uint32_t i = 0; i < sv.num_spheres; ++i) sphere_hit(sv.spheres[i], sh);
        for (uint32_t i = 0; i < sv.num_triangles; ++i) tri_hit(sv.triangles[i], sh);
        if (r.t > sh.t) {
            r.t = sh.t;
            r.mat = sh.mat;
            r.N = sh.N;
            r.inside = sh.inside;
            vox = -1;
        }
    }
    vpx_hit h;
    h.t = r.t;
    h.normal[0] = r.N.x, h.normal[1] = r.N.y, h.normal[2] = r.N.z;
    h.vox_index = vox;
    h.material = r.mat;
    h.cells = ncells;
    h.inside_glass = r.inside ? 1u : 0u;
    *hit_out = h;
    if (CELLS) {  // hit_cell_record's words, as two 16-byte stores
        int4 a = make_int4(0, 0, 0, 0), b = make_int4(0, 0, 0, 0);
        if (vox >= 0) {
            a = make_int4((int32_t)wk.X, (int32_t)wk.Y, (int32_t)wk.Z, (int32_t)vol.grid_id);
            uint32_t fl = VPX_CELL_HIT;
            if (last >= 0) {
                const int32_t step = last == 0 ? wk.sx : (last == 1 ? wk.sy : wk.sz);
                b = make_int4(a.x - (last == 0 ? step : 0), a.y - (last == 1 ? step : 0), a.z - (last == 2 ? step : 0), 0);
                const int32_t fc = last == 0 ? b.x : (last == 1 ? b.y : b.z);
                fl |= VPX_CELL_FACE | (uint32_t)last << 8 | (step < 0 ? 1u : 0u) << 10 |
                      (fc >= 0 && fc < (int32_t)gn ? VPX_CELL_FACE_IN : 0u);
            }
            b.w = (int32_t)fl;
        }
        int4* out = reinterpret_cast<int4*>(cell_out);
        out[0] = a;
        out[1] = b;
    }
}

// Waves per SIMD of the cast pools: 5 (96 VGPRs, as k_nearest_pool); the hit-cell form carries
// the last step's axis through the walk as well and spills 24 to 32 VGPRs there, so it takes 4.
#ifndef VPX_WPE_CAST
#define VPX_WPE_CAST 5
#endif
#ifndef VPX_WPE_CAST_CELLS
#define VPX_WPE_CAST_CELLS 4
#endif
// FindNearest (filtered) for a device batch on persistent waves that refill their finished lanes:
// k_nearest_pool's scheme with the rays taken from the batch itself, kPoolChunk per grab, each
// lane under its own bound (the ray's tmax).  A lane that hit an excepted cell takes the cell's
// leaving event (find_nearest_filtered's pass-through) and stays in the walk, so the pool needs
// no re-entry rounds of its own.  Every ray is walked by exactly the per-lane sequence of
// find_nearest_filtered's visit of the volume (same cells, same counts, same records); a lane's
// cell counter starts from zero with each ray it takes, so the record holds that ray's cells.
// Why the outer loop ends.  Every pass of the refill loop either hands out at least one ray
// (avail > 0 and an idle lane: take >= 1), or takes one grab (the counter only grows, so at most
// `chunks` succeed per wave and the next clears `more`), or leaves; n is finite, so it leaves,
// and a last chunk of n % kPoolChunk rays is avail = n - cur, never past the batch.  A lane whose
// setup fails keeps its ray with mode kWalkMiss: the pass then goes round without the walk, the
// top writes the miss record and frees the lane, and the refill hands it another ray; each such
// round retires at least one ray, so a grab whose rays all fail setup, or a batch of misses only,
// costs n / 64 rounds at most and never enters the walk.  Otherwise every lane with a ray walks.
// While `more` holds all 64 do, the walk starts with no finished lane and returns only after
// kPoolLeave walks ended, and a lane that then passes through an excepted cell has advanced one
// cell of a finite grid: progress either way.  With `more == false` the walk runs with leave = 65,
// which no count of lanes reaches, until every lane has finished; pass-through re-entries are
// bounded by the cells on the rays; no lane takes a ray any more, each round retires the finished
// ones, and the ballot over q ends the loop.  One wave alone drains the whole batch the same way.
template <bool X86, bool CELLS>
__global__ __launch_bounds__(kPoolWg) VPX_WPE(CELLS ? VPX_WPE_CAST_CELLS : VPX_WPE_CAST) void k_cast_pool(SceneView sv_, const vpx_ray* __restrict__ rays,
                                                                           uint32_t n, vpx_ray_filter f,
                                                                           uint32_t* __restrict__ grab, uint32_t waves,
                                                                           vpx_hit* __restrict__ hits,
                                                                           vpx_hit_cell* __restrict__ cells) {
    if (blockIdx.x * (kPoolWg / 64u) + (threadIdx.x >> 6) >= waves) return;  // max_waves: the last workgroup's spare waves
    const SceneView sv = arith_view<X86>(sv_);
    const uint32_t vi = sv.num_volumes - 1u;
    const vpx_volume* vol = uni_ptr(&sv.volumes[vi]);
    const DevGrid g = sv.grids[vol->grid_id];
    const skip::GridView gv = grid_view(g);
    const uint32_t chunks = (n + kPoolChunk - 1u) / kPoolChunk;
    skip::Walk wk;
    uint32_t q = ~0u;  // the ray this lane walks (~0u: none)
    int mode = kWalkMiss, last = -1;
    float bound = 0.f;
    uint32_t ncells = 0u;
    uint32_t avail = 0u, cur = 0u;  // grabbed rays not yet handed out, and where they start
    bool more = true;               // rays may be left in the batch
    uint32_t line = pool_line0();
    for (;;) {
        if (q != ~0u && mode >= kWalkMiss) {
            uint32_t mat = kNone;
            if (mode == kWalkHit) {
                mat = gv.cells[(uint64_t)wk.X + (uint64_t)wk.Y * gv.n + (uint64_t)wk.Z * ((uint64_t)gv.n * gv.n)];
                if (mat >= f.mat_lo && mat <= f.mat_hi) {  // scene.cpp:826: passed through
                    const uint32_t ox = wk.X, oy = wk.Y;
                    const bool on = skip::step1<BounceWalk::min2>(wk, gv.n);
                    if (CELLS) last = stepped_axis(wk, ox, oy);
                    mode = on ? kWalkStep : kWalkMiss;
                }
            }
            if (mode >= kWalkMiss) {  // finished: its records
                asm volatile("" ::: "memory");  // re-read the ray instead of keeping it live
                cast_nearest_end<CELLS>(sv, *vol, vi, g.n, rays[q], f, wk, mode == kWalkHit, mat, last, ncells, &hits[q],
                                        CELLS ? &cells[q] : nullptr);
                q = ~0u;
            }
        }
        while (more) {
            const uint64_t idle = __ballot(q == ~0u);
            if (!idle) break;
            if (avail == 0u) {
                const uint32_t gi = pool_grab(grab, chunks, line);
                if (gi == ~0u) {
                    more = false;
                    break;
                }
                cur = gi * kPoolChunk;
                avail = min(kPoolChunk, n - cur);
                continue;
            }
            const uint32_t take = min((uint32_t)__popcll(idle), avail);
            const uint32_t r = lane_rank(idle);
            if (q == ~0u && r < take) {
                q = cur + r;
                ncells = 0u;
                last = -1;
                mode = cast_nearest_begin(sv, *vol, vi, g.n, rays[q], f.flags, wk, bound) ? kWalkStep : kWalkMiss;
            }
            cur += take;
            avail -= take;
        }
        if (!__ballot(q != ~0u)) break;  // the batch is done and every lane is done
        // lanes whose setup failed: their miss records (above) and other rays in their place first
        if (__ballot(q != ~0u && mode >= kWalkMiss)) continue;
        walk_wave<BounceWalk, true, CELLS>(gv, wk, bound, ncells, &mode, more ? kPoolLeave : 65u, &last);
    }
}

// IsOccluded (filtered: one visited volume, the shapes unless VPX_QUERY_NO_SHAPES) for a device
// batch, on the same pool: is_occluded's visit of the volume per lane (scalar transforms, exact
// 1 / D in both arithmetic modes), then its shape tests for the rays the volume left unoccluded.
// The outer loop ends as k_cast_pool's does (no pass-through here).
__global__ __launch_bounds__(kPoolWg) VPX_WPE(VPX_WPE_CAST) void k_cast_occluded_pool(SceneView sv, const vpx_ray* __restrict__ rays,
                                                                                    uint32_t n, vpx_ray_filter f,
                                                                                    uint32_t* __restrict__ grab, uint32_t waves,
                                                                                    uint8_t* __restrict__ occ) {
    if (blockIdx.x * (kPoolWg / 64u) + (threadIdx.x >> 6) >= waves) return;
    const uint32_t vi = sv.num_volumes - 1u;
    const vpx_volume* vol = uni_ptr(&sv.volumes[vi]);
    const DevGrid g = sv.grids[vol->grid_id];
    const skip::GridView gv = grid_view(g);
    const uint32_t chunks = (n + kPoolChunk - 1u) / kPoolChunk;
    const bool shapes = !(f.flags & VPX_QUERY_NO_SHAPES);
    auto finish = [&](uint32_t i, bool hit) {
        bool o = hit;
        if (!o && shapes) {
            const Ray r = ray_from(rays[i], f.flags);
            for (uint32_t j = 0; j < sv.num_spheres && !o; ++j) o = sphere_is_hit(sv.spheres[j], r);
            for (uint32_t j = 0; j < sv.num_triangles && !o; ++j) o = tri_is_hit(sv.triangles[j], r);
        }
        occ[i] = o ? 1 : 0;
    };
    skip::Walk wk;
    uint32_t q = ~0u;
    int mode = kWalkMiss;
    float bound = 0.f;
    uint32_t ncells = 0u;
    uint32_t avail = 0u, cur = 0u;
    bool more = true;
    uint32_t line = pool_line0();
    for (;;) {
        if (q != ~0u && mode >= kWalkMiss) {
            asm volatile("" ::: "memory");
            finish(q, mode == kWalkHit);
            q = ~0u;
        }
        while (more) {
            const uint64_t idle = __ballot(q == ~0u);
            if (!idle) break;
            if (avail == 0u) {
                const uint32_t gi = pool_grab(grab, chunks, line);
                if (gi == ~0u) {
                    more = false;
                    break;
                }
                cur = gi * kPoolChunk;
                avail = min(kPoolChunk, n - cur);
                continue;
            }
            const uint32_t take = min((uint32_t)__popcll(idle), avail);
            const uint32_t r = lane_rank(idle);
            if (q == ~0u && r < take) {
                q = cur + r;
                const Ray ry = ray_from(rays[q], f.flags);
                bound = ry.t;
                bool ok = !misses_volume_u(sv.vbounds, vi, ry.O, world_inv(ry.D), ry.t);
                if (ok) {
                    ORay o;
                    o.O = xform_pos(ry.O, vol->inv_matrix);
                    o.D = xform_vec(ry.D, vol->inv_matrix);
                    o.rD = mk(__fdiv_rn(1.0f, o.D.x), __fdiv_rn(1.0f, o.D.y), __fdiv_rn(1.0f, o.D.z));
                    Dda s;
                    ok = dda_setup(*vol, g.n, o, s);
                    if (ok) wk = to_walk(s);
                }
                mode = ok ? kWalkStep : kWalkMiss;  // a miss: the volume reads no cell, the shapes answer
            }
            cur += take;
            avail -= take;
        }
        if (!__ballot(q != ~0u)) break;
        if (__ballot(q != ~0u && mode >= kWalkMiss)) continue;  // setup failed: their bytes first, as k_cast_pool
        walk_wave<ShadowPoolWalk, true>(gv, wk, bound, ncells, &mode, more ? kPoolLeave : 65u);
    }
}

// ------------------------------------------------------------------ plane-keyed denoise
// vpx_denoise_ids (vpx_denoise.hpp holds the definition and the arithmetic).  Images are
// row-major float4[W*H]; a workgroup filters one 16x16 tile, lane t at (t & 15, t >> 4): a wave's
// loads are four runs of 256 contiguous bytes (the frame kernels' 8x8-quadrant lane order measured
// the same: DESIGN.md §4).
struct DenoiseArgs {
    uint32_t width, height, tiles_x;
    int32_t step;
    float inv_sigma;
};

// ids -> keys: one 8-byte store per pixel.
__global__ __launch_bounds__(kThreads) void k_plane_key(uint32_t pixels, const uint4* __restrict__ ids,
                                                        uint2* __restrict__ keys) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= pixels) return;
    const uint4 r = ids[p];
    const denoise::Key k = denoise::plane_key(r.y, r.z, r.w);
    keys[p] = make_uint2(k.a, k.b);
}

__device__ __forceinline__ void denoise_store(uint64_t q, float4 o, float4* __restrict__ D,
                                              uint32_t* __restrict__ rgb8) {
    D[q] = o;
    if (rgb8) rgb8[q] = tonemap_pack(o);  // the last pass only
}

// Steps 1 and 2: the tile and its halo of 2 * STEP pixels (20x20, 24x24) staged in LDS, keys and
// colours (9.6 / 13.8 KiB).  A pixel outside the image is staged with the invalid key, which
// matches no valid one, so the tap loop needs no bounds test; a colour is loaded only under a
// valid key.
template <bool LUM, int STEP>
__global__ __launch_bounds__(kThreads) void k_atrous_lds(DenoiseArgs a, const uint2* __restrict__ keys,
                                                         const float4* __restrict__ S, float4* __restrict__ D,
                                                         uint32_t* __restrict__ rgb8) {
    constexpr int R = 2 * STEP, DIM = kTile + 2 * R;
    __shared__ uint2 lk[DIM * DIM];
    __shared__ float4 lc[DIM * DIM];
    const int tx0 = (int)(blockIdx.x % a.tiles_x) * kTile, ty0 = (int)(blockIdx.x / a.tiles_x) * kTile;
    for (int e = threadIdx.x; e < DIM * DIM; e += kThreads) {
        const int gx = tx0 - R + e % DIM, gy = ty0 - R + e / DIM;
        uint2 k = make_uint2(0u, 0u);
        if (gx >= 0 && gy >= 0 && gx < (int)a.width && gy < (int)a.height) {
            const uint64_t p = (uint64_t)gy * a.width + (uint32_t)gx;
            k = keys[p];
            if (k.y) lc[e] = S[p];
        }
        lk[e] = k;
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const uint32_t x = tx0 + lx, y = ty0 + ly;
    if (x >= a.width || y >= a.height) return;
    const uint64_t q = (uint64_t)y * a.width + x;
    const int eq = (ly + R) * DIM + lx + R;
    const uint2 kq = lk[eq];
    if (!kq.y) {
        denoise_store(q, S[q], D, rgb8);
        return;
    }
    const float4 cq = lc[eq];
    const float lq = LUM ? denoise::lum(cq.x, cq.y, cq.z) : 0.f;
    denoise::Sum s;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int e = eq + j * STEP * DIM + i * STEP;
            const uint2 k = lk[e];
            if (k.x == kq.x && k.y == kq.y) {
                const float4 c = lc[e];
                denoise::tap<LUM>(s, denoise::base_weight(j, i), c.x, c.y, c.z, lq, a.inv_sigma);
            }
        }
    denoise_store(q, make_float4(s.r / s.w, s.g / s.w, s.b / s.w, cq.w), D, rgb8);
}

// Steps 4 and up (the halo outgrows the tile): 25 taps gathered from global memory through L2.
// First the 25 keys, from clamped addresses so that the loads need no branch and go out together,
// folded into a match mask; then the colours of the matching taps only.
template <bool LUM>
__global__ __launch_bounds__(kThreads) void k_atrous_gather(DenoiseArgs a, const uint2* __restrict__ keys,
                                                            const float4* __restrict__ S, float4* __restrict__ D,
                                                            uint32_t* __restrict__ rgb8) {
    const int x = (int)(blockIdx.x % a.tiles_x) * kTile + (int)(threadIdx.x & 15);
    const int y = (int)(blockIdx.x / a.tiles_x) * kTile + (int)(threadIdx.x >> 4);
    const int W = (int)a.width, H = (int)a.height;
    if (x >= W || y >= H) return;
    const uint64_t q = (uint64_t)y * a.width + (uint32_t)x;
    const uint2 kq = keys[q];
    const float4 cq = S[q];
    if (!kq.y) {
        denoise_store(q, cq, D, rgb8);
        return;
    }
    uint32_t match = 0u;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int rx = x + i * a.step, ry = y + j * a.step;
            const bool in = rx >= 0 && ry >= 0 && rx < W && ry < H;
            const int cx = min(max(rx, 0), W - 1), cy = min(max(ry, 0), H - 1);
            const uint2 k = keys[(uint64_t)cy * a.width + (uint32_t)cx];
            match |= (uint32_t)(in && k.x == kq.x && k.y == kq.y) << ((j + 2) * 5 + i + 2);
        }
    const float lq = LUM ? denoise::lum(cq.x, cq.y, cq.z) : 0.f;
    denoise::Sum s;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i)
            if (match >> ((j + 2) * 5 + i + 2) & 1u) {  // in the image: the mask says so
                const float4 c = S[(uint64_t)(y + j * a.step) * a.width + (uint32_t)(x + i * a.step)];
                denoise::tap<LUM>(s, denoise::base_weight(j, i), c.x, c.y, c.z, lq, a.inv_sigma);
            }
    denoise_store(q, make_float4(s.r / s.w, s.g / s.w, s.b / s.w, cq.w), D, rgb8);
}

template <bool LUM>
void launch_atrous(hipStream_t st, uint32_t tiles, const DenoiseArgs& a, const uint2* keys, const float4* src,
                          float4* dst, uint32_t* rgb8) {
#if VPX_DENOISE_LDS
    if (a.step == 1) {
        hipLaunchKernelGGL((k_atrous_lds<LUM, 1>), dim3(tiles), dim3(kThreads), 0, st, a, keys, src, dst, rgb8);
        return;
    }
    if (a.step == 2) {
        hipLaunchKernelGGL((k_atrous_lds<LUM, 2>), dim3(tiles), dim3(kThreads), 0, st, a, keys, src, dst, rgb8);
        return;
    }
#endif
    hipLaunchKernelGGL((k_atrous_gather<LUM>), dim3(tiles), dim3(kThreads), 0, st, a, keys, src, dst, rgb8);
}

// ------------------------------------------------------------------ variance-guided denoise
// vpx_denoise_var (vpx_denoise_var.hpp holds the definition and the arithmetic).  The images of the
// passes are float4 whose .w is the variance, so a tap is one 16-byte load and the LDS tiles are
// k_atrous_lds' (keys + float4); the prefilter's 3x3 lies inside the halo (R >= 2).  Only the last
// pass (restore != NULL) puts in.w back.
struct DenoiseVarArgs {
    uint32_t width, height, tiles_x;
    int32_t step;
    float sigma_v, epsilon, min_history;
};

// Step V: V0 = (in.rgb, var0).  The temporal arm reads the pixel's own moments; the spatial arm
// gathers the 5x5 neighbourhood: the keys first, from clamped addresses, folded into a match
// mask, then the moments of the matching taps only (mom, or the luminance of `in`).
template <bool MOM>
__global__ __launch_bounds__(kThreads) void k_var_estimate(DenoiseVarArgs a, const uint2* __restrict__ keys,
                                                           const float4* __restrict__ in,
                                                           const float2* __restrict__ mom, float4* __restrict__ V0) {
    const int x = (int)(blockIdx.x % a.tiles_x) * kTile + (int)(threadIdx.x & 15);
    const int y = (int)(blockIdx.x / a.tiles_x) * kTile + (int)(threadIdx.x >> 4);
    const int W = (int)a.width, H = (int)a.height;
    if (x >= W || y >= H) return;
    const uint64_t q = (uint64_t)y * a.width + (uint32_t)x;
    const uint2 kq = keys[q];
    const float4 cq = in[q];
    float var = 0.0f;
    auto moments = [&](uint64_t r) {
        if (MOM) {
            const float2 m = mom[r];
            return denoise_var::Mom{m.x, m.y};
        }
        const float4 c = in[r];
        return denoise_var::self_moments(c.x, c.y, c.z);
    };
    if (kq.y) {
        if (MOM && cq.w >= a.min_history) {
            var = denoise_var::temporal_var(moments(q));
        } else {
            uint32_t match = 0u;
#pragma unroll
            for (int j = -2; j <= 2; ++j)
#pragma unroll
                for (int i = -2; i <= 2; ++i) {
                    const int rx = x + i, ry = y + j;
                    const bool inside = rx >= 0 && ry >= 0 && rx < W && ry < H;
                    const int cx = min(max(rx, 0), W - 1), cy = min(max(ry, 0), H - 1);
                    const uint2 k = keys[(uint64_t)cy * a.width + (uint32_t)cx];
                    match |= (uint32_t)(inside && k.x == kq.x && k.y == kq.y) << ((j + 2) * 5 + i + 2);
                }
            denoise_var::Spatial s;
#pragma unroll
            for (int j = -2; j <= 2; ++j)
#pragma unroll
                for (int i = -2; i <= 2; ++i)
                    if (match >> ((j + 2) * 5 + i + 2) & 1u)  // in the image: the mask says so
                        denoise_var::spatial_tap(s, moments((uint64_t)(y + j) * a.width + (uint32_t)(x + i)));
            var = denoise_var::spatial_var(s);
        }
    }
    V0[q] = make_float4(cq.x, cq.y, cq.z, var);
}

__device__ __forceinline__ void denoise_var_store(uint64_t q, float4 o, float4* __restrict__ D,
                                                  const float4* __restrict__ restore, uint32_t* __restrict__ rgb8) {
    if (restore) o.w = restore[q].w;  // the last pass only
    D[q] = o;
    if (rgb8) rgb8[q] = tonemap_pack(o);
}

// Steps 1 and 2: k_atrous_lds' staging (tile + halo of 2 * STEP pixels, keys and float4s).
template <int STEP>
__global__ __launch_bounds__(kThreads) void k_atrous_var_lds(DenoiseVarArgs a, const uint2* __restrict__ keys,
                                                             const float4* __restrict__ S, float4* __restrict__ D,
                                                             const float4* __restrict__ restore,
                                                             uint32_t* __restrict__ rgb8) {
    constexpr int R = 2 * STEP, DIM = kTile + 2 * R;
    __shared__ uint2 lk[DIM * DIM];
    __shared__ float4 lc[DIM * DIM];
    const int tx0 = (int)(blockIdx.x % a.tiles_x) * kTile, ty0 = (int)(blockIdx.x / a.tiles_x) * kTile;
    for (int e = threadIdx.x; e < DIM * DIM; e += kThreads) {
        const int gx = tx0 - R + e % DIM, gy = ty0 - R + e / DIM;
        uint2 k = make_uint2(0u, 0u);
        if (gx >= 0 && gy >= 0 && gx < (int)a.width && gy < (int)a.height) {
            const uint64_t p = (uint64_t)gy * a.width + (uint32_t)gx;
            k = keys[p];
            if (k.y) lc[e] = S[p];
        }
        lk[e] = k;
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const uint32_t x = tx0 + lx, y = ty0 + ly;
    if (x >= a.width || y >= a.height) return;
    const uint64_t q = (uint64_t)y * a.width + x;
    const int eq = (ly + R) * DIM + lx + R;
    const uint2 kq = lk[eq];
    if (!kq.y) {
        denoise_var_store(q, S[q], D, restore, rgb8);
        return;
    }
    denoise_var::Pre pre;
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int e = eq + j * DIM + i;
            const uint2 k = lk[e];
            if (k.x == kq.x && k.y == kq.y) denoise_var::pre_tap(pre, denoise_var::pre_weight(j, i), lc[e].w);
        }
    const float inv = denoise_var::inv_tolerance(pre, a.sigma_v, a.epsilon);
    const float4 cq = lc[eq];
    const float lq = denoise::lum(cq.x, cq.y, cq.z);
    denoise_var::Sum s;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int e = eq + j * STEP * DIM + i * STEP;
            const uint2 k = lk[e];
            if (k.x == kq.x && k.y == kq.y) {
                const float4 c = lc[e];
                denoise_var::tap(s, denoise::base_weight(j, i), c.x, c.y, c.z, c.w, lq, inv);
            }
        }
    denoise_var_store(q, make_float4(s.r / s.w, s.g / s.w, s.b / s.w, denoise_var::out_var(s)), D, restore, rgb8);
}

// Steps 4 and up: k_atrous_gather's key-mask-then-colour scheme, plus the nine step-1 taps of the
// prefilter (their keys into a second mask, then 4 bytes of variance under a matching one).
__global__ __launch_bounds__(kThreads) void k_atrous_var_gather(DenoiseVarArgs a, const uint2* __restrict__ keys,
                                                                const float4* __restrict__ S, float4* __restrict__ D,
                                                                const float4* __restrict__ restore,
                                                                uint32_t* __restrict__ rgb8) {
    const int x = (int)(blockIdx.x % a.tiles_x) * kTile + (int)(threadIdx.x & 15);
    const int y = (int)(blockIdx.x / a.tiles_x) * kTile + (int)(threadIdx.x >> 4);
    const int W = (int)a.width, H = (int)a.height;
    if (x >= W || y >= H) return;
    const uint64_t q = (uint64_t)y * a.width + (uint32_t)x;
    const uint2 kq = keys[q];
    const float4 cq = S[q];
    if (!kq.y) {
        denoise_var_store(q, cq, D, restore, rgb8);
        return;
    }
    uint32_t match = 0u, near = 0u;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int rx = x + i * a.step, ry = y + j * a.step;
            const bool inside = rx >= 0 && ry >= 0 && rx < W && ry < H;
            const int cx = min(max(rx, 0), W - 1), cy = min(max(ry, 0), H - 1);
            const uint2 k = keys[(uint64_t)cy * a.width + (uint32_t)cx];
            match |= (uint32_t)(inside && k.x == kq.x && k.y == kq.y) << ((j + 2) * 5 + i + 2);
        }
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int rx = x + i, ry = y + j;
            const bool inside = rx >= 0 && ry >= 0 && rx < W && ry < H;
            const int cx = min(max(rx, 0), W - 1), cy = min(max(ry, 0), H - 1);
            const uint2 k = keys[(uint64_t)cy * a.width + (uint32_t)cx];
            near |= (uint32_t)(inside && k.x == kq.x && k.y == kq.y) << ((j + 1) * 3 + i + 1);
        }
    denoise_var::Pre pre;
#pragma unroll
    for (int j = -1; j <= 1; ++j)
#pragma unroll
        for (int i = -1; i <= 1; ++i)
            if (near >> ((j + 1) * 3 + i + 1) & 1u)
                denoise_var::pre_tap(pre, denoise_var::pre_weight(j, i), S[(uint64_t)(y + j) * a.width + (uint32_t)(x + i)].w);
    const float inv = denoise_var::inv_tolerance(pre, a.sigma_v, a.epsilon);
    const float lq = denoise::lum(cq.x, cq.y, cq.z);
    denoise_var::Sum s;
#pragma unroll
    for (int j = -2; j <= 2; ++j)
#pragma unroll
        for (int i = -2; i <= 2; ++i)
            if (match >> ((j + 2) * 5 + i + 2) & 1u) {  // in the image: the mask says so
                const float4 c = S[(uint64_t)(y + j * a.step) * a.width + (uint32_t)(x + i * a.step)];
                denoise_var::tap(s, denoise::base_weight(j, i), c.x, c.y, c.z, c.w, lq, inv);
            }
    denoise_var_store(q, make_float4(s.r / s.w, s.g / s.w, s.b / s.w, denoise_var::out_var(s)), D, restore, rgb8);
}

void launch_atrous_var(hipStream_t st, uint32_t tiles, const DenoiseVarArgs& a, const uint2* keys, const float4* src,
                       float4* dst, const float4* restore, uint32_t* rgb8) {
    if (a.step == 1)
        hipLaunchKernelGGL((k_atrous_var_lds<1>), dim3(tiles), dim3(kThreads), 0, st, a, keys, src, dst, restore, rgb8);
    else if (a.step == 2)
        hipLaunchKernelGGL((k_atrous_var_lds<2>), dim3(tiles), dim3(kThreads), 0, st, a, keys, src, dst, restore, rgb8);
    else
        hipLaunchKernelGGL(k_atrous_var_gather, dim3(tiles), dim3(kThreads), 0, st, a, keys, src, dst, restore, rgb8);
}

// ------------------------------------------------------------------ plane-keyed reprojection
// vpx_reproject_ids (vpx_reproject.hpp holds the definition and the arithmetic: reproject::pixel).
// One lane per pixel, a 16x16 tile per workgroup, lane t at (t & 15, t >> 4) as the denoise; the
// record and the sample are one 16-byte load each, the result one 16-byte store.  pixel() asks for
// the four previous keys from clamped addresses before any history colour, so the four loads go
// out together, and for a colour only under a tap that is in the image, weighs and has the key.
// PREKEY: the previous keys come from k_plane_key's uint2 array (8 bytes per tap, one more
// launch) instead of the ids themselves (16 bytes per tap, 12 of them used).  MOVING = false
// carries no volume table, RGB8 = false no tonemap.
template <bool MOVING, bool RGB8, bool PREKEY>
__global__ __launch_bounds__(kThreads) void k_reproject_ids(reproject::Args a, uint32_t tiles_x,
                                                            const uint4* __restrict__ ids_cur,
                                                            const void* __restrict__ prev, const float4* __restrict__ cur,
                                                            const float4* __restrict__ hist_in,
                                                            float4* __restrict__ hist_out, uint32_t* __restrict__ rgb8,
                                                            const float* __restrict__ tab,
                                                            const uint32_t* __restrict__ moved) {
    const uint32_t x = (blockIdx.x % tiles_x) * kTile + (threadIdx.x & 15u);
    const uint32_t y = (blockIdx.x / tiles_x) * kTile + (threadIdx.x >> 4);
    if (x >= a.width || y >= a.height) return;
    const uint64_t q = (uint64_t)y * a.width + x;
    const uint4 id = ids_cur[q];
    const float4 c = cur[q];
    auto prev_key = [prev](uint64_t i) {
        if (PREKEY) {
            const uint2 k = reinterpret_cast<const uint2*>(prev)[i];
            return denoise::Key{k.x, k.y};
        }
        const uint4 r = reinterpret_cast<const uint4*>(prev)[i];
        return denoise::plane_key(r.y, r.z, r.w);
    };
    auto hist = [hist_in](uint64_t i) {
        const float4 h = hist_in[i];
        return reproject::Rgbw{h.x, h.y, h.z, h.w};
    };
    const reproject::Rgbw o = reproject::pixel<MOVING>(a, x, y, reproject::Id{id.x, id.y, id.z, id.w},
                                                       reproject::Rgbw{c.x, c.y, c.z, c.w}, prev_key, hist, tab, moved);
    const float4 out = make_float4(o.r, o.g, o.b, o.w);
    hist_out[q] = out;
    if (RGB8) rgb8[q] = tonemap_pack(out);
}

template <bool MOVING, bool RGB8>
void launch_reproject(hipStream_t st, uint32_t tiles, const reproject::Args& a, uint32_t tiles_x, const uint4* ids_cur,
                      const void* prev, const float4* cur, const float4* hist_in, float4* hist_out, uint32_t* rgb8,
                      const float* tab, const uint32_t* moved) {
    hipLaunchKernelGGL((k_reproject_ids<MOVING, RGB8, VPX_REPROJECT_PREKEY != 0>), dim3(tiles), dim3(kThreads), 0, st, a,
                       tiles_x, ids_cur, prev, cur, hist_in, hist_out, rgb8, tab, moved);
}

// vpx_reproject_moments: k_reproject_ids with reproject::pixel's moments payload, 8 bytes more per
// usable tap and one 8-byte store more per pixel.
struct DeviceMoments {
    static constexpr bool on = true;
    const float2* m;
    __device__ __forceinline__ reproject::Mom operator()(uint64_t i) const {
        const float2 v = m[i];
        return reproject::Mom{v.x, v.y};
    }
};
template <bool MOVING, bool RGB8, bool PREKEY>
__global__ __launch_bounds__(kThreads) void k_reproject_moments(reproject::Args a, uint32_t tiles_x,
                                                                const uint4* __restrict__ ids_cur,
                                                                const void* __restrict__ prev,
                                                                const float4* __restrict__ cur,
                                                                const float4* __restrict__ hist_in,
                                                                const float2* __restrict__ mom_in,
                                                                float4* __restrict__ hist_out,
                                                                float2* __restrict__ mom_out, uint32_t* __restrict__ rgb8,
                                                                const float* __restrict__ tab,
                                                                const uint32_t* __restrict__ moved) {
    const uint32_t x = (blockIdx.x % tiles_x) * kTile + (threadIdx.x & 15u);
    const uint32_t y = (blockIdx.x / tiles_x) * kTile + (threadIdx.x >> 4);
    if (x >= a.width || y >= a.height) return;
    const uint64_t q = (uint64_t)y * a.width + x;
    const uint4 id = ids_cur[q];
    const float4 c = cur[q];
    auto prev_key = [prev](uint64_t i) {
        if (PREKEY) {
            const uint2 k = reinterpret_cast<const uint2*>(prev)[i];
            return denoise::Key{k.x, k.y};
        }
        const uint4 r = reinterpret_cast<const uint4*>(prev)[i];
        return denoise::plane_key(r.y, r.z, r.w);
    };
    auto hist = [hist_in](uint64_t i) {
        const float4 h = hist_in[i];
        return reproject::Rgbw{h.x, h.y, h.z, h.w};
    };
    reproject::Mom mo{0.f, 0.f};
    const reproject::Rgbw o = reproject::pixel<MOVING>(a, x, y, reproject::Id{id.x, id.y, id.z, id.w},
                                                       reproject::Rgbw{c.x, c.y, c.z, c.w}, prev_key, hist, tab, moved,
                                                       DeviceMoments{mom_in}, mo);
    const float4 out = make_float4(o.r, o.g, o.b, o.w);
    hist_out[q] = out;
    mom_out[q] = make_float2(mo.x, mo.y);
    if (RGB8) rgb8[q] = tonemap_pack(out);
}

template <bool MOVING, bool RGB8>
void launch_reproject_moments(hipStream_t st, uint32_t tiles, const reproject::Args& a, uint32_t tiles_x,
                              const uint4* ids_cur, const void* prev, const float4* cur, const float4* hist_in,
                              const float2* mom_in, float4* hist_out, float2* mom_out, uint32_t* rgb8, const float* tab,
                              const uint32_t* moved) {
    hipLaunchKernelGGL((k_reproject_moments<MOVING, RGB8, VPX_REPROJECT_PREKEY != 0>), dim3(tiles), dim3(kThreads), 0, st,
                       a, tiles_x, ids_cur, prev, cur, hist_in, mom_in, hist_out, mom_out, rgb8, tab, moved);
}

// BasicBVH::IntersectBVH (src/BVH/BasicBVH.cpp:19-70), one ray per lane.  The workgroup
// stages the whole BVH in LDS (nodes, then the triangles already permuted into tri_idx
// order, so a leaf's triangles are contiguous); the recursion (node test, then left
// subtree, then right) becomes an explicit stack that pops the left child first.  Float
// expressions keep the reference's operand order: IEEE divisions, std::min / std::max.
constexpr int kBvhStack = 64;
__global__ __launch_bounds__(256) void bvh_intersect_k(const uint32_t* __restrict__ bvh, uint32_t n_nodes,
                                                       uint32_t n_tris, const vpx_ray* rays, uint32_t n,
                                                       float* t_out) {
    extern __shared__ uint32_t lds_bvh[];
    const uint32_t words = n_nodes * 8u + n_tris * 9u;
    for (uint32_t i = threadIdx.x; i < words; i += blockDim.x) lds_bvh[i] = bvh[i];
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const vpx_bvh_node* nodes = (const vpx_bvh_node*)lds_bvh;
    const vpx_bvh_tri* tris = (const vpx_bvh_tri*)(lds_bvh + n_nodes * 8u);
    Ray r = ray_from(rays[i]);
    uint32_t stack[kBvhStack];
    int sp = 0;
    stack[sp++] = 0;
    while (sp > 0) {
        const vpx_bvh_node& nd = nodes[stack[--sp]];
        // IntersectAABB (BasicBVH.cpp:38-48)
        const float tx1 = (nd.aabb_min[0] - r.O.x) / r.D.x, tx2 = (nd.aabb_max[0] - r.O.x) / r.D.x;
        float tmin = smin(tx1, tx2), tmax = smax(tx1, tx2);
        const float ty1 = (nd.aabb_min[1] - r.O.y) / r.D.y, ty2 = (nd.aabb_max[1] - r.O.y) / r.D.y;
        tmin = smax(tmin, smin(ty1, ty2)), tmax = smin(tmax, smax(ty1, ty2));
        const float tz1 = (nd.aabb_min[2] - r.O.z) / r.D.z, tz2 = (nd.aabb_max[2] - r.O.z) / r.D.z;
        tmin = smax(tmin, smin(tz1, tz2)), tmax = smin(tmax, smax(tz1, tz2));
        if (!(tmax >= tmin && tmin < r.t && tmax > 0)) continue;
        if (nd.tri_count == 0) {  // interior: left subtree first
            stack[sp++] = nd.left_first + 1u;
            stack[sp++] = nd.left_first;
            continue;
        }
        for (uint32_t k = 0; k < nd.tri_count; ++k) {  // IntersectTri (BasicBVH.cpp:19-36)
            const vpx_bvh_tri& t = tris[nd.left_first + k];
            const f3 v0 = ld3(t.v0);
            const f3 e1 = ld3(t.v1) - v0, e2 = ld3(t.v2) - v0;
            const f3 h = cross(r.D, e2);
            const float a = dot(e1, h);
            if (a > -0.0001f && a < 0.0001f) continue;
            const float f = __fdiv_rn(1.0f, a);
            const f3 sv = r.O - v0;
            const float u = f * dot(sv, h);
            if (u < 0 || u > 1) continue;
            const f3 q = cross(sv, e1);
            const float v = f * dot(r.D, q);
            if (v < 0 || u + v > 1) continue;
            const float tt = f * dot(e2, q);
            if (tt > 0.0001f) r.t = smin(r.t, tt);
        }
    }
    t_out[i] = r.t;
}

template <int LEVELS>
__global__ __launch_bounds__(256) void trace_k(SceneView sv, const vpx_ray* rays, const uint32_t* seeds, uint32_t n, int32_t depth,
                        float* out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng g{seeds[i]};
    Counters k{0u, 0u, 0u};
    const f3 v = trace_path<LEVELS>(sv, ray_from(rays[i]), depth, g, k);
    out[3 * i] = v.x, out[3 * i + 1] = v.y, out[3 * i + 2] = v.z;
}

// vpx_trace_probe: trace_k plus the ray's player light probes (out may be null).
template <int LEVELS>
__global__ __launch_bounds__(256) void trace_probe_k(SceneView sv, const vpx_ray* rays, const uint32_t* seeds, uint32_t n,
                                                     int32_t depth, float* out, vpx_ray_probe* probes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Rng g{seeds[i]};
    Counters k{0u, 0u, 0u};
    PathProbe pp{0u, 0u, 0u};
    const f3 v = trace_path<LEVELS, true>(sv, ray_from(rays[i]), depth, g, k, &pp);
    if (out) out[3 * i] = v.x, out[3 * i + 1] = v.y, out[3 * i + 2] = v.z;
    probes[i] = vpx_ray_probe{pp.probes, pp.lit, __uint_as_float(pp.max_bits), 0u};
}

__global__ void focus_k(SceneView sv, FrameArgs f, float* out) {
    // Renderer::Tick focus ray (renderer.cpp:1987-1991): integer screen centre, no lens
    // jitter, tested against each Scene in WORLD space (no instance transform).
    const float u = (float)(f.width / 2) * __fdiv_rn(1.0f, (float)f.width);
    const float v = (float)(f.height / 2) * __fdiv_rn(1.0f, (float)f.height);
    const f3 tl = ld3(f.cam.top_left), tr = ld3(f.cam.top_right), bl = ld3(f.cam.bottom_left);
    const f3 P = (tl + (tr - tl) * u) + (bl - tl) * v;
    const f3 cp = ld3(f.cam.cam_pos);
    const f3 focal = cp + normalize(P - cp) * f.cam.focal_distance;
    Ray r = make_ray(cp, focal - cp);
    uint32_t cells = 0;
    for (uint32_t i = 0; i < sv.num_volumes; ++i) {
        const vpx_volume& vol = sv.volumes[i];
        ORay o{r.O, r.D, mk(__fdiv_rn(1.0f, r.D.x), __fdiv_rn(1.0f, r.D.y), __fdiv_rn(1.0f, r.D.z))};
        const DevGrid g = sv.grids[vol.grid_id];
        Dda s;
        if (!dda_setup(vol, g.n, o, s)) continue;
        skip::Walk w = to_walk(s);
        if (skip::walk_skip(grid_view(g), w, r.t, cells)) r.t = w.t;
    }
    *out = smax(-1.0f, smin(r.t, 1e4f));
}

// --------------------------------------------------------------- world kernels
__global__ void tiled_world_k(uint8_t* __restrict__ out, uint32_t n, const uint8_t* __restrict__ model, uint32_t mx,
                              uint32_t my, uint32_t mz, uint32_t px, uint32_t py, uint32_t pz, uint32_t ground) {
    // one thread per 16 consecutive x-cells of a row (n % 16 == 0) or per cell otherwise
    const uint64_t n64 = n;
    const bool wide = (n % 16u) == 0;
    const uint64_t per_row = wide ? n64 / 16 : n64;
    const uint64_t total = per_row * n64 * n64;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / per_row;
        const uint64_t x0 = (i % per_row) * (wide ? 16 : 1);
        const uint64_t y = row % n64, z = row / n64;
        uint8_t vals[16];
        const int cnt = wide ? 16 : 1;
        if (y < ground) {
            for (int c = 0; c < cnt; ++c) vals[c] = VPX_MAT_NON_METAL_WHITE;
        } else {
            const uint64_t ly = (y - ground) % py, lz = z % pz;
            for (int c = 0; c < cnt; ++c) {
                const uint64_t lx = (x0 + c) % px;
                vals[c] = (lx < mx && ly < my && lz < mz) ? model[lx + ly * mx + lz * mx * my] : (uint8_t)kNone;
            }
        }
        uint8_t* dst = out + z * n64 * n64 + y * n64 + x0;
        if (wide) {
            uint4 w;
            memcpy(&w, vals, 16);
            *reinterpret_cast<uint4*>(dst) = w;
        } else {
            dst[0] = vals[0];
        }
    }
}

// Scene::LoadModel / LoadModelPartial / LoadModelRandomMaterials (template/scene.cpp:449-683):
// every cell of the grid gathers its last writer through the plan's preimage tables
// (vpx_model.hpp), cells no voxel reaches get NONE — the ResetGrid() is part of the pass.
// One thread per 16 consecutive x-cells of a row (n % 16 == 0) or per cell otherwise.
__global__ __launch_bounds__(256) void model_gather_k(uint8_t* __restrict__ out, uint32_t n,
                                                      const uint8_t* __restrict__ plan, const uint8_t* __restrict__ vox,
                                                      const uint8_t* __restrict__ mat, uint32_t sx, uint32_t sy) {
    const model::PlanView pv{plan, reinterpret_cast<const uint16_t*>(plan + model::kSrcBytes), n};
    const uint64_t n64 = n;
    const bool wide = (n % 16u) == 0;
    const uint64_t per_row = wide ? n64 / 16 : n64;
    const uint64_t total = per_row * n64 * n64;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t row = i / per_row;
        const uint32_t x0 = (uint32_t)(i % per_row) * (wide ? 16u : 1u);
        const uint32_t y = (uint32_t)(row % n64), z = (uint32_t)(row / n64);
        uint8_t* dst = out + z * n64 * n64 + y * n64 + x0;
        if (wide) {
            uint8_t vals[16];
            model::place_span<16>(pv, vox, mat, sx, sy, x0, y, z, vals);
            uint32_t w[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                w[q] = (uint32_t)vals[4 * q] | (uint32_t)vals[4 * q + 1] << 8 | (uint32_t)vals[4 * q + 2] << 16 |
                       (uint32_t)vals[4 * q + 3] << 24;
            *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
        } else {
            uint8_t v;
            model::place_span<1>(pv, vox, mat, sx, sy, x0, y, z, &v);
            dst[0] = v;
        }
    }
}

// LoadModelRandomMaterials' draws (scene.cpp:661): the material of every voxel, empty ones
// included, into `mat` (whole chunks of model::kChunk voxels); a thread jumps to its chunk's
// first xorshift32 state and steps from there.
__global__ __launch_bounds__(256) void model_random_k(const uint32_t* __restrict__ tables, uint32_t seed, uint64_t count,
                                                      float lo, float hi, uint8_t* __restrict__ mat) {
    const uint64_t chunks = (count + model::kChunk - 1) / model::kChunk;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (uint64_t)gridDim.x * blockDim.x)
        model::random_chunk(tables, seed, c * model::kChunk, lo, hi, mat);
}

// Gather a box of the grid into a staging buffer (x fastest): write_box_k's inverse.
__global__ void read_box_k(const uint8_t* __restrict__ grid, uint32_t n, uint8_t* __restrict__ dst, uint32_t x0,
                           uint32_t y0, uint32_t z0, uint32_t dx, uint32_t dy, uint32_t dz) {
    const uint64_t total = (uint64_t)dx * dy * dz;
    const uint64_t n64 = n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t x = i % dx, y = (i / dx) % dy, z = i / ((uint64_t)dx * dy);
        dst[i] = grid[(x0 + x) + (y0 + y) * n64 + (z0 + z) * n64 * n64];
    }
}

// ------------------------------------------------------------- noise generators
// Scene::GenerateSomeNoise / GenerateSomeSmoke (template/scene.cpp:226-356, vpx_noise.hpp).  A
// workgroup takes blocks of noise::kBlockCells consecutive cells, a thread the span of kSpan
// cells at 16 * threadIdx.x of the block: one 16-byte store when n % 16 == 0 (a span then lies
// in one grid row), byte stores with the grid's end checked otherwise.  Every cell is written:
// the ResetGrid() is part of the pass.

__device__ __forceinline__ void span_store(uint8_t* __restrict__ out, uint64_t first, uint32_t count, bool row,
                                           const uint8_t (&v)[noise::kSpan]) {
    if (row) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            w[q] = (uint32_t)v[4 * q] | (uint32_t)v[4 * q + 1] << 8 | (uint32_t)v[4 * q + 2] << 16 |
                   (uint32_t)v[4 * q + 3] << 24;
        *reinterpret_cast<uint4*>(out + first) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (uint32_t c = 0; c < noise::kSpan; ++c)
            if (c < count) out[first + c] = v[c];
    }
}

// The drawers of a wave, span masks in lane order: how many lie in the lanes below this one,
// and how many the wave has (wave64: a ballot per span position, counted below the lane by
// mbcnt).  Every lane of the wave must call it.
__device__ __forceinline__ void wave_rank(uint32_t mask, uint32_t& below, uint32_t& total) {
    below = 0, total = 0;
#pragma unroll
    for (uint32_t c = 0; c < noise::kSpan; ++c) {
        const unsigned long long b = __ballot((mask >> c) & 1u);
        below += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
        total += (uint32_t)__popcll(b);
    }
}

// GenerateSomeSmoke: one pass.  Cell i draws twice, so the block's first state is the jump of
// 1 + 2 * (its first cell) steps — the same for the whole workgroup — and a thread jumps the
// 32 * threadIdx.x steps of the spans before its own from there.
__global__ __launch_bounds__(256) void smoke_gen_k(uint8_t* __restrict__ out, uint32_t n, float f, int32_t nseed,
                                                   const uint32_t* __restrict__ tables, uint32_t seed, uint64_t blocks) {
    const uint64_t total = (uint64_t)n * n * n;
    const bool row = (n % noise::kSpan) == 0;
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t first = b * noise::kBlockCells + (uint64_t)threadIdx.x * noise::kSpan;
        if (first >= total) continue;
        const uint32_t base = model::xs32_jump(tables, seed, 1 + 2 * b * noise::kBlockCells);
        const uint32_t s = model::xs32_jump(tables, base, 2ull * noise::kSpan * threadIdx.x);
        const uint32_t count = (uint32_t)(total - first < noise::kSpan ? total - first : noise::kSpan);
        uint8_t v[noise::kSpan];
        if (row)
            noise::smoke_span<true>(nseed, n, f, first, noise::kSpan, s, v);
        else
            noise::smoke_span<false>(nseed, n, f, first, count, s, v);
        span_store(out, first, count, row, v);
    }
}

// GenerateSomeNoise, pass 1: every cell's material, noise::kDrawMark where the cell draws, and
// the number of drawers of each block into counts.
__global__ __launch_bounds__(256) void noise_mark_k(uint8_t* __restrict__ out, uint32_t n, float f, int32_t nseed,
                                                    uint64_t blocks, uint32_t* __restrict__ counts) {
    __shared__ uint32_t wsum[noise::kBlockThreads / 64];
    const uint64_t total = (uint64_t)n * n * n;
    const bool row = (n % noise::kSpan) == 0;
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        const uint64_t first = b * noise::kBlockCells + (uint64_t)threadIdx.x * noise::kSpan;
        uint32_t mask = 0;
        if (first < total) {
            const uint32_t count = (uint32_t)(total - first < noise::kSpan ? total - first : noise::kSpan);
            uint8_t v[noise::kSpan];
            mask = row ? noise::noise_span<true>(nseed, n, f, first, noise::kSpan, v)
                       : noise::noise_span<false>(nseed, n, f, first, count, v);
            span_store(out, first, count, row, v);
        }
        uint32_t below, wave;
        wave_rank(mask, below, wave);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = wave;
        __syncthreads();
        if (threadIdx.x == 0) counts[b] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
}

// Pass 2: offsets[b] = the drawers of the blocks before b, total[0] = all of them, 64-bit.  One
// workgroup walks the counts noise::kScanPass at a time and carries the sum from pass to pass,
// so the prefix is exact for any number of blocks (a pass sums at most 256 * 4096).
__global__ __launch_bounds__(256) void noise_scan_k(const uint32_t* __restrict__ counts, uint64_t blocks,
                                                    uint64_t* __restrict__ offsets, uint64_t* __restrict__ total) {
    __shared__ uint32_t wsum[noise::kScanPass / 64];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint64_t carry = 0;
    for (uint64_t at = 0; at < blocks; at += noise::kScanPass) {
        const uint64_t i = at + threadIdx.x;
        const uint32_t v = i < blocks ? counts[i] : 0u;
        uint32_t incl = v;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wsum[w] = incl;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t k = 0; k < noise::kScanPass / 64; ++k) {
            before += k < w ? wsum[k] : 0u;
            all += wsum[k];
        }
        if (i < blocks) offsets[i] = carry + before + (incl - v);
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = carry;
}

// Pass 3: every marked cell takes its draw.  Its rank among the drawers is the block's offset
// plus the drawers of the block's spans before its own plus its place in the span; the state is
// the jump to the block's first rank — the same for the whole workgroup — then the jump by the
// in-block rank (< 4096), then plain steps along the span.  Spans without a mark are not
// touched; a block without drawers is skipped by all its threads alike.
__global__ __launch_bounds__(256) void noise_draw_k(uint8_t* __restrict__ out, uint32_t n,
                                                    const uint32_t* __restrict__ tables, uint32_t seed, uint64_t blocks,
                                                    const uint32_t* __restrict__ counts,
                                                    const uint64_t* __restrict__ offsets) {
    __shared__ uint32_t wsum[noise::kBlockThreads / 64];
    const uint64_t total = (uint64_t)n * n * n;
    const bool row = (n % noise::kSpan) == 0;
    for (uint64_t b = blockIdx.x; b < blocks; b += gridDim.x) {
        if (counts[b] == 0) continue;
        const uint64_t first = b * noise::kBlockCells + (uint64_t)threadIdx.x * noise::kSpan;
        const uint32_t count = first >= total ? 0u : (uint32_t)(total - first < noise::kSpan ? total - first : noise::kSpan);
        uint8_t v[noise::kSpan];
        if (row) {
            const uint4 q = *reinterpret_cast<const uint4*>(out + first);
            const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (uint32_t c = 0; c < noise::kSpan; ++c) v[c] = (uint8_t)(w[c >> 2] >> (8 * (c & 3)));
        } else {
#pragma unroll
            for (uint32_t c = 0; c < noise::kSpan; ++c) v[c] = c < count ? out[first + c] : noise::kNone;
        }
        uint32_t mask = 0;
#pragma unroll
        for (uint32_t c = 0; c < noise::kSpan; ++c) mask |= (uint32_t)(v[c] == noise::kDrawMark) << c;
        uint32_t below, wave;
        wave_rank(mask, below, wave);
        if ((threadIdx.x & 63u) == 0) wsum[threadIdx.x >> 6] = wave;
        __syncthreads();
        uint32_t before = below;
#pragma unroll
        for (uint32_t k = 0; k < noise::kBlockThreads / 64; ++k) before += k < (threadIdx.x >> 6) ? wsum[k] : 0u;
        if (mask) {
            const uint32_t base = model::xs32_jump(tables, seed, 1 + offsets[b]);
            noise::noise_fill_span(model::xs32_jump(tables, base, before), mask, v);
            span_store(out, first, count, row, v);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------- occupancy masks
// Layout: vpx_skip.hpp blk_index (l1, l2 blocked by parent) / lin_index (l3).
// l1: one thread per output word (padded space nb2^3 * 64) reads its brick's 64 cells.
__global__ void build_l1_k(const uint8_t* __restrict__ cells, uint32_t n, uint32_t nb1, uint32_t nb2,
                           uint64_t* __restrict__ l1) {
    const uint64_t total = (uint64_t)nb2 * nb2 * nb2 * 64;
    const uint64_t n64 = n;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t parent = s >> 6;
        const uint32_t j = (uint32_t)(s & 63u);
        const uint32_t bx = (uint32_t)(parent % nb2) * 4 + (j & 3u);
        const uint32_t by = (uint32_t)((parent / nb2) % nb2) * 4 + ((j >> 2) & 3u);
        const uint32_t bz = (uint32_t)(parent / ((uint64_t)nb2 * nb2)) * 4 + (j >> 4);
        uint64_t m = 0;
        if (bx < nb1 && by < nb1 && bz < nb1) {
            for (uint32_t lz = 0; lz < 4; ++lz)
                for (uint32_t ly = 0; ly < 4; ++ly) {
                    const uint32_t y = by * 4 + ly, z = bz * 4 + lz;
                    if (y >= n || z >= n) continue;
                    const uint8_t* row = cells + (uint64_t)y * n64 + (uint64_t)z * n64 * n64;
                    for (uint32_t lx = 0; lx < 4; ++lx) {
                        const uint32_t x = bx * 4 + lx;
                        if (x < n && row[x] != kNone) m |= 1ull << (lx + 4 * ly + 16 * lz);
                    }
                }
        }
        l1[s] = m;
    }
}

// One level up: the word of parent block P (np parents per axis, linear P) ORs the 64
// consecutive child words child[P*64 + j] into bit j (child words are fresh cell masks).
// Output blocked by grandparent (ngp per axis, words ngp^3 * 64).
__global__ void build_up_k(const uint64_t* __restrict__ child, uint32_t np, uint32_t ngp, uint64_t* __restrict__ out) {
    const uint64_t total = (uint64_t)ngp * ngp * ngp * 64;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < total; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t gp = s >> 6;
        const uint32_t j = (uint32_t)(s & 63u);
        const uint32_t px = (uint32_t)(gp % ngp) * 4 + (j & 3u);
        const uint32_t py = (uint32_t)((gp / ngp) % ngp) * 4 + ((j >> 2) & 3u);
        const uint32_t pz = (uint32_t)(gp / ((uint64_t)ngp * ngp)) * 4 + (j >> 4);
        uint64_t m = 0;
        if (px < np && py < np && pz < np) {
            const uint64_t* c = child + (((uint64_t)pz * np + py) * np + px) * 64;
            for (uint32_t j = 0; j < 64; ++j) m |= (c[j] != 0ull ? 1ull : 0ull) << j;
        }
        out[s] = m;
    }
}

// One plane fx + fy + fz = s of the distance-field sweep (build_df), thread = (fx, fy,
// octant o); (fx, fy, fz) are brick coordinates flipped so that octant o's "ahead" is +1.
// Reads bytes o of the words on planes s+1..s+3 (earlier launches), writes plane s.
__global__ void df_plane_k(uint8_t* __restrict__ l1b, const uint64_t* __restrict__ l2, uint32_t nb1, uint32_t nb2,
                           uint32_t nb3, uint32_t s) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t o = (uint32_t)(t & 7u);
    const uint64_t q = t >> 3;
    const uint32_t fx = (uint32_t)(q % nb1), fy = (uint32_t)(q / nb1);
    if (fy >= nb1 || fx + fy > s || s - fx - fy >= nb1) return;
    const uint32_t fz = s - fx - fy;
    const uint32_t x = (o & 1u) ? nb1 - 1u - fx : fx, y = (o & 2u) ? nb1 - 1u - fy : fy, z = (o & 4u) ? nb1 - 1u - fz : fz;
    auto occ = [&](uint32_t a, uint32_t b, uint32_t c) -> bool {
        return (l2[skip::blk_index(a >> 2, b >> 2, c >> 2, nb3)] >> ((a & 3u) | ((b & 3u) << 2) | ((c & 3u) << 4))) & 1ull;
    };
    if (occ(x, y, z)) return;
    auto get = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t oo) -> uint32_t {
        return l1b[(size_t)skip::blk_index(a, b, c, nb2) * 8 + oo];
    };
    l1b[(size_t)skip::blk_index(x, y, z, nb2) * 8 + o] = skip::df_value(x, y, z, o, nb1, occ, get);
}

// The octant planes from the built levels (after build_df): byte o of an empty brick's l1
// word into plane o, 0 for an occupied brick (and for the padding bricks, never walked).
__global__ void build_planes_k(const uint64_t* __restrict__ l1, const uint64_t* __restrict__ l2, uint32_t nb2,
                               uint32_t nb3, uint8_t* __restrict__ dfp) {
    const uint64_t plane = (uint64_t)nb2 * nb2 * nb2 * 64;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < plane; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t parent = s >> 6;
        const uint32_t j = (uint32_t)(s & 63u);
        const uint32_t bx = (uint32_t)(parent % nb2) * 4 + (j & 3u);
        const uint32_t by = (uint32_t)((parent / nb2) % nb2) * 4 + ((j >> 2) & 3u);
        const uint32_t bz = (uint32_t)(parent / ((uint64_t)nb2 * nb2)) * 4 + (j >> 4);
        const bool occ = (l2[skip::blk_index(bx >> 2, by >> 2, bz >> 2, nb3)] >> ((bx & 3u) | ((by & 3u) << 2) | ((bz & 3u) << 4))) & 1ull;
        const uint64_t m = occ ? 0ull : l1[s];
#pragma unroll
        for (uint32_t o = 0; o < 8; ++o) dfp[o * plane + s] = (uint8_t)(m >> (8 * o));
    }
}

// The axis planes from the octant planes (after build_planes_k): thread = (brick, octant,
// axis), scanning at most 255 bricks ahead along the axis (skip::axis_len).  Writes the words'
// k | L << 8 halves, as skip::build_wide_planes_host's first pass; the widths are build_wide_k's.
// dfw follows the octant planes in dfp's buffer.
__global__ void build_axis_k(const uint8_t* __restrict__ dfp, uint32_t nb1, uint32_t nb2, uint32_t* __restrict__ dfw) {
    const uint64_t plane = (uint64_t)nb2 * nb2 * nb2 * 64;
    const uint64_t total = plane * 24;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t oa = (uint32_t)(t / plane);
        const uint64_t s = t - (uint64_t)oa * plane;
        const uint32_t o = oa / 3u, a = oa - o * 3u;
        const uint64_t parent = s >> 6;
        const uint32_t j = (uint32_t)(s & 63u);
        const uint32_t bx = (uint32_t)(parent % nb2) * 4 + (j & 3u);
        const uint32_t by = (uint32_t)((parent / nb2) % nb2) * 4 + ((j >> 2) & 3u);
        const uint32_t bz = (uint32_t)(parent / ((uint64_t)nb2 * nb2)) * 4 + (j >> 4);
        const uint8_t* pl = dfp + (uint64_t)o * plane;
        const uint32_t k = pl[s];  // 0: occupied, or a padding brick (bx, by or bz >= nb1), never walked
        auto cube = [&](uint32_t x, uint32_t y, uint32_t z) -> uint32_t { return pl[skip::blk_index(x, y, z, nb2)]; };
        dfw[t] = k ? k | skip::axis_len(bx, by, bz, o, a, k, nb1, cube) << 8 : 0u;
    }
}

// The widths Mb | Mc << 8 into the words' high halves (after build_axis_k; skip::axis_wids,
// the same words as skip::build_wide_planes_host).  A thread reads other bricks' low halves
// while their threads write the high ones, so both sides go through 16-bit accesses.
__global__ void build_wide_k(uint16_t* dfh, uint32_t nb1, uint32_t nb2) {
    const uint64_t plane = (uint64_t)nb2 * nb2 * nb2 * 64;
    const uint64_t total = plane * 24;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t oa = (uint32_t)(t / plane);
        const uint64_t s = t - (uint64_t)oa * plane;
        const uint32_t o = oa / 3u, a = oa - o * 3u;
        const uint64_t parent = s >> 6;
        const uint32_t j = (uint32_t)(s & 63u);
        const uint32_t bx = (uint32_t)(parent % nb2) * 4 + (j & 3u);
        const uint32_t by = (uint32_t)((parent / nb2) % nb2) * 4 + ((j >> 2) & 3u);
        const uint32_t bz = (uint32_t)(parent / ((uint64_t)nb2 * nb2)) * 4 + (j >> 4);
        const uint16_t* pl = dfh + 2 * (uint64_t)oa * plane;
        const uint32_t kl = pl[2 * s];
        if (!kl || bx >= nb1 || by >= nb1 || bz >= nb1) continue;  // the high half is build_axis_k's 0
        auto word = [&](uint32_t x, uint32_t y, uint32_t z) -> uint32_t { return pl[2 * (uint64_t)skip::blk_index(x, y, z, nb2)]; };
        dfh[2 * t + 1] = (uint16_t)skip::axis_wids(bx, by, bz, o, a, kl & 255u, kl >> 8, nb1, word);
    }
}

// ------------------------------------------------------- region-local level refresh
// What an edit leaves to do (refresh_levels, DESIGN §4 "Brush edits"): the stages of the full
// build over the boxes that the flipped bricks can reach, marked with vpx_skip.hpp's predicates
// from the words' old values.  The boxes travel between the stages in RefreshDev.
struct RefreshDev {
    unsigned long long changed;  // cells the call's brushes changed
    uint32_t flipped, pad;       // bricks whose emptiness flipped
    skip::Box3 E;                // their box
    skip::Box3 C[8];             // per octant: the cube bytes recomputed (stage 1)
    skip::Box3 D[24];            // per plane: the low halves recomputed (stage 3)
};
struct Boxes8 {
    skip::Box3 b[8];
};

__device__ __forceinline__ uint64_t box_dims(const skip::Box3& b, uint32_t c[3]) {
    const bool none = skip::box_empty(b);
    for (int q = 0; q < 3; ++q) c[q] = none ? 0u : (uint32_t)(b.hi[q] - b.lo[q] + 1);
    return (uint64_t)c[0] * c[1] * c[2];
}
__device__ __forceinline__ void box_brick(const skip::Box3& b, const uint32_t c[3], uint64_t i, uint32_t p[3]) {
    p[0] = (uint32_t)b.lo[0] + (uint32_t)(i % c[0]);
    p[1] = (uint32_t)b.lo[1] + (uint32_t)((i / c[0]) % c[1]);
    p[2] = (uint32_t)b.lo[2] + (uint32_t)(i / ((uint64_t)c[0] * c[1]));
}
// Grow a box in device memory by the bricks p of the lanes with `on`: a reduction over the wave,
// then at most six atomics from its first lane.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_box_add(skip::Box3* box, bool on, const uint32_t p[3]) {
    if (!__any(on)) return;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        int32_t lo = on ? (int32_t)p[q] : skip::kBoxNone, hi = on ? (int32_t)p[q] : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = min(lo, __shfl_xor(lo, o, 64));
            hi = max(hi, __shfl_xor(hi, o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMin(&box->lo[q], lo);
            atomicMax(&box->hi[q], hi);
        }
    }
}

// One brush over its clipped bounding box (cells lo .. lo + c - 1, x fastest), vpx_brush.hpp's
// tests; the changed cells are counted per wave.
__global__ __launch_bounds__(256) void brush_k(uint8_t* __restrict__ grid, uint32_t n, vpx_brush b, uint32_t x0, uint32_t y0,
                                               uint32_t z0, uint32_t cx, uint32_t cy, uint32_t cz, RefreshDev* rd) {
    const uint64_t total = (uint64_t)cx * cy * cz, n64 = n;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < total; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        bool ch = false;
        if (i < total) {
            const uint32_t x = x0 + (uint32_t)(i % cx), y = y0 + (uint32_t)((i / cx) % cy), z = z0 + (uint32_t)(i / ((uint64_t)cx * cy));
            uint8_t* cell = grid + (x + y * n64 + z * n64 * n64);
            ch = brush::in_shape(b, x, y, z) && brush::writes(b, *cell);
            if (ch) *cell = b.value;
        }
        const uint64_t m = __ballot(ch);
        if (m && (threadIdx.x & 63) == 0) atomicAdd(&rd->changed, (unsigned long long)__popcll(m));
    }
}

// One stamp over its clipped box (vpx_stamp.hpp's plan and per-cell rule): a gather, every cell
// reads one voxel and is written by its own thread.  kWide (n % 16 == 0): a thread owns one
// 16-byte-aligned span of a row that meets the box (spans [s0, s0 + spans) of the row), loads it
// with one vector load, merges the cells inside the box and stores it once if a byte changed;
// no model index is formed for a cell outside the box.  Otherwise one thread per cell.  The
// changed cells are counted per wave, the ballots of the count's five bits, summed over the
// wave's strides; one atomic per workgroup ends the kernel (16384 atomics on one address, one
// per wave and stride, were the whole time of a 256^3 stamp: DESIGN §4 "Stamps").
template <bool kWide>
__global__ __launch_bounds__(256) void stamp_k(uint8_t* __restrict__ grid, uint32_t n, const uint8_t* __restrict__ vox,
                                               stamp::Plan p, uint32_t s0, uint32_t spans, RefreshDev* rd) {
    const uint32_t cy = p.hi[1] - p.lo[1] + 1, cz = p.hi[2] - p.lo[2] + 1;
    const uint32_t per_row = kWide ? spans : p.hi[0] - p.lo[0] + 1;
    const uint64_t total = (uint64_t)per_row * cy * cz, n64 = n;
    unsigned long long wave = 0;  // cells this wave changed
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < total; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        uint32_t ch = 0;  // cells this thread changed, 0..16
        if (i < total) {
            const uint32_t k = (uint32_t)(i % per_row);
            const uint32_t y = p.lo[1] + (uint32_t)((i / per_row) % cy), z = p.lo[2] + (uint32_t)(i / ((uint64_t)per_row * cy));
            const int32_t row = stamp::row_base(p, y, z);
            uint8_t* cells = grid + (y * n64 + z * n64 * n64);
            if (kWide) {
                const uint32_t x0 = (s0 + k) * 16u;
                uint4* span = reinterpret_cast<uint4*>(cells + x0);
                const uint4 in = *span;
                uint32_t w[4] = {in.x, in.y, in.z, in.w};
                const uint32_t first = x0 < p.lo[0] ? p.lo[0] - x0 : 0u, last = min(p.hi[0] - x0, 15u);
                const int32_t m0 = row + p.step[0] * ((int32_t)(x0 + first) - p.origin[0]);
                // the 16 voxel loads first, none waiting for a merge; a cell outside the box has no
                // voxel of its own (its coordinate is out of range): its load repeats the nearest
                // inside cell's and is not used
                uint8_t v[16];
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j) v[j] = vox[m0 + p.step[0] * (int32_t)(min(max(j, first), last) - first)];
#pragma unroll
                for (uint32_t j = 0; j < 16; ++j) {
                    const uint32_t sh = 8 * (j & 3u);
                    uint8_t out;
                    if (stamp::writes(p, v[j], (uint8_t)(w[j >> 2] >> sh), out) && j >= first && j <= last) {
                        w[j >> 2] = (w[j >> 2] & ~(255u << sh)) | (uint32_t)out << sh;
                        ++ch;
                    }
                }
                if (ch) *span = make_uint4(w[0], w[1], w[2], w[3]);
            } else {
                const uint32_t x = p.lo[0] + k;
                uint8_t out;
                if (stamp::writes(p, vox[row + p.step[0] * ((int32_t)x - p.origin[0])], cells[x], out)) cells[x] = out, ch = 1;
            }
        }
#pragma unroll
        for (uint32_t b = 0; b < (kWide ? 5u : 1u); ++b) wave += (unsigned long long)__popcll(__ballot((ch >> b) & 1u)) << b;
    }
    __shared__ unsigned long long waves[4];
    if ((threadIdx.x & 63) == 0) waves[threadIdx.x >> 6] = wave;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long sum = waves[0] + waves[1] + waves[2] + waves[3];
        if (sum) atomicAdd(&rd->changed, sum);
    }
}

// vpx_model_capture: the cells of a box into a model, index x + y*dx + z*dx*dy.  kWide (the grid's
// rows, x0 and dx are multiples of 16): 16 bytes per thread, loaded and stored as one vector.
template <bool kWide>
__global__ __launch_bounds__(256) void capture_k(const uint8_t* __restrict__ grid, uint32_t n, uint8_t* __restrict__ vox, uint32_t x0,
                                                 uint32_t y0, uint32_t z0, uint32_t dx, uint32_t dy, uint32_t dz) {
    const uint32_t per_row = kWide ? dx / 16u : dx;
    const uint64_t total = (uint64_t)per_row * dy * dz, n64 = n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = (uint32_t)(i % per_row) * (kWide ? 16u : 1u), y = (uint32_t)((i / per_row) % dy), z = (uint32_t)(i / ((uint64_t)per_row * dy));
        const uint8_t* src = grid + ((x0 + x) + (y0 + y) * n64 + (z0 + z) * n64 * n64);
        uint8_t* dst = vox + (x + (uint64_t)y * dx + (uint64_t)z * dx * dy);
        if (kWide)
            *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
        else
            *dst = *src;
    }
}

// Stage 0: the cell masks of the bricks [b0, b0 + c) from the edited cells, and l2's bits.  The
// l1 word of an empty brick holds its distance-field bytes: a brick that stays empty keeps them,
// one that empties gets 0 until stage 1 (it lies in E).  Flips are counted and boxed in rd.
__global__ __launch_bounds__(256) void refresh_l1_k(const uint8_t* __restrict__ cells, uint32_t n, uint32_t nb2, uint32_t nb3,
                                                    uint64_t* __restrict__ l1, uint64_t* l2, uint32_t bx0, uint32_t by0, uint32_t bz0,
                                                    uint32_t cx, uint32_t cy, uint32_t cz, RefreshDev* rd) {
    const uint64_t total = (uint64_t)cx * cy * cz, n64 = n;
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < total; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        bool flip = false;
        uint32_t p[3] = {0u, 0u, 0u};
        if (i < total) {
            p[0] = bx0 + (uint32_t)(i % cx), p[1] = by0 + (uint32_t)((i / cx) % cy), p[2] = bz0 + (uint32_t)(i / ((uint64_t)cx * cy));
            uint64_t m = 0;
            for (uint32_t lz = 0; lz < 4; ++lz)
                for (uint32_t ly = 0; ly < 4; ++ly) {
                    const uint32_t y = p[1] * 4 + ly, z = p[2] * 4 + lz;
                    if (y >= n || z >= n) continue;
                    const uint8_t* row = cells + (uint64_t)y * n64 + (uint64_t)z * n64 * n64;
                    for (uint32_t lx = 0; lx < 4; ++lx) {
                        const uint32_t x = p[0] * 4 + lx;
                        if (x < n && row[x] != kNone) m |= 1ull << (lx + 4 * ly + 16 * lz);
                    }
                }
            unsigned long long* w2 = (unsigned long long*)l2 + skip::blk_index(p[0] >> 2, p[1] >> 2, p[2] >> 2, nb3);
            const unsigned long long bit = 1ull << ((p[0] & 3u) | ((p[1] & 3u) << 2) | ((p[2] & 3u) << 4));
            const bool was = *w2 & bit, is = m != 0ull;
            if (is || was) l1[skip::blk_index(p[0], p[1], p[2], nb2)] = m;
            flip = is != was;
            if (flip) atomicXor(w2, bit);  // other lanes own the word's other bits
        }
        const uint64_t fm = __ballot(flip);
        if (fm && (threadIdx.x & 63) == 0) atomicAdd(&rd->flipped, (uint32_t)__popcll(fm));
        wave_box_add(&rd->E, flip, p);
    }
}

// Stage 1, marking: blockIdx.y = octant o; the candidates cand.b[o] (E grown backward by the
// reach) test their old cube byte, which the octant planes still hold, and box the marked in rd->C[o].
__global__ __launch_bounds__(256) void df_mark_k(const uint8_t* __restrict__ dfp, uint64_t plane, uint32_t nb2, Boxes8 cand,
                                                 skip::Box3 E, RefreshDev* rd) {
    const uint32_t o = blockIdx.y;
    uint32_t c[3];
    const uint64_t total = box_dims(cand.b[o], c);
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < total; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        bool dirty = false;
        uint32_t p[3] = {0u, 0u, 0u};
        if (i < total) {
            box_brick(cand.b[o], c, i, p);
            dirty = skip::cube_dirty(p, o, dfp[o * plane + skip::blk_index(p[0], p[1], p[2], nb2)], E);
        }
        wave_box_add(&rd->C[o], dirty, p);
    }
}

// Stage 1, sweep: one anti-diagonal fx + fy + fz = s of every octant's box C.b[o] (blockIdx.y =
// o), f counted from the box's corner furthest ahead, as df_plane_k does for the whole grid: the
// neighbours ahead lie on earlier diagonals or outside the box, where no byte changes.
__global__ __launch_bounds__(256) void df_diag_k(uint8_t* l1b, const uint64_t* __restrict__ l2, uint32_t nb1, uint32_t nb2,
                                                 uint32_t nb3, Boxes8 C, uint32_t s) {
    const uint32_t o = blockIdx.y;
    uint32_t c[3];
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (!box_dims(C.b[o], c)) return;
    const uint32_t fx = (uint32_t)(q % c[0]);
    const uint64_t fy = q / c[0];
    if (fy >= c[1] || fx + fy > s || s - fx - fy >= c[2]) return;
    const uint32_t fz = s - fx - (uint32_t)fy;
    const skip::Box3& b = C.b[o];
    const uint32_t x = (o & 1u) ? (uint32_t)b.lo[0] + fx : (uint32_t)b.hi[0] - fx, y = (o & 2u) ? (uint32_t)b.lo[1] + (uint32_t)fy : (uint32_t)b.hi[1] - (uint32_t)fy,
                   z = (o & 4u) ? (uint32_t)b.lo[2] + fz : (uint32_t)b.hi[2] - fz;
    auto occ = [&](uint32_t a, uint32_t bb, uint32_t cc) -> bool {
        return (l2[skip::blk_index(a >> 2, bb >> 2, cc >> 2, nb3)] >> ((a & 3u) | ((bb & 3u) << 2) | ((cc & 3u) << 4))) & 1ull;
    };
    if (occ(x, y, z)) return;
    auto get = [&](uint32_t a, uint32_t bb, uint32_t cc, uint32_t oo) -> uint32_t {
        return l1b[(size_t)skip::blk_index(a, bb, cc, nb2) * 8 + oo];
    };
    l1b[(size_t)skip::blk_index(x, y, z, nb2) * 8 + o] = skip::df_value(x, y, z, o, nb1, occ, get);
}

// Stage 2: build_planes_k limited to the boxes: byte o of the bricks of C.b[o] into plane o, 0
// for an occupied brick (one that filled included).
__global__ __launch_bounds__(256) void df_planes_box_k(const uint8_t* __restrict__ l1b, const uint64_t* __restrict__ l2, uint32_t nb2,
                                                       uint32_t nb3, uint8_t* __restrict__ dfp, uint64_t plane, Boxes8 C) {
    const uint32_t o = blockIdx.y;
    uint32_t c[3];
    const uint64_t total = box_dims(C.b[o], c);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t p[3];
        box_brick(C.b[o], c, i, p);
        const bool occ = (l2[skip::blk_index(p[0] >> 2, p[1] >> 2, p[2] >> 2, nb3)] >> ((p[0] & 3u) | ((p[1] & 3u) << 2) | ((p[2] & 3u) << 4))) & 1ull;
        const uint32_t s = skip::blk_index(p[0], p[1], p[2], nb2);
        dfp[o * plane + s] = occ ? (uint8_t)0 : l1b[(size_t)s * 8 + o];
    }
}

// Stage 3: blockIdx.y = plane (o, a); the candidates are C.b[o] grown backward along a.  A
// thread tests its own old word (skip::len_dirty), recomputes the low half with axis_len from the
// refreshed octant plane and boxes what it recomputed in rd->D.  A brick that filled gets 0.
__global__ __launch_bounds__(256) void axis_box_k(const uint8_t* __restrict__ dfp, uint32_t nb1, uint32_t nb2, uint32_t* dfw, Boxes8 C,
                                                  RefreshDev* rd) {
    const uint32_t oa = blockIdx.y, o = oa / 3u, a = oa - o * 3u;
    const uint64_t plane = (uint64_t)nb2 * nb2 * nb2 * 64;
    uint32_t ext[3] = {1u, 1u, 1u};
    ext[a] = skip::kReach;
    const skip::Box3 cand = skip::box_behind(C.b[o], o, ext, nb1);
    uint32_t c[3];
    const uint64_t total = box_dims(cand, c);
    const uint8_t* pl = dfp + (uint64_t)o * plane;
    auto cube = [&](uint32_t x, uint32_t y, uint32_t z) -> uint32_t { return pl[skip::blk_index(x, y, z, nb2)]; };
    for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < total; base += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = base + threadIdx.x;
        bool dirty = false;
        uint32_t p[3] = {0u, 0u, 0u};
        if (i < total) {
            box_brick(cand, c, i, p);
            const uint32_t s = skip::blk_index(p[0], p[1], p[2], nb2);
            uint32_t* w = dfw + (uint64_t)oa * plane + s;
            const uint32_t old = *w;
            dirty = skip::len_dirty(p, o, a, old & 255u, (old >> 8) & 255u, C.b[o]);
            if (dirty) {
                const uint32_t k = pl[s];
                if (k) *(uint16_t*)w = (uint16_t)(k | skip::axis_len(p[0], p[1], p[2], o, a, k, nb1, cube) << 8);
                else *w = 0u;
            }
        }
        wave_box_add(&rd->D[oa], dirty, p);
    }
}

// Stage 4: blockIdx.y = plane (o, a); the candidates are the cone behind rd->D[oa], read from
// device memory (stage 3 left it there), taken macro by macro: a wave reads the 64 contiguous
// words of one 4^3 group of bricks, a workgroup kWideMacros of them per round.  A thread tests
// its own word (skip::wid_dirty: the low half is final, and old outside D; the high half is
// still the old one) and queues it in LDS when it is dirty; the workgroup then recomputes the
// queued words' widths with axis_wids, one per thread, so the few dirty words of a sparse cone
// do not each hold a wave.  As in build_wide_k other threads read low halves while high halves
// are written, so both sides go through 16-bit accesses.  Bricks of a macro outside the cone
// fail the test, and padding bricks hold 0.
constexpr uint32_t kWideMacros = 32;
__global__ __launch_bounds__(256) void wide_box_k(uint16_t* dfh, uint32_t nb1, uint32_t nb2, const RefreshDev* rd) {
    __shared__ uint32_t queue[kWideMacros * 64];
    __shared__ uint32_t queued;
    const uint32_t oa = blockIdx.y, o = oa / 3u, a = oa - o * 3u;
    const uint64_t plane = (uint64_t)nb2 * nb2 * nb2 * 64;
    const skip::Box3 D = rd->D[oa];
    if (skip::box_empty(D)) return;
    const uint32_t reach[3] = {skip::kReach, skip::kReach, skip::kReach};
    const skip::Box3 cand = skip::box_behind(D, o, reach, nb1);
    const uint32_t m0[3] = {(uint32_t)cand.lo[0] >> 2, (uint32_t)cand.lo[1] >> 2, (uint32_t)cand.lo[2] >> 2};
    const uint32_t mc[3] = {((uint32_t)cand.hi[0] >> 2) - m0[0] + 1u, ((uint32_t)cand.hi[1] >> 2) - m0[1] + 1u,
                            ((uint32_t)cand.hi[2] >> 2) - m0[2] + 1u};
    const uint32_t macros = mc[0] * mc[1] * mc[2], rounds = (macros + kWideMacros - 1u) / kWideMacros;
    uint16_t* pl = dfh + 2 * (uint64_t)oa * plane;
    auto word = [&](uint32_t x, uint32_t y, uint32_t z) -> uint32_t { return pl[2 * (uint64_t)skip::blk_index(x, y, z, nb2)]; };
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        if (threadIdx.x == 0) queued = 0u;
        __syncthreads();
        for (uint32_t j = wave; j < kWideMacros; j += 4u) {
            const uint32_t mi = r * kWideMacros + j;
            if (mi >= macros) break;
            const uint32_t P[3] = {m0[0] + mi % mc[0], m0[1] + (mi / mc[0]) % mc[1], m0[2] + mi / (mc[0] * mc[1])};
            const uint32_t p[3] = {P[0] * 4u + (lane & 3u), P[1] * 4u + ((lane >> 2) & 3u), P[2] * 4u + (lane >> 4)};
            const uint32_t s = (((P[2] * nb2 + P[1]) * nb2 + P[0]) << 6) | lane;
            const uint32_t kl = pl[2 * (uint64_t)s];
            if (!kl) continue;
            const uint32_t m = pl[2 * (uint64_t)s + 1];
            if (skip::wid_dirty(p, o, a, kl & 255u, kl >> 8, m & 255u, m >> 8, D)) queue[atomicAdd(&queued, 1u)] = s;
        }
        __syncthreads();
        for (uint32_t e = threadIdx.x; e < queued; e += blockDim.x) {
            const uint32_t s = queue[e], parent = s >> 6;
            const uint32_t x = (parent % nb2) * 4u + (s & 3u), y = ((parent / nb2) % nb2) * 4u + ((s >> 2) & 3u),
                           z = (parent / (nb2 * nb2)) * 4u + ((s >> 4) & 3u);
            const uint32_t kl = pl[2 * (uint64_t)s];
            pl[2 * (uint64_t)s + 1] = (uint16_t)skip::axis_wids(x, y, z, o, a, kl & 255u, kl >> 8, nb1, word);
        }
        __syncthreads();
    }
}

// Scatter a staged box (x fastest) into the grid.
__global__ void write_box_k(uint8_t* __restrict__ grid, uint32_t n, const uint8_t* __restrict__ src, uint32_t x0,
                            uint32_t y0, uint32_t z0, uint32_t dx, uint32_t dy, uint32_t dz) {
    const uint64_t total = (uint64_t)dx * dy * dz;
    const uint64_t n64 = n;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t x = i % dx, y = (i / dx) % dy, z = i / ((uint64_t)dx * dy);
        grid[(x0 + x) + (y0 + y) * n64 + (z0 + z) * n64 * n64] = src[i];
    }
}

// Scene::CreateEmmisiveSphere (template/scene.cpp:685-711) over the sphere's bounding box:
// point = float3(x, y, z), d = length(float3(worldsize / 2) - point) (sqrtf of the
// left-to-right dot), set when d < radius.
__global__ void emissive_sphere_k(uint8_t* __restrict__ grid, uint32_t n, uint8_t mat, float radius, uint32_t x0,
                                  uint32_t cnt) {
    const uint64_t total = (uint64_t)cnt * cnt * cnt;
    const uint64_t n64 = n;
    const float c = (float)n / 2.0f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t x = x0 + (uint32_t)(i % cnt), y = x0 + (uint32_t)((i / cnt) % cnt), z = x0 + (uint32_t)(i / ((uint64_t)cnt * cnt));
        const float vx = c - (float)x, vy = c - (float)y, vz = c - (float)z;
        const float d = sqrtf(vx * vx + vy * vy + vz * vz);
        if (d < radius) grid[x + y * n64 + z * n64 * n64] = mat;
    }
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ull;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}

__global__ void checksum_k(const uint8_t* __restrict__ cells, uint64_t count, unsigned long long* out) {
    uint64_t s = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count;
         i += (uint64_t)gridDim.x * blockDim.x)
        s += (uint64_t)(cells[i] + 1u) * splitmix64(i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(out, (unsigned long long)s);
}

}  // namespace

// =========================================================================== host side
struct vpx_ctx;
namespace {
int fail(vpx_ctx* c, int code, const std::string& msg);
hipError_t sync_all(vpx_ctx* c);
}  // namespace

#define VPX_HIP(c, expr)                                                                            \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return fail((c), e_ == hipErrorOutOfMemory ? VPX_E_NOMEM : VPX_E_DEVICE,                \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                         \
    } while (0)

// Every device or pinned allocation of the library is held by an Owned: move-only, it knows its
// pointer and its size in bytes and frees in its destructor (the current device is the
// allocation's: vpx_destroy sets it before `delete`).  g_live_buffers counts what the Owneds of
// the process hold (vpx_debug_live_buffers); it is touched in alloc and release only.
static std::atomic<uint64_t> g_live_buffers{0};
template <typename T, bool kHost = false>  // kHost: pinned host memory instead of device memory
struct Owned {
    T* p = nullptr;
    size_t bytes = 0;
    Owned() = default;
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr, o.bytes = 0; }
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            release();
            p = o.p, bytes = o.bytes;
            o.p = nullptr, o.bytes = 0;
        }
        return *this;
    }
    ~Owned() { release(); }
    void release() {
        if (p) {
            (void)(kHost ? hipHostFree(p) : hipFree(p));
            g_live_buffers.fetch_sub(1);
        }
        p = nullptr, bytes = 0;
    }
    // exactly n bytes (what it held is freed first); on failure empty
    hipError_t alloc(size_t n) {
        release();
        void* q = nullptr;
        const hipError_t e = kHost ? hipHostMalloc(&q, n) : hipMalloc(&q, n);
        if (e != hipSuccess || !q) return e;
        p = static_cast<T*>(q), bytes = n;
        g_live_buffers.fetch_add(1);
        return hipSuccess;
    }
    // at least n bytes: a larger one replaces a smaller (wait: after everything the context has
    // queued, which may still read the old one); on failure empty
    int grow(vpx_ctx* c, size_t n, bool wait) {
        if (n <= bytes) return VPX_OK;
        if (wait && p) VPX_HIP(c, sync_all(c));
        VPX_HIP(c, alloc(n));
        return VPX_OK;
    }
    T* get() const { return p; }
    operator T*() const { return p; }
    template <typename U>
    U* as() const {
        return reinterpret_cast<U*>(p);
    }
};
template <typename T>
using Pinned = Owned<T, true>;
// a table of n records: the count travels with the pointer (upload_table)
template <typename T>
struct Table {
    Owned<T> buf;
    uint32_t n = 0;
};

// One allocation divided into sub-buffers, each starting 256-byte aligned.  On a null base the
// same sequence of takes gives the bytes the allocation needs (used()).
struct Carve {
    uintptr_t base, q;
    explicit Carve(void* b) : base((uintptr_t)b), q((uintptr_t)b) {}
    template <typename T = void>
    T* take(size_t n) {
        const uintptr_t r = q;
        q += (n + 255) & ~(size_t)255;
        return reinterpret_cast<T*>(r);
    }
    size_t used() const { return (size_t)(q - base); }
};

struct vpx_ctx {
    int device = 0;
    uint32_t cus = 256;  // compute units of the device (the bounce pool's grid)
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    struct GridBuf {
        Owned<uint8_t> ptr;
        Owned<uint64_t> l1, l2;
        Owned<uint8_t> dfp;  // distance-field octant planes (build_planes_k)
        uint32_t n = 0, nb1 = 0, nb2 = 0, nb3 = 0;
        uint64_t plane() const { return 64ull * nb2 * nb2 * nb2; }
    };
    std::vector<GridBuf> grids;
    // resident .vox models (vpx_model_upload) and what a load needs, allocated with the first
    // model so that vpx_grid_load_model allocates nothing: the xorshift32 jump tables followed
    // by the load's plan (d_model_aux, the plan staged in the pinned h_plan)
    struct ModelBuf {
        Owned<uint8_t> vox;  // voxel_data, sx*sy*sz bytes
        Owned<uint8_t> mat;  // random materials, whole chunks of model::kChunk
        uint32_t sx = 0, sy = 0, sz = 0;
    };
    std::vector<ModelBuf> models;
    Owned<uint8_t> d_model_aux;
    Pinned<uint8_t> h_plan;
    // the level refresh's record (refresh_begin), allocated with the context's first edit: the
    // device copy, and pinned [0] its initial state, [1] the read-back
    Owned<RefreshDev> d_refresh;
    Pinned<RefreshDev> h_refresh;
    Owned<DevGrid> d_grids;  // grown for grids.size() records (sync_grids)
    // the volumes: the host copy (its size is the kernels' count), the device table with each
    // volume's inflated world box (lo, hi: volume_bounds); both grow together (vpx_set_volumes)
    std::vector<vpx_volume> volumes;
    Owned<vpx_volume> d_volumes;
    Owned<float4> d_vbounds;
    Owned<TlasNode> d_tlas;  // instance TLAS: nodes, then the leaf volume list (build_tlas)
    uint32_t tlas_nodes = 0;
    bool tlas_on = false;
    uint64_t tlas_always = 0;
    int last_frame_kernel = 0;  // the last launch_render's form (vpx_debug_last_frame_kernel)
    struct Bvh {  // BasicBVH: nodes, then the triangles in tri_idx order (vpx_bvh_set)
        Owned<uint32_t> img;
        uint32_t nodes = 0, tris = 0;
    } bvh;
    Owned<vpx_material> d_materials;
    Table<vpx_point_light> points;
    Table<vpx_spot_light> spots;
    Table<vpx_area_light> areas;
    Table<vpx_sphere> spheres;
    Table<vpx_triangle> triangles;
    vpx_dir_light dir{{1, 0, 0}, {0, 0, 0}};  // DirectionalLight default (DirectionalLight.h:12)
    vpx_camera cam{};
    bool have_materials = false, have_camera = false;
    // sky dome (vpx_set_sky): RGB float texels, equirectangular
    struct Sky {
        Owned<float> px;
        uint32_t w = 0, h = 0;
    } sky;
    float sky_hdr = 1.0f;
    // reference arithmetic (vpx_set_arithmetic): the host's captured rcpss / rsqrtss tables
    Owned<uint32_t> d_x86;
    X86Arith x86{nullptr, 0u, 0u, 0u, 0u};
    Owned<unsigned long long> d_ctr;  // striped work counters (vpx_wavefront.hpp flush_counters)
    // per-stage profile: event pairs around stage launches while enabled
    std::vector<hipEvent_t> prof_ev;
    std::vector<int> prof_stage;
    uint32_t prof_cap = 0, prof_used = 0;
    uint32_t prof_mask = 0xffffffffu;  // stages timed (vpx_profile_select)
    Owned<unsigned long long> d_sum;
    Owned<void> d_scratch;  // the host-memory entries' staging (run_batch); every user ends in sync_all
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    // wavefront path state (vpx_wavefront.hpp), grown on demand: one store per stream that
    // renders (the caller's stream, and each pipeline lane)
    struct WaveStore {
        Owned<void> d;
        WaveBufs w{};
        // the level fork (launch_render): a second stream for the bounce walks, forked after a
        // level's shade and joined before the next one's, so that they overlap the shadow walks
        hipStream_t fork = nullptr;
        hipEvent_t ev_fork = nullptr, ev_join = nullptr;
        bool fork_dedicated = false;  // on a CU-mask stream, counted in g_lane_queues
    };
    WaveStore wave;
    // frames in flight (vpx_set_pipeline): each lane renders a whole frame on its own library
    // stream into its own path state and packed sample buffer; the caller's stream only runs
    // the frames' composites, in frame order (each waits for its lane's render), so frame f+1's
    // walks fill the GPU while frame f's last tiles drain.  Empty: frames render on the stream.
    struct Lane {
        hipStream_t s = nullptr;
        WaveStore ws;
        Owned<float4> packed;   // the lane's frame: one float4 sample per path (tile order)
        Owned<float4> packed2;  // its second buffer (frames alternate: VPX_LANE_DOUBLE)
        hipEvent_t rendered = nullptr, consumed = nullptr, consumed2 = nullptr;
        bool used2 = false;
        uint32_t flip = 0;
        float4* cur = nullptr;             // the buffer of the lane's latest frame (lane_render)
        hipEvent_t cur_consumed = nullptr; // the event its blend records
        hipEvent_t caller = nullptr;  // the caller's stream at the frame's vpx_render (lane_tail_ok frames)
        bool used = false;
        bool dedicated = false;  // on a CU-mask stream (its own hardware queue), counted in g_lane_queues
    };
    std::vector<Lane> lanes;
    uint32_t lane_next = 0;
    // static-camera path images (float4[W*H] each): albedo, illumination, ray data, temp
    Owned<float4> rp_buf;
    // a window chain's samples when no lanes run (vpx_render_window)
    Owned<float4> win_buf;
    // vpx_denoise_ids' scratch: the keys (uint2 per pixel), then two float4 images when a call
    // ran more than one pass; carved per call for the call's size
    Owned<void> dn_buf;
    // vpx_denoise_var's scratch: the keys, then one float4 image (V0) and a second when a call ran
    // more than one pass, .w the variance; carved per call for the call's size
    Owned<void> dv_buf;
    // vpx_reproject_ids' scratch: the volume table (24 floats per volume, then a moved flag per
    // volume) and, in the VPX_REPROJECT_PREKEY form, the previous keys; rj_host: the table's pinned
    // staging copy, rewritten only after rj_ev (its last upload) has passed; rj_last: the table the
    // device holds, so that an unchanged one is not uploaded again
    Owned<void> rj_buf;
    Pinned<void> rj_host;
    hipEvent_t rj_ev = nullptr;
    std::vector<uint32_t> rj_last;
    // vpx_cast_*: the pool form's grab block (kGrabBlock words, zeroed on the stream per call; comes
    // with the first call), and what the last call launched (vpx_debug_last_cast_kernel)
    Owned<uint32_t> cast_grab;
    int last_cast = 0;
    // device set (vpx_create_multi): one member context per device; this context only
    // forwards (VPX_GROUP_*) and runs the tile-sharded vpx_render (group_render)
    struct Member {
        vpx_ctx* ctx = nullptr;
        Owned<void> packed;       // packed float4 samples / RGB8 (member device)
        Owned<float> accum;       // packed accumulator (accum == NULL mode)
        hipEvent_t ev = nullptr;  // its render done (copy path)
    };
    std::vector<Member> members;
    std::vector<ncclComm_t> comms;  // RCCL, one per member (distinct devices only)
    Owned<void> g_gathered;         // member 0's device: the members' packed buffers back to back
    hipEvent_t g_copied = nullptr;  // member 0: gather copies done (copy path)
    // display interop (vpx_gl_*): a registered GL pixel-unpack buffer on this context's
    // device (device set: devices[0]); mapped between vpx_gl_map and vpx_gl_unmap
    hipGraphicsResource_t gl_res = nullptr;
    bool gl_mapped = false;
};

namespace {

int fail(vpx_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}

// Wait for everything the context has queued: its stream and its pipeline lanes (frames in
// flight read the world, tables and path buffers that later calls may replace).
hipError_t sync_all(vpx_ctx* c) {
    for (const auto& l : c->lanes)
        if (l.s) {
            const hipError_t e = hipStreamSynchronize(l.s);
            if (e != hipSuccess) return e;
        }
    return hipStreamSynchronize(c->stream);
}

// The caller's current HIP device, restored when the scope ends: a device-set call sets each
// member's device in turn and must not leave the caller on the last one (torch tensors or
// buffers the caller allocates afterwards belong on devices[0]).
struct DeviceGuard {
    int dev = -1;
    DeviceGuard() {
        if (hipGetDevice(&dev) != hipSuccess) dev = -1;
    }
    ~DeviceGuard() {
        if (dev >= 0) (void)hipSetDevice(dev);
    }
};

// Device-set contexts forward to their members: every member (uploads / state) or member 0
// (unit entries, profiles, the single-image static-camera path, the rank-level primitives).
template <class F>
int group_all(vpx_ctx* c, F f) {
    DeviceGuard keep;
    for (const auto& mem : c->members) {
        vpx_ctx* m = mem.ctx;
        if (hipSetDevice(m->device) != hipSuccess) return fail(c, VPX_E_DEVICE, "hipSetDevice");
        const int rc = f(m);
        if (rc) return fail(c, rc, "device " + std::to_string(m->device) + ": " + m->err);
    }
    return VPX_OK;
}
template <class F>
int group_first(vpx_ctx* c, F f) {
    DeviceGuard keep;
    vpx_ctx* m = c->members[0].ctx;
    if (hipSetDevice(m->device) != hipSuccess) return fail(c, VPX_E_DEVICE, "hipSetDevice");
    const int rc = f(m);
    return rc ? fail(c, rc, m->err) : VPX_OK;
}
#define VPX_GROUP_ALL(c, call) \
    if ((c) && !(c)->members.empty()) return group_all((c), [&](vpx_ctx* m_) { return call; })
#define VPX_GROUP_FIRST(c, call) \
    if ((c) && !(c)->members.empty()) return group_first((c), [&](vpx_ctx* m_) { return call; })

// A table replaced: the old one goes first and the count with it, so a failure leaves the table
// empty with count 0 (the caller has waited for the frames that read it).
template <typename T>
int upload_table(vpx_ctx* c, Table<T>& t, const T* src, uint32_t n) {
    t.buf.release();
    t.n = 0;
    if (n == 0) return VPX_OK;
    if (!src) return fail(c, VPX_E_INVALID, "null table with non-zero count");
    VPX_HIP(c, t.buf.alloc(sizeof(T) * n));
    VPX_HIP(c, hipMemcpyAsync(t.buf, src, sizeof(T) * n, hipMemcpyHostToDevice, c->stream));
    t.n = n;
    return VPX_OK;
}

// No wait before the old scratch goes: every user of d_scratch ends in sync_all, so nothing
// queued still reads it.
int ensure_scratch(vpx_ctx* c, size_t bytes) { return c->d_scratch.grow(c, bytes, false); }

// The entries that take and return host memory: the inputs are uploaded into the scratch, `run`
// launches on c->stream with the device pointers (din[i], dout[j], in the order given), the
// outputs come back, and the call ends synchronised.  An output with a null host pointer still
// gets its device buffer; it is only not fetched.
struct HostIn {
    const void* host;
    size_t bytes;
};
struct HostOut {
    void* host;
    size_t bytes;
};
template <typename Run>
int run_batch(vpx_ctx* c, std::initializer_list<HostIn> in, std::initializer_list<HostOut> out, Run run) {
    constexpr size_t kMost = 4;
    void *din[kMost] = {}, *dout[kMost] = {};
    if (in.size() > kMost || out.size() > kMost) return fail(c, VPX_E_INVALID, "run_batch: too many buffers");
    auto carve = [&](Carve cv) {
        size_t i = 0, o = 0;
        for (const HostIn& b : in) din[i++] = cv.take(b.bytes);
        for (const HostOut& b : out) dout[o++] = cv.take(b.bytes);
        return cv.used();
    };
    if (int rc = ensure_scratch(c, carve(Carve(nullptr)))) return rc;
    carve(Carve(c->d_scratch));
    size_t i = 0, o = 0;
    for (const HostIn& b : in) VPX_HIP(c, hipMemcpyAsync(din[i++], b.host, b.bytes, hipMemcpyHostToDevice, c->stream));
    run(din, dout);
    VPX_HIP(c, hipGetLastError());
    for (const HostOut& b : out) {
        if (b.host) VPX_HIP(c, hipMemcpyAsync(b.host, dout[o], b.bytes, hipMemcpyDeviceToHost, c->stream));
        ++o;
    }
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

// the constant sky of the query entries (misses report it; vpx_focus_distance has its own)
constexpr float kQuerySky[3] = {0.392f, 0.584f, 0.829f};

int check_ready(vpx_ctx* c) {
    if (c->volumes.empty()) return fail(c, VPX_E_STATE, "no volumes set (vpx_set_volumes)");
    if (!c->have_materials) return fail(c, VPX_E_STATE, "no materials set (vpx_set_materials)");
    for (const auto& v : c->volumes) {
        if (v.grid_id >= c->grids.size() || !c->grids[v.grid_id].ptr)
            return fail(c, VPX_E_STATE, "volume references a grid that was not uploaded");
    }
    return VPX_OK;
}

int sync_grids(vpx_ctx* c) {
    const uint32_t n = (uint32_t)c->grids.size();
    // no wait of its own: its callers (alloc_grid's) have waited for the frames in flight
    if (int rc = c->d_grids.grow(c, sizeof(DevGrid) * n, false)) return rc;
    std::vector<DevGrid> h(n);
    for (uint32_t i = 0; i < n; ++i) {
        const auto& g = c->grids[i];
        h[i] = DevGrid{g.ptr, g.l1, g.l2, g.n, g.nb1, g.nb2, g.nb3, g.dfp, g.plane()};
    }
    if (n) VPX_HIP(c, hipMemcpy(c->d_grids, h.data(), sizeof(DevGrid) * n, hipMemcpyHostToDevice));
    return VPX_OK;
}

SceneView view_of(const vpx_ctx* c, const float sky[3], int32_t area_samples, bool sky_tex = false) {
    SceneView sv;
    sv.grids = c->d_grids;
    sv.volumes = c->d_volumes;
    sv.vbounds = c->d_vbounds;
    sv.tlas = c->d_tlas;
    sv.tlas_on = c->tlas_on ? 1u : 0u;
    sv.tlas_nodes = c->tlas_nodes;
    sv.tlas_always = c->tlas_always;
    sv.materials = c->d_materials;
    sv.points = c->points.buf;
    sv.spots = c->spots.buf;
    sv.areas = c->areas.buf;
    sv.spheres = c->spheres.buf;
    sv.triangles = c->triangles.buf;
    sv.num_volumes = (uint32_t)c->volumes.size();
    sv.num_points = c->points.n;
    sv.num_spots = c->spots.n;
    sv.num_areas = c->areas.n;
    sv.num_spheres = c->spheres.n;
    sv.num_triangles = c->triangles.n;
    sv.dir = c->dir;
    sv.sky[0] = sky[0], sv.sky[1] = sky[1], sv.sky[2] = sky[2];
    sv.area_samples = area_samples;
    sv.sky_px = c->sky.px;
    sv.sky_w = c->sky.w, sv.sky_h = c->sky.h;
    sv.sky_hdr = c->sky_hdr;
    sv.sky_tex = (sky_tex && c->sky.px) ? 1u : 0u;
    sv.x86 = c->x86;
    // one grid for every volume after the world: lane_volumes (vpx_trace.hpp)
    sv.inst_grid = -1;
    for (size_t i = 1; i < c->volumes.size(); ++i) {
        const int32_t gi = (int32_t)c->volumes[i].grid_id;
        if (i == 1) sv.inst_grid = gi;
        else if (gi != sv.inst_grid) { sv.inst_grid = -1; break; }
    }
    return sv;
}

FrameArgs frame_of(const vpx_ctx* c, const vpx_frame_params* p, uint32_t rank, uint32_t n_ranks) {
    FrameArgs f;
    f.cam = c->cam;
    f.width = p->width;
    f.height = p->height;
    f.max_bounces = p->max_bounces;
    f.frame_index = p->frame_index;
    f.seed_base = p->seed_base;
    f.flags = p->flags;
    f.aa = p->aa_strength;
    f.weight = 1.0f / ((float)p->frame_index + 1.0f);  // renderer.cpp:1651
    f.inv_weight = 1.0f - f.weight;
    f.tiles_x = (p->width + kTile - 1) / kTile;
    f.tiles_y = (p->height + kTile - 1) / kTile;
    f.num_tiles = f.tiles_x * f.tiles_y;
    f.rank = rank;
    f.n_ranks = n_ranks;
    f.tiles_per_rank = (f.num_tiles + n_ranks - 1) / n_ranks;
    f.batch_tiles = 0;
    return f;
}

int validate_frame(vpx_ctx* c, const vpx_frame_params* p) {
    if (!p) return fail(c, VPX_E_INVALID, "null frame params");
    if (p->width == 0 || p->height == 0 || p->width > 32768 || p->height > 32768)
        return fail(c, VPX_E_INVALID, "frame size out of range");
    // the shadow lists pack a path index into 27 bits beside the slot number (shadow_tile)
    if ((uint64_t)((p->width + kTile - 1) / kTile) * ((p->height + kTile - 1) / kTile) * (uint64_t)kTilePix > (1ull << 27))
        return fail(c, VPX_E_INVALID, "frame larger than 2^27 tile-padded pixels");
    if (p->max_bounces < -1 || p->max_bounces > kMaxLevels - 2)
        return fail(c, VPX_E_INVALID, "max_bounces must be in [-1, 14]");
    if (p->area_samples < 0 || p->area_samples > 15) return fail(c, VPX_E_INVALID, "area_samples must be in [0, 15]");
    if (!c->have_camera) return fail(c, VPX_E_STATE, "no camera set (vpx_set_camera)");
    if ((p->flags & VPX_FLAG_SKY) && !c->sky.px)
        return fail(c, VPX_E_STATE, "VPX_FLAG_SKY without a sky texture (vpx_set_sky)");
    return check_ready(c);
}

// The wavefront buffers for P paths, L levels and S shadow slots, taken in this order from one
// allocation: the same sequence sizes it (on a null base) and divides it.
void carve_wave(Carve& cv, WaveBufs& w, uint32_t P, uint32_t L, uint32_t S) {
    const size_t f4 = sizeof(float4);
    w.P = P;
    w.S = S;
    w.O = cv.take<float4>(f4 * P);
    w.D = cv.take<float4>(f4 * P);
    w.H = cv.take<float4>(f4 * P);
    w.leaf = cv.take<float4>(f4 * P);
    w.SM = cv.take<float4>(f4 * P);
    w.LA = cv.take<float4>(f4 * P * (size_t)L);
    w.LB = cv.take<float4>(f4 * P * (size_t)L);
    w.SO = cv.take<float4>(f4 * P * (size_t)S);
    w.SD = cv.take<float4>(f4 * P * (size_t)S);
    w.SL = cv.take<float4>(f4 * P * (size_t)S);
    w.HM = cv.take<uint32_t>(4 * (size_t)P);
    w.depth = cv.take<int32_t>(4 * (size_t)P);
    w.forms = cv.take<uint32_t>(4 * (size_t)P);
    w.smask = cv.take<uint32_t>(4 * (size_t)P);
    w.live0 = cv.take<uint32_t>(4 * (size_t)P);
    w.live1 = cv.take<uint32_t>(4 * (size_t)P);
    w.amask = cv.take<uint64_t>((size_t)P / 8);  // P is a multiple of 256
    w.pool = cv.take<uint32_t>(sizeof(uint32_t) * kPoolWords);
    w.occb = cv.take<uint8_t>((size_t)P * S);
    (void)cv.take(sizeof(uint32_t) * (size_t)P * S);  // slot_list (vpx_wavefront.hpp), right after occb
}

// Grown on demand, never inside a capture; a store that is replaced waits for the frames in
// flight, which still walk in the old one.
int ensure_wave(vpx_ctx* c, vpx_ctx::WaveStore& ws, uint32_t P, uint32_t L, uint32_t S) {
    Carve size(nullptr);
    WaveBufs sized{};
    carve_wave(size, sized, P, L, S);
    if (int rc = ws.d.grow(c, size.used(), true)) return rc;
    Carve cv(ws.d);
    carve_wave(cv, ws.w, P, L, S);
    return VPX_OK;
}

std::atomic<int> g_lane_queues{0};
constexpr int kMaxLaneQueues = 16;

// The level fork's stream and events (created on first use): a CU-mask stream of all the
// device's CUs (a hardware queue of its own) while the process's lane-queue cap allows, else
// a plain non-blocking stream.  Its work always joins back into the owner's stream within the
// frame, so synchronising the owner covers it.
void free_fork(vpx_ctx::WaveStore& ws);
int ensure_fork(vpx_ctx* c, vpx_ctx::WaveStore& ws) {
    if (ws.fork && ws.ev_fork && ws.ev_join) return VPX_OK;
    free_fork(ws);  // a partly created fork (an earlier failure): start clean
    std::vector<uint32_t> all_cus((c->cus + 31u) / 32u, 0xffffffffu);
    ws.fork_dedicated = g_lane_queues.fetch_add(1) < kMaxLaneQueues;
    if (!ws.fork_dedicated) g_lane_queues.fetch_sub(1);
    const hipError_t se = ws.fork_dedicated
                              ? hipExtStreamCreateWithCUMask(&ws.fork, (uint32_t)all_cus.size(), all_cus.data())
                              : hipStreamCreateWithFlags(&ws.fork, hipStreamNonBlocking);
    if (se != hipSuccess) ws.fork = nullptr;
    if (se != hipSuccess || hipEventCreateWithFlags(&ws.ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&ws.ev_join, hipEventDisableTiming) != hipSuccess) {
        free_fork(ws);  // releases the counted queue and whatever was created
        return fail(c, VPX_E_DEVICE, "level fork: stream / event creation failed");
    }
    return VPX_OK;
}
void free_fork(vpx_ctx::WaveStore& ws) {
    if (ws.fork) (void)hipStreamSynchronize(ws.fork);
    if (ws.ev_fork) (void)hipEventDestroy(ws.ev_fork);
    if (ws.ev_join) (void)hipEventDestroy(ws.ev_join);
    if (ws.fork) (void)hipStreamDestroy(ws.fork);
    if (ws.fork_dedicated) g_lane_queues.fetch_sub(1);
    ws.fork = nullptr, ws.ev_fork = ws.ev_join = nullptr, ws.fork_dedicated = false;
}

// Profile marks: a stage's start (stage >= 0) or end (-1) event on the stream, while the
// event pool lasts; a start without room for its end is not recorded.
static void prof_mark(vpx_ctx* c, hipStream_t s, int stage) {
    if (!c->prof_cap) return;
    if (stage >= 0 && !((c->prof_mask >> stage) & 1u)) return;  // not selected (its end is dropped too)
    if (stage >= 0 && c->prof_used + 2 > c->prof_cap) return;
    if (stage < 0 && (c->prof_used & 1u) == 0) return;  // its start was dropped
    if (hipEventRecord(c->prof_ev[c->prof_used], s) != hipSuccess) return;
    c->prof_stage[c->prof_used] = stage;
    ++c->prof_used;
}

// The frame: primary -> [shade -> shadow -> resolve -> nearest]* -> finish, all on
// c->stream, one 256-thread workgroup per 16x16 tile in every kernel.
struct Reproj {  // the static-camera tail (vpx_render_reproject)
    PrevCam prev;
    float4 *alb, *ill, *rd, *temp, *hist;
};

// tail_wait: an event the frame's separate tail launch (k_resolve_finish, after the shadow
// pool) waits for — frames in flight that blend on their own lane (lane_tail_ok).  wtail: a
// window chain (tiles = B frames' tiles) whose separate tail blends its frames in order
// (k_finish_window) instead of writing samples.
template <int MODE>
int launch_render(vpx_ctx* c, hipStream_t s, vpx_ctx::WaveStore& ws, const SceneView& sv, const FrameArgs& f,
                  uint32_t tiles, float4* accum, uint32_t* rgb8, float4* packed, const Reproj* rp = nullptr,
                  const hipEvent_t* tail_wait = nullptr, const WindowTail* wtail = nullptr) {
    const uint32_t P = tiles * (uint32_t)kTilePix;
    const uint32_t L = (uint32_t)std::max(1, f.max_bounces + 1);
    // shadow slots per path: an area-light sample each, else one (point / spot / directional
    // lights and the smoke probe use slot 0 only)
    const uint32_t S = sv.num_areas ? (uint32_t)std::max(1, sv.area_samples) : 1u;
    int rc = ensure_wave(c, ws, P, L, S);
    if (rc) return rc;
    WaveBufs w = ws.w;
    if (rp) w.RD = rp->rd;
    const dim3 grid(tiles), block(kThreads);
    const size_t slds = sizeof(uint32_t) * S * kThreads;
    // single volume, no analytic shapes: the DDA kernels' lean instances
    const bool one = sv.num_volumes == 1 && !(sv.num_spheres | sv.num_triangles);
    const bool x86 = sv.x86.tab != nullptr;  // the reference-arithmetic instances of the hot kernels
    // the multi-volume walkers' rcp table in LDS (x86_stage_lds): its dynamic LDS bytes
    const size_t xlds = x86 ? sizeof(uint32_t) * sv.x86.rsq_off : 0;
    // the last level's shadow -> resolve -> finish as one launch (k_shadow_finish), except
    // on the static-camera path, whose tail is the reprojection
    const bool fuse_tail = !rp;
    // The shadow pool (k_shadow_pool, results in occb) for the single-volume walks towards area
    // lights (several slots per path, long walks), except on the static-camera path (its
    // reprojection test reads the tile kernel's SD flags).  Measured (ms per step, two runs
    // each, pool / tile kernels): C3 3.72, 3.71 / 4.96, 4.94; C2 (one point light, one slot per
    // path) 2.83, 2.84 / 2.64, 2.71 (round 3) — so point / spot / directional lights kept the
    // tile kernels; since round 6 single-volume frames in flight use the pool for them too
    // (VPX_SPOOL_ONE_SLOT below: C2 -2.4 %).
    // Multi-volume / shape scenes: the world's walks (volume 0, first in IsOccluded's loop) in
    // the pool, the rest of the loop for the slots the world left unoccluded: k_shadow_inst per
    // tile (round 3: C4 51.7 -> 47.6 ms per 16-spp step), then (round 6) k_shadow_slots over the
    // pool's list of the slots whose segment may meet a later volume.
// Round 6: single-volume frames with one slot per path (C2's point light) through the pool
// too — C2 at 3 lanes 2.294-2.353 vs 2.352-2.400 ms per step (three interleaved runs; at 2
// lanes with forks 2.45-2.47 vs 2.40-2.41).  (Round 3, before the live lists and the lanes'
// double buffers, it had measured 2.83 vs 2.64-2.71.)
#ifndef VPX_SPOOL_ONE_SLOT
#define VPX_SPOOL_ONE_SLOT 1
#endif
// Only for frames in flight: the serial frames (the context's stream, with the level fork)
// keep the tile kernels — C2 serial 3.32-3.33 ms per frame vs 3.51-3.54 with the pool (tile
// kernels everywhere: 3.31-3.35 serial, 2.35-2.39 in flight; three interleaved runs).
#ifndef VPX_SPOOL_ONE_SERIAL
#define VPX_SPOOL_ONE_SERIAL 0
#endif
    const bool spool = !rp && (S > 1 || (one && VPX_SPOOL_ONE_SLOT && (VPX_SPOOL_ONE_SERIAL || &ws != &c->wave)));
    if (wtail && (!spool || f.max_bounces < 0 || !f.batch_tiles || tiles % wtail->B))
        return fail(c, VPX_E_INVALID, "window tail: needs a window chain with the shadow pool");
    if (!spool) w.occb = nullptr;  // k_resolve reads the slots' SD flags
    const uint32_t sgrab = std::max(1u, std::min(4u, kShadowList / (64u * S)));
    // persistent launches over a level's live list (its length is on the device): as many
    // workgroups as the device keeps resident, capped by the frame's tiles
    auto resident = [&](uint32_t waves_per_simd) { return dim3(std::min(tiles, c->cus * waves_per_simd)); };
    auto shadow_pool = [&](int level) {
        const uint32_t grabs = (P / 64u + sgrab - 1u) / sgrab;
        const uint32_t waves = std::min(grabs, c->cus * 4u * (uint32_t)VPX_WPE_SPOOL);
        const uint32_t wpb = kPoolWg / 64u;
        hipLaunchKernelGGL(one ? k_shadow_pool<false> : k_shadow_pool<true>, dim3((waves + wpb - 1u) / wpb), dim3(kPoolWg), 0,
                           s, sv, w, level, sgrab, c->d_ctr);
        if (!one)  // the pool's list of the slots a later volume may occlude
            hipLaunchKernelGGL(k_shadow_slots, dim3(std::min(tiles * S, c->cus * (uint32_t)VPX_WPE_SHADOW_SLOTS)), block, 0, s, sv,
                               w, level, c->d_ctr);
    };
    c->last_frame_kernel = 0;
    if (frame0_fits(sv, f, S, rp != nullptr) && tiles <= kFuseFrameTiles) {
        // the whole depth-0 frame in one launch (k_frame0), its path state and one shadow slot
        // per path in LDS; with area lights the frame splits to use the shadow pool.
        // frame0_fits is what the kernel's kFrameGuaranteed view folds in as constants, and
        // frame0_lean what kFrameLean adds (vpx_wavefront.hpp, side by side with the views): the
        // form is chosen here, from the same sv / f the kernel receives.
        prof_mark(c, s, VPX_STAGE_FRAME);
#ifndef VPX_FRAME_EXTRA_LDS
#define VPX_FRAME_EXTRA_LDS 0  // A/B hook: bytes of unused LDS added per k_frame0 workgroup (occupancy sensitivity)
#endif
// The views that are built and launched: 2 = lean where frame0_lean holds, else guaranteed;
// 1 = guaranteed only; 0 = the kernel as it was, on the runtime values (the A/B baseline).
#ifndef VPX_FRAME_VIEWS
#define VPX_FRAME_VIEWS 2
#endif
        constexpr int kBase = VPX_FRAME_VIEWS >= 1 ? kFrameGuaranteed : kFrameAsGiven;
        constexpr int kLean = VPX_FRAME_VIEWS >= 2 ? kFrameLean : kBase;
        const bool lean = VPX_FRAME_VIEWS >= 2 && frame0_lean(sv, f);
        c->last_frame_kernel = lean ? 2 : 1;
        hipLaunchKernelGGL((lean ? (x86 ? k_frame0<true, MODE, true, kLean> : k_frame0<true, MODE, false, kLean>)
                                 : (x86 ? k_frame0<true, MODE, true, kBase> : k_frame0<true, MODE, false, kBase>)),
                           grid, block, VPX_FRAME_EXTRA_LDS, s, sv, f, w, c->d_ctr, accum, rgb8, packed);
        prof_mark(c, s, -1);
        VPX_HIP(c, hipGetLastError());
        return VPX_OK;
    }
    // the frame's level counters (grabs, live-list lengths; kPool*): zeroed before the head,
    // whose level-0 shade appends level 1's list
    VPX_HIP(c, hipMemsetAsync(w.pool, 0, sizeof(uint32_t) * kPoolWords, s));
    prof_mark(c, s, VPX_STAGE_PRIMARY);
    const bool fuse_head = f.max_bounces >= 0;  // level 0's shade at the end of k_primary
    // multi-volume / shape scenes: the world walk in the lean head, then the instance pass
    // (the rest of FindNearest for the rays that can still meet a later volume or a shape, and
    // level 0's shade; k_instances)
    // (scenes with analytic shapes test them on every ray, so no ray skips the second pass
    // there: they keep the one-launch kernel — Z1 2.61-2.62 vs 2.63 ms split, round 4)
    const bool split = !one && fuse_head && VPX_SPLIT_PRIMARY && !(sv.num_spheres | sv.num_triangles);
    // at depth 0 the world head shades the paths that cannot meet an instance itself and the
    // instance pass takes only the others (k_primary / k_instances DEFER)
    const bool defer = split && f.max_bounces == 0 && VPX_DEFER_INSTANCES;
    if (defer)
        hipLaunchKernelGGL((x86 ? k_primary<true, true, true, true> : k_primary<true, true, false, true>), grid, block, 0, s,
                           sv, f, w, c->d_ctr);
    else if (split)
        hipLaunchKernelGGL((x86 ? k_primary<true, false, true> : k_primary<true, false, false>), grid, block, 0, s, sv, f, w,
                           c->d_ctr);
    else if (fuse_head)
        hipLaunchKernelGGL((one ? (x86 ? k_primary<true, true, true> : k_primary<true, true, false>)
                                : (x86 ? k_primary<false, true, true> : k_primary<false, true, false>)),
                           grid, block, 0, s, sv, f, w,
                           c->d_ctr);
    else
        hipLaunchKernelGGL((one ? (x86 ? k_primary<true, false, true> : k_primary<true, false, false>)
                                : (x86 ? k_primary<false, false, true> : k_primary<false, false, false>)),
                           grid, block, 0, s, sv, f,
                           w, c->d_ctr);
    prof_mark(c, s, -1);
    if (split) {
        prof_mark(c, s, VPX_STAGE_INSTANCES);
        if (defer) {  // the deferred paths as a dense list (k_compact), then k_instances_list
            hipLaunchKernelGGL(k_compact, dim3((P / 64u + 255u) / 256u), block, 0, s, w, 0);
            hipLaunchKernelGGL(k_instances_list, grid, block, xlds, s, sv, f, w, c->d_ctr);
        } else {
            hipLaunchKernelGGL(k_instances, grid, block, xlds, s, sv, f, w, c->d_ctr);
        }
        prof_mark(c, s, -1);
    }
    // FindNearest for the traced rays of the next level: the bounce pool (single volume, no
    // shapes) or the tile kernel
    auto bounce = [&](hipStream_t bs, int level) {
        prof_mark(c, bs, VPX_STAGE_BOUNCE);
        if (one) {  // the bounce pool: persistent waves, as many as the device keeps resident
            const uint32_t chunks = (P + kPoolChunk - 1u) / kPoolChunk;
            const uint32_t waves = std::min(chunks, c->cus * 4u * (uint32_t)VPX_WPE_BOUNCE);
            const uint32_t wpb = kPoolWg / 64u;
            hipLaunchKernelGGL(x86 ? k_nearest_pool<true> : k_nearest_pool<false>, dim3((waves + wpb - 1u) / wpb),
                               dim3(kPoolWg), 0, bs, sv, w, level,
                               c->d_ctr);
        } else {  // multi-volume / shape scenes: persistent waves over the live list, 64 rays a grab
            hipLaunchKernelGGL(k_nearest_tile, grid, block, xlds, bs, sv, w, level, c->d_ctr);
        }
        prof_mark(c, bs, -1);
    };
    // Where it pays (ms per step, one MI355X, tools/gpu_r4h/j/k.sh): every frame on the
    // context's stream (serial C2 3.70-3.74 vs 4.49-4.54, Z1 3.44-3.47 vs 3.89-3.90), and
    // single-volume frames in flight with at most two lanes (C2 at 2 lanes 2.50-2.52 vs 2.65-2.67
    // at the 3 lanes without forks).  Not with three or more lanes (C2 3.17-3.28 at 3, 4.0-4.3 at
    // 4: more dedicated queues than the device runs at once; forks from the shared queue pool
    // 2.80-2.86), nor for multi-volume / shape frames in flight (Z1 3.20-3.25 at 2 lanes vs
    // 2.50 at 3 without).
    const bool fork = VPX_LEVEL_FORK && f.max_bounces > 0 && !rp && (&ws == &c->wave || (one && c->lanes.size() <= 2));
    if (fork && (rc = ensure_fork(c, ws))) return rc;
    // deep frames: the levels from tail_from on in one launch (k_tail), then k_finish
    // (frames on the context's stream — a per-frame synchronous Tick — start it a level earlier:
    // with no other frame to overlap, the per-level latency costs more; Z1 serial 2.50 from
    // level 6 vs 2.65 from 7, 2.69 from 5; frames in flight 1.54 from 7 vs 1.56-1.64 from 6)
    const int tail_at = &ws == &c->wave ? VPX_TAIL_LEVEL - 1 : VPX_TAIL_LEVEL;
    const int tail_from = (VPX_TAIL_LEVEL > 0 && f.max_bounces >= VPX_TAIL_MIN_DEPTH && !rp) ? tail_at : -1;
    bool tailed = false;
    // the last level's shadow -> resolve -> finish as one launch (k_shadow_finish)
    for (int level = 0; level <= f.max_bounces; ++level) {
        if (!(fuse_head && level == 0)) {  // (level >= 1: the head shades level 0)
            prof_mark(c, s, VPX_STAGE_SHADE);
            hipLaunchKernelGGL(k_shade, grid, block, 0, s, sv, f, w, level, c->d_ctr);
            prof_mark(c, s, -1);
        }
        if (fuse_tail && level == f.max_bounces) {
            prof_mark(c, s, VPX_STAGE_SHADOW);
            if (spool)
                shadow_pool(level);
            else
                hipLaunchKernelGGL((one ? k_shadow_finish<true, MODE> : k_shadow_finish<false, MODE>), grid, block,
                                   slds, s, sv, f, w, c->d_ctr, accum, rgb8, packed);
            prof_mark(c, s, -1);
            if (spool) {
                if (tail_wait) VPX_HIP(c, hipStreamWaitEvent(s, *tail_wait, 0));
                prof_mark(c, s, VPX_STAGE_FINISH);
                if (wtail)
                    hipLaunchKernelGGL(k_finish_window<true>, dim3(tiles / wtail->B), block, 0, s, sv, f, w, *wtail,
                                       accum, rgb8);
                else
                    hipLaunchKernelGGL((k_resolve_finish<MODE>), grid, block, 0, s, sv, f, w, accum, rgb8, packed);
                prof_mark(c, s, -1);
            }
            break;
        }
        // the next level's live list from this level's shade bits
        if (level < f.max_bounces)
            hipLaunchKernelGGL(k_compact, dim3((P / 64u + 255u) / 256u), block, 0, s, w, level);
        // the level fork: the next level's bounce walks read only the rays and live list this
        // level's shade and k_compact wrote and write only the hit records, which the shadow
        // walks and the light sums do not touch — so they run beside them on the fork stream
        const bool tail_next = level + 1 == tail_from;  // the next levels run in k_tail
        const bool forked = fork && level < f.max_bounces && !tail_next;
        if (forked) {
            VPX_HIP(c, hipEventRecord(ws.ev_fork, s));
            VPX_HIP(c, hipStreamWaitEvent(ws.fork, ws.ev_fork, 0));
            bounce(ws.fork, level);
            VPX_HIP(c, hipEventRecord(ws.ev_join, ws.fork));
        }
        prof_mark(c, s, VPX_STAGE_SHADOW);
        if (spool)
            shadow_pool(level);
        else if (level == 0)
            hipLaunchKernelGGL(one ? k_shadow_tile<true> : k_shadow_tile<false>, grid, block, slds, s, sv, w, c->d_ctr);
        else
            hipLaunchKernelGGL(one ? k_shadow_list<true> : k_shadow_list<false>, grid, block, slds, s, sv, w, level,
                               c->d_ctr);
        prof_mark(c, s, -1);
        prof_mark(c, s, VPX_STAGE_RESOLVE);
        hipLaunchKernelGGL(k_resolve, level ? resident(8) : grid, block, 0, s, sv, w, level);
        prof_mark(c, s, -1);
        if (forked)
            VPX_HIP(c, hipStreamWaitEvent(s, ws.ev_join, 0));
        else if (level < f.max_bounces && !tail_next)
            bounce(s, level);
        if (tail_next) {
            WaveBufs wt = w;
            wt.occb = nullptr;  // k_tail marks occluded slots in their SD words, as the tile kernels do
            prof_mark(c, s, VPX_STAGE_BOUNCE);
            hipLaunchKernelGGL(k_tail, grid, block, xlds, s, sv, f, wt, level + 1, c->d_ctr);
            prof_mark(c, s, -1);
            tailed = true;
            break;
        }
    }
    // (fused tail: k_shadow_finish already finished the frame; max_bounces = -1 runs no
    // level, so the finish folds the zero leaf here)
    const bool finished = fuse_tail && f.max_bounces >= 0 && !tailed;
    // a frame in flight that blends on its lane (tail_wait) blends here when k_tail ran: the
    // blend must follow the caller's earlier writes and the previous frame's blend
    if (!finished && tail_wait) VPX_HIP(c, hipStreamWaitEvent(s, *tail_wait, 0));
    if (!finished) prof_mark(c, s, VPX_STAGE_FINISH);
    if (!rp) {
        if (!finished && wtail)
            hipLaunchKernelGGL(k_finish_window<false>, dim3(tiles / wtail->B), block, 0, s, sv, f, w, *wtail, accum,
                               rgb8);
        else if (!finished)
            hipLaunchKernelGGL((k_finish<MODE>), grid, block, 0, s, f, w, accum, rgb8, packed);
    } else {  // Renderer::Tick static branch, second pass (renderer.cpp:2024-2100)
        hipLaunchKernelGGL(k_finish_reproject, grid, block, 0, s, f, w, rp->alb, rp->ill);
        hipLaunchKernelGGL(k_reproject_setup, grid, block, 0, s, f, w, rp->prev);
        hipLaunchKernelGGL(one ? k_shadow_tile<true> : k_shadow_tile<false>, grid, block, slds, s, sv, w, c->d_ctr);
        hipLaunchKernelGGL(k_reproject_resolve, grid, block, 0, s, f, w, rp->alb, rp->ill, rp->hist, rp->temp,
                           rgb8);
        VPX_HIP(c, hipMemcpyAsync(rp->hist, rp->temp, sizeof(float4) * (size_t)f.width * f.height,
                                  hipMemcpyDeviceToDevice, s));  // history = temp
    }
    if (!finished) prof_mark(c, s, -1);
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

// Whether a frame's blend can run as its own tail launch on the lane (launch_render's spool
// tail, k_resolve_finish): area lights with several samples (the shadow pool).
bool lane_tail_ok(const SceneView& sv, const FrameArgs& f) {
    const uint32_t S = sv.num_areas ? (uint32_t)std::max(1, sv.area_samples) : 1u;
    return VPX_LANE_TAIL && S > 1 && f.max_bounces >= 0;
}

// Frames in flight: render `tiles` tiles of frame f as packed float4 samples (into `out`, or
// the lane's own buffer when null) on the next lane's stream, in that lane's path state; the
// caller's stream waits for the render.  The caller then queues the frame's composite on
// s and records the lane's `consumed` event after it.
int lane_render(vpx_ctx* c, const SceneView& sv, const FrameArgs& f, uint32_t tiles, float4* out, vpx_ctx::Lane*& lane) {
    vpx_ctx::Lane& L = c->lanes[c->lane_next];
    c->lane_next = (c->lane_next + 1u) % (uint32_t)c->lanes.size();
    float4* dst = out;
    // Two sample buffers per lane, alternating: the lane's next frame waits only for the blend
    // of the frame before its previous one, not for the previous one's (which waits for every
    // earlier blend on the caller's stream).  The path state needs no wait: the lane's frames
    // run in its stream's order, and the blends read only the samples.
    const uint32_t b = L.flip;
    L.flip = VPX_LANE_DOUBLE ? L.flip ^ 1u : 0u;
    if (!dst) {
        const size_t need = (size_t)tiles * kTilePix;
        // blends queued on the caller's stream still read the old samples: wait
        if (int rc = L.packed.grow(c, sizeof(float4) * need, true)) return rc;
        if (VPX_LANE_DOUBLE)
            if (int rc = L.packed2.grow(c, sizeof(float4) * need, true)) return rc;
        dst = b ? L.packed2.get() : L.packed.get();
    }
    bool& used = b ? L.used2 : L.used;
    L.cur = dst;
    L.cur_consumed = b ? L.consumed2 : L.consumed;
    // this buffer's previous frame has been blended
    if (used) VPX_HIP(c, hipStreamWaitEvent(L.s, L.cur_consumed, 0));
    int rc = launch_render<kFinishPackedSample>(c, L.s, L.ws, sv, f, tiles, nullptr, nullptr, dst);
    if (rc) return rc;
    VPX_HIP(c, hipEventRecord(L.rendered, L.s));
    VPX_HIP(c, hipStreamWaitEvent(c->stream, L.rendered, 0));
    used = true;
    lane = &L;
    return VPX_OK;
}

// Lanes on dedicated hardware queues across the process (every context, every device-set
// member; level forks too): each takes a queue of its own, so the count is capped
// (kMaxLaneQueues, g_lane_queues above); lanes past the cap are plain non-blocking streams
// from the shared pool.

void free_lanes(vpx_ctx* c) {
    for (auto& L : c->lanes) {
        if (L.dedicated) g_lane_queues.fetch_sub(1);
        if (L.s) (void)hipStreamSynchronize(L.s);
        free_fork(L.ws);
        if (L.rendered) (void)hipEventDestroy(L.rendered);
        if (L.consumed) (void)hipEventDestroy(L.consumed);
        if (L.consumed2) (void)hipEventDestroy(L.consumed2);
        if (L.caller) (void)hipEventDestroy(L.caller);
        if (L.s) (void)hipStreamDestroy(L.s);
    }
    c->lanes.clear();  // the lanes' buffers go with them
    c->lane_next = 0;
}

int snapshot_counters(vpx_ctx* c, unsigned long long out[kCtrWords]) {
    unsigned long long all[kCtrWords * kCtrStripes];
    VPX_HIP(c, hipMemcpyAsync(all, c->d_ctr, sizeof(all), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, sync_all(c));
    for (uint32_t i = 0; i < kCtrWords; ++i) {
        out[i] = 0;
        for (uint32_t s = 0; s < kCtrStripes; ++s) out[i] += all[kCtrWords * s + i];
    }
    return VPX_OK;
}

void fill_stats(vpx_stats* s, const unsigned long long a[kCtrWords], const unsigned long long b[kCtrWords]) {
    s->shadow_rays = b[0] - a[0];
    s->primary_rays = b[3] - a[3];
    const unsigned long long nearest = b[1] - a[1];  // 0 for Trace(ray, -1): no bounce rays
    s->bounce_rays = nearest > s->primary_rays ? nearest - s->primary_rays : 0;
    s->dda_cells = b[2] - a[2];
}

}  // namespace

// =============================================================================== C-ABI
extern "C" {

int vpx_abi_version(void) { return VPX_ABI_VERSION; }

int vpx_create(int device, vpx_ctx** out) {
    if (!out) return VPX_E_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return VPX_E_DEVICE;
    if (device < 0 || device >= count) return VPX_E_INVALID;
    if (hipSetDevice(device) != hipSuccess) return VPX_E_DEVICE;
    vpx_ctx* c = new (std::nothrow) vpx_ctx();
    if (!c) return VPX_E_NOMEM;
    c->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        c->cus = (uint32_t)cus;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess ||
        c->d_ctr.alloc(kCtrWords * kCtrStripes * sizeof(unsigned long long)) != hipSuccess ||
        c->d_sum.alloc(sizeof(unsigned long long)) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipEventCreate(&c->ev2) != hipSuccess) {
        vpx_destroy(c);
        return VPX_E_DEVICE;
    }
    c->stream = c->own_stream;
    (void)hipMemset(c->d_ctr, 0, kCtrWords * kCtrStripes * sizeof(unsigned long long));
    *out = c;
    return VPX_OK;
}

int vpx_destroy(vpx_ctx* c) {
    if (!c) return VPX_E_INVALID;
    if (c->gl_res) {  // a context destroyed while its GL buffer is mapped: unmap, then unregister
        vpx_ctx* h = c->members.empty() ? c : c->members[0].ctx;
        (void)hipSetDevice(h->device);
        if (c->gl_mapped) (void)hipGraphicsUnmapResources(1, &c->gl_res, h->stream);
        (void)hipGraphicsUnregisterResource(c->gl_res);
        c->gl_res = nullptr;
        c->gl_mapped = false;
    }
    // Only what depends on an order is released by hand; every buffer is an Owned and goes with
    // its holder, on the device that is current then.
    if (!c->members.empty()) {  // device set: its events, communicators and members
        DeviceGuard keep;
        for (auto& slot : c->members) {
            const vpx_ctx::Member mem = std::move(slot);  // its buffers go with `mem`, on its device
            (void)hipSetDevice(mem.ctx->device);
            (void)hipStreamSynchronize(mem.ctx->stream);
            if (mem.ev) (void)hipEventDestroy(mem.ev);
        }
        const int first = c->members[0].ctx->device;  // where the gathered buffer lives
        (void)hipSetDevice(first);
        if (c->g_copied) (void)hipEventDestroy(c->g_copied);
        for (ncclComm_t cm : c->comms) (void)ncclCommDestroy(cm);
        for (const auto& slot : c->members) vpx_destroy(slot.ctx);
        (void)hipSetDevice(first);
        delete c;
        return VPX_OK;
    }
    (void)hipSetDevice(c->device);
    if (c->stream) (void)sync_all(c);
    free_lanes(c);
    free_fork(c->wave);
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    if (c->rj_ev) (void)hipEventDestroy(c->rj_ev);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
    return VPX_OK;
}

const char* vpx_last_error(const vpx_ctx* c) { return c ? c->err.c_str() : "null context"; }

int vpx_set_stream(vpx_ctx* c, void* s) {
    if (!c) return VPX_E_INVALID;
    if (!c->members.empty()) return vpx_set_stream(c->members[0].ctx, s);  // a stream of the first device
    VPX_HIP(c, sync_all(c));
    // (the context's own stream is kept while unused: releasing it measured slower with
    // pipeline lanes — C2 3.75 vs 2.97 ms at 3 lanes — the lanes' hardware-queue sharing
    // changes with the number of live streams)
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return VPX_OK;
}

int vpx_set_pipeline(vpx_ctx* c, uint32_t depth) {
    VPX_GROUP_ALL(c, vpx_set_pipeline(m_, depth));
    if (!c) return VPX_E_INVALID;
    if (depth > 4) return fail(c, VPX_E_INVALID, "pipeline depth must be in [0, 4]");
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));
    free_lanes(c);
    if (depth < 2) return VPX_OK;
    // the context's own level fork (taken by a depth > 0 frame on the context's stream) gives
    // its dedicated queue back: the lanes need them, and it is recreated if such a frame comes
    free_fork(c->wave);
    c->lanes.resize(depth);
    // Each lane on a hardware queue of its own.  Plain streams share the process's pool of
    // GPU_MAX_HW_QUEUES (4) queues: a kernel trace shows two of three lanes on one queue and
    // the third on the caller's (blend) queue, so a lane's frame waited behind another's.  A
    // stream with an explicit CU mask (here: every CU) gets a dedicated queue.  Measured on
    // one box (C1 ms, two processes x two contexts, 20 frames): 3 lanes 0.551-0.554 vs
    // 0.578-0.598 on pooled streams (4 pooled lanes 0.567-0.572, 4 dedicated 0.578-0.594).
    int n_cu = 0;
    VPX_HIP(c, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device));
    std::vector<uint32_t> all_cus(((uint32_t)n_cu + 31u) / 32u, 0xffffffffu);
    // CU-mask streams are blocking streams (no flags argument): they synchronise with the
    // legacy null stream like any default-flag stream (documented in vpx.h).
    for (auto& L : c->lanes) {
        L.dedicated = g_lane_queues.fetch_add(1) < kMaxLaneQueues;
        if (!L.dedicated) g_lane_queues.fetch_sub(1);
        const hipError_t se = L.dedicated
                                  ? hipExtStreamCreateWithCUMask(&L.s, (uint32_t)all_cus.size(), all_cus.data())
                                  : hipStreamCreateWithFlags(&L.s, hipStreamNonBlocking);
        if (se != hipSuccess ||
            hipEventCreateWithFlags(&L.rendered, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.consumed, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.consumed2, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&L.caller, hipEventDisableTiming) != hipSuccess) {
            free_lanes(c);
            return fail(c, VPX_E_DEVICE, "pipeline lane stream / events");
        }
    }
    return VPX_OK;
}

// ---------------------------------------------------------------- display interop
// GLTexture::CopyFrom (template/opengl.cpp:144-149) uploads the host screen every frame; here
// the RGB8 pack writes into a GL pixel-unpack buffer the host registered once, and the host
// updates its texture from that buffer (glTexSubImage2D with the PBO bound) — the frame stays
// on the GPU.  A device set registers and maps on devices[0], where vpx_render composites.
static vpx_ctx* gl_home(vpx_ctx* c) { return c->members.empty() ? c : c->members[0].ctx; }

int vpx_gl_register_buffer(vpx_ctx* c, unsigned int gl_buffer) {
    if (!c) return VPX_E_INVALID;
    if (c->gl_mapped) return fail(c, VPX_E_STATE, "the GL buffer is mapped (vpx_gl_unmap first)");
    vpx_ctx* h = gl_home(c);
    VPX_HIP(c, hipSetDevice(h->device));
    if (c->gl_res) {
        const hipError_t e = hipGraphicsUnregisterResource(c->gl_res);
        c->gl_res = nullptr;
        if (e != hipSuccess) return fail(c, VPX_E_DEVICE, std::string("hipGraphicsUnregisterResource: ") + hipGetErrorString(e));
    }
    if (gl_buffer == 0u) return VPX_OK;
    hipGraphicsResource_t r = nullptr;
    const hipError_t e = hipGraphicsGLRegisterBuffer(&r, (GLuint)gl_buffer, hipGraphicsRegisterFlagsWriteDiscard);
    if (e != hipSuccess || !r)
        return fail(c, VPX_E_DEVICE, std::string("hipGraphicsGLRegisterBuffer (needs the buffer's GL context current on "
                                                 "this thread, on this context's GPU): ") + hipGetErrorString(e));
    c->gl_res = r;
    return VPX_OK;
}

int vpx_gl_map(vpx_ctx* c, uint32_t** rgb8, size_t* bytes) {
    if (!c || !rgb8) return VPX_E_INVALID;
    if (!c->gl_res) return fail(c, VPX_E_STATE, "no GL buffer registered (vpx_gl_register_buffer)");
    if (c->gl_mapped) return fail(c, VPX_E_STATE, "the GL buffer is already mapped");
    vpx_ctx* h = gl_home(c);
    VPX_HIP(c, hipSetDevice(h->device));
    VPX_HIP(c, hipGraphicsMapResources(1, &c->gl_res, h->stream));
    void* ptr = nullptr;
    size_t n = 0;
    const hipError_t e = hipGraphicsResourceGetMappedPointer(&ptr, &n, c->gl_res);
    if (e != hipSuccess) {
        (void)hipGraphicsUnmapResources(1, &c->gl_res, h->stream);
        return fail(c, VPX_E_DEVICE, std::string("hipGraphicsResourceGetMappedPointer: ") + hipGetErrorString(e));
    }
    c->gl_mapped = true;
    *rgb8 = static_cast<uint32_t*>(ptr);
    if (bytes) *bytes = n;
    return VPX_OK;
}

int vpx_gl_unmap(vpx_ctx* c) {
    if (!c) return VPX_E_INVALID;
    if (!c->gl_mapped) return fail(c, VPX_E_STATE, "the GL buffer is not mapped");
    vpx_ctx* h = gl_home(c);
    VPX_HIP(c, hipSetDevice(h->device));
    c->gl_mapped = false;
    VPX_HIP(c, hipGraphicsUnmapResources(1, &c->gl_res, h->stream));
    return VPX_OK;
}

int vpx_synchronize(vpx_ctx* c) {
    VPX_GROUP_ALL(c, vpx_synchronize(m_));
    if (!c) return VPX_E_INVALID;
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

static int alloc_grid(vpx_ctx* c, uint32_t id, uint32_t n) {
    if (id > 4096) return fail(c, VPX_E_INVALID, "grid_id too large");
    if (n == 0 || n > 4096) return fail(c, VPX_E_INVALID, "grid size must be in [1, 4096]");
    VPX_HIP(c, hipSetDevice(c->device));
    if (id >= c->grids.size()) c->grids.resize(id + 1);
    auto& g = c->grids[id];
    const size_t bytes = (size_t)n * n * n;
    if (!g.ptr || g.n != n) {  // a grid of another size is a new grid; a failure leaves none
        if (g.ptr) VPX_HIP(c, sync_all(c));
        vpx_ctx::GridBuf fresh;
        fresh.n = n;
        fresh.nb1 = (n + 3) / 4;
        fresh.nb2 = (fresh.nb1 + 3) / 4;
        fresh.nb3 = (fresh.nb2 + 3) / 4;
        g = vpx_ctx::GridBuf{};
        VPX_HIP(c, fresh.ptr.alloc(bytes));
        VPX_HIP(c, fresh.l1.alloc(sizeof(uint64_t) * (size_t)fresh.nb2 * fresh.nb2 * fresh.nb2 * 64));
        VPX_HIP(c, fresh.l2.alloc(sizeof(uint64_t) * (size_t)fresh.nb3 * fresh.nb3 * fresh.nb3 * 64));
        VPX_HIP(c, fresh.dfp.alloc((8 + 4 * 24) * fresh.plane()));  // 8 octant planes of bytes, 24 axis planes of 32-bit words
        g = std::move(fresh);
    }
    return sync_grids(c);
}

// The distance-field words of every empty brick (recurrence: skip::df_value), one
// anti-diagonal plane per launch from the far corner — all 8 octants at once, each in its
// own flipped coordinates and its own byte of the word.  Needs l2 (occupancy) current.
static int build_df(vpx_ctx* c, const vpx_ctx::GridBuf& g) {
    const uint64_t threads = (uint64_t)g.nb1 * g.nb1 * 8;
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    for (uint32_t s = 3 * (g.nb1 - 1) + 1; s-- > 0;) {
        hipLaunchKernelGGL(df_plane_k, dim3(blocks), dim3(256), 0, c->stream, g.l1.as<uint8_t>(), g.l2, g.nb1, g.nb2, g.nb3, s);
        VPX_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(build_planes_k, dim3(2048), dim3(256), 0, c->stream, g.l1, g.l2, g.nb2, g.nb3, g.dfp);
    VPX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(build_axis_k, dim3(8192), dim3(256), 0, c->stream, g.dfp, g.nb1, g.nb2, (uint32_t*)(g.dfp + 8 * g.plane()));
    VPX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(build_wide_k, dim3(8192), dim3(256), 0, c->stream, (uint16_t*)(g.dfp + 8 * g.plane()), g.nb1, g.nb2);
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

// Rebuild the occupancy levels and the distance field after the grid bytes changed.
static int build_masks(vpx_ctx* c, uint32_t id) {
    auto& g = c->grids[id];
    hipLaunchKernelGGL(build_l1_k, dim3(2048), dim3(256), 0, c->stream, g.ptr, g.n, g.nb1, g.nb2, g.l1);
    VPX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(build_up_k, dim3(512), dim3(256), 0, c->stream, g.l1, g.nb2, g.nb3, g.l2);
    VPX_HIP(c, hipGetLastError());
    if (int r = build_df(c, g)) return r;
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

// The refresh's record, reset on the stream; before the first launch that counts into it.
static int refresh_begin(vpx_ctx* c) {
    if (!c->d_refresh) {
        VPX_HIP(c, c->h_refresh.alloc(2 * sizeof(RefreshDev)));
        VPX_HIP(c, c->d_refresh.alloc(sizeof(RefreshDev)));
        RefreshDev& init = c->h_refresh[0];
        std::memset(&init, 0, sizeof(init));
        init.E = skip::box_none();
        for (auto& b : init.C) b = skip::box_none();
        for (auto& b : init.D) b = skip::box_none();
    }
    VPX_HIP(c, hipMemcpyAsync(c->d_refresh, &c->h_refresh[0], sizeof(RefreshDev), hipMemcpyHostToDevice, c->stream));
    return VPX_OK;
}

// The levels after the cells of `count` boxes (inclusive cell coordinates, inside the grid)
// changed: the region-local refresh (DESIGN §4 "Brush edits"; the host restatement is
// skip::refresh_masks_host / refresh_levels_host).  Stage 0 takes one launch per box; where no
// brick's emptiness flipped the call ends there, after one read-back.  Otherwise: one marking
// launch and a second read-back (the boxes of stage 1 set the number of launches), one launch
// per anti-diagonal of the largest box, then one each for the planes, the low halves and the
// widths.  Ends synchronised, like build_masks.
static int refresh_levels(vpx_ctx* c, const vpx_ctx::GridBuf& g, const skip::Box3* cells, uint32_t count, vpx_brush_result* res) {
    RefreshDev* rd = c->d_refresh;
    RefreshDev& back = c->h_refresh[1];
    auto blocks = [](uint64_t threads, uint64_t cap) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(cap, (threads + 255) / 256)); };
    auto volume = [](const skip::Box3& b) -> uint64_t {
        return skip::box_empty(b) ? (uint64_t)0 : (uint64_t)(b.hi[0] - b.lo[0] + 1) * (uint64_t)(b.hi[1] - b.lo[1] + 1) * (uint64_t)(b.hi[2] - b.lo[2] + 1);
    };
    for (uint32_t i = 0; i < count; ++i) {
        const uint32_t b0[3] = {(uint32_t)cells[i].lo[0] >> 2, (uint32_t)cells[i].lo[1] >> 2, (uint32_t)cells[i].lo[2] >> 2};
        const uint32_t cx = ((uint32_t)cells[i].hi[0] >> 2) - b0[0] + 1, cy = ((uint32_t)cells[i].hi[1] >> 2) - b0[1] + 1,
                       cz = ((uint32_t)cells[i].hi[2] >> 2) - b0[2] + 1;
        hipLaunchKernelGGL(refresh_l1_k, dim3(blocks((uint64_t)cx * cy * cz, 4096)), dim3(256), 0, c->stream, g.ptr, g.n, g.nb2, g.nb3,
                           g.l1, g.l2, b0[0], b0[1], b0[2], cx, cy, cz, rd);
        VPX_HIP(c, hipGetLastError());
    }
    VPX_HIP(c, hipMemcpyAsync(&back, rd, offsetof(RefreshDev, C), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, hipStreamSynchronize(c->stream));
    if (res) res->changed = back.changed, res->flipped = back.flipped;
    if (!back.flipped) return VPX_OK;  // only cell masks changed: no distance-field word can

    const skip::Box3 E = back.E;
    const uint32_t reach[3] = {skip::kReach, skip::kReach, skip::kReach};
    const uint64_t plane = g.plane();
    uint32_t* dfw = (uint32_t*)(g.dfp + 8 * plane);
    Boxes8 cand;
    uint64_t most = 0;
    for (uint32_t o = 0; o < 8; ++o) {
        cand.b[o] = skip::box_behind(E, o, reach, g.nb1);
        most = std::max(most, volume(cand.b[o]));
    }
    hipLaunchKernelGGL(df_mark_k, dim3(blocks(most, 2048), 8), dim3(256), 0, c->stream, g.dfp, plane, g.nb2, cand, E, rd);
    VPX_HIP(c, hipGetLastError());
    VPX_HIP(c, hipMemcpyAsync(back.C, (const uint8_t*)rd + offsetof(RefreshDev, C), sizeof(back.C), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, hipStreamSynchronize(c->stream));

    Boxes8 C;
    uint32_t diagonals = 0;
    uint64_t face = 0, most_c = 0, most_a = 0, most_w = 0;
    for (uint32_t o = 0; o < 8; ++o) {
        const skip::Box3& b = C.b[o] = back.C[o];
        if (skip::box_empty(b)) continue;
        const uint32_t cx = (uint32_t)(b.hi[0] - b.lo[0] + 1), cy = (uint32_t)(b.hi[1] - b.lo[1] + 1), cz = (uint32_t)(b.hi[2] - b.lo[2] + 1);
        diagonals = std::max(diagonals, cx + cy + cz - 2);
        face = std::max<uint64_t>(face, (uint64_t)cx * cy);
        most_c = std::max(most_c, volume(b));
        for (uint32_t a = 0; a < 3; ++a) {  // stage 3's candidates, and the cone behind them that bounds stage 4's
            uint32_t ext[3] = {1u, 1u, 1u};
            ext[a] = skip::kReach;
            const skip::Box3 ca = skip::box_behind(b, o, ext, g.nb1);
            most_a = std::max(most_a, volume(ca));
            most_w = std::max(most_w, volume(skip::box_behind(ca, o, reach, g.nb1)));
        }
    }
    for (uint32_t s = 0; s < diagonals; ++s) {
        hipLaunchKernelGGL(df_diag_k, dim3(blocks(face, ~0ull), 8), dim3(256), 0, c->stream, g.l1.as<uint8_t>(), g.l2, g.nb1, g.nb2, g.nb3, C, s);
        VPX_HIP(c, hipGetLastError());
    }
    hipLaunchKernelGGL(df_planes_box_k, dim3(blocks(most_c, 2048), 8), dim3(256), 0, c->stream, g.l1.as<const uint8_t>(), g.l2, g.nb2, g.nb3,
                       g.dfp, plane, C);
    VPX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(axis_box_k, dim3(blocks(most_a, 1024), 24), dim3(256), 0, c->stream, g.dfp, g.nb1, g.nb2, dfw, C, rd);
    VPX_HIP(c, hipGetLastError());
    hipLaunchKernelGGL(wide_box_k, dim3(blocks(most_w / 8, 4096), 24), dim3(256), 0, c->stream, (uint16_t*)dfw, g.nb1, g.nb2,
                       (const RefreshDev*)rd);
    VPX_HIP(c, hipGetLastError());
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

// After an edit of the cells [x0, x1) x [y0, y1) x [z0, z1): the cell masks of their bricks,
// then the distance field where the edit can reach it (refresh_levels).  The loaders, the
// generators, vpx_upload_grid and vpx_grid_fill rebuild everything (build_masks).
static int build_masks_box(vpx_ctx* c, uint32_t id, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t x1, uint32_t y1,
                           uint32_t z1) {
    if (x0 >= x1 || y0 >= y1 || z0 >= z1) return VPX_OK;
    if (int r = refresh_begin(c)) return r;
    const skip::Box3 cells{{(int32_t)x0, (int32_t)y0, (int32_t)z0}, {(int32_t)x1 - 1, (int32_t)y1 - 1, (int32_t)z1 - 1}};
    return refresh_levels(c, c->grids[id], &cells, 1, nullptr);
}

int vpx_grid_brush(vpx_ctx* c, uint32_t id, const vpx_brush* brushes, uint32_t count, vpx_brush_result* out) {
    VPX_GROUP_ALL(c, vpx_grid_brush(m_, id, brushes, count, out));
    if (!c) return VPX_E_INVALID;
    if (const char* why = brush::check_brushes(brushes, count)) return fail(c, VPX_E_INVALID, why);
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    auto& g = c->grids[id];
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    if (int r = refresh_begin(c)) return r;
    skip::Box3 boxes[brush::kMaxBrushes];
    uint32_t n_boxes = 0;
    for (uint32_t i = 0; i < count; ++i) {
        uint32_t lo[3], hi[3];
        if (!brush::clipped_box(brushes[i], g.n, lo, hi)) continue;
        const uint32_t cx = hi[0] - lo[0] + 1, cy = hi[1] - lo[1] + 1, cz = hi[2] - lo[2] + 1;
        hipLaunchKernelGGL(brush_k, dim3((unsigned)std::min<uint64_t>(4096, ((uint64_t)cx * cy * cz + 255) / 256)), dim3(256), 0,
                           c->stream, g.ptr, g.n, brushes[i], lo[0], lo[1], lo[2], cx, cy, cz, c->d_refresh);
        VPX_HIP(c, hipGetLastError());
        boxes[n_boxes++] = skip::Box3{{(int32_t)lo[0], (int32_t)lo[1], (int32_t)lo[2]}, {(int32_t)hi[0], (int32_t)hi[1], (int32_t)hi[2]}};
    }
    vpx_brush_result res{};
    if (int r = refresh_levels(c, g, boxes, n_boxes, &res)) return r;
    if (out) *out = res;
    return VPX_OK;
}

int vpx_grid_stamp(vpx_ctx* c, uint32_t id, const vpx_stamp* stamps, uint32_t count, vpx_brush_result* out) {
    VPX_GROUP_ALL(c, vpx_grid_stamp(m_, id, stamps, count, out));
    if (!c) return VPX_E_INVALID;
    if (const char* why = stamp::check_stamps(stamps, count)) return fail(c, VPX_E_INVALID, why);
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    for (uint32_t i = 0; i < count; ++i)
        if (stamps[i].model_id >= c->models.size() || !c->models[stamps[i].model_id].vox) return fail(c, VPX_E_INVALID, "unknown model");
    auto& g = c->grids[id];
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    if (int r = refresh_begin(c)) return r;
    skip::Box3 boxes[stamp::kMaxStamps];
    uint32_t n_boxes = 0;
    const bool wide = (g.n % 16u) == 0;
    for (uint32_t i = 0; i < count; ++i) {
        const auto& m = c->models[stamps[i].model_id];
        stamp::Plan p;
        if (!stamp::plan(stamps[i], m.sx, m.sy, m.sz, g.n, p)) continue;
        const uint32_t s0 = p.lo[0] >> 4, spans = (p.hi[0] >> 4) - s0 + 1;
        const uint64_t threads = (uint64_t)(wide ? spans : p.hi[0] - p.lo[0] + 1) * (p.hi[1] - p.lo[1] + 1) * (p.hi[2] - p.lo[2] + 1);
        const dim3 blocks((unsigned)std::min<uint64_t>(2048, (threads + 255) / 256));
        if (wide)
            hipLaunchKernelGGL(stamp_k<true>, blocks, dim3(256), 0, c->stream, g.ptr, g.n, (const uint8_t*)m.vox, p, s0, spans, c->d_refresh);
        else
            hipLaunchKernelGGL(stamp_k<false>, blocks, dim3(256), 0, c->stream, g.ptr, g.n, (const uint8_t*)m.vox, p, s0, spans, c->d_refresh);
        VPX_HIP(c, hipGetLastError());
        boxes[n_boxes++] = skip::Box3{{(int32_t)p.lo[0], (int32_t)p.lo[1], (int32_t)p.lo[2]}, {(int32_t)p.hi[0], (int32_t)p.hi[1], (int32_t)p.hi[2]}};
    }
    vpx_brush_result res{};
    if (int r = refresh_levels(c, g, boxes, n_boxes, &res)) return r;
    if (out) *out = res;
    return VPX_OK;
}

int vpx_grid_fill(vpx_ctx* c, uint32_t id, uint8_t value) {
    VPX_GROUP_ALL(c, vpx_grid_fill(m_, id, value));
    if (!c) return VPX_E_INVALID;
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    auto& g = c->grids[id];
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    VPX_HIP(c, hipMemsetAsync(g.ptr, value, (size_t)g.n * g.n * g.n, c->stream));
    return build_masks(c, id);
}

int vpx_grid_write_box(vpx_ctx* c, uint32_t id, const uint8_t* src, uint32_t x0, uint32_t y0, uint32_t z0,
                       uint32_t dx, uint32_t dy, uint32_t dz) {
    VPX_GROUP_ALL(c, vpx_grid_write_box(m_, id, src, x0, y0, z0, dx, dy, dz));
    if (!c || !src) return fail(c, VPX_E_INVALID, "null argument");
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    auto& g = c->grids[id];
    if ((uint64_t)x0 + dx > g.n || (uint64_t)y0 + dy > g.n || (uint64_t)z0 + dz > g.n)
        return fail(c, VPX_E_INVALID, "box outside the grid");
    const size_t bytes = (size_t)dx * dy * dz;
    if (!bytes) return VPX_OK;
    Owned<uint8_t> d;  // the box on the device, for this call
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    VPX_HIP(c, d.alloc(bytes));
    if (hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return fail(c, VPX_E_DEVICE, "box upload failed");
    hipLaunchKernelGGL(write_box_k, dim3((unsigned)std::min<size_t>(4096, (bytes + 255) / 256)), dim3(256), 0, c->stream,
                       g.ptr, g.n, d, x0, y0, z0, dx, dy, dz);
    const hipError_t e = sync_all(c);
    d.release();
    if (e != hipSuccess) return fail(c, VPX_E_DEVICE, hipGetErrorString(e));
    return build_masks_box(c, id, x0, y0, z0, x0 + dx, y0 + dy, z0 + dz);
}

int vpx_grid_emissive_sphere(vpx_ctx* c, uint32_t id, uint8_t mat, float radius) {
    VPX_GROUP_ALL(c, vpx_grid_emissive_sphere(m_, id, mat, radius));
    if (!c) return VPX_E_INVALID;
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    auto& g = c->grids[id];
    if (!(radius > 0.0f)) return VPX_OK;  // no cell has length < radius <= 0 (NaN: none either)
    // cells with |c - x| < radius per axis, c = n/2: a conservative integer box
    const double cc = g.n / 2.0, r = std::min<double>(radius, 4.0 * g.n);
    const int64_t a = std::max<int64_t>(0, (int64_t)std::floor(cc - r) - 1);
    const int64_t b = std::min<int64_t>((int64_t)g.n - 1, (int64_t)std::ceil(cc + r) + 1);
    if (b < a) return VPX_OK;
    const uint32_t x0 = (uint32_t)a, cnt = (uint32_t)(b - a + 1);
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    hipLaunchKernelGGL(emissive_sphere_k, dim3((unsigned)std::min<uint64_t>(4096, ((uint64_t)cnt * cnt * cnt + 255) / 256)),
                       dim3(256), 0, c->stream, g.ptr, g.n, mat, radius, x0, cnt);
    VPX_HIP(c, hipGetLastError());
    return build_masks_box(c, id, x0, x0, x0, x0 + cnt, x0 + cnt, x0 + cnt);
}

int vpx_upload_grid(vpx_ctx* c, uint32_t id, const uint8_t* cells, uint32_t n) {
    VPX_GROUP_ALL(c, vpx_upload_grid(m_, id, cells, n));
    if (!c || !cells) return fail(c, VPX_E_INVALID, "null argument");
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    int rc = alloc_grid(c, id, n);
    if (rc) return rc;
    VPX_HIP(c, hipMemcpy(c->grids[id].ptr, cells, (size_t)n * n * n, hipMemcpyHostToDevice));
    return build_masks(c, id);
}

int vpx_generate_tiled_grid(vpx_ctx* c, uint32_t id, uint32_t n, const uint8_t* model, uint32_t mx, uint32_t my,
                            uint32_t mz, uint32_t px, uint32_t py, uint32_t pz, uint32_t ground) {
    VPX_GROUP_ALL(c, vpx_generate_tiled_grid(m_, id, n, model, mx, my, mz, px, py, pz, ground));
    if (!c || !model) return fail(c, VPX_E_INVALID, "null argument");
    if (!mx || !my || !mz || !px || !py || !pz) return fail(c, VPX_E_INVALID, "zero model size or period");
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    int rc = alloc_grid(c, id, n);
    if (rc) return rc;
    const size_t mbytes = (size_t)mx * my * mz;
    Owned<uint8_t> dm;  // the model on the device, for this call
    VPX_HIP(c, dm.alloc(mbytes));
    VPX_HIP(c, hipMemcpy(dm, model, mbytes, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(tiled_world_k, dim3(4096), dim3(256), 0, c->stream, c->grids[id].ptr, n, dm, mx, my, mz, px,
                       py, pz, ground);
    VPX_HIP(c, hipGetLastError());
    VPX_HIP(c, sync_all(c));
    dm.release();
    return build_masks(c, id);
}

constexpr size_t kJumpBytes = sizeof(uint32_t) * 32 * model::kJumpDevice;

// The jump tables, once, with room for the plan of the largest grid (n = 4096) behind them.
static int ensure_model_aux(vpx_ctx* c) {
    if (c->d_model_aux) return VPX_OK;
    std::vector<uint32_t> t(32 * model::kJumpDevice);
    model::xs32_build_tables(t.data(), model::kJumpDevice);
    if (!c->h_plan) VPX_HIP(c, c->h_plan.alloc(model::plan_bytes(4096)));
    Owned<uint8_t> aux;  // the context's only once the tables are in it
    VPX_HIP(c, aux.alloc(kJumpBytes + model::plan_bytes(4096)));
    const hipError_t e = hipMemcpy(aux, t.data(), kJumpBytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) return fail(c, VPX_E_DEVICE, std::string("jump tables: ") + hipGetErrorString(e));
    c->d_model_aux = std::move(aux);
    return VPX_OK;
}

// Resident model `id` replaced by an empty one of sx * sy * sz voxels in `m` (vpx_model_upload,
// vpx_model_capture): the checks, the wait for the frames in flight, the old model released,
// the aux buffers, the voxels and the `mat` scratch.  Without `fill` the id is only emptied.
// The caller fills m.vox and moves m into c->models[id]: a failure leaves the id empty.
static int model_replace(vpx_ctx* c, uint32_t id, bool fill, uint32_t sx, uint32_t sy, uint32_t sz, vpx_ctx::ModelBuf& m) {
    if (id > 4096) return fail(c, VPX_E_INVALID, "model_id too large");
    if (fill && (!sx || !sy || !sz || sx > model::kMaxDim || sy > model::kMaxDim || sz > model::kMaxDim))
        return fail(c, VPX_E_INVALID, "model dimension outside 1..256");
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));
    if (id < c->models.size()) c->models[id] = vpx_ctx::ModelBuf{};
    if (!fill) return VPX_OK;
    if (int rc = ensure_model_aux(c)) return rc;
    if (id >= c->models.size()) c->models.resize(id + 1);
    const size_t count = (size_t)sx * sy * sz;
    VPX_HIP(c, m.vox.alloc(count));
    VPX_HIP(c, m.mat.alloc((count + model::kChunk - 1) / model::kChunk * model::kChunk));
    m.sx = sx, m.sy = sy, m.sz = sz;
    return VPX_OK;
}

int vpx_model_upload(vpx_ctx* c, uint32_t id, const uint8_t* voxels, uint32_t sx, uint32_t sy, uint32_t sz) {
    VPX_GROUP_ALL(c, vpx_model_upload(m_, id, voxels, sx, sy, sz));
    if (!c) return VPX_E_INVALID;
    vpx_ctx::ModelBuf m;  // the context's only when complete: a failure leaves the id empty
    if (int rc = model_replace(c, id, voxels != nullptr, sx, sy, sz, m)) return rc;
    if (!voxels) return VPX_OK;
    VPX_HIP(c, hipMemcpy(m.vox, voxels, (size_t)sx * sy * sz, hipMemcpyHostToDevice));
    c->models[id] = std::move(m);
    return VPX_OK;
}

int vpx_model_capture(vpx_ctx* c, uint32_t model_id, uint32_t id, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t dx,
                      uint32_t dy, uint32_t dz) {
    VPX_GROUP_ALL(c, vpx_model_capture(m_, model_id, id, x0, y0, z0, dx, dy, dz));
    if (!c) return VPX_E_INVALID;
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    const auto& g = c->grids[id];
    if (dx && dy && dz && ((uint64_t)x0 + dx > g.n || (uint64_t)y0 + dy > g.n || (uint64_t)z0 + dz > g.n))
        return fail(c, VPX_E_INVALID, "box outside the grid");
    vpx_ctx::ModelBuf m;  // the context's only when complete: a failure leaves the id empty
    if (int rc = model_replace(c, model_id, true, dx, dy, dz, m)) return rc;
    const bool wide = g.n % 16u == 0 && x0 % 16u == 0 && dx % 16u == 0;
    const uint64_t threads = (uint64_t)(wide ? dx / 16u : dx) * dy * dz;
    const dim3 blocks((unsigned)std::min<uint64_t>(4096, (threads + 255) / 256));
    if (wide)
        hipLaunchKernelGGL(capture_k<true>, blocks, dim3(256), 0, c->stream, (const uint8_t*)g.ptr, g.n, m.vox.get(), x0, y0, z0, dx, dy, dz);
    else
        hipLaunchKernelGGL(capture_k<false>, blocks, dim3(256), 0, c->stream, (const uint8_t*)g.ptr, g.n, m.vox.get(), x0, y0, z0, dx, dy, dz);
    VPX_HIP(c, hipGetLastError());
    VPX_HIP(c, sync_all(c));
    c->models[model_id] = std::move(m);
    return VPX_OK;
}

int vpx_model_read(vpx_ctx* c, uint32_t model_id, uint8_t* dst, uint64_t cap, uint32_t size_out[3]) {
    VPX_GROUP_FIRST(c, vpx_model_read(m_, model_id, dst, cap, size_out));
    if (!c || !size_out) return fail(c, VPX_E_INVALID, "null argument");
    if (model_id >= c->models.size() || !c->models[model_id].vox) return fail(c, VPX_E_INVALID, "unknown model");
    const auto& m = c->models[model_id];
    size_out[0] = m.sx, size_out[1] = m.sy, size_out[2] = m.sz;
    if (!dst) return VPX_OK;
    const uint64_t count = (uint64_t)m.sx * m.sy * m.sz;
    if (cap < count) return fail(c, VPX_E_INVALID, "cap smaller than the model");
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));
    VPX_HIP(c, hipMemcpy(dst, m.vox, count, hipMemcpyDeviceToHost));
    return VPX_OK;
}

int vpx_grid_load_model(vpx_ctx* c, uint32_t id, uint32_t n, uint32_t model_id, const vpx_model_load* in,
                        vpx_model_result* out) {
    VPX_GROUP_ALL(c, vpx_grid_load_model(m_, id, n, model_id, in, out));
    if (!c) return VPX_E_INVALID;
    if (!in) return fail(c, VPX_E_INVALID, "null vpx_model_load");
    if (model_id >= c->models.size() || !c->models[model_id].vox) return fail(c, VPX_E_INVALID, "unknown model");
    const auto& m = c->models[model_id];
    if (const char* why = model::check_load(in, m.sx, m.sy, m.sz, n)) return fail(c, VPX_E_INVALID, why);
    if (id > 4096) return fail(c, VPX_E_INVALID, "grid_id too large");
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    if (id >= c->grids.size() || !c->grids[id].ptr || c->grids[id].n != n)
        if (int rc = alloc_grid(c, id, n)) return rc;
    vpx_model_result res{};
    model::plan_load(c->h_plan, in, m.sx, m.sy, m.sz, n, res.scale_model);
    res.seed = in->seed;
    uint8_t* d_plan = c->d_model_aux.get() + kJumpBytes;
    VPX_HIP(c, hipMemcpyAsync(d_plan, c->h_plan, model::plan_bytes(n), hipMemcpyHostToDevice, c->stream));
    const uint64_t count = (uint64_t)m.sx * m.sy * m.sz;
    const uint8_t* mat = m.vox;
    if (in->mode == VPX_LOAD_RANDOM) {
        const uint64_t chunks = (count + model::kChunk - 1) / model::kChunk;
        hipLaunchKernelGGL(model_random_k, dim3((unsigned)std::min<uint64_t>(1024, (chunks + 255) / 256)), dim3(256), 0,
                           c->stream, c->d_model_aux.as<const uint32_t>(), in->seed, count, in->rand_lo, in->rand_hi, m.mat);
        VPX_HIP(c, hipGetLastError());
        res.seed = vpx_xorshift32_jump(in->seed, count);
        mat = m.mat;
    }
    const uint64_t threads = (uint64_t)n * n * ((n % 16u) ? n : n / 16);
    hipLaunchKernelGGL(model_gather_k, dim3((unsigned)std::min<uint64_t>(4096, (threads + 255) / 256)), dim3(256), 0,
                       c->stream, c->grids[id].ptr, n, (const uint8_t*)d_plan, m.vox, mat, m.sx, m.sy);
    VPX_HIP(c, hipGetLastError());
    if (int rc = build_masks(c, id)) return rc;
    if (out) *out = res;
    return VPX_OK;
}

int vpx_grid_generate_noise(vpx_ctx* c, uint32_t id, uint32_t n, const vpx_noise_gen* in, vpx_noise_result* out) {
    VPX_GROUP_ALL(c, vpx_grid_generate_noise(m_, id, n, in, out));
    if (!c) return VPX_E_INVALID;
    if (const char* why = noise::check_gen(in, n)) return fail(c, VPX_E_INVALID, why);
    if (id > 4096) return fail(c, VPX_E_INVALID, "grid_id too large");
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));  // frames in flight still read the grid
    if (int rc = ensure_model_aux(c)) return rc;
    const uint64_t total = (uint64_t)n * n * n, blocks = (total + noise::kBlockCells - 1) / noise::kBlockCells;
    uint64_t drawers = 2 * total;  // SMOKE: two per cell
    uint32_t *d_counts = nullptr;
    uint64_t *d_total = nullptr, *d_offsets = nullptr;
    if (in->mode == VPX_GEN_NOISE) {  // the prefix buffer of this call: total | offsets | counts
        if (int rc = ensure_scratch(c, (size_t)(8 + 12 * blocks))) return rc;
        d_total = c->d_scratch.as<uint64_t>();
        d_offsets = d_total + 1;
        d_counts = (uint32_t*)(d_offsets + blocks);
    }
    if (id >= c->grids.size() || !c->grids[id].ptr || c->grids[id].n != n)
        if (int rc = alloc_grid(c, id, n)) return rc;
    uint8_t* cells = c->grids[id].ptr;
    const uint32_t* tables = c->d_model_aux.as<const uint32_t>();
    const uint32_t noise_seed = model::xs32_step(in->seed);
    const dim3 grid((unsigned)std::min<uint64_t>(8192, blocks)), wg(noise::kBlockThreads);
    if (in->mode == VPX_GEN_SMOKE) {
        hipLaunchKernelGGL(smoke_gen_k, grid, wg, 0, c->stream, cells, n, in->frequency, (int32_t)noise_seed, tables,
                           in->seed, blocks);
        VPX_HIP(c, hipGetLastError());
    } else {
        hipLaunchKernelGGL(noise_mark_k, grid, wg, 0, c->stream, cells, n, in->frequency, (int32_t)noise_seed, blocks,
                           d_counts);
        VPX_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(noise_scan_k, dim3(1), dim3(noise::kScanPass), 0, c->stream, (const uint32_t*)d_counts, blocks,
                           d_offsets, d_total);
        VPX_HIP(c, hipGetLastError());
        hipLaunchKernelGGL(noise_draw_k, grid, wg, 0, c->stream, cells, n, tables, in->seed, blocks,
                           (const uint32_t*)d_counts, (const uint64_t*)d_offsets);
        VPX_HIP(c, hipGetLastError());
        VPX_HIP(c, hipMemcpyAsync(&drawers, d_total, sizeof(drawers), hipMemcpyDeviceToHost, c->stream));
    }
    if (int rc = build_masks(c, id)) return rc;  // ends with sync_all: `drawers` has arrived
    if (out) {
        out->noise_seed = noise_seed;
        out->draws = 1 + drawers;
        out->seed = vpx_xorshift32_jump(in->seed, out->draws);
    }
    return VPX_OK;
}

int vpx_grid_read_box(vpx_ctx* c, uint32_t id, uint8_t* dst, uint32_t x0, uint32_t y0, uint32_t z0, uint32_t dx,
                      uint32_t dy, uint32_t dz) {
    VPX_GROUP_FIRST(c, vpx_grid_read_box(m_, id, dst, x0, y0, z0, dx, dy, dz));
    if (!c || !dst) return fail(c, VPX_E_INVALID, "null argument");
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    const auto& g = c->grids[id];
    if ((uint64_t)x0 + dx > g.n || (uint64_t)y0 + dy > g.n || (uint64_t)z0 + dz > g.n)
        return fail(c, VPX_E_INVALID, "box outside the grid");
    const size_t bytes = (size_t)dx * dy * dz;
    if (!bytes) return VPX_OK;
    VPX_HIP(c, sync_all(c));
    if (dx == g.n && dy == g.n) {  // whole slabs are contiguous
        VPX_HIP(c, hipMemcpy(dst, g.ptr + (size_t)z0 * g.n * g.n, bytes, hipMemcpyDeviceToHost));
        return VPX_OK;
    }
    if (int rc = ensure_scratch(c, bytes)) return rc;
    hipLaunchKernelGGL(read_box_k, dim3((unsigned)std::min<size_t>(4096, (bytes + 255) / 256)), dim3(256), 0, c->stream,
                       g.ptr, g.n, c->d_scratch.as<uint8_t>(), x0, y0, z0, dx, dy, dz);
    VPX_HIP(c, hipGetLastError());
    VPX_HIP(c, hipMemcpyAsync(dst, c->d_scratch, bytes, hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

int vpx_grid_checksum(vpx_ctx* c, uint32_t id, uint64_t* out) {
    VPX_GROUP_FIRST(c, vpx_grid_checksum(m_, id, out));
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    const uint64_t count = (uint64_t)c->grids[id].n * c->grids[id].n * c->grids[id].n;
    VPX_HIP(c, hipMemsetAsync(c->d_sum, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(checksum_k, dim3(2048), dim3(256), 0, c->stream, c->grids[id].ptr, count, c->d_sum);
    VPX_HIP(c, hipGetLastError());
    unsigned long long h = 0;
    VPX_HIP(c, hipMemcpyAsync(&h, c->d_sum, sizeof(h), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, sync_all(c));
    *out = (uint64_t)h;
    return VPX_OK;
}

int vpx_grid_wide_planes(vpx_ctx* c, uint32_t id, uint32_t* out, uint64_t count) {
    VPX_GROUP_FIRST(c, vpx_grid_wide_planes(m_, id, out, count));
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    const auto& g = c->grids[id];
    if (count > 24 * g.plane()) return fail(c, VPX_E_INVALID, "more words than the axis planes hold");
    VPX_HIP(c, hipMemcpyAsync(out, g.dfp + 8 * g.plane(), count * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

int vpx_grid_axis_planes(vpx_ctx* c, uint32_t id, uint16_t* out, uint64_t count) {
    VPX_GROUP_FIRST(c, vpx_grid_axis_planes(m_, id, out, count));
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    if (count > 24 * c->grids[id].plane()) return fail(c, VPX_E_INVALID, "more words than the axis planes hold");
    std::vector<uint32_t> words(count);
    if (int r = vpx_grid_wide_planes(c, id, words.data(), count)) return r;
    for (uint64_t i = 0; i < count; ++i) out[i] = (uint16_t)words[i];
    return VPX_OK;
}

int vpx_grid_level_words(vpx_ctx* c, uint32_t id, uint32_t level, uint64_t* out, uint64_t count) {
    VPX_GROUP_FIRST(c, vpx_grid_level_words(m_, id, level, out, count));
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    if (id >= c->grids.size() || !c->grids[id].ptr) return fail(c, VPX_E_INVALID, "unknown grid");
    if (level != 1u && level != 2u) return fail(c, VPX_E_INVALID, "level must be 1 or 2");
    const auto& g = c->grids[id];
    const uint64_t words = level == 1u ? g.plane() : 64ull * g.nb3 * g.nb3 * g.nb3;
    if (count > words) return fail(c, VPX_E_INVALID, "more words than the level holds");
    VPX_HIP(c, hipMemcpyAsync(out, level == 1u ? g.l1 : g.l2, count * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

// The world box a volume's walks are culled with (misses_volume, the TLAS): the cube b0..b1
// through the inverse of inv_matrix's affine part (rows 0-2: every transform of the path —
// xform_pos_ssem / xform_pos, TransformPosition(_SSEM), tmpl8math.cpp:345-402 — reads only
// those; SetTransform's inverse leaves m[15] = 1 +- 1 ulp on a third of C4's instances), its 8
// corners in double, padded by 0.1 % of the half-diagonal + 1e-3 of the scale and rounded
// outward to float, so that the reference's float cube test (Setup3DDDA) can only succeed, and
// its walk only read a cell, for rays whose segment meets the box.  A singular 3x3 part gives
// an infinite box (never culled).  [0] = lo, [1] = hi (w = 0).
struct VolBox {
    float4 lo, hi;
};
static VolBox volume_bounds(const vpx_volume& v) {
    const float* m = v.inv_matrix;
    const double a[3][3] = {{m[0], m[1], m[2]}, {m[4], m[5], m[6]}, {m[8], m[9], m[10]}};
    const double det = a[0][0] * (a[1][1] * a[2][2] - a[1][2] * a[2][1]) -
                       a[0][1] * (a[1][0] * a[2][2] - a[1][2] * a[2][0]) +
                       a[0][2] * (a[1][0] * a[2][1] - a[1][1] * a[2][0]);
    const VolBox none{make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f), make_float4(INFINITY, INFINITY, INFINITY, 0.f)};
    if (!(std::fabs(det) > 1e-30)) return none;
    double r[3][3];  // inverse of the 3x3 part
    r[0][0] = (a[1][1] * a[2][2] - a[1][2] * a[2][1]) / det;
    r[0][1] = (a[0][2] * a[2][1] - a[0][1] * a[2][2]) / det;
    r[0][2] = (a[0][1] * a[1][2] - a[0][2] * a[1][1]) / det;
    r[1][0] = (a[1][2] * a[2][0] - a[1][0] * a[2][2]) / det;
    r[1][1] = (a[0][0] * a[2][2] - a[0][2] * a[2][0]) / det;
    r[1][2] = (a[0][2] * a[1][0] - a[0][0] * a[1][2]) / det;
    r[2][0] = (a[1][0] * a[2][1] - a[1][1] * a[2][0]) / det;
    r[2][1] = (a[0][1] * a[2][0] - a[0][0] * a[2][1]) / det;
    r[2][2] = (a[0][0] * a[1][1] - a[0][1] * a[1][0]) / det;
    const double t[3] = {m[3], m[7], m[11]};
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 8; ++k) {
        const double q[3] = {(k & 1) ? v.b1[0] : v.b0[0], (k & 2) ? v.b1[1] : v.b0[1], (k & 4) ? v.b1[2] : v.b0[2]};
        for (int i = 0; i < 3; ++i) {
            const double p = r[i][0] * (q[0] - t[0]) + r[i][1] * (q[1] - t[1]) + r[i][2] * (q[2] - t[2]);
            lo[i] = std::min(lo[i], p), hi[i] = std::max(hi[i], p);
        }
    }
    double half = 0.0, cen = 0.0;
    for (int i = 0; i < 3; ++i) {
        half += (hi[i] - lo[i]) * (hi[i] - lo[i]) / 4.0;
        cen += std::fabs((lo[i] + hi[i]) / 2.0);
    }
    half = std::sqrt(half);
    const double pad = half * 1e-3 + 1e-3 * (1.0 + cen + half);
    VolBox b;
    float* out[2] = {&b.lo.x, &b.hi.x};
    for (int i = 0; i < 3; ++i) {
        if (!std::isfinite(lo[i] - pad) || !std::isfinite(hi[i] + pad)) return none;
        out[0][i] = std::nextafter((float)(lo[i] - pad), -INFINITY);
        out[1][i] = std::nextafter((float)(hi[i] + pad), INFINITY);
    }
    b.lo.w = b.hi.w = 0.f;
    return b;
}

// Instance TLAS (the C4 lattice of 64 instances over the world volume): a BVH over the
// inflated world boxes (volume_bounds) of volumes 1..n-1, built once per
// vpx_set_volumes (volume 0, first in the reference's loop, is walked before the tree is
// asked, so the instances' candidates are bounded by its hit).
// Boxes are the volumes' boxes widened by a further 1e-4 of the scale and rounded outward to
// float, so every volume misses_volume keeps is a candidate.  Median split on the
// longest centroid axis (ties by index), leaves of <= 4 volumes (their bit mask), nodes in
// depth-first order with skip links (TlasNode).  Volumes without finite bounds go to the
// always-set.
#ifndef VPX_TLAS_LEAF
#define VPX_TLAS_LEAF 4  // volumes per TLAS leaf
#endif
struct TlasBuild {
    std::vector<TlasNode> nodes;
    struct Item {
        double lo[3], hi[3], c[3];
        uint32_t id;
    };
    std::vector<Item> items;
    void build(uint32_t first, uint32_t count) {
        const uint32_t me = (uint32_t)nodes.size();
        nodes.push_back(TlasNode{});
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t i = first; i < first + count; ++i)
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(lo[k], items[i].lo[k]), hi[k] = std::max(hi[k], items[i].hi[k]);
                clo[k] = std::min(clo[k], items[i].c[k]), chi[k] = std::max(chi[k], items[i].c[k]);
            }
        TlasNode nd{};
        for (int k = 0; k < 3; ++k) {
            nd.lo[k] = std::nextafter((float)lo[k], -INFINITY);
            nd.hi[k] = std::nextafter((float)hi[k], INFINITY);
        }
        if (count <= (uint32_t)VPX_TLAS_LEAF) {
            nd.leaf = 1;
            for (uint32_t i = first; i < first + count; ++i) nd.mask |= 1ull << (items[i].id - 1u);
            nodes[me] = nd;
            return;
        }
        int axis = 0;
        for (int k = 1; k < 3; ++k)
            if (chi[k] - clo[k] > chi[axis] - clo[axis]) axis = k;
        std::stable_sort(items.begin() + first, items.begin() + first + count,
                         [axis](const Item& x, const Item& y) { return x.c[axis] < y.c[axis]; });
        const uint32_t half = count / 2;
        build(first, half);
        build(first + half, count - half);
        nd.skip = (uint32_t)nodes.size();  // the node after this subtree
        nodes[me] = nd;
    }
};

int build_tlas(vpx_ctx* c, const std::vector<VolBox>& bounds) {
    c->tlas_on = false;
    c->tlas_nodes = 0;
    c->tlas_always = 0;
    const uint32_t count = (uint32_t)bounds.size();
    if (count < 2 || count > kTlasMaxVolumes) return VPX_OK;  // one volume / too many: the linear loop
    TlasBuild b;
    for (uint32_t i = 1; i < count; ++i) {  // volume 0 is walked first, outside the tree
        const VolBox& vb = bounds[i];
        const double lo[3] = {vb.lo.x, vb.lo.y, vb.lo.z}, hi[3] = {vb.hi.x, vb.hi.y, vb.hi.z};
        if (!std::isfinite(lo[0] + lo[1] + lo[2] + hi[0] + hi[1] + hi[2])) {
            c->tlas_always |= 1ull << (i - 1u);
            continue;
        }
        double half = 0.0, cen = 0.0;
        for (int k = 0; k < 3; ++k) half += (hi[k] - lo[k]) * (hi[k] - lo[k]) / 4.0, cen += std::fabs((lo[k] + hi[k]) / 2.0);
        half = std::sqrt(half);
        const double pad = half * 1e-4 + 1e-4 * (1.0 + cen + half);
        TlasBuild::Item it{};
        for (int k = 0; k < 3; ++k) it.lo[k] = lo[k] - pad, it.hi[k] = hi[k] + pad, it.c[k] = (lo[k] + hi[k]) / 2.0;
        it.id = i;
        b.items.push_back(it);
    }
    if (!b.items.empty()) b.build(0, (uint32_t)b.items.size());
    if (b.nodes.size() > kTlasMaxNodes) return fail(c, VPX_E_INVALID, "TLAS node budget exceeded");
    if (!c->d_tlas) VPX_HIP(c, c->d_tlas.alloc(sizeof(TlasNode) * kTlasMaxNodes));
    if (!b.nodes.empty())
        VPX_HIP(c, hipMemcpy(c->d_tlas, b.nodes.data(), sizeof(TlasNode) * b.nodes.size(), hipMemcpyHostToDevice));
    c->tlas_nodes = (uint32_t)b.nodes.size();
    c->tlas_on = true;
    return VPX_OK;
}

int vpx_set_volumes(vpx_ctx* c, const vpx_volume* v, uint32_t count) {
    VPX_GROUP_ALL(c, vpx_set_volumes(m_, v, count));
    if (!c || (!v && count)) return fail(c, VPX_E_INVALID, "null argument");
    if (count > 65536) return fail(c, VPX_E_INVALID, "too many volumes");
    VPX_HIP(c, sync_all(c));
    if (sizeof(vpx_volume) * count > c->d_volumes.bytes) {
        // the tables grow together, and the host copy (the kernels' count) is empty until both
        // are there; the wait above covers the frames that read the old ones
        c->volumes.clear();
        c->d_volumes.release();
        c->d_vbounds.release();
        VPX_HIP(c, c->d_volumes.alloc(sizeof(vpx_volume) * count));
        VPX_HIP(c, c->d_vbounds.alloc(sizeof(VolBox) * count));
    }
    // Invariant: d_volumes, d_vbounds and the TLAS (d_tlas) describe the same volumes.  The
    // instance kernels cull by the TLAS root box and the bounding spheres (FindNearest's
    // candidates, the shadow pool's slot list), so a volume update that skipped build_tlas would
    // silently drop instance hits and shadows: every writer of d_volumes goes through here.
    c->volumes.assign(v, v + count);
    std::vector<VolBox> bounds(count);
    for (uint32_t i = 0; i < count; ++i) bounds[i] = volume_bounds(v[i]);
    if (count) {
        VPX_HIP(c, hipMemcpy(c->d_volumes, v, sizeof(vpx_volume) * count, hipMemcpyHostToDevice));
        VPX_HIP(c, hipMemcpy(c->d_vbounds, bounds.data(), sizeof(VolBox) * count, hipMemcpyHostToDevice));
    }
    return build_tlas(c, bounds);
}

int vpx_volume_bounds(const vpx_volume* v, float out[6]) {
    if (!v || !out) return VPX_E_INVALID;
    const VolBox b = volume_bounds(*v);
    out[0] = b.lo.x, out[1] = b.lo.y, out[2] = b.lo.z, out[3] = b.hi.x, out[4] = b.hi.y, out[5] = b.hi.z;
    return VPX_OK;
}

int vpx_set_materials(vpx_ctx* c, const vpx_material* m, uint32_t count) {
    VPX_GROUP_ALL(c, vpx_set_materials(m_, m, count));
    if (!c || !m) return fail(c, VPX_E_INVALID, "null argument");
    if (count == 0 || count > VPX_NUM_MATERIALS) return fail(c, VPX_E_INVALID, "material count must be 1..256");
    vpx_material full[VPX_NUM_MATERIALS];
    // entries past `count` behave like MaterialSetUp's padding: white, roughness 1
    for (auto& e : full) e = vpx_material{{1, 1, 1}, 1.0f, 0.0f, 1.5f, {0, 0}};
    std::memcpy(full, m, sizeof(vpx_material) * count);
    VPX_HIP(c, sync_all(c));
    // the table's allocation is made once and ends in the player light record (probe_record):
    // a new table leaves what the record has accumulated
    if (!c->d_materials) {
        static_assert(sizeof(full) == kProbeOffset, "the table's size is the record's offset");
        VPX_HIP(c, c->d_materials.alloc(kMaterialTableBytes));
        VPX_HIP(c, hipMemsetAsync(probe_record_of(c->d_materials), 0, kProbeBytes, c->stream));
    }
    VPX_HIP(c, hipMemcpyAsync(c->d_materials, full, sizeof(full), hipMemcpyHostToDevice, c->stream));
    VPX_HIP(c, sync_all(c));
    c->have_materials = true;
    return VPX_OK;
}

int vpx_set_lights(vpx_ctx* c, const vpx_point_light* p, uint32_t np, const vpx_spot_light* s, uint32_t ns,
                   const vpx_area_light* a, uint32_t na, const vpx_dir_light* d) {
    VPX_GROUP_ALL(c, vpx_set_lights(m_, p, np, s, ns, a, na, d));
    if (!c) return VPX_E_INVALID;
    VPX_HIP(c, sync_all(c));
    int rc;
    if ((rc = upload_table(c, c->points, p, np))) return rc;
    if ((rc = upload_table(c, c->spots, s, ns))) return rc;
    if ((rc = upload_table(c, c->areas, a, na))) return rc;
    VPX_HIP(c, sync_all(c));
    if (d) c->dir = *d;
    return VPX_OK;
}

int vpx_set_shapes(vpx_ctx* c, const vpx_sphere* s, uint32_t ns, const vpx_triangle* t, uint32_t nt) {
    VPX_GROUP_ALL(c, vpx_set_shapes(m_, s, ns, t, nt));
    if (!c) return VPX_E_INVALID;
    VPX_HIP(c, sync_all(c));
    int rc;
    if ((rc = upload_table(c, c->spheres, s, ns))) return rc;
    if ((rc = upload_table(c, c->triangles, t, nt))) return rc;
    VPX_HIP(c, sync_all(c));
    return VPX_OK;
}

int vpx_set_sky(vpx_ctx* c, const float* rgb, uint32_t width, uint32_t height, float hdr_contribution) {
    VPX_GROUP_ALL(c, vpx_set_sky(m_, rgb, width, height, hdr_contribution));
    if (!c) return VPX_E_INVALID;
    VPX_HIP(c, hipSetDevice(c->device));
    if (!rgb || !width || !height) {  // remove the texture (misses use the constant sky)
        if (c->sky.px) VPX_HIP(c, sync_all(c));
        c->sky = vpx_ctx::Sky{};
        return VPX_OK;
    }
    if ((uint64_t)width * height > (1ull << 28)) return fail(c, VPX_E_INVALID, "sky texture too large");
    const size_t bytes = sizeof(float) * 3 * (size_t)width * height;
    if ((size_t)c->sky.w * c->sky.h != (size_t)width * height) {  // no sky until the new one is whole
        VPX_HIP(c, sync_all(c));
        c->sky = vpx_ctx::Sky{};
        VPX_HIP(c, c->sky.px.alloc(bytes));
    }
    VPX_HIP(c, sync_all(c));  // frames in flight still read the texture
    VPX_HIP(c, hipMemcpyAsync(c->sky.px, rgb, bytes, hipMemcpyHostToDevice, c->stream));
    VPX_HIP(c, sync_all(c));
    c->sky.w = width, c->sky.h = height;
    c->sky_hdr = hdr_contribution;
    return VPX_OK;
}

int vpx_set_arithmetic(vpx_ctx* c, uint32_t mode) {
    VPX_GROUP_ALL(c, vpx_set_arithmetic(m_, mode));
    if (!c) return VPX_E_INVALID;
    if (mode != VPX_ARITH_EXACT && mode != VPX_ARITH_X86_HOST) return fail(c, VPX_E_INVALID, "unknown arithmetic mode");
    VPX_HIP(c, hipSetDevice(c->device));
    VPX_HIP(c, sync_all(c));  // frames in flight read the tables
    c->d_x86.release();
    c->x86 = X86Arith{nullptr, 0u, 0u, 0u, 0u};
    if (mode == VPX_ARITH_EXACT) return VPX_OK;
    uint32_t info[4];
    if (vpx_x86_arith_tables(nullptr, 0, info) != VPX_OK)
        return fail(c, VPX_E_STATE, "the host's rcpss / rsqrtss do not follow the table model (or the host is not x86)");
    if (23u - info[0] > kX86LdsBits)  // the multi-volume walkers stage the rcp table in LDS
        return fail(c, VPX_E_STATE, "the host's rcpss key is wider than the LDS-staged table allows");
    std::vector<uint32_t> tab(info[3]);
    if (vpx_x86_arith_tables(tab.data(), tab.size(), info) != VPX_OK) return fail(c, VPX_E_STATE, "table capture failed");
    VPX_HIP(c, c->d_x86.alloc(sizeof(uint32_t) * tab.size()));
    VPX_HIP(c, hipMemcpy(c->d_x86, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
    c->x86 = X86Arith{c->d_x86, info[0], info[1], info[2], 0u};
    return VPX_OK;
}

int vpx_set_camera(vpx_ctx* c, const vpx_camera* cam) {
    VPX_GROUP_ALL(c, vpx_set_camera(m_, cam));
    if (!c || !cam) return fail(c, VPX_E_INVALID, "null argument");
    c->cam = *cam;
    c->have_camera = true;
    return VPX_OK;
}

static int group_render(vpx_ctx* c, const vpx_frame_params* p, float* accum, uint32_t* rgb8, vpx_stats* stats);

int vpx_render(vpx_ctx* c, const vpx_frame_params* p, float* accum, uint32_t* rgb8, vpx_stats* stats) {
    if (!c) return VPX_E_INVALID;
    if (!c->members.empty()) return group_render(c, p, accum, rgb8, stats);
    int rc = validate_frame(c, p);
    if (rc) return rc;
    if (!accum) return fail(c, VPX_E_INVALID, "accum (device float4[W*H]) is required");
    VPX_HIP(c, hipSetDevice(c->device));
    const SceneView sv = view_of(c, p->sky, p->area_samples, (p->flags & VPX_FLAG_SKY) != 0);
    const FrameArgs f = frame_of(c, p, 0, 1);
    if (!c->lanes.empty() && !stats && !(p->flags & VPX_FLAG_NO_TONEMAP) && lane_tail_ok(sv, f)) {
        // frames in flight whose tail is a launch of its own (k_resolve_finish after the shadow
        // pool): the whole frame runs on its lane, the tail blending straight into the caller's
        // accumulator once the caller's stream has reached this call (which orders it after
        // the previous frame's tail): no packed sample, no composite (32 B per pixel less)
        vpx_ctx::Lane& L = c->lanes[c->lane_next];
        c->lane_next = (c->lane_next + 1u) % (uint32_t)c->lanes.size();
        if (L.used) VPX_HIP(c, hipStreamWaitEvent(L.s, L.consumed, 0));
        VPX_HIP(c, hipEventRecord(L.caller, c->stream));
        if ((rc = launch_render<kFinishImage>(c, L.s, L.ws, sv, f, f.num_tiles, reinterpret_cast<float4*>(accum), rgb8,
                                              nullptr, nullptr, &L.caller)))
            return rc;
        VPX_HIP(c, hipEventRecord(L.rendered, L.s));
        VPX_HIP(c, hipStreamWaitEvent(c->stream, L.rendered, 0));
        VPX_HIP(c, hipEventRecord(L.consumed, L.s));
        L.used = true;
        return VPX_OK;
    }
    if (!c->lanes.empty() && !stats && !(p->flags & VPX_FLAG_NO_TONEMAP)) {
        // frames in flight: the frame renders on a lane; its accumulate / tonemap runs on the
        // caller's stream after the previous frame's (the same blend of the same sample)
        vpx_ctx::Lane* L = nullptr;
        if ((rc = lane_render(c, sv, f, f.num_tiles, nullptr, L))) return rc;
        hipLaunchKernelGGL(composite_tiles, dim3(f.num_tiles), dim3(kThreads), 0, c->stream, f, L->cur,
                           reinterpret_cast<float4*>(accum), rgb8);
        VPX_HIP(c, hipGetLastError());
        VPX_HIP(c, hipEventRecord(L->cur_consumed, c->stream));
        return VPX_OK;
    }
    unsigned long long before[kCtrWords] = {};
    if (stats && (rc = snapshot_counters(c, before))) return rc;
    if (stats) VPX_HIP(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = launch_render<kFinishImage>(c, c->stream, c->wave, sv, f, f.num_tiles, reinterpret_cast<float4*>(accum), rgb8,
                                          nullptr)))
        return rc;
    if (stats) {
        VPX_HIP(c, hipEventRecord(c->ev1, c->stream));
        unsigned long long after[kCtrWords];
        if ((rc = snapshot_counters(c, after))) return rc;
        std::memset(stats, 0, sizeof(*stats));
        fill_stats(stats, before, after);
        float ms = 0.f;
        VPX_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        stats->kernel_ms = ms;
        stats->total_ms = ms;
    }
    return VPX_OK;
}

int vpx_render_reproject(vpx_ctx* c, const vpx_frame_params* p, const vpx_prev_camera* prev, float* history,
                         uint32_t* rgb8, vpx_stats* stats) {
    VPX_GROUP_FIRST(c, vpx_render_reproject(m_, p, prev, history, rgb8, stats));
    if (!c) return VPX_E_INVALID;
    int rc = validate_frame(c, p);
    if (rc) return rc;
    if (!prev || !history) return fail(c, VPX_E_INVALID, "prev camera and history (device float4[W*H]) are required");
    VPX_HIP(c, hipSetDevice(c->device));
    const size_t pix = (size_t)p->width * p->height;
    // an earlier frame of the path may still read the old images: wait
    if ((rc = c->rp_buf.grow(c, sizeof(float4) * 4 * pix, true))) return rc;
    Reproj rp;
    auto h3 = [](const float* v) { return f3{v[0], v[1], v[2]}; };
    rp.prev = PrevCam{h3(prev->cam_pos), h3(prev->left_normal), h3(prev->right_normal), h3(prev->top_normal),
                      h3(prev->bottom_normal)};
    rp.alb = c->rp_buf, rp.ill = c->rp_buf + pix, rp.rd = c->rp_buf + 2 * pix, rp.temp = c->rp_buf + 3 * pix;
    rp.hist = reinterpret_cast<float4*>(history);
    unsigned long long before[kCtrWords] = {};
    if (stats && (rc = snapshot_counters(c, before))) return rc;
    const SceneView sv = view_of(c, p->sky, p->area_samples, (p->flags & VPX_FLAG_SKY) != 0);
    FrameArgs f = frame_of(c, p, 0, 1);
    f.flags = (f.flags & ~(VPX_FLAG_AA | VPX_FLAG_DOF)) | kFlagReproject;  // GetPrimaryRayNoDOF
    if (stats) VPX_HIP(c, hipEventRecord(c->ev0, c->stream));
    if ((rc = launch_render<kFinishImage>(c, c->stream, c->wave, sv, f, f.num_tiles, nullptr, rgb8, nullptr, &rp))) return rc;
    if (stats) {
        VPX_HIP(c, hipEventRecord(c->ev1, c->stream));
        unsigned long long after[kCtrWords];
        if ((rc = snapshot_counters(c, after))) return rc;
        std::memset(stats, 0, sizeof(*stats));
        fill_stats(stats, before, after);
        float ms = 0.f;
        VPX_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        stats->kernel_ms = ms;
        stats->total_ms = ms;
    }
    return VPX_OK;
}

uint64_t vpx_tiles_packed_len(uint32_t width, uint32_t height, uint32_t tile_w, uint32_t tile_h, uint32_t n_ranks) {
    if (!width || !height || !n_ranks || tile_w != kTile || tile_h != kTile) return 0;
    const uint64_t tiles = (uint64_t)((width + kTile - 1) / kTile) * ((height + kTile - 1) / kTile);
    return ((tiles + n_ranks - 1) / n_ranks) * (uint64_t)(kTile * kTile);
}

// Shared body of vpx_render_tiles (packed samples) and vpx_render_tiles_accum (this rank's
// packed accumulator + RGB8); MODE is a FinishMode.
static int render_tiles_impl(int MODE, vpx_ctx* c, const vpx_frame_params* p, uint32_t tile_w, uint32_t tile_h,
                             uint32_t rank, uint32_t n_ranks, float4* accum, uint32_t* rgb8, float4* packed,
                             vpx_stats* stats) {
    if (!c) return VPX_E_INVALID;
    int rc = validate_frame(c, p);
    if (rc) return rc;
    if (tile_w != kTile || tile_h != kTile) return fail(c, VPX_E_INVALID, "tiles must be 16x16");
    if (n_ranks == 0 || rank >= n_ranks) return fail(c, VPX_E_INVALID, "bad rank");
    if (MODE == kFinishPackedSample ? !packed : (!accum || !rgb8))
        return fail(c, VPX_E_INVALID, "null packed buffer");
    VPX_HIP(c, hipSetDevice(c->device));
    const SceneView sv = view_of(c, p->sky, p->area_samples, (p->flags & VPX_FLAG_SKY) != 0);
    const FrameArgs f = frame_of(c, p, rank, n_ranks);
    // frames in flight (vpx_set_pipeline) for the sharded accumulator: the frame renders into
    // the lane's own samples and only the blend runs on the caller's stream.  Packed samples
    // into the caller's buffer stay serial: a lane would not wait for the caller's use of the
    // previous frame's samples (e.g. a gather queued on its stream).
    if (MODE == kFinishPackedAccum && !c->lanes.empty() && !stats) {
        vpx_ctx::Lane* L = nullptr;
        if ((rc = lane_render(c, sv, f, f.tiles_per_rank, nullptr, L))) return rc;
        const uint32_t P = f.tiles_per_rank * (uint32_t)kTilePix;  // this rank's running average, in frame order
        hipLaunchKernelGGL(blend_packed, dim3(f.tiles_per_rank), dim3(kThreads), 0, c->stream, f, L->cur, accum, rgb8,
                           P);
        VPX_HIP(c, hipGetLastError());
        VPX_HIP(c, hipEventRecord(L->cur_consumed, c->stream));
        return VPX_OK;
    }
    unsigned long long before[kCtrWords] = {};
    if (stats && (rc = snapshot_counters(c, before))) return rc;
    if (stats) VPX_HIP(c, hipEventRecord(c->ev0, c->stream));
    rc = MODE == kFinishPackedSample
             ? launch_render<kFinishPackedSample>(c, c->stream, c->wave, sv, f, f.tiles_per_rank, accum, rgb8, packed)
             : launch_render<kFinishPackedAccum>(c, c->stream, c->wave, sv, f, f.tiles_per_rank, accum, rgb8, packed);
    if (rc) return rc;
    if (stats) {
        VPX_HIP(c, hipEventRecord(c->ev1, c->stream));
        unsigned long long after[kCtrWords];
        if ((rc = snapshot_counters(c, after))) return rc;
        std::memset(stats, 0, sizeof(*stats));
        fill_stats(stats, before, after);
        float ms = 0.f;
        VPX_HIP(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
        stats->kernel_ms = ms;
        stats->total_ms = ms;
    }
    return VPX_OK;
}

// Tiles per window chain: frames join a chain while it holds at most this many tiles, and
// (with lanes) a window keeps at least one chain per lane.  C4 (32400 tiles a frame, 16 spp,
// 4 lanes): one GPU renders 4 chains of 4 frames (26.9 ms a step against 28.5 frame by
// frame), rank 0 of 8 (4050 tiles) 4 chains of 4 frames (3.7 ms against 7.3): profiles/r06_window_ab.txt.
#ifndef VPX_WINDOW_TILES
#define VPX_WINDOW_TILES 131072
#endif
// Window chains of big frames (at least this many tiles a frame) whose tail is a launch of
// its own blend in that tail (k_finish_window), once the previous chain's tail has run: C4 one
// GPU 26.60-26.66 vs 26.95 ms per step.  Small shares keep the blend on the caller's stream
// (blend_window): the tail's wait for the previous chain held each lane (C4 rank 0 of 8: 4.12
// vs 3.68 ms), profiles/r06_window_ab.txt.  0 = never.
#ifndef VPX_WINDOW_FUSED
#define VPX_WINDOW_FUSED 16384
#endif
#ifndef VPX_WINDOW_LANE_CAP
#define VPX_WINDOW_LANE_CAP 1
#endif

static int render_window_impl(vpx_ctx* c, const vpx_frame_params* p, uint32_t n, uint32_t rank, uint32_t n_ranks,
                              bool image, float* accum, uint32_t* rgb8) {
    if (!c) return VPX_E_INVALID;
    int rc = validate_frame(c, p);
    if (rc) return rc;
    if (n == 0) return VPX_OK;
    if (image ? !accum : (!accum || !rgb8)) return fail(c, VPX_E_INVALID, "null accumulator buffer");
    if (n_ranks == 0 || rank >= n_ranks) return fail(c, VPX_E_INVALID, "bad rank");
    const FrameArgs f0 = frame_of(c, p, rank, n_ranks);
    const uint32_t T = image ? f0.num_tiles : f0.tiles_per_rank;
    uint32_t bmax = std::min<uint32_t>(kMaxWindow, std::max<uint32_t>(1u, VPX_WINDOW_TILES / T));
    // at least one chain per lane, so the lanes keep chains in flight as they do frames
    if (VPX_WINDOW_LANE_CAP && c->lanes.size() > 1)
        bmax = std::min<uint32_t>(bmax, std::max<uint32_t>(1u, (n + (uint32_t)c->lanes.size() - 1) / (uint32_t)c->lanes.size()));
    // the shadow lists pack a path index into 27 bits (validate_frame's bound per chain)
    while (bmax > 1 && (uint64_t)bmax * T * kTilePix > (1ull << 27)) --bmax;
    const bool per_frame = bmax == 1 || n == 1 || (p->flags & VPX_FLAG_NO_TONEMAP);  // (a device set never gets here)
    for (uint32_t i = 0; i < n;) {
        vpx_frame_params q = *p;
        q.frame_index = p->frame_index + i;
        if (per_frame) {
            rc = image ? vpx_render(c, &q, accum, rgb8, nullptr)
                       : vpx_render_tiles_accum(c, &q, kTile, kTile, rank, n_ranks, accum, rgb8, nullptr);
            if (rc) return rc;
            ++i;
            continue;
        }
        const uint32_t B = std::min(bmax, n - i);
        VPX_HIP(c, hipSetDevice(c->device));
        const SceneView sv = view_of(c, q.sky, q.area_samples, (q.flags & VPX_FLAG_SKY) != 0);
        FrameArgs f = frame_of(c, &q, rank, n_ranks);
        f.batch_tiles = T;
        WindowWeights ww;
        for (uint32_t b = 0; b < B; ++b) {  // frame_of's weight per frame
            ww.w[b] = 1.0f / ((float)(q.frame_index + b) + 1.0f);
            ww.iw[b] = 1.0f - ww.w[b];
        }
        float4* samples = nullptr;
        vpx_ctx::Lane* L = nullptr;
        if (!c->lanes.empty() && VPX_WINDOW_FUSED && T >= VPX_WINDOW_FUSED && lane_tail_ok(sv, f)) {
            // the chain's own tail blends its frames into the accumulator (k_finish_window) on
            // its lane, once the caller's stream has reached this call — which orders it after
            // the previous chain's tail, as vpx_render's lane_tail_ok frames
            vpx_ctx::Lane& FL = c->lanes[c->lane_next];
            c->lane_next = (c->lane_next + 1u) % (uint32_t)c->lanes.size();
            if (FL.used) VPX_HIP(c, hipStreamWaitEvent(FL.s, FL.consumed, 0));
            VPX_HIP(c, hipEventRecord(FL.caller, c->stream));
            WindowTail wt;
            wt.B = B;
            wt.image = image ? 1 : 0;
            wt.ww = ww;
            if ((rc = launch_render<kFinishPackedSample>(c, FL.s, FL.ws, sv, f, B * T, reinterpret_cast<float4*>(accum),
                                                         rgb8, nullptr, nullptr, &FL.caller, &wt)))
                return rc;
            VPX_HIP(c, hipEventRecord(FL.rendered, FL.s));
            VPX_HIP(c, hipStreamWaitEvent(c->stream, FL.rendered, 0));
            VPX_HIP(c, hipEventRecord(FL.consumed, FL.s));
            FL.used = true;
            i += B;
            continue;
        }
        if (!c->lanes.empty()) {
            if ((rc = lane_render(c, sv, f, B * T, nullptr, L))) return rc;
            samples = L->cur;
        } else {
            const size_t need = (size_t)B * T * kTilePix;
            // the previous chain's blend still reads the old samples: wait (no lanes here, so
            // everything queued is the stream's)
            if ((rc = c->win_buf.grow(c, sizeof(float4) * need, true))) return rc;
            samples = c->win_buf;
            if ((rc = launch_render<kFinishPackedSample>(c, c->stream, c->wave, sv, f, B * T, nullptr, nullptr,
                                                         samples)))
                return rc;
        }
        hipLaunchKernelGGL(blend_window, dim3(T), dim3(kThreads), 0, c->stream, f, samples, B, ww, image ? 1 : 0,
                           reinterpret_cast<float4*>(accum), rgb8);
        VPX_HIP(c, hipGetLastError());
        if (L) VPX_HIP(c, hipEventRecord(L->cur_consumed, c->stream));
        i += B;
    }
    return VPX_OK;
}

int vpx_render_window(vpx_ctx* c, const vpx_frame_params* p, uint32_t n_frames, float* accum, uint32_t* rgb8) {
    if (c && !c->members.empty()) {
        // a device set keeps its camera and world in its members: frame by frame through
        // vpx_render (group_render validates, and takes accum == NULL with rgb8 given)
        if (!p) return fail(c, VPX_E_INVALID, "null params");
        for (uint32_t i = 0; i < n_frames; ++i) {
            vpx_frame_params q = *p;
            q.frame_index = p->frame_index + i;
            if (int rc = vpx_render(c, &q, accum, rgb8, nullptr)) return rc;
        }
        return VPX_OK;
    }
    return render_window_impl(c, p, n_frames, 0, 1, true, accum, rgb8);
}

int vpx_render_tiles_accum_window(vpx_ctx* c, const vpx_frame_params* p, uint32_t n_frames, uint32_t tile_w,
                                  uint32_t tile_h, uint32_t rank, uint32_t n_ranks, float* accum_packed,
                                  uint32_t* rgb8_packed) {
    VPX_GROUP_FIRST(c, vpx_render_tiles_accum_window(m_, p, n_frames, tile_w, tile_h, rank, n_ranks, accum_packed,
                                                     rgb8_packed));
    if (c && (tile_w != kTile || tile_h != kTile)) return fail(c, VPX_E_INVALID, "tiles must be 16x16");
    return render_window_impl(c, p, n_frames, rank, n_ranks, false, accum_packed, rgb8_packed);
}

int vpx_render_tiles(vpx_ctx* c, const vpx_frame_params* p, uint32_t tile_w, uint32_t tile_h, uint32_t rank,
                     uint32_t n_ranks, float* packed, vpx_stats* stats) {
    VPX_GROUP_FIRST(c, vpx_render_tiles(m_, p, tile_w, tile_h, rank, n_ranks, packed, stats));
    return render_tiles_impl(kFinishPackedSample, c, p, tile_w, tile_h, rank, n_ranks, nullptr, nullptr,
                                                  reinterpret_cast<float4*>(packed), stats);
}

int vpx_render_tiles_accum(vpx_ctx* c, const vpx_frame_params* p, uint32_t tile_w, uint32_t tile_h, uint32_t rank,
                           uint32_t n_ranks, float* accum_packed, uint32_t* rgb8_packed, vpx_stats* stats) {
    VPX_GROUP_FIRST(c, vpx_render_tiles_accum(m_, p, tile_w, tile_h, rank, n_ranks, accum_packed, rgb8_packed, stats));
    return render_tiles_impl(kFinishPackedAccum, c, p, tile_w, tile_h, rank, n_ranks,
                                                 reinterpret_cast<float4*>(accum_packed), rgb8_packed, nullptr, stats);
}

int vpx_composite_rgb8(vpx_ctx* c, const vpx_frame_params* p, uint32_t tile_w, uint32_t tile_h, uint32_t n_ranks,
                       const uint32_t* gathered, uint32_t* rgb8) {
    VPX_GROUP_FIRST(c, vpx_composite_rgb8(m_, p, tile_w, tile_h, n_ranks, gathered, rgb8));
    if (!c || !p || !gathered || !rgb8) return fail(c, VPX_E_INVALID, "null argument");
    if (tile_w != kTile || tile_h != kTile || n_ranks == 0) return fail(c, VPX_E_INVALID, "tiles must be 16x16");
    if (p->width == 0 || p->height == 0) return fail(c, VPX_E_INVALID, "empty frame");
    VPX_HIP(c, hipSetDevice(c->device));
    const FrameArgs f = frame_of(c, p, 0, n_ranks);
    hipLaunchKernelGGL(composite_rgb8, dim3(f.num_tiles), dim3(kThreads), 0, c->stream, f, gathered, rgb8);
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

int vpx_composite_tiles(vpx_ctx* c, const vpx_frame_params* p, uint32_t tile_w, uint32_t tile_h, uint32_t n_ranks,
                        const float* gathered, float* accum, uint32_t* rgb8) {
    VPX_GROUP_FIRST(c, vpx_composite_tiles(m_, p, tile_w, tile_h, n_ranks, gathered, accum, rgb8));
    if (!c || !p || !gathered || !accum) return fail(c, VPX_E_INVALID, "null argument");
    if (tile_w != kTile || tile_h != kTile || n_ranks == 0) return fail(c, VPX_E_INVALID, "tiles must be 16x16");
    if (p->width == 0 || p->height == 0) return fail(c, VPX_E_INVALID, "empty frame");
    VPX_HIP(c, hipSetDevice(c->device));
    const FrameArgs f = frame_of(c, p, 0, n_ranks);
    hipLaunchKernelGGL(composite_tiles, dim3(f.num_tiles), dim3(kThreads), 0, c->stream, f,
                       reinterpret_cast<const float4*>(gathered), reinterpret_cast<float4*>(accum), rgb8);
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

int vpx_get_counters(vpx_ctx* c, vpx_stats* out, int reset) {
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    if (!c->members.empty()) {  // sum over the devices
        std::memset(out, 0, sizeof(*out));
        return group_all(c, [&](vpx_ctx* m) {
            vpx_stats one;
            const int rc = vpx_get_counters(m, &one, reset);
            out->primary_rays += one.primary_rays, out->shadow_rays += one.shadow_rays;
            out->bounce_rays += one.bounce_rays, out->dda_cells += one.dda_cells;
            return rc;
        });
    }
    unsigned long long now[kCtrWords];
    int rc = snapshot_counters(c, now);
    if (rc) return rc;
    const unsigned long long zero[kCtrWords] = {};
    std::memset(out, 0, sizeof(*out));
    fill_stats(out, zero, now);
    if (reset) {
        VPX_HIP(c, hipMemsetAsync(c->d_ctr, 0, kCtrWords * kCtrStripes * sizeof(unsigned long long), c->stream));
        VPX_HIP(c, sync_all(c));
    }
    return VPX_OK;
}

int vpx_get_player_light(vpx_ctx* c, vpx_player_light* out, int reset) {
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    if (!c->members.empty()) {  // sums over the devices, the largest maximum
        const int rc = group_all(c, [&](vpx_ctx* m) {
            vpx_player_light one;
            const int r = vpx_get_player_light(m, &one, reset);
            out->probes += one.probes, out->lit += one.lit;
            out->max_sqr = std::max(out->max_sqr, one.max_sqr);
            return r;
        });
        out->in_light = out->lit ? 1u : 0u;
        return rc;
    }
    if (!c->d_materials) {  // no table yet, so no render yet: the stream's order still holds
        VPX_HIP(c, sync_all(c));
        return VPX_OK;
    }
    unsigned long long all[kProbeWords * kProbeStripes];
    static_assert(sizeof(all) == kProbeBytes, "the whole record");
    unsigned long long* rec = probe_record_of(c->d_materials);
    VPX_HIP(c, sync_all(c));  // frames in flight on lanes (their level forks join them) included
    VPX_HIP(c, hipMemcpyAsync(all, rec, sizeof(all), hipMemcpyDeviceToHost, c->stream));
    VPX_HIP(c, hipStreamSynchronize(c->stream));
    uint32_t bits = 0u;
    for (uint32_t s = 0; s < kProbeStripes; ++s) {
        out->probes += all[kProbeWords * s], out->lit += all[kProbeWords * s + 1];
        bits = std::max(bits, (uint32_t)all[kProbeWords * s + 2]);
    }
    std::memcpy(&out->max_sqr, &bits, sizeof(bits));
    out->in_light = out->lit ? 1u : 0u;
    if (reset) {
        VPX_HIP(c, hipMemsetAsync(rec, 0, kProbeBytes, c->stream));
        VPX_HIP(c, sync_all(c));
    }
    return VPX_OK;
}

int vpx_find_nearest(vpx_ctx* c, const vpx_ray* rays, uint32_t n, vpx_hit* hits) {
    VPX_GROUP_FIRST(c, vpx_find_nearest(m_, rays, n, hits));
    if (!c || (n && (!rays || !hits))) return fail(c, VPX_E_INVALID, "null argument");
    int rc = check_ready(c);
    if (rc) return rc;
    if (n == 0) return VPX_OK;
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}}, {{hits, sizeof(vpx_hit) * n}}, [&](void* const* in, void* const* out) {
        hipLaunchKernelGGL(find_nearest_k, dim3((n + 255) / 256), dim3(256), 0, c->stream, view_of(c, kQuerySky, 3),
                           (vpx_ray*)in[0], n, (vpx_hit*)out[0]);
    });
}

int vpx_is_occluded(vpx_ctx* c, const vpx_ray* rays, uint32_t n, uint8_t* occ) {
    VPX_GROUP_FIRST(c, vpx_is_occluded(m_, rays, n, occ));
    if (!c || (n && (!rays || !occ))) return fail(c, VPX_E_INVALID, "null argument");
    int rc = check_ready(c);
    if (rc) return rc;
    if (n == 0) return VPX_OK;
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}}, {{occ, n}}, [&](void* const* in, void* const* out) {
        hipLaunchKernelGGL(is_occluded_k, dim3((n + 255) / 256), dim3(256), 0, c->stream, view_of(c, kQuerySky, 3),
                           (vpx_ray*)in[0], n, (uint8_t*)out[0]);
    });
}

// The filter's refusals, the same for n == 0.  occlusion: the reference has no IsOccludedExcept,
// so a material range is refused there.
static int check_filter(vpx_ctx* c, const vpx_ray_filter* f, bool occlusion) {
    if (!f) return fail(c, VPX_E_INVALID, "null filter");
    if (f->flags & ~(VPX_QUERY_NO_SHAPES | VPX_QUERY_RAW_DIRECTION)) return fail(c, VPX_E_INVALID, "unknown VPX_QUERY_* flag");
    if (f->mat_lo <= f->mat_hi) {
        if (occlusion) return fail(c, VPX_E_INVALID, "vpx_is_occluded_filtered takes no material range (mat_lo > mat_hi)");
        if (f->mat_hi > 255u) return fail(c, VPX_E_INVALID, "material range above 255");
    }
    return VPX_OK;
}

int vpx_find_nearest_filtered(vpx_ctx* c, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, vpx_hit* hits) {
    VPX_GROUP_FIRST(c, vpx_find_nearest_filtered(m_, rays, n, f, hits));
    if (!c || (n && (!rays || !hits))) return fail(c, VPX_E_INVALID, "null argument");
    int rc = check_filter(c, f, false);
    if (rc) return rc;
    if ((rc = check_ready(c))) return rc;
    if (n == 0) return VPX_OK;
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}}, {{hits, sizeof(vpx_hit) * n}}, [&](void* const* in, void* const* out) {
        hipLaunchKernelGGL(find_nearest_filtered_k, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                           view_of(c, kQuerySky, 3), (vpx_ray*)in[0], n, *f, (vpx_hit*)out[0]);
    });
}

int vpx_is_occluded_filtered(vpx_ctx* c, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, uint8_t* occ) {
    VPX_GROUP_FIRST(c, vpx_is_occluded_filtered(m_, rays, n, f, occ));
    if (!c || (n && (!rays || !occ))) return fail(c, VPX_E_INVALID, "null argument");
    int rc = check_filter(c, f, true);
    if (rc) return rc;
    if ((rc = check_ready(c))) return rc;
    if (n == 0) return VPX_OK;
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}}, {{occ, n}}, [&](void* const* in, void* const* out) {
        hipLaunchKernelGGL(is_occluded_filtered_k, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                           view_of(c, kQuerySky, 3), (vpx_ray*)in[0], n, *f, (uint8_t*)out[0]);
    });
}

int vpx_find_nearest_cells(vpx_ctx* c, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, vpx_hit* hits,
                           vpx_hit_cell* cells) {
    VPX_GROUP_FIRST(c, vpx_find_nearest_cells(m_, rays, n, f, hits, cells));
    if (!c || (n && (!rays || !hits || !cells))) return fail(c, VPX_E_INVALID, "null argument");
    int rc = check_filter(c, f, false);
    if (rc) return rc;
    if ((rc = check_ready(c))) return rc;
    if (n == 0) return VPX_OK;
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}}, {{hits, sizeof(vpx_hit) * n}, {cells, sizeof(vpx_hit_cell) * n}},
                     [&](void* const* in, void* const* out) {
                         hipLaunchKernelGGL(find_nearest_cells_k, dim3((n + 255) / 256), dim3(256), 0, c->stream,
                                            view_of(c, kQuerySky, 3), (vpx_ray*)in[0], n, *f, (vpx_hit*)out[0],
                                            (vpx_hit_cell*)out[1]);
                     });
}

// The pixel entries' shared checks and frame: the filter (NULL = neutral, no raw directions: the
// library builds these rays), the size, the camera; the frame of the static-camera path's
// GetPrimaryRayNoDOF (kFlagReproject keeps the ray's arithmetic exact in both modes).
static int pixel_frame(vpx_ctx* c, uint32_t width, uint32_t height, const vpx_ray_filter* f, vpx_ray_filter& flt,
                       FrameArgs& fa) {
    flt = f ? *f : vpx_ray_filter{0u, 1u, 0u, 0u};
    int rc = check_filter(c, &flt, false);
    if (rc) return rc;
    if (flt.flags & VPX_QUERY_RAW_DIRECTION)
        return fail(c, VPX_E_INVALID, "VPX_QUERY_RAW_DIRECTION on a pixel query (the library builds the ray)");
    if (width == 0 || height == 0 || width > 32768 || height > 32768)
        return fail(c, VPX_E_INVALID, "frame size out of range");
    if (!c->have_camera) return fail(c, VPX_E_STATE, "no camera set (vpx_set_camera)");
    if ((rc = check_ready(c))) return rc;
    if (c->volumes.size() > 65533u) return fail(c, VPX_E_STATE, "more than 65533 volumes: vox_index does not fit the ID word");
    vpx_frame_params p = {};
    p.width = width, p.height = height;
    fa = frame_of(c, &p, 0, 1);
    fa.flags = kFlagReproject;
    return VPX_OK;
}

int vpx_pick_pixel(vpx_ctx* c, uint32_t width, uint32_t height, uint32_t x, uint32_t y, const vpx_ray_filter* f,
                   vpx_hit* hit, vpx_hit_cell* cell) {
    VPX_GROUP_FIRST(c, vpx_pick_pixel(m_, width, height, x, y, f, hit, cell));
    if (!c || !hit || !cell) return fail(c, VPX_E_INVALID, "null argument");
    vpx_ray_filter flt;
    FrameArgs fa;
    int rc = pixel_frame(c, width, height, f, flt, fa);
    if (rc) return rc;
    if (x >= width || y >= height) return fail(c, VPX_E_INVALID, "pixel outside the frame");
    VPX_HIP(c, hipSetDevice(c->device));
    return run_batch(c, {}, {{hit, sizeof(vpx_hit)}, {cell, sizeof(vpx_hit_cell)}}, [&](void* const*, void* const* out) {
        hipLaunchKernelGGL(pick_pixel_k, dim3(1), dim3(1), 0, c->stream, view_of(c, kQuerySky, 3), fa, flt, x, y,
                           (vpx_hit*)out[0], (vpx_hit_cell*)out[1]);
    });
}

int vpx_render_ids(vpx_ctx* c, const vpx_frame_params* p, const vpx_ray_filter* f, uint32_t* ids) {
    VPX_GROUP_FIRST(c, vpx_render_ids(m_, p, f, ids));
    if (!c || !p || !ids) return fail(c, VPX_E_INVALID, "null argument");
    vpx_ray_filter flt;
    FrameArgs fa;
    const int rc = pixel_frame(c, p->width, p->height, f, flt, fa);
    if (rc) return rc;
    VPX_HIP(c, hipSetDevice(c->device));
    hipLaunchKernelGGL(k_ids, dim3(fa.num_tiles), dim3(kThreads), 0, c->stream, view_of(c, kQuerySky, 3), fa, flt,
                       reinterpret_cast<uint4*>(ids));
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

// vpx_cast_*: the shared checks (the filter as vpx_find_nearest_cells takes it, NULL = neutral;
// the options), and which form serves the batch: the pool only where the batch visits exactly one
// volume, the scene's last.  What flags == 0 takes there was decided on incoherent rays (origins
// uniform in the world box, directions uniform on the sphere, 2^22 rays, one run, median [p5, p95]
// ms; DESIGN.md section 4, "Device ray batches"): FindNearest with cells C1 pool 1.716 [1.647,
// 1.791] vs per lane 2.186 [2.175, 2.197], C2 1.407 [1.381, 1.426] vs 2.105 [2.096, 2.130]: the
// pool; IsOccluded C1 1.693 [1.577, 1.735] vs 1.688 [1.664, 1.710], inside the spread (C2 1.366
// vs 1.612): per lane.  Rays in pixel order are the other way round (C1 0.506 vs 0.340): such a
// caller asks for VPX_CAST_PER_LANE.
constexpr bool kCastNearestDefaultPool = true, kCastOccludedDefaultPool = false;
static int cast_begin(vpx_ctx* c, uint32_t n, const vpx_ray_filter* f, const vpx_cast* opt, bool occlusion,
                      vpx_ray_filter& flt, vpx_cast& o, bool& pool) {
    c->last_cast = 0;
    if (n > (1u << 30)) return fail(c, VPX_E_INVALID, "more than 2^30 rays in one batch");
    flt = f ? *f : vpx_ray_filter{0u, 1u, 0u, 0u};
    int rc = check_filter(c, &flt, occlusion);
    if (rc) return rc;
    o = opt ? *opt : vpx_cast{0u, 0u, {0u, 0u}};
    if (o.flags & ~(VPX_CAST_PER_LANE | VPX_CAST_POOL)) return fail(c, VPX_E_INVALID, "unknown VPX_CAST_* flag");
    if ((o.flags & VPX_CAST_PER_LANE) && (o.flags & VPX_CAST_POOL))
        return fail(c, VPX_E_INVALID, "VPX_CAST_PER_LANE and VPX_CAST_POOL together");
    if (o.reserved[0] | o.reserved[1]) return fail(c, VPX_E_INVALID, "vpx_cast.reserved must be 0");
    if ((rc = check_ready(c))) return rc;
    const bool reach = (uint64_t)flt.first_volume + 1u == c->volumes.size();
    pool = reach && ((o.flags & VPX_CAST_POOL) || (o.flags == 0u && (occlusion ? kCastOccludedDefaultPool : kCastNearestDefaultPool)));
    return VPX_OK;
}
// The pool's launch: its grab block zeroed on the stream, then at most max_waves persistent waves
// (whole workgroups are launched; the last one's waves beyond the count leave at once), never more
// than the batch has grabs or the device holds at once (wpe: the kernel's waves per SIMD).
static int cast_pool_grid(vpx_ctx* c, uint32_t n, const vpx_cast& o, uint32_t wpe, uint32_t& waves, uint32_t& blocks) {
    if (!c->cast_grab) VPX_HIP(c, c->cast_grab.alloc(sizeof(uint32_t) * kGrabBlock));
    VPX_HIP(c, hipMemsetAsync(c->cast_grab, 0, sizeof(uint32_t) * kGrabBlock, c->stream));
    const uint32_t chunks = (n + kPoolChunk - 1u) / kPoolChunk, wpb = kPoolWg / 64u;
    waves = std::min(chunks, c->cus * 4u * wpe);
    if (o.max_waves) waves = std::min(waves, o.max_waves);
    blocks = (waves + wpb - 1u) / wpb;
    return VPX_OK;
}

int vpx_cast_nearest(vpx_ctx* c, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, const vpx_cast* opt,
                     vpx_hit* hits, vpx_hit_cell* cells) {
    VPX_GROUP_FIRST(c, vpx_cast_nearest(m_, rays, n, f, opt, hits, cells));
    if (!c || (n && (!rays || !hits))) return fail(c, VPX_E_INVALID, "null argument");
    vpx_ray_filter flt;
    vpx_cast o;
    bool pool = false;
    int rc = cast_begin(c, n, f, opt, false, flt, o, pool);
    if (rc) return rc;
    if (n == 0) return VPX_OK;
    VPX_HIP(c, hipSetDevice(c->device));
    const SceneView sv = view_of(c, kQuerySky, 3);
    if (pool) {
        uint32_t waves = 0, blocks = 0;
        if ((rc = cast_pool_grid(c, n, o, cells ? VPX_WPE_CAST_CELLS : VPX_WPE_CAST, waves, blocks))) return rc;
        const bool x86 = sv.x86.tab != nullptr;
        auto k = cells ? (x86 ? k_cast_pool<true, true> : k_cast_pool<false, true>)
                       : (x86 ? k_cast_pool<true, false> : k_cast_pool<false, false>);
        hipLaunchKernelGGL(k, dim3(blocks), dim3(kPoolWg), 0, c->stream, sv, rays, n, flt, c->cast_grab, waves, hits, cells);
    } else {
        hipLaunchKernelGGL(cells ? k_cast_lane<true> : k_cast_lane<false>, dim3((n + kThreads - 1) / kThreads), dim3(kThreads),
                           0, c->stream, sv, rays, n, flt, hits, cells);
    }
    VPX_HIP(c, hipGetLastError());
    c->last_cast = pool ? 2 : 1;
    return VPX_OK;
}

int vpx_cast_occluded(vpx_ctx* c, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, const vpx_cast* opt,
                      uint8_t* occ) {
    VPX_GROUP_FIRST(c, vpx_cast_occluded(m_, rays, n, f, opt, occ));
    if (!c || (n && (!rays || !occ))) return fail(c, VPX_E_INVALID, "null argument");
    vpx_ray_filter flt;
    vpx_cast o;
    bool pool = false;
    int rc = cast_begin(c, n, f, opt, true, flt, o, pool);
    if (rc) return rc;
    if (n == 0) return VPX_OK;
    VPX_HIP(c, hipSetDevice(c->device));
    const SceneView sv = view_of(c, kQuerySky, 3);
    if (pool) {
        uint32_t waves = 0, blocks = 0;
        if ((rc = cast_pool_grid(c, n, o, VPX_WPE_CAST, waves, blocks))) return rc;
        hipLaunchKernelGGL(k_cast_occluded_pool, dim3(blocks), dim3(kPoolWg), 0, c->stream, sv, rays, n, flt, c->cast_grab, waves, occ);
    } else {
        hipLaunchKernelGGL(k_cast_occluded_lane, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, c->stream, sv, rays, n,
                           flt, occ);
    }
    VPX_HIP(c, hipGetLastError());
    c->last_cast = pool ? 2 : 1;
    return VPX_OK;
}

int vpx_debug_last_cast_kernel(vpx_ctx* c) {
    if (!c) return 0;
    return c->members.empty() ? c->last_cast : c->members[0].ctx->last_cast;
}

int vpx_denoise_ids(vpx_ctx* c, const vpx_frame_params* p, const uint32_t* ids, const float* in, float* out,
                    uint32_t* rgb8, const vpx_denoise* d) {
    VPX_GROUP_FIRST(c, vpx_denoise_ids(m_, p, ids, in, out, rgb8, d));
    if (!c || !p) return fail(c, VPX_E_INVALID, "null argument");
    if (const char* why = denoise::check_call(p->width, p->height, ids, in, out, d)) return fail(c, VPX_E_INVALID, why);
    VPX_HIP(c, hipSetDevice(c->device));
    const size_t pixels = (size_t)p->width * p->height;
    uint2* keys = nullptr;
    float4* img[2] = {nullptr, nullptr};
    auto carve = [&](Carve cv) {  // the keys, then the two images of a call with several passes
        keys = cv.take<uint2>(pixels * sizeof(uint2));
        if (d->passes > 1)
            for (auto& i : img) i = cv.take<float4>(pixels * sizeof(float4));
        return cv.used();
    };
    // an earlier call may still read the old scratch: wait
    if (int rc = c->dn_buf.grow(c, carve(Carve(nullptr)), true)) return rc;
    carve(Carve(c->dn_buf));
    hipLaunchKernelGGL(k_plane_key, dim3((uint32_t)((pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                       (uint32_t)pixels, reinterpret_cast<const uint4*>(ids), keys);
    DenoiseArgs a;
    a.width = p->width, a.height = p->height, a.tiles_x = (p->width + kTile - 1) / kTile;
    a.inv_sigma = d->sigma_l > 0.0f ? 1.0f / d->sigma_l : 0.0f;
    const uint32_t tiles = a.tiles_x * ((p->height + kTile - 1) / kTile);
    const float4* src = reinterpret_cast<const float4*>(in);
    for (uint32_t k = 0; k < d->passes; ++k) {
        const bool last = k + 1 == d->passes;
        float4* dst = last ? reinterpret_cast<float4*>(out) : img[k & 1u];
        a.step = 1 << k;
        if (d->sigma_l > 0.0f)
            launch_atrous<true>(c->stream, tiles, a, keys, src, dst, last ? rgb8 : nullptr);
        else
            launch_atrous<false>(c->stream, tiles, a, keys, src, dst, last ? rgb8 : nullptr);
        src = dst;
    }
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

// The volume table of a vpx_reproject_ids call into c->rj_buf, on the stream; skipped when the
// device already holds these bytes.
static int reproject_table(vpx_ctx* c, uint32_t n, const vpx_volume* cur_volumes, const vpx_volume* prev_volumes) {
    const size_t words = (size_t)n * (reproject::kTabFloats + 1u);
    std::vector<uint32_t> t;
    try {
        t.resize(words);
    } catch (const std::bad_alloc&) {
        return fail(c, VPX_E_NOMEM, "reproject volume table");
    }
    reproject::build_table(n, cur_volumes, prev_volumes, reinterpret_cast<float*>(t.data()),
                           t.data() + (size_t)n * reproject::kTabFloats);
    if (t == c->rj_last) return VPX_OK;
    if (!c->rj_ev) VPX_HIP(c, hipEventCreateWithFlags(&c->rj_ev, hipEventDisableTiming));
    VPX_HIP(c, hipEventSynchronize(c->rj_ev));  // the staging copy's last upload (long past, as a rule)
    // no wait: rj_ev, just above, was this staging copy's only reader
    if (int rc = c->rj_host.grow(c, words * 4, false)) return rc;
    memcpy(c->rj_host, t.data(), words * 4);
    c->rj_last.clear();
    VPX_HIP(c, hipMemcpyAsync(c->rj_buf, c->rj_host, words * 4, hipMemcpyHostToDevice, c->stream));
    VPX_HIP(c, hipEventRecord(c->rj_ev, c->stream));
    c->rj_last.swap(t);
    return VPX_OK;
}

int vpx_denoise_var(vpx_ctx* c, const vpx_frame_params* p, const uint32_t* ids, const float* in, const float* mom,
                    float* out, uint32_t* rgb8, const vpx_denoise_var_params* d) {
    VPX_GROUP_FIRST(c, vpx_denoise_var(m_, p, ids, in, mom, out, rgb8, d));
    if (!c || !p) return fail(c, VPX_E_INVALID, "null argument");
    if (const char* why = denoise_var::check_call(p->width, p->height, ids, in, mom, out, d))
        return fail(c, VPX_E_INVALID, why);
    VPX_HIP(c, hipSetDevice(c->device));
    const size_t pixels = (size_t)p->width * p->height;
    uint2* keys = nullptr;
    float4* img[2] = {nullptr, nullptr};
    auto carve = [&](Carve cv) {  // the keys, V0, and the second image of a call with several passes
        keys = cv.take<uint2>(pixels * sizeof(uint2));
        img[0] = cv.take<float4>(pixels * sizeof(float4));
        if (d->passes > 1) img[1] = cv.take<float4>(pixels * sizeof(float4));
        return cv.used();
    };
    // an earlier call may still read the old scratch: wait
    if (int rc = c->dv_buf.grow(c, carve(Carve(nullptr)), true)) return rc;
    carve(Carve(c->dv_buf));
    hipLaunchKernelGGL(k_plane_key, dim3((uint32_t)((pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                       (uint32_t)pixels, reinterpret_cast<const uint4*>(ids), keys);
    DenoiseVarArgs a;
    a.width = p->width, a.height = p->height, a.tiles_x = (p->width + kTile - 1) / kTile;
    a.step = 1;
    a.sigma_v = d->sigma_v, a.epsilon = d->epsilon, a.min_history = d->min_history;
    const uint32_t tiles = a.tiles_x * ((p->height + kTile - 1) / kTile);
    const float4* src = reinterpret_cast<const float4*>(in);
    if (mom)
        hipLaunchKernelGGL(k_var_estimate<true>, dim3(tiles), dim3(kThreads), 0, c->stream, a, keys, src,
                           reinterpret_cast<const float2*>(mom), img[0]);
    else
        hipLaunchKernelGGL(k_var_estimate<false>, dim3(tiles), dim3(kThreads), 0, c->stream, a, keys, src,
                           static_cast<const float2*>(nullptr), img[0]);
    for (uint32_t k = 0; k < d->passes; ++k) {
        const bool last = k + 1 == d->passes;
        a.step = 1 << k;
        launch_atrous_var(c->stream, tiles, a, keys, img[k & 1u], last ? reinterpret_cast<float4*>(out) : img[(k + 1u) & 1u],
                          last ? src : nullptr, last ? rgb8 : nullptr);
    }
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

// vpx_reproject_ids and vpx_reproject_moments (mom_out != NULL): one body, one scratch.
static int reproject_call(vpx_ctx* c, const vpx_frame_params* p, const uint32_t* ids_cur, const uint32_t* ids_prev,
                          const float* cur, const float* hist_in, const float* mom_in, float* hist_out, float* mom_out,
                          uint32_t* rgb8, const vpx_reproject* r, const vpx_volume* cur_volumes,
                          const vpx_volume* prev_volumes);

int vpx_reproject_ids(vpx_ctx* c, const vpx_frame_params* p, const uint32_t* ids_cur, const uint32_t* ids_prev,
                      const float* cur, const float* hist_in, float* hist_out, uint32_t* rgb8, const vpx_reproject* r,
                      const vpx_volume* cur_volumes, const vpx_volume* prev_volumes) {
    VPX_GROUP_FIRST(c, vpx_reproject_ids(m_, p, ids_cur, ids_prev, cur, hist_in, hist_out, rgb8, r, cur_volumes, prev_volumes));
    if (!c || !p) return fail(c, VPX_E_INVALID, "null argument");
    if (const char* why = reproject::check_call(p->width, p->height, ids_cur, ids_prev, cur, hist_in, hist_out, r, cur_volumes,
                                                prev_volumes))
        return fail(c, VPX_E_INVALID, why);
    return reproject_call(c, p, ids_cur, ids_prev, cur, hist_in, nullptr, hist_out, nullptr, rgb8, r, cur_volumes, prev_volumes);
}

int vpx_reproject_moments(vpx_ctx* c, const vpx_frame_params* p, const uint32_t* ids_cur, const uint32_t* ids_prev,
                          const float* cur, const float* hist_in, const float* mom_in, float* hist_out, float* mom_out,
                          uint32_t* rgb8, const vpx_reproject* r, const vpx_volume* cur_volumes,
                          const vpx_volume* prev_volumes) {
    VPX_GROUP_FIRST(c, vpx_reproject_moments(m_, p, ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out, rgb8, r,
                                             cur_volumes, prev_volumes));
    if (!c || !p) return fail(c, VPX_E_INVALID, "null argument");
    if (const char* why = reproject::check_call_moments(p->width, p->height, ids_cur, ids_prev, cur, hist_in, mom_in, hist_out,
                                                        mom_out, r, cur_volumes, prev_volumes))
        return fail(c, VPX_E_INVALID, why);
    return reproject_call(c, p, ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out, rgb8, r, cur_volumes, prev_volumes);
}

static int reproject_call(vpx_ctx* c, const vpx_frame_params* p, const uint32_t* ids_cur, const uint32_t* ids_prev,
                          const float* cur, const float* hist_in, const float* mom_in, float* hist_out, float* mom_out,
                          uint32_t* rgb8, const vpx_reproject* r, const vpx_volume* cur_volumes,
                          const vpx_volume* prev_volumes) {
    VPX_HIP(c, hipSetDevice(c->device));
    const bool have_prev = ids_prev != nullptr;
    const size_t pixels = (size_t)p->width * p->height;
    const bool prekey = VPX_REPROJECT_PREKEY && have_prev;
    const float* tab = nullptr;
    uint2* keys = nullptr;
    auto carve = [&](Carve cv) {  // the volume table (at the base: reproject_table), then the optional keys
        tab = cv.take<const float>((size_t)r->n_volumes * (reproject::kTabFloats + 1u) * 4);
        if (prekey) keys = cv.take<uint2>(pixels * sizeof(uint2));
        return cv.used();
    };
    const size_t bytes = carve(Carve(nullptr));
    if (bytes > c->rj_buf.bytes) {
        c->rj_last.clear();  // the new scratch does not hold the table
        // an earlier call may still read the old scratch: wait
        if (int rc = c->rj_buf.grow(c, bytes, true)) return rc;
    }
    carve(Carve(c->rj_buf));
    const uint32_t* moved = reinterpret_cast<const uint32_t*>(tab) + (size_t)r->n_volumes * reproject::kTabFloats;
    if (r->n_volumes)
        if (int rc = reproject_table(c, r->n_volumes, cur_volumes, prev_volumes)) return rc;
    const void* prev = ids_prev;
    if (prekey) {
        hipLaunchKernelGGL(k_plane_key, dim3((uint32_t)((pixels + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream,
                           (uint32_t)pixels, reinterpret_cast<const uint4*>(ids_prev), keys);
        prev = keys;
    }
    const reproject::Args a = reproject::make_args(p->width, p->height, *r, have_prev);
    const uint32_t tiles_x = (p->width + kTile - 1) / kTile;
    const uint32_t tiles = tiles_x * ((p->height + kTile - 1) / kTile);
    const uint4* ic = reinterpret_cast<const uint4*>(ids_cur);
    const float4 *cu = reinterpret_cast<const float4*>(cur), *hi = reinterpret_cast<const float4*>(hist_in);
    float4* ho = reinterpret_cast<float4*>(hist_out);
    if (mom_out) {
        const float2* mi = reinterpret_cast<const float2*>(mom_in);
        float2* mo = reinterpret_cast<float2*>(mom_out);
        if (r->n_volumes) {
            if (rgb8)
                launch_reproject_moments<true, true>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, mi, ho, mo, rgb8, tab, moved);
            else
                launch_reproject_moments<true, false>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, mi, ho, mo, rgb8, tab, moved);
        } else {
            if (rgb8)
                launch_reproject_moments<false, true>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, mi, ho, mo, rgb8, tab, moved);
            else
                launch_reproject_moments<false, false>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, mi, ho, mo, rgb8, tab, moved);
        }
    } else if (r->n_volumes) {
        if (rgb8)
            launch_reproject<true, true>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, ho, rgb8, tab, moved);
        else
            launch_reproject<true, false>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, ho, rgb8, tab, moved);
    } else {
        if (rgb8)
            launch_reproject<false, true>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, ho, rgb8, tab, moved);
        else
            launch_reproject<false, false>(c->stream, tiles, a, tiles_x, ic, prev, cu, hi, ho, rgb8, tab, moved);
    }
    VPX_HIP(c, hipGetLastError());
    return VPX_OK;
}

// vpx_trace (probes == nullptr: trace_k, as before) and vpx_trace_probe (trace_probe_k; radiance
// may be null).
static int trace_rays(vpx_ctx* c, const vpx_ray* rays, const uint32_t* seeds, uint32_t n, int32_t depth,
                      const float sky[3], int32_t area_samples, float* radiance, vpx_ray_probe* probes) {
    if (depth < -1 || depth > kMaxLevels - 2) return fail(c, VPX_E_INVALID, "depth must be in [-1, 14]");
    if (!sky && !c->sky.px) return fail(c, VPX_E_STATE, "sky == NULL (textured sky) without vpx_set_sky");
    int rc = check_ready(c);
    if (rc) return rc;
    static const float kNoSky[3] = {0.f, 0.f, 0.f};
    if (n == 0) return VPX_OK;
    const SceneView sv = view_of(c, sky ? sky : kNoSky, area_samples, sky == nullptr);
    const dim3 g((n + 255) / 256), b(256);
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}, {seeds, 4ull * n}},
                     {{radiance, 12ull * n}, {probes, probes ? sizeof(vpx_ray_probe) * n : 0}},
                     [&](void* const* in, void* const* out) {
                         vpx_ray* dr = (vpx_ray*)in[0];
                         uint32_t* ds = (uint32_t*)in[1];
                         float* dout = (float*)out[0];
                         vpx_ray_probe* dp = (vpx_ray_probe*)out[1];
                         if (probes) {
                             float* po = radiance ? dout : nullptr;
                             if (depth <= 0)
                                 hipLaunchKernelGGL(trace_probe_k<1>, g, b, 0, c->stream, sv, dr, ds, n, depth, po, dp);
                             else if (depth <= 4)
                                 hipLaunchKernelGGL(trace_probe_k<5>, g, b, 0, c->stream, sv, dr, ds, n, depth, po, dp);
                             else
                                 hipLaunchKernelGGL(trace_probe_k<kMaxLevels>, g, b, 0, c->stream, sv, dr, ds, n, depth, po, dp);
                         } else if (depth <= 0)
                             hipLaunchKernelGGL(trace_k<1>, g, b, 0, c->stream, sv, dr, ds, n, depth, dout);
                         else if (depth <= 4)
                             hipLaunchKernelGGL(trace_k<5>, g, b, 0, c->stream, sv, dr, ds, n, depth, dout);
                         else
                             hipLaunchKernelGGL(trace_k<kMaxLevels>, g, b, 0, c->stream, sv, dr, ds, n, depth, dout);
                     });
}

int vpx_trace(vpx_ctx* c, const vpx_ray* rays, const uint32_t* seeds, uint32_t n, int32_t depth, const float sky[3],
              int32_t area_samples, float* radiance) {
    VPX_GROUP_FIRST(c, vpx_trace(m_, rays, seeds, n, depth, sky, area_samples, radiance));
    if (!c || (n && (!rays || !seeds || !radiance))) return fail(c, VPX_E_INVALID, "null argument");
    return trace_rays(c, rays, seeds, n, depth, sky, area_samples, radiance, nullptr);
}

int vpx_trace_probe(vpx_ctx* c, const vpx_ray* rays, const uint32_t* seeds, uint32_t n, int32_t depth,
                    const float sky[3], int32_t area_samples, float* radiance, vpx_ray_probe* probes) {
    VPX_GROUP_FIRST(c, vpx_trace_probe(m_, rays, seeds, n, depth, sky, area_samples, radiance, probes));
    if (!c || (n && (!rays || !seeds || !probes))) return fail(c, VPX_E_INVALID, "null argument");
    return trace_rays(c, rays, seeds, n, depth, sky, area_samples, radiance, probes);
}

int vpx_bvh_set(vpx_ctx* c, const vpx_bvh_tri* tris, uint32_t n) {
    VPX_GROUP_ALL(c, vpx_bvh_set(m_, tris, n));
    if (!c || (n && !tris)) return fail(c, VPX_E_INVALID, "null argument");
    if (n > VPX_BVH_MAX_TRIS) return fail(c, VPX_E_INVALID, "more triangles than VPX_BVH_MAX_TRIS");
    VPX_HIP(c, sync_all(c));
    c->bvh = vpx_ctx::Bvh{};
    if (!n) return VPX_OK;
    std::vector<vpx_bvh_node> nodes(2 * (size_t)n - 1);
    std::vector<uint32_t> idx(n);
    uint32_t used = 0;
    int rc = vpx_bvh_build_host(tris, n, nodes.data(), idx.data(), &used);
    if (rc) return fail(c, rc, "vpx_bvh_build_host failed");
    // the traversal pushes both children of every interior node it enters
    static_assert(VPX_BVH_MAX_DEPTH + 1 <= kBvhStack, "traversal stack: one pending sibling per level + the root");
    if (vpx_bvh_depth(nodes.data(), used) > VPX_BVH_MAX_DEPTH)
        return fail(c, VPX_E_INVALID, "BVH deeper than VPX_BVH_MAX_DEPTH (the traversal stack)");
    std::vector<uint32_t> img(used * 8u + n * 9u);
    std::memcpy(img.data(), nodes.data(), sizeof(vpx_bvh_node) * used);
    for (uint32_t k = 0; k < n; ++k) std::memcpy(&img[used * 8u + k * 9u], &tris[idx[k]], sizeof(vpx_bvh_tri));
    vpx_ctx::Bvh bvh;  // the context's only with its image and counts together
    VPX_HIP(c, bvh.img.alloc(sizeof(uint32_t) * img.size()));
    VPX_HIP(c, hipMemcpy(bvh.img, img.data(), sizeof(uint32_t) * img.size(), hipMemcpyHostToDevice));
    bvh.nodes = used, bvh.tris = n;
    c->bvh = std::move(bvh);
    return VPX_OK;
}

int vpx_bvh_intersect(vpx_ctx* c, const vpx_ray* rays, uint32_t n, float* t_out) {
    VPX_GROUP_FIRST(c, vpx_bvh_intersect(m_, rays, n, t_out));
    if (!c || (n && (!rays || !t_out))) return fail(c, VPX_E_INVALID, "null argument");
    if (!c->bvh.img) return fail(c, VPX_E_STATE, "no BVH set (vpx_bvh_set)");
    if (n == 0) return VPX_OK;
    const vpx_ctx::Bvh& bvh = c->bvh;
    const size_t lds = sizeof(uint32_t) * (bvh.nodes * 8u + bvh.tris * 9u);  // <= 51 KiB (512 triangles)
    return run_batch(c, {{rays, sizeof(vpx_ray) * n}}, {{t_out, sizeof(float) * n}}, [&](void* const* in, void* const* out) {
        hipLaunchKernelGGL(bvh_intersect_k, dim3((n + 255) / 256), dim3(256), lds, c->stream, bvh.img,
                           bvh.nodes, bvh.tris, (vpx_ray*)in[0], n, (float*)out[0]);
    });
}

int vpx_focus_distance(vpx_ctx* c, uint32_t width, uint32_t height, float* fd) {
    VPX_GROUP_FIRST(c, vpx_focus_distance(m_, width, height, fd));
    if (!c || !fd || !width || !height) return fail(c, VPX_E_INVALID, "bad argument");
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->have_camera) return fail(c, VPX_E_STATE, "no camera set");
    vpx_frame_params p{};
    p.width = width, p.height = height;
    const float sky[3] = {0, 0, 0};
    return run_batch(c, {}, {{fd, sizeof(float)}}, [&](void* const*, void* const* out) {
        hipLaunchKernelGGL(focus_k, dim3(1), dim3(1), 0, c->stream, view_of(c, sky, 3), frame_of(c, &p, 0, 1), (float*)out[0]);
    });
}

uint32_t vpx_pixel_seed(uint32_t base, uint32_t frame, uint32_t w, uint32_t h, uint32_t x, uint32_t y) {
    return pixel_seed(base, frame, w, h, x, y);
}


// ------------------------------------------------------------------ device sets
// One frame on a device set (vpx_create_multi): the 16x16 tiles are dealt round-robin to
// the members (tile t -> member t % n, as dist.py deals them to ranks), each member renders
// its tiles on its own device and stream, and the packed results are gathered to member 0
// over RCCL (grouped ncclSend / ncclRecv: n - 1 point-to-point transfers into device 0,
// each on its own xGMI link on an MI355X node) — or by device copies when the set repeats
// a device (RCCL communicators need distinct devices).  Member 0 then composites:
//   accum != NULL: float4 samples (16 B/pixel) -> vpx_composite_tiles into the caller's
//     accumulator + screen, bit-identical to vpx_render on one device;
//   accum == NULL: each member keeps the running average of ITS tiles (sharded
//     accumulator, reset by frame_index 0) and only packed RGB8 (4 B/pixel) travels ->
//     vpx_composite_rgb8 into the screen.
static int group_render(vpx_ctx* c, const vpx_frame_params* p, float* accum, uint32_t* rgb8, vpx_stats* stats) {
    DeviceGuard keep;
    if (!p) return fail(c, VPX_E_INVALID, "null params");
    if (!accum && !rgb8) return fail(c, VPX_E_INVALID, "accum or rgb8 (device pointers on the first device) required");
    const uint32_t n = (uint32_t)c->members.size();
    const uint64_t L = vpx_tiles_packed_len(p->width, p->height, kTile, kTile, n);
    if (!L) return fail(c, VPX_E_INVALID, "empty frame");
    const bool samples = accum != nullptr;
    const size_t elem = samples ? sizeof(float4) : sizeof(uint32_t);
    int rc;
    // (re)size the per-member buffers, all of them together: each waits for its member's queued
    // work (which still writes the old one), the gathered buffer for member 0's composite
    const size_t room = sizeof(float4) * L;
    bool fits = c->g_gathered.bytes >= room * n;
    for (const auto& mem : c->members) fits = fits && mem.packed.bytes >= room && mem.accum.bytes >= room;
    if (!fits) {
        for (uint32_t r = 0; r < n; ++r) {
            auto& mem = c->members[r];
            vpx_ctx* m = mem.ctx;
            VPX_HIP(c, hipSetDevice(m->device));
            if ((rc = mem.packed.grow(m, room, true)) || (rc = mem.accum.grow(m, room, true)) ||
                (r == 0 && (rc = c->g_gathered.grow(m, room * n, true))))
                return fail(c, rc, "device " + std::to_string(m->device) + ": " + m->err);
            VPX_HIP(c, hipMemsetAsync(mem.accum, 0, room, m->stream));
        }
    }
    vpx_ctx* m0 = c->members[0].ctx;
    if (stats) std::memset(stats, 0, sizeof(*stats));
    // stats: every member's counters are read BEFORE any member launches and after the whole
    // set is done, and each member's render is bracketed by events on its own stream, so
    // taking stats does not serialise the members (their launches still overlap)
    std::vector<std::array<unsigned long long, kCtrWords>> before(stats ? n : 0);
    if (stats)
        for (uint32_t r = 0; r < n; ++r) {
            vpx_ctx* m = c->members[r].ctx;
            VPX_HIP(c, hipSetDevice(m->device));
            if ((rc = snapshot_counters(m, before[r].data()))) return fail(c, rc, m->err);
        }
    // 1. every member renders its tiles (launches are asynchronous: the devices overlap)
    for (uint32_t r = 0; r < n; ++r) {
        auto& mem = c->members[r];
        vpx_ctx* m = mem.ctx;
        VPX_HIP(c, hipSetDevice(m->device));
        if (c->comms.empty())  // copy path: the previous frame's copy of this buffer is done
            VPX_HIP(c, hipStreamWaitEvent(m->stream, c->g_copied, 0));
        if (stats) VPX_HIP(c, hipEventRecord(m->ev0, m->stream));
        rc = samples ? vpx_render_tiles(m, p, kTile, kTile, r, n, mem.packed.as<float>(), nullptr)
                     : vpx_render_tiles_accum(m, p, kTile, kTile, r, n, mem.accum, mem.packed.as<uint32_t>(), nullptr);
        if (rc) return fail(c, rc, "device " + std::to_string(m->device) + ": " + m->err);
        if (stats) VPX_HIP(c, hipEventRecord(m->ev1, m->stream));
        if (c->comms.empty()) VPX_HIP(c, hipEventRecord(mem.ev, m->stream));
    }
    // 2. gather the packed buffers to member 0
    char* dst = c->g_gathered.as<char>();
    const size_t bytes = elem * L;
    if (!c->comms.empty()) {
        VPX_HIP(c, hipSetDevice(m0->device));
        VPX_HIP(c, hipMemcpyAsync(dst, c->members[0].packed, bytes, hipMemcpyDeviceToDevice, m0->stream));
        if (ncclGroupStart() != ncclSuccess) return fail(c, VPX_E_DEVICE, "ncclGroupStart");
        for (uint32_t r = 1; r < n; ++r) {
            if (ncclRecv(dst + bytes * r, bytes, ncclChar, (int)r, c->comms[0], m0->stream) != ncclSuccess ||
                ncclSend(c->members[r].packed, bytes, ncclChar, 0, c->comms[r], c->members[r].ctx->stream) != ncclSuccess) {
                (void)ncclGroupEnd();
                return fail(c, VPX_E_DEVICE, "RCCL gather");
            }
        }
        if (ncclGroupEnd() != ncclSuccess) return fail(c, VPX_E_DEVICE, "ncclGroupEnd");
    } else {
        VPX_HIP(c, hipSetDevice(m0->device));
        for (uint32_t r = 0; r < n; ++r) {
            const auto& mem = c->members[r];
            VPX_HIP(c, hipStreamWaitEvent(m0->stream, mem.ev, 0));
            VPX_HIP(c, hipMemcpyPeerAsync(dst + bytes * r, m0->device, mem.packed, mem.ctx->device, bytes, m0->stream));
        }
        VPX_HIP(c, hipEventRecord(c->g_copied, m0->stream));
    }
    // 3. member 0 composites into the caller's buffers
    rc = samples ? vpx_composite_tiles(m0, p, kTile, kTile, n, (const float*)dst, accum, rgb8)
                 : vpx_composite_rgb8(m0, p, kTile, kTile, n, (const uint32_t*)dst, rgb8);
    if (rc) return fail(c, rc, m0->err);
    if (stats) {  // kernel_ms: the slowest member's render; total_ms: member 0's start to the composite's end
        VPX_HIP(c, hipSetDevice(m0->device));
        VPX_HIP(c, hipEventRecord(m0->ev2, m0->stream));
        for (uint32_t r = 0; r < n; ++r) {
            vpx_ctx* m = c->members[r].ctx;
            VPX_HIP(c, hipSetDevice(m->device));
            unsigned long long after[kCtrWords];
            if ((rc = snapshot_counters(m, after))) return fail(c, rc, m->err);  // synchronises m's stream
            vpx_stats one;
            std::memset(&one, 0, sizeof(one));
            fill_stats(&one, before[r].data(), after);
            stats->primary_rays += one.primary_rays, stats->shadow_rays += one.shadow_rays;
            stats->bounce_rays += one.bounce_rays, stats->dda_cells += one.dda_cells;
            float ms = 0.f;
            VPX_HIP(c, hipEventElapsedTime(&ms, m->ev0, m->ev1));
            stats->kernel_ms = std::max(stats->kernel_ms, ms);
        }
        VPX_HIP(c, hipSetDevice(m0->device));
        float tot = 0.f;
        VPX_HIP(c, hipEventElapsedTime(&tot, m0->ev0, m0->ev2));
        stats->total_ms = std::max(tot, stats->kernel_ms);
    }
    return VPX_OK;
}

int vpx_create_multi(const int* devices, int ndev, vpx_ctx** out) {
    if (!out) return VPX_E_INVALID;
    *out = nullptr;
    if (!devices || ndev < 1 || ndev > 64) return VPX_E_INVALID;
    DeviceGuard keep;
    vpx_ctx* c = new (std::nothrow) vpx_ctx();
    if (!c) return VPX_E_NOMEM;
    c->device = devices[0];
    bool distinct = true;
    for (int r = 0; r < ndev; ++r) {
        for (int q = 0; q < r; ++q) distinct &= devices[q] != devices[r];
        vpx_ctx* m = nullptr;
        const int rc = vpx_create(devices[r], &m);
        if (rc) {
            vpx_destroy(c);
            return rc;
        }
        c->members.emplace_back();
        c->members.back().ctx = m;
        if (hipEventCreateWithFlags(&c->members.back().ev, hipEventDisableTiming) != hipSuccess) {
            vpx_destroy(c);
            return VPX_E_DEVICE;
        }
    }
    (void)hipSetDevice(devices[0]);
    if (hipEventCreateWithFlags(&c->g_copied, hipEventDisableTiming) != hipSuccess) {
        vpx_destroy(c);
        return VPX_E_DEVICE;
    }
    if (distinct && ndev > 1) {  // one RCCL communicator per device, all in this process
        c->comms.assign(ndev, nullptr);
        if (ncclCommInitAll(c->comms.data(), ndev, devices) != ncclSuccess) {
            c->comms.clear();
            vpx_destroy(c);
            return VPX_E_DEVICE;
        }
    }
    *out = c;
    return VPX_OK;
}

}  // extern "C"

extern "C" int vpx_profile_select(vpx_ctx* c, uint32_t stage_mask) {
    VPX_GROUP_FIRST(c, vpx_profile_select(m_, stage_mask));
    if (!c) return VPX_E_INVALID;
    c->prof_mask = stage_mask;
    return VPX_OK;
}

extern "C" int vpx_profile_enable(vpx_ctx* c, uint32_t max_launches) {
    VPX_GROUP_FIRST(c, vpx_profile_enable(m_, max_launches));
    if (!c) return VPX_E_INVALID;
    VPX_HIP(c, sync_all(c));
    for (hipEvent_t e : c->prof_ev) (void)hipEventDestroy(e);
    c->prof_ev.clear();
    c->prof_stage.clear();
    c->prof_cap = c->prof_used = 0;
    if (!max_launches) return VPX_OK;
    if (max_launches > 1u << 16) return fail(c, VPX_E_INVALID, "max_launches too large");
    c->prof_ev.resize(2 * (size_t)max_launches, nullptr);
    c->prof_stage.resize(2 * (size_t)max_launches, -1);
    for (auto& e : c->prof_ev) VPX_HIP(c, hipEventCreate(&e));
    c->prof_cap = 2 * max_launches;
    return VPX_OK;
}

// Length of the union of [first, second) intervals (any sign), overlaps counted once.
static float interval_union_ms(std::vector<std::pair<float, float>>& iv) {
    if (iv.empty()) return 0.f;
    std::sort(iv.begin(), iv.end());
    float busy = 0.f, lo = iv[0].first, hi = iv[0].second;
    for (const auto& v : iv) {
        if (v.first > hi) {
            busy += hi - lo;
            lo = v.first, hi = v.second;
        } else if (v.second > hi) {
            hi = v.second;
        }
    }
    return busy + (hi - lo);
}

// Host check of the union (tests/test_abi.py): n intervals as (start, end) pairs.
extern "C" float vpx_profile_busy_union(const float* se, uint32_t n) {
    std::vector<std::pair<float, float>> iv;
    for (uint32_t i = 0; i < n; ++i) iv.emplace_back(se[2 * i], se[2 * i + 1]);
    return interval_union_ms(iv);
}

extern "C" int vpx_profile_read(vpx_ctx* c, vpx_profile* out, int reset) {
    VPX_GROUP_FIRST(c, vpx_profile_read(m_, out, reset));
    if (!c || !out) return fail(c, VPX_E_INVALID, "null argument");
    std::memset(out, 0, sizeof(*out));
    unsigned long long now[kCtrWords];
    int rc = snapshot_counters(c, now);  // synchronises the stream
    if (rc) return rc;
    for (uint32_t st = 0; st < 8; ++st) out->stage_cells[st] = now[8 + st];
    std::vector<std::pair<float, float>> iv[8];  // per stage: launch intervals, ms after the first event
    for (uint32_t i = 0; i + 1 < c->prof_used; i += 2) {
        float ms = 0.f, t0 = 0.f;
        VPX_HIP(c, hipEventElapsedTime(&ms, c->prof_ev[i], c->prof_ev[i + 1]));
        VPX_HIP(c, hipEventElapsedTime(&t0, c->prof_ev[0], c->prof_ev[i]));
        const int st = c->prof_stage[i];
        if (st >= 0 && st < 8) {
            out->stage_ms[st] += ms;
            ++out->stage_launches[st];
            iv[st].emplace_back(t0, t0 + ms);
        }
    }
    // busy time: the union of the intervals.  Offsets are measured from prof_ev[0], which may
    // sit on another lane's stream, so a launch can start before it (a negative offset): the
    // union starts from the first sorted interval, not from a sentinel at 0.
    for (uint32_t st = 0; st < 8; ++st) out->stage_busy_ms[st] = interval_union_ms(iv[st]);
    if (reset) {
        c->prof_used = 0;
        unsigned long long* d = c->d_ctr;
        std::vector<unsigned long long> h(kCtrWords * kCtrStripes);
        VPX_HIP(c, hipMemcpy(h.data(), d, sizeof(unsigned long long) * h.size(), hipMemcpyDeviceToHost));
        for (uint32_t s = 0; s < kCtrStripes; ++s)
            for (uint32_t st = 8; st < 16; ++st) h[kCtrWords * s + st] = 0;
        VPX_HIP(c, hipMemcpy(d, h.data(), sizeof(unsigned long long) * h.size(), hipMemcpyHostToDevice));
    }
    return VPX_OK;
}

int vpx_debug_last_frame_kernel(vpx_ctx* c) {
    VPX_GROUP_FIRST(c, vpx_debug_last_frame_kernel(m_));
    return c ? c->last_frame_kernel : VPX_E_INVALID;
}

uint64_t vpx_debug_live_buffers(void) { return g_live_buffers.load(); }

#ifdef VPX_PHASE_PROF
// out: 48 words: g_phase, then the frame kernel's phases (g_frame_phase summed over its stripes)
extern "C" int vpx_debug_phase(unsigned long long* out, int reset) {
    static unsigned long long fp[vpx::kFrameStripes][16];
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(vpx::g_phase), sizeof(unsigned long long) * 32) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(fp, HIP_SYMBOL(vpx::g_frame_phase), sizeof(fp)) != hipSuccess) return -1;
    for (int k = 0; k < 16; ++k) {
        out[32 + k] = 0;
        for (int s = 0; s < vpx::kFrameStripes; ++s) out[32 + k] += fp[s][k];
    }
    if (reset) {
        const unsigned long long z[32] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(vpx::g_phase), z, sizeof(z)) != hipSuccess) return -1;
        std::memset(fp, 0, sizeof(fp));
        if (hipMemcpyToSymbol(HIP_SYMBOL(vpx::g_frame_phase), fp, sizeof(fp)) != hipSuccess) return -1;
    }
    return 0;
}
#endif
