/*
 * vpx.h — C-ABI of the MI355X (gfx950) voxel ray-trace library `libvpx_hip.so`.
 *
 * This is the drop-in boundary behind `Renderer::Tick(deltaTime)` of
 * Tycro-Games/Raytracer-VoxPopuli.  The host keeps its tmpl8 template, window,
 * UI and game logic; inside `Renderer::Update()` it calls `vpx_render` instead
 * of the per-pixel `Trace` loop (reference renderer.cpp:1646-1891), and the
 * library owns persistent device copies of the voxel grids, the volume
 * transforms and the material / light tables.
 *
 * Every function returns VPX_OK (0) or a negative VPX_E_* status; nothing
 * throws across the ABI and nothing aborts.  `vpx_last_error(ctx)` returns a
 * human-readable message for the last failure on that context.
 *
 * All structs are plain-old-data with fixed layout (asserted in vpx_api.cpp);
 * matrices are tmpl8 `mat4::cell` order (row-major, translation in cells 3/7/11).
 *
 * Reference interfaces replaced (file:line in the reference tree):
 *   vpx_create[_multi]    Renderer::Init (device side) renderer.cpp:688-736
 *   vpx_render            Renderer::Update            renderer.cpp:1646-1891
 *                         (+ Renderer::Trace           renderer.cpp:1076-1328)
 *   vpx_find_nearest      Renderer::FindNearest       renderer.cpp:946-1018
 *                         Scene::FindNearest          template/scene.cpp:751-811
 *   vpx_is_occluded       Renderer::IsOccluded        renderer.cpp:209-243
 *                         Scene::IsOccluded           template/scene.cpp:1009-1047
 *   vpx_trace             Renderer::Trace(Ray&, int)  renderer.cpp:1076
 *   vpx_focus_distance    focus ray in Renderer::Tick renderer.cpp:1987-1991
 *   vpx_find_nearest_filtered  Renderer::FindNearestPlayer  renderer.cpp:1020-1071 (Tick :2139-2152)
 *                              Scene::FindNearestExcept     template/scene.cpp:813-873
 *   vpx_is_occluded_filtered   Renderer::IsOccludedPlayerClimbable  renderer.cpp:245-273
 *   vpx_find_nearest_cells / vpx_pick_pixel / vpx_render_ids   no reference counterpart; the cell of
 *                              Scene::FindNearest's return, template/scene.cpp:751-811
 *   vpx_cast_nearest / vpx_cast_occluded / vpx_debug_last_cast_kernel   no reference counterpart; the
 *                              records of Renderer::FindNearest / IsOccluded per ray, on device memory
 *   vpx_reproject_ids / vpx_reproject_ids_host   no reference counterpart; temporal accumulation
 *                              under camera motion, its rejection test the vpx_render_ids record
 *                              (Camera::PointToUV template/camera.h:34-49, TransformPosition tmpl8math.cpp:345-353)
 *   vpx_reproject_moments / vpx_denoise_var (+ _host)   no reference counterpart; the luminance's first
 *                              two moments through the reprojection, and the a-trous filter with a
 *                              per-pixel tolerance from their variance
 *   vpx_get_player_light  Renderer::inLight           renderer.h:231; set renderer.cpp:1228-1240,
 *                                                     1438-1450; read :2112-2118, cleared :2206
 *   vpx_trace_probe       Trace's smoke-branch probe  renderer.cpp:1228-1240 (per ray)
 *   vpx_upload_grid       Scene::grid (owned by host) template/scene.h:258
 *   vpx_model_upload      ogt_vox models[0]->voxel_data  template/scene.cpp:474 (kept on the device)
 *   vpx_grid_load_model   Scene::LoadModel               template/scene.cpp:449-529
 *                         Scene::LoadModelPartial        template/scene.cpp:531-604
 *                           (ModifyingProp::Update, src/Game/ModifyingProp.cpp:11-21)
 *                         Scene::LoadModelRandomMaterials template/scene.cpp:606-683
 *                           (renderer.cpp:628, 2190)
 *   vpx_grid_generate_noise  Scene::GenerateSomeNoise    template/scene.cpp:226-282 (renderer.cpp:2883-2898)
 *                            Scene::GenerateSomeSmoke    template/scene.cpp:285-356 (renderer.cpp:626, 2174)
 *   vpx_grid_brush        Scene::Set over a sphere / box   template/scene.h (Set), edits of a few voxels
 *   vpx_grid_stamp        Scene::Set over an oriented model  template/scene.h (Set); a prop put into, dug
 *                                                          out of or moved within a world that holds content
 *   vpx_model_capture / vpx_model_read   no reference counterpart; a box of a grid as a resident model
 *   vpx_grid_read_box     Scene::grid read back (debug)  template/scene.h:258
 *   vpx_set_volumes       Renderer::voxelVolumes      renderer.h:211
 *   vpx_set_materials     Renderer::materials         renderer.h:190, MaterialSetUp renderer.cpp:357-443
 *   vpx_set_lights        point/spot/area/dirLight    renderer.h:193-197
 *   vpx_set_shapes        Renderer::spheres/triangles renderer.h:207-208
 *   vpx_set_camera        Renderer::camera            renderer.h:181, template/camera.h:14-192
 *   vpx_set_sky           Renderer::skyPixels (+ SampleSky) renderer.cpp:691, 2308-2326
 *   vpx_bvh_set           Renderer::bvh (BasicBVH)    renderer.h:220, src/BVH/BasicBVH.cpp:72-136
 *   vpx_bvh_intersect     BasicBVH::IntersectBVH      src/BVH/BasicBVH.cpp:19-70
 * Host-side helpers that restate reference host code (no GPU needed):
 *   vpx_camera_look_at       Camera::HandleInput basis   template/camera.h:113-181
 *   vpx_volume_set_transform Scene::SetTransform         template/scene.cpp:373-405
 *   vpx_default_materials    Renderer::MaterialSetUp     renderer.cpp:357-443
 *   vpx_bvh_build_host       BasicBVH::BuildBVH          src/BVH/BasicBVH.cpp:72-136
 *   vpx_bvh_random_tris      BasicBVH::BasicBVH()        src/BVH/BasicBVH.cpp:4-16
 *   vpx_bvh_depth            (recursion depth of IntersectBVH, src/BVH/BasicBVH.cpp:47-61)
 *   vpx_vox_decode           ogt_vox_read_scene ->models[0], ->palette, template/scene.cpp:474-475
 *   vpx_model_place_host     the three loaders' placement loop  template/scene.cpp:449-683
 *   vpx_xorshift32_jump      RandomUInt, k steps at once        template/tmpl8math.cpp:119-125
 *   vpx_model_palette_materials  LoadModel's palette override   template/scene.cpp:516-520
 *   vpx_noise_generate_host  the two generators' loops          template/scene.cpp:226-356
 *   vpx_perlin3              the noise field (this project's definition, DESIGN parity decision 9)
 *   vpx_brush_apply_host     vpx_grid_brush's cells on a host grid
 *   vpx_stamp_apply_host     vpx_grid_stamp's cells on a host grid
 */
#ifndef VPX_H_
#define VPX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VPX_ABI_VERSION 2  /* 1 -> 2: vpx_profile grew to 160 bytes (stage_busy_ms); packed tiles hold 8x8 quadrants */

/* ---- status codes ---------------------------------------------------------------- */
#define VPX_OK 0
#define VPX_E_INVALID (-1)   /* bad argument (null pointer, size, id)           */
#define VPX_E_DEVICE (-2)    /* HIP runtime error                              */
#define VPX_E_NOMEM (-3)     /* device allocation failed                       */
#define VPX_E_STATE (-4)     /* call order (e.g. render before any volume)     */

/* ---- material indices (MaterialType::MatType, template/scene.h:36-58) ------------- */
#define VPX_MAT_NON_METAL_WHITE 0
#define VPX_MAT_NON_METAL_PINK 4
#define VPX_MAT_METAL_HIGH 5
#define VPX_MAT_METAL_LOW 7
#define VPX_MAT_GLASS 8
#define VPX_MAT_SMOKE_LOW_DENSITY 9
#define VPX_MAT_SMOKE_PLAYER 14
#define VPX_MAT_EMISSIVE 15
#define VPX_MAT_NONE 255
#define VPX_NUM_MATERIALS 256

/* ---- frame flags -------------------------------------------------------------------- */
#define VPX_FLAG_AA 0x1u        /* sub-pixel jitter x+RandomFloat()*aa (renderer.cpp:1682-1708)   */
#define VPX_FLAG_DOF 0x2u       /* thin-lens jitter (template/camera.h:68-83)                    */
#define VPX_FLAG_NO_TONEMAP 0x4u /* skip accumulate/tonemap: write raw radiance to accum (tests) */
#define VPX_FLAG_SKY 0x8u       /* activateSky: misses sample the vpx_set_sky texture (renderer.cpp:2308-2326) */

/* ---- POD scene description -------------------------------------------------------- */

/* One voxel volume (a `Scene` in the reference, template/scene.h:173-266). */
typedef struct vpx_volume {
    uint32_t grid_id;       /* grid uploaded with vpx_upload_grid; volumes may share a grid */
    uint32_t reserved;
    float matrix[16];       /* Scene::matrix    (object -> world)                */
    float inv_matrix[16];   /* Scene::invMatrix (world -> object) — used as-is    */
    float b0[3];            /* Scene::cube.b[0]                                  */
    float b1[3];            /* Scene::cube.b[1]                                  */
} vpx_volume;               /* 160 bytes */

/* Material (src/Materials/Material.h:3-12), indexed by voxel value. */
typedef struct vpx_material {
    float albedo[3];
    float roughness;
    float emissive;         /* emissiveStrength */
    float ior;              /* IOR */
    float pad[2];
} vpx_material;             /* 32 bytes */

typedef struct vpx_point_light {  /* PointLightData, src/Lighting/PointLight.h:3-7 */
    float position[3];
    float color[3];
} vpx_point_light;

typedef struct vpx_spot_light {   /* SpotLightData, src/Lighting/SpotLight.h:12-18 */
    float position[3];
    float direction[3];
    float color[3];
    float angle;                  /* cosine of the cone half-angle */
} vpx_spot_light;

typedef struct vpx_area_light {   /* SphereAreaLightData, src/Lighting/SphereAreaLight.h:2-9 */
    float position[3];
    float color[3];
    float color_multiplier;
    float radius;
} vpx_area_light;

typedef struct vpx_dir_light {    /* DirectionalLightData, src/Lighting/DirectionalLight.h:2-6 */
    float direction[3];
    float color[3];
} vpx_dir_light;

typedef struct vpx_sphere {       /* Sphere, src/BVH/Shapes.h:4-68 */
    float center[3];
    float radius;
    uint32_t material;
    uint32_t pad[3];
} vpx_sphere;

typedef struct vpx_triangle {     /* Triangle, src/BVH/Shapes.h:71-150 */
    float position[3];
    float v0[3], v1[3], v2[3];
    uint32_t material;
    uint32_t pad[3];
} vpx_triangle;

/* Camera state used by primary-ray generation (template/camera.h:68-110, 183-191). */
typedef struct vpx_camera {
    float cam_pos[3];
    float top_left[3];
    float top_right[3];
    float bottom_left[3];
    float right[3];
    float up[3];
    float focal_distance;
    float defocus_jitter;
} vpx_camera;

/* Per-frame parameters (the knobs of Renderer::Update / Trace). */
typedef struct vpx_frame_params {
    uint32_t width, height;       /* SCRWIDTH/SCRHEIGHT (compile-time in the reference);    */
                                  /* each <= 32768, 16x16-tile-padded W*H <= 2^27           */
    int32_t max_bounces;          /* depth handed to Trace (Renderer::maxBounces)           */
    uint32_t frame_index;         /* numRenderedFrames: weight 1/(n+1) and seed stream      */
    uint32_t seed_base;           /* added to the pixel key of the per-pixel seed           */
    uint32_t flags;               /* VPX_FLAG_*                                             */
    float aa_strength;            /* antiAliasingStrength                                   */
    int32_t area_samples;         /* numCheckShadowsAreaLight                               */
    float sky[3];                 /* SampleSky colour when activateSky == false             */
    uint32_t reserved;
} vpx_frame_params;

/* Ray for the unit entries (a `Ray` built with Ray(origin, direction), scene.cpp:83-93). */
typedef struct vpx_ray {
    float origin[3];
    float direction[3];           /* normalised by the library exactly like the Ray ctor   */
    float tmax;                   /* Ray::t on entry (1e34 = unbounded)                     */
    uint32_t inside_glass;        /* Ray::isInsideGlass                                     */
} vpx_ray;

typedef struct vpx_hit {
    float t;                      /* Ray::t after the call                                  */
    float normal[3];              /* Ray::rayNormal                                         */
    int32_t vox_index;            /* Renderer::FindNearest return: -2 none, -1 analytic, i  */
    uint32_t material;            /* Ray::indexMaterial (255 = NONE)                        */
    uint32_t cells;               /* DDA cells read for this ray                            */
    uint32_t inside_glass;        /* Ray::isInsideGlass after the call                      */
} vpx_hit;

/* Work counters of one render call (always on; per-wave reduced on device). */
typedef struct vpx_stats {
    uint64_t primary_rays;        /* W*H                                                     */
    uint64_t shadow_rays;         /* IsOccluded calls actually made                          */
    uint64_t bounce_rays;         /* FindNearest calls beyond the primary                    */
    uint64_t dda_cells;           /* grid cells read by every DDA (nearest + shadow + exits) */
    float kernel_ms;              /* device time of the trace kernel (HIP events)            */
    float total_ms;               /* device time of the whole call                           */
} vpx_stats;

typedef struct vpx_ctx vpx_ctx;

/* ---- lifetime ------------------------------------------------------------------------ */
int vpx_create(int device, vpx_ctx** out);
/* A device set for a single-process host (the tmpl8 Renderer::Tick on a multi-GPU node):
   one member context per entry of devices[0..ndev) (the world and tables are uploaded to
   every member by the same calls as for one device).  vpx_render deals the 16x16 tiles
   round-robin to the members, renders them concurrently, gathers the packed results to
   devices[0] over RCCL (one communicator per device, ncclCommInitAll; device copies when
   the set repeats a device) and composites there: with accum != NULL the float4 samples
   travel and accum / rgb8 (devices[0] pointers) are bit-identical to vpx_render on one
   device; with accum == NULL each member keeps the running average of its own tiles and
   only RGB8 travels into rgb8.  vpx_set_stream sets devices[0]'s stream; unit entries,
   profiles, vpx_render_reproject and the rank-level entries (vpx_render_tiles*,
   vpx_composite_*) run on devices[0]; vpx_get_counters sums the members.  Every call on a
   set restores the caller's current HIP device before it returns; stats (vpx_render) read
   the members' counters outside the launches, so the members still overlap.
   Verification status: sets that repeat a device (the device-copy gather) are tested bit
   for bit on one GPU; the distinct-device RCCL gather has its test
   (test_device_set_equals_single_device[devices3]) but runs only on a node with >= 2 GPUs
   and has not yet executed on hardware. */
int vpx_create_multi(const int* devices, int ndev, vpx_ctx** out);
int vpx_destroy(vpx_ctx* ctx);
const char* vpx_last_error(const vpx_ctx* ctx);
int vpx_abi_version(void);
/* Use an external HIP stream (hipStream_t as void*); NULL = the context's own stream. */
int vpx_set_stream(vpx_ctx* ctx, void* hip_stream);
int vpx_synchronize(vpx_ctx* ctx);
/* Frames in flight (depth 2..4; 0 / 1 = off, the default).  With depth D, vpx_render and
   vpx_render_tiles_accum render each frame on the next of D library-owned streams ("lanes",
   each with its own path-state buffers and its own hardware queue — CU-mask streams, outside
   the GPU_MAX_HW_QUEUES pool the caller's streams share) into packed float4 samples, and queue only the
   frame's accumulate / tonemap / RGB8 pack (or the rank's packed running average) on the
   context's stream, after the previous frame's: frame f+1's walks run while frame f's last
   tiles drain.  Results are bit-identical (the same blend of the same sample, in frame order);
   accum / rgb8 are complete when the context's stream is.  Renders that take stats, the
   static-camera path, VPX_FLAG_NO_TONEMAP frames and vpx_render_tiles (samples into the
   caller's buffer) run on the stream as without lanes.
   World / table updates wait for the frames in flight.  No reference counterpart: the
   reference renders one frame per Tick (renderer.cpp:1646-1891).
   Queues and ordering: each lane takes a hardware queue of its own (D per context, and per
   member of a device set), up to 16 such lanes per process; lanes past that cap are plain
   non-blocking streams from the process's shared queue pool.  Frames with bounce levels also
   take one more such queue per path state (the context's own, and each lane's when at most two
   lanes run a single-volume scene): the level fork, a second stream that runs a level's
   bounce walks beside its shadow walks and joins back within the frame.  Dedicated-queue lanes are
   blocking streams: they synchronise with the legacy null stream (hipStreamLegacy / torch's
   default stream), so work the caller queues there serialises with the frames in flight —
   render on a created stream (vpx_set_stream) to keep them overlapped. */
int vpx_set_pipeline(vpx_ctx* ctx, uint32_t depth);

/* ---- world ----------------------------------------------------------------------------- */
/* Upload a dense N^3 grid of MatType bytes, index x + y*N + z*N*N (scene.h:241-248).
   Device memory per grid: N^3 bytes + the walkers' levels built from them, about N^3 / 4
   bytes (l1 cell masks N^3/8, distance-field octant planes N^3/8, l2 N^3/512), and the
   distance field's 24 axis planes of 32-bit words, 96 bytes per 4^3 brick where the octant
   planes take 8: 3 N^3 / 2 bytes, 1.5 GiB at N = 1024 and 12 GiB at 2048.  In all 2.75 GiB
   at N = 1024, 22 GiB at 2048, 176 GiB at 4096 (the maximum).  An allocation that fails returns
   VPX_E_NOMEM. */
int vpx_upload_grid(vpx_ctx* ctx, uint32_t grid_id, const uint8_t* cells, uint32_t n);
/* Build-defined world generator on device: a grid-oriented model
   (mx*my*mz bytes, index x + y*mx + z*mx*my) tiled with period (px,py,pz) above a
   NON_METAL_WHITE ground slab of `ground` cells.  Same result as oracle_tiled_world. */
int vpx_generate_tiled_grid(vpx_ctx* ctx, uint32_t grid_id, uint32_t n, const uint8_t* model,
                            uint32_t mx, uint32_t my, uint32_t mz,
                            uint32_t px, uint32_t py, uint32_t pz, uint32_t ground);
/* In-place world edits.  Each refreshes the occupancy levels
   of the touched bricks only.
   Scene::ResetGrid(type) (template/scene.cpp:356-359): every cell = value. */
int vpx_grid_fill(vpx_ctx* ctx, uint32_t grid_id, uint8_t value);
/* Dirty-region upload: a box of cells, host bytes x fastest (src[x + y*dx + z*dx*dy]),
   written at (x0, y0, z0) — what Scene::Set-based edits change (LoadModelPartial from
   ModifyingProp::Update, src/Game/ModifyingProp.cpp:11-21; zone changes). */
int vpx_grid_write_box(vpx_ctx* ctx, uint32_t grid_id, const uint8_t* src, uint32_t x0, uint32_t y0,
                       uint32_t z0, uint32_t dx, uint32_t dy, uint32_t dz);
/* Scene::CreateEmmisiveSphere(mat, radius) (template/scene.cpp:685-711) on the device:
   cells with length(worldsize/2 - (x,y,z)) < radius get `mat` (others unchanged). */
int vpx_grid_emissive_sphere(vpx_ctx* ctx, uint32_t grid_id, uint8_t mat, float radius);
/* Resident models: ogt_vox's models[0]->voxel_data as vpx_vox_decode returns it
   (index x + y*sx + z*sx*sy, 0 = empty), each dimension 1..256.  voxels == NULL removes the
   model.  A device set keeps a copy on every member. */
int vpx_model_upload(vpx_ctx* ctx, uint32_t model_id, const uint8_t* voxels,
                     uint32_t sx, uint32_t sy, uint32_t sz);

#define VPX_LOAD_FULL    0u  /* Scene::LoadModel placement            scene.cpp:449-529 */
#define VPX_LOAD_PARTIAL 1u  /* Scene::LoadModelPartial               scene.cpp:531-604 */
#define VPX_LOAD_RANDOM  2u  /* Scene::LoadModelRandomMaterials       scene.cpp:606-683 */
typedef struct vpx_model_load {      /* 40 bytes */
    float    scale_model[3];         /* Scene::scaleModel on entry */
    uint32_t mode;                   /* VPX_LOAD_* */
    uint32_t columns, thickness;     /* PARTIAL: keep model x in [columns - thickness, columns + thickness],
                                        uint32 arithmetic as written (the lower bound wraps) */
    uint32_t seed;                   /* RANDOM: the caller's xorshift32 state (tmpl8math.cpp:16) */
    float    rand_lo, rand_hi;       /* RANDOM: Rand(rand_lo, rand_hi); the reference passes 12, 13 */
    uint32_t reserved;               /* 0 */
} vpx_model_load;
typedef struct vpx_model_result {    /* 16 bytes */
    float    scale_model[3];         /* Scene::scaleModel as the call leaves it */
    uint32_t seed;                   /* RANDOM: state after sx*sy*sz draws; else the seed given */
} vpx_model_result;
/* ResetGrid() to NONE, then the placement, on the device: no host grid, one level rebuild.
   Creates the grid (or resizes it), like vpx_generate_tiled_grid: a fresh Scene(position, n)
   needs no host upload.  The result is the grid the reference's loop leaves, bit for bit:
     - when sx > n, scale_model is multiplied by (float)n / (float)size per axis — on every
       call, as the reference does, so `out->scale_model` carries the multiplied value and a
       host that mirrors Scene::scaleModel feeds it back;
     - voxel (x, y, z) goes to the cell (trunc(x * s.x), trunc(z * s.y), trunc(y * s.z)), y and z
       swapped; a NaN or an overflowing product truncates to INT_MIN as on x86;
     - empty voxels and targets outside [0, n) are skipped (the reference's Set does not check);
     - where several voxels land in one cell the last one of the loop (z outer, y, x inner) stays,
       whatever order the device works in;
     - RANDOM: voxel i = x + y*sx + z*sx*sy draws u_i, the state after i + 1 steps from `seed`
       (empty voxels draw too, scene.cpp:661), and a non-empty one writes
       (uint8_t)(rand_lo + (float)u_i * 2.3283064365387e-10f * (rand_hi - rand_lo)).
   VPX_E_INVALID: in == NULL, reserved != 0, unknown mode, unknown model_id, n outside
   vpx_upload_grid's range, RANDOM with a range not in 0 <= rand_lo <= rand_hi <= 255 (NaN
   included).  Like every world edit the call waits for the frames in flight. */
int vpx_grid_load_model(vpx_ctx* ctx, uint32_t grid_id, uint32_t n, uint32_t model_id,
                        const vpx_model_load* in, vpx_model_result* out /* may be NULL */);

#define VPX_GEN_NOISE 0u   /* Scene::GenerateSomeNoise  scene.cpp:226-282 */
#define VPX_GEN_SMOKE 1u   /* Scene::GenerateSomeSmoke  scene.cpp:285-356 */
typedef struct vpx_noise_gen {       /* 16 bytes */
    uint32_t mode;                   /* VPX_GEN_* */
    float    frequency;              /* the generators' argument (0.167f at renderer.cpp:626, 2174) */
    uint32_t seed;                   /* the caller's xorshift32 state (tmpl8math.cpp:16) */
    uint32_t reserved;               /* 0 */
} vpx_noise_gen;
typedef struct vpx_noise_result {    /* 16 bytes */
    uint32_t seed;                   /* the state the reference's thread-local seed is left in */
    uint32_t noise_seed;             /* the call's first RandomUInt(), the field's seed */
    uint64_t draws;                  /* every RandomUInt() of the call, the noise seed included */
} vpx_noise_result;
/* ResetGrid(), then Scene::GenerateSomeNoise or GenerateSomeSmoke on the device: no host grid,
   no host noise library, one level rebuild.  Creates the grid (or resizes it) like
   vpx_grid_load_model.  Every cell is written exactly once:
     - the field: cell (x, y, z) samples vpx_perlin3((int32_t)noise_seed, x*f, y*f, z*f), all
       float32; FastNoise2 is a binary in the reference, so the noise VALUES are this project's
       definition (csrc/vpx_noise.hpp) while positions, thresholds and RNG order are the
       reference's;
     - NOISE: the chain of scene.cpp:250-275 as written — n <= 0.04f NONE; (double)n < 0.08 draws
       (uint8_t)(RandomFloat() * 8.0f), 0..8; (double)n < 0.2 NON_METAL_RED; n < 0.17f is dead;
       (double)n < 0.3 EMISSIVE; n < 0.5f METAL_HIGH; n < 0.7f METAL_MID; n < 0.9f METAL_LOW;
       otherwise (NaN included) NONE.  The k-th drawing cell in loop order (z outer, y, x inner),
       0-based, uses the state after 2 + k steps from `seed`;
     - SMOKE: cell i = x + y*n + z*n*n draws randomX and randomZ from the states after 2 + 2i and
       3 + 2i steps; the ellipsoid test and the five densities are scene.cpp:306-349.
   VPX_E_INVALID: in == NULL, reserved != 0, unknown mode, n outside vpx_upload_grid's range, a
   non-finite frequency, (n - 1) * |frequency| >= 2^30 (the float-to-int conversion of a lattice
   coordinate stays in range below that).  VPX_E_NOMEM when the per-call prefix buffer cannot
   be had.  Like every world edit the call waits for the frames in flight. */
int vpx_grid_generate_noise(vpx_ctx* ctx, uint32_t grid_id, uint32_t n, const vpx_noise_gen* in,
                            vpx_noise_result* out /* may be NULL */);
#define VPX_BRUSH_SPHERE 0u  /* cells with dx*dx + dy*dy + dz*dz <= r2 (int64), d = cell - center */
#define VPX_BRUSH_BOX    1u  /* cells with lo <= cell <= hi per axis */
typedef struct vpx_brush {           /* 48 bytes */
    uint32_t shape;                  /* VPX_BRUSH_* */
    int32_t  center[3];              /* SPHERE; may lie outside the grid */
    uint32_t r2;                     /* SPHERE: squared radius in cells */
    int32_t  lo[3], hi[3];           /* BOX, inclusive; clipped to the grid; lo > hi on an axis: empty */
    uint8_t  value;                  /* byte written; 255 (NONE) digs */
    uint8_t  match_lo, match_hi;     /* only cells whose current byte m has match_lo <= m <= match_hi are
                                        written: 0..255 all, 255..255 place into empty cells only,
                                        0..254 repaint solid only */
    uint8_t  reserved;               /* 0 */
} vpx_brush;
typedef struct vpx_brush_result {    /* 16 bytes */
    uint64_t changed;                /* cells whose byte changed, over all brushes of the call */
    uint32_t flipped;                /* 4^3 bricks whose emptiness changed (0: no distance-field work was needed) */
    uint32_t reserved;
} vpx_brush_result;
/* Device-side edit: `count` (1..256) brushes applied in order, one launch each over the brush's
   clipped bounding box, so a later brush's filter sees the bytes an earlier one left; all
   arithmetic is integer.  Then ONE region-local refresh of the occupancy levels and the distance
   field for the whole call (DESIGN §4 "Brush edits"): the cell masks of the touched bricks, and
   when a brick's emptiness flipped, only the distance-field bytes, lengths and widths that the
   flipped bricks can reach — the words a full rebuild would leave, bit for bit.  The call
   allocates nothing (its few hundred bytes of scratch come with the context's first brush call).
   VPX_E_INVALID: brushes == NULL, count outside 1..256, unknown shape, reserved != 0,
   match_lo > match_hi, unknown grid.  Like every world edit the call waits for the frames in
   flight; a device set applies it to every member.  Which cell a ray or a pixel points at comes
   from vpx_find_nearest_cells / vpx_pick_pixel; which ray to cast and what to do with the cell
   is the host's business. */
int vpx_grid_brush(vpx_ctx* ctx, uint32_t grid_id, const vpx_brush* brushes, uint32_t count,
                   vpx_brush_result* out /* may be NULL */);
/* The same brushes on a host grid of n^3 bytes (host only, the code the device runs);
   `flipped` from the host level builder before and after.  VPX_E_INVALID as above, and for
   cells == NULL or n outside vpx_upload_grid's range. */
int vpx_brush_apply_host(uint8_t* cells, uint32_t n, const vpx_brush* brushes, uint32_t count,
                         vpx_brush_result* out /* may be NULL */);

#define VPX_STAMP_GRID_BYTES 0x1u  /* model bytes are grid bytes: 255 is empty, 0 is a material
                                      (what vpx_model_capture stores).  Default: 0 is empty and
                                      byte k writes k, vpx_grid_load_model's convention */
#define VPX_STAMP_CONSTANT   0x2u  /* non-empty voxels write `value` instead of their own byte;
                                      value 255 digs the model's shape out */
/* orient: which model axis feeds each grid axis, and mirrored or not.
   bits 0-1 / 2-3 / 4-5: model axis (0 = x, 1 = y, 2 = z) of grid x / y / z, a permutation;
   bits 8 / 9 / 10: grid x / y / z runs against that model axis.  All other bits 0. */
#define VPX_ORIENT_IDENTITY   0x24u /* x<-x, y<-y, z<-z */
#define VPX_ORIENT_LOAD_MODEL 0x18u /* x<-x, y<-z, z<-y: Scene::LoadModel's swap at scale 1 */
typedef struct vpx_stamp {           /* 32 bytes */
    uint32_t model_id;               /* a resident model (vpx_model_upload, vpx_model_capture) */
    int32_t  origin[3];              /* grid cell of the box's low corner; may lie outside the grid */
    uint32_t orient;                 /* VPX_ORIENT_*, or any of the 48 */
    uint32_t flags;                  /* VPX_STAMP_* */
    uint8_t  value;                  /* CONSTANT: the byte written */
    uint8_t  match_lo, match_hi;     /* the filter on the cell's current byte, as vpx_brush */
    uint8_t  reserved;               /* 0 */
    uint32_t reserved2;              /* 0 */
} vpx_stamp;
/* Device-side edit: `count` (1..256) resident models gathered into an existing grid, in order,
   one launch each, so a later stamp's filter sees the bytes an earlier one left; all arithmetic
   is integer.  With s = (sx, sy, sz) the model's size, a_q the model axis of grid axis q and
   e_q = s[a_q]:
     - the stamp's box is origin[q] .. origin[q] + e_q - 1 per axis, clipped to [0, n) in int64;
       a box that holds no cell is skipped;
     - a cell g of the clipped box has d_q = g[q] - origin[q], m[a_q] = (flip_q ? e_q - 1 - d_q : d_q)
       and reads v = voxels[m0 + m1*sx + m2*sx*sy];
     - the voxel is empty when v == 0, or when v == 255 under GRID_BYTES; an empty voxel leaves
       the cell alone;
     - otherwise w = (CONSTANT ? value : v), and a cell holding c with match_lo <= c <= match_hi
       and c != w becomes w and counts as changed.  Under the default convention a voxel byte
       255 therefore writes NONE.
   A cell reads one voxel and is written by its own thread only, so the result does not depend
   on the order the device works in.  Then ONE region-local refresh over the stamps' clipped
   boxes, as vpx_grid_brush ends (DESIGN §4 "Stamps"); `out` is filled as for brushes.  The call
   allocates nothing beyond the refresh's record, which comes with the context's first edit.
   VPX_E_INVALID: stamps == NULL, count outside 1..256, unknown grid, unknown model, an orient
   whose axes are not a permutation or that has other bits set, unknown flags, reserved or
   reserved2 != 0, match_lo > match_hi.  Like every world edit the call waits for the frames in
   flight; a device set applies it to every member. */
int vpx_grid_stamp(vpx_ctx* ctx, uint32_t grid_id, const vpx_stamp* stamps, uint32_t count,
                   vpx_brush_result* out /* may be NULL */);
/* Make (or replace) resident model `model_id` from the cells of a box of a grid, on the device:
   raw grid bytes, model index x + y*dx + z*dx*dy = cell (x0 + x, y0 + y, z0 + z), so a stamp with
   VPX_ORIENT_IDENTITY | VPX_STAMP_GRID_BYTES at (x0, y0, z0) puts it back.  Allocates like
   vpx_model_upload; a failure leaves the id empty.  VPX_E_INVALID: unknown grid, model_id above
   vpx_model_upload's cap, a dimension outside 1..256, a box not inside the grid.  Waits for the
   frames in flight; a device set captures on every member. */
int vpx_model_capture(vpx_ctx* ctx, uint32_t model_id, uint32_t grid_id, uint32_t x0, uint32_t y0, uint32_t z0,
                      uint32_t dx, uint32_t dy, uint32_t dz);
/* Debug read-back of a resident model: its size into size_out, and, when dst != NULL, its
   sx*sy*sz bytes (a device set reads its first member).  VPX_E_INVALID: unknown model,
   size_out == NULL, dst != NULL with cap < sx*sy*sz. */
int vpx_model_read(vpx_ctx* ctx, uint32_t model_id, uint8_t* dst /* may be NULL: size only */, uint64_t cap,
                   uint32_t size_out[3]);
typedef struct vpx_stamp_source {    /* 24 bytes */
    const uint8_t* voxels;           /* sx*sy*sz bytes, index x + y*sx + z*sx*sy */
    uint32_t sx, sy, sz, reserved;   /* each dimension 1..256; reserved 0 */
} vpx_stamp_source;
/* The same stamps on a host grid of n^3 bytes (host only, the code the device runs); model_id
   indexes `models`; `flipped` from the host level builder before and after.  VPX_E_INVALID as
   above (an unknown model: model_id >= n_models, NULL voxels, a dimension outside 1..256, reserved
   != 0), and for cells == NULL, models == NULL or n outside vpx_upload_grid's range. */
int vpx_stamp_apply_host(uint8_t* cells, uint32_t n, const vpx_stamp_source* models, uint32_t n_models,
                         const vpx_stamp* stamps, uint32_t count, vpx_brush_result* out /* may be NULL */);
/* Debug read-back of a box of cells, host bytes x fastest: the inverse of vpx_grid_write_box
   (a device set reads its first member). */
int vpx_grid_read_box(vpx_ctx* ctx, uint32_t grid_id, uint8_t* dst, uint32_t x0, uint32_t y0, uint32_t z0,
                      uint32_t dx, uint32_t dy, uint32_t dz);
/* FNV-1a-style 64-bit checksum of a device grid (for size-independent parity checks). */
int vpx_grid_checksum(vpx_ctx* ctx, uint32_t grid_id, uint64_t* out);
/* Debug read-back of a grid's 24 distance-field axis planes as the walkers read them
   (vpx_skip.hpp GridView::dfw): `count` 32-bit words k | L << 8 | Mb << 16 | Mc << 24 from the
   first plane on, at most 24 * 64 * ceil(ceil(N / 4) / 4)^3. */
int vpx_grid_wide_planes(vpx_ctx* ctx, uint32_t grid_id, uint32_t* out, uint64_t count);
/* The same words' low halves, k | L << 8 (GridView::dfa). */
int vpx_grid_axis_planes(vpx_ctx* ctx, uint32_t grid_id, uint16_t* out, uint64_t count);
/* Debug read-back of the mask levels (GridView::l1 for level 1, l2 for level 2): `count` 64-bit
   words from the first on, at most 64 * ceil(ceil(N / 4) / 4)^3 (level 1) or
   64 * ceil(ceil(ceil(N / 4) / 4) / 4)^3 (level 2).  VPX_E_INVALID for another level. */
int vpx_grid_level_words(vpx_ctx* ctx, uint32_t grid_id, uint32_t level, uint64_t* out, uint64_t count);
int vpx_set_volumes(vpx_ctx* ctx, const vpx_volume* volumes, uint32_t count);
int vpx_set_materials(vpx_ctx* ctx, const vpx_material* materials, uint32_t count);
int vpx_set_lights(vpx_ctx* ctx,
                   const vpx_point_light* points, uint32_t n_points,
                   const vpx_spot_light* spots, uint32_t n_spots,
                   const vpx_area_light* areas, uint32_t n_areas,
                   const vpx_dir_light* dir);
int vpx_set_shapes(vpx_ctx* ctx, const vpx_sphere* spheres, uint32_t n_spheres,
                   const vpx_triangle* triangles, uint32_t n_triangles);
int vpx_set_camera(vpx_ctx* ctx, const vpx_camera* camera);
/* Sky dome: Renderer::skyPixels / skyWidth / skyHeight (stbi_loadf RGB floats of the
   equirectangular HDR, renderer.cpp:691; renderer.h:224-226) and HDRLightContribution.
   Texel (u, v) at rgb[3*(u + v*width)].  Used by SampleSky (renderer.cpp:2308-2326) when a
   frame sets VPX_FLAG_SKY, and by vpx_trace when its sky argument is NULL.
   rgb == NULL (or a zero size) removes the texture. */
int vpx_set_sky(vpx_ctx* ctx, const float* rgb, uint32_t width, uint32_t height,
                float hdr_contribution);

/* ---- arithmetic mode ----------------------------------------------------------------
   VPX_ARITH_EXACT (the default): exact 1/x and 1/sqrtf where the reference uses x86
   approximations.  VPX_ARITH_X86_HOST: the reference's own arithmetic,
   bit for bit as THIS host's CPU computes it — FastReciprocal (rcpps + one Newton step,
   renderer.cpp:929-934) for every Renderer::FindNearest volume visit (:969), and
   normalize(__m128) = v * rsqrtps(dpps(v, v, 0x7F)) (template/tmpl8math.h:2356-2360) for the
   primary directions of Renderer::Update (:1735-1765).  rcpps / rsqrtps differ between CPU
   vendors, so the call captures the host's tables (vpx_x86_arith_tables) and uploads them;
   VPX_E_STATE when the host is not x86 or its instructions do not follow the table model.
   The static-camera path's primary rays (GetPrimaryRayNoDOF, the Ray constructor) stay exact,
   as in the reference. */
#define VPX_ARITH_EXACT 0u
#define VPX_ARITH_X86_HOST 1u
int vpx_set_arithmetic(vpx_ctx* ctx, uint32_t mode);
/* Host only (no device): capture this CPU's rcpss / rsqrtss tables under FTZ | DAZ and
   spot-check the model (vpx_x86.hpp) against the instructions.  info = {rcp key shift, rsqrt
   key shift, first rsqrt entry, entries}; out (may be NULL: sizes only) receives the entries
   (cap >= info[3]).  VPX_E_STATE: not x86, or the spot check failed. */
int vpx_x86_arith_tables(uint32_t* out, uint64_t cap, uint32_t info[4]);
/* Host only: the model against this CPU's rcpss and rsqrtss for every input bit pattern in
   [lo, hi] (0, 0xffffffff = all 2^32) on `threads` threads; mismatches[0] / [1] count rcp /
   rsqrt disagreements, first_bad[] the first input of each. */
int vpx_x86_arith_verify(uint32_t lo, uint32_t hi, uint32_t threads, uint64_t mismatches[2],
                         uint32_t first_bad[2]);

/* ---- display interop ---------------------------------------------
   Replaces the per-frame host upload of Surface::pixels in GLTexture::CopyFrom
   (template/opengl.cpp:144-149, called from template/template.cpp:305).  The host creates a
   GL_PIXEL_UNPACK_BUFFER of W*H*4 bytes once and registers it with its GL context current on
   the calling thread, on this context's GPU (device set: devices[0]); gl_buffer == 0
   unregisters (vpx_destroy does too).  Per frame: vpx_gl_map returns the buffer's device
   address (ordered on the context's stream), the host passes it as `rgb8` to vpx_render or
   vpx_render_reproject, vpx_gl_unmap hands it back to GL, and glTexSubImage2D with the
   buffer bound updates the texture — the frame never crosses PCIe.  `bytes` (may be NULL)
   receives the buffer size; the host checks it against W*H*4.  Errors: VPX_E_DEVICE when
   HIP cannot register the buffer (no current GL context, another GPU), VPX_E_STATE for
   map / unmap / register out of order.  Unmeasured on hardware: no GL display here. */
int vpx_gl_register_buffer(vpx_ctx* ctx, unsigned int gl_buffer);
int vpx_gl_map(vpx_ctx* ctx, uint32_t** rgb8, size_t* bytes);
int vpx_gl_unmap(vpx_ctx* ctx);

/* ---- the hot path -------------------------------------------------------------------- */
/* One frame: primary rays, Trace(ray, max_bounces) per pixel, running-average accumulate
   (w = 1/(frame_index+1)), Reinhard-Jodie tonemap, RGB8 pack.  `accum` (float4[W*H]) and
   `rgb8` (uint32[W*H]) are DEVICE pointers; accum is read-modify-write. Either may be NULL
   when VPX_FLAG_NO_TONEMAP is not set for rgb8.  `stats` (host) may be NULL.            */
int vpx_render(vpx_ctx* ctx, const vpx_frame_params* params, float* accum, uint32_t* rgb8,
               vpx_stats* stats);
/* Tile-sharded variant for multi-GPU: render the tiles t (tile_w x tile_h, row-major tile
   order) with t % n_ranks == rank into a packed float4 buffer (tile after tile; inside a
   16x16 tile entry i is pixel (8*((i>>6)&1) + (i&7), 8*(i>>7) + ((i>>3)&7)): the four 8x8
   quadrants in row-major order, row-major inside each; partial edge tiles padded with
   zeros).  DEVICE pointer.                                                               */
int vpx_render_tiles(vpx_ctx* ctx, const vpx_frame_params* params, uint32_t tile_w,
                     uint32_t tile_h, uint32_t rank, uint32_t n_ranks, float* packed,
                     vpx_stats* stats);
/* Number of float4 elements one rank's packed buffer holds (all ranks use the max). */
uint64_t vpx_tiles_packed_len(uint32_t width, uint32_t height, uint32_t tile_w,
                              uint32_t tile_h, uint32_t n_ranks);
/* Tile-sharded render with the accumulator sharded with the tiles: the rank keeps the
   running average of ITS tiles in `accum_packed` (float4[vpx_tiles_packed_len], DEVICE,
   persistent across frames, packed layout as vpx_render_tiles; blended with weight
   1/(frame_index+1) like vpx_render's accumulator, so start it finite, e.g. zeroed) and
   tonemaps them into `rgb8_packed` (uint32[len], DEVICE) — the only bytes rank 0 needs
   for the screen.  Bit-identical to vpx_render's accumulator / screen for those pixels. */
int vpx_render_tiles_accum(vpx_ctx* ctx, const vpx_frame_params* params, uint32_t tile_w,
                           uint32_t tile_h, uint32_t rank, uint32_t n_ranks, float* accum_packed,
                           uint32_t* rgb8_packed, vpx_stats* stats);
/* Accumulation windows: frames frame_index .. frame_index + n_frames - 1 of params (the
   reference's spp loop of Renderer::Tick calls, renderer.cpp:1646-1891, one per frame with
   w = 1/(n+1)), with the same results as n_frames calls of vpx_render /
   vpx_render_tiles_accum (bit-identical accumulator and RGB8).  When a frame's share is small
   (a rank's 1/n_ranks of the tiles), several frames render in ONE chain of launches — frame b
   in tile blocks [b*T, (b+1)*T) with its own seeds — and a single blend folds their samples
   into the accumulator in frame order; large frames render one chain each.  Lanes
   (vpx_set_pipeline) carry the chains as they carry frames.  VPX_FLAG_NO_TONEMAP frames
   render frame by frame.  On a device set (vpx_create_multi) vpx_render_window is n_frames
   calls of vpx_render on the set and takes what that takes (accum may be NULL with rgb8
   given: the members' sharded accumulators). */
int vpx_render_window(vpx_ctx* ctx, const vpx_frame_params* params, uint32_t n_frames, float* accum,
                      uint32_t* rgb8);
int vpx_render_tiles_accum_window(vpx_ctx* ctx, const vpx_frame_params* params, uint32_t n_frames,
                                  uint32_t tile_w, uint32_t tile_h, uint32_t rank, uint32_t n_ranks,
                                  float* accum_packed, uint32_t* rgb8_packed);
/* Rank 0: scatter n_ranks gathered packed RGB8 buffers (back to back, DEVICE) into the
   screen rgb8 (uint32[W*H], DEVICE). */
int vpx_composite_rgb8(vpx_ctx* ctx, const vpx_frame_params* params, uint32_t tile_w,
                       uint32_t tile_h, uint32_t n_ranks, const uint32_t* gathered, uint32_t* rgb8);
/* Rank-0 composite: `gathered` = n_ranks packed buffers back to back (DEVICE); unpack,
   accumulate into accum and tonemap into rgb8 exactly like vpx_render's epilogue.      */
int vpx_composite_tiles(vpx_ctx* ctx, const vpx_frame_params* params, uint32_t tile_w,
                        uint32_t tile_h, uint32_t n_ranks, const float* gathered,
                        float* accum, uint32_t* rgb8);

/* ---- static-camera path ------------------------------------ */
/* Renderer::prevCamera as CopyToPrevCamera leaves it (renderer.cpp:1893-1902): position
   and the four frustum-plane normals of Camera::SetFrustumNormals (camera.h:53-66). */
typedef struct vpx_prev_camera {
    float cam_pos[3];
    float left_normal[3];
    float right_normal[3];
    float top_normal[3];
    float bottom_normal[3];
    float pad;
} vpx_prev_camera;  /* 64 bytes */
/* One frame of Renderer::Tick's static branch (renderer.cpp:1996-2101): TraceReproject
   (renderer.cpp:1330-1585) of Camera::GetPrimaryRayNoDOF per pixel (AA / DOF flags are
   ignored), then per pixel PointToUV into `prev`, IsOccludedPrevFrame, SampleHistory,
   ClampHistory, the material weight, lerp, ApplyReinhardJodie, RGB8.  `history`
   (float4[W*H], DEVICE) is illuminationHistoryBuffer: read, then replaced by this frame's
   illumination (tempIlluminationBuffer).  `rgb8` DEVICE uint32[W*H] (may be NULL). */
int vpx_render_reproject(vpx_ctx* ctx, const vpx_frame_params* params, const vpx_prev_camera* prev,
                         float* history, uint32_t* rgb8, vpx_stats* stats);

/* Work counters accumulated on device over every render call since the last reset
   (no per-frame synchronisation); kernel_ms/total_ms are not filled here.            */
int vpx_get_counters(vpx_ctx* ctx, vpx_stats* out, int reset);

/* ---- the player light probe (Renderer::inLight, renderer.h:231) ---------------------- */
/* A path that reaches smoke (materials 9..14) in volume 0, the player, runs
   Illumination(ray, incLight) and sets Renderer::inLight when sqrLength(incLight) exceeds
   sqrThreshold (Trace renderer.cpp:1228-1240, TraceSmoke :1438-1450).  Renderer::Tick reads
   the flag (:2112-2118) and clears it (:2206).  The record accumulates on the device over
   every render call since the last reset (vpx_render, vpx_render_tiles[_accum], the window
   entries, vpx_render_reproject; a device set sums its members and takes the largest
   max_sqr), with no per-frame synchronisation; the read synchronises like
   vpx_get_counters.  Counts and maximum do not depend on execution order.  The unit
   entries (vpx_trace, vpx_trace_probe) do not add to it; vpx_get_counters' reset does not
   clear it, and this reset leaves the work counters alone. */
#define VPX_PLAYER_LIGHT_SQR 16.0f            /* sqrThreshold, renderer.cpp:1233, 1443 */
typedef struct vpx_player_light {             /* 24 bytes */
    uint64_t probes;    /* probe Illumination calls: paths that reached smoke in volume 0 */
    uint64_t lit;       /* of them, sqrLength(incLight) > VPX_PLAYER_LIGHT_SQR (a NaN is not) */
    float    max_sqr;   /* largest sqrLength(incLight) seen (NaNs apart), 0 when none */
    uint32_t in_light;  /* lit != 0: Renderer::inLight */
} vpx_player_light;
int vpx_get_player_light(vpx_ctx* ctx, vpx_player_light* out, int reset);

/* ---- per-stage profile (measurement; off by default) ------------------------------ */
/* Stages of one vpx_render / vpx_render_tiles call. */
#define VPX_STAGE_PRIMARY 0  /* primary rays + Renderer::FindNearest                   */
#define VPX_STAGE_SHADE 1    /* Trace material switch (+ glass/smoke exit marches)      */
#define VPX_STAGE_SHADOW 2   /* Renderer::IsOccluded of the emitted shadow rays         */
#define VPX_STAGE_RESOLVE 3  /* light sums                                              */
#define VPX_STAGE_BOUNCE 4   /* Renderer::FindNearest of bounce rays                    */
#define VPX_STAGE_FINISH 5   /* fold + accumulate + tonemap (or tile pack)              */
#define VPX_STAGE_FRAME 6    /* a whole Trace-depth-0 frame in one launch (small launches,
                                single volume: stages 0, 1, 2, 3, 5 fused)    */
#define VPX_STAGE_INSTANCES 7 /* multi-volume scenes: the primary rays' Renderer::FindNearest
                                over the volumes after the world (volume 0, walked in stage 0)
                                and the analytic shapes, then level 0's shade */
#define VPX_NUM_STAGES 8
typedef struct vpx_profile {
    float stage_ms[8];            /* summed device time per stage (HIP events on the stream) */
    uint32_t stage_launches[8];   /* kernel launches timed per stage                         */
    uint64_t stage_cells[8];      /* DDA cells read per stage (all launches, incl. untimed)  */
    float stage_busy_ms[8];       /* union of the stage's launch intervals: launches that run
                                     at the same time (frames in flight, vpx_set_pipeline)
                                     count once; equals stage_ms when they do not overlap     */
} vpx_profile;
/* Time every stage launch of the next renders with HIP events on the library's stream
   (up to `max_launches` launches; 0 turns profiling off).  Adds no synchronisation. */
int vpx_profile_enable(vpx_ctx* ctx, uint32_t max_launches);
/* Time only the stages whose bit (1 << VPX_STAGE_*) is set in `stage_mask` (default: all).
   Each timed launch adds two event records to the stream: timing all five C1 stages
   slowed the frame by 4.3 %, so a benchmark times only the stage it reports. */
int vpx_profile_select(vpx_ctx* ctx, uint32_t stage_mask);
/* Synchronise, sum the recorded stage times and return them (reset: clear events and
   the per-stage cell counters). */
int vpx_profile_read(vpx_ctx* ctx, vpx_profile* out, int reset);
/* The busy-time rule vpx_profile_read applies (host only, no device): the length of the union
   of n intervals [se[2i], se[2i+1]) in ms, overlaps counted once.  Starts may be negative
   (a lane's launch that began before the first recorded event). */
float vpx_profile_busy_union(const float* se, uint32_t n);
/* Debug: which form of the one-launch depth-0 frame kernel the context's last render launched:
   0 = none (the frame ran as separate stages), 1 = the kernel specialised on what its launch
   guarantees (one volume, no shapes, depth 0, one shadow slot per path), 2 = the lean form on
   top (no spot or area lights, constant sky, no VPX_FLAG_DOF).  The forms compute the same
   bits; tests use it to know which one they compared.  Host state only, no synchronisation. */
int vpx_debug_last_frame_kernel(vpx_ctx* ctx);
/* Debug: the device and pinned-host allocations the library holds right now, over every context
   of the process.  A context gives all of its allocations back in vpx_destroy, so the count
   after it equals the count before vpx_create.  Host state only, no GPU call. */
uint64_t vpx_debug_live_buffers(void);

/* ---- unit entries (host pointers; mirror the reference per-ray functions) ---------- */
int vpx_find_nearest(vpx_ctx* ctx, const vpx_ray* rays, uint32_t n, vpx_hit* hits);
int vpx_is_occluded(vpx_ctx* ctx, const vpx_ray* rays, uint32_t n, uint8_t* occluded);
/* Trace(ray, depth) with an explicit xorshift32 state per ray; radiance = float3[n].
   sky: the constant SampleSky colour (activateSky == false), or NULL for the texture. */
int vpx_trace(vpx_ctx* ctx, const vpx_ray* rays, const uint32_t* seeds, uint32_t n,
              int32_t depth, const float sky[3], int32_t area_samples, float* radiance);
/* vpx_trace plus each ray's player light probes (the smoke branch's Illumination call in
   volume 0, renderer.cpp:1228-1240; a path can probe once per level): their number, how many
   exceeded VPX_PLAYER_LIGHT_SQR and the largest sqrLength(incLight).  radiance (may be NULL)
   is bit-identical to vpx_trace's; probes = vpx_ray_probe[n], host. */
typedef struct vpx_ray_probe { uint32_t probes, lit; float max_sqr; uint32_t reserved; } vpx_ray_probe; /* 16 */
int vpx_trace_probe(vpx_ctx* ctx, const vpx_ray* rays, const uint32_t* seeds, uint32_t n, int32_t depth,
                    const float sky[3], int32_t area_samples, float* radiance /* may be NULL */,
                    vpx_ray_probe* probes /* n, host */);
/* Filtered ray queries: a batch of rays cast against a chosen part of the scene, with a material
   range treated as transparent.  Renderer::FindNearestPlayer (renderer.cpp:1020-1071, the
   player's ray in Renderer::Tick, :2139-2152) is FindNearest from volume 1 on (volume 0 is the
   player), without the spheres and triangles, each volume walked with
   Scene::FindNearestExcept(ray, SMOKE_LOW_DENSITY, SMOKE_PLAYER) (template/scene.cpp:813-873):
   filter {1, VPX_MAT_SMOKE_LOW_DENSITY, VPX_MAT_SMOKE_PLAYER, VPX_QUERY_NO_SHAPES |
   VPX_QUERY_RAW_DIRECTION}.  Renderer::IsOccludedPlayerClimbable (renderer.cpp:245-273) is
   IsOccluded from volume 1 on without the shapes: {1, 1, 0, VPX_QUERY_NO_SHAPES}.
   {0, 1, 0, 0} is vpx_find_nearest / vpx_is_occluded, bit for bit.
   vpx_hit keeps its meaning: vox_index is the index in the context's volume list (not offset by
   first_volume; first_volume >= count visits none: -2 and t = tmax, or the shapes' result),
   cells counts every cell read, the excepted ones the ray passed included, and inside_glass
   comes back as given when the shapes are off.  In VPX_ARITH_X86_HOST the filtered FindNearest
   takes FastReciprocal (renderer.cpp:1043) like vpx_find_nearest; the occlusion keeps 1 / D.
   VPX_E_INVALID (also with n == 0): f == NULL, unknown flag bits, a non-empty range with an
   end above 255, and any non-empty range in vpx_is_occluded_filtered (the reference has no
   IsOccludedExcept). */
#define VPX_QUERY_NO_SHAPES     0x1u  /* do not test spheres / triangles (FindNearestPlayer, IsOccludedPlayerClimbable) */
#define VPX_QUERY_RAW_DIRECTION 0x2u  /* vpx_ray.direction is used as given: Ray(O, D, rD, Dsign, len), scene.cpp:29-37
                                         (PlayerCharacter::GetRay normalises by itself, src/Game/PlayerCharacter.cpp:11-18;
                                         normalising twice changes low bits of D, and with them t) */
typedef struct vpx_ray_filter {       /* 16 bytes */
    uint32_t first_volume;            /* volumes first_volume .. count-1 are visited, in index order */
    uint32_t mat_lo, mat_hi;          /* cells with mat_lo <= m <= mat_hi are read and passed through (scene.cpp:826);
                                         mat_lo > mat_hi: no material is excepted */
    uint32_t flags;                   /* VPX_QUERY_* ; other bits: VPX_E_INVALID */
} vpx_ray_filter;
int vpx_find_nearest_filtered(vpx_ctx* ctx, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, vpx_hit* hits);
int vpx_is_occluded_filtered(vpx_ctx* ctx, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f, uint8_t* occluded);
/* Hit cells: the filtered FindNearest that also reports WHICH cell was hit and through which face
   the walk entered it, so that "point at a voxel, dig it; point at a face, build on it" needs no
   guess from O + t * D (a point that lies on a cell face by construction).  The record describes
   the winning volume's walk as the reference's plain loop runs it (Scene::FindNearest /
   FindNearestExcept, template/scene.cpp:751-873): `cell` is the (X, Y, Z) at which the loop
   returned, axis and step are those of the last tmax advance before it, face_cell = cell -
   step * e_axis, the cell the walk visited immediately before.  A hit in the walk's first cell
   (Setup3DDDA's start cell: the ray starts inside a solid cell or enters the cube straight into
   one) took no step: VPX_CELL_FACE is clear, face_cell is zero, and the host falls back on the
   normal.  Cells that the material range lets the ray pass through count as visited, so face_cell
   holds NONE or an excepted material, never another solid one; it is a visited cell, so
   VPX_CELL_FACE_IN comes with every VPX_CELL_FACE.  Misses and shape wins (vox_index < 0) give an
   all-zero record.  hits[i] is vpx_find_nearest_filtered's, bit for bit, in both arithmetic modes,
   and the refusals are the same. */
#define VPX_CELL_HIT     0x1u  /* a voxel volume won (vox_index >= 0): cell[], grid_id valid */
#define VPX_CELL_FACE    0x2u  /* the walk stepped INTO the hit cell: axis, face_cell valid   */
#define VPX_CELL_FACE_IN 0x4u  /* face_cell lies inside the grid [0, n)^3                      */
typedef struct vpx_hit_cell {      /* 32 bytes */
    int32_t  cell[3];              /* the hit cell in the winning volume's grid                */
    uint32_t grid_id;              /* that volume's grid                                       */
    int32_t  face_cell[3];         /* the cell the walk visited immediately before: cell - step on `axis` */
    uint32_t flags;                /* VPX_CELL_* | axis << 8 (0..2) | (step < 0 ? 1 : 0) << 10 */
} vpx_hit_cell;
int vpx_find_nearest_cells(vpx_ctx* ctx, const vpx_ray* rays, uint32_t n, const vpx_ray_filter* f,
                           vpx_hit* hits, vpx_hit_cell* cells);            /* host pointers */
/* The same query for the ray of integer pixel (x, y): Camera::GetPrimaryRayNoDOF with the
   context's camera (template/camera.h:103-110), the ray of the static-camera path
   (vpx_render_reproject), built with exact arithmetic in both arithmetic modes as on that path.
   f == NULL is the neutral filter {0, 1, 0, 0}; VPX_QUERY_RAW_DIRECTION is refused
   (VPX_E_INVALID: the library builds these rays); VPX_E_STATE without a camera; VPX_E_INVALID
   for a zero size, x >= width, y >= height or a null output. */
int vpx_pick_pixel(vpx_ctx* ctx, uint32_t width, uint32_t height, uint32_t x, uint32_t y,
                   const vpx_ray_filter* f /* NULL = {0,1,0,0} */, vpx_hit* hit, vpx_hit_cell* cell);
/* vpx_pick_pixel for every pixel of params->width x height at once (AA and DOF flags ignored; of
   params only the size is used), one uint4 per pixel, row-major, in DEVICE memory:
     .x  the bits of t (tmax = 1e34 on a miss)
     .y  (uint16)(vox_index + 2) | material << 16 | face << 24, face = 0 for none (VPX_CELL_FACE
         clear), else 1 + 2 * axis + (step < 0)
     .z  cell.x | cell.y << 16          .w  cell.z
   Bit for bit vpx_pick_pixel's records.  Runs on the context's stream without synchronising,
   ordered like vpx_render_reproject; adds nothing to the work counters or the player-light
   record.  VPX_E_STATE with more than 65533 volumes.  On a device set all three entries run on
   devices[0]. */
int vpx_render_ids(vpx_ctx* ctx, const vpx_frame_params* params, const vpx_ray_filter* f /* NULL = neutral */,
                   uint32_t* ids /* uint4[W*H], DEVICE */);
/* Ray batches that already live on the device: vpx_find_nearest_cells / vpx_is_occluded_filtered on
   DEVICE pointers (no reference counterpart; the records of Renderer::FindNearest / IsOccluded per
   ray).  hits[i] and cells[i] are vpx_find_nearest_cells' records for rays[i] and occluded[i] is
   vpx_is_occluded_filtered's byte, bit for bit, in both arithmetic modes, with the same filter
   semantics and refusals (f == NULL is the neutral filter {0, 1, 0, 0}; VPX_QUERY_RAW_DIRECTION is
   allowed; vpx_cast_occluded refuses a material range).  The results do not depend on the order of
   the rays, the form, max_waves or which lane walked a ray; vpx_hit.cells is per ray.
   The calls are queued on the context's stream, ordered like vpx_render_ids (frames in flight and
   world edits included), and do not synchronise; they add nothing to the work counters or the
   player-light record; on a device set they run on devices[0].
   Two forms.  Per lane: one thread per ray, every scene and filter.  Pool: persistent waves that
   take the batch's rays in grabs and hand a new ray to each lane as its walk ends, so a wave is
   not held by its longest walk; it serves the batches that visit exactly one volume
   (first_volume == count - 1), with or without a material range or the shapes and with any tmax.
   VPX_CAST_POOL on any other batch takes the per-lane form; flags == 0 is the library's choice
   (DESIGN.md section 4); vpx_debug_last_cast_kernel tells which form the last call launched.
   The pool's grab counter (a few cache lines) belongs to the context: allocated with the first
   pool call, zeroed on the stream per call; later calls allocate nothing.
   VPX_E_INVALID: a null context; null rays, hits or occluded with n > 0; n > 2^30; unknown flags
   bits, both form bits, nonzero reserved; the filter refusals.  VPX_E_STATE as the host entries.
   n == 0 is VPX_OK and launches nothing.  Overlapping buffers are the caller's error. */
#define VPX_CAST_PER_LANE 0x1u   /* one thread per ray, no refill (the unit entries' form) */
#define VPX_CAST_POOL     0x2u   /* the pool form wherever it can serve the batch (above)  */
typedef struct vpx_cast {        /* 16 bytes */
    uint32_t flags;              /* 0 = the library's choice; both bits: VPX_E_INVALID     */
    uint32_t max_waves;          /* pool form: at most this many persistent waves, rounded up to whole
                                    workgroups; 0 = the library's choice.  Leaves CUs to frames in
                                    flight, and lets a small batch exercise many refills per wave */
    uint32_t reserved[2];        /* 0 */
} vpx_cast;
int vpx_cast_nearest(vpx_ctx* ctx, const vpx_ray* rays /* DEVICE, n */, uint32_t n,
                     const vpx_ray_filter* f /* NULL = {0,1,0,0} */, const vpx_cast* opt /* NULL = zeros */,
                     vpx_hit* hits /* DEVICE, n */, vpx_hit_cell* cells /* DEVICE, n; may be NULL */);
int vpx_cast_occluded(vpx_ctx* ctx, const vpx_ray* rays /* DEVICE */, uint32_t n, const vpx_ray_filter* f,
                      const vpx_cast* opt, uint8_t* occluded /* DEVICE, n */);
int vpx_debug_last_cast_kernel(vpx_ctx* ctx);  /* 0 none launched, 1 per-lane, 2 pool; host state only */
/* Plane-keyed denoise: an a-trous filter over a float4 image (a vpx_render accumulator) whose edge
   test is an integer equality on the vpx_render_ids record (no reference counterpart; the
   reference's only filter is the static-camera history, renderer.cpp:1996-2101).  A pixel's key:
   with v = .y & 0xffff and face = .y >> 24, valid iff v >= 2 (a voxel volume won) and
   1 <= face <= 6; then axis = (face - 1) >> 1, coord = .z & 0xffff / .z >> 16 / .w for axis
   0 / 1 / 2, and the key is the pair (.y, 0x80000000 | coord): same volume, material, face and
   plane.  Every other pixel (miss, shape win, first-cell hit, a malformed face) has the invalid
   key (0, 0); the key is only compared, never used as an index.
   Pass p (0-based, step s = 1 << p) reads image S and writes D.  A pixel q with an invalid key
   keeps S(q), all four channels.  Otherwise, over the taps r = (x + i*s, y + j*s), j = -2..2 outer,
   i = -2..2 inner, that lie inside the image and have q's key:
     h = H[|j|] * H[|i|], H = {0.375, 0.25, 0.0625}
     w = h                                           (sigma_l == 0)
     w = h / (1 + d*d), d = (lum(S(r)) - lum(S(q))) * (1.0f / sigma_l), lum(c) = (c.x*0.2126f +
         c.y*0.7152f) + c.z*0.0722f                  (sigma_l > 0)
     acc = acc + w * S(r) per colour channel (the product rounded, then the sum), wsum = wsum + w
   and D(q) = (acc / wsum, S(q).w).  A tap that does not match is not read into the arithmetic, so
   a NaN on another surface stays there; the centre always matches, so wsum >= 9/64.  Every
   operation rounds once to float32; the result is defined bit for bit (NaN payloads apart).  The
   call runs d->passes passes, the first reading `in`, the last writing `out`; when rgb8 is not
   NULL it receives the frame's tonemap (Reinhard-Jodie + RGB8 pack, as vpx_render's) of `out`.
   vpx_denoise_ids runs on the context's stream without synchronising, ordered like
   vpx_render_ids (it follows a vpx_render on that stream, frames in flight included); adds
   nothing to the work counters or the player-light record; needs no camera and no world; on a
   device set it runs on devices[0].  Its scratch (the keys, and two images when passes > 1)
   belongs to the context, comes with the first call and grows with the size: VPX_E_NOMEM when
   that fails.  VPX_E_INVALID: a null p, ids, in, out or d; a zero size or one beyond
   vpx_frame_params' limits; passes outside 1..5; a negative, NaN or infinite sigma_l; nonzero
   flags or reserved; out == in or out == ids.  Any other overlap of the buffers is the caller's
   error and gives undefined pixels.
   Limits: the ids come from the un-jittered pixel-centre ray, so with VPX_FLAG_AA / VPX_FLAG_DOF
   they guide a slightly different ray; a path through glass, smoke or a mirror is keyed by its
   first hit only; shadows on one surface are softened unless sigma_l is set, and sigma_l
   protects little at one sample per pixel. */
typedef struct vpx_denoise {      /* 16 bytes */
    uint32_t passes;              /* 1..5: steps 1, 2, 4, 8, 16 */
    float    sigma_l;             /* 0 = plane key only; else finite and > 0 */
    uint32_t flags;               /* 0 */
    uint32_t reserved;            /* 0 */
} vpx_denoise;
int vpx_denoise_ids(vpx_ctx* ctx, const vpx_frame_params* p /* only width, height */,
                    const uint32_t* ids /* uint4[W*H], DEVICE */, const float* in /* float4[W*H], DEVICE */,
                    float* out /* float4[W*H], DEVICE */, uint32_t* rgb8 /* uint32[W*H], DEVICE, may be NULL */,
                    const vpx_denoise* d);
/* The same filter on host memory (no device, no context): the CPU path of the same code
   (csrc/vpx_denoise.hpp).  VPX_E_NOMEM when its scratch cannot be allocated. */
int vpx_denoise_host(uint32_t width, uint32_t height, const uint32_t* ids, const float* in, float* out,
                     uint32_t* rgb8 /* may be NULL */, const vpx_denoise* d);
/* Plane-keyed reprojection: temporal accumulation under camera motion (no reference counterpart:
   Renderer::Tick resets its accumulator when the camera moves, and vpx_render_reproject's history,
   renderer.cpp:1996-2101, holds only while it stands still).  The history of the previous frame is
   carried to the current camera and blended with this frame's samples; a history pixel is taken
   only where its vpx_render_ids record has the current pixel's key (vpx_denoise_ids' key: volume,
   material, entry face, hit-cell coordinate along the face's axis), an integer equality in place
   of depth / normal / albedo thresholds.  hist.w carries the history length as a float.  Every
   operation rounds once to float32, nothing is contracted; the result is defined bit for bit (NaN
   payloads apart).  Per pixel q = (x, y), with W, H = p->width, p->height:
   0. No history, out = (cur.rgb, 1.0f), when Key(q) is invalid; when q's material (.y >> 16 & 255)
      lies in nohist_lo..nohist_hi; when ids_prev / hist_in are NULL; when max_history is 1 (the
      blend below would have a = 1, and h + (cur - h) is not cur in float32: the arm is defined,
      not computed); and wherever a step below says so.
   1. Key(q) is vpx_denoise_ids' key of ids_cur[q].
   2. q's ray is vpx_pick_pixel's: Camera::GetPrimaryRayNoDOF (camera.h:103-110) from r->cur through
      Ray::Ray, exact arithmetic: u = (float)x * (1.0f / (float)W), v likewise, E = (top_left +
      (top_right - top_left) * u) + (bottom_left - top_left) * v, d = E - cam_pos, D = d * (1.0f /
      sqrtf(d.x*d.x + d.y*d.y + d.z*d.z)).  With t the float whose bits are ids_cur[q].x the hit
      point is P = cam_pos + t * D per component (the product, then the sum).
   3. n_volumes > 0 (moving volumes): v = (.y & 0xffff) - 2; v >= n_volumes: no history; when
      cur_volumes[v] and prev_volumes[v] differ in a byte of matrix or inv_matrix, P =
      TransformPosition(TransformPosition(P, cur_volumes[v].inv_matrix), prev_volumes[v].matrix),
      rows 0-2, m[0]*x + m[1]*y + m[2]*z + m[3]*1.0f summed left to right (tmpl8math.cpp:345-353);
      else P stays.  The key is in object space and survives the move.
   4. Camera::PointToUV (camera.h:34-49) into r->prev: delta = P - cam_pos, ld / rd / td / bd =
      dot(left / right / top / bottom normal, delta) (n.x*d.x + n.y*d.y + n.z*d.z, left to right).
      No history unless all four are > 0: SetFrustumNormals' normals point into the pyramid, so a
      point behind the previous camera or outside its view fails (the reference has no such test;
      its IsValid tests u, v, which a point behind the camera can pass).  px = (ld / (ld + rd)) * W,
      py = (td / (td + bd)) * H, no half-pixel offsets: pixel x's ray passes through u = x / W.
      (px or py NaN, from inf / inf: no history.)  tlx = trunc(px), fx = px - (float)tlx, gx =
      1.0f - fx; likewise tly, fy, gy.
   5. The taps, in this order: (tlx, tly), (tlx+1, tly), (tlx, tly+1), (tlx+1, tly+1), weights
      gx*gy, fx*gy, gx*fy, fx*fy.  A tap r is usable iff it is inside the image, its weight is
      > 0, Key(ids_prev[r]) equals Key(q), and hist_in[r].w >= 1.0f (a NaN fails).  An unusable tap
      never enters the arithmetic (no multiplication by zero: a NaN on another surface stays
      there).  No usable tap: no history.
   6. Over the usable taps in order: hs = hs + w * hist_in[r].rgb per channel, ws = ws + w; then
      h = hs / ws, n = min(min over the usable taps of hist_in[r].w, max_history - 1) + 1,
      a = 1.0f / n, out.rgb = h + (cur.rgb - h) * a, out.w = n.
   7. rgb8, when not NULL, receives the frame's tonemap (as vpx_denoise_ids') of out, same launch.
   Per tick of a moving camera: vpx_render at frame_index 0 into `cur`, vpx_render_ids, this call,
   vpx_denoise_ids on hist_out, RGB8.  Feed hist_out, not the denoised image, back as the next
   hist_in, and this frame's ids as the next ids_prev.
   vpx_reproject_ids runs on the context's stream without synchronising, ordered like
   vpx_denoise_ids; adds nothing to the work counters or the player-light record; needs no camera
   and no world in the context; on a device set it runs on devices[0].  Its scratch (the volume
   table: 2 * n_volumes * 12 floats and a moved flag per volume, uploaded on the stream) belongs
   to the context and grows with the size: VPX_E_NOMEM when that fails.  VPX_E_INVALID: a null p,
   ids_cur, cur, hist_out or r; exactly one of ids_prev / hist_in null; a zero size or one beyond
   vpx_frame_params' limits; max_history not integer-valued in 1..65536; nohist_hi > 255 with
   nohist_lo <= nohist_hi; nonzero flags or reserved; n_volumes > 65534; n_volumes > 0 with a null
   volume array; hist_out equal to any input.  Any other overlap is the caller's error.
   Limits: sky, shape and first-cell pixels (invalid keys) never accumulate; the ids guide the
   un-jittered pixel-centre ray, so with VPX_FLAG_AA / VPX_FLAG_DOF the samples belong to a
   slightly different ray; a path through glass, smoke or a mirror is view-dependent and keyed by
   its first hit only (hence nohist_lo..hi); a lighting change fades in over max_history frames:
   there is no neighbourhood clamp. */
typedef struct vpx_reproject {    /* 168 bytes */
    vpx_camera      cur;          /* the camera ids_cur was rendered with (vpx_render_ids' ray) */
    vpx_prev_camera prev;         /* the camera ids_prev / hist_in were rendered with            */
    float    max_history;         /* integer-valued, 1..65536: the history length's cap          */
    uint32_t nohist_lo, nohist_hi;/* first-hit materials that take no history (view-dependent:
                                     5..14 = metal, glass, smoke); lo > hi: none                 */
    uint32_t n_volumes;           /* 0: static world; else the length of the two arrays below   */
    uint32_t flags, reserved;     /* 0 */
} vpx_reproject;
int vpx_reproject_ids(vpx_ctx* ctx, const vpx_frame_params* p /* only width, height */,
                      const uint32_t* ids_cur, const uint32_t* ids_prev /* uint4[W*H], DEVICE; prev may be NULL */,
                      const float* cur /* float4[W*H], DEVICE: this frame's samples */,
                      const float* hist_in /* float4[W*H], DEVICE; NULL with ids_prev */,
                      float* hist_out /* float4[W*H], DEVICE */, uint32_t* rgb8 /* uint32[W*H], DEVICE, may be NULL */,
                      const vpx_reproject* r,
                      const vpx_volume* cur_volumes, const vpx_volume* prev_volumes /* HOST, n_volumes each, or NULL */);
/* The same pass on host memory (no device, no context): the CPU path of the same code
   (csrc/vpx_reproject.hpp).  VPX_E_NOMEM when the volume table cannot be allocated. */
int vpx_reproject_ids_host(uint32_t width, uint32_t height, const uint32_t* ids_cur, const uint32_t* ids_prev,
                           const float* cur, const float* hist_in, float* hist_out, uint32_t* rgb8 /* may be NULL */,
                           const vpx_reproject* r, const vpx_volume* cur_volumes, const vpx_volume* prev_volumes);
/* Variance-guided denoise: vpx_reproject_ids carrying the first two moments of the luminance, and
   vpx_denoise_ids with a per-pixel luminance tolerance derived from them (SVGF's structure; no
   reference counterpart).  The edge test stays the integer plane key; only the one soft weight
   becomes local: a shadow edge on a floor whose history says "this pixel does not vary" is kept,
   where a global sigma_l would either leave the noise in or smear it.  lum and Key are
   vpx_denoise_ids'; every operation rounds once to float32, products before sums, nothing
   contracted, / and sqrtf correctly rounded; the results are defined bit for bit (NaN payloads apart).

   vpx_reproject_moments: hist_out and rgb8 are vpx_reproject_ids' for the same arguments, bit for
   bit.  In addition, per pixel q with l = lum(cur.rgb), l2 = l * l:
     no history (every case in which vpx_reproject_ids gives (cur.rgb, 1)): mom_out = (l, l2);
     history: over the same usable taps, in the same order, with the same weights,
       s1 = s1 + w * mom_in[r].x, s2 = s2 + w * mom_in[r].y; h1 = s1 / ws, h2 = s2 / ws; with the
       blend's a = 1.0f / n: mom_out = (h1 + (l - h1) * a, h2 + (l2 - h2) * a).
   mom_in[r] is read only under a usable tap.  Stream order, counters, device sets and the scratch
   (shared) are vpx_reproject_ids'.  VPX_E_INVALID: vpx_reproject_ids' refusals; a null mom_out;
   exactly one of mom_in / hist_in null; mom_out equal to any input or to hist_out; hist_out equal
   to mom_in.  Feed mom_out back as the next mom_in, beside hist_out.

   vpx_denoise_var: `in` is a float4 image; with mom != NULL its .w is the history length
   (vpx_reproject_moments' hist_out), else .w is only carried through.
   Step V, the variance estimate.  A pixel q with an invalid key: var0 = 0.  Else the moments of a
   pixel r are (m1, m2)(r) = mom[r], or (lum(in[r]), lum(in[r]) * lum(in[r])) when mom == NULL, and
     temporal arm (mom != NULL and in[q].w >= min_history; a NaN fails): v = m2(q) - m1(q) * m1(q);
     spatial arm (otherwise): over the taps (x + i, y + j), j = -2..2 outer, i = -2..2 inner, inside
       the image and carrying q's key: s1 = s1 + m1(r), s2 = s2 + m2(r), cnt = cnt + 1.0f; then
       mean = s1 / cnt, v = s2 / cnt - mean * mean;
     var0(q) = v > 0.0f ? v : 0.0f (a NaN gives 0).
   Pass p (step s = 1 << p) reads image S and variance var, writes D and var'.  An invalid key keeps
   S(q) and var(q).  Otherwise:
     prefilter (sets the weight only): over the 3x3 taps at distance 1 (never dilated), j outer, i
       inner, inside the image and carrying q's key: g = G[|j|] * G[|i|], G = {0.5, 0.25};
       gs = gs + g * var(r), gw = gw + g; gv = gs / gw; tol = sigma_v * sqrtf(gv) + epsilon;
       inv = 1.0f / tol;
     taps: vpx_denoise_ids' 25 taps, same order, matching, same base weight h:
       dd = (lum(S(r)) - lum(S(q))) * inv; w = h / (1.0f + dd * dd); acc = acc + w * S(r) per
       channel; wsum = wsum + w; vacc = vacc + (w * w) * var(r);
     D(q).rgb = acc / wsum, var'(q) = vacc / (wsum * wsum).
   The last pass writes out = (D.rgb, in.w) and, when rgb8 is not NULL, its tonemap in the same
   launch.  A tap that does not match is never read into the arithmetic, colour and variance alike.
   Order, counters, device sets as vpx_denoise_ids; the scratch (keys and two float4 images whose
   .w is the variance) belongs to the context and grows with the size: VPX_E_NOMEM when that
   fails.  VPX_E_INVALID: vpx_denoise_ids' size and pointer refusals; passes outside 1..5; sigma_v
   or epsilon not finite and positive; min_history not integer-valued in 1..65536; nonzero flags or
   reserved; out == in, out == ids or out == mom.
   Limits: vpx_denoise_ids'; and a lighting change that the history has not seen yet reads as
   variance for max_history frames, which widens the tolerance there: the safe side. */
typedef struct vpx_denoise_var_params {  /* 32 bytes */
    uint32_t passes;              /* 1..5: steps 1, 2, 4, 8, 16 */
    float    sigma_v;             /* finite, > 0: the tolerance in standard deviations */
    float    epsilon;             /* finite, > 0: added to the tolerance (keeps dd finite at zero variance) */
    float    min_history;         /* integer-valued, 1..65536: in.w >= this takes the temporal variance */
    uint32_t flags;               /* 0 */
    uint32_t reserved[3];         /* 0 */
} vpx_denoise_var_params;
int vpx_reproject_moments(vpx_ctx* ctx, const vpx_frame_params* p /* only width, height */,
                          const uint32_t* ids_cur, const uint32_t* ids_prev, const float* cur, const float* hist_in,
                          const float* mom_in /* float2[W*H], DEVICE; NULL with hist_in */,
                          float* hist_out, float* mom_out /* float2[W*H], DEVICE */, uint32_t* rgb8 /* may be NULL */,
                          const vpx_reproject* r, const vpx_volume* cur_volumes, const vpx_volume* prev_volumes);
int vpx_reproject_moments_host(uint32_t width, uint32_t height, const uint32_t* ids_cur, const uint32_t* ids_prev,
                               const float* cur, const float* hist_in, const float* mom_in, float* hist_out,
                               float* mom_out, uint32_t* rgb8 /* may be NULL */, const vpx_reproject* r,
                               const vpx_volume* cur_volumes, const vpx_volume* prev_volumes);
int vpx_denoise_var(vpx_ctx* ctx, const vpx_frame_params* p /* only width, height */,
                    const uint32_t* ids /* uint4[W*H], DEVICE */,
                    const float* in /* float4[W*H], DEVICE; .w = history length when mom != NULL */,
                    const float* mom /* float2[W*H], DEVICE, may be NULL */, float* out /* float4[W*H], DEVICE */,
                    uint32_t* rgb8 /* uint32[W*H], DEVICE, may be NULL */, const vpx_denoise_var_params* d);
/* The same two on host memory (no device, no context): the CPU paths of the same code
   (csrc/vpx_denoise_var.hpp, csrc/vpx_reproject.hpp).  VPX_E_NOMEM when the scratch cannot be allocated. */
int vpx_denoise_var_host(uint32_t width, uint32_t height, const uint32_t* ids, const float* in, const float* mom,
                         float* out, uint32_t* rgb8 /* may be NULL */, const vpx_denoise_var_params* d);
/* Focus ray of Renderer::Tick (world-space ray against every Scene::FindNearest). */
int vpx_focus_distance(vpx_ctx* ctx, uint32_t width, uint32_t height, float* focal_distance);

/* ---- BasicBVH (src/BVH/BasicBVH.{h,cpp}) ----------------------- */
/* The reference's triangle BVH: midpoint split on the longest axis, leaves of <= 2
   triangles, recursive left-then-right traversal that only shortens Ray::t.  A Renderer
   member (renderer.h:220) that Renderer::Trace does not call; offered as the reference
   offers it.  The device traversal stages the whole BVH (nodes, triangles, indices) in
   LDS per workgroup, one ray per lane. */
#define VPX_BVH_MAX_TRIS 512
#define VPX_BVH_MAX_DEPTH 63   /* deepest tree the device traversal stack holds (root = 1) */
typedef struct vpx_bvh_tri {       /* Tri (BasicBVH.h:3-7) without the centroid */
    float v0[3], v1[3], v2[3];
} vpx_bvh_tri;                     /* 36 bytes */
typedef struct vpx_bvh_node {      /* BVHNode (BasicBVH.h:11-20) */
    float aabb_min[3], aabb_max[3];
    uint32_t left_first, tri_count;
} vpx_bvh_node;                    /* 32 bytes */
/* Build (vpx_bvh_build_host) and upload the BVH of n triangles (1..VPX_BVH_MAX_TRIS;
   n = 0 removes it).  The midpoint split has no depth cap (as the reference's recursion):
   a tree deeper than VPX_BVH_MAX_DEPTH (vpx_bvh_depth) is refused with VPX_E_INVALID. */
int vpx_bvh_set(vpx_ctx* ctx, const vpx_bvh_tri* tris, uint32_t n);
/* IntersectBVH(ray, 0) per ray: rays built as in vpx_find_nearest (Ray(O, D) normalises D,
   t = tmax); t_out[i] = ray.t afterwards (tmax when nothing closer is hit). */
int vpx_bvh_intersect(vpx_ctx* ctx, const vpx_ray* rays, uint32_t n, float* t_out);

/* ---- host-side helpers restating reference host code (no device work) -------------- */
/* Camera basis exactly as Camera::HandleInput(0) leaves it (camera.h:121-178). */
int vpx_camera_look_at(const float pos[3], const float target[3], uint32_t width,
                       uint32_t height, vpx_camera* out);
/* Scene::SetCubeBoundaries + Scene::SetTransform (scene.cpp:213-217, 373-405). */
int vpx_volume_set_transform(const float position[3], const float scale[3],
                             const float rotation[3], vpx_volume* out);
/* Camera::HandleInput(0) basis + SetFrustumNormals + CopyToPrevCamera
   (camera.h:53-66, 113-181; renderer.cpp:710-711, 1893-1902). */
int vpx_prev_camera_look_at(const float pos[3], const float target[3], uint32_t width, uint32_t height,
                            vpx_prev_camera* out);
/* Renderer::MaterialSetUp table, padded to 256 entries (renderer.cpp:357-443). */
int vpx_default_materials(vpx_material* out256);
/* Per-pixel xorshift32 state used by vpx_render: 0x12345678 + WangHash((k+1)*17),
   k = seed_base + frame_index*W*H + y*W + x  (InitSeed, template/tmpl8math.cpp:35-38). */
uint32_t vpx_pixel_seed(uint32_t seed_base, uint32_t frame_index, uint32_t width,
                        uint32_t height, uint32_t x, uint32_t y);
/* BasicBVH::BuildBVH (BasicBVH.cpp:72-136): nodes needs 2n-1 entries, tri_idx n; the
   number of nodes used is stored in *nodes_used. */
int vpx_bvh_build_host(const vpx_bvh_tri* tris, uint32_t n, vpx_bvh_node* nodes, uint32_t* tri_idx,
                       uint32_t* nodes_used);
/* MagicaVoxel .vox (versions 150 / 200) decoded as ogt_vox v0.997 hands it to
   Scene::LoadModel (template/scene.cpp:449-529: read_scene_with_flags(buf, n, 0)->models[0]
   and ->palette): size_out = (size_x, size_y, size_z); voxels (if not NULL, capacity
   voxels_cap >= sx*sy*sz) = voxel_data, index x + y*sx + z*sx*sy, palette index, 0 = empty,
   after the IMAP remap; palette_rgba (if not NULL) = 256 RGBA, voxel byte k's colour at
   4k.  voxels == palette_rgba == NULL only queries the size.  VPX_E_INVALID for a malformed
   file, VPX_E_STATE when a palette is asked of a file without an RGBA chunk (MagicaVoxel's
   built-in default palette is not carried). */
int vpx_vox_decode(const uint8_t* data, uint64_t len, uint32_t size_out[3], uint8_t* voxels,
                   uint64_t voxels_cap, uint8_t palette_rgba[1024]);
/* vpx_grid_load_model on the host (no device): cells = n^3 bytes.  The CPU path of the same
   code (csrc/vpx_model.hpp); a model dimension outside 1..256 is VPX_E_INVALID too. */
int vpx_model_place_host(const uint8_t* voxels, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n,
                         const vpx_model_load* in, uint8_t* cells, vpx_model_result* out);
/* The xorshift32 state (13, 17, 5: RandomUInt, tmpl8math.cpp:119-125) after `steps` steps,
   by the jump: the step is linear over GF(2), so T^steps is a product of the T^(2^j). */
uint32_t vpx_xorshift32_jump(uint32_t state, uint64_t steps);
/* vpx_grid_generate_noise on the host (no device): cells = n^3 bytes.  The CPU path of the same
   code (csrc/vpx_noise.hpp), block by block with the prefix and the jump like the kernels. */
int vpx_noise_generate_host(uint32_t n, const vpx_noise_gen* in, uint8_t* cells, vpx_noise_result* out);
/* One sample of the noise field: gradient noise on the integer lattice, float32 throughout,
   exactly 0 on lattice points. */
float vpx_perlin3(int32_t seed, float x, float y, float z);
/* LoadModel's palette override (scene.cpp:516-520) on a 256-entry table: every index used
   by a non-empty voxel gets albedo = rgb / 255.0f and roughness 1. */
int vpx_model_palette_materials(vpx_material* mats256, const uint8_t* voxels, uint64_t count,
                                const uint8_t palette_rgba[1024]);
/* Depth of a tree built by vpx_bvh_build_host (a leaf root = 1; 0 when nodes_used == 0). */
uint32_t vpx_bvh_depth(const vpx_bvh_node* nodes, uint32_t nodes_used);
/* BasicBVH::BasicBVH() triangle set (BasicBVH.cpp:4-16): 64 triangles, vertex0 = r0*9-5,
   vertex1 = vertex0+r1, vertex2 = vertex0+r2, each r a float3 of RandomFloat() from the
   xorshift32 state *seed (advanced; the three draws of a float3 taken left to right —
   C++ leaves that order unspecified). */
int vpx_bvh_random_tris(uint32_t* seed, vpx_bvh_tri out[64]);
/* The world box the device culls a volume's walks with (no reference counterpart: the
   reference sets up every volume in Renderer::FindNearest / IsOccluded, renderer.cpp:209-243,
   946-1018): out = (lo x, y, z, hi x, y, z), the box of the cube b0..b1's corners mapped by the
   inverse of the affine part of inv_matrix (rows 0-2, as TransformPosition reads it), padded by
   0.1 % of the half-diagonal + 1e-3 of the scale and rounded outward; +-inf when the 3x3 part
   is singular (never culled).  A ray's segment [0, t] that misses the box reads no cell of the
   volume in the reference's loop. */
int vpx_volume_bounds(const vpx_volume* v, float out[6]);

#ifdef __cplusplus
}
#endif
#endif /* VPX_H_ */
