"""ctypes mirror of include/vpx.h and the loader for libvpx_hip.so.

The library is the product: there is no fallback.  `load_library()` raises when the
shared object is missing or does not export the ABI version this module expects.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvpx_hip.so")
ABI_VERSION = 2  # 2: vpx_profile 160 B (stage_busy_ms), packed tiles in 8x8 quadrants

VPX_OK = 0
VPX_E_INVALID, VPX_E_DEVICE, VPX_E_NOMEM, VPX_E_STATE = -1, -2, -3, -4  # include/vpx.h status codes
VPX_FLAG_AA = 0x1
VPX_FLAG_DOF = 0x2
VPX_FLAG_NO_TONEMAP = 0x4
VPX_ARITH_EXACT, VPX_ARITH_X86_HOST = 0, 1  # vpx_set_arithmetic modes
VPX_FLAG_SKY = 0x8  # activateSky: misses sample the vpx_set_sky texture (renderer.cpp:2308-2326)
MAT_NONE = 255
SKY_DEFAULT = (0.392, 0.584, 0.829)  # SampleSky with activateSky == false, renderer.cpp:2310-2313

f3 = C.c_float * 3


class Volume(C.Structure):
    _fields_ = [("grid_id", C.c_uint32), ("reserved", C.c_uint32), ("matrix", C.c_float * 16),
                ("inv_matrix", C.c_float * 16), ("b0", f3), ("b1", f3)]


class Material(C.Structure):
    _fields_ = [("albedo", f3), ("roughness", C.c_float), ("emissive", C.c_float), ("ior", C.c_float),
                ("pad", C.c_float * 2)]


class PointLight(C.Structure):
    _fields_ = [("position", f3), ("color", f3)]


class SpotLight(C.Structure):
    _fields_ = [("position", f3), ("direction", f3), ("color", f3), ("angle", C.c_float)]


class AreaLight(C.Structure):
    _fields_ = [("position", f3), ("color", f3), ("color_multiplier", C.c_float), ("radius", C.c_float)]


class DirLight(C.Structure):
    _fields_ = [("direction", f3), ("color", f3)]


class Sphere(C.Structure):
    _fields_ = [("center", f3), ("radius", C.c_float), ("material", C.c_uint32), ("pad", C.c_uint32 * 3)]


class Triangle(C.Structure):
    _fields_ = [("position", f3), ("v0", f3), ("v1", f3), ("v2", f3), ("material", C.c_uint32),
                ("pad", C.c_uint32 * 3)]


class Camera(C.Structure):
    _fields_ = [("cam_pos", f3), ("top_left", f3), ("top_right", f3), ("bottom_left", f3), ("right", f3),
                ("up", f3), ("focal_distance", C.c_float), ("defocus_jitter", C.c_float)]


class FrameParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("max_bounces", C.c_int32),
                ("frame_index", C.c_uint32), ("seed_base", C.c_uint32), ("flags", C.c_uint32),
                ("aa_strength", C.c_float), ("area_samples", C.c_int32), ("sky", f3), ("reserved", C.c_uint32)]


class Ray(C.Structure):
    _fields_ = [("origin", f3), ("direction", f3), ("tmax", C.c_float), ("inside_glass", C.c_uint32)]


class Hit(C.Structure):
    _fields_ = [("t", C.c_float), ("normal", f3), ("vox_index", C.c_int32), ("material", C.c_uint32),
                ("cells", C.c_uint32), ("inside_glass", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("shadow_rays", C.c_uint64), ("bounce_rays", C.c_uint64),
                ("dda_cells", C.c_uint64), ("kernel_ms", C.c_float), ("total_ms", C.c_float)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PlayerLight(C.Structure):  # vpx_player_light: Renderer::inLight (renderer.h:231) and what is behind it
    _fields_ = [("probes", C.c_uint64), ("lit", C.c_uint64), ("max_sqr", C.c_float), ("in_light", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class RayProbe(C.Structure):  # vpx_ray_probe: one ray's player light probes (vpx_trace_probe)
    _fields_ = [("probes", C.c_uint32), ("lit", C.c_uint32), ("max_sqr", C.c_float), ("reserved", C.c_uint32)]


PLAYER_LIGHT_SQR = 16.0  # VPX_PLAYER_LIGHT_SQR: sqrThreshold, renderer.cpp:1233, 1443


class RayFilter(C.Structure):  # vpx_ray_filter: which volumes, which materials pass, VPX_QUERY_* flags
    _fields_ = [("first_volume", C.c_uint32), ("mat_lo", C.c_uint32), ("mat_hi", C.c_uint32), ("flags", C.c_uint32)]


QUERY_NO_SHAPES = 0x1      # VPX_QUERY_NO_SHAPES: no spheres / triangles (FindNearestPlayer, IsOccludedPlayerClimbable)
QUERY_RAW_DIRECTION = 0x2  # VPX_QUERY_RAW_DIRECTION: direction used as given (the five-argument Ray constructor)
MAT_SMOKE_LOW_DENSITY, MAT_SMOKE_PLAYER = 9, 14  # VPX_MAT_SMOKE_*: the range FindNearestPlayer passes through


class HitCell(C.Structure):  # vpx_hit_cell: the hit cell and the face the walk entered it through
    _fields_ = [("cell", C.c_int32 * 3), ("grid_id", C.c_uint32), ("face_cell", C.c_int32 * 3), ("flags", C.c_uint32)]


CELL_HIT, CELL_FACE, CELL_FACE_IN = 0x1, 0x2, 0x4  # VPX_CELL_*; flags also hold axis << 8 | (step < 0) << 10


class Cast(C.Structure):  # vpx_cast: the form of a device ray batch (vpx_cast_nearest / vpx_cast_occluded) and its wave cap
    _fields_ = [("flags", C.c_uint32), ("max_waves", C.c_uint32), ("reserved", C.c_uint32 * 2)]


CAST_PER_LANE, CAST_POOL = 0x1, 0x2  # VPX_CAST_*: one thread per ray / persistent waves that refill (one visited volume)


class Denoise(C.Structure):  # vpx_denoise: passes 1..5 (steps 1..16), sigma_l (0: plane key only), flags, reserved
    _fields_ = [("passes", C.c_uint32), ("sigma_l", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class DenoiseVar(C.Structure):  # vpx_denoise_var: passes 1..5, the tolerance in standard deviations, its floor, the arm's threshold
    _fields_ = [("passes", C.c_uint32), ("sigma_v", C.c_float), ("epsilon", C.c_float), ("min_history", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 3)]


def denoise_var(passes=5, sigma_v=4.0, epsilon=2.0**-10, min_history=4):
    """abi.DenoiseVar with Renderer's defaults."""
    return DenoiseVar(int(passes), float(sigma_v), float(epsilon), float(min_history), 0, (C.c_uint32 * 3)(0, 0, 0))


LOAD_FULL, LOAD_PARTIAL, LOAD_RANDOM = 0, 1, 2  # VPX_LOAD_*: Scene::LoadModel / LoadModelPartial / LoadModelRandomMaterials


class ModelLoad(C.Structure):  # vpx_model_load: one placement of a resident model (vpx_grid_load_model)
    _fields_ = [("scale_model", f3), ("mode", C.c_uint32), ("columns", C.c_uint32), ("thickness", C.c_uint32),
                ("seed", C.c_uint32), ("rand_lo", C.c_float), ("rand_hi", C.c_float), ("reserved", C.c_uint32)]


class ModelResult(C.Structure):  # vpx_model_result: Scene::scaleModel and the xorshift32 state after the load
    _fields_ = [("scale_model", f3), ("seed", C.c_uint32)]


def model_load(mode=LOAD_FULL, scale_model=(1.0, 1.0, 1.0), columns=0, thickness=0, seed=0, rand_lo=12.0,
               rand_hi=13.0):
    """abi.ModelLoad; the defaults of the random range are the reference's
    Rand(SMOKE_MID2_DENSITY, SMOKE_HIGH_DENSITY) (scene.cpp:661-662)."""
    return ModelLoad(vec3(scale_model), int(mode), int(columns) & 0xFFFFFFFF, int(thickness) & 0xFFFFFFFF,
                     int(seed) & 0xFFFFFFFF, float(rand_lo), float(rand_hi), 0)


GEN_NOISE, GEN_SMOKE = 0, 1  # VPX_GEN_*: Scene::GenerateSomeNoise / GenerateSomeSmoke


class NoiseGen(C.Structure):  # vpx_noise_gen: one generator call (vpx_grid_generate_noise)
    _fields_ = [("mode", C.c_uint32), ("frequency", C.c_float), ("seed", C.c_uint32), ("reserved", C.c_uint32)]


class NoiseResult(C.Structure):  # vpx_noise_result: the state left behind, the field's seed, every RandomUInt of the call
    _fields_ = [("seed", C.c_uint32), ("noise_seed", C.c_uint32), ("draws", C.c_uint64)]


def noise_gen(mode=GEN_NOISE, frequency=0.03, seed=0x12345678):
    """abi.NoiseGen; the default frequency is GenerateSomeNoise's (scene.cpp:226)."""
    return NoiseGen(int(mode), float(frequency), int(seed) & 0xFFFFFFFF, 0)


BRUSH_SPHERE, BRUSH_BOX = 0, 1  # VPX_BRUSH_*


class Brush(C.Structure):  # vpx_brush: one sphere or box of cells, the byte written and the filter (vpx_grid_brush)
    _fields_ = [("shape", C.c_uint32), ("center", C.c_int32 * 3), ("r2", C.c_uint32), ("lo", C.c_int32 * 3),
                ("hi", C.c_int32 * 3), ("value", C.c_uint8), ("match_lo", C.c_uint8), ("match_hi", C.c_uint8),
                ("reserved", C.c_uint8)]


class BrushResult(C.Structure):  # vpx_brush_result: cells changed, bricks whose emptiness flipped
    _fields_ = [("changed", C.c_uint64), ("flipped", C.c_uint32), ("reserved", C.c_uint32)]


STAMP_GRID_BYTES, STAMP_CONSTANT = 1, 2  # VPX_STAMP_*
ORIENT_IDENTITY, ORIENT_LOAD_MODEL = 0x24, 0x18  # VPX_ORIENT_*


class Stamp(C.Structure):  # vpx_stamp: one resident model, where and how turned, the filter (vpx_grid_stamp)
    _fields_ = [("model_id", C.c_uint32), ("origin", C.c_int32 * 3), ("orient", C.c_uint32), ("flags", C.c_uint32),
                ("value", C.c_uint8), ("match_lo", C.c_uint8), ("match_hi", C.c_uint8), ("reserved", C.c_uint8),
                ("reserved2", C.c_uint32)]


class StampSource(C.Structure):  # vpx_stamp_source: a model in host memory (vpx_stamp_apply_host)
    _fields_ = [("voxels", C.c_void_p), ("sx", C.c_uint32), ("sy", C.c_uint32), ("sz", C.c_uint32),
                ("reserved", C.c_uint32)]


class PrevCamera(C.Structure):
    _fields_ = [("cam_pos", f3), ("left_normal", f3), ("right_normal", f3), ("top_normal", f3),
                ("bottom_normal", f3), ("pad", C.c_float)]


class Reproject(C.Structure):  # vpx_reproject: the two cameras, the history cap, the materials without history
    _fields_ = [("cur", Camera), ("prev", PrevCamera), ("max_history", C.c_float), ("nohist_lo", C.c_uint32),
                ("nohist_hi", C.c_uint32), ("n_volumes", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Profile(C.Structure):
    _fields_ = [("stage_ms", C.c_float * 8), ("stage_launches", C.c_uint32 * 8), ("stage_cells", C.c_uint64 * 8),
                ("stage_busy_ms", C.c_float * 8)]


class BvhTri(C.Structure):  # vpx_bvh_tri: BasicBVH Tri (BasicBVH.h:3-7) without the centroid
    _fields_ = [("v0", C.c_float * 3), ("v1", C.c_float * 3), ("v2", C.c_float * 3)]


class BvhNode(C.Structure):  # vpx_bvh_node: BVHNode (BasicBVH.h:11-20)
    _fields_ = [("aabb_min", C.c_float * 3), ("aabb_max", C.c_float * 3), ("left_first", C.c_uint32),
                ("tri_count", C.c_uint32)]


BVH_MAX_TRIS = 512
BVH_MAX_DEPTH = 63

STAGES = ("primary", "shade", "shadow", "resolve", "bounce", "finish", "frame", "instances")

STRUCT_SIZES = {PrevCamera: 64, Profile: 160, Volume: 160, Material: 32, PointLight: 24, SpotLight: 40, AreaLight: 32, DirLight: 24,
                Sphere: 32, Triangle: 64, Camera: 80, FrameParams: 48, Ray: 32, Hit: 32, Stats: 40,
                BvhTri: 36, BvhNode: 32, PlayerLight: 24, RayProbe: 16, RayFilter: 16, HitCell: 32, ModelLoad: 40, ModelResult: 16,
                NoiseGen: 16, NoiseResult: 16, Brush: 48, BrushResult: 16, Denoise: 16, Cast: 16, Reproject: 168,
                DenoiseVar: 32, Stamp: 32, StampSource: 24}


def np_dtype(struct):
    """numpy dtype with the exact layout of a ctypes Structure (for record arrays)."""
    return np.dtype(struct)


def as_ptr(arr, struct=None):
    if arr is None:
        return None
    if struct is not None:
        return arr.ctypes.data_as(C.POINTER(struct))
    return arr.ctypes.data_as(C.c_void_p)


# name -> (restype, argtypes); every symbol include/vpx.h declares
SIGNATURES = {
    "vpx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "vpx_create_multi": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_void_p)]),
    "vpx_destroy": (C.c_int, [C.c_void_p]),
    "vpx_last_error": (C.c_char_p, [C.c_void_p]),
    "vpx_abi_version": (C.c_int, []),
    "vpx_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "vpx_synchronize": (C.c_int, [C.c_void_p]),
    "vpx_set_pipeline": (C.c_int, [C.c_void_p, C.c_uint32]),
    "vpx_gl_register_buffer": (C.c_int, [C.c_void_p, C.c_uint]),
    "vpx_gl_map": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "vpx_gl_unmap": (C.c_int, [C.c_void_p]),
    "vpx_upload_grid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32]),
    "vpx_generate_tiled_grid": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p] + [C.c_uint32] * 7),
    "vpx_grid_checksum": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64)]),
    "vpx_grid_axis_planes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "vpx_grid_wide_planes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64]),
    "vpx_set_volumes": (C.c_int, [C.c_void_p, C.POINTER(Volume), C.c_uint32]),
    "vpx_set_materials": (C.c_int, [C.c_void_p, C.POINTER(Material), C.c_uint32]),
    "vpx_set_lights": (C.c_int, [C.c_void_p, C.POINTER(PointLight), C.c_uint32, C.POINTER(SpotLight), C.c_uint32,
                                 C.POINTER(AreaLight), C.c_uint32, C.POINTER(DirLight)]),
    "vpx_set_shapes": (C.c_int, [C.c_void_p, C.POINTER(Sphere), C.c_uint32, C.POINTER(Triangle), C.c_uint32]),
    "vpx_set_camera": (C.c_int, [C.c_void_p, C.POINTER(Camera)]),
    "vpx_set_sky": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float]),
    "vpx_render": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "vpx_render_tiles": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_uint32, C.c_uint32, C.c_uint32,
                                   C.c_uint32, C.c_void_p, C.POINTER(Stats)]),
    "vpx_render_tiles_accum": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Stats)]),
    "vpx_composite_rgb8": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p]),
    "vpx_render_window": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_uint32, C.c_void_p, C.c_void_p]),
    "vpx_render_tiles_accum_window": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "vpx_tiles_packed_len": (C.c_uint64, [C.c_uint32] * 5),
    "vpx_composite_tiles": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_void_p]),
    "vpx_get_counters": (C.c_int, [C.c_void_p, C.POINTER(Stats), C.c_int]),
    "vpx_grid_fill": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint8]),
    "vpx_grid_write_box": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 6),
    "vpx_grid_emissive_sphere": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint8, C.c_float]),
    "vpx_render_reproject": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.POINTER(PrevCamera), C.c_void_p,
                                       C.c_void_p, C.POINTER(Stats)]),
    "vpx_prev_camera_look_at": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32,
                                          C.POINTER(PrevCamera)]),
    "vpx_profile_enable": (C.c_int, [C.c_void_p, C.c_uint32]),
    "vpx_profile_select": (C.c_int, [C.c_void_p, C.c_uint32]),
    "vpx_profile_read": (C.c_int, [C.c_void_p, C.POINTER(Profile), C.c_int]),
    "vpx_profile_busy_union": (C.c_float, [C.POINTER(C.c_float), C.c_uint32]),
    "vpx_debug_last_frame_kernel": (C.c_int, [C.c_void_p]),
    "vpx_debug_live_buffers": (C.c_uint64, []),
    "vpx_find_nearest": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_uint32, C.POINTER(Hit)]),
    "vpx_is_occluded": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_uint32, C.c_void_p]),
    "vpx_trace": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_float),
                            C.c_int32, C.c_void_p]),
    "vpx_trace_probe": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_void_p, C.c_uint32, C.c_int32, C.POINTER(C.c_float),
                                  C.c_int32, C.c_void_p, C.POINTER(RayProbe)]),
    "vpx_get_player_light": (C.c_int, [C.c_void_p, C.POINTER(PlayerLight), C.c_int]),
    "vpx_find_nearest_filtered": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_uint32, C.POINTER(RayFilter), C.POINTER(Hit)]),
    "vpx_is_occluded_filtered": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_uint32, C.POINTER(RayFilter), C.c_void_p]),
    "vpx_find_nearest_cells": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_uint32, C.POINTER(RayFilter), C.POINTER(Hit),
                                         C.POINTER(HitCell)]),
    "vpx_pick_pixel": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [C.POINTER(RayFilter), C.POINTER(Hit), C.POINTER(HitCell)]),
    "vpx_render_ids": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.POINTER(RayFilter), C.c_void_p]),
    "vpx_cast_nearest": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RayFilter), C.POINTER(Cast), C.c_void_p,
                                   C.c_void_p]),
    "vpx_cast_occluded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(RayFilter), C.POINTER(Cast), C.c_void_p]),
    "vpx_debug_last_cast_kernel": (C.c_int, [C.c_void_p]),
    "vpx_denoise_ids": (C.c_int, [C.c_void_p, C.POINTER(FrameParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.POINTER(Denoise)]),
    "vpx_denoise_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.POINTER(Denoise)]),
    "vpx_reproject_ids": (C.c_int, [C.c_void_p, C.POINTER(FrameParams)] + [C.c_void_p] * 6 +
                          [C.POINTER(Reproject), C.POINTER(Volume), C.POINTER(Volume)]),
    "vpx_reproject_ids_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 +
                               [C.POINTER(Reproject), C.POINTER(Volume), C.POINTER(Volume)]),
    "vpx_reproject_moments": (C.c_int, [C.c_void_p, C.POINTER(FrameParams)] + [C.c_void_p] * 8 +
                              [C.POINTER(Reproject), C.POINTER(Volume), C.POINTER(Volume)]),
    "vpx_reproject_moments_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 8 +
                                   [C.POINTER(Reproject), C.POINTER(Volume), C.POINTER(Volume)]),
    "vpx_denoise_var": (C.c_int, [C.c_void_p, C.POINTER(FrameParams)] + [C.c_void_p] * 5 + [C.POINTER(DenoiseVar)]),
    "vpx_denoise_var_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 + [C.POINTER(DenoiseVar)]),
    "vpx_focus_distance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "vpx_camera_look_at": (C.c_int, [C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32, C.c_uint32,
                                     C.POINTER(Camera)]),
    "vpx_volume_set_transform": (C.c_int, [C.POINTER(C.c_float)] * 3 + [C.POINTER(Volume)]),
    "vpx_volume_bounds": (C.c_int, [C.POINTER(Volume), C.POINTER(C.c_float)]),
    "vpx_default_materials": (C.c_int, [C.POINTER(Material)]),
    "vpx_pixel_seed": (C.c_uint32, [C.c_uint32] * 6),
    "vpx_bvh_set": (C.c_int, [C.c_void_p, C.POINTER(BvhTri), C.c_uint32]),
    "vpx_bvh_intersect": (C.c_int, [C.c_void_p, C.POINTER(Ray), C.c_uint32, C.POINTER(C.c_float)]),
    "vpx_bvh_build_host": (C.c_int, [C.POINTER(BvhTri), C.c_uint32, C.POINTER(BvhNode), C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32)]),
    "vpx_bvh_random_tris": (C.c_int, [C.POINTER(C.c_uint32), C.POINTER(BvhTri)]),
    "vpx_bvh_depth": (C.c_uint32, [C.POINTER(BvhNode), C.c_uint32]),
    "vpx_set_arithmetic": (C.c_int, [C.c_void_p, C.c_uint32]),
    "vpx_x86_arith_tables": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
    "vpx_x86_arith_verify": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint32)]),
    "vpx_vox_decode": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint64, C.c_void_p]),
    "vpx_model_upload": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 3),
    "vpx_grid_load_model": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(ModelLoad),
                                      C.POINTER(ModelResult)]),
    "vpx_model_place_host": (C.c_int, [C.c_void_p] + [C.c_uint32] * 4 + [C.POINTER(ModelLoad), C.c_void_p,
                                                                         C.POINTER(ModelResult)]),
    "vpx_grid_read_box": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p] + [C.c_uint32] * 6),
    "vpx_xorshift32_jump": (C.c_uint32, [C.c_uint32, C.c_uint64]),
    "vpx_model_palette_materials": (C.c_int, [C.POINTER(Material), C.c_void_p, C.c_uint64, C.c_void_p]),
    "vpx_grid_generate_noise": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(NoiseGen), C.POINTER(NoiseResult)]),
    "vpx_noise_generate_host": (C.c_int, [C.c_uint32, C.POINTER(NoiseGen), C.c_void_p, C.POINTER(NoiseResult)]),
    "vpx_perlin3": (C.c_float, [C.c_int32, C.c_float, C.c_float, C.c_float]),
    "vpx_grid_brush": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(Brush), C.c_uint32, C.POINTER(BrushResult)]),
    "vpx_brush_apply_host": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(Brush), C.c_uint32, C.POINTER(BrushResult)]),
    "vpx_grid_level_words": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64]),
    "vpx_grid_stamp": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(Stamp), C.c_uint32, C.POINTER(BrushResult)]),
    "vpx_stamp_apply_host": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(StampSource), C.c_uint32, C.POINTER(Stamp), C.c_uint32,
                                       C.POINTER(BrushResult)]),
    "vpx_model_capture": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32] + [C.c_uint32] * 6),
    "vpx_model_read": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]),
}

_LIB = None


class VpxError(RuntimeError):
    pass


def load_library(path=None):
    """Load libvpx_hip.so (in-tree) and bind every exported symbol.  Raises if absent."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or os.environ.get("VPX_LIB") or LIB_PATH
    if not os.path.exists(p):
        raise VpxError(f"{p} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    # One HIP runtime per process: torch's wheel bundles its own libamdhip64 (soname
    # libamdhip64.so.7, but needed by torch as libamdhip64.so).  Loaded first, the library would
    # bind /opt/rocm's copy and torch would then load a second runtime, after which the
    # library's first hipGetDeviceCount fails (measured on the box: vpx_create -> VPX_E_DEVICE).
    # With torch loaded first the library's DT_NEEDED resolves to torch's runtime by soname.
    try:
        import torch  # noqa: F401
    except ImportError:  # plain C-ABI use without torch: /opt/rocm's runtime only
        pass
    lib = C.CDLL(p)
    old_ok = os.environ.get("VPX_LIB_OLD") == "1"  # A/B runs against an earlier build (tools/gpu_ab.sh)
    for name, (res, args) in SIGNATURES.items():
        if old_ok and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError = the library does not export the ABI
        fn.restype = res
        fn.argtypes = args
    if lib.vpx_abi_version() != ABI_VERSION:
        raise VpxError(f"ABI version mismatch: library {lib.vpx_abi_version()} != {ABI_VERSION}")
    if path is None:
        _LIB = lib
    return lib


def check(lib, ctx, rc, what):
    if rc != VPX_OK:
        msg = lib.vpx_last_error(ctx).decode() if ctx else ""
        raise VpxError(f"{what} failed ({rc}): {msg}")


def vec3(v):
    return f3(*[float(x) for x in v])


def rays_tensor(rays, device):
    """A ctypes array of abi.Ray as the float32 torch tensor [n, 8] that cast_nearest / cast_occluded
    take (vpx_ray's layout; inside_glass carried as bits) on `device`: for tests and small callers."""
    import torch

    n = len(rays)
    host = np.frombuffer(rays, dtype=np.float32, count=8 * n).reshape(n, 8).copy() if n else np.zeros((0, 8), np.float32)
    return torch.from_numpy(host).to(device)


def sky_arg(sky):
    """vpx_trace's sky argument: a constant colour, or None = the uploaded sky texture."""
    return None if sky is None else vec3(sky)
