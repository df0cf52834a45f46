"""Python handle on one libvpx_hip.so context (one GPU).  Thin: every call is the C-ABI."""
import ctypes as C

import numpy as np

from . import abi


class Context:
    def __init__(self, device=0, devices=None):
        """One device (vpx_create), or a device set (vpx_create_multi: `devices` list, the
        frame tile-sharded over them and gathered to devices[0])."""
        self.lib = abi.load_library()
        h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self.lib.vpx_create_multi(arr, len(devices), C.byref(h))
            if rc != abi.VPX_OK:
                raise abi.VpxError(f"vpx_create_multi(devices={list(devices)}) failed ({rc})")
            device = int(devices[0])
        else:
            rc = self.lib.vpx_create(int(device), C.byref(h))
            if rc != abi.VPX_OK:
                raise abi.VpxError(f"vpx_create(device={device}) failed ({rc}): no usable HIP device")
        self.h = h
        self.device = device
        self.devices = list(devices) if devices is not None else [device]
        self.scene = None
        self.stream_handle = None

    # ------------------------------------------------------------------ lifetime
    def close(self):
        if self.h:
            self.lib.vpx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        abi.check(self.lib, self.h, rc, what)

    def set_stream(self, stream_handle):
        self._chk(self.lib.vpx_set_stream(self.h, C.c_void_p(stream_handle or 0)), "vpx_set_stream")
        self.stream_handle = stream_handle or None  # None: the context's own stream

    def synchronize(self):
        self._chk(self.lib.vpx_synchronize(self.h), "vpx_synchronize")

    def set_pipeline(self, depth):
        """Frames in flight (vpx_set_pipeline): 0 / 1 off, 2..4 lanes."""
        self._chk(self.lib.vpx_set_pipeline(self.h, int(depth)), "vpx_set_pipeline")

    def set_arithmetic(self, mode):
        """vpx_set_arithmetic: abi.VPX_ARITH_EXACT (default) or abi.VPX_ARITH_X86_HOST (the
        reference's rcpps+NR / rsqrtps as this host's CPU computes them)."""
        self._chk(self.lib.vpx_set_arithmetic(self.h, int(mode)), "vpx_set_arithmetic")

    # ------------------------------------------------------------------- scene
    def load_scene(self, desc, upload_grids=True):
        if upload_grids:
            for gid, g in enumerate(desc.grids):
                g.upload(self.lib, self.h, gid)
        self._chk(self.lib.vpx_set_volumes(self.h, desc.volumes, len(desc.volumes)), "vpx_set_volumes")
        self._chk(self.lib.vpx_set_materials(self.h, desc.materials, 256), "vpx_set_materials")
        pts = (abi.PointLight * max(1, len(desc.points)))(*desc.points)
        sps = (abi.SpotLight * max(1, len(desc.spots)))(*desc.spots)
        ars = (abi.AreaLight * max(1, len(desc.areas)))(*desc.areas)
        self._chk(self.lib.vpx_set_lights(self.h, pts, len(desc.points), sps, len(desc.spots), ars, len(desc.areas),
                                          C.byref(desc.dir_light)), "vpx_set_lights")
        sph = (abi.Sphere * max(1, len(desc.spheres)))(*desc.spheres)
        tri = (abi.Triangle * max(1, len(desc.triangles)))(*desc.triangles)
        self._chk(self.lib.vpx_set_shapes(self.h, sph, len(desc.spheres), tri, len(desc.triangles)),
                  "vpx_set_shapes")
        self.set_camera(desc.camera)
        self.set_sky(desc.sky_texture, desc.sky_hdr)
        self.scene = desc

    def set_sky(self, rgb, hdr_contribution=1.0):
        """Renderer::skyPixels (float32 (H, W, 3) equirectangular) + HDRLightContribution;
        None removes the texture."""
        if rgb is None:
            self._chk(self.lib.vpx_set_sky(self.h, None, 0, 0, float(hdr_contribution)), "vpx_set_sky")
            return
        a = np.ascontiguousarray(rgb, np.float32)
        h, w, ch = a.shape
        assert ch == 3, "sky texture must be (H, W, 3) RGB floats"
        self._chk(self.lib.vpx_set_sky(self.h, a.ctypes.data_as(C.c_void_p), w, h, float(hdr_contribution)),
                  "vpx_set_sky")

    def set_materials(self, materials):
        """Renderer::materials: a ctypes array of 256 abi.Material (vpx_set_materials)."""
        self._chk(self.lib.vpx_set_materials(self.h, materials, 256), "vpx_set_materials")

    def set_camera(self, cam):
        self._chk(self.lib.vpx_set_camera(self.h, C.byref(cam)), "vpx_set_camera")

    # ------------------------------------------------------------ world edits
    def grid_fill(self, grid_id, value):
        """Scene::ResetGrid(type) (template/scene.cpp:356-359) on the device copy."""
        self._chk(self.lib.vpx_grid_fill(self.h, grid_id, int(value)), "vpx_grid_fill")

    def grid_write_box(self, grid_id, box, origin):
        """Dirty-region upload: box = uint8 array (dz, dy, dx) written at origin (x0, y0, z0)."""
        b = np.ascontiguousarray(box, np.uint8)
        dz, dy, dx = b.shape
        x0, y0, z0 = origin
        self._chk(self.lib.vpx_grid_write_box(self.h, grid_id, b.ctypes.data_as(C.c_void_p), x0, y0, z0, dx, dy, dz),
                  "vpx_grid_write_box")

    def grid_emissive_sphere(self, grid_id, mat, radius):
        """Scene::CreateEmmisiveSphere(mat, radius) (template/scene.cpp:685-711)."""
        self._chk(self.lib.vpx_grid_emissive_sphere(self.h, grid_id, int(mat), float(radius)),
                  "vpx_grid_emissive_sphere")

    def grid_brush(self, grid_id, brushes):
        """Device-side edit (vpx_grid_brush): a list of abi.Brush (scene.sphere_brush / box_brush)
        applied in order, then one region-local refresh of the levels.  Returns the
        abi.BrushResult: cells changed, bricks whose emptiness flipped."""
        arr = (abi.Brush * max(1, len(brushes)))(*brushes)
        res = abi.BrushResult()
        self._chk(self.lib.vpx_grid_brush(self.h, grid_id, arr, len(brushes), C.byref(res)), "vpx_grid_brush")
        return res

    def grid_stamp(self, grid_id, stamps):
        """Device-side edit (vpx_grid_stamp): a list of abi.Stamp (scene.stamp) gathered into the
        grid in order, then one region-local refresh of the levels.  Returns the abi.BrushResult:
        cells changed, bricks whose emptiness flipped."""
        arr = (abi.Stamp * max(1, len(stamps)))(*stamps)
        res = abi.BrushResult()
        self._chk(self.lib.vpx_grid_stamp(self.h, grid_id, arr, len(stamps), C.byref(res)), "vpx_grid_stamp")
        return res

    def model_capture(self, model_id, grid_id, origin, shape):
        """Resident model model_id made from the cells of the box at origin (x0, y0, z0) of shape
        (dz, dy, dx), on the device (vpx_model_capture): raw grid bytes, so a stamp with
        abi.STAMP_GRID_BYTES puts them back."""
        dz, dy, dx = (int(s) for s in shape)
        x0, y0, z0 = (int(s) for s in origin)
        self._chk(self.lib.vpx_model_capture(self.h, model_id, grid_id, x0, y0, z0, dx, dy, dz), "vpx_model_capture")

    def model_read(self, model_id):
        """Debug read-back of a resident model (vpx_model_read): uint8 array of shape (sz, sy, sx)."""
        size = (C.c_uint32 * 3)()
        self._chk(self.lib.vpx_model_read(self.h, model_id, None, 0, size), "vpx_model_read")
        sx, sy, sz = (int(s) for s in size)
        out = np.empty((sz, sy, sx), np.uint8)
        self._chk(self.lib.vpx_model_read(self.h, model_id, out.ctypes.data_as(C.c_void_p), out.size, size), "vpx_model_read")
        return out

    def model_upload(self, model_id, size, voxels):
        """A resident model (vpx_model_upload): ogt_vox's voxel_data as scene.load_model returns
        it, size = (sx, sy, sz); voxels None removes it."""
        if voxels is None:
            self._chk(self.lib.vpx_model_upload(self.h, model_id, None, 0, 0, 0), "vpx_model_upload")
            return
        v = np.ascontiguousarray(voxels, np.uint8).reshape(-1)
        sx, sy, sz = (int(s) for s in size)
        assert v.size == sx * sy * sz, "voxels do not match the model size"
        self._chk(self.lib.vpx_model_upload(self.h, model_id, v.ctypes.data_as(C.c_void_p), sx, sy, sz),
                  "vpx_model_upload")

    def grid_load_model(self, grid_id, n, model_id, mode=abi.LOAD_FULL, scale_model=(1.0, 1.0, 1.0), columns=0,
                        thickness=0, seed=0, rand_lo=12.0, rand_hi=13.0, load=None):
        """Scene::LoadModel / LoadModelPartial / LoadModelRandomMaterials of a resident model into
        grid grid_id (n^3, created or resized as needed) on the device (vpx_grid_load_model).
        load: an abi.ModelLoad instead of the keywords.  Returns the abi.ModelResult:
        Scene::scaleModel as the call leaves it and the xorshift32 state after the draws."""
        ld = load if load is not None else abi.model_load(mode, scale_model, columns, thickness, seed, rand_lo, rand_hi)
        res = abi.ModelResult()
        self._chk(self.lib.vpx_grid_load_model(self.h, grid_id, int(n), model_id, C.byref(ld), C.byref(res)),
                  "vpx_grid_load_model")
        return res

    def grid_generate_noise(self, grid_id, n, mode=abi.GEN_NOISE, frequency=0.03, seed=0x12345678, gen=None):
        """Scene::GenerateSomeNoise / GenerateSomeSmoke into grid grid_id (n^3, created or resized
        as needed) on the device (vpx_grid_generate_noise).  gen: an abi.NoiseGen instead of the
        keywords.  Returns the abi.NoiseResult: the xorshift32 state the call leaves, the field's
        seed and the number of draws."""
        g = gen if gen is not None else abi.noise_gen(mode, frequency, seed)
        res = abi.NoiseResult()
        self._chk(self.lib.vpx_grid_generate_noise(self.h, grid_id, int(n), C.byref(g), C.byref(res)),
                  "vpx_grid_generate_noise")
        return res

    def grid_read_box(self, grid_id, origin, shape):
        """Debug read-back (vpx_grid_read_box): the cells of the box at origin (x0, y0, z0) as a
        uint8 array of shape (dz, dy, dx), the inverse of grid_write_box."""
        dz, dy, dx = (int(s) for s in shape)
        x0, y0, z0 = (int(s) for s in origin)
        out = np.empty((dz, dy, dx), np.uint8)
        self._chk(self.lib.vpx_grid_read_box(self.h, grid_id, out.ctypes.data_as(C.c_void_p), x0, y0, z0, dx, dy, dz),
                  "vpx_grid_read_box")
        return out

    def grid_checksum(self, grid_id=0):
        out = C.c_uint64()
        self._chk(self.lib.vpx_grid_checksum(self.h, grid_id, C.byref(out)), "vpx_grid_checksum")
        return out.value

    def grid_axis_planes(self, grid_id, n):
        """The 24 distance-field axis planes of an n^3 grid (debug read-back): uint16 (24, words per plane)."""
        nb2 = ((n + 3) // 4 + 3) // 4
        out = np.zeros((24, 64 * nb2 ** 3), np.uint16)
        self._chk(self.lib.vpx_grid_axis_planes(self.h, grid_id, out.ctypes.data_as(C.c_void_p), out.size),
                  "vpx_grid_axis_planes")
        return out

    def grid_wide_planes(self, grid_id, n):
        """The same planes' whole words, k | L << 8 | Mb << 16 | Mc << 24: uint32 (24, words per plane)."""
        nb2 = ((n + 3) // 4 + 3) // 4
        out = np.zeros((24, 64 * nb2 ** 3), np.uint32)
        self._chk(self.lib.vpx_grid_wide_planes(self.h, grid_id, out.ctypes.data_as(C.c_void_p), out.size),
                  "vpx_grid_wide_planes")
        return out

    def grid_level_words(self, grid_id, n, level):
        """The mask level 1 (bricks; an empty brick's word holds its distance-field bytes) or 2
        (macros) of an n^3 grid (debug read-back): uint64 words in blocked order."""
        nb = ((n + 3) // 4 + 3) // 4
        if level == 2:
            nb = (nb + 3) // 4
        out = np.zeros(64 * nb ** 3, np.uint64)
        self._chk(self.lib.vpx_grid_level_words(self.h, grid_id, int(level), out.ctypes.data_as(C.c_void_p), out.size),
                  "vpx_grid_level_words")
        return out

    # ---------------------------------------------------------------- hot path
    def render(self, params, accum_ptr, rgb_ptr=None, stats=False):
        st = abi.Stats() if stats else None
        self._chk(self.lib.vpx_render(self.h, C.byref(params), C.c_void_p(accum_ptr), C.c_void_p(rgb_ptr or 0),
                                      C.byref(st) if st is not None else None), "vpx_render")
        return st

    def render_reproject(self, params, prev, history_ptr, rgb_ptr=None, stats=False):
        """One frame of the static-camera path (vpx_render_reproject); history is a DEVICE
        float4[W*H] pointer (illuminationHistoryBuffer, updated in place)."""
        st = abi.Stats() if stats else None
        self._chk(self.lib.vpx_render_reproject(self.h, C.byref(params), C.byref(prev), C.c_void_p(history_ptr),
                                                C.c_void_p(rgb_ptr or 0), C.byref(st) if st is not None else None),
                  "vpx_render_reproject")
        return st

    def render_tiles(self, params, rank, n_ranks, packed_ptr, stats=False, tile=16):
        st = abi.Stats() if stats else None
        self._chk(self.lib.vpx_render_tiles(self.h, C.byref(params), tile, tile, rank, n_ranks,
                                            C.c_void_p(packed_ptr), C.byref(st) if st is not None else None),
                  "vpx_render_tiles")
        return st

    def render_tiles_accum(self, params, rank, n_ranks, accum_packed_ptr, rgb_packed_ptr, stats=False, tile=16):
        """This rank's tiles, accumulated into its own packed accumulator + packed RGB8."""
        st = abi.Stats() if stats else None
        self._chk(self.lib.vpx_render_tiles_accum(self.h, C.byref(params), tile, tile, rank, n_ranks,
                                                  C.c_void_p(accum_packed_ptr), C.c_void_p(rgb_packed_ptr),
                                                  C.byref(st) if st is not None else None), "vpx_render_tiles_accum")
        return st

    def render_window(self, params, n_frames, accum_ptr, rgb_ptr=None):
        """Frames params.frame_index .. + n_frames - 1 accumulated in order (vpx_render_window):
        the results of n_frames render() calls; small frames share one chain of launches."""
        self._chk(self.lib.vpx_render_window(self.h, C.byref(params), n_frames, C.c_void_p(accum_ptr),
                                             C.c_void_p(rgb_ptr or 0)), "vpx_render_window")

    def render_tiles_accum_window(self, params, n_frames, rank, n_ranks, accum_packed_ptr, rgb_packed_ptr, tile=16):
        """render_tiles_accum over an accumulation window (vpx_render_tiles_accum_window): the
        rank's share of several frames in one chain of launches."""
        self._chk(self.lib.vpx_render_tiles_accum_window(self.h, C.byref(params), n_frames, tile, tile, rank, n_ranks,
                                                         C.c_void_p(accum_packed_ptr), C.c_void_p(rgb_packed_ptr)),
                  "vpx_render_tiles_accum_window")

    def composite_rgb8(self, params, n_ranks, gathered_ptr, rgb_ptr, tile=16):
        self._chk(self.lib.vpx_composite_rgb8(self.h, C.byref(params), tile, tile, n_ranks, C.c_void_p(gathered_ptr),
                                              C.c_void_p(rgb_ptr)), "vpx_composite_rgb8")

    def packed_len(self, width, height, n_ranks, tile=16):
        return int(self.lib.vpx_tiles_packed_len(width, height, tile, tile, n_ranks))

    def composite_tiles(self, params, n_ranks, gathered_ptr, accum_ptr, rgb_ptr=None, tile=16):
        self._chk(self.lib.vpx_composite_tiles(self.h, C.byref(params), tile, tile, n_ranks, C.c_void_p(gathered_ptr),
                                               C.c_void_p(accum_ptr), C.c_void_p(rgb_ptr or 0)),
                  "vpx_composite_tiles")

    def profile_enable(self, max_launches):
        self._chk(self.lib.vpx_profile_enable(self.h, int(max_launches)), "vpx_profile_enable")

    def bvh_set(self, tris):
        """BasicBVH of `tris` (ctypes array of abi.BvhTri) built and uploaded (vpx_bvh_set)."""
        self._chk(self.lib.vpx_bvh_set(self.h, tris, len(tris)), "vpx_bvh_set")

    def bvh_intersect(self, rays):
        """BasicBVH::IntersectBVH per ray: float32 t after the traversal."""
        out = np.zeros(len(rays), np.float32)
        self._chk(self.lib.vpx_bvh_intersect(self.h, rays, len(rays), out.ctypes.data_as(C.POINTER(C.c_float))),
                  "vpx_bvh_intersect")
        return out

    def profile_select(self, stages=None):
        """Time only these stage names (abi.STAGES); None: all."""
        mask = 0xFFFFFFFF if stages is None else sum(1 << abi.STAGES.index(s) for s in stages)
        self._chk(self.lib.vpx_profile_select(self.h, mask), "vpx_profile_select")

    def profile_read(self, reset=True):
        """Per-stage device times / launches / DDA cells / busy time (the union of the launch
        intervals): {stage: (ms_total, launches, cells, busy_ms)}."""
        pr = abi.Profile()
        self._chk(self.lib.vpx_profile_read(self.h, C.byref(pr), 1 if reset else 0), "vpx_profile_read")
        return {name: (pr.stage_ms[i], pr.stage_launches[i], pr.stage_cells[i], pr.stage_busy_ms[i])
                for i, name in enumerate(abi.STAGES)}

    def last_frame_kernel(self):
        """Debug (vpx_debug_last_frame_kernel): the form of the one-launch depth-0 frame kernel the
        last render launched: 0 none, 1 specialised on its launch condition, 2 the lean form."""
        return int(self.lib.vpx_debug_last_frame_kernel(self.h))

    def live_buffers(self):
        """Debug (vpx_debug_live_buffers): device and pinned allocations the library holds, process-wide."""
        return int(self.lib.vpx_debug_live_buffers())

    def counters(self, reset=False):
        st = abi.Stats()
        self._chk(self.lib.vpx_get_counters(self.h, C.byref(st), 1 if reset else 0), "vpx_get_counters")
        return st

    def player_light(self, reset=False):
        """The player light record since the last reset (vpx_get_player_light): abi.PlayerLight
        with probes, lit, max_sqr and in_light = Renderer::inLight (renderer.h:231).  Synchronises."""
        pl = abi.PlayerLight()
        self._chk(self.lib.vpx_get_player_light(self.h, C.byref(pl), 1 if reset else 0), "vpx_get_player_light")
        return pl

    # ------------------------------------------------------------- unit entries
    def find_nearest(self, rays):
        n = len(rays)
        hits = (abi.Hit * max(1, n))()
        self._chk(self.lib.vpx_find_nearest(self.h, rays, n, hits), "vpx_find_nearest")
        return hits

    def is_occluded(self, rays):
        n = len(rays)
        occ = np.zeros(max(1, n), np.uint8)
        self._chk(self.lib.vpx_is_occluded(self.h, rays, n, occ.ctypes.data_as(C.c_void_p)), "vpx_is_occluded")
        return occ[:n]

    @staticmethod
    def ray_filter(first_volume=0, except_materials=None, shapes=True, raw_direction=False):
        """abi.RayFilter: except_materials = (lo, hi), the cells read and passed through; None: none."""
        lo, hi = (1, 0) if except_materials is None else except_materials
        flags = (0 if shapes else abi.QUERY_NO_SHAPES) | (abi.QUERY_RAW_DIRECTION if raw_direction else 0)
        return abi.RayFilter(int(first_volume), int(lo), int(hi), flags)

    def find_nearest_filtered(self, rays, first_volume=0, except_materials=None, shapes=True, raw_direction=False,
                              filter=None):
        """vpx_find_nearest_filtered: FindNearest over the volumes first_volume .. count-1 with the
        materials except_materials = (lo, hi) passed through (Scene::FindNearestExcept), without
        the spheres / triangles when shapes is False; raw_direction: direction used as given.
        filter: an abi.RayFilter instead of the keywords."""
        n = len(rays)
        hits = (abi.Hit * max(1, n))()
        f = filter if filter is not None else self.ray_filter(first_volume, except_materials, shapes, raw_direction)
        self._chk(self.lib.vpx_find_nearest_filtered(self.h, rays, n, C.byref(f), hits), "vpx_find_nearest_filtered")
        return hits

    def is_occluded_filtered(self, rays, first_volume=0, shapes=True, raw_direction=False, filter=None):
        """vpx_is_occluded_filtered: IsOccluded over the volumes first_volume .. count-1, without the
        spheres / triangles when shapes is False (Renderer::IsOccludedPlayerClimbable: 1, False)."""
        n = len(rays)
        occ = np.zeros(max(1, n), np.uint8)
        f = filter if filter is not None else self.ray_filter(first_volume, None, shapes, raw_direction)
        self._chk(self.lib.vpx_is_occluded_filtered(self.h, rays, n, C.byref(f), occ.ctypes.data_as(C.c_void_p)),
                  "vpx_is_occluded_filtered")
        return occ[:n]

    def find_nearest_cells(self, rays, first_volume=0, except_materials=None, shapes=True, raw_direction=False,
                           filter=None):
        """vpx_find_nearest_cells: find_nearest_filtered's hits plus, per ray, the abi.HitCell with the
        hit cell and the face the walk entered it through.  Returns (hits, cells), ctypes arrays
        (hits_to_numpy / cells_to_numpy)."""
        n = len(rays)
        hits = (abi.Hit * max(1, n))()
        cells = (abi.HitCell * max(1, n))()
        f = filter if filter is not None else self.ray_filter(first_volume, except_materials, shapes, raw_direction)
        self._chk(self.lib.vpx_find_nearest_cells(self.h, rays, n, C.byref(f), hits, cells), "vpx_find_nearest_cells")
        return hits, cells

    def pick_pixel(self, width, height, x, y, first_volume=0, except_materials=None, shapes=True, filter=None):
        """vpx_pick_pixel: the same query for the ray of integer pixel (x, y) (GetPrimaryRayNoDOF with the
        context's camera).  Returns (abi.Hit, abi.HitCell)."""
        hit, cell = abi.Hit(), abi.HitCell()
        f = filter if filter is not None else self.ray_filter(first_volume, except_materials, shapes, False)
        self._chk(self.lib.vpx_pick_pixel(self.h, int(width), int(height), int(x), int(y), C.byref(f), C.byref(hit),
                                          C.byref(cell)), "vpx_pick_pixel")
        return hit, cell

    def render_ids(self, params, filter=None):
        """vpx_render_ids: pick_pixel for every pixel, a torch int32 [H, W, 4] tensor on the
        context's device (unpack_ids reads it).  Runs on the context's stream, unsynchronised."""
        import torch

        out = torch.empty((int(params.height), int(params.width), 4), dtype=torch.int32,
                          device=f"cuda:{self.device}")
        self._chk(self.lib.vpx_render_ids(self.h, C.byref(params), C.byref(filter) if filter is not None else None,
                                          C.c_void_p(out.data_ptr())), "vpx_render_ids")
        return out

    unpack_ids = staticmethod(lambda ids: unpack_ids(ids))

    def _cast_args(self, rays, form, max_waves):
        import torch

        if not (isinstance(rays, torch.Tensor) and rays.dtype == torch.float32 and rays.dim() == 2
                and rays.shape[1] == 8 and rays.is_contiguous() and rays.is_cuda
                and rays.device.index == self.device):
            raise ValueError(f"rays: a contiguous float32 torch tensor [n, 8] on cuda:{self.device} (abi.rays_tensor)")
        return torch, int(rays.shape[0]), abi.Cast(int(form or 0), int(max_waves), (C.c_uint32 * 2)(0, 0))

    def cast_nearest(self, rays, first_volume=0, except_materials=None, shapes=True, raw_direction=False, filter=None,
                     cells=True, form=None, max_waves=0):
        """vpx_cast_nearest: find_nearest_cells for rays that already live on the device.  rays: a
        contiguous float32 torch tensor [n, 8] on the context's device with vpx_ray's layout
        (inside_glass as bits; abi.rays_tensor converts).  Returns (hits, cells): int32 tensors
        [n, 8] (unpack_hits / unpack_cells read them), cells None with cells=False.  form:
        abi.CAST_PER_LANE, abi.CAST_POOL or None (the library's choice); max_waves caps the pool's
        persistent waves.  Runs on the context's stream, unsynchronised; last_cast_kernel() tells
        which form ran.  torch orders and recycles tensors by ITS current stream: produce the rays,
        cast and read the results under torch.cuda.stream() of the stream given to set_stream, or
        keep the tensors alive and synchronize() before reading."""
        torch, n, opt = self._cast_args(rays, form, max_waves)
        f = filter if filter is not None else self.ray_filter(first_volume, except_materials, shapes, raw_direction)
        hits = torch.empty((n, 8), dtype=torch.int32, device=rays.device)
        cell = torch.empty((n, 8), dtype=torch.int32, device=rays.device) if cells else None
        self._chk(self.lib.vpx_cast_nearest(self.h, C.c_void_p(rays.data_ptr()), n, C.byref(f), C.byref(opt),
                                            C.c_void_p(hits.data_ptr()), C.c_void_p(cell.data_ptr()) if cells else None),
                  "vpx_cast_nearest")
        return hits, cell

    def cast_occluded(self, rays, first_volume=0, shapes=True, raw_direction=False, filter=None, form=None, max_waves=0):
        """vpx_cast_occluded: is_occluded_filtered for rays on the device (cast_nearest's tensor).
        Returns a uint8 tensor [n].  Runs on the context's stream, unsynchronised."""
        torch, n, opt = self._cast_args(rays, form, max_waves)
        f = filter if filter is not None else self.ray_filter(first_volume, None, shapes, raw_direction)
        occ = torch.empty((n,), dtype=torch.uint8, device=rays.device)
        self._chk(self.lib.vpx_cast_occluded(self.h, C.c_void_p(rays.data_ptr()), n, C.byref(f), C.byref(opt),
                                             C.c_void_p(occ.data_ptr())), "vpx_cast_occluded")
        return occ

    def last_cast_kernel(self):
        """vpx_debug_last_cast_kernel: 0 nothing launched, 1 the per-lane form, 2 the pool."""
        return int(self.lib.vpx_debug_last_cast_kernel(self.h))

    unpack_hits = staticmethod(lambda hits: unpack_hits(hits))
    unpack_cells = staticmethod(lambda cells: unpack_cells(cells))

    def denoise(self, params, ids, src, out=None, passes=5, sigma_l=0.0, rgb_ptr=None):
        """vpx_denoise_ids: the plane-keyed a-trous filter of `src` (a float32 torch tensor of
        4 * W * H elements on the context's device, e.g. a render accumulator) guided by `ids`
        (render_ids' tensor), `passes` passes (steps 1, 2, 4, ...), sigma_l 0 = plane key only.
        Returns `out` (allocated like src when None; never src itself); rgb_ptr: a device uint32[W*H]
        pointer that receives the tonemapped result.  Runs on the context's stream, unsynchronised."""
        import torch

        if out is None:
            out = torch.empty_like(src)
        d = abi.Denoise(int(passes), float(sigma_l), 0, 0)
        self._chk(self.lib.vpx_denoise_ids(self.h, C.byref(params), C.c_void_p(ids.data_ptr()),
                                           C.c_void_p(src.data_ptr()), C.c_void_p(out.data_ptr()),
                                           C.c_void_p(rgb_ptr or 0), C.byref(d)), "vpx_denoise_ids")
        return out

    def denoise_host(self, width, height, ids, src, passes=5, sigma_l=0.0, rgb=False):
        return denoise_host(width, height, ids, src, passes, sigma_l, rgb, lib=self.lib)

    def reproject(self, params, ids_cur, ids_prev, cur, hist_in, camera, prev_camera, out=None, max_history=32,
                  nohist=(1, 0), cur_volumes=None, prev_volumes=None, rgb_ptr=None):
        """vpx_reproject_ids: the previous frame's history `hist_in` (float32 torch tensor, 4 * W * H,
        .w the history length) carried from `prev_camera` (abi.PrevCamera) to `camera` (abi.Camera)
        and blended with this frame's samples `cur`, a history pixel taken only where its record in
        `ids_prev` has the key of the pixel's record in `ids_cur` (render_ids' tensors).  ids_prev
        and hist_in None together: no history yet.  nohist: the (lo, hi) range of first-hit materials
        that take none; cur_volumes / prev_volumes: sequences of abi.Volume when volumes move.
        Returns `out` (allocated like cur when None; never an input).  Runs on the context's stream,
        unsynchronised."""
        import torch

        if out is None:
            out = torch.empty_like(cur)
        r, cv, pv = reproject_desc(camera, prev_camera, max_history, nohist, cur_volumes, prev_volumes)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        self._chk(self.lib.vpx_reproject_ids(self.h, C.byref(params), ptr(ids_cur), ptr(ids_prev), ptr(cur), ptr(hist_in),
                                             ptr(out), C.c_void_p(rgb_ptr or 0), C.byref(r), cv, pv), "vpx_reproject_ids")
        return out

    def reproject_host(self, width, height, ids_cur, ids_prev, cur, hist_in, camera, prev_camera, **kw):
        return reproject_host(width, height, ids_cur, ids_prev, cur, hist_in, camera, prev_camera, lib=self.lib, **kw)

    def reproject_moments(self, params, ids_cur, ids_prev, cur, hist_in, mom_in, camera, prev_camera, out=None,
                          mom_out=None, max_history=32, nohist=(1, 0), cur_volumes=None, prev_volumes=None, rgb_ptr=None):
        """vpx_reproject_moments: reproject() carrying the luminance's first two moments along.
        mom_in: float32 torch tensor of 2 * W * H (None together with hist_in).  Returns (out, mom_out),
        allocated when None; never an input."""
        import torch

        if out is None:
            out = torch.empty_like(cur)
        if mom_out is None:
            mom_out = torch.empty(cur.numel() // 2, dtype=torch.float32, device=cur.device)
        r, cv, pv = reproject_desc(camera, prev_camera, max_history, nohist, cur_volumes, prev_volumes)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else 0)  # noqa: E731
        self._chk(self.lib.vpx_reproject_moments(self.h, C.byref(params), ptr(ids_cur), ptr(ids_prev), ptr(cur),
                                                 ptr(hist_in), ptr(mom_in), ptr(out), ptr(mom_out),
                                                 C.c_void_p(rgb_ptr or 0), C.byref(r), cv, pv), "vpx_reproject_moments")
        return out, mom_out

    def reproject_moments_host(self, width, height, ids_cur, ids_prev, cur, hist_in, mom_in, camera, prev_camera, **kw):
        return reproject_moments_host(width, height, ids_cur, ids_prev, cur, hist_in, mom_in, camera, prev_camera,
                                      lib=self.lib, **kw)

    def denoise_var(self, params, ids, src, mom=None, out=None, passes=5, sigma_v=4.0, epsilon=2.0**-10, min_history=4,
                    rgb_ptr=None):
        """vpx_denoise_var: denoise() with a per-pixel luminance tolerance of sigma_v standard
        deviations (+ epsilon).  mom: reproject_moments' moments tensor (then src.w is the history
        length and pixels with at least min_history frames take their temporal variance), or None
        (the variance of the 5x5 neighbourhood on the pixel's plane).  Returns `out` (allocated like
        src when None; never src itself).  Runs on the context's stream, unsynchronised."""
        import torch

        if out is None:
            out = torch.empty_like(src)
        d = abi.denoise_var(passes, sigma_v, epsilon, min_history)
        self._chk(self.lib.vpx_denoise_var(self.h, C.byref(params), C.c_void_p(ids.data_ptr()), C.c_void_p(src.data_ptr()),
                                           C.c_void_p(mom.data_ptr() if mom is not None else 0),
                                           C.c_void_p(out.data_ptr()), C.c_void_p(rgb_ptr or 0), C.byref(d)),
                  "vpx_denoise_var")
        return out

    def denoise_var_host(self, width, height, ids, src, mom=None, **kw):
        return denoise_var_host(width, height, ids, src, mom, lib=self.lib, **kw)

    def trace(self, rays, seeds, depth, sky=abi.SKY_DEFAULT, area_samples=3):
        """Renderer::Trace per ray; sky=None samples the sky texture (activateSky)."""
        n = len(rays)
        seeds = np.ascontiguousarray(seeds, np.uint32)
        out = np.zeros((max(1, n), 3), np.float32)
        self._chk(self.lib.vpx_trace(self.h, rays, seeds.ctypes.data_as(C.c_void_p), n, depth, abi.sky_arg(sky),
                                     area_samples, out.ctypes.data_as(C.c_void_p)), "vpx_trace")
        return out[:n]

    def trace_probe(self, rays, seeds, depth, sky=abi.SKY_DEFAULT, area_samples=3, radiance=True):
        """trace() plus each ray's player light probes (vpx_trace_probe): (radiance or None,
        record array with probes, lit, max_sqr, reserved)."""
        n = len(rays)
        seeds = np.ascontiguousarray(seeds, np.uint32)
        out = np.zeros((max(1, n), 3), np.float32) if radiance else None
        pr = np.zeros(max(1, n), abi.np_dtype(abi.RayProbe))
        self._chk(self.lib.vpx_trace_probe(self.h, rays, seeds.ctypes.data_as(C.c_void_p), n, depth, abi.sky_arg(sky),
                                           area_samples, out.ctypes.data_as(C.c_void_p) if radiance else None,
                                           abi.as_ptr(pr, abi.RayProbe)), "vpx_trace_probe")
        return (out[:n] if radiance else None), pr[:n]

    def focus_distance(self, width, height):
        f = C.c_float()
        self._chk(self.lib.vpx_focus_distance(self.h, width, height, C.byref(f)), "vpx_focus_distance")
        return f.value


def make_rays(origins, directions, tmax=1e34, inside=0):
    """ctypes array of abi.Ray from (n,3) arrays."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    n = len(o)
    arr = (abi.Ray * n)()
    view = np.frombuffer(arr, dtype=np.dtype([("o", "<f4", 3), ("d", "<f4", 3), ("t", "<f4"), ("g", "<u4")]))
    view["o"] = o
    view["d"] = d
    view["t"] = np.broadcast_to(np.asarray(tmax, np.float32), (n,))
    view["g"] = np.broadcast_to(np.asarray(inside, np.uint32), (n,))
    return arr


def hits_to_numpy(hits, n):
    dt = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("vox_index", "<i4"), ("material", "<u4"), ("cells", "<u4"),
                   ("inside_glass", "<u4")])
    return np.frombuffer(hits, dtype=dt, count=n).copy()


def cells_to_numpy(cells, n):
    dt = np.dtype([("cell", "<i4", 3), ("grid_id", "<u4"), ("face_cell", "<i4", 3), ("flags", "<u4")])
    return np.frombuffer(cells, dtype=dt, count=n).copy()


def unpack_ids(ids):
    """The fields of a vpx_render_ids buffer ([H, W, 4] int32 / uint32, torch or numpy) as numpy
    arrays of shape [H, W]: t (float32), vox_index (-2 miss, -1 shape), material, face (0 none,
    else 1 + 2 * axis + (step < 0)), axis and step (0 where face is 0), cell ([H, W, 3])."""
    if hasattr(ids, "cpu"):
        ids = ids.cpu().numpy()
    w = np.ascontiguousarray(ids).view(np.uint32)
    y = w[..., 1]
    face = (y >> 24).astype(np.int32)
    cell = np.stack([w[..., 2] & 0xFFFF, w[..., 2] >> 16, w[..., 3]], axis=-1).astype(np.int32)
    return {"t": np.ascontiguousarray(w[..., 0]).view(np.float32),
            "vox_index": (y & 0xFFFF).astype(np.int32) - 2,
            "material": ((y >> 16) & 0xFF).astype(np.uint32),
            "face": face,
            "axis": np.where(face > 0, (face - 1) >> 1, 0).astype(np.int32),
            "step": np.where(face > 0, 1 - 2 * ((face - 1) & 1), 0).astype(np.int32),
            "cell": cell}


_HIT_DT = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("vox_index", "<i4"), ("material", "<u4"), ("cells", "<u4"),
                    ("inside_glass", "<u4")])
_CELL_DT = np.dtype([("cell", "<i4", 3), ("grid_id", "<u4"), ("face_cell", "<i4", 3), ("flags", "<u4")])


def _records(buf, dt):
    if hasattr(buf, "cpu"):
        buf = buf.cpu().numpy()
    return np.ascontiguousarray(buf).view(np.uint8).reshape(-1).view(dt)


def unpack_hits(hits):
    """cast_nearest's hits ([n, 8] int32, torch or numpy) as hits_to_numpy's record array (a view
    of the host copy)."""
    return _records(hits, _HIT_DT)


def unpack_cells(cells):
    """cast_nearest's cells ([n, 8] int32, torch or numpy) as cells_to_numpy's record array."""
    return _records(cells, _CELL_DT)


def denoise_host(width, height, ids, src, passes=5, sigma_l=0.0, rgb=False, lib=None):
    """vpx_denoise_host: the same filter on numpy arrays, no device.  ids: uint32 [H, W, 4] (or
    anything of that size), src: float32 [H, W, 4].  Returns out [H, W, 4], or (out, rgb8 [H, W])
    with rgb=True."""
    lib = lib or abi.load_library()
    w, h = int(width), int(height)
    i = np.ascontiguousarray(ids).view(np.uint32).reshape(h, w, 4)
    s = np.ascontiguousarray(src, np.float32).reshape(h, w, 4)
    out = np.empty_like(s)
    rgb8 = np.empty((h, w), np.uint32) if rgb else None
    d = abi.Denoise(int(passes), float(sigma_l), 0, 0)
    abi.check(lib, None, lib.vpx_denoise_host(w, h, abi.as_ptr(i), abi.as_ptr(s), abi.as_ptr(out), abi.as_ptr(rgb8),
                                              C.byref(d)), "vpx_denoise_host")
    return (out, rgb8) if rgb else out


def reproject_desc(camera, prev_camera, max_history=32, nohist=(1, 0), cur_volumes=None, prev_volumes=None):
    """(vpx_reproject, cur volume array or None, prev volume array or None) for the two reproject entries."""
    r = abi.Reproject()
    r.cur, r.prev = camera, prev_camera
    r.max_history = float(max_history)
    r.nohist_lo, r.nohist_hi = int(nohist[0]), int(nohist[1])
    n = len(cur_volumes) if cur_volumes is not None else 0
    if n != (len(prev_volumes) if prev_volumes is not None else 0):
        raise ValueError("cur_volumes and prev_volumes differ in length")
    r.n_volumes = n
    cv = (abi.Volume * n)(*cur_volumes) if n else None
    pv = (abi.Volume * n)(*prev_volumes) if n else None
    return r, cv, pv


def reproject_host(width, height, ids_cur, ids_prev, cur, hist_in, camera, prev_camera, max_history=32, nohist=(1, 0),
                   cur_volumes=None, prev_volumes=None, rgb=False, lib=None):
    """vpx_reproject_ids_host: the same pass on numpy arrays, no device.  ids: uint32 [H, W, 4], cur /
    hist_in: float32 [H, W, 4]; ids_prev and hist_in None together.  Returns hist_out [H, W, 4], or
    (hist_out, rgb8 [H, W]) with rgb=True."""
    lib = lib or abi.load_library()
    w, h = int(width), int(height)
    ids = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint32).reshape(h, w, 4)  # noqa: E731
    img = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).reshape(h, w, 4)  # noqa: E731
    ic, ip, c, hi = ids(ids_cur), ids(ids_prev), img(cur), img(hist_in)
    out = np.empty_like(c)
    rgb8 = np.empty((h, w), np.uint32) if rgb else None
    r, cv, pv = reproject_desc(camera, prev_camera, max_history, nohist, cur_volumes, prev_volumes)
    abi.check(lib, None, lib.vpx_reproject_ids_host(w, h, abi.as_ptr(ic), abi.as_ptr(ip), abi.as_ptr(c), abi.as_ptr(hi),
                                                    abi.as_ptr(out), abi.as_ptr(rgb8), C.byref(r), cv, pv),
              "vpx_reproject_ids_host")
    return (out, rgb8) if rgb else out


def reproject_moments_host(width, height, ids_cur, ids_prev, cur, hist_in, mom_in, camera, prev_camera, max_history=32,
                           nohist=(1, 0), cur_volumes=None, prev_volumes=None, rgb=False, lib=None):
    """vpx_reproject_moments_host: reproject_host carrying the moments (mom_in: float32 [H, W, 2], None
    together with hist_in).  Returns (hist_out [H, W, 4], mom_out [H, W, 2]), and rgb8 [H, W] with
    rgb=True."""
    lib = lib or abi.load_library()
    w, h = int(width), int(height)
    ids = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint32).reshape(h, w, 4)  # noqa: E731
    img = lambda a, k=4: None if a is None else np.ascontiguousarray(a, np.float32).reshape(h, w, k)  # noqa: E731
    ic, ip, c, hi, mi = ids(ids_cur), ids(ids_prev), img(cur), img(hist_in), img(mom_in, 2)
    out = np.empty_like(c)
    mom_out = np.empty((h, w, 2), np.float32)
    rgb8 = np.empty((h, w), np.uint32) if rgb else None
    r, cv, pv = reproject_desc(camera, prev_camera, max_history, nohist, cur_volumes, prev_volumes)
    abi.check(lib, None, lib.vpx_reproject_moments_host(w, h, abi.as_ptr(ic), abi.as_ptr(ip), abi.as_ptr(c), abi.as_ptr(hi),
                                                        abi.as_ptr(mi), abi.as_ptr(out), abi.as_ptr(mom_out),
                                                        abi.as_ptr(rgb8), C.byref(r), cv, pv),
              "vpx_reproject_moments_host")
    return (out, mom_out, rgb8) if rgb else (out, mom_out)


def denoise_var_host(width, height, ids, src, mom=None, passes=5, sigma_v=4.0, epsilon=2.0**-10, min_history=4, rgb=False,
                     lib=None):
    """vpx_denoise_var_host: the variance-guided filter on numpy arrays, no device.  ids: uint32
    [H, W, 4], src: float32 [H, W, 4], mom: float32 [H, W, 2] or None.  Returns out [H, W, 4], or
    (out, rgb8 [H, W]) with rgb=True."""
    lib = lib or abi.load_library()
    w, h = int(width), int(height)
    i = np.ascontiguousarray(ids).view(np.uint32).reshape(h, w, 4)
    s = np.ascontiguousarray(src, np.float32).reshape(h, w, 4)
    m = None if mom is None else np.ascontiguousarray(mom, np.float32).reshape(h, w, 2)
    out = np.empty_like(s)
    rgb8 = np.empty((h, w), np.uint32) if rgb else None
    d = abi.denoise_var(passes, sigma_v, epsilon, min_history)
    abi.check(lib, None, lib.vpx_denoise_var_host(w, h, abi.as_ptr(i), abi.as_ptr(s), abi.as_ptr(m), abi.as_ptr(out),
                                                  abi.as_ptr(rgb8), C.byref(d)), "vpx_denoise_var_host")
    return (out, rgb8) if rgb else out
