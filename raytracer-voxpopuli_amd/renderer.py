"""Host mirror of the reference Renderer's hot-path surface (renderer.h:42-245).

`Renderer.Tick(deltaTime)` keeps the reference's contract (template/precomp.h:399,
renderer.cpp:1972-1995): optional focus ray, then `Update()`, which here is ONE call into
libvpx_hip.so (`vpx_render`) instead of the execution::par pixel loop
(renderer.cpp:1646-1891).  The accumulator (float4[W*H]) and the screen (uint32
0x00RRGGBB, template/surface.h) live in HBM as torch tensors; `screen_host()` copies the
8-bit frame out for display.  The C++ twin of this class is host/vpx_renderer.{h,cpp}.
"""
import ctypes as C

import numpy as np
import torch

from . import abi
from .context import Context, make_rays


class ModifyingProp:
    """src/Game/ModifyingProp.{h,cpp}: every `toChange` seconds (0.9 in the game) the prop's
    Scene shows the next slice of its model, LoadModelPartial(model, index, increaseRate).
    Update() here is one due edit (the timer stays with the host): one call into the library."""

    def __init__(self, renderer, volume, model_id, startingIndex, increasingRate):
        self.renderer, self.volume, self.model_id = renderer, volume, model_id
        self.index, self.increaseRate = int(startingIndex), int(increasingRate)

    def Update(self):  # ModifyingProp.cpp:11-21
        self.renderer.LoadModelPartial(self.volume, self.model_id, self.index, self.increaseRate)
        self.index += self.increaseRate
        if self.index > 64:
            self.index = self.increaseRate


def player_vox_index(vox, n_volumes, current_chunk):
    """The end of Renderer::FindNearestPlayer (renderer.cpp:1068-1069): from chunk 2 on, an index
    above size - 4 in the reference's unsigned compare becomes -1: the last three volumes,
    and a miss too (-2 is a huge uint32_t).  size() - 4 is a size_t: it wraps below four volumes."""
    if current_chunk >= 2 and (int(vox) & 0xFFFFFFFF) > ((int(n_volumes) - 4) & 0xFFFFFFFFFFFFFFFF):
        return -1
    return int(vox)


class Ray:
    """The fields of the reference Ray (template/scene.h) that the player's casts read and write:
    O, D (used as given: PlayerCharacter::GetRay normalises by itself), t, rayNormal, indexMaterial."""

    def __init__(self, origin, direction, t=1e34):
        self.O, self.D, self.t = tuple(origin), tuple(direction), float(t)
        self.rayNormal = (0.0, 0.0, 0.0)
        self.indexMaterial = abi.MAT_NONE


class Renderer:
    def __init__(self, scene, device=0, ctx=None, temporal=None):
        self.scene = scene
        # temporal accumulation under camera motion (vpx_reproject_ids; no reference counterpart).
        # None / False: Tick's moving-camera branch as the reference has it.  True or a dict of
        # max_history (32), nohist (the (lo, hi) first-hit materials without history: metal, glass
        # and smoke, 5..14), denoise (None, or a dict of passes / sigma_l for Denoise's filter on
        # the result), variance (None, or a dict of sigma_v / epsilon / min_history / passes: the
        # luminance's moments ride along the history (vpx_reproject_moments) and the filter on the
        # result is vpx_denoise_var; takes the place of denoise): see _tick_temporal.
        self.temporal = None
        if temporal:
            self.temporal = dict(max_history=32, nohist=(5, 14), denoise=None)
            if isinstance(temporal, dict):
                self.temporal.update(temporal)
            if self.temporal.get("variance"):  # the key is there only when asked for
                given = self.temporal["variance"] if isinstance(self.temporal["variance"], dict) else {}
                self.temporal["variance"] = dict(dict(sigma_v=4.0, epsilon=2.0 ** -10, min_history=4, passes=5), **given)
        self.history = None           # the temporal mode's current history image, float4[W*H], .w its length
        self._t_ids, self._t_hist = None, None   # two ID buffers and two history images, swapped per tick
        self._t_mom = None            # ... and, with temporal variance, two moments images (float2[W*H])
        self.moments = None           # the current one
        self._t_cur, self._t_valid, self._t_ticks = 0, False, 0
        self._t_prev_camera, self._t_prev_volumes = None, None
        self.device = torch.device("cuda", device)
        self.ctx = ctx or Context(device)
        self.maxBounces = scene.max_bounces               # renderer.h:175
        self.numRenderedFrames = 0                        # renderer.h:204
        self.antiAliasingStrength = scene.aa_strength     # renderer.h:185
        self.numCheckShadowsAreaLight = scene.area_samples  # renderer.h:205
        self.staticCamera = False
        self.activateSky = bool(scene.flags & abi.VPX_FLAG_SKY)  # renderer.h:216
        self.HDRLightContribution = scene.sky_hdr               # renderer.h:224
        self.skyPixels = scene.sky_texture                      # renderer.h:226 (float32 (H, W, 3))
        self.prevCamera = None             # renderer.h:182 (vpx_prev_camera)
        self.illuminationHistory = None    # renderer.h:242, float4[W*H] in HBM
        self.accumulator = None
        self.screen = None
        self.denoised = None   # Denoise()'s image, float4[W*H] in HBM
        self.ids = None        # ... and the ID buffer that guided it (vpx_render_ids)
        self.last_stats = None
        # Renderer::inLight (renderer.h:231): a path reached the player's smoke and found more
        # light there than VPX_PLAYER_LIGHT_SQR.  Kept up to date by Tick only while
        # trackPlayerLight is set: reading the record synchronises once per Tick, which frames
        # in flight exist to avoid.
        self.inLight = False
        self.trackPlayerLight = False
        self.last_player_light = None  # abi.PlayerLight of the last tracked Tick
        self.currentChunk = 0  # renderer.h: read by FindNearestPlayer (renderer.cpp:1068)
        self.seed = 0x12345678  # the xorshift32 state LoadModelRandomMaterials draws from (tmpl8math.cpp:16)
        self.scaleModel = {}    # volume index -> Scene::scaleModel, (1, 1, 1) until a loader multiplies it
        self._models = {}       # model_id -> (voxels, palette) of the resident models (UploadModel)

    def Init(self):
        """Renderer::Init minus window/asset/game setup (renderer.cpp:688-736)."""
        w, h = self.scene.width, self.scene.height
        self.accumulator = torch.zeros(w * h * 4, dtype=torch.float32, device=self.device)
        self.screen = torch.zeros(w * h, dtype=torch.int32, device=self.device)
        torch.cuda.synchronize(self.device)
        # the library launches on this torch stream (never the legacy NULL stream, whose
        # handle 0 would select the context's own stream instead)
        self.stream = torch.cuda.Stream(self.device)
        self.ctx.set_stream(self.stream.cuda_stream)
        self.ctx.load_scene(self.scene)
        self._sky_uploaded = (self.skyPixels, self.HDRLightContribution)
        return self

    def SetArithmetic(self, mode):
        """abi.VPX_ARITH_X86_HOST: the reference's FastReciprocal / rsqrtps as this host computes
        them (vpx_set_arithmetic); abi.VPX_ARITH_EXACT: exact 1/x, 1/sqrtf (default)."""
        self.ctx.set_arithmetic(mode)
        return self

    def _frame_params(self):
        p = self.scene.frame_params(frame_index=self.numRenderedFrames)
        p.max_bounces = self.maxBounces
        p.area_samples = self.numCheckShadowsAreaLight
        up_px, up_hdr = self._sky_uploaded
        if self.skyPixels is not up_px or self.HDRLightContribution != up_hdr:  # ImGui edits, renderer.cpp:2591
            self.ctx.set_sky(self.skyPixels, self.HDRLightContribution)
            self._sky_uploaded = (self.skyPixels, self.HDRLightContribution)
        p.flags = (p.flags & ~abi.VPX_FLAG_SKY) | (abi.VPX_FLAG_SKY if self.activateSky else 0)
        return p

    def ResetAccumulator(self):  # renderer.cpp:343-346
        self.numRenderedFrames = 0

    def Update(self, stats=False):
        p = self._frame_params()
        p.aa_strength = self.antiAliasingStrength
        self.last_stats = self.ctx.render(p, self.accumulator.data_ptr(), self.screen.data_ptr(), stats=stats)
        self.numRenderedFrames += 1
        return self.last_stats

    def CopyToPrevCamera(self):  # renderer.cpp:1893-1902
        from .scene import prev_camera
        self.prevCamera = prev_camera(self.scene._cam_pos, self.scene._cam_target, self.scene.width, self.scene.height)

    def Tick(self, deltaTime=0.0, stats=False):
        if not self.staticCamera:
            if self.scene.flags & abi.VPX_FLAG_DOF:  # focus ray, renderer.cpp:1987-1991
                self.scene.camera.focal_distance = self.ctx.focus_distance(self.scene.width, self.scene.height)
                self.ctx.set_camera(self.scene.camera)
            st = self._tick_temporal(stats) if self.temporal else self.Update(stats=stats)
            self._read_player_light()
            return st
        # static branch (renderer.cpp:1996-2101): TraceReproject + history reprojection
        if self.prevCamera is None:
            self.CopyToPrevCamera()
        if self.illuminationHistory is None:
            w, h = self.scene.width, self.scene.height
            self.illuminationHistory = torch.zeros(w * h * 4, dtype=torch.float32, device=self.device)
            torch.cuda.synchronize(self.device)  # allocated on torch's stream; the library uses its own
        p = self._frame_params()
        st = self.ctx.render_reproject(p, self.prevCamera, self.illuminationHistory.data_ptr(), self.screen.data_ptr(),
                                       stats=stats)
        self.numRenderedFrames += 1
        self._read_player_light()
        return st

    def LookAt(self, pos, target):
        """Move the camera (Camera::HandleInput's basis, vpx_camera_look_at) and hand it to the context."""
        from .scene import look_at
        self.scene.camera = look_at(pos, target, self.scene.width, self.scene.height)
        self.scene._cam_pos, self.scene._cam_target = tuple(pos), tuple(target)
        self.ctx.set_camera(self.scene.camera)

    def DropHistory(self):
        """Forget the temporal mode's history, and the moments that ride along it: the next Tick
        starts from its own samples."""
        self._t_valid = False

    ResetTemporal = DropHistory

    def _tick_temporal(self, stats=False):
        """One Tick of a moving camera with temporal accumulation, queued on the renderer's stream
        without synchronising: vpx_render with frame_index 0 (the accumulator holds this tick's
        samples alone; the seed stream is the tick number's, so that a camera that stands still for
        a tick does not draw the same noise again), vpx_render_ids, vpx_reproject_ids from the
        previous tick's ids, history and camera into self.history, then optionally vpx_denoise_ids
        on self.history into self.denoised; the screen shows the last of them.  The history, not
        the denoised image, is what the next tick reads.  A change of the frame's size drops the
        history; so does DropHistory().  Volumes whose matrices changed since the previous tick are
        followed (vpx_reproject's moving volumes).  With temporal["variance"] the reprojection is
        vpx_reproject_moments, a moments image ping-pongs beside the history, and the filter is
        vpx_denoise_var on (history, moments): pixels whose history is at least min_history frames
        long take their temporal variance, the others their neighbourhood's."""
        from .scene import prev_camera
        t = self.temporal
        w, h = self.scene.width, self.scene.height
        if self._t_hist is None or self._t_hist[0].numel() != w * h * 4:
            with torch.cuda.stream(self.stream):
                self._t_ids = [torch.empty(w * h * 4, dtype=torch.int32, device=self.device) for _ in range(2)]
                self._t_hist = [torch.empty(w * h * 4, dtype=torch.float32, device=self.device) for _ in range(2)]
                if t.get("variance"):
                    self._t_mom = [torch.empty(w * h * 2, dtype=torch.float32, device=self.device) for _ in range(2)]
            self._t_valid = False
        p = self._frame_params()
        p.frame_index = 0
        p.seed_base = (p.seed_base + self._t_ticks * w * h) & 0xFFFFFFFF
        p.aa_strength = self.antiAliasingStrength
        self.last_stats = self.ctx.render(p, self.accumulator.data_ptr(), None, stats=stats)
        self.numRenderedFrames = 1
        cur, prev = self._t_cur, 1 - self._t_cur
        ids, hist = self._t_ids, self._t_hist
        self.ctx._chk(self.ctx.lib.vpx_render_ids(self.ctx.h, C.byref(p), None, C.c_void_p(ids[cur].data_ptr())),
                      "vpx_render_ids")
        volumes = [abi.Volume.from_buffer_copy(v) for v in self.scene.volumes]
        here = prev_camera(self.scene._cam_pos, self.scene._cam_target, w, h)
        moved = (self._t_valid and self._t_prev_volumes is not None and len(self._t_prev_volumes) == len(volumes) and
                 any(bytes(a) != bytes(b) for a, b in zip(volumes, self._t_prev_volumes)))
        with torch.cuda.stream(self.stream):
            if (t["denoise"] or t.get("variance")) and self.denoised is None:
                self.denoised = torch.empty_like(self.accumulator)
        common = dict(max_history=t["max_history"], nohist=t["nohist"], cur_volumes=volumes if moved else None,
                      prev_volumes=self._t_prev_volumes if moved else None)
        if t.get("variance"):
            v, mom = t.get("variance"), self._t_mom
            self.ctx.reproject_moments(p, ids[cur], ids[prev] if self._t_valid else None, self.accumulator,
                                       hist[prev] if self._t_valid else None, mom[prev] if self._t_valid else None,
                                       self.scene.camera, self._t_prev_camera if self._t_valid else here, out=hist[cur],
                                       mom_out=mom[cur], **common)
            self.ctx.denoise_var(p, ids[cur], hist[cur], mom[cur], self.denoised, v["passes"], v["sigma_v"], v["epsilon"],
                                 v["min_history"], self.screen.data_ptr())
            self.moments = mom[cur]
        else:
            self.ctx.reproject(p, ids[cur], ids[prev] if self._t_valid else None, self.accumulator,
                               hist[prev] if self._t_valid else None, self.scene.camera,
                               self._t_prev_camera if self._t_valid else here, out=hist[cur],
                               rgb_ptr=None if t["denoise"] else self.screen.data_ptr(), **common)
        if t["denoise"] and not t.get("variance"):
            self.ctx.denoise(p, ids[cur], hist[cur], self.denoised, t["denoise"].get("passes", 5),
                             t["denoise"].get("sigma_l", 0.0), self.screen.data_ptr())
        self.history, self.ids = hist[cur], ids[cur]
        self._t_prev_camera, self._t_prev_volumes = here, volumes
        self._t_cur, self._t_valid, self._t_ticks = prev, True, self._t_ticks + 1
        return self.last_stats

    def temporal_history_host(self):
        self.synchronize()
        return self.history.cpu().numpy().reshape(self.scene.height, self.scene.width, 4)

    def temporal_moments_host(self):
        self.synchronize()
        return self.moments.cpu().numpy().reshape(self.scene.height, self.scene.width, 2)

    def _read_player_light(self):
        """The frame's flag, read and cleared after the render on both branches: the reference's
        Tick reads inLight (renderer.cpp:2112-2118) and clears it (:2206)."""
        if self.trackPlayerLight:
            self.last_player_light = self.ctx.player_light(reset=True)
            self.inLight = bool(self.last_player_light.in_light)

    def FindNearestPlayer(self, ray):
        """Renderer::FindNearestPlayer (renderer.cpp:1020-1071), the player's cast in Tick
        (:2139-2152): volumes 1 .. n-1 (0 is the player), smoke passed through
        (Scene::FindNearestExcept), no spheres / triangles, ray.D as given.  Returns the volume
        index (player_vox_index) and, on a hit, leaves t, rayNormal and indexMaterial in `ray`."""
        h = self.ctx.find_nearest_filtered(make_rays([ray.O], [ray.D], ray.t), 1,
                                           (abi.MAT_SMOKE_LOW_DENSITY, abi.MAT_SMOKE_PLAYER), shapes=False,
                                           raw_direction=True)[0]
        if h.vox_index >= 0:
            ray.t, ray.rayNormal, ray.indexMaterial = h.t, tuple(h.normal), h.material
        return player_vox_index(h.vox_index, len(self.scene.volumes), self.currentChunk)

    def FindNearestCells(self, ray):
        """FindNearestPlayer's query with the hit cell (vpx_find_nearest_cells): the same filter and
        the same update of `ray`.  Returns (volume index as FindNearestPlayer, abi.HitCell): the
        cell the player points at and the neighbour a new voxel would go into."""
        hits, cells = self.ctx.find_nearest_cells(make_rays([ray.O], [ray.D], ray.t), 1,
                                                  (abi.MAT_SMOKE_LOW_DENSITY, abi.MAT_SMOKE_PLAYER), shapes=False,
                                                  raw_direction=True)
        h = hits[0]
        if h.vox_index >= 0:
            ray.t, ray.rayNormal, ray.indexMaterial = h.t, tuple(h.normal), h.material
        return player_vox_index(h.vox_index, len(self.scene.volumes), self.currentChunk), cells[0]

    def PickPixel(self, x, y, filter=None):
        """The hit and the hit cell under pixel (x, y) of the frame (vpx_pick_pixel): (abi.Hit,
        abi.HitCell).  Which pixel to pick and what to do with the cell is the game's business."""
        return self.ctx.pick_pixel(self.scene.width, self.scene.height, x, y, filter=filter)

    pick_pixel = PickPixel

    def Denoise(self, passes=5, sigma_l=0.0, variance=None):
        """The plane-keyed a-trous filter of the current accumulator (no reference counterpart: the
        reference shows a moving camera's frame as it is): the ids of the current camera
        (vpx_render_ids), then vpx_denoise_ids from self.accumulator into self.denoised, tonemapped
        into self.screen.  Three launches or more on the renderer's stream, no synchronisation.
        The ids are those of the un-jittered pixel-centre ray; paths through glass, smoke or a
        mirror are keyed by their first hit.  variance: True or a dict of sigma_v / epsilon (and
        passes): vpx_denoise_var without moments instead, the luminance tolerance from the variance
        of each pixel's 5x5 neighbourhood on its plane (sigma_l is not used)."""
        p = self._frame_params()
        with torch.cuda.stream(self.stream):  # the tensors belong to the stream their kernels run on
            self.ids = self.ctx.render_ids(p)
            if self.denoised is None:
                self.denoised = torch.empty_like(self.accumulator)
        if variance:
            v = dict(dict(sigma_v=4.0, epsilon=2.0 ** -10, passes=passes), **(variance if isinstance(variance, dict) else {}))
            self.ctx.denoise_var(p, self.ids, self.accumulator, None, self.denoised, v["passes"], v["sigma_v"], v["epsilon"],
                                 1, self.screen.data_ptr())
        else:
            self.ctx.denoise(p, self.ids, self.accumulator, self.denoised, passes, sigma_l, self.screen.data_ptr())
        return self.denoised

    def CastRays(self, rays, filter=None, cells=True, form=None, max_waves=0):
        """A batch of rays that already live on the device (no reference counterpart; per ray the
        records of Renderer::FindNearest with the hit cell): ctx.cast_nearest on the renderer's
        stream, unsynchronised.  Returns (hits, cells) device tensors."""
        with torch.cuda.stream(self.stream):  # the tensors belong to the stream their kernel runs on
            return self.ctx.cast_nearest(rays, filter=filter, cells=cells, form=form, max_waves=max_waves)

    def CastOccluded(self, rays, filter=None, form=None, max_waves=0):
        """Renderer::IsOccluded per ray of a device batch: ctx.cast_occluded on the renderer's stream,
        unsynchronised.  Returns a uint8 device tensor."""
        with torch.cuda.stream(self.stream):
            return self.ctx.cast_occluded(rays, filter=filter, form=form, max_waves=max_waves)

    def denoised_host(self):
        self.synchronize()
        return self.denoised.cpu().numpy().reshape(self.scene.height, self.scene.width, 4)

    def IsOccludedPlayerClimbable(self, ray):
        """Renderer::IsOccludedPlayerClimbable (renderer.cpp:245-273): IsOccluded from volume 1 on,
        without the spheres / triangles, ray.D as given."""
        return bool(self.ctx.is_occluded_filtered(make_rays([ray.O], [ray.D], ray.t), 1, shapes=False,
                                                  raw_direction=True)[0])

    # ------------------------------------------------------------ model loaders
    def UploadModel(self, model_id, size, voxels, palette=None):
        """Make a decoded .vox model (scene.load_model / decode_vox) resident on the device; the
        loaders below then place it by id.  The palette stays on the host for LoadModel's
        material override."""
        self.ctx.model_upload(model_id, size, voxels)
        self._models[model_id] = (np.ascontiguousarray(voxels, np.uint8).reshape(-1),
                                  None if palette is None else np.ascontiguousarray(palette, np.uint8))

    def _load(self, volume, model_id, **kw):
        """One loader call on the Scene of `volume`: its grid, its size and its scaleModel member
        (template/scene.h), which the loaders multiply when the model is larger than the grid."""
        gid = self.scene.volumes[volume].grid_id
        res = self.ctx.grid_load_model(gid, self.scene.grids[gid].n, model_id,
                                       scale_model=self.scaleModel.get(volume, (1.0, 1.0, 1.0)), **kw)
        self.scaleModel[volume] = tuple(res.scale_model)
        return res

    def LoadModel(self, volume, model_id):
        """Scene::LoadModel (template/scene.cpp:449-529) on the device, then its palette override
        of Renderer::materials (:516-520) and the table re-sent."""
        self._load(volume, model_id, mode=abi.LOAD_FULL)
        vox, pal = self._models[model_id]
        if pal is not None:
            abi.check(self.ctx.lib, None,
                      self.ctx.lib.vpx_model_palette_materials(self.scene.materials, vox.ctypes.data, vox.size,
                                                               pal.ctypes.data), "vpx_model_palette_materials")
            self.ctx.set_materials(self.scene.materials)

    def LoadModelPartial(self, volume, model_id, columns, thickness):
        """Scene::LoadModelPartial (template/scene.cpp:531-604) on the device."""
        self._load(volume, model_id, mode=abi.LOAD_PARTIAL, columns=columns, thickness=thickness)

    def LoadModelRandomMaterials(self, volume, model_id):
        """Scene::LoadModelRandomMaterials (template/scene.cpp:606-683) on the device: the draws
        come from, and advance, self.seed (the thread's xorshift32 state, tmpl8math.cpp:16)."""
        self.seed = self._load(volume, model_id, mode=abi.LOAD_RANDOM, seed=self.seed, rand_lo=12.0, rand_hi=13.0).seed

    # ------------------------------------------------------------ noise generators
    def _generate(self, volume, mode, frequency):
        gid = self.scene.volumes[volume].grid_id
        res = self.ctx.grid_generate_noise(gid, self.scene.grids[gid].n, mode, frequency, self.seed)
        self.seed = res.seed
        return res

    def GenerateSomeNoise(self, volume, frequency=0.03):
        """Scene::GenerateSomeNoise (template/scene.cpp:226-282) on the device, on the Scene of
        `volume`: the draws come from, and advance, self.seed."""
        return self._generate(volume, abi.GEN_NOISE, frequency)

    def GenerateSomeSmoke(self, volume, frequency=0.001):
        """Scene::GenerateSomeSmoke (template/scene.cpp:285-356) on the device, as
        voxelVolumes[5].GenerateSomeSmoke(0.167f) of renderer.cpp:626 and :2174."""
        return self._generate(volume, abi.GEN_SMOKE, frequency)

    def history_host(self):
        self.synchronize()
        return self.illuminationHistory.cpu().numpy().reshape(self.scene.height, self.scene.width, 4)

    def synchronize(self):
        self.stream.synchronize()

    def screen_host(self):
        self.synchronize()
        return self.screen.cpu().numpy().view("uint32").reshape(self.scene.height, self.scene.width)

    def accumulator_host(self):
        self.synchronize()
        return self.accumulator.cpu().numpy().reshape(self.scene.height, self.scene.width, 4)
