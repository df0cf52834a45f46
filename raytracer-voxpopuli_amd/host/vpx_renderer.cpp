// vpx_renderer.cpp — see vpx_renderer.h.
#include "vpx_renderer.h"

#include <hip/hip_runtime_api.h>

#include <cstring>

namespace vpxhost {

Renderer::Renderer(int device) : device_(device) { status_ = vpx_create(device, &ctx_); }

Renderer::Renderer(const std::vector<int>& devices) : device_(devices.empty() ? 0 : devices[0]) {
    status_ = devices.empty() ? VPX_E_INVALID : vpx_create_multi(devices.data(), (int)devices.size(), &ctx_);
}

Renderer::~Renderer() {
    if (accumulator_) (void)hipFree(accumulator_);
    if (screen_) (void)hipFree(screen_);
    if (history_) (void)hipFree(history_);
    if (denoised_) (void)hipFree(denoised_);
    if (ids_) (void)hipFree(ids_);
    for (void* b : {(void*)tIds_[0], (void*)tIds_[1], (void*)tHist_[0], (void*)tHist_[1], (void*)tMom_[0], (void*)tMom_[1]})
        if (b) (void)hipFree(b);
    if (ctx_) vpx_destroy(ctx_);
}

const char* Renderer::LastError() const {
    if (!err_.empty()) return err_.c_str();
    return ctx_ ? vpx_last_error(ctx_) : "vpx_create failed (no usable HIP device)";
}

int Renderer::Init(uint32_t width, uint32_t height) {
    if (status_) return status_;
    if (vpx_abi_version() != VPX_ABI_VERSION) {  // a stale libvpx_hip.so
        err_ = "libvpx_hip.so ABI version differs from include/vpx.h";
        return status_ = VPX_E_STATE;
    }
    if (!width || !height) return VPX_E_INVALID;
    if (hipSetDevice(device_) != hipSuccess ||
        hipMalloc(&accumulator_, sizeof(float) * 4 * width * height) != hipSuccess ||
        hipMalloc(&screen_, sizeof(uint32_t) * width * height) != hipSuccess ||
        hipMemset(accumulator_, 0, sizeof(float) * 4 * width * height) != hipSuccess ||
        hipMemset(screen_, 0, sizeof(uint32_t) * width * height) != hipSuccess) {
        err_ = "frame buffer allocation failed";
        return VPX_E_NOMEM;
    }
    if (width != width_ || height != height_) {  // a resize drops the temporal history and its buffers
        for (void* b : {(void*)tIds_[0], (void*)tIds_[1], (void*)tHist_[0], (void*)tHist_[1], (void*)tMom_[0], (void*)tMom_[1]})
            if (b) (void)hipFree(b);
        tIds_[0] = tIds_[1] = nullptr, tHist_[0] = tHist_[1] = nullptr, tMom_[0] = tMom_[1] = nullptr;
        tValid_ = false;
    }
    width_ = width, height_ = height;
    numRenderedFrames = 0;
    return VPX_OK;
}

int Renderer::UploadGrid(uint32_t grid_id, const uint8_t* cells, uint32_t n) {
    if (status_) return status_;
    const int rc = vpx_upload_grid(ctx_, grid_id, cells, n);
    if (rc == VPX_OK) CreateGrid(grid_id, n);
    return rc;
}

void Renderer::CreateGrid(uint32_t grid_id, uint32_t n) {
    if (grid_id > 4096) return;  // the library refuses such ids
    if (grid_id >= gridSize_.size()) gridSize_.resize(grid_id + 1, 0u);
    gridSize_[grid_id] = n;
}

int Renderer::SetVolumes(const std::vector<vpx_volume>& v) {
    if (status_) return status_;
    const int rc = vpx_set_volumes(ctx_, v.data(), (uint32_t)v.size());
    if (rc == VPX_OK) numVolumes_ = v.size(), volumes_ = v;
    return rc;
}

int Renderer::SetMaterials(const std::vector<vpx_material>& m) {
    if (status_) return status_;
    const int rc = vpx_set_materials(ctx_, m.data(), (uint32_t)m.size());
    if (rc == VPX_OK) materials_ = m;
    return rc;
}

int Renderer::UploadModel(uint32_t model_id, const uint8_t* voxels, uint32_t sx, uint32_t sy, uint32_t sz,
                          const uint8_t* palette_rgba) {
    if (status_) return status_;
    const int rc = vpx_model_upload(ctx_, model_id, voxels, sx, sy, sz);
    if (rc || !voxels) return rc;
    if (model_id >= models_.size()) models_.resize(model_id + 1);
    models_[model_id].voxels.assign(voxels, voxels + (size_t)sx * sy * sz);
    models_[model_id].palette.clear();
    if (palette_rgba) models_[model_id].palette.assign(palette_rgba, palette_rgba + 1024);
    return VPX_OK;
}

const float* Renderer::ScaleModel(uint32_t volume) {
    if (volume >= scaleModel_.size()) scaleModel_.resize(volume + 1, {1.0f, 1.0f, 1.0f});
    return scaleModel_[volume].data();
}

// One loader call on the Scene of `volume`: its grid, its size and its scaleModel member, which
// the loaders multiply when the model is larger than the grid (so the result is fed back).
int Renderer::Load(uint32_t volume, uint32_t model_id, vpx_model_load in, vpx_model_result* out) {
    if (status_) return status_;
    if (volume >= volumes_.size()) return VPX_E_INVALID;
    const uint32_t gid = volumes_[volume].grid_id;
    if (gid >= gridSize_.size() || !gridSize_[gid]) return VPX_E_STATE;  // CreateGrid / UploadGrid first
    const float* s = ScaleModel(volume);
    for (int k = 0; k < 3; ++k) in.scale_model[k] = s[k];
    vpx_model_result res{};
    const int rc = vpx_grid_load_model(ctx_, gid, gridSize_[gid], model_id, &in, &res);
    if (rc) return rc;
    for (int k = 0; k < 3; ++k) scaleModel_[volume][k] = res.scale_model[k];
    if (out) *out = res;
    return VPX_OK;
}

int Renderer::LoadModel(uint32_t volume, uint32_t model_id) {
    vpx_model_load in{};
    in.mode = VPX_LOAD_FULL;
    int rc = Load(volume, model_id, in, nullptr);
    if (rc || model_id >= models_.size() || models_[model_id].palette.empty()) return rc;
    if (materials_.size() < VPX_NUM_MATERIALS) return VPX_E_STATE;  // SetMaterials first
    const Model& m = models_[model_id];
    rc = vpx_model_palette_materials(materials_.data(), m.voxels.data(), m.voxels.size(), m.palette.data());
    return rc ? rc : vpx_set_materials(ctx_, materials_.data(), (uint32_t)materials_.size());
}

int Renderer::LoadModelPartial(uint32_t volume, uint32_t model_id, uint32_t columns, uint32_t thickness) {
    vpx_model_load in{};
    in.mode = VPX_LOAD_PARTIAL;
    in.columns = columns, in.thickness = thickness;
    return Load(volume, model_id, in, nullptr);
}

int Renderer::LoadModelRandomMaterials(uint32_t volume, uint32_t model_id) {
    vpx_model_load in{};
    in.mode = VPX_LOAD_RANDOM;
    in.seed = seed;
    in.rand_lo = 12.0f, in.rand_hi = 13.0f;  // SMOKE_MID2_DENSITY, SMOKE_HIGH_DENSITY (scene.cpp:661-662)
    vpx_model_result res{};
    const int rc = Load(volume, model_id, in, &res);
    if (rc == VPX_OK) seed = res.seed;
    return rc;
}

// Scene::GenerateSomeNoise / GenerateSomeSmoke on the Scene of `volume`: its grid and its size;
// the draws come from, and advance, `seed`.
int Renderer::Generate(uint32_t volume, uint32_t mode, float frequency, vpx_noise_result* out) {
    if (status_) return status_;
    if (volume >= volumes_.size()) return VPX_E_INVALID;
    const uint32_t gid = volumes_[volume].grid_id;
    if (gid >= gridSize_.size() || !gridSize_[gid]) return VPX_E_STATE;  // CreateGrid / UploadGrid first
    vpx_noise_gen in{};
    in.mode = mode, in.frequency = frequency, in.seed = seed;
    vpx_noise_result res{};
    const int rc = vpx_grid_generate_noise(ctx_, gid, gridSize_[gid], &in, &res);
    if (rc) return rc;
    seed = res.seed;
    if (out) *out = res;
    return VPX_OK;
}

int Renderer::GenerateSomeNoise(uint32_t volume, float frequency, vpx_noise_result* out) {
    return Generate(volume, VPX_GEN_NOISE, frequency, out);
}

int Renderer::GenerateSomeSmoke(uint32_t volume, float frequency, vpx_noise_result* out) {
    return Generate(volume, VPX_GEN_SMOKE, frequency, out);
}

int Renderer::SetLights(const std::vector<vpx_point_light>& p, const std::vector<vpx_spot_light>& s,
                        const std::vector<vpx_area_light>& a, const vpx_dir_light& d) {
    if (status_) return status_;
    return vpx_set_lights(ctx_, p.data(), (uint32_t)p.size(), s.data(), (uint32_t)s.size(), a.data(),
                          (uint32_t)a.size(), &d);
}

int Renderer::SetShapes(const std::vector<vpx_sphere>& s, const std::vector<vpx_triangle>& t) {
    if (status_) return status_;
    return vpx_set_shapes(ctx_, s.data(), (uint32_t)s.size(), t.data(), (uint32_t)t.size());
}

int Renderer::LookAt(const float pos[3], const float target[3]) {
    if (status_) return status_;
    const float keep_focal = camera.focal_distance, keep_jitter = camera.defocus_jitter;
    int rc = vpx_camera_look_at(pos, target, width_, height_, &camera);
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) camPos_[i] = pos[i], camTarget_[i] = target[i];
    if (keep_focal > 0.0f) camera.focal_distance = keep_focal, camera.defocus_jitter = keep_jitter;
    return vpx_set_camera(ctx_, &camera);
}

int Renderer::Update(vpx_stats* stats) {
    if (status_) return status_;
    if (!accumulator_) return VPX_E_STATE;
    vpx_frame_params p{};
    p.width = width_, p.height = height_;
    p.max_bounces = maxBounces;
    p.frame_index = numRenderedFrames;
    p.seed_base = 0;
    p.flags = (flags & ~VPX_FLAG_SKY) | (activateSky ? VPX_FLAG_SKY : 0u);
    p.aa_strength = antiAliasingStrength;
    p.area_samples = numCheckShadowsAreaLight;
    p.sky[0] = sky[0], p.sky[1] = sky[1], p.sky[2] = sky[2];
    uint32_t* target = nullptr;
    int rc = MapScreen(&target);
    if (rc) return rc;
    rc = UnmapScreen(vpx_render(ctx_, &p, accumulator_, target, stats));
    if (rc == VPX_OK) ++numRenderedFrames;
    return rc;
}

int Renderer::SetSky(const float* rgb, uint32_t width, uint32_t height, float hdr_contribution) {
    return status_ ? status_ : vpx_set_sky(ctx_, rgb, width, height, hdr_contribution);
}

int Renderer::SetArithmetic(uint32_t mode) { return status_ ? status_ : vpx_set_arithmetic(ctx_, mode); }

int Renderer::CopyToPrevCamera() {
    if (status_) return status_;
    const int rc = vpx_prev_camera_look_at(camPos_, camTarget_, width_, height_, &prevCamera);
    if (rc == VPX_OK) havePrev_ = true;
    return rc;
}

// The static branch of Renderer::Tick (renderer.cpp:1996-2101): TraceReproject per pixel,
// reprojection into prevCamera, SampleHistory / ClampHistory, blend, tonemap, RGB8.
int Renderer::UpdateStatic(vpx_stats* stats) {
    if (!history_) {
        const size_t bytes = sizeof(float) * 4 * (size_t)width_ * height_;
        if (hipMalloc(&history_, bytes) != hipSuccess || hipMemset(history_, 0, bytes) != hipSuccess) {
            err_ = "history allocation failed";
            return VPX_E_NOMEM;
        }
    }
    if (!havePrev_) {
        const int rc = CopyToPrevCamera();
        if (rc) return rc;
    }
    vpx_frame_params p{};
    p.width = width_, p.height = height_;
    p.max_bounces = maxBounces;
    p.frame_index = numRenderedFrames;
    p.flags = activateSky ? VPX_FLAG_SKY : 0u;
    p.aa_strength = antiAliasingStrength;
    p.area_samples = numCheckShadowsAreaLight;
    p.sky[0] = sky[0], p.sky[1] = sky[1], p.sky[2] = sky[2];
    uint32_t* target = nullptr;
    int rc = MapScreen(&target);
    if (rc) return rc;
    rc = UnmapScreen(vpx_render_reproject(ctx_, &p, &prevCamera, history_, target, stats));
    if (rc == VPX_OK) ++numRenderedFrames;
    return rc;
}

int Renderer::CopyHistory(float* host_rgba) const {
    if (status_) return status_;
    if (!history_) return VPX_E_STATE;
    int rc = vpx_synchronize(ctx_);
    if (rc) return rc;
    return hipMemcpy(host_rgba, history_, sizeof(float) * 4 * width_ * height_, hipMemcpyDeviceToHost) == hipSuccess
               ? VPX_OK
               : VPX_E_DEVICE;
}

int Renderer::Tick(float /*deltaTime*/, vpx_stats* stats) {
    if (status_) return status_;
    if (staticCamera) return ReadPlayerLight(UpdateStatic(stats));
    if (flags & VPX_FLAG_DOF) {  // focus ray of Renderer::Tick (renderer.cpp:1987-1991)
        int rc = vpx_focus_distance(ctx_, width_, height_, &camera.focal_distance);
        if (rc) return rc;
        rc = vpx_set_camera(ctx_, &camera);
        if (rc) return rc;
    }
    return ReadPlayerLight(temporal ? UpdateTemporal(stats) : Update(stats));
}

// The moving-camera branch with temporal accumulation (no reference counterpart): vpx_render at
// frame_index 0 (the accumulator holds this tick's samples alone; the seed stream is the tick
// number's), vpx_render_ids, vpx_reproject_ids from the previous tick's ids, history and camera,
// then optionally vpx_denoise_ids on the new history; the screen shows the last of them.  The
// history, not the denoised image, is what the next tick reads.  Volumes whose matrices changed
// since the previous tick are followed.  Queued on the context's stream.
int Renderer::UpdateTemporal(vpx_stats* stats) {
    if (status_) return status_;
    if (!accumulator_) return VPX_E_STATE;
    const size_t pixels = (size_t)width_ * height_;
    if (!tHist_[0]) {
        if (hipSetDevice(device_) != hipSuccess || hipMalloc(&tIds_[0], 16 * pixels) != hipSuccess ||
            hipMalloc(&tIds_[1], 16 * pixels) != hipSuccess || hipMalloc(&tHist_[0], 16 * pixels) != hipSuccess ||
            hipMalloc(&tHist_[1], 16 * pixels) != hipSuccess ||
            (temporalDenoisePasses && !denoised_ && hipMalloc(&denoised_, 16 * pixels) != hipSuccess)) {
            err_ = "temporal buffer allocation failed";
            return VPX_E_NOMEM;
        }
        tValid_ = false;
    }
    const bool filter = temporalVariance || temporalDenoisePasses;
    if (filter && !denoised_ && hipMalloc(&denoised_, 16 * pixels) != hipSuccess) {
        err_ = "denoise buffer allocation failed";
        return VPX_E_NOMEM;
    }
    if (temporalVariance && !tMom_[0]) {  // switched on after the first tick: the history has no moments yet
        if (hipMalloc(&tMom_[0], 8 * pixels) != hipSuccess || hipMalloc(&tMom_[1], 8 * pixels) != hipSuccess) {
            err_ = "moments buffer allocation failed";
            return VPX_E_NOMEM;
        }
        tValid_ = false;
    }
    vpx_frame_params p{};
    p.width = width_, p.height = height_;
    p.max_bounces = maxBounces;
    p.frame_index = 0;
    p.seed_base = tTicks_ * (width_ * height_);
    p.flags = (flags & ~VPX_FLAG_SKY) | (activateSky ? VPX_FLAG_SKY : 0u);
    p.aa_strength = antiAliasingStrength;
    p.area_samples = numCheckShadowsAreaLight;
    p.sky[0] = sky[0], p.sky[1] = sky[1], p.sky[2] = sky[2];
    int rc = vpx_render(ctx_, &p, accumulator_, nullptr, stats);
    if (rc) return rc;
    numRenderedFrames = 1;
    const int cur = tCur_, prev = 1 - tCur_;
    if ((rc = vpx_render_ids(ctx_, &p, nullptr, tIds_[cur]))) return rc;
    vpx_reproject r{};
    r.cur = camera;
    vpx_prev_camera here{};
    if ((rc = vpx_prev_camera_look_at(camPos_, camTarget_, width_, height_, &here))) return rc;
    r.prev = tValid_ ? tPrevCamera_ : here;
    r.max_history = temporalMaxHistory;
    r.nohist_lo = temporalNohistLo, r.nohist_hi = temporalNohistHi;
    bool moved = false;
    if (tValid_ && tPrevVolumes_.size() == volumes_.size())
        for (size_t v = 0; v < volumes_.size() && !moved; ++v)
            moved = memcmp(volumes_[v].matrix, tPrevVolumes_[v].matrix, sizeof(volumes_[v].matrix)) != 0 ||
                    memcmp(volumes_[v].inv_matrix, tPrevVolumes_[v].inv_matrix, sizeof(volumes_[v].inv_matrix)) != 0;
    r.n_volumes = moved ? (uint32_t)volumes_.size() : 0u;
    uint32_t* target = nullptr;
    if ((rc = MapScreen(&target))) return rc;
    if (temporalVariance) {
        rc = vpx_reproject_moments(ctx_, &p, tIds_[cur], tValid_ ? tIds_[prev] : nullptr, accumulator_,
                                   tValid_ ? tHist_[prev] : nullptr, tValid_ ? tMom_[prev] : nullptr, tHist_[cur], tMom_[cur],
                                   nullptr, &r, moved ? volumes_.data() : nullptr, moved ? tPrevVolumes_.data() : nullptr);
        if (rc == VPX_OK)
            rc = vpx_denoise_var(ctx_, &p, tIds_[cur], tHist_[cur], tMom_[cur], denoised_, target, &temporalVarianceParams);
    } else {
        rc = vpx_reproject_ids(ctx_, &p, tIds_[cur], tValid_ ? tIds_[prev] : nullptr, accumulator_,
                               tValid_ ? tHist_[prev] : nullptr, tHist_[cur], temporalDenoisePasses ? nullptr : target, &r,
                               moved ? volumes_.data() : nullptr, moved ? tPrevVolumes_.data() : nullptr);
    }
    if (rc == VPX_OK && temporalDenoisePasses && !temporalVariance) {
        const vpx_denoise d{temporalDenoisePasses, temporalSigmaL, 0u, 0u};
        rc = vpx_denoise_ids(ctx_, &p, tIds_[cur], tHist_[cur], denoised_, target, &d);
    }
    rc = UnmapScreen(rc);
    if (rc) return rc;
    temporalHistory_ = tHist_[cur];
    tPrevCamera_ = here, tPrevVolumes_ = volumes_;
    tCur_ = prev, tValid_ = true, ++tTicks_;
    return VPX_OK;
}

int Renderer::CopyTemporalHistory(float* host_rgba) const {
    if (status_) return status_;
    if (!temporalHistory_) return VPX_E_STATE;
    const int rc = vpx_synchronize(ctx_);
    if (rc) return rc;
    return hipMemcpy(host_rgba, temporalHistory_, sizeof(float) * 4 * width_ * height_, hipMemcpyDeviceToHost) == hipSuccess
               ? VPX_OK
               : VPX_E_DEVICE;
}

int Renderer::ReadPlayerLight(int rc) {
    if (rc || !trackPlayerLight) return rc;
    rc = vpx_get_player_light(ctx_, &playerLight, 1);
    if (!rc) inLight = playerLight.in_light != 0;
    return rc;
}

static vpx_ray player_ray(const PlayerRay& ray) {
    vpx_ray r{};
    for (int i = 0; i < 3; ++i) r.origin[i] = ray.O[i], r.direction[i] = ray.D[i];
    r.tmax = ray.t;
    return r;
}

int Renderer::FindNearestPlayer(PlayerRay& ray, int32_t* vox_index) {
    if (status_) return status_;
    if (!vox_index) return VPX_E_INVALID;
    const vpx_ray r = player_ray(ray);
    const vpx_ray_filter f{1u, VPX_MAT_SMOKE_LOW_DENSITY, VPX_MAT_SMOKE_PLAYER, VPX_QUERY_NO_SHAPES | VPX_QUERY_RAW_DIRECTION};
    vpx_hit h{};
    const int rc = vpx_find_nearest_filtered(ctx_, &r, 1, &f, &h);
    if (rc) return rc;
    if (h.vox_index >= 0) {
        ray.t = h.t;
        for (int i = 0; i < 3; ++i) ray.rayNormal[i] = h.normal[i];
        ray.indexMaterial = h.material;
    }
    *vox_index = player_vox_index(h.vox_index, numVolumes_, currentChunk);
    return VPX_OK;
}

int Renderer::FindNearestCells(PlayerRay& ray, int32_t* vox_index, vpx_hit_cell* cell) {
    if (status_) return status_;
    if (!vox_index || !cell) return VPX_E_INVALID;
    const vpx_ray r = player_ray(ray);
    const vpx_ray_filter f{1u, VPX_MAT_SMOKE_LOW_DENSITY, VPX_MAT_SMOKE_PLAYER, VPX_QUERY_NO_SHAPES | VPX_QUERY_RAW_DIRECTION};
    vpx_hit h{};
    const int rc = vpx_find_nearest_cells(ctx_, &r, 1, &f, &h, cell);
    if (rc) return rc;
    if (h.vox_index >= 0) {
        ray.t = h.t;
        for (int i = 0; i < 3; ++i) ray.rayNormal[i] = h.normal[i];
        ray.indexMaterial = h.material;
    }
    *vox_index = player_vox_index(h.vox_index, numVolumes_, currentChunk);
    return VPX_OK;
}

int Renderer::PickPixel(uint32_t x, uint32_t y, const vpx_ray_filter* filter, vpx_hit* hit, vpx_hit_cell* cell) {
    if (status_) return status_;
    return vpx_pick_pixel(ctx_, width_, height_, x, y, filter, hit, cell);
}

int Renderer::Denoise(uint32_t passes, float sigma_l) {
    if (status_) return status_;
    if (!accumulator_) return VPX_E_STATE;
    const size_t pixels = (size_t)width_ * height_;
    if (!denoised_ && (hipSetDevice(device_) != hipSuccess || hipMalloc(&denoised_, sizeof(float) * 4 * pixels) != hipSuccess ||
                       hipMalloc(&ids_, sizeof(uint32_t) * 4 * pixels) != hipSuccess)) {
        err_ = "denoise buffer allocation failed";
        return VPX_E_NOMEM;
    }
    vpx_frame_params p{};
    p.width = width_, p.height = height_;
    int rc = vpx_render_ids(ctx_, &p, nullptr, ids_);
    if (rc) return rc;
    const vpx_denoise d{passes, sigma_l, 0u, 0u};
    uint32_t* target = nullptr;
    if ((rc = MapScreen(&target))) return rc;
    return UnmapScreen(vpx_denoise_ids(ctx_, &p, ids_, accumulator_, denoised_, target, &d));
}

int Renderer::DenoiseVariance(const vpx_denoise_var_params* d) {
    if (status_) return status_;
    if (!accumulator_) return VPX_E_STATE;
    const size_t pixels = (size_t)width_ * height_;
    if (hipSetDevice(device_) != hipSuccess ||
        (!denoised_ && hipMalloc(&denoised_, sizeof(float) * 4 * pixels) != hipSuccess) ||
        (!ids_ && hipMalloc(&ids_, sizeof(uint32_t) * 4 * pixels) != hipSuccess)) {
        err_ = "denoise buffer allocation failed";
        return VPX_E_NOMEM;
    }
    vpx_frame_params p{};
    p.width = width_, p.height = height_;
    int rc = vpx_render_ids(ctx_, &p, nullptr, ids_);
    if (rc) return rc;
    const vpx_denoise_var_params defaults{5u, 4.0f, 0.0009765625f, 1.0f, 0u, {0u, 0u, 0u}};
    uint32_t* target = nullptr;
    if ((rc = MapScreen(&target))) return rc;
    return UnmapScreen(vpx_denoise_var(ctx_, &p, ids_, accumulator_, nullptr, denoised_, target, d ? d : &defaults));
}

int Renderer::CastRays(const vpx_ray* rays, uint32_t n, const vpx_ray_filter* filter, const vpx_cast* opt, vpx_hit* hits,
                       vpx_hit_cell* cells) {
    if (status_) return status_;
    return vpx_cast_nearest(ctx_, rays, n, filter, opt, hits, cells);
}

int Renderer::CastOccluded(const vpx_ray* rays, uint32_t n, const vpx_ray_filter* filter, const vpx_cast* opt,
                           uint8_t* occluded) {
    if (status_) return status_;
    return vpx_cast_occluded(ctx_, rays, n, filter, opt, occluded);
}

int Renderer::CopyDenoised(float* host_rgba) const {
    if (status_) return status_;
    if (!denoised_) return VPX_E_STATE;
    const int rc = vpx_synchronize(ctx_);
    if (rc) return rc;
    return hipMemcpy(host_rgba, denoised_, sizeof(float) * 4 * width_ * height_, hipMemcpyDeviceToHost) == hipSuccess
               ? VPX_OK
               : VPX_E_DEVICE;
}

int Renderer::IsOccludedPlayerClimbable(const PlayerRay& ray, bool* occluded) {
    if (status_) return status_;
    if (!occluded) return VPX_E_INVALID;
    const vpx_ray r = player_ray(ray);
    const vpx_ray_filter f{1u, 1u, 0u, VPX_QUERY_NO_SHAPES | VPX_QUERY_RAW_DIRECTION};
    uint8_t occ = 0;
    const int rc = vpx_is_occluded_filtered(ctx_, &r, 1, &f, &occ);
    if (rc == VPX_OK) *occluded = occ != 0;
    return rc;
}

int Renderer::UseGLBuffer(unsigned int pbo) {
    if (status_) return status_;
    const int rc = vpx_gl_register_buffer(ctx_, pbo);
    glBuffer_ = rc == VPX_OK && pbo != 0u;
    return rc;
}

int Renderer::MapScreen(uint32_t** out) const {
    if (!glBuffer_) {
        *out = screen_;
        return VPX_OK;
    }
    size_t bytes = 0;
    int rc = vpx_gl_map(ctx_, out, &bytes);
    if (rc) return rc;
    if (bytes < sizeof(uint32_t) * (size_t)width_ * height_) {
        (void)vpx_gl_unmap(ctx_);
        return VPX_E_INVALID;  // the GL buffer is smaller than the frame
    }
    return VPX_OK;
}

int Renderer::UnmapScreen(int rc) const {
    if (!glBuffer_) return rc;
    const int rc2 = vpx_gl_unmap(ctx_);
    return rc ? rc : rc2;
}

int Renderer::CopyScreen(uint32_t* host_pixels) const {
    if (status_) return status_;
    uint32_t* src = nullptr;
    int rc = MapScreen(&src);
    if (rc) return rc;
    rc = vpx_synchronize(ctx_);
    if (rc == VPX_OK && hipMemcpy(host_pixels, src, sizeof(uint32_t) * width_ * height_, hipMemcpyDeviceToHost) != hipSuccess)
        rc = VPX_E_DEVICE;
    return UnmapScreen(rc);
}

int Renderer::CopyAccumulator(float* host_rgba) const {
    if (status_) return status_;
    int rc = vpx_synchronize(ctx_);
    if (rc) return rc;
    return hipMemcpy(host_rgba, accumulator_, sizeof(float) * 4 * width_ * height_, hipMemcpyDeviceToHost) ==
                   hipSuccess
               ? VPX_OK
               : VPX_E_DEVICE;
}

}  // namespace vpxhost
