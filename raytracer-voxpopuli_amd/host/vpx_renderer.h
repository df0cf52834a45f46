// vpx_renderer.h — C++ host mirror of the reference Renderer's hot-path surface.
//
// The reference keeps its game loop in `Renderer::Tick(float deltaTime)` (renderer.cpp:1972,
// virtual in template/precomp.h:399) and renders with `Renderer::Update()`
// (renderer.cpp:1646-1891): a parallel loop over pixels calling `Trace(ray, maxBounces)`,
// a running-average accumulator and a Reinhard-Jodie tonemap into `Surface::pixels`.
// This class keeps that surface — same member names, same meaning — and replaces the loop
// by ONE call into libvpx_hip.so (include/vpx.h).  It talks to the library only through
// the C-ABI; HIP is used here just for the two HBM frame buffers and the D2H copy.
//
// Errors: every method returns the VPX_* status of the first failing call (0 = ok) and
// never throws; `LastError()` is the library's message.
#pragma once

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/vpx.h"

namespace vpxhost {

// The end of Renderer::FindNearestPlayer (renderer.cpp:1068-1069): from chunk 2 on, an index
// above size() - 4 in the reference's unsigned compare becomes -1 — the last three volumes,
// and a miss too (-2 is a huge uint32_t; size() - 4 is a size_t and wraps below four volumes).
inline int32_t player_vox_index(int32_t vox, size_t n_volumes, int32_t current_chunk) {
    if (current_chunk >= 2 && static_cast<uint32_t>(vox) > n_volumes - 4) return -1;
    return vox;
}

// The fields of the reference Ray (template/scene.h) that the player's casts read and write.
struct PlayerRay {
    float O[3], D[3];  // D is used as given (PlayerCharacter::GetRay normalises by itself)
    float t;
    float rayNormal[3] = {0, 0, 0};
    uint32_t indexMaterial = VPX_MAT_NONE;
};

class Renderer {
public:
    explicit Renderer(int device = 0);
    // A device set (vpx_create_multi): frames tile-sharded over `devices`, gathered over
    // RCCL to devices[0], where the accumulator and screen live.
    explicit Renderer(const std::vector<int>& devices);
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    // Renderer::Init minus window/asset/game setup (renderer.cpp:688-736): frame buffers.
    int Init(uint32_t width, uint32_t height);

    // --- world (the host owns Scene::grid; the library keeps the device copy) -----------
    int UploadGrid(uint32_t grid_id, const uint8_t* cells, uint32_t n);  // Scene::grid
    int SetVolumes(const std::vector<vpx_volume>& volumes);               // voxelVolumes
    int SetMaterials(const std::vector<vpx_material>& materials);         // materials
    int SetLights(const std::vector<vpx_point_light>& points, const std::vector<vpx_spot_light>& spots,
                  const std::vector<vpx_area_light>& areas, const vpx_dir_light& dir);
    int SetShapes(const std::vector<vpx_sphere>& spheres, const std::vector<vpx_triangle>& triangles);
    // Camera::camPos / camTarget + HandleInput(0) (template/camera.h:113-181).
    int LookAt(const float pos[3], const float target[3]);
    // skyPixels / skyWidth / skyHeight (stbi_loadf RGB floats, renderer.cpp:691) and
    // HDRLightContribution; sampled when activateSky is set.  rgb == nullptr removes it.
    int SetSky(const float* rgb, uint32_t width, uint32_t height, float hdr_contribution);
    // prevCamera = the current camera (CopyToPrevCamera, renderer.cpp:1893-1902).
    int CopyToPrevCamera();
    // The reference's own x86 arithmetic (FastReciprocal in FindNearest, rsqrtps for the
    // primary rays) as this host computes it: VPX_ARITH_X86_HOST; VPX_ARITH_EXACT (default).
    int SetArithmetic(uint32_t mode);

    // --- model loaders (template/scene.cpp:449-683) on the device: no host grid ------------
    // A decoded .vox model (vpx_vox_decode) made resident; palette_rgba (1024 bytes, may be
    // nullptr) stays on the host for LoadModel's material override.
    int UploadModel(uint32_t model_id, const uint8_t* voxels, uint32_t sx, uint32_t sy, uint32_t sz,
                    const uint8_t* palette_rgba);
    // Scene(position, n) without a host grid: the grid a volume's loaders fill (UploadGrid
    // records its size too).
    void CreateGrid(uint32_t grid_id, uint32_t n);
    // Scene::LoadModel (:449-529) into the volume's grid, then its palette override of
    // Renderer::materials (:516-520) and the table re-sent.
    int LoadModel(uint32_t volume, uint32_t model_id);
    int LoadModelPartial(uint32_t volume, uint32_t model_id, uint32_t columns, uint32_t thickness);  // :531-604
    // :606-683; draws Rand(SMOKE_MID2_DENSITY, SMOKE_HIGH_DENSITY) from, and advances, `seed`.
    int LoadModelRandomMaterials(uint32_t volume, uint32_t model_id);
    // Scene::scaleModel of a volume ((1, 1, 1) until a loader multiplies it).
    const float* ScaleModel(uint32_t volume);
    // Scene::GenerateSomeNoise (template/scene.cpp:226-282) and GenerateSomeSmoke (:285-356) into the
    // volume's grid on the device, as voxelVolumes[5].GenerateSomeSmoke(0.167f) (renderer.cpp:626,
    // 2174) and the volume UI (:2883-2898); the draws come from, and advance, `seed`.
    int GenerateSomeNoise(uint32_t volume, float frequency = 0.03f, vpx_noise_result* out = nullptr);
    int GenerateSomeSmoke(uint32_t volume, float frequency = 0.001f, vpx_noise_result* out = nullptr);

    // --- per frame -----------------------------------------------------------------------
    void ResetAccumulator() { numRenderedFrames = 0; }  // renderer.cpp:343-346
    int Update(vpx_stats* stats = nullptr);             // renderer.cpp:1646-1891
    // Tick: moving camera -> focus ray + Update; staticCamera -> the reprojection branch
    // (renderer.cpp:1996-2101) through vpx_render_reproject with the history in HBM.
    int Tick(float deltaTime, vpx_stats* stats = nullptr);
    // Surface::pixels (0x00RRGGBB, W*H) for display: device -> host copy of the frame.
    int CopyScreen(uint32_t* host_pixels) const;
    // Display interop in place of GLTexture::CopyFrom (template/opengl.cpp:144-149): with a
    // GL pixel-unpack buffer of W*H*4 bytes registered (its GL context current on this
    // thread), Update / Tick pack the frame straight into it (vpx_gl_map -> render ->
    // vpx_gl_unmap) and the window updates its texture from the buffer; CopyScreen then reads
    // the screen out of it.  pbo == 0 returns to the HBM screen.
    int UseGLBuffer(unsigned int pbo);
    int CopyAccumulator(float* host_rgba) const;
    int CopyHistory(float* host_rgba) const;  // illuminationHistoryBuffer (static branch)

    // --- the player's casts (Renderer::Tick, renderer.cpp:2139-2152) -----------------------
    // Renderer::FindNearestPlayer (renderer.cpp:1020-1071): volumes 1 .. n-1 (0 is the player),
    // smoke passed through (Scene::FindNearestExcept), no spheres / triangles.  *vox_index = the
    // volume index after player_vox_index; on a hit t, rayNormal and indexMaterial are updated.
    int FindNearestPlayer(PlayerRay& ray, int32_t* vox_index);
    // The same cast with the hit cell (vpx_find_nearest_cells): *cell names the cell the player
    // points at and, with VPX_CELL_FACE, the empty neighbour a new voxel would go into.
    int FindNearestCells(PlayerRay& ray, int32_t* vox_index, vpx_hit_cell* cell);
    // The hit and the hit cell under pixel (x, y) of the frame (vpx_pick_pixel; filter NULL =
    // everything).  Which pixel to pick and what to do with the cell is the game's business.
    int PickPixel(uint32_t x, uint32_t y, const vpx_ray_filter* filter, vpx_hit* hit, vpx_hit_cell* cell);
    // The plane-keyed a-trous filter of the current accumulator (vpx_render_ids, then
    // vpx_denoise_ids; no reference counterpart: the reference shows a moving camera's frame as
    // it is): `passes` passes (1..5), sigma_l 0 = plane key only, the result in the denoised
    // image (CopyDenoised) and tonemapped into the screen.  Queued on the context's stream.
    int Denoise(uint32_t passes = 5, float sigma_l = 0.0f);
    // The same with a per-pixel luminance tolerance (vpx_denoise_var without moments: the variance
    // of each pixel's 5x5 neighbourhood on its plane); d NULL: 5 passes, sigma_v 4, epsilon 2^-10.
    int DenoiseVariance(const vpx_denoise_var_params* d = nullptr);
    int CopyDenoised(float* host_rgba) const;
    // Temporal accumulation under camera motion (vpx_reproject_ids; no reference counterpart: the
    // reference resets its accumulator when the camera moves).  With `temporal` set, Tick's
    // moving-camera branch renders one sample per pixel, carries the previous tick's history to the
    // new camera where the ID buffer names the same plane, and optionally runs the plane-keyed
    // filter on the result (temporalDenoisePasses > 0); the history image is kept for the next tick
    // (CopyTemporalHistory reads it, .w the history length).  DropHistory starts afresh; so does a
    // resize (Init).  Off by default.
    bool temporal = false;
    float temporalMaxHistory = 32.0f;
    uint32_t temporalNohistLo = 5, temporalNohistHi = 14;  // metal, glass, smoke: view-dependent
    uint32_t temporalDenoisePasses = 0;
    float temporalSigmaL = 0.0f;
    // temporalVariance: the luminance's first two moments ride along the history
    // (vpx_reproject_moments) and the filter on the result is vpx_denoise_var with these
    // parameters (in place of temporalDenoisePasses / temporalSigmaL): pixels whose history is at
    // least min_history frames long take their temporal variance, the others their neighbourhood's.
    bool temporalVariance = false;
    vpx_denoise_var_params temporalVarianceParams{5u, 4.0f, 0.0009765625f, 4.0f, 0u, {0u, 0u, 0u}};
    void DropHistory() { tValid_ = false; }  // the moments go with the history
    void ResetTemporal() { DropHistory(); }
    int CopyTemporalHistory(float* host_rgba) const;
    // Ray batches that already live on the device (vpx_cast_nearest / vpx_cast_occluded; no reference
    // counterpart: per ray the records of Renderer::FindNearest / IsOccluded): rays, hits, cells and
    // occluded are DEVICE pointers of n elements, cells may be NULL; filter NULL = everything, opt
    // NULL = the library's choice of form.  Queued on the context's stream like Denoise, no
    // synchronisation: read the records after vpx_synchronize or from a later kernel on that stream.
    int CastRays(const vpx_ray* rays, uint32_t n, const vpx_ray_filter* filter, const vpx_cast* opt, vpx_hit* hits,
                 vpx_hit_cell* cells);
    int CastOccluded(const vpx_ray* rays, uint32_t n, const vpx_ray_filter* filter, const vpx_cast* opt, uint8_t* occluded);
    // Renderer::IsOccludedPlayerClimbable (renderer.cpp:245-273).
    int IsOccludedPlayerClimbable(const PlayerRay& ray, bool* occluded);

    const char* LastError() const;
    vpx_ctx* Context() const { return ctx_; }

    // Members of the reference Renderer this path reads (renderer.h:175-205).
    int32_t maxBounces = 0;
    uint32_t numRenderedFrames = 0;
    float antiAliasingStrength = 1.0f;
    int32_t numCheckShadowsAreaLight = 3;
    bool staticCamera = false;  // renderer.h:229: Tick takes the reprojection branch
    bool activateSky = false;   // renderer.h:216 (needs SetSky; the reference's HDR is missing)
    uint32_t flags = 0;         // VPX_FLAG_AA / VPX_FLAG_DOF
    float sky[3] = {0.392f, 0.584f, 0.829f};  // SampleSky, activateSky == false (renderer.cpp:2310-2313)
    vpx_camera camera{};
    vpx_prev_camera prevCamera{};  // renderer.h:182
    // renderer.h:231: a path reached the player's smoke (volume 0) and found more light there
    // than VPX_PLAYER_LIGHT_SQR.  Tick keeps it up to date only while trackPlayerLight is set
    // (off by default: the read synchronises once per Tick, which frames in flight exist to
    // avoid): it reads and resets the record after the render on both branches, as the
    // reference's Tick reads the flag (renderer.cpp:2112-2118) and clears it (:2206).
    bool inLight = false;
    bool trackPlayerLight = false;
    vpx_player_light playerLight{};  // the last tracked Tick's record
    int32_t currentChunk = 0;        // read by FindNearestPlayer (renderer.cpp:1068)
    uint32_t seed = 0x12345678u;     // the xorshift32 state the loaders and generators draw from (tmpl8math.cpp:16)

private:
    int Load(uint32_t volume, uint32_t model_id, vpx_model_load in, vpx_model_result* out);
    int Generate(uint32_t volume, uint32_t mode, float frequency, vpx_noise_result* out);
    struct Model { std::vector<uint8_t> voxels, palette; };
    std::vector<Model> models_;
    std::vector<vpx_volume> volumes_;      // voxelVolumes as SetVolumes left them
    std::vector<vpx_material> materials_;  // materials as SetMaterials / LoadModel left them
    std::vector<uint32_t> gridSize_;       // grid id -> n (0: unknown)
    std::vector<std::array<float, 3>> scaleModel_;
    size_t numVolumes_ = 0;  // voxelVolumes.size() as SetVolumes left it
    int UpdateStatic(vpx_stats* stats);
    int UpdateTemporal(vpx_stats* stats);
    int ReadPlayerLight(int rc);  // after a Tick's render (rc: its status)
    int MapScreen(uint32_t** out) const;  // the frame's RGB8 target: the GL buffer or screen_
    int UnmapScreen(int rc) const;
    bool glBuffer_ = false;
    float camPos_[3] = {0, 0, 0}, camTarget_[3] = {0, 0, 1};
    bool havePrev_ = false;
    float* history_ = nullptr;      // illuminationHistoryBuffer float4[W*H] in HBM
    int status_ = VPX_OK;
    int device_ = 0;
    vpx_ctx* ctx_ = nullptr;
    uint32_t width_ = 0, height_ = 0;
    float* accumulator_ = nullptr;  // float4[W*H] in HBM
    uint32_t* screen_ = nullptr;    // uint32[W*H] in HBM
    float* denoised_ = nullptr;     // Denoise(): float4[W*H] in HBM
    uint32_t* ids_ = nullptr;       // ... and its ID buffer, uint4[W*H]
    uint32_t* tIds_[2] = {nullptr, nullptr};  // UpdateTemporal(): this tick's and the previous tick's ids ...
    float* tHist_[2] = {nullptr, nullptr};    // ... and history images, swapped per tick
    float* tMom_[2] = {nullptr, nullptr};     // ... and, with temporalVariance, moments images (float2[W*H])
    float* temporalHistory_ = nullptr;        // the one the last tick wrote
    int tCur_ = 0;
    bool tValid_ = false;
    uint32_t tTicks_ = 0;
    vpx_prev_camera tPrevCamera_{};
    std::vector<vpx_volume> tPrevVolumes_;
    std::string err_;
};

// src/Game/ModifyingProp.{h,cpp}: every toChange seconds (0.9 in the game) the prop's Scene shows
// the next slice of its model.  Update() is one due edit (the timer stays with the host): one
// call into the library instead of a host loop, a ResetGrid and a box upload.
struct ModifyingProp {
    Renderer& renderer;
    uint32_t volume, model_id;
    uint32_t index, increaseRate;
    int Update() {  // ModifyingProp.cpp:11-21
        const int rc = renderer.LoadModelPartial(volume, model_id, index, increaseRate);
        index += increaseRate;
        if (index > 64) index = increaseRate;
        return rc;
    }
};

}  // namespace vpxhost
