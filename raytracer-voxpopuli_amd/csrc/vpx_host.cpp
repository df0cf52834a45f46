// vpx_host.cpp — host-side helpers of libvpx_hip.so that restate reference HOST code
// (camera basis, volume transforms, the default material table).  No device work.
//
// They exist so a caller that does not link the tmpl8 template (tests, bench, the C++
// host mirror in host/) builds exactly the inputs the reference would hand the trace
// path.  Float expressions keep the reference's operand order (built -ffp-contract=off);
// sinf/cosf are the correctly rounded values (f64 evaluation), as on the device.
#include <cmath>
#include <cstring>
#include <new>
#include <utility>
#include <vector>

#include "../../include/vpx.h"
#include "vpx_model.hpp"
#include "vpx_noise.hpp"
#include "vpx_brush.hpp"
#include "vpx_stamp.hpp"
#include "vpx_denoise.hpp"
#include "vpx_denoise_var.hpp"
#include "vpx_reproject.hpp"
#include "vpx_skip.hpp"

namespace {

struct v3 {
    float x, y, z;
};
inline v3 add(v3 a, v3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline v3 sub(v3 a, v3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline v3 mul(v3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline v3 cross(v3 a, v3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline v3 normalize(v3 v) {  // tmpl8math.h:2350-2354 (rsqrtf = 1 / sqrtf)
    const float inv = 1.0f / std::sqrt(dot(v, v));
    return mul(v, inv);
}
inline void put(float* d, v3 v) { d[0] = v.x, d[1] = v.y, d[2] = v.z; }

// mat4 (tmpl8math.h:2592-2873): row-major cells, default identity.
struct mat4 {
    float c[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
};
mat4 matmul(const mat4& a, const mat4& b) {  // operator*(mat4, mat4), tmpl8math.cpp:281-294
    mat4 r;
    for (int i = 0; i < 16; i += 4)
        for (int j = 0; j < 4; ++j)
            r.c[i + j] = (a.c[i + 0] * b.c[j + 0]) + (a.c[i + 1] * b.c[j + 4]) + (a.c[i + 2] * b.c[j + 8]) +
                         (a.c[i + 3] * b.c[j + 12]);
    return r;
}
mat4 translate(v3 p) {
    mat4 r;
    r.c[3] = p.x, r.c[7] = p.y, r.c[11] = p.z;
    return r;
}
mat4 scale(v3 s) {
    mat4 r;
    r.c[0] = s.x, r.c[5] = s.y, r.c[10] = s.z;
    return r;
}

// 4x4 inverse by cofactors (the MESA gluInvertMatrix formulation that mat4::Inverted
// uses, tmpl8math.h:2828-2873), products and sums evaluated left to right.
mat4 inverted(const mat4& m) {
    const float* c = m.c;
    float inv[16];
    inv[0] = c[5] * c[10] * c[15] - c[5] * c[11] * c[14] - c[9] * c[6] * c[15] + c[9] * c[7] * c[14] +
             c[13] * c[6] * c[11] - c[13] * c[7] * c[10];
    inv[1] = -c[1] * c[10] * c[15] + c[1] * c[11] * c[14] + c[9] * c[2] * c[15] - c[9] * c[3] * c[14] -
             c[13] * c[2] * c[11] + c[13] * c[3] * c[10];
    inv[2] = c[1] * c[6] * c[15] - c[1] * c[7] * c[14] - c[5] * c[2] * c[15] + c[5] * c[3] * c[14] +
             c[13] * c[2] * c[7] - c[13] * c[3] * c[6];
    inv[3] = -c[1] * c[6] * c[11] + c[1] * c[7] * c[10] + c[5] * c[2] * c[11] - c[5] * c[3] * c[10] -
             c[9] * c[2] * c[7] + c[9] * c[3] * c[6];
    inv[4] = -c[4] * c[10] * c[15] + c[4] * c[11] * c[14] + c[8] * c[6] * c[15] - c[8] * c[7] * c[14] -
             c[12] * c[6] * c[11] + c[12] * c[7] * c[10];
    inv[5] = c[0] * c[10] * c[15] - c[0] * c[11] * c[14] - c[8] * c[2] * c[15] + c[8] * c[3] * c[14] +
             c[12] * c[2] * c[11] - c[12] * c[3] * c[10];
    inv[6] = -c[0] * c[6] * c[15] + c[0] * c[7] * c[14] + c[4] * c[2] * c[15] - c[4] * c[3] * c[14] -
             c[12] * c[2] * c[7] + c[12] * c[3] * c[6];
    inv[7] = c[0] * c[6] * c[11] - c[0] * c[7] * c[10] - c[4] * c[2] * c[11] + c[4] * c[3] * c[10] +
             c[8] * c[2] * c[7] - c[8] * c[3] * c[6];
    inv[8] = c[4] * c[9] * c[15] - c[4] * c[11] * c[13] - c[8] * c[5] * c[15] + c[8] * c[7] * c[13] +
             c[12] * c[5] * c[11] - c[12] * c[7] * c[9];
    inv[9] = -c[0] * c[9] * c[15] + c[0] * c[11] * c[13] + c[8] * c[1] * c[15] - c[8] * c[3] * c[13] -
             c[12] * c[1] * c[11] + c[12] * c[3] * c[9];
    inv[10] = c[0] * c[5] * c[15] - c[0] * c[7] * c[13] - c[4] * c[1] * c[15] + c[4] * c[3] * c[13] +
              c[12] * c[1] * c[7] - c[12] * c[3] * c[5];
    inv[11] = -c[0] * c[5] * c[11] + c[0] * c[7] * c[9] + c[4] * c[1] * c[11] - c[4] * c[3] * c[9] -
              c[8] * c[1] * c[7] + c[8] * c[3] * c[5];
    inv[12] = -c[4] * c[9] * c[14] + c[4] * c[10] * c[13] + c[8] * c[5] * c[14] - c[8] * c[6] * c[13] -
              c[12] * c[5] * c[10] + c[12] * c[6] * c[9];
    inv[13] = c[0] * c[9] * c[14] - c[0] * c[10] * c[13] - c[8] * c[1] * c[14] + c[8] * c[2] * c[13] +
              c[12] * c[1] * c[10] - c[12] * c[2] * c[9];
    inv[14] = -c[0] * c[5] * c[14] + c[0] * c[6] * c[13] + c[4] * c[1] * c[14] - c[4] * c[2] * c[13] -
              c[12] * c[1] * c[6] + c[12] * c[2] * c[5];
    inv[15] = c[0] * c[5] * c[10] - c[0] * c[6] * c[9] - c[4] * c[1] * c[10] + c[4] * c[2] * c[9] +
              c[8] * c[1] * c[6] - c[8] * c[2] * c[5];
    const float det = c[0] * inv[0] + c[1] * inv[4] + c[2] * inv[8] + c[3] * inv[12];
    mat4 r;
    if (det != 0) {
        const float invdet = 1.0f / det;
        for (int i = 0; i < 16; i++) r.c[i] = inv[i] * invdet;
    }
    return r;
}

// quat (tmpl8math.h:2951-3066): fromAxisAngle, Hamilton product, toMatrix.
struct quat {
    float w = 1, x = 0, y = 0, z = 0;
};
quat from_axis_angle(v3 axis, float theta) {
    quat q;
    q.w = (float)std::cos((double)(theta / 2));
    const float s = (float)std::sin((double)(theta / 2));
    q.x = axis.x * s, q.y = axis.y * s, q.z = axis.z * s;
    return q;
}
quat qmul(const quat& a, const quat& q) {
    quat r;
    r.w = a.w * q.w - a.x * q.x - a.y * q.y - a.z * q.z;
    r.x = a.w * q.x + a.x * q.w + a.y * q.z - a.z * q.y;
    r.y = a.w * q.y - a.x * q.z + a.y * q.w + a.z * q.x;
    r.z = a.w * q.z + a.x * q.y - a.y * q.x + a.z * q.w;
    return r;
}
mat4 to_matrix(const quat& q) {
    const float w = q.w, x = q.x, y = q.y, z = q.z;
    mat4 m;
    m.c[0] = 1 - 2 * y * y - 2 * z * z;
    m.c[1] = 2 * x * y - 2 * w * z, m.c[2] = 2 * x * z + 2 * w * y, m.c[4] = 2 * x * y + 2 * w * z;
    m.c[5] = 1 - 2 * x * x - 2 * z * z;
    m.c[6] = 2 * y * z - 2 * w * x, m.c[8] = 2 * x * z - 2 * w * y, m.c[9] = 2 * y * z + 2 * w * x;
    m.c[10] = 1 - 2 * x * x - 2 * y * y;
    return m;
}

}  // namespace

extern "C" {

// Camera basis as Camera::HandleInput(0) leaves it with no key held (camera.h:113-181).
static void look_at_basis(const float pos[3], const float target[3], v3& cam, v3& ahead, v3& right, v3& up) {
    cam = {pos[0], pos[1], pos[2]};
    v3 tgt = {target[0], target[1], target[2]};
    const v3 tmp_up = {0, 1, 0};
    ahead = normalize(sub(tgt, cam));
    right = normalize(cross(tmp_up, ahead));
    up = normalize(cross(ahead, right));
    ahead = normalize(sub(tgt, cam));
    right = normalize(cross(tmp_up, ahead));
    up = normalize(cross(ahead, right));
    tgt = add(cam, ahead);
    ahead = normalize(sub(tgt, cam));
    up = normalize(cross(ahead, right));
    right = normalize(cross(up, ahead));
}

int vpx_camera_look_at(const float pos[3], const float target[3], uint32_t width, uint32_t height,
                       vpx_camera* out) {
    if (!pos || !target || !out || !width || !height) return VPX_E_INVALID;
    v3 cam, ahead, right, up;
    look_at_basis(pos, target, cam, ahead, right, up);
    const float aspect = (float)width / (float)height;  // ASPECT, camera.h:183
    const v3 base = add(cam, mul(ahead, 2.0f));
    put(out->cam_pos, cam);
    put(out->top_left, add(sub(base, mul(right, aspect)), up));
    put(out->top_right, add(add(base, mul(right, aspect)), up));
    put(out->bottom_left, sub(sub(base, mul(right, aspect)), up));
    put(out->right, right);
    put(out->up, up);
    out->focal_distance = 1.0f;  // Camera::focalDistance default, camera.h:189
    out->defocus_jitter = 2.0f;  // Camera::defocusJitter default, camera.h:191
    return VPX_OK;
}

int vpx_prev_camera_look_at(const float pos[3], const float target[3], uint32_t width, uint32_t height,
                            vpx_prev_camera* out) {
    if (!pos || !target || !out || !width || !height) return VPX_E_INVALID;
    v3 cam, ahead, right, up;
    look_at_basis(pos, target, cam, ahead, right, up);
    const float aspect = (float)width / (float)height;
    const v3 a2 = mul(ahead, 2.0f);  // 2 * ahead
    const v3 lf = sub(a2, mul(right, aspect)), rf = add(a2, mul(right, aspect));
    const v3 tf = add(a2, up), bf = sub(a2, up);
    std::memset(out, 0, sizeof(*out));
    put(out->cam_pos, cam);
    put(out->left_normal, cross(up, lf));
    put(out->right_normal, cross(rf, up));
    put(out->top_normal, cross(right, tf));
    put(out->bottom_normal, cross(bf, right));
    return VPX_OK;
}

// Scene(position, N) cube + Scene::SetTransform(rotation) with Scene::scale = scale and
// Scene::position (the member, distinct from the cube position) = 0
// (template/scene.cpp:213-217, 373-405, 431-445).
int vpx_volume_set_transform(const float position[3], const float scl[3], const float rotation[3],
                             vpx_volume* out) {
    if (!position || !scl || !rotation || !out) return VPX_E_INVALID;
    const v3 b0 = {position[0], position[1], position[2]};
    const v3 b1 = add(b0, v3{1, 1, 1});
    const v3 center = mul(add(b0, b1), 0.5f);
    const mat4 to_pivot = translate(add(center, v3{0, 0, 0}));
    const mat4 back = translate(v3{-center.x, -center.y, -center.z});
    const mat4 s = scale(v3{scl[0], scl[1], scl[2]});
    quat q = from_axis_angle(v3{1, 0, 0}, rotation[0]);
    q = qmul(from_axis_angle(v3{0, 1, 0}, rotation[1]), q);
    q = qmul(from_axis_angle(v3{0, 0, 1}, rotation[2]), q);
    const mat4 rot = to_matrix(q);
    const mat4 m = matmul(matmul(matmul(to_pivot, s), rot), back);
    const mat4 inv = inverted(matmul(matmul(matmul(to_pivot, rot), s), back));
    std::memcpy(out->matrix, m.c, sizeof(m.c));
    std::memcpy(out->inv_matrix, inv.c, sizeof(inv.c));
    put(out->b0, b0);
    put(out->b1, b1);
    return VPX_OK;
}

// Renderer::MaterialSetUp (renderer.cpp:357-443); entries 16..255 white, roughness 1.
int vpx_default_materials(vpx_material* out) {
    if (!out) return VPX_E_INVALID;
    auto mk = [](float r, float g, float b, float rough) {
        vpx_material m{};
        m.albedo[0] = r, m.albedo[1] = g, m.albedo[2] = b;
        m.roughness = rough;
        m.emissive = 0.0f;
        m.ior = 1.5f;  // Material::IOR default, Material.h:11
        return m;
    };
    for (int i = 0; i < VPX_NUM_MATERIALS; ++i) out[i] = mk(1, 1, 1, 1.0f);
    out[0] = mk(1, 1, 1, 1.0f);      // NON_METAL_WHITE
    out[1] = mk(1, 0, 0, 0.6f);      // NON_METAL_RED
    out[2] = mk(0, 0, 1, 0.25f);     // NON_METAL_BLUE
    out[3] = mk(0, 1, 0, 0.0f);      // NON_METAL_GREEN
    out[4] = mk(1, .6f, .8f, 0.3f);  // NON_METAL_PINK (partialMetal)
    out[5] = mk(1, 1, 1, 1.0f);      // METAL_HIGH
    out[6] = mk(0, 1, 1, 0.5f);      // METAL_MID
    out[7] = mk(0.9f, 0.9f, 0.9f, 0.01f);  // METAL_LOW
    out[8] = mk(1, 0.5f, 1, 1.0f);   // GLASS
    out[8].ior = 1.45f;
    const float smoke_em[6] = {3.0f, 8.0f, 12.0f, 15.0f, 16.0f, 22.0f};
    for (int i = 0; i < 6; ++i) {    // SMOKE_LOW_DENSITY .. SMOKE_PLAYER
        out[9 + i] = mk(1.0f, 0.7f, 1.0f, 1.0f);
        out[9 + i].ior = 1.0f;
        out[9 + i].emissive = smoke_em[i];
    }
    out[14].albedo[0] = out[14].albedo[1] = out[14].albedo[2] = 0.0f;  // smoke5 float3{0}
    out[15] = mk(1.0f, 0.7f, 1.0f, 1.0f);  // EMISSIVE
    out[15].emissive = 5.0f;
    return VPX_OK;
}

}  // extern "C"

// Fixed POD layouts of the ABI (mirrored by raytracer-voxpopuli_amd/abi.py STRUCT_SIZES).
static_assert(sizeof(vpx_volume) == 160, "vpx_volume layout");
static_assert(sizeof(vpx_material) == 32, "vpx_material layout");
static_assert(sizeof(vpx_point_light) == 24 && sizeof(vpx_spot_light) == 40, "light layout");
static_assert(sizeof(vpx_profile) == 160, "vpx_profile layout");
static_assert(sizeof(vpx_prev_camera) == 64, "vpx_prev_camera layout");
static_assert(sizeof(vpx_player_light) == 24 && sizeof(vpx_ray_probe) == 16, "player light layout");
static_assert(sizeof(vpx_ray_filter) == 16, "ray filter layout");
static_assert(sizeof(vpx_hit_cell) == 32, "hit cell layout");
static_assert(sizeof(vpx_cast) == 16 && offsetof(vpx_cast, max_waves) == 4 && offsetof(vpx_cast, reserved) == 8, "cast options layout");
static_assert(sizeof(vpx_model_load) == 40 && sizeof(vpx_model_result) == 16, "model load layout");
static_assert(sizeof(vpx_noise_gen) == 16 && sizeof(vpx_noise_result) == 16, "noise generator layout");
static_assert(sizeof(vpx_brush) == 48 && sizeof(vpx_brush_result) == 16, "brush layout");
static_assert(sizeof(vpx_stamp) == 32 && offsetof(vpx_stamp, orient) == 16 && offsetof(vpx_stamp, value) == 24 &&
                  offsetof(vpx_stamp, reserved2) == 28 && sizeof(vpx_stamp_source) == 24 && offsetof(vpx_stamp_source, sx) == 8,
              "stamp layout");
static_assert(sizeof(vpx_area_light) == 32 && sizeof(vpx_dir_light) == 24, "light layout");
static_assert(sizeof(vpx_sphere) == 32 && sizeof(vpx_triangle) == 64, "shape layout");
static_assert(sizeof(vpx_camera) == 80 && sizeof(vpx_frame_params) == 48, "camera/frame layout");
static_assert(sizeof(vpx_ray) == 32 && sizeof(vpx_hit) == 32 && sizeof(vpx_stats) == 40, "ray/hit/stats layout");
static_assert(sizeof(vpx_bvh_tri) == 36 && sizeof(vpx_bvh_node) == 32, "bvh layout");

// ---------------------------------------------------------------------- BasicBVH
// src/BVH/BasicBVH.cpp, host side: the constructor's triangle set and BuildBVH.  The
// device traversal is vpx_bvh_intersect (vpx_kernels.hip).
namespace {

struct BvhBuilder {
    const vpx_bvh_tri* tri;
    vpx_bvh_node* node;
    uint32_t* idx;
    std::vector<v3> centroid;
    uint32_t used = 1;

    static float lo(float a, float b) { return a < b ? a : b; }  // fminf, tmpl8math.h:401-404
    static float hi(float a, float b) { return a > b ? a : b; }  // fmaxf, tmpl8math.h:406-409

    // UpdateNodeBounds (BasicBVH.cpp:87-103): vertex0, vertex1, vertex2 folded in that order
    void bounds(uint32_t ni) {
        vpx_bvh_node& nd = node[ni];
        float mn[3] = {1e30f, 1e30f, 1e30f}, mx[3] = {-1e30f, -1e30f, -1e30f};
        for (uint32_t i = 0; i < nd.tri_count; ++i) {
            const vpx_bvh_tri& t = tri[idx[nd.left_first + i]];
            for (const float* v : {t.v0, t.v1, t.v2})
                for (int k = 0; k < 3; ++k) mn[k] = lo(mn[k], v[k]), mx[k] = hi(mx[k], v[k]);
        }
        std::memcpy(nd.aabb_min, mn, sizeof mn);
        std::memcpy(nd.aabb_max, mx, sizeof mx);
    }

    // Subdivide (BasicBVH.cpp:105-136): midpoint of the longest axis, in-place partition
    void split(uint32_t ni) {
        vpx_bvh_node& nd = node[ni];
        if (nd.tri_count <= 2) return;
        const float ext[3] = {nd.aabb_max[0] - nd.aabb_min[0], nd.aabb_max[1] - nd.aabb_min[1],
                              nd.aabb_max[2] - nd.aabb_min[2]};
        int axis = ext[1] > ext[0] ? 1 : 0;
        if (ext[2] > ext[axis]) axis = 2;
        const float pos = nd.aabb_min[axis] + ext[axis] * 0.5f;
        int i = (int)nd.left_first, j = i + (int)nd.tri_count - 1;
        while (i <= j) {
            const v3& c = centroid[idx[i]];
            if ((axis == 0 ? c.x : axis == 1 ? c.y : c.z) < pos)
                ++i;
            else
                std::swap(idx[i], idx[j--]);
        }
        const uint32_t left = (uint32_t)(i - (int)nd.left_first);
        if (left == 0 || left == nd.tri_count) return;
        const uint32_t l = used++, r = used++;
        node[l].left_first = nd.left_first, node[l].tri_count = left;
        node[r].left_first = (uint32_t)i, node[r].tri_count = nd.tri_count - left;
        nd.left_first = l, nd.tri_count = 0;
        bounds(l);
        bounds(r);
        split(l);
        split(r);
    }
};

float bvh_random_float(uint32_t& s) {  // RandomFloat (tmpl8math.cpp:119-133)
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return (float)s * 2.3283064365387e-10f;
}

}  // namespace

extern "C" {

int vpx_bvh_build_host(const vpx_bvh_tri* tris, uint32_t n, vpx_bvh_node* nodes, uint32_t* tri_idx,
                       uint32_t* nodes_used) {
    if ((n && (!tris || !nodes || !tri_idx)) || !nodes_used) return VPX_E_INVALID;
    *nodes_used = 0;
    if (!n) return VPX_OK;
    BvhBuilder b;
    b.tri = tris, b.node = nodes, b.idx = tri_idx;
    b.centroid.resize(n);
    for (uint32_t i = 0; i < n; ++i) {  // BuildBVH (BasicBVH.cpp:72-85)
        tri_idx[i] = i;
        const v3 v0{tris[i].v0[0], tris[i].v0[1], tris[i].v0[2]}, v1{tris[i].v1[0], tris[i].v1[1], tris[i].v1[2]},
            v2{tris[i].v2[0], tris[i].v2[1], tris[i].v2[2]};
        b.centroid[i] = mul(add(add(v0, v1), v2), 0.3333f);
    }
    std::memset(nodes, 0, sizeof(vpx_bvh_node) * (2 * (size_t)n - 1));
    nodes[0].left_first = 0, nodes[0].tri_count = n;
    b.bounds(0);
    b.split(0);
    *nodes_used = b.used;
    return VPX_OK;
}

uint32_t vpx_bvh_depth(const vpx_bvh_node* nodes, uint32_t nodes_used) {
    if (!nodes || !nodes_used) return 0;
    // iterative (a degenerate chain of VPX_BVH_MAX_TRIS triangles is 511 deep)
    std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 1u}};
    uint32_t best = 0;
    while (!st.empty()) {
        const auto [ni, d] = st.back();
        st.pop_back();
        if (ni >= nodes_used) return 0;  // not a tree built by vpx_bvh_build_host
        best = d > best ? d : best;
        if (!nodes[ni].tri_count) {
            st.push_back({nodes[ni].left_first, d + 1});
            st.push_back({nodes[ni].left_first + 1, d + 1});
        }
    }
    return best;
}

int vpx_bvh_random_tris(uint32_t* seed, vpx_bvh_tri out[64]) {
    if (!seed || !out) return VPX_E_INVALID;
    for (int i = 0; i < 64; ++i) {  // BasicBVH::BasicBVH (BasicBVH.cpp:4-16)
        float r[9];
        for (float& x : r) x = bvh_random_float(*seed);
        const v3 a = sub(mul(v3{r[0], r[1], r[2]}, 9.0f), v3{5.0f, 5.0f, 5.0f});
        put(out[i].v0, a);
        put(out[i].v1, add(a, v3{r[3], r[4], r[5]}));
        put(out[i].v2, add(a, v3{r[6], r[7], r[8]}));
    }
    return VPX_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ .vox decoder
// MagicaVoxel .vox (versions 150 / 200) decoded to what Scene::LoadModel receives from
// ogt_vox v0.997 (template/scene.cpp:474-475: ogt_vox_read_scene_with_flags(buf, n, 0)
// ->models[0] and ->palette), restated from the format and ogt's documented read rules:
//   - chunks are (id, size, child size, payload); MAIN's payload is its children;
//   - every SIZE + XYZI pair is a model (voxel_data x + y*sx + z*sx*sy, palette index,
//     0 = empty); a model whose XYZI holds no voxel is culled, so models[0] is the first
//     model with voxels (de-duplication only ever drops later copies);
//   - RGBA holds 256 RGBA colours, colour k of the file describing palette index k + 1;
//   - IMAP (display index -> file index) reorders the palette into display order,
//     palette[i] = file[(imap[i] + 255) & 255], and every voxel byte v of every model
//     (empty ones included) becomes (uint8)(1 + inverse_imap[v]);
//   - finally the palette is rotated by one so a voxel byte indexes it directly:
//     palette[i] = file[i - 1], palette[0] = file[255] with alpha 0.
namespace {
struct VoxReader {
    const uint8_t* p;
    uint64_t n, at = 0;
    bool u32(uint32_t& v) {
        if (n - at < 4) return false;
        std::memcpy(&v, p + at, 4);
        at += 4;
        return true;
    }
};
constexpr uint32_t vox_id(char a, char b, char c, char d) {
    return (uint32_t)(uint8_t)a | (uint32_t)(uint8_t)b << 8 | (uint32_t)(uint8_t)c << 16 | (uint32_t)(uint8_t)d << 24;
}
}  // namespace

extern "C" {

int vpx_vox_decode(const uint8_t* data, uint64_t len, uint32_t size_out[3], uint8_t* voxels, uint64_t voxels_cap,
                   uint8_t palette_rgba[1024]) {
    if (!data || !size_out) return VPX_E_INVALID;
    VoxReader r{data, len};
    uint32_t magic = 0, version = 0;
    if (!r.u32(magic) || !r.u32(version) || magic != vox_id('V', 'O', 'X', ' ') || (version != 150 && version != 200))
        return VPX_E_INVALID;
    uint32_t sx = 0, sy = 0, sz = 0;
    bool have_model = false, have_rgba = false, have_imap = false;
    uint32_t m0[3] = {0, 0, 0};
    std::vector<uint8_t> model;
    uint8_t rgba[1024];
    uint8_t imap[256];
    while (len - r.at >= 12) {
        uint32_t id, size, child;
        r.u32(id), r.u32(size), r.u32(child);
        if (id == vox_id('M', 'A', 'I', 'N')) continue;  // its children follow
        if (size > len - r.at) return VPX_E_INVALID;
        const uint8_t* body = data + r.at;
        if (id == vox_id('S', 'I', 'Z', 'E')) {
            if (size != 12) return VPX_E_INVALID;
            std::memcpy(&sx, body, 4), std::memcpy(&sy, body + 4, 4), std::memcpy(&sz, body + 8, 4);
            if (!sx || !sy || !sz) return VPX_E_INVALID;
        } else if (id == vox_id('X', 'Y', 'Z', 'I')) {
            if (!sx || size < 4) return VPX_E_INVALID;
            uint32_t nv;
            std::memcpy(&nv, body, 4);
            if (nv && !have_model) {  // models[0]: the first model holding voxels
                const uint64_t count = (uint64_t)sx * sy * sz;
                if (count > (1ull << 32)) return VPX_E_INVALID;
                model.assign(count, 0);
                const uint64_t avail = (size - 4) / 4;
                const uint64_t m = nv < avail ? nv : avail;
                for (uint64_t i = 0; i < m; ++i) {
                    const uint8_t* v = body + 4 + 4 * i;
                    if (v[0] >= sx || v[1] >= sy || v[2] >= sz) return VPX_E_INVALID;
                    model[v[0] + (uint64_t)v[1] * sx + (uint64_t)v[2] * sx * sy] = v[3];
                }
                m0[0] = sx, m0[1] = sy, m0[2] = sz;
                have_model = true;
            }
        } else if (id == vox_id('R', 'G', 'B', 'A')) {
            if (size != 1024) return VPX_E_INVALID;
            std::memcpy(rgba, body, 1024);
            have_rgba = true;
        } else if (id == vox_id('I', 'M', 'A', 'P')) {
            if (size != 256) return VPX_E_INVALID;
            std::memcpy(imap, body, 256);
            have_imap = true;
        }
        r.at += size;  // every other chunk (scene graph, layers, materials, cameras) is skipped
    }
    if (!have_model) return VPX_E_INVALID;
    size_out[0] = m0[0], size_out[1] = m0[1], size_out[2] = m0[2];
    const uint64_t count = (uint64_t)m0[0] * m0[1] * m0[2];
    if (!voxels && !palette_rgba) return VPX_OK;  // size query
    if (palette_rgba && !have_rgba) return VPX_E_STATE;  // MagicaVoxel's default palette is not carried
    uint8_t inv[256] = {0};
    if (have_imap) {
        bool seen[256] = {false};
        for (int i = 0; i < 256; ++i) {
            if (seen[imap[i]]) return VPX_E_INVALID;  // not a permutation
            seen[imap[i]] = true;
            inv[imap[i]] = (uint8_t)i;
        }
    }
    if (voxels) {
        if (voxels_cap < count) return VPX_E_INVALID;
        for (uint64_t i = 0; i < count; ++i) voxels[i] = have_imap ? (uint8_t)(1u + inv[model[i]]) : model[i];
    }
    if (palette_rgba) {
        uint8_t disp[1024];  // display order
        for (int i = 0; i < 256; ++i)
            std::memcpy(disp + 4 * i, rgba + 4 * (have_imap ? ((imap[i] + 255) & 255) : i), 4);
        for (int i = 1; i < 256; ++i) std::memcpy(palette_rgba + 4 * i, disp + 4 * (i - 1), 4);
        std::memcpy(palette_rgba, disp + 4 * 255, 4);
        palette_rgba[3] = 0;
    }
    return VPX_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ model loaders
// Scene::LoadModel / LoadModelPartial / LoadModelRandomMaterials (template/scene.cpp:449-683)
// on the host, through the code the device runs (vpx_model.hpp).
namespace {
const uint32_t* jump_tables() {  // T^(2^j), j < 64
    static const std::vector<uint32_t> t = [] {
        std::vector<uint32_t> v(32 * vpx::model::kJumpHost);
        vpx::model::xs32_build_tables(v.data(), vpx::model::kJumpHost);
        return v;
    }();
    return t.data();
}
}  // namespace

extern "C" {

uint32_t vpx_xorshift32_jump(uint32_t state, uint64_t steps) {
    return vpx::model::xs32_jump(jump_tables(), state, steps);
}

int vpx_model_place_host(const uint8_t* voxels, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n,
                         const vpx_model_load* in, uint8_t* cells, vpx_model_result* out) {
    namespace m = vpx::model;
    if (!voxels || !cells || m::check_load(in, sx, sy, sz, n)) return VPX_E_INVALID;
    const uint64_t count = (uint64_t)sx * sy * sz;
    std::vector<uint16_t> plan(m::plan_bytes(n) / 2);
    uint8_t* pb = reinterpret_cast<uint8_t*>(plan.data());
    vpx_model_result res{};
    m::plan_load(pb, in, sx, sy, sz, n, res.scale_model);
    res.seed = in->seed;
    std::vector<uint8_t> mat;
    if (in->mode == VPX_LOAD_RANDOM) {
        mat.resize((count + m::kChunk - 1) / m::kChunk * m::kChunk);
        for (uint64_t first = 0; first < count; first += m::kChunk)
            m::random_chunk(jump_tables(), in->seed, first, in->rand_lo, in->rand_hi, mat.data());
        res.seed = vpx_xorshift32_jump(in->seed, count);
    }
    m::place_grid(m::plan_view(pb, n), voxels, mat.empty() ? voxels : mat.data(), sx, sy, cells);
    if (out) *out = res;
    return VPX_OK;
}

int vpx_model_palette_materials(vpx_material* mats, const uint8_t* voxels, uint64_t count,
                                const uint8_t palette_rgba[1024]) {
    if (!mats || !voxels || !palette_rgba) return VPX_E_INVALID;
    bool used[256] = {false};
    for (uint64_t i = 0; i < count; ++i) used[voxels[i]] = true;
    for (int i = 1; i < 256; ++i) {
        if (!used[i]) continue;
        for (int k = 0; k < 3; ++k) mats[i].albedo[k] = (float)palette_rgba[4 * i + k] / 255.0f;
        mats[i].roughness = 1.0f;
    }
    return VPX_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ noise generators
// Scene::GenerateSomeNoise / GenerateSomeSmoke (template/scene.cpp:226-356) on the host, through
// the code the device runs (vpx_noise.hpp).
extern "C" {

int vpx_noise_generate_host(uint32_t n, const vpx_noise_gen* in, uint8_t* cells, vpx_noise_result* out) {
    if (!cells || vpx::noise::check_gen(in, n)) return VPX_E_INVALID;
    vpx::noise::generate_host(jump_tables(), n, in, cells, out);
    return VPX_OK;
}

float vpx_perlin3(int32_t seed, float x, float y, float z) { return vpx::noise::perlin3(seed, x, y, z); }

}  // extern "C"

// ------------------------------------------------------------------ brush edits
// vpx_grid_brush's cells on the host, through the tests the device runs (vpx_brush.hpp); the
// flipped bricks from the host level builder's l2 before and after.
extern "C" {

int vpx_brush_apply_host(uint8_t* cells, uint32_t n, const vpx_brush* brushes, uint32_t count, vpx_brush_result* out) {
    if (!cells || n == 0 || n > 4096 || vpx::brush::check_brushes(brushes, count)) return VPX_E_INVALID;
#if !defined(__HIP_DEVICE_COMPILE__)  // the host builders exist in the host pass only
    const uint32_t nb1 = (n + 3) / 4, nb2 = (nb1 + 3) / 4, nb3 = (nb2 + 3) / 4;
    std::vector<uint64_t> l1(64ull * nb2 * nb2 * nb2), before(64ull * nb3 * nb3 * nb3), after(before.size());
    if (out) vpx::skip::build_masks_host(cells, n, l1.data(), before.data());
    vpx_brush_result res{};
    for (uint32_t i = 0; i < count; ++i) res.changed += vpx::brush::apply_host(cells, n, brushes[i]);
    if (out) {
        vpx::skip::build_masks_host(cells, n, l1.data(), after.data());
        for (size_t i = 0; i < after.size(); ++i) res.flipped += (uint32_t)__builtin_popcountll(before[i] ^ after[i]);
        *out = res;
    }
#endif
    return VPX_OK;
}

// vpx_grid_stamp's cells on the host, through the plan and the per-cell rule the device runs
// (vpx_stamp.hpp); `flipped` as above.
int vpx_stamp_apply_host(uint8_t* cells, uint32_t n, const vpx_stamp_source* models, uint32_t n_models, const vpx_stamp* stamps,
                         uint32_t count, vpx_brush_result* out) {
    if (!cells || !models || n == 0 || n > 4096 || vpx::stamp::check_stamps(stamps, count)) return VPX_E_INVALID;
    for (uint32_t i = 0; i < count; ++i) {
        if (stamps[i].model_id >= n_models) return VPX_E_INVALID;
        const vpx_stamp_source& m = models[stamps[i].model_id];
        if (!m.voxels || m.reserved != 0 || !m.sx || !m.sy || !m.sz || m.sx > vpx::stamp::kMaxDim || m.sy > vpx::stamp::kMaxDim ||
            m.sz > vpx::stamp::kMaxDim)
            return VPX_E_INVALID;
    }
#if !defined(__HIP_DEVICE_COMPILE__)  // the host builders exist in the host pass only
    const uint32_t nb1 = (n + 3) / 4, nb2 = (nb1 + 3) / 4, nb3 = (nb2 + 3) / 4;
    std::vector<uint64_t> l1(64ull * nb2 * nb2 * nb2), before(64ull * nb3 * nb3 * nb3), after(before.size());
    if (out) vpx::skip::build_masks_host(cells, n, l1.data(), before.data());
    vpx_brush_result res{};
    for (uint32_t i = 0; i < count; ++i) {
        const vpx_stamp_source& m = models[stamps[i].model_id];
        vpx::stamp::Plan p;
        if (vpx::stamp::plan(stamps[i], m.sx, m.sy, m.sz, n, p)) res.changed += vpx::stamp::apply_host(cells, n, p, m.voxels);
    }
    if (out) {
        vpx::skip::build_masks_host(cells, n, l1.data(), after.data());
        for (size_t i = 0; i < after.size(); ++i) res.flipped += (uint32_t)__builtin_popcountll(before[i] ^ after[i]);
        *out = res;
    }
#endif
    return VPX_OK;
}

// vpx_denoise_ids on host memory: vpx_denoise.hpp's host loops, the code the kernels share.
int vpx_denoise_host(uint32_t width, uint32_t height, const uint32_t* ids, const float* in, float* out, uint32_t* rgb8,
                     const vpx_denoise* d) {
    if (vpx::denoise::check_call(width, height, ids, in, out, d)) return VPX_E_INVALID;
    const size_t pixels = (size_t)width * height;
    try {
        std::vector<vpx::denoise::Key> keys(pixels);
        std::vector<float> scratch(d->passes > 1 ? 8 * pixels : 0);
        vpx::denoise::run_host(width, height, ids, in, out, rgb8, *d, keys.data(), scratch.data(),
                               scratch.data() + (d->passes > 1 ? 4 * pixels : 0));
    } catch (const std::bad_alloc&) {
        return VPX_E_NOMEM;
    }
    return VPX_OK;
}

static_assert(sizeof(vpx_denoise) == 16 && sizeof(vpx::denoise::Key) == 8, "denoise layout");

// vpx_reproject_ids on host memory: vpx_reproject.hpp's host loop over the pixel function the kernel shares.
int vpx_reproject_ids_host(uint32_t width, uint32_t height, const uint32_t* ids_cur, const uint32_t* ids_prev,
                           const float* cur, const float* hist_in, float* hist_out, uint32_t* rgb8, const vpx_reproject* r,
                           const vpx_volume* cur_volumes, const vpx_volume* prev_volumes) {
    if (vpx::reproject::check_call(width, height, ids_cur, ids_prev, cur, hist_in, hist_out, r, cur_volumes, prev_volumes))
        return VPX_E_INVALID;
    try {
        std::vector<float> tab((size_t)r->n_volumes * vpx::reproject::kTabFloats);
        std::vector<uint32_t> moved(r->n_volumes);
        vpx::reproject::build_table(r->n_volumes, cur_volumes, prev_volumes, tab.data(), moved.data());
        vpx::reproject::run_host(width, height, ids_cur, ids_prev, cur, hist_in, hist_out, rgb8, *r, tab.data(), moved.data());
    } catch (const std::bad_alloc&) {
        return VPX_E_NOMEM;
    }
    return VPX_OK;
}

static_assert(sizeof(vpx_reproject) == 168, "reproject layout");

// vpx_reproject_moments on host memory: the same loop with reproject::pixel's moments payload.
int vpx_reproject_moments_host(uint32_t width, uint32_t height, const uint32_t* ids_cur, const uint32_t* ids_prev,
                               const float* cur, const float* hist_in, const float* mom_in, float* hist_out,
                               float* mom_out, uint32_t* rgb8, const vpx_reproject* r, const vpx_volume* cur_volumes,
                               const vpx_volume* prev_volumes) {
    if (vpx::reproject::check_call_moments(width, height, ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out, r,
                                           cur_volumes, prev_volumes))
        return VPX_E_INVALID;
    try {
        std::vector<float> tab((size_t)r->n_volumes * vpx::reproject::kTabFloats);
        std::vector<uint32_t> moved(r->n_volumes);
        vpx::reproject::build_table(r->n_volumes, cur_volumes, prev_volumes, tab.data(), moved.data());
        vpx::reproject::run_host_moments(width, height, ids_cur, ids_prev, cur, hist_in, mom_in, hist_out, mom_out, rgb8, *r,
                                         tab.data(), moved.data());
    } catch (const std::bad_alloc&) {
        return VPX_E_NOMEM;
    }
    return VPX_OK;
}

// vpx_denoise_var on host memory: vpx_denoise_var.hpp's host loops, the code the kernels share.
int vpx_denoise_var_host(uint32_t width, uint32_t height, const uint32_t* ids, const float* in, const float* mom,
                         float* out, uint32_t* rgb8, const vpx_denoise_var_params* d) {
    if (vpx::denoise_var::check_call(width, height, ids, in, mom, out, d)) return VPX_E_INVALID;
    const size_t pixels = (size_t)width * height;
    try {
        std::vector<vpx::denoise::Key> keys(pixels);
        std::vector<float> scratch((d->passes > 1 ? 8 : 4) * pixels);
        vpx::denoise_var::run_host(width, height, ids, in, mom, out, rgb8, *d, keys.data(), scratch.data(),
                                   scratch.data() + (d->passes > 1 ? 4 * pixels : 0));
    } catch (const std::bad_alloc&) {
        return VPX_E_NOMEM;
    }
    return VPX_OK;
}

static_assert(sizeof(vpx_denoise_var_params) == 32, "denoise_var layout");

}  // extern "C"
