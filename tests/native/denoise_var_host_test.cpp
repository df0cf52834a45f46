// denoise_var_host_test.cpp — the host paths of csrc/vpx_denoise_var.hpp and of vpx_reproject.hpp's
// moments payload in a stand-alone program, meant to be built with -fsanitize=address,undefined:
// every buffer is a heap block of exactly the size the call is entitled to, so a tap, a prefilter
// tap or a moment read outside the image is a report.
// Denoise: stripes of width 3, and one plane mixed with the four kinds of invalid record; 1x1, 5x3
// (every tap of steps 4..16 outside) and 67x35; passes 1..5; moments NULL and given (history
// lengths on both sides of min_history, NaN among them).  Checked here: invalid keys and .w pass
// through bit for bit, a constant colour comes back exactly, rgb8 is the tonemap of out.
// Reprojection: a plane facing the camera striped into two keys with a band of invalid records;
// the previous camera beside, behind or where the current one stands; static and moving volumes;
// with and without a previous frame.  Checked here: hist_out is run_host's bit for bit, and a
// pixel without history has the moments of its own sample.
// (The bits are tests/test_denoise_var.py's business.)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vpx_denoise_var.hpp"
#include "vpx_reproject.hpp"

using namespace vpx;

static uint32_t rng_state = 0x13572468u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
    return rng_state;
}

static std::vector<uint32_t> denoise_ids(uint32_t W, uint32_t H, int pattern) {
    std::vector<uint32_t> ids((size_t)W * H * 4);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            uint32_t* r = &ids[4 * ((size_t)y * W + x)];
            r[0] = rnd(), r[2] = rnd(), r[3] = rnd();  // t and the cell: any bits
            if (pattern == 0) {
                r[1] = 2u | 3u << 16 | 3u << 24;  // face 3: axis 1
                r[2] = (r[2] & 0xffffu) | (7u + (x / 3u) % 2u) << 16;
            } else {
                const uint32_t kind = y * 5 < H * 3 ? 0u : 1u + x * 4 / W;
                const uint32_t v = kind == 1 ? 0u : kind == 2 ? 1u : 2u;
                const uint32_t face = kind == 0 ? 6u : kind == 1 ? 0u : kind == 2 ? 2u : kind == 3 ? 0u : 7u + (rnd() & 0xf8u);
                r[1] = v | (rnd() & 0xffu) << 16 | face << 24;
                if (kind == 0) r[1] = 2u | 5u << 16 | 6u << 24, r[3] = 4095u;  // face 6: axis 2
            }
        }
    return ids;
}

static void denoise_part(long& calls, long& bad) {
    const uint32_t sizes[3][2] = {{1, 1}, {5, 3}, {67, 35}};
    for (const auto& sz : sizes)
        for (int pattern = 0; pattern < 2; ++pattern)
            for (uint32_t passes = 1; passes <= denoise::kMaxPasses; ++passes)
                for (int given = 0; given < 2; ++given)
                    for (int constant = 0; constant < 2; ++constant) {
                        const uint32_t W = sz[0], H = sz[1];
                        const size_t n = (size_t)W * H;
                        const std::vector<uint32_t> ids = denoise_ids(W, H, pattern);
                        std::vector<float> in(4 * n), mom(2 * n), out(4 * n, -1.f), a(4 * n), b(passes > 1 ? 4 * n : 0);
                        std::vector<uint32_t> rgb(n);
                        std::vector<denoise::Key> keys(n);
                        for (size_t p = 0; p < n; ++p) {
                            for (int k = 0; k < 3; ++k) in[4 * p + k] = constant ? 0.75f : 0.015625f * (float)(1u + rnd() % 4096u);
                            const uint32_t pick = rnd() % 8u;
                            in[4 * p + 3] = pick == 0 ? NAN : pick == 1 ? -3.f : (float)pick;
                            const float l = denoise::lum(in[4 * p], in[4 * p + 1], in[4 * p + 2]);
                            mom[2 * p] = l, mom[2 * p + 1] = l * l + (constant ? 0.f : 0.25f * (float)(rnd() % 16u));
                        }
                        const vpx_denoise_var_params d{passes, 4.0f, 0.0009765625f, 4.0f, 0u, {0u, 0u, 0u}};
                        const float* m = given ? mom.data() : nullptr;
                        if (denoise_var::check_call(W, H, ids.data(), in.data(), m, out.data(), &d)) ++bad;
                        denoise_var::run_host(W, H, ids.data(), in.data(), m, out.data(), rgb.data(), d, keys.data(), a.data(),
                                              b.data());
                        ++calls;
                        for (size_t p = 0; p < n; ++p) {
                            const bool ok = denoise::valid(keys[p]);
                            if (std::memcmp(&out[4 * p + 3], &in[4 * p + 3], 4)) ++bad;
                            if (!ok && std::memcmp(&out[4 * p], &in[4 * p], 16)) ++bad;
                            if (ok && constant && std::memcmp(&out[4 * p], &in[4 * p], 12)) ++bad;
                            if (rgb[p] != denoise::tonemap_pack_host(&out[4 * p])) ++bad;
                        }
                    }
}

// A camera at `pos` looking down +z: the image plane two units ahead, 2 * aspect wide and 2 high.
static vpx_camera camera_at(float x, float y, float z, float aspect) {
    vpx_camera c{};
    const float p[3] = {x, y, z};
    for (int k = 0; k < 3; ++k) c.cam_pos[k] = c.top_left[k] = c.top_right[k] = c.bottom_left[k] = p[k];
    c.top_left[0] -= aspect, c.top_left[1] += 1.f, c.top_left[2] += 2.f;
    c.top_right[0] += aspect, c.top_right[1] += 1.f, c.top_right[2] += 2.f;
    c.bottom_left[0] -= aspect, c.bottom_left[1] -= 1.f, c.bottom_left[2] += 2.f;
    return c;
}
// Its frustum normals, pointing into the pyramid; sign: -1 looks down -z.
static vpx_prev_camera prev_at(float x, float y, float z, float aspect, float sign) {
    vpx_prev_camera p{};
    p.cam_pos[0] = x, p.cam_pos[1] = y, p.cam_pos[2] = z;
    p.left_normal[0] = 2.f, p.left_normal[2] = aspect * sign;
    p.right_normal[0] = -2.f, p.right_normal[2] = aspect * sign;
    p.top_normal[1] = -2.f, p.top_normal[2] = sign;
    p.bottom_normal[1] = 2.f, p.bottom_normal[2] = sign;
    return p;
}

static std::vector<uint32_t> reproject_ids(uint32_t W, uint32_t H, const vpx_camera& c, uint32_t n_volumes) {
    std::vector<uint32_t> ids((size_t)W * H * 4);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            uint32_t* r = &ids[4 * ((size_t)y * W + x)];
            const float u = (float)x / (float)W, v = (float)y / (float)H;  // the ray's length to the plane z = 4
            const float dx = (c.top_left[0] + (c.top_right[0] - c.top_left[0]) * u) - c.cam_pos[0];
            const float dy = (c.top_left[1] + (c.bottom_left[1] - c.top_left[1]) * v) - c.cam_pos[1];
            const float t = (4.f - c.cam_pos[2]) * std::sqrt(dx * dx + dy * dy + 4.f) / 2.f;
            memcpy(&r[0], &t, 4);
            r[2] = rnd(), r[3] = (x / 3u) % 2u;  // face 5: axis 2, the coordinate in .w
            const uint32_t kind = y * 5 < H * 4 ? 0u : 1u + x * 4 / W;
            const uint32_t vol = 2u + (n_volumes ? rnd() % (n_volumes + 1u) : 0u);  // one past the table too
            const uint32_t v16 = kind == 1 ? 0u : kind == 2 ? 1u : vol;
            const uint32_t face = kind == 0 ? 5u : kind == 1 ? 0u : kind == 2 ? 2u : kind == 3 ? 0u : 7u;
            r[1] = v16 | (kind == 0 ? 3u + (rnd() & 3u) : rnd() & 0xffu) << 16 | face << 24;
            if (kind != 0) r[0] = rnd();  // any t at all, NaN and infinity included
        }
    return ids;
}

static void reproject_part(long& calls, long& bad, long& took) {
    using namespace reproject;
    const uint32_t sizes[3][2] = {{1, 1}, {5, 3}, {67, 35}};
    const float prevs[4][4] = {{0.f, 0.f, 0.f, 1.f}, {0.15f, -0.1f, 0.2f, 1.f}, {0.f, 0.f, -0.5f, 1.f}, {0.f, 0.f, 8.f, -1.f}};
    for (const auto& sz : sizes)
        for (const auto& pv : prevs)
            for (uint32_t n_volumes = 0; n_volumes <= 3; n_volumes += 3)
                for (int with_prev = 0; with_prev < 2; ++with_prev) {
                    const uint32_t W = sz[0], H = sz[1];
                    const size_t n = (size_t)W * H;
                    const float aspect = (float)W / (float)H;
                    vpx_reproject r{};
                    r.cur = camera_at(0.f, 0.f, 0.f, aspect);
                    r.prev = prev_at(pv[0], pv[1], pv[2], aspect, pv[3]);
                    r.max_history = 8.f;
                    r.nohist_lo = 6u, r.nohist_hi = 6u;
                    r.n_volumes = n_volumes;
                    std::vector<vpx_volume> cv(n_volumes), pvol(n_volumes);
                    for (uint32_t v = 0; v < n_volumes; ++v) {
                        for (int k = 0; k < 4; ++k)
                            cv[v].matrix[5 * k] = cv[v].inv_matrix[5 * k] = pvol[v].matrix[5 * k] = pvol[v].inv_matrix[5 * k] = 1.f;
                        if (v == 1) pvol[v].matrix[3] = 0.05f, pvol[v].inv_matrix[3] = -0.05f;  // moved along x
                    }
                    const std::vector<uint32_t> ids_cur = reproject_ids(W, H, r.cur, n_volumes);
                    const std::vector<uint32_t> ids_prev = reproject_ids(W, H, camera_at(pv[0], pv[1], pv[2], aspect), n_volumes);
                    std::vector<float> cur(4 * n), hist(4 * n), mom(2 * n), out(4 * n, -1.f), plain(4 * n, -2.f), mo(2 * n, -1.f);
                    std::vector<uint32_t> rgb(n);
                    for (size_t p = 0; p < n; ++p) {
                        for (int k = 0; k < 3; ++k) {
                            cur[4 * p + k] = 0.015625f * (float)(1u + rnd() % 4096u);
                            hist[4 * p + k] = 0.015625f * (float)(1u + rnd() % 4096u);
                        }
                        const uint32_t wbits = rnd();
                        memcpy(&cur[4 * p + 3], &wbits, 4);
                        hist[4 * p + 3] = (rnd() & 7u) == 0u ? 0.5f : (float)(1u + rnd() % 20u);
                        mom[2 * p] = 0.015625f * (float)(1u + rnd() % 4096u), mom[2 * p + 1] = 0.015625f * (float)(1u + rnd() % 4096u);
                    }
                    const uint32_t* ip = with_prev ? ids_prev.data() : nullptr;
                    const float* hi = with_prev ? hist.data() : nullptr;
                    const float* mi = with_prev ? mom.data() : nullptr;
                    if (check_call_moments(W, H, ids_cur.data(), ip, cur.data(), hi, mi, out.data(), mo.data(), &r, cv.data(),
                                           pvol.data()))
                        ++bad;
                    std::vector<float> tab((size_t)n_volumes * kTabFloats);
                    std::vector<uint32_t> moved(n_volumes);
                    build_table(n_volumes, cv.data(), pvol.data(), tab.data(), moved.data());
                    run_host_moments(W, H, ids_cur.data(), ip, cur.data(), hi, mi, out.data(), mo.data(),
                                     (calls & 1) ? rgb.data() : nullptr, r, tab.data(), moved.data());
                    run_host(W, H, ids_cur.data(), ip, cur.data(), hi, plain.data(), nullptr, r, tab.data(), moved.data());
                    if (memcmp(out.data(), plain.data(), 16 * n)) ++bad;
                    for (size_t p = 0; p < n; ++p) {
                        const float len = out[4 * p + 3];
                        if (len > 1.f) ++took;
                        if (len == 1.f) {
                            const float l = denoise::lum(cur[4 * p], cur[4 * p + 1], cur[4 * p + 2]);
                            if (mo[2 * p] != l || mo[2 * p + 1] != l * l) ++bad;
                        }
                        if (!(mo[2 * p] > 0.f && mo[2 * p] <= 65.f && mo[2 * p + 1] > 0.f && mo[2 * p + 1] <= 4100.f)) ++bad;
                        if ((calls & 1) && rgb[p] != denoise::tonemap_pack_host(&out[4 * p])) ++bad;
                    }
                    ++calls;
                }
}

int main() {
    long dcalls = 0, rcalls = 0, bad = 0, took = 0;
    denoise_part(dcalls, bad);
    reproject_part(rcalls, bad, took);
    std::printf("denoise_var host: calls=%ld reproject_moments host: calls=%ld took_history=%s bad=%ld\n", dcalls, rcalls,
                took > 1000 ? "yes" : "no", bad);
    return bad || took <= 1000 ? 1 : 0;
}
