// model_place_test.cpp — csrc/vpx_model.hpp (the model loaders' placement, shared by the host
// entry and the device kernel) against the reference's loop restated naively
// (template/scene.cpp:449-683): ResetGrid() to NONE, then z outer, y, x inner, every non-empty
// voxel written to (trunc(x * s.x), trunc(z * s.y), trunc(y * s.z)), later writes replacing
// earlier ones, writes outside the grid dropped.  Also the xorshift32 jump against looped steps
// and the chunked random materials against the sequential draw.  Prints bad=0.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I csrc model_place_test.cpp   (also with
//   -fsanitize=address,undefined: every table index and every voxel read is in bounds)
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "vpx_model.hpp"

namespace m = vpx::model;

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

static int trunc_x86(float f) {
    if (!(f > -2147483904.0f && f < 2147483648.0f)) return INT_MIN;
    return (int)f;
}

// the loop of the three loaders; mat == nullptr: the voxel's own byte
static void naive(const std::vector<uint8_t>& vox, const uint8_t* mat, uint32_t sx, uint32_t sy, uint32_t sz, uint32_t n,
                  const float scl[3], uint32_t lo, uint32_t hi, std::vector<uint8_t>& out) {
    out.assign((size_t)n * n * n, 255);
    for (uint32_t z = 0; z < sz; ++z)
        for (uint32_t y = 0; y < sy; ++y)
            for (uint32_t x = 0; x < sx; ++x) {
                const int gx = trunc_x86((float)x * scl[0]);
                const int gy = trunc_x86((float)z * scl[1]);
                const int gz = trunc_x86((float)y * scl[2]);
                const size_t i = x + (size_t)y * sx + (size_t)z * sx * sy;
                if (vox[i] == 0 || !(x >= lo && x <= hi)) continue;
                if (gx < 0 || gy < 0 || gz < 0 || (uint32_t)gx >= n || (uint32_t)gy >= n || (uint32_t)gz >= n) continue;
                out[(size_t)gx + (size_t)gy * n + (size_t)gz * n * n] = mat ? mat[i] : vox[i];
            }
}

int main() {
    unsigned long long bad = 0, cases = 0, collisions = 0;
    uint32_t rng = 12345u;

    // ---- jump against looped steps
    std::vector<uint32_t> t(32 * m::kJumpHost);
    m::xs32_build_tables(t.data(), m::kJumpHost);
    const uint64_t ks[] = {0, 1, 2, 31, 32, 33, 147, 558, 1ull << 18, (1ull << 24) - 1};
    const uint32_t seeds[] = {0u, 1u, 0x12345678u, 0xffffffffu, 0x80000000u, 2463534242u};
    for (uint32_t s : seeds) {
        uint64_t done = 0;
        uint32_t cur = s;
        for (uint64_t k : ks) {
            for (; done < k; ++done) cur = m::xs32_step(cur);
            bad += m::xs32_jump(t.data(), s, k) != cur;
            ++cases;
        }
        bad += m::xs32_jump(t.data(), s, 0xffffffffull) != s;  // the period (the zero state is a fixed point)
        bad += m::xs32_jump(t.data(), s, (1ull << 40) + 5) != m::xs32_jump(t.data(), m::xs32_jump(t.data(), s, 1ull << 40), 5);
    }
    std::printf("jump: cases=%llu bad=%llu\n", cases, bad);

    // ---- placement
    const uint32_t dims[][3] = {{7, 5, 9}, {33, 17, 20}, {40, 30, 21}, {256, 3, 2}, {1, 1, 1}, {2, 256, 3}, {16, 16, 16}};
    const uint32_t grids[] = {1, 5, 16, 20, 32};
    const float nan = std::nanf("");
    const float scales[][3] = {{1, 1, 1},          {0.5f, 0.5f, 0.5f},   {1.0f / 3.0f, 1.0f / 3.0f, 1.0f / 3.0f},
                               {0.999f, 0.999f, 0.999f}, {-0.5f, 1, 1},  {1, -1, 0.5f},
                               {nan, 1, 1},        {1, 1, nan},          {2.5f, 0.75f, 1.5f},
                               {0, 0, 0},          {3e9f, 1, 1},         {1, 0.25f, 1.0f / 3.0f}};
    const uint32_t cols[][2] = {{0, 0xffffffffu}, {30 - 6, 30 + 6}, {3u - 13u, 3 + 13}, {0, 0}, {5, 4}};
    for (const auto& d : dims)
        for (uint32_t n : grids)
            for (const auto& sc : scales)
                for (const auto& cl : cols)
                    for (int downscale = 0; downscale < 2; ++downscale) {
                        const uint32_t sx = d[0], sy = d[1], sz = d[2];
                        const size_t count = (size_t)sx * sy * sz;
                        std::vector<uint8_t> vox(count), mat((count + m::kChunk - 1) / m::kChunk * m::kChunk);
                        for (auto& v : vox) v = (lcg(rng) >> 24) % 5 < 2 ? (uint8_t)(1 + (lcg(rng) >> 24) % 254) : 0;
                        float scl[3] = {sc[0], sc[1], sc[2]};
                        if (downscale) m::scale_rule(sc, sx, sy, sz, n, scl);
                        const bool random = (cases & 3) == 0;
                        const uint32_t seed = lcg(rng);
                        if (random) {
                            for (size_t f = 0; f < count; f += m::kChunk) m::random_chunk(t.data(), seed, f, 9.0f, 15.0f, mat.data());
                            uint32_t s = seed;  // against the sequential draw
                            for (size_t i = 0; i < count; ++i) {
                                s = m::xs32_step(s);
                                const float r = (float)s * 2.3283064365387e-10f;
                                const float p = r * (15.0f - 9.0f);
                                bad += mat[i] != (uint8_t)(9.0f + p);
                            }
                        }
                        std::vector<uint16_t> plan(m::plan_bytes(n) / 2);
                        uint8_t* pb = reinterpret_cast<uint8_t*>(plan.data());
                        m::build_plan(pb, sx, sy, sz, n, scl, cl[0], cl[1]);
                        std::vector<uint8_t> got((size_t)n * n * n, 7), want;
                        m::place_grid(m::plan_view(pb, n), vox.data(), random ? mat.data() : vox.data(), sx, sy, got.data());
                        naive(vox, random ? mat.data() : nullptr, sx, sy, sz, n, scl, cl[0], cl[1], want);
                        if (got != want) {
                            if (bad < 5)
                                std::printf("MISMATCH dims %u %u %u n %u scale %g %g %g cols %u %u\n", sx, sy, sz, n, scl[0],
                                            scl[1], scl[2], cl[0], cl[1]);
                            ++bad;
                        }
                        if (n % 16 == 0) {  // the 16-cell span the wide device path takes
                            uint8_t vals[16];
                            for (uint32_t gz = 0; gz < n; gz += 3)
                                for (uint32_t gy = 0; gy < n; gy += 5)
                                    for (uint32_t gx = 0; gx < n; gx += 16) {
                                        m::place_span<16>(m::plan_view(pb, n), vox.data(), random ? mat.data() : vox.data(), sx,
                                                          sy, gx, gy, gz, vals);
                                        bad += std::memcmp(vals, &want[gx + (size_t)gy * n + (size_t)gz * n * n], 16) != 0;
                                    }
                        }
                        // a first-writer-wins grid differs wherever order matters
                        size_t nonempty = 0;
                        for (uint8_t v : want) nonempty += v != 255;
                        size_t sources = 0;
                        for (size_t i = 0; i < count; ++i) sources += vox[i] != 0;
                        collisions += sources > nonempty;
                        ++cases;
                    }
    std::printf("placement: cases=%llu with_collisions=%llu\n", cases, collisions);
    if (collisions < 100) ++bad;  // the cases must exercise the last-writer rule
    std::printf("bad=%llu\n", bad);
    return bad != 0;
}
