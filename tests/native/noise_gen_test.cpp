// noise_gen_test.cpp — csrc/vpx_noise.hpp (Scene::GenerateSomeNoise / GenerateSomeSmoke, shared
// by the host entry and the device kernels) against the two loops restated naively
// (template/scene.cpp:226-356): z outer, y, x inner, one cell at a time through perlin3, the
// xorshift32 state stepped once per draw.  Checked on random (n, frequency, seed):
//   - the span path (16 cells of a row, the row's terms shared) equals the cell path, bit for bit;
//   - the block-wise path (counts, exclusive prefix, jump) equals sequential stepping: cells,
//     the state left behind, the noise seed and the number of draws;
//   - the classifier's known answers at every threshold, and the draw at its ends.
// Prints bad=0.
//
//   g++ -O2 -std=c++17 -ffp-contract=off -I include -I csrc noise_gen_test.cpp   (also with
//   -fsanitize=address,undefined: every cell index and every table read is in bounds)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "vpx.h"
#include "vpx_noise.hpp"

namespace nz = vpx::noise;
namespace m = vpx::model;

static uint32_t lcg(uint32_t& s) {  // the low bits of an LCG cycle quickly: fold the high ones in
    s = s * 1664525u + 1013904223u;
    return s ^ (s >> 15);
}

static uint32_t bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// the two loops as the reference writes them, with the sequential RNG
static void naive(uint32_t n, uint32_t mode, float f, uint32_t seed, std::vector<uint8_t>& out, vpx_noise_result& res) {
    out.assign((size_t)n * n * n, 77);
    uint32_t s = m::xs32_step(seed);
    const int32_t nseed = (int32_t)s;
    uint64_t draws = 1;
    for (uint32_t z = 0; z < n; ++z)
        for (uint32_t y = 0; y < n; ++y)
            for (uint32_t x = 0; x < n; ++x) {
                const float nv = nz::perlin3(nseed, (float)x * f, (float)y * f, (float)z * f);
                uint8_t v;
                if (mode == VPX_GEN_NOISE) {
                    v = nz::noise_class(nv);
                    if (v == nz::kDrawMark) {
                        s = m::xs32_step(s);
                        ++draws;
                        v = nz::noise_draw(s);
                    }
                } else {
                    const uint32_t ux = m::xs32_step(s);
                    s = m::xs32_step(ux);
                    draws += 2;
                    v = nz::smoke_cell(nv, x, y, z, n, ux, s);
                }
                out[x + (size_t)y * n + (size_t)z * n * n] = v;
            }
    res.seed = s;
    res.noise_seed = (uint32_t)nseed;
    res.draws = draws;
}

int main() {
    std::vector<uint32_t> t(32 * m::kJumpHost);
    m::xs32_build_tables(t.data(), m::kJumpHost);
    long bad = 0, cases = 0, drawers = 0, multi_block = 0, smoke_cells = 0;

    // ---- classifier known answers (scene.cpp:250-275): float against double literals
    {
        const float nan = std::numeric_limits<float>::quiet_NaN();
        struct {
            float n;
            uint8_t want;
        } ka[] = {{0.04f, nz::kNone},        {std::nextafterf(0.04f, 1.0f), nz::kDrawMark},
                  {0.08f, nz::kDrawMark},    {std::nextafterf(0.08f, 1.0f), nz::kNonMetalRed},
                  {0.17f, nz::kNonMetalRed}, {0.2f, nz::kEmissive},
                  {std::nextafterf(0.2f, 0.0f), nz::kNonMetalRed},
                  {0.3f, nz::kMetalHigh},    {std::nextafterf(0.3f, 0.0f), nz::kEmissive},
                  {0.5f, nz::kMetalMid},     {std::nextafterf(0.5f, 0.0f), nz::kMetalHigh},
                  {0.7f, nz::kMetalLow},     {std::nextafterf(0.7f, 0.0f), nz::kMetalMid},
                  {0.9f, nz::kNone},         {std::nextafterf(0.9f, 0.0f), nz::kMetalLow},
                  {nan, nz::kNone},          {-1.0f, nz::kNone},
                  {0.0f, nz::kNone},         {2.0f, nz::kNone}};
        for (const auto& k : ka)
            if (nz::noise_class(k.n) != k.want) {
                printf("noise_class(%.9g) = %u, want %u\n", k.n, nz::noise_class(k.n), k.want);
                ++bad;
            }
        if (nz::noise_draw(0u) != 0 || nz::noise_draw(0x7FFFFFFFu) != 4 || nz::noise_draw(0xFFFFFFFFu) != 8 ||
            nz::noise_draw(0xFFFFFF7Fu) != 7) {
            printf("noise_draw ends\n");
            ++bad;
        }
        // lattice points are exact zeros, also negative ones
        for (int i = -3; i <= 3; ++i)
            if (bits(nz::perlin3(1234, (float)i, (float)(2 * i), (float)-i)) != 0) ++bad;
    }

    // ---- span path == cell path, on random rows (n % 16 == 0) and random seeds / frequencies
    uint32_t rs = 99;
    for (int it = 0; it < 3000; ++it) {
        const uint32_t n = 16 * (1 + lcg(rs) % 8);
        const float f = (float)(lcg(rs) % 100000) * 1e-5f * ((lcg(rs) & 1) ? -1.0f : 1.0f) * ((lcg(rs) & 3) ? 1.0f : 40.0f);
        const int32_t nseed = (int32_t)lcg(rs);
        const uint64_t first = (uint64_t)(lcg(rs) % (n * n * n / 16)) * 16;
        float a[nz::kSpan], b[nz::kSpan];
        nz::field_span<true>(nseed, n, f, first, nz::kSpan, a);
        nz::field_span<false>(nseed, n, f, first, nz::kSpan, b);
        for (uint32_t c = 0; c < nz::kSpan; ++c) {
            const nz::Cell p = nz::cell_of(first + c, n);
            const float d = nz::perlin3(nseed, (float)p.x * f, (float)p.y * f, (float)p.z * f);
            if (bits(a[c]) != bits(b[c]) || bits(a[c]) != bits(d)) ++bad;
        }
    }

    // ---- block-wise path == sequential stepping, whole grids
    std::vector<uint8_t> want, got;
    for (int it = 0; it < 2400; ++it) {
        const uint32_t pick = lcg(rs) % 8;
        // small grids mostly; every so often one with several blocks (n^3 > 4096), rows or not
        const uint32_t n = pick == 0 ? 32 : pick == 1 ? 21 + lcg(rs) % 6 : pick == 2 ? 16 : 1 + lcg(rs) % 15;
        vpx_noise_gen in{};
        in.mode = lcg(rs) & 1;
        in.frequency = (float)(1 + lcg(rs) % 4000) * 1e-4f * ((lcg(rs) % 8) ? 1.0f : -1.0f);
        in.seed = (lcg(rs) % 16) ? lcg(rs) : 0u;
        if (nz::check_gen(&in, n)) {
            ++bad;
            continue;
        }
        vpx_noise_result a{}, b{};
        naive(n, in.mode, in.frequency, in.seed, want, a);
        got.assign(want.size(), 78);
        nz::generate_host(t.data(), n, &in, got.data(), &b);
        if (want != got || a.seed != b.seed || a.noise_seed != b.noise_seed || a.draws != b.draws) {
            printf("grid differs: n=%u mode=%u f=%.9g seed=%08x\n", n, in.mode, in.frequency, in.seed);
            ++bad;
        }
        for (uint8_t v : got)
            if (v == nz::kDrawMark) ++bad;  // no marker survives
        ++cases;
        if (in.mode == VPX_GEN_NOISE) {
            drawers += (long)(a.draws - 1);
            if (a.draws > 1 && (uint64_t)n * n * n > nz::kBlockCells) ++multi_block;
        } else {
            for (uint8_t v : got) smoke_cells += v != nz::kNone;
        }
    }
    // the random cases must have exercised what they are for
    if (drawers < 1000 || multi_block < 20 || smoke_cells < 1000) {
        printf("thin coverage: drawers=%ld multi_block=%ld smoke_cells=%ld\n", drawers, multi_block, smoke_cells);
        ++bad;
    }
    printf("cases=%ld drawers=%ld multi_block=%ld smoke_cells=%ld bad=%ld\n", cases, drawers, multi_block, smoke_cells, bad);
    return bad ? 1 : 0;
}
