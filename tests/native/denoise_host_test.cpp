// denoise_host_test.cpp — csrc/vpx_denoise.hpp's host path in a stand-alone program, meant to be
// built with -fsanitize=address,undefined: every buffer is a heap block of exactly the size the
// call is entitled to, so a tap read outside the image or a key used as an index is a report.
// Patterns: stripes of width 3, and a mix of one plane with the four kinds of invalid record and
// arbitrary bits in every field the key must not read; 5x3 (every tap of steps 4..16 outside) and
// 67x35; passes 1..5, sigma_l 0 and 0.5.  Checked here: invalid keys and .w pass through bit for
// bit, and a constant colour on a plane comes back exactly with sigma_l == 0.  (The bits of the
// filtered pixels are tests/test_denoise.py's business.)
#include <cstdio>
#include <cstring>
#include <vector>

#include "vpx_denoise.hpp"

using namespace vpx::denoise;

static uint32_t rng_state = 0x12345678u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 17, rng_state ^= rng_state << 5;
    return rng_state;
}

static std::vector<uint32_t> make_ids(uint32_t W, uint32_t H, int pattern) {
    std::vector<uint32_t> ids((size_t)W * H * 4);
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) {
            uint32_t* r = &ids[4 * ((size_t)y * W + x)];
            r[0] = rnd(), r[2] = rnd(), r[3] = rnd();  // t and the cell: any bits (coordinates beyond 4095 too)
            if (pattern == 0) {
                r[1] = 2u | 3u << 16 | 3u << 24;                               // face 3: axis 1
                r[2] = (r[2] & 0xffffu) | (7u + (x / 3u) % 2u) << 16;
            } else {
                const uint32_t kind = y * 5 < H * 3 ? 0u : 1u + x * 4 / W;
                const uint32_t v = kind == 1 ? 0u : kind == 2 ? 1u : 2u;
                const uint32_t face = kind == 0 ? 6u : kind == 1 ? 0u : kind == 2 ? 2u : kind == 3 ? 0u : 7u + (rnd() & 0xf8u);
                r[1] = v | (rnd() & 0xffu) << 16 | face << 24;
                if (kind == 0) r[1] = 2u | 5u << 16 | 6u << 24, r[3] = 4095u;   // face 6: axis 2
            }
        }
    return ids;
}

int main() {
    long bad = 0, calls = 0;
    const uint32_t sizes[2][2] = {{5, 3}, {67, 35}};
    for (const auto& sz : sizes)
        for (int pattern = 0; pattern < 2; ++pattern)
            for (uint32_t passes = 1; passes <= kMaxPasses; ++passes)
                for (int lum_on = 0; lum_on < 2; ++lum_on)
                    for (int constant = 0; constant < 2; ++constant) {
                        const uint32_t W = sz[0], H = sz[1];
                        const size_t n = (size_t)W * H;
                        const std::vector<uint32_t> ids = make_ids(W, H, pattern);
                        std::vector<float> in(4 * n), out(4 * n, -1.f), a(passes > 1 ? 4 * n : 0), b(passes > 1 ? 4 * n : 0);
                        std::vector<uint32_t> rgb(n);
                        std::vector<Key> keys(n);
                        for (size_t p = 0; p < n; ++p) {
                            for (int k = 0; k < 3; ++k) in[4 * p + k] = constant ? 0.75f : 0.015625f * (float)(1u + rnd() % 4096u);
                            const uint32_t wbits = rnd();
                            std::memcpy(&in[4 * p + 3], &wbits, 4);
                        }
                        const vpx_denoise d{passes, lum_on ? 0.5f : 0.0f, 0u, 0u};
                        if (check_call(W, H, ids.data(), in.data(), out.data(), &d)) ++bad;
                        run_host(W, H, ids.data(), in.data(), out.data(), rgb.data(), d, keys.data(), a.data(), b.data());
                        ++calls;
                        for (size_t p = 0; p < n; ++p) {
                            const bool ok = valid(keys[p]);
                            if (std::memcmp(&out[4 * p + 3], &in[4 * p + 3], 4)) ++bad;
                            if (!ok && std::memcmp(&out[4 * p], &in[4 * p], 16)) ++bad;
                            if (ok && constant && !lum_on && std::memcmp(&out[4 * p], &in[4 * p], 12)) ++bad;
                            if (rgb[p] != tonemap_pack_host(&out[4 * p])) ++bad;
                        }
                    }
    std::printf("denoise host: calls=%ld bad=%ld\n", calls, bad);
    return bad ? 1 : 0;
}
