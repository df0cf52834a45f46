// The axis planes' widths (vpx_skip.hpp GridView::dfw): Mb and Mc of every word of the host
// builder against a brute-force scan, and vpx::skip::walk_skip on those planes against the
// plain cell-by-cell reference march (template/scene.cpp:751-811).
// Worlds: a street canyon (64^3), a ground slab with pillars (48^3), an empty grid (32^3) and
// a grid whose only solid cell sits in its far corner (37^3).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I raytracer-voxpopuli_amd/csrc tests/native/wide_box_test.cpp
// and again with -DVPX_WID_CAP=3u: the cap of the widths, which no grid this small reaches at 255.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <xmmintrin.h>
#include "vpx_skip.hpp"

using namespace vpx::skip;

struct World {
    uint32_t n, nb1, nb2, nb3;
    std::vector<uint8_t> cells;
    std::vector<uint64_t> l1, l2;
    std::vector<uint8_t> dfp;
    std::vector<uint16_t> dfa;
    std::vector<uint32_t> dfw;
    GridView view() const {
        return GridView{cells.data(), l1.data(), l2.data(), n, nb1, nb2, nb3, dfp.data(), 64ull * nb2 * nb2 * nb2, nullptr, dfw.data()};
    }
};

static void build_levels(World& w) {
    const uint32_t n = w.n;
    w.nb1 = (n + 3) / 4, w.nb2 = (w.nb1 + 3) / 4, w.nb3 = (w.nb2 + 3) / 4;
    const size_t plane = 64ull * w.nb2 * w.nb2 * w.nb2;
    w.l1.assign(plane, 0);
    w.l2.assign((size_t)w.nb3 * w.nb3 * w.nb3 * 64, 0);
    build_masks_host(w.cells.data(), n, w.l1.data(), w.l2.data());
    w.dfp.assign(8 * plane, 0);
    build_planes_host(w.l1.data(), w.l2.data(), n, w.dfp.data());
    w.dfa.assign(24 * plane, 0xffff);
    build_axis_planes_host(w.dfp.data(), n, w.dfa.data());
    w.dfw.assign(24 * plane, 0xffffffffu);
    build_wide_planes_host(w.dfp.data(), n, w.dfw.data());
}

// kind 0: street canyon; 1: ground slab with pillars; 2: empty; 3: one solid cell in the far corner
static World make_world(int kind, uint64_t seed) {
    static const uint32_t sizes[4] = {64, 48, 32, 37};
    World w;
    const uint32_t n = w.n = sizes[kind];
    w.cells.assign((size_t)n * n * n, 255);
    std::mt19937_64 r(seed);
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) -> uint8_t& { return w.cells[x + (size_t)y * n + (size_t)z * n * n]; };
    if (kind == 0) {  // ground, two walls 10 cells apart along z and 40 high, a crossing street, a pillar
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t x = 0; x < n; ++x) {
                at(x, 0, z) = 1;
                if ((x == 26 || x == 37) && !(z >= 30 && z < 36))
                    for (uint32_t y = 1; y < 41; ++y) at(x, y, z) = 5;
            }
        for (uint32_t y = 1; y < 20; ++y) at(31, y, 50) = 2;
    } else if (kind == 1) {
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t x = 0; x < n; ++x) at(x, 0, z) = 1, at(x, 1, z) = 1;
        for (uint32_t p = 0; p < 6; ++p) {
            const uint32_t px = r() % n, pz = r() % n, h = 2 + r() % (n - 2);
            for (uint32_t y = 0; y < h; ++y) at(px, y, pz) = 2;
        }
    } else if (kind == 3) {
        at(n - 1, n - 1, n - 1) = 3;
    }
    build_levels(w);
    return w;
}

struct Seen {
    long wider = 0;  // a width above the cube's k, ended by an occupied brick inside the grid
    long edge = 0;   // a width that reached the grid's face
    long cap = 0;    // a width that stopped at the cap with empty layers left
    long flat = 0;   // Mb != Mc
};

// Every (brick, octant, axis) word: the low half is the 16-bit builder's, and each width is the
// largest for which the box holds no solid cell, by a 3-D prefix sum of solid cells per brick.
static long check_builder(const World& W, Seen& seen) {
    const uint32_t nb = W.nb1, n = W.n;
    const size_t P = nb + 1;
    std::vector<uint32_t> sum(P * P * P, 0);  // sum[x][y][z]: solid cells in bricks [0,x) x [0,y) x [0,z)
    auto S = [&](uint32_t x, uint32_t y, uint32_t z) -> uint32_t& { return sum[x + P * (y + P * z)]; };
    std::vector<uint32_t> cnt((size_t)nb * nb * nb, 0);
    for (uint32_t z = 0; z < n; ++z)
        for (uint32_t y = 0; y < n; ++y)
            for (uint32_t x = 0; x < n; ++x)
                if (W.cells[x + (size_t)y * n + (size_t)z * n * n] != 255) ++cnt[(x >> 2) + (size_t)nb * ((y >> 2) + (size_t)nb * (z >> 2))];
    for (uint32_t z = 1; z <= nb; ++z)
        for (uint32_t y = 1; y <= nb; ++y)
            for (uint32_t x = 1; x <= nb; ++x)
                S(x, y, z) = cnt[(x - 1) + (size_t)nb * ((y - 1) + (size_t)nb * (z - 1))] + S(x - 1, y, z) + S(x, y - 1, z) + S(x, y, z - 1) -
                             S(x - 1, y - 1, z) - S(x - 1, y, z - 1) - S(x, y - 1, z - 1) + S(x - 1, y - 1, z - 1);
    // solid cells in the box of bricks that starts at b and has extent e[q] toward the octant,
    // clipped to the grid; *inside: the whole box lies in the grid
    auto solid = [&](const uint32_t b[3], uint32_t o, const int64_t e[3], bool* inside) {
        uint32_t lo[3], hi[3];
        *inside = true;
        for (uint32_t q = 0; q < 3; ++q) {
            const int64_t s = ((o >> q) & 1u) ? -1 : 1;
            int64_t far = (int64_t)b[q] + s * (e[q] - 1);
            if (far < 0 || far >= (int64_t)nb) *inside = false;
            far = far < 0 ? 0 : (far >= (int64_t)nb ? nb - 1 : far);
            lo[q] = s > 0 ? b[q] : (uint32_t)far, hi[q] = s > 0 ? (uint32_t)far : b[q];
        }
        const uint32_t a = lo[0], bb = lo[1], c = lo[2], d = hi[0] + 1, ee = hi[1] + 1, f = hi[2] + 1;
        return S(d, ee, f) - S(a, ee, f) - S(d, bb, f) - S(d, ee, c) + S(a, bb, f) + S(a, ee, c) + S(d, bb, c) - S(a, bb, c);
    };
    const uint64_t plane = 64ull * W.nb2 * W.nb2 * W.nb2;
    const uint32_t cap = VPX_WID_CAP;
    long bad = 0;
    for (uint32_t z = 0; z < nb; ++z)
        for (uint32_t y = 0; y < nb; ++y)
            for (uint32_t x = 0; x < nb; ++x) {
                const uint32_t bi = blk_index(x, y, z, W.nb2);
                const bool occupied = cnt[x + (size_t)nb * (y + (size_t)nb * z)] != 0;
                for (uint32_t o = 0; o < 8; ++o)
                    for (uint32_t a = 0; a < 3; ++a) {
                        const uint32_t word = W.dfw[(o * 3 + a) * plane + bi], k = word & 255u, L = (word >> 8) & 255u;
                        bool ok = (word & 0xffffu) == W.dfa[(o * 3 + a) * plane + bi] && (occupied ? word == 0 : k >= 1);
                        const uint32_t others[2] = {a == 0 ? 1u : 0u, a == 2 ? 1u : 2u};  // b < c
                        uint32_t M[2] = {0, 0};
                        for (uint32_t h = 0; h < 2 && ok && !occupied; ++h) {
                            const uint32_t sec = others[h], third = others[1 - h];
                            M[h] = (word >> (16 + 8 * h)) & 255u;
                            // the widest empty box, layer by layer from the cube's k (brute force)
                            const uint32_t b[3] = {x, y, z};
                            int64_t e[3];
                            e[a] = L, e[third] = k;
                            uint32_t want = k;
                            bool at_edge = false, at_cap = false;
                            for (;;) {
                                bool inside;
                                e[sec] = want;
                                if (solid(b, o, e, &inside) != 0) { ok = false; break; }  // even the k-wide box is not empty
                                const int64_t s = ((o >> sec) & 1u) ? -1 : 1, next = (int64_t)b[sec] + s * (int64_t)want;
                                if (next < 0 || next >= (int64_t)nb) { at_edge = true; want = k > cap ? k : cap; break; }
                                if (want >= cap) { at_cap = want == cap; break; }
                                e[sec] = want + 1;
                                if (solid(b, o, e, &inside) != 0) break;
                                ++want;
                            }
                            if (ok && M[h] != want) ok = false;
                            if (ok) {
                                seen.edge += at_edge;
                                seen.cap += at_cap;
                                seen.wider += !at_edge && !at_cap && want > k;
                            }
                            if (!ok && bad < 5)
                                printf("n=%u brick (%u,%u,%u) octant %u axis %u second %u: k %u L %u M %u want %u\n", n, x, y, z, o, a, sec, k, L,
                                       M[h], want);
                        }
                        if (ok && !occupied) seen.flat += M[0] != M[1];
                        if (!ok) {
                            if (bad < 5) printf("plane word n=%u brick (%u,%u,%u) octant %u axis %u: %08x occupied %d\n", n, x, y, z, o, a, word, (int)occupied);
                            ++bad;
                        }
                    }
            }
    return bad;
}

// Setup3DDDA for the unit cube (template/scene.cpp:719-749); false = misses the cube.
static bool setup(uint32_t n, const float O[3], const float D[3], Walk& w) {
    float rD[3], ds[3];
    for (int k = 0; k < 3; ++k) {
        rD[k] = 1.0f / D[k];
        uint32_t b;
        std::memcpy(&b, &D[k], 4);
        ds[k] = (float)(b >> 31);
    }
    float t = 0;
    const bool inside = O[0] >= 0 && O[1] >= 0 && O[2] >= 0 && O[0] <= 1 && O[1] <= 1 && O[2] <= 1;
    if (!inside) {
        float tmin = -1e30f, tmax = 1e30f;
        for (int k = 0; k < 3; ++k) {
            const int sg = D[k] < 0;
            float a = ((sg ? 1.f : 0.f) - O[k]) * rD[k], b = ((sg ? 0.f : 1.f) - O[k]) * rD[k];
            if (k == 0) { tmin = a, tmax = b; continue; }
            if (tmin > b || a > tmax) return false;
            tmin = tmin < a ? a : tmin;
            tmax = b < tmax ? b : tmax;
        }
        if (!(tmin > 0)) return false;
        t = tmin;
    }
    const float g = (float)n, cell = 1.0f / g;
    w = Walk{};
    uint32_t* P[3] = {&w.X, &w.Y, &w.Z};
    int32_t* st[3] = {&w.sx, &w.sy, &w.sz};
    float* tm[3] = {&w.tx, &w.ty, &w.tz};
    float* td[3] = {&w.dx, &w.dy, &w.dz};
    for (int k = 0; k < 3; ++k) {
        *st[k] = (int)(1.0f - ds[k] * 2.0f);
        const float pos = (O[k] + D[k] * (t + 0.00005f)) * g;
        const float plane = (std::ceil(pos) - ds[k]) * cell;
        const int p = (pos > -2147483904.0f && pos < 2147483648.0f) ? (int)pos : (int)0x80000000u;
        *P[k] = (uint32_t)(p < 0 ? 0 : (p > (int)n - 1 ? (int)n - 1 : p));
        *td[k] = cell * (float)*st[k] * rD[k];
        *tm[k] = (plane - O[k]) * rD[k];
    }
    w.t = t;
    walk_begin(w);
    return true;
}

// Scene::FindNearest's loop, cell by cell.
static bool walk_naive(const World& W, Walk s, float bound, uint32_t& cells, Walk& out) {
    const uint32_t n = W.n;
    while (s.t < bound) {
        const uint8_t c = W.cells[s.X + (size_t)s.Y * n + (size_t)s.Z * n * n];
        ++cells;
        if (c != 255 && s.t < bound) { out = s; return true; }
        if (s.tx < s.ty) {
            if (s.tx < s.tz) { s.t = s.tx; s.X += s.sx; if (s.X >= n) break; s.tx += s.dx; }
            else { s.t = s.tz; s.Z += s.sz; if (s.Z >= n) break; s.tz += s.dz; }
        } else {
            if (s.ty < s.tz) { s.t = s.ty; s.Y += s.sy; if (s.Y >= n) break; s.ty += s.dy; }
            else { s.t = s.tz; s.Z += s.sz; if (s.Z >= n) break; s.tz += s.dz; }
        }
    }
    return false;
}

// `planes <cells file> <n> <out file>`: the host builder's 24 planes of 32-bit words of an n^3
// grid of cell bytes, for the comparison with the device's (tests/test_wide_boxes_gpu.py).
static int dump_planes(const char* in, uint32_t n, const char* out) {
    World w;
    w.n = n;
    w.cells.resize((size_t)n * n * n);
    FILE* f = fopen(in, "rb");
    if (!f || fread(w.cells.data(), 1, w.cells.size(), f) != w.cells.size()) return 2;
    fclose(f);
    build_levels(w);
    f = fopen(out, "wb");
    if (!f || fwrite(w.dfw.data(), 4, w.dfw.size(), f) != w.dfw.size()) return 2;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "planes")) return dump_planes(argv[2], (uint32_t)atol(argv[3]), argv[4]);
    _mm_setcsr(_mm_getcsr() | 0x8040u);
    const long rays = argc > 1 ? atol(argv[1]) : 5000;
    long bad_words = 0, bad_rays = 0, total = 0, kinds[5] = {0, 0, 0, 0, 0}, hits = 0;
    uint64_t cells_all = 0, cells_skip = 0;
    Seen seen;
    for (int kind = 0; kind < 4; ++kind) {
        const World W = make_world(kind, 977 + kind);
        const uint32_t n = W.n;
        bad_words += check_builder(W, seen);
        std::mt19937_64 r(n * 7 + kind);
        std::uniform_real_distribution<float> U(0.f, 1.f);
        for (long i = 0; i < rays; ++i) {
            float O[3], D[3];
            // 0: from outside; 1: from inside; 2: parallel to an axis (two infinite tdeltas);
            // 3: two equal components (tied tdeltas); 4: in a coordinate plane (one infinite tdelta)
            const int rk = (int)(i % 5);
            for (int k = 0; k < 3; ++k) {
                O[k] = (rk == 0 || (rk >= 2 && i % 2)) ? -0.6f + 2.2f * U(r) : U(r);
                D[k] = 0.05f + 0.9f * U(r) - O[k];
            }
            const int ax = (int)(r() % 3);
            if (rk == 2) {
                for (int k = 0; k < 3; ++k)
                    if (k != ax) D[k] = 0.0f, O[k] = U(r);
                if (D[ax] == 0.0f) D[ax] = 1.0f;
            }
            if (rk == 3) {
                D[(ax + 1) % 3] = (r() & 1) ? D[ax] : -D[ax];
                if (i % 10 == 3) D[(ax + 2) % 3] = (r() & 1) ? D[ax] : -D[ax];  // all three tied
            }
            if (rk == 4) D[ax] = 0.0f, O[ax] = (r() & 1) ? U(r) : (float)(r() % n) / (float)n;
            const float len = std::sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
            if (!(len > 0)) continue;
            for (int k = 0; k < 3; ++k) D[k] = D[k] * (1.0f / len);
            Walk s;
            if (!setup(n, O, D, s)) continue;
            const float bound = (i % 3 == 0) ? 1e34f : 0.2f + 2.0f * U(r);
            uint32_t c0 = 0, c1 = 0;
            Walk h0{}, h1 = s;
            const bool r0 = walk_naive(W, s, bound, c0, h0);
            const bool r1 = walk_skip(W.view(), h1, bound, c1);
            ++total, ++kinds[rk];
            hits += r0;
            cells_all += c0, cells_skip += c1;
            bool ok = r0 == r1 && c0 == c1;
            if (ok && r0) ok = std::memcmp(&h0.t, &h1.t, 4) == 0 && h0.X == h1.X && h0.Y == h1.Y && h0.Z == h1.Z;
            if (!ok) {
                if (bad_rays < 10)
                    printf("n=%u kind %d ray %ld (%d): hit %d/%d cells %u/%u t %a/%a cell (%u,%u,%u)/(%u,%u,%u)\n", n, kind, i, rk, r0, r1, c0,
                           c1, h0.t, h1.t, h0.X, h0.Y, h0.Z, h1.X, h1.Y, h1.Z);
                ++bad_rays;
            }
        }
    }
    printf("cap=%u plane words bad=%ld\n", (unsigned)VPX_WID_CAP, bad_words);
    printf("rays=%ld (outside %ld inside %ld parallel %ld tied %ld planar %ld) hits=%ld cells=%llu/%llu ray bad=%ld\n", total, kinds[0],
           kinds[1], kinds[2], kinds[3], kinds[4], hits, (unsigned long long)cells_all, (unsigned long long)cells_skip, bad_rays);
    printf("seen: wider=%ld edge=%ld cap=%ld flat=%ld\n", seen.wider, seen.edge, seen.cap, seen.flat);
    // the cap shows only in the build that lowers it: at 255 no box of these grids reaches it
    const bool spread = seen.wider > 0 && seen.edge > 0 && seen.flat > 0 && (VPX_WID_CAP >= 255u || seen.cap > 0) && hits > 0 &&
                        kinds[1] > 0 && kinds[2] > 0 && kinds[3] > 0;
    if (!spread) printf("input spread missing\n");
    return (bad_words || bad_rays || !spread) ? 1 : 0;
}
