// The distance field's axis planes (vpx_skip.hpp GridView::dfa): every word of the host
// builder against a brute-force scan, and vpx::skip::walk_skip on those planes against the
// plain cell-by-cell reference march (template/scene.cpp:751-811).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I raytracer-voxpopuli_amd/csrc tests/native/axis_box_test.cpp
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
    GridView view() const {
        return GridView{cells.data(), l1.data(), l2.data(), n, nb1, nb2, nb3, dfp.data(), 64ull * nb2 * nb2 * nb2, dfa.data()};
    }
};

// kind 0: empty; 1: 1 % of the cells solid; 2: 30 %; 3: a ground plane with pillars
static World make_world(uint32_t n, int kind, uint64_t seed) {
    World w;
    w.n = n;
    w.cells.assign((size_t)n * n * n, 255);
    std::mt19937_64 r(seed);
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) -> uint8_t& { return w.cells[x + (size_t)y * n + (size_t)z * n * n]; };
    if (kind == 1 || kind == 2) {
        for (auto& c : w.cells)
            if (r() % 100 < (kind == 1 ? 1u : 30u)) c = (uint8_t)(r() % 200);
    } else if (kind == 3) {
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t x = 0; x < n; ++x) at(x, 0, z) = 1, at(x, 1, z) = 1;
        for (uint32_t p = 0; p < 1 + n / 12; ++p) {
            const uint32_t px = r() % n, pz = r() % n, h = 2 + r() % (n - 2);
            for (uint32_t y = 0; y < h; ++y) at(px, y, pz) = 2;
        }
    }
    w.nb1 = (n + 3) / 4, w.nb2 = (w.nb1 + 3) / 4, w.nb3 = (w.nb2 + 3) / 4;
    const size_t plane = 64ull * w.nb2 * w.nb2 * w.nb2;
    w.l1.assign(plane, 0);
    w.l2.assign((size_t)w.nb3 * w.nb3 * w.nb3 * 64, 0);
    build_masks_host(w.cells.data(), n, w.l1.data(), w.l2.data());
    w.dfp.assign(8 * plane, 0);
    build_planes_host(w.l1.data(), w.l2.data(), n, w.dfp.data());
    w.dfa.assign(24 * plane, 0xffff);
    build_axis_planes_host(w.dfp.data(), n, w.dfa.data());
    return w;
}

struct Seen {
    long corridor = 0;  // a box at least 8 bricks long on a cube of 1 or 2, ended by a solid cell inside the grid
    long edge = 0;      // a box that the grid's faces clip
    long cap = 0;       // L = 255
};

// Every (brick, octant, axis) word against the cells: brick occupancy and box emptiness by
// a 3-D prefix sum of solid cells per brick, counted from the cell bytes themselves.
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
    // solid cells in the bricks [lo, hi] (inclusive, already inside the grid)
    auto solid = [&](const uint32_t lo[3], const uint32_t hi[3]) {
        const uint32_t a = lo[0], b = lo[1], c = lo[2], d = hi[0] + 1, e = hi[1] + 1, f = hi[2] + 1;
        return S(d, e, f) - S(a, e, f) - S(d, b, f) - S(d, e, c) + S(a, b, f) + S(a, e, c) + S(d, b, c) - S(a, b, c);
    };
    const uint64_t plane = 64ull * W.nb2 * W.nb2 * W.nb2;
    long bad = 0;
    for (uint32_t z = 0; z < nb; ++z)
        for (uint32_t y = 0; y < nb; ++y)
            for (uint32_t x = 0; x < nb; ++x) {
                const uint32_t bi = blk_index(x, y, z, W.nb2);
                const bool occupied = cnt[x + (size_t)nb * (y + (size_t)nb * z)] != 0;
                for (uint32_t o = 0; o < 8; ++o)
                    for (uint32_t a = 0; a < 3; ++a) {
                        const uint32_t word = W.dfa[(o * 3 + a) * plane + bi], k = word & 255u, L = word >> 8;
                        bool ok = true;
                        if (occupied) {
                            ok = word == 0;
                        } else {
                            ok = k >= 1 && L >= k && k == W.dfp[o * plane + bi];
                            // the box, and the box one brick longer, in bricks; clipped to the grid
                            const uint32_t b[3] = {x, y, z};
                            uint32_t lo[3], hi[3], lo1[3], hi1[3];
                            bool clipped = false, longer_inside = true;
                            for (uint32_t q = 0; q < 3; ++q) {
                                const int64_t e = q == a ? L : k, s = ((o >> q) & 1u) ? -1 : 1;
                                int64_t far = (int64_t)b[q] + s * (e - 1), far1 = q == a ? far + s : far;
                                if (q == a && (far1 < 0 || far1 >= (int64_t)nb)) longer_inside = false;
                                if (far < 0 || far >= (int64_t)nb) clipped = true;
                                far = far < 0 ? 0 : (far >= (int64_t)nb ? nb - 1 : far);
                                far1 = far1 < 0 ? 0 : (far1 >= (int64_t)nb ? nb - 1 : far1);
                                lo[q] = s > 0 ? b[q] : (uint32_t)far, hi[q] = s > 0 ? (uint32_t)far : b[q];
                                lo1[q] = s > 0 ? b[q] : (uint32_t)far1, hi1[q] = s > 0 ? (uint32_t)far1 : b[q];
                            }
                            if (ok && solid(lo, hi) != 0) ok = false;  // the box is empty
                            // one brick longer is not, unless capped or at the grid edge
                            if (ok && L < 255u && (!longer_inside || solid(lo1, hi1) == 0)) ok = false;
                            if (ok) {
                                seen.edge += clipped;
                                seen.cap += L == 255u;
                                seen.corridor += k <= 2u && L >= 8u && L < 255u;
                            }
                        }
                        if (!ok) {
                            if (bad < 5) printf("plane word n=%u brick (%u,%u,%u) octant %u axis %u: k %u L %u occupied %d\n", n, x, y, z, o, a, k, L, (int)occupied);
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

// `planes <cells file> <n> <out file>`: the host builder's 24 planes of an n^3 grid of cell
// bytes, for the comparison with the device's (tests/test_axis_boxes.py).
static int dump_planes(const char* in, uint32_t n, const char* out) {
    std::vector<uint8_t> cells((size_t)n * n * n);
    FILE* f = fopen(in, "rb");
    if (!f || fread(cells.data(), 1, cells.size(), f) != cells.size()) return 2;
    fclose(f);
    const uint32_t nb1 = (n + 3) / 4, nb2 = (nb1 + 3) / 4, nb3 = (nb2 + 3) / 4;
    const size_t plane = 64ull * nb2 * nb2 * nb2;
    std::vector<uint64_t> l1(plane), l2((size_t)nb3 * nb3 * nb3 * 64);
    build_masks_host(cells.data(), n, l1.data(), l2.data());
    std::vector<uint8_t> dfp(8 * plane);
    build_planes_host(l1.data(), l2.data(), n, dfp.data());
    std::vector<uint16_t> dfa(24 * plane);
    build_axis_planes_host(dfp.data(), n, dfa.data());
    f = fopen(out, "wb");
    if (!f || fwrite(dfa.data(), 2, dfa.size(), f) != dfa.size()) return 2;
    fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "planes")) return dump_planes(argv[2], (uint32_t)atol(argv[3]), argv[4]);
    _mm_setcsr(_mm_getcsr() | 0x8040u);
    const long rays = argc > 1 ? atol(argv[1]) : 20000;
    long bad_words = 0, bad_rays = 0, total = 0, kinds[5] = {0, 0, 0, 0, 0};
    uint64_t cells_all = 0, cells_skip = 0;
    Seen seen;
    for (uint32_t n : {16u, 37u, 100u})
        for (int kind = 0; kind < 4; ++kind) {
            const World W = make_world(n, kind, n * 131 + kind);
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
                if (rk == 3) D[(ax + 1) % 3] = (r() & 1) ? D[ax] : -D[ax];
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
                cells_all += c0, cells_skip += c1;
                bool ok = r0 == r1 && c0 == c1;
                if (ok && r0) ok = std::memcmp(&h0.t, &h1.t, 4) == 0 && h0.X == h1.X && h0.Y == h1.Y && h0.Z == h1.Z;
                if (!ok) {
                    if (bad_rays < 10)
                        printf("n=%u kind %d ray %ld (%d): hit %d/%d cells %u/%u t %a/%a cell (%u,%u,%u)/(%u,%u,%u)\n", n, kind, i, rk, r0,
                               r1, c0, c1, h0.t, h1.t, h0.X, h0.Y, h0.Z, h1.X, h1.Y, h1.Z);
                    ++bad_rays;
                }
            }
        }
    printf("plane words bad=%ld\n", bad_words);
    printf("rays=%ld (outside %ld inside %ld parallel %ld tied %ld planar %ld) cells=%llu/%llu ray bad=%ld\n", total, kinds[0], kinds[1],
           kinds[2], kinds[3], kinds[4], (unsigned long long)cells_all, (unsigned long long)cells_skip, bad_rays);
    printf("seen: corridor=%ld edge=%ld cap255=%ld\n", seen.corridor, seen.edge, seen.cap);
    const bool spread = seen.corridor > 0 && seen.edge > 0 && seen.cap > 0 && kinds[2] > 0 && kinds[3] > 0 && kinds[1] > 0;
    if (!spread) printf("input spread missing\n");
    return (bad_words || bad_rays || !spread) ? 1 : 0;
}
