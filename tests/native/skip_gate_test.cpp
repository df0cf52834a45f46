// The walkers' maturity gate and further lean segments (vpx_skip.hpp gate_open, axis_rebase):
// 1. skip_box_lean<true, MORE>, MORE = 1..4, against the general skip_box on the box it clipped
//    to, on random boxes and on boxes of 255 bricks whose heads start in [0.25, 0.5) and cross two
//    and three binade boundaries (taken whole with MORE >= 1 and MORE >= 2);
// 2. walk_skip with the gate for G in {1, 2, 3} x N in {4, 8, 16}, with MORE = 0..4 and with
//    both, against the plain cell-by-cell reference march (template/scene.cpp:751-811) on random
//    64^3 and 128^3 worlds with streets and walls: hit, cell count, and at a hit the cell, the t
//    bits and the three heads' bits.  Rays from outside, from inside (t = 0), from a cell face at
//    t = 0, parallel to an axis (infinite tdeltas), in a coordinate plane, with tied components;
// 3. the same walks from states whose heads and tdeltas are drawn from the suite's small value
//    set (skip_walk_test.cpp), dense in ties, zeros, infinities and NaNs.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I raytracer-voxpopuli_amd/csrc tests/native/skip_gate_test.cpp
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
    std::vector<uint32_t> dfw;
    GridView view() const {
        return GridView{cells.data(), l1.data(), l2.data(), n, nb1, nb2, nb3, dfp.data(), 64ull * nb2 * nb2 * nb2, nullptr, dfw.data()};
    }
};

// Ground, a grid of streets between blocks of random height with holes, and free-standing walls.
static World make_world(uint32_t n, uint64_t seed) {
    World w;
    w.n = n;
    w.cells.assign((size_t)n * n * n, 255);
    std::mt19937_64 r(seed);
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) -> uint8_t& { return w.cells[x + (size_t)y * n + (size_t)z * n * n]; };
    const uint32_t pitch = n / 4, street = 5 + (uint32_t)(r() % 4);
    for (uint32_t z = 0; z < n; ++z)
        for (uint32_t x = 0; x < n; ++x) at(x, 0, z) = 1;
    for (uint32_t bz = 0; bz < 4; ++bz)
        for (uint32_t bx = 0; bx < 4; ++bx) {
            const uint32_t h = 3 + (uint32_t)(r() % (n / 2));
            for (uint32_t z = bz * pitch + street; z < (bz + 1) * pitch; ++z)
                for (uint32_t x = bx * pitch + street; x < (bx + 1) * pitch; ++x)
                    for (uint32_t y = 1; y < h; ++y)
                        if (r() % 17) at(x, y, z) = (uint8_t)(2 + r() % 100);
        }
    for (int k = 0; k < 3; ++k) {  // thin walls across a street, one cell thick
        const uint32_t x = (uint32_t)(r() % n), z0 = (uint32_t)(r() % n), len = 4 + (uint32_t)(r() % (n / 3)), h = 2 + (uint32_t)(r() % (n / 3));
        for (uint32_t z = z0; z < std::min(n, z0 + len); ++z)
            for (uint32_t y = 1; y < h; ++y) at(x, y, z) = 7;
    }
    w.nb1 = (n + 3) / 4, w.nb2 = (w.nb1 + 3) / 4, w.nb3 = (w.nb2 + 3) / 4;
    const size_t plane = 64ull * w.nb2 * w.nb2 * w.nb2;
    w.l1.assign(plane, 0);
    w.l2.assign((size_t)w.nb3 * w.nb3 * w.nb3 * 64, 0);
    build_masks_host(w.cells.data(), n, w.l1.data(), w.l2.data());
    w.dfp.assign(8 * plane, 0);
    build_planes_host(w.l1.data(), w.l2.data(), n, w.dfp.data());
    w.dfw.assign(24 * plane, 0xffffffffu);
    build_wide_planes_host(w.dfp.data(), n, w.dfw.data());
    return w;
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

// The variants: 0 = the plain walk (the baseline of the baseline), then the nine gates, the
// four segment counts, and gates on top of further segments.
static std::vector<uint32_t> variants() {
    std::vector<uint32_t> v{0u};
    for (uint32_t G = 1; G <= 3; ++G)
        for (uint32_t f = 0; f <= 2; ++f) v.push_back(gate_word(G, f));
    for (uint32_t m = 1; m <= 4; ++m) v.push_back(m << 5);
    for (uint32_t m = 1; m <= 3; ++m)
        for (uint32_t G = 1; G <= 2; ++G) v.push_back(gate_word(G, m - 1u) | m << 5);
    return v;
}

struct Tally {
    long total = 0, bad = 0, hits = 0;
    uint64_t cells = 0;
};

// One start state through the cell march and every variant.
static void check_walk(const World& W, const Walk& s, float bound, const std::vector<uint32_t>& vs, Tally& T, const char* what, long i) {
    uint32_t c0 = 0;
    Walk h0{};
    const bool r0 = walk_naive(W, s, bound, c0, h0);
    ++T.total, T.hits += r0, T.cells += c0;
    for (uint32_t v : vs) {
        uint32_t c1 = 0;
        Walk h1 = s;
        const bool r1 = walk_skip(W.view(), h1, bound, c1, v);
        bool ok = r0 == r1 && c0 == c1;
        if (ok && r0)
            ok = !std::memcmp(&h0.t, &h1.t, 4) && h0.X == h1.X && h0.Y == h1.Y && h0.Z == h1.Z && !std::memcmp(&h0.tx, &h1.tx, 4) &&
                 !std::memcmp(&h0.ty, &h1.ty, 4) && !std::memcmp(&h0.tz, &h1.tz, 4);
        if (!ok) {
            if (T.bad < 10)
                printf("n=%u %s %ld variant %#x: hit %d/%d cells %u/%u t %a/%a cell (%u,%u,%u)/(%u,%u,%u) heads %a %a %a / %a %a %a\n"
                       "   start X %u %u %u s %d %d %d t %a h %a %a %a d %a %a %a bound %a\n",
                       W.n, what, i, v, r0, r1, c0, c1, h0.t, h1.t, h0.X, h0.Y, h0.Z, h1.X, h1.Y, h1.Z, h0.tx, h0.ty, h0.tz, h1.tx, h1.ty,
                       h1.tz, s.X, s.Y, s.Z, s.sx, s.sy, s.sz, s.t, s.tx, s.ty, s.tz, s.dx, s.dy, s.dz, bound);
            ++T.bad;
        }
    }
}

// Part 1.  Returns the number of failures.
static float rnd_head(std::mt19937_64& r, std::uniform_real_distribution<double>& U, int kind) {
    switch (kind) {
        case 0: return (float)std::exp(std::log(1e-3) + U(r) * (std::log(8.0) - std::log(1e-3)));
        case 1: return std::nextafter((float)std::ldexp(1.0, (int)(r() % 6) - 3), 0.f) - (float)(U(r) * 1e-3);  // just below 2^k
        default: return (float)std::ldexp(1.0, (int)(r() % 6) - 3) * (float)(1.0 + (r() % 64) * std::ldexp(1.0, -20));
    }
}
template <int MORE>
static long box_check(long iters) {
    std::mt19937_64 r(4242 + MORE);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long bad = 0, taken = 0, whole = 0, whole0 = 0, shrunk = 0, long2 = 0, long3 = 0, long2_whole = 0, long3_whole = 0;
    for (long i = 0; i < iters; ++i) {
        Walk w{};
        // every fourth box: 255 bricks a side, heads in [0.25, 0.5), tdeltas that put the far face
        // two or three binade boundaries on (kind 1: two, kind 2: three)
        const int long_kind = (i & 3) == 3 ? 1 + (int)(r() & 1) : 0;
        const uint32_t m = long_kind ? 1019u : (i & 3) == 0 ? 15u : (i & 3) == 1 ? 63u : 255u;
        uint32_t lo[3], hi[3];
        uint32_t* C3[3] = {&w.X, &w.Y, &w.Z};
        float* H3[3] = {&w.tx, &w.ty, &w.tz};
        float* D3[3] = {&w.dx, &w.dy, &w.dz};
        int32_t* S3[3] = {&w.sx, &w.sy, &w.sz};
        float tmin = 1e30f;
        for (int k = 0; k < 3; ++k) {
            lo[k] = long_kind ? 0u : (uint32_t)(r() % 4) * (m + 1);
            hi[k] = lo[k] + m;
            *S3[k] = (r() & 1) ? 1 : -1;
            *C3[k] = long_kind ? (*S3[k] > 0 ? lo[k] : hi[k]) : lo[k] + (uint32_t)(r() % (m + 1));
            float h, d;
            if (long_kind) {
                h = 0.25f + 0.25f * (float)U(r);
                // the far face at A(1019) ~ h + 1019 d, inside [1, 2) or [2, 4)
                const float far = long_kind == 1 ? 1.05f + 0.9f * (float)U(r) : 2.1f + 1.8f * (float)U(r);
                d = (far - h) / 1019.0f;
            } else {
                h = rnd_head(r, U, (int)(r() % 3));
                switch (r() % 4) {
                    case 0: d = (float)std::exp(std::log(1e-5) + U(r) * (std::log(0.5) - std::log(1e-5))); break;
                    case 1: d = h * (float)std::ldexp(1.0, -(int)(1 + r() % 26)); break;  // ties / stuck
                    case 2: d = (float)std::ldexp(1.0, -(int)(4 + r() % 12)) * (float)(1 + r() % 8); break;
                    default: d = h * (float)(U(r) * 0.05); break;
                }
            }
            *H3[k] = h, *D3[k] = d;
            tmin = h < tmin ? h : tmin;
        }
        w.t = tmin * (float)U(r);
        const float hmax = w.tx > w.ty ? (w.tx > w.tz ? w.tx : w.tz) : (w.ty > w.tz ? w.ty : w.tz);
        const int bk = (int)(r() % 4);
        const float bound = (long_kind || bk == 0) ? 1e34f : bk == 1 ? INFINITY : (float)(tmin + U(r) * (hmax * 4 - tmin));
        Walk a = w, b = w, a0 = w;
        uint32_t lo1[3] = {lo[0], lo[1], lo[2]}, hi1[3] = {hi[0], hi[1], hi[2]}, lo0[3] = {lo[0], lo[1], lo[2]}, hi0[3] = {hi[0], hi[1], hi[2]};
        uint32_t ca = 7, cb = 7, c0 = 7;
        const int ra = skip_box_lean<true, MORE>(a, lo1, hi1, bound, ca);
        const int r0 = skip_box_lean(a0, lo0, hi0, bound, c0);
        if ((ra == 2) != (r0 == 2)) { ++bad; continue; }
        if (ra == 2) continue;
        ++taken;
        bool clipped = false, clipped0 = false, smaller = false;
        for (int k = 0; k < 3; ++k) {
            clipped |= lo1[k] != lo[k] || hi1[k] != hi[k];
            clipped0 |= lo0[k] != lo[k] || hi0[k] != hi[k];
            smaller |= lo1[k] > lo0[k] || hi1[k] < hi0[k];  // never a smaller box than the two segments'
        }
        whole += !clipped, whole0 += !clipped0, shrunk += smaller;
        if (long_kind == 1) ++long2, long2_whole += !clipped;
        if (long_kind == 2) ++long3, long3_whole += !clipped;
        const int rb = skip_box(b, lo1, hi1, bound, cb);
        if (!(ra == rb && ca == cb && (ra == 1 || !memcmp(&a, &b, sizeof(Walk))))) {
            if (bad < 10)
                printf("MORE=%d mismatch r %d/%d cells %u/%u t %a/%a\n  in: X %u %u %u s %d %d %d lo %u %u %u hi %u %u %u t %a h %a %a %a d %a %a %a bound %a\n"
                       "  out lean: h %a %a %a XYZ %u %u %u | ref: h %a %a %a XYZ %u %u %u\n",
                       MORE, ra, rb, ca, cb, a.t, b.t, w.X, w.Y, w.Z, w.sx, w.sy, w.sz, lo1[0], lo1[1], lo1[2], hi1[0], hi1[1], hi1[2], w.t, w.tx,
                       w.ty, w.tz, w.dx, w.dy, w.dz, bound, a.tx, a.ty, a.tz, a.X, a.Y, a.Z, b.tx, b.ty, b.tz, b.X, b.Y, b.Z);
            ++bad;
        }
    }
    printf("segments MORE=%d: %ld taken, whole %ld (two segments: %ld), smaller boxes %ld, 255-brick boxes over two boundaries %ld/%ld whole, over three "
           "%ld/%ld, bad=%ld\n", MORE, taken, whole, whole0, shrunk, long2_whole, long2, long3_whole, long3, bad);
    // The boxes this tier is for are taken whole, unless a tie in a later binade keeps an axis
    // clipped: a tdelta whose low sh bits are 10...0 at that binade's shift sh.  Here h / d >= 69,
    // so sh >= 7, 8, 9 in the second to fourth binade: at most 2^-7 + 2^-8 + 2^-9 per axis, 4.1 % for
    // the three.  Hence 95 %.
    const bool reach = long2 > 0 && long3 > 0 && long2_whole * 100 >= long2 * 95 && (MORE < 2 || long3_whole * 100 >= long3 * 95) && whole > whole0;
    if (!reach) printf("MORE=%d: the long boxes are not taken whole\n", MORE);
    return bad + shrunk + !reach;
}

int main(int argc, char** argv) {
    _mm_setcsr(_mm_getcsr() | 0x8040u);
    const long rays = argc > 1 ? atol(argv[1]) : 3000;
    long bad_boxes = box_check<1>(150000) + box_check<2>(150000) + box_check<3>(150000) + box_check<4>(150000);
    printf("box bad=%ld\n", bad_boxes);
    const std::vector<uint32_t> vs = variants();
    Tally rt, st;
    long kinds[6] = {0, 0, 0, 0, 0, 0};
    for (uint32_t n : {64u, 128u}) {
        const World W = make_world(n, 31 * n + 5);
        std::mt19937_64 r(n * 13 + 1);
        std::uniform_real_distribution<float> U(0.f, 1.f);
        for (long i = 0; i < rays; ++i) {
            float O[3], D[3];
            // 0: from outside; 1: from inside (t = 0); 2: parallel to an axis (two infinite tdeltas);
            // 3: two equal components (tied tdeltas); 4: in a coordinate plane (one infinite tdelta);
            // 5: from inside, on a cell face (t = 0 and a head of 0 or a whole tdelta)
            const int rk = (int)(i % 6);
            for (int k = 0; k < 3; ++k) {
                O[k] = (rk == 0 || ((rk == 2 || rk == 3 || rk == 4) && i % 2)) ? -0.6f + 2.2f * U(r) : U(r);
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
                if (i % 12 == 3) D[(ax + 2) % 3] = (r() & 1) ? D[ax] : -D[ax];  // all three tied
            }
            if (rk == 4) D[ax] = 0.0f, O[ax] = (r() & 1) ? U(r) : (float)(r() % n) / (float)n;
            if (rk == 5) {
                O[ax] = (float)(1 + r() % (n - 1)) / (float)n;
                if (i % 12 == 5) O[(ax + 1) % 3] = (float)(1 + r() % (n - 1)) / (float)n;  // on a cell edge
            }
            const float len = std::sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
            if (!(len > 0)) continue;
            for (int k = 0; k < 3; ++k) D[k] = D[k] * (1.0f / len);
            Walk s;
            if (!setup(n, O, D, s)) continue;
            const float bound = (i % 3 == 0) ? 1e34f : 0.2f + 2.0f * U(r);
            ++kinds[rk];
            check_walk(W, s, bound, vs, rt, "ray", i);
        }
        // Part 3: heads and tdeltas from the value set
        const float vals[] = {0.0f, -0.0f, 1.0f, 1.0f, 0.5f, 2.0f, 1e-30f, 3.4e38f, INFINITY, -INFINITY, NAN, 0.25f};
        for (long i = 0; i < rays * 2; ++i) {
            Walk s{};
            s.X = (uint32_t)(r() % n), s.Y = (uint32_t)(1 + r() % (n - 1)), s.Z = (uint32_t)(r() % n);
            s.sx = (r() & 1) ? 1 : -1, s.sy = (r() & 1) ? 1 : -1, s.sz = (r() & 1) ? 1 : -1;
            float* h[3] = {&s.tx, &s.ty, &s.tz};
            float* d[3] = {&s.dx, &s.dy, &s.dz};
            for (int k = 0; k < 3; ++k) {
                *h[k] = (r() % 4) ? vals[r() % 12] : (float)(r() % 1000) * 0.001f;
                *d[k] = (r() % 3) ? ((r() & 1) ? vals[r() % 12] : vals[r() % 12] * (1.0f / 64.0f)) : (float)(1 + r() % 64) * (1.0f / 1024.0f);
            }
            s.t = (r() & 1) ? 0.0f : vals[r() % 12];
            walk_begin(s);
            const float bound = (i % 3 == 0) ? 1e34f : (i % 3 == 1 ? INFINITY : 0.5f + 4.0f * U(r));
            check_walk(W, s, bound, vs, st, "state", i);
        }
    }
    printf("variants=%zu rays=%ld (outside %ld inside %ld parallel %ld tied %ld planar %ld face %ld) hits=%ld cells=%llu ray bad=%ld\n", vs.size(),
           rt.total, kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], kinds[5], rt.hits, (unsigned long long)rt.cells, rt.bad);
    printf("states=%ld hits=%ld cells=%llu state bad=%ld\n", st.total, st.hits, (unsigned long long)st.cells, st.bad);
    const bool spread = rt.hits > 0 && st.hits > 0 && kinds[1] > 0 && kinds[2] > 0 && kinds[3] > 0 && kinds[4] > 0 && kinds[5] > 0;
    if (!spread) printf("input spread missing\n");
    return (bad_boxes || rt.bad || st.bad || !spread) ? 1 : 0;
}
