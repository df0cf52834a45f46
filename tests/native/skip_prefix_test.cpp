// The lean tier's plain-step prefix (vpx_skip.hpp skip_box_lean's PRE, walk_skip's kGatePre):
// 1. skip_box_lean<true, 0, true> and <false, 0, true> against each other and against the general
//    skip_box on the box they clipped to, on random boxes whose heads are drawn so that one, two or
//    all three axes are immature (h < d, h in d's binade, h one ulp below a power of two, a d that
//    makes the plain step a tie), the other axes mature;
// 2. walk_skip with the bit, alone, with every gate G in {1, 2, 3} x N in {4, 8, 16} and with further
//    segments, against the cell-by-cell reference march on 64^3 and 128^3 street worlds: hit, cell
//    count, and at a hit the cell, the t bits and the heads' bits.  Rays start at t = 0 inside the
//    grid, on a cell face, with tied components and parallel to an axis, and from outside;
// 3. an instrumented copy of walk_skip's loop counts the skips that advanced an axis the lean tier
//    without the bit clips to zero events (its first segment refused): per ray class, printed, and
//    not zero in the t = 0 classes, where every axis starts immature;
// 4. with the bit off the results are the ones of the tier before the bit: a checksum over every
//    box's and every walk's outcome, recorded from the header before the change (built with
//    -DSKIP_PREFIX_PARENT, which leaves out everything that names the bit).
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I raytracer-voxpopuli_amd/csrc tests/native/skip_prefix_test.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <xmmintrin.h>
#include "vpx_skip.hpp"

using namespace vpx::skip;

// The outcomes without the bit, from the header before it (see 4. above).
static const uint64_t kBoxSumOff = 0xfcf4eb40ede0ca83ull;
static const uint64_t kWalkSumOff = 0xc01321da70ac8693ull;

static uint64_t g_sum = 1469598103934665603ull;  // FNV-1a over the words fed
static void feed(uint64_t v) {
    for (int i = 0; i < 8; ++i) g_sum = (g_sum ^ ((v >> (8 * i)) & 255u)) * 1099511628211ull;
}
static void feed_walk(const Walk& w) {
    feed(w.X), feed(w.Y), feed(w.Z), feed(fbits(w.t)), feed(fbits(w.tx)), feed(fbits(w.ty)), feed(fbits(w.tz));
}

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

#ifndef SKIP_PREFIX_PARENT
// walk_skip's loop on the wide boxes with the bit (no gate), counting the skips that advanced an
// axis whose first segment is refused: the tier without the bit clips that axis to zero events.
static bool walk_counted(const GridView& g, Walk& w, float bound, uint32_t& cells, long& skips, long& reached) {
    const uint32_t axis = dom_axis(w), sec = sec_axis(w);
    const uint32_t apar = plane_parent(g, (w.osh >> 3) * 3u + axis);
    for (;;) {
        if (!(w.t < bound)) return false;
        const int cls = classify_axis_o(w, g, apar);
        if (cls == 0) {
            ++cells;
            return true;
        }
        if (cls == 2) {
            uint32_t lo[3], hi[3], b, c, e;
            df_box_axis(w, g.n, cube_dfp(w), len_dfa(w), axis, lo, hi, sec, wid_dfw(w, axis, sec));
            const bool rx = !seg_params_nb(w.tx, w.dx, b, c, e), ry = !seg_params_nb(w.ty, w.dy, b, c, e),
                       rz = !seg_params_nb(w.tz, w.dz, b, c, e);
            const uint32_t X = w.X, Y = w.Y, Z = w.Z;
            const int sr = skip_box_lean<true, 0, true>(w, lo, hi, bound, cells);
            if (sr == 1) return false;
            if (sr == 0) {
                ++skips;
                reached += (rx && w.X != X) || (ry && w.Y != Y) || (rz && w.Z != Z);
            }
        }
        ++cells;
        if (!step1(w, g.n)) return false;
    }
}
#endif

struct Tally {
    long total = 0, bad = 0, hits = 0;
    uint64_t cells = 0;
};

static bool same_end(bool r0, bool r1, uint32_t c0, uint32_t c1, const Walk& h0, const Walk& h1) {
    bool ok = r0 == r1 && c0 == c1;
    if (ok && r0)
        ok = !std::memcmp(&h0.t, &h1.t, 4) && h0.X == h1.X && h0.Y == h1.Y && h0.Z == h1.Z && !std::memcmp(&h0.tx, &h1.tx, 4) &&
             !std::memcmp(&h0.ty, &h1.ty, 4) && !std::memcmp(&h0.tz, &h1.tz, 4);
    return ok;
}

// One start state through the cell march, the walk without the bit (fed to the checksum) and the
// variants with it.
static void check_walk(const World& W, const Walk& s, float bound, const std::vector<uint32_t>& vs, Tally& T, int rk, long i, long skips[],
                       long reached[]) {
    uint32_t c0 = 0;
    Walk h0{};
    const bool r0 = walk_naive(W, s, bound, c0, h0);
    ++T.total, T.hits += r0, T.cells += c0;
    for (uint32_t off : {0u, gate_word(1u, 0u)}) {  // without the bit: plain, and the shipped gate
        uint32_t c1 = 0;
        Walk h1 = s;
        const bool r1 = walk_skip(W.view(), h1, bound, c1, off);
        feed(r1), feed(c1);
        if (r1) feed_walk(h1);
        if (!same_end(r0, r1, c0, c1, h0, h1)) ++T.bad;
    }
#ifndef SKIP_PREFIX_PARENT
    for (uint32_t v : vs) {
        uint32_t c1 = 0;
        Walk h1 = s;
        const bool r1 = walk_skip(W.view(), h1, bound, c1, v);
        if (!same_end(r0, r1, c0, c1, h0, h1)) {
            if (T.bad < 10)
                printf("n=%u class %d ray %ld variant %#x: hit %d/%d cells %u/%u t %a/%a cell (%u,%u,%u)/(%u,%u,%u) heads %a %a %a / %a %a %a\n"
                       "   start X %u %u %u s %d %d %d t %a h %a %a %a d %a %a %a bound %a\n",
                       W.n, rk, i, v, r0, r1, c0, c1, h0.t, h1.t, h0.X, h0.Y, h0.Z, h1.X, h1.Y, h1.Z, h0.tx, h0.ty, h0.tz, h1.tx, h1.ty,
                       h1.tz, s.X, s.Y, s.Z, s.sx, s.sy, s.sz, s.t, s.tx, s.ty, s.tz, s.dx, s.dy, s.dz, bound);
            ++T.bad;
        }
    }
    {
        uint32_t c1 = 0;
        Walk h1 = s;
        const bool r1 = walk_counted(W.view(), h1, bound, c1, skips[rk], reached[rk]);
        if (!same_end(r0, r1, c0, c1, h0, h1)) {
            if (T.bad < 10) printf("n=%u class %d ray %ld counted walk: hit %d/%d cells %u/%u\n", W.n, rk, i, r0, r1, c0, c1);
            ++T.bad;
        }
    }
#else
    (void)vs, (void)rk, (void)i, (void)skips, (void)reached;
#endif
}

// A head and tdelta for one axis.  kind 0: mature (the existing suites' draws); 1: h < d, any
// distance; 2: h in d's binade; 3: h one ulp below a power of two, d at or above that power; 4: h
// with an odd significand and d = 2^(exponent(h) + 1), so that h + d is a tie in the next binade;
// 5: h far below d (d's own significand survives the plain step or loses bits to it).
static void draw_axis(std::mt19937_64& r, std::uniform_real_distribution<double>& U, int kind, float& h, float& d) {
    const int e = (int)(r() % 8) - 6;  // 2^-6 .. 2^1
    switch (kind) {
        case 0:
            h = (float)std::exp(std::log(1e-3) + U(r) * (std::log(8.0) - std::log(1e-3)));
            d = (r() & 1) ? h * (float)(U(r) * 0.05) : h * (float)std::ldexp(1.0, -(int)(1 + r() % 26));
            break;
        case 1:
            d = (float)std::ldexp(1.0 + U(r), e);
            h = d * (float)(1e-4 + U(r) * 0.9999);
            break;
        case 2:
            d = (float)std::ldexp(1.0 + U(r), e);
            h = (float)std::ldexp(1.0 + U(r), e);
            break;
        case 3:
            h = std::nextafter((float)std::ldexp(1.0, e), 0.f);
            d = (float)std::ldexp(1.0, e + (int)(r() % 3)) * (float)(1.0 + (r() % 3 ? U(r) : 0.0));
            break;
        case 4: {
            uint32_t hb = fbits((float)std::ldexp(1.0 + U(r), e)) | 1u;
            h = bitsf(hb);
            d = (float)std::ldexp(1.0, e + 1);
            break;
        }
        default:
            d = (float)std::ldexp(1.0 + U(r), e);
            h = d * (float)std::ldexp(1.0 + U(r), -(int)(1 + r() % 30));
            break;
    }
}

// Part 1 (and the boxes of part 4).  Returns the number of failures.
static long box_check(long iters) {
    std::mt19937_64 r(777);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    long bad = 0, taken = 0, whole = 0, whole_off = 0, grown = 0, byimm[4] = {0, 0, 0, 0};
    for (long i = 0; i < iters; ++i) {
        Walk w{};
        const uint32_t m = (i & 3) == 0 ? 15u : (i & 3) == 1 ? 63u : (i & 3) == 2 ? 255u : 1023u;
        uint32_t lo[3], hi[3];
        uint32_t* C3[3] = {&w.X, &w.Y, &w.Z};
        float* H3[3] = {&w.tx, &w.ty, &w.tz};
        float* D3[3] = {&w.dx, &w.dy, &w.dz};
        int32_t* S3[3] = {&w.sx, &w.sy, &w.sz};
        // one, two or all three axes immature, which ones at random
        const int nimm = 1 + (int)(i % 3), first = (int)(r() % 3);
        float tmin = 1e30f;
        int imm = 0;
        for (int k = 0; k < 3; ++k) {
            lo[k] = (uint32_t)(r() % 4) * (m + 1);
            hi[k] = lo[k] + m;
            *C3[k] = lo[k] + (uint32_t)(r() % (m + 1));
            *S3[k] = (r() & 1) ? 1 : -1;
            const bool immature = (k + 3 - first) % 3 < nimm;
            draw_axis(r, U, immature ? 1 + (int)(r() % 5) : 0, *H3[k], *D3[k]);
            uint32_t sb, sc, se;
            imm += seg_params_nb(*H3[k], *D3[k], sb, sc, se) ? 0 : 1;
            tmin = *H3[k] < tmin ? *H3[k] : tmin;
        }
        byimm[imm]++;
        w.t = tmin * (float)U(r);
        const float hmax = w.tx > w.ty ? (w.tx > w.tz ? w.tx : w.tz) : (w.ty > w.tz ? w.ty : w.tz);
        const int bk = (int)(r() % 4);
        const float bound = bk == 0 ? 1e34f : bk == 1 ? INFINITY : (float)(tmin + U(r) * (hmax * 4 - tmin));
        // without the bit: both forms, fed to the checksum
        Walk o1 = w, o0 = w;
        uint32_t lo_o[3] = {lo[0], lo[1], lo[2]}, hi_o[3] = {hi[0], hi[1], hi[2]}, lo_p[3] = {lo[0], lo[1], lo[2]}, hi_p[3] = {hi[0], hi[1], hi[2]};
        uint32_t co1 = 7, co0 = 7;
        const int ro1 = skip_box_lean<true>(o1, lo_o, hi_o, bound, co1);
        const int ro0 = skip_box_lean<false>(o0, lo_p, hi_p, bound, co0);
        feed((uint64_t)ro1), feed(co1), feed((uint64_t)ro0), feed(co0);
        for (int k = 0; k < 3; ++k) feed(lo_o[k]), feed(hi_o[k]), feed(lo_p[k]), feed(hi_p[k]);
        if (ro1 == 0) feed_walk(o1);
        if (ro0 == 0) feed_walk(o0);
#ifndef SKIP_PREFIX_PARENT
        Walk a1 = w, a0 = w, b = w;
        uint32_t lo1[3] = {lo[0], lo[1], lo[2]}, hi1[3] = {hi[0], hi[1], hi[2]}, lo0[3] = {lo[0], lo[1], lo[2]}, hi0[3] = {hi[0], hi[1], hi[2]};
        uint32_t c1 = 7, c0 = 7, cb = 7;
        const int r1 = skip_box_lean<true, 0, true>(a1, lo1, hi1, bound, c1);
        const int r0 = skip_box_lean<false, 0, true>(a0, lo0, hi0, bound, c0);
        if (r0 != r1 || c0 != c1 || memcmp(lo0, lo1, sizeof lo0) || memcmp(hi0, hi1, sizeof hi0) || (r0 == 0 && memcmp(&a0, &a1, sizeof(Walk)))) {
            if (bad < 10) printf("box %ld: the two forms differ, r %d/%d cells %u/%u\n", i, r0, r1, c0, c1);
            ++bad;
        }
        if ((r1 == 2) != (ro1 == 2)) { ++bad; continue; }
        if (r1 == 2) continue;
        ++taken;
        bool clipped = false, clipped_off = false, smaller = false, larger = false;
        for (int k = 0; k < 3; ++k) {
            clipped |= lo1[k] != lo[k] || hi1[k] != hi[k];
            clipped_off |= lo_o[k] != lo[k] || hi_o[k] != hi[k];
            smaller |= lo1[k] > lo_o[k] || hi1[k] < hi_o[k];  // never a smaller box than without the bit
            larger |= lo1[k] < lo_o[k] || hi1[k] > hi_o[k];
        }
        whole += !clipped, whole_off += !clipped_off, grown += larger;
        if (smaller) {
            if (bad < 10) printf("box %ld: smaller with the bit\n", i);
            ++bad;
        }
        const int rb = skip_box(b, lo1, hi1, bound, cb);
        if (!(r1 == rb && c1 == cb && (r1 == 1 || !memcmp(&a1, &b, sizeof(Walk))))) {
            if (bad < 10)
                printf("box %ld mismatch r %d/%d cells %u/%u t %a/%a\n  in: X %u %u %u s %d %d %d lo %u %u %u hi %u %u %u t %a h %a %a %a d %a %a %a bound %a\n"
                       "  out lean: h %a %a %a XYZ %u %u %u | ref: h %a %a %a XYZ %u %u %u\n",
                       i, r1, rb, c1, cb, a1.t, b.t, w.X, w.Y, w.Z, w.sx, w.sy, w.sz, lo1[0], lo1[1], lo1[2], hi1[0], hi1[1], hi1[2], w.t, w.tx,
                       w.ty, w.tz, w.dx, w.dy, w.dz, bound, a1.tx, a1.ty, a1.tz, a1.X, a1.Y, a1.Z, b.tx, b.ty, b.tz, b.X, b.Y, b.Z);
            ++bad;
        }
#endif
    }
    printf("boxes: %ld with 1 / %ld with 2 / %ld with 3 refused first segments; %ld taken, whole %ld (without the bit: %ld), larger than without %ld, bad=%ld\n",
           byimm[1], byimm[2], byimm[3], taken, whole, whole_off, grown, bad);
#ifndef SKIP_PREFIX_PARENT
    const bool spread = byimm[1] > 0 && byimm[2] > 0 && byimm[3] > 0 && grown > 0;
    if (!spread) printf("box spread missing\n");
    return bad + !spread;
#else
    return bad;
#endif
}

int main(int argc, char** argv) {
    _mm_setcsr(_mm_getcsr() | 0x8040u);  // FTZ|DAZ like the device build
    const long rays = argc > 1 ? atol(argv[1]) : 3000;
    const long bad_boxes = box_check(600000);
    printf("box bad=%ld\n", bad_boxes);
    const uint64_t box_sum = g_sum;
    std::vector<uint32_t> vs;
#ifndef SKIP_PREFIX_PARENT
    vs.push_back(kGatePre);
    for (uint32_t G = 1; G <= 3; ++G)
        for (uint32_t f = 0; f <= 2; ++f) vs.push_back(kGatePre | gate_word(G, f));
    for (uint32_t m = 1; m <= 4; ++m) vs.push_back(kGatePre | m << 5);
    vs.push_back(kGatePre | gate_word(1u, 0u) | 1u << 5);
#endif
    Tally rt;
    // 0: from outside; 1: inside (t = 0); 2: inside on a cell face or edge (t = 0, a head of 0 or a
    // whole tdelta); 3: inside with two or three equal components (tied tdeltas); 4: inside,
    // parallel to an axis (two infinite tdeltas)
    long kinds[5] = {0, 0, 0, 0, 0}, skips[5] = {0, 0, 0, 0, 0}, reached[5] = {0, 0, 0, 0, 0};
    for (uint32_t n : {64u, 128u}) {
        const World W = make_world(n, 31 * n + 5);
        std::mt19937_64 r(n * 17 + 3);
        std::uniform_real_distribution<float> U(0.f, 1.f);
        for (long i = 0; i < rays; ++i) {
            float O[3], D[3];
            const int rk = (int)(i % 5);
            for (int k = 0; k < 3; ++k) {
                O[k] = rk == 0 ? -0.6f + 2.2f * U(r) : U(r);
                D[k] = 0.05f + 0.9f * U(r) - O[k];
            }
            if (rk != 0) O[1] = 0.3f + 0.7f * U(r);  // mostly above the roofs: open space to skip
            const int ax = (int)(r() % 3);
            if (rk == 2) {
                O[ax] = (float)(1 + r() % (n - 1)) / (float)n;
                if (i % 10 == 2) O[(ax + 1) % 3] = (float)(1 + r() % (n - 1)) / (float)n;  // on a cell edge
            }
            if (rk == 3) {
                D[(ax + 1) % 3] = (r() & 1) ? D[ax] : -D[ax];
                if (i % 10 == 3) D[(ax + 2) % 3] = (r() & 1) ? D[ax] : -D[ax];  // all three tied
            }
            if (rk == 4) {
                for (int k = 0; k < 3; ++k)
                    if (k != ax) D[k] = 0.0f;
                if (D[ax] == 0.0f) D[ax] = 1.0f;
            }
            const float len = std::sqrt(D[0] * D[0] + D[1] * D[1] + D[2] * D[2]);
            if (!(len > 0)) continue;
            for (int k = 0; k < 3; ++k) D[k] = D[k] * (1.0f / len);
            Walk s;
            if (!setup(n, O, D, s)) continue;
            const float bound = (i % 3 == 0) ? 1e34f : 0.2f + 2.0f * U(r);
            ++kinds[rk];
            check_walk(W, s, bound, vs, rt, rk, i, skips, reached);
        }
    }
    printf("variants=%zu rays=%ld (outside %ld inside %ld face %ld tied %ld parallel %ld) hits=%ld cells=%llu ray bad=%ld\n", vs.size(), rt.total,
           kinds[0], kinds[1], kinds[2], kinds[3], kinds[4], rt.hits, (unsigned long long)rt.cells, rt.bad);
    printf("box checksum %#llx walk checksum %#llx\n", (unsigned long long)box_sum, (unsigned long long)g_sum);
    int fail = (bad_boxes || rt.bad) ? 1 : 0;
#ifndef SKIP_PREFIX_PARENT
    const char* names[5] = {"outside", "inside", "face", "tied", "parallel"};
    for (int k = 0; k < 5; ++k) {
        printf("%s: %ld skips, %ld past an axis clipped to zero without the bit\n", names[k], skips[k], reached[k]);
        if (k > 0 && reached[k] == 0) printf("no skip of the t = 0 class %s took the plain step\n", names[k]), fail = 1;
    }
    if (rays == 3000 && (box_sum != kBoxSumOff || g_sum != kWalkSumOff)) printf("bit off: results differ from the tier before the bit\n"), fail = 1;
    const bool spread = rt.hits > 0 && kinds[0] > 0 && kinds[1] > 0 && kinds[2] > 0 && kinds[3] > 0 && kinds[4] > 0;
    if (!spread) printf("input spread missing\n"), fail = 1;
#endif
    return fail;
}
