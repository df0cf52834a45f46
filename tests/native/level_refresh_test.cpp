// The region-local level refresh (vpx_skip.hpp refresh_masks_host / refresh_levels_host) against
// the full host builders: after every edit l1, l2, the 8 octant planes and the 24 axis planes
// must be byte-equal to a rebuild from the edited cells.
// Worlds of side 37, 50 and 64: 1 % noise, a street canyon, a solid block (edited at its
// surface) and a near-empty grid; 10 random box set / erase edits each, applied one after the
// other to the refreshed levels (120 in all), then one edit of several boxes at once.  Last, a
// one-brick edit inside the 64^3 canyon must recompute strictly less than everything.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I raytracer-voxpopuli_amd/csrc tests/native/level_refresh_test.cpp
// and again with -DVPX_WID_CAP=3u: the cap of the widths, which no grid this small reaches at 255.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "vpx_skip.hpp"

using namespace vpx::skip;

struct Levels {
    std::vector<uint64_t> l1, l2;
    std::vector<uint8_t> dfp;
    std::vector<uint32_t> dfw;
};

static Levels full_build(const std::vector<uint8_t>& cells, uint32_t n) {
    const uint32_t nb1 = (n + 3) / 4, nb2 = (nb1 + 3) / 4, nb3 = (nb2 + 3) / 4;
    const size_t plane = 64ull * nb2 * nb2 * nb2;
    Levels v;
    v.l1.assign(plane, 0);
    v.l2.assign((size_t)nb3 * nb3 * nb3 * 64, 0);
    build_masks_host(cells.data(), n, v.l1.data(), v.l2.data());
    v.dfp.assign(8 * plane, 0);
    build_planes_host(v.l1.data(), v.l2.data(), n, v.dfp.data());
    v.dfw.assign(24 * plane, 0);
    build_wide_planes_host(v.dfp.data(), n, v.dfw.data());
    return v;
}

// kind 0: 1 % noise; 1: street canyon; 2: solid block in the middle; 3: one solid cell
static std::vector<uint8_t> make_cells(int kind, uint32_t n, uint64_t seed) {
    std::vector<uint8_t> c((size_t)n * n * n, 255);
    std::mt19937_64 r(seed);
    auto at = [&](uint32_t x, uint32_t y, uint32_t z) -> uint8_t& { return c[x + (size_t)y * n + (size_t)z * n * n]; };
    if (kind == 0) {
        for (auto& v : c)
            if (r() % 100 == 0) v = 3;
    } else if (kind == 1) {
        const uint32_t a = 26 * n / 64, b = 37 * n / 64, top = 41 * n / 64;
        for (uint32_t z = 0; z < n; ++z)
            for (uint32_t x = 0; x < n; ++x) {
                at(x, 0, z) = 1;
                if ((x == a || x == b) && !(z >= 30 * n / 64 && z < 36 * n / 64))
                    for (uint32_t y = 1; y < top; ++y) at(x, y, z) = 5;
            }
        for (uint32_t y = 1; y < 20 * n / 64; ++y) at(31 * n / 64, y, 50 * n / 64) = 2;
    } else if (kind == 2) {
        for (uint32_t z = n / 4; z < 3 * n / 4; ++z)
            for (uint32_t y = n / 4; y < 3 * n / 4; ++y)
                for (uint32_t x = n / 4; x < 3 * n / 4; ++x) at(x, y, z) = 4;
    } else {
        at(n / 3, n / 2, n - 2) = 3;
    }
    return c;
}

struct CellBox {
    uint32_t lo[3], hi[3];  // inclusive
    uint8_t value;
};

static CellBox random_box(std::mt19937_64& r, int kind, uint32_t n) {
    CellBox b;
    for (int q = 0; q < 3; ++q) {
        const uint32_t size = 1 + r() % 12;
        uint32_t c = (uint32_t)(r() % n);
        if (kind == 2 && q == (int)(r() % 3)) c = (r() & 1) ? n / 4 : 3 * n / 4 - 1;  // at a face of the block
        b.lo[q] = c;
        b.hi[q] = c + size - 1 < n ? c + size - 1 : n - 1;
    }
    b.value = (r() & 1) ? 255 : (uint8_t)(1 + r() % 8);
    return b;
}

static void write_box(std::vector<uint8_t>& c, uint32_t n, const CellBox& b) {
    for (uint32_t z = b.lo[2]; z <= b.hi[2]; ++z)
        for (uint32_t y = b.lo[1]; y <= b.hi[1]; ++y)
            for (uint32_t x = b.lo[0]; x <= b.hi[0]; ++x) c[x + (size_t)y * n + (size_t)z * n * n] = b.value;
}

struct Share {
    RefreshCount cnt;
    uint32_t flipped = 0;
};

// Apply the boxes, refresh `lv` locally, compare with a full rebuild; returns the differing words.
static long edit_and_check(std::vector<uint8_t>& cells, uint32_t n, Levels& lv, const std::vector<CellBox>& boxes, Share& sh,
                           const char* what) {
    Box3 T = box_none();
    for (const CellBox& b : boxes) {
        write_box(cells, n, b);
        const uint32_t lo[3] = {b.lo[0] >> 2, b.lo[1] >> 2, b.lo[2] >> 2}, hi[3] = {b.hi[0] >> 2, b.hi[1] >> 2, b.hi[2] >> 2};
        box_add(T, lo);
        box_add(T, hi);
    }
    const Box3 E = refresh_masks_host(cells.data(), n, T, lv.l1.data(), lv.l2.data(), &sh.flipped);
    const Levels before = sh.flipped ? Levels{} : lv;
    sh.cnt = refresh_levels_host(cells.data(), n, E, lv.l1.data(), lv.l2.data(), lv.dfp.data(), lv.dfw.data());
    const Levels want = full_build(cells, n);
    long bad = 0;
    for (size_t i = 0; i < want.l1.size(); ++i) bad += want.l1[i] != lv.l1[i];
    for (size_t i = 0; i < want.l2.size(); ++i) bad += want.l2[i] != lv.l2[i];
    for (size_t i = 0; i < want.dfp.size(); ++i) bad += want.dfp[i] != lv.dfp[i];
    for (size_t i = 0; i < want.dfw.size(); ++i) bad += want.dfw[i] != lv.dfw[i];
    if (!sh.flipped) {  // no brick flipped: no distance-field word may have moved
        bad += before.dfp != lv.dfp || before.dfw != lv.dfw;
        bad += sh.cnt.bytes + sh.cnt.halves + sh.cnt.widths != 0;
    }
    if (bad) printf("%s n=%u: %ld words differ from the full rebuild (flipped %u)\n", what, n, bad, sh.flipped);
    return bad;
}

int main() {
    static const uint32_t sizes[3] = {37, 50, 64};
    static const char* names[4] = {"noise", "canyon", "block", "sparse"};
    long bad = 0, edits = 0, flips = 0, noflips = 0;
    for (uint32_t n : sizes)
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<uint8_t> cells = make_cells(kind, n, 1000 + n + kind);
            Levels lv = full_build(cells, n);
            std::mt19937_64 r(n * 31 + kind);
            const uint32_t nb1 = (n + 3) / 4;
            const double all = (double)nb1 * nb1 * nb1;
            RefreshCount sum;
            for (int e = 0; e < 10; ++e) {
                Share sh;
                bad += edit_and_check(cells, n, lv, {random_box(r, kind, n)}, sh, names[kind]);
                ++edits, flips += sh.flipped != 0, noflips += sh.flipped == 0;
                sum.bytes += sh.cnt.bytes, sum.halves += sh.cnt.halves, sum.widths += sh.cnt.widths;
            }
            Share sh;  // several boxes in one refresh
            bad += edit_and_check(cells, n, lv, {random_box(r, kind, n), random_box(r, kind, n), random_box(r, kind, n), random_box(r, kind, n)},
                                  sh, "multi-box");
            printf("n=%u %-6s recomputed per edit: bytes %.1f %% halves %.1f %% widths %.1f %%\n", n, names[kind],
                   100.0 * sum.bytes / (10 * 8 * all), 100.0 * sum.halves / (10 * 24 * all), 100.0 * sum.widths / (10 * 24 * all));
        }
    // a one-brick edit inside the canyon: brick (8, 9, 6) between the walls, high above the street
    {
        const uint32_t n = 64, nb1 = 16;
        std::vector<uint8_t> cells = make_cells(1, n, 0);
        Levels lv = full_build(cells, n);
        Share sh;
        bad += edit_and_check(cells, n, lv, {CellBox{{32, 36, 24}, {35, 39, 27}, 1}}, sh, "one brick");
        const uint64_t all = (uint64_t)nb1 * nb1 * nb1;
        printf("one brick: flipped %u, recomputed bytes %llu / %llu halves %llu / %llu widths %llu / %llu\n", sh.flipped,
               (unsigned long long)sh.cnt.bytes, (unsigned long long)(8 * all), (unsigned long long)sh.cnt.halves,
               (unsigned long long)(24 * all), (unsigned long long)sh.cnt.widths, (unsigned long long)(24 * all));
        const bool local = sh.flipped == 1 && sh.cnt.bytes > 0 && sh.cnt.bytes < 8 * all && sh.cnt.halves > 0 && sh.cnt.halves < 24 * all &&
                           sh.cnt.widths > 0 && sh.cnt.widths < 24 * all;
        if (!local) printf("the refresh is not local\n"), ++bad;
    }
    printf("cap=%u edits=%ld (flipping %ld, not flipping %ld) refresh bad=%ld\n", (unsigned)VPX_WID_CAP, edits, flips, noflips, bad);
    if (!flips || !noflips) printf("input spread missing\n");
    return (bad || !flips || !noflips) ? 1 : 0;
}
