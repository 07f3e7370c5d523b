// Host sweep of the derivative passes' launch geometry (xchu_slam_amd/csrc/ndt_geom.h: the functions host_align.hip
// launches through and ndt_pass_geometry reports from) and of the two-level hand-off's grouping (ndt_types.h
// group_size / partial_stride, as pass_handoff uses them).  Prints "mismatched: 0" when every property holds.
#include <cstdio>
#include <set>
#include <vector>
#include "../../xchu_slam_amd/csrc/ndt_geom.h"

using namespace ndt;
using namespace ndt::host;

static long long bad = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (bad < 20) {                                  \
                std::printf("FAIL %s: ", #cond);             \
                std::printf(__VA_ARGS__);                    \
                std::printf("\n");                           \
            }                                                \
            ++bad;                                           \
        }                                                    \
    } while (0)

static constexpr int kMaxN = 1 << 23;

// every value within +-2 of each threshold of the geometry, plus a stride in between
static std::vector<int> sweep_sizes(int n_cu) {
    std::set<int> s;
    auto around = [&](long long t) {
        for (long long d = -2; d <= 2; ++d)
            if (t + d >= 1 && t + d <= kMaxN + 2) s.insert((int)(t + d));
    };
    around(1);
    around(4096);
    around((long long)n_cu * kLeadBlock1);
    around(262144);
    around(393216);
    around(1048576);
    for (long long p = 1; p <= kMaxN; p *= 2) around(p);
    for (long long n = 1; n <= kMaxN; n += 4099) s.insert((int)n);
    return std::vector<int>(s.begin(), s.end());
}

static void check_geom_points() {
    int prev = 0;
    for (int n = 1; n <= kMaxN + 2; n += (n < (1 << 18) ? 1 : 61)) {
        const int g = geom_points(n);
        CHECK(g >= n, "n %d -> %d", n, g);
        CHECK(g >= prev, "n %d -> %d after %d", n, g, prev);
        // a multiple of 256 up to 4096 points and wherever 1/64 of the power of two is one (n >= 16384); the 64- and
        // 128-point steps of 4097..16383 points are whole waves (nothing downstream needs more: every kernel masks by n)
        int p = 1;
        while (p * 2 <= n) p *= 2;
        const int step = n <= 4096 ? 256 : p / 64;
        CHECK(g % step == 0 && g % 64 == 0, "n %d -> %d (step %d)", n, g, step);
        if (n <= 4096 || n >= 16384) CHECK(g % 256 == 0, "n %d -> %d", n, g);
        CHECK((long long)g * 64 <= (long long)n * 65 || n <= 4096, "n %d -> %d: more than 1/64 over", n, g);
        prev = g;
    }
}

static void check_pass(const PassShape& s, int which) {
    int o[8];
    CHECK(describe_pass(s, which, o), "which %d", which);
    const int n = geom_points(s.N);
    const int nb = o[0], block = o[1], ppb = o[2], ppt = o[3], one = o[4], tiles = o[5];
    const char* fmt = "n_cu %d N %d M %d search %d ppt %d which %d: nb %d block %d ppb %d ppt %d one %d tiles %d";
#define ARGS s.n_cu, s.N, s.M, s.search, s.ppt, which, nb, block, ppb, ppt, one, tiles
    CHECK(nb >= 1 && ppb >= 1 && tiles >= 1, fmt, ARGS);
    CHECK(block == pass_block(s.search, which == 1, which == 1 && one), fmt, ARGS);
    CHECK(block % 64 == 0 && block <= 1024, fmt, ARGS);
    CHECK(ppt == 1 || ppt == 2, fmt, ARGS);
    // a tile's points have a thread slot each (thread k holds tile-local points k, k + block)
    CHECK(ppb <= block * ppt, fmt, ARGS);
    // the workgroups' tiles cover the bucket, with no tile to spare
    CHECK((long long)nb * tiles * ppb >= n, fmt, ARGS);
    CHECK((long long)nb * (tiles - 1) * ppb < n, fmt, ARGS);
    if (one) CHECK(tiles == 1 && ppt == 1, fmt, ARGS);
    if (which == 2) {
        CHECK(nb == std::min(2048, (n + 255) / 256) && block == 256 && ppb == 256 && ppt == 1 && !one, fmt, ARGS);
    } else {
        const PassGeom g = direct_geom(s, which == 1);
        CHECK(g.nb == nb && g.ppb == ppb && g.block == block, fmt, ARGS);
    }
    if (which == 0) {
        // two points per thread: the packed pair word holds a 22-bit cloud index
        const long long max_cloud = (long long)s.M / std::max(1, s.min_points_per_voxel) + 1;
        if (ppt == 2) CHECK(max_cloud < (1ll << 22) && s.ppt == 2 && s.search != S_DIRECT26 && tiles >= 2, fmt, ARGS);
        if (s.search == S_DIRECT26) CHECK(ppt == 1 && !one && block == kBlock, fmt, ARGS);
        CHECK(one == (grid_one_tile(s) ? 1 : 0), fmt, ARGS);
        if (grid_one_tile(s)) CHECK(nb == (n + 255) / 256 && ppb == 256 && s.ppt == 3, fmt, ARGS);
    }
    if (which == 1) CHECK(nb <= s.n_cu && o[6] == 0 && o[7] == 0, fmt, ARGS);
    // the hand-off the grid takes
    if (which != 1) {
        if (nb > kTwoLevelMinBlocks) {
            CHECK(o[7] == group_size(nb) && o[6] == (nb + o[7] - 1) / o[7], fmt, ARGS);
        } else {
            CHECK(o[6] == 0 && o[7] == 0, fmt, ARGS);
        }
    }
#undef ARGS
}

// pass_handoff's two-level grouping of an nb-workgroup grid
static void check_groups() {
    for (int nb = kTwoLevelMinBlocks + 1; nb <= kMaxN / 256; ++nb) {
        const int G = group_size(nb), ng = (nb + G - 1) / G, ps = partial_stride(nb);
        // group g's columns start at partials + g * G and are loaded as 16-byte pairs (reduce_partials_block)
        CHECK(G % 2 == 0, "nb %d: group size %d", nb, G);
        CHECK(ps % 2 == 0 && ps >= nb, "nb %d: stride %d", nb, ps);
        CHECK(G >= 1 && ng >= 1 && ng <= kMaxGroups, "nb %d: %d groups of %d", nb, ng, G);
        const int last = nb - (ng - 1) * G;
        CHECK(last >= 1 && last <= G, "nb %d: last group holds %d of %d", nb, last, G);
        // a closer's pair loads stay inside its rows (the pair past an odd last column is the row's padding)
        CHECK((ng - 1) * G + ((last + 1) & ~1) <= ps, "nb %d: last group's pairs leave the row", nb);
        // the group partials [kNumAcc][kMaxGroups] follow the [kNumAcc][ps] workgroup partials in the buffer
        // ensure_align_buffers sizes as kNumAcc * (partial_stride(nb) + kMaxGroups)
        const long long cap = (long long)kNumAcc * (ps + kMaxGroups);
        const long long top = (long long)kNumAcc * ps + (long long)(kNumAcc - 1) * kMaxGroups + (ng - 1);
        CHECK(top < cap, "nb %d: group partials end at %lld of %lld", nb, top, cap);
        if (nb <= 4096) CHECK(G == 64, "nb %d: group size %d", nb, G);
    }
}

// the geometries tests/test_gpu_pass_geometry.py names, on 256 CUs
static void check_pins() {
    struct Pin {
        int N, search, ppt, which, nb, ppb, kppt, one, tiles, ng, G;
    };
    const Pin pins[] = {
        {200000, S_DIRECT7, 3, 0, 784, 256, 1, 1, 1, 0, 0},    {200000, S_DIRECT1, 3, 0, 784, 256, 1, 1, 1, 0, 0},
        {266240, S_DIRECT7, 3, 0, 1040, 256, 1, 1, 1, 17, 64}, {262145, S_DIRECT7, 3, 0, 1040, 256, 1, 1, 1, 17, 64},
        {266240, S_KDTREE, 2, 2, 1040, 256, 1, 0, 1, 17, 64},  {394000, S_DIRECT7, 1, 0, 512, 194, 1, 0, 4, 0, 0},
        {394000, S_DIRECT7, 2, 0, 512, 388, 2, 0, 2, 0, 0},    {394000, S_DIRECT7, 3, 0, 1552, 256, 1, 1, 1, 25, 64},
        {394000, S_DIRECT1, 2, 0, 512, 388, 2, 0, 2, 0, 0},    {540000, S_KDTREE, 2, 2, 2048, 256, 1, 0, 2, 32, 64},
        {1050000, S_DIRECT7, 3, 0, 4160, 256, 1, 1, 1, 64, 66},
    };
    for (const Pin& p : pins) {
        const PassShape s{256, p.N, 112890, p.search, 6, p.ppt};
        int o[8];
        describe_pass(s, p.which, o);
        CHECK(o[0] == p.nb && o[2] == p.ppb && o[3] == p.kppt && o[4] == p.one && o[5] == p.tiles && o[6] == p.ng && o[7] == p.G,
              "N %d search %d ppt %d: nb %d ppb %d ppt %d one %d tiles %d groups %d of %d", p.N, p.search, p.ppt, o[0], o[2], o[3], o[4],
              o[5], o[6], o[7]);
    }
}

int main() {
    check_geom_points();
    long long shapes = 0;
    const int cus[] = {1, 8, 104, 256, 304};
    const int searches[] = {S_DIRECT7, S_DIRECT26, S_DIRECT1};
    // targets around the two-points-per-thread kernel's 2^22 cloud-index limit (min_points 6) beside an ordinary one
    const int targets[] = {112890, 6 * ((1 << 22) - 2), 6 * ((1 << 22) - 1), 6 * (1 << 22), 30000000};
    for (int n_cu : cus) {
        const std::vector<int> sizes = sweep_sizes(n_cu);
        for (int search : searches)
            for (int ppt = 1; ppt <= 3; ++ppt)
                for (int M : targets)
                    for (int N : sizes) {
                        const PassShape s{n_cu, N, M, search, 6, ppt};
                        for (int lead = 0; lead <= 1; ++lead) check_pass(s, lead);
                        ++shapes;
                    }
        for (int N : sizes) check_pass(PassShape{n_cu, N, 112890, S_KDTREE, 6, 2}, 2);
    }
    check_groups();
    check_pins();
    std::printf("shapes: %lld\nmismatched: %lld\n", shapes, bad);
    return bad ? 1 : 0;
}
