// Host check of the steps every host unit shares (csrc/ndt_geom.h): pack_cloud4 against the literal loop the units used
// to spell out, xyzi_layout_ok on the layouts tests/test_gpu_front_end_edges.py accepts and rejects, and grid_for around
// its two clamps.  Every record buffer is allocated at exactly n * stride bytes, so that a sanitizer build sees a read
// past the last record (intensity_offset 7 of a 32-byte record reads its last four bytes).
// Prints "mismatched: 0" when every value agrees.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>
#include "../../xchu_slam_amd/csrc/ndt_geom.h"

using namespace ndt::host;

static long long bad = 0;

static void expect(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (ok) return;
    ++bad;
    std::printf("FAIL %s (%lld, %lld)\n", what, a, b);
}

// n records of stride bytes holding distinct floats; intensity_offset < 0: w = 1
static void pack_case(size_t n, size_t stride, int intensity_offset) {
    const size_t fpr = stride / sizeof(float);
    std::unique_ptr<float[]> rec(new float[n * fpr]);  // exactly the records, no slack behind them
    for (size_t k = 0; k < n * fpr; ++k) rec[k] = 0.25f * (float)k - 3.0f;
    std::vector<float> want(4 * n);
    for (size_t i = 0; i < n; ++i) {
        const float* f = rec.get() + i * fpr;
        want[4 * i] = f[0];
        want[4 * i + 1] = f[1];
        want[4 * i + 2] = f[2];
        want[4 * i + 3] = intensity_offset < 0 ? 1.0f : f[intensity_offset];
    }
    const std::vector<float> got = pack_cloud4(rec.get(), n, stride, intensity_offset);
    expect(got.size() == want.size(), "pack size", (long long)got.size(), (long long)want.size());
    expect(got.size() == want.size() && (n == 0 || std::memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0), "pack bytes",
           (long long)stride, intensity_offset);
}

int main() {
    for (size_t n : {(size_t)0, (size_t)1, (size_t)5, (size_t)1000}) {
        pack_case(n, 12, -1);
        pack_case(n, 16, 3);
        pack_case(n, 32, 4);
        pack_case(n, 32, 7);
    }
    expect(pack_cloud4(nullptr, 0, 16, 3).empty(), "pack of no records");

    const int reject[4][2] = {{2, 32}, {3, 12}, {8, 32}, {4, 16}}, accept[3][2] = {{3, 16}, {4, 32}, {7, 32}};
    for (const auto& r : reject) expect(!xyzi_layout_ok((size_t)r[1], r[0]), "layout rejected", r[0], r[1]);
    for (const auto& a : accept) expect(xyzi_layout_ok((size_t)a[1], a[0]), "layout accepted", a[0], a[1]);

    const int shapes[5][2] = {{256, 2048}, {1024, 512}, {16, 16384}, {1, 7}, {4, 1}};  // per, cap
    for (const auto& s : shapes) {
        const long long per = s[0], cap = s[1];
        const long long ns[6] = {0, 1, per, per + 1, cap * per, cap * per + 1};
        const long long want[6] = {1, 1, 1, cap >= 2 ? 2 : 1, cap, cap};
        for (int k = 0; k < 6; ++k) expect(grid_for(ns[k], per, (int)cap) == want[k], "grid_for", ns[k], grid_for(ns[k], per, (int)cap));
    }
    expect(grid_for(0x7fffffffLL, 1, 0x7fffffff) == 0x7fffffff, "grid_for at INT_MAX");
    expect(pass_blocks(256 * 2048 + 1) == 2048 && pass_blocks(257) == 2 && pass_blocks(0) == 1, "pass_blocks");
    std::printf("mismatched: %lld\n", bad);
    return bad ? 1 : 0;
}
