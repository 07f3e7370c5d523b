// Host check of the pass kernels' in-wave reduce-scatter (csrc/ndt_rstree.h: rs22_reduce, 22 values in 23 exchanges)
// against an emulation of the schedule it replaced (the 22 values padded to 32 slots, rs_step<16> .. rs_step<1> of
// csrc/ndt_device.h, which block_reduce_store still uses): the wave total of every value, in both half-waves, bit for bit.
// A wave is 64 lanes x 22 doubles; lanes 0-31 and 32-63 carry different value sets and never meet (the lane bit 32 step
// ran before).  The partner of a lane is lane ^ 16, ^ 8, ^ 7 (row_half_mirror), ^ 2, ^ 1, as on the device.
// NaN results compare as NaN (a sum of two NaNs takes its payload from one operand, and which one is the hardware's
// choice, not the schedule's); everything else, signed zeros and infinities included, compares by bits.
// Also checked: every half-wave's 22 values are reported by exactly one lane each (rs22_reports / rs22_value).  The run
// fails unless both half-waves and all 22 values were compared.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>
#include "../../xchu_slam_amd/csrc/ndt_rstree.h"

namespace {

using ndt::kRsValues;
struct Wave {
    double x[64];
};

int partner(int lane, int m) { return m == 4 ? (lane ^ 7) : (lane ^ m); }

// the device's exchanges on a whole wave
struct HostOps {
    using T = Wave;
    Wave swap16(const Wave& A, const Wave& B) const {
        Wave r;
        // v_permlane16_swap + add: lanes of even rows A[own] + A[partner], lanes of odd rows B[partner] + B[own]
        for (int l = 0; l < 64; ++l) r.x[l] = (l & 16) ? B.x[l ^ 16] + B.x[l] : A.x[l] + A.x[l ^ 16];
        return r;
    }
    template <int M>
    Wave xchg(const Wave& A, const Wave& B) const {
        Wave r;
        for (int l = 0; l < 64; ++l) {
            const int p = partner(l, M);
            // the partner sends what it does not keep: a lane with bit M clear sends B, one with it set sends A
            const double keep = (l & M) ? B.x[l] : A.x[l];
            const double recv = (p & M) ? A.x[p] : B.x[p];
            // (l & M) != (p & M) for every partner, so recv is the partner's copy of what this lane keeps
            r.x[l] = keep + recv;
        }
        return r;
    }
    template <int M>
    Wave both(const Wave& A) const {
        Wave r;
        for (int l = 0; l < 64; ++l) r.x[l] = A.x[l] + A.x[partner(l, M)];
        return r;
    }
};

// The replaced schedule: 32 slots per lane (22 values, then zeros), rs_step<16>, <8>, <4>, <2>, <1>; lane l ends with
// value l & 31 in slot 0
void old_reduce(const Wave (&v)[kRsValues], double (&out)[64]) {
    static double a[64][32];
    for (int l = 0; l < 64; ++l)
        for (int s = 0; s < 32; ++s) a[l][s] = s < kRsValues ? v[s].x[l] : 0.0;
    {
        double n[64][16];
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 16; ++i) n[l][i] = (l & 16) ? a[l ^ 16][i + 16] + a[l][i + 16] : a[l][i] + a[l ^ 16][i];
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < 16; ++i) a[l][i] = n[l][i];
    }
    for (int m = 8; m >= 1; m >>= 1) {
        double n[64][8];
        for (int l = 0; l < 64; ++l) {
            const int p = partner(l, m);
            for (int i = 0; i < m; ++i) {
                const double keep = (l & m) ? a[l][i + m] : a[l][i];
                const double send_p = (p & m) ? a[p][i] : a[p][i + m];
                n[l][i] = keep + send_p;
            }
        }
        for (int l = 0; l < 64; ++l)
            for (int i = 0; i < m; ++i) a[l][i] = n[l][i];
    }
    for (int l = 0; l < 64; ++l) out[l] = a[l][0];
}

uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}
bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || bits(a) == bits(b); }

long long g_mismatched = 0, g_compared = 0;
bool g_seen[2][kRsValues];

void check_wave(const Wave (&v)[kRsValues]) {
    double want[64];
    old_reduce(v, want);
    const Wave got = ndt::rs22_reduce(HostOps{}, v);
    for (int l = 0; l < 64; ++l) {
        const int k = ndt::rs22_value(l & 31), half = l >> 5;
        // every lane that holds value k (the reporting one and its duplicate) against the old schedule's lane for k
        if (!same(got.x[l], want[half * 32 + k])) {
            if (g_mismatched < 10)
                std::printf("lane %d value %d half %d: %016llx vs %016llx\n", l, k, half, (unsigned long long)bits(got.x[l]),
                            (unsigned long long)bits(want[half * 32 + k]));
            ++g_mismatched;
        }
        ++g_compared;
        if (ndt::rs22_reports(l & 31)) g_seen[half][k] = true;
    }
}

double from_bits(uint64_t u) {
    double d;
    std::memcpy(&d, &u, 8);
    return d;
}

}  // namespace

int main() {
    // the map: 22 reporting lanes per half-wave, one per value
    int bad_map = 0;
    for (int half = 0; half < 2; ++half) {
        int count[kRsValues] = {};
        for (int l = 0; l < 32; ++l) {
            const int k = ndt::rs22_value(l);
            if (k < 0 || k >= kRsValues) { ++bad_map; continue; }
            if (ndt::rs22_reports(l)) ++count[k];
        }
        for (int k = 0; k < kRsValues; ++k) bad_map += count[k] != 1;
    }
    std::mt19937_64 rng(20240611);
    static Wave v[kRsValues];
    auto fill = [&](auto&& gen) {
        for (int k = 0; k < kRsValues; ++k)
            for (int l = 0; l < 64; ++l) v[k].x[l] = gen(k, l);
    };
    // 1. random sign, mantissa and exponent over the full finite range (sums overflow to infinities, cancel to NaN)
    auto any_finite = [&]() {
        uint64_t u = rng();
        const uint64_t e = (u >> 52) & 0x7ff;
        if (e == 0x7ff) u &= ~(1ull << 62);
        return from_bits(u);
    };
    for (int rep = 0; rep < 400; ++rep) {
        fill([&](int, int) { return any_finite(); });
        check_wave(v);
    }
    // 2. sums of like magnitude (every addition rounds): the pass's own regime
    std::uniform_real_distribution<double> u11(-1.0, 1.0);
    for (int rep = 0; rep < 400; ++rep) {
        fill([&](int k, int) { return u11(rng) * std::ldexp(1.0, 3 * k - 30); });
        check_wave(v);
    }
    // 3. +0.0 / -0.0 everywhere, then one non-zero, one -0.0 or one +0.0 at every (value, lane) among zeros of the other
    //    sign: -0.0 + +0.0 = +0.0 but -0.0 + -0.0 = -0.0, so an operand that meets a padding zero shows
    for (double z : {0.0, -0.0}) {
        fill([&](int, int) { return z; });
        check_wave(v);
        for (int k = 0; k < kRsValues; ++k)
            for (int l = 0; l < 64; ++l)
                for (double s : {-z, 1.5, -1.5}) {
                    fill([&](int, int) { return z; });
                    v[k].x[l] = s;
                    check_wave(v);
                }
    }
    // 4. infinities, NaNs and subnormals at every (value, lane) among random finite numbers, and mixed waves
    const double specials[] = {std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(),
                               std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::denorm_min(),
                               -std::numeric_limits<double>::denorm_min(), from_bits(0x000fffffffffffffull),
                               std::numeric_limits<double>::min(), std::numeric_limits<double>::max()};
    for (double s : specials)
        for (int k = 0; k < kRsValues; ++k)
            for (int l = 0; l < 64; l += 3) {
                fill([&](int, int) { return u11(rng) * 1e-300; });
                v[k].x[(l + k) & 63] = s;
                check_wave(v);
            }
    for (int rep = 0; rep < 200; ++rep) {
        fill([&](int, int) {
            const uint64_t r = rng();
            return (r & 7) == 0 ? specials[(r >> 3) % 8] : from_bits(rng() & 0x800fffffffffffffull);  // subnormals
        });
        check_wave(v);
    }
    int unseen = 0;
    for (int half = 0; half < 2; ++half)
        for (int k = 0; k < kRsValues; ++k) unseen += !g_seen[half][k];
    std::printf("waves x lanes compared: %lld\nmap errors: %d\nunseen (half, value): %d\nmismatched: %lld\n", g_compared, bad_map,
                unseen, g_mismatched);
    return (g_mismatched == 0 && bad_map == 0 && unseen == 0 && g_compared > 0) ? 0 : 1;
}
