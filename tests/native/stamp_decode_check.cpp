// The stamp decoder of csrc/ndt_stamps.h (accumulate_pass_stats) on synthetic stamp tables.  Every expected value is
// written down from the slot meanings: each phase gets its own tick count, so that a decoded phase is ticks * 1e-5 ms by
// construction.  Tables are exactly as large as their shape says (the program also runs under the host sanitizers).
//   g++ -O2 -std=c++17 stamp_decode_check.cpp && ./a.out      -> "mismatched: 0"
#include <cstdio>
#include <vector>
#include "../../xchu_slam_amd/csrc/ndt_stamps.h"

using namespace ndt;
using namespace ndt::host;
using u64 = unsigned long long;

static int g_bad = 0;
static void expect(const char* what, int idx, double got, double want) {
    if (got != want) {
        std::printf("MISMATCH %s[%d]: got %.17g want %.17g\n", what, idx, got, want);
        ++g_bad;
    }
}
static double ms(double ticks) { return ticks * 1e-5; }

// pass rows as k_align_init leaves them
static std::vector<u64> fresh_rows(int passes) {
    std::vector<u64> ts((size_t)passes * kTsStride, 0ull);
    for (int p = 0; p < passes; ++p) ts[(size_t)p * kTsStride + kTsEntry] = kTsUnstamped;
    return ts;
}
// a last-workgroup-tail pass: entry at t0, then the seven product phases
static void stamp_pass(std::vector<u64>& ts, int p, u64 t0, const int (&ph)[7]) {
    u64* t = &ts[(size_t)p * kTsStride];
    t[kTsEntry] = t0;
    t[kTsBodyEnd] = t[kTsEntry] + ph[0];
    t[kTsAcquired] = t[kTsBodyEnd] + ph[1];
    t[kTsReduced] = t[kTsAcquired] + ph[2];
    t[kTsStaged] = t[kTsReduced] + ph[3];
    t[kTsControl] = t[kTsStaged] + ph[4];
    t[kTsTables] = t[kTsControl] + ph[5];
    t[kTsEnd] = t[kTsTables] + ph[6];
}
// a leading-tail pass: its kernel stamps entry and end only
static void stamp_lead_pass(std::vector<u64>& ts, int p, u64 t0, int dur) {
    ts[(size_t)p * kTsStride + kTsEntry] = t0;
    ts[(size_t)p * kTsStride + kTsEnd] = t0 + dur;
}
static std::vector<PassRecordDev> records(std::initializer_list<long long> pairs) {
    std::vector<PassRecordDev> h;
    for (long long p : pairs) {
        PassRecordDev r = {};
        r.pairs = p;
        h.push_back(r);
    }
    return h;
}
// one workgroup row: body start `delay` ticks after t0, then the marks, the block reduction, the three tile sums
static void stamp_wg(std::vector<u64>& blk, BlkShape s, int pass, int wg, u64 t0, int delay, int reduce, int s_probe, int s_compact,
                     int s_pairs) {
    u64* e = &blk[blk_row_at(s.rows, pass, wg)];
    e[kWgBodyStart] = t0 + delay;
    e[kWgProbed] = e[kWgBodyStart] + 50;
    e[kWgCompacted] = e[kWgProbed] + 25;
    e[kWgPaired] = e[kWgCompacted] + 150;
    e[kWgBodyEnd] = e[kWgPaired] + reduce;
    e[kWgSumProbe] = s_probe;
    e[kWgSumCompact] = s_compact;
    e[kWgSumPairs] = s_pairs;
}
static void expect_zero_blk(const PassStats& ps, const char* what) {
    for (int q = 0; q < kWgPhases; ++q) expect(what, q, ps.body_sum[q], 0.0);
    for (int q = 0; q < kTailPhases; ++q) expect(what, 10 + q, ps.tail_sum[q], 0.0);
    expect(what, 100, ps.body_count, 0);
    expect(what, 101, ps.tail_count, 0);
}

static const int kPh[7] = {100, 10, 20, 5, 40, 15, 10};  // bodies, handoff, reduce, stage, control, tables, drain: 200 ticks

// 1. product stamps only
static void case_product() {
    auto ts = fresh_rows(1);
    stamp_pass(ts, 0, 1000, kPh);
    const auto hist = records({5000});
    const StampView v = {ts.data(), nullptr, kBlkShape, hist.data(), 1000, 4, false};
    PassStats ps;
    accumulate_pass_stats(v, 0, 1, ps);
    for (int q = 0; q < 7; ++q) expect("product phase", q, ps.phase_sum[q], ms(kPh[q]));
    expect("product phase_count", 0, ps.phase_count, 1);
    expect("product ms_sum", 0, ps.ms_sum, ms(200));
    expect("product count", 0, (double)ps.count, 1);
    expect("product bytes", 0, ps.bytes_sum, 16.0 * 1000 + 36.0 * 5000);
    expect_zero_blk(ps, "product blk");
}

// 2. a row never stamped, a row with end <= entry
static void case_untimed() {
    auto ts = fresh_rows(2);
    ts[1 * kTsStride + kTsEntry] = 500;
    ts[1 * kTsStride + kTsEnd] = 500;
    ts[1 * kTsStride + kTsBodyEnd] = 500;
    const auto hist = records({111, 222});
    const StampView v = {ts.data(), nullptr, kBlkShape, hist.data(), 1000, 4, false};
    PassStats ps;
    accumulate_pass_stats(v, 0, 2, ps);
    for (int q = 0; q < 7; ++q) expect("untimed phase", q, ps.phase_sum[q], 0.0);
    expect("untimed phase_count", 0, ps.phase_count, 0);
    expect("untimed ms_sum", 0, ps.ms_sum, 0.0);
    expect("untimed bytes", 0, ps.bytes_sum, 0.0);
    expect("untimed count", 0, (double)ps.count, 0);
    expect_zero_blk(ps, "untimed blk");
}

// 3. a leading-tail row: timed, no phases
static void case_lead_row() {
    auto ts = fresh_rows(1);
    stamp_lead_pass(ts, 0, 1000, 300);
    const auto hist = records({7});
    const StampView v = {ts.data(), nullptr, kBlkShape, hist.data(), 10, 4, true};
    PassStats ps;
    accumulate_pass_stats(v, 0, 1, ps);
    expect("lead row ms_sum", 0, ps.ms_sum, ms(300));
    expect("lead row count", 0, (double)ps.count, 1);
    expect("lead row bytes", 0, ps.bytes_sum, 16.0 * 10 + 36.0 * 7);
    expect("lead row phase_count", 0, ps.phase_count, 0);
    for (int q = 0; q < 7; ++q) expect("lead row phase", q, ps.phase_sum[q], 0.0);
}

// 4. workgroup means
static void case_wg_means() {
    const BlkShape s = {2, 6};  // four workgroup rows, the prologue row, the tail row
    std::vector<u64> blk(blk_words(s), 0ull);
    auto ts = fresh_rows(2);
    stamp_pass(ts, 0, 1000, kPh);
    stamp_pass(ts, 1, 3000, kPh);
    const auto hist = records({1, 2});
    // pass 0: entry delays 10 / 20 / 60 (mean 30), block reductions 30 / 60 / 90 (mean 60), tile sums with means 100 / 50 / 300
    stamp_wg(blk, s, 0, 0, 1000, 10, 30, 80, 40, 240);
    stamp_wg(blk, s, 0, 1, 1000, 20, 60, 100, 50, 300);
    stamp_wg(blk, s, 0, 2, 1000, 60, 90, 120, 60, 360);
    stamp_wg(blk, s, 0, 3, 1000, 5, 7, 999, 999, 999);
    blk[blk_row_at(s.rows, 0, 3) + kWgProbed] = 0;  // past the scan's points: never reached its first tile mark
    // pass 1: workgroup 1 out of order
    stamp_wg(blk, s, 1, 0, 3000, 10, 30, 80, 40, 240);
    stamp_wg(blk, s, 1, 1, 3000, 20, 60, 100, 50, 300);
    blk[blk_row_at(s.rows, 1, 1) + kWgCompacted] = blk[blk_row_at(s.rows, 1, 1) + kWgProbed] - 1;
    const StampView v = {ts.data(), blk.data(), s, hist.data(), 1000, 4, false};
    PassStats ps;
    accumulate_pass_stats(v, 0, 1, ps);
    const double want[5] = {30, 100, 50, 300, 60};
    for (int q = 0; q < 5; ++q) expect("wg mean", q, ps.body_sum[q], ms(want[q]));
    expect("wg body_count", 0, ps.body_count, 1);
    expect("wg tail_count (tail row unstamped)", 0, ps.tail_count, 0);
    PassStats ps1;
    accumulate_pass_stats(v, 1, 1, ps1);
    expect("wg out of order: count", 0, (double)ps1.count, 1);
    expect("wg out of order: phase_count", 0, ps1.phase_count, 1);
    expect_zero_blk(ps1, "wg out of order");
}

// 5. the last-workgroup tail
static void case_tail() {
    const BlkShape s = {1, 3};
    std::vector<u64> blk(blk_words(s), 0ull);
    auto ts = fresh_rows(1);
    stamp_pass(ts, 0, 1000, kPh);  // staged 1135, control 1175, tables 1190
    const auto hist = records({1});
    stamp_wg(blk, s, 0, 0, 1000, 10, 30, 80, 40, 240);
    // record 3, machine 7, solve_setup 4, solve 11, post_solve 15 (= control 40); sincos 6, rows 5, writeback 4 (= tables 15)
    u64* tl = &blk[blk_row_at(s.rows, 0, tail_row(s.rows))];
    const u64* t = &ts[0];
    tl[kTailRecord] = t[kTsStaged] + 3;
    tl[kTailMachine] = tl[kTailRecord] + 7;
    tl[kTailSolveBegin] = tl[kTailMachine] + 4;
    tl[kTailSolveEnd] = tl[kTailSolveBegin] + 11;
    const bool adds_up = tl[kTailSolveEnd] + 15 == t[kTsControl];
    tl[kTailSinCos] = t[kTsControl] + 6;
    tl[kTailRows] = tl[kTailSinCos] + 5;
    expect("tail fixture adds up", 0, adds_up && tl[kTailRows] + 4 == t[kTsTables], 1);
    tl[kTailSpecBegin] = t[kTsStaged] + 2;  // spec_solve_start 2, spec_solve 9
    tl[kTailSpecEnd] = tl[kTailSpecBegin] + 9;
    const StampView v = {ts.data(), blk.data(), s, hist.data(), 1000, 1, false};
    PassStats ps;
    accumulate_pass_stats(v, 0, 1, ps);
    const double want[10] = {3, 7, 4, 11, 15, 6, 5, 4, 2, 9};
    for (int q = 0; q < 10; ++q) expect("tail phase", q, ps.tail_sum[q], ms(want[q]));
    expect("tail count", 0, ps.tail_count, 1);
    expect("tail body_count", 0, ps.body_count, 1);
    // the speculative pair out of order: the tail sample is taken without it
    const u64 keep = tl[kTailSpecBegin];
    tl[kTailSpecBegin] = t[kTsStaged] - 1;
    PassStats ps2;
    accumulate_pass_stats(v, 0, 1, ps2);
    for (int q = 0; q < 8; ++q) expect("tail phase (spec out of order)", q, ps2.tail_sum[q], ms(want[q]));
    expect("spec out of order", 8, ps2.tail_sum[8], 0.0);
    expect("spec out of order", 9, ps2.tail_sum[9], 0.0);
    expect("spec out of order: tail count", 0, ps2.tail_count, 1);
    tl[kTailSpecBegin] = keep;
    // one tail stamp out of order: no tail sample, the body sample still taken
    tl[kTailSinCos] = t[kTsControl] - 1;
    PassStats ps3;
    accumulate_pass_stats(v, 0, 1, ps3);
    for (int q = 0; q < 10; ++q) expect("tail out of order", q, ps3.tail_sum[q], 0.0);
    expect("tail out of order: tail count", 0, ps3.tail_count, 0);
    expect("tail out of order: body count", 0, ps3.body_count, 1);
    expect("tail out of order: body entry", 0, ps3.body_sum[0], ms(10));
}

// 6. the leading-tail kernel's tail: pass k's prologue row around pass k - 1's tail row
static void case_lead_tail() {
    const BlkShape s = {2, 3};
    std::vector<u64> blk(blk_words(s), 0ull);
    auto ts = fresh_rows(2);
    stamp_lead_pass(ts, 0, 1000, 900);
    stamp_lead_pass(ts, 1, 2010, 900);
    const auto hist = records({1, 2});
    stamp_wg(blk, s, 0, 0, 1000, 10, 30, 80, 40, 240);
    stamp_wg(blk, s, 1, 0, 2010, 50, 30, 80, 40, 240);
    // pass 0's kernel: a prologue with nothing to consume
    u64* r0 = &blk[blk_row_at(s.rows, 0, prologue_row(s.rows))];
    r0[kProEntry] = 990; r0[kProStaged] = 998; r0[kProReduced] = 998; r0[kProControlled] = 1001;
    // pass 1's kernel consumes pass 0: record 8, machine 12, solve_setup 3, solve 7, post_solve 11, sincos 5, rows 6, writeback 2
    u64* r1 = &blk[blk_row_at(s.rows, 1, prologue_row(s.rows))];
    u64* tl = &blk[blk_row_at(s.rows, 0, tail_row(s.rows))];
    r1[kProEntry] = 2000;
    r1[kProStaged] = r1[kProEntry] + 8;
    r1[kProReduced] = r1[kProStaged] + 12;
    tl[kTailRecord] = r1[kProReduced] + 3;
    tl[kTailMachine] = tl[kTailRecord] + 7;
    tl[kTailSolveBegin] = tl[kTailMachine] + 11;  // the fast path stamps both solve slots at the step's end
    tl[kTailSolveEnd] = tl[kTailMachine] + 11;
    tl[kTailSinCos] = tl[kTailSolveEnd] + 5;
    tl[kTailRows] = tl[kTailSinCos] + 6;
    r1[kProControlled] = tl[kTailRows] + 2;
    tl[kTailSpecBegin] = r1[kProReduced] + 1;  // stamped by the kernel, not decoded for leading-tail chains
    tl[kTailSpecEnd] = tl[kTailSpecBegin] + 9;
    const StampView v = {ts.data(), blk.data(), s, hist.data(), 1000, 1, true};
    PassStats ps0;
    accumulate_pass_stats(v, 0, 1, ps0);  // k == 0: no consumed pass
    expect("lead tail k=0: tail count", 0, ps0.tail_count, 0);
    expect("lead tail k=0: body count", 0, ps0.body_count, 1);
    for (int q = 0; q < 10; ++q) expect("lead tail k=0", q, ps0.tail_sum[q], 0.0);
    PassStats ps;
    accumulate_pass_stats(v, 0, 2, ps);
    const double want[10] = {8, 12, 3, 7, 11, 5, 6, 2, 0, 0};
    for (int q = 0; q < 10; ++q) expect("lead tail phase", q, ps.tail_sum[q], ms(want[q]));
    expect("lead tail count", 0, ps.tail_count, 1);
    expect("lead tail body count", 0, ps.body_count, 2);
    expect("lead tail body entry", 0, ps.body_sum[0], ms(10) + ms(50));
    expect("lead tail pass count", 0, (double)ps.count, 2);
    expect("lead tail phase_count", 0, ps.phase_count, 0);
    // a prologue row never stamped gives no sample
    r1[kProEntry] = 0;
    PassStats ps2;
    accumulate_pass_stats(v, 1, 1, ps2);
    expect("lead tail, prologue unstamped", 0, ps2.tail_count, 0);
}

// 7. a second round: only rows [first, first + count) are read, sums accumulate across calls
static void case_rounds() {
    auto ts = fresh_rows(4);
    const int dur[4] = {100, 200, 300, 400};
    for (int p = 0; p < 4; ++p) {
        const int ph[7] = {dur[p] - 60, 10, 10, 10, 10, 10, 10};
        stamp_pass(ts, p, 1000 * (p + 1), ph);
    }
    const auto hist = records({10, 20, 30, 40});
    const StampView v = {ts.data(), nullptr, kBlkShape, hist.data(), 100, 4, false};
    PassStats ps;
    accumulate_pass_stats(v, 2, 2, ps);
    expect("round 2 ms_sum", 0, ps.ms_sum, ms(300) + ms(400));
    expect("round 2 count", 0, (double)ps.count, 2);
    expect("round 2 bytes", 0, ps.bytes_sum, 2 * 16.0 * 100 + 36.0 * (30 + 40));
    expect("round 2 bodies", 0, ps.phase_sum[0], ms(240) + ms(340));
    expect("round 2 phase_count", 0, ps.phase_count, 2);
    accumulate_pass_stats(v, 0, 2, ps);
    expect("both rounds ms_sum", 0, ps.ms_sum, (ms(300) + ms(400)) + (ms(100) + ms(200)));
    expect("both rounds count", 0, (double)ps.count, 4);
    expect("both rounds bytes", 0, ps.bytes_sum, 4 * 16.0 * 100 + 36.0 * 100);
    expect("both rounds phase_count", 0, ps.phase_count, 4);
    expect("both rounds handoff", 1, ps.phase_sum[1], ((ms(10) + ms(10)) + ms(10)) + ms(10));
}

// 8. passes past the table and more workgroups than rows: block stamps clamped, pass rows still counted
static void case_clamped() {
    const BlkShape s = {2, 4};
    std::vector<u64> blk(blk_words(s), 0ull);
    auto ts = fresh_rows(3);
    for (int p = 0; p < 3; ++p) stamp_pass(ts, p, 1000 * (p + 1), kPh);
    const auto hist = records({1, 2, 3});
    for (int p = 0; p < 2; ++p) {
        stamp_wg(blk, s, p, 0, 1000 * (p + 1), 10, 30, 80, 40, 240);
        stamp_wg(blk, s, p, 1, 1000 * (p + 1), 30, 50, 120, 60, 360);
    }
    const StampView v = {ts.data(), blk.data(), s, hist.data(), 1000, 10 /* workgroups > rows */, false};
    PassStats ps;
    accumulate_pass_stats(v, 0, 3, ps);
    expect("clamped count", 0, (double)ps.count, 3);
    expect("clamped phase_count", 0, ps.phase_count, 3);
    expect("clamped ms_sum", 0, ps.ms_sum, (ms(200) + ms(200)) + ms(200));
    expect("clamped body_count", 0, ps.body_count, 2);
    const double want[5] = {20, 100, 50, 300, 40};
    for (int q = 0; q < 5; ++q) expect("clamped wg mean", q, ps.body_sum[q], ms(want[q]) + ms(want[q]));
    PassStats ps2;
    accumulate_pass_stats(v, 2, 1, ps2);  // a pass past the table alone
    expect("past the table: count", 0, (double)ps2.count, 1);
    expect_zero_blk(ps2, "past the table");
}

int main() {
    static_assert(sizeof(kPhaseNames) / sizeof(kPhaseNames[0]) == 22, "ndt_pass_phases reports 22 columns");
    static_assert(blk_words(kBlkShape) == (size_t)kBlkPasses * kBlkMax * kBlkSlots, "table shape");
    case_product();
    case_untimed();
    case_lead_row();
    case_wg_means();
    case_tail();
    case_lead_tail();
    case_rounds();
    case_clamped();
    std::printf("mismatched: %d\n", g_bad);
    return g_bad ? 1 : 0;
}
