// ndt_stamps.h — the one description of the derivative passes' profiling stamps (s_memrealtime, 100 MHz): which slot
// of which row means what, the order in which the slots of a healthy pass follow each other, and the decoder that turns
// read-back rows into the statistics ndt_last_timings / ndt_pass_phases report.
// The host part has no HIP dependency: host_prof.hip decodes through it and tests/native/stamp_decode_check.cpp runs it
// with a host compiler.  The device part holds the stamping helpers of the kernels and the profiling build's device
// objects; only a unit that stamps gets it, by defining NDT_STAMPS_DEVICE before the include (ndt_control.h does, for
// derivatives.hip and solver.hip; radix_pass's NDT_SORT_STAMP* of voxel_build.hip are a separate, unit-local set).
//
// Two tables:
//   * the pass rows, ts[kTsStride * pass + PassSlot]: the product library's stamps, taken when ndt_set_profiling is
//     on; k_align_init resets slot kTsEntry of every row to kTsUnstamped and the other slots to 0;
//   * the block table, [BlkShape.passes][BlkShape.rows][kBlkSlots]: the profiling build's stamps (-DNDT_BODY_STAMPS,
//     `make VARIANT=dbg`), one WgSlot row per workgroup, plain stores into private slots, never reset (0 = never
//     stamped).  The last two rows of a pass are reserved: the leading-tail kernel's prologue (PrologueSlot) and the
//     control step's tail (TailSlot).
#ifndef NDT_STAMPS_H_
#define NDT_STAMPS_H_
#include <cstddef>
#ifndef __host__  // a host compiler: ndt_types.h marks its constexpr helpers for both sides
#define __host__
#define __device__
#endif
#include "ndt_types.h"

namespace ndt {

// ---- pass rows --------------------------------------------------------------------------------------------------
constexpr int kTsStride = 16;  // words per pass row (the slots below, the rest unused)
constexpr unsigned long long kTsUnstamped = ~0ull;  // kTsEntry of a row no kernel stamped (k_align_init)
enum PassSlot : int {
    kTsEntry = 0,      // the pass kernel's start (workgroup 0; a leading-tail kernel: after its state staging)
    kTsEnd = 1,        // its end (the tail workgroup's last stamp; a leading-tail chain: the next kernel's start)
    kTsBodyEnd = 2,    // the last workgroup's body done, partials stored
    kTsAcquired = 3,   // hand-off: last ticket drawn, partials acquired
    kTsReduced = 4,    // partials reduced in fixed order
    kTsTables = 5,     // next transform and angle tables written (the control step's end)
    kTsStaged = 6,     // AlignState staged into LDS
    kTsControl = 7,    // Newton / More-Thuente step done
};

// ---- block table (profiling build) --------------------------------------------------------------------------------
constexpr int kBlkPasses = 64, kBlkMax = 1024, kBlkSlots = 8;
struct BlkShape {
    int passes, rows;  // stamped passes; rows per pass: rows - 2 workgroup rows, then the prologue and the tail row
};
constexpr BlkShape kBlkShape = {kBlkPasses, kBlkMax};
#ifdef NDT_BODY_STAMPS
constexpr bool kHaveBlkStamps = true;   // this build's pass kernels fill the block table (dbg_read_blk reads it)
#else
constexpr bool kHaveBlkStamps = false;
#endif
constexpr size_t blk_words(BlkShape s) { return (size_t)s.passes * s.rows * kBlkSlots; }
constexpr int prologue_row(int rows) { return rows - 2; }
constexpr int tail_row(int rows) { return rows - 1; }
constexpr size_t blk_row_at(int rows, int pass, int row) { return ((size_t)pass * rows + row) * kBlkSlots; }

enum WgSlot : int {
    kWgBodyStart = 0,
    kWgProbed = 1,       // tile marks: the last tile's probes done (0: a workgroup past the scan's points),
    kWgCompacted = 2,    //   its pairs compacted,
    kWgPaired = 3,       //   its pair math done
    kWgBodyEnd = 4,      // block reduction done, partials stored
    kWgSumProbe = 5,     // tile sums (ticks over all tiles of the workgroup): probes,
    kWgSumCompact = 6,   //   compaction,
    kWgSumPairs = 7,     //   pair math
};
enum TailSlot : int {
    kTailSolveBegin = 0,  // before the Newton LU solve (fast path: with the next three, at the step's end)
    kTailSolveEnd = 1,    // after it
    kTailSinCos = 2,      // sin / cos of the next angles ready
    kTailRows = 3,        // transform and table rows written
    kTailRecord = 4,      // pass record written
    kTailMachine = 5,     // state machine done
    kTailSpecBegin = 6,   // the speculative solve on wave 0: its start,
    kTailSpecEnd = 7,     //   its end
};
enum PrologueSlot : int {  // workgroup 0 of k_pass_lead, in the row of its body's pass
    kProEntry = 0,
    kProStaged = 1,
    kProReduced = 2,     // the consumed pass's partials reduced (= kProStaged when none were pending)
    kProControlled = 3,  // its control step done
};

// ---- phase sequences ----------------------------------------------------------------------------------------------
// A sequence names stamps in the order a healthy pass takes them: it holds when they are non-decreasing, and its
// phases are the consecutive differences.
enum StampRow : int { kRowPass, kRowWg, kRowTail, kRowPrologue, kStampRows };
struct StampRef {
    int row, slot;
};
struct StampRows {
    const unsigned long long* r[kStampRows];
};

// bodies, hand-off, reduce, stage, control, tables, drain
constexpr StampRef kSeqPass[8] = {{kRowPass, kTsEntry},   {kRowPass, kTsBodyEnd}, {kRowPass, kTsAcquired}, {kRowPass, kTsReduced},
                                  {kRowPass, kTsStaged},  {kRowPass, kTsControl}, {kRowPass, kTsTables},   {kRowPass, kTsEnd}};
// the last-workgroup tail, from the state's staging to the tables: record, machine, solve_setup, solve, post_solve,
// sincos, rows, writeback
constexpr StampRef kSeqTail[9] = {{kRowPass, kTsStaged},     {kRowTail, kTailRecord},   {kRowTail, kTailMachine},
                                  {kRowTail, kTailSolveBegin}, {kRowTail, kTailSolveEnd}, {kRowPass, kTsControl},
                                  {kRowTail, kTailSinCos},   {kRowTail, kTailRows},     {kRowPass, kTsTables}};
// spec_solve_start, spec_solve (taken only with a kSeqTail sample)
constexpr StampRef kSeqSpec[3] = {{kRowPass, kTsStaged}, {kRowTail, kTailSpecBegin}, {kRowTail, kTailSpecEnd}};
// the leading-tail kernel: pass k's prologue row around pass k - 1's tail row, in the same eight columns (staging,
// partial reduction, pass record, state machine, to the step, step + sin / cos, T + tables, to the body)
constexpr StampRef kSeqLead[9] = {{kRowPrologue, kProEntry}, {kRowPrologue, kProStaged}, {kRowPrologue, kProReduced},
                                  {kRowTail, kTailRecord},   {kRowTail, kTailMachine},   {kRowTail, kTailSolveEnd},
                                  {kRowTail, kTailSinCos},   {kRowTail, kTailRows},      {kRowPrologue, kProControlled}};
// a workgroup row's ordering (its phases are the tile sums, not differences)
constexpr StampRef kSeqWg[5] = {{kRowWg, kWgBodyStart}, {kRowWg, kWgProbed}, {kRowWg, kWgCompacted}, {kRowWg, kWgPaired},
                                {kRowWg, kWgBodyEnd}};

constexpr double kMsPerTick = 1e-5;  // 100 MHz

// True if the sequence holds; then (sum != nullptr) its N - 1 phases are added to sum[], in ms.
template <int N>
inline bool add_phases(const StampRows& rows, const StampRef (&seq)[N], double* sum) {
    unsigned long long e[N];
    for (int q = 0; q < N; ++q) {
        if (!rows.r[seq[q].row]) return false;
        e[q] = rows.r[seq[q].row][seq[q].slot];
        if (q && e[q] < e[q - 1]) return false;
    }
    if (sum)
        for (int q = 0; q + 1 < N; ++q) sum[q] += (double)(e[q + 1] - e[q]) * kMsPerTick;
    return true;
}

// ---- the 22 outputs of ndt_pass_phases ----------------------------------------------------------------------------
constexpr int kPassPhases = 7, kWgPhases = 5, kTailPhases = 10;
constexpr int kTailSpecPhase = 8;  // kSeqSpec's two columns behind the eight of kSeqTail / kSeqLead
constexpr const char* kPhaseNames[kPassPhases + kWgPhases + kTailPhases] = {
    // [0..6] kSeqPass (product library)
    "bodies", "handoff", "reduce", "stage", "control", "tables", "drain",
    // [7..11] workgroup means (profiling build, else 0)
    "entry", "probe", "compact", "pairs", "block_reduce",
    // [12..19] kSeqTail / kSeqLead, [20..21] kSeqSpec (profiling build, else 0)
    "record", "machine", "solve_setup", "solve", "post_solve", "sincos", "rows", "writeback", "spec_solve_start", "spec_solve",
};

namespace host {

// the statistics ndt_set_profiling resets: sums over the decoded passes, divided by their counts when reported
struct PassStats {
    double phase_sum[kPassPhases] = {0, 0, 0, 0, 0, 0, 0};
    int phase_count = 0;
    double body_sum[kWgPhases] = {0, 0, 0, 0, 0};
    int body_count = 0;
    double tail_sum[kTailPhases] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int tail_count = 0;
    double ms_sum = 0, bytes_sum = 0;
    long long count = 0;
};

// What an align read back, all indexed from pass 0
struct StampView {
    const unsigned long long* ts;   // pass rows
    const unsigned long long* blk;  // block table of `shape`, or nullptr (product library)
    BlkShape shape;
    const PassRecordDev* hist;      // pass records (their pair counts)
    int N;                          // source points
    int nb;                         // workgroups of the launched pass geometry
    bool lead;                      // leading-tail chain
};

inline bool pass_row_timed(const unsigned long long* t) { return t[kTsEntry] != kTsUnstamped && t[kTsEnd] > t[kTsEntry]; }

// Mean per-workgroup phases of pass pidx in ticks (entry delay after the pass stamp, the three tile sums, block
// reduction): false if the pass is outside the table, any live workgroup row is out of order, or none is live.
// A workgroup past the scan's points (the geometry covers its size bucket) never stamps kWgProbed and is skipped.
inline bool wg_means(const StampView& v, int pidx, double mean[kWgPhases]) {
    if (!v.blk || pidx >= v.shape.passes) return false;
    const int nbk = v.nb < v.shape.rows ? v.nb : v.shape.rows;
    const unsigned long long t0 = v.ts[kTsStride * (size_t)pidx + kTsEntry];
    double ph[kWgPhases] = {0, 0, 0, 0, 0};
    int nb_used = 0;
    for (int b = 0; b < nbk; ++b) {
        const unsigned long long* e = v.blk + blk_row_at(v.shape.rows, pidx, b);
        if (e[kWgProbed] == 0) continue;
        StampRows rows = {};
        rows.r[kRowWg] = e;
        if (!add_phases(rows, kSeqWg, nullptr)) return false;
        ++nb_used;
        ph[0] += e[kWgBodyStart] > t0 ? (double)(e[kWgBodyStart] - t0) : 0.0;
        for (int q = 0; q < 3; ++q) ph[1 + q] += (double)e[kWgSumProbe + q];
        ph[4] += (double)(e[kWgBodyEnd] - e[kWgPaired]);
    }
    if (nb_used == 0) return false;
    for (int q = 0; q < kWgPhases; ++q) mean[q] = ph[q] / nb_used;
    return true;
}

// Adds passes [first, first + count) to ps.  A pass row counts (ms_sum, bytes_sum = 16 N + 36 pairs, count) when it
// was stamped and ends after it starts, and in the seven phases when kSeqPass holds (a leading-tail kernel stamps only
// entry and end).  With a block table: the workgroup means of every pass inside it, and — only for a pass that gave
// those — the tail phases: kSeqTail (+ kSeqSpec) of the pass's own rows, or, leading-tail, kSeqLead of its prologue row
// and the previous pass's tail row (none for pass 0, or while the prologue row is unstamped).
inline void accumulate_pass_stats(const StampView& v, int first, int count, PassStats& ps) {
    double sum = 0, bytes = 0;
    int cnt = 0;
    for (int pidx = first; pidx < first + count; ++pidx) {
        const unsigned long long* t = v.ts + kTsStride * (size_t)pidx;
        if (!pass_row_timed(t)) continue;
        sum += (double)(t[kTsEnd] - t[kTsEntry]) * kMsPerTick;
        bytes += 16.0 * v.N + 36.0 * (double)v.hist[pidx].pairs;  // B_pass = 16 N + 36 P
        ++cnt;
        StampRows rows = {};
        rows.r[kRowPass] = t;
        if (add_phases(rows, kSeqPass, ps.phase_sum)) ++ps.phase_count;
    }
    for (int pidx = first; v.blk && pidx < first + count && pidx < v.shape.passes; ++pidx) {
        double mean[kWgPhases];
        if (!wg_means(v, pidx, mean)) continue;
        for (int q = 0; q < kWgPhases; ++q) ps.body_sum[q] += mean[q] * kMsPerTick;
        ++ps.body_count;
        const int R = v.shape.rows;
        StampRows rows = {};
        rows.r[kRowPass] = v.ts + kTsStride * (size_t)pidx;
        if (v.lead) {
            rows.r[kRowPrologue] = v.blk + blk_row_at(R, pidx, prologue_row(R));
            rows.r[kRowTail] = pidx >= 1 ? v.blk + blk_row_at(R, pidx - 1, tail_row(R)) : nullptr;
            if (rows.r[kRowPrologue][kProEntry] > 0 && add_phases(rows, kSeqLead, ps.tail_sum)) ++ps.tail_count;
            continue;
        }
        rows.r[kRowTail] = v.blk + blk_row_at(R, pidx, tail_row(R));
        if (add_phases(rows, kSeqTail, ps.tail_sum)) {
            add_phases(rows, kSeqSpec, ps.tail_sum + kTailSpecPhase);
            ++ps.tail_count;
        }
    }
    ps.ms_sum += sum;
    ps.bytes_sum += bytes;
    ps.count += cnt;
}

}  // namespace host
}  // namespace ndt
#endif  // NDT_STAMPS_H_

// ---- device side: the stamping helpers, empty in the product build --------------------------------------------------
#if defined(__HIPCC__) && defined(NDT_STAMPS_DEVICE) && !defined(NDT_STAMPS_DEVICE_H_)
#define NDT_STAMPS_DEVICE_H_
namespace ndt {
#ifdef NDT_BODY_STAMPS
// Internal linkage: every unit that includes this header has its own copy of the three objects.  derivatives.hip is
// the unit whose kernels stamp, and dbg_read_blk (defined there) reads that unit's table.  solver.hip's copy of
// g_tail_ts is never set, so the tail stamps k_svd_resume inherits from solve_loop / prepare_pass_parallel store nothing.
static __device__ unsigned long long g_blk_ts[blk_words(kBlkShape)];
// the tail of pass p stamps into row tail_row of pass p
static __device__ unsigned long long* g_tail_ts;
static __device__ unsigned g_tail_wg;  // the workgroup whose tail stamps g_tail_ts (leading-tail kernels: workgroup 0)

static_assert(sizeof(g_blk_ts) == blk_words(kBlkShape) * sizeof(unsigned long long), "the table dbg_read_blk copies is the decoder's");
// host side: this unit's table into host[count] (count = blk_words(kBlkShape) reads all of it)
static inline hipError_t read_blk_table(unsigned long long* host, size_t count) {
    const size_t n = count < blk_words(kBlkShape) ? count : blk_words(kBlkShape);
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(g_blk_ts), n * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
}
// this workgroup's WgSlot `slot` of `pass`, behind a workgroup barrier (part of what the profiling build measures)
#define NDT_BLK_STAMP(pass, slot)                                                                                     \
    do {                                                                                                              \
        __syncthreads();                                                                                              \
        if (threadIdx.x == 0 && (pass) >= 0 && (pass) < kBlkPasses && blockIdx.x < kBlkMax)                           \
            g_blk_ts[((size_t)(pass) * kBlkMax + blockIdx.x) * kBlkSlots + (slot)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
#define NDT_TAIL_STAMP(slot)                                                                            \
    do {                                                                                                \
        if (g_tail_ts && g_tail_wg == blockIdx.x) g_tail_ts[(slot)] = __builtin_amdgcn_s_memrealtime(); \
    } while (0)
// the workgroup barrier the profiling build takes before a stamp that is not an NDT_BLK_STAMP
#define NDT_STAMP_BARRIER() __syncthreads()
// the lanes for which `lane` holds (one): the tail stamps that follow belong to workgroup wg's control step of `pass`
#define NDT_TAIL_STAMPS_BEGIN(lane, pass, wg)                                                                                \
    do {                                                                                                                     \
        if (lane) {                                                                                                          \
            const int _p = (pass);                                                                                           \
            g_tail_ts = _p < kBlkPasses ? &g_blk_ts[((size_t)_p * kBlkMax + tail_row(kBlkMax)) * kBlkSlots] : nullptr;       \
            g_tail_wg = (wg);                                                                                                \
        }                                                                                                                    \
    } while (0)
// the tile clock of one workgroup's body: per-tile phase sums acc[3] (probe, compaction, pairs) since `mark`, stored
// into kWgSumProbe.. at the body's end
#define NDT_TILE_CLOCK(mark, acc) unsigned long long mark = 0, acc[3] = {0ull, 0ull, 0ull}
#define NDT_TILE_START(mark)                            \
    do {                                                \
        __syncthreads();                                \
        (mark) = __builtin_amdgcn_s_memrealtime();      \
    } while (0)
#define NDT_TILE_ACC(acc, mark, sum_slot) /* the time since mark into the sum of slot kWgSumProbe.. */ \
    do {                                                                  \
        __syncthreads();                                                  \
        const unsigned long long _n = __builtin_amdgcn_s_memrealtime();   \
        (acc)[(sum_slot) - kWgSumProbe] += _n - (mark);                   \
        (mark) = _n;                                                      \
    } while (0)
#define NDT_TILE_ACC_STORE(pass, acc)                                                                          \
    do {                                                                                                       \
        if (threadIdx.x == 0 && (pass) >= 0 && (pass) < kBlkPasses && blockIdx.x < kBlkMax)                     \
            for (int _k = 0; _k < 3; ++_k) g_blk_ts[((size_t)(pass) * kBlkMax + blockIdx.x) * kBlkSlots + kWgSumProbe + _k] = (acc)[_k]; \
    } while (0)
// k_pass_lead's prologue clock t[kProEntry .. kProReduced] of every workgroup; workgroup 0 stores it, and the time of
// the store as kProControlled, into row prologue_row of its body's pass
#define NDT_PROLOGUE_CLOCK(t) unsigned long long t[3]
#define NDT_PROLOGUE_MARK(t, slot) (t)[slot] = __builtin_amdgcn_s_memrealtime()
#define NDT_PROLOGUE_COPY(t, to, from) (t)[to] = (t)[from]
#define NDT_PROLOGUE_STORE(t, pass)                                                                                     \
    do {                                                                                                                \
        if (blockIdx.x == 0 && threadIdx.x == 0 && (pass) < kBlkPasses) {                                               \
            unsigned long long* _r = &g_blk_ts[((size_t)(pass) * kBlkMax + prologue_row(kBlkMax)) * kBlkSlots];         \
            _r[kProEntry] = (t)[kProEntry]; _r[kProStaged] = (t)[kProStaged]; _r[kProReduced] = (t)[kProReduced];       \
            _r[kProControlled] = __builtin_amdgcn_s_memrealtime();                                                      \
        }                                                                                                               \
    } while (0)
#else
static inline hipError_t read_blk_table(unsigned long long*, size_t) { return hipErrorNotSupported; }
#define NDT_BLK_STAMP(pass, slot) do { } while (0)
#define NDT_TAIL_STAMP(slot) do { } while (0)
#define NDT_STAMP_BARRIER() do { } while (0)
#define NDT_TAIL_STAMPS_BEGIN(lane, pass, wg) do { } while (0)
#define NDT_TILE_CLOCK(mark, acc) do { } while (0)
#define NDT_TILE_START(mark) do { } while (0)
#define NDT_TILE_ACC(acc, mark, sum_slot) do { } while (0)
#define NDT_TILE_ACC_STORE(pass, acc) do { } while (0)
#define NDT_PROLOGUE_CLOCK(t) do { } while (0)
#define NDT_PROLOGUE_MARK(t, slot) do { } while (0)
#define NDT_PROLOGUE_COPY(t, to, from) do { } while (0)
#define NDT_PROLOGUE_STORE(t, pass) do { } while (0)
#endif
}  // namespace ndt
#endif  // NDT_STAMPS_DEVICE
