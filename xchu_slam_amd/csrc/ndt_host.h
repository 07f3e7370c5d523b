// ndt_host.h — what the host units of the library share (internal; the C-ABI is include/ndt_hip.h): the context, its
// buffers and lanes, the error helpers, and the host functions that cross unit boundaries.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include <cstring>
#include <cstdlib>
#include <cstdio>
#include <algorithm>
#include <cmath>
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <thread>

#include "../../include/ndt_hip.h"
#include "ndt_kernels.h"
#include "ndt_geom.h"
#include "ndt_stamps.h"

namespace ndt::host {

constexpr int kTileKeys = kBlock * 16;

// The owners of the host side's GPU resources.  Nothing outside them releases device memory, pinned memory, an event, a
// stream or a graph exec: an owner's member order in its struct is the release order (reverse of declaration).
// A device buffer that owns its memory: freed with its owner (the ctx, a lane's scratch, a call's temporaries)
template <typename T> struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {  // by swap: what this held goes with o
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() { if (p) (void)hipFree(p); }
};

struct PinnedFree { void operator()(void* p) const { (void)hipHostFree(p); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); } };
struct GraphExecDestroy { void operator()(hipGraphExec_t g) const { (void)hipGraphExecDestroy(g); } };
template <typename T> using Pinned = std::unique_ptr<T, PinnedFree>;  // pinned host memory: Pinned<X> or Pinned<X[]>
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
using GraphExec = std::unique_ptr<std::remove_pointer_t<hipGraphExec_t>, GraphExecDestroy>;

// A captured graph kept with the key it was captured for: the launch shape and every buffer its nodes name that can be
// reallocated between two uses (keyed_graph)
template <int N> struct KeyedGraph {
    GraphExec exec;
    long long key[N] = {0};
};

struct Scratch {
    DevBuf<int> k0, v0, k1, v1, radix_aux, seg_start, flags, cloud_idx;
    DevBuf<int2> cloud_span;
    DevBuf<unsigned> radix_status;
    DevBuf<float> mm;
    DevBuf<float4> sorted_pts;   // points gathered into voxel order (VoxelGrid filter)
    DevBuf<unsigned long long> scan_status;   // single-pass scan look-back words (epoch-tagged, never cleared)
    DevBuf<unsigned long long> scan_ticket;   // monotone tile ticket of the single-pass scan
    unsigned long long scan_tickets = 0;      // host copy of the ticket counter
    unsigned scan_epoch = 0;
};

// Where a sort / scan runs: a stream and the scratch its kernels own (radix buffers, look-back words).  The ctx's
// main stream owns ndt_ctx::s; getFitnessScore (index build + query) and the keyframe insertion run on side lanes with
// scratch of their own, so that odom_node's per-scan tail overlaps the main stream's target build and align (C3).
struct Lane {
    hipStream_t st;
    Scratch& s;
};

// The host thread of a side lane: the lane's launches (a sort is ~13 kernels, ~4 us of host time each) are issued from
// it in FIFO order, so the caller only records a main-stream marker and posts the job.  A job's failure is kept until
// the lane's result call (take_error).
struct LaneWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv_job, cv_idle;
    std::deque<std::function<ndt_status()>> jobs;
    int pending = 0;
    bool stop = false;
    ndt_status st = NDT_OK;  // first failure not yet taken
    std::string msg;
    int device = 0;
    std::shared_mutex* capture_mu;  // the ctx's align-graph capture lock, held shared while a job runs (see ndt_ctx::capture_mu)

    LaneWorker(int dev, std::shared_mutex* cap) : device(dev), capture_mu(cap) { th = std::thread([this] { run(); }); }
    ~LaneWorker() {
        {
            std::lock_guard<std::mutex> g(mu);
            stop = true;
        }
        cv_job.notify_one();
        th.join();
    }
    void post(std::function<ndt_status()> f) {
        {
            std::lock_guard<std::mutex> g(mu);
            jobs.push_back(std::move(f));
            ++pending;
        }
        cv_job.notify_one();
    }
    // waits until every posted job has been issued; returns the pending failure (kept)
    ndt_status drain(std::string* err) {
        std::unique_lock<std::mutex> g(mu);
        cv_idle.wait(g, [this] { return pending == 0; });
        if (st != NDT_OK && err) *err = msg;
        return st;
    }
    // a job failed and its failure has not been taken yet (non-blocking)
    bool failed() {
        std::lock_guard<std::mutex> g(mu);
        return st != NDT_OK;
    }
    ndt_status take_error(std::string* err) {
        const ndt_status s = drain(err);
        std::lock_guard<std::mutex> g(mu);
        st = NDT_OK;
        return s;
    }
    void run();  // host_lanes.hip
};

// A descriptor database's per-slot arrays (Scan Context, Intensity Scan Context), carved from one device block:
// arr[k] holds cap slots of the k-th array (reserve_slots)
struct SlotArrays {
    DevBuf<char> block;
    size_t cap = 0;  // slots allocated
    std::vector<char*> arr;
    template <typename T> T* at(int k) const { return reinterpret_cast<T*>(arr[k]); }
};

// Exact nearest-neighbour index over a cloud (block-major binning, layout 1 of k_header): the points sorted into
// 8x8x8-cell blocks, a block table and per-occupied-block cell offsets.
struct NNIndex {
    DevBuf<GridHeader> hdr;             // binning (device)
    DevBuf<float4> pts;                 // points in (block, cell) order
    DevBuf<int> keys, start;            // per occupied cell: key, first point
    DevBuf<int> blk, off;               // block table + per-occupied-block cell offsets
    DevBuf<int> idx;                    // per sorted point: its index in the caller's order (built on request: ICP)
};

}  // namespace ndt::host

using namespace ndt;
using namespace ndt::host;

// The members below that only one host unit touches (plus ndt_create / ndt_destroy) are grouped by that unit.

// The caller-set options (ndt_set_pass_options, ndt_set_build_options, ndt_set_profiling) as one struct: the batched
// replay's helper contexts take them by one assignment (hand_options)
struct CtxOptions {
    // pass chains: leading-tail chains where an align is latency-bound, two points per thread in large
    // last-workgroup-tail passes, the source in target-cell order
    bool lead_tail = true;
    int ppt = 2;
    bool order_source = true;
    // target build (test hook): radix_force fixes the radix pass count; tile_tickets (sticky once a look-back timed out,
    // or set by the hook) takes every sort's tiles by atomic ticket
    int radix_force = 0;
    bool tile_tickets = false;
    bool profiling = false;
};

// host_lanes.hip — the side lanes, created as a whole on the first side-lane call (side_lanes): fit_stream runs
// getFitnessScore's index build and query, ins_stream the keyframe insertion, each issued by its own host thread.
// ev_main_* are the main-stream markers a side-lane job waits on; ev_fit_src / ev_fit_tgt mark (fit_stream) the end of
// the last query that read the ctx's source / of the last index build that read the ctx's target points (main waits
// on them before it rewrites what the index or query read); ev_fit / ev_ins mark a result in ndt_ctx::h_async.
// Streams first, workers last: a worker is joined before anything it launches on or into is released.
struct SideLanes {
    Stream fit_stream, ins_stream;
    Event ev_main_fit, ev_main_ins, ev_fit_src, ev_fit_tgt, ev_fit, ev_ins;
    Scratch s_fit, s_ins;
    DevBuf<GridHeader> d_hdr_ins;       // keyframe insertion's VoxelGrid binning
    DevBuf<float4> ins_tr, ins_ds;      // keyframe insertion scratch (transformed scan, VoxelGrid output)
    size_t ins_n_in = 0;
    int marked = 0;  // ndt_side_lanes_mark: bit 0 the next fitness query, bit 1 the next insertion use ev_main_fit as is
    bool fit_pending = false, ins_pending = false;
    bool fit_src_used = false, fit_tgt_used = false;
    std::unique_ptr<LaneWorker> fit_worker, ins_worker;  // host threads issuing the side lanes' launches
};

// host_front_end.hip — filter_node's front end (ndt_filter_scan): scratch + the last call's SOR statistics
struct FrontEnd {
    DevBuf<GridHeader> d_hdr;           // the filter's compaction scans: pad[0] look-back timeout flag, pad[1] kept count
    NNIndex sor_ix;                     // nearest-neighbour index over a filtered scan (StatisticalOutlierRemoval)
    DevBuf<int> flags, idx;
    DevBuf<float4> in, crop, ds, out;
    DevBuf<float> dist;
    DevBuf<double> thr;
    size_t nvox = 0;
};

// host_prof.hip — pass profiling: the stamp buffer (host_align.hip's launches carry it) and its pinned copies, which
// are part of every graph's cache key and stay, and the statistics ndt_set_profiling resets (ndt_stamps.h)
struct PassProf {
    DevBuf<unsigned long long> ts;      // the pass rows: kTsStride s_memrealtime stamps per pass
    Pinned<unsigned long long[]> h_ts;  // pinned copies, filled by k_readback before the align's sync (made together)
    Pinned<PassRecordDev[]> h_hist;
    using Stats = PassStats;
    Stats stats;
};

// host_icp.hip — point-to-point ICP (ndt_icp_align): the cumulative cloud X, per-point match / d2 of the last pass, the
// pass partials and ticket, the device state and history with the pinned state copies ([0] read back, [1] the initial
// state; the three made together), and the last run's result.  The graph exec last: released before the buffers it names.
struct IcpRun {
    DevBuf<float4> x;
    DevBuf<int> match;
    DevBuf<float> d2;
    DevBuf<double> part;
    DevBuf<unsigned> ticket;
    DevBuf<IcpState> d_state;
    DevBuf<IcpRecordDev> d_hist;
    Pinned<IcpState[]> h_state;
    bool used = false;                  // the fit index of this ctx carries the points' original indices from now on
    bool last = false;                  // the result have_result speaks of is the ICP's or GICP's (final_tf), not the NDT align's
    float final_tf[16] = {0};
    int n = 0;                          // source points of the last ICP align
    std::vector<IcpRecordDev> hist;
    KeyedGraph<12> graph;               // one run of passes and the state read-back
};

// host_gicp.hip — Generalized-ICP (ndt_gicp_align): the source's own neighbour index, the per-point covariances of both
// clouds (9 f64 each, kept until the cloud, k or epsilon changes), the last outer iteration's per-point pair data, the
// evaluation partials and the two tickets, the device state and history with the pinned state copies ([0] read back,
// [1] the state uploaded; the three made together), and the last run's record.
struct GicpRun {
    struct Cov {
        DevBuf<double> buf;
        bool valid = false;
        unsigned long long gen = 0;
        int k = 0;
        double eps = 0.0;
    };
    NNIndex src_ix;
    Cov cov_src, cov_tgt;
    DevBuf<double> raw;                 // test hook: the covariances before the SVD
    DevBuf<int> match;
    DevBuf<float> d2;
    DevBuf<float4> qt, gp;              // matched target point, guess * p
    DevBuf<double> M, part;
    DevBuf<unsigned> ticket;
    DevBuf<GicpState> d_state;
    DevBuf<GicpRecordDev> d_hist;
    Pinned<GicpState[]> h_state;
    int n = 0;                          // source points of the last GICP align
    unsigned long long src_gen = 0;     // the source that align ran over (the hooks refuse another)
    KeyedGraph<16> graph;               // one round of launches and the state read-back
    int launches = 0, rounds = 0;       // of the last align
    std::vector<GicpRecordDev> hist;
};

// host_ground.hip — filter_node's ground detection (ndt_ground_detect): the scan's copy and its tilted form, the clipped
// cloud and the cloud after the normal filter with their input indices, the clipped cloud's neighbour index, the
// per-point normals, the RANSAC state with its pinned copy (made together), the generator table and the sampler's
// hash, the hypotheses, the flag arrays of the three clouds, and the last call's record.
struct GroundRun {
    DevBuf<GridHeader> d_hdr;           // the compaction scans: pad[0] look-back timeout flag, pad[1] the clipped count
    NNIndex ix;                         // over the clipped cloud (k_ground_normals)
    DevBuf<float4> in, tilted, clip, nrm_t, nrm, normal4, cloud, cloud_ds;
    DevBuf<int> flags, idx, clip_org, nrm_org, nbr, gflag, mark;
    DevBuf<GroundState> d_state;
    Pinned<GroundState[]> h_state;      // [0] read back, [1] the state uploaded
    Pinned<int[]> h_words;              // [0..1] a compaction's flag and count, [2] the scans' flag, [3] the index sort's
    DevBuf<unsigned> table;             // the generator's first table_words outputs (seed 12345)
    size_t table_words = 0;
    DevBuf<int2> hash;                  // touched entries of shuffled_indices_ (2 x table_words slots)
    DevBuf<int4> tri;                   // per hypothesis: the sample and the sampler's status
    DevBuf<float4> coef;
    DevBuf<int> stat, cnt;
    size_t hyp_cap = 0;
    DevBuf<double> part;
    DevBuf<unsigned> ticket;
    std::vector<int> inject;            // ndt_ground_set_samples
    ndt_ground_params prm{};            // of the last detect
    ndt_ground_result res{};
    bool valid = false;                 // a detect has run: the hooks and ndt_ground_cloud have something to read
    int n_in = 0, n_clip = 0;
};

// Member order is part of the design: members are released in reverse order of declaration (delete c, the last step of
// ndt_destroy, after it has joined the lane workers, synchronised the three streams and dropped the graph execs).  So
// the main stream is declared before everything that is queued or released on it, capture_mu before the lane workers
// that hold its address, and the graph execs (icp.graph, gicp.graph, graphs) after the buffers their nodes name.
struct ndt_ctx {
    ndt_params prm{};
    int device = 0;
    int n_cu = 256;  // compute units the main stream's passes spread over (direct-pass grid)
    Stream stream;
    std::string err;
    CtxOptions opt;
    // held exclusively while the main stream captures an align graph and shared while a lane thread runs a job: a stream
    // wait issued by a lane thread during the capture is rejected by the runtime ("dependency created on uncaptured
    // work"), and the lanes' allocations (hipMalloc / hipFree on growth) stay out of it too; the two lanes issue side by
    // side
    std::shared_mutex capture_mu;
    // target grid
    DevBuf<float4> target;            // owned copy for host-provided targets
    const float4* target_ptr = nullptr;  // points the build reads (owned copy or the caller's device buffer)
    int M = 0;
    int target_dense = 1;
    bool has_target = false;
    bool grid_valid = false;
    float grid_res = 0.f;
    DevBuf<GridHeader> d_hdr, d_hdr_ds;
    Pinned<GridHeader> h_hdr;
    NNIndex fit_ix;                     // nearest-neighbour index over the target (getFitnessScore, ICP)
    DevBuf<int> fit_cnt;
    DevBuf<unsigned> fit_ticket;        // last-workgroup ticket of k_fitness (re-armed by that workgroup)
    DevBuf<double> fit_sum;
    DevBuf<float> fit_d2;
    int fit_n = 0;                      // source points of the last query
    bool fit_valid = false;             // index matches the current target
    // ev_tgt marks (main stream) the current target's points in place — recorded ahead of each build once the fit lane is
    // in use (tgt_ev_valid); the index build waits on it, not on the voxel build
    Event ev_tgt;
    bool tgt_ev_valid = false;
    // asynchronous getFitnessScore / keyframe insertion / scan filter: results land in pinned memory, an event marks them
    struct AsyncOut {
        double fit_sum;
        long long fit_cnt;
        GridHeader ins_hdr;
        int fe_words[4];  // ndt_filter_scan_device: [0] scan flag, [1] scan count, [2] outlier index sort flag
    };
    DevBuf<AsyncOut> d_async;
    Pinned<AsyncOut> h_async;
    SideLanes lanes;
    Scratch s;
    // merge-extended targets (ndt_set_target_append_device): the new points' sort scratch, the previous header, and whether
    // s's sorted keys / indices and d_hdr still describe the current target (no other main-stream sort since its build)
    Scratch s_inc;
    DevBuf<GridHeader> d_hdr_prev;
    bool inc_ok = false;
    // target-build robustness (GridHeader::pad[0] bits, checked by the align read-back or settle_build): radix passes
    // launched = the key width of the last grid read back, +1 bit of margin (radix_pred; 4 until a grid was seen, or
    // what opt.radix_force fixes); counters for ndt_build_stats
    int radix_pred = 4;
    bool build_unchecked = false;   // a target build queued whose error bits no align / settle_build has read yet
    bool rerun_full = false;        // a re-run build and its align's source sort: all four radix passes whatever the prediction or the hook says
    float al_guess[16] = {0};       // the guess of the align in flight (re-run after a flagged build)
    int al_berr = 0;                // build error bits the align's read-back found (align_finish_once)
    long long n_builds_full = 0, n_builds_merge = 0, n_builds_rerun = 0, n_rerun_lookback = 0;
    // target generations (one per setInputTarget): of the current target, of the one the fit index was last queued
    // for, and of the one the last align result belongs to (ndt_fitness_score_async_aligned)
    unsigned long long tgt_gen = 0, fit_ix_gen = ~0ull, align_tgt_gen = ~0ull;
    DevBuf<VoxelRec> recs;
    DevBuf<float4> cent;
    DevBuf<double> icovd, evals;
    DevBuf<int> cloud_key;
    DevBuf<int> valid_part;             // usable-voxel count per finalize wave (summed by ndt_grid_info)
    DevBuf<int2> table;
    unsigned max_log2cap = 6;
    DevBuf<int> grid;                   // dense cell -> cloud index grid (used when the bbox fits)
    long long grid_cells_seen = 0;      // largest target cell count read back (align, single pass, grid info): sizes the grid
    // source
    DevBuf<float4> source;
    int N = 0;
    bool has_source = false;
    unsigned long long src_gen = 0;     // one per setInputSource (GICP's source covariances)
    const float4* src_pend = nullptr;   // ndt_set_source_device's copy, deferred to the next align (its k_align_init) or flush_source
    // source in target-cell order for the passes of an align (k_src_keys): the cloud the pass kernels read
    DevBuf<float4> source_ord;
    DevBuf<int> ord_k0, ord_v0, ord_k1, ord_v1;
    const float4* pass_src = nullptr;
    FrontEnd fe;
    // align
    DevBuf<AlignState> d_state;
    // leading-tail chains (k_pass_lead): the second state / partials buffer of the ping-pong and the parity of the next
    // kernel of the align in flight (kernel j reads state j & 1, writes state (j + 1) & 1, writes partials j & 1)
    DevBuf<AlignState> d_state2;
    int lead = 0, lead_par = 0;
    bool no_lead = false;  // batched replay: several aligns in flight share the CUs, the redundant tails would cost CU time
    Pinned<AlignState> h_state;  // coherent, written by k_readback
    // read-back words (pinned, coherent): [0] sequence number of the last finished round, [1..2] device clock of the
    // align's start / that round's end (100 MHz); d_clk[0]: the start stamp k_align_init takes
    Pinned<unsigned long long[]> h_rb;
    DevBuf<unsigned long long> d_clk;
    unsigned long long rb_seq = 0, al_seq = 0;
    DevBuf<double> partials;
    DevBuf<double> partials2;  // leading-tail chains: the other partials buffer
    DevBuf<int4> nbr;                   // DIRECT7 neighbour cache of the align's source points (2 x int4 per point)
    DevBuf<double> score_part;          // calculateScore per-workgroup partial sums
    // gauss_d1_/d2_/d3_ as the reference holds them: set by the constructor for resolution 1.0 / outlier 0.55
    // (ndt_omp_impl.hpp:46-63) and recomputed at the start of every align (:80-87); calculateScore reads them
    double gauss_cur[3] = {0.0, 0.0, 0.0};
    DevBuf<double> reduce_out;
    DevBuf<unsigned> counter;           // last-workgroup ticket of the pass epilogue (re-armed by the last workgroup)
    DevBuf<PassRecordDev> d_hist;
    int hist_cap = kMaxHistory;
    DevBuf<float4> out_cloud;
    PassProf prof;
    bool have_result = false;
    IcpRun icp;
    GicpRun gicp;
    GroundRun ground;
    // graph cache: a few captured chains (different slot counts / buffers), round-robin replacement
    static constexpr int kGraphKey = 23;
    static constexpr int kGraphCache = 64;
    struct GraphEntry {
        GraphExec exec;
        long long key[kGraphKey] = {0};
    };
    GraphEntry graphs[kGraphCache];  // scans of a few neighbouring size buckets (geom_points) x both lead parities
    int graph_next = 0;
    int last_passes = 0;                // passes of the previous align: sizes the first graph round of the next
    // timing
    bool built_since_align = false;  // ms_build: a target build was queued since the last align
    double ms_build = 0, ms_align = 0;
    // align in flight (align_enqueue -> align_finish)
    bool al_inflight = false, al_mt = false;
    int al_full = 0, al_slots = 0;
    // helper contexts of the batched replay (one stream each), created on first use; ndt_destroy destroys them first
    std::vector<ndt_ctx*> helpers;
};

namespace ndt::host {

// sets the error text of the call (the ctx's, or on a side lane's host thread that thread's own) and returns st
ndt_status fail(ndt_ctx* c, ndt_status st, const std::string& msg);

inline Lane main_lane(ndt_ctx* c) { return Lane{c->stream.get(), c->s}; }

// what the pass geometry (ndt_geom.h) reads of a ctx
inline PassShape pass_shape(const ndt_ctx* c) {
    return PassShape{c->n_cu, c->N, c->M, c->prm.search, c->prm.min_points_per_voxel, c->opt.ppt};
}

// final_transformation_ of the last align, NDT or ICP (valid while have_result)
inline const float* last_final(const ndt_ctx* c) { return c->icp.last ? c->icp.final_tf : c->h_state->T; }

#define HIPCHK(ctx, expr)                                                                       \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail(ctx, NDT_EDEVICE, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)

// frees early (a DevBuf otherwise lives as long as its owner)
template <typename T> void release(DevBuf<T>& b) { DevBuf<T> gone(std::move(b)); }

template <typename T> ndt_status ensure(ndt_ctx* c, DevBuf<T>& b, size_t n) {
    if (n == 0) n = 1;
    if (b.cap >= n) return NDT_OK;
    const size_t want = std::max(n, b.cap + b.cap / 2);
    release(b);
    if (hipMalloc(&b.p, want * sizeof(T)) != hipSuccess) {
        b.p = nullptr;
        return fail(c, NDT_ENOMEM, "hipMalloc failed");
    }
    b.cap = want;
    return NDT_OK;
}

#define TRY(expr)                          \
    do {                                   \
        ndt_status _s = (expr);            \
        if (_s != NDT_OK) return _s;       \
    } while (0)

// Creation into an owner: the owner is set only when the runtime call succeeded (n elements of pinned memory with
// hipHostMalloc's flags; an event with hipEventCreateWithFlags's; a non-blocking stream of the given priority)
template <typename T> ndt_status make_pinned(ndt_ctx* c, Pinned<T>& out, size_t n, unsigned flags) {
    void* p = nullptr;
    if (hipHostMalloc(&p, n * sizeof(std::remove_extent_t<T>), flags) != hipSuccess) return fail(c, NDT_ENOMEM, "hipHostMalloc failed");
    out.reset(static_cast<std::remove_extent_t<T>*>(p));
    return NDT_OK;
}
inline ndt_status make_event(ndt_ctx* c, Event& out, unsigned flags) {
    hipEvent_t e = nullptr;
    HIPCHK(c, hipEventCreateWithFlags(&e, flags));
    out.reset(e);
    return NDT_OK;
}
inline ndt_status make_stream(ndt_ctx* c, Stream& out, int priority) {
    hipStream_t st = nullptr;
    HIPCHK(c, hipStreamCreateWithPriority(&st, hipStreamNonBlocking, priority));
    out.reset(st);
    return NDT_OK;
}

// The device state of a run, its device history and the pinned pair of state copies, made together or not at all
// (what: the error text when one of them cannot be allocated)
template <typename S, typename R>
ndt_status make_run_state(ndt_ctx* c, DevBuf<S>& d_state, DevBuf<R>& d_hist, size_t hist_cap, Pinned<S[]>& h_state,
                          unsigned pinned_flags, const char* what) {
    if (h_state) return NDT_OK;
    DevBuf<S> ds;
    DevBuf<R> dh;
    Pinned<S[]> hs;
    if (ensure(c, ds, 1) != NDT_OK || ensure(c, dh, hist_cap) != NDT_OK || make_pinned(c, hs, 2, pinned_flags) != NDT_OK)
        return fail(c, NDT_ENOMEM, what);
    d_state = std::move(ds);
    d_hist = std::move(dh);
    h_state = std::move(hs);
    return NDT_OK;
}

// the caller-set options handed to a helper context of the batched replay; tile_tickets stays set once a look-back of
// the helper's own timed out
inline void hand_options(ndt_ctx* h, const ndt_ctx* c) {
    const bool sticky = h->opt.tile_tickets;
    h->opt = c->opt;
    h->opt.tile_tickets = sticky || c->opt.tile_tickets;
}

inline ndt_status set_dev(ndt_ctx* c) {
    HIPCHK(c, hipSetDevice(c->device));
    return NDT_OK;
}

// ahead of a handle's delete (ndt_sc, ndt_isc, ndt_pgo, ndt_map): launches queued on its ctx's stream still read its buffers
inline void drain_for_destroy(const ndt_ctx* c) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream.get());
}

// what every registration call needs: a target and a non-empty source
inline ndt_status need_target_and_source(ndt_ctx* c) {
    if (!c->has_target) return fail(c, NDT_ENOTARGET, "no input target");
    if (!c->has_source || c->N == 0) return fail(c, NDT_ENOSOURCE, "no input source");
    return NDT_OK;
}

// host_sort.hip
ndt_status scan_ctx(ndt_ctx* c, Lane L, int nb, ScanCtx* sc);
ndt_status enqueue_scan(ndt_ctx* c, Lane L, const int* in, int n_host, const int* n_dev, int* out, int* total_out, GridHeader* herr);
int radix_items(const ndt_ctx* c, int n);
size_t radix_status_words(int nb);
void launch_radix_pass(const ndt_ctx* c, Lane L, int items, int nb, int* k0, int* v0, int* k1, int* v1, int n, int pass,
                       const GridHeader* h, GridHeader* herr, int last_pass = 3);
int radix_launch_passes(const ndt_ctx* c);
void note_grid_width(ndt_ctx* c, long long cells, int dense);
ndt_status enqueue_bin_and_sort(ndt_ctx* c, Lane L, const float4* pts, int n, int dense, GridHeader* h, float leaf, int layout = 0,
                                int binning = 0, int2* cloud_span = nullptr, int passes = 4);
ndt_status enqueue_voxel_grid(ndt_ctx* c, Lane L, const float4* in, int n, float leaf, GridHeader* h, float4* out);
// host_target.hip
ndt_status build_target(ndt_ctx* c);
ndt_status rerun_build(ndt_ctx* c, int berr);
ndt_status settle_build(ndt_ctx* c);
ndt_status upload_points(ndt_ctx* c, DevBuf<float4>& dst, const float* xyz, size_t n, size_t stride_bytes);
// host_align.hip
void invalidate_graph(ndt_ctx* c);
ndt_status copy16(ndt_ctx* c, hipStream_t stream, void* dst, const void* src, size_t bytes);
ndt_status flush_source(ndt_ctx* c);
ndt_status capture_graph(ndt_ctx* c, const char* end_what, const std::function<ndt_status()>& body, GraphExec* out);
// g's graph when it was captured for this key; else the main stream synchronised, the old graph dropped and body captured
template <int N>
ndt_status keyed_graph(ndt_ctx* c, KeyedGraph<N>& g, const long long (&key)[N], const char* end_what,
                       const std::function<ndt_status()>& body, hipGraphExec_t* out) {
    if (!g.exec || std::memcmp(key, g.key, sizeof(key)) != 0) {
        if (g.exec) {
            HIPCHK(c, hipStreamSynchronize(c->stream.get()));
            g.exec.reset();
        }
        TRY(capture_graph(c, end_what, body, &g.exec));
        std::memcpy(g.key, key, sizeof(key));
    }
    *out = g.exec.get();
    return NDT_OK;
}
// host_prof.hip
ndt_status ensure_stamp_copies(ndt_ctx* c);
ndt_status collect_pass_times(ndt_ctx* c, int hist_before);
// host_lanes.hip
ndt_status main_after_fit(ndt_ctx* c, bool source);
ndt_status enqueue_nn_index(ndt_ctx* c, Lane L, const float4* pts, int n, int dense, float cell, NNIndex& ix, bool want_idx = false);
ndt_status ensure_fit_index(ndt_ctx* c);
ndt_status target_nn_index(ndt_ctx* c, const char* prefix);
ndt_status check_index_sort(ndt_ctx* c, const NNIndex& ix, const char* prefix);
// host_front_end.hip
ndt_status voxel_downsample_dev(ndt_ctx* c, const float4* in, size_t n, float leaf, float4* out, size_t* n_out,
                                const char* what = "voxel downsample");
ndt_status enqueue_compact4(ndt_ctx* c, const float4* in, const int* flags, int* idx, int n, float4* out, int* d_count, GridHeader* herr);
ndt_status compact4_count(ndt_ctx* c, GridHeader* herr, int* h_words, const char* timeout_text);
// host_sc.hip
ndt_status reserve_slots(ndt_ctx* c, SlotArrays& a, size_t size, size_t need, std::initializer_list<size_t> slot_bytes, const char* what);

}  // namespace ndt::host
