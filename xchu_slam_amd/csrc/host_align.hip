// host_align.hip — the align: pass geometry, the captured pass chains and their read-back, the align state machine,
// the batched replay, and the source / result entry points.
#include "ndt_host.h"

namespace ndt::host {

// Drops every cached chain; a chain may still be in flight on the stream, so the stream is waited for first (see build_graph)
void invalidate_graph(ndt_ctx* c) {
    bool any = false;
    for (auto& g : c->graphs) any = any || g.exec;
    if (any && c->stream) (void)hipStreamSynchronize(c->stream.get());
    for (auto& g : c->graphs) g.exec.reset();
}

// Device copy on `stream` by k_copy16 when both pointers and the size are 16-byte aligned, else a runtime copy
ndt_status copy16(ndt_ctx* c, hipStream_t stream, void* dst, const void* src, size_t bytes) {
    if (!bytes) return NDT_OK;
    if (((uintptr_t)dst | (uintptr_t)src | bytes) & 15) {
        HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
        return NDT_OK;
    }
    const size_t n = bytes / 16;
    const int nb = (int)std::min<size_t>(std::max<size_t>(1, (n + kBlock - 1) / kBlock), 1024);
    hipLaunchKernelGGL(k_copy16, dim3(nb), dim3(kBlock), 0, stream, reinterpret_cast<const uint4*>(src), reinterpret_cast<uint4*>(dst), n);
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

// The deferred source copy (ndt_set_source_device), issued now on the ctx stream for a reader other than an align
ndt_status flush_source(ndt_ctx* c) {
    if (!c->src_pend) return NDT_OK;
    const float4* p = c->src_pend;
    c->src_pend = nullptr;
    if (c->N) TRY(copy16(c, c->stream.get(), c->source.p, p, (size_t)c->N * sizeof(float4)));
    return NDT_OK;
}

// One graph from what `body` queues on the ctx stream: captured under capture_mu (see ndt_ctx), instantiated into *out
// (empty on failure).  end_what prefixes the error text of a capture the runtime rejects.
ndt_status capture_graph(ndt_ctx* c, const char* end_what, const std::function<ndt_status()>& body, GraphExec* out) {
    out->reset();
    hipGraph_t g = nullptr;
    std::unique_lock<std::shared_mutex> capture(c->capture_mu);
    HIPCHK(c, hipStreamBeginCapture(c->stream.get(), hipStreamCaptureModeThreadLocal));
    const ndt_status st = body();
    hipError_t e = hipStreamEndCapture(c->stream.get(), &g);
    capture.unlock();
    if (st != NDT_OK) {
        if (e == hipSuccess) (void)hipGraphDestroy(g);
        return st;
    }
    if (e != hipSuccess) return fail(c, NDT_EDEVICE, std::string(end_what) + hipGetErrorString(e));
    hipGraphExec_t gx = nullptr;
    e = hipGraphInstantiate(&gx, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) return fail(c, NDT_EDEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
    out->reset(gx);
    return NDT_OK;
}

namespace {

bool needs_direct(const ndt_params& p) { return p.precision_mode == 0 && p.search != NDT_KDTREE; }
bool needs_radius(const ndt_params& p, bool mt_possible) { return !needs_direct(p) || mt_possible; }

// The launch geometry (ndt_geom.h) of this ctx's source, target, params and options
bool grid_one_tile(const ndt_ctx* c) { return grid_one_tile(pass_shape(c)); }
bool pass_ppt2(const ndt_ctx* c) { return pass_ppt2(pass_shape(c)); }
bool lead_one_tile(const ndt_ctx* c) { return lead_one_tile(pass_shape(c)); }
PassGeom direct_geom(const ndt_ctx* c, bool lead) { return direct_geom(pass_shape(c), lead); }

// The neighbour cache the direct passes of an align read and write (DIRECT7 only; sized by ensure_align_buffers); the
// single-pass test hook (mode 1) runs without it
// one tile per workgroup only (C2 / C3 / C4 scans): its entries are read at kernel start beside the points; where
// workgroups walk several tiles (C5) the later tiles' entry loads and the registers they hold cost more than the
// probes they save (C5 88.6 vs 81.3 us per pass, C2 20.6 vs 21.1 us)
bool nbr_single_tile(const ndt_ctx* c, bool lead) {
    const int n = geom_points(std::max(1, c->N));
    const PassGeom g = direct_geom(c, lead);
    const int per_tile = g.block * ((!lead && pass_ppt2(c)) ? 2 : 1);
    return ceil_div(n, g.nb * per_tile) <= 1;
}
// allocation: whichever chain (leading tail or not) the next align picks
bool nbr_cache_wanted(const ndt_ctx* c) {
    if (c->prm.search != NDT_DIRECT7) return false;
    return nbr_single_tile(c, true) || nbr_single_tile(c, false);
}
int4* nbr_cache(ndt_ctx* c, int mode) {
    if (mode != 0 || c->prm.search != NDT_DIRECT7 || !nbr_single_tile(c, c->lead != 0)) return nullptr;
    return c->nbr.cap >= 2 * (size_t)geom_points(std::max(1, c->N)) ? c->nbr.p : nullptr;
}

void launch_pass(ndt_ctx* c, int mode) {
    const ndt_params& p = c->prm;
    if (!needs_direct(p)) return;
    const PassGeom g = direct_geom(c, false);
    const bool ppt2 = pass_ppt2(c), one = grid_one_tile(c);
    auto* kern = p.search == NDT_DIRECT26 ? k_pass_direct<S_DIRECT26, 1, false>
                 : p.search == NDT_DIRECT1
                     ? (ppt2 ? k_pass_direct<S_DIRECT1, 2, false> : (one ? k_pass_direct<S_DIRECT1, 1, true> : k_pass_direct<S_DIRECT1, 1, false>))
                     : (ppt2 ? k_pass_direct<S_DIRECT7, 2, false> : (one ? k_pass_direct<S_DIRECT7, 1, true> : k_pass_direct<S_DIRECT7, 1, false>));
    hipLaunchKernelGGL(kern, dim3(g.nb), dim3(g.block), 0, c->stream.get(), c->pass_src, geom_points(c->N), g.ppb, c->d_hdr.p,
                       c->table.p, c->grid.p, c->recs.p, c->d_state.p, c->d_state.p, c->partials.p, c->counter.p, c->reduce_out.p,
                       c->d_hist.p, c->hist_cap, mode, c->opt.profiling ? c->prof.ts.p : nullptr, nbr_cache(c, mode));
}

void launch_radius(ndt_ctx* c, int mode) {
    const int nb = pass_blocks(geom_points(c->N));
    hipLaunchKernelGGL(k_pass_radius, dim3(nb), dim3(kBlock), 0, c->stream.get(), c->pass_src, geom_points(c->N), c->d_hdr.p, c->table.p, c->grid.p, c->recs.p,
                       c->cent.p, c->icovd.p, c->d_state.p, c->d_state.p, c->partials.p, c->counter.p, c->reduce_out.p, c->d_hist.p,
                       c->hist_cap, mode,
                       c->opt.profiling ? c->prof.ts.p : nullptr);
}

// One leading-tail pass kernel (k_pass_lead) as kernel j = c->lead_par of the align's chain (see ndt_ctx::lead); the
// one-tile kernel (768 threads, three waves per SIMD) wherever the scan's point bucket fits one tile per workgroup.
void launch_lead(ndt_ctx* c, int j) {
    const PassGeom g = direct_geom(c, true);
    const bool one = lead_one_tile(c);
    AlignState* st[2] = {c->d_state.p, c->d_state2.p};
    double* pp[2] = {c->partials.p, c->partials2.p};
    const AlignState* sin = st[j & 1];
    AlignState* sout = st[(j + 1) & 1];
    const double* pin = pp[(j + 1) & 1];
    double* pout = pp[j & 1];
    unsigned long long* ts = c->opt.profiling ? c->prof.ts.p : nullptr;
    auto* kern = c->prm.search == NDT_DIRECT26  ? k_pass_lead<S_DIRECT26, false>
                 : c->prm.search == NDT_DIRECT1 ? (one ? k_pass_lead<S_DIRECT1, true> : k_pass_lead<S_DIRECT1, false>)
                                                : (one ? k_pass_lead<S_DIRECT7, true> : k_pass_lead<S_DIRECT7, false>);
    hipLaunchKernelGGL(kern, dim3(g.nb), dim3(g.block), 0, c->stream.get(), c->pass_src, geom_points(c->N), g.ppb, c->d_hdr.p, c->table.p,
                       c->grid.p, c->recs.p, sin, sout, pin, pout, c->d_hist.p, c->hist_cap, ts, nbr_cache(c, 0));
}

// enqueue `slots` (pass, control) pairs
ndt_status enqueue_chain(ndt_ctx* c, int slots, bool mt_possible) {
    for (int s = 0; s < slots; ++s) {
        if (c->lead) {
            launch_lead(c, c->lead_par + s);
        } else {
            launch_pass(c, 0);
            if (needs_radius(c->prm, mt_possible)) launch_radius(c, 0);
        }
    }
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

void init_state(ndt_ctx* c, const float guess[16], AlignState* st) {
    std::memset(st, 0, sizeof(AlignState));
    const ndt_params& p = c->prm;
    gauss_constants(p.outlier_ratio, p.resolution, &st->gauss_d1, &st->gauss_d2, &st->gauss_d3);
    c->gauss_cur[0] = st->gauss_d1;
    c->gauss_cur[1] = st->gauss_d2;
    c->gauss_cur[2] = st->gauss_d3;
    st->step_max = p.step_size;
    st->step_min = p.trans_eps / 2;
    st->trans_eps = p.trans_eps;
    st->max_iter = p.max_iter;
    st->n_src = c->N;
    st->search = p.search;
    st->precision = p.precision_mode;
    st->mt_possible = (st->step_max - st->step_min) > 0 ? 0 : 1;
    st->radius = p.resolution;
    // pcl::Registration::align: final = I; computeTransformation: guess != I -> final = guess, output = guess * input
    bool ident = true;
    for (int k = 0; k < 16; ++k)
        if (guess[k] != ((k % 5 == 0) ? 1.f : 0.f)) ident = false;
    float F[16];
    for (int k = 0; k < 16; ++k) F[k] = ident ? ((k % 5 == 0) ? 1.f : 0.f) : guess[k];
    for (int k = 0; k < 16; ++k) st->T[k] = F[k];
    // p = [translation, rotation().eulerAngles(0,1,2)] in f32 (ndt_omp_impl.hpp:96-104)
    float L[9], R[9], eul[3];
    for (int j = 0; j < 3; ++j)
        for (int i = 0; i < 3; ++i) L[i + 3 * j] = F[i + 4 * j];
    polar_rotation_f(L, R);
    euler012_f(R, eul);
    st->p[0] = F[12]; st->p[1] = F[13]; st->p[2] = F[14];
    st->p[3] = eul[0]; st->p[4] = eul[1]; st->p[5] = eul[2];
    for (int k = 0; k < 6; ++k) { st->x_eval[k] = st->p[k]; st->x_t[k] = st->p[k]; }
    angle_tables(st->p, st->jang, st->hang, st->jang_d, st->hang_d);
    st->phase = 0;
    st->pending = 1;
    st->pass_kind = PASS_FULL;
}

ndt_status ensure_align_buffers(ndt_ctx* c) {
    const int nb = pass_blocks(geom_points(c->N));
    const int nbd = std::max(nb, std::max(direct_geom(c, false).nb, direct_geom(c, true).nb));
    // + the group partials of the two-level hand-off (grids of more than kTwoLevelMinBlocks workgroups)
    TRY(ensure(c, c->partials, (size_t)kNumAcc * (partial_stride(nbd) + kMaxGroups)));
    TRY(ensure(c, c->partials2, (size_t)kNumAcc * (partial_stride(nbd) + kMaxGroups)));
    TRY(ensure(c, c->reduce_out, kNumAcc));
    TRY(ensure(c, c->counter, kPassCounterWords));
    // the neighbour cache only where the passes read it (32 B per point; a multi-tile geometry such as C5's never does)
    if (nbr_cache_wanted(c)) TRY(ensure(c, c->nbr, 2 * (size_t)geom_points(c->N)));
    else if (c->nbr.p) release(c->nbr);
    return NDT_OK;
}

// The device state after `ahead` more kernels of the chain: the only state buffer without leading-tail chains, else
// the ping-pong buffer kernel lead_par + ahead reads.
AlignState* lead_state(ndt_ctx* c, int ahead) {
    if (!c->lead) return c->d_state.p;
    return ((c->lead_par + ahead) & 1) ? c->d_state2.p : c->d_state.p;
}

// End-of-round read-back, queued on the stream before the align's own synchronisation (no extra round trip): the
// optimiser state and, when profiling, the stamps and pass records of passes [from, to), all by one k_readback launch
// straight into pinned host memory (blit copies would cost a launch + gap each), then the round's sequence number.
ndt_status prepare_readback(ndt_ctx* c, int from, int to) {
    to = std::min(to, c->hist_cap);
    const bool prof = c->opt.profiling && to > from;
    if (prof) TRY(ensure_stamp_copies(c));
    return NDT_OK;
}

// seq: the round's sequence number, or 0 for the one k_align_init stored in d_clk[2] (the launch is then graph-capturable)
void launch_readback(ndt_ctx* c, int from, int to, const AlignState* d_src, unsigned long long seq) {
    to = std::min(to, c->hist_cap);
    const bool prof = c->opt.profiling && to > from;
    static_assert(sizeof(PassRecordDev) % 8 == 0, "pass records copied as 8-byte words");
    using u64 = unsigned long long;
    const int ts_words = prof ? kTsStride * (to - from) : 0;
    const int hist_words = prof ? (int)((to - from) * sizeof(PassRecordDev) / 8) : 0;
    const u64* ts = prof ? c->prof.ts.p + kTsStride * (size_t)from : nullptr;
    u64* h_ts = prof ? c->prof.h_ts.get() + kTsStride * (size_t)from : nullptr;
    const u64* hist = prof ? reinterpret_cast<const u64*>(c->d_hist.p + from) : nullptr;
    u64* h_hist = prof ? reinterpret_cast<u64*>(c->prof.h_hist.get() + from) : nullptr;
    hipLaunchKernelGGL(k_readback, dim3(1), dim3(kBlock), 0, c->stream.get(), reinterpret_cast<const u64*>(d_src),
                       reinterpret_cast<u64*>(c->h_state.get()), (int)(sizeof(AlignState) / 8), ts, h_ts, ts_words, hist, h_hist, hist_words,
                       c->d_clk.p, c->h_rb.get() + 1, c->h_rb.get(), seq,
                       d_src != c->d_state.p ? reinterpret_cast<u64*>(c->d_state.p) : nullptr, c->d_hdr.p);
}

// with_readback: the round's k_readback is captured as the graph's last node (the first round of an align: from 0 to
// the round's passes, its sequence number read from d_clk[2]) — a kernel queued behind a graph launch starts ~8.7 us after
// the graph's last kernel (rocprofv3, C2 step), inside the graph it follows at once
ndt_status build_graph(ndt_ctx* c, int slots, bool mt_possible, hipGraphExec_t* out, bool with_readback) {
    constexpr int kGraphKey = ndt_ctx::kGraphKey;
    // every pointer / size baked into the captured kernels
    // (one slot per captured pointer: a combined key could collide after a reallocation and replay freed buffers)
    const long long key[kGraphKey] = {geom_points(c->N), (long long)(uintptr_t)c->pass_src, (long long)(uintptr_t)c->table.p, c->prm.search,
                                      c->prm.precision_mode,
                                      mt_possible | (c->opt.profiling ? 2 : 0) | (c->lead ? 4 : 0) | ((c->lead_par & 1) ? 8 : 0) |
                                          (pass_ppt2(c) ? 16 : 0), slots,
                                      (long long)(uintptr_t)c->recs.p, (long long)(uintptr_t)c->partials.p,
                                      (long long)(uintptr_t)c->grid.p, (long long)(uintptr_t)c->reduce_out.p,
                                      (long long)(uintptr_t)c->counter.p, (long long)(uintptr_t)c->cent.p,
                                      (long long)(uintptr_t)c->icovd.p, (long long)(uintptr_t)c->prof.ts.p,
                                      (long long)(uintptr_t)c->d_hdr.p, (long long)(uintptr_t)c->d_state.p,
                                      (long long)(uintptr_t)c->d_hist.p, (long long)(uintptr_t)c->partials2.p,
                                      (long long)(uintptr_t)nbr_cache(c, 0), with_readback ? 1 : 0,
                                      (long long)(uintptr_t)c->prof.h_ts.get(), (long long)(uintptr_t)c->prof.h_hist.get()};
    for (auto& g : c->graphs)
        if (g.exec && std::memcmp(key, g.key, sizeof(key)) == 0) {
            *out = g.exec.get();
            return NDT_OK;
        }
    ndt_ctx::GraphEntry& slot = c->graphs[c->graph_next];
    c->graph_next = (c->graph_next + 1) % ndt_ctx::kGraphCache;
    if (slot.exec) {
        // the evicted chain may still run on the stream (an earlier align of this ctx, an async align whose wait has not
        // come): its executable owns the kernel arguments of its nodes, so it is destroyed only once the stream is past it
        HIPCHK(c, hipStreamSynchronize(c->stream.get()));
        slot.exec.reset();
    }
    if (c->opt.profiling) TRY(ensure(c, c->prof.ts, kTsStride * (size_t)c->hist_cap));
    const int rb_to = slots * (mt_possible ? 4 : 1);
    if (with_readback) TRY(prepare_readback(c, 0, rb_to));
    TRY(capture_graph(c, "hipStreamEndCapture: ", [&]() -> ndt_status {
        TRY(enqueue_chain(c, slots, mt_possible));
        if (with_readback) launch_readback(c, 0, rb_to, lead_state(c, slots), 0ull);
        return NDT_OK;
    }, &slot.exec));
    std::memcpy(slot.key, key, sizeof(key));
    *out = slot.exec.get();
    return NDT_OK;
}

// The pass chain of one round: the captured graph (one hipGraphLaunch per round).
ndt_status launch_chain(ndt_ctx* c, int slots, bool mt, bool with_readback = false) {
    hipGraphExec_t gx = nullptr;
    TRY(build_graph(c, slots, mt, &gx, with_readback));
    HIPCHK(c, hipGraphLaunch(gx, c->stream.get()));
    return NDT_OK;
}

// A continuation round's read-back, queued behind its graph
ndt_status enqueue_readback(ndt_ctx* c, int from, int to, const AlignState* d_src) {
    TRY(prepare_readback(c, from, to));
    c->al_seq = ++c->rb_seq;
    launch_readback(c, from, to, d_src, c->al_seq);
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

// Source order of this align (k_src_keys): points sorted by the target cell they fall into under the initial
// transform, so that neighbouring lanes of a pass probe and gather neighbouring cells.  Clouds below 256 Ki points keep
// their order: there the sort (~35 us) costs about what it saves (C2: 1.5 us per pass over 33 passes; C3: 2-4 passes).
constexpr int kOrderMinPoints = 262144;
constexpr int kLeadMaxPoints = 262144;  // leading-tail chains below this many source points (align_enqueue)
ndt_status enqueue_source_order(ndt_ctx* c, const float T[16]) {
    c->pass_src = c->source.p;
    const int n = c->N;
    if (!c->opt.order_source || n < kOrderMinPoints) return NDT_OK;
    TRY(ensure(c, c->source_ord, geom_points(n)));
    TRY(ensure(c, c->ord_k0, n)); TRY(ensure(c, c->ord_v0, n)); TRY(ensure(c, c->ord_k1, n)); TRY(ensure(c, c->ord_v1, n));
    const int items = radix_items(c, n);
    const int nb_sort = std::max(1, ceil_div(n, kBlock * items));
    TRY(ensure(c, c->s.radix_aux, kRadixAuxWords));
    TRY(ensure(c, c->s.radix_status, radix_status_words(nb_sort)));
    Mat4f Tm;
    std::memcpy(Tm.m, T, sizeof(Tm.m));
    HIPCHK(c, hipMemsetAsync(c->s.radix_aux.p, 0, kRadixAuxWords * sizeof(int), c->stream.get()));
    const int nb_keys = grid_for(n, kBlock, 1024);
    hipLaunchKernelGGL(k_src_keys, dim3(nb_keys), dim3(kBlock), 0, c->stream.get(), c->source.p, n, Tm, c->d_hdr.p, c->ord_k0.p, c->ord_v0.p,
                       c->s.radix_aux.p, c->s.radix_status.p, (int)radix_status_words(nb_sort));
    const int passes = radix_launch_passes(c);
    for (int pass = 0; pass < passes; ++pass)
        launch_radix_pass(c, main_lane(c), items, nb_sort, c->ord_k0.p, c->ord_v0.p, c->ord_k1.p, c->ord_v1.p, n, pass, c->d_hdr.p, c->d_hdr.p,
                          passes - 1);
    hipLaunchKernelGGL(k_src_gather, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, c->stream.get(), c->source.p,
                       c->ord_v0.p, c->ord_v1.p, c->d_hdr.p, c->source_ord.p, n);
    HIPCHK(c, hipGetLastError());
    c->pass_src = c->source_ord.p;
    return NDT_OK;
}

// Waits for the read-back of round `seq`: spins on the sequence word k_readback releases last (a stream
// synchronisation sleeps on the completion interrupt and wakes tens of microseconds after the GPU is done); a device
// error still surfaces through the periodic stream query.  NDT_SPIN_WAIT=0 synchronises the stream instead (A/B).
ndt_status wait_readback(ndt_ctx* c, unsigned long long seq) {
    const volatile unsigned long long* w = c->h_rb.get();
    for (unsigned it = 1;; ++it) {
        if (*w == seq) break;
        if ((it & 1023u) == 0) {
            const hipError_t e = hipStreamQuery(c->stream.get());
            if (e == hipSuccess) {
                if (*w == seq) break;
                return fail(c, NDT_EDEVICE, "align read-back missing after the stream finished");
            }
            if (e != hipErrorNotReady) return fail(c, NDT_EDEVICE, std::string("align: ") + hipGetErrorString(e));
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return NDT_OK;
}

// An align in two halves: align_enqueue queues the initial state and the first round of the pass chain (a graph of
// last_passes+1 passes, which normally covers the whole align) with the read-back of the final state, without waiting;
// align_finish waits, runs any further rounds (slow convergence, SVD fallback) synchronously and records timings.
// ndt_align = both back to back; ndt_align_async / ndt_align_wait and the batched replay keep several contexts
// (streams) in flight.
ndt_status align_enqueue(ndt_ctx* c, const float guess[16]) {
    TRY(ensure_align_buffers(c));
    std::memcpy(c->al_guess, guess, sizeof(c->al_guess));
    init_state(c, guess, c->h_state.get());
    const bool mt = c->h_state->mt_possible != 0;
    // Newton-only chains: the first round covers the previous align's pass count + 1 (scan-to-scan replay converges
    // in a similar number of iterations), continuation rounds 8 passes; passes queued after convergence exit at
    // once but still cost a launch each.  More-Thuente chains (4 passes per slot possible) keep 16-slot rounds.
    // leading-tail chain (ndt_set_pass_options(lead_tail = 0): last-workgroup tails) whenever the align runs direct passes only
    // Used where the align is latency-bound: one registration at a time (not the batched replay, where the other
    // streams' bodies fill the CUs a last-workgroup tail leaves idle: C4 1437 vs 1156 pairs/s) and below kLeadMaxPoints
    // source points (C5's 1 M-point passes are body-bound: 227.7 vs 225.3 scans/s); C2 954 -> 1022, C3 2219 -> 2334.
    // ndt_set_pass_options(lead_tail = 0) forces last-workgroup tails (tests/test_gpu_lead.py compares the two chains)
    c->lead = (c->opt.lead_tail && !c->no_lead && c->N < kLeadMaxPoints && needs_direct(c->prm) && !needs_radius(c->prm, mt)) ? 1 : 0;
    c->lead_par = 0;
    // a leading-tail chain needs one kernel more than it has passes (the last pass's step runs in the next kernel)
    const int full = mt ? 16 : c->prm.max_iter + 3 + c->lead;
    int slots = full;
    if (!mt && c->last_passes > 0) slots = std::min(full, std::max(3, c->last_passes + 1 + c->lead));
    if (c->opt.profiling) TRY(ensure(c, c->prof.ts, kTsStride * (size_t)c->hist_cap));
    {
        // state upload + ticket reset (+ stamp reset) + the align's start stamp as one launch; the state is passed by
        // value (kernel argument)
        const int ts_words = c->opt.profiling ? kTsStride * c->hist_cap : 0;
        // + the source copy ndt_set_source_device deferred (four 16-byte words per thread and round; a source that is not
        // 16-byte aligned is copied by copy16 first)
        if (c->src_pend && (reinterpret_cast<uintptr_t>(c->src_pend) & 15)) TRY(flush_source(c));
        const long long cp_words = c->src_pend ? (long long)c->N : 0;
        const int nb = std::max({1, std::min(256, ceil_div(ts_words, kBlock)), (int)std::min<long long>(1024, ceil_div(cp_words, 4LL * kBlock))});
        const uint4* cp_src = reinterpret_cast<const uint4*>(c->src_pend);
        c->src_pend = nullptr;
        c->al_seq = ++c->rb_seq;
        c->lanes.marked = 0;  // a side-lane mark not taken before this align is dropped
        hipLaunchKernelGGL(k_align_init, dim3(nb), dim3(kBlock), 0, c->stream.get(), *c->h_state, c->d_state.p, c->counter.p,
                           c->opt.profiling ? c->prof.ts.p : nullptr, ts_words, c->d_clk.p, c->grid_valid ? c->d_hdr.p : nullptr, c->al_seq,
                           cp_src, reinterpret_cast<uint4*>(c->source.p), cp_words);
        HIPCHK(c, hipGetLastError());
    }
    TRY(enqueue_source_order(c, c->h_state->T));
    TRY(launch_chain(c, slots, mt, true));  // the round's read-back is the graph's last node
    c->lead_par += slots;
    c->al_inflight = true;
    c->al_mt = mt;
    c->al_full = full;
    c->al_slots = slots;
    return NDT_OK;
}

ndt_status align_finish_once(ndt_ctx* c) {
    if (!c->al_inflight) return fail(c, NDT_EINVAL, "no align in flight");
    c->al_inflight = false;
    const bool mt = c->al_mt;
    const int full = c->al_full;
    int slots = c->al_slots;
    int hist_before = 0;
    int rounds = 0;
    const int max_rounds = 1 + (c->prm.max_iter + 3) * 12 / 3 + 4 + 64;
    for (;;) {
        TRY(wait_readback(c, c->al_seq));
        ++rounds;
        if (c->opt.profiling) TRY(collect_pass_times(c, hist_before));
        if (c->h_state->done || rounds >= max_rounds) break;
        if (!mt) slots = std::min(full, 8);
        if (c->h_state->needs_svd) {
            hipLaunchKernelGGL(k_svd_resume, dim3(1), dim3(kBlock), 0, c->stream.get(), lead_state(c, 0));
            HIPCHK(c, hipGetLastError());
        }
        hist_before = std::min(c->h_state->hist_count, c->hist_cap);
        TRY(launch_chain(c, slots, mt));
        TRY(enqueue_readback(c, hist_before, hist_before + slots * (mt ? 4 : 1), lead_state(c, slots)));
        c->lead_par += slots;
    }
    c->ms_align = (double)(c->h_rb[2] - c->h_rb[1]) * 1e-5;  // 100 MHz device clock: k_align_init .. last read-back
    // a build queued since the previous align: its start (k_minmax) .. this align's start (100 MHz device clock)
    if (c->built_since_align && c->h_rb[1] > c->h_rb[3]) c->ms_build = (double)(c->h_rb[1] - c->h_rb[3]) * 1e-5;
    c->built_since_align = false;
    c->grid_cells_seen = std::max(c->grid_cells_seen, c->h_state->grid_cells);
    c->have_result = true;
    c->icp.last = false;
    c->align_tgt_gen = c->tgt_gen;
    c->last_passes = c->h_state->n_passes;
    if (!c->h_state->done) return fail(c, NDT_EDEVICE, "align did not finish within the slot budget");
    // the target build's error bits (GridHeader::pad[0]): latched by k_align_init for the build queued ahead of the align,
    // and read again by the last read-back (the align's own source-order sort reports into the same header)
    c->al_berr = c->h_state->build_error | (int)c->h_rb[4];
    if (!c->al_berr) {
        c->build_unchecked = false;
        note_grid_width(c, c->h_state->grid_cells, c->target_dense);
    }
    return NDT_OK;
}

// align_finish_once, and after a flagged target build: the build re-run and the align with it (same guess, same source)
ndt_status align_finish(ndt_ctx* c) {
    TRY(align_finish_once(c));
    if (!c->al_berr) return NDT_OK;
    const int berr = c->al_berr;
    TRY(rerun_build(c, berr));
    // the re-run align sorts its source against the new grid (enqueue_source_order) before any read-back of that grid
    // could renew the radix prediction: all four passes for that sort too.  Once this align has read the grid back the
    // prediction follows it again (note_grid_width in align_finish_once).
    c->rerun_full = true;
    ndt_status st = align_enqueue(c, c->al_guess);
    c->rerun_full = false;
    TRY(st);
    TRY(align_finish_once(c));
    if (c->al_berr)
        return fail(c, NDT_EDEVICE, std::string("target build failed twice (error bits ") + std::to_string(berr) + ", " +
                                        std::to_string(c->al_berr) + ")");
    return NDT_OK;
}

ndt_status run_align(ndt_ctx* c, const float guess[16]) {
    TRY(align_enqueue(c, guess));
    return align_finish(c);
}

void fill_result(ndt_ctx* c, ndt_result* out) {
    const AlignState* st = c->h_state.get();
    for (int k = 0; k < 16; ++k) out->final_tf[k] = st->T[k];
    out->nr_iterations = st->nr_iterations;
    out->converged = st->converged;
    out->trans_probability = st->trans_probability;
    out->score = st->score;
    out->n_passes = st->n_passes;
    out->n_pairs = st->pairs_total;
    out->solver_fallbacks = st->solver_fallbacks;
}

static ndt_status single_pass(ndt_ctx* c, const double p[6], const float T[16], int kind, bool force_radius, double* res44) {
    TRY(need_target_and_source(c));
    TRY(set_dev(c));
    if (!c->grid_valid) TRY(build_target(c));
    TRY(settle_build(c));
    TRY(flush_source(c));
    TRY(ensure_align_buffers(c));
    TRY(ensure(c, c->reduce_out, kNumAcc));
    c->pass_src = c->source.p;
    AlignState* st = c->h_state.get();
    init_state(c, T, st);
    for (int k = 0; k < 16; ++k) st->T[k] = T[k];
    for (int k = 0; k < 6; ++k) { st->p[k] = p[k]; st->x_eval[k] = p[k]; st->x_t[k] = p[k]; }
    angle_tables(p, st->jang, st->hang, st->jang_d, st->hang_d);
    st->pass_kind = kind;
    st->pending = 1;
    HIPCHK(c, hipMemcpyAsync(c->d_state.p, st, sizeof(AlignState), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipMemsetAsync(c->counter.p, 0, kPassCounterWords * sizeof(unsigned), c->stream.get()));
    if (kind == PASS_HESS || force_radius || !needs_direct(c->prm)) launch_radius(c, 1);
    else launch_pass(c, 1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(res44, c->reduce_out.p, kNumAcc * sizeof(double), hipMemcpyDeviceToHost, c->stream.get()));
    // the target's cell count sizes the next dense grid, as an align's read-back does (align_finish)
    long long cells = 0;
    HIPCHK(c, hipMemcpyAsync(&cells, &c->d_hdr.p->cells, sizeof(cells), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    c->grid_cells_seen = std::max(c->grid_cells_seen, cells);
    c->have_result = false;
    return NDT_OK;
}

}  // namespace

}  // namespace ndt::host

extern "C" {

ndt_status ndt_set_source(ndt_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
    if (!c || (n && !xyz) || stride_bytes < 12 || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad source");
    TRY(set_dev(c));
    const float4* old = c->source.p;
    TRY(main_after_fit(c, true));  // a fitness query may still read the source
    TRY(ensure(c, c->source, geom_points((int)n)));
    c->src_pend = nullptr;  // replaced before it was copied
    TRY(upload_points(c, c->source, xyz, n, stride_bytes));
    if (c->source.p != old) invalidate_graph(c);  // a new size alone keeps the chains (geom_points)
    c->N = (int)n;
    c->has_source = true;
    ++c->src_gen;
    c->have_result = false;
    return NDT_OK;
}

ndt_status ndt_set_source_device(ndt_ctx* c, const float* d_xyz4, size_t n) {
    if (!c || (n && !d_xyz4) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad source");
    TRY(set_dev(c));
    const float4* old = c->source.p;
    TRY(main_after_fit(c, true));  // a fitness query may still read the source
    TRY(ensure(c, c->source, geom_points((int)n)));
    if (c->source.p != old) invalidate_graph(c);  // a new size alone keeps the chains (geom_points)
    // the copy is deferred: the next align does it in its k_align_init (one launch less), any other reader of the source
    // first (flush_source); stream order is unchanged (nothing between reads the ctx source)
    c->src_pend = n ? reinterpret_cast<const float4*>(d_xyz4) : nullptr;
    c->N = (int)n;
    c->has_source = true;
    ++c->src_gen;
    c->have_result = false;
    return NDT_OK;
}

ndt_status ndt_align(ndt_ctx* c, const float guess[16], ndt_result* out) {
    if (!c || !guess || !out) return fail(c, NDT_EINVAL, "null argument");
    TRY(need_target_and_source(c));
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    TRY(set_dev(c));
    if (!c->grid_valid) TRY(build_target(c));
    TRY(run_align(c, guess));
    fill_result(c, out);
    return NDT_OK;
}

ndt_status ndt_get_output(ndt_ctx* c, float* xyz, size_t stride_bytes) {
    if (!c || !xyz || stride_bytes < 12) return fail(c, NDT_EINVAL, "bad output");
    if (!c->have_result) return fail(c, NDT_EINVAL, "no align result");
    TRY(set_dev(c));
    TRY(flush_source(c));
    TRY(ensure(c, c->out_cloud, c->N));
    if (c->icp.last) {
        // an ICP align: the source transformed by its final transformation (PCL returns the cloud it transformed
        // cumulatively, iteration by iteration: the same points up to f32 rounding)
        Mat4f Tm;
        for (int k = 0; k < 16; ++k) Tm.m[k] = c->icp.final_tf[k];
        hipLaunchKernelGGL(k_transform_mat, dim3(std::max(1, ceil_div(c->N, kBlock))), dim3(kBlock), 0, c->stream.get(), c->source.p, c->N, Tm,
                           c->out_cloud.p);
    } else
    hipLaunchKernelGGL(k_transform, dim3(std::max(1, ceil_div(c->N, kBlock))), dim3(kBlock), 0, c->stream.get(), c->source.p, c->N, c->d_state.p,
                       c->out_cloud.p);
    std::vector<float4> tmp(c->N);
    if (c->N) HIPCHK(c, hipMemcpyAsync(tmp.data(), c->out_cloud.p, c->N * sizeof(float4), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    char* base = reinterpret_cast<char*>(xyz);
    for (int i = 0; i < c->N; ++i) {
        float* f = reinterpret_cast<float*>(base + (size_t)i * stride_bytes);
        f[0] = tmp[i].x; f[1] = tmp[i].y; f[2] = tmp[i].z;
    }
    return NDT_OK;
}

ndt_status ndt_get_history(ndt_ctx* c, ndt_pass_record* out, int cap, int* n_out) {
    if (!c || !n_out || (cap > 0 && !out)) return fail(c, NDT_EINVAL, "bad history args");
    TRY(set_dev(c));
    const int n = std::min(std::min(c->h_state->hist_count, c->hist_cap), std::max(cap, 0));
    std::vector<PassRecordDev> tmp(n);
    if (n) HIPCHK(c, hipMemcpy(tmp.data(), c->d_hist.p, n * sizeof(PassRecordDev), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; ++i) {
        out[i].kind = tmp[i].kind;
        out[i].newton_iter = tmp[i].newton_iter;
        for (int k = 0; k < 6; ++k) { out[i].x[k] = tmp[i].x[k]; out[i].g[k] = tmp[i].g[k]; }
        out[i].score = tmp[i].score;
        for (int k = 0; k < 36; ++k) out[i].H[k] = tmp[i].H[k];
        out[i].pairs = tmp[i].pairs;
    }
    *n_out = std::min(c->h_state->hist_count, c->hist_cap);
    return NDT_OK;
}

ndt_status ndt_derivatives(ndt_ctx* c, const double p[6], const float T[16], int compute_hessian, double* score, double g[6], double H[36],
                           long long* pairs) {
    if (!c || !p || !T) return fail(c, NDT_EINVAL, "null argument");
    double r[kNumAcc];
    TRY(single_pass(c, p, T, compute_hessian ? PASS_FULL : PASS_GRAD, false, r));
    if (score) *score = r[0];
    if (g) for (int k = 0; k < 6; ++k) g[k] = r[1 + k];
    if (H) for (int k = 0; k < 36; ++k) H[k] = r[7 + k];
    if (pairs) *pairs = (long long)r[43];
    return NDT_OK;
}

ndt_status ndt_hessian_radius(ndt_ctx* c, const double p[6], const float T[16], double H[36], long long* pairs) {
    if (!c || !p || !T) return fail(c, NDT_EINVAL, "null argument");
    double r[kNumAcc];
    TRY(single_pass(c, p, T, PASS_HESS, true, r));
    if (H) for (int k = 0; k < 36; ++k) H[k] = r[7 + k];
    if (pairs) *pairs = (long long)r[43];
    return NDT_OK;
}

ndt_status ndt_calculate_score(ndt_ctx* c, const float T[16], double* out) {
    if (!c || !T || !out) return fail(c, NDT_EINVAL, "null argument");
    TRY(need_target_and_source(c));
    TRY(set_dev(c));
    if (!c->grid_valid) TRY(build_target(c));
    TRY(settle_build(c));
    TRY(flush_source(c));
    const int nb = grid_for(c->N, kBlock, 1024);
    TRY(ensure(c, c->score_part, nb));
    Mat4f Tm;
    for (int k = 0; k < 16; ++k) Tm.m[k] = T[k];
    const double d1 = c->gauss_cur[0], d2 = c->gauss_cur[1], d3 = c->gauss_cur[2];
    hipLaunchKernelGGL(k_score_radius, dim3(nb), dim3(kBlock), 0, c->stream.get(), c->source.p, c->N, Tm, c->d_hdr.p, c->table.p, c->grid.p,
                       c->recs.p, c->cent.p, c->icovd.p, d1, d2, d3, c->prm.resolution, c->score_part.p);
    HIPCHK(c, hipGetLastError());
    std::vector<double> part(nb);
    HIPCHK(c, hipMemcpyAsync(part.data(), c->score_part.p, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    double score = 0.0;
    for (int b = 0; b < nb; ++b) score += part[b];
    *out = score / (double)c->N;
    return NDT_OK;
}

ndt_status ndt_align_async(ndt_ctx* c, const float guess[16]) {
    if (!c || !guess) return fail(c, NDT_EINVAL, "null argument");
    TRY(need_target_and_source(c));
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an align is already in flight on this context");
    TRY(set_dev(c));
    if (!c->grid_valid) TRY(build_target(c));
    return align_enqueue(c, guess);
}

ndt_status ndt_align_wait(ndt_ctx* c, ndt_result* out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    TRY(align_finish(c));
    fill_result(c, out);
    return NDT_OK;
}

// Batched offline replay on this device: pairs round-robin over the context and its helper contexts (one HIP stream
// each, three in flight), every context keeping one registration in flight, so that one pair's target
// build and pass-kernel tails overlap another pair's passes.  Each pair runs exactly the code of a single align:
// results are bit-identical to registering the pairs one by one.
ndt_status ndt_align_batch(ndt_ctx* c, const ndt_pair_desc* pairs, int n_pairs, ndt_result* out) {
    if (!c || (n_pairs > 0 && (!pairs || !out))) return fail(c, NDT_EINVAL, "bad batch");
    TRY(set_dev(c));
    // three registrations in flight (measured on C4 pairs: 2 streams 1257, 3 streams 1385, 4 streams 1193 pairs/s — the
    // 4th stream competes for the process's 4 hardware queues and the pass bodies already fill every CU)
    int streams = 3;
    if (const char* e = std::getenv("NDT_BATCH_STREAMS")) streams = std::max(1, std::min(16, std::atoi(e)));  // A/B runs
    streams = std::max(1, std::min(streams, n_pairs));
    while ((int)c->helpers.size() < streams - 1) {
        ndt_ctx* h = nullptr;
        ndt_params p = c->prm;
        p.device = c->device;
        TRY(ndt_create(&p, &h));
        c->helpers.push_back(h);
    }
    std::vector<ndt_ctx*> ctxs(1, c);
    for (int k = 0; k < streams - 1; ++k) {
        ndt_ctx* h = c->helpers[k];
        h->prm = c->prm;
        hand_options(h, c);  // a helper created after ndt_set_pass_options / ndt_set_build_options gets them too
        ctxs.push_back(h);
    }
    // every registration in flight spreads its passes over all CUs (spreading each over n_cu / streams CUs was
    // measured neutral) and keeps last-workgroup tails (the other streams' bodies fill the CUs a tail leaves idle)
    for (ndt_ctx* x : ctxs) x->no_lead = streams > 1;
    std::vector<int> slot_pair(streams, -1);
    ndt_status rs = NDT_OK;
    auto drain = [&](int k) -> ndt_status {
        if (slot_pair[k] < 0) return NDT_OK;
        ndt_status st = ndt_align_wait(ctxs[k], &out[slot_pair[k]]);
        if (st != NDT_OK && ctxs[k] != c) c->err = ctxs[k]->err;
        slot_pair[k] = -1;
        return st;
    };
    for (int i = 0; i < n_pairs && rs == NDT_OK; ++i) {
        const int k = i % streams;
        if ((rs = drain(k)) != NDT_OK) break;
        ndt_ctx* x = ctxs[k];
        if ((rs = ndt_set_target_device(x, pairs[i].d_target_xyz4, pairs[i].n_target, 1)) == NDT_OK &&
            (rs = ndt_set_source_device(x, pairs[i].d_source_xyz4, pairs[i].n_source)) == NDT_OK &&
            (rs = ndt_align_async(x, pairs[i].guess)) == NDT_OK)
            slot_pair[k] = i;
        if (rs != NDT_OK && x != c) c->err = x->err;
    }
    for (int k = 0; k < streams; ++k) {
        const ndt_status st = drain(k);
        if (rs == NDT_OK) rs = st;
    }
    c->no_lead = false;
    return rs;
}

}  // extern "C"
