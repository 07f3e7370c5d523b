// host_prof.hip — the host side of pass profiling: the pinned copies k_readback fills, the decoding of an align's stamps
// into the context's statistics (ndt_stamps.h: accumulate_pass_stats), the profiling build's workgroup dump, and the
// three entry points that switch profiling and report it.  The launches that carry the stamp pointer stay in
// host_align.hip.
#include "ndt_host.h"

namespace ndt::host {

static_assert(blk_words(kBlkShape) == (size_t)kBlkPasses * kBlkMax * kBlkSlots, "one table shape for dbg_read_blk and the decoder");

// The pinned stamp and pass-record copies: both blocks or neither (hist_cap is fixed: made once)
ndt_status ensure_stamp_copies(ndt_ctx* c) {
    if (c->prof.h_ts) return NDT_OK;
    Pinned<unsigned long long[]> h_ts;
    Pinned<PassRecordDev[]> h_hist;
    TRY(make_pinned(c, h_ts, kTsStride * (size_t)c->hist_cap, hipHostMallocCoherent));
    TRY(make_pinned(c, h_hist, (size_t)c->hist_cap, hipHostMallocCoherent));
    c->prof.h_hist = std::move(h_hist);
    c->prof.h_ts = std::move(h_ts);
    return NDT_OK;
}

// NDT_BLK_DUMP=file (profiling build): every workgroup's body start and end (ticks from the pass stamp) and tile sums
// of pass NDT_BLK_DUMP_PASS (default 10), one line per workgroup, appended — the spread of the workgroups' finish times
// behind the means.  Only a pass whose workgroup rows gave a body sample is dumped.
static void dump_blk_pass(const StampView& v, int first, int count) {
    static const char* dump = getenv("NDT_BLK_DUMP");
    static const int dump_pass = getenv("NDT_BLK_DUMP_PASS") ? atoi(getenv("NDT_BLK_DUMP_PASS")) : 10;
    double mean[kWgPhases];
    if (!dump || dump_pass < first || dump_pass >= first + count || !wg_means(v, dump_pass, mean)) return;
    FILE* f = fopen(dump, "a");
    if (!f) return;
    const unsigned long long t0 = v.ts[kTsStride * (size_t)dump_pass + kTsEntry];
    for (int b = 0; b < std::min(v.nb, v.shape.rows); ++b) {
        const unsigned long long* e = v.blk + blk_row_at(v.shape.rows, dump_pass, b);
        if (e[kWgProbed] == 0 || e[kWgBodyEnd] < t0) continue;
        fprintf(f, "%d %llu %llu %llu %llu %llu\n", b, e[kWgBodyStart] > t0 ? e[kWgBodyStart] - t0 : 0ull, e[kWgBodyEnd] - t0,
                e[kWgSumProbe], e[kWgSumCompact], e[kWgSumPairs]);
    }
    fclose(f);
}

// The statistics of the passes this align ran since hist_before, from the rows k_readback copied (and, profiling build,
// the block table of the pass kernels' unit)
ndt_status collect_pass_times(ndt_ctx* c, int hist_before) {
    const int total = std::min(c->h_state->hist_count, c->hist_cap);
    const int ran = total - hist_before;
    if (ran <= 0 || !c->prof.h_ts) return NDT_OK;
    std::vector<unsigned long long> blk;
    if (kHaveBlkStamps) {
        blk.resize(blk_words(kBlkShape));
        if (dbg_read_blk(blk.data(), blk.size()) != hipSuccess) blk.clear();
    }
    const bool lead = c->lead != 0;
    const StampView v = {c->prof.h_ts.get(), blk.empty() ? nullptr : blk.data(), kBlkShape, c->prof.h_hist.get(), c->N,
                         direct_geom(pass_shape(c), lead).nb, lead};
    accumulate_pass_stats(v, hist_before, ran, c->prof.stats);
    if (v.blk) dump_blk_pass(v, hist_before, ran);
    return NDT_OK;
}

}  // namespace ndt::host

extern "C" {

ndt_status ndt_last_timings(ndt_ctx* c, double* ms_build, double* ms_align, double* ms_pass_avg, double* pass_bytes_avg) {
    if (!c) return NDT_EINVAL;
    if (ms_build) *ms_build = c->ms_build;
    if (ms_align) *ms_align = c->ms_align;
    // pass statistics over this ctx and the helper contexts of ndt_align_batch (the batch's other streams)
    double ms = c->prof.stats.ms_sum, bytes = c->prof.stats.bytes_sum;
    long long cnt = c->prof.stats.count;
    for (const ndt_ctx* h : c->helpers) {
        ms += h->prof.stats.ms_sum;
        bytes += h->prof.stats.bytes_sum;
        cnt += h->prof.stats.count;
    }
    if (ms_pass_avg) *ms_pass_avg = cnt ? ms / cnt : 0.0;
    if (pass_bytes_avg) *pass_bytes_avg = cnt ? bytes / cnt : 0.0;
    return NDT_OK;
}

// the columns of kPhaseNames (ndt_stamps.h)
ndt_status ndt_pass_phases(ndt_ctx* c, double ms[22]) {
    if (!c || !ms) return NDT_EINVAL;
    static_assert(kPassPhases + kWgPhases + kTailPhases == 22, "ndt_pass_phases' layout (NDT_HIP_ABI_VERSION)");
    const PassProf::Stats& ps = c->prof.stats;
    for (int q = 0; q < kPassPhases; ++q) ms[q] = ps.phase_count ? ps.phase_sum[q] / ps.phase_count : 0.0;
    for (int q = 0; q < kWgPhases; ++q) ms[kPassPhases + q] = ps.body_count ? ps.body_sum[q] / ps.body_count : 0.0;
    for (int q = 0; q < kTailPhases; ++q) ms[kPassPhases + kWgPhases + q] = ps.tail_count ? ps.tail_sum[q] / ps.tail_count : 0.0;
    return NDT_OK;
}

ndt_status ndt_set_profiling(ndt_ctx* c, int enable) {
    if (!c) return NDT_EINVAL;
    for (ndt_ctx* h : c->helpers) TRY(ndt_set_profiling(h, enable));
    c->opt.profiling = enable != 0;
    c->prof.stats = PassProf::Stats{};
    // no graph invalidation: the profiling flag and the stamp buffer are part of every graph's cache key, so a call
    // that only resets the statistics keeps the captured chains
    return NDT_OK;
}

}  // extern "C"
