// ndt_api.hip — C-ABI (include/ndt_hip.h) of the MI355X NDT library.
//
// Host-side mirror of pclomp::NormalDistributionsTransform's registration surface
// (ndt_omp.h:70-497 + pcl::Registration::align): setInputTarget -> device voxel build,
// setInputSource -> device copy, align -> device-resident Newton chain captured in a hipGraph.
// The host only prepares the initial state (guess -> p0, exactly ndt_omp_impl.hpp:89-104 in f32),
// launches, and reads back one small result record: one synchronisation per align.
// This unit: the context's life cycle and the small entry points; the rest of the host side is in host_*.hip.
#include "ndt_host.h"

static bool valid_params(const ndt_params* p) {
    return p && p->resolution > 0.f && std::isfinite(p->resolution) && p->max_iter >= 0 && p->search >= 0 && p->search <= 3 &&
           p->min_points_per_voxel >= 1 && p->precision_mode >= 0 && p->precision_mode <= 2;
}

// what every ctx holds from its creation on: the fixed-size device objects, their pinned counterparts, the target marker
static ndt_status create_buffers(ndt_ctx* c) {
    for (DevBuf<GridHeader>* h : {&c->d_hdr, &c->d_hdr_ds, &c->d_hdr_prev, &c->fe.d_hdr, &c->fit_ix.hdr, &c->fe.sor_ix.hdr}) TRY(ensure(c, *h, 1));
    HIPCHK(c, hipMemset(c->fe.d_hdr.p, 0, sizeof(GridHeader)));
    TRY(make_pinned(c, c->h_hdr, 1, hipHostMallocDefault));
    TRY(ensure(c, c->d_state, 1));
    TRY(ensure(c, c->d_state2, 1));
    TRY(make_pinned(c, c->h_state, 1, hipHostMallocCoherent));
    TRY(make_pinned(c, c->h_rb, 8, hipHostMallocCoherent));
    TRY(ensure(c, c->d_clk, 4));
    TRY(ensure(c, c->d_hist, c->hist_cap));
    TRY(ensure(c, c->d_async, 1));
    TRY(make_pinned(c, c->h_async, 1, hipHostMallocDefault));
    TRY(make_event(c, c->ev_tgt, hipEventDisableTiming));
    std::memset(c->h_state.get(), 0, sizeof(AlignState));
    std::memset(c->h_rb.get(), 0, 8 * sizeof(unsigned long long));
    return NDT_OK;
}

extern "C" {

ndt_status ndt_default_params(ndt_params* out) {
    if (!out) return NDT_EINVAL;
    out->resolution = 1.0f;
    out->step_size = 0.1;
    out->trans_eps = 0.1;
    out->outlier_ratio = 0.55;
    out->max_iter = 35;
    out->search = NDT_DIRECT7;
    out->min_points_per_voxel = 6;
    out->min_covar_eigvalue_mult = 0.01;
    out->precision_mode = 0;
    out->device = 0;
    return NDT_OK;
}

ndt_status ndt_create(const ndt_params* params, ndt_ctx** out) {
    if (!out) return NDT_EINVAL;
    *out = nullptr;
    ndt_params p;
    if (params) p = *params; else ndt_default_params(&p);
    if (!valid_params(&p)) return NDT_EINVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return NDT_EDEVICE;
    if (p.device < 0 || p.device >= ndev) return NDT_EINVAL;
    ndt_ctx* c = new ndt_ctx();
    c->prm = p;
    c->device = p.device;
    // the main stream (target build, align: a scan loop's critical path) at the highest priority, the side lanes
    // (getFitnessScore, keyframe insertion) at the lowest
    int prio_least = 0, prio_greatest = 0;
    if (hipSetDevice(c->device) != hipSuccess || hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess ||
        make_stream(c, c->stream, prio_greatest) != NDT_OK) {
        delete c;
        return NDT_EDEVICE;
    }
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device) == hipSuccess && n_cu > 0) c->n_cu = n_cu;
    if (const char* e = std::getenv("NDT_PPT")) c->opt.ppt = std::max(1, std::min(3, std::atoi(e)));  // A/B runs (pass geometry)
    gauss_constants(0.55, 1.0f, &c->gauss_cur[0], &c->gauss_cur[1], &c->gauss_cur[2]);
    if (create_buffers(c) != NDT_OK) {
        ndt_destroy(c);
        return NDT_ENOMEM;
    }
    *out = c;
    return NDT_OK;
}

ndt_status ndt_set_params(ndt_ctx* c, const ndt_params* p) {
    if (!c || !valid_params(p)) return fail(c, NDT_EINVAL, "invalid params");
    if (p->device != c->device) return fail(c, NDT_EINVAL, "device cannot change on an existing ctx");
    // pclomp::setResolution (ndt_omp.h:127-137): re-init the grid only when the resolution changed AND a
    // source is set; otherwise the grid keeps its leaf size until the next setInputTarget.
    const bool res_changed = p->resolution != c->prm.resolution;
    // the ndt_cpu backend (precision_mode 2) keeps its own cpu::VoxelGrid (division binning, its eigen solver): a
    // change between it and the pclomp/pcl grids rebuilds the target as a fresh setInputTarget would
    const bool grid_kind_changed = (p->precision_mode == 2) != (c->prm.precision_mode == 2);
    c->prm = *p;
    c->inc_ok = false;  // the next target is built from scratch under the new parameters
    invalidate_graph(c);
    if (c->has_target && ((res_changed && c->has_source) || grid_kind_changed)) {
        TRY(set_dev(c));
        TRY(build_target(c));
    }
    return NDT_OK;
}

ndt_status ndt_memcpy_d2d(ndt_ctx* c, void* d_dst, const void* d_src, size_t bytes) {
    if (!c || (bytes && (!d_dst || !d_src))) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    if (bytes) TRY(copy16(c, c->stream.get(), d_dst, d_src, bytes));
    return NDT_OK;
}

ndt_status ndt_device_alloc(ndt_ctx* c, size_t bytes, void** d_ptr) {
    if (!c || !d_ptr) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) return fail(c, NDT_ENOMEM, "hipMalloc failed");
    return NDT_OK;
}

ndt_status ndt_device_free(ndt_ctx* c, void* d_ptr) {
    if (!c) return NDT_EINVAL;
    TRY(set_dev(c));
    if (d_ptr) HIPCHK(c, hipFree(d_ptr));
    return NDT_OK;
}

ndt_status ndt_memcpy_h2d(ndt_ctx* c, void* d_dst, const void* h_src, size_t bytes) {
    if (!c || (bytes && (!d_dst || !h_src))) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    if (bytes) HIPCHK(c, hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return NDT_OK;
}

ndt_status ndt_memcpy_d2h(ndt_ctx* c, void* h_dst, const void* d_src, size_t bytes) {
    if (!c || (bytes && (!h_dst || !d_src))) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    if (bytes) HIPCHK(c, hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return NDT_OK;
}

ndt_status ndt_synchronize(ndt_ctx* c) {
    if (!c) return NDT_EINVAL;
    TRY(set_dev(c));
    TRY(flush_source(c));  // after a synchronize the caller may reuse the buffer it set as source
    // the side lanes' host threads first (every posted job issued; a job's failure stays for its result call)
    for (LaneWorker* w : {c->lanes.fit_worker.get(), c->lanes.ins_worker.get()}) if (w) (void)w->drain(nullptr);
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    if (c->lanes.fit_stream) HIPCHK(c, hipStreamSynchronize(c->lanes.fit_stream.get()));
    if (c->lanes.ins_stream) HIPCHK(c, hipStreamSynchronize(c->lanes.ins_stream.get()));
    return NDT_OK;
}

ndt_status ndt_set_pass_options(ndt_ctx* c, int lead_tail, int points_per_thread, int source_order) {
    if (!c || lead_tail < 0 || lead_tail > 1 || points_per_thread < 1 || points_per_thread > 3 || source_order < 0 ||
        source_order > 1)
        return fail(c, NDT_EINVAL, "bad pass options");
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    c->opt.lead_tail = lead_tail != 0;
    c->opt.ppt = points_per_thread;
    c->opt.order_source = source_order != 0;
    for (ndt_ctx* h : c->helpers) hand_options(h, c);
    return NDT_OK;
}

ndt_status ndt_pass_geometry(ndt_ctx* c, int which, int out[8]) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    if (!describe_pass(pass_shape(c), which, out)) return fail(c, NDT_EINVAL, "bad pass kernel index");
    return NDT_OK;
}

ndt_status ndt_set_build_options(ndt_ctx* c, int tile_tickets, int radix_passes) {
    if (!c || tile_tickets < 0 || tile_tickets > 1 || radix_passes < 0 || radix_passes > 4) return fail(c, NDT_EINVAL, "bad build options");
    if (c->al_inflight) return fail(c, NDT_EINVAL, "an asynchronous align is in flight (ndt_align_wait first)");
    c->opt.tile_tickets = tile_tickets != 0;
    c->opt.radix_force = radix_passes;
    for (ndt_ctx* h : c->helpers) h->opt = c->opt;  // tile_tickets = 0 clears a helper's sticky flag too
    return NDT_OK;
}

ndt_status ndt_build_stats(ndt_ctx* c, long long out[6]) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    out[0] = c->n_builds_full;
    out[1] = c->n_builds_merge;
    out[2] = c->n_builds_rerun;
    out[3] = c->n_rerun_lookback;
    out[4] = c->opt.tile_tickets ? 1 : 0;
    out[5] = radix_launch_passes(c);
    for (const ndt_ctx* h : c->helpers) {  // ndt_align_batch's helper contexts (their own streams and builds)
        out[0] += h->n_builds_full;
        out[1] += h->n_builds_merge;
        out[2] += h->n_builds_rerun;
        out[3] += h->n_rerun_lookback;
        out[4] += h->opt.tile_tickets ? 1 : 0;
    }
    return NDT_OK;
}

const char* ndt_last_error(const ndt_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int ndt_abi_version(void) { return NDT_HIP_ABI_VERSION; }

// Only what is about order; every resource is released by its owner when the ctx goes (member order: see ndt_ctx)
void ndt_destroy(ndt_ctx* c) {
    if (!c) return;
    for (ndt_ctx* h : c->helpers) ndt_destroy(h);
    c->helpers.clear();
    (void)hipSetDevice(c->device);
    c->lanes.fit_worker.reset();  // joins the side lanes' host threads after their queued jobs
    c->lanes.ins_worker.reset();
    for (hipStream_t st : {c->stream.get(), c->lanes.fit_stream.get(), c->lanes.ins_stream.get()}) if (st) (void)hipStreamSynchronize(st);
    invalidate_graph(c);
    c->icp.graph.exec.reset();
    c->gicp.graph.exec.reset();
    delete c;
}

}  // extern "C"
