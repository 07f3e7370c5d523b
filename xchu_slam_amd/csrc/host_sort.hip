// host_sort.hip — sort / scan plumbing of the host side: the single-pass scans, the radix passes and the
// bin-and-sort sequence every binning of the library runs (target build, VoxelGrid, nearest-neighbour index), and
// VoxelGrid's enqueue half (enqueue_voxel_grid).
#include "ndt_host.h"

namespace ndt::host {

// launch context of one single-pass scan over nb tiles (look-back words grown and zeroed on demand; the epoch tag
// makes words of earlier launches stale, so they are never cleared again)
ndt_status scan_ctx(ndt_ctx* c, Lane L, int nb, ScanCtx* sc) {
    sc->tickets = c->opt.tile_tickets ? 1 : 0;
    if ((size_t)nb > L.s.scan_status.cap) {
        TRY(ensure(c, L.s.scan_status, (size_t)nb));
        HIPCHK(c, hipMemsetAsync(L.s.scan_status.p, 0, L.s.scan_status.cap * sizeof(unsigned long long), L.st));
    }
    if (!L.s.scan_ticket.p) {
        TRY(ensure(c, L.s.scan_ticket, 1));
        HIPCHK(c, hipMemsetAsync(L.s.scan_ticket.p, 0, sizeof(unsigned long long), L.st));
        L.s.scan_tickets = 0;
    }
    sc->status = L.s.scan_status.p;
    sc->ticket = L.s.scan_ticket.p;
    sc->ticket_base = L.s.scan_tickets;
    sc->epoch = ++L.s.scan_epoch;
    sc->nb = nb;
    // the device counter advances only in ticket mode (each of the nb tiles takes one): the host copy must follow it
    // exactly, or a ctx switched to tickets after a look-back timeout computes negative tiles from a stale base
    if (sc->tickets) L.s.scan_tickets += (unsigned long long)nb;
    return NDT_OK;
}

// exclusive scan of n ints (n_dev optional device count), total written to total_out (device, optional):
// one single-pass kernel (decoupled look-back; a timed-out look-back raises herr's error flag)
ndt_status enqueue_scan(ndt_ctx* c, Lane L, const int* in, int n_host, const int* n_dev, int* out, int* total_out, GridHeader* herr) {
    const int nb = std::max(1, ceil_div(n_host, kTileKeys));
    ScanCtx sc;
    TRY(scan_ctx(c, L, nb, &sc));
    hipLaunchKernelGGL(k_scan_onepass, dim3(nb), dim3(kBlock), 0, L.st, in, n_host, n_dev, out, total_out, sc, herr);
    return NDT_OK;
}

// Radix tile size (keys per thread) for a sort of n keys: 16 (4096-key tiles) when there are at least as many tiles
// as CUs, else 4 (1024-key tiles: 4x the workgroups for a small sort); 24 (6144-key tiles, 24 keys per digit run of the
// staged scatter instead of 16) from 4 M keys: C5's 18.7 M-key target sort 117 -> 111 us per pass, while C2's ~2 M-key
// sorts lose 2 % with it (32: 256 VGPRs, one wave per SIMD, 156 us).
constexpr int kRadixWideKeys = 4 << 20;
int radix_items(const ndt_ctx* c, int n) {
    return ceil_div(n, kTileKeys) < c->n_cu ? 4 : (n >= kRadixWideKeys ? 24 : 16);
}
// look-back status words of a sort of nb tiles: [4 passes][nb tiles][256 digits], then the group totals of the two-level
// look-back, [4 passes][ceil(nb / 16) groups][256] (voxel_build.hip kGroupTiles); the key kernels clear all of them
size_t radix_status_words(int nb) { return (size_t)4 * 256 * ((size_t)nb + (size_t)ceil_div(nb, 16)); }
void launch_radix_pass(const ndt_ctx* c, Lane L, int items, int nb, int* k0, int* v0, int* k1, int* v1, int n, int pass,
                       const GridHeader* h, GridHeader* herr, int last_pass) {
    auto* kern = items == 4 ? k_radix_onesweep<4> : items == 16 ? k_radix_onesweep<16> : k_radix_onesweep<24>;
    hipLaunchKernelGGL(kern, dim3(nb), dim3(kBlock), 0, L.st, k0, v0, k1, v1, n, pass, h, L.s.radix_aux.p, L.s.radix_status.p, nb,
                       herr, last_pass, c->opt.tile_tickets ? 1 : 0);
}

// Radix passes a main-stream sort against the target grid launches (target build, merge-extended build, source order):
// a key of b bits needs ceil(b / 8); the host does not know b before the build ran (the box is reduced on the device), so
// it launches what the last grid read back needed with one bit of margin (radix_pred) — the fourth pass of C2's 23-bit
// keys was an empty launch (~5.5 us per build).  A key wider than predicted is flagged by the last launched pass and the
// build re-run with four (align_finish / settle_build).
int radix_launch_passes(const ndt_ctx* c) {
    if (c->rerun_full) return 4;
    return c->opt.radix_force > 0 ? std::min(c->opt.radix_force, 4) : c->radix_pred;
}
void note_grid_width(ndt_ctx* c, long long cells, int dense) {
    if (cells <= 0) return;
    const long long top = dense ? cells - 1 : cells;
    int bits = 0;
    while (bits < 31 && (top >> bits) != 0) ++bits;
    c->radix_pred = std::min(4, std::max(1, (bits + 1 + 7) / 8));
}

// keys -> stable sort -> segments on header h; leaves h->n_leaves, seg_start, sorted buffers
// cloud_span (target build): the cloud voxels' (>= min points) point ranges in ascending key order as well (k_cloud_scan)
// cloud_span != nullptr: the target build (lookup structure chosen and cleared by k_keys, header completed by k_cloud_scan)
ndt_status enqueue_bin_and_sort(ndt_ctx* c, Lane L, const float4* pts, int n, int dense, GridHeader* h, float leaf, int layout,
                                int binning, int2* cloud_span, int passes) {
    if (&L.s == &c->s && !cloud_span) c->inc_ok = false;  // another main-stream sort overwrites the target's sorted keys
    const int nb_mm = grid_for(n, 4 * kBlock, 1024);  // k_minmax: four points per thread per round
    TRY(ensure(c, L.s.mm, (size_t)nb_mm * 7));
    // small sorts (fewer 4096-key tiles than CUs) use 1024-key tiles: 4x the workgroups, a quarter of the latency
    const int items = radix_items(c, n);
    const int nb_sort = std::max(1, ceil_div(n, kBlock * items));
    // a target's sorted keys / indices get a quarter of headroom: a merge-extended target (enqueue_target_append) reads the
    // previous sort in place and needs room for the grown one
    const size_t n_kv = cloud_span ? (size_t)n + (size_t)n / 4 : (size_t)n;
    TRY(ensure(c, L.s.k0, n_kv)); TRY(ensure(c, L.s.v0, n_kv)); TRY(ensure(c, L.s.k1, n_kv)); TRY(ensure(c, L.s.v1, n_kv));
    TRY(ensure(c, L.s.radix_aux, kRadixAuxWords));
    TRY(ensure(c, L.s.radix_status, radix_status_words(nb_sort)));
    TRY(ensure(c, L.s.seg_start, (size_t)n + 1));
    // min/max partials (and the digit histograms cleared), then keys: every keys workgroup derives the header itself
    hipLaunchKernelGGL(k_minmax, dim3(nb_mm), dim3(kBlock), 0, L.st, pts, n, dense, L.s.mm.p, L.s.radix_aux.p,
                       cloud_span ? c->d_clk.p + 3 : nullptr, nullptr, nullptr, nullptr);
    const int nb_keys = grid_for(n, 4 * kBlock, 512);
    hipLaunchKernelGGL(k_keys, dim3(nb_keys), dim3(kBlock), 0, L.st, pts, n, dense, L.s.mm.p, nb_mm, h, leaf, c->prm.min_points_per_voxel,
                       c->prm.min_covar_eigvalue_mult, layout, binning, L.s.k0.p, L.s.v0.p, L.s.radix_aux.p, L.s.radix_status.p,
                       (int)radix_status_words(nb_sort), cloud_span ? c->grid.p : nullptr, (long long)c->grid.cap, cloud_span ? c->table.p : nullptr,
                       1LL << c->max_log2cap, nullptr, 0);
    for (int pass = 0; pass < passes; ++pass)
        launch_radix_pass(c, L, items, nb_sort, L.s.k0.p, L.s.v0.p, L.s.k1.p, L.s.v1.p, n, pass, h, h, passes - 1);
    const int nb_seg = std::max(1, ceil_div(n, kTileKeys));
    ScanCtx sc;
    TRY(scan_ctx(c, L, nb_seg, &sc));
    hipLaunchKernelGGL(k_seg_scan, dim3(nb_seg), dim3(kBlock), 0, L.st, L.s.k0.p, L.s.k1.p, n, h, L.s.seg_start.p, sc);
    if (cloud_span) {
        ScanCtx sc2;
        TRY(scan_ctx(c, L, nb_seg, &sc2));
        hipLaunchKernelGGL(k_cloud_scan, dim3(nb_seg), dim3(kBlock), 0, L.st, L.s.seg_start.p, n, h, cloud_span, sc2, c->max_log2cap);
    }
    return NDT_OK;
}

// pcl::VoxelGrid's enqueue half, on the lane's stream, scratch and header h: the n points binned and sorted by leaf, then
// the voxel means into out: gather into voxel order, one serial sum per voxel.  h ends with n_leaves, overflow and the
// sort's look-back flag (pad[0]) for the caller to read back.
ndt_status enqueue_voxel_grid(ndt_ctx* c, Lane L, const float4* in, int n, float leaf, GridHeader* h, float4* out) {
    TRY(enqueue_bin_and_sort(c, L, in, n, 1, h, leaf));
    TRY(ensure(c, L.s.sorted_pts, std::max(n, 1)));
    const int nb = grid_for(n, 4 * kBlock, 2048);  // four points per thread per round
    hipLaunchKernelGGL(k_sorted_gather, dim3(nb), dim3(kBlock), 0, L.st, in, L.s.v0.p, L.s.v1.p, h, L.s.sorted_pts.p, n);
    hipLaunchKernelGGL(k_downsample_finalize, dim3(std::max(1, ceil_div(n, kBlock))), dim3(kBlock), 0, L.st, L.s.sorted_pts.p,
                       L.s.seg_start.p, h, out);
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

}  // namespace ndt::host
