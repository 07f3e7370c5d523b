// host_front_end.hip — filter_node's front end on the device: cloud transform, VoxelGrid, and the scan filter
// (crop, VoxelGrid, outlier removal).  Also the two host steps other units share with the filter: VoxelGrid over device
// points (voxel_downsample_dev) and the stream compaction in its two halves (enqueue_compact4, compact4_count).
#include "ndt_host.h"

namespace ndt::host {

// pcl::VoxelGrid over n device points: the voxel means in out (room for n points), their count in *n_out; synchronises.
// what: the prefix of a look-back timeout's text.  NDT_EOVERFLOW leaves the input's copy in out and n in *n_out.
ndt_status voxel_downsample_dev(ndt_ctx* c, const float4* in, size_t n, float leaf, float4* out, size_t* n_out, const char* what) {
    TRY(enqueue_voxel_grid(c, main_lane(c), in, (int)n, leaf, c->d_hdr_ds.p, out));
    HIPCHK(c, hipMemcpyAsync(c->h_hdr.get(), c->d_hdr_ds.p, sizeof(GridHeader), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    if (c->h_hdr->pad[0]) return fail(c, NDT_EDEVICE, std::string(what) + ": radix look-back timed out");
    if (c->h_hdr->overflow) {
        // pcl::VoxelGrid: "Leaf size is too small for the input dataset" -> output = input copy
        HIPCHK(c, hipMemcpyAsync(out, in, n * sizeof(float4), hipMemcpyDeviceToDevice, c->stream.get()));
        *n_out = n;
        c->err = "voxel downsample: leaf size too small, output = input";
        return NDT_EOVERFLOW;
    }
    *n_out = (size_t)c->h_hdr->n_leaves;
    return NDT_OK;
}

// Stream compaction on the main stream, the enqueue half: the n points of in whose flag is set go to out in input order
// (scan of the flags into idx, k_compact4).  The kept count lands in the device word d_count; a look-back timeout of the
// scan is raised in herr->pad[0].
ndt_status enqueue_compact4(ndt_ctx* c, const float4* in, const int* flags, int* idx, int n, float4* out, int* d_count, GridHeader* herr) {
    TRY(enqueue_scan(c, main_lane(c), flags, n, nullptr, idx, d_count, herr));
    hipLaunchKernelGGL(k_compact4, dim3(grid_for(n, kBlock, 2048)), dim3(kBlock), 0, c->stream.get(), in, flags, idx, n, out);
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

// The read-back half, for a compaction whose count went to herr->pad[1]: flag and count in one copy into the pinned
// h_words[0..1], one synchronise.  A raised flag is cleared (only then) and fails the call with timeout_text.
ndt_status compact4_count(ndt_ctx* c, GridHeader* herr, int* h_words, const char* timeout_text) {
    HIPCHK(c, hipMemcpyAsync(h_words, &herr->pad[0], 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    if (!h_words[0]) return NDT_OK;
    (void)hipMemsetAsync(&herr->pad[0], 0, sizeof(int), c->stream.get());
    return fail(c, NDT_EDEVICE, timeout_text);
}

}  // namespace ndt::host

extern "C" {

ndt_status ndt_transform_device(ndt_ctx* c, const float T[16], const float* d_in4, size_t n, float* d_out4) {
    if (!c || !T || (n && (!d_in4 || !d_out4)) || n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "bad transform args");
    TRY(set_dev(c));
    if (n == 0) return NDT_OK;
    Mat4f Tm;
    for (int k = 0; k < 16; ++k) Tm.m[k] = T[k];
    hipLaunchKernelGGL(k_transform_mat, dim3(ceil_div((long long)n, kBlock)), dim3(kBlock), 0, c->stream.get(),
                       reinterpret_cast<const float4*>(d_in4), (int)n, Tm, reinterpret_cast<float4*>(d_out4));
    HIPCHK(c, hipGetLastError());
    return NDT_OK;
}

ndt_status ndt_voxel_downsample(ndt_ctx* c, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset, float leaf, float* out4,
                                size_t cap, size_t* n_out) {
    if (!c || (n && !xyzi) || !n_out || !xyzi_layout_ok(stride_bytes, intensity_offset) || !(leaf > 0.f) || n > 0x7fffffffULL)
        return fail(c, NDT_EINVAL, "bad downsample args");
    TRY(set_dev(c));
    *n_out = 0;
    if (n == 0) return NDT_OK;
    DevBuf<float4> in, outb;  // this call's temporaries
    const std::vector<float> tmp = pack_cloud4(xyzi, n, stride_bytes, intensity_offset);  // lives until the synchronise inside the call
    TRY(ensure(c, in, n)); TRY(ensure(c, outb, n));
    HIPCHK(c, hipMemcpyAsync(in.p, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
    const ndt_status rs = voxel_downsample_dev(c, in.p, n, leaf, outb.p, n_out);
    if (rs != NDT_OK && rs != NDT_EOVERFLOW) return rs;
    // the voxel means, or after an overflow the input copy
    const size_t m = std::min(cap, *n_out);
    if (m) HIPCHK(c, hipMemcpyAsync(out4, outb.p, m * sizeof(float4), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    return rs;
}

ndt_status ndt_voxel_downsample_device(ndt_ctx* c, const float* d_in4, size_t n, float leaf, float* d_out4, size_t* n_out) {
    if (!c || !n_out || (n && (!d_in4 || !d_out4)) || !(leaf > 0.f) || n > 0x7fffffffULL)
        return fail(c, NDT_EINVAL, "bad downsample args");
    TRY(set_dev(c));
    *n_out = 0;
    if (n == 0) return NDT_OK;
    return voxel_downsample_dev(c, reinterpret_cast<const float4*>(d_in4), n, leaf, reinterpret_cast<float4*>(d_out4), n_out);
}

// ---------------------------------------------------------------- filter_node front end
ndt_status ndt_filter_default_params(ndt_filter_params* out) {
    if (!out) return NDT_EINVAL;
    out->leaf = 0.5f;
    out->r_min = 1.0;
    out->r_max = 60.0;
    out->mean_k = 30;
    out->stddev_mul = 1.0;
    out->outlier_method = 0;
    out->ror_radius = 0.8;
    out->ror_min_neighbors = 5;
    return NDT_OK;
}

ndt_status ndt_filter_scan_device(ndt_ctx* c, const ndt_filter_params* prm, const float* d_in4, size_t n, float* d_out4, size_t* n_out) {
    if (!c || !prm || !n_out || (n && (!d_in4 || !d_out4 || d_in4 == d_out4)) || n > 0x7fffffffULL || !(prm->leaf > 0.f) ||
        prm->mean_k < 1 || prm->mean_k > 63 || !(prm->r_min < prm->r_max) || prm->outlier_method < 0 || prm->outlier_method > 1 ||
        (prm->outlier_method == 1 && !(prm->ror_radius > 0.0)))
        return fail(c, NDT_EINVAL, "bad filter args");
    TRY(set_dev(c));
    *n_out = 0;
    c->fe.nvox = 0;
    if (n == 0) return NDT_OK;
    const int N = (int)n;
    const float4* in = reinterpret_cast<const float4*>(d_in4);
    float4* out = reinterpret_cast<float4*>(d_out4);
    TRY(ensure(c, c->fe.flags, n)); TRY(ensure(c, c->fe.idx, n)); TRY(ensure(c, c->fe.crop, n));
    TRY(ensure(c, c->fe.ds, n)); TRY(ensure(c, c->fe.dist, n)); TRY(ensure(c, c->fe.thr, 4));
    // the two compactions (enqueue_compact4 / compact4_count) write their count to fe.d_hdr->pad[1] and raise a look-back
    // timeout in fe.d_hdr->pad[0] (its own header: the VoxelGrid build rewrites d_hdr_ds); both come back in one copy into
    // pinned memory
    GridHeader* hdr = c->fe.d_hdr.p;
    int* fw = c->h_async->fe_words;
    // 1. removeNaNFromPointCloud + range crop (filter_node.cpp:236-247), input order kept
    hipLaunchKernelGGL(k_crop_flags, dim3(grid_for(N, kBlock, 2048)), dim3(kBlock), 0, c->stream.get(), in, N, prm->r_min, prm->r_max,
                       c->fe.flags.p);
    TRY(enqueue_compact4(c, in, c->fe.flags.p, c->fe.idx.p, N, c->fe.crop.p, &hdr->pad[1], hdr));
    TRY(compact4_count(c, hdr, fw, "filter: crop compaction scan: look-back timed out"));
    const int m = fw[1];
    if (m == 0) return NDT_OK;
    // 2. VoxelGrid (filter_node.cpp:249-251); a leaf too small for the cloud leaves the cropped cloud itself, and the
    // filter carries on over it
    size_t n_vox = 0;
    const ndt_status vs = voxel_downsample_dev(c, c->fe.crop.p, (size_t)m, prm->leaf, c->fe.ds.p, &n_vox, "filter: VoxelGrid sort");
    if (vs != NDT_OK && vs != NDT_EOVERFLOW) return vs;
    const int nv = (int)n_vox;
    c->fe.nvox = n_vox;
    const int nbq = grid_for(nv, kBlock / 16, 16384);  // 16-lane team per query
    if (prm->outlier_method == 1) {
        // 3'. RadiusOutlierRemoval (filter_node.cpp:265-272): index cell just above the radius (one ring of cells)
        TRY(enqueue_nn_index(c, main_lane(c), c->fe.ds.p, nv, 1, (float)(1.01 * prm->ror_radius), c->fe.sor_ix));
        hipLaunchKernelGGL(k_ror_keep, dim3(nbq), dim3(kBlock), 0, c->stream.get(), c->fe.ds.p, nv, prm->ror_radius, prm->ror_min_neighbors,
                           c->fe.sor_ix.hdr.p, c->fe.sor_ix.blk.p, c->fe.sor_ix.off.p, c->fe.sor_ix.pts.p, c->fe.flags.p);
    } else {
        // 3. StatisticalOutlierRemoval (filter_node.cpp:253-263)
        if (nv <= prm->mean_k) {
            HIPCHK(c, hipMemcpyAsync(out, c->fe.ds.p, (size_t)nv * sizeof(float4), hipMemcpyDeviceToDevice, c->stream.get()));
            HIPCHK(c, hipStreamSynchronize(c->stream.get()));
            *n_out = (size_t)nv;
            return NDT_OK;
        }
        // k-NN index over the voxel-filtered cloud: base cell 3 leaves (the mean_k = 30 neighbours of a surface point lie
        // within the 3x3x3 cells around it on a 0.5 m grid)
        TRY(enqueue_nn_index(c, main_lane(c), c->fe.ds.p, nv, 1, 3.0f * prm->leaf, c->fe.sor_ix));
        if (prm->mean_k + 1 <= 32)
            hipLaunchKernelGGL(k_sor_knn<32>, dim3(nbq), dim3(kBlock), 0, c->stream.get(), c->fe.ds.p, nv, prm->mean_k, c->fe.sor_ix.hdr.p,
                               c->fe.sor_ix.blk.p, c->fe.sor_ix.off.p, c->fe.sor_ix.pts.p, c->fe.dist.p);
        else
            hipLaunchKernelGGL(k_sor_knn<64>, dim3(nbq), dim3(kBlock), 0, c->stream.get(), c->fe.ds.p, nv, prm->mean_k, c->fe.sor_ix.hdr.p,
                               c->fe.sor_ix.blk.p, c->fe.sor_ix.off.p, c->fe.sor_ix.pts.p, c->fe.dist.p);
        hipLaunchKernelGGL(k_sor_stats, dim3(1), dim3(kBlock), 0, c->stream.get(), c->fe.dist.p, nv, prm->stddev_mul, c->fe.thr.p);
        const int nbk = grid_for(nv, kBlock, 2048);
        hipLaunchKernelGGL(k_sor_keep, dim3(nbk), dim3(kBlock), 0, c->stream.get(), c->fe.dist.p, nv, c->fe.thr.p, c->fe.flags.p);
    }
    TRY(enqueue_compact4(c, c->fe.ds.p, c->fe.flags.p, c->fe.idx.p, nv, out, &hdr->pad[1], hdr));
    // the outlier filter's neighbour index (enqueue_nn_index: its own sort, header rewritten per build) flags its
    // look-back timeouts in sor_ix.hdr: the word rides with the compaction's read-back
    fw[2] = 0;
    HIPCHK(c, hipMemcpyAsync(&fw[2], &c->fe.sor_ix.hdr.p->pad[0], sizeof(int), hipMemcpyDeviceToHost, c->stream.get()));
    const ndt_status cs = compact4_count(c, hdr, fw, "filter: outlier compaction scan: look-back timed out");
    // the index's timeout is the one reported when both were raised; the compaction's flag has been cleared either way, or
    // the next call would report a stale timeout
    if (fw[2]) return fail(c, NDT_EDEVICE, "filter: outlier neighbour index sort: radix look-back timed out");
    TRY(cs);
    *n_out = (size_t)fw[1];
    return NDT_OK;
}

ndt_status ndt_filter_scan(ndt_ctx* c, const ndt_filter_params* prm, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset,
                           float* out4, size_t cap, size_t* n_out) {
    if (!c || !prm || !n_out || (n && (!xyzi || !out4)) || !xyzi_layout_ok(stride_bytes, intensity_offset) || n > 0x7fffffffULL)
        return fail(c, NDT_EINVAL, "bad filter args");
    TRY(set_dev(c));
    *n_out = 0;
    if (n == 0) return ndt_filter_scan_device(c, prm, nullptr, 0, nullptr, n_out);
    const std::vector<float> tmp = pack_cloud4(xyzi, n, stride_bytes, intensity_offset);  // lives until the synchronise inside the call
    TRY(ensure(c, c->fe.in, n)); TRY(ensure(c, c->fe.out, n));
    HIPCHK(c, hipMemcpyAsync(c->fe.in.p, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
    TRY(ndt_filter_scan_device(c, prm, reinterpret_cast<const float*>(c->fe.in.p), n, reinterpret_cast<float*>(c->fe.out.p), n_out));
    const size_t k = std::min(cap, *n_out);
    if (k) HIPCHK(c, hipMemcpy(out4, c->fe.out.p, k * sizeof(float4), hipMemcpyDeviceToHost));
    return NDT_OK;
}

ndt_status ndt_filter_last_stats(ndt_ctx* c, float* dist, size_t cap, size_t* n_voxel, double thr[3]) {
    if (!c || !n_voxel) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    *n_voxel = c->fe.nvox;
    const size_t k = std::min(cap, c->fe.nvox);
    if (dist && k) HIPCHK(c, hipMemcpy(dist, c->fe.dist.p, k * sizeof(float), hipMemcpyDeviceToHost));
    if (thr) {
        if (c->fe.thr.p) HIPCHK(c, hipMemcpy(thr, c->fe.thr.p, 3 * sizeof(double), hipMemcpyDeviceToHost));
        else thr[0] = thr[1] = thr[2] = 0.0;
    }
    return NDT_OK;
}

}  // extern "C"
