// host_isc.hip — Intensity Scan Context on a ctx (ISCGeneration of isc/ISCGeneration.{h,cpp}, pgo_node's loop_method 2):
// ndt_isc_*.  The database lives on the device; every launch goes to the ctx stream and only result records come back.
#include "ndt_host.h"

struct ndt_isc {
    ndt_ctx* c = nullptr;
    ndt_isc_params prm{};
    int size = 0;
    SlotArrays mem;                  // the database's arrays
    IscDb db{nullptr, nullptr, nullptr, nullptr, nullptr};
    // pos_arr and travel_distance_arr (the prefix sum is sequential: accumulated here, the device gets the arrays)
    std::vector<double> pos, travel;
    DevBuf<unsigned> img;            // k_isc_make's merged cell image of the descriptor being added
    DevBuf<float4> pts;              // ndt_isc_add's upload
    DevBuf<int> d_query;             // ndt_isc_detect_batch's argument
    DevBuf<IscPartial> d_part;
    DevBuf<ndt_isc_result> d_res;
};

static bool isc_valid_params(const ndt_isc_params* p) {
    return p && p->rings >= 1 && p->rings <= kIscMaxRings && p->sectors >= kIscMinSectors && p->sectors <= kIscMaxSectors &&
           p->max_dis > 0.0 && std::isfinite(p->max_dis) && !std::isnan(p->skip_neighbour_distance) && !std::isnan(p->inflation_covariance) &&
           !std::isnan(p->geometry_threshold) && !std::isnan(p->intensity_threshold) && !std::isnan(p->z_min) && !std::isnan(p->z_max);
}

// Room for one more slot, as the Scan Context database grows (reserve_slots)
static ndt_status isc_reserve(ndt_isc* h, size_t need) {
    const size_t S = (size_t)h->prm.sectors, colb = S * kIscColBytes, maskb = S * sizeof(unsigned long long);
    TRY(reserve_slots(h->c, h->mem, (size_t)h->size, need, {colb, maskb, maskb, 3 * sizeof(double), sizeof(double)}, "ISC"));
    h->db = IscDb{h->mem.at<unsigned char>(0), h->mem.at<unsigned long long>(1), h->mem.at<unsigned long long>(2), h->mem.at<double>(3),
                  h->mem.at<double>(4)};
    return NDT_OK;
}

// makeAndSavedec's bookkeeping (:201-213): the position as a pcl::PointXYZI holds it, the travel distance so far; then
// the finalize launch that fills slot `size` (img == nullptr: its columns are in place)
static ndt_status isc_finish_add(ndt_isc* h, const unsigned* img, const double pos[3], int* index) {
    ndt_ctx* c = h->c;
    const double p[3] = {(double)(float)pos[0], (double)(float)pos[1], (double)(float)pos[2]};
    double travel = 0.0;
    if (h->size) {
        const double* b = &h->pos[(size_t)(h->size - 1) * 3];
        const double dx = b[0] - p[0], dy = b[1] - p[1], dz = b[2] - p[2];
        travel = h->travel.back() + std::sqrt((dx * dx + dy * dy) + dz * dz);
    }
    hipLaunchKernelGGL(k_isc_finalize, dim3(1), dim3(kIscBlock), 0, c->stream.get(), img, h->db, h->size, h->prm.rings, h->prm.sectors, p[0], p[1],
                       p[2], travel);
    HIPCHK(c, hipGetLastError());
    h->pos.insert(h->pos.end(), p, p + 3);
    h->travel.push_back(travel);
    if (index) *index = h->size;
    ++h->size;
    return NDT_OK;
}

static ndt_status isc_add_points(ndt_isc* h, const float4* d_pts, size_t n, const double pos[3], int* index) {
    ndt_ctx* c = h->c;
    if (n > 0x7fffffffULL) return fail(c, NDT_EINVAL, "cloud too large");
    TRY(isc_reserve(h, (size_t)h->size + 1));
    const size_t cells = (size_t)kIscMaxSectors * kIscColBytes;
    TRY(ensure(c, h->img, cells));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)h->img.p, 0, cells, c->stream.get()));
    if (n) {
        IscGeom g;
        g.rings = h->prm.rings;
        g.sectors = h->prm.sectors;
        g.max_dis = h->prm.max_dis;
        g.ring_step = h->prm.max_dis / h->prm.rings;
        g.sector_step = 2 * 3.14159265358979323846 / h->prm.sectors;
        g.z_min = h->prm.z_min;
        g.z_max = h->prm.z_max;
        const int nb = std::min(ceil_div((long long)n, kIscBlock * kIscMakePerThread), kIscMakeMaxBlocks);
        hipLaunchKernelGGL(k_isc_make, dim3(nb), dim3(kIscBlock), 0, c->stream.get(), d_pts, (int)n, g, h->img.p);
    }
    return isc_finish_add(h, h->img.p, pos, index);
}

static IscDetectArgs isc_args(const ndt_isc* h, int n_chunks, int pair_j, int pair_angle) {
    IscDetectArgs a;
    a.rings = h->prm.rings;
    a.sectors = h->prm.sectors;
    a.skip_distance = h->prm.skip_neighbour_distance;
    a.inflation = h->prm.inflation_covariance;
    a.geo_thres = h->prm.geometry_threshold;
    a.inten_thres = h->prm.intensity_threshold;
    a.n_chunks = n_chunks;
    a.pair_j = pair_j;
    a.pair_angle = pair_angle;
    return a;
}

// one detection submission over n queries (a device array, or the single q0): k_isc_detect over (queries, chunks of the largest
// query), k_isc_reduce, the records copied to out; synchronises once, at the end
static ndt_status isc_run(ndt_isc* h, const int* d_query, int q0, int q_max, int pair_j, int pair_angle, int n, ndt_isc_result* out) {
    ndt_ctx* c = h->c;
    const int n_chunks = pair_j >= 0 ? 1 : q_max / kIscChunk + 1;
    TRY(ensure(c, h->d_res, (size_t)n));
    TRY(ensure(c, h->d_part, (size_t)n * n_chunks));
    const IscDetectArgs a = isc_args(h, n_chunks, pair_j, pair_angle);
    hipLaunchKernelGGL(k_isc_detect, dim3(n, n_chunks), dim3(kIscBlock), 0, c->stream.get(), h->db, d_query, q0, a, h->d_part.p);
    hipLaunchKernelGGL(k_isc_reduce, dim3(ceil_div(n, kIscBlock)), dim3(kIscBlock), 0, c->stream.get(), (const IscPartial*)h->d_part.p, d_query, q0, n,
                       a, h->d_res.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, h->d_res.p, (size_t)n * sizeof(ndt_isc_result), hipMemcpyDeviceToHost, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    return NDT_OK;
}

extern "C" {

// init_param as pgo_node calls it (pgo_node.cpp:61-64) and the #defines of ISCGeneration.h:36-43; ground_filter's limits
ndt_status ndt_isc_default_params(ndt_isc_params* out) {
    if (!out) return NDT_EINVAL;
    out->rings = 60;
    out->sectors = 60;
    out->max_dis = 40.0;
    out->skip_neighbour_distance = 20.0;
    out->inflation_covariance = 0.03;
    out->geometry_threshold = 0.67;
    out->intensity_threshold = 0.91;
    out->z_min = -0.9f;
    out->z_max = 30.0f;
    return NDT_OK;
}

ndt_status ndt_isc_create(ndt_ctx* c, const ndt_isc_params* prm, ndt_isc** out) {
    if (!c || !out) return fail(c, NDT_EINVAL, "null argument");
    *out = nullptr;
    ndt_isc_params p;
    (void)ndt_isc_default_params(&p);
    if (prm) p = *prm;
    if (!isc_valid_params(&p)) return fail(c, NDT_EINVAL, "invalid ISC params (1 <= rings <= 64, 20 <= sectors <= 128, max_dis > 0)");
    ndt_isc* h = new ndt_isc();
    h->c = c;
    h->prm = p;
    *out = h;
    return NDT_OK;
}

void ndt_isc_destroy(ndt_isc* h) {
    if (!h) return;
    drain_for_destroy(h->c);
    delete h;
}

int ndt_isc_size(const ndt_isc* h) { return h ? h->size : -1; }

ndt_status ndt_isc_add_device(ndt_isc* h, const float* d_xyzi4, size_t n, const double pos[3], int* index) {
    if (!h) return NDT_EINVAL;
    if (!pos || (n && !d_xyzi4)) return fail(h->c, NDT_EINVAL, "null argument");
    TRY(set_dev(h->c));
    return isc_add_points(h, reinterpret_cast<const float4*>(d_xyzi4), n, pos, index);
}

ndt_status ndt_isc_add(ndt_isc* h, const float* xyzi, size_t n, size_t stride_bytes, int intensity_offset, const double pos[3], int* index) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (!pos || n > 0x7fffffffULL || (n && (!xyzi || !xyzi_layout_ok(stride_bytes, intensity_offset))))
        return fail(c, NDT_EINVAL, "bad cloud arguments");
    TRY(set_dev(c));
    TRY(ensure(c, h->pts, n));
    const std::vector<float> tmp = pack_cloud4(xyzi, n, stride_bytes, intensity_offset);
    if (n) HIPCHK(c, hipMemcpyAsync(h->pts.p, tmp.data(), n * sizeof(float4), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // tmp is free; the previous add has read h->pts
    return isc_add_points(h, h->pts.p, n, pos, index);
}

ndt_status ndt_isc_add_descriptor(ndt_isc* h, const unsigned char* bytes, const double pos[3], int* index) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (!bytes || !pos) return fail(c, NDT_EINVAL, "null argument");
    TRY(set_dev(c));
    TRY(isc_reserve(h, (size_t)h->size + 1));
    const int R = h->prm.rings, S = h->prm.sectors;
    std::vector<unsigned char> cols((size_t)S * kIscColBytes, 0);  // sector-major, each column zero-padded
    for (int q = 0; q < R; ++q)
        for (int p = 0; p < S; ++p) cols[(size_t)p * kIscColBytes + q] = bytes[(size_t)q * S + p];
    HIPCHK(c, hipMemcpyAsync(h->db.cols + (size_t)h->size * cols.size(), cols.data(), cols.size(), hipMemcpyHostToDevice, c->stream.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));  // cols is free
    return isc_finish_add(h, nullptr, pos, index);
}

ndt_status ndt_isc_detect(ndt_isc* h, ndt_isc_result* out) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (!out) return fail(c, NDT_EINVAL, "null argument");
    if (h->size == 0) return fail(c, NDT_EINVAL, "no descriptor stored");
    TRY(set_dev(c));
    return isc_run(h, nullptr, h->size - 1, h->size - 1, -1, -1, 1, out);
}

ndt_status ndt_isc_detect_batch(ndt_isc* h, const int* query, int n, ndt_isc_result* out) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (n < 0 || (n && (!query || !out))) return fail(c, NDT_EINVAL, "bad batch arguments");
    if (n == 0) return NDT_OK;
    int q_max = 0;
    for (int i = 0; i < n; ++i) {
        if (query[i] < 0 || query[i] >= h->size) return fail(c, NDT_EINVAL, "query outside the stored descriptors");
        q_max = std::max(q_max, query[i]);
    }
    TRY(set_dev(c));
    TRY(ensure(c, h->d_query, (size_t)n));
    HIPCHK(c, hipMemcpyAsync(h->d_query.p, query, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream.get()));
    return isc_run(h, h->d_query.p, 0, q_max, -1, -1, n, out);
}

ndt_status ndt_isc_pair(ndt_isc* h, int i, int j, double* geo, int* angle, double* inten, int* is_loop) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (i < 0 || j < 0 || i >= h->size || j >= h->size) return fail(c, NDT_EINVAL, "descriptor index out of range");
    TRY(set_dev(c));
    ndt_isc_result r;
    TRY(isc_run(h, nullptr, i, i, j, -1, 1, &r));
    if (geo) *geo = r.geo_score;
    if (angle) *angle = r.angle;
    if (inten) *inten = r.inten_score;
    if (is_loop) *is_loop = r.n_loop_pairs;
    return NDT_OK;
}

ndt_status ndt_isc_intensity(ndt_isc* h, int i, int j, int angle, double* inten) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (i < 0 || j < 0 || i >= h->size || j >= h->size) return fail(c, NDT_EINVAL, "descriptor index out of range");
    if (angle < 0 || angle >= h->prm.sectors) return fail(c, NDT_EINVAL, "column shift out of range");
    TRY(set_dev(c));
    ndt_isc_result r;
    TRY(isc_run(h, nullptr, i, i, j, angle, 1, &r));
    if (inten) *inten = r.inten_score;
    return NDT_OK;
}

ndt_status ndt_isc_get(ndt_isc* h, int index, unsigned char* bytes, double* pos, double* travel) {
    if (!h) return NDT_EINVAL;
    ndt_ctx* c = h->c;
    if (index < 0 || index >= h->size) return fail(c, NDT_EINVAL, "descriptor index out of range");
    TRY(set_dev(c));
    HIPCHK(c, hipStreamSynchronize(c->stream.get()));
    const size_t k = (size_t)index;
    const int R = h->prm.rings, S = h->prm.sectors;
    if (bytes) {
        std::vector<unsigned char> cols((size_t)S * kIscColBytes);
        HIPCHK(c, hipMemcpy(cols.data(), h->db.cols + k * cols.size(), cols.size(), hipMemcpyDeviceToHost));
        for (int q = 0; q < R; ++q)
            for (int p = 0; p < S; ++p) bytes[(size_t)q * S + p] = cols[(size_t)p * kIscColBytes + q];
    }
    if (pos) HIPCHK(c, hipMemcpy(pos, h->db.pos + k * 3, 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (travel) HIPCHK(c, hipMemcpy(travel, h->db.travel + k, sizeof(double), hipMemcpyDeviceToHost));
    return NDT_OK;
}

}  // extern "C"
