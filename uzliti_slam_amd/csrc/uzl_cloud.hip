// uzl_cloud.hip — colour point-cloud registration: TYPE_3D_FULL edges by GICP-6D (host + C ABI uzl_cloud_*).
//
// Mirrors CloudTransformationEstimator::estimateEdgeImpl / estimateTransform (transformation_estimation/src/
// cloud_transformation_estimator.cpp:40-161) and GeneralizedIterativeClosestPoint6D (transformation_estimation/external/gicp6d/
// gicp6d.cpp); include/uzl_mi355x.h states the contract.  HBM layout as the laser store: append-only arrays of points (xyz f32,
// bgr u8, CIELAB f32, covariance f64 x 6), one record per cloud.  An estimate uploads the pairs, enqueues the prepare kernel and
// max_iterations x (search, step) launches in which the blocks of a finished pair exit at once, waits once, and finishes each
// result on the host: T_final^-1 T_diff, the score, the gates.
#include "cloud_types.hpp"
#include "laserline_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>

using namespace uzl;

struct uzl_cloud : HandleBase {
    uzl_cloud_cfg cfg;
    HandleStream stream;
    std::vector<CloudRec> clouds;
    int64_t n_points = 0;
    DevBuf<float> d_xyz, d_lab;
    DevBuf<uint8_t> d_bgr;
    DevBuf<double> d_cov;
    DevBuf<CloudRec> d_clouds;
    DevBuf<double> d_table;               // step 3's linearisation table, made by the host's libm at create
    // work, reused between calls
    PinBuf<uint8_t> h_work;
    DevBuf<CloudPairRec> d_pairs;
    DevBuf<CloudPairState> d_state;
    DevBuf<float> d_tgt, d_nn_d;
    DevBuf<int32_t> d_nn_j;
    DevBuf<double> d_M;
#ifdef UZL_DIAG
    DevBuf<CloudStepLog> d_log;
#endif
    // work of an add from images
    DevBuf<uint8_t> d_chunk, d_sort_temp;
    DevBuf<uint32_t> d_bbox, d_vals[2], d_flag, d_rank;
    DevBuf<int32_t> d_info;
    DevBuf<uint64_t> d_keys[2];
};

namespace {

int check_cfg(const uzl_cloud_cfg& c)
{
    const double pos[] = {c.leaf_size, c.gicp_epsilon, c.max_correspondence_dist, c.rotation_epsilon, c.transformation_epsilon};
    for (double v : pos) if (!(v > 0.) || !std::isfinite(v)) return UZL_ERR_BAD_ARG;
    const double nonneg[] = {c.lab_weight, c.min_score, c.max_translation, c.max_rotation_deg};
    for (double v : nonneg) if (!(v >= 0.) || !std::isfinite(v)) return UZL_ERR_BAD_ARG;
    if (!(c.z_min <= c.z_max)) return UZL_ERR_BAD_ARG;
    if (!(c.gicp_epsilon <= 1.)) return UZL_ERR_BAD_ARG;
    // step 4 scales n n^T by 1 - gicp_epsilon: where that rounds to 1 (below 2^-53), C of an exact plane is singular and M not finite
    if (!(1.0 - c.gicp_epsilon < 1.0)) return UZL_ERR_BAD_ARG;
    if (c.k_neighbours < kCloudMinPoints || c.k_neighbours > kCloudK) return UZL_ERR_BAD_ARG;
    if (c.max_iterations < 1 || c.max_iterations > UZL_CLOUD_MAX_ITERATIONS) return UZL_ERR_BAD_ARG;
    if (c.inner_iterations < 1 || c.inner_iterations > 100) return UZL_ERR_BAD_ARG;
    return UZL_OK;
}

int check_pair(uzl_cloud* h, const uzl_cloud_pair& p)
{
    const int32_t nc = (int32_t)h->clouds.size();
    if (p.cloud_from < 0 || p.cloud_from >= nc || p.cloud_to < 0 || p.cloud_to >= nc) return fail(h, UZL_ERR_BAD_ARG, "cloud index out of range");
    if (!h->clouds[p.cloud_from].k || !h->clouds[p.cloud_to].k) return fail(h, UZL_ERR_BAD_ARG, "a cloud with fewer points than k_neighbours has no covariances");
    if (!finite12(p.first_guess)) return fail(h, UZL_ERR_BAD_ARG, "non-finite first guess");
    return UZL_OK;
}

// Grow the store for `total` more points in `n` more clouds; the bookkeeping changes only in commit().
void reserve_store(uzl_cloud* h, int64_t total, int32_t n)
{
    hipStream_t st = h->stream;
    const size_t np = (size_t)std::max<int64_t>(h->n_points + total, 1);
    h->d_xyz.reserve(3 * np, true, st);
    h->d_lab.reserve(3 * np, true, st);
    h->d_bgr.reserve(3 * np, true, st);
    h->d_cov.reserve(6 * np, true, st);
    h->d_clouds.reserve(std::max<size_t>(h->clouds.size() + n, 1), true, st);
}

// Steps 3-4 over the points [n_points, n_points + total) that the caller has put into xyz and bgr, as the clouds `recs`.
void finish_append(uzl_cloud* h, const std::vector<CloudRec>& recs, int64_t total, int32_t* first_cloud)
{
    hipStream_t st = h->stream;
    const size_t have = h->clouds.size();
    int32_t max_n = 0;
    for (const CloudRec& r : recs) max_n = std::max(max_n, r.n);
    if (!recs.empty())
        UZL_HIP(hipMemcpyAsync(h->d_clouds.p + have, recs.data(), recs.size() * sizeof(CloudRec), hipMemcpyHostToDevice, st));
    launch_cloud_lab(h->d_bgr.p + 3 * h->n_points, h->d_lab.p + 3 * h->n_points, h->d_table.p, total, st);
    UZL_HIP(hipGetLastError());
    launch_cloud_cov(h->d_clouds.p + have, (int32_t)recs.size(), max_n, h->d_xyz.p, h->d_cov.p, h->cfg.k_neighbours, h->cfg.gicp_epsilon, st);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(st));
    if (first_cloud) *first_cloud = (int32_t)have;
    h->clouds.insert(h->clouds.end(), recs.begin(), recs.end());
    h->n_points += total;
}

size_t align16(size_t v) { return (v + 15) / 16 * 16; }

size_t color_image_bytes(const uzl_color_image& c) { return c.height <= 0 ? 0 : (size_t)(c.height - 1) * (size_t)c.step + 3 * (size_t)c.width; }

int check_colors(uzl_cloud* h, int32_t n, const uzl_depth_image* images, const uzl_color_image* colors)
{
    if (n > 0 && !colors) return fail(h, UZL_ERR_BAD_ARG, "null colour images");
    for (int32_t i = 0; i < n; i++) {
        const uzl_color_image& c = colors[i];
        if (c.width != images[i].width || c.height != images[i].height) return fail(h, UZL_ERR_BAD_ARG, "a colour image's size differs from its depth image's");
        if (c.encoding != UZL_COLOR_BGR8 && c.encoding != UZL_COLOR_RGB8) return fail(h, UZL_ERR_BAD_ARG, "unknown colour encoding");
        if (c.width > 0 && (!c.data || c.step < 3 * c.width || (int64_t)c.height * c.step > INT32_MAX))
            return fail(h, UZL_ERR_BAD_ARG, "a colour image without data, with a step smaller than a row, or height * step beyond 2^31");
    }
    return UZL_OK;
}

// Steps 1-4 over n checked image pairs; d_depth[i] != NULL (or d_depth == NULL for none): image i's f32 pixels are on the device
// already.  Nothing is stored unless every cloud is accepted.
int append_images(uzl_cloud* h, int32_t n, const uzl_depth_image* images, const float* const* d_depth, const uzl_color_image* colors,
                  int32_t* first_cloud)
{
    if ((int64_t)h->clouds.size() + n > INT32_MAX) return fail(h, UZL_ERR_BAD_ARG, "too many clouds");
    if (n == 0) { if (first_cloud) *first_cloud = (int32_t)h->clouds.size(); return UZL_OK; }
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t recs_bytes = align16((size_t)n * sizeof(CloudImageRec));
    size_t total_bytes = recs_bytes;
    int64_t n_pixels = 0;
    int32_t max_pixels = 0;
    for (int32_t i = 0; i < n; i++) {
        const bool on_device = d_depth && d_depth[i];
        total_bytes += align16(color_image_bytes(colors[i])) + (on_device ? 0 : align16(depth_image_bytes(images[i])));
        const int64_t px = (int64_t)images[i].width * images[i].height;
        n_pixels += px;
        max_pixels = (int32_t)std::max<int64_t>(max_pixels, px);
    }
    if (n_pixels > INT32_MAX) return fail(h, UZL_ERR_BAD_ARG, "more than 2^31 pixels in one call");
    h->h_work.reserve(std::max(total_bytes, (size_t)n * 8));
    h->d_chunk.reserve(total_bytes);
    uint8_t* w = h->h_work.p;
    CloudImageRec* recs = reinterpret_cast<CloudImageRec*>(w);
    size_t off = recs_bytes;
    int64_t pix = 0;
    for (int32_t i = 0; i < n; i++) {
        const uzl_depth_image& im = images[i];
        const uzl_color_image& c = colors[i];
        CloudImageRec& r = recs[i];
        r.pix_off = pix; r.width = im.width; r.height = im.height;
        r.fx = im.fx; r.fy = im.fy; r.cx = im.cx; r.cy = im.cy;
        r.color_step = c.step; r.swap_rb = c.encoding == UZL_COLOR_RGB8 ? 1 : 0;
        r.color = h->d_chunk.p + off;
        size_t nb = color_image_bytes(c);
        if (nb) memcpy(w + off, c.data, nb);
        off += align16(nb);
        if (d_depth && d_depth[i]) {
            r.depth = reinterpret_cast<const uint8_t*>(d_depth[i]); r.depth_step = 4 * im.width; r.encoding = UZL_DEPTH_F32_M;
        } else {
            r.depth = h->d_chunk.p + off; r.depth_step = im.step; r.encoding = im.encoding;
            nb = depth_image_bytes(im);
            if (nb) memcpy(w + off, im.data, nb);
            off += align16(nb);
        }
        pix += (int64_t)im.width * im.height;
    }
    UZL_HIP(hipMemcpyAsync(h->d_chunk.p, w, total_bytes, hipMemcpyHostToDevice, st));
    const size_t P = (size_t)std::max<int64_t>(n_pixels, 1);
    CloudVoxelWork vw{};
    vw.temp_bytes = cloud_voxel_temp_bytes(n_pixels, n);
    h->d_sort_temp.reserve(std::max<size_t>(vw.temp_bytes, 1));
    h->d_bbox.reserve(6 * (size_t)n); h->d_info.reserve(2 * (size_t)n);
    for (int k = 0; k < 2; k++) { h->d_keys[k].reserve(P); h->d_vals[k].reserve(P); }
    h->d_flag.reserve(P); h->d_rank.reserve(P);
    vw.bbox = h->d_bbox.p; vw.info = h->d_info.p; vw.flag = h->d_flag.p; vw.rank = h->d_rank.p; vw.temp = h->d_sort_temp.p;
    for (int k = 0; k < 2; k++) { vw.keys[k] = h->d_keys[k].p; vw.vals[k] = h->d_vals[k].p; }
    const CloudImageRec* d_recs = reinterpret_cast<const CloudImageRec*>(h->d_chunk.p);
    const uzl_cloud_cfg& c = h->cfg;
    cloud_voxel_sort(d_recs, n, n_pixels, max_pixels, c.leaf_size, c.z_min, c.z_max, vw, st);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(st));                     // the staging area is free again
    int32_t* info = reinterpret_cast<int32_t*>(h->h_work.p);
    UZL_HIP(hipMemcpyAsync(info, h->d_info.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    UZL_HIP(hipStreamSynchronize(st));
    std::vector<CloudRec> clouds((size_t)n);
    int64_t total = 0;
    for (int32_t i = 0; i < n; i++) {
        if (info[2 * i + 1]) return fail(h, UZL_ERR_BAD_ARG, "the voxel grid of an image overflows int32 (leaf_size too small for its extent)");
        if (info[2 * i] > kCloudMaxPoints) return fail(h, UZL_ERR_BAD_ARG, "an image gives more points than UZL_CLOUD_MAX_POINTS");
        clouds[i] = CloudRec{h->n_points + total, info[2 * i], info[2 * i] >= c.k_neighbours ? c.k_neighbours : 0};
        total += info[2 * i];
    }
    if (h->n_points + total >= ((int64_t)1 << 40)) return fail(h, UZL_ERR_BAD_ARG, "too many points");
    reserve_store(h, total, n);
    launch_cloud_voxel_points(d_recs, n_pixels, c.leaf_size, c.z_min, c.z_max, vw, h->d_xyz.p + 3 * h->n_points, h->d_bgr.p + 3 * h->n_points, st);
    UZL_HIP(hipGetLastError());
    finish_append(h, clouds, total, first_cloud);
    return UZL_OK;
}

CloudIcpArgs icp_args(uzl_cloud* h)
{
    const uzl_cloud_cfg& c = h->cfg;
    CloudIcpArgs a{};
    a.clouds = h->d_clouds.p; a.xyz = h->d_xyz.p; a.lab = h->d_lab.p; a.cov = h->d_cov.p;
    a.max_corr_sq = c.max_correspondence_dist * c.max_correspondence_dist;
    a.rot_eps = c.rotation_epsilon; a.trans_eps = c.transformation_epsilon;
    a.lab_weight = c.lab_weight;
    a.max_iterations = c.max_iterations; a.inner_iterations = c.inner_iterations;
    return a;
}

// The pairs on the device with their work arrays; T0 = NULL starts every pair at the identity.
void upload_pairs(uzl_cloud* h, int32_t n_pairs, const uzl_cloud_pair* pairs, const double* T0, CloudIcpArgs& a, int32_t* max_from,
                  int32_t* max_to)
{
    hipStream_t s = h->stream;
    h->h_work.reserve(std::max((size_t)n_pairs * sizeof(CloudPairRec), (size_t)n_pairs * sizeof(CloudPairState)));
    CloudPairRec* recs = reinterpret_cast<CloudPairRec*>(h->h_work.p);
    int64_t tgt = 0, src = 0;
    *max_from = 0; *max_to = 0;
    static const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int32_t i = 0; i < n_pairs; i++) {
        const uzl_cloud_pair& p = pairs[i];
        CloudPairRec& r = recs[i];
        r.from = p.cloud_from; r.to = p.cloud_to; r.tgt_off = tgt; r.src_off = src;
        memcpy(r.G, p.first_guess, sizeof(r.G));
        memcpy(r.T0, T0 ? T0 : I, sizeof(r.T0));
        tgt += h->clouds[p.cloud_to].n; src += h->clouds[p.cloud_from].n;
        *max_from = std::max(*max_from, h->clouds[p.cloud_from].n);
        *max_to = std::max(*max_to, h->clouds[p.cloud_to].n);
    }
    h->d_pairs.reserve(n_pairs);
    h->d_state.reserve(n_pairs);
    h->d_tgt.reserve(8 * (size_t)tgt);
    h->d_nn_j.reserve((size_t)src);
    h->d_nn_d.reserve((size_t)src);
    h->d_M.reserve(6 * (size_t)src);
    UZL_HIP(hipMemcpyAsync(h->d_pairs.p, recs, (size_t)n_pairs * sizeof(CloudPairRec), hipMemcpyHostToDevice, s));
    a.pairs = h->d_pairs.p; a.state = h->d_state.p; a.tgt = h->d_tgt.p; a.nn_j = h->d_nn_j.p; a.nn_d = h->d_nn_d.p; a.M = h->d_M.p;
}

void mul34(const double* A, const double* B, double* C)      // C = A B for 3x4 rigid-form matrices (last row 0 0 0 1)
{
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 4; c++)
            C[4 * r + c] = (A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c];
        C[4 * r + 3] += A[4 * r + 3];
    }
}

void inv34(const double* A, double* B)                        // the affine inverse, as Eigen's Affine3d::inverse(): 3x3 by the adjugate
{
    const double a = A[0], b = A[1], c = A[2], d = A[4], e = A[5], f = A[6], g = A[8], h = A[9], i = A[10];
    const double c00 = e * i - f * h, c01 = c * h - b * i, c02 = b * f - c * e;
    const double c10 = f * g - d * i, c11 = a * i - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double det = (a * c00 + b * c10) + c * c20;
    const double R[9] = {c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det};
    for (int r = 0; r < 3; r++) {
        for (int k = 0; k < 3; k++) B[4 * r + k] = R[3 * r + k];
        B[4 * r + 3] = 0.0 - ((R[3 * r] * A[3] + R[3 * r + 1] * A[7]) + R[3 * r + 2] * A[11]);
    }
}

// steps 9-10 of one pair on the host
void finish(const uzl_cloud_cfg& c, const uzl_cloud_pair& p, const CloudPairState& o, int32_t n_from, int32_t n_to, uzl_cloud_edge* e)
{
    memset(e, 0, sizeof(*e));
    e->status = o.status; e->iterations = o.iterations; e->num_corr = o.num_corr; e->n_from = n_from; e->n_to = n_to;
    memcpy(e->num_corr_iter, o.num_corr_iter, sizeof(e->num_corr_iter));
    double Tf[12], Ti[12], X[12], Xi[12], Tc[12];
    for (int k = 0; k < 12; k++) Tf[k] = (double)(float)o.T[k];
    inv34(Tf, Ti);
    mul34(Ti, p.first_guess, X);
    memcpy(e->transform, X, sizeof(X));
    e->match_score = (double)o.num_corr / (double)std::max(n_from, n_to);
    if (o.status != UZL_CLOUD_OK) return;
    if (!(e->match_score > c.min_score)) { e->status = UZL_CLOUD_LOW_SCORE; return; }
    inv34(X, Xi);
    mul34(p.first_guess, Xi, Tc);
    const double tn = std::sqrt((Tc[3] * Tc[3] + Tc[7] * Tc[7]) + Tc[11] * Tc[11]);
    const double cosang = std::min(1.0, std::max(-1.0, (((Tc[0] + Tc[5]) + Tc[10]) - 1.0) / 2.0));
    const double deg = std::fabs(std::acos(cosang)) * 180.0 / M_PI;
    if (!(tn <= c.max_translation) || !(deg <= c.max_rotation_deg)) { e->status = UZL_CLOUD_TOO_FAR; return; }
    for (int k = 0; k < 3; k++) { e->information[7 * k] = 1e4; e->information[7 * (k + 3)] = 1e6; }
    e->matching_score = 1.0;
}

}  // namespace

extern "C" {

void uzl_cloud_cfg_default(uzl_cloud_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->leaf_size = 0.05f; c->z_min = 0.0f; c->z_max = 5.0f; c->lab_weight = 0.024f;
    c->k_neighbours = 20; c->max_iterations = 20; c->inner_iterations = 10; c->device = 0;
    c->gicp_epsilon = 0.001; c->max_correspondence_dist = 0.2; c->rotation_epsilon = 2e-3; c->transformation_epsilon = 5e-4;
    c->min_score = 0.3; c->max_translation = 1.0; c->max_rotation_deg = 30.0;
}

int uzl_cloud_create(const uzl_cloud_cfg* cfg, uzl_cloud** out)
{
    return create_handle(cfg, uzl_cloud_cfg_default, out, check_cfg, [](uzl_cloud* h) {
        // step 3: the sRGB linearisation, from the host's libm
        double table[256];
        for (int v = 0; v < 256; v++) {
            const double x = v / 255.0;
            table[v] = x > 0.04045 ? std::pow((x + 0.055) / 1.055, 2.4) : x / 12.92;
        }
        h->d_table.reserve(256);
        UZL_HIP(hipMemcpyAsync(h->d_table.p, table, sizeof(table), hipMemcpyHostToDevice, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));
    });
}

void uzl_cloud_destroy(uzl_cloud* h) { destroy_handle(h); }

const char* uzl_cloud_last_error(uzl_cloud* h) { return last_error_of(h); }

int uzl_cloud_set_config(uzl_cloud* h, const uzl_cloud_cfg* cfg) { return set_config_of(h, cfg, check_cfg); }

int uzl_cloud_add_points(uzl_cloud* h, int32_t n_points, const float* xyz, const uint8_t* bgr, int32_t* cloud)
{
    UZL_GUARD_BEGIN(h)
    if (!xyz || !bgr) return fail(h, UZL_ERR_BAD_ARG, "null points or colours");
    if (n_points < h->cfg.k_neighbours) return fail(h, UZL_ERR_BAD_ARG, "fewer points than k_neighbours");
    if (n_points > kCloudMaxPoints) return fail(h, UZL_ERR_BAD_ARG, "more points than UZL_CLOUD_MAX_POINTS");
    for (int64_t i = 0; i < 3 * (int64_t)n_points; i++) if (!std::isfinite(xyz[i])) return fail(h, UZL_ERR_BAD_ARG, "non-finite point");
    if ((int64_t)h->clouds.size() + 1 > INT32_MAX || h->n_points + n_points >= ((int64_t)1 << 40)) return fail(h, UZL_ERR_BAD_ARG, "too many clouds");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    reserve_store(h, n_points, 1);
    h->h_work.reserve((size_t)n_points * 15);
    memcpy(h->h_work.p, xyz, (size_t)n_points * 12);
    memcpy(h->h_work.p + (size_t)n_points * 12, bgr, (size_t)n_points * 3);
    UZL_HIP(hipMemcpyAsync(h->d_xyz.p + 3 * h->n_points, h->h_work.p, (size_t)n_points * 12, hipMemcpyHostToDevice, st));
    UZL_HIP(hipMemcpyAsync(h->d_bgr.p + 3 * h->n_points, h->h_work.p + (size_t)n_points * 12, (size_t)n_points * 3, hipMemcpyHostToDevice, st));
    finish_append(h, {CloudRec{h->n_points, n_points, h->cfg.k_neighbours}}, n_points, cloud);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_cloud_add_images(uzl_cloud* h, int32_t n, const uzl_depth_image* images, const uzl_color_image* colors, int32_t* first_cloud)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = depth_images_check(h, n, images)) return rc;
    if (int rc = check_colors(h, n, images, colors)) return rc;
    return append_images(h, n, images, nullptr, colors, first_cloud);
    UZL_GUARD_END(h)
}

int uzl_cloud_count(uzl_cloud* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return (int)h->clouds.size();
}

int uzl_cloud_read(uzl_cloud* h, int32_t cloud, int32_t cap, float* xyz, uint8_t* bgr, float* lab, double* cov)
{
    UZL_GUARD_BEGIN(h)
    if (cloud < 0 || cloud >= (int32_t)h->clouds.size()) return fail(h, UZL_ERR_BAD_ARG, "cloud index out of range");
    if (cap < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    const CloudRec& r = h->clouds[cloud];
    if (!xyz && !bgr && !lab && !cov) return r.n;
    if (cap < r.n) return fail(h, UZL_ERR_TRUNCATED, "capacity smaller than the cloud");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    const size_t n = (size_t)r.n;
    std::vector<double> c6(cov ? 6 * n : 0);
    if (xyz) UZL_HIP(hipMemcpyAsync(xyz, h->d_xyz.p + 3 * r.off, n * 12, hipMemcpyDeviceToHost, st));
    if (bgr) UZL_HIP(hipMemcpyAsync(bgr, h->d_bgr.p + 3 * r.off, n * 3, hipMemcpyDeviceToHost, st));
    if (lab) UZL_HIP(hipMemcpyAsync(lab, h->d_lab.p + 3 * r.off, n * 12, hipMemcpyDeviceToHost, st));
    if (cov) UZL_HIP(hipMemcpyAsync(c6.data(), h->d_cov.p + 6 * r.off, n * 48, hipMemcpyDeviceToHost, st));
    UZL_HIP(hipStreamSynchronize(st));
    if (cov)
        for (size_t i = 0; i < n; i++) {
            const double* s = &c6[6 * i];
            const double m[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]};
            memcpy(cov + 9 * i, m, sizeof(m));
        }
    return r.n;
    UZL_GUARD_END(h)
}

int uzl_cloud_estimate(uzl_cloud* h, int32_t n_pairs, const uzl_cloud_pair* pairs, uzl_cloud_edge* results)
{
    UZL_GUARD_BEGIN(h)
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !results))) return fail(h, UZL_ERR_BAD_ARG, "bad pair count, null pairs or null results");
    for (int32_t i = 0; i < n_pairs; i++)
        if (int rc = check_pair(h, pairs[i])) return rc;
    if (n_pairs == 0) return UZL_OK;
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    CloudIcpArgs a = icp_args(h);
    int32_t max_from, max_to;
    upload_pairs(h, n_pairs, pairs, nullptr, a, &max_from, &max_to);
    launch_cloud_prepare(a, n_pairs, max_to, s);
    for (int it = 0; it < h->cfg.max_iterations; it++) {
        launch_cloud_nn6(a, n_pairs, max_from, s);
        launch_cloud_step(a, n_pairs, s);
    }
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));                      // the staging area is free again
    CloudPairState* outs = reinterpret_cast<CloudPairState*>(h->h_work.p);
    UZL_HIP(hipMemcpyAsync(outs, h->d_state.p, (size_t)n_pairs * sizeof(CloudPairState), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < n_pairs; i++)
        finish(h->cfg, pairs[i], outs[i], h->clouds[pairs[i].cloud_from].n, h->clouds[pairs[i].cloud_to].n, &results[i]);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_cloud_correspondences(uzl_cloud* h, const uzl_cloud_pair* pair, const double* T, int32_t* j, float* dist2, int32_t* kept)
{
    UZL_GUARD_BEGIN(h)
    if (!pair || !T) return fail(h, UZL_ERR_BAD_ARG, "null pair or estimate");
    if (int rc = check_pair(h, *pair)) return rc;
    for (int k = 0; k < 12; k++) if (!std::isfinite(T[k])) return fail(h, UZL_ERR_BAD_ARG, "non-finite estimate");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    CloudIcpArgs a = icp_args(h);
    int32_t max_from, max_to;
    upload_pairs(h, 1, pair, T, a, &max_from, &max_to);
    launch_cloud_prepare(a, 1, max_to, s);
    launch_cloud_nn6(a, 1, max_from, s);
    UZL_HIP(hipGetLastError());
    const int32_t nf = max_from;
    std::vector<float> d(nf);
    if (j) UZL_HIP(hipMemcpyAsync(j, a.nn_j, (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(d.data(), a.nn_d, (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < nf; i++) {
        if (dist2) dist2[i] = d[i];
        if (kept) kept[i] = (double)d[i] < a.max_corr_sq ? 1 : 0;
    }
    return nf;
    UZL_GUARD_END(h)
}

}  // extern "C"

#ifdef UZL_DIAG
// Stage hook of the diagnostic library (tests/test_cloud_step_gpu.py): one outer iteration of one pair from the estimate T, through
// the kernels an estimate runs - the pair uploaded with T0 = T, then cloud_prepare, cloud_nn6 and cloud_step_kernel once each.  Any
// output may be NULL.  M: 6 f64 per point of `from`, zero rows where the correspondence is not kept; sums: the 28 sums at T; T_next:
// the pose after the inner loop; state: status, done, num_corr, n_trials; trials: 100 x 9 f64, per trial mu as used, the outcome
// (0 refused, 1 accepted, 2 rejected), delta and the trial pose's f (delta and f zero for a refused trial), zero beyond n_trials.
// Returns n_points(from); errors as uzl_cloud_correspondences.
extern "C" UZL_DIAG_EXPORT int uzl_debug_cloud_step(uzl_cloud* h, const uzl_cloud_pair* pair, const double* T, double* M, double* sums,
                                                    double* T_next, int32_t* state, double* trials)
{
    UZL_GUARD_BEGIN(h)
    if (!pair || !T) return fail(h, UZL_ERR_BAD_ARG, "null pair or estimate");
    if (int rc = check_pair(h, *pair)) return rc;
    if (!finite12(T)) return fail(h, UZL_ERR_BAD_ARG, "non-finite estimate");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    CloudIcpArgs a = icp_args(h);
    int32_t max_from, max_to;
    upload_pairs(h, 1, pair, T, a, &max_from, &max_to);
    h->d_log.reserve(1);
    UZL_HIP(hipMemsetAsync(h->d_log.p, 0, sizeof(CloudStepLog), s));
    a.log = h->d_log.p;
    launch_cloud_prepare(a, 1, max_to, s);
    launch_cloud_nn6(a, 1, max_from, s);
    launch_cloud_step(a, 1, s);
    UZL_HIP(hipGetLastError());
    const int32_t nf = max_from;
    std::vector<float> d(nf);
    std::vector<double> m(6 * (size_t)nf);
    std::vector<CloudStepLog> log(1);
    CloudPairState st;
    UZL_HIP(hipMemcpyAsync(d.data(), a.nn_d, (size_t)nf * 4, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(m.data(), a.M, (size_t)nf * 48, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(log.data(), a.log, sizeof(CloudStepLog), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(&st, a.state, sizeof(st), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    if (M)
        for (int32_t i = 0; i < nf; i++) {
            const bool kept = (double)d[i] < a.max_corr_sq;
            for (int k = 0; k < 6; k++) M[6 * (size_t)i + k] = kept ? m[6 * (size_t)i + k] : 0.0;
        }
    if (sums) memcpy(sums, log[0].sums, sizeof(log[0].sums));
    if (T_next) memcpy(T_next, st.T, sizeof(st.T));
    if (state) { state[0] = st.status; state[1] = st.done; state[2] = st.num_corr; state[3] = log[0].n_trials; }
    if (trials) memcpy(trials, log[0].trial, sizeof(log[0].trial));
    return nf;
    UZL_GUARD_END(h)
}
#endif  // UZL_DIAG

int uzl::cloud_add_device_images(uzl_cloud* h, int device, int32_t n, const uzl_depth_image* geom, const float* const* d_depth,
                                 const uzl_color_image* colors, int32_t* first_cloud)
{
    UZL_GUARD_BEGIN(h)
    if (device != h->cfg.device) return fail(h, UZL_ERR_BAD_ARG, "the images are on another device than the cloud handle");
    if (n < 0 || (n > 0 && (!geom || !d_depth))) return fail(h, UZL_ERR_BAD_ARG, "bad image count or null images");
    if (int rc = check_colors(h, n, geom, colors)) return rc;
    return append_images(h, n, geom, d_depth, colors, first_cloud);
    UZL_GUARD_END(h)
}
