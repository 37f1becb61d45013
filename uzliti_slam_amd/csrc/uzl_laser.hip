// uzl_laser.hip — laser scan matching: TYPE_2D_LASER edges by point-to-line ICP (host + C ABI uzl_laser_*).
//
// Mirrors LaserTransformationEstimator::estimateEdgeImpl / estimateTransform / laserScanToLDP
// (transformation_estimation/src/laser_transformation_estimator.cpp:134-443); include/uzl_mi355x.h states the contract.  HBM
// layout as the occupancy grid's store: one append-only arena of readings (f32, scan after scan), one of (cos, sin) tables shared
// by scans of the same (angle_min, angle_increment, n), one record per scan.  An estimate uploads the pairs (the first guess's
// rotation as (cos, sin) of the host's libm), runs one workgroup per pair (laser_kernels.hip) and finishes each result on the host:
// theta by atan2, the information block, the plausibility test.
#include "laser_types.hpp"
#include "scan_store.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>

using namespace uzl;

struct uzl_laser : HandleBase {
    uzl_laser_cfg cfg;
    HandleStream stream;
    std::vector<LaserScanRec> scans;
    ScanStore store;             // the readings and their (cos, sin) tables
    DevBuf<LaserScanRec> d_scans;
    // work, reused between calls
    PinBuf<uint8_t> h_work;
    DevBuf<LaserPairRec> d_pairs;
    DevBuf<LaserPairOut> d_out;
    DevBuf<uint8_t> d_stage;
};

namespace {

int check_cfg(const uzl_laser_cfg& c)
{
    const double thr[] = {c.epsilon_xy, c.epsilon_theta, c.max_correspondence_dist, c.outliers_adaptive_mult, c.max_angular_correction_deg,
                          c.max_linear_correction, c.goal_trace, c.other_information};
    for (double v : thr) if (std::isnan(v) || v < 0.) return UZL_ERR_BAD_ARG;
    const double frac[] = {c.outliers_max_perc, c.outliers_adaptive_order, c.min_valid_fraction, c.fail_fraction};
    for (double v : frac) if (std::isnan(v) || v < 0. || v > 1.) return UZL_ERR_BAD_ARG;
    if (c.max_iterations < 1) return UZL_ERR_BAD_ARG;
    return UZL_OK;
}

// One scan to append: what uzl_laser_scan says about it, without its values.
struct ScanIn {
    int32_t n;
    float angle_min, angle_increment, range_min, range_max;
};

int check_scan(uzl_laser* h, const ScanIn& s)
{
    if (s.n < kIcpMinBeams || s.n > kIcpMaxBeams) return fail(h, UZL_ERR_BAD_ARG, "n_beams outside 8..4096");
    if (!std::isfinite(s.angle_min) || !std::isfinite(s.angle_increment)) return fail(h, UZL_ERR_BAD_ARG, "non-finite scan angle");
    if (!(s.range_min >= 0.f)) return fail(h, UZL_ERR_BAD_ARG, "range_min negative or NaN");
    if (!std::isfinite(s.range_max)) return fail(h, UZL_ERR_BAD_ARG, "range_max not finite");
    return UZL_OK;
}

// Append checked scans to the store (scan_store.hpp; the tables are contract step 1): the `total` values are put at the arena's
// end by copy(dst, stream), the records go up on the same stream, and the bookkeeping changes only when everything before it
// succeeded.
template <typename Copy>
void append(uzl_laser* h, const std::vector<ScanIn>& in, int64_t total, int32_t* first_scan, Copy&& copy)
{
    const size_t n = in.size(), have = h->scans.size();
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t st = h->stream;
    ScanStore::Pending p = h->store.begin(st, in, total);
    std::vector<LaserScanRec> recs(n);
    for (size_t i = 0; i < n; i++) recs[i] = LaserScanRec{p.values_off[i], p.trig_off[i], in[i].n, in[i].range_min, in[i].range_max, 0};
    h->d_scans.reserve(std::max<size_t>(have + n, 1), true, st);
    if (n) UZL_HIP(hipMemcpyAsync(h->d_scans.p + have, recs.data(), n * sizeof(LaserScanRec), hipMemcpyHostToDevice, st));
    if (total) copy(p.dst, st);
    UZL_HIP(hipStreamSynchronize(st));
    h->scans.insert(h->scans.end(), recs.begin(), recs.end());
    h->store.commit(p);
    if (first_scan) *first_scan = (int32_t)have;
}

int check_pair(uzl_laser* h, const uzl_laser_pair& p)
{
    const int32_t ns = (int32_t)h->scans.size();
    if (p.scan_from < 0 || p.scan_from >= ns || p.scan_to < 0 || p.scan_to >= ns) return fail(h, UZL_ERR_BAD_ARG, "scan index out of range");
    if (!finite12(p.first_guess)) return fail(h, UZL_ERR_BAD_ARG, "non-finite first guess");
    return UZL_OK;
}

LaserIcpArgs icp_args(const uzl_laser* h)
{
    const uzl_laser_cfg& c = h->cfg;
    LaserIcpArgs a{};
    a.values = h->store.d_values.p; a.trig = h->store.d_trig.p; a.scans = h->d_scans.p;
    a.max_corr_sq = c.max_correspondence_dist * c.max_correspondence_dist;
    a.max_perc = c.outliers_max_perc; a.adaptive_order = c.outliers_adaptive_order; a.adaptive_mult = c.outliers_adaptive_mult;
    a.fail_fraction = c.fail_fraction;
    a.eps_xy_sq = c.epsilon_xy * c.epsilon_xy;
    a.sin_eps_theta = std::sin(std::min(c.epsilon_theta, M_PI / 2));
    a.max_iterations = c.max_iterations;
    return a;
}

// steps 8-10 of one pair on the host
void finish(const uzl_laser_cfg& c, const uzl_laser_pair& p, const LaserPairOut& o, uzl_laser_edge* e)
{
    memset(e, 0, sizeof(*e));
    e->status = o.status; e->nvalid = o.nvalid; e->scan_valid = o.scan_valid; e->deg_count = o.deg_count; e->iterations = o.iterations;
    e->error = o.error;
    const double T[12] = {o.c, -o.s, 0, o.tx, o.s, o.c, 0, o.ty, 0, 0, 1, 0};
    memcpy(e->transform, T, sizeof(T));
    for (int k = 0; k < 6; k++) e->information[7 * k] = c.other_information;
    if (o.status != UZL_LASER_OK) return;
    if (o.deg_count <= 0) { e->status = UZL_LASER_VIEWPOINT; return; }
    const double trace = (o.H[0] + o.H[3]) + o.H[5];
    const double scale = c.goal_trace / trace;
    e->information[0] = o.H[0] * scale; e->information[1] = o.H[1] * scale; e->information[6] = o.H[1] * scale;
    e->information[7] = o.H[3] * scale; e->information[35] = o.H[5] * scale;
    if (c.min_valid_fraction * (double)o.scan_valid > (double)o.nvalid) { e->status = UZL_LASER_FEW_MATCHES; return; }
    // step 10: diff = T_guess^-1 T in the plane
    const double th0 = std::atan2(p.first_guess[4], p.first_guess[0]);
    const double c0 = std::cos(th0), s0 = std::sin(th0);
    const double dx = o.tx - p.first_guess[3], dy = o.ty - p.first_guess[7];
    const double angle_deg = std::fabs(std::atan2(c0 * o.s - s0 * o.c, c0 * o.c + s0 * o.s)) * 180.0 / M_PI;
    if (1.5 * std::sqrt(dx * dx + dy * dy) > c.max_linear_correction || 1.5 * angle_deg > c.max_angular_correction_deg) {
        e->status = UZL_LASER_TOO_FAR;
        return;
    }
    e->matching_score = (double)o.nvalid;
}

}  // namespace

extern "C" {

void uzl_laser_cfg_default(uzl_laser_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_iterations = 10; c->device = 0;
    c->epsilon_xy = 0.01; c->epsilon_theta = 0.02; c->max_correspondence_dist = 0.3;
    c->outliers_max_perc = 0.80; c->outliers_adaptive_order = 0.7; c->outliers_adaptive_mult = 2.0;
    c->max_angular_correction_deg = 45.0; c->max_linear_correction = 1.5;
    c->min_valid_fraction = 0.25; c->fail_fraction = 0.05; c->goal_trace = 10000.0; c->other_information = 100.0;
}

int uzl_laser_create(const uzl_laser_cfg* cfg, uzl_laser** out)
{
    return create_handle(cfg, uzl_laser_cfg_default, out, check_cfg, [](uzl_laser*) { laser_icp_prepare(); });
}

void uzl_laser_destroy(uzl_laser* h) { destroy_handle(h); }

const char* uzl_laser_last_error(uzl_laser* h) { return last_error_of(h); }

int uzl_laser_set_config(uzl_laser* h, const uzl_laser_cfg* cfg) { return set_config_of(h, cfg, check_cfg); }

int uzl_laser_add_scans(uzl_laser* h, int32_t n, const uzl_laser_scan* scans, int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    if (n < 0 || (n > 0 && !scans)) return fail(h, UZL_ERR_BAD_ARG, "bad scan count or null scans");
    std::vector<ScanIn> in(n);
    int64_t total = 0;
    for (int32_t i = 0; i < n; i++) {
        const uzl_laser_scan& s = scans[i];
        in[i] = ScanIn{s.n_beams, s.angle_min, s.angle_increment, s.range_min, s.range_max};
        if (int rc = check_scan(h, in[i])) return rc;
        if (!s.values) return fail(h, UZL_ERR_BAD_ARG, "null values");
        total += s.n_beams;
    }
    if ((int64_t)h->scans.size() + n > INT32_MAX || h->store.n_values + total >= ((int64_t)1 << 40)) return fail(h, UZL_ERR_BAD_ARG, "too many scans");
    append(h, in, total, first_scan, [&](float* dst, hipStream_t st) {
        h->h_work.reserve((size_t)total * 4);
        float* w = reinterpret_cast<float*>(h->h_work.p);
        int64_t o = 0;
        for (int32_t i = 0; i < n; i++) { memcpy(w + o, scans[i].values, (size_t)scans[i].n_beams * 4); o += scans[i].n_beams; }
        UZL_HIP(hipMemcpyAsync(dst, w, (size_t)total * 4, hipMemcpyHostToDevice, st));
    });
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_laser_scan_count(uzl_laser* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return (int)h->scans.size();
}

int uzl_laser_estimate(uzl_laser* h, int32_t n_pairs, const uzl_laser_pair* pairs, uzl_laser_edge* results)
{
    UZL_GUARD_BEGIN(h)
    if (n_pairs < 0 || (n_pairs > 0 && (!pairs || !results))) return fail(h, UZL_ERR_BAD_ARG, "bad pair count, null pairs or null results");
    for (int32_t i = 0; i < n_pairs; i++)
        if (int rc = check_pair(h, pairs[i])) return rc;
    if (n_pairs == 0) return UZL_OK;
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    const size_t in_bytes = (size_t)n_pairs * sizeof(LaserPairRec), out_bytes = (size_t)n_pairs * sizeof(LaserPairOut);
    h->h_work.reserve(std::max(in_bytes, out_bytes));
    h->d_pairs.reserve(n_pairs);
    h->d_out.reserve(n_pairs);
    LaserIcpArgs a = icp_args(h);
    LaserPairRec* recs = reinterpret_cast<LaserPairRec*>(h->h_work.p);
    for (int32_t i = 0; i < n_pairs; i++) {
        const uzl_laser_pair& p = pairs[i];
        const double th = std::atan2(p.first_guess[4], p.first_guess[0]);
        recs[i] = LaserPairRec{p.scan_from, p.scan_to, p.first_guess[3], p.first_guess[7], std::cos(th), std::sin(th)};
        a.max_from = std::max(a.max_from, h->scans[p.scan_from].n);
        a.max_to = std::max(a.max_to, h->scans[p.scan_to].n);
    }
    UZL_HIP(hipMemcpyAsync(h->d_pairs.p, recs, in_bytes, hipMemcpyHostToDevice, s));
    a.pairs = h->d_pairs.p; a.out = h->d_out.p;
    launch_laser_icp(a, n_pairs, s);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));                      // the staging area is free again
    LaserPairOut* outs = reinterpret_cast<LaserPairOut*>(h->h_work.p);
    UZL_HIP(hipMemcpyAsync(outs, h->d_out.p, out_bytes, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    for (int32_t i = 0; i < n_pairs; i++) finish(h->cfg, pairs[i], outs[i], &results[i]);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_laser_correspondences(uzl_laser* h, const uzl_laser_pair* pair, const double* x, int32_t* j1, int32_t* j2, int32_t* valid, double* dist)
{
    UZL_GUARD_BEGIN(h)
    if (!pair || !x) return fail(h, UZL_ERR_BAD_ARG, "null pair or estimate");
    if (int rc = check_pair(h, *pair)) return rc;
    if (!std::isfinite(x[0]) || !std::isfinite(x[1]) || !std::isfinite(x[2])) return fail(h, UZL_ERR_BAD_ARG, "non-finite estimate");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    const int32_t nt = h->scans[pair->scan_to].n;
    h->h_work.reserve(sizeof(LaserPairRec));
    h->d_pairs.reserve(1);
    h->d_stage.reserve((size_t)nt * 20);
    LaserIcpArgs a = icp_args(h);
    LaserPairRec* rec = reinterpret_cast<LaserPairRec*>(h->h_work.p);
    *rec = LaserPairRec{pair->scan_from, pair->scan_to, x[0], x[1], std::cos(x[2]), std::sin(x[2])};
    a.max_from = h->scans[pair->scan_from].n; a.max_to = nt;
    UZL_HIP(hipMemcpyAsync(h->d_pairs.p, rec, sizeof(LaserPairRec), hipMemcpyHostToDevice, s));
    a.pairs = h->d_pairs.p; a.out = nullptr; a.stage = 1;
    a.st_dist = reinterpret_cast<double*>(h->d_stage.p);
    a.st_j1 = reinterpret_cast<int32_t*>(h->d_stage.p + (size_t)nt * 8);
    a.st_j2 = a.st_j1 + nt;
    a.st_valid = a.st_j2 + nt;
    launch_laser_icp(a, 1, s);
    UZL_HIP(hipGetLastError());
    if (dist) UZL_HIP(hipMemcpyAsync(dist, a.st_dist, (size_t)nt * 8, hipMemcpyDeviceToHost, s));
    if (j1) UZL_HIP(hipMemcpyAsync(j1, a.st_j1, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
    if (j2) UZL_HIP(hipMemcpyAsync(j2, a.st_j2, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
    if (valid) UZL_HIP(hipMemcpyAsync(valid, a.st_valid, (size_t)nt * 4, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    return nt;
    UZL_GUARD_END(h)
}

}  // extern "C"

// The way into the store for scans that already lie in device memory (declared in laser_types.hpp): n_scans scans, scan i as
// scan_at(i) describes it, one after the other at d_values and complete.  Called with the handle's lock held.
namespace {

template <typename ScanAt>
int append_device(uzl_laser* h, int device, int32_t n_scans, ScanAt&& scan_at, const float* d_values, int32_t* first_scan)
{
    if (device != h->cfg.device) return fail(h, UZL_ERR_BAD_ARG, "the scans are on another device than the laser handle");
    if (n_scans < 0 || (n_scans > 0 && !d_values)) return fail(h, UZL_ERR_BAD_ARG, "bad scan count or null scans");
    std::vector<ScanIn> in(n_scans);
    int64_t total = 0;
    for (int32_t i = 0; i < n_scans; i++) {
        const DeviceScan s = scan_at(i);
        in[i] = ScanIn{s.n, s.angle_min, s.angle_increment, s.range_min, s.range_max};
        if (int rc = check_scan(h, in[i])) return rc;
        total += s.n;
    }
    if ((int64_t)h->scans.size() + n_scans > INT32_MAX || h->store.n_values + total >= ((int64_t)1 << 40)) return fail(h, UZL_ERR_BAD_ARG, "too many scans");
    append(h, in, total, first_scan, [&](float* dst, hipStream_t st) {
        UZL_HIP(hipMemcpyAsync(dst, d_values, (size_t)total * 4, hipMemcpyDeviceToDevice, st));
    });
    return UZL_OK;
}

}  // namespace

// uzl_laserline_to_laser: every scan with the same beam count, grid and limits
int uzl::laser_append_device(uzl_laser* h, int device, int32_t n_scans, int32_t n_beams, const float* d_values, float angle_min,
                             float angle_increment, float range_min, float range_max, int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    const DeviceScan one{n_beams, angle_min, angle_increment, range_min, range_max};
    return append_device(h, device, n_scans, [&](int32_t) { return one; }, d_values, first_scan);
    UZL_GUARD_END(h)
}

// uzl_scanmerge_to_laser: scans that differ in beam count, grid or limits
int uzl::laser_append_device_scans(uzl_laser* h, int device, int32_t n_scans, const DeviceScan* scans, const float* d_values,
                                   int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    if (n_scans > 0 && !scans) return fail(h, UZL_ERR_BAD_ARG, "bad scan count or null scans");
    return append_device(h, device, n_scans, [&](int32_t i) { return scans[i]; }, d_values, first_scan);
    UZL_GUARD_END(h)
}
