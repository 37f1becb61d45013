// uzl_scanmerge.hip — the laser scans of merged nodes folded into one (host + C ABI uzl_scanmerge_*).
//
// Mirrors the LaserscanDataPtr overload of GraphGridMapper::mergeLaserScans with scanToPoints / scanToIntensities / scanMean
// (map_projection/src/graph_grid_mapper.cpp:45-133, 575-621) as mergeNodes calls it (graph_slam/src/graph_slam_node.cpp:955,
// 999-1002); include/uzl_mi355x.h states the contract.  A run checks every pair, composes the displacements on the host, packs the
// pairs' records and readings into one pinned area, moves it in one copy and merges every pair in one launch (scanmerge_kernels.hip).
// The (cos, sin) tables (n + 1 entries each, the host's libm) are kept between runs, one per distinct (angle_min, increment, n).
// The merged scans and the call's inputs stay in HBM: uzl_scanmerge_to_grid / _to_laser hand the scans on without leaving the
// device, and uzl_scanmerge_points runs the point stage of one pair again over the resident inputs.
#include "grid_types.hpp"
#include "laser_types.hpp"
#include "scan_store.hpp"
#include "scanmerge_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>

using namespace uzl;

namespace {

using TableKey = std::tuple<uint32_t, uint32_t, int32_t>;   // (angle_min bits, increment bits, n)

// What the host remembers of a merged pair.
struct PairHost {
    int32_t n_a, n_b;
    float amin, inc, lo, hi0;     // a's message fields: the merged scan's
    int64_t out_off;
};

}  // namespace

struct uzl_scanmerge : HandleBase {
    uzl_scanmerge_cfg cfg;
    HandleStream stream;
    // tables
    std::map<TableKey, int64_t> tables;
    int64_t n_trig = 0;
    DevBuf<double2> d_trig;
    // the resident result, and the inputs it was made from (for the stage entry)
    bool have = false;
    std::vector<PairHost> pairs;
    int64_t total = 0;
    DevBuf<float> d_ranges, d_intensities;
    DevBuf<double> d_centers;
    DevBuf<uint8_t> d_in;
    size_t values_at = 0;         // byte offset of the readings in d_in, behind the records
    // work
    PinBuf<uint8_t> h_in;
    DevBuf<int32_t> d_st_bin;
    DevBuf<float> d_st_rho;
};

namespace {

int check_cfg(const uzl_scanmerge_cfg&) { return UZL_OK; }

// A * B of two 3 x 4 transforms [R|t]: rows of A times columns of B, summed left to right (merge._compose)
void compose(const double* A, const double* B, double* out)
{
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
        out[4 * i + 3] = ((A[4 * i] * B[3] + A[4 * i + 1] * B[7]) + A[4 * i + 2] * B[11]) + A[4 * i + 3];
    }
}

int check_scan(uzl_scanmerge* h, const uzl_scanmerge_scan* s)
{
    if (!s) return fail(h, UZL_ERR_BAD_ARG, "null scan");
    if (s->n_beams < kScanMergeMinBeams || s->n_beams > kScanMergeMaxBeams) return fail(h, UZL_ERR_BAD_ARG, "n_beams outside 8..4096");
    if (!s->ranges || !s->intensities) return fail(h, UZL_ERR_BAD_ARG, "null ranges or intensities");
    if (!std::isfinite(s->angle_min) || !std::isfinite(s->angle_increment)) return fail(h, UZL_ERR_BAD_ARG, "non-finite scan angle");
    if (!std::isfinite(s->range_min) || !std::isfinite(s->range_max)) return fail(h, UZL_ERR_BAD_ARG, "non-finite range limit");
    if (s->range_min < 0.f) return fail(h, UZL_ERR_BAD_ARG, "range_min negative");
    if (s->range_max < s->range_min) return fail(h, UZL_ERR_BAD_ARG, "range_max below range_min");
    if (!finite12(s->displacement)) return fail(h, UZL_ERR_BAD_ARG, "non-finite displacement entry");
    return UZL_OK;
}

// the scope: keep lies on a laser-line grid (laser-line contract step 1)
bool on_laserline_grid(const uzl_scanmerge_scan& s)
{
    const float amin = (float)(-M_PI), amax = (float)M_PI;
    if (memcmp(&s.angle_min, &amin, 4) != 0) return false;
    const float nf = ceilf((amax - amin) / s.angle_increment);
    return nf >= (float)kScanMergeMinBeams && nf <= (float)kScanMergeMaxBeams && (int32_t)(uint32_t)nf == s.n_beams;
}

TableKey key_of(const uzl_scanmerge_scan& s)
{
    uint32_t ka, ki;
    memcpy(&ka, &s.angle_min, 4); memcpy(&ki, &s.angle_increment, 4);
    return std::make_tuple(ka, ki, s.n_beams);
}

void fill_scan(ScanMergeScanRec* r, const uzl_scanmerge_scan& s, const double* D, int64_t trig_off, int64_t* at, float* values)
{
    r->n = s.n_beams;
    r->amin = s.angle_min; r->inc = s.angle_increment; r->range_min = s.range_min; r->range_max = s.range_max;
    r->trig_off = trig_off;
    r->D[0] = (float)D[0]; r->D[1] = (float)D[1]; r->D[2] = (float)D[3];
    r->D[3] = (float)D[4]; r->D[4] = (float)D[5]; r->D[5] = (float)D[7];
    r->_pad = 0;
    r->ranges_off = *at;
    memcpy(values + *at, s.ranges, (size_t)s.n_beams * 4);
    *at += s.n_beams;
    r->intensities_off = *at;
    memcpy(values + *at, s.intensities, (size_t)s.n_beams * 4);
    *at += s.n_beams;
}

ScanMergeArgs kernel_args(const uzl_scanmerge* h)
{
    ScanMergeArgs a{};
    a.values = reinterpret_cast<const float*>(h->d_in.p + h->values_at);
    a.trig = h->d_trig.p;
    a.pairs = reinterpret_cast<const ScanMergePairRec*>(h->d_in.p);
    a.ranges = h->d_ranges.p; a.intensities = h->d_intensities.p; a.centers = h->d_centers.p;
    a.stage_pair = -1; a.stage_which = 0;
    return a;
}

int check_pair_index(uzl_scanmerge* h, int32_t pair)
{
    if (!h->have) return fail(h, UZL_ERR_STATE, "no run yet");
    if (pair < 0 || (size_t)pair >= h->pairs.size()) return fail(h, UZL_ERR_BAD_ARG, "pair index out of range");
    return UZL_OK;
}

std::vector<DeviceScan> merged_scans(const uzl_scanmerge* h)
{
    std::vector<DeviceScan> out(h->pairs.size());
    for (size_t i = 0; i < out.size(); i++) {
        const PairHost& p = h->pairs[i];
        out[i] = DeviceScan{p.n_a, p.amin, p.inc, p.lo, p.hi0};
    }
    return out;
}

}  // namespace

extern "C" {

void uzl_scanmerge_cfg_default(uzl_scanmerge_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
}

int uzl_scanmerge_create(const uzl_scanmerge_cfg* cfg, uzl_scanmerge** out)
{
    return create_handle(cfg, uzl_scanmerge_cfg_default, out, check_cfg, [](uzl_scanmerge*) {});
}

void uzl_scanmerge_destroy(uzl_scanmerge* h) { destroy_handle(h); }

const char* uzl_scanmerge_last_error(uzl_scanmerge* h) { return last_error_of(h); }

int uzl_scanmerge_run(uzl_scanmerge* h, int32_t n_pairs, const uzl_scanmerge_pair* pairs)
{
    UZL_GUARD_BEGIN(h)
    if (n_pairs < 0 || (n_pairs > 0 && !pairs)) return fail(h, UZL_ERR_BAD_ARG, "bad pair count or null pairs");
    int64_t n_values = 0, total = 0;
    for (int32_t i = 0; i < n_pairs; i++) {
        const uzl_scanmerge_pair& p = pairs[i];
        if (int rc = check_scan(h, p.keep)) return rc;
        if (int rc = check_scan(h, p.drop)) return rc;
        if (!finite12(p.keep_displacement) || !finite12(p.drop_displacement)) return fail(h, UZL_ERR_BAD_ARG, "non-finite displacement entry");
        if (!on_laserline_grid(*p.keep))
            return fail(h, UZL_ERR_UNSUPPORTED, "the keep scan does not lie on a laser-line grid (angle_min = (float)-pi, n = ceilf(2 pi / inc))");
        n_values += 2 * ((int64_t)p.keep->n_beams + p.drop->n_beams);
        total += p.keep->n_beams;
    }
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    // tables the call adds: entered in the handle's books only after everything below succeeded
    std::map<TableKey, int64_t> tables = h->tables;
    int64_t n_trig = h->n_trig;
    std::vector<double2> fresh;
    auto table_of = [&](const uzl_scanmerge_scan& sc) {
        const TableKey key = key_of(sc);
        auto it = tables.find(key);
        if (it != tables.end()) return it->second;
        for (int32_t k = 0; k <= sc.n_beams; k++) {
            const double th = (double)sc.angle_min + (double)k * (double)sc.angle_increment;
            fresh.push_back(make_double2(std::cos(th), std::sin(th)));
        }
        const int64_t off = n_trig;
        tables.emplace(key, off);
        n_trig += sc.n_beams + 1;
        return off;
    };
    const size_t recs_bytes = align256((size_t)n_pairs * sizeof(ScanMergePairRec));
    const size_t in_bytes = recs_bytes + (size_t)n_values * 4;
    h->h_in.reserve(std::max<size_t>(in_bytes, 256));
    ScanMergePairRec* recs = reinterpret_cast<ScanMergePairRec*>(h->h_in.p);
    float* values = reinterpret_cast<float*>(h->h_in.p + recs_bytes);
    std::vector<PairHost> host(n_pairs);
    int64_t at = 0, out_off = 0;
    for (int32_t i = 0; i < n_pairs; i++) {
        const uzl_scanmerge_pair& p = pairs[i];
        double Da[12], Db[12];
        compose(p.keep_displacement, p.keep->displacement, Da);     // step 1
        compose(p.drop_displacement, p.drop->displacement, Db);
        ScanMergePairRec& r = recs[i];
        fill_scan(&r.a, *p.keep, Da, table_of(*p.keep), &at, values);
        fill_scan(&r.b, *p.drop, Db, table_of(*p.drop), &at, values);
        r.out_off = out_off;
        r.b_newer = p.drop->stamp_ns > p.keep->stamp_ns ? 1 : 0;
        r._pad = 0;
        host[i] = PairHost{p.keep->n_beams, p.drop->n_beams, p.keep->angle_min, p.keep->angle_increment, p.keep->range_min,
                           p.keep->range_max, out_off};
        out_off += p.keep->n_beams;
    }
    h->have = false;                                       // a failure below leaves no half-made result behind
    h->d_trig.reserve((size_t)std::max<int64_t>(n_trig, 1), true, s);
    if (!fresh.empty())
        UZL_HIP(hipMemcpyAsync(h->d_trig.p + h->n_trig, fresh.data(), fresh.size() * sizeof(double2), hipMemcpyHostToDevice, s));
    h->d_in.reserve(std::max<size_t>(in_bytes, 256));
    h->d_ranges.reserve((size_t)std::max<int64_t>(total, 1)); h->d_intensities.reserve((size_t)std::max<int64_t>(total, 1));
    h->d_centers.reserve(std::max<size_t>(3 * (size_t)n_pairs, 1));
    h->values_at = recs_bytes;
    if (n_pairs) {
        UZL_HIP(hipMemcpyAsync(h->d_in.p, h->h_in.p, in_bytes, hipMemcpyHostToDevice, s));
        launch_scanmerge(kernel_args(h), n_pairs, s);
        UZL_HIP(hipGetLastError());
    }
    UZL_HIP(hipStreamSynchronize(s));                      // `fresh` is pageable and goes out of scope; the staging area is free again
    h->tables.swap(tables);
    h->n_trig = n_trig;
    h->pairs.swap(host);
    h->total = total;
    h->have = true;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scanmerge_read(uzl_scanmerge* h, int32_t pair, int32_t cap, float* ranges, float* intensities, double* scan_center)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_pair_index(h, pair)) return rc;
    const PairHost& p = h->pairs[pair];
    if (cap < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    if (cap < p.n_a && (ranges || intensities)) return fail(h, UZL_ERR_TRUNCATED, "capacity below the number of beams");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    if (ranges) UZL_HIP(hipMemcpyAsync(ranges, h->d_ranges.p + p.out_off, (size_t)p.n_a * 4, hipMemcpyDeviceToHost, s));
    if (intensities) UZL_HIP(hipMemcpyAsync(intensities, h->d_intensities.p + p.out_off, (size_t)p.n_a * 4, hipMemcpyDeviceToHost, s));
    if (scan_center) UZL_HIP(hipMemcpyAsync(scan_center, h->d_centers.p + 3 * (size_t)pair, 3 * 8, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    return p.n_a;
    UZL_GUARD_END(h)
}

int uzl_scanmerge_points(uzl_scanmerge* h, int32_t pair, int32_t which, int32_t cap, int32_t* bin, float* rho)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_pair_index(h, pair)) return rc;
    if (which < 0 || which > 3) return fail(h, UZL_ERR_BAD_ARG, "which outside 0..3");
    const int32_t n = which < 2 ? h->pairs[pair].n_a : h->pairs[pair].n_b;
    if (cap < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    if (cap < n && (bin || rho)) return fail(h, UZL_ERR_TRUNCATED, "capacity below the number of beams");
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    h->d_st_bin.reserve(kScanMergeMaxBeams); h->d_st_rho.reserve(kScanMergeMaxBeams);
    ScanMergeArgs a = kernel_args(h);
    a.stage_pair = pair; a.stage_which = which; a.st_bin = h->d_st_bin.p; a.st_rho = h->d_st_rho.p;
    launch_scanmerge(a, 1, s);
    UZL_HIP(hipGetLastError());
    if (bin) UZL_HIP(hipMemcpyAsync(bin, a.st_bin, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    if (rho) UZL_HIP(hipMemcpyAsync(rho, a.st_rho, (size_t)n * 4, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    return n;
    UZL_GUARD_END(h)
}

int uzl_scanmerge_to_grid(uzl_scanmerge* h, uzl_grid* grid, const int32_t* nodes, int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    if (!grid) return fail(h, UZL_ERR_BAD_ARG, "null grid handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no run yet");
    // the scans are complete (run synchronises); the grid handle's lock is taken inside, after this handle's
    const std::vector<DeviceScan> scans = merged_scans(h);
    const int rc = grid_append_device_scans(grid, h->cfg.device, (int32_t)scans.size(), scans.data(), h->d_ranges.p, nodes, first_scan);
    if (rc != UZL_OK) return fail(h, rc, "the grid handle refused the scans (see its last_error)");
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scanmerge_to_laser(uzl_scanmerge* h, uzl_laser* laser, int32_t use_near, int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    if (!laser) return fail(h, UZL_ERR_BAD_ARG, "null laser handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no run yet");
    // the scans are complete (run synchronises); the laser handle's lock is taken inside, after this handle's
    const std::vector<DeviceScan> scans = merged_scans(h);
    const int rc = laser_append_device_scans(laser, h->cfg.device, (int32_t)scans.size(), scans.data(),
                                             use_near ? h->d_ranges.p : h->d_intensities.p, first_scan);
    if (rc != UZL_OK) return fail(h, rc, "the laser handle refused the scans (see its last_error)");
    return UZL_OK;
    UZL_GUARD_END(h)
}

}  // extern "C"
