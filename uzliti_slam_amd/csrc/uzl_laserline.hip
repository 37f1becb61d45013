// uzl_laserline.hip — laser line from depth images (host + C ABI uzl_laserline_*).
//
// Mirrors GraphGridMapper::extractImageLaserLine / mergeLaserScans / scanMean (map_projection/src/graph_grid_mapper.cpp:420-468,
// 135-212, 605-621); include/uzl_mi355x.h states the contract.  An extract checks every image, then moves the images to the device
// in chunks through two pinned staging halves (the host packs one half while the other half's copy and bin kernel run), each
// chunk's image records in front of its pixels so that a chunk is one copy; the per-image bins (min s / max s, u32) and the scans
// stay in HBM, and uzl_laserline_to_grid hands the scans to a grid handle's store without leaving the device.
#include "grid_types.hpp"
#include "image_stager.hpp"
#include "laser_types.hpp"
#include "laserline_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>

namespace uzl {

// contract step 1
struct LaserGrid {
    float amin, amax, inc;
    int32_t n;
};

}  // namespace uzl

using namespace uzl;

struct uzl_laserline : HandleBase {
    uzl_laserline_cfg cfg;
    HandleStream stream;
    // the table of the angular grid last used
    bool have_table = false;
    LaserGrid table_grid{};
    DevBuf<double2> d_trig;
    // the resident result and the grid it was made with
    bool have = false;
    int32_t n_scans = 0;
    LaserGrid grid{};
    float lo = 0.f, hi0 = 0.f;
    DevBuf<float> d_ranges, d_intensities;
    DevBuf<double> d_centers;
    // work
    ImageStager stage;
    DevBuf<uint32_t> d_smin, d_smax;
    DevBuf<int32_t> d_first;
};

namespace {

bool angular_grid(const uzl_laserline_cfg& c, LaserGrid* g)
{
    g->amin = (float)(-M_PI);
    g->amax = (float)M_PI;
    g->inc = (float)c.angle_increment;
    const float nf = ceilf((g->amax - g->amin) / g->inc);
    if (!(nf >= 8.f) || !(nf <= (float)kLaserMaxBeams)) return false;
    g->n = (int32_t)(uint32_t)nf;
    return true;
}

int check_cfg(const uzl_laserline_cfg& c)
{
    if (std::isnan(c.min_height) || std::isnan(c.max_height) || std::isnan(c.angle_increment) || std::isnan(c.range_min) ||
        std::isnan(c.range_max) || std::isnan(c.depth_scale))
        return UZL_ERR_BAD_ARG;
    if (c.range_max < c.range_min || c.range_min < 0. || !(c.depth_scale > 0.)) return UZL_ERR_BAD_ARG;
    LaserGrid g;
    return angular_grid(c, &g) ? UZL_OK : UZL_ERR_BAD_ARG;
}

int bytes_per_pixel(int32_t encoding) { return encoding == UZL_DEPTH_F32_M ? 4 : 2; }

}  // namespace

size_t uzl::depth_image_bytes(const uzl_depth_image& im)
{
    if (im.height <= 0) return 0;
    return (size_t)(im.height - 1) * (size_t)im.step + (size_t)im.width * bytes_per_pixel(im.encoding);
}

int uzl::depth_images_check(HandleBase* h, int32_t n, const uzl_depth_image* images)
{
    if (n < 0 || (n > 0 && !images)) return fail(h, UZL_ERR_BAD_ARG, "bad image count or null images");
    for (int32_t i = 0; i < n; i++) {
        const uzl_depth_image& im = images[i];
        if (im.encoding != UZL_DEPTH_F32_M && im.encoding != UZL_DEPTH_U16_MM) return fail(h, UZL_ERR_BAD_ARG, "unknown depth encoding");
        const bool empty = im.width == 0 && im.height == 0 && !im.data, full = im.width > 0 && im.height > 0 && im.data;
        if (!empty && !full) return fail(h, UZL_ERR_BAD_ARG, "an image is width, height > 0 with data or 0 x 0 without");
        if (full && ((int64_t)im.step < (int64_t)im.width * bytes_per_pixel(im.encoding) || (int64_t)im.height * im.step > INT32_MAX))
            return fail(h, UZL_ERR_BAD_ARG, "step smaller than a row, or height * step beyond 2^31");
        if (!std::isfinite(im.fx) || !std::isfinite(im.fy) || im.fx == 0. || im.fy == 0. || !std::isfinite(im.cx) || !std::isfinite(im.cy))
            return fail(h, UZL_ERR_BAD_ARG, "fx / fy zero or non-finite, or cx / cy non-finite");
        if (!finite12(im.camera_transform)) return fail(h, UZL_ERR_BAD_ARG, "non-finite camera_transform entry");
        if (i > 0 && im.group != images[i - 1].group && im.group != images[i - 1].group + 1)
            return fail(h, UZL_ERR_BAD_ARG, "groups are not ascending and contiguous");
    }
    return UZL_OK;
}

namespace {

// Lanes across a row of nvec vectors: among 1..8 passes over the row, the split that keeps most of the workgroup's lanes busy
// (kLaserBlock / lanes rows are walked side by side).
int32_t lanes_for(int nvec)
{
    int32_t best = 1;
    double best_use = 0.;
    for (int passes = 1; passes <= 8; passes++) {
        const int lanes = (nvec + passes - 1) / passes;
        if (lanes < 1 || lanes > kLaserBlock) continue;
        const double use = (double)nvec / ((double)passes * lanes) * (double)(lanes * (kLaserBlock / lanes)) / kLaserBlock;
        if (use > best_use) { best_use = use; best = lanes; }
    }
    return best_use > 0. ? best : kLaserBlock;
}

void upload_table(uzl_laserline* h, const LaserGrid& g)
{
    if (h->have_table && h->table_grid.n == g.n && memcmp(&h->table_grid.inc, &g.inc, 4) == 0) return;
    std::vector<double2> trig((size_t)g.n + 1);
    for (int32_t k = 0; k <= g.n; k++) {
        const double th = (double)g.amin + (double)k * (double)g.inc;
        trig[k] = make_double2(std::cos(th), std::sin(th));
    }
    h->have_table = false;
    h->d_trig.reserve(trig.size());
    UZL_HIP(hipMemcpyAsync(h->d_trig.p, trig.data(), trig.size() * sizeof(double2), hipMemcpyHostToDevice, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));              // trig is pageable and goes out of scope
    h->table_grid = g;
    h->have_table = true;
}

// One launch of the bin kernel over `count` image records on the device, their pixels at d_pixels (`rows` rows in all).
void launch_bin(uzl_laserline* h, const LaserImageRec* d_recs, const uint8_t* d_pixels, int32_t count, int64_t rows, int32_t max_height,
                const LaserGrid& g)
{
    LaserBinArgs a;
    a.pixels = d_pixels;
    a.images = d_recs;
    a.trig = h->d_trig.p;
    a.smin = h->d_smin.p; a.smax = h->d_smax.p;
    a.min_height = h->cfg.min_height; a.max_height = h->cfg.max_height; a.depth_scale = h->cfg.depth_scale;
    a.amin = g.amin; a.inc = g.inc; a.n = g.n;
    // bands: about 2,048 workgroups per chunk, 8 to 64 rows each (any split gives the same bins)
    a.band_rows = (int32_t)std::min<int64_t>(std::max<int64_t>((rows + 2047) / 2048, 8), 64);
    launch_laser_bin(a, (max_height + a.band_rows - 1) / a.band_rows, count, h->stream);
    UZL_HIP(hipGetLastError());
}

// Images [i0, i1) through staging half `half`: records and pixels packed, one copy, one launch of the bin kernel.
void run_chunk(uzl_laserline* h, const uzl_depth_image* images, int32_t i0, int32_t i1, int half, const LaserGrid& g)
{
    const size_t recs_bytes = align256((size_t)(i1 - i0) * sizeof(LaserImageRec));
    size_t total = recs_bytes;
    int64_t rows = 0;
    for (int32_t i = i0; i < i1; i++) { total += align256(depth_image_bytes(images[i])); rows += images[i].height; }
    uint8_t* w = h->stage.open(half, total);
    LaserImageRec* recs = reinterpret_cast<LaserImageRec*>(w);
    size_t off = 0;
    int32_t max_height = 0;
    for (int32_t i = i0; i < i1; i++) {
        const uzl_depth_image& im = images[i];
        LaserImageRec& r = recs[i - i0];
        r.data_off = (int64_t)off;
        r.width = im.width; r.height = im.height; r.step = im.step; r.encoding = im.encoding;
        r.lanes = lanes_for((im.width + kLaserVec - 1) / kLaserVec);
        r.out = i;
        r.fx = im.fx; r.fy = im.fy; r.cx = im.cx; r.cy = im.cy;
        for (int k = 0; k < 12; k++) r.T[k] = (float)im.camera_transform[k];
        const size_t nb = depth_image_bytes(im);
        if (nb) memcpy(w + recs_bytes + off, im.data, nb);
        off += align256(nb);
        max_height = std::max(max_height, im.height);
    }
    const uint8_t* d = h->stage.send(half, total, h->stream);
    launch_bin(h, reinterpret_cast<const LaserImageRec*>(d), d + recs_bytes, i1 - i0, rows, max_height, g);
}

// Steps 1-9 over n_images images, image i in group group_of(i): feed(grid) queues the bin launches of every image on the handle's
// stream (from the host through the staging halves, or over pixels that already lie on the device); the rest is the same.
template <typename GroupOf, typename Feed>
void extract_with(uzl_laserline* h, int32_t n_images, GroupOf&& group_of, Feed&& feed, int32_t* n_scans, int32_t* n_beams)
{
    LaserGrid g;
    angular_grid(h->cfg, &g);
    std::vector<int32_t> first;                            // images first[s] .. first[s + 1] make scan s
    for (int32_t i = 0; i < n_images; i++)
        if (i == 0 || group_of(i) != group_of(i - 1)) first.push_back(i);
    const int32_t ns = (int32_t)first.size();
    first.push_back(n_images);
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    h->have = false;                                       // a failure below leaves no half-made result behind
    upload_table(h, g);
    const size_t bins = (size_t)n_images * g.n, beams = (size_t)ns * g.n;
    h->d_smin.reserve(std::max<size_t>(bins, 1)); h->d_smax.reserve(std::max<size_t>(bins, 1));
    h->d_ranges.reserve(std::max<size_t>(beams, 1)); h->d_intensities.reserve(std::max<size_t>(beams, 1));
    h->d_centers.reserve(std::max<size_t>(3 * (size_t)ns, 1));
    h->d_first.reserve(first.size());
    if (bins) {
        UZL_HIP(hipMemsetD32Async((hipDeviceptr_t)h->d_smin.p, (int)kLaserInfBits, bins, s));
        UZL_HIP(hipMemsetAsync(h->d_smax.p, 0, bins * 4, s));
    }
    feed(g);
    if (ns) {
        UZL_HIP(hipMemcpyAsync(h->d_first.p, first.data(), first.size() * 4, hipMemcpyHostToDevice, s));
        LaserFinishArgs f;
        f.smin = h->d_smin.p; f.smax = h->d_smax.p; f.group_first = h->d_first.p; f.trig = h->d_trig.p;
        f.ranges = h->d_ranges.p; f.intensities = h->d_intensities.p; f.centers = h->d_centers.p;
        f.lo = (float)h->cfg.range_min; f.hi0 = (float)h->cfg.range_max; f.n = g.n;
        launch_laser_finish(f, ns, s);
        UZL_HIP(hipGetLastError());
    }
    UZL_HIP(hipStreamSynchronize(s));                      // `first` and the caller's images are free again
    h->n_scans = ns;
    h->grid = g;
    h->lo = (float)h->cfg.range_min;
    h->hi0 = (float)h->cfg.range_max;
    h->have = true;
    if (n_scans) *n_scans = ns;
    if (n_beams) *n_beams = g.n;
}

}  // namespace

extern "C" {

void uzl_laserline_cfg_default(uzl_laserline_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->min_height = 0.0; c->max_height = 1.0; c->angle_increment = M_PI / 360.0; c->range_min = 0.45; c->range_max = 5.0;
    c->depth_scale = 1.0; c->device = 0;
}

int uzl_laserline_create(const uzl_laserline_cfg* cfg, uzl_laserline** out)
{
    return create_handle(cfg, uzl_laserline_cfg_default, out, check_cfg, [](uzl_laserline* h) { h->stage.create(); laser_prepare(); });
}

void uzl_laserline_destroy(uzl_laserline* h) { destroy_handle(h); }

const char* uzl_laserline_last_error(uzl_laserline* h) { return last_error_of(h); }

int uzl_laserline_set_config(uzl_laserline* h, const uzl_laserline_cfg* cfg) { return set_config_of(h, cfg, check_cfg); }

int uzl_laserline_extract(uzl_laserline* h, int32_t n_images, const uzl_depth_image* images, int32_t* n_scans, int32_t* n_beams)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = depth_images_check(h, n_images, images)) return rc;
    extract_with(h, n_images, [&](int32_t i) { return images[i].group; }, [&](const LaserGrid& g) {
        const std::vector<int32_t> first = plan_chunks([&](int32_t i) { return align256(depth_image_bytes(images[i])); }, n_images,
                                                       kStageChunkBytes, kStageChunkImages);
        for (size_t k = 0; k + 1 < first.size(); k++) run_chunk(h, images, first[k], first[k + 1], (int)(k & 1), g);
    }, n_scans, n_beams);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_laserline_read(uzl_laserline* h, int32_t cap_scans, float* ranges, float* intensities, double* scan_center)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    if (cap_scans < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    if (cap_scans < h->n_scans) return fail(h, UZL_ERR_TRUNCATED, "capacity below the number of scans");
    const size_t beams = (size_t)h->n_scans * h->grid.n;
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (beams && ranges) UZL_HIP(hipMemcpyAsync(ranges, h->d_ranges.p, beams * 4, hipMemcpyDeviceToHost, h->stream));
    if (beams && intensities) UZL_HIP(hipMemcpyAsync(intensities, h->d_intensities.p, beams * 4, hipMemcpyDeviceToHost, h->stream));
    if (h->n_scans && scan_center)
        UZL_HIP(hipMemcpyAsync(scan_center, h->d_centers.p, 3 * (size_t)h->n_scans * 8, hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    return h->n_scans;
    UZL_GUARD_END(h)
}

int uzl_laserline_to_grid(uzl_laserline* h, uzl_grid* grid, const int32_t* nodes, int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    if (!grid) return fail(h, UZL_ERR_BAD_ARG, "null grid handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    // the scans are complete (extract synchronises); the grid handle's lock is taken inside, after this handle's
    const int rc = grid_append_device(grid, h->cfg.device, h->n_scans, h->grid.n, h->d_ranges.p, h->grid.amin, h->grid.inc, h->lo,
                                      nodes, first_scan);
    if (rc != UZL_OK) return fail(h, rc, "the grid handle refused the scans (see its last_error)");
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_laserline_to_laser(uzl_laserline* h, uzl_laser* laser, int32_t use_near, int32_t* first_scan)
{
    UZL_GUARD_BEGIN(h)
    if (!laser) return fail(h, UZL_ERR_BAD_ARG, "null laser handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    // the scans are complete (extract synchronises); the laser handle's lock is taken inside, after this handle's
    const int rc = laser_append_device(laser, h->cfg.device, h->n_scans, h->grid.n, use_near ? h->d_ranges.p : h->d_intensities.p,
                                       h->grid.amin, h->grid.inc, h->lo, h->hi0, first_scan);
    if (rc != UZL_OK) return fail(h, rc, "the laser handle refused the scans (see its last_error)");
    return UZL_OK;
    UZL_GUARD_END(h)
}

}  // extern "C"

int uzl::laserline_extract_device(uzl_laserline* h, int device, int32_t n_images, LaserImageRec* recs, const int32_t* groups,
                                  const uint8_t* d_pixels, int32_t* n_scans, int32_t* n_beams)
{
    UZL_GUARD_BEGIN(h)
    if (device != h->cfg.device) return fail(h, UZL_ERR_BAD_ARG, "the images are on another device than the laser-line handle");
    if (h->cfg.depth_scale != 1.0) return fail(h, UZL_ERR_BAD_ARG, "depth_scale must be 1: the images on the device are already scaled");
    if (n_images < 0 || (n_images > 0 && (!recs || !groups || !d_pixels))) return fail(h, UZL_ERR_BAD_ARG, "bad image count or null images");
    extract_with(h, n_images, [&](int32_t i) { return groups[i]; }, [&](const LaserGrid& g) {
        if (n_images == 0) return;
        // all records in one copy through staging half 0, then one launch per kStageChunkImages of them
        const size_t bytes = (size_t)n_images * sizeof(LaserImageRec);
        uint8_t* w = h->stage.open(0, bytes);
        for (int32_t i = 0; i < n_images; i++) {
            recs[i].lanes = lanes_for((recs[i].width + kLaserVec - 1) / kLaserVec);
            recs[i].out = i;
        }
        memcpy(w, recs, bytes);
        const LaserImageRec* d_recs = reinterpret_cast<const LaserImageRec*>(h->stage.send(0, bytes, h->stream));
        for (int32_t i0 = 0; i0 < n_images; i0 += kStageChunkImages) {
            const int32_t i1 = std::min(n_images, i0 + kStageChunkImages);
            int64_t rows = 0;
            int32_t max_height = 0;
            for (int32_t i = i0; i < i1; i++) { rows += recs[i].height; max_height = std::max(max_height, recs[i].height); }
            launch_bin(h, d_recs + i0, d_pixels, i1 - i0, rows, max_height, g);
        }
    }, n_scans, n_beams);
    return UZL_OK;
    UZL_GUARD_END(h)
}

#ifdef UZL_DIAG
// Test hook (tests/test_stage_chunks_cpu.py): plan_chunks over n items of bytes[i] bytes each.  first_out, with room for n + 1
// entries, takes the boundaries; returns the number of chunks, or -1 for arguments plan_chunks does not take.
extern "C" UZL_DIAG_EXPORT int uzl_debug_plan_chunks(int32_t n, const int64_t* bytes, int64_t max_bytes, int32_t max_items, int32_t* first_out)
{
    if (n < 0 || (n > 0 && !bytes) || max_bytes < 0 || max_items < 1 || !first_out) return -1;
    for (int32_t i = 0; i < n; i++) if (bytes[i] < 0) return -1;
    const std::vector<int32_t> first = uzl::plan_chunks([&](int32_t i) { return (size_t)bytes[i]; }, n, (size_t)max_bytes, max_items);
    std::copy(first.begin(), first.end(), first_out);
    return (int)first.size() - 1;
}
#endif
