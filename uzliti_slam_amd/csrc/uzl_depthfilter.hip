// uzl_depthfilter.hip — depth refinement and 3-D keypoint lifting (host + C ABI uzl_depthfilter_*).
//
// Mirrors the front end's depth path (feature_extraction_service_node.cpp:120-149: scale, jointBilateralFilter, jointNearestFilter)
// and FeatureExtractionCore::extract3dFeatures (feature_extraction_core.cpp:254-295); include/uzl_mi355x.h states the contract.  A
// refine checks every image, then moves depth and guide images to the device in chunks through two pinned staging halves (the host
// packs one half while the other half's copy and kernel run), each chunk's image records in front of its pixels so that a chunk
// is one copy; the refined images stay in HBM as compact f32, where uzl_depthfilter_lift gathers from them and
// uzl_depthfilter_to_laserline lets a laser-line handle bin them without a copy.
#include "cloud_types.hpp"
#include "depthfilter_types.hpp"
#include "image_stager.hpp"
#include "laserline_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>

namespace uzl {

constexpr size_t kDepthAlign = 64;                      // floats: every resident image starts on a 256-byte boundary

// A resident image: where it lies and what its depth image came with
struct DepthResident {
    int64_t off;              // first float in d_images
    int32_t width, height, group;
    double fx, fy, cx, cy;
    double T[12];
};

}  // namespace uzl

using namespace uzl;

struct uzl_depthfilter : HandleBase {
    uzl_depthfilter_cfg cfg;
    HandleStream stream;
    // the tables last uploaded (contract step 2)
    bool have_tables = false;
    int32_t table_radius = 0;
    double table_space = 0., table_color = 0.;
    DevBuf<float> d_tables;
    // the resident set
    bool have = false;
    std::vector<DepthResident> resident;
    DevBuf<float> d_images;
    // work
    ImageStager stage;
    PinBuf<uint8_t> h_lift;
    DevBuf<uint8_t> d_lift;
};

namespace {

int check_cfg(const uzl_depthfilter_cfg& c)
{
    if (c.radius < 0 || c.radius > kDepthMaxRadius || c.nearest_radius < 0 || c.nearest_radius > kDepthMaxNearest) return UZL_ERR_BAD_ARG;
    if (std::isnan(c.sigma_space) || std::isnan(c.sigma_color) || std::isnan(c.depth_scale) || !(c.depth_scale > 0.)) return UZL_ERR_BAD_ARG;
    return UZL_OK;
}

size_t guide_bytes(const uzl_guide_image& g) { return g.height <= 0 ? 0 : (size_t)(g.height - 1) * (size_t)g.step + (size_t)g.width; }

int check_guides(uzl_depthfilter* h, int32_t n, const uzl_depth_image* images, const uzl_guide_image* guides)
{
    if (!h->cfg.use_bilateral_filter) return UZL_OK;       // the guides are not read
    if (n > 0 && !guides) return fail(h, UZL_ERR_BAD_ARG, "null guides with the filter on");
    for (int32_t i = 0; i < n; i++) {
        const uzl_guide_image& g = guides[i];
        if (g.width != images[i].width || g.height != images[i].height) return fail(h, UZL_ERR_BAD_ARG, "a guide's size differs from its depth image's");
        if (g.width > 0 && (!g.data || g.step < g.width || (int64_t)g.height * g.step > INT32_MAX))
            return fail(h, UZL_ERR_BAD_ARG, "a guide without data, with a step smaller than a row, or height * step beyond 2^31");
    }
    return UZL_OK;
}

// contract step 2
void upload_tables(uzl_depthfilter* h)
{
    const int R = h->cfg.radius;
    const double ss = h->cfg.sigma_space <= 0. ? 1. : h->cfg.sigma_space, sc = h->cfg.sigma_color <= 0. ? 1. : h->cfg.sigma_color;
    if (h->have_tables && h->table_radius == R && h->table_space == ss && h->table_color == sc) return;
    std::vector<float> t(kDepthColours + 2 * R + 1);
    const double cc = -0.5 / (sc * sc), cs = -0.5 / (ss * ss);
    for (int i = 0; i < kDepthColours; i++) t[i] = (float)std::exp((double)(i * i) * cc);
    for (int k = -R; k <= R; k++) {
        const double r = (double)std::abs(k);
        t[kDepthColours + k + R] = (float)std::exp(r * r * cs);
    }
    h->have_tables = false;
    h->d_tables.reserve(kDepthColours + 2 * kDepthMaxRadius + 1);
    UZL_HIP(hipMemcpyAsync(h->d_tables.p, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));              // t is pageable and goes out of scope
    h->table_radius = R; h->table_space = ss; h->table_color = sc;
    h->have_tables = true;
}

// Images [i0, i1) through staging half `half`: records, depth and guide pixels packed, one copy, one launch.
void run_chunk(uzl_depthfilter* h, const uzl_depth_image* images, const uzl_guide_image* guides, int32_t i0, int32_t i1, int half)
{
    hipStream_t s = h->stream;
    const bool filter = h->cfg.use_bilateral_filter != 0;
    const size_t recs_bytes = align256((size_t)(i1 - i0) * sizeof(DepthImageRec));
    size_t total = recs_bytes;
    for (int32_t i = i0; i < i1; i++) total += align256(depth_image_bytes(images[i])) + (filter ? align256(guide_bytes(guides[i])) : 0);
    uint8_t* w = h->stage.open(half, total);
    DepthImageRec* recs = reinterpret_cast<DepthImageRec*>(w);
    size_t off = 0;
    int32_t max_width = 0, max_height = 0;
    for (int32_t i = i0; i < i1; i++) {
        const uzl_depth_image& im = images[i];
        DepthImageRec& r = recs[i - i0];
        r.width = im.width; r.height = im.height; r.depth_step = im.step; r.encoding = im.encoding; r._pad = 0;
        r.out_off = h->resident[i].off;
        r.depth_off = (int64_t)off;
        size_t nb = depth_image_bytes(im);
        if (nb) memcpy(w + recs_bytes + off, im.data, nb);
        off += align256(nb);
        r.guide_off = (int64_t)off;
        r.guide_step = 0;
        if (filter) {
            r.guide_step = guides[i].step;
            nb = guide_bytes(guides[i]);
            if (nb) memcpy(w + recs_bytes + off, guides[i].data, nb);
            off += align256(nb);
        }
        max_width = std::max(max_width, im.width);
        max_height = std::max(max_height, im.height);
    }
    const uint8_t* d = h->stage.send(half, total, s);
    DepthRefineArgs a;
    a.pixels = d + recs_bytes;
    a.images = reinterpret_cast<const DepthImageRec*>(d);
    a.tables = h->d_tables.p;
    a.out = h->d_images.p;
    a.depth_scale = h->cfg.depth_scale;
    a.radius = h->cfg.radius; a.nearest = h->cfg.nearest_radius; a.filter = filter ? 1 : 0;
    launch_depth_refine(a, (max_width + kDepthTileW - 1) / kDepthTileW, (max_height + kDepthTileH - 1) / kDepthTileH, i1 - i0, s);
    UZL_HIP(hipGetLastError());
}

}  // namespace

extern "C" {

void uzl_depthfilter_cfg_default(uzl_depthfilter_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->radius = 3; c->nearest_radius = 2; c->sigma_space = 3.0; c->sigma_color = 5.0; c->depth_scale = 1.0;
    c->use_bilateral_filter = 1; c->device = 0;
}

int uzl_depthfilter_create(const uzl_depthfilter_cfg* cfg, uzl_depthfilter** out)
{
    return create_handle(cfg, uzl_depthfilter_cfg_default, out, check_cfg, [](uzl_depthfilter* h) { h->stage.create(); });
}

void uzl_depthfilter_destroy(uzl_depthfilter* h) { destroy_handle(h); }

const char* uzl_depthfilter_last_error(uzl_depthfilter* h) { return last_error_of(h); }

int uzl_depthfilter_set_config(uzl_depthfilter* h, const uzl_depthfilter_cfg* cfg) { return set_config_of(h, cfg, check_cfg); }

int uzl_depthfilter_refine(uzl_depthfilter* h, int32_t n_images, const uzl_depth_image* images, const uzl_guide_image* guides)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = depth_images_check(h, n_images, images)) return rc;
    if (int rc = check_guides(h, n_images, images, guides)) return rc;
    std::vector<DepthResident> set((size_t)n_images);
    size_t floats = 0;
    for (int32_t i = 0; i < n_images; i++) {
        const uzl_depth_image& im = images[i];
        DepthResident& r = set[i];
        r.off = (int64_t)floats;
        r.width = im.width; r.height = im.height; r.group = im.group;
        r.fx = im.fx; r.fy = im.fy; r.cx = im.cx; r.cy = im.cy;
        memcpy(r.T, im.camera_transform, sizeof(r.T));
        floats += ((size_t)im.width * (size_t)im.height + kDepthAlign - 1) / kDepthAlign * kDepthAlign;
    }
    UZL_HIP(hipSetDevice(h->cfg.device));
    h->have = false;                                       // a failure below leaves no half-made set behind
    h->resident.swap(set);
    if (h->cfg.use_bilateral_filter) upload_tables(h);
    h->d_images.reserve(std::max<size_t>(floats, 1));
    const std::vector<int32_t> first = plan_chunks([&](int32_t i) {
        return align256(depth_image_bytes(images[i])) + (h->cfg.use_bilateral_filter ? align256(guide_bytes(guides[i])) : 0);
    }, n_images, kStageChunkBytes, kStageChunkImages);
    for (size_t k = 0; k + 1 < first.size(); k++) run_chunk(h, images, guides, first[k], first[k + 1], (int)(k & 1));
    UZL_HIP(hipStreamSynchronize(h->stream));              // the caller's images are free again, the set is complete
    h->have = true;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_depthfilter_image_count(uzl_depthfilter* h)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no refine yet");
    return (int)h->resident.size();
    UZL_GUARD_END(h)
}

int uzl_depthfilter_read(uzl_depthfilter* h, int32_t image, float* out, int64_t cap_pixels)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no refine yet");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    if (cap_pixels < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    const DepthResident& r = h->resident[image];
    const int64_t n = (int64_t)r.width * r.height;         // < 2^31: refine checked height * step
    if (!out) return (int)n;
    if (cap_pixels < n) return fail(h, UZL_ERR_TRUNCATED, "capacity below the number of pixels");
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (n) UZL_HIP(hipMemcpyAsync(out, h->d_images.p + r.off, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    return (int)n;
    UZL_GUARD_END(h)
}

}  // extern "C"

namespace {

// uzl_depthfilter_lift under the handle's lock.  The keypoints come from the host (u, v) or, with d_u, lie on the handle's device
// already (complete: the caller has synchronised the stream that made them).
int lift_locked(uzl_depthfilter* h, int32_t image, int32_t n, const int32_t* u, const int32_t* v, const int32_t* d_u, const int32_t* d_v,
                double max_depth, double* pos_xyz, uint8_t* valid3d)
{
    if (!h->have) return fail(h, UZL_ERR_STATE, "no refine yet");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    if (n < 0 || (n > 0 && ((!d_u && (!u || !v)) || !pos_xyz || !valid3d))) return fail(h, UZL_ERR_BAD_ARG, "bad keypoint count or null arrays");
    if (std::isnan(max_depth) || max_depth < 0.) return fail(h, UZL_ERR_BAD_ARG, "max_depth is NaN or negative");
    const DepthResident& r = h->resident[image];
    if (n > 0 && r.width == 0) return fail(h, UZL_ERR_BAD_ARG, "keypoints on a 0 x 0 image");
    if (n == 0) return UZL_OK;
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    // staging: u, v in; pos, valid out (pos first: 8-byte aligned)
    const size_t in_bytes = (size_t)n * 8, pos_bytes = (size_t)n * 24, all = in_bytes + pos_bytes + (size_t)n;
    h->h_lift.reserve(all);
    h->d_lift.reserve(all);
    uint8_t* w = h->h_lift.p;
    uint8_t* d = h->d_lift.p;
    if (!d_u) {
        memcpy(w + pos_bytes, u, (size_t)n * 4);
        memcpy(w + pos_bytes + (size_t)n * 4, v, (size_t)n * 4);
        UZL_HIP(hipMemcpyAsync(d + pos_bytes, w + pos_bytes, in_bytes, hipMemcpyHostToDevice, s));
    }
    DepthLiftArgs a;
    a.image = h->d_images.p + r.off;
    a.pos = reinterpret_cast<double*>(d);
    a.u = d_u ? d_u : reinterpret_cast<const int32_t*>(d + pos_bytes);
    a.v = d_u ? d_v : a.u + n;
    a.valid = d + pos_bytes + in_bytes;
    a.fx = r.fx; a.fy = r.fy; a.cx = r.cx; a.cy = r.cy; a.max_depth = max_depth;
    a.width = r.width; a.height = r.height; a.n = n;
    launch_depth_lift(a, s);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipMemcpyAsync(w, d, pos_bytes, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(w + pos_bytes + in_bytes, d + pos_bytes + in_bytes, (size_t)n, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    memcpy(pos_xyz, w, pos_bytes);
    memcpy(valid3d, w + pos_bytes + in_bytes, (size_t)n);
    return UZL_OK;
}

}  // namespace

namespace uzl {

int depthfilter_lift_device(uzl_depthfilter* h, int device, int32_t image, int32_t n, const int32_t* d_u, const int32_t* d_v,
                            double max_depth, double* pos_xyz, uint8_t* valid3d)
{
    UZL_GUARD_BEGIN(h)
    if (device != h->cfg.device) return fail(h, UZL_ERR_BAD_ARG, "the keypoints lie on another device");
    if (n > 0 && (!d_u || !d_v)) return fail(h, UZL_ERR_BAD_ARG, "null device keypoints");
    return lift_locked(h, image, n, nullptr, nullptr, d_u, d_v, max_depth, pos_xyz, valid3d);
    UZL_GUARD_END(h)
}

}  // namespace uzl

extern "C" {

int uzl_depthfilter_lift(uzl_depthfilter* h, int32_t image, int32_t n, const int32_t* u, const int32_t* v, double max_depth,
                         double* pos_xyz, uint8_t* valid3d)
{
    UZL_GUARD_BEGIN(h)
    return lift_locked(h, image, n, u, v, nullptr, nullptr, max_depth, pos_xyz, valid3d);
    UZL_GUARD_END(h)
}

int uzl_depthfilter_to_laserline(uzl_depthfilter* h, uzl_laserline* laserline, int32_t* n_scans, int32_t* n_beams)
{
    UZL_GUARD_BEGIN(h)
    if (!laserline) return fail(h, UZL_ERR_BAD_ARG, "null laser-line handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no refine yet");
    const int32_t n = (int32_t)h->resident.size();
    std::vector<LaserImageRec> recs((size_t)n);
    std::vector<int32_t> groups((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const DepthResident& r = h->resident[i];
        LaserImageRec& l = recs[i];
        l.data_off = r.off * (int64_t)sizeof(float);
        l.width = r.width; l.height = r.height; l.step = r.width * (int32_t)sizeof(float); l.encoding = UZL_DEPTH_F32_M;
        l.lanes = 0; l.out = i;
        l.fx = r.fx; l.fy = r.fy; l.cx = r.cx; l.cy = r.cy;
        for (int k = 0; k < 12; k++) l.T[k] = (float)r.T[k];
        groups[i] = r.group;
    }
    // the images are complete (refine synchronises) and stay while this handle's lock is held; the laser-line handle's lock is
    // taken inside, after this handle's
    const int rc = laserline_extract_device(laserline, h->cfg.device, n, recs.data(), groups.data(),
                                            reinterpret_cast<const uint8_t*>(h->d_images.p), n_scans, n_beams);
    if (rc != UZL_OK) return fail(h, rc, "the laser-line handle refused the images (see its last_error)");
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_depthfilter_to_cloud(uzl_depthfilter* h, uzl_cloud* cloud, const uzl_color_image* colors, int32_t* first_cloud)
{
    UZL_GUARD_BEGIN(h)
    if (!cloud) return fail(h, UZL_ERR_BAD_ARG, "null cloud handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no refine yet");
    const int32_t n = (int32_t)h->resident.size();
    if (n > 0 && !colors) return fail(h, UZL_ERR_BAD_ARG, "null colour images");
    std::vector<uzl_depth_image> geom((size_t)n);
    std::vector<const float*> d_depth((size_t)n);
    for (int32_t i = 0; i < n; i++) {
        const DepthResident& r = h->resident[i];
        uzl_depth_image& g = geom[i];
        memset(&g, 0, sizeof(g));
        g.encoding = UZL_DEPTH_F32_M; g.width = r.width; g.height = r.height; g.step = 4 * r.width;
        g.fx = r.fx; g.fy = r.fy; g.cx = r.cx; g.cy = r.cy;
        d_depth[i] = h->d_images.p + r.off;
    }
    // the images are complete (refine synchronises) and stay while this handle's lock is held; the cloud handle's lock is taken
    // inside, after this handle's
    const int rc = cloud_add_device_images(cloud, h->cfg.device, n, geom.data(), d_depth.data(), colors, first_cloud);
    if (rc != UZL_OK) return fail(h, rc, "the cloud handle refused the images (see its last_error)");
    return UZL_OK;
    UZL_GUARD_END(h)
}

}  // extern "C"
