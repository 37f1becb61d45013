// uzl_orb.hip — ORB keypoints, descriptors and binary GIST from grey images (host + C ABI uzl_orb_*).
//
// Mirrors FeatureExtractionCore::extractFeatures and ::extractBinaryGist (feature_extraction_core.cpp:93-102, 119-162) over
// cv::AORB (feature_extraction/external/aorb/aorb.cpp); include/uzl_mi355x.h states the contract.  An extract checks every image,
// lays out every unit (grid cell or whole image), level and buffer on the host - sizes only, no pixel is touched - and moves images
// and masks to the device in chunks through the image stager, each chunk's records in front of its pixels so that a chunk is one
// copy.  A chunk then takes a fixed sequence of launches (orb_kernels.hip) with no host round trip between them; keypoints,
// descriptors, counts and gists stay in HBM, sized for the most a level can keep (ties are never cut), until a read asks for them.
#include "depthfilter_types.hpp"
#include "image_stager.hpp"
#include "orb_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>

namespace uzl {

// A resident image: where its keypoints lie
struct OrbResident {
    int64_t kp_off;
    int32_t kp_cap, width, height;
};

}  // namespace uzl

using namespace uzl;

struct uzl_orb : HandleBase {
    uzl_orb_cfg cfg;
    HandleStream stream;
    DevBuf<int8_t> d_pattern;
    // the resident set
    bool have = false, have_gist = false, have_counts = false;
    std::vector<OrbResident> resident;
    std::vector<uint32_t> counts;              // fetched by the first read after an extract
    DevBuf<OrbKp> d_kp;
    DevBuf<uint8_t> d_desc, d_gist;
    DevBuf<uint32_t> d_count;
    // work
    ImageStager stage;
    DevBuf<uint8_t> d_pyr, d_blur, d_cand_score;
    DevBuf<uint2> d_cand_xy;
    DevBuf<uint32_t> d_counters;               // hist, n_cand, thr of one chunk
    DevBuf<OrbKp> d_kp_tmp;
    PinBuf<uint8_t> h_read;
    DevBuf<int32_t> d_uv;
    // the last staging chunk as its launches saw it (the stage entry): its records, its first image, its grid and level count
    std::vector<OrbImage> chunk_images;
    std::vector<OrbUnit> chunk_units;
    int32_t chunk_first = 0, chunk_cells = 0, chunk_levels = 0;
};

namespace {

int check_cfg(const uzl_orb_cfg& c)
{
    if (c.patch_size != 31 || c.edge_threshold < 19) return UZL_ERR_BAD_ARG;
    if (c.n_levels < 1 || c.n_levels > kOrbMaxLevels || !(c.scale_factor > 1.0f) || !(c.scale_factor <= 2.0f)) return UZL_ERR_BAD_ARG;
    if (c.fast_threshold < 1 || c.fast_threshold > 254) return UZL_ERR_BAD_ARG;
    if (c.number_of_features < 1 || c.grid_rows < 1 || c.grid_rows > 8 || c.grid_cols < 1 || c.grid_cols > 8) return UZL_ERR_BAD_ARG;
    if (c.gist_size != kOrbGist) return UZL_ERR_BAD_ARG;
    return UZL_OK;
}

size_t mono_bytes(const uzl_guide_image& g) { return g.height <= 0 ? 0 : (size_t)(g.height - 1) * (size_t)g.step + (size_t)g.width; }

bool mono_ok(const uzl_guide_image& g)
{
    if (g.width == 0 && g.height == 0) return true;
    return g.width > 0 && g.height > 0 && g.data && g.step >= g.width && (int64_t)g.height * g.step <= INT32_MAX;
}

// cvRound of an f32 on the host (the rounding mode is the default one: half to even)
int rnd(float x) { return (int)std::nearbyint((double)x); }

// What the config fixes for every image: contract steps 2, 6 and 8
struct OrbPlan {
    float level_scale[kOrbMaxLevels];
    int32_t n_per_level[kOrbMaxLevels];
    int32_t n_per_cell;
};

OrbPlan plan_of(const uzl_orb_cfg& c)
{
    OrbPlan p{};
    for (int l = 0; l < kOrbMaxLevels; l++) p.level_scale[l] = (float)std::pow((double)c.scale_factor, (double)l);
    // aorb.cpp:620-633 with nfeatures = 2 * number_of_features
    const int nfeatures = 2 * c.number_of_features;
    const float factor = (float)(1.0 / (double)c.scale_factor);
    float per_scale = (float)nfeatures * (1.f - factor) / (1.f - (float)std::pow((double)factor, (double)c.n_levels));
    int sum = 0;
    for (int l = 0; l < c.n_levels - 1; l++) {
        p.n_per_level[l] = rnd(per_scale);
        sum += p.n_per_level[l];
        per_scale = per_scale * factor;
    }
    p.n_per_level[c.n_levels - 1] = std::max(nfeatures - sum, 0);
    p.n_per_cell = c.number_of_features / (c.grid_rows * c.grid_cols);
    return p;
}

int level_dim(int n, float level_scale) { return rnd((float)n * (1.0f / level_scale)); }

// the most strict 3 x 3 maxima the border leaves on a w x h level: one per 2 x 2 block
int64_t cand_cap_of(int w, int h, int edge)
{
    const int64_t rw = (int64_t)w - 2 * edge, rh = (int64_t)h - 2 * edge;
    return rw <= 0 || rh <= 0 ? 0 : ((rw + 1) / 2) * ((rh + 1) / 2);
}

void cell_rect(const uzl_orb_cfg& c, int W, int H, int cell, int* x0, int* y0, int* w, int* h)
{
    const int64_t i = cell / c.grid_cols, j = cell % c.grid_cols;
    *y0 = (int)(i * H / c.grid_rows); *h = (int)((i + 1) * H / c.grid_rows) - *y0;
    *x0 = (int)(j * W / c.grid_cols); *w = (int)((j + 1) * W / c.grid_cols) - *x0;
}

int64_t kp_cap_of(const uzl_orb_cfg& c, const OrbPlan& p, int W, int H)
{
    int64_t cap = 0;
    for (int cell = 0; cell < c.grid_rows * c.grid_cols; cell++) {
        int x0, y0, w, h;
        cell_rect(c, W, H, cell, &x0, &y0, &w, &h);
        for (int l = 0; l < c.n_levels; l++) cap += cand_cap_of(level_dim(w, p.level_scale[l]), level_dim(h, p.level_scale[l]), c.edge_threshold);
    }
    return cap;
}

// Images [i0, i1) through staging half `half`: records, images and masks packed, one copy, the chunk's launches.
void run_chunk(uzl_orb* h, const OrbPlan& plan, const uzl_guide_image* images, const uzl_guide_image* masks, const float* angles,
               int32_t i0, int32_t i1, int half)
{
    hipStream_t s = h->stream;
    const uzl_orb_cfg& c = h->cfg;
    const int ni = i1 - i0, cells = c.grid_rows * c.grid_cols, L = c.n_levels;
    const int n_cell_units = ni * cells, n_units = n_cell_units + ni;
    const size_t images_bytes = align256((size_t)ni * sizeof(OrbImage)), recs_bytes = images_bytes + align256((size_t)n_units * sizeof(OrbUnit));
    size_t total = recs_bytes;
    for (int32_t i = i0; i < i1; i++) total += align256(mono_bytes(images[i])) + (masks ? align256(mono_bytes(masks[i])) : 0);
    uint8_t* w = h->stage.open(half, total);
    memset(w, 0, recs_bytes);
    OrbImage* ims = reinterpret_cast<OrbImage*>(w);
    OrbUnit* units = reinterpret_cast<OrbUnit*>(w + images_bytes);
    size_t off = 0, pyr = 0, blur = 0;
    int64_t cand = 0, tmp = 0;
    int max_w = 1, max_h = 1, max_cw = 1, max_ch = 1;
    int64_t max_cand = 1, max_kp = 1;
    for (int32_t i = i0; i < i1; i++) {
        const uzl_guide_image& im = images[i];
        const bool masked = masks && im.width > 0;
        OrbImage& r = ims[i - i0];
        const OrbResident& res = h->resident[i];
        r.kp_off = res.kp_off; r.kp_cap = res.kp_cap; r.tmp_off = tmp; r.width = im.width; r.height = im.height; r.slot = i;
        r.whole = n_cell_units + (i - i0);
        r.gist_angle = angles ? angles[i] : 0.f;
        tmp += res.kp_cap;
        max_kp = std::max<int64_t>(max_kp, res.kp_cap);
        const size_t img_off = off;
        size_t nb = mono_bytes(im);
        if (nb) memcpy(w + recs_bytes + off, im.data, nb);
        off += align256(nb);
        const size_t mask_off = off;
        if (masks) {
            nb = mono_bytes(masks[i]);
            if (nb) memcpy(w + recs_bytes + off, masks[i].data, nb);
            off += align256(nb);
        }
        max_w = std::max(max_w, im.width); max_h = std::max(max_h, im.height);
        for (int k = 0; k <= cells; k++) {                  // the cells, then the whole image
            const bool whole = k == cells;
            OrbUnit& u = units[whole ? r.whole : (i - i0) * cells + k];
            int x0 = 0, y0 = 0, cw = im.width, ch = im.height;
            if (!whole) cell_rect(c, im.width, im.height, k, &x0, &y0, &cw, &ch);
            u.image = i - i0; u.x0 = x0; u.y0 = y0; u.has_mask = masked && !whole ? 1 : 0;
            if (!whole) { max_cw = std::max(max_cw, cw); max_ch = std::max(max_ch, ch); }
            for (int l = 0; l < L; l++) {
                OrbLevel& v = u.lev[l];
                v.w = l == 0 ? cw : level_dim(cw, plan.level_scale[l]);
                v.h = l == 0 ? ch : level_dim(ch, plan.level_scale[l]);
                if (l == 0) {
                    v.step = im.step; v.img_off = (int64_t)(img_off + (size_t)y0 * (size_t)im.step + (size_t)x0);
                    if (u.has_mask) { v.mask_step = masks[i].step; v.mask_off = (int64_t)(mask_off + (size_t)y0 * (size_t)masks[i].step + (size_t)x0); }
                } else {
                    v.step = v.w; v.img_off = (int64_t)pyr; pyr += align256((size_t)v.w * (size_t)v.h);
                    if (u.has_mask) { v.mask_step = v.w; v.mask_off = (int64_t)pyr; pyr += align256((size_t)v.w * (size_t)v.h); }
                }
                if (whole) { v.blur_off = (int64_t)blur; blur += align256((size_t)v.w * (size_t)v.h); }
                else {
                    v.cand_off = cand; v.cand_cap = (int32_t)cand_cap_of(v.w, v.h, c.edge_threshold);
                    cand += v.cand_cap;
                    max_cand = std::max<int64_t>(max_cand, v.cand_cap);
                }
            }
        }
        r.gist_off = (int64_t)pyr; pyr += align256((size_t)kOrbGist * kOrbGist);
        r.gist_blur_off = (int64_t)blur; blur += align256((size_t)kOrbGist * kOrbGist);
    }
    const size_t jobs = (size_t)n_cell_units * (size_t)L, n_counters = jobs * (kOrbBins + 2);
    h->d_pyr.reserve(std::max<size_t>(pyr, 1));
    h->d_blur.reserve(std::max<size_t>(blur, 1));
    h->d_cand_xy.reserve(std::max<size_t>((size_t)cand, 1));
    h->d_cand_score.reserve(std::max<size_t>((size_t)cand, 1));
    h->d_kp_tmp.reserve(std::max<size_t>((size_t)tmp, 1));
    h->d_counters.reserve(std::max<size_t>(n_counters, 1));
    h->chunk_images.assign(ims, ims + ni);                 // the work buffers belong to this chunk until the next one
    h->chunk_units.assign(units, units + n_units);
    h->chunk_first = i0; h->chunk_cells = cells; h->chunk_levels = L;
    const uint8_t* d = h->stage.send(half, total, s);
    if (n_counters) UZL_HIP(hipMemsetAsync(h->d_counters.p, 0, n_counters * sizeof(uint32_t), s));
    OrbArgs a{};
    a.pixels = d + recs_bytes;
    a.images = reinterpret_cast<const OrbImage*>(d);
    a.units = reinterpret_cast<const OrbUnit*>(d + images_bytes);
    a.pyr = h->d_pyr.p; a.blur = h->d_blur.p; a.cand_xy = h->d_cand_xy.p; a.cand_score = h->d_cand_score.p;
    a.hist = h->d_counters.p; a.n_cand = a.hist + jobs * kOrbBins; a.thr = a.n_cand + jobs;
    a.count = h->d_count.p; a.kp_tmp = h->d_kp_tmp.p; a.kp = h->d_kp.p; a.desc = h->d_desc.p; a.gist = h->d_gist.p;
    a.pattern = h->d_pattern.p;
    memcpy(a.level_scale, plan.level_scale, sizeof(a.level_scale));
    memcpy(a.n_per_level, plan.n_per_level, sizeof(a.n_per_level));
    a.n_per_cell = plan.n_per_cell;
    a.n_levels = L; a.edge = c.edge_threshold; a.fast_threshold = c.fast_threshold;
    a.n_cell_units = n_cell_units; a.n_images = ni; a.do_gist = angles ? 1 : 0;
    for (int l = 1; l < L; l++) launch_orb_resize(a, l, n_units, max_w, max_h, s);
    if (angles) launch_orb_gist_resize(a, s);
    launch_orb_fast(a, max_cw, max_ch, s);
    launch_orb_cut(a, s);
    launch_orb_orient(a, (int)std::min<int64_t>(max_cand, INT32_MAX), s);
    launch_orb_order(a, (int)std::min<int64_t>(max_kp, INT32_MAX), s);
    launch_orb_blur(a, max_w, max_h, s);
    launch_orb_describe(a, s);
    UZL_HIP(hipGetLastError());
}

// the counts of the resident set, fetched once per extract
void fetch_counts(uzl_orb* h)
{
    if (h->have_counts) return;
    const size_t n = h->resident.size();
    h->counts.assign(n, 0);
    if (n) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        UZL_HIP(hipMemcpyAsync(h->counts.data(), h->d_count.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));
        for (size_t i = 0; i < n; i++) h->counts[i] = std::min<uint32_t>(h->counts[i], (uint32_t)h->resident[i].kp_cap);
    }
    h->have_counts = true;
}

// The stage entry's way to a unit of the last chunk: the checks every stage read shares.  cell = -1 is the whole image.
int stage_unit(uzl_orb* h, int32_t image, int32_t cell, int32_t level, const OrbImage** im, const OrbUnit** un)
{
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    if (cell < -1 || cell >= h->chunk_cells) return fail(h, UZL_ERR_BAD_ARG, "no such cell");
    if (level < 0 || level >= h->chunk_levels) return fail(h, UZL_ERR_BAD_ARG, "no such level");
    const int64_t k = (int64_t)image - h->chunk_first;
    if (k < 0 || k >= (int64_t)h->chunk_images.size())
        return fail(h, UZL_ERR_STATE, "the image is outside the last staging chunk: the work buffers hold that chunk only");
    *im = &h->chunk_images[(size_t)k];
    *un = &h->chunk_units[cell < 0 ? (size_t)(*im)->whole : (size_t)k * (size_t)h->chunk_cells + (size_t)cell];
    return UZL_OK;
}

// n bytes of a work buffer through the pinned read buffer
void stage_fetch(uzl_orb* h, const void* src, size_t n, void* out)
{
    if (!n) return;
    UZL_HIP(hipSetDevice(h->cfg.device));
    h->h_read.reserve(n);
    UZL_HIP(hipMemcpyAsync(h->h_read.p, src, n, hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    memcpy(out, h->h_read.p, n);
}

}  // namespace

extern "C" {

void uzl_orb_cfg_default(uzl_orb_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->number_of_features = 300; c->grid_rows = 2; c->grid_cols = 2; c->n_levels = 2; c->scale_factor = 1.2f;
    c->edge_threshold = 31; c->patch_size = 31; c->fast_threshold = 5; c->gist_size = kOrbGist; c->device = 0;
}

int uzl_orb_create(const uzl_orb_cfg* cfg, const int8_t* pattern, uzl_orb** out)
{
    if (out) *out = nullptr;
    if (!pattern) return UZL_ERR_BAD_ARG;
    for (int i = 0; i < 2 * kOrbPoints; i++) if (pattern[i] < -15 || pattern[i] > 15) return UZL_ERR_BAD_ARG;
    return create_handle(cfg, uzl_orb_cfg_default, out, check_cfg, [pattern](uzl_orb* h) {
        h->stage.create();
        h->d_pattern.reserve(2 * kOrbPoints);
        UZL_HIP(hipMemcpyAsync(h->d_pattern.p, pattern, 2 * kOrbPoints, hipMemcpyHostToDevice, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));          // the pattern is the caller's and pageable
    });
}

void uzl_orb_destroy(uzl_orb* h) { destroy_handle(h); }

const char* uzl_orb_last_error(uzl_orb* h) { return last_error_of(h); }

int uzl_orb_set_config(uzl_orb* h, const uzl_orb_cfg* cfg) { return set_config_of(h, cfg, check_cfg); }

int uzl_orb_extract(uzl_orb* h, int32_t n_images, const uzl_guide_image* images, const uzl_guide_image* masks, const float* gist_angle_deg)
{
    UZL_GUARD_BEGIN(h)
    if (n_images < 0 || (n_images > 0 && !images)) return fail(h, UZL_ERR_BAD_ARG, "negative image count or null images");
    for (int32_t i = 0; i < n_images; i++) {
        if (!mono_ok(images[i]))
            return fail(h, UZL_ERR_BAD_ARG, "an image that is neither width, height > 0 with data nor 0 x 0, with a step smaller than a row, or height * step beyond 2^31");
        if (masks && (masks[i].width != images[i].width || masks[i].height != images[i].height)) return fail(h, UZL_ERR_BAD_ARG, "a mask's size differs from its image's");
        if (masks && !mono_ok(masks[i])) return fail(h, UZL_ERR_BAD_ARG, "a mask without data, with a step smaller than a row, or height * step beyond 2^31");
        if (gist_angle_deg && !(std::fabs(gist_angle_deg[i]) <= 1.0e6f)) return fail(h, UZL_ERR_BAD_ARG, "a gist angle that is NaN or beyond 1e6 degrees");
    }
    const OrbPlan plan = plan_of(h->cfg);
    std::vector<OrbResident> set((size_t)n_images);
    int64_t total = 0;
    for (int32_t i = 0; i < n_images; i++) {
        OrbResident& r = set[i];
        r.kp_off = total; r.width = images[i].width; r.height = images[i].height;
        r.kp_cap = (int32_t)kp_cap_of(h->cfg, plan, r.width, r.height);        // < 2^29: width * height < 2^31
        total += r.kp_cap;
    }
    UZL_HIP(hipSetDevice(h->cfg.device));
    h->have = false;                                       // a failure below leaves no half-made set behind
    h->have_counts = false;
    h->resident.swap(set);
    h->d_kp.reserve(std::max<size_t>((size_t)total, 1));
    h->d_desc.reserve(std::max<size_t>((size_t)total * kOrbDescBytes, 1));
    h->d_count.reserve(std::max<size_t>((size_t)n_images, 1));
    h->d_gist.reserve(std::max<size_t>((size_t)n_images * kOrbDescBytes, 1));
    if (n_images) UZL_HIP(hipMemsetAsync(h->d_count.p, 0, (size_t)n_images * sizeof(uint32_t), h->stream));
    const std::vector<int32_t> first = plan_chunks([&](int32_t i) {
        return align256(mono_bytes(images[i])) + (masks ? align256(mono_bytes(masks[i])) : 0);
    }, n_images, kStageChunkBytes, std::max(1, kStageChunkImages / (h->cfg.grid_rows * h->cfg.grid_cols + 1)));
    for (size_t k = 0; k + 1 < first.size(); k++) run_chunk(h, plan, images, masks, gist_angle_deg, first[k], first[k + 1], (int)(k & 1));
    UZL_HIP(hipStreamSynchronize(h->stream));              // the caller's images are free again, the set is complete
    h->have = true;
    h->have_gist = gist_angle_deg != nullptr;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_orb_image_count(uzl_orb* h)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    return (int)h->resident.size();
    UZL_GUARD_END(h)
}

int uzl_orb_count(uzl_orb* h, int32_t image)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    fetch_counts(h);
    return (int)h->counts[image];
    UZL_GUARD_END(h)
}

int uzl_orb_read(uzl_orb* h, int32_t image, int32_t cap, float* u, float* v, float* response, float* angle, int32_t* octave, uint8_t* desc)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    if (cap < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    fetch_counts(h);
    const int32_t n = (int32_t)h->counts[image];
    if (!u && !v && !response && !angle && !octave && !desc) return n;
    if (cap < n) return fail(h, UZL_ERR_TRUNCATED, "capacity below the number of keypoints");
    if (n == 0) return 0;
    const OrbResident& r = h->resident[image];
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    const size_t kp_bytes = align256((size_t)n * sizeof(OrbKp)), desc_bytes = (size_t)n * kOrbDescBytes;
    h->h_read.reserve(kp_bytes + desc_bytes);
    UZL_HIP(hipMemcpyAsync(h->h_read.p, h->d_kp.p + r.kp_off, (size_t)n * sizeof(OrbKp), hipMemcpyDeviceToHost, s));
    if (desc) UZL_HIP(hipMemcpyAsync(h->h_read.p + kp_bytes, h->d_desc.p + r.kp_off * kOrbDescBytes, desc_bytes, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    const OrbKp* kp = reinterpret_cast<const OrbKp*>(h->h_read.p);
    for (int32_t i = 0; i < n; i++) {
        if (u) u[i] = kp[i].u;
        if (v) v[i] = kp[i].v;
        if (response) response[i] = kp[i].response;
        if (angle) angle[i] = kp[i].angle;
        if (octave) octave[i] = kp[i].octave;
    }
    if (desc) memcpy(desc, h->h_read.p + kp_bytes, desc_bytes);
    return n;
    UZL_GUARD_END(h)
}

int uzl_orb_gist(uzl_orb* h, int32_t image, uint8_t* out32)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    if (!h->have_gist) return fail(h, UZL_ERR_STATE, "the last extract had no gist angles");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    if (!out32) return fail(h, UZL_ERR_BAD_ARG, "null output");
    UZL_HIP(hipSetDevice(h->cfg.device));
    h->h_read.reserve(kOrbDescBytes);
    UZL_HIP(hipMemcpyAsync(h->h_read.p, h->d_gist.p + (size_t)image * kOrbDescBytes, kOrbDescBytes, hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    memcpy(out32, h->h_read.p, kOrbDescBytes);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_orb_lift(uzl_orb* h, int32_t image, uzl_depthfilter* depthfilter, int32_t df_image, double max_depth, double* pos_xyz, uint8_t* valid3d)
{
    UZL_GUARD_BEGIN(h)
    if (!depthfilter) return fail(h, UZL_ERR_BAD_ARG, "null filter handle");
    if (!h->have) return fail(h, UZL_ERR_STATE, "no extract yet");
    if (image < 0 || (size_t)image >= h->resident.size()) return fail(h, UZL_ERR_BAD_ARG, "no such image");
    fetch_counts(h);
    const int32_t n = (int32_t)h->counts[image];
    UZL_HIP(hipSetDevice(h->cfg.device));
    h->d_uv.reserve(std::max<size_t>(2 * (size_t)n, 1));
    OrbRoundArgs a;
    a.kp = h->d_kp.p + h->resident[image].kp_off; a.u = h->d_uv.p; a.v = h->d_uv.p + n; a.n = n;
    launch_orb_round(a, h->stream);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(h->stream));
    // the rounded keypoints are complete and stay while this handle's lock is held; the filter handle's lock is taken inside, after
    // this handle's
    const int rc = depthfilter_lift_device(depthfilter, h->cfg.device, df_image, n, a.u, a.v, max_depth, pos_xyz, valid3d);
    if (rc != UZL_OK) return fail(h, rc, "the filter handle refused the keypoints (see its last_error)");
    return n;
    UZL_GUARD_END(h)
}

int uzl_orb_stage_image(uzl_orb* h, int32_t image, int32_t what, int32_t cell, int32_t level, int64_t cap, uint8_t* out, int32_t* width,
                        int32_t* height)
{
    UZL_GUARD_BEGIN(h)
    if (what < UZL_ORB_STAGE_LEVEL || what > UZL_ORB_STAGE_GIST_BLUR) return fail(h, UZL_ERR_BAD_ARG, "no such stage image");
    const bool gist = what == UZL_ORB_STAGE_GIST || what == UZL_ORB_STAGE_GIST_BLUR;
    if (gist) { cell = -1; level = 0; }
    const OrbImage* im = nullptr;
    const OrbUnit* un = nullptr;
    const int rc = stage_unit(h, image, cell, level, &im, &un);
    if (rc != UZL_OK) return rc;
    if (cap < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    if ((what == UZL_ORB_STAGE_LEVEL || what == UZL_ORB_STAGE_MASK) && level == 0)
        return fail(h, UZL_ERR_BAD_ARG, "level 0 of an image or a mask is the caller's own input");
    if (what == UZL_ORB_STAGE_MASK && cell < 0) return fail(h, UZL_ERR_BAD_ARG, "masks are cut per cell: the whole image has no mask levels");
    if (what == UZL_ORB_STAGE_BLUR && cell >= 0) return fail(h, UZL_ERR_BAD_ARG, "only the whole image's levels are blurred");
    if (gist && !h->have_gist) return fail(h, UZL_ERR_STATE, "the last extract had no gist angles");
    if (what == UZL_ORB_STAGE_MASK && im->width > 0 && !un->has_mask) return fail(h, UZL_ERR_STATE, "the last extract had no masks");
    const OrbLevel& lv = un->lev[level];
    const int32_t w = im->width == 0 ? 0 : gist ? kOrbGist : lv.w, ht = im->width == 0 ? 0 : gist ? kOrbGist : lv.h;
    if (width) *width = w;
    if (height) *height = ht;
    const int64_t n = (int64_t)w * ht;
    if (!out) return UZL_OK;
    if (cap < n) return fail(h, UZL_ERR_TRUNCATED, "capacity below the image's width * height");
    const uint8_t* src = what == UZL_ORB_STAGE_LEVEL ? h->d_pyr.p + lv.img_off : what == UZL_ORB_STAGE_MASK ? h->d_pyr.p + lv.mask_off
                         : what == UZL_ORB_STAGE_BLUR ? h->d_blur.p + lv.blur_off : what == UZL_ORB_STAGE_GIST ? h->d_pyr.p + im->gist_off
                         : h->d_blur.p + im->gist_blur_off;
    stage_fetch(h, src, (size_t)n, out);                   // every one of these is compact: its pitch is its width
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_orb_stage_candidates(uzl_orb* h, int32_t image, int32_t cell, int32_t level, int32_t cap, int32_t* x, int32_t* y, uint8_t* score,
                             int32_t* thr)
{
    UZL_GUARD_BEGIN(h)
    const OrbImage* im = nullptr;
    const OrbUnit* un = nullptr;
    const int rc = stage_unit(h, image, cell, level, &im, &un);
    if (rc != UZL_OK) return rc;
    if (cell < 0) return fail(h, UZL_ERR_BAD_ARG, "candidates belong to a cell");
    if (cap < 0) return fail(h, UZL_ERR_BAD_ARG, "negative capacity");
    const OrbLevel& lv = un->lev[level];
    // the chunk's counters: hist, n_cand, thr, one entry per (cell unit, level)
    const size_t jobs = (size_t)h->chunk_images.size() * (size_t)h->chunk_cells * (size_t)h->chunk_levels;
    const size_t job = ((size_t)(image - h->chunk_first) * (size_t)h->chunk_cells + (size_t)cell) * (size_t)h->chunk_levels + (size_t)level;
    uint32_t nc = 0, t = 0;
    stage_fetch(h, h->d_counters.p + jobs * kOrbBins + job, sizeof(uint32_t), &nc);
    stage_fetch(h, h->d_counters.p + jobs * kOrbBins + jobs + job, sizeof(uint32_t), &t);
    const int32_t n = (int32_t)std::min<uint32_t>(nc, (uint32_t)lv.cand_cap);
    if ((x || y || score) && cap < n) return fail(h, UZL_ERR_TRUNCATED, "capacity below the number of candidates");
    if (thr) *thr = (int32_t)t;
    if (n == 0 || (!x && !y && !score)) return n;
    if (x || y) {
        std::vector<uint2> xy((size_t)n);
        stage_fetch(h, h->d_cand_xy.p + lv.cand_off, (size_t)n * sizeof(uint2), xy.data());
        for (int32_t i = 0; i < n; i++) {
            if (x) x[i] = (int32_t)xy[i].x;
            if (y) y[i] = (int32_t)xy[i].y;
        }
    }
    if (score) stage_fetch(h, h->d_cand_score.p + lv.cand_off, (size_t)n, score);
    return n;
    UZL_GUARD_END(h)
}

}  // extern "C"
