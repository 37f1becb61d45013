// uzl_gfr.hip — global-feature-repository place recognition (host + C ABI uzl_gfr_*).
//
// Mirrors GlobalFeatureRepositoryRecognizer (place_recognition/src/global_feature_repository_recognizer.cpp) over
// GlobalFeatureRepository (global_feature_repository.cpp) behind the filters of PlaceRecognizer (place_recognizer.cpp:71-180), with
// the exact nearest-feature search in place of FLANN's LSH index (include/uzl_mi355x.h states the contract).
// HBM layout: one feature store, row f = feature f, rows zero-padded to a 16-byte multiple; head[f] = first entry of the feature's
// link chain in an append-only arena of (next, place) entries, like the entry lists of uzl_places.hip.  Store, heads and arena
// double when full (a new allocation and a device-to-device copy on the handle's stream).  A call is one upload of the node's rows,
// up to four launches (gfr_kernels.hip: nearest, vote, select, integrate), one download of (candidate count, new feature count, new
// link count, the first kGfrInline candidates) and one wait; a node with more candidates than that costs a second download.  The
// host orders the candidates by (votes descending, place ascending) and applies PlaceRecognizer's filters (place_filters.hpp).
#include "gfr_types.hpp"
#include "place_filters.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <unordered_set>

namespace uzl {

constexpr int32_t kGfrInline = 1022;            // candidates that travel with the result's head (8 KB in all)
constexpr int32_t kGfrMaxInitial = 1 << 30;

}  // namespace uzl

using namespace uzl;

struct uzl_gfr : HandleBase {
    uzl_gfr_cfg cfg;
    HandleStream stream;
    int32_t type = -1;                              // GlobalFeatureRepository::descriptor_
    int32_t bytes = 0, chunks = 0;                  // of the stored features (free again while F == 0)
    int32_t F = 0, L = 0;                           // features, link entries
    size_t cap_f = 0, cap_l = 0;
    DevBuf<uint4> d_store, d_rows;
    DevBuf<int32_t> d_head, d_votes;
    DevBuf<GfrLink> d_link;
    DevBuf<unsigned long long> d_key;
    DevBuf<int2> d_res;                             // GfrResult (two int2), then the candidates
    PinBuf<uint4> h_rows;
    PinBuf<int2> h_res;
    std::vector<int64_t> stamp; std::vector<uint8_t> alive;
    std::unordered_set<uint64_t> checked;
    int32_t live = 0;
    int32_t last_rows = 0, last_n_votes = 0;        // what uzl_gfr_last_matches / last_votes read from d_key / d_votes
    bool mirrored = false;                          // uzl_gfr_get_feature's host copy of store, heads and arena is current
    std::vector<uint4> m_store; std::vector<int32_t> m_head; std::vector<GfrLink> m_link;
};

namespace {

bool has_rows(const uint8_t* desc, int32_t rows) { return desc && rows > 0; }

// the arguments of a call that matches rows x bytes descriptors of type feature_type; `integrates`: it may add rows features and links
int check_rows(uzl_gfr* h, const uint8_t* desc, int32_t rows, int32_t bytes, int32_t feature_type, bool integrates)
{
    if (rows < 0 || rows > kGfrMaxRows) return fail(h, UZL_ERR_BAD_ARG, "rows must be 0-4096");
    if (!has_rows(desc, rows)) return UZL_OK;
    if (bytes < 1 || bytes > kGfrMaxBytes) return fail(h, UZL_ERR_BAD_ARG, "descriptor length must be 1-64 bytes");
    const bool clears = feature_type != h->type;
    if (!clears && h->F > 0 && bytes != h->bytes)
        return fail(h, UZL_ERR_BAD_ARG, "descriptor length differs from the repository's stored features");
    if (integrates && !clears && ((int64_t)h->F + rows > INT32_MAX || (int64_t)h->L + rows > INT32_MAX))
        return fail(h, UZL_ERR_BAD_ARG, "feature and link indices must stay below 2^31");
    return UZL_OK;
}

int check_outputs(uzl_gfr* h, int32_t cap, const int32_t* neighbors, const int32_t* n_neighbors)
{
    if (!n_neighbors || cap < 0 || (cap > 0 && !neighbors)) return fail(h, UZL_ERR_BAD_ARG, "bad outputs");
    return UZL_OK;
}

// GlobalFeatureRepository::match on the device: type change, nearest feature per row, and as asked the votes with the candidates
// (into cand, ordered) and the integration of the node as place `place`.
void match(uzl_gfr* h, const uint8_t* desc, int32_t rows, int32_t bytes, int32_t feature_type, bool votes, bool integrate,
           int32_t place, std::vector<int2>& cand)
{
    hipStream_t s = h->stream;
    if (feature_type != h->type) {                                             // global_feature_repository.cpp:49-52
        h->type = feature_type; h->F = 0; h->L = 0; h->mirrored = false;
    }
    if (h->F == 0) { h->bytes = bytes; h->chunks = (bytes + 15) / 16; }
    const int32_t ch = h->chunks;
    if (integrate) {
        h->mirrored = false;
        while (h->cap_f < (size_t)h->F + rows) h->cap_f *= 2;
        while (h->cap_l < (size_t)h->L + rows) h->cap_l *= 2;
        h->d_store.reserve(h->cap_f * ch, true, s);
        h->d_head.reserve(h->cap_f, true, s);
        h->d_link.reserve(h->cap_l, true, s);
    }
    h->h_rows.reserve((size_t)rows * ch);
    h->d_rows.reserve((size_t)rows * ch);
    h->d_key.reserve(rows);
    uint8_t* hr = reinterpret_cast<uint8_t*>(h->h_rows.p);
    const size_t st = (size_t)ch * 16;
    memset(hr, 0, (size_t)rows * st);
    for (int32_t i = 0; i < rows; i++) memcpy(hr + (size_t)i * st, desc + (size_t)i * bytes, (size_t)bytes);
    UZL_HIP(hipMemcpyAsync(h->d_rows.p, hr, (size_t)rows * st, hipMemcpyHostToDevice, s));
    UZL_HIP(hipMemsetAsync(h->d_key.p, 0xff, (size_t)rows * sizeof(unsigned long long), s));
    const int32_t n_votes = (int32_t)h->stamp.size() + 1;                      // all_matches(place_count_ + 1, 0)
    h->d_res.reserve(2 + (size_t)(votes ? n_votes : 0));
    h->h_res.reserve(2 + (size_t)(votes ? n_votes : 0));

    GfrArgs a;
    a.rows_d = h->d_rows.p; a.rows = rows; a.chunks = ch; a.bytes = h->bytes;
    a.F = h->F; a.L = h->L; a.max_distance = h->cfg.max_distance; a.place = place;
    a.n_votes = n_votes;
    const double T = h->cfg.T;                                                 // votes > 0 and votes >= T, votes an int
    a.min_votes = T >= 2147483647. ? INT32_MAX : std::max(1, (int32_t)std::ceil(T));
    a.store = h->d_store.p; a.head = h->d_head.p; a.link = h->d_link.p; a.key = h->d_key.p;
    a.votes = h->d_votes.p; a.result = reinterpret_cast<GfrResult*>(h->d_res.p);
    launch_gfr_nearest(a, s);
    if (votes) {
        h->d_votes.reserve(n_votes);
        a.votes = h->d_votes.p;
        UZL_HIP(hipMemsetAsync(h->d_votes.p, 0, (size_t)n_votes * 4, s));
        launch_gfr_vote(a, s);
        launch_gfr_select(a, s);
    }
    if (integrate) launch_gfr_integrate(a, s);
    UZL_HIP(hipGetLastError());
    const int32_t n_inline = votes ? std::min(n_votes, kGfrInline) : 0;
    UZL_HIP(hipMemcpyAsync(h->h_res.p, h->d_res.p, (2 + (size_t)n_inline) * sizeof(int2), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    const GfrResult r = *reinterpret_cast<const GfrResult*>(h->h_res.p);
    h->last_rows = rows;
    cand.clear();
    if (votes) {
        h->last_n_votes = n_votes;
        const int32_t n = std::min(std::max(r.n_cand, 0), n_votes);
        if (n > n_inline) {
            UZL_HIP(hipMemcpyAsync(h->h_res.p + 2 + n_inline, h->d_res.p + 2 + n_inline, (size_t)(n - n_inline) * sizeof(int2),
                                   hipMemcpyDeviceToHost, s));
            UZL_HIP(hipStreamSynchronize(s));
        }
        cand.assign(h->h_res.p + 2, h->h_res.p + 2 + n);
        // (votes descending, place ascending): the reference's std::sort is unstable, the order among equal votes is fixed here
        std::sort(cand.begin(), cand.end(), [](const int2& x, const int2& y) { return x.y != y.y ? x.y > y.y : x.x < y.x; });
    }
    if (integrate) { h->F = r.n_features; h->L = r.n_links; }
}

void commit_place(uzl_gfr* h, int64_t stamp_ns)
{
    h->stamp.push_back(stamp_ns); h->alive.push_back(1); h->live++;            // place_id_map_.insert, place_count_++
}

void finish(uzl_gfr* h, const std::vector<int2>& cand, int64_t stamp_q, int32_t id_q, int32_t cap, int32_t* neighbors, int32_t* n_neighbors)
{
    std::vector<int32_t> res;
    place_filters(h->stamp, h->alive, h->checked, h->cfg.min_time_gap, h->cfg.k_nearest_neighbors, (int32_t)cand.size(),
                  [&cand](int32_t j) { return cand[j].x; }, stamp_q, id_q, res);
    write_places(res, 0, cap, neighbors);
    *n_neighbors = (int32_t)res.size();
}

void mirror(uzl_gfr* h)
{
    if (h->mirrored) return;
    hipStream_t s = h->stream;
    h->m_store.resize((size_t)h->F * h->chunks); h->m_head.resize(h->F); h->m_link.resize(h->L);
    if (h->F > 0) {
        UZL_HIP(hipMemcpyAsync(h->m_store.data(), h->d_store.p, h->m_store.size() * sizeof(uint4), hipMemcpyDeviceToHost, s));
        UZL_HIP(hipMemcpyAsync(h->m_head.data(), h->d_head.p, h->m_head.size() * 4, hipMemcpyDeviceToHost, s));
    }
    if (h->L > 0) UZL_HIP(hipMemcpyAsync(h->m_link.data(), h->d_link.p, h->m_link.size() * sizeof(GfrLink), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    h->mirrored = true;
}

}  // namespace

extern "C" {

void uzl_gfr_cfg_default(uzl_gfr_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->T = 10.0; c->k_nearest_neighbors = 10; c->max_distance = 40; c->device = 0; c->min_time_gap = 5.0; c->initial_features = 65536;
}

int uzl_gfr_create(const uzl_gfr_cfg* cfg, uzl_gfr** out)
{
    return create_handle(cfg, uzl_gfr_cfg_default, out, [](const uzl_gfr_cfg& c) {
        return std::isnan(c.T) || std::isnan(c.min_time_gap) || c.k_nearest_neighbors < 0 || c.k_nearest_neighbors > kGfrMaxK ||
                       c.max_distance < 1 || c.max_distance > kGfrMaxDistance || c.initial_features < 1 || c.initial_features > kGfrMaxInitial
                   ? UZL_ERR_BAD_ARG : UZL_OK;
    }, [](uzl_gfr* h) {
        h->cap_f = h->cap_l = (size_t)h->cfg.initial_features;
        h->d_res.reserve(2); h->h_res.reserve(2);
    });
}

void uzl_gfr_destroy(uzl_gfr* h) { destroy_handle(h); }

const char* uzl_gfr_last_error(uzl_gfr* h) { return last_error_of(h); }

int uzl_gfr_search_and_add(uzl_gfr* h, const uint8_t* desc, int32_t rows, int32_t bytes, int32_t feature_type, int64_t stamp_ns,
                           int32_t cap, int32_t* neighbors, int32_t* n_neighbors, int32_t* place_index)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_rows(h, desc, rows, bytes, feature_type, true)) return rc;
    if (int rc = check_outputs(h, cap, neighbors, n_neighbors)) return rc;
    const int32_t id = (int32_t)h->stamp.size();
    std::vector<int2> cand;
    if (has_rows(desc, rows)) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        match(h, desc, rows, bytes, feature_type, true, true, id, cand);
    }
    commit_place(h, stamp_ns);                                                 // inserted before the filters run (place_recognizer.cpp:84-86)
    finish(h, cand, stamp_ns, id, cap, neighbors, n_neighbors);
    if (place_index) *place_index = id;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gfr_add(uzl_gfr* h, const uint8_t* desc, int32_t rows, int32_t bytes, int32_t feature_type, int64_t stamp_ns, int32_t* place_index)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_rows(h, desc, rows, bytes, feature_type, true)) return rc;
    const int32_t id = (int32_t)h->stamp.size();
    std::vector<int2> cand;
    if (has_rows(desc, rows)) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        // addPlaceImpl hands match() an empty vote vector, which global_feature_repository.cpp:60-62 then writes out of bounds: nothing is counted here
        match(h, desc, rows, bytes, feature_type, false, true, id, cand);
    }
    commit_place(h, stamp_ns);
    if (place_index) *place_index = id;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gfr_search(uzl_gfr* h, const uint8_t* desc, int32_t rows, int32_t bytes, int32_t feature_type, int64_t stamp_ns,
                   int32_t query_place, int32_t cap, int32_t* neighbors, int32_t* n_neighbors)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_rows(h, desc, rows, bytes, feature_type, false)) return rc;
    if (int rc = check_outputs(h, cap, neighbors, n_neighbors)) return rc;
    *n_neighbors = 0;
    if (h->live == 0 || !has_rows(desc, rows)) return UZL_OK;                  // place_recognizer.cpp:153-156 / no FeatureData
    UZL_HIP(hipSetDevice(h->cfg.device));
    std::vector<int2> cand;
    match(h, desc, rows, bytes, feature_type, true, false, -1, cand);
    finish(h, cand, stamp_ns, query_place, cap, neighbors, n_neighbors);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gfr_remove(uzl_gfr* h, int32_t place_index)
{
    UZL_GUARD_BEGIN(h)
    if (place_index < 0 || place_index >= (int32_t)h->stamp.size() || !h->alive[place_index])
        return fail(h, UZL_ERR_NOT_FOUND, "tried to remove a non-existing place");
    h->alive[place_index] = 0; h->live--;                                      // removePlaceImpl is a TODO (recognizer.cpp:155-158): the links stay
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gfr_count(uzl_gfr* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return (int)h->stamp.size();
}

int uzl_gfr_feature_count(uzl_gfr* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return h->F;
}

int uzl_gfr_link_count(uzl_gfr* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return h->L;
}

int uzl_gfr_last_matches(uzl_gfr* h, int32_t cap, int32_t* feature, int32_t* dist)
{
    UZL_GUARD_BEGIN(h)
    const int32_t n = h->last_rows, m = std::min(n, std::max(cap, 0));
    if (m > 0 && (feature || dist)) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        std::vector<unsigned long long> key((size_t)m);
        UZL_HIP(hipMemcpyAsync(key.data(), h->d_key.p, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));
        for (int32_t i = 0; i < m; i++) {
            const bool none = key[i] == kGfrNoKey;
            const int32_t d = none ? -1 : (int32_t)(key[i] >> 32);
            if (feature) feature[i] = (!none && d < h->cfg.max_distance) ? (int32_t)(uint32_t)key[i] : -1;
            if (dist) dist[i] = d;
        }
    }
    return n;
    UZL_GUARD_END(h)
}

int uzl_gfr_last_votes(uzl_gfr* h, int32_t cap, int32_t* votes)
{
    UZL_GUARD_BEGIN(h)
    const int32_t n = h->last_n_votes, m = std::min(n, std::max(cap, 0));
    if (m > 0 && votes) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        UZL_HIP(hipMemcpyAsync(votes, h->d_votes.p, (size_t)m * 4, hipMemcpyDeviceToHost, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));
    }
    return n;
    UZL_GUARD_END(h)
}

int uzl_gfr_get_feature(uzl_gfr* h, int32_t feature, uint8_t* desc_out, int32_t cap, int32_t* places, int32_t* n_places)
{
    UZL_GUARD_BEGIN(h)
    if (feature < 0 || feature >= h->F) return fail(h, UZL_ERR_NOT_FOUND, "no such feature");
    if (cap < 0 || (cap > 0 && !places)) return fail(h, UZL_ERR_BAD_ARG, "bad outputs");
    UZL_HIP(hipSetDevice(h->cfg.device));
    mirror(h);
    if (desc_out) memcpy(desc_out, h->m_store.data() + (size_t)feature * h->chunks, (size_t)h->bytes);
    std::vector<int32_t> pl;
    for (int32_t e = h->m_head[feature]; e >= 0 && e < h->L && (int32_t)pl.size() < h->L; e = h->m_link[e].next) pl.push_back(h->m_link[e].place);
    std::sort(pl.begin(), pl.end());                                           // place indices only grow: this is the reference's insertion order
    for (size_t j = 0; j < pl.size() && (int32_t)j < cap; j++) places[j] = pl[j];
    if (n_places) *n_places = (int32_t)pl.size();
    return UZL_OK;
    UZL_GUARD_END(h)
}

}  // extern "C"
