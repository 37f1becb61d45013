// uzl_gist.hip — binary-GIST place recognition (host + C ABI uzl_gist_*).
//
// Mirrors BinaryGistRecognizer (place_recognition/src/binary_gist_recognizer.cpp) behind the filters of PlaceRecognizer
// (place_recognizer.cpp:71-180), with the exact k-NN in place of FLANN's LSH index (include/uzl_mi355x.h states the contract).
// HBM layout: one descriptor store, row p = place p, rows zero-padded to a 16-byte multiple (the kernel's dwordx4 loads), grown
// geometrically by appending (a row never moves relative to the others); a live byte per place (indexed and not removed).
// A single call is a batch of one: its row is appended first and the query reads it from the store, seeing the places before it.
// The kernel (gist_kernels.hip) returns per query the <= k nearest live places within T in (distance, place) order; the time gap,
// k and reported-once filters run here, in the reference's order, node after node.
#include "gist_types.hpp"
#include "place_filters.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cmath>
#include <new>
#include <unordered_set>

namespace uzl {

constexpr int kGistSlice = 4096;      // queries per launch of a batch (bounds the (place, distance) output buffer)

}  // namespace uzl

using namespace uzl;

struct uzl_gist : HandleBase {
    uzl_gist_cfg cfg;
    HandleStream stream;
    int32_t bytes = 0, stride = 0;                 // fixed by the first indexed descriptor
    DevBuf<uint8_t> d_store, d_live, d_query;
    DevBuf<int2> d_out; DevBuf<int32_t> d_out_n;
    PinBuf<uint8_t> h_rows, h_live;
    PinBuf<int2> h_out; PinBuf<int32_t> h_out_n;
    std::vector<int64_t> stamp; std::vector<uint8_t> alive, indexed;
    std::unordered_set<uint64_t> checked;
    std::vector<int2> last_knn;
};

namespace {

// descriptor length of a call that indexes or searches with `bytes`
int check_bytes(uzl_gist* h, int32_t bytes)
{
    if (bytes < 1 || bytes > kGistMaxBytes) return fail(h, UZL_ERR_BAD_ARG, "descriptor length must be 1-256 bytes");
    if (h->bytes && bytes != h->bytes) return fail(h, UZL_ERR_BAD_ARG, "descriptor length differs from the handle's first indexed descriptor");
    return UZL_OK;
}

bool has(const uint8_t* desc, const uint8_t* has_gist, int32_t i) { return desc && (!has_gist || has_gist[i]); }

// Append n places (indexed where has(desc, has_gist, i)) at place indices base .. base + n - 1 on the device; host state follows in
// commit_place once the searches of the batch have run.
void append_places(uzl_gist* h, int32_t n, const uint8_t* desc, const uint8_t* has_gist, int32_t bytes)
{
    hipStream_t s = h->stream;
    const int32_t base = (int32_t)h->stamp.size();
    bool any = false;
    for (int32_t i = 0; i < n && !any; i++) any = has(desc, has_gist, i);
    if (any && !h->bytes) { h->bytes = bytes; h->stride = (bytes + 15) / 16 * 16; }
    const size_t rows = (size_t)base + n;
    h->d_live.reserve(std::max<size_t>(rows, 1), true, s);
    h->h_live.reserve(std::max(n, 1));
    for (int32_t i = 0; i < n; i++) h->h_live.p[i] = has(desc, has_gist, i) ? 1 : 0;
    if (n > 0) UZL_HIP(hipMemcpyAsync(h->d_live.p + base, h->h_live.p, (size_t)n, hipMemcpyHostToDevice, s));
    if (h->bytes) h->d_store.reserve(rows * (size_t)h->stride, true, s);     // row p exists for every place p once the length is known
    if (any) {
        const size_t st = (size_t)h->stride;
        h->h_rows.reserve((size_t)n * st);
        memset(h->h_rows.p, 0, (size_t)n * st);
        for (int32_t i = 0; i < n; i++)
            if (has(desc, has_gist, i)) memcpy(h->h_rows.p + (size_t)i * st, desc + (size_t)i * bytes, (size_t)bytes);
        UZL_HIP(hipMemcpyAsync(h->d_store.p + (size_t)base * st, h->h_rows.p, (size_t)n * st, hipMemcpyHostToDevice, s));
    }
}

void commit_place(uzl_gist* h, bool idx, int64_t stamp_ns)
{
    h->stamp.push_back(stamp_ns); h->alive.push_back(1); h->indexed.push_back(idx ? 1 : 0);   // place_id_map_.insert, place_count_++
}

int32_t dmax_of(const uzl_gist* h)
{
    const double T = h->cfg.T;
    if (!(T >= 0.)) return -1;                                                 // dist <= T with T < 0: nothing
    const int32_t bits = 8 * h->bytes;
    return T >= (double)bits ? bits : (int32_t)std::floor(T);                  // int <= double, inclusive (T = 10.5 acts as 10)
}

// k-NN of n queries (rows `queries`, stride h->stride) against the places [0, base + q); results in h->h_out / h->h_out_n
void run_knn(uzl_gist* h, const uint8_t* queries, const uint8_t* qvalid, int32_t base, int32_t n)
{
    hipStream_t s = h->stream;
    const int k = h->cfg.k_nearest_neighbors;
    h->h_out_n.reserve(std::max(n, 1));
    h->h_out.reserve((size_t)std::max(n, 1) * std::max(k, 1));
    const int32_t dmax = dmax_of(h);
    if (k <= 0 || dmax < 0 || !h->bytes || n <= 0) {                           // FLANN size 0 / nn = 0 / nothing within T
        memset(h->h_out_n.p, 0, (size_t)std::max(n, 1) * 4);
        UZL_HIP(hipStreamSynchronize(s));                                       // the staging buffers of append_places are free again
        return;
    }
    const int slice = std::min(n, kGistSlice);
    h->d_out.reserve((size_t)slice * k); h->d_out_n.reserve(slice);
    for (int32_t q0 = 0; q0 < n; q0 += slice) {
        const int32_t m = std::min(slice, n - q0);
        GistKnnArgs a;
        a.store = h->d_store.p; a.live = h->d_live.p;
        a.queries = queries + (size_t)q0 * h->stride; a.qvalid = qvalid ? qvalid + q0 : nullptr;
        a.stride = h->stride; a.base = base + q0; a.k = k; a.dmax = dmax;
        a.out = h->d_out.p; a.out_n = h->d_out_n.p;
        launch_gist_knn(a, m, s);
        UZL_HIP(hipGetLastError());
        UZL_HIP(hipMemcpyAsync(h->h_out.p + (size_t)q0 * k, h->d_out.p, (size_t)m * k * sizeof(int2), hipMemcpyDeviceToHost, s));
        UZL_HIP(hipMemcpyAsync(h->h_out_n.p + q0, h->d_out_n.p, (size_t)m * 4, hipMemcpyDeviceToHost, s));
    }
    UZL_HIP(hipStreamSynchronize(s));
}

// PlaceRecognizer's filters (place_filters.hpp) over knn = the impl's result (k nearest within T, nearest first)
void finish(uzl_gist* h, const int2* knn, int32_t n, int64_t stamp_q, int32_t id_q, std::vector<int32_t>& res)
{
    place_filters(h->stamp, h->alive, h->checked, h->cfg.min_time_gap, h->cfg.k_nearest_neighbors, n,
                  [knn](int32_t j) { return knn[j].x; }, stamp_q, id_q, res);
}

int check_batch(uzl_gist* h, int32_t n, const uint8_t* desc, const uint8_t* has_gist, int32_t bytes, const int64_t* stamps_ns)
{
    if (n < 0 || (n > 0 && !stamps_ns)) return fail(h, UZL_ERR_BAD_ARG, "bad node count or null stamps");
    bool any = false;
    for (int32_t i = 0; i < n && !any; i++) any = has(desc, has_gist, i);
    if (any) return check_bytes(h, bytes);
    return UZL_OK;
}

// n successive searchAndAddPlace calls; nb_cap / neighbors / count_per_node / n_total as uzl_gist_search_and_add_batch
void search_and_add_n(uzl_gist* h, int32_t n, const uint8_t* desc, const uint8_t* has_gist, int32_t bytes, const int64_t* stamps_ns,
                      int64_t cap, int32_t* neighbors, int32_t* count_per_node, int64_t* n_total)
{
    const int32_t base = (int32_t)h->stamp.size();
    append_places(h, n, desc, has_gist, bytes);
    if (h->bytes) run_knn(h, h->d_store.p + (size_t)base * h->stride, h->d_live.p + base, base, n);
    else run_knn(h, nullptr, nullptr, base, 0);
    const int k = std::max(h->cfg.k_nearest_neighbors, 1);
    int64_t total = 0;
    std::vector<int32_t> res;
    for (int32_t i = 0; i < n; i++) {
        const int32_t nk = h->bytes ? h->h_out_n.p[i] : 0;
        const int2* knn = h->h_out.p + (size_t)i * k;
        commit_place(h, has(desc, has_gist, i), stamps_ns[i]);                // inserted before the filters run (:84-85)
        res.clear();
        finish(h, knn, nk, stamps_ns[i], base + i, res);
        write_places(res, total, cap, neighbors);
        if (count_per_node) count_per_node[i] = (int32_t)res.size();
        total += (int64_t)res.size();
        if (i == n - 1) h->last_knn.assign(knn, knn + nk);
    }
    *n_total = total;
}

}  // namespace

extern "C" {

void uzl_gist_cfg_default(uzl_gist_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->T = 10.0; c->k_nearest_neighbors = 10; c->device = 0; c->min_time_gap = 5.0;
}

int uzl_gist_create(const uzl_gist_cfg* cfg, uzl_gist** out)
{
    return create_handle(cfg, uzl_gist_cfg_default, out, [](const uzl_gist_cfg& c) {
        return std::isnan(c.T) || c.k_nearest_neighbors < 0 || c.k_nearest_neighbors > kGistMaxK ? UZL_ERR_BAD_ARG : UZL_OK;
    }, [](uzl_gist* h) { h->d_query.reserve(kGistMaxBytes); });
}

void uzl_gist_destroy(uzl_gist* h) { destroy_handle(h); }

const char* uzl_gist_last_error(uzl_gist* h) { return last_error_of(h); }

int uzl_gist_search_and_add(uzl_gist* h, const uint8_t* desc, int32_t bytes, int64_t stamp_ns, int32_t cap, int32_t* neighbors,
                            int32_t* n_neighbors, int32_t* place_index)
{
    UZL_GUARD_BEGIN(h)
    if (desc) if (int rc = check_bytes(h, bytes)) return rc;
    if (!n_neighbors || cap < 0 || (cap > 0 && !neighbors)) return fail(h, UZL_ERR_BAD_ARG, "bad outputs");
    UZL_HIP(hipSetDevice(h->cfg.device));
    const int32_t id = (int32_t)h->stamp.size();
    int64_t total = 0;
    search_and_add_n(h, 1, desc, nullptr, bytes, &stamp_ns, cap, neighbors, nullptr, &total);
    *n_neighbors = (int32_t)total;
    if (place_index) *place_index = id;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gist_add(uzl_gist* h, const uint8_t* desc, int32_t bytes, int64_t stamp_ns, int32_t* place_index)
{
    return uzl_gist_add_batch(h, 1, desc, nullptr, bytes, &stamp_ns, place_index);
}

int uzl_gist_search(uzl_gist* h, const uint8_t* desc, int32_t bytes, int64_t stamp_ns, int32_t query_place, int32_t cap,
                    int32_t* neighbors, int32_t* n_neighbors)
{
    UZL_GUARD_BEGIN(h)
    if (desc) if (int rc = check_bytes(h, bytes)) return rc;
    if (!n_neighbors || cap < 0 || (cap > 0 && !neighbors)) return fail(h, UZL_ERR_BAD_ARG, "bad outputs");
    *n_neighbors = 0;
    h->last_knn.clear();
    const int32_t n = (int32_t)h->stamp.size();
    if (!desc || !h->bytes || n == 0) return UZL_OK;                          // no GIST sensor / empty index (:152-155)
    UZL_HIP(hipSetDevice(h->cfg.device));
    std::vector<uint8_t> row((size_t)h->stride, 0);
    memcpy(row.data(), desc, (size_t)bytes);
    UZL_HIP(hipMemcpyAsync(h->d_query.p, row.data(), row.size(), hipMemcpyHostToDevice, h->stream));
    run_knn(h, h->d_query.p, nullptr, n, 1);
    const int2* knn = h->h_out.p;
    const int32_t nk = h->h_out_n.p[0];
    h->last_knn.assign(knn, knn + nk);
    std::vector<int32_t> res;
    finish(h, knn, nk, stamp_ns, query_place, res);
    write_places(res, 0, cap, neighbors);
    *n_neighbors = (int32_t)res.size();
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gist_remove(uzl_gist* h, int32_t place_index)
{
    UZL_GUARD_BEGIN(h)
    if (place_index < 0 || place_index >= (int32_t)h->stamp.size() || !h->alive[place_index])
        return fail(h, UZL_ERR_NOT_FOUND, "tried to remove a non-existing place");
    if (h->indexed[place_index]) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        UZL_HIP(hipMemsetAsync(h->d_live.p + place_index, 0, 1, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));
    }
    h->alive[place_index] = 0;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gist_count(uzl_gist* h)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    return (int)h->stamp.size();
}

int uzl_gist_search_and_add_batch(uzl_gist* h, int32_t n, const uint8_t* desc, const uint8_t* has_gist, int32_t bytes,
                                  const int64_t* stamps_ns, int64_t cap, int32_t* neighbors, int32_t* count_per_node, int64_t* n_total,
                                  int32_t* first_place_index)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_batch(h, n, desc, has_gist, bytes, stamps_ns)) return rc;
    if (!n_total || cap < 0 || (cap > 0 && !neighbors)) return fail(h, UZL_ERR_BAD_ARG, "bad outputs");
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (first_place_index) *first_place_index = (int32_t)h->stamp.size();
    search_and_add_n(h, n, desc, has_gist, bytes, stamps_ns, cap, neighbors, count_per_node, n_total);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gist_add_batch(uzl_gist* h, int32_t n, const uint8_t* desc, const uint8_t* has_gist, int32_t bytes, const int64_t* stamps_ns,
                       int32_t* first_place_index)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_batch(h, n, desc, has_gist, bytes, stamps_ns)) return rc;
    UZL_HIP(hipSetDevice(h->cfg.device));
    if (first_place_index) *first_place_index = (int32_t)h->stamp.size();
    append_places(h, n, desc, has_gist, bytes);                               // addPlaceImpl: index only (binary_gist_recognizer.cpp:82-104)
    UZL_HIP(hipStreamSynchronize(h->stream));
    for (int32_t i = 0; i < n; i++) commit_place(h, has(desc, has_gist, i), stamps_ns[i]);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_gist_last_knn(uzl_gist* h, int32_t cap, int32_t* place, int32_t* dist)
{
    if (!h) return UZL_ERR_BAD_ARG;
    std::lock_guard<std::mutex> lock(h->mu);
    const int32_t n = (int32_t)h->last_knn.size();
    for (int32_t i = 0; i < n && i < cap; i++) {
        if (place) place[i] = h->last_knn[i].x;
        if (dist) dist[i] = h->last_knn[i].y;
    }
    return n;
}

}  // extern "C"
