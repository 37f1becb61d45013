// uzl_scope.hip — node uncertainty and local scope (host + C ABI uzl_scope_*).
//
// Mirrors SlamGraph::reevaluateUncertainty() / reevaluateUncertainty(id) (graph_slam_common/src/slam_graph.cpp:506-556) over
// dijkstra (:765-797), getNeighbors (:558-578) and oldestReachableNode (:892-910), getOutOfScopeNodes (:216-229) behind
// scopeRequestTimerCallback (graph_slam/src/graph_slam_node.cpp:578-663) and the node test of scopeRequestCallback (:535-559);
// include/uzl_mi355x.h states the contract.
// Host side: the edge list (from, to, type, valid), and from it - integer work, redone only when edges or flags change - the CSR of
// the edges dijkstra walks (valid, not TYPE_2D_LASER) and a union-find over ALL non-laser edges whose component minimum is
// oldestReachableNode's answer, as setFixedNodes' components are host work in the solver.
// HBM: positions SoA, uncertainty_, distance_ (bit patterns), the CSR, the pass's edge lengths and node records.  A pass is one
// upload of nothing (or of a rebuilt CSR), one launch (scope_kernels.hip), one 32-byte download and one wait; the positions arrive
// from the host (set_poses) or straight from a uzl_pgo handle's pose buffer (poses_from_pgo: one small kernel, no host copy).
#include "graph_csr.hpp"
#include "scope_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cfloat>
#include <new>
#include <numeric>

using namespace uzl;

struct uzl_scope : HandleBase {
    uzl_scope_cfg cfg;
    HandleStream stream;
    int32_t n = 0;
    using Edge = GraphEdge;
    std::vector<Edge> edges;
    bool plan_stale = true;                         // edges or flags changed since the CSR and the components were built
    std::vector<int32_t> comp_min;                  // per node: smallest index of its component over all non-laser edges
    int32_t m = 0;                                  // CSR slots
    DevBuf<double> d_x, d_y, d_z, d_unc, d_w;
    DevBuf<unsigned long long> d_dist;
    DevBuf<int32_t> d_row_ptr, d_row, d_col, d_count, d_out, d_total;
    DevBuf<uint32_t> d_front, d_have;
    DevBuf<ScopeRec> d_rec;
    DevBuf<ScopeResult> d_res;
    DevBuf<double> d_radius;
    bool have_pass = false;                         // d_dist holds the distance_ of a pass over the current n nodes
    long long rounds = 0, relaxations = 0;
    int32_t in_lds = 0;
};

namespace {

bool joins(const uzl_scope::Edge& e) { return e.type != UZL_EDGE_TYPE_2D_LASER; }             // slam_graph.cpp:569
bool walked(const uzl_scope::Edge& e) { return e.valid != 0 && joins(e); }                     // ... with only_valid (:787)

int check_edges(uzl_scope* h, int32_t n_nodes, int32_t n_edges, const uzl_gate_edge* edges)
{
    if (n_edges < 0 || (n_edges > 0 && !edges)) return fail(h, UZL_ERR_BAD_ARG, "null edges");
    for (int32_t k = 0; k < n_edges; k++)
        if (edges[k].from < 0 || edges[k].from >= n_nodes || edges[k].to < 0 || edges[k].to >= n_nodes)
            return fail(h, UZL_ERR_BAD_ARG, "an edge names a node outside the graph");
    if ((int64_t)h->edges.size() + n_edges > INT32_MAX / 2) return fail(h, UZL_ERR_BAD_ARG, "too many edges");
    return UZL_OK;
}

// nodes [first, first + count): positions and uncertainty_ behind those already on the device
void upload_nodes(uzl_scope* h, int32_t first, int32_t count, const double* poses, const double* uncertainty)
{
    hipStream_t s = h->stream;
    const size_t total = (size_t)first + count;
    h->d_x.reserve(total, true, s); h->d_y.reserve(total, true, s); h->d_z.reserve(total, true, s); h->d_unc.reserve(total, true, s);
    if (count == 0) return;
    std::vector<double> x((size_t)count), y(x.size()), z(x.size()), u(x.size(), 0.);
    for (int32_t i = 0; i < count; i++) {
        const double* T = poses + 12 * (size_t)i;
        x[i] = T[3]; y[i] = T[7]; z[i] = T[11];
        if (uncertainty) u[i] = uncertainty[i];
    }
    UZL_HIP(hipMemcpyAsync(h->d_x.p + first, x.data(), (size_t)count * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipMemcpyAsync(h->d_y.p + first, y.data(), (size_t)count * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipMemcpyAsync(h->d_z.p + first, z.data(), (size_t)count * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipMemcpyAsync(h->d_unc.p + first, u.data(), (size_t)count * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipStreamSynchronize(s));
}

void append_edges(uzl_scope* h, int32_t n_edges, const uzl_gate_edge* edges)
{
    h->edges.reserve(h->edges.size() + (size_t)n_edges);
    for (int32_t k = 0; k < n_edges; k++) h->edges.push_back({edges[k].from, edges[k].to, edges[k].type, edges[k].valid});
    h->plan_stale = true;
}

int32_t find_root(std::vector<int32_t>& parent, int32_t v)
{
    while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }
    return v;
}

// the CSR of the walked edges (both directions, a self-loop once) and the component minima, uploaded
void ensure_plan(uzl_scope* h)
{
    if (!h->plan_stale) return;
    hipStream_t s = h->stream;
    const int32_t n = h->n;
    std::vector<int32_t> parent((size_t)n);
    std::iota(parent.begin(), parent.end(), 0);
    for (const auto& e : h->edges) {
        if (!joins(e)) continue;
        const int32_t a = find_root(parent, e.from), b = find_root(parent, e.to);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);            // the root of a component is its smallest index
    }
    h->comp_min.resize((size_t)n);
    for (int32_t v = 0; v < n; v++) h->comp_min[v] = find_root(parent, v);
    std::vector<int32_t> row_ptr, row, col;
    const int32_t m = build_csr(n, h->edges, walked, row_ptr, &row, col);
    h->m = m;
    h->d_row_ptr.reserve((size_t)n + 1); h->d_row.reserve(row.size()); h->d_col.reserve(row.size()); h->d_w.reserve(row.size());
    UZL_HIP(hipMemcpyAsync(h->d_row_ptr.p, row_ptr.data(), ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s));
    if (m > 0) {
        UZL_HIP(hipMemcpyAsync(h->d_row.p, row.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
        UZL_HIP(hipMemcpyAsync(h->d_col.p, col.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
    }
    UZL_HIP(hipStreamSynchronize(s));                                  // the vectors go out of scope
    h->plan_stale = false;
}

int check_list(uzl_scope* h, int32_t cap, const int32_t* out, const int32_t* n)
{
    if (!n || cap < 0 || (cap > 0 && !out)) return fail(h, UZL_ERR_BAD_ARG, "bad outputs");
    return UZL_OK;
}

// both passes of scope_scan_kernel, then the hits (at most cap) and their total
void scan(uzl_scope* h, ScopeScanArgs& a, double* radius, int32_t cap, int32_t* out, int32_t* n)
{
    hipStream_t s = h->stream;
    const int32_t blocks = (h->n + kScanSlab - 1) / kScanSlab, w = std::min(cap, h->n);
    h->d_count.reserve((size_t)blocks); h->d_out.reserve((size_t)std::max(w, 1)); h->d_total.reserve(1); h->d_radius.reserve(1);
    a.n = h->n; a.x = h->d_x.p; a.y = h->d_y.p; a.z = h->d_z.p; a.unc = h->d_unc.p;
    a.count = h->d_count.p; a.out = h->d_out.p; a.cap = w; a.radius_out = h->d_radius.p; a.total = h->d_total.p;
    launch_scope_scan(a, s);
    UZL_HIP(hipGetLastError());
    int32_t total = 0;
    UZL_HIP(hipMemcpyAsync(&total, h->d_total.p, 4, hipMemcpyDeviceToHost, s));
    if (radius) UZL_HIP(hipMemcpyAsync(radius, h->d_radius.p, 8, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    const int32_t got = std::min(total, w);
    if (got > 0) {
        UZL_HIP(hipMemcpyAsync(out, h->d_out.p, (size_t)got * 4, hipMemcpyDeviceToHost, s));
        UZL_HIP(hipStreamSynchronize(s));
    }
    *n = total;
}

int read_doubles(uzl_scope* h, const void* src, int32_t cap, double* out)
{
    if (cap < h->n || (h->n > 0 && !out)) return fail(h, UZL_ERR_BAD_ARG, "cap is smaller than the node count");
    if (h->n == 0) return 0;
    UZL_HIP(hipSetDevice(h->cfg.device));
    UZL_HIP(hipMemcpyAsync(out, src, (size_t)h->n * 8, hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    return h->n;
}

}  // namespace

extern "C" {

void uzl_scope_cfg_default(uzl_scope_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->scope_size_min = 8.0; c->scope_size_factor = 0.1; c->out_margin = 4.0; c->device = 0;
}

int uzl_scope_create(const uzl_scope_cfg* cfg, uzl_scope** out)
{
    return create_handle(cfg, uzl_scope_cfg_default, out, [](const uzl_scope_cfg& c) {
        return std::isnan(c.scope_size_min) || std::isnan(c.scope_size_factor) || std::isnan(c.out_margin) ? UZL_ERR_BAD_ARG : UZL_OK;
    }, [](uzl_scope* h) { h->d_res.reserve(1); });
}

void uzl_scope_destroy(uzl_scope* h) { destroy_handle(h); }

const char* uzl_scope_last_error(uzl_scope* h) { return last_error_of(h); }

int32_t uzl_scope_lds_nodes(void) { return kScopeLdsNodes; }

int uzl_scope_set_graph(uzl_scope* h, int32_t n_nodes, const double* poses, const double* uncertainty, int32_t n_edges,
                        const uzl_gate_edge* edges)
{
    UZL_GUARD_BEGIN(h)
    if (n_nodes < 0 || (n_nodes > 0 && !poses)) return fail(h, UZL_ERR_BAD_ARG, "null poses");
    std::vector<uzl_scope::Edge> kept;
    kept.swap(h->edges);                                               // check_edges counts against an empty graph
    if (int rc = check_edges(h, n_nodes, n_edges, edges)) { h->edges.swap(kept); return rc; }
    UZL_HIP(hipSetDevice(h->cfg.device));
    upload_nodes(h, 0, n_nodes, poses, uncertainty);
    h->n = n_nodes;
    append_edges(h, n_edges, edges);
    h->have_pass = false;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_add(uzl_scope* h, int32_t n_new_nodes, const double* poses, const double* uncertainty, int32_t n_new_edges,
                  const uzl_gate_edge* edges)
{
    UZL_GUARD_BEGIN(h)
    if (n_new_nodes < 0 || (n_new_nodes > 0 && !poses)) return fail(h, UZL_ERR_BAD_ARG, "null poses");
    if ((int64_t)h->n + n_new_nodes > INT32_MAX / 2) return fail(h, UZL_ERR_BAD_ARG, "too many nodes");
    if (int rc = check_edges(h, h->n + n_new_nodes, n_new_edges, edges)) return rc;
    UZL_HIP(hipSetDevice(h->cfg.device));
    upload_nodes(h, h->n, n_new_nodes, poses, uncertainty);
    h->n += n_new_nodes;
    append_edges(h, n_new_edges, edges);
    if (n_new_nodes > 0) { h->have_pass = false; h->plan_stale = true; }
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_set_poses(uzl_scope* h, int32_t n_nodes, const double* poses)
{
    UZL_GUARD_BEGIN(h)
    if (n_nodes != h->n) return fail(h, UZL_ERR_BAD_ARG, "the node count differs from the graph's");
    if (n_nodes > 0 && !poses) return fail(h, UZL_ERR_BAD_ARG, "null poses");
    if (n_nodes == 0) return UZL_OK;
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    std::vector<double> x((size_t)n_nodes), y(x.size()), z(x.size());
    for (int32_t i = 0; i < n_nodes; i++) { const double* T = poses + 12 * (size_t)i; x[i] = T[3]; y[i] = T[7]; z[i] = T[11]; }
    UZL_HIP(hipMemcpyAsync(h->d_x.p, x.data(), (size_t)n_nodes * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipMemcpyAsync(h->d_y.p, y.data(), (size_t)n_nodes * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipMemcpyAsync(h->d_z.p, z.data(), (size_t)n_nodes * 8, hipMemcpyHostToDevice, s));
    UZL_HIP(hipStreamSynchronize(s));
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_poses_from_pgo(uzl_scope* h, uzl_pgo* solver)
{
    UZL_GUARD_BEGIN(h)
    if (!solver) return fail(h, UZL_ERR_BAD_ARG, "null solver");
    UZL_HIP(hipSetDevice(h->cfg.device));
    const int rc = pgo_positions_to(solver, h->cfg.device, h->n, h->d_x.p, h->d_y.p, h->d_z.p, h->stream);
    if (rc == UZL_ERR_STATE) return fail(h, rc, "the solver holds no graph");
    if (rc != UZL_OK) return fail(h, rc, "the solver's device or node count differs from the scope's");
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_set_valid(uzl_scope* h, int32_t n, const int32_t* edge_index, const uint8_t* valid)
{
    UZL_GUARD_BEGIN(h)
    if (n < 0 || (n > 0 && (!edge_index || !valid))) return fail(h, UZL_ERR_BAD_ARG, "null arrays");
    for (int32_t k = 0; k < n; k++)
        if (edge_index[k] < 0 || (size_t)edge_index[k] >= h->edges.size()) return fail(h, UZL_ERR_BAD_ARG, "no such edge");
    for (int32_t k = 0; k < n; k++) {
        uzl_scope::Edge& e = h->edges[edge_index[k]];
        if ((e.valid != 0) != (valid[k] != 0)) h->plan_stale = true;
        e.valid = valid[k] != 0;
    }
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_set_uncertainty(uzl_scope* h, int32_t node, double value)
{
    UZL_GUARD_BEGIN(h)
    if (node < 0 || node >= h->n) return fail(h, UZL_ERR_NOT_FOUND, "no such node");
    UZL_HIP(hipSetDevice(h->cfg.device));
    UZL_HIP(hipMemcpyAsync(h->d_unc.p + node, &value, 8, hipMemcpyHostToDevice, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_reevaluate(uzl_scope* h, int32_t node, int32_t* start, int32_t* n_reached)
{
    UZL_GUARD_BEGIN(h)
    if (start) *start = -1;
    if (n_reached) *n_reached = 0;
    if (h->n == 0 || node >= h->n) return UZL_OK;                      // size() == 0 (:508) / existsNode(id) == false (:539)
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    ensure_plan(h);
    const int32_t n = h->n, source = node < 0 ? 0 : h->comp_min[node];
    h->d_dist.reserve((size_t)n); h->d_rec.reserve((size_t)n);
    const bool lds = n <= kScopeLdsNodes;
    if (!lds) h->d_front.reserve(2 * (((size_t)n + 31) / 32));
    ScopeArgs a;
    memset(&a, 0, sizeof(a));
    a.n = n; a.m = h->m; a.source = source; a.add_initial = node >= 0;
    a.x = h->d_x.p; a.y = h->d_y.p; a.z = h->d_z.p;
    a.row_ptr = h->d_row_ptr.p; a.row = h->d_row.p; a.col = h->d_col.p; a.w = h->d_w.p; a.rec = h->d_rec.p;
    a.dist = h->d_dist.p; a.front = h->d_front.p; a.unc = h->d_unc.p; a.result = h->d_res.p;
    launch_scope_sssp(a, s);
    UZL_HIP(hipGetLastError());
    ScopeResult r;
    UZL_HIP(hipMemcpyAsync(&r, h->d_res.p, sizeof(r), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    h->rounds = r.rounds; h->relaxations = r.relaxations; h->in_lds = lds; h->have_pass = true;
    if (start) *start = source;
    if (n_reached) *n_reached = (int32_t)r.n_reached;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_uncertainty(uzl_scope* h, int32_t cap, double* out)
{
    UZL_GUARD_BEGIN(h)
    return read_doubles(h, h->d_unc.p, cap, out);
    UZL_GUARD_END(h)
}

int uzl_scope_distance(uzl_scope* h, int32_t cap, double* out)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_pass && h->n > 0) return fail(h, UZL_ERR_STATE, "no pass has run over these nodes");
    return read_doubles(h, h->d_dist.p, cap, out);
    UZL_GUARD_END(h)
}

int uzl_scope_request(uzl_scope* h, int32_t current_node, double* radius, int32_t cap, int32_t* out, int32_t* n)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_list(h, cap, out, n)) return rc;
    *n = 0;
    if (current_node < 0 || current_node >= h->n) return fail(h, UZL_ERR_NOT_FOUND, "no such node");
    UZL_HIP(hipSetDevice(h->cfg.device));
    ScopeScanArgs a;
    memset(&a, 0, sizeof(a));
    a.current = current_node;
    a.scope_size_min = h->cfg.scope_size_min; a.scope_size_factor = h->cfg.scope_size_factor; a.out_margin = h->cfg.out_margin;
    scan(h, a, radius, cap, out, n);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_select(uzl_scope* h, const double* center, double radius, int32_t n_have, const int32_t* have, int32_t cap, int32_t* out,
                     int32_t* n)
{
    UZL_GUARD_BEGIN(h)
    if (int rc = check_list(h, cap, out, n)) return rc;
    *n = 0;
    if (!center || n_have < 0 || (n_have > 0 && !have)) return fail(h, UZL_ERR_BAD_ARG, "null centre or have[]");
    if (h->n == 0) return UZL_OK;
    UZL_HIP(hipSetDevice(h->cfg.device));
    std::vector<uint32_t> bits(((size_t)h->n + 31) / 32, 0u);
    for (int32_t k = 0; k < n_have; k++)
        if (have[k] >= 0 && have[k] < h->n) bits[(size_t)have[k] >> 5] |= 1u << (have[k] & 31);      // an id the graph lacks matches no node
    h->d_have.reserve(bits.size());
    UZL_HIP(hipMemcpyAsync(h->d_have.p, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, h->stream));
    ScopeScanArgs a;
    memset(&a, 0, sizeof(a));
    a.current = -1; a.cx = center[0]; a.cy = center[1]; a.cz = center[2]; a.radius = radius; a.have = h->d_have.p;
    scan(h, a, nullptr, cap, out, n);                                  // its waits cover the upload of bits
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_scope_stats(uzl_scope* h, int64_t* rounds, int64_t* relaxations, int32_t* in_lds)
{
    UZL_GUARD_BEGIN(h)
    if (rounds) *rounds = h->rounds;
    if (relaxations) *relaxations = h->relaxations;
    if (in_lds) *in_lds = h->in_lds;
    return UZL_OK;
    UZL_GUARD_END(h)
}

}  // extern "C"
