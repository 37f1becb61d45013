// uzl_merge.hip — node merging: the hop-limited merge search on the device and the rewrite plan on the host (C ABI uzl_merge_*).
//
// Mirrors GraphSlamNode::mergeTimerCallback (graph_slam/src/graph_slam_node.cpp:665-777) over SlamGraph::getNodesWithinHops
// (graph_slam_common/src/slam_graph.cpp:231-264), and mergeNodes (:919-986); include/uzl_mi355x.h states the contract.
// Host side: the edge list (from, to, type, valid) and from it - integer work, redone only when edges or flags change - the CSR of the
// valid edges of every type, a node's row in ascending edge index (graph_csr.hpp, shared with uzl_scope.hip).
// HBM: the poses as n x 12 (the rotations are needed, and a solver's poses arrive in that form) and their translations SoA, the CSR,
// partner[], the list of flagged starts.  A search is an upload of nothing (or of a rebuilt CSR), four launches (merge_kernels.hip),
// one 16-byte download and one wait.  The plan is a pure function of two poses and the edge list (merge_plan below); only the two
// poses come from the device, where set_poses or poses_from_pgo left them.
#include "graph_csr.hpp"
#include "merge_types.hpp"
#include "uzl_common.hpp"
#include "uzl_streams.hpp"

#include <algorithm>
#include <cfloat>
#include <new>

using namespace uzl;

struct uzl_merge : HandleBase {
    uzl_merge_cfg cfg;
    HandleStream stream;
    double trace_bound = 0.;                        // 1 + 2 cos(max_rotation_deg), computed once at create
    int32_t n = 0;
    std::vector<GraphEdge> edges;
    bool csr_stale = true;                          // edges or flags changed since the CSR was built
    DevBuf<double> d_pose12, d_x, d_y, d_z;
    DevBuf<int32_t> d_row_ptr, d_col, d_partner, d_starts, d_nstarts;
    DevBuf<unsigned long long> d_visited;
    DevBuf<MergeResult> d_res;
    bool searched = false;                          // d_nstarts / d_visited hold the counts of a search
};

namespace {

enum : int8_t { kUntouched = UZL_MERGE_EDGE_UNTOUCHED, kKeepFrom = UZL_MERGE_EDGE_KEEP_FROM, kKeepTo = UZL_MERGE_EDGE_KEEP_TO,
                kRetargetFrom = UZL_MERGE_EDGE_RETARGET_FROM, kRetargetTo = UZL_MERGE_EDGE_RETARGET_TO, kDelete = UZL_MERGE_EDGE_DELETE };

int check_cfg(const uzl_merge_cfg& c)
{
    if (std::isnan(c.max_distance) || std::isnan(c.max_rotation_deg) || std::isnan(c.scope_margin)) return UZL_ERR_BAD_ARG;
    if (c.max_hops < 0 || c.max_hops > UZL_MERGE_MAX_HOPS) return UZL_ERR_BAD_ARG;
    return UZL_OK;
}

bool walked(const GraphEdge& e) { return e.valid != 0; }                // only_valid = true (slam_graph.h:92); every type counts

void ensure_csr(uzl_merge* h)
{
    if (!h->csr_stale) return;
    hipStream_t s = h->stream;
    std::vector<int32_t> row_ptr, col;
    const int32_t m = build_csr(h->n, h->edges, walked, row_ptr, nullptr, col);
    h->d_row_ptr.reserve((size_t)h->n + 1); h->d_col.reserve(col.size());
    UZL_HIP(hipMemcpyAsync(h->d_row_ptr.p, row_ptr.data(), ((size_t)h->n + 1) * 4, hipMemcpyHostToDevice, s));
    if (m > 0) UZL_HIP(hipMemcpyAsync(h->d_col.p, col.data(), (size_t)m * 4, hipMemcpyHostToDevice, s));
    UZL_HIP(hipStreamSynchronize(s));                                  // the vectors go out of scope
    h->csr_stale = false;
}

// the three search launches over the starts >= first: partner[] is left on the device
MergeArgs search(uzl_merge* h, int32_t first, const double* center, double radius)
{
    hipStream_t s = h->stream;
    ensure_csr(h);
    const size_t n = (size_t)std::max(h->n, 1);
    h->d_partner.reserve(n); h->d_starts.reserve(n); h->d_nstarts.reserve(1); h->d_visited.reserve(1);
    MergeArgs a;
    memset(&a, 0, sizeof(a));
    a.n = h->n; a.first = first; a.max_hops = h->cfg.max_hops;
    a.cx = center[0]; a.cy = center[1]; a.cz = center[2];
    a.start_bound = radius + h->cfg.scope_margin;                       // :696
    a.max_distance = h->cfg.max_distance; a.trace_bound = h->trace_bound;
    a.pose12 = h->d_pose12.p; a.x = h->d_x.p; a.y = h->d_y.p; a.z = h->d_z.p;
    a.row_ptr = h->d_row_ptr.p; a.col = h->d_col.p;
    a.partner = h->d_partner.p; a.starts = h->d_starts.p; a.n_starts = h->d_nstarts.p; a.visited = h->d_visited.p; a.result = h->d_res.p;
    launch_merge_near(a, s);
    UZL_HIP(launch_merge_walk(a, s));
    UZL_HIP(hipGetLastError());
    h->searched = true;
    return a;
}

void upload_poses(uzl_merge* h, int32_t n, const double* poses)
{
    hipStream_t s = h->stream;
    const size_t room = (size_t)std::max(n, 1);
    h->d_pose12.reserve(room * 12); h->d_x.reserve(room); h->d_y.reserve(room); h->d_z.reserve(room);
    if (n == 0) return;
    UZL_HIP(hipMemcpyAsync(h->d_pose12.p, poses, (size_t)n * 96, hipMemcpyHostToDevice, s));
    launch_merge_split(h->d_pose12.p, n, h->d_x.p, h->d_y.p, h->d_z.p, s);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));                                  // the caller's array is free again
}

// ---------------------------------------------------------------------------------------------------------------------------------
// The rewrite plan: mergeNodes :919-986 for first = keep, second = drop.  Pure host arithmetic, one rounding per operation
// (-ffp-contract=off), written step for step as tests/merge_reference.py.  [EXT]: what the reference hands to Eigen.

struct Quat { double w, x, y, z; };

// Eigen::Quaterniond(Matrix3d) [EXT]; T is 3 x 4 row-major, not normalised
Quat quat_of(const double* T)
{
    const double m[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    Quat q;
    double t = m[0] + m[4] + m[8];
    if (t > 0.) {
        t = sqrt(t + 1.0);
        q.w = 0.5 * t; t = 0.5 / t;
        q.x = (m[7] - m[5]) * t; q.y = (m[2] - m[6]) * t; q.z = (m[3] - m[1]) * t;
    } else if (m[0] >= m[4] && m[0] >= m[8]) {
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q.x = 0.5 * t; t = 0.5 / t;
        q.w = (m[7] - m[5]) * t; q.y = (m[3] + m[1]) * t; q.z = (m[6] + m[2]) * t;
    } else if (m[4] > m[0] && m[4] >= m[8]) {
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q.y = 0.5 * t; t = 0.5 / t;
        q.w = (m[2] - m[6]) * t; q.z = (m[7] + m[5]) * t; q.x = (m[1] + m[3]) * t;
    } else {
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q.z = 0.5 * t; t = 0.5 / t;
        q.w = (m[3] - m[1]) * t; q.x = (m[2] + m[6]) * t; q.y = (m[5] + m[7]) * t;
    }
    return q;
}

// Eigen::Quaterniond::slerp [EXT]
Quat slerp(double t, const Quat& a, const Quat& b)
{
    const double d = ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w;
    const double ad = fabs(d);
    double s0, s1;
    if (ad >= 1.0 - DBL_EPSILON) { s0 = 1.0 - t; s1 = t; }
    else {
        const double theta = acos(ad), st = sin(theta);
        s0 = sin((1.0 - t) * theta) / st;
        s1 = sin(t * theta) / st;
    }
    if (d < 0.) s1 = -s1;
    return Quat{s0 * a.w + s1 * b.w, s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z};
}

// Eigen::AngleAxisd(Quaterniond) and its toRotationMatrix [EXT] -> R row-major
void rotation_of(const Quat& q, double* R)
{
    double n = sqrt((q.x * q.x + q.y * q.y) + q.z * q.z);
    double angle = 0., ax = 1., ay = 0., az = 0.;
    if (n != 0.) {
        angle = 2.0 * atan2(n, fabs(q.w));
        if (q.w < 0.) n = -n;
        ax = q.x / n; ay = q.y / n; az = q.z / n;
    }
    const double s = sin(angle), c = cos(angle);
    const double sx = s * ax, sy = s * ay, sz = s * az;
    const double cx = (1.0 - c) * ax, cy = (1.0 - c) * ay, cz = (1.0 - c) * az;
    double t = cx * ay; R[1] = t - sz; R[3] = t + sz;
    t = cx * az; R[2] = t + sy; R[6] = t - sy;
    t = cy * az; R[5] = t - sx; R[7] = t + sx;
    R[0] = cx * ax + c; R[4] = cy * ay + c; R[8] = cz * az + c;
}

// new_pose.inverse() * T for new_pose = [R | t]: rotation R^T R_T, translation R^T t_T + (-(R^T t))
void displacement_of(const double* R, const double* t, const double* T, double* out)
{
    const double Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out[4 * i + j] = (Rt[3 * i] * T[j] + Rt[3 * i + 1] * T[4 + j]) + Rt[3 * i + 2] * T[8 + j];
        const double inv_t = -((Rt[3 * i] * t[0] + Rt[3 * i + 1] * t[1]) + Rt[3 * i + 2] * t[2]);
        out[4 * i + 3] = ((Rt[3 * i] * T[3] + Rt[3 * i + 1] * T[7]) + Rt[3 * i + 2] * T[11]) + inv_t;
    }
}

// action [edges.size()] (may be null when there are none)
void merge_plan(const double* Tk, const double* Td, const std::vector<GraphEdge>& edges, int32_t keep, int32_t drop, int32_t ns_keep,
                int32_t ns_drop, uzl_merge_plan_out* out, int8_t* action)
{
    memset(out, 0, sizeof(*out));
    const double ratio = (double)ns_drop / ((double)ns_keep + (double)ns_drop);                          // :920-922
    double R[9];
    rotation_of(slerp(ratio, quat_of(Tk), quat_of(Td)), R);                                              // :923, :926
    const double t[3] = {(1.0 - ratio) * Tk[3] + ratio * Td[3], (1.0 - ratio) * Tk[7] + ratio * Td[7],
                         (1.0 - ratio) * Tk[11] + ratio * Td[11]};                                       // :924
    out->ratio = ratio;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) out->new_pose[4 * i + j] = R[3 * i + j];
        out->new_pose[4 * i + 3] = t[i];
    }
    displacement_of(R, t, Tk, out->keep_displacement);                                                   // :928
    displacement_of(R, t, Td, out->drop_displacement);                                                   // :929

    const int32_t ne = (int32_t)edges.size();
    std::vector<GraphEdge> now(edges);                                  // the ends as the loop of :960-986 leaves them
    std::vector<int32_t> of_keep;                                       // first.edges_
    for (int32_t k = 0; k < ne; k++) {                                  // :943-953
        action[k] = kUntouched;
        if (now[k].from == keep || now[k].to == keep) {
            of_keep.push_back(k);
            action[k] = now[k].from == keep ? kKeepFrom : kKeepTo;
        }
    }
    for (int32_t k = 0; k < ne; k++) {                                  // second.edges_ in ascending edge id
        GraphEdge& e = now[k];
        if (e.from != drop && e.to != drop) continue;
        if (e.from == keep || e.to == keep) { action[k] = kDelete; continue; }                           // :963
        const int32_t other = e.from == drop ? e.to : e.from;
        bool exists = false;                                            // existsEdge(first, other, type), slam_graph.cpp:407-422
        for (int32_t j : of_keep) {
            const GraphEdge& f = now[j];
            if (f.type == e.type && ((f.from == keep && f.to == other) || (f.from == other && f.to == keep))) { exists = true; break; }
        }
        if (exists) { action[k] = kDelete; continue; }
        if (e.from == drop) { action[k] = kRetargetFrom; e.from = keep; }
        else { action[k] = kRetargetTo; e.to = keep; }
        of_keep.push_back(k);                                           // :979
    }
    for (int32_t k = 0; k < ne; k++) {
        out->n_touched += action[k] != kUntouched;
        out->n_retargeted += action[k] == kRetargetFrom || action[k] == kRetargetTo;
        out->n_deleted += action[k] == kDelete;
    }
}

int check_plan_args(int32_t n, int32_t keep, int32_t drop, int32_t ns_keep, int32_t ns_drop)
{
    if (keep < 0 || keep >= n || drop < 0 || drop >= n || keep == drop) return UZL_ERR_BAD_ARG;
    if (ns_keep < 0 || ns_drop < 0 || (int64_t)ns_keep + ns_drop <= 0) return UZL_ERR_BAD_ARG;
    return UZL_OK;
}

}  // namespace

extern "C" {

void uzl_merge_cfg_default(uzl_merge_cfg* c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->max_distance = 0.25; c->max_rotation_deg = 15.; c->scope_margin = 6.; c->max_hops = 10; c->device = 0;
}

int uzl_merge_create(const uzl_merge_cfg* cfg, uzl_merge** out)
{
    return create_handle(cfg, uzl_merge_cfg_default, out, check_cfg, [](uzl_merge* h) {
        h->trace_bound = 1.0 + 2.0 * cos(h->cfg.max_rotation_deg * M_PI / 180.0);
        h->d_res.reserve(1);
    });
}

void uzl_merge_destroy(uzl_merge* h) { destroy_handle(h); }

const char* uzl_merge_last_error(uzl_merge* h) { return last_error_of(h); }

int32_t uzl_merge_max_nodes(void) { return kMergeMaxNodes; }

int uzl_merge_set_graph(uzl_merge* h, int32_t n_nodes, const double* poses, int32_t n_edges, const uzl_gate_edge* edges)
{
    UZL_GUARD_BEGIN(h)
    if (n_nodes < 0 || (n_nodes > 0 && !poses)) return fail(h, UZL_ERR_BAD_ARG, "null poses");
    if (n_nodes > kMergeMaxNodes) return fail(h, UZL_ERR_BAD_ARG, "more nodes than uzl_merge_max_nodes()");
    if (n_edges < 0 || (n_edges > 0 && !edges)) return fail(h, UZL_ERR_BAD_ARG, "null edges");
    if (n_edges > INT32_MAX / 2) return fail(h, UZL_ERR_BAD_ARG, "too many edges");
    for (int32_t k = 0; k < n_edges; k++)
        if (edges[k].from < 0 || edges[k].from >= n_nodes || edges[k].to < 0 || edges[k].to >= n_nodes)
            return fail(h, UZL_ERR_BAD_ARG, "an edge names a node outside the graph");
    UZL_HIP(hipSetDevice(h->cfg.device));
    upload_poses(h, n_nodes, poses);
    h->n = n_nodes;
    h->edges.clear();
    h->edges.reserve((size_t)n_edges);
    for (int32_t k = 0; k < n_edges; k++) h->edges.push_back({edges[k].from, edges[k].to, edges[k].type, edges[k].valid != 0});
    h->csr_stale = true; h->searched = false;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_merge_set_poses(uzl_merge* h, int32_t n_nodes, const double* poses)
{
    UZL_GUARD_BEGIN(h)
    if (n_nodes != h->n) return fail(h, UZL_ERR_BAD_ARG, "the node count differs from the graph's");
    if (n_nodes > 0 && !poses) return fail(h, UZL_ERR_BAD_ARG, "null poses");
    UZL_HIP(hipSetDevice(h->cfg.device));
    upload_poses(h, n_nodes, poses);
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_merge_poses_from_pgo(uzl_merge* h, uzl_pgo* solver)
{
    UZL_GUARD_BEGIN(h)
    if (!solver) return fail(h, UZL_ERR_BAD_ARG, "null solver");
    UZL_HIP(hipSetDevice(h->cfg.device));
    const int rc = pgo_poses12_to(solver, h->cfg.device, h->n, h->d_pose12.p, h->stream);
    if (rc == UZL_ERR_STATE) return fail(h, rc, "the solver holds no graph");
    if (rc != UZL_OK) return fail(h, rc, "the solver's device or node count differs from the merge handle's");
    launch_merge_split(h->d_pose12.p, h->n, h->d_x.p, h->d_y.p, h->d_z.p, h->stream);
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(h->stream));
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_merge_set_valid(uzl_merge* h, int32_t n, const int32_t* edge_index, const uint8_t* valid)
{
    UZL_GUARD_BEGIN(h)
    if (n < 0 || (n > 0 && (!edge_index || !valid))) return fail(h, UZL_ERR_BAD_ARG, "null arrays");
    for (int32_t k = 0; k < n; k++)
        if (edge_index[k] < 0 || (size_t)edge_index[k] >= h->edges.size()) return fail(h, UZL_ERR_BAD_ARG, "no such edge");
    for (int32_t k = 0; k < n; k++) {
        GraphEdge& e = h->edges[edge_index[k]];
        if ((e.valid != 0) != (valid[k] != 0)) h->csr_stale = true;
        e.valid = valid[k] != 0;
    }
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_merge_search(uzl_merge* h, int32_t first_index, const double* center, double radius, int32_t* keep, int32_t* drop, int32_t* next_index)
{
    UZL_GUARD_BEGIN(h)
    if (!center || !keep || !drop || !next_index) return fail(h, UZL_ERR_BAD_ARG, "null centre or outputs");
    if (first_index < 0) return fail(h, UZL_ERR_BAD_ARG, "negative first_index");
    *keep = *drop = -1; *next_index = first_index;
    if (h->n < 2) return UZL_OK;                                        // :671: current_merge_index_ stays as it is
    if (first_index >= h->n) first_index = 1;                           // :677-679
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    const MergeArgs a = search(h, first_index, center, radius);
    launch_merge_tick(a, s);
    UZL_HIP(hipGetLastError());
    MergeResult r;
    UZL_HIP(hipMemcpyAsync(&r, h->d_res.p, sizeof(r), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    *keep = r.keep; *drop = r.drop; *next_index = r.next_index;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_merge_partners(uzl_merge* h, const double* center, double radius, int32_t cap, int32_t* partner)
{
    UZL_GUARD_BEGIN(h)
    if (!center) return fail(h, UZL_ERR_BAD_ARG, "null centre");
    if (cap < h->n || (h->n > 0 && !partner)) return fail(h, UZL_ERR_BAD_ARG, "cap is smaller than the node count");
    if (h->n == 0) return 0;
    UZL_HIP(hipSetDevice(h->cfg.device));
    hipStream_t s = h->stream;
    search(h, 0, center, radius);
    UZL_HIP(hipMemcpyAsync(partner, h->d_partner.p, (size_t)h->n * 4, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    return h->n;
    UZL_GUARD_END(h)
}

int uzl_merge_stats(uzl_merge* h, int64_t* starts_walked, int64_t* nodes_visited)
{
    UZL_GUARD_BEGIN(h)
    int32_t starts = 0;
    unsigned long long visited = 0ull;
    if (h->searched) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        UZL_HIP(hipMemcpyAsync(&starts, h->d_nstarts.p, 4, hipMemcpyDeviceToHost, h->stream));
        UZL_HIP(hipMemcpyAsync(&visited, h->d_visited.p, 8, hipMemcpyDeviceToHost, h->stream));
        UZL_HIP(hipStreamSynchronize(h->stream));
    }
    if (starts_walked) *starts_walked = starts;
    if (nodes_visited) *nodes_visited = (int64_t)visited;
    return UZL_OK;
    UZL_GUARD_END(h)
}

int uzl_merge_plan(uzl_merge* h, int32_t keep, int32_t drop, int32_t n_stamps_keep, int32_t n_stamps_drop, uzl_merge_plan_out* out,
                   int32_t cap_edges, int8_t* edge_action)
{
    UZL_GUARD_BEGIN(h)
    if (!out) return fail(h, UZL_ERR_BAD_ARG, "null plan");
    if (check_plan_args(h->n, keep, drop, n_stamps_keep, n_stamps_drop)) return fail(h, UZL_ERR_BAD_ARG, "keep / drop must be two nodes of the graph, the stamp counts non-negative and not both zero");
    const int32_t ne = (int32_t)h->edges.size();
    if (cap_edges < ne || (ne > 0 && !edge_action)) return fail(h, UZL_ERR_BAD_ARG, "cap_edges is smaller than the edge count");
    UZL_HIP(hipSetDevice(h->cfg.device));
    double Tk[12], Td[12];
    UZL_HIP(hipMemcpyAsync(Tk, h->d_pose12.p + (size_t)keep * 12, 96, hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipMemcpyAsync(Td, h->d_pose12.p + (size_t)drop * 12, 96, hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    merge_plan(Tk, Td, h->edges, keep, drop, n_stamps_keep, n_stamps_drop, out, edge_action);
    return ne;
    UZL_GUARD_END(h)
}

}  // extern "C"

// merge_plan() without a handle or a device (tests/test_merge_plan_cpu.py): the plan for the two poses given (12 doubles each) and
// the edge list (from, to, type are read) of a graph of n_nodes nodes.
extern "C" UZL_DIAG_EXPORT int uzl_debug_merge_plan(int32_t n_nodes, const double* pose_keep, const double* pose_drop, int32_t n_edges,
                                                    const uzl_gate_edge* edges, int32_t keep, int32_t drop, int32_t n_stamps_keep,
                                                    int32_t n_stamps_drop, uzl_merge_plan_out* out, int8_t* edge_action)
{
    if (!pose_keep || !pose_drop || !out || n_edges < 0 || (n_edges > 0 && (!edges || !edge_action))) return UZL_ERR_BAD_ARG;
    if (check_plan_args(n_nodes, keep, drop, n_stamps_keep, n_stamps_drop)) return UZL_ERR_BAD_ARG;
    try {
        std::vector<GraphEdge> e;
        e.reserve((size_t)n_edges);
        for (int32_t k = 0; k < n_edges; k++) {
            if (edges[k].from < 0 || edges[k].from >= n_nodes || edges[k].to < 0 || edges[k].to >= n_nodes) return UZL_ERR_BAD_ARG;
            e.push_back({edges[k].from, edges[k].to, edges[k].type, edges[k].valid != 0});
        }
        merge_plan(pose_keep, pose_drop, e, keep, drop, n_stamps_keep, n_stamps_drop, out, edge_action);
        return n_edges;
    } catch (...) { return UZL_ERR_OOM; }
}
