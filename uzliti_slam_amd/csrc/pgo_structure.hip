// pgo_structure.hip — the structure of a pose graph as host-side values (pgo_structure.hpp): skip rules, gauge, vertex order, block
// system, and the decisions around it.  No handle, no HIP call, no environment.
#include "uzl_common.hpp"
#include "pgo_structure.hpp"

#include <algorithm>
#include <numeric>

namespace uzl {
// the skip rules of addGraphImpl: odometry edges are added while iterating (:78-79), filtered feature edges after (:100-103)
FlatEdges flatten_edges(int n_nodes, const std::vector<InEdge>& in_edges, const std::vector<uint8_t>& fixed_in)
{
    FlatEdges F;
    const int n_edges = (int)in_edges.size();
    for (int pass = 0; pass < 2; pass++) {
        for (int k = 0; k < n_edges; k++) {
            const InEdge& ed = in_edges[k];
            if (ed.from < 0 || ed.to < 0 || ed.from >= n_nodes || ed.to >= n_nodes) continue;     // :77, :194-201, :263-268
            if (ed.from == ed.to) continue;                                                        // degenerate self edge
            if ((pass == 0) != (ed.odom != 0)) continue;
            if (ed.odom) {
                if (fixed_in[ed.from] && !fixed_in[ed.to]) continue;                               // :203-206
            } else {
                if (!ed.valid) continue;                                                           // not in validEdges() (:98)
                if (fixed_in[ed.from] && fixed_in[ed.to]) continue;                                // :270-274
            }
            F.ij.push_back(ed.from); F.ij.push_back(ed.to);
            F.src.push_back(k);
            F.edge_w.push_back(ed.w);
            F.robust.push_back(ed.odom ? 0 : 1);                                                   // Huber on feature edges (:292-294)
        }
    }
    return F;
}

namespace {
// union-find root with path halving (gauge_fix)
int32_t uf_find(std::vector<int32_t>& p, int32_t x)
{
    while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; }
    return x;
}
}  // namespace

// G2: setFixedNodes (g2o_optimizer.cpp:301-349): per connected component (over the system edges) without a
// fixed vertex, fix the vertex with the smallest index (= lexicographically smallest node id, :338).
int32_t gauge_fix(int n, const std::vector<int32_t>& ij, std::vector<uint8_t>& fixed_eff)
{
    const int e = (int)(ij.size() / 2);
    std::vector<int32_t> p((size_t)n);
    std::iota(p.begin(), p.end(), 0);
    for (int k = 0; k < e; k++) {
        int32_t a = uf_find(p, ij[2 * k]), b = uf_find(p, ij[2 * k + 1]);
        if (a != b) { if (a < b) p[b] = a; else p[a] = b; }
    }
    std::vector<uint8_t> has((size_t)n, 0);
    for (int v = 0; v < n; v++) if (fixed_eff[v]) has[uf_find(p, v)] = 1;
    int32_t cnt = 0;
    for (int v = 0; v < n; v++) {
        const int32_t r = uf_find(p, v);
        if (!has[r]) { fixed_eff[r] = 1; has[r] = 1; cnt++; }
    }
    return cnt;
}

// Order of the free vertices in the block system.  The multilevel preconditioner aggregates 8 CONSECUTIVE blocks, which is only a
// good coarse space when consecutive blocks are strongly coupled.  In a single session the node ids are time-ordered (std::map
// order = trajectory order, graph_slam_node.cpp:294) and the index order is already that; in merged / global-scope graphs
// (graph_slam_node.cpp:401-576, 665-777: ids of several sessions interleave) or graphs without an odometry chain it is not, and
// the PCG iteration count grows 4-7x (tests/diag/vertex_order.py).  So the order is computed from the graph: starting at the
// lowest-index unvisited free vertex, follow the heaviest edge (trace of the information matrix; odometry edges are the stiff
// ones) to an unvisited free vertex until stuck, then extend the same chain backwards from the start; repeat.  Ties go to the lower
// index.  A time-ordered single-session graph comes out in index order (nothing changes for it); O(N + E), deterministic.
std::vector<int32_t> aggregation_order(int n, const std::vector<int32_t>& ij, const std::vector<uint8_t>& fixed_eff, const std::vector<double>& edge_w)
{
    const int e = (int)(ij.size() / 2);
    std::vector<int32_t> ptr((size_t)n + 1, 0);
    auto is_free = [&](int v) { return !fixed_eff[v]; };
    for (int k = 0; k < e; k++) {
        const int a = ij[2 * k], b = ij[2 * k + 1];
        if (is_free(a) && is_free(b)) { ptr[a + 1]++; ptr[b + 1]++; }
    }
    for (int v = 0; v < n; v++) ptr[v + 1] += ptr[v];
    std::vector<int32_t> nbr((size_t)std::max(ptr[n], 1));
    std::vector<double> wgt((size_t)std::max(ptr[n], 1));
    std::vector<int32_t> fill(ptr.begin(), ptr.end() - 1);
    const bool have_w = edge_w.size() == (size_t)e;
    for (int k = 0; k < e; k++) {
        const int a = ij[2 * k], b = ij[2 * k + 1];
        if (!(is_free(a) && is_free(b))) continue;
        const double w = have_w ? edge_w[k] : 1.;
        nbr[fill[a]] = b; wgt[fill[a]++] = w;
        nbr[fill[b]] = a; wgt[fill[b]++] = w;
    }
    std::vector<uint8_t> seen((size_t)std::max(n, 1), 0);
    std::vector<int32_t> order, back;
    order.reserve((size_t)n);
    auto next_of = [&](int v) {
        int best = -1; double bw = -1.;
        for (int q = ptr[v]; q < ptr[v + 1]; q++) {
            const int u = nbr[q];
            if (seen[u]) continue;
            if (wgt[q] > bw || (wgt[q] == bw && u < best)) { bw = wgt[q]; best = u; }
        }
        return best;
    };
    for (int start = 0; start < n; start++) {
        if (!is_free(start) || seen[start]) continue;
        const size_t first = order.size();
        for (int v = start; v >= 0; v = next_of(v)) { seen[v] = 1; order.push_back(v); }
        back.clear();
        for (int v = next_of(start); v >= 0; v = next_of(v)) { seen[v] = 1; back.push_back(v); }
        if (!back.empty()) {                                     // chain = reverse(back) + forward part
            order.insert(order.begin() + (std::ptrdiff_t)first, back.rbegin(), back.rend());
        }
    }
    return order;
}

// row blocks of the Hessian build: consecutive rows with <= 256 slots and <= 42 rows, so that a workgroup makes one pass (a row with
// more slots is a block of its own and loops); beyond kMaxPartials blocks (> ~1M slots) blocks hold more and loop as well
std::vector<int32_t> row_blocks(int nb, const std::vector<int32_t>& row_ptr, int32_t* caps)
{
    const int nslots = row_ptr[nb];
    std::vector<int32_t> rb_ptr(1, 0);
    const int cap_slots = std::max(256, (int)(((int64_t)nslots + kMaxPartials / 2 - 1) / (kMaxPartials / 2) + 255) / 256 * 256);
    const int cap_rows = std::max(42, (nb + kMaxPartials / 2 - 1) / (kMaxPartials / 2));
    int rows = 0, slots = 0;
    for (int a = 0; a < nb; a++) {
        const int d = row_ptr[a + 1] - row_ptr[a];
        if (rows > 0 && (rows >= cap_rows || slots + d > cap_slots)) { rb_ptr.push_back(a); rows = 0; slots = 0; }
        rows++; slots += d;
    }
    rb_ptr.push_back(nb);
    if (caps) { caps[0] = cap_slots; caps[1] = cap_rows; }
    return rb_ptr;
}

std::vector<int32_t> row_headers(int nb, const std::vector<int32_t>& row_ptr, const std::vector<int32_t>& col)
{
    std::vector<int32_t> hdr((size_t)std::max(nb, 1) * kRowHdr, -1);
    for (int a = 0; a < nb; a++) {
        hdr[(size_t)a * kRowHdr] = row_ptr[a]; hdr[(size_t)a * kRowHdr + 1] = row_ptr[a + 1];
        for (int k = 0; k < 20 && row_ptr[a] + k < row_ptr[a + 1]; k++) hdr[(size_t)a * kRowHdr + 2 + k] = col[row_ptr[a] + k];
    }
    return hdr;
}

// block-CSR structure over the free vertices (one slot per (free endpoint, system edge))
SystemPlan system_plan(int n, const std::vector<int32_t>& ij, const std::vector<uint8_t>& robust, std::vector<int32_t> b2v_in)
{
    SystemPlan Y;
    Y.b2v = std::move(b2v_in);
    const int e = (int)(ij.size() / 2), nb = (int)Y.b2v.size();
    const std::vector<int32_t>& b2v = Y.b2v;
    std::vector<int32_t>& v2b = Y.v2b;
    v2b.assign((size_t)std::max(n, 1), -1);
    for (int b = 0; b < nb; b++) v2b[b2v[b]] = b;
    Y.nb = nb;
    std::vector<int32_t>& row_ptr = Y.row_ptr;
    row_ptr.assign((size_t)nb + 1, 0);
    for (int k = 0; k < e; k++) {
        const int a = v2b[ij[2 * k]], b = v2b[ij[2 * k + 1]];
        if (a >= 0) row_ptr[a + 1]++;
        if (b >= 0) row_ptr[b + 1]++;
    }
    for (int a = 0; a < nb; a++) row_ptr[a + 1] += row_ptr[a];
    const int nslots = row_ptr[nb];
    Y.nslots = nslots;
    std::vector<int32_t> fill(row_ptr.begin(), row_ptr.end() - 1);
    std::vector<int32_t> slot_i((size_t)std::max(e, 1)), slot_j((size_t)std::max(e, 1));
    std::vector<int32_t>& col = Y.col;
    std::vector<int32_t>& slot_edge = Y.slot_edge;
    col.resize((size_t)std::max(nslots, 1)); slot_edge.resize((size_t)std::max(nslots, 1));
    for (int k = 0; k < e; k++) {
        const int a = v2b[ij[2 * k]], b = v2b[ij[2 * k + 1]];
        slot_i[k] = -1; slot_j[k] = -1;
        if (a >= 0) { const int s = fill[a]++; slot_i[k] = s; col[s] = b; slot_edge[s] = 2 * k; }
        if (b >= 0) { const int s = fill[b]++; slot_j[k] = s; col[s] = a; slot_edge[s] = 2 * k + 1; }
    }
    Y.smeta.resize((size_t)std::max(nslots, 1) * 4);
    for (int q = 0; q < nslots; q++) {
        const int k = slot_edge[q] >> 1, other = (slot_edge[q] & 1) ? slot_i[k] : slot_j[k];
        int32_t* m = &Y.smeta[(size_t)q * 4];
        m[0] = slot_edge[q]; m[1] = ij[2 * k]; m[2] = ij[2 * k + 1]; m[3] = (other + 1) | (robust[k] ? 1 << 30 : 0);
    }
    Y.rb_ptr = row_blocks(nb, row_ptr);
    Y.rowhdr = row_headers(nb, row_ptr, col);
    return Y;
}

std::vector<double> slot_weights(const SystemPlan& Y, const std::vector<double>& edge_w)
{
    std::vector<double> slot_w((size_t)std::max(Y.nslots, 1));
    for (int q = 0; q < Y.nslots; q++) slot_w[q] = edge_w[Y.slot_edge[q] >> 1];
    return slot_w;
}

std::vector<int32_t> reduced_b2v(const std::vector<int32_t>& sep_rows, const std::vector<int32_t>& b2v)
{
    std::vector<int32_t> rb2v(sep_rows.size());
    for (size_t i = 0; i < sep_rows.size(); i++) rb2v[i] = sep_rows[i] >= 0 ? b2v[sep_rows[i]] : -1;
    return rb2v;
}

// The reduced system of a large chain-like graph is numbered by strong aggregates (pgo_schur.hpp) and takes the AGG = 4 hierarchy: the
// separators an aggregate holds then move (nearly) rigidly together, which is what its six coarse modes can represent.  In row order
// "8 consecutive separators" put loop-closure partners into different aggregates and the two ends of a long soft run into the same
// one: config 5's last re-optimisation took 70 - 140 PCG iterations per LM iteration (tests/diag/reduced_proto.py: 70 -> 23).
ReducedNumbering reduced_numbering(int cfg_numbering, int preconditioner, bool may_shard, const double num_its[2])
{
    int strong_min = (may_shard || preconditioner == 0) ? 0 : kSchurStrongMin;
    // Which numbering (uzl_pgo_cfg::reduced_numbering)?  Strong aggregates pay where loop closures are stiffer than the runs between
    // separators (config 5: 71 -> 31 PCG iterations per LM iteration); where the runs are the stiff part the matching follows the chain,
    // the groups are runs of consecutive separators anyway, and the row order with its level-1 path is better (tests/diag/strong_ab.py).
    // A handle's first structure goes by that shape; afterwards by what its own solves measured - PCG iterations per LM trial of the last
    // solve in either numbering, an iteration on the padded AGG = 4 layout counted as 1.3 (the measured 1.5x per iteration less the rebuilds it saves; up to 256 groups
    // the strong layout runs on the level-1 path, at the row order's cost per iteration) - so an online session that
    // started on the wrong foot corrects itself.  Iteration counts only: deterministic.
    double max_contig = 2.;
    const double cost_strong = 1.;                                       // (the weight of the layout is in the figure: do_optimize)
    if (cfg_numbering == 1) strong_min = 0;
    else if (cfg_numbering != 2 && strong_min > 0) {
        const double ir = num_its[0], is = num_its[1];
        bool strong;
        if (ir >= 0. && is >= 0.) strong = cost_strong * is < ir;        // both known: the cheaper (the figures are of different solves: a hard
                                                                          // interval can send it the wrong way for one solve - whose own figure sets it right)
        else if (ir >= 0.) strong = ir > 40.;                            // only the row order known: if it is doing badly, try
        else if (is >= 0.) strong = !(is > 40.);                         // only strong aggregates known: likewise
        else { strong = true; max_contig = 0.6; }                        // first structure: by the shape of the groups
        if (!strong) strong_min = 0;
    }
    return {strong_min, max_contig};
}

// (reduced when >= 64 rows and >= kSchurMinPct of the rows go: the plan stops early otherwise)
int schur_min_interiors(int nb) { return std::max(64, (int)(((int64_t)kSchurMinPct * nb + 99) / 100)); }
bool schur_admitted(int nb, int n_int) { return n_int >= 64 && (int64_t)100 * n_int >= (int64_t)kSchurMinPct * nb; }

ShardRange shard_range(int e, int rank, int world)
{
    const int base = e / world, rem = e % world;
    ShardRange r;
    r.e_begin = rank * base + std::min(rank, rem);
    r.e_end = r.e_begin + base + (rank < rem ? 1 : 0);
    r.diag_owner = rank == 0 ? 1 : 0;
    return r;
}

ExchangeLayout exchange_layout(int nbp, const MlPlan& P)
{
    const int gl = P.gather_level;
    const size_t ng6 = gl ? (size_t)P.n[gl] * 6 * (gl == 2 ? 2 : 1) : 0;      // gather level 2: two half-aggregate parts per entity (sg_at)
    ExchangeLayout X;
    X.sg = (size_t)nbp * 6;
    X.part_a = (size_t)nbp * 6 + ng6;
    X.iter_span = (int64_t)((size_t)nbp * 6 + ng6 + (gl ? (size_t)g_ml_spmv(nbp, P.agg) : 0));
    return X;
}

// What a handle learned about the numbering of its reduced systems (uzl_pgo::num_its) belongs to the session it came from: it is
// kept while the graph is the previous one, unchanged or GROWN - at least as many nodes, the old nodes' fixed flags in front, AND the old
// system edges still there in their order (nine in ten of them found in order in the new list: an online session appends edges and
// invalidates a few, graph_slam_node.cpp:1138-1150) - and dropped for anything else: an unrelated graph on a reused handle then solves
// as on a fresh one (round 5 looked at the fixed flags only, which for most graphs is "node 0 is fixed").
bool edges_survive_in_order(const std::vector<int32_t>& old_ij, const std::vector<int32_t>& new_ij, size_t window)
{
    const size_t n_old = old_ij.size() / 2, n_new = new_ij.size() / 2;
    if (n_old == 0) return true;
    size_t at = 0, found = 0;
    for (size_t k = 0; k < n_old; k++) {
        const int32_t a = old_ij[2 * k], c = old_ij[2 * k + 1];
        const size_t end = std::min(n_new, at + window);
        for (size_t q = at; q < end; q++)
            if (new_ij[2 * q] == a && new_ij[2 * q + 1] == c) { found++; at = q + 1; break; }
        if (10 * (found + (n_old - k - 1)) < 9 * n_old) return false;      // out of reach already: an unrelated graph costs n_old / 10 windows, not n_old
    }
    return 10 * found >= 9 * n_old;
}
bool graph_grown(int n_old, const std::vector<uint8_t>& old_fixed, const std::vector<int32_t>& old_ij, int n_new, const std::vector<uint8_t>& new_fixed,
                 const std::vector<int32_t>& new_ij, size_t window)
{
    return n_new >= n_old && (size_t)n_old <= old_fixed.size() && std::equal(old_fixed.begin(), old_fixed.begin() + n_old, new_fixed.begin()) &&
           edges_survive_in_order(old_ij, new_ij, window);
}

// uzl_pgo_rewrite_graph's host half: validation first (a refused rewrite changes nothing), then the two compactions.  The ops are the
// actions of uzl_merge_plan (contract 6): KEEP_x multiplies one side's displacement, RETARGET_x also moves that endpoint, DELETE removes;
// removeNode's edge removal (graph_slam_node.cpp:636-660) is the second rule - an edge that still names a dropped node goes with it.
RewritePlan rewrite_plan(int n, const std::vector<InEdge>& in_edges, const std::vector<uint8_t>& fixed_in, const RewriteIn& rw)
{
    RewritePlan P;
    const int e_in = (int)in_edges.size();
    auto refuse = [&](const char* why) { P = RewritePlan(); P.why = why; return P; };
    std::vector<uint8_t> dropped((size_t)n, 0), posed((size_t)n, 0);
    for (int32_t v : rw.drop_nodes) {
        if (v < 0 || v >= n) return refuse("drop_nodes: node index out of range");
        if (dropped[v]) return refuse("drop_nodes: a node is listed twice");
        dropped[v] = 1;
    }
    for (int32_t v : rw.pose_nodes) {
        if (v < 0 || v >= n) return refuse("pose_nodes: node index out of range");
        if (dropped[v]) return refuse("pose_nodes: the node is dropped");
        if (posed[v]) return refuse("pose_nodes: a node is listed twice");
        posed[v] = 1;
    }
    // per edge: what its ops leave of it
    struct Touch { int32_t from, to, xf_from = -1, xf_to = -1; bool on_from = false, on_to = false, del = false; };
    std::vector<Touch> T((size_t)e_in);
    for (int k = 0; k < e_in; k++) { T[k].from = in_edges[k].from; T[k].to = in_edges[k].to; }
    for (const RewriteOp& op : rw.ops) {
        if (op.edge < 0 || op.edge >= e_in) return refuse("ops: edge index out of range");
        Touch& t = T[op.edge];
        if (op.action == UZL_MERGE_EDGE_DELETE) {
            if (t.del || t.on_from || t.on_to) return refuse("ops: DELETE stands alone on its edge");
            t.del = true;
            continue;
        }
        const bool from_side = op.action == UZL_MERGE_EDGE_KEEP_FROM || op.action == UZL_MERGE_EDGE_RETARGET_FROM;
        const bool to_side = op.action == UZL_MERGE_EDGE_KEEP_TO || op.action == UZL_MERGE_EDGE_RETARGET_TO;
        if (!from_side && !to_side) return refuse("ops: unknown action");
        if (t.del) return refuse("ops: DELETE stands alone on its edge");
        if (from_side ? t.on_from : t.on_to) return refuse("ops: two ops on one side of an edge");
        if (op.xf < 0 || op.xf >= rw.n_xf) return refuse("ops: xf index out of range");
        const bool retarget = op.action == UZL_MERGE_EDGE_RETARGET_FROM || op.action == UZL_MERGE_EDGE_RETARGET_TO;
        if (retarget && (op.node < 0 || op.node >= n)) return refuse("ops: RETARGET to a node out of range");
        if (retarget && dropped[op.node]) return refuse("ops: RETARGET to a dropped node");
        if (from_side) { t.on_from = true; t.xf_from = op.xf; if (retarget) t.from = op.node; }
        else { t.on_to = true; t.xf_to = op.xf; if (retarget) t.to = op.node; }
    }
    P.old_to_new_node.assign((size_t)n, -1);
    for (int v = 0; v < n; v++) {
        if (dropped[v]) continue;
        P.old_to_new_node[v] = (int32_t)P.new_to_old_node.size();
        P.new_to_old_node.push_back(v);
        P.fixed_in.push_back(fixed_in[v]);
    }
    auto names_dropped = [&](int32_t v) { return v >= 0 && v < n && dropped[v]; };
    auto renumber = [&](int32_t v) { return (v >= 0 && v < n) ? P.old_to_new_node[v] : v; };
    P.old_to_new_edge.assign((size_t)e_in, -1);
    for (int k = 0; k < e_in; k++) {
        const Touch& t = T[k];
        if (t.del || names_dropped(t.from) || names_dropped(t.to)) continue;
        P.old_to_new_edge[k] = (int32_t)P.new_to_old_edge.size();
        P.new_to_old_edge.push_back(k);
        P.rec.push_back({renumber(t.from), renumber(t.to), t.xf_from, t.xf_to});
        InEdge ed = in_edges[k];
        ed.from = P.rec.back().from_new; ed.to = P.rec.back().to_new;
        P.in_edges.push_back(ed);
    }
    return P;
}
}  // namespace uzl

#ifdef UZL_DIAG
#include "pgo_schur.hpp"
// The structure's plans without a handle or a device (tests/test_pgo_structure_plan.py).  One stage per call, one output array per call;
// stateless: the stage is recomputed per call.  iv / dv: the stage's integer / double scalars; *nbytes: in = the room at `out` (ignored
// when out is null), out = the array's size in bytes.  Arrays a stage does not read may be null.
//   stage 0 flatten_edges   iv {n, e_in}; fixed [n]; aux [e_in][4] = {from, to, odom, valid}; edge_w [e_in] (the input edges' weights)
//                           what 0 ij, 1 src (i32), 2 robust (u8), 3 edge_w (f64)
//   stage 1 gauge_fix       iv {n, e}; fixed [n]; ij.                 what 0 fixed_eff (u8), 1 {vertices it fixed} (i32)
//   stage 2 aggregation_order  iv {n, e}; fixed [n] (effective); ij; edge_w [e] or null.   what 0 b2v (i32)
//   stage 3 system_plan     iv {n, e, nb}; ij; robust [e]; aux = b2v [nb].    what 0 {nb, nslots, row blocks}, 1 v2b, 2 row_ptr, 3 col,
//                           4 slot_edge, 5 smeta [nslots][4], 6 rb_ptr, 7 row headers [max(nb, 1)][kRowHdr] (all i32)
//   stage 4 row_blocks      iv {nb}; aux = row_ptr [nb + 1].           what 0 rb_ptr, 1 {cap_slots, cap_rows, kMaxPartials} (i32)
//   stage 5 reduced_numbering  iv {cfg.reduced_numbering, cfg.preconditioner, may_shard}; dv = num_its [2].   what 0 {strong_min, max_contig} (f64)
//   stage 6 Schur admission iv {nb, n_int}.                            what 0 {min_interiors, admitted} (i32)
//   stage 7 shard_range     iv {e, rank, world}.                       what 0 {e_begin, e_end, diag_owner} (i32)
//   stage 8 exchange_layout iv {nb, flags of uzl_debug_ml_plan}; aux = row_ptr [nb + 1]; ij = col: of the system the PCG solves.
//                           what 0 {Sg offset, part_a offset, iter_span, gather level, n of the gather level} (i64)
//   stage 9 graph_grown     iv {n_old, n_new, e_old, e_new, window}; fixed = old flags [n_old] then new flags [n_new]; aux = old ij; ij = new ij.
//                           what 0 {edges_survive_in_order, graph_grown} (i32)
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_structure_plan(int32_t stage, const int32_t* iv, const double* dv, const uint8_t* fixed, const int32_t* ij,
                                                            const uint8_t* robust, const double* edge_w, const int32_t* aux, int32_t what, void* out, int64_t* nbytes)
{
    using namespace uzl;
    if (!iv || !nbytes || what < 0) return UZL_ERR_BAD_ARG;
    try {
        std::vector<int32_t> oi; std::vector<uint8_t> ob; std::vector<double> od; std::vector<int64_t> ol;
        int kind = 0;                                          // which of the four holds the answer: 0 i32, 1 u8, 2 f64, 3 i64
        auto vec_i = [](const int32_t* p, size_t n) { return p ? std::vector<int32_t>(p, p + n) : std::vector<int32_t>(n, 0); };
        auto vec_b = [](const uint8_t* p, size_t n) { return p ? std::vector<uint8_t>(p, p + n) : std::vector<uint8_t>(n, 0); };
        switch (stage) {
        case 0: {
            const int n = iv[0], e_in = iv[1];
            if (n < 0 || e_in < 0 || (e_in > 0 && (!aux || !edge_w)) || (n > 0 && !fixed)) return UZL_ERR_BAD_ARG;
            std::vector<InEdge> in((size_t)e_in);
            for (int k = 0; k < e_in; k++) in[k] = {aux[4 * k], aux[4 * k + 1], (uint8_t)(aux[4 * k + 2] ? 1 : 0), (uint8_t)(aux[4 * k + 3] ? 1 : 0), edge_w[k]};
            FlatEdges F = flatten_edges(n, in, vec_b(fixed, (size_t)n));
            if (what == 0) oi.swap(F.ij); else if (what == 1) oi.swap(F.src); else if (what == 2) { ob.swap(F.robust); kind = 1; }
            else if (what == 3) { od.swap(F.edge_w); kind = 2; } else return UZL_ERR_BAD_ARG;
            break;
        }
        case 1: {
            const int n = iv[0], e = iv[1];
            if (n < 0 || e < 0 || (e > 0 && !ij) || (n > 0 && !fixed) || what > 1) return UZL_ERR_BAD_ARG;
            ob = vec_b(fixed, (size_t)n);
            const int32_t cnt = gauge_fix(n, vec_i(ij, 2 * (size_t)e), ob);
            if (what == 0) kind = 1; else oi.assign(1, cnt);
            break;
        }
        case 2: {
            const int n = iv[0], e = iv[1];
            if (n < 0 || e < 0 || (e > 0 && !ij) || (n > 0 && !fixed) || what > 0) return UZL_ERR_BAD_ARG;
            oi = aggregation_order(n, vec_i(ij, 2 * (size_t)e), vec_b(fixed, (size_t)n), edge_w ? std::vector<double>(edge_w, edge_w + e) : std::vector<double>());
            break;
        }
        case 3: {
            const int n = iv[0], e = iv[1], nb = iv[2];
            if (n < 0 || e < 0 || nb < 0 || nb > n || (e > 0 && (!ij || !robust)) || (nb > 0 && !aux) || what > 7) return UZL_ERR_BAD_ARG;
            for (int b = 0; b < nb; b++) if (aux[b] < 0 || aux[b] >= n) return UZL_ERR_BAD_ARG;
            for (int k = 0; k < 2 * e; k++) if (ij[k] < 0 || ij[k] >= n) return UZL_ERR_BAD_ARG;
            SystemPlan Y = system_plan(n, vec_i(ij, 2 * (size_t)e), vec_b(robust, (size_t)e), vec_i(aux, (size_t)nb));
            Y.col.resize((size_t)Y.nslots); Y.slot_edge.resize((size_t)Y.nslots); Y.smeta.resize((size_t)Y.nslots * 4); Y.v2b.resize((size_t)n);
            std::vector<int32_t>* v[8] = {nullptr, &Y.v2b, &Y.row_ptr, &Y.col, &Y.slot_edge, &Y.smeta, &Y.rb_ptr, &Y.rowhdr};
            if (what == 0) oi = {Y.nb, Y.nslots, (int32_t)Y.rb_ptr.size() - 1}; else oi.swap(*v[what]);
            break;
        }
        case 4: {
            const int nb = iv[0];
            if (nb < 0 || !aux || what > 1) return UZL_ERR_BAD_ARG;
            int32_t caps[2];
            oi = row_blocks(nb, vec_i(aux, (size_t)nb + 1), caps);
            if (what == 1) oi = {caps[0], caps[1], kMaxPartials};
            break;
        }
        case 5: {
            if (!dv || what > 0) return UZL_ERR_BAD_ARG;
            const ReducedNumbering R = reduced_numbering(iv[0], iv[1], iv[2] != 0, dv);
            od = {(double)R.strong_min, R.max_contig}; kind = 2;
            break;
        }
        case 6:
            if (what > 0) return UZL_ERR_BAD_ARG;
            oi = {schur_min_interiors(iv[0]), schur_admitted(iv[0], iv[1]) ? 1 : 0};
            break;
        case 7: {
            if (what > 0 || iv[2] < 1 || iv[1] < 0 || iv[1] >= iv[2] || iv[0] < 0) return UZL_ERR_BAD_ARG;
            const ShardRange R = shard_range(iv[0], iv[1], iv[2]);
            oi = {R.e_begin, R.e_end, R.diag_owner};
            break;
        }
        case 8: {
            const int nb = iv[0], flags = iv[1];
            if (nb < 0 || !aux || (aux[nb] > 0 && !ij) || what > 0) return UZL_ERR_BAD_ARG;
            MlPlanIn in;
            in.nb = nb; in.nslots = aux[nb];
            in.precond_on = flags & 1; in.strong_blocks = flags & 2; in.mult_banned = flags & 4; in.comp4_off = flags & 8;
            const MlPlan P = ml_plan(in, vec_i(aux, (size_t)nb + 1), vec_i(ij, (size_t)aux[nb]));
            const ExchangeLayout X = exchange_layout(nb, P);
            ol = {(int64_t)X.sg, (int64_t)X.part_a, X.iter_span, P.gather_level, P.gather_level ? P.n[P.gather_level] : 0}; kind = 3;
            break;
        }
        case 9: {
            const int n_old = iv[0], n_new = iv[1], e_old = iv[2], e_new = iv[3], window = iv[4];
            if (n_old < 0 || n_new < 0 || e_old < 0 || e_new < 0 || window < 1 || (n_old + n_new > 0 && !fixed) || (e_old > 0 && !aux) || (e_new > 0 && !ij) || what > 0)
                return UZL_ERR_BAD_ARG;
            const std::vector<int32_t> o = vec_i(aux, 2 * (size_t)e_old), w = vec_i(ij, 2 * (size_t)e_new);
            oi = {edges_survive_in_order(o, w, (size_t)window) ? 1 : 0,
                  graph_grown(n_old, vec_b(fixed, (size_t)n_old), o, n_new, vec_b(fixed ? fixed + n_old : nullptr, (size_t)n_new), w, (size_t)window) ? 1 : 0};
            break;
        }
        default: return UZL_ERR_BAD_ARG;
        }
        const void* src = kind == 0 ? (const void*)oi.data() : kind == 1 ? (const void*)ob.data() : kind == 2 ? (const void*)od.data() : (const void*)ol.data();
        const int64_t bytes = kind == 0 ? (int64_t)oi.size() * 4 : kind == 1 ? (int64_t)ob.size() : kind == 2 ? (int64_t)od.size() * 8 : (int64_t)ol.size() * 8;
        if (out && bytes) {
            if (*nbytes < bytes) return UZL_ERR_BAD_ARG;
            memcpy(out, src, (size_t)bytes);
        }
        *nbytes = bytes;
        return UZL_OK;
    } catch (const std::bad_alloc&) {
        return UZL_ERR_OOM;
    }
}

// rewrite_plan without a handle or a device (tests/test_pgo_rewrite_plan_cpu.py), one output array per call like the hook above.
//   iv {n, e_in, n_drop, n_pose, n_xf, n_ops}; fixed [n]; in_edges [e_in][4] = {from, to, odom, valid}; drop [n_drop]; pose_nodes [n_pose];
//   ops [n_ops][4] = {edge, action, xf, node} (uzl_pgo_edge_op).  A rewrite the plan refuses returns UZL_ERR_BAD_ARG, as uzl_pgo_rewrite_graph does.
//   what 0 {n_new, e_new}, 1 old_to_new_node, 2 new_to_old_node, 3 old_to_new_edge, 4 new_to_old_edge, 5 the surviving edges' records
//   [e_new][4] = {from_new, to_new, xf_from, xf_to}, 6 the new in_edges [e_new][4] (all i32), 7 the new fixed flags (u8)
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_rewrite_plan(const int32_t* iv, const uint8_t* fixed, const int32_t* in_edges, const int32_t* drop, const int32_t* pose_nodes,
                                                          const int32_t* ops, int32_t what, void* out, int64_t* nbytes)
{
    using namespace uzl;
    if (!iv || !nbytes || what < 0 || what > 7) return UZL_ERR_BAD_ARG;
    const int n = iv[0], e_in = iv[1], n_drop = iv[2], n_pose = iv[3], n_xf = iv[4], n_ops = iv[5];
    if (n < 0 || e_in < 0 || n_drop < 0 || n_pose < 0 || n_xf < 0 || n_ops < 0 || (n > 0 && !fixed) || (e_in > 0 && !in_edges) || (n_drop > 0 && !drop) ||
        (n_pose > 0 && !pose_nodes) || (n_ops > 0 && !ops))
        return UZL_ERR_BAD_ARG;
    try {
        std::vector<InEdge> in((size_t)e_in);
        for (int k = 0; k < e_in; k++) in[k] = {in_edges[4 * k], in_edges[4 * k + 1], (uint8_t)(in_edges[4 * k + 2] ? 1 : 0), (uint8_t)(in_edges[4 * k + 3] ? 1 : 0), 1.};
        RewriteIn rw;
        rw.drop_nodes.assign(drop, drop + n_drop); rw.pose_nodes.assign(pose_nodes, pose_nodes + n_pose); rw.n_xf = n_xf;
        for (int q = 0; q < n_ops; q++) rw.ops.push_back({ops[4 * q], ops[4 * q + 1], ops[4 * q + 2], ops[4 * q + 3]});
        const RewritePlan P = rewrite_plan(n, in, std::vector<uint8_t>(fixed, fixed + n), rw);
        if (P.why) return UZL_ERR_BAD_ARG;
        std::vector<int32_t> oi;
        switch (what) {
        case 0: oi = {(int32_t)P.new_to_old_node.size(), (int32_t)P.new_to_old_edge.size()}; break;
        case 1: oi = P.old_to_new_node; break;
        case 2: oi = P.new_to_old_node; break;
        case 3: oi = P.old_to_new_edge; break;
        case 4: oi = P.new_to_old_edge; break;
        case 5: for (const RewriteEdge& r : P.rec) oi.insert(oi.end(), {r.from_new, r.to_new, r.xf_from, r.xf_to}); break;
        case 6: for (const InEdge& ed : P.in_edges) oi.insert(oi.end(), {ed.from, ed.to, (int32_t)ed.odom, (int32_t)ed.valid}); break;
        default: break;
        }
        const void* src = what == 7 ? (const void*)P.fixed_in.data() : (const void*)oi.data();
        const int64_t bytes = what == 7 ? (int64_t)P.fixed_in.size() : (int64_t)oi.size() * 4;
        if (out && bytes) {
            if (*nbytes < bytes) return UZL_ERR_BAD_ARG;
            memcpy(out, src, (size_t)bytes);
        }
        *nbytes = bytes;
        return UZL_OK;
    } catch (const std::bad_alloc&) {
        return UZL_ERR_OOM;
    }
}
#endif
