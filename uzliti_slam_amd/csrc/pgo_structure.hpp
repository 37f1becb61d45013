// pgo_structure.hpp — the structure of a pose graph as host-side values: the system edges the skip rules leave, the gauge, the order of
// the free vertices, the block system every later plan and every kernel is indexed by (block-CSR, slot records' metadata, the Hessian
// kernel's row blocks, row headers), and the small decisions around it - which numbering the reduced system takes, whether a Schur plan
// is adopted, a rank's share of the edges, the layout of the per-iteration exchange buffer, whether a new graph is the previous one
// grown.  Pure integer work (the edge weights are only compared): no handle, no HIP call, no environment, deterministic.  A structure is
// made in three steps, each "plan -> upload -> bind" (uzl_pgo.hip: build_structure): system_plan -> schur_plan (pgo_schur.hpp) -> ml_plan
// (pgo_ml_plan.hpp).  tests/test_pgo_structure_plan.py holds every rule on the CPU through uzl_debug_pgo_structure_plan.
#pragma once
#include "pgo_types.hpp"
#include "pgo_ml_plan.hpp"

#include <cstddef>
#include <vector>

namespace uzl {
// what the skip rules need of every INPUT edge of uzl_pgo_add_graph (kept so that uzl_pgo_append_graph can grow the graph in place)
struct InEdge { int32_t from, to; uint8_t odom, valid; double w; };
// the system edges: 2 endpoints per edge, system edge -> input edge, Huber flag, trace of the information matrix
struct FlatEdges {
    std::vector<int32_t> ij, src;
    std::vector<uint8_t> robust;
    std::vector<double> edge_w;
};
// the skip rules of addGraphImpl: odometry edges are added while iterating (:78-79), filtered feature edges after (:100-103)
FlatEdges flatten_edges(int n, const std::vector<InEdge>& in_edges, const std::vector<uint8_t>& fixed_in);
// G2: setFixedNodes (g2o_optimizer.cpp:301-349) on fixed_eff in place; returns how many vertices it fixed
int32_t gauge_fix(int n, const std::vector<int32_t>& ij, std::vector<uint8_t>& fixed_eff);
// order of the free vertices in the block system (b2v); edge_w of another size than the edges: every edge weighs 1
std::vector<int32_t> aggregation_order(int n, const std::vector<int32_t>& ij, const std::vector<uint8_t>& fixed_eff, const std::vector<double>& edge_w);

// block-CSR over the free vertices in the order b2v: one slot per (free endpoint, system edge), in edge order within a row
struct SystemPlan {
    int32_t nb = 0, nslots = 0;
    std::vector<int32_t> b2v, v2b;                 // [nb] block row -> vertex; [max(n, 1)] vertex -> block row, -1: fixed
    std::vector<int32_t> row_ptr, col, slot_edge;  // col: -1 = the neighbour is fixed; slot_edge: 2 * edge + (1: the row is the edge's second endpoint)
    std::vector<int32_t> smeta;                    // [nslots][4] = {slot_edge, i, j, (partner slot + 1) | robust << 30}: what slot_records / the Hessian kernel read
    std::vector<int32_t> rb_ptr;                   // row blocks of the Hessian build (row_blocks)
    std::vector<int32_t> rowhdr;                   // row_headers
};
SystemPlan system_plan(int n, const std::vector<int32_t>& ij, const std::vector<uint8_t>& robust, std::vector<int32_t> b2v);
// Row blocks of the Hessian build: consecutive rows with <= 256 slots and <= 42 rows, so that a workgroup makes one pass (a row with
// more slots is a block of its own and loops); beyond kMaxPartials blocks (> ~1M slots) blocks hold more and loop as well.
// caps (may be null): {cap_slots, cap_rows}
std::vector<int32_t> row_blocks(int nb, const std::vector<int32_t>& row_ptr, int32_t* caps = nullptr);
// [max(nb, 1)][kRowHdr] = {row_ptr[a], row_ptr[a + 1], col of the first 20 slots (-1 past the end), pad}: of the full and of the reduced system
std::vector<int32_t> row_headers(int nb, const std::vector<int32_t>& row_ptr, const std::vector<int32_t>& col);
// per slot, the weight of its edge (edge_w: one per system edge): what the strong grouping of schur_plan weighs
std::vector<double> slot_weights(const SystemPlan& Y, const std::vector<double>& edge_w);
// the reduced system's rows as vertices (-1: an empty row of the strong-aggregate numbering)
std::vector<int32_t> reduced_b2v(const std::vector<int32_t>& sep_rows, const std::vector<int32_t>& b2v);

constexpr int kSchurStrongMin = 32;                   // separators from which on the reduced system is numbered by strong aggregates
constexpr int kSchurMinPct = 33;                      // reduced when at least this share of the free vertices goes
// Which numbering the reduced system takes (uzl_pgo_cfg::reduced_numbering): strong_min = 0 is the row order; max_contig: the share of
// separators whose strong group is a run of consecutive separators anyway, above which schur_plan keeps the row order.
// num_its[2]: PCG iterations per LM trial of the handle's last solve in row order / by strong aggregates, < 0: none yet.
struct ReducedNumbering { int strong_min; double max_contig; };
ReducedNumbering reduced_numbering(int cfg_numbering, int preconditioner, bool may_shard, const double num_its[2]);
// a Schur plan is adopted when >= 64 rows and >= kSchurMinPct of the rows go; min_interiors: what schur_plan is told, so that it stops early otherwise
int schur_min_interiors(int nb);
bool schur_admitted(int nb, int n_int);

// sharded solve (BASELINE config 4): this rank linearises a contiguous range of the system edges; the diagonal's lambda is rank 0's
struct ShardRange { int32_t e_begin, e_end, diag_owner; };
ShardRange shard_range(int e, int rank, int world);
// per-iteration exchange buffer inside the PCG system's `ap`: [A p (6 nbp) | restricted A p (6 n_g) | p.Ap partials], offsets in doubles
struct ExchangeLayout { size_t sg, part_a; int64_t iter_span; };
ExchangeLayout exchange_layout(int nbp, const MlPlan& P);

// Is the new graph the previous one, unchanged or GROWN: at least as many nodes, the old nodes' fixed flags in front, and the old system
// edges still there in their order (edges_survive_in_order)?  window: how far ahead a surviving edge may have moved.
bool edges_survive_in_order(const std::vector<int32_t>& old_ij, const std::vector<int32_t>& new_ij, size_t window = 4096);
bool graph_grown(int n_old, const std::vector<uint8_t>& old_fixed, const std::vector<int32_t>& old_ij, int n_new, const std::vector<uint8_t>& new_fixed,
                 const std::vector<int32_t>& new_ij, size_t window = 4096);

// The resident graph SHRUNK in place (uzl_pgo_rewrite_graph): nodes leave, edges are deleted, retargeted or take a left multiplier on
// one side's displacement; what survives closes up in its order.  The rewrite as the caller states it (the fields of uzl_pgo_rewrite,
// minus the values: which multiplier and which pose are indices here) ...
struct RewriteOp { int32_t edge, action, xf, node; };          // uzl_pgo_edge_op
struct RewriteIn {
    std::vector<int32_t> drop_nodes, pose_nodes;
    int32_t n_xf = 0;
    std::vector<RewriteOp> ops;
};
// ... and what it does to a graph of n nodes with these input edges.  why != nullptr: the rewrite is refused (nothing else is filled).
// An edge goes if it has a DELETE op or if, after its ops, it still names a dropped node; endpoints outside [0, n) stay as they are.
struct RewriteEdge { int32_t from_new, to_new, xf_from, xf_to; };      // per surviving edge: its endpoints in the new numbering, the multiplier of either side (-1: untouched)
struct RewritePlan {
    const char* why = nullptr;
    std::vector<int32_t> old_to_new_node, new_to_old_node;     // -1: dropped
    std::vector<int32_t> old_to_new_edge, new_to_old_edge;     // -1: deleted
    std::vector<RewriteEdge> rec;                              // [surviving edges]
    std::vector<InEdge> in_edges;                              // the new graph's, for flatten_edges
    std::vector<uint8_t> fixed_in;
};
RewritePlan rewrite_plan(int n, const std::vector<InEdge>& in_edges, const std::vector<uint8_t>& fixed_in, const RewriteIn& rw);
}  // namespace uzl
