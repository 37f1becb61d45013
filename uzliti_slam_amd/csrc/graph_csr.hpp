// graph_csr.hpp — the host-side edge list of the handles that walk the pose graph (uzl_scope.hip, uzl_merge.hip) and the CSR built
// from it: integer work, redone only when edges or flags change.
#pragma once
#include <cstdint>
#include <vector>

namespace uzl {

struct GraphEdge { int32_t from, to, type, valid; };

// The CSR of the edges `walked` admits, both directions, a self-loop once.  A node's row holds its edges in ascending edge index
// (std::set<std::string> node.edges_ of the reference).  row_ptr [n + 1]; col [max(m, 1)] the other end of a slot; row (may be null)
// the node a slot belongs to.  Returns m, the number of slots.
template <typename Walked>
int32_t build_csr(int32_t n, const std::vector<GraphEdge>& edges, Walked&& walked, std::vector<int32_t>& row_ptr, std::vector<int32_t>* row,
                  std::vector<int32_t>& col)
{
    row_ptr.assign((size_t)n + 1, 0);
    for (const auto& e : edges) {
        if (!walked(e)) continue;
        row_ptr[(size_t)e.from + 1]++;
        if (e.to != e.from) row_ptr[(size_t)e.to + 1]++;
    }
    for (int32_t v = 0; v < n; v++) row_ptr[(size_t)v + 1] += row_ptr[v];
    const int32_t m = row_ptr[n];
    col.assign((size_t)(m > 0 ? m : 1), 0);
    if (row) row->assign(col.size(), 0);
    std::vector<int32_t> fill(row_ptr.begin(), row_ptr.end() - 1);
    for (const auto& e : edges) {
        if (!walked(e)) continue;
        int32_t k = fill[e.from]++; col[k] = e.to; if (row) (*row)[k] = e.from;
        if (e.to != e.from) { k = fill[e.to]++; col[k] = e.from; if (row) (*row)[k] = e.to; }
    }
    return m;
}

}  // namespace uzl
