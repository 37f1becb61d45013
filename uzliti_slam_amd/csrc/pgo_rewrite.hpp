// pgo_rewrite.hpp — launchers of pgo_rewrite_kernels.hip: what uzl_pgo_rewrite_graph (uzl_pgo.hip) runs on the device once rewrite_plan
// (pgo_structure.hpp) has decided what survives.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "../../include/uzl_mi355x.h"

namespace uzl {
constexpr int kRwBlock = 256;                        // both kernels: 4 waves, i.e. 4 edges, or 64 nodes of 4 pieces
constexpr int kRwWordFrom = 15, kRwWordTo = 27;      // uzl_edge::displacement_from / _to as 8-byte words of the record (static_assert in the kernel file)
// out[k] = in[new_to_old[k]] with rec[k] = {from_new, to_new, xf_from, xf_to} applied (4 x int32 per edge, 16-byte aligned), k < e_new
// ev_a / ev_b (may be null): the dispatch's own timestamps, as KernelTimer::pair hands them out
void k_rewrite_edges(const uzl_edge* in, uzl_edge* out, const int32_t* new_to_old, const int32_t* rec, int e_new, const double* xf, hipStream_t s,
                     hipEvent_t ev_a = nullptr, hipEvent_t ev_b = nullptr);
// out[v] = src[v] >= 0 ? cur[src[v]] : placed[~src[v]], 8 doubles per node, v < n_new
void k_rewrite_nodes(const double* cur, const double* placed, const int32_t* src, int n_new, double* out, hipStream_t s, hipEvent_t ev_a = nullptr,
                     hipEvent_t ev_b = nullptr);
}  // namespace uzl
