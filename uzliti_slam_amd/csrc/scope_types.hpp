// scope_types.hpp — POD shared by scope_kernels.hip and uzl_scope.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

// The LDS bound: graphs of up to this many nodes keep their distances (8 B each, 128 KiB) and both frontier bitmaps (2 x 2 KiB) in
// the 160 KiB LDS of the one CU the pass runs on; above it both live in global memory (L2-resident).
constexpr int kScopeLdsNodes = 16384;
constexpr int kScopeBlk = 1024;                 // lanes of the one workgroup of scope_sssp_kernel
constexpr int kScopeLaneDeg = 3;                // a frontier node of at most this degree is relaxed by its own lane (one dependent load and atomic after the other), a larger one by the lanes of its wave at once
constexpr double kScopeBucketEdges = 4.;        // a round serves the frontier nodes within this many mean edge lengths of the frontier's minimum
constexpr unsigned long long kScopeInf = 0x7fefffffffffffffull;     // DBL_MAX: distance_ of a node not reached
constexpr int kScanBlk = 256;                   // lanes of a workgroup of scope_scan_kernel
constexpr int kScanSlab = kScanBlk * 8;         // nodes one workgroup streams

// What a lane needs of a node it has just improved, in one 32-byte load: its CSR row, and for a node of degree 2 both neighbours
// with the lengths of the edges to them (written by the pass itself from the current positions).
struct ScopeRec { int32_t first, deg, a, b; double wa, wb; };

// What a pass brings back to the host.
struct ScopeResult { long long rounds, relaxations, n_reached, pad; };

struct ScopeArgs {
    int32_t n, m;                       // nodes, CSR slots (two per participating edge, one for a self-loop)
    int32_t source;                     // node 0, or oldestReachableNode(id)
    int32_t add_initial;                // reevaluateUncertainty(id): uncertainty_ = uncertainty_[source] + distance_
    const double* x; const double* y; const double* z;
    const int32_t* row_ptr;             // [n + 1]
    const int32_t* row;                 // [m] the node a slot belongs to
    const int32_t* col;                 // [m] its neighbour
    double* w;                          // [m] edge lengths of this pass
    ScopeRec* rec;                      // [n]
    unsigned long long* dist;           // [n] distance_ as bit patterns: the pass's result, and its working set above the LDS bound
    uint32_t* front;                    // [2][(n + 31) / 32] frontier bitmaps above the LDS bound
    double* unc;                        // [n] uncertainty_
    ScopeResult* result;
};

struct ScopeScanArgs {
    int32_t n;
    int32_t current;                    // request: the centre is this node and the radius comes from its uncertainty_; select: -1
    const double* x; const double* y; const double* z;
    const double* unc;
    double cx, cy, cz, radius;          // select
    double scope_size_min, scope_size_factor, out_margin;       // request
    const uint32_t* have;               // select: bitmap of the nodes the requester holds
    int32_t* count;                     // [workgroups] hits of each slab
    int32_t* out;                       // [cap] hits in index order
    int32_t cap;
    double* radius_out;                 // request: current_scope_
    int32_t* total;
};

void launch_scope_sssp(const ScopeArgs& a, hipStream_t s);
void launch_scope_scan(const ScopeScanArgs& a, hipStream_t s);       // the count pass, then the write pass
void launch_scope_pgo_poses(const double* pose8, int32_t n, double* x, double* y, double* z, hipStream_t s);
// uzl_pgo.hip: the solver's current translations into x / y / z (device, n each) on stream s, waited for; UZL_ERR_STATE without a
// graph, UZL_ERR_BAD_ARG for another device or node count; throws HipError
int pgo_positions_to(uzl_pgo* solver, int32_t device, int32_t n, double* x, double* y, double* z, hipStream_t s);

}  // namespace uzl
