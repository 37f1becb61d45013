// merge_types.hpp — POD shared by merge_kernels.hip and uzl_merge.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

// The one bound of the one path.  A wave of merge_walk_kernel owns a visited bitmap of one bit per node in LDS, and a workgroup's
// bitmaps must fit the 160 KiB of a CU beside nothing else (the stack of a walk lives in registers, one frame per lane):
//     kMergeWaves (4) x kMergeBitmapBytes (32 KiB) = 128 KiB <= 160 KiB,   32 KiB x 8 bits = 262,144 nodes.
// A launch asks for the bitmaps of the graph it has, (n + 31) / 32 words a wave, so small graphs leave room for more workgroups
// on a CU.  Above the bound uzl_merge_set_graph refuses; there is no second path.
constexpr int kMergeWaves = 4;                          // waves of a workgroup of merge_walk_kernel, one start each at a time
constexpr int kMergeBitmapBytes = 32 * 1024;
constexpr int kMergeMaxNodes = kMergeBitmapBytes * 8;   // = uzl_merge_max_nodes()
static_assert(kMergeWaves * kMergeBitmapBytes <= 160 * 1024, "the bitmaps of a workgroup must fit the LDS of a CU");
static_assert(UZL_MERGE_MAX_HOPS <= 64, "the stack of a walk is one frame per lane of a wave");
constexpr int kMergeWalkBlk = kMergeWaves * 64;
constexpr int kMergeWalkGroups = 1024;                  // workgroups of a walk launch at most (4 a CU): the waves stride over the starts
constexpr int kMergeNearBlk = 256;                      // lanes of a workgroup of merge_near_kernel = nodes of its LDS tile
constexpr int kMergeTickBlk = 1024;                     // lanes of the one workgroup of merge_tick_kernel

// What a tick brings back to the host in one 16-byte read.
struct MergeResult { int32_t keep, drop, next_index, pad; };

struct MergeArgs {
    int32_t n;
    int32_t first;                      // starts below this index are not looked at (0: the whole table)
    int32_t max_hops;
    int32_t pad;
    double cx, cy, cz;                  // last_scope_center_
    double start_bound;                 // last_scope_radius_ + scope_margin
    double max_distance;
    double trace_bound;                 // 1 + 2 cos(max_rotation_deg)
    const double* pose12;               // [n][12] row-major [R|t]
    const double* x; const double* y; const double* z;     // [n] the translations, SoA
    const int32_t* row_ptr;             // [n + 1]
    const int32_t* col;                 // [m] a node's row: the other ends of its valid edges in ascending edge index
    int32_t* partner;                   // [n]
    int32_t* starts;                    // [n] the flagged starts, in no particular order
    int32_t* n_starts;                  // [1]
    unsigned long long* visited;        // [1] nodes the walks of this launch marked
    MergeResult* result;
};

void launch_merge_split(const double* pose12, int32_t n, double* x, double* y, double* z, hipStream_t s);
void launch_merge_near(const MergeArgs& a, hipStream_t s);          // clears partner / n_starts / visited, then flags the starts
hipError_t launch_merge_walk(const MergeArgs& a, hipStream_t s);         // an error: the LDS of the bitmaps could not be had
void launch_merge_tick(const MergeArgs& a, hipStream_t s);
// uzl_pgo.hip: the solver's current estimates as n x 12 [R|t] into out12 (device), by the kernel its own pose read-back runs, on
// stream s, waited for; UZL_ERR_STATE without a graph, UZL_ERR_BAD_ARG for another device or node count; throws HipError
int pgo_poses12_to(uzl_pgo* solver, int32_t device, int32_t n, double* out12, hipStream_t s);

}  // namespace uzl
