// gist_types.hpp — POD shared by gist_kernels.hip and uzl_gist.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kGistBlock = 256;       // one workgroup per query
constexpr int kGistMaxK = 256;        // k_nearest_neighbors range (the reference's cfg allows 0-100)
constexpr int kGistMaxBytes = 256;    // descriptor bytes; the histogram then spans distances 0..2048
constexpr int kGistMaxBins = 8 * kGistMaxBytes + 1;

// One launch = n queries.  Query q sees the places [0, base + q): base = places before the batch, so batch node q searches the
// earlier places plus batch nodes 0..q-1, exactly as q successive single calls would.
struct GistKnnArgs {
    const uint8_t* store;       // [rows][stride] descriptors, zero-padded rows, stride a multiple of 16
    const uint8_t* live;        // [rows] 1 = indexed and not removed
    const uint8_t* queries;     // [n][stride]
    const uint8_t* qvalid;      // [n] 0 = the node has no GIST sensor (no search); nullptr = all valid
    int32_t stride;
    int32_t base;
    int32_t k;                  // 1..kGistMaxK
    int32_t dmax;               // min(floor(T), 8 * bytes), >= 0
    int2* out;                  // [n][k] (place, distance), ascending (distance, place)
    int32_t* out_n;             // [n]
};

void launch_gist_knn(const GistKnnArgs& a, int n, hipStream_t s);

}  // namespace uzl
