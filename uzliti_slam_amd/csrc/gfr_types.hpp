// gfr_types.hpp — POD shared by gfr_kernels.hip and uzl_gfr.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kGfrMaxBytes = 64;        // descriptor bytes (rows of 1-4 uint4 in the store)
constexpr int kGfrMaxRows = 4096;       // rows of one node
constexpr int kGfrMaxK = 256;           // k_nearest_neighbors range, as uzl_gist_*
constexpr int kGfrMaxDistance = 512;    // max_distance range: 8 * kGfrMaxBytes
constexpr int kGfrTileBits = 9;
constexpr int kGfrTile = 1 << kGfrTileBits;   // features staged in LDS at a time (32 KB at 64 bytes per row)
constexpr int kGfrMaxBlock = 512;       // lanes (= query rows) of one workgroup of gfr_nearest_kernel
constexpr int kGfrMaxGridX = 1024;      // workgroups along the repository; each strides over the tiles
constexpr int kGfrBlock = 256;          // the three small kernels
constexpr unsigned long long kGfrNoKey = ~0ull;

// One arena entry of a feature's link chain: the next entry of the same feature (-1 = end) and the place that saw the feature.
struct GfrLink { int32_t next, place; };

// What one call brings back to the host: a fixed head, then the candidates in place order.
struct GfrResult { int32_t n_cand, n_features, n_links, pad; };

struct GfrArgs {
    const uint4* rows_d;            // [rows][chunks] the node's descriptors, zero-padded to 16 bytes
    int32_t rows, chunks, bytes;
    int32_t F, L;                   // features / link entries before this node
    int32_t max_distance;
    int32_t place;                  // the index this node takes (integration)
    int32_t n_votes;                // place_count + 1
    int32_t min_votes;              // max(1, ceil(T))
    uint4* store;                   // [capacity][chunks]
    int32_t* head;                  // [capacity] first arena entry of the feature's chain
    GfrLink* link;                  // [link capacity]
    unsigned long long* key;        // [rows] (distance << 32 | feature) of the nearest feature, kGfrNoKey when F == 0
    int32_t* votes;                 // [n_votes]
    GfrResult* result;              // head, followed by int2 (place, votes) x n_cand
};

void launch_gfr_nearest(const GfrArgs& a, hipStream_t s);
void launch_gfr_vote(const GfrArgs& a, hipStream_t s);
void launch_gfr_select(const GfrArgs& a, hipStream_t s);
void launch_gfr_integrate(const GfrArgs& a, hipStream_t s);

}  // namespace uzl
