// scanmerge_types.hpp — POD shared by scanmerge_kernels.hip and uzl_scanmerge.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kScanMergeBlock = 256;       // one workgroup per pair
constexpr int kScanMergeMinBeams = 8;
constexpr int kScanMergeMaxBeams = 4096;   // a key is bin << 12 | beam
constexpr int kScanMergeKeyShift = 12;

// One scan of a pair as the kernel reads it.
struct ScanMergeScanRec {
    int64_t ranges_off, intensities_off;   // first reading in the call's value area
    int64_t trig_off;                      // first (cos, sin) of its table (n + 1 entries)
    int32_t n;
    float amin, inc;                       // for the first guess of a bin only (keep scan)
    float range_min, range_max;
    float D[6];                            // (float)D: rows x and y of [R | t] without the z column: r00 r01 tx r10 r11 ty
    int32_t _pad;
};

struct ScanMergePairRec {
    ScanMergeScanRec a, b;                 // keep, drop
    int64_t out_off;                       // first merged reading of the pair (n_a of them)
    int32_t b_newer;                       // b.stamp_ns > a.stamp_ns
    int32_t _pad;
};

struct ScanMergeArgs {
    const float* values;                   // every scan's ranges and intensities
    const double2* trig;
    const ScanMergePairRec* pairs;
    float* ranges;                         // merged, pair after pair
    float* intensities;
    double* centers;                       // 3 per pair
    // stage launch (one workgroup, pair `stage_pair`, list `stage_which`): per beam of the list the bin and rho; nothing else is written
    int32_t stage_pair, stage_which;
    int32_t* st_bin;
    float* st_rho;
};

void launch_scanmerge(const ScanMergeArgs& a, int n_pairs, hipStream_t s);

}  // namespace uzl
