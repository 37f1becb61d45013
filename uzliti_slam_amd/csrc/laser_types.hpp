// laser_types.hpp — POD shared by laser_kernels.hip and uzl_laser.hip (and uzl_laserline.hip's way into the scan store)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kIcpBlock = 256;            // one workgroup per pair; lane t owns beams t, t + 256, ... of `to`
constexpr int kIcpWaves = kIcpBlock / 64;
constexpr int kIcpMinBeams = 8;
constexpr int kIcpMaxBeams = 4096;        // j1 and j2 share one 32-bit word (12 bits each), LDS holds one scan's points
constexpr int kIcpSums = 15;              // M (10), v (4), sum w b^2
constexpr int kIcpBisections = 64;        // contract step 6: halvings of [lo, lo + |h|]

// One stored scan.
struct LaserScanRec {
    int64_t values_off, trig_off;         // into the values and (cos, sin) arenas
    int32_t n;
    float range_min, range_max;
    int32_t _pad;
};

// One pair as the kernel reads it: the first guess with its rotation as (c, s) from the host's libm.
struct LaserPairRec {
    int32_t from, to;
    double tx, ty, c, s;
};

// What the kernel leaves per pair; the host makes a uzl_laser_edge of it (theta, information, step 10).
struct LaserPairOut {
    double tx, ty, c, s;
    double H[6];                          // Gauss-Newton Hessian in (x, y, theta): 00 01 02 11 12 22
    double error;
    int32_t status, nvalid, scan_valid, deg_count, iterations, _pad;
};

struct LaserIcpArgs {
    const float* values;
    const double2* trig;
    const LaserScanRec* scans;
    const LaserPairRec* pairs;
    LaserPairOut* out;
    double max_corr_sq, max_perc, adaptive_order, adaptive_mult, fail_fraction, eps_xy_sq, sin_eps_theta;
    int32_t max_iterations;
    int32_t stage;                        // 1: steps 2-4 once at the pair's estimate, written to st_* (one pair)
    int32_t max_from, max_to;             // the largest beam counts among the call's pairs: they place the LDS arrays
    int32_t* st_j1;
    int32_t* st_j2;
    int32_t* st_valid;
    double* st_dist;
};

// LDS of one workgroup: from's points (double2), the smallest squared distance per from beam (u64 bits), then per to beam the
// packed correspondence (i32) and its distance (f64); the reductions' 4 x 15 partial sums and a few words are static.
inline size_t laser_icp_lds(int32_t max_from, int32_t max_to)
{
    return (size_t)max_from * (sizeof(double2) + sizeof(unsigned long long)) + (size_t)max_to * (sizeof(double) + sizeof(int32_t));
}

void laser_icp_prepare();                 // on the current device: allows the kernel its largest LDS request (144 KiB at 4096 beams)
void launch_laser_icp(const LaserIcpArgs& a, int n_pairs, hipStream_t s);

// uzl_laserline_to_laser's way into the store: n_scans scans of n_beams values each, contiguous in the memory of `device` and
// complete, appended as uzl_laser_add_scans appends them.
int laser_append_device(uzl_laser* h, int device, int32_t n_scans, int32_t n_beams, const float* d_values, float angle_min,
                        float angle_increment, float range_min, float range_max, int32_t* first_scan);
// The same for scans that differ in beam count, grid or limits (uzl_scanmerge_to_laser): scan i has scans[i].n values, and the
// scans lie one after the other at d_values.  One device-to-device copy; the same checks, messages and lock.
struct DeviceScan;
int laser_append_device_scans(uzl_laser* h, int device, int32_t n_scans, const DeviceScan* scans, const float* d_values,
                              int32_t* first_scan);

}  // namespace uzl
