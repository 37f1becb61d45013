// laser_bins.hpp — the bin of a point on a laser-line angular grid (contract: include/uzl_mi355x.h, "Laser line from depth
// images", step 6), shared by laserline_kernels.hip (pixels into bins) and scanmerge_kernels.hip (re-projected beams into bins).
// trig = (c_k, s_k) for k = 0..n, the grid's table from the host's libm.
#pragma once
#include <hip/hip_runtime.h>

namespace uzl {

// contract step 6: boundary t = (c_k, s_k) holds the point
__device__ inline bool holds(const double2 t, double X, double Y) { return (t.x * X + t.y * Y > 0.0) && (t.x * Y >= t.y * X); }

__device__ inline bool candidate(const double2* trig, int k, double X, double Y) { return holds(trig[k], X, Y) && !holds(trig[k + 1], X, Y); }

// step 6 as it is written: every boundary tested; -1 = dropped
__device__ inline int bin_by_definition(const double2* trig, int n, double X, double Y)
{
    int first = -1, last = -1;
    bool here = holds(trig[0], X, Y);
    for (int k = 0; k < n; k++) {
        const bool next = holds(trig[k + 1], X, Y);
        if (here && !next && first < 0) first = k;
        if (here) last = k;
        here = next;
    }
    return Y < 0.0 ? first : last;
}

// The same bin from a guess.  Away from the seam the boundaries that hold a point are one run of k, and the bin is where the run
// ends: an atan2f guess is at most one bin off it.  At the seam the run wraps: bins 0 and n - 1 settle it between them as step 6
// says.  Whatever the guess misses goes through the definition.
__device__ inline int bin_of(const double2* trig, int n, double X, double Y, float qx, float qy, float amin, float inc)
{
    if (X == 0.0 && Y == 0.0) return -1;
    if (!(isfinite(X) && isfinite(Y))) return bin_by_definition(trig, n, X, Y);
    const bool below = Y < 0.0;
    int k = (int)((atan2f(qy, qx) - amin) / inc);
    k = min(max(k, 0), n - 1);
    // on or above the x axis boundary n does not count: bin n - 1 ends the run if it holds
    if (!below && holds(trig[n - 1], X, Y)) return n - 1;
    int c;
    if (candidate(trig, k, X, Y)) c = k;
    else if (k + 1 < n && candidate(trig, k + 1, X, Y)) c = k + 1;
    else if (k > 0 && candidate(trig, k - 1, X, Y)) c = k - 1;
    else return bin_by_definition(trig, n, X, Y);
    if (c == n - 1 && below && candidate(trig, 0, X, Y)) c = 0;
    return c;
}

}  // namespace uzl
