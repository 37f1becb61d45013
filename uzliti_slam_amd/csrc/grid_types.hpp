// grid_types.hpp — POD shared by grid_kernels.hip and uzl_grid.hip
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/uzl_mi355x.h"

namespace uzl {

constexpr int kGridTile = 128;        // cells per tile side: hits + passes of one tile are 128 KiB of LDS
constexpr int kGridBlock = 1024;      // one workgroup per tile
constexpr int kGridStatsBlock = 256;  // one workgroup per scan (valid-beam count)

// One scan as a build projects it: S = P_node * D (the rows x, y of its rotation and its translation) and cell(o).
struct GridScanRec {
    double r00, r01, r10, r11, tx, ty;
    int64_t ranges_off;       // first range in the arena
    int64_t trig_off;         // first (cos, sin) of its table
    int32_t n;
    float range_min;
    int32_t ocx, ocy;         // cell of the sensor position o = S.t
};

// A build's work: tiles[b] is the tile of workgroup b; its rays are the beams of the scans ent_scan[ent_start[b] ..
// ent_start[b + 1]) (ent_beam = their exclusive prefix of beams, per tile), its known-free squares kf_rect[kf_start[b] ..
// kf_start[b + 1]) (x0, y0, x1, y1, inclusive, already clipped to the grid).
struct GridTileArgs {
    const float* ranges;
    const double2* trig;
    const GridScanRec* scans;
    const int32_t* tiles;
    const int32_t* ent_start;
    const int32_t* ent_scan;
    const int64_t* ent_beam;
    const int32_t* kf_start;
    const int4* kf_rect;
    uint32_t* hits;
    uint32_t* passes;
    int8_t* grid;
    unsigned long long* hit_total;
    double origin_x, origin_y, resolution, range_max, max_distance, occupancy_threshold;
    int32_t width, height, tiles_x;
    int32_t min_pass_through;
    int32_t fresh;            // 1: the tile starts from zero counts (full build), 0: from the stored ones (extend)
};

struct GridStatsArgs {
    const float* ranges;
    const GridScanRec* scans;
    double range_max;
    unsigned long long* valid_total;
};

void launch_grid_tiles(const GridTileArgs& a, int n_tiles, hipStream_t s);
void launch_grid_stats(const GridStatsArgs& a, int n_scans, hipStream_t s);

// Append scans that already lie in device memory to a grid handle's store (uzl_grid.hip; used by uzl_laserline_to_grid).  Takes the
// grid handle's lock; failures are reported through the grid handle's last_error.
int grid_append_device(uzl_grid* h, int device, int32_t n_scans, int32_t n_beams, const float* d_ranges, float angle_min,
                       float angle_increment, float range_min, const int32_t* nodes, int32_t* first_scan);
// The same for scans that differ in beam count, grid or range_min (uzl_scanmerge_to_grid): scan i has scans[i].n ranges, and the
// scans lie one after the other at d_ranges.  One device-to-device copy; the same checks, messages and lock.
struct DeviceScan;
int grid_append_device_scans(uzl_grid* h, int device, int32_t n_scans, const DeviceScan* scans, const float* d_ranges,
                             const int32_t* nodes, int32_t* first_scan);

// The part of the ray cell(o) = (x0, y0) -> (x1, y1) (steps 0..L of contract step 5) inside the cell rectangle [ux0, ux1] x
// [uy0, uy1]: calls visit(x, y) for exactly those cells, in walk order.  Bresenham's state after k steps in closed form: with
// L = max(|dx|, |dy|) and m = min, the major coordinate moves every step and the minor one has moved floor((2 m k + L) / (2 L))
// after k (the e2 >= dy / e2 <= dx rule of the contract gives exactly this, ties included).  The major clip and the minor clip
// (the minor offset never decreases) give the first and last step inside; the walk between them is incremental.
template <typename F>
__host__ __device__ inline void grid_ray_clip(int32_t x0, int32_t y0, int32_t x1, int32_t y1, int32_t ux0, int32_t uy0, int32_t ux1,
                                              int32_t uy1, F&& visit)
{
    const int32_t adx = x1 > x0 ? x1 - x0 : x0 - x1, ady = y1 > y0 ? y1 - y0 : y0 - y1;
    const int32_t sx = x1 >= x0 ? 1 : -1, sy = y1 >= y0 ? 1 : -1;
    const bool xmaj = adx >= ady;
    const int32_t L = xmaj ? adx : ady, m = xmaj ? ady : adx;
    const int32_t u0 = xmaj ? x0 : y0, v0 = xmaj ? y0 : x0, su = xmaj ? sx : sy, sv = xmaj ? sy : sx;
    const int32_t ulo = xmaj ? ux0 : uy0, uhi = xmaj ? ux1 : uy1, vlo = xmaj ? uy0 : ux0, vhi = xmaj ? uy1 : ux1;
    // steps with the major coordinate inside
    int64_t ka = su > 0 ? (int64_t)ulo - u0 : (int64_t)u0 - uhi;
    int64_t kb = su > 0 ? (int64_t)uhi - u0 : (int64_t)u0 - ulo;
    // minor offsets inside
    int64_t dlo = sv > 0 ? (int64_t)vlo - v0 : (int64_t)v0 - vhi;
    int64_t dhi = sv > 0 ? (int64_t)vhi - v0 : (int64_t)v0 - vlo;
    if (ka < 0) ka = 0;
    if (kb > L) kb = L;
    if (dlo < 0) dlo = 0;
    if (dhi > m) dhi = m;
    if (ka > kb || dlo > dhi) return;
    const int64_t twoL = 2 * (int64_t)L, twom = 2 * (int64_t)m;
    if (dlo > 0) {                          // first k with floor((2mk + L) / 2L) >= dlo  (m >= dlo > 0)
        const int64_t num = twoL * dlo - L, k = (num + twom - 1) / twom;
        if (k > ka) ka = k;
    }
    if (dhi < m) {                          // last k with floor((2mk + L) / 2L) <= dhi  (m > dhi >= 0)
        const int64_t num = twoL * (dhi + 1) - L, k = (num + twom - 1) / twom - 1;
        if (k < kb) kb = k;
    }
    if (ka > kb) return;
    if (L == 0) { visit(x0, y0); return; }
    const int64_t D = twom * ka + L;
    int32_t rem = (int32_t)(D % twoL);
    int32_t u = u0 + su * (int32_t)ka, v = v0 + sv * (int32_t)(D / twoL);
    const int32_t tL = (int32_t)twoL, tm = (int32_t)twom;
    for (int32_t k = (int32_t)ka; k <= (int32_t)kb; k++) {
        if (xmaj) visit(u, v); else visit(v, u);
        u += su;
        rem += tm;
        if (rem >= tL) { rem -= tL; v += sv; }
    }
}

}  // namespace uzl
