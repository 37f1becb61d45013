// grid_kernels.hip — occupancy-grid projection on gfx950 (contract: include/uzl_mi355x.h, "Occupancy-grid map").
//
// grid_tile_kernel: one 1024-thread workgroup per non-empty 128 x 128-cell tile.  The tile's hits and passes live in LDS (2 x 64 KiB)
// for the whole kernel: known-free squares (ds_max_u32), then every ray of the scans binned to the tile, each entering at its first
// step inside the tile (grid_ray_clip) and counting with ds_add_u32, then one pass that stores the counts and the classified cells.
// No global atomic touches a cell; the one global atomic per workgroup adds its hit total.  Built with -ffp-contract=off: the beam
// arithmetic rounds after every operation, as the contract says.
#include "grid_types.hpp"

namespace uzl {

namespace {

__device__ inline int32_t cell_of(double v, double origin, double res) { return (int32_t)floor((v - origin) / res); }

__global__ __launch_bounds__(kGridBlock) void grid_tile_kernel(GridTileArgs a)
{
    __shared__ uint32_t s_hits[kGridTile * kGridTile];
    __shared__ uint32_t s_pass[kGridTile * kGridTile];
    __shared__ unsigned int s_hit_total;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int tile = a.tiles[b];
    const int32_t tx0 = (tile % a.tiles_x) * kGridTile, ty0 = (tile / a.tiles_x) * kGridTile;
    const int32_t tw = min(kGridTile, a.width - tx0), th = min(kGridTile, a.height - ty0);
    const int32_t tx1 = tx0 + tw - 1, ty1 = ty0 + th - 1;

    if (tid == 0) s_hit_total = 0;
    for (int i = tid; i < kGridTile * kGridTile; i += kGridBlock) {
        const int ly = i / kGridTile, lx = i % kGridTile;
        uint32_t h = 0, p = 0;
        if (!a.fresh && lx < tw && ly < th) {
            const size_t g = (size_t)(ty0 + ly) * (size_t)a.width + (size_t)(tx0 + lx);
            h = a.hits[g]; p = a.passes[g];
        }
        s_hits[i] = h; s_pass[i] = p;
    }
    __syncthreads();

    // step 2: known-free squares of the nodes this call adds, before any ray
    if (a.min_pass_through > 0) {
        const uint32_t mpt = (uint32_t)a.min_pass_through;
        for (int e = a.kf_start[b]; e < a.kf_start[b + 1]; e++) {
            const int4 r = a.kf_rect[e];
            const int32_t x0 = max(r.x, tx0), y0 = max(r.y, ty0), x1 = min(r.z, tx1), y1 = min(r.w, ty1);
            if (x0 > x1 || y0 > y1) continue;
            const int32_t nx = x1 - x0 + 1, nc = nx * (y1 - y0 + 1);
            for (int j = tid; j < nc; j += kGridBlock) {
                const int32_t x = x0 + j % nx, y = y0 + j / nx;
                atomicMax(&s_pass[(y - ty0) * kGridTile + (x - tx0)], mpt);
            }
        }
    }
    __syncthreads();

    // steps 3-5: beam i of the tile's list = beam i - ent_beam[e] of scan ent_scan[e]; each thread walks its entry index forward
    const int e0 = a.ent_start[b], e1 = a.ent_start[b + 1];
    if (e1 > e0) {
        const int64_t nb = a.ent_beam[e1 - 1] + a.scans[a.ent_scan[e1 - 1]].n;
        int e = e0;
        unsigned int my_hits = 0;
        for (int64_t i = tid; i < nb; i += kGridBlock) {
            while (e + 1 < e1 && a.ent_beam[e + 1] <= i) e++;
            const GridScanRec& s = a.scans[a.ent_scan[e]];
            const int64_t bi = i - a.ent_beam[e];
            const double r = (double)a.ranges[s.ranges_off + bi];
            if (!((double)s.range_min <= r && r < a.range_max)) continue;
            const double2 cs = a.trig[s.trig_off + bi];
            const double px = (double)(float)(r * cs.x), py = (double)(float)(r * cs.y);
            double qx = (s.r00 * px + s.r01 * py) + s.tx;
            double qy = (s.r10 * px + s.r11 * py) + s.ty;
            const bool hit = r <= a.max_distance;
            if (!hit) {
                const double f = a.max_distance / r;
                qx = s.tx + f * (qx - s.tx);
                qy = s.ty + f * (qy - s.ty);
            }
            const int32_t ex = cell_of(qx, a.origin_x, a.resolution), ey = cell_of(qy, a.origin_y, a.resolution);
            grid_ray_clip(s.ocx, s.ocy, ex, ey, tx0, ty0, tx1, ty1,
                          [&](int32_t x, int32_t y) { atomicAdd(&s_pass[(y - ty0) * kGridTile + (x - tx0)], 1u); });
            if (hit && ex >= tx0 && ex <= tx1 && ey >= ty0 && ey <= ty1) {
                atomicAdd(&s_hits[(ey - ty0) * kGridTile + (ex - tx0)], 1u);
                my_hits++;
            }
        }
        if (my_hits) atomicAdd(&s_hit_total, my_hits);
    }
    __syncthreads();

    // step 6 and the stores: row-contiguous, one cell per lane
    for (int i = tid; i < kGridTile * kGridTile; i += kGridBlock) {
        const int ly = i / kGridTile, lx = i % kGridTile;
        if (lx >= tw || ly >= th) continue;
        const size_t g = (size_t)(ty0 + ly) * (size_t)a.width + (size_t)(tx0 + lx);
        const uint32_t h = s_hits[i], p = s_pass[i];
        a.hits[g] = h;
        a.passes[g] = p;
        a.grid[g] = (int64_t)p < (int64_t)a.min_pass_through ? (int8_t)-1
                    : ((double)h > a.occupancy_threshold * (double)p ? (int8_t)100 : (int8_t)0);
    }
    if (tid == 0 && s_hit_total) atomicAdd(a.hit_total, (unsigned long long)s_hit_total);
}

// valid beams (step 3) of each projected scan, whether or not its rays reach the grid
__global__ __launch_bounds__(kGridStatsBlock) void grid_stats_kernel(GridStatsArgs a)
{
    __shared__ unsigned int s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const GridScanRec& s = a.scans[blockIdx.x];
    unsigned int c = 0;
    for (int i = threadIdx.x; i < s.n; i += kGridStatsBlock) {
        const double r = (double)a.ranges[s.ranges_off + i];
        c += ((double)s.range_min <= r && r < a.range_max) ? 1u : 0u;
    }
    if (c) atomicAdd(&s_n, c);
    __syncthreads();
    if (threadIdx.x == 0 && s_n) atomicAdd(a.valid_total, (unsigned long long)s_n);
}

}  // namespace

void launch_grid_tiles(const GridTileArgs& a, int n_tiles, hipStream_t s)
{
    if (n_tiles > 0) hipLaunchKernelGGL(grid_tile_kernel, dim3(n_tiles), dim3(kGridBlock), 0, s, a);
}

void launch_grid_stats(const GridStatsArgs& a, int n_scans, hipStream_t s)
{
    if (n_scans > 0) hipLaunchKernelGGL(grid_stats_kernel, dim3(n_scans), dim3(kGridStatsBlock), 0, s, a);
}

}  // namespace uzl
