// cloud_voxel.hip — steps 1-2 of the colour point-cloud contract on the device: the cloud of a depth and a colour image, and its
// voxel grid (include/uzl_mi355x.h).  A pixel's point is recomputed from its depth wherever it is needed, so nothing per pixel is
// kept but its key.  The order of a voxel's f32 sums is the ascending pixel index: the keys (image << 32 | voxel key) are sorted
// by rocPRIM's radix sort, which is stable, with the pixel indices as values; one thread per voxel then walks its run.  Nothing
// depends on the schedule: the bounding box is an integer min / max, the rest has one writer per value.
#include "cloud_types.hpp"

#include <cstring>
#include <rocprim/rocprim.hpp>

namespace uzl {
namespace {

constexpr uint32_t kDropped = 0xffffffffu;       // low word of the key of a pixel that gives no point (sorts behind the image's voxels)

__device__ inline uint32_t code(float f)         // order-preserving: a < b iff code(a) < code(b), for finite a, b
{
    const uint32_t b = __float_as_uint(f);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ inline float decode(uint32_t c) { return __uint_as_float((c >> 31) ? (c & 0x7fffffffu) : ~c); }

// step 1 and step 2's filter for pixel `local` of an image: false when it gives no point or the grid does not keep it
__device__ inline bool pixel_point(const CloudImageRec& r, int local, float z_min, float z_max, float& x, float& y, float& z)
{
    const int v = local / r.width, u = local - v * r.width;
    const uint8_t* row = r.depth + (size_t)v * r.depth_step;
    float d;
    if (r.encoding == UZL_DEPTH_U16_MM) d = (float)((double)reinterpret_cast<const uint16_t*>(row)[u] * 0.001);
    else d = reinterpret_cast<const float*>(row)[u];
    if (!(d > 0.f)) return false;                  // also NaN
    x = (float)((((double)u - r.cx) * (double)d) / r.fx);
    y = (float)((((double)v - r.cy) * (double)d) / r.fy);
    z = d;
    const float big = 3.4028234663852886e38f;
    if (!(fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big)) return false;
    return z >= z_min && z <= z_max;
}

__global__ __launch_bounds__(256) void cloud_bbox_kernel(const CloudImageRec* __restrict__ recs, uint32_t* __restrict__ bbox, float z_min,
                                                         float z_max)
{
    const CloudImageRec r = recs[blockIdx.y];
    const int n = r.width * r.height;
    if ((int)blockIdx.x * 256 >= n) return;
    const int local = blockIdx.x * 256 + threadIdx.x;
    float x, y, z;
    const bool ok = local < n && pixel_point(r, local, z_min, z_max, x, y, z);
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (ok) { lo[0] = hi[0] = code(x); lo[1] = hi[1] = code(y); lo[2] = hi[2] = code(z); }
#pragma unroll
    for (int a = 0; a < 3; a++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            lo[a] = min(lo[a], (uint32_t)__shfl_xor((int)lo[a], off));
            hi[a] = max(hi[a], (uint32_t)__shfl_xor((int)hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0 && lo[0] != 0xffffffffu) {
        uint32_t* b_lo = bbox + 3 * blockIdx.y;
        uint32_t* b_hi = bbox + 3 * (gridDim.y + blockIdx.y);
#pragma unroll
        for (int a = 0; a < 3; a++) { atomicMin(b_lo + a, lo[a]); atomicMax(b_hi + a, hi[a]); }
    }
}

// The grid of an image from its bounding box: min_b and the divisions per axis; false when no point is kept or dx dy dz overflows int32
// (*overflow says which).
__device__ inline bool voxel_grid(const uint32_t* b_lo, const uint32_t* b_hi, float inv, long long* min_b, long long* dim, bool* overflow)
{
    *overflow = false;
    if (b_lo[0] == 0xffffffffu) return false;
    double cells = 1.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double lo = (double)floorf(decode(b_lo[a]) * inv), hi = (double)floorf(decode(b_hi[a]) * inv);
        const double d = (hi - lo) + 1.0;
        cells = cells * d;
        if (!(d <= 2147483647.0)) { *overflow = true; return false; }
        min_b[a] = (long long)lo; dim[a] = (long long)d;
    }
    if (!(cells <= 2147483647.0)) { *overflow = true; return false; }
    return true;
}

__global__ __launch_bounds__(256) void cloud_key_kernel(const CloudImageRec* __restrict__ recs, const uint32_t* __restrict__ bbox,
                                                        int32_t* __restrict__ info, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                                        float leaf, float z_min, float z_max)
{
    const CloudImageRec r = recs[blockIdx.y];
    const int n = r.width * r.height;
    if ((int)blockIdx.x * 256 >= n) return;
    const int local = blockIdx.x * 256 + threadIdx.x;
    if (local >= n) return;
    const float inv = 1.0f / leaf;
    long long min_b[3], dim[3];
    bool overflow;
    const bool grid = voxel_grid(bbox + 3 * blockIdx.y, bbox + 3 * (gridDim.y + blockIdx.y), inv, min_b, dim, &overflow);
    if (local == 0) info[2 * blockIdx.y + 1] = overflow ? 1 : 0;
    float x, y, z;
    uint32_t key = kDropped;
    if (grid && pixel_point(r, local, z_min, z_max, x, y, z)) {
        const long long i = (long long)floorf(x * inv) - min_b[0], j = (long long)floorf(y * inv) - min_b[1],
                        k = (long long)floorf(z * inv) - min_b[2];
        key = (uint32_t)(i + j * dim[0] + k * dim[0] * dim[1]);
    }
    keys[r.pix_off + local] = ((uint64_t)blockIdx.y << 32) | key;
    vals[r.pix_off + local] = (uint32_t)(r.pix_off + local);
}

__global__ __launch_bounds__(256) void cloud_head_kernel(const uint64_t* __restrict__ keys, uint32_t* __restrict__ flag, int64_t n)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const uint64_t k = keys[s];
    flag[s] = ((uint32_t)k != kDropped && (s == 0 || keys[s - 1] != k)) ? 1u : 0u;
}

// voxel count of image i = the heads in its segment [pix_off, pix_off + pixels) of the sorted array
__global__ void cloud_count_kernel(const CloudImageRec* __restrict__ recs, int32_t n_images, int64_t n_pixels, const uint32_t* __restrict__ flag,
                                   const uint32_t* __restrict__ rank, int32_t* __restrict__ info)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_images) return;
    const int64_t a = recs[i].pix_off, b = a + (int64_t)recs[i].width * recs[i].height;
    const uint32_t total = n_pixels > 0 ? rank[n_pixels - 1] + flag[n_pixels - 1] : 0u;
    const uint32_t ra = a < n_pixels ? rank[a] : total, rb = b < n_pixels ? rank[b] : total;
    info[2 * i] = (int32_t)(rb - ra);
}

__global__ __launch_bounds__(256) void cloud_voxel_kernel(const CloudImageRec* __restrict__ recs, const uint64_t* __restrict__ keys,
                                                          const uint32_t* __restrict__ vals, const uint32_t* __restrict__ flag,
                                                          const uint32_t* __restrict__ rank, int64_t n, float z_min, float z_max,
                                                          float* __restrict__ xyz, uint8_t* __restrict__ bgr)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n || !flag[s]) return;
    const uint64_t k = keys[s];
    const CloudImageRec r = recs[k >> 32];
    float sum[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int cnt = 0;
    for (int64_t t = s; t < n && keys[t] == k; t++) {
        const int local = (int)((int64_t)vals[t] - r.pix_off);
        float x, y, z;
        pixel_point(r, local, z_min, z_max, x, y, z);        // kept: it has a key
        const int v = local / r.width, u = local - v * r.width;
        const uint8_t* c = r.color + (size_t)v * r.color_step + 3 * (size_t)u;
        const float cb = (float)c[r.swap_rb ? 2 : 0], cg = (float)c[1], cr = (float)c[r.swap_rb ? 0 : 2];
        sum[0] += x; sum[1] += y; sum[2] += z; sum[3] += cr; sum[4] += cg; sum[5] += cb;
        cnt++;
    }
    const float c = (float)cnt;
    const size_t o = 3 * (size_t)rank[s];
    xyz[o] = sum[0] / c; xyz[o + 1] = sum[1] / c; xyz[o + 2] = sum[2] / c;
    bgr[o] = (uint8_t)(sum[5] / c); bgr[o + 1] = (uint8_t)(sum[4] / c); bgr[o + 2] = (uint8_t)(sum[3] / c);
}

int key_bits(int32_t n_images)
{
    int b = 1;
    while (b < 31 && ((int64_t)1 << b) < n_images) b++;
    return 32 + b;
}

}  // namespace

size_t cloud_voxel_temp_bytes(int64_t n_pixels, int32_t n_images)
{
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)n_pixels,
                                    0, key_bits(n_images));
    (void)rocprim::exclusive_scan(nullptr, b, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, (size_t)n_pixels, rocprim::plus<uint32_t>());
    return a > b ? a : b;
}

void cloud_voxel_sort(const CloudImageRec* recs, int32_t n_images, int64_t n_pixels, int32_t max_pixels, float leaf, float z_min,
                      float z_max, const CloudVoxelWork& w, hipStream_t s)
{
    (void)hipMemsetAsync(w.bbox, 0xff, (size_t)n_images * 12, s);                    // the minima ...
    (void)hipMemsetAsync(w.bbox + 3 * (size_t)n_images, 0, (size_t)n_images * 12, s);  // ... and, behind them, the maxima
    (void)hipMemsetAsync(w.info, 0, (size_t)n_images * 8, s);
    if (n_pixels > 0) {
        const dim3 grid((max_pixels + 255) / 256, n_images);
        hipLaunchKernelGGL(cloud_bbox_kernel, grid, dim3(256), 0, s, recs, w.bbox, z_min, z_max);
        hipLaunchKernelGGL(cloud_key_kernel, grid, dim3(256), 0, s, recs, w.bbox, w.info, w.keys[0], w.vals[0], leaf, z_min, z_max);
        size_t bytes = w.temp_bytes;
        (void)rocprim::radix_sort_pairs(w.temp, bytes, w.keys[0], w.keys[1], w.vals[0], w.vals[1], (size_t)n_pixels, 0, key_bits(n_images), s);
        hipLaunchKernelGGL(cloud_head_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, w.keys[1], w.flag, n_pixels);
        bytes = w.temp_bytes;
        (void)rocprim::exclusive_scan(w.temp, bytes, w.flag, w.rank, 0u, (size_t)n_pixels, rocprim::plus<uint32_t>(), s);
    }
    hipLaunchKernelGGL(cloud_count_kernel, dim3((n_images + 63) / 64), dim3(64), 0, s, recs, n_images, n_pixels, w.flag, w.rank, w.info);
}

void launch_cloud_voxel_points(const CloudImageRec* recs, int64_t n_pixels, float leaf, float z_min, float z_max, const CloudVoxelWork& w,
                               float* xyz, uint8_t* bgr, hipStream_t s)
{
    (void)leaf;
    if (n_pixels > 0)
        hipLaunchKernelGGL(cloud_voxel_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, s, recs, w.keys[1], w.vals[1], w.flag,
                           w.rank, n_pixels, z_min, z_max, xyz, bgr);
}

}  // namespace uzl
