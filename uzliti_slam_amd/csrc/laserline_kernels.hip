// laserline_kernels.hip — laser line from depth images on gfx950 (contract: include/uzl_mi355x.h, "Laser line from depth images").
//
// laser_bin_kernel: one 256-thread workgroup per (band of rows, image).  The (cos, sin) table and the workgroup's min s / max s per
// bin (bit patterns of non-negative floats, so integer min / max) live in LDS.  Lanes run across columns, four pixels per lane and
// row from one vector load, and each lane walks down the band's rows: for a roughly level camera a column stays in one bin, so the
// running min / max of a column's current bin stay in registers together with the bin's two boundaries, and LDS is touched only
// when the bin changes or the band ends.  The workgroup then folds its non-empty bins into the image's arrays with global
// atomicMin / atomicMax on u32: the result does not depend on the schedule.
// laser_finish_kernel: one workgroup per group of images: square roots and fill values (step 7), the merge of the group's images in
// order (step 8), the scan centre by one lane in beam order (step 9).
// Built with -ffp-contract=off and correctly rounded f32 divide / sqrt: every operation rounds as the contract says.
#include "laser_bins.hpp"
#include "laserline_types.hpp"

namespace uzl {

namespace {

// The bin a column is in, its two boundaries and the running min / max of s (bits) since the lane entered it.
struct Column {
    int bin;
    uint32_t mn, mx;
    double2 t0, t1;
};

__device__ inline void flush(const Column& c, uint32_t* s_min, uint32_t* s_max)
{
    if (c.bin < 0) return;
    atomicMin(&s_min[c.bin], c.mn);
    atomicMax(&s_max[c.bin], c.mx);
}

// steps 2-7 for one pixel value d (step 2's encoding already applied) at column u, row v
__device__ inline void pixel(const LaserBinArgs& a, const LaserImageRec& im, const double2* trig, uint32_t* s_min, uint32_t* s_max,
                             float d, int u, int v, Column& col)
{
    if (a.depth_scale != 1.0) d = (float)((double)d * a.depth_scale);
    if (!(d > 0.f) || isinf(d)) return;
    const float x = (float)((((double)u - im.cx) * (double)d) / im.fx);
    const float y = (float)((((double)v - im.cy) * (double)d) / im.fy);
    const float* T = im.T;
    const float qx = ((T[0] * x + T[1] * y) + T[2] * d) + T[3];
    const float qy = ((T[4] * x + T[5] * y) + T[6] * d) + T[7];
    const float qz = ((T[8] * x + T[9] * y) + T[10] * d) + T[11];
    if (isnan(qz) || (double)qz < a.min_height || (double)qz > a.max_height) return;
    const double X = (double)qx, Y = (double)qy;
    // an inner bin that holds the point while the next one does not is the point's bin: the column has stayed where it was
    if (!(col.bin > 0 && col.bin < a.n - 1 && holds(col.t0, X, Y) && !holds(col.t1, X, Y))) {
        const int b = bin_of(trig, a.n, X, Y, qx, qy, a.amin, a.inc);
        if (b < 0) return;
        if (b != col.bin) {
            flush(col, s_min, s_max);
            col.bin = b; col.mn = kLaserInfBits; col.mx = 0u;
            col.t0 = trig[b]; col.t1 = trig[b + 1];
        }
    }
    const float s = qx * qx + qy * qy;
    const uint32_t bits = __float_as_uint(s);
    col.mn = min(col.mn, bits);
    col.mx = max(col.mx, bits);
}

template <int ENC>
__device__ inline float depth_of(const uint8_t* p)
{
    if (ENC == UZL_DEPTH_F32_M) return *reinterpret_cast<const float*>(p);
    return (float)((double)*reinterpret_cast<const uint16_t*>(p) * 0.001);
}

template <int ENC>
__device__ void bin_band(const LaserBinArgs& a, const LaserImageRec& im, const uint8_t* base, int r0, int r1, const double2* trig,
                         uint32_t* s_min, uint32_t* s_max)
{
    constexpr int kBpp = ENC == UZL_DEPTH_F32_M ? 4 : 2;
    const int nvec = (im.width + kLaserVec - 1) / kLaserVec;
    const int lanes = im.lanes, side = kLaserBlock / lanes;
    const int t = (int)threadIdx.x;
    if (t >= lanes * side) return;
    const bool rows_aligned = im.step % (kLaserVec * kBpp) == 0;
    for (int cv = t % lanes; cv < nvec; cv += lanes) {
        const int u0 = cv * kLaserVec;
        const bool whole = rows_aligned && u0 + kLaserVec <= im.width;
        Column col[kLaserVec];
#pragma unroll
        for (int j = 0; j < kLaserVec; j++) col[j].bin = -1;
        for (int r = r0 + t / lanes; r < r1; r += side) {
            const uint8_t* row = base + (size_t)r * (size_t)im.step + (size_t)u0 * kBpp;
            float d[kLaserVec];
            if (whole) {
                if (ENC == UZL_DEPTH_F32_M) {
                    const float4 q = *reinterpret_cast<const float4*>(row);
                    d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
                } else {
                    const uint2 q = *reinterpret_cast<const uint2*>(row);
                    d[0] = (float)((double)(q.x & 0xffffu) * 0.001); d[1] = (float)((double)(q.x >> 16) * 0.001);
                    d[2] = (float)((double)(q.y & 0xffffu) * 0.001); d[3] = (float)((double)(q.y >> 16) * 0.001);
                }
            } else {
#pragma unroll
                for (int j = 0; j < kLaserVec; j++) d[j] = u0 + j < im.width ? depth_of<ENC>(row + j * kBpp) : 0.f;
            }
#pragma unroll
            for (int j = 0; j < kLaserVec; j++)
                if (u0 + j < im.width) pixel(a, im, trig, s_min, s_max, d[j], u0 + j, r, col[j]);
        }
#pragma unroll
        for (int j = 0; j < kLaserVec; j++) flush(col[j], s_min, s_max);
    }
}

__global__ __launch_bounds__(kLaserBlock) void laser_bin_kernel(LaserBinArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    double2* trig = reinterpret_cast<double2*>(lds);
    uint32_t* s_min = reinterpret_cast<uint32_t*>(lds + (size_t)(a.n + 1) * sizeof(double2));
    uint32_t* s_max = s_min + a.n;
    const LaserImageRec& im = a.images[blockIdx.y];
    const int r0 = (int)blockIdx.x * a.band_rows;
    if (r0 >= im.height) return;                            // the whole workgroup: this image has fewer bands
    const int r1 = min(r0 + a.band_rows, im.height);
    const int tid = (int)threadIdx.x;
    for (int k = tid; k <= a.n; k += kLaserBlock) trig[k] = a.trig[k];
    for (int k = tid; k < a.n; k += kLaserBlock) { s_min[k] = kLaserInfBits; s_max[k] = 0u; }
    __syncthreads();
    const uint8_t* base = a.pixels + im.data_off;
    if (im.encoding == UZL_DEPTH_F32_M) bin_band<UZL_DEPTH_F32_M>(a, im, base, r0, r1, trig, s_min, s_max);
    else bin_band<UZL_DEPTH_U16_MM>(a, im, base, r0, r1, trig, s_min, s_max);
    __syncthreads();
    uint32_t* gmin = a.smin + (size_t)im.out * (size_t)a.n;
    uint32_t* gmax = a.smax + (size_t)im.out * (size_t)a.n;
    for (int k = tid; k < a.n; k += kLaserBlock) {
        const uint32_t mn = s_min[k], mx = s_max[k];
        if (mn != kLaserInfBits) atomicMin(&gmin[k], mn);
        if (mx != 0u) atomicMax(&gmax[k], mx);
    }
}

__global__ __launch_bounds__(kLaserFinishBlock) void laser_finish_kernel(LaserFinishArgs a)
{
    __shared__ float s_ranges[kLaserMaxBeams];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int i0 = a.group_first[g], i1 = a.group_first[g + 1];
    const float lo = a.lo, hi0 = a.hi0, hi = hi0 + 1.0f, hi_sq = hi * hi;
    for (int k = tid; k < a.n; k += kLaserFinishBlock) {
        float range = 0.f, far = 0.f;
        for (int i = i0; i < i1; i++) {
            // step 7: the scan of image i at beam k
            const float mn = __uint_as_float(a.smin[(size_t)i * a.n + k]), mx = __uint_as_float(a.smax[(size_t)i * a.n + k]);
            const float r = mn < hi_sq ? sqrtf(mn) : hi;
            const float f = mx > 0.f ? sqrtf(mx) : 0.f;
            if (i == i0) { range = r; far = f; continue; }
            // step 8: merged into the group's first
            if (!(isnan(r) || r < lo || r > hi0)) {
                if (isnan(range) || range == 0.f || range > hi0) range = r;
                else if (fabsf(range - r) < 0.1f) range = 0.5f * (range + r);
                else range = 0.0f;
            }
            if (!(isnan(f) || f < lo)) {
                if (isnan(far) || far == 0.f || far > hi0) far = f;
                else if (fabsf(far - f) < 0.1f) far = 0.5f * (far + f);
                else if (far > f) far = 0.0f;
            }
        }
        a.ranges[(size_t)g * a.n + k] = range;
        a.intensities[(size_t)g * a.n + k] = far;
        s_ranges[k] = range;
    }
    __syncthreads();
    if (tid == 0) {                                         // step 9, in beam order
        double sx = 0.0, sy = 0.0;
        int count = 0;
        for (int k = 0; k < a.n; k++) {
            const float r = s_ranges[k];
            if (isnan(r) || !(r > lo) || !(r <= hi0)) continue;
            const double2 t = a.trig[k];
            sx += t.x * (double)r;
            sy += t.y * (double)r;
            count++;
        }
        double cx = 0.0, cy = 0.0;
        if (count > 0) { cx = (double)(float)(sx / (double)count); cy = (double)(float)(sy / (double)count); }
        a.centers[3 * (size_t)g] = cx;
        a.centers[3 * (size_t)g + 1] = cy;
        a.centers[3 * (size_t)g + 2] = 0.0;
    }
}

}  // namespace

void laser_prepare()
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(laser_bin_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)laser_bin_lds(kLaserMaxBeams));
}

void launch_laser_bin(const LaserBinArgs& a, int max_bands, int n_images, hipStream_t s)
{
    if (max_bands > 0 && n_images > 0)
        hipLaunchKernelGGL(laser_bin_kernel, dim3(max_bands, n_images), dim3(kLaserBlock), laser_bin_lds(a.n), s, a);
}

void launch_laser_finish(const LaserFinishArgs& a, int n_groups, hipStream_t s)
{
    if (n_groups > 0) hipLaunchKernelGGL(laser_finish_kernel, dim3(n_groups), dim3(kLaserFinishBlock), 0, s, a);
}

}  // namespace uzl
