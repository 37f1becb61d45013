// scanmerge_kernels.hip — the laser scans of two merged nodes folded into one on gfx950 (contract: include/uzl_mi355x.h, "Node
// merging: the two nodes' laser scans").
//
// scanmerge_kernel: one 256-thread workgroup per (keep, drop) pair.  A scan has four point lists (keep's ranges and intensities,
// drop's ranges and intensities); a list is made with one lane per beam (steps 2-3: the reading through the scan's own (cos, sin)
// table and its displacement, the bin on keep's grid by the laser line's boundary tests, rho), as 64-bit elements
// (bin << 12 | beam) << 32 | bits of rho, and sorted in LDS (bitonic, unused beams at the end): the points of one bin then lie side
// by side in beam order.  Of keep's lists the last element of a run is the bin's value (step 5); of drop's lists the lane at a
// run's head folds its run into the bin in beam order (step 6).  The merged array of the moment lives in LDS; ranges are finished
// (and the scan centre summed in beam order by the first wave, step 7) before the intensities reuse both buffers: 48 KiB per workgroup,
// so three pairs share a CU.  The tables stay in global memory: a lane reads one entry of its scan's and a few of keep's.
// No float atomics: every bin is written by one lane, and the result does not depend on the schedule.
// Built with -ffp-contract=off and correctly rounded f32 sqrt: every operation rounds as the contract says.
#include "laser_bins.hpp"
#include "scanmerge_types.hpp"

namespace uzl {

namespace {

constexpr uint64_t kUnused = ~0ull;
constexpr int kWave = 64;

__device__ inline int elem_bin(uint64_t e) { return (int)(e >> (32 + kScanMergeKeyShift)); }
__device__ inline float elem_rho(uint64_t e) { return __uint_as_float((uint32_t)e); }

// steps 2-3 for beam i of list `values` of scan S: the bin on a's grid (-1: unused or dropped) and rho
__device__ inline int point(const ScanMergeScanRec& S, const float* values, const double2* trig, const ScanMergeScanRec& A, const double2* trig_a,
                            int i, float* rho)
{
    *rho = 0.f;
    const float r = values[i];
    if (isnan(r) || !(r >= S.range_min) || !(r <= S.range_max)) return -1;
    const double2 t = trig[S.trig_off + i];
    const float x = (float)(t.x * (double)r);
    const float y = (float)(t.y * (double)r);
    const float qx = (S.D[0] * x + S.D[1] * y) + S.D[2];
    const float qy = (S.D[3] * x + S.D[4] * y) + S.D[5];
    const int b = bin_of(trig_a, A.n, (double)qx, (double)qy, qx, qy, A.amin, A.inc);
    if (b < 0) return -1;
    *rho = sqrtf(qx * qx + qy * qy);
    return b;
}

// ascending bitonic sort of s[0 .. P), P a power of two >= 2; every lane of the workgroup calls it
__device__ void sort_list(uint64_t* s, int P, int tid)
{
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += kScanMergeBlock) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i + j;
                const uint64_t x = s[i], y = s[l];
                if ((x > y) == ((i & k) == 0)) { s[i] = y; s[l] = x; }
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kScanMergeBlock) void scanmerge_kernel(ScanMergeArgs a)
{
    __shared__ uint64_t s_sort[kScanMergeMaxBeams];
    __shared__ float s_out[kScanMergeMaxBeams];
    const int tid = (int)threadIdx.x;
    const bool stage = a.stage_pair >= 0;
    const int pair = stage ? a.stage_pair : (int)blockIdx.x;
    const ScanMergePairRec& p = a.pairs[pair];
    const ScanMergeScanRec& A = p.a;
    const double2* trig_a = a.trig + A.trig_off;
    const int na = A.n;
    const float lo = A.range_min, hi0 = A.range_max;

    for (int arr = 0; arr < 2; arr++) {                     // 0: ranges, 1: intensities
        for (int k = tid; k < na; k += kScanMergeBlock) s_out[k] = arr == 0 ? hi0 + 1.0f : 0.f;   // step 4
        for (int src = 0; src < 2; src++) {                 // 0: a's list (step 5), 1: b's (step 6)
            const int which = 2 * src + arr;
            if (stage && which != a.stage_which) continue;  // the whole workgroup
            const ScanMergeScanRec& S = src == 0 ? p.a : p.b;
            const float* values = a.values + (arr == 0 ? S.ranges_off : S.intensities_off);
            int P = 2;
            while (P < S.n) P <<= 1;
            for (int i = tid; i < P; i += kScanMergeBlock) {
                uint64_t e = kUnused;
                if (i < S.n) {
                    float rho;
                    const int b = point(S, values, a.trig, A, trig_a, i, &rho);
                    if (stage) { a.st_bin[i] = b; a.st_rho[i] = rho; }
                    if (b >= 0) e = ((uint64_t)(((uint32_t)b << kScanMergeKeyShift) | (uint32_t)i) << 32) | (uint64_t)__float_as_uint(rho);
                }
                s_sort[i] = e;
            }
            if (stage) return;                              // the whole workgroup
            __syncthreads();
            sort_list(s_sort, P, tid);
            for (int j = tid; j < P; j += kScanMergeBlock) {
                const uint64_t e = s_sort[j];
                if (e == kUnused) continue;
                const int b = elem_bin(e);
                if (src == 0) {
                    // the highest beam of the bin wins
                    const uint64_t next = j + 1 < P ? s_sort[j + 1] : kUnused;
                    if (next == kUnused || elem_bin(next) != b) s_out[b] = elem_rho(e);
                    continue;
                }
                if (j > 0 && elem_bin(s_sort[j - 1]) == b) continue;    // not the head of its run
                float cur = s_out[b];
                for (int m = j; m < P; m++) {
                    const uint64_t f = s_sort[m];
                    if (f == kUnused || elem_bin(f) != b) break;
                    const float rho = elem_rho(f);
                    if (isnan(cur) || cur < lo || (arr == 0 && cur > hi0)) cur = rho;
                    else if (fabsf(cur - rho) < 0.1f) cur = 0.5f * (cur + rho);
                    else if (p.b_newer) cur = rho;
                }
                s_out[b] = cur;
            }
            __syncthreads();
        }
        if (stage) continue;
        float* out = (arr == 0 ? a.ranges : a.intensities) + p.out_off;
        for (int k = tid; k < na; k += kScanMergeBlock) out[k] = s_out[k];
        if (arr == 0 && tid < kWave) {
            // step 7 by the first wave.  The sums run in beam order, so they are one chain of additions; what the lanes share
            // is everything in front of it: 64 beams at a time each lane loads its table entry and rounds its two products, then
            // every lane adds the 64 pairs in lane order (the same chain in every lane), skipping the beams that do not count.
            double sx = 0.0, sy = 0.0;
            int count = 0;
            for (int k0 = 0; k0 < na; k0 += kWave) {
                const int k = k0 + tid;
                double px = 0.0, py = 0.0;
                bool ok = false;
                if (k < na) {
                    const float r = s_out[k];
                    ok = !(isnan(r) || !(r > lo) || !(r <= hi0));
                    const double2 t = trig_a[k];
                    px = t.x * (double)r;
                    py = t.y * (double)r;
                }
                const unsigned long long counted = __ballot(ok);
#pragma unroll
                for (int j = 0; j < kWave; j++) {
                    const double vx = __shfl(px, j), vy = __shfl(py, j);
                    if ((counted >> j) & 1ull) { sx += vx; sy += vy; count++; }
                }
            }
            if (tid == 0) {
                double cx = 0.0, cy = 0.0;
                if (count > 0) { cx = (double)(float)(sx / (double)count); cy = (double)(float)(sy / (double)count); }
                a.centers[3 * (size_t)pair] = cx;
                a.centers[3 * (size_t)pair + 1] = cy;
                a.centers[3 * (size_t)pair + 2] = 0.0;
            }
        }
        __syncthreads();                                    // s_out is read to the end before the intensities start it anew
    }
}

}  // namespace

void launch_scanmerge(const ScanMergeArgs& a, int n_pairs, hipStream_t s)
{
    if (n_pairs > 0) hipLaunchKernelGGL(scanmerge_kernel, dim3(n_pairs), dim3(kScanMergeBlock), 0, s, a);
}

}  // namespace uzl
