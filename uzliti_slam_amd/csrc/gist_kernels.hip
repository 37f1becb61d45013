// gist_kernels.hip — device side of the binary-GIST place recognizer (uzl_gist.hip): exact k nearest live places under the
// Hamming distance, for a batch of queries, on gfx950.
//
// One workgroup of 256 lanes per query; lane i takes places i, i + 256, ... so adjacent lanes read adjacent descriptor rows
// (16-byte loads of rows padded to a 16-byte multiple).  Distance = xor + v_bcnt_u32_b32, integer only.
//   pass 1  histogram in LDS of the distances 0..dmax (dmax = min(floor(T), 8 bytes) <= 2048); the cutoff d* is the smallest distance
//           whose cumulative count reaches k, quota = k - (places below d*)
//   pass 2  the distances again (the store is L2-resident at these sizes); 256-place chunks in index order, a wave ballot + v_mbcnt
//           prefix places every hit: places below d* all, places at d* in index order up to the quota
//   sort    the <= k survivors by (distance, place) by rank counting; written out in that order
// No atomic decides where a survivor lands (the histogram's LDS atomics only count), so the output is deterministic.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gist_types.hpp"

namespace uzl {

namespace {

constexpr int kGistWaves = kGistBlock / 64;

__device__ __forceinline__ int gist_dist(const uint8_t* __restrict__ row, const uint4* q, int chunks)
{
    const uint4* r = reinterpret_cast<const uint4*>(row);
    int d = 0;
    for (int c = 0; c < chunks; c++) {
        const uint4 a = r[c], b = q[c];
        d += __popc(a.x ^ b.x) + __popc(a.y ^ b.y) + __popc(a.z ^ b.z) + __popc(a.w ^ b.w);
    }
    return d;
}

// distance of place p to the query, -1 when p is outside [0, limit) or not live.  The row is read whether or not the place is live
// (every row below limit is allocated: uzl_gist.hip sizes the store for all places once the length is known), so the row and live
// loads do not wait for each other (measured at 20k places: 33.2 us per query with the row load behind the live byte, 31.6 us so)
__device__ __forceinline__ int gist_place_dist(const GistKnnArgs& a, const uint4* q, int chunks, int p, int limit)
{
    if (p >= limit) return -1;
    const int d = gist_dist(a.store + (size_t)p * a.stride, q, chunks);
    return a.live[p] ? d : -1;
}

__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

}  // namespace

__global__ __launch_bounds__(kGistBlock) void gist_knn_kernel(GistKnnArgs a)
{
    __shared__ uint4 s_q[kGistMaxBytes / 16];
    __shared__ int s_hist[kGistMaxBins];
    __shared__ int2 s_sel[kGistMaxK];
    __shared__ int2 s_wc[2][kGistWaves];      // per wave (hits below d*, hits at d*), double-buffered over the chunks
    __shared__ int s_cut[3];                  // d*, places below d*, quota at d* (d* = -1: no place within dmax)

    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int2* out = a.out + (size_t)q * a.k;
    if (a.qvalid && !a.qvalid[q]) {
        if (tid == 0) a.out_n[q] = 0;
        return;
    }
    const int limit = a.base + q, chunks = a.stride / 16, nb = a.dmax + 1;
    const uint4* qrow = reinterpret_cast<const uint4*>(a.queries + (size_t)q * a.stride);
    if (tid < chunks) s_q[tid] = qrow[tid];
    for (int b = tid; b < nb; b += kGistBlock) s_hist[b] = 0;
    __syncthreads();

    // ---- pass 1: histogram of the distances within dmax
    for (int p = tid; p < limit; p += kGistBlock) {
        const int d = gist_place_dist(a, s_q, chunks, p, limit);
        if (d >= 0 && d <= a.dmax) atomicAdd(&s_hist[d], 1);
    }
    __syncthreads();

    // ---- the cutoff: wave 0, each lane sums a contiguous run of bins, inclusive scan over the lanes
    if (wave == 0) {
        const int per = (nb + 63) / 64, b0 = min(lane * per, nb), b1 = min(b0 + per, nb);
        int own = 0;
        for (int b = b0; b < b1; b++) own += s_hist[b];
        int incl = own;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, 64);
            if (lane >= o) incl += v;
        }
        const int total = __shfl(incl, 63, 64);
        const unsigned long long reach = __ballot(incl >= a.k);
        if (total == 0) {
            if (lane == 0) { s_cut[0] = -1; s_cut[1] = 0; s_cut[2] = 0; }
        } else if (reach == 0ull) {                                   // fewer than k within dmax: every one of them
            if (lane == 0) { s_cut[0] = a.dmax; s_cut[1] = total - s_hist[a.dmax]; s_cut[2] = s_hist[a.dmax]; }
        } else if (lane == __ffsll((long long)reach) - 1) {
            int c = incl - own;
            for (int b = b0; b < b1; b++) {
                if (c + s_hist[b] >= a.k) { s_cut[0] = b; s_cut[1] = c; s_cut[2] = a.k - c; break; }
                c += s_hist[b];
            }
        }
    }
    __syncthreads();
    const int dstar = s_cut[0], below = s_cut[1], quota = s_cut[2];
    if (dstar < 0) {
        if (tid == 0) a.out_n[q] = 0;
        return;
    }

    // ---- pass 2: places below d* and the first `quota` places at d*, positions from ballot prefixes in index order
    int taken_lt = 0, taken_eq = 0, buf = 0;
    for (int c0 = 0; c0 < limit; c0 += kGistBlock) {
        const int p = c0 + tid;
        const int d = gist_place_dist(a, s_q, chunks, p, limit);
        const bool lt = d >= 0 && d < dstar, eq = d == dstar;
        const unsigned long long mlt = __ballot(lt), meq = __ballot(eq);
        if (lane == 0) s_wc[buf][wave] = make_int2(__popcll(mlt), __popcll(meq));
        __syncthreads();
        int olt = taken_lt, oeq = taken_eq, tlt = 0, teq = 0;
        for (int w = 0; w < kGistWaves; w++) {
            const int2 c = s_wc[buf][w];
            if (w < wave) { olt += c.x; oeq += c.y; }
            tlt += c.x; teq += c.y;
        }
        if (lt) s_sel[olt + lanes_below(mlt)] = make_int2(p, d);
        if (eq) {
            const int r = oeq + lanes_below(meq);
            if (r < quota) s_sel[below + r] = make_int2(p, d);
        }
        taken_lt += tlt; taken_eq += teq; buf ^= 1;
        if (taken_lt == below && taken_eq >= quota) break;           // uniform: every lane summed the same counts
    }
    const int n_out = below + min(quota, taken_eq);
    __syncthreads();

    // ---- order by (distance, place): rank of each survivor among the <= k (places are distinct, so ranks are too)
    for (int i = tid; i < n_out; i += kGistBlock) {
        const int2 me = s_sel[i];
        int rank = 0;
        for (int j = 0; j < n_out; j++) {
            const int2 o = s_sel[j];
            rank += (o.y < me.y || (o.y == me.y && o.x < me.x)) ? 1 : 0;
        }
        out[rank] = me;
    }
    if (tid == 0) a.out_n[q] = n_out;
}

void launch_gist_knn(const GistKnnArgs& a, int n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(gist_knn_kernel, dim3(n), dim3(kGistBlock), 0, s, a);
}

}  // namespace uzl
