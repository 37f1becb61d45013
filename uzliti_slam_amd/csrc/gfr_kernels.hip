// gfr_kernels.hip — device side of the global-feature-repository place recognizer (uzl_gfr.hip), on gfx950.  Integer only.
//
//   gfr_nearest_kernel    per query row the nearest feature of the repository under the Hamming distance, as one packed key
//                         (distance << 32 | feature): the minimum is exact and ties go to the lower feature index
//   gfr_vote_kernel       one lane per matched row walks its feature's link chain and counts one vote per entry
//   gfr_select_kernel     the places whose votes reach the threshold, compacted in place order
//   gfr_integrate_kernel  the node's rows become new features or new links; indices from ballot prefixes in row order
// No atomic decides where anything is stored: the 64-bit atomicMin merges order-independent minima, the vote atomics only count,
// and the atomicExch of the integration only decides the order of entries within one feature's chain, which no result reads.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "gfr_types.hpp"

namespace uzl {

namespace {

constexpr int kGfrWaves = kGfrBlock / 64;

__device__ __forceinline__ int lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ bool gfr_matched(unsigned long long key, int max_distance)
{
    return key != kGfrNoKey && (int)(key >> 32) < max_distance;               // strict (global_feature_repository.cpp:89)
}

}  // namespace

// The pattern of knn2_lds_kernel with the train side in HBM: one lane per query row (the row's words in registers), the repository
// staged tile by tile in LDS with coalesced 16-byte loads, every lane reading each staged feature at the same address (a broadcast
// ds_read_b128: conflict-free).  grid = (workgroups along the repository) x (blocks of query rows): a workgroup strides over the
// tiles, so the repository is read once per block of query rows.  Within a tile the running minimum is a 32-bit key
// (distance << kGfrTileBits | index in the tile), one v_min_u32 per feature; tiles are merged into the 64-bit key, and the
// workgroups' partial minima meet in one 64-bit atomicMin per row.  The plain read in front of it only spares atomics: keys
// never grow, so a stale value is an upper bound of the current one.
template <int CH>
__global__ __launch_bounds__(kGfrMaxBlock) void gfr_nearest_kernel(GfrArgs a)
{
    __shared__ uint4 st[kGfrTile * CH];
    const int row = blockIdx.y * blockDim.x + threadIdx.x;
    const int rc = row < a.rows ? row : a.rows - 1;                            // lanes beyond the node compute on its last row, write nothing
    uint32_t q[4 * CH];
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const uint4 v = a.rows_d[(size_t)rc * CH + k];
        q[4 * k] = v.x; q[4 * k + 1] = v.y; q[4 * k + 2] = v.z; q[4 * k + 3] = v.w;
    }
    unsigned long long best = kGfrNoKey;
    const int tiles = (a.F + kGfrTile - 1) >> kGfrTileBits;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {             // uniform per workgroup
        const int t0 = tile << kGfrTileBits;
        const int tn = (a.F - t0 < kGfrTile) ? a.F - t0 : kGfrTile;            // features beyond F are neither staged nor read
        __syncthreads();
        for (int i = threadIdx.x; i < tn * CH; i += blockDim.x) st[i] = a.store[(size_t)t0 * CH + i];
        __syncthreads();
        uint32_t b = 0xffffffffu;
#pragma unroll 4
        for (int t = 0; t < tn; ++t) {
            uint32_t d0 = 0, d1 = 0;
#pragma unroll
            for (int k = 0; k < CH; k++) {
                const uint4 v = st[t * CH + k];
                d0 += __popc(q[4 * k] ^ v.x) + __popc(q[4 * k + 2] ^ v.z);
                d1 += __popc(q[4 * k + 1] ^ v.y) + __popc(q[4 * k + 3] ^ v.w);
            }
            b = min(b, ((d0 + d1) << kGfrTileBits) | (uint32_t)t);
        }
        const unsigned long long key = ((unsigned long long)(b >> kGfrTileBits) << 32) | (uint32_t)(t0 + (int)(b & (kGfrTile - 1)));
        best = key < best ? key : best;
    }
    if (row < a.rows && best < a.key[row]) atomicMin(&a.key[row], best);
}

// A matched row counts once for every entry of its feature's chain: duplicates count again (global_feature_repository.cpp:58-63).
__global__ __launch_bounds__(kGfrBlock) void gfr_vote_kernel(GfrArgs a)
{
    const int row = blockIdx.x * kGfrBlock + threadIdx.x;
    if (row >= a.rows) return;
    const unsigned long long key = a.key[row];
    if (!gfr_matched(key, a.max_distance)) return;
    const int f = (int)(uint32_t)key;
    if (f >= a.F) return;
    int e = a.head[f];
    for (int n = 0; e >= 0 && e < a.L && n < a.L; n++) {                       // a chain holds at most L entries
        const GfrLink l = a.link[e];
        if (l.place >= 0 && l.place < a.n_votes) atomicAdd(&a.votes[l.place], 1);
        e = l.next;
    }
}

// One workgroup: the places with votes >= min_votes (>= 1) in place order, positions from ballot prefixes.
__global__ __launch_bounds__(kGfrBlock) void gfr_select_kernel(GfrArgs a)
{
    __shared__ int s_wc[2][kGfrWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int2* cand = reinterpret_cast<int2*>(a.result + 1);
    int taken = 0, buf = 0;
    for (int c0 = 0; c0 < a.n_votes; c0 += kGfrBlock) {
        const int p = c0 + tid;
        const int v = p < a.n_votes ? a.votes[p] : 0;
        const bool hit = v >= a.min_votes;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) s_wc[buf][wave] = __popcll(m);
        __syncthreads();
        int off = taken, total = 0;
        for (int w = 0; w < kGfrWaves; w++) {
            const int c = s_wc[buf][w];
            if (w < wave) off += c;
            total += c;
        }
        if (hit) cand[off + lanes_below(m)] = make_int2(p, v);
        taken += total; buf ^= 1;
    }
    if (tid == 0) a.result->n_cand = taken;
}

// One workgroup, rows in row order (global_feature_repository_recognizer.cpp:76-82): an unmatched row with more than 3 * bytes set
// bits becomes feature F + (its rank among such rows) with one link; a matched row appends a link to its feature.  Entry index =
// L + rank among the rows that link.  Every row was matched against the repository as it stood before the node.
__global__ __launch_bounds__(kGfrBlock) void gfr_integrate_kernel(GfrArgs a)
{
    __shared__ int2 s_wc[2][kGfrWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int taken_new = 0, taken_link = 0, buf = 0;
    for (int c0 = 0; c0 < a.rows; c0 += kGfrBlock) {
        const int row = c0 + tid;
        const bool valid = row < a.rows;
        const unsigned long long key = valid ? a.key[row] : kGfrNoKey;
        const bool matched = valid && gfr_matched(key, a.max_distance);
        uint4 w[kGfrMaxBytes / 16];
        int bits = 0;
#pragma unroll
        for (int k = 0; k < kGfrMaxBytes / 16; k++) {
            w[k] = make_uint4(0u, 0u, 0u, 0u);
            if (valid && !matched && k < a.chunks) w[k] = a.rows_d[(size_t)row * a.chunks + k];
            bits += __popc(w[k].x) + __popc(w[k].y) + __popc(w[k].z) + __popc(w[k].w);
        }
        const bool fresh = valid && !matched && bits > 3 * a.bytes;            // addDescriptor's rule (global_feature_repository.cpp:117-123)
        const bool links = matched || fresh;
        const unsigned long long mn = __ballot(fresh), ml = __ballot(links);
        if (lane == 0) s_wc[buf][wave] = make_int2(__popcll(mn), __popcll(ml));
        __syncthreads();
        int on = taken_new, ol = taken_link, tn = 0, tl = 0;
        for (int v = 0; v < kGfrWaves; v++) {
            const int2 c = s_wc[buf][v];
            if (v < wave) { on += c.x; ol += c.y; }
            tn += c.x; tl += c.y;
        }
        const int e = a.L + ol + lanes_below(ml);
        if (fresh) {
            const int f = a.F + on + lanes_below(mn);
#pragma unroll
            for (int k = 0; k < kGfrMaxBytes / 16; k++)
                if (k < a.chunks) a.store[(size_t)f * a.chunks + k] = w[k];
            a.head[f] = e;
            a.link[e] = GfrLink{-1, a.place};
        } else if (matched) {
            const int f = (int)(uint32_t)key;
            a.link[e] = GfrLink{atomicExch(&a.head[f], e), a.place};
        }
        taken_new += tn; taken_link += tl; buf ^= 1;
    }
    if (tid == 0) { a.result->n_features = a.F + taken_new; a.result->n_links = a.L + taken_link; }
}

void launch_gfr_nearest(const GfrArgs& a, hipStream_t s)
{
    if (a.rows <= 0 || a.F <= 0) return;
    const int block = a.rows >= kGfrMaxBlock ? kGfrMaxBlock : (a.rows + 63) / 64 * 64;
    const int tiles = (a.F + kGfrTile - 1) >> kGfrTileBits;
    const dim3 grid(tiles < kGfrMaxGridX ? tiles : kGfrMaxGridX, (a.rows + block - 1) / block);
    switch (a.chunks) {
    case 1: hipLaunchKernelGGL(gfr_nearest_kernel<1>, grid, dim3(block), 0, s, a); break;
    case 2: hipLaunchKernelGGL(gfr_nearest_kernel<2>, grid, dim3(block), 0, s, a); break;
    case 3: hipLaunchKernelGGL(gfr_nearest_kernel<3>, grid, dim3(block), 0, s, a); break;
    default: hipLaunchKernelGGL(gfr_nearest_kernel<4>, grid, dim3(block), 0, s, a); break;
    }
}

void launch_gfr_vote(const GfrArgs& a, hipStream_t s)
{
    if (a.rows <= 0 || a.F <= 0) return;
    hipLaunchKernelGGL(gfr_vote_kernel, dim3((a.rows + kGfrBlock - 1) / kGfrBlock), dim3(kGfrBlock), 0, s, a);
}

void launch_gfr_select(const GfrArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(gfr_select_kernel, dim3(1), dim3(kGfrBlock), 0, s, a);
}

void launch_gfr_integrate(const GfrArgs& a, hipStream_t s)
{
    if (a.rows <= 0) return;
    hipLaunchKernelGGL(gfr_integrate_kernel, dim3(1), dim3(kGfrBlock), 0, s, a);
}

}  // namespace uzl
