// merge_kernels.hip — the merge search of uzl_merge_* (uzl_merge.hip): which node would mergeTimerCallback
// (graph_slam/src/graph_slam_node.cpp:665-777) merge with which, for every start at once.
//
// partner(i) = min Q(i), Q(i) = the nodes getNodesWithinHops (graph_slam_common/src/slam_graph.cpp:231-264) marks from i that are
// not i, not node 0, closer than max_distance (:740) and turned by at most max_rotation_deg (:743-747), for every i the start test
// (:696) admits; include/uzl_mi355x.h states the contract.  Three launches:
//
// merge_near_kernel   all nodes against all nodes, no graph: a start is flagged iff the start test holds and some node other than
//                     itself and node 0 passes both geometry tests.  Q(i) is a subset of those nodes, so a start that is not flagged
//                     has no partner and needs no walk.  Positions go through LDS in tiles; a rotation is read only where the
//                     distance passes.  The output is one list of flagged starts (a vector atomic add hands out its slots; the
//                     order of the list does not matter, every start writes its own partner[]).  No candidate lists, no counts.
// merge_walk_kernel   one wave per flagged start.  getNodesWithinHopsHelper is a recursion with one visited_ flag per node whose
//                     result depends on the order of node.edges_, so it is run as written: depth first over the CSR rows (ascending
//                     edge index), a visited bitmap of n bits in the wave's LDS, and the recursion's stack as one frame (cursor and
//                     end of a row) per lane.  The walk is serial by definition; the wave's 64 lanes work WITHIN a step: they load
//                     the next 64 row entries from the cursor, test their visited bits, and a ballot names the first unvisited one
//                     - what the reference's loop would reach next, since the entries before it are visited and stay so.  A hub
//                     costs ceil(deg / 64) steps.  Afterwards the wave reads its bitmap in ascending order, applies the geometry
//                     tests and writes the first hit.  The walk is never cut short: it ends when the recursion ends.
// merge_tick_kernel   the smallest start >= first with a partner, as (keep, drop, next_index) in 16 bytes.
//
// A wave never waits for another one: there is no barrier and no flag in merge_walk_kernel, every branch is wave-uniform.
// -ffp-contract=off: every product and sum rounds on its own, as in tests/merge_reference.py.
#include "merge_types.hpp"

#include <mutex>

namespace uzl {

namespace {

__device__ __forceinline__ double merge_len(double dx, double dy, double dz) { return sqrt((dx * dx + dy * dy) + dz * dz); }

// tr(R_a^T R_b) >= bound: the nine entry-wise products in row-major order, summed left to right
__device__ __forceinline__ bool merge_rot_ok(const double* __restrict__ A, const double* __restrict__ B, double bound)
{
    double s = A[0] * B[0];
    s = s + A[1] * B[1]; s = s + A[2] * B[2];
    s = s + A[4] * B[4]; s = s + A[5] * B[5]; s = s + A[6] * B[6];
    s = s + A[8] * B[8]; s = s + A[9] * B[9]; s = s + A[10] * B[10];
    return s >= bound;
}

}  // namespace

__global__ __launch_bounds__(kMergeNearBlk) void merge_split_kernel(const double* __restrict__ pose12, int n, double* __restrict__ x,
                                                                    double* __restrict__ y, double* __restrict__ z)
{
    const int v = blockIdx.x * kMergeNearBlk + threadIdx.x;
    if (v >= n) return;
    const double* T = pose12 + (size_t)v * 12;
    x[v] = T[3]; y[v] = T[7]; z[v] = T[11];
}

__global__ __launch_bounds__(kMergeNearBlk) void merge_clear_kernel(MergeArgs a)
{
    const int v = blockIdx.x * kMergeNearBlk + threadIdx.x;
    if (v < a.n) a.partner[v] = -1;
    if (v == 0) { *a.n_starts = 0; *a.visited = 0ull; }
}

__global__ __launch_bounds__(kMergeNearBlk) void merge_near_kernel(MergeArgs a)
{
    __shared__ double s_x[kMergeNearBlk], s_y[kMergeNearBlk], s_z[kMergeNearBlk];
    const int tid = threadIdx.x, n = a.n;
    const int i = blockIdx.x * kMergeNearBlk + tid;
    double xi = 0., yi = 0., zi = 0.;
    bool open = false;                                                  // a start that has no candidate yet
    if (i < n && i >= a.first) {
        xi = a.x[i]; yi = a.y[i]; zi = a.z[i];
        open = merge_len(xi - a.cx, yi - a.cy, zi - a.cz) > a.start_bound;                   // :696, strict
    }
    bool found = false;
    for (int j0 = 0; j0 < n; j0 += kMergeNearBlk) {
        const int jl = j0 + tid;
        __syncthreads();                                                // the tile before this one has been read
        if (jl < n) { s_x[tid] = a.x[jl]; s_y[tid] = a.y[jl]; s_z[tid] = a.z[jl]; }
        __syncthreads();
        if (!open) continue;
        const int cnt = n - j0 < kMergeNearBlk ? n - j0 : kMergeNearBlk;
        for (int k = 0; k < cnt; k++) {
            const int j = j0 + k;
            if (!(merge_len(xi - s_x[k], yi - s_y[k], zi - s_z[k]) < a.max_distance)) continue;          // :740
            if (j == i || j == 0) continue;
            if (merge_rot_ok(a.pose12 + (size_t)i * 12, a.pose12 + (size_t)j * 12, a.trace_bound)) { found = true; open = false; break; }
        }
    }
    if (found) a.starts[atomicAdd(a.n_starts, 1)] = i;                 // at most n entries: one per node
}

__global__ __launch_bounds__(kMergeWalkBlk) void merge_walk_kernel(MergeArgs a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_bits[];  // [kMergeWaves][words]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = a.n, words = (n + 31) >> 5;
    uint32_t* bits = s_bits + (size_t)wave * words;
    const int n_starts = *a.n_starts;
    const int stride = gridDim.x * kMergeWaves;
    unsigned long long marked = 0ull;

    for (int q = blockIdx.x * kMergeWaves + wave; q < n_starts; q += stride) {
        const int start = a.starts[q];
        for (int w = lane; w < words; w += 64) bits[w] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (lane == 0) bits[start >> 5] = 1u << (start & 31);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        marked++;

        // frame d of the recursion (a node with max_hops - d > 0 hops left) lives in lane d: the cursor into its row and the row's end
        int cur = 0, end = 0;
        int depth = -1;
        if (a.max_hops > 0) {
            depth = 0;
            if (lane == 0) { cur = a.row_ptr[start]; end = a.row_ptr[start + 1]; }
        }
        while (depth >= 0) {
            const int c = __shfl(cur, depth), e = __shfl(end, depth);
            if (c >= e) { depth--; continue; }                          // the loop of :238 is over: return
            const int idx = c + lane;
            int nb = -1;
            if (idx < e) nb = a.col[idx];
            const bool fresh = nb >= 0 && !((bits[nb >> 5] >> (nb & 31)) & 1u);                          // :245
            const unsigned long long m = __ballot(fresh);
            if (m == 0ull) {                                            // these entries are visited, and stay so
                if (lane == depth) cur = c + 64 < e ? c + 64 : e;
                continue;
            }
            const int l = __ffsll((long long)m) - 1;
            const int v = __shfl(nb, l);
            if (lane == depth) cur = c + l + 1;
            if (lane == 0) bits[v >> 5] |= 1u << (v & 31);             // :233-235
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            marked++;
            if (depth + 1 < a.max_hops) {                               // hops - 1 > 0: its own loop runs (:237)
                depth++;
                if (lane == depth) { cur = a.row_ptr[v]; end = a.row_ptr[v + 1]; }
            }
        }

        // min Q(start): the set bits in ascending order, 64 words at a time - lane l holds the nodes [32 (w0 + l), 32 (w0 + l) + 32)
        const double xs = a.x[start], ys = a.y[start], zs = a.z[start];
        int partner = -1;
        for (int w0 = 0; w0 < words && partner < 0; w0 += 64) {
            const int w = w0 + lane;
            uint32_t word = w < words ? bits[w] : 0u;
            int hit = -1;
            while (word && hit < 0) {
                const int b = __ffs((int)word) - 1;
                word &= word - 1u;
                const int v = (w << 5) + b;
                if (v == start || v == 0) continue;
                if (!(merge_len(xs - a.x[v], ys - a.y[v], zs - a.z[v]) < a.max_distance)) continue;
                if (merge_rot_ok(a.pose12 + (size_t)start * 12, a.pose12 + (size_t)v * 12, a.trace_bound)) hit = v;
            }
            const unsigned long long m = __ballot(hit >= 0);
            if (m) partner = __shfl(hit, __ffsll((long long)m) - 1);
        }
        if (lane == 0) a.partner[start] = partner;
    }
    if (lane == 0 && marked) atomicAdd(a.visited, marked);
}

__global__ __launch_bounds__(kMergeTickBlk) void merge_tick_kernel(MergeArgs a)
{
    __shared__ int s_best;
    if (threadIdx.x == 0) s_best = INT32_MAX;
    __syncthreads();
    int best = INT32_MAX;
    for (int i = a.first + (int)threadIdx.x; i < a.n; i += kMergeTickBlk)
        if (a.partner[i] >= 0) { best = i; break; }                     // a lane's indices ascend
    if (best != INT32_MAX) atomicMin(&s_best, best);
    __syncthreads();
    if (threadIdx.x == 0) {
        MergeResult r{-1, -1, a.n, 0};
        const int i = s_best;
        if (i != INT32_MAX) {
            const int p = a.partner[i];
            r.keep = i > p ? i : p; r.drop = i > p ? p : i; r.next_index = i;                           // :751-753
        }
        *a.result = r;
    }
}

void launch_merge_split(const double* pose12, int32_t n, double* x, double* y, double* z, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(merge_split_kernel, dim3((n + kMergeNearBlk - 1) / kMergeNearBlk), dim3(kMergeNearBlk), 0, s, pose12, n, x, y, z);
}

void launch_merge_near(const MergeArgs& a, hipStream_t s)
{
    const dim3 grid((a.n + kMergeNearBlk - 1) / kMergeNearBlk > 0 ? (a.n + kMergeNearBlk - 1) / kMergeNearBlk : 1);
    hipLaunchKernelGGL(merge_clear_kernel, grid, dim3(kMergeNearBlk), 0, s, a);
    if (a.n > 0) hipLaunchKernelGGL(merge_near_kernel, grid, dim3(kMergeNearBlk), 0, s, a);
}

hipError_t launch_merge_walk(const MergeArgs& a, hipStream_t s)
{
    if (a.n <= 0) return hipSuccess;
    const int bytes = kMergeWaves * ((a.n + 31) / 32) * 4;              // <= kMergeWaves * kMergeBitmapBytes: set_graph holds n to the bound
    static int configured = 0;                                          // process-wide: the kernel is a symbol of the code object
    static std::mutex mu;
    if (bytes > 48 * 1024) {
        std::lock_guard<std::mutex> lock(mu);
        if (!configured) {
            const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(merge_walk_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                     kMergeWaves * kMergeBitmapBytes);
            if (e != hipSuccess) return e;
            configured = 1;
        }
    }
    const int want = (a.n + kMergeWaves - 1) / kMergeWaves;             // a wave per start if every node were one
    hipLaunchKernelGGL(merge_walk_kernel, dim3(want < kMergeWalkGroups ? want : kMergeWalkGroups), dim3(kMergeWalkBlk), bytes, s, a);
    return hipSuccess;
}

void launch_merge_tick(const MergeArgs& a, hipStream_t s)
{
    hipLaunchKernelGGL(merge_tick_kernel, dim3(1), dim3(kMergeTickBlk), 0, s, a);
}

}  // namespace uzl
