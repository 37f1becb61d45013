// scope_kernels.hip — node uncertainty (a whole-graph shortest-path pass) and the scope scans, for uzl_scope_* (uzl_scope.hip).
//
// scope_sssp_kernel restates SlamGraph::dijkstra (graph_slam_common/src/slam_graph.cpp:765-797) and the write-back of both
// reevaluateUncertainty forms (:506-517, :519-556) as ONE persistent workgroup per pass.
//
// Why a parallel relaxation gives the reference's bits.  The reference's distance_ is the least fixed point of
//     d[source] = 0,   d[u] = min over edges (v,u) of fl(d[v] + w(v,u)),
// w(v,u) = sqrt((dx*dx + dy*dy) + dz*dz) >= 0 from the current translations (Eigen's norm(); the operand order of rec_dist in
// gate_kernels.hip and of radius_kernel).  Floating-point addition is monotone in its first operand and fl(d + w) >= d for
// w >= 0, so every label a relaxation ever writes is the rounded length of a real path and never below the fixed point, and a
// state in which no relaxation improves anything IS the fixed point, whatever order led there.  The reference's heap order, with
// its lazy duplicate entries, is one such order; the frontier rounds below are another.  A non-negative double orders as its bit
// pattern (-0.0 cannot come out of a sqrt or a sum of non-negatives; +inf and NaN lie above DBL_MAX and never improve anything,
// as in `new_dist < distance_`), so a relaxation is one unsigned 64-bit atomic min.
//
// Rounds: two frontier bitmaps; a round relaxes every edge of every frontier node, a strict improvement puts the improved node on
// the next frontier, and the pass ends with the round that improves nothing.  Trajectory graphs are long chains, and one barrier
// round per hop would lose to a heap, so a lane that has strictly improved a node of degree 2 carries on through it to its other
// neighbour (the neighbour it came from cannot improve: fl(fl(d + w) + w) >= d) until it reaches a node of another degree, which
// goes on the frontier, or fails to improve.  Strictness ends the walk on a ring and on zero-length edges.  Only the source and
// nodes of degree != 2 are ever on a frontier.  A round serves the frontier nodes whose label lies within kScopeBucketEdges mean
// edge lengths of the frontier's smallest label and hands the others on to the next round (serving everything at once improves a
// node of a loopy graph some fifty times before it is final; the order changes the work, never the result).  The frontier node of
// the smallest label is final - a label that is not final hangs off a frontier node with a smaller, final one - and a final node
// never returns, so every round settles at least one node of degree != 2: rounds <= (nodes of degree != 2) + 2, whatever the hops.
//
// Storage: up to kScopeLdsNodes nodes the distances and bitmaps live in LDS (ds_min_rtn_u64); above, in global memory with
// agent-scope atomics (the L1 is not updated by an atomic, so the distances are also read with atomic loads).  Synchronisation is
// __syncthreads() only; no lane waits on a flag.
//
// scope_scan_kernel restates getOutOfScopeNodes (slam_graph.cpp:216-229) behind scopeRequestTimerCallback's radius
// (graph_slam_node.cpp:586, :623) and the test of scopeRequestCallback (:549-559): it streams the SoA positions once per pass and
// appends hits in index order with radius_kernel's ballot + prefix scheme, a count pass and a write pass.
// -ffp-contract=off: every sum and product rounds on its own, as on the host.
#include "scope_types.hpp"

namespace uzl {

namespace {

__device__ __forceinline__ double scope_len(double ax, double ay, double az, double bx, double by, double bz)
{
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

template <bool LDS>
__device__ __forceinline__ unsigned long long dist_load(unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ unsigned long long dist_min(unsigned long long* p, unsigned long long v)
{
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ uint32_t front_load(uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ void front_set(uint32_t* f, int v)
{
    __hip_atomic_fetch_or(f + (v >> 5), 1u << (v & 31), __ATOMIC_RELAXED, LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT);
}

// Relax the edge prev -> v of length w from the label d_prev, and walk on through nodes of degree 2 while the improvement is strict.
// Returns whether a node went on the next frontier.
template <bool LDS>
__device__ __forceinline__ bool relax_walk(const ScopeRec* __restrict__ rec, unsigned long long* dist, uint32_t* f_next, int prev,
                                           unsigned long long d_prev, int v, double w, long long& relaxations)
{
    unsigned long long nd = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)d_prev) + w);
    if (!(nd < dist_min<LDS>(dist + v, nd))) return false;               // slam_graph.cpp:790, strict
    relaxations++;
    ScopeRec r = rec[v];
    for (;;) {
        if (r.deg != 2) { front_set<LDS>(f_next, v); return true; }
        const bool back_a = r.a == prev;
        const int nxt = back_a ? r.b : r.a;
        const ScopeRec rn = rec[nxt];                                    // issued beside the atomic, needed only if it improves
        const unsigned long long nd2 = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)nd) + (back_a ? r.wb : r.wa));
        if (!(nd2 < dist_min<LDS>(dist + nxt, nd2))) return false;
        relaxations++;
        prev = v; v = nxt; nd = nd2; r = rn;
    }
}

}  // namespace

template <bool LDS>
__global__ __launch_bounds__(kScopeBlk) void scope_sssp_kernel(ScopeArgs a)
{
    __shared__ unsigned long long s_dist[LDS ? kScopeLdsNodes : 1];
    __shared__ uint32_t s_front[2][LDS ? kScopeLdsNodes / 32 : 1];
    __shared__ int s_any[2];
    __shared__ unsigned long long s_lo[2];
    __shared__ double s_wsum;
    __shared__ unsigned long long s_relax;
    __shared__ int s_reached;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int kWaves = kScopeBlk / 64;
    const int n = a.n, words = (n + 31) >> 5;
    unsigned long long* dist = LDS ? s_dist : a.dist;
    uint32_t* front0 = LDS ? s_front[0] : a.front;
    uint32_t* front1 = LDS ? s_front[1] : a.front + words;
    const double initial = a.add_initial ? a.unc[a.source] : 0.;        // slam_graph.cpp:547: read before any write

    // ---- this pass's edge lengths, node records, and distance_ = DBL_MAX (:768-771)
    if (tid == 0) { s_any[0] = s_any[1] = 0; s_lo[0] = s_lo[1] = ~0ull; s_wsum = 0.; s_relax = 0ull; s_reached = 0; }
    __syncthreads();
    double wsum = 0.;
    for (int e = tid; e < a.m; e += kScopeBlk) {
        const int u = a.row[e], v = a.col[e];
        const double w = scope_len(a.x[u], a.y[u], a.z[u], a.x[v], a.y[v], a.z[v]);
        a.w[e] = w;
        if (w < __longlong_as_double((long long)kScopeInf)) wsum += w;
    }
    if (wsum > 0.) atomicAdd(&s_wsum, wsum);
    for (int v = tid; v < n; v += kScopeBlk) {
        ScopeRec r;
        r.first = a.row_ptr[v]; r.deg = a.row_ptr[v + 1] - r.first; r.a = r.b = -1; r.wa = r.wb = 0.;
        if (r.deg == 2) {
            r.a = a.col[r.first]; r.b = a.col[r.first + 1];
            const double vx = a.x[v], vy = a.y[v], vz = a.z[v];
            r.wa = scope_len(vx, vy, vz, a.x[r.a], a.y[r.a], a.z[r.a]);
            r.wb = scope_len(vx, vy, vz, a.x[r.b], a.y[r.b], a.z[r.b]);
        }
        a.rec[v] = r;
        dist[v] = kScopeInf;
    }
    for (int k = tid; k < words; k += kScopeBlk) { front0[k] = 0u; front1[k] = 0u; }
    if (!LDS) __threadfence();
    __syncthreads();
    if (tid == 0) {
        dist[a.source] = 0ull;                                          // :773-774
        front0[a.source >> 5] = 1u << (a.source & 31);
    }
    if (!LDS) __threadfence();
    __syncthreads();

    // the bucket of a round: the frontier nodes within this much of the frontier's smallest label (a few mean edge lengths)
    const double delta = kScopeBucketEdges * (s_wsum / (double)(a.m > 0 ? a.m : 1));
    long long rounds = 0, relaxations = 0;
    uint32_t* f_cur = front0; uint32_t* f_next = front1;
    for (;;) {
        const int par = (int)(rounds & 1);
        bool any = false;
        // the smallest label on the frontier: that node is final (every label that is not final hangs off a frontier node with a
        // smaller, final one), so a round settles at least one node for good
        unsigned long long lo = ~0ull;
        for (int base = wave * 64; base < n; base += kWaves * 64) {
            const int u = base + lane;
            if (u < n && ((front_load<LDS>(f_cur + (u >> 5)) >> (u & 31)) & 1u)) {
                const unsigned long long d = dist_load<LDS>(dist + u);
                lo = d < lo ? d : lo;
            }
        }
        if (lo != ~0ull) __hip_atomic_fetch_min(&s_lo[par], lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __syncthreads();
        lo = s_lo[par];
        const unsigned long long near = (unsigned long long)__double_as_longlong(__longlong_as_double((long long)lo) + delta);
        for (int base = wave * 64; base < n; base += kWaves * 64) {
            const int u = base + lane;
            bool in_front = false;
            if (u < n) in_front = (front_load<LDS>(f_cur + (u >> 5)) >> (u & 31)) & 1u;
            int first = 0, deg = 0;
            unsigned long long du = 0ull;
            if (in_front) {
                du = dist_load<LDS>(dist + u);
                if (du > near && du != lo) {                              // beyond the bucket: its turn comes in a later round
                    front_set<LDS>(f_next, u); any = true; in_front = false;
                }
            }
            if (in_front) { first = a.row_ptr[u]; deg = a.row_ptr[u + 1] - first; }
            if (in_front && deg <= kScopeLaneDeg)
                for (int s = first; s < first + deg; s++) any |= relax_walk<LDS>(a.rec, dist, f_next, u, du, a.col[s], a.w[s], relaxations);
            // a hub's edges go over the lanes of its wave
            unsigned long long hubs = __ballot(in_front && deg > kScopeLaneDeg);
            while (hubs) {
                const int l = __ffsll((long long)hubs) - 1;
                hubs &= hubs - 1ull;
                const int hf = __shfl(first, l), hd = __shfl(deg, l);
                const unsigned long long hdu = __shfl(du, l);
                for (int s = lane; s < hd; s += 64) any |= relax_walk<LDS>(a.rec, dist, f_next, base + l, hdu, a.col[hf + s], a.w[hf + s], relaxations);
            }
        }
        if (any) s_any[par] = 1;
        if (!LDS) __threadfence();
        __syncthreads();
        rounds++;
        const bool more = s_any[par] != 0;
        // the frontier just served becomes the one after next: clear it, and the flag the round after this one raises
        for (int k = tid; k < words; k += kScopeBlk) f_cur[k] = 0u;
        if (tid == 0) { s_any[par ^ 1] = 0; s_lo[par ^ 1] = ~0ull; }
        if (!LDS) __threadfence();
        __syncthreads();
        if (!more) break;
        uint32_t* t = f_cur; f_cur = f_next; f_next = t;
    }

    // ---- distance_ out, and the write-back (:511-515, :550-554): nodes not reached keep their uncertainty_
    int reached = 0;
    for (int v = tid; v < n; v += kScopeBlk) {
        const unsigned long long d = dist_load<LDS>(dist + v);
        if (LDS) a.dist[v] = d;
        if (d != kScopeInf) {
            const double dd = __longlong_as_double((long long)d);
            a.unc[v] = a.add_initial ? initial + dd : dd;
            reached++;
        }
    }
    atomicAdd(&s_reached, reached);
    atomicAdd(&s_relax, (unsigned long long)relaxations);
    __syncthreads();
    if (tid == 0) {
        a.result->rounds = rounds; a.result->relaxations = (long long)s_relax; a.result->n_reached = s_reached; a.result->pad = 0;
    }
}

// WRITE = false: count[block] = hits of the block's slab.  WRITE = true: the hits go to out[] behind those of the slabs before.
template <bool WRITE>
__global__ __launch_bounds__(kScanBlk) void scope_scan_kernel(ScopeScanArgs a)
{
    __shared__ int s_wave[kScanBlk / 64];
    __shared__ int s_base;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bool request = a.current >= 0;
    double cx = a.cx, cy = a.cy, cz = a.cz, thr = a.radius;
    if (request) {
        cx = a.x[a.current]; cy = a.y[a.current]; cz = a.z[a.current];
        const double su = a.scope_size_factor * a.unc[a.current];
        const double scope = a.scope_size_min < su ? su : a.scope_size_min;      // std::max, graph_slam_node.cpp:586
        thr = (double)(float)(scope + a.out_margin);                             // :623 into getOutOfScopeNodes(std::string, float)
        if (!WRITE && blockIdx.x == 0 && tid == 0) *a.radius_out = scope;
    }
    int before_me = 0;
    if (WRITE) for (int b = 0; b < (int)blockIdx.x; b++) before_me += a.count[b];
    if (tid == 0) s_base = 0;
    __syncthreads();
    const int lo = blockIdx.x * kScanSlab;
    const int hi = lo + kScanSlab < a.n ? lo + kScanSlab : a.n;
    for (int c0 = lo; c0 < hi; c0 += kScanBlk) {
        const int c = c0 + tid;
        bool hit = false;
        if (c < hi) {
            const double dx = a.x[c] - cx, dy = a.y[c] - cy, dz = a.z[c] - cz;
            const double norm = sqrt((dx * dx + dy * dy) + dz * dz);
            if (request) hit = norm > thr;                                                            // slam_graph.cpp:223
            else hit = norm < thr && !((a.have[c >> 5] >> (c & 31)) & 1u);                            // graph_slam_node.cpp:551-553
        }
        const unsigned long long m = __ballot(hit);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) s_wave[wv] = __popcll(m);
        __syncthreads();
        int wave_off = 0, slab = 0;
#pragma unroll
        for (int w = 0; w < kScanBlk / 64; w++) { if (w < wv) wave_off += s_wave[w]; slab += s_wave[w]; }
        const int base = s_base;
        if (WRITE && hit) {
            const int pos = before_me + base + wave_off + before;
            if (pos < a.cap) a.out[pos] = c;
        }
        __syncthreads();
        if (tid == 0) s_base = base + slab;
        __syncthreads();
    }
    if (!WRITE && tid == 0) a.count[blockIdx.x] = s_base;
    if (WRITE && tid == 0 && blockIdx.x == gridDim.x - 1) *a.total = before_me + s_base;
}

// the translations of a solver's pose buffer (8 doubles per node, the translation first: pgo_device.hpp load_pose) as SoA positions
__global__ __launch_bounds__(kScanBlk) void scope_pgo_poses_kernel(const double* __restrict__ pose8, int n, double* __restrict__ x,
                                                                   double* __restrict__ y, double* __restrict__ z)
{
    const int v = blockIdx.x * kScanBlk + threadIdx.x;
    if (v >= n) return;
    const double2 q = *reinterpret_cast<const double2*>(pose8 + (size_t)v * 8);
    x[v] = q.x; y[v] = q.y; z[v] = pose8[(size_t)v * 8 + 2];
}

void launch_scope_sssp(const ScopeArgs& a, hipStream_t s)
{
    if (a.n <= kScopeLdsNodes) hipLaunchKernelGGL(scope_sssp_kernel<true>, dim3(1), dim3(kScopeBlk), 0, s, a);
    else hipLaunchKernelGGL(scope_sssp_kernel<false>, dim3(1), dim3(kScopeBlk), 0, s, a);
}

void launch_scope_scan(const ScopeScanArgs& a, hipStream_t s)
{
    const dim3 grid((a.n + kScanSlab - 1) / kScanSlab);
    hipLaunchKernelGGL(scope_scan_kernel<false>, grid, dim3(kScanBlk), 0, s, a);
    hipLaunchKernelGGL(scope_scan_kernel<true>, grid, dim3(kScanBlk), 0, s, a);
}

void launch_scope_pgo_poses(const double* pose8, int32_t n, double* x, double* y, double* z, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(scope_pgo_poses_kernel, dim3((n + kScanBlk - 1) / kScanBlk), dim3(kScanBlk), 0, s, pose8, n, x, y, z);
}

}  // namespace uzl
