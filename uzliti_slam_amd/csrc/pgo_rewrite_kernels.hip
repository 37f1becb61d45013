// pgo_rewrite_kernels.hip — the device half of uzl_pgo_rewrite_graph: the resident input edges (608-byte uzl_edge records) and the current
// estimates compacted through the index maps of rewrite_plan (pgo_structure.hpp), out of place into the handle's spare buffers.
//
// Compiled with -ffp-contract=off (the Makefile's default flags, unlike pgo_kernels.hip): a displacement that takes a left multiplier
// must come out with the bits of uzliti_slam_amd.merge._compose, so that a rewritten handle equals uzl_pgo_add_graph of the arrays the
// host rewrite makes -
//     rotation entry     (a0*b0 + a1*b1) + a2*b2
//     translation entry  ((a0*B3 + a1*B7) + a2*B11) + a3
// with every product and sum rounded on its own.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstddef>
#include <cstdint>

#include "uzl_common.hpp"
#include "pgo_rewrite.hpp"

namespace uzl {

static_assert(sizeof(uzl_edge) == 608, "a uzl_edge is 38 pieces of 16 bytes: records in an array are 16-byte aligned");
static_assert(offsetof(uzl_edge, from) == 0 && offsetof(uzl_edge, to) == 4, "lane 0's piece starts with the two endpoints");
static_assert(offsetof(uzl_edge, displacement_from) == 8 * kRwWordFrom && offsetof(uzl_edge, displacement_to) == 8 * kRwWordTo,
              "the displacements as 8-byte words of the record");
constexpr int kRwPieces = (int)(sizeof(uzl_edge) / 16);

// One wave per surviving edge k: lanes 0-37 each move one 16-byte piece of d_edges[new_to_old[k]] to out[k] (one coalesced 608-byte read,
// one coalesced write).  In between, the lanes that hold words of a touched displacement replace them with xf * displacement - the
// operands come from the other lanes' registers - and lane 0 patches the endpoints.
// rec[k] = {from_new, to_new, xf_from, xf_to} (RewriteEdge; -1: that side is untouched); xf: [.][12] row-major [R|t].
__global__ __launch_bounds__(kRwBlock) void rewrite_edges_kernel(const uzl_edge* __restrict__ in, uzl_edge* __restrict__ out,
                                                                 const int32_t* __restrict__ new_to_old, const int4* __restrict__ rec,
                                                                 int e_new, const double* __restrict__ xf)
{
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (kRwBlock / 64) + (threadIdx.x >> 6);
    if (k >= e_new) return;                                             // (the whole wave)
    const int4 r = rec[k];
    const bool mine = lane < kRwPieces;
    int4 p = make_int4(0, 0, 0, 0);
    if (mine) p = reinterpret_cast<const int4*>(in + new_to_old[k])[lane];
    if (r.z >= 0 || r.w >= 0) {                                        // (wave-uniform)
        const double lo = __hiloint2double(p.y, p.x), hi = __hiloint2double(p.w, p.z);          // words 2 lane, 2 lane + 1 of the record
        double w2[2] = {lo, hi};
#pragma unroll
        for (int half = 0; half < 2; half++) {
            const int w = 2 * lane + half;
            const bool on_from = w >= kRwWordFrom && w < kRwWordFrom + 12, on_to = w >= kRwWordTo && w < kRwWordTo + 12;
            const int ix = on_from ? r.z : (on_to ? r.w : -1);
            const bool touched = ix >= 0;
            const int base = on_to ? kRwWordTo : kRwWordFrom;
            const int idx = touched ? w - base : 0, row = idx >> 2, col = idx & 3;
            double b[3];
#pragma unroll
            for (int q = 0; q < 3; q++) {                               // B[col], B[4 + col], B[8 + col]: every lane takes part in the exchange
                const int src = base + col + 4 * q;
                const double vlo = __shfl(lo, src >> 1), vhi = __shfl(hi, src >> 1);
                b[q] = (src & 1) ? vhi : vlo;
            }
            if (touched) {
                const double* __restrict__ A = xf + 12 * (size_t)ix + 4 * row;
                double v = (A[0] * b[0] + A[1] * b[1]) + A[2] * b[2];
                if (col == 3) v = v + A[3];
                w2[half] = v;
            }
        }
        p.x = __double2loint(w2[0]); p.y = __double2hiint(w2[0]);
        p.z = __double2loint(w2[1]); p.w = __double2hiint(w2[1]);
    }
    if (lane == 0) { p.x = r.x; p.y = r.y; }
    if (mine) reinterpret_cast<int4*>(out + k)[lane] = p;
}

// The estimates of the surviving nodes, 8 doubles each, gathered into the other pose buffer: src[v] >= 0 names the old node whose
// estimate node v keeps bit for bit, src[v] < 0 the row ~src[v] of `placed` - a pose_nodes entry as prepare_nodes_kernel prepared it.
// One lane per 16-byte piece.
__global__ __launch_bounds__(kRwBlock) void rewrite_nodes_kernel(const double* __restrict__ cur, const double* __restrict__ placed,
                                                                 const int32_t* __restrict__ src, int n_new, double* __restrict__ out)
{
    const int i = blockIdx.x * kRwBlock + threadIdx.x;
    const int v = i >> 2, piece = i & 3;
    if (v >= n_new) return;
    const int s = src[v];
    const double2* from = reinterpret_cast<const double2*>(s >= 0 ? cur + (size_t)s * 8 : placed + (size_t)(~s) * 8);
    reinterpret_cast<double2*>(out + (size_t)v * 8)[piece] = from[piece];
}

void k_rewrite_edges(const uzl_edge* in, uzl_edge* out, const int32_t* new_to_old, const int32_t* rec, int e_new, const double* xf, hipStream_t s,
                     hipEvent_t ev_a, hipEvent_t ev_b)
{
    if (e_new <= 0) return;
    const dim3 grid((e_new + kRwBlock / 64 - 1) / (kRwBlock / 64));
    if (ev_a) hipExtLaunchKernelGGL(rewrite_edges_kernel, grid, dim3(kRwBlock), 0, s, ev_a, ev_b, 0, in, out, new_to_old, reinterpret_cast<const int4*>(rec), e_new, xf);
    else hipLaunchKernelGGL(rewrite_edges_kernel, grid, dim3(kRwBlock), 0, s, in, out, new_to_old, reinterpret_cast<const int4*>(rec), e_new, xf);
}
void k_rewrite_nodes(const double* cur, const double* placed, const int32_t* src, int n_new, double* out, hipStream_t s, hipEvent_t ev_a, hipEvent_t ev_b)
{
    if (n_new <= 0) return;
    const dim3 grid((4 * n_new + kRwBlock - 1) / kRwBlock);
    if (ev_a) hipExtLaunchKernelGGL(rewrite_nodes_kernel, grid, dim3(kRwBlock), 0, s, ev_a, ev_b, 0, cur, placed, src, n_new, out);
    else hipLaunchKernelGGL(rewrite_nodes_kernel, grid, dim3(kRwBlock), 0, s, cur, placed, src, n_new, out);
}
}  // namespace uzl
