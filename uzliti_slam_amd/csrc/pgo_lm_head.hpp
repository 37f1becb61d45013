// pgo_lm_head.hpp — the body of lm_head_kernel (pgo_lm_kernels.hip), shared with the launch that carries a one-graph pass's PCG init
// beside it (lm_head_init_pcg_kernel, pgo_ml_kernels.hip).  One workgroup of kBlk lanes per graph.  Both files compile it with
// -ffp-contract=off, like every file that shares arithmetic with the host.
#pragma once
#include "pgo_device.hpp"
#include "pgo_lm.hpp"

namespace uzl {

// one workgroup per graph: the state staged in LDS, the sums of a fresh linearisation, lane 0 decides (pgo_lm.hpp: lm_head_decide), write-back
__device__ __forceinline__ void lm_head_body(const LmSlot& S, int pass_flags)
{
    __shared__ double s4[4];
    __shared__ LmDev L;                                      // the state, staged: lane 0's decisions are a chain of reads and writes of its
                                                             // fields, each a round trip to memory when taken from the global copy
    LmDev* lm = &L;
    constexpr int kLmWords = (int)(sizeof(LmDev) / 8);
    static_assert(sizeof(LmDev) % 8 == 0 && kLmWords <= kBlk, "LmDev is copied as 8-byte words");
    if ((int)threadIdx.x < kLmWords) reinterpret_cast<unsigned long long*>(&L)[threadIdx.x] = reinterpret_cast<const unsigned long long*>(S.lm)[threadIdx.x];
    __syncthreads();
    const int phase = lm->phase;
    double chi = 0., dmax = 0.;
    if (phase == kLmLin) {                                   // (uniform) finalize_kernel(what = 2): chi2 + max diagonal
        chi = sum_partials(S.D.part_a, S.g_edges, s4);
        double v = 0.;
        for (int i = threadIdx.x; i < S.g_asm; i += kBlk) v = fmax(v, S.D.part_c[i]);
        dmax = block_max(v, s4);
    }
    if (threadIdx.x == 0) lm_head_decide(lm, S.D.scal, S.red, phase, chi, dmax, pass_flags);
    __syncthreads();
    if ((int)threadIdx.x < kLmWords) reinterpret_cast<unsigned long long*>(S.lm)[threadIdx.x] = reinterpret_cast<const unsigned long long*>(&L)[threadIdx.x];
}

}  // namespace uzl
