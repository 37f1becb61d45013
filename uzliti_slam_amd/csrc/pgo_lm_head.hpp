// pgo_lm_head.hpp — the body of lm_head_kernel (pgo_lm_kernels.hip), shared with the launch that carries a one-graph pass's PCG init
// beside it (lm_head_init_pcg_kernel, pgo_ml_kernels.hip).  One workgroup of kBlk lanes per graph.  Both files compile it with
// -ffp-contract=off, like every file that shares arithmetic with the host.
#pragma once
#include "pgo_device.hpp"
#include "pgo_lm.hpp"

namespace uzl {

// lane 0 of the head workgroup, on the staged state
__device__ __forceinline__ void lm_head_decide(const LmSlot& S, LmDev* lm, int phase, double chi, double dmax, int pass_flags)
{
    const int p = lm->pass + 1;
    lm->pass = p;
    double* __restrict__ scal = S.D.scal;
    int need = 0;
    if (phase == kLmLin) {
        scal[4] = chi; scal[6] = dmax;
        if (lm->it == 0) {
            lm->chi_cur = chi; lm->chi2_initial = chi;
            lm->lambda = 1e-5 * dmax;                        // computeLambdaInit: tau * max diag
            lm->ni = 2.;
        }
        lm->adopted = lm->pending ? 1 : 0;                   // the copy built during the last iteration
        lm->ix = lm_pass_ix(phase, lm->ix, lm->pending);
        lm->pending = 0;
        if (lm_refresh(lm->it, lm->iterations, lm->sync_rebuild != 0, lm->last_rel, lm->refresh_rel, lm->rate_ref, lm->rate_last, lm->rate_drop)) {
            lm->st_precond_builds++;
            need |= (lm->it == 0 || lm->sync_rebuild) ? (kNeedNumeric | kNeedTrial) : kNeedRebuild;
        }
        lm->qmax = 0;
        if (S.red) lm->schur_pass = p;                       // (H + lambda I) with the chain interiors eliminated: per lambda
    } else if (phase == kLmRetry) {
        if (S.red) lm->schur_pass = p;                       // a rejected step moved lambda: the Schur complement with it
    } else if (phase == kLmNeedSetup) {
        need = lm->need;                                     // (its Schur reduction ran in the pass that stalled)
    } else {
        return;                                              // solving (the pass goes on iterating), done, anomaly
    }
    // ---- start of a trial: setLambda, this trial's PCG floor and step accuracy
    const double lambda = lm->lambda;
    scal[3] = lambda; scal[8] = lm->tol_f2; scal[12] = lm->eps_t; scal[13] = lm->eps_r;
    // the lambda-dependent inverses of the hierarchy are kept across trials; after rejected steps lambda grows geometrically and
    // inverses taken at a much smaller lambda stop being a preconditioner at all
    if (lambda > lm->lambda_retake * lm->lambda_setup[lm->ix]) need |= kNeedTrial;
    if (((need & (kNeedNumeric | kNeedTrial)) && !(pass_flags & kPassSetup)) || ((need & kNeedRebuild) && !(pass_flags & kPassRebuild))) {
        lm->need = need; lm->phase = kLmNeedSetup; lm->flags[0] = 1;              // this pass lacks the segment: the PCG kernels stay no-ops
        return;
    }
    if (need & kNeedRebuild) {                               // into the copy the PCG does not use, with this iteration's lambda; adopted next iteration
        lm->build_pass = p; lm->build_ix = lm->ix ^ 1; lm->build_cur = lm->cur;
        lm->scal2[3] = lambda; lm->lambda_setup[lm->ix ^ 1] = lambda; lm->pending = 1;
    }
    if (need & kNeedNumeric) lm->numeric_pass = p;
    if (need & kNeedTrial) { lm->trial_pass = p; lm->lambda_setup[lm->ix] = lambda; }
    lm->fresh = ((need & kNeedTrial) || (lm->adopted && lm->qmax == 0)) ? 1 : 0;
    lm->need = 0;
    lm->init_pass = p;
    lm->phase = kLmSolve;
    // The solve's done / iterations / breakdown / look words and rz_prev start here, on the staged copy: the PCG init of a one-graph
    // pass may run as further workgroups of this very launch (lm_head_init_pcg_kernel), where a store of theirs into the state would
    // race with the write-back below.  A separate ml_init clears them once more, to the same values.
    lm->flags[0] = 0; lm->flags[1] = 0; lm->flags[2] = 0; lm->flags[3] = 0;
    scal[2] = 1.;
}

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
    if (threadIdx.x == 0) lm_head_decide(S, lm, phase, chi, dmax, pass_flags);
    __syncthreads();
    if ((int)threadIdx.x < kLmWords) reinterpret_cast<unsigned long long*>(S.lm)[threadIdx.x] = reinterpret_cast<const unsigned long long*>(&L)[threadIdx.x];
}

}  // namespace uzl
