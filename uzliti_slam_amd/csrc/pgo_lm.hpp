// pgo_lm.hpp — the Levenberg-Marquardt loop's STATE MACHINE, written once: g2o's OptimizationAlgorithmLevenberg::solve [EXT], which the
// reference runs through optimizer_.optimize(iterations) (graph_optimization/src/g2o_optimizer.cpp:148), as functions over an LmDev
// (pgo_types.hpp) and the solve's scalar array.  One state machine, two drivers: lane 0 of lm_head_kernel / lm_tail_kernel
// (pgo_lm_head.hpp, pgo_lm_kernels.hip) applies it to the state on the device, do_optimize_host (uzl_pgo.hip) to a state on the host, and
// uzl_debug_lm_decide (uzl_pgo_debug.hip) to a state a CPU test wrote (tests/test_lm_decide.py).
//   lm_head_decide   in front of a trial: lambda_0, adoption of a copy rebuilt ahead, lazy refresh, the lambda-retake rule, `fresh`, the
//                    stamps (*_pass == pass) that say which segments this pass runs, or a stall for a segment the pass lacks
//   lm_solve_verdict over a solve the PCG kernels have left: stands / still iterating / which anomaly
//   lm_trial_decide  over an evaluated trial: counters, PCG rate, rho, accept / reject, retry / next iteration / done / Terminate
//   lm_tail_decide   the two as lm_tail_kernel's lane 0 applies them
// Both drivers must take the SAME decisions from the same numbers - tests hold their poses to array_equal - so nothing here may depend
// on who compiles it: no contraction of a * b + c, no library pow / log whose last bit differs between libm and the device library.
#pragma once
#include <cmath>
#include <hip/hip_runtime.h>

#include "pgo_types.hpp"

namespace uzl {

#define UZL_HD __host__ __device__ __forceinline__

// |r|^2 / |b|^2 a solve under the multiplicative operator must reach (DESIGN.md "Safeguards"); the stop test lets a solve go at 0.2
constexpr double kResidualGuard = 0.25;
// a kept preconditioner is rebuilt when its contraction per PCG iteration has fallen below this share of what it delivered when fresh
constexpr double kRateDrop = 0.6;
// factor on pcg_tol^2 of the relative floor under the step-error stop test (scal[8])
constexpr double kTolFloor2 = 1e-4;
// step accuracy asked of a solve, per unit of cfg.pcg_tol: metres, and quaternion-vector units (~ half radians)
constexpr double kStepT = 1.0, kStepR = 0.1;

// t^3 rounded once (g2o: pow(2 rho - 1, 3)): the product is carried exactly in two doubles and summed at the end.  Correctly rounded
// up to a second-order term far below half an ulp; the same bits from x86 and gfx950, which libm's and the device library's pow are not.
UZL_HD double lm_cube(double t)
{
#pragma clang fp contract(off)
    const double p = t * t, pe = fma(t, t, -p);          // t^2 = p + pe
    const double q = p * t, qe = fma(p, t, -q);          // p t = q + qe
    return q + (qe + pe * t);
}

// ln(x) for x > 0 from exponent + atanh series: plain arithmetic, identical on both sides.  Only ratios of such logs are compared
// (pcg_rate), so 1e-15 relative accuracy is ample.
UZL_HD double lm_log(double x)
{
#pragma clang fp contract(off)
    if (!(x < 1e300)) return 690.77552789821368;         // (ln 1e300: an overflowed ratio, or not a number; nothing compares that finely)
    if (!(x > 1e-300)) return -690.77552789821368;
    int e = 0;
    double m = x;
    // frexp by hand: scale into [sqrt(1/2), sqrt(2))
    while (m >= 1.4142135623730951) { m *= 0.5; e++; }
    while (m < 0.70710678118654757) { m *= 2.0; e--; }
    const double s = (m - 1.) / (m + 1.), s2 = s * s;
    double term = s, sum = 0.;
    for (int k = 1; k < 60; k += 2) {
        sum += term / k;
        term *= s2;
        if (term < 1e-20 && term > -1e-20) break;
    }
    return 2. * sum + e * 0.69314718055994529;
}

// How stale is a kept preconditioner?  The CONTRACTION it delivers, nats of r.M^-1 r per PCG iteration (rz_stop = scal[1] is
// pcg_tol^2 * tol_f2 * (r_0.M^-1 r_0)); -1 = no estimate (too few iterations).
UZL_HD double lm_pcg_rate(double rz_stop, double rz_end, int its, double tol2, double tol_f2)
{
#pragma clang fp contract(off)
    const double rz0 = rz_stop / (tol2 * tol_f2);
    return (its >= 16 && rz0 > 0. && rz_end > 0. && rz_end < rz0) ? lm_log(rz0 / rz_end) / its : -1.;
}

// does this linearisation rebuild the multilevel preconditioner?  (lazy refresh)
UZL_HD bool lm_refresh(int it, int iterations, bool may_run_last, double last_rel, double refresh_rel, double rate_ref, double rate_last,
                       double rate_drop = kRateDrop)
{
#pragma clang fp contract(off)
    return it == 0 || ((last_rel > refresh_rel || (rate_ref > 0. && rate_last > 0. && rate_last < rate_drop * rate_ref)) &&
                       (may_run_last || it + 1 < iterations));
}

// The hierarchy copy a graph's PCG applies in the pass that finds it in this state: a copy that was rebuilt ahead is adopted when the
// pass linearises, and at no other time.  lm_head_kernel moves LmDev::ix by this rule; the host applies it to the snapshot it holds
// before it enqueues the pass, and hands the small-graph class's PCG launches the result by value (pgo_types.hpp: PcgArgs).
UZL_HD int lm_pass_ix(int phase, int ix, int pending) { return (phase == kLmLin && pending) ? (ix ^ 1) : ix; }

// the step control of one evaluated trial: rho from chi2 before / after and computeScale() + 1e-3; updates lambda, ni; returns rho
struct LmStep { double rho; bool accepted; double last_rel; };
UZL_HD LmStep lm_step(double current_chi, double temp_chi, double scale_sum, double& lambda, double& ni)
{
#pragma clang fp contract(off)
    LmStep r;
    const double scale = scale_sum + 1e-3;                                       // computeScale + 1e-3
    r.rho = (current_chi - temp_chi) / scale;
    r.accepted = r.rho > 0 && std::isfinite(temp_chi);
    r.last_rel = 0.;
    if (r.accepted) {                                                            // good step
        double alpha = 1. - lm_cube(2 * r.rho - 1);
        alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
        const double scaleFactor = (1. / 3. > alpha) ? 1. / 3. : alpha;
        lambda *= scaleFactor;
        ni = 2.;
        const double at = temp_chi < 0 ? -temp_chi : temp_chi, d = current_chi - temp_chi;
        r.last_rel = (d < 0 ? -d : d) / (at > 1e-300 ? at : 1e-300);
    } else {
        lambda *= ni;
        ni *= 2.;
    }
    return r;
}

// ---- in front of a trial.  phase: the state's phase when the pass found it; chi, dmax: chi2 and the largest diagonal entry of a fresh
//      linearisation (read in phase kLmLin only); red: the PCG solves a Schur complement; pass_flags: the segments the pass can run
//      (LmPassFlags).  scal: PgoDev::scal of the graph, or the host driver's image of it.
UZL_HD void lm_head_decide(LmDev* lm, double* __restrict__ scal, int red, int phase, double chi, double dmax, int pass_flags)
{
    const int p = lm->pass + 1;
    lm->pass = p;
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
        if (red) lm->schur_pass = p;                         // (H + lambda I) with the chain interiors eliminated: per lambda
    } else if (phase == kLmRetry) {
        if (red) lm->schur_pass = p;                         // a rejected step moved lambda: the Schur complement with it
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
    // The solve's done / iterations / breakdown / look words and rz_prev start here, on the driver's copy of the state: the PCG init of a
    // one-graph pass may run as further workgroups of the head's launch (lm_head_init_pcg_kernel), where a store of theirs into the
    // state would race with the head's write-back.  A separate ml_init clears them once more, to the same values.
    lm->flags[0] = 0; lm->flags[1] = 0; lm->flags[2] = 0; lm->flags[3] = 0;
    scal[2] = 1.;
}

// ---- behind a trial's solve, on what the PCG kernels left in LmDev::flags (0 done, 1 iterations, 2 breakdown) and the residual guard's
//      |r|^2 / |b|^2.  The device-resident loop hands a graph with an anomaly to the host-driven one, which knows the remedies (retake
//      the inverses, additive operator) and evaluates the trial whatever the verdict.
enum LmVerdict : int32_t {
    kLmIterating = -1,        // the solve goes on in the next pass
    kLmSolved = 0,            // converged, and inside the residual guard where the operator needs one
    kLmAnomalyCap = 1,        // the PCG hit its cap (LmDev::max_it)
    kLmAnomalyBreakdown = 2,  // PCG breakdown
    kLmAnomalyGuard = 3,      // DESIGN.md "Safeguards": the multiplicative operator is not SPD by construction
    kLmAnomalyIx = 4          // PcgArgs::ix was not the state's (kBreakdownIx)
};
UZL_HD int lm_solve_verdict(const LmDev* lm, double ratio)
{
    if (!lm->flags[0]) return lm->flags[1] >= lm->max_it ? kLmAnomalyCap : kLmIterating;
    if (lm->flags[2]) return lm->flags[2] == kBreakdownIx ? kLmAnomalyIx : kLmAnomalyBreakdown;
    return (lm->guarded && !(ratio <= kResidualGuard)) ? kLmAnomalyGuard : kLmSolved;
}

// ---- over an evaluated trial: chi_t, sc = chi2 at the trial poses and computeScale; scal[0], scal[1] = r.M^-1 r at the solve's end and
//      its stop threshold, LmDev::flags[1] = the solve's PCG iterations
UZL_HD void lm_trial_decide(LmDev* lm, double* __restrict__ scal, double chi_t, double sc)
{
    const int its = lm->flags[1];
    scal[4] = chi_t; scal[5] = sc;
    lm->st_pcg_iterations += its; lm->st_lm_trials++; lm->pcg_last = its;
    const double rate = lm_pcg_rate(scal[1], scal[0], its, lm->tol2, lm->tol_f2);
    if (rate > 0.) { lm->rate_last = rate; if (lm->fresh || lm->rate_ref < 0.) lm->rate_ref = rate; }
    double lambda = lm->lambda, ni = lm->ni;
    const LmStep st = lm_step(lm->chi_cur, chi_t, sc, lambda, ni);
    lm->lambda = lambda; lm->ni = ni;
    if (st.accepted) { lm->last_rel = st.last_rel; lm->chi_cur = chi_t; lm->cur ^= 1; }      // discardTop
    const int qmax = lm->qmax + 1;
    lm->qmax = qmax;
    if (st.rho < 0 && qmax < 10) lm->phase = kLmRetry;                    // another trial on the same linearisation
    else {
        lm->st_iterations_done = lm->it + 1;
        if (qmax == 10 || st.rho == 0) { lm->st_terminated_early = 1; lm->phase = kLmDone; }      // Terminate
        else { lm->it += 1; lm->qmax = 0; lm->phase = (lm->it >= lm->iterations) ? kLmDone : kLmLin; }
    }
}

// ---- lane 0 of lm_tail_kernel: the verdict, and the decision over the trial when the solve stands.  ratio, chi_t, sc: read only
//      when the pass's evaluation kernels ran for the graph (solving, done, no breakdown); scal[7] = ratio then
UZL_HD void lm_tail_decide(LmDev* lm, double* __restrict__ scal, double chi_t, double sc, double ratio)
{
    if (lm->phase != kLmSolve) return;
    const int verdict = lm_solve_verdict(lm, ratio);
    if (verdict == kLmSolved || verdict == kLmAnomalyGuard) scal[7] = ratio;
    if (verdict > kLmSolved) { lm->phase = kLmAnomaly; lm->anomaly_code = verdict; lm->flags[0] = 1; }
    else if (verdict == kLmSolved) lm_trial_decide(lm, scal, chi_t, sc);
}

}  // namespace uzl
