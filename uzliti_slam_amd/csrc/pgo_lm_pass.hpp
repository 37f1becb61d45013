// pgo_lm_pass.hpp — what the HOST predicts about the next pass of the device-resident Levenberg-Marquardt loop (uzl_pgo_lm.hip), as
// plain values: which segments the pass carries, how many PCG iterations it holds and how they split into launches, which hierarchy
// copy its PCG applies - and the batch sizes of the host-driven loop's solve (uzl_pgo.hip: pcg_solve), the same kind of rule.
// Predictions only: the DEVICE takes every decision from the graph's own state, so a slip here never changes a result - it costs
// passes, 50 - 100 us each.  Host integer work: no HIP call, no handle, no allocation per pass.  tests/test_lm_pass_plan.py holds every
// rule on the CPU through uzl_debug_lm_pass_plan (uzl_pgo_debug.hip) against tests/lm_pass_reference.py.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "pgo_lm.hpp"

namespace uzl {

constexpr double kLambdaRetake = 32.;                 // lambda grown by this factor since the inverses were taken: take them again
constexpr int kGraphPairs = 8;                        // one long PCG replay = 2 x kGraphPairs iterations
constexpr int kShortPairs = 2;                        // ... a short one 2 x kShortPairs
constexpr int kPcgStep = 2 * kShortPairs, kPcgLong = 2 * kGraphPairs;

// Newton-Schulz steps of a synchronous set-up at LM iteration `it` for a structure that asks for `structure_steps` (4 on large loopy
// graphs): 2 in the first kNsEarlyIts iterations (against the full count from the start: -3.4 % over fourteen large shapes at the same
// PCG iteration count; 4 iterations instead of 2 gain on the largest and lose at 10k, 8 lose everywhere; NO step at all in those two - the
// cycle's operator as it comes - another -2.5 %, not taken: that operator is what the residual guard exists for)
inline int ml_ns_steps_at(int structure_steps, int it)
{
    constexpr int kNsEarlyIts = 2, kNsEarlySteps = 2;
    return (structure_steps > 2 && it < kNsEarlyIts) ? kNsEarlySteps : structure_steps;
}

// ---- what the host reads of a snapshot: the contract between lm_tail_kernel's LmHost and the predictions below
struct LmPlanView {
    // (the hook's integer row, in this order)
    int32_t phase, need, it, iterations, sync_rebuild, pending, ix, pcg_last, st_lm_trials, max_it;
    int32_t pcg_its;                                  // LmDev::flags[1]: PCG iterations of the running solve
    // (its double row)
    double last_rel, refresh_rel, rate_ref, rate_last, rate_drop, lambda, lambda_setup[2], tol2;
};
constexpr int kPlanViewInts = 11, kPlanViewDoubles = 9;
inline LmPlanView lm_plan_view(const LmDev& v)
{
    return {v.phase, v.need, v.it, v.iterations, v.sync_rebuild, v.pending, v.ix, v.pcg_last, v.st_lm_trials, v.max_it, v.flags[1],
            v.last_rel, v.refresh_rel, v.rate_ref, v.rate_last, v.rate_drop, v.lambda, {v.lambda_setup[0], v.lambda_setup[1]}, v.tol2};
}

// ---- PCG iterations of every trial of the last drive's jobs and of the running one's.  A re-optimisation of an unchanged graph
// (uzl_pgo_reset, a timer-driven one) walks through much the same solves, trial for trial: where the count RISES from one trial to the
// next (config 2: 24 -> 40 iterations from the first trial to the second) the last solve alone under-predicts and the solve needs a second
// and third pass (tail, look and a fresh launch sequence each)
struct LmPassHistory {
    int first_solve_its = 0;                 // PCG iterations of the first solve of the last optimize (sizes the first pass of the next)
    std::vector<std::vector<int>> trial_its_prev, trial_its_cur;      // [job][trial]
    std::vector<uint64_t> hist_gen;          // structure generation of every job the counts belong to (a batch: its graphs in order)
};
// start of a drive over jobs of structure generations gen[0..Q): the last drive's counts are this drive's history where every job is
// the same structure again
inline void lm_history_begin(LmPassHistory& H, const uint64_t* gen, int Q)
{
    if (H.hist_gen.size() == (size_t)Q && std::equal(gen, gen + Q, H.hist_gen.begin())) H.trial_its_prev.swap(H.trial_its_cur);
    else H.trial_its_prev.clear();
    H.trial_its_prev.resize((size_t)Q);
    H.trial_its_cur.assign((size_t)Q, std::vector<int>());
    H.hist_gen.assign(gen, gen + Q);
}

// ---- what the predictor remembers of a slot between passes
struct LmSlotTrack {
    int job = -1;                            // the job in the slot (-1: idle - every kernel no-ops on its state)
    bool active = false;                     // ... and not through yet (a finished graph waits in its slot for its cohort)
    // uzl_pgo_cfg::pass_history = 1: nothing an earlier optimize of this handle learned sizes a pass (the first solve starts with two
    // long replays, every later one follows its predecessor in the same optimize)
    bool no_history = false;
    const int* hist = nullptr;               // the job's row of LmPassHistory::trial_its_prev (fixed for the drive)
    int n_hist = 0;
    int solve_passes = 0;                    // continuation passes of the running solve so far
    int prev_last = 0, cur_last = 0;         // PCG counts of the last two trials that ended
    int seen_trials = 0;
};
inline void lm_track_load(LmSlotTrack& T, int job, bool no_history, const LmPassHistory& H)
{
    T = LmSlotTrack();
    T.job = job; T.active = job >= 0; T.no_history = no_history;
    if (job >= 0) { T.hist = H.trial_its_prev[(size_t)job].data(); T.n_hist = (int)H.trial_its_prev[(size_t)job].size(); }
}
// the look's bookkeeping: a slot's new snapshot into its track and the run's history; true when its graph is through
inline bool lm_track_look(const LmPlanView& v, LmSlotTrack& T, LmPassHistory& H)
{
    if (v.st_lm_trials > T.seen_trials) { T.seen_trials = v.st_lm_trials; T.prev_last = T.cur_last; T.cur_last = v.pcg_last; }      // a trial ended: its count and the one before
    if (v.st_lm_trials == 1 && v.pcg_last > 0 && T.job == 0) H.first_solve_its = v.pcg_last;
    std::vector<int>& cur = H.trial_its_cur[(size_t)T.job];
    if (v.st_lm_trials > 0 && (size_t)v.st_lm_trials > cur.size()) cur.resize((size_t)v.st_lm_trials, v.pcg_last);
    if (v.phase == kLmDone || v.phase == kLmAnomaly) T.active = false;
    return !T.active;
}

// ---- the next pass
struct LmPassPlan {
    int flags = 0;                           // LmPassFlags: the segments it carries
    int want = 0, base = 0;                  // PCG iterations it holds; iteration index of the first
    int ix = 0;                              // the hierarchy copy a one-graph pass applies
    int ns_steps = 0;                        // Newton-Schulz steps of its set-up segment
    bool setup_captured = false;             // ... which is the captured segment's sequence (else: launched as it is)
    bool any_start = false;                  // some graph starts a trial: the pass has a head and an init
    double tol2 = 0.;                        // pcg_tol^2 of a one-graph pass
};
// Predictions from the slots' last snapshots.  first_solve_its: LmPassHistory's; shape_ns_steps: LmShape::ns_steps; wrong_ix: the
// diagnostic build's UZL_LM_WRONG_IX (the other hierarchy copy)
inline LmPassPlan lm_plan_pass(const LmPlanView* views, LmSlotTrack* tracks, int nS, int first_solve_its, int shape_ns_steps, bool wrong_ix)
{
    LmPassPlan P;
    // One graph: exactly count + 1 launches (odd or even; a continuation pass picks the parity up from the solve's own
    // iteration count).  A batch keeps whole pairs: its graphs share the launches' parity.
    auto up = [nS](int count) { return nS == 1 ? count + 1 : ((count + 2) & ~1); };
    for (int sl = 0; sl < nS; sl++) {
        LmSlotTrack& T = tracks[sl];
        if (!T.active) continue;             // (idle, or a finished graph waiting for its cohort)
        const LmPlanView& v = views[sl];
        int w;
        if (v.phase == kLmSolve) {
            // A solve that outlasted its pass.  Nothing says how much longer it takes, but a launch past the end is a 1.2-us no-op
            // and another pass is 50 - 100 us of tail, look and restart: a short batch, then half of what the solve has taken so far (round
            // 4: two batches of 4, then 16s - config 2's second trial, 48 iterations against 30 predicted, took four passes; now three)
            w = T.solve_passes == 0 ? kPcgStep : std::min(std::max(kPcgStep, (v.pcg_its / 2 + 1) & ~1), 4 * kPcgLong);      // (most often it was one launch short: a short batch first)
            T.solve_passes++;
        } else {
            P.any_start = true; T.solve_passes = 0;
            if (v.phase == kLmNeedSetup) P.flags |= ((v.need & (kNeedNumeric | kNeedTrial)) ? kPassSetup : 0) | ((v.need & kNeedRebuild) ? kPassRebuild : 0);
            else if (v.phase == kLmLin) {
                if (lm_refresh(v.it, v.iterations, v.sync_rebuild != 0, v.last_rel, v.refresh_rel, v.rate_ref, v.rate_last, v.rate_drop))
                    P.flags |= (v.it == 0 || v.sync_rebuild) ? kPassSetup : kPassRebuild;
                if (v.it > 0 && v.lambda > kLambdaRetake * v.lambda_setup[v.ix ^ (v.pending ? 1 : 0)]) P.flags |= kPassSetup;
            } else if (v.phase == kLmRetry) {
                if (v.lambda > kLambdaRetake * v.lambda_setup[v.ix]) P.flags |= kPassSetup;
            }
            // The solve's length: the previous solve's count + 1 (a solve that the stop test ends after k iterations is declared done by
            // the ml_spmv of iteration k + 1): too many is a ~3.5-us no-op per launch, too few another pass.  The
            // first solve of an optimize has no predecessor: the first solve of the last optimize stands in (same structure or a grown
            // one: a re-optimisation), a fresh run starts with two long replays.
            w = v.pcg_last > 0 ? up(v.pcg_last) : ((first_solve_its > 0 && !T.no_history) ? up(first_solve_its) : 2 * kPcgLong);
            // counts that RISE from trial to trial (lambda falls after accepted steps, the system gets harder: chain-like graphs climb by 2
            // per trial for ten trials, each time one launch short of `last + 2`): extrapolate the last rise
            if (v.pcg_last > 0 && T.prev_last > 0 && v.pcg_last > T.prev_last) w = up(v.pcg_last + std::min(v.pcg_last - T.prev_last, 16));
            if (!T.no_history && v.st_lm_trials >= 0 && v.st_lm_trials < T.n_hist) w = std::max(w, up(T.hist[v.st_lm_trials]));
            w = std::min(w, ((v.max_it + 1) & ~1));
        }
        P.want = std::max(P.want, w);
    }
    P.want = std::max(2, P.want);
    // iteration index of the pass's first PCG launch: a single graph's continuation goes on where its solve stands (its count may be
    // odd); in a batch every pass holds whole pairs, so every solve stands at an even count
    P.base = (nS == 1 && tracks[0].job >= 0 && views[0].phase == kLmSolve) ? views[0].pcg_its : 0;
    // the hierarchy copy a one-graph pass applies: lm_head_kernel's rule on the snapshot this pass starts from (the kernels hold it
    // against LmDev::ix and end the solve as an anomaly if it is not the state's)
    P.ix = lm_pass_ix(views[0].phase, views[0].ix, views[0].pending) ^ (wrong_ix ? 1 : 0);
    P.tol2 = views[0].tol2;
    // The synchronous set-ups of the first kNsEarlyIts linearisations refine the dense operator with two Newton-Schulz steps where the
    // structure asks for four (large loopy graphs): the problem still changes wholesale there and a rougher operator costs no PCG
    // iterations (ml_ns_steps_at).  Launched as they are - the captured segment holds the full sequence.
    P.ns_steps = nS == 1 ? ml_ns_steps_at(shape_ns_steps, views[0].it) : shape_ns_steps;
    P.setup_captured = P.ns_steps == shape_ns_steps;
    return P;
}

// Does the PCG init of this pass go out as further workgroups of the head's launch (lm_head_init_pcg_kernel) instead of a launch of
// its own?  pcg_args_pass: one graph of the small-graph class, launched by value (PcgArgs); reduced: its PCG solves the Schur complement.
// Not with a synchronous set-up in the pass - it rewrites the geometry of the hierarchy copy in use behind the head, and the init reads
// it - and not on a reduced system, whose right-hand side the reduction behind the head makes.  (A rebuild runs on the other copy.)
inline bool lm_init_rides(const LmPassPlan& P, bool pcg_args_pass, bool reduced)
{
    return P.any_start && !(P.flags & kPassSetup) && pcg_args_pass && !reduced;
}

// How a pass's `want` iterations from index `base` go out: short solves are launched kernel by kernel, long ones as captured replays of
// kPcgLong iterations plus a remainder.  The captured replay starts at an even iteration: one single launch in front where base is odd.
struct LmPcgLaunches {
    int lead;                                // 1: one launch of iteration `base` in front
    int long_first, n_long;                  // replays of kPcgLong iterations from this (even) index on
    int rem_first, rem;                      // the remainder, launched as it is
};
inline LmPcgLaunches lm_pcg_launches(int base, int want, bool eager)
{
    LmPcgLaunches L;
    L.lead = (!eager && (base & 1)) ? 1 : 0;
    L.long_first = base + L.lead;
    L.n_long = eager ? 0 : (want - L.lead) / kPcgLong;
    L.rem_first = L.long_first + L.n_long * kPcgLong;
    L.rem = want - L.lead - L.n_long * kPcgLong;
    return L;
}

// The host-driven loop's solve (pcg_solve) launches in batches and looks after each: the first sized from the previous solve - 95 % of
// its count, + 1: a solve that ends by the stop test after k iterations is declared done by the ml_spmv of iteration k + 1 - in steps
// of kPcgStep iterations (none: one long replay), then two short ones, then long ones; never past max_it by more than the rounding.
// The kernels no-op once `done` is set.
inline int lm_host_batch(int round, int prev_pcg_iters, int max_it, int launched)
{
    constexpr int kFirstPct = 95;
    auto round_up = [](int v) { return ((v + kPcgStep - 1) / kPcgStep) * kPcgStep; };
    const int ask = round > 2 ? kPcgLong : round > 0 ? kPcgStep : prev_pcg_iters > 0 ? std::max(kPcgStep, round_up((prev_pcg_iters * kFirstPct) / 100 + 1)) : kPcgLong;
    return round_up(std::max(1, std::min(ask, max_it - launched)));
}

}  // namespace uzl
