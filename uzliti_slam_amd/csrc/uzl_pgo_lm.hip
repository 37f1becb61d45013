// uzl_pgo_lm.hip — the device-resident Levenberg-Marquardt loop behind uzl_pgo_optimize and uzl_pgo_batch_optimize.
//
// G2oOptimizer::optimizeImpl (graph_optimization/src/g2o_optimizer.cpp:137-149) hands the graph to optimizer_.optimize(iterations),
// i.e. g2o's OptimizationAlgorithmLevenberg::solve [EXT]: linearise, then trials (lambda, solve, evaluate, accept / reject) until a step
// is accepted.  That loop is ONE STATE MACHINE - lm_head_decide / lm_tail_decide over an LmDev, pgo_lm.hpp - WITH TWO DRIVERS.
// uzl_pgo.hip's do_optimize_host keeps the state on the host and launches what it stamps, scalar round trip by scalar round trip.  Here
// the state lives on the device, lane 0 of two one-workgroup kernels applies the same two functions to it (pgo_lm_kernels.hip), every
// other kernel is a slot twin that predicates itself on that state, and one trial is a PASS, a fixed sequence of segments:
//     head  = linearise, assemble | lm_head (chi2, lambda_0, adoption, refresh decision, setLambda) | [Schur reduction]
//     setup = numeric + trial part of the hierarchy copy in use        (first iteration; synchronous rebuilds; lambda grown 32x)
//     reb   = rebuild of the OTHER copy on the second stream           (lazy refresh: adopted by the next iteration)
//     init  = x = 0, r = b, first application of the preconditioner  (x = 0, r = b of one small graph: workgroups of the head's launch,
//             unless the pass has a set-up segment or the system is Schur-reduced - lm_init_rides, pgo_lm_pass.hpp)
//     pcg   = K iterations                                             (no-ops once the solve's `done` flag is set)
//     tail  = [back-substitution], retraction, chi2 | lm_tail (residual guard, rho, accept / reject, next phase, snapshot for the host)
// The host enqueues a pass, looks at the snapshot ONCE, and chooses the next pass's segments and K from it (lm_plan_pass,
// pgo_lm_pass.hpp: every rule of that choice, as a value the CPU tests hold).  Its choices are predictions only: lm_head stalls a graph whose pass lacks a segment it needs (kLmNeedSetup) and the next pass brings it; a solve that outlasts
// its pass goes on in the next.  The DEVICE takes every decision from the graph's own state, so results do not depend on what the host
// guessed.  Same kernel bodies, same order of operations, the very same decisions (pgo_lm.hpp) as the host-driven loop: tests hold the
// two to array_equal poses, and both start from lm_initial_state below.
//
// One driver serves one graph (uzl_pgo_optimize) and many (uzl_pgo_batch_optimize): R slots, blockIdx.z = slot, a queue of graphs
// behind them.  Graphs in different phases of their loops share the launches of a pass - none waits for another's trial count - and a
// slot whose graph is through takes the next one of the queue.  The host-driven loop remains for sharded and profiled single solves
// and block-Jacobi, and takes a graph over - from its start poses - when its solve meets an anomaly (PCG breakdown, not converged,
// residual guard): it knows the remedies (retake the inverses, additive operator).
#include "pgo_handle.hpp"

namespace uzl {

struct LmRun {
    int nslots = 0;
    DevBuf<LmSlot> d_slots;
    DevBuf<LmDev> d_lm;
    PinBuf<LmHost> h_pub;                    // mapped + coherent: written by lm_tail_kernel, polled by the host
    LmHost* d_pub = nullptr;
    PinBuf<LmDev> h_init;                    // staging of the slots' initial states
    std::vector<LmSlot> slots;               // host copies of the slots (by-value launches of a one-graph pass; refill copies)
    LmShape shape{};
    DevBuf<double> d_start;                  // poses at the start of the solve (anomaly fallback)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool join_pending = false;               // a rebuild is in flight on the second stream
    uint64_t gen = ~0ull;                    // single handle: structure generation the slot and the captured segments belong to
    int solves_of_gen = 0;                   // optimizes of the current structure so far (single-graph driver)
    LmPassHistory hist;                      // what earlier solves took, trial by trial: sizes the passes of the next drive (pgo_lm_pass.hpp)
    struct Seg { hipGraph_t g = nullptr; hipGraphExec_t x = nullptr; };
    Seg setup, reb, pcg_long[2];            // pcg_long: per hierarchy copy (a one-graph pass's PCG launches carry the copy's arrays by value)
    void drop(Seg& q) { if (q.x) { (void)hipGraphExecDestroy(q.x); q.x = nullptr; } if (q.g) { (void)hipGraphDestroy(q.g); q.g = nullptr; } }
    void drop_all() { drop(setup); drop(reb); drop(pcg_long[0]); drop(pcg_long[1]); }
};

void lm_run_destroy(LmRun* r)
{
    if (!r) return;
    r->drop_all();
    if (r->ev_fork) (void)hipEventDestroy(r->ev_fork);
    if (r->ev_join) (void)hipEventDestroy(r->ev_join);
    delete r;
}

namespace {

LmRun* new_run()
{
    LmRun* R = new LmRun();
    if (hipEventCreateWithFlags(&R->ev_fork, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&R->ev_join, hipEventDisableTiming) != hipSuccess) {
        lm_run_destroy(R);
        throw HipError{hipErrorUnknown, "hipEventCreate", __FILE__, __LINE__};
    }
    return R;
}
void reserve_slots(LmRun* R, int n)
{
    R->nslots = n;
    R->d_slots.reserve((size_t)n); R->d_lm.reserve((size_t)n);
    R->h_pub.reserve((size_t)n, hipHostMallocMapped | hipHostMallocCoherent);
    R->h_init.reserve((size_t)n);
    UZL_HIP(hipHostGetDevicePointer((void**)&R->d_pub, R->h_pub.p, 0));
    R->slots.resize((size_t)n);
}

// ---- the segments of a pass, as launch sequences
void enq_linearize(LmRun* R, hipStream_t s)
{
    const LmShape& sh = R->shape;
    UZL_HIP(kl_linearize(R->d_slots.p, sh.nslots, sh.g_edges, sh.g_asm, s));
}
const LmSlot* by_value_slot(LmRun* R) { return (R->shape.nslots == 1 && !R->shape.batch_geometry) ? R->slots.data() : nullptr; }
// init_ix >= 0: the pass's PCG init rides in the head's launch (lm_init_rides), for hierarchy copy init_ix
void enq_head(LmRun* R, int pass_flags, bool linearized, int init_ix, hipStream_t s)
{
    const LmShape& sh = R->shape;
    if (!linearized) enq_linearize(R, s);
    if (init_ix >= 0) kl_lm_head_init(R->d_slots.p, by_value_slot(R), pass_flags, init_ix, s);
    else k_lm_head(R->d_slots.p, sh.nslots, pass_flags, s);
    if (sh.red) kl_schur_reduce(R->d_slots.p, sh, s);
}
void enq_setup(LmRun* R, int which, int ns_steps, hipStream_t s)
{
    kl_ml_numeric(R->d_slots.p, R->shape, which, s);
    kl_ml_trial(R->d_slots.p, R->shape, which, ns_steps, s);
}
// ix, tol2: the hierarchy copy of a one-graph pass (lm_pass_ix) and its pcg_tol^2, by value to the small-graph class's launches
// (in_head: x = 0, r = b went out with the head - the first application of the preconditioner is what is left)
void enq_init(LmRun* R, int ix, bool in_head, hipStream_t s) { UZL_HIP(kl_ml_init(R->d_slots.p, by_value_slot(R), R->shape, ix, in_head, s)); }
void enq_pcg(LmRun* R, int ix, double tol2, int first, int n, hipStream_t s, hipEvent_t* ev = nullptr)
{
    UZL_HIP(kl_ml_pcg_its(R->d_slots.p, by_value_slot(R), R->shape, ix, tol2, first, n, s, ev));
}
void enq_tail(LmRun* R, hipStream_t s)
{
    const LmShape& sh = R->shape;
    if (sh.red) kl_schur_backsub(R->d_slots.p, sh, s);
    kl_eval(R->d_slots.p, sh.nslots, sh.g_edges, sh.g_oplus, s);
    k_lm_tail(R->d_slots.p, sh.nslots, s);
}
// a long launch sequence as a captured graph (a hipGraphLaunch costs ~10 us whatever it holds, a launch ~3 us of host time: short
// sequences are launched as they are)
template <class F>
void run_seg(LmRun::Seg& q, bool eager, hipStream_t s, F&& enqueue)
{
    if (eager) { enqueue(s); return; }
    if (!q.x) {
        UZL_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        try { enqueue(s); }
        catch (...) {                                           // a launch that fails must not leave the stream in capture mode: every later
            hipGraph_t part = nullptr;                          // call on the handle (synchronize, store, destroy) would fail with it
            (void)hipStreamEndCapture(s, &part);
            if (part) (void)hipGraphDestroy(part);
            (void)hipGetLastError();
            throw;
        }
        UZL_HIP(hipStreamEndCapture(s, &q.g));
        UZL_HIP(hipGraphInstantiate(&q.x, q.g, nullptr, nullptr, 0));
    }
    UZL_HIP(hipGraphLaunch(q.x, s));
}

}  // namespace

// the slot of a handle's current structure, its LM state in lm / snapshot in pub (both null: a solve of the host-driven loop - HostSlot)
LmSlot make_slot(const uzl_pgo* h, LmDev* d_lm, LmHost* d_pub)
{
    LmSlot S;
    memset(&S, 0, sizeof(S));
    S.D = h->D; S.Dp = h->Dp;
    if (d_lm) { S.D.flags = d_lm->flags; S.Dp.flags = d_lm->flags; }      // the PCG kernels' done / iterations / breakdown words live in the LM state
    S.D.pose = nullptr; S.D.pose_trial = nullptr; S.Dp.pose = nullptr; S.Dp.pose_trial = nullptr;
    S.SD = h->red.S; S.red = h->red.on ? 1 : 0;
    S.lm = d_lm; S.pub = d_pub;
    for (int c = 0; c < 2; c++) {
        S.hot[c] = h->mlb[c].hot; S.dml[c] = h->mlb[c].dml;
        S.rg[c][0] = h->mlb[c].rg[0]; S.rg[c][1] = h->mlb[c].rg[1];
        for (int l = 0; l <= kMlMaxLevels; l++) S.dense[c][l] = h->ml_dense_ptr[c][l];
        S.nsT[c] = h->mlb[c].nsT; S.nsX[c] = h->mlb[c].nsX;
    }
    S.pbuf[0] = h->pbuf[0]; S.pbuf[1] = h->pbuf[1];
    S.pose[0] = h->pose_a.p; S.pose[1] = h->pose_b.p;
    S.g_edges = g_edges_for(h->e); S.g_asm = h->D.n_rb; S.g_oplus = g_oplus_for(h->n);
    S.g_rows = g_ml_rows(h->Dp.nb, h->mlp.agg); S.g_spmv = g_ml_spmv(h->Dp.nb, h->mlp.agg);
    S.copy_stride = (int64_t)h->ml_copy_stride;
    return S;
}

// launch geometry for the graphs `hs` (one, or a batch of one hierarchy shape from level 1 up): the largest extents
LmShape make_shape(const std::vector<uzl_pgo*>& hs, int nslots, bool batch_geometry)
{
    const uzl_pgo* h = hs[0];
    for (const uzl_pgo* g : hs) if (g->mlp.levels >= 1 && g->mlp.n[1] > h->mlp.n[1]) h = g;       // the ml_cg variant that covers the largest level 1
    LmShape sh;
    memset(&sh, 0, sizeof(sh));
    sh.nslots = nslots; sh.batch_geometry = batch_geometry ? 1 : 0;
    sh.levels = h->mlp.levels; sh.cl = h->mlp.cl; sh.agg = h->mlp.agg;
    sh.mult = h->ml_mult ? 1 : 0; sh.ns_steps = h->ml_ns_steps; sh.upper_ns = kUpperNs;
    ml_cg_variant(h->mlb[0].hot, h->mlp.agg, h->mlp.lds, &sh.cg_variant, &sh.comp_u, &sh.cg_lds);
    for (const uzl_pgo* g : hs) {
        for (int l = 0; l <= g->mlp.levels; l++) { sh.n_lv[l] = std::max(sh.n_lv[l], g->mlp.n[l]); sh.work_t[l] = std::max(sh.work_t[l], g->mlp.nslots[l] + g->mlp.n[l]); sh.chunks[l] = std::max(sh.chunks[l], g->mlp.chunks[l]); }
        sh.inner_aggs = std::max(sh.inner_aggs, g->mlp.inner_aggs);
        sh.g_edges = std::max(sh.g_edges, g_edges_for(g->e)); sh.g_asm = std::max(sh.g_asm, g->D.n_rb); sh.g_oplus = std::max(sh.g_oplus, g_oplus_for(g->n));
        sh.g_rows = std::max(sh.g_rows, g_ml_rows(g->Dp.nb, g->mlp.agg)); sh.g_spmv = std::max(sh.g_spmv, g_ml_spmv(g->Dp.nb, g->mlp.agg));
        if (g->red.on) {
            const SchurDev& SD = g->red.S;
            sh.red = 1;
            sh.schur_runs = std::max(sh.schur_runs, SD.n_runs);
            sh.schur_items = std::max<int64_t>(sh.schur_items, (int64_t)(SD.nslots_r + SD.nbr) * 36);
            sh.schur_backsub_grid = std::max(sh.schur_backsub_grid, SD.n_runs + (SD.nbr * 6 + 63) / 64);
        }
    }
    return sh;
}

// The state a graph starts its LM loop in, for both drivers of the state machine (pgo_lm.hpp).  sync_rebuild: every rebuild of the
// hierarchy runs in front of the solve it serves, none ahead on the second stream
LmDev lm_initial_state(const uzl_pgo* h, int iterations, bool sync_rebuild)
{
    LmDev I;
    memset(&I, 0, sizeof(I));
    I.flags[0] = 1;                                          // PCG kernels are no-ops until a solve is initialised
    I.phase = kLmLin; I.cur = 0; I.ix = 0;
    I.init_pass = I.schur_pass = I.numeric_pass = I.trial_pass = I.build_pass = -1;
    I.iterations = iterations;
    I.max_it = h->cfg.pcg_max_iter > 0 ? h->cfg.pcg_max_iter : 6 * std::max(h->Dp.nb, 1);
    I.sync_rebuild = sync_rebuild ? 1 : 0;
    I.guarded = (h->ml_mult || h->ml_ns_steps > 0) ? 1 : 0;
    I.ni = 2.; I.last_rel = 1e300; I.rate_ref = -1.; I.rate_last = -1.;
    I.tol_f2 = pgo_tol_f2(h->cfg); I.eps_t = pgo_eps_t(h->cfg); I.eps_r = pgo_eps_r(h->cfg);
    I.refresh_rel = ml_async_level(h) ? kRefreshRel : kRefreshRelSync; I.rate_drop = ml_rate_drop(h); I.tol2 = h->cfg.pcg_tol * h->cfg.pcg_tol; I.lambda_retake = kLambdaRetake; I.delta = h->cfg.huber_delta;
    return I;
}
// what a loop's final state says in uzl_pgo_stats (both drivers)
void lm_stats(const LmDev& v, uzl_pgo_stats& S)
{
    S.iterations_done = v.st_iterations_done; S.lm_trials = v.st_lm_trials; S.pcg_iterations = v.st_pcg_iterations;
    S.terminated_early = v.st_terminated_early; S.precond_builds = v.st_precond_builds;
    S.chi2_initial = v.chi2_initial; S.chi2_final = v.chi_cur; S.lambda_final = v.lambda;
}

namespace {

LmDev idle_state()
{
    LmDev I;
    memset(&I, 0, sizeof(I));
    I.flags[0] = 1; I.phase = kLmDone;
    I.init_pass = I.schur_pass = I.numeric_pass = I.trial_pass = I.build_pass = -1;
    return I;
}

// Waits until lm_tail launch number `seq` (or a later one) of slot `sl` has published and copies the snapshot; returns its number.
// lm_tail writes the fields and seq_begin (unordered among themselves), waits until they have been acknowledged, then seq
// (publish_wait_own_stores, pgo_device.hpp).  What keeps a copy whole is the DRIVER'S ORDER: a slot's snapshot is copied here before the
// pass whose tail writes the next one is enqueued; seq_begin == seq around the copy cross-checks it.
uint32_t wait_pub(hipStream_t s, LmRun* R, int sl, uint32_t seq, LmHost* out)
{
    const auto t0 = std::chrono::steady_clock::now();
    volatile LmHost* pub = R->h_pub.p + sl;
    for (int spin = 0;; spin++) {
        const uint32_t s1 = __atomic_load_n(&R->h_pub.p[sl].seq, __ATOMIC_ACQUIRE);
        if ((int32_t)(s1 - seq) >= 0) {
            memcpy(out, const_cast<const LmHost*>(R->h_pub.p + sl), sizeof(LmHost));
            __atomic_thread_fence(__ATOMIC_ACQUIRE);
            if (pub->seq_begin == s1 && out->seq == s1) return s1;           // (else a later tail is writing: its seq will land)
        }
        if ((spin & 1023) == 1023 && std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() > 200.0) {
            UZL_HIP(hipStreamSynchronize(s));
            const uint32_t s2 = __atomic_load_n(&R->h_pub.p[sl].seq, __ATOMIC_ACQUIRE);
            if ((int32_t)(s2 - seq) < 0) throw HipError{hipErrorUnknown, "lm_tail_kernel did not publish", __FILE__, __LINE__};
            memcpy(out, const_cast<const LmHost*>(R->h_pub.p + sl), sizeof(LmHost));      // (the stream is idle: nothing writes the snapshot now)
            if (out->seq_begin != out->seq) throw HipError{hipErrorUnknown, "lm_tail_kernel: torn snapshot on an idle stream", __FILE__, __LINE__};
            return s2;
        }
    }
}

// one graph of a drive
struct LmJob {
    uzl_pgo* h = nullptr;
    size_t start_off = 0;                    // its start poses in LmRun::d_start
    LmHost last;                             // the snapshot it finished with
    bool finished = false, anomaly = false;
    int32_t passes = 0;
};

struct LmDriveOpts {
    hipStream_t s = nullptr, s2 = nullptr;
    int iterations = 0;
    bool eager = false;                      // no captured graphs (UZL_NO_GRAPH=1, profiling)
    bool verbose = false;
    KernelTimer* timer = nullptr;            // profiling: the two PCG kernels with dispatch timestamps
    const char* spmv_name = "pcg_spmv";
    const char* cg_name = "ml_cg";
};

// what the steps of one drive share
struct LmDrive {
    LmRun* R;
    std::vector<LmJob>& jobs;
    const LmDriveOpts& o;
    std::vector<LmSlotTrack> tracks;         // per slot: its job and what the planner remembers of it (pgo_lm_pass.hpp)
    std::vector<LmPlanView> views;           // ... what the planner reads of its last snapshot
    std::vector<LmHost> snap;                // ... the snapshot itself
    std::vector<uint32_t> sent;              // ... lm_tail launches enqueued since its load (= the sequence word expected)
    int next_job = 0, n_active = 0, passes = 0;
    // The next pass's linearisation goes out right behind a pass's tail, BEFORE the look: hessian_lm_kernel takes nothing from the host
    // (it works on the graphs the tail has left in phase kLmLin and is a no-op for the others), so the GPU builds the Hessian while the
    // host reads the snapshot, chooses the next pass and launches it - otherwise ~12 us of idle GPU per pass (tail -> hessian in the
    // kernel trace).  Not while a rebuild on the second stream still reads H, and a refill sends the linearisation again.
    bool lin_ahead = false;
    PhaseMarks<7> phases;                    // diagnostic build, UZL_PHASES=1: GPU time between the segment boundaries of every pass
    bool timed() const { return o.timer && o.timer->on; }
};

// Start poses of every job (anomaly fallback); its current estimate goes to pose buffer 0 (accepted steps flip LmDev::cur; an earlier
// solve may have left it in buffer 1)
void save_start_poses(LmDrive& d)
{
    LmRun* R = d.R;
    size_t tot = 0;
    for (LmJob& j : d.jobs) { j.start_off = tot; tot += (size_t)std::max(j.h->n, 1) * 8; }
    R->d_start.reserve(tot);
    for (LmJob& j : d.jobs) {
        uzl_pgo* h = j.h;
        if (h->cur != h->pose_a.p) {
            UZL_HIP(hipMemcpyAsync(h->pose_a.p, h->cur, sizeof(double) * 8 * (size_t)h->n, hipMemcpyDeviceToDevice, d.o.s));
            h->cur = h->pose_a.p; h->trial = h->pose_b.p;
        }
        UZL_HIP(hipMemcpyAsync(R->d_start.p + j.start_off, h->cur, sizeof(double) * 8 * (size_t)h->n, hipMemcpyDeviceToDevice, d.o.s));
    }
}

// The next job of the queue into slot sl (stream-ordered behind what the slot ran).  A REFILL keeps the slot's sequence word running
// (LmDev::tails starts at what the slot has sent): lm_tail_kernel publishes for every slot in every pass and the look waits for the
// unfinished ones only, so the last snapshot of a finished or idle slot may still be on its way to h_pub when the slot is reloaded -
// with the sequence restarted at 0 that late write (an old, larger number with phase = done) would pass for the new graph's.  Only
// the first load of a drive (everything drained by the previous drive's final synchronize) zeroes the snapshot.
void load_slot(LmDrive& d, int sl, bool first)
{
    LmRun* R = d.R;
    hipStream_t s = d.o.s;
    LmDev I;
    if (d.next_job < (int)d.jobs.size()) {
        const int j = d.next_job++;
        uzl_pgo* h = d.jobs[(size_t)j].h;
        lm_track_load(d.tracks[sl], j, h->cfg.pass_history == 1, R->hist);
        R->slots[sl] = make_slot(h, R->d_lm.p + sl, R->d_pub + sl);
        UZL_HIP(hipMemcpyAsync(R->d_slots.p + sl, &R->slots[sl], sizeof(LmSlot), hipMemcpyHostToDevice, s));
        // (rebuilds run ahead for the small-graph class only - at 10k vertices the rebuild's GEMMs take more from the overlapped PCG than they give back)
        I = lm_initial_state(h, d.o.iterations, !ml_async_level(h));
        d.n_active++;
    } else {
        lm_track_load(d.tracks[sl], -1, false, R->hist);
        I = idle_state();                                // (the slot keeps its last graph's arguments: every kernel no-ops on the state)
    }
    if (first) { memset(R->h_pub.p + sl, 0, sizeof(LmHost)); d.sent[sl] = 0; }
    I.tails = (int32_t)d.sent[sl];
    R->h_init.p[sl] = I;
    UZL_HIP(hipMemcpyAsync(R->d_lm.p + sl, R->h_init.p + sl, sizeof(LmDev), hipMemcpyHostToDevice, s));
    memset(&d.snap[sl], 0, sizeof(LmHost));
    d.snap[sl].lm = I;
    d.views[sl] = lm_plan_view(I);
}

// One pass as the plan says: join wait | head [+ init] | set-up | fork, rebuild, join record | init | PCG | tail | linearise-ahead
void enqueue_pass(LmDrive& d, const LmPassPlan& P)
{
    LmRun* R = d.R;
    hipStream_t s = d.o.s, s2 = d.o.s2;
    const bool eager = d.o.eager;
    d.phases.mark(0, s);
    if (P.any_start && R->join_pending) { UZL_HIP(hipStreamWaitEvent(s, R->ev_join, 0)); R->join_pending = false; }      // the rebuild of an earlier pass reads H and the poses
    d.phases.mark(1, s);
    const bool init_in_head = lm_init_rides(P, lm_init_rides_shape(by_value_slot(R), R->shape), R->shape.red != 0);
    if (P.any_start) enq_head(R, P.flags, d.lin_ahead, init_in_head ? P.ix : -1, s);
    d.lin_ahead = false;
    d.phases.mark(2, s);
    if (P.flags & kPassSetup) {
        if (!P.setup_captured) enq_setup(R, 1, P.ns_steps, s);
        else run_seg(R->setup, eager, s, [&](hipStream_t q) { enq_setup(R, 1, P.ns_steps, q); });
    }
    if (P.flags & kPassRebuild) {
        UZL_HIP(hipEventRecord(R->ev_fork, s));
        UZL_HIP(hipStreamWaitEvent(s2, R->ev_fork, 0));
        run_seg(R->reb, eager, s2, [&](hipStream_t q) { enq_setup(R, 0, R->shape.ns_steps, q); });
        UZL_HIP(hipEventRecord(R->ev_join, s2));
        R->join_pending = true;
    }
    d.phases.mark(3, s);
    if (P.any_start) enq_init(R, P.ix, init_in_head, s);
    d.phases.mark(4, s);
    if (d.timed()) {
        KernelTimer* tm = d.o.timer;
        std::vector<hipEvent_t> ev((size_t)4 * P.want);
        for (int q = 0; q < P.want; q++) { tm->pair(d.o.spmv_name, &ev[4 * q], &ev[4 * q + 1]); tm->pair(d.o.cg_name, &ev[4 * q + 2], &ev[4 * q + 3]); }
        enq_pcg(R, P.ix, P.tol2, P.base, P.want, s, ev.data());
    } else {
        const LmPcgLaunches L = lm_pcg_launches(P.base, P.want, eager);
        if (L.lead) enq_pcg(R, P.ix, P.tol2, P.base, 1, s);
        for (int i = 0; i < L.n_long; i++) run_seg(R->pcg_long[P.ix], false, s, [&](hipStream_t q) { enq_pcg(R, P.ix, P.tol2, 0, kPcgLong, q); });
        if (L.rem > 0) enq_pcg(R, P.ix, P.tol2, L.rem_first, L.rem, s);
    }
    d.phases.mark(5, s);
    enq_tail(R, s);
    if (!R->join_pending && !d.timed()) { enq_linearize(R, s); d.lin_ahead = true; }
    d.phases.mark(6, s);
    d.passes++;
    for (uint32_t& n : d.sent) n++;
}

// The look: every unfinished slot's snapshot of the pass just enqueued.  True when a graph got through.
bool look(LmDrive& d)
{
    bool through = false;
    for (int sl = 0; sl < (int)d.tracks.size(); sl++) {
        LmSlotTrack& T = d.tracks[sl];
        if (!T.active) continue;
        (void)wait_pub(d.o.s, d.R, sl, d.sent[sl], &d.snap[sl]);
        LmJob& J = d.jobs[(size_t)T.job];
        const LmDev& v = d.snap[sl].lm;
        J.passes++;
        if (d.o.verbose)
            fprintf(stderr, "[uzl_pgo] pass %d, graph %d -> it %d trial %d phase %d: pcg %d done %d (last solve %d) lambda %.3e chi2 %.9g |r|2/|b|2 %.3e need %d\n", d.passes - 1,
                    T.job, v.it, v.qmax, v.phase, v.flags[1], v.flags[0], v.pcg_last, v.lambda, v.chi_cur, d.snap[sl].scal[7], v.need);
        d.views[sl] = lm_plan_view(v);
        if (lm_track_look(d.views[sl], T, d.R->hist)) {
            J.last = d.snap[sl]; J.finished = true; J.anomaly = v.phase == kLmAnomaly;
            d.n_active--; through = true;
        }
    }
    if (d.timed()) { UZL_HIP(hipStreamSynchronize(d.o.s)); d.o.timer->resolve(); }
    return through;
}

// A queue longer than the slots is worked off in COHORTS: the slots are refilled when every resident graph is through, so that the
// residents walk through their LM iterations together - their solves need similar numbers of PCG iterations, and a pass is as long
// as its longest solve.  Refilling slot by slot mixes converged graphs (4 iterations
// per solve) with fresh ones (60): measured on 256 queued config-2 graphs through 16 / 64 slots 49 / 69 M edges/s against 60 / 74 M.
void refill(LmDrive& d)
{
    LmRun* R = d.R;
    // (a rebuild of the outgoing graphs may still read the slot table and their LM state)
    if (R->join_pending && d.next_job < (int)d.jobs.size()) { UZL_HIP(hipStreamWaitEvent(d.o.s, R->ev_join, 0)); R->join_pending = false; }
    for (int sl = 0; sl < (int)d.tracks.size(); sl++)
        if (d.tracks[sl].job >= 0 && !d.tracks[sl].active) load_slot(d, sl, false);
    d.lin_ahead = false;                                 // (the new graphs were not in their slots when the linearisation ran)
}

// Solves `jobs` through the slots of R (shape and slot count set up by the caller; structures prepared): plan the next pass from the
// slots' snapshots (pgo_lm_pass.hpp), enqueue it, look, refill.  Returns passes enqueued.
int lm_drive(LmRun* R, std::vector<LmJob>& jobs, const LmDriveOpts& o)
{
    const int nS = R->shape.nslots;
    LmDrive d{R, jobs, o, std::vector<LmSlotTrack>((size_t)nS), std::vector<LmPlanView>((size_t)nS), std::vector<LmHost>((size_t)nS), std::vector<uint32_t>((size_t)nS, 0)};
    save_start_poses(d);
    {
        std::vector<uint64_t> gen;
        for (const LmJob& j : jobs) gen.push_back(j.h->structure_gen);
        lm_history_begin(R->hist, gen.data(), (int)gen.size());
    }
    for (int sl = 0; sl < nS; sl++) load_slot(d, sl, true);
    R->join_pending = false;
    struct Drain {                           // an exception must not leave a rebuild running on stream2 behind the caller's back
        LmRun* R; hipStream_t s2;
        ~Drain() { if (R->join_pending) { (void)hipStreamSynchronize(s2); R->join_pending = false; } }
    } drain{R, o.s2};
    static const bool wrong_ix = diag_flag("UZL_LM_WRONG_IX");      // diagnostic build: a one-graph pass names the other hierarchy copy
    double enq_ms = 0., wait_ms = 0.;
    while (d.n_active > 0) {
        const auto tp0 = std::chrono::steady_clock::now();
        const int in_slots = d.n_active;
        const LmPassPlan P = lm_plan_pass(d.views.data(), d.tracks.data(), nS, R->hist.first_solve_its, R->shape.ns_steps, wrong_ix);
        enqueue_pass(d, P);
        const auto tp1 = std::chrono::steady_clock::now();
        if (o.verbose) fprintf(stderr, "[uzl_pgo]   pass %d enqueued: segments %d, %d PCG iterations, %d graph(s) in the slots\n", d.passes - 1, P.flags, P.want, in_slots);
        if (look(d) && (d.n_active == 0 || nS == 1)) refill(d);
        const auto tp2 = std::chrono::steady_clock::now();
        enq_ms += std::chrono::duration<double, std::milli>(tp1 - tp0).count(); wait_ms += std::chrono::duration<double, std::milli>(tp2 - tp1).count();
    }
    UZL_HIP(hipGetLastError());
    if (o.verbose) fprintf(stderr, "[uzl_pgo] device-resident loop: %d passes, host time enqueueing %.3f ms, waiting for snapshots %.3f ms\n", d.passes, enq_ms, wait_ms);
    if (R->join_pending) { UZL_HIP(hipStreamSynchronize(o.s2)); R->join_pending = false; }      // a rebuild nobody will use: let it drain
    UZL_HIP(hipStreamSynchronize(o.s));
    static const char* const kSegmentNames[7] = {"wait for the rebuild (0->1)", "linearise + head (1->2)", "set-up / fork (2->3)", "init (3->4)", "pcg (4->5)", "tail (5->6)", "between passes (6->0)"};
    d.phases.report("segments", d.passes, "passes", kSegmentNames);
    return d.passes;
}

// what a finished job leaves in its handle and in the caller's stats
void finish_job(LmJob& J, uzl_pgo_stats* st, double wall_ms)
{
    uzl_pgo* h = J.h;
    const LmDev& v = J.last.lm;
    h->cur = v.cur ? h->pose_b.p : h->pose_a.p; h->trial = v.cur ? h->pose_a.p : h->pose_b.p;
    h->prev_pcg_iters = v.pcg_last;
    h->last_residual_ratio = J.last.scal[7];
    if (!st) return;
    uzl_pgo_stats S;
    memset(&S, 0, sizeof(S));
    stats_head(h, S);
    lm_stats(v, S);
    S.lm_passes = J.passes;
    S.solve_ms = wall_ms;
    S.structure_ms = h->structure_ms;
    *st = S;
}

}  // namespace

// which solves take the device-resident loop
bool lm_eligible(const uzl_pgo* h)
{
    return h->cfg.lm_loop != 1 && h->mlp.levels > 0 && !h->sharded && h->nb > 0 && h->e > 0 && h->Dp.nb > 0 && !h->timer.on &&
           h->stream2 != nullptr;
}

int do_optimize_lm(uzl_pgo* h, int32_t iterations, uzl_pgo_stats* st)
{
    hipStream_t s = h->stream;
    if (!h->lm) h->lm = new_run();
    LmRun* R = h->lm;
    // ---- shape of this structure (captured segments belong to it)
    if (R->gen != h->structure_gen || R->nslots != 1) {
        const auto ts = std::chrono::steady_clock::now();
        UZL_HIP(hipStreamSynchronize(s));
        R->drop_all();
        reserve_slots(R, 1);
        R->shape = make_shape({h}, 1, false);
        R->gen = h->structure_gen;
        R->solves_of_gen = 0;
        R->hist.hist_gen.clear();                                     // (a grown graph's solves are not the old graph's: measured on config 5, +5 % per solve with the old counts)
        h->structure_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts).count();
    }
    std::vector<LmJob> jobs(1);
    jobs[0].h = h;
    LmDriveOpts o;
    // The FIRST solve of a structure launches everything kernel by kernel: capturing and instantiating its segments costs ~0.5 ms and dropping
    // them again ~0.7 ms, which a structure that is solved once - every re-optimisation of a growing graph - never earns back (config 5:
    // 16.2 -> 15.7 ms per solve, structure 1.9 -> 1.2 ms).  A structure that comes back (uzl_pgo_reset, a timer-driven re-optimisation of an
    // unchanged graph) replays captured segments from its second solve on.  Same kernels, same results either way.
    o.s = s; o.s2 = h->stream2; o.iterations = iterations; o.eager = h->no_graph || R->solves_of_gen == 0; o.verbose = h->cfg.verbose != 0;
    R->solves_of_gen++;
    lm_drive(R, jobs, o);
    LmJob& J = jobs[0];
    if (J.anomaly) {             // the host-driven loop knows the remedies (retake the inverses, additive operator): from the start poses
        if (h->cfg.verbose) fprintf(stderr, "[uzl_pgo] device-resident loop: anomaly %d at it %d trial %d -> host-driven loop\n", J.last.lm.anomaly_code, J.last.lm.it, J.last.lm.qmax);
        UZL_HIP(hipMemcpyAsync(h->pose_a.p, R->d_start.p + J.start_off, sizeof(double) * 8 * (size_t)h->n, hipMemcpyDeviceToDevice, s));
        h->cur = h->pose_a.p; h->trial = h->pose_b.p;
        return do_optimize_host(h, iterations, st);
    }
    finish_job(J, st, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h->t_start).count());
    return UZL_OK;
}

// ---- many graphs through one launch sequence (uzl_pgo_batch_optimize) ---------------------------------------------------------
// Batched together are graphs of the small-graph class (dense level-1 operator, multiplicative cycle: the class whose kernels have a
// throughput geometry - four rows per wave in 128-lane workgroups, wave sums through the LDS crossbar; same bits as the single
// solve's geometry) with one hierarchy shape from level 1 up, Schur-reduced or not: the shape of the SYSTEM THE PCG SOLVES decides, so
// chain-like graphs (graph_slam_node.cpp:578-663: an odometry chain plus a few loop closures) batch on their reduced systems.
bool lm_batch_eligible(const std::vector<uzl_pgo*>& hs)
{
    if (hs.empty() || (int)hs.size() > kBatchMax) return false;
    const uzl_pgo* a = hs[0];
    for (const uzl_pgo* h : hs) {
        if (!(h->cfg.lm_loop != 1 && h->mlp.levels > 0 && h->mlp.agg == 1 && h->ml_mult && h->mlp.cl == 1 && 6 * h->mlp.n[1] <= 1536 && !h->sharded && h->nb > 0 &&
              h->e > 0 && h->Dp.nb > 0 && !h->timer.on)) return false;
        // one depth of the hierarchy (the launch sequence of a pass): sizes may differ - every launch takes the largest graph's grid and a
        // twin leaves past its own graph's extent
        if (h->mlp.levels != a->mlp.levels || h->ml_ns_steps != a->ml_ns_steps || h->cfg.device != a->cfg.device) return false;
    }
    return true;
}

// returns graphs solved by the batch (anomalies go through the single-graph path and are not counted); < 0: graph -1 - g failed with *rc_all
int batch_optimize_lm(LmRun*& Rp, const std::vector<uzl_pgo*>& hs, int resident, hipStream_t s, hipStream_t s2, int32_t iterations, bool eager, bool verbose, KernelTimer* timer,
                      uzl_pgo_stats* stats, int* rc_all)
{
    const auto t0 = std::chrono::steady_clock::now();
    if (!Rp) Rp = new_run();
    LmRun* R = Rp;
    const int Q = (int)hs.size(), nS = std::max(1, std::min(resident > 0 ? resident : Q, Q));
    const LmShape sh = make_shape(hs, nS, true);
    if (R->nslots != nS || memcmp(&sh, &R->shape, sizeof(LmShape)) != 0) {      // captured segments hold the grids
        UZL_HIP(hipStreamSynchronize(s));
        R->drop_all();
        reserve_slots(R, nS);
        R->shape = sh;
    }
    std::vector<LmJob> jobs((size_t)Q);
    for (int g = 0; g < Q; g++) jobs[g].h = hs[g];
    LmDriveOpts o;
    o.s = s; o.s2 = s2; o.iterations = iterations; o.eager = eager || (timer && timer->on); o.verbose = verbose; o.timer = timer;
    o.spmv_name = "ml_spmv_batch"; o.cg_name = "ml_cg_comp_batch";
    lm_drive(R, jobs, o);
    const double wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    int batched = 0;
    for (int g = 0; g < Q; g++) {
        LmJob& J = jobs[g];
        uzl_pgo* h = hs[g];
        // (diagnostic build: UZL_BATCH_FORCE_ANOMALY_N = n sends every graph of n nodes down the anomaly path - tests/test_batch_gpu.py)
        static const int force_n = diag_int("UZL_BATCH_FORCE_ANOMALY_N", -1);
        if (!J.anomaly && h->n != force_n) { finish_job(J, stats ? stats + g : nullptr, wall); batched++; continue; }
        if (verbose) fprintf(stderr, "[uzl_pgo_batch] graph %d: anomaly %d at it %d trial %d -> single-graph path\n", g, J.last.lm.anomaly_code, J.last.lm.it, J.last.lm.qmax);
        UZL_HIP(hipMemcpyAsync(h->pose_a.p, R->d_start.p + J.start_off, sizeof(double) * 8 * (size_t)h->n, hipMemcpyDeviceToDevice, s));
        UZL_HIP(hipStreamSynchronize(s));
        h->cur = h->pose_a.p; h->trial = h->pose_b.p;
        own_streams(h, false);                             // (sequence 0 may be capturing on the streams h borrowed: not synchronized, h has nothing on them)
        h->t_start = std::chrono::steady_clock::now();
        uzl_pgo_stats S;
        const int rc = do_optimize_host(h, iterations, &S);
        if (rc != UZL_OK && rc != UZL_ERR_NOT_CONVERGED) { *rc_all = rc; return -1 - g; }
        if (rc != UZL_OK) *rc_all = rc;
        if (stats) stats[g] = S;
    }
    return batched;
}

}  // namespace uzl
