// uzl_pgo_debug.hip — stage-level test hooks of the pose-graph solver (uzl_debug_pgo_*): diagnostic library only.  Each drives the pieces
// of the host-driven loop (pgo_handle.hpp; uzl_pgo.hip) one by one and copies out what the production kernels wrote.
#include "pgo_handle.hpp"

using namespace uzl;

#ifdef UZL_DIAG
// ---- stage-level test hooks of the pose-graph linear system (tests/test_pgo_system_gpu.py).  Diagnostic build only; every hook takes a
//      handle made by THIS library's uzl_pgo_create / uzl_pgo_add_graph, runs the production kernels and host steps (no arithmetic of its
//      own), and leaves the handle as usable as it found it: the poses are not touched and every buffer it writes is rewritten by the
//      next optimize.  Array outputs: a call with null arrays returns the sizes only.
namespace {
// gauge + structure + slot records (as optimize), then one linearisation at the current poses: H in D.blk / D.hdiag, b, chi2, max diag
void debug_linearize(uzl_pgo* h)
{
    if (h->sharded) throw HipError{hipErrorNotSupported, "stage hooks: not on a sharded handle", __FILE__, __LINE__};
    UZL_HIP(hipSetDevice(h->cfg.device));
    prepare_optimize(h);
    PgoDev& D = h->D;
    D.pose = h->cur; D.pose_trial = h->trial;
    h->Dp.pose = h->cur; h->Dp.pose_trial = h->trial;
    if (h->nb == 0 || h->e == 0) return;
    int gl = 0, ga = 0;
    UZL_HIP(k_hessian(D, h->cur, h->cfg.huber_delta, &gl, &ga, h->stream, true));
    k_finalize(D, gl, 0, ga, 2, h->stream);
}
// the Schur reduction for this lambda, as an LM trial makes it (do_optimize_host: schur_reduce)
void debug_reduce(uzl_pgo* h, double lambda)
{
    if (!h->red.on) return;
    k_set_scalar(h->D.scal + 3, lambda, h->stream);
    kl_schur_reduce(host_slot(h), h->ml_shape, h->stream, nullptr);
}
double debug_lambda(uzl_pgo* h, double lambda)
{
    if (lambda >= 0.) return lambda;
    double sc[16];
    UZL_HIP(hipMemcpyAsync(sc, h->D.scal, sizeof(sc), hipMemcpyDeviceToHost, h->stream));
    UZL_HIP(hipStreamSynchronize(h->stream));
    return 1e-5 * sc[6];                                       // computeLambdaInit
}
// The set-up an LM trial of the host-driven loop makes after the linearisation, into hierarchy copy 0, for lambda (< 0: lambda_init; the
// value used is written back): Schur reduction, set_lambda (before the lambda-dependent set-up, as in pcg_solve), the preconditioner's
// numeric part and its lambda-dependent part with ns_steps Newton-Schulz steps at the composite level.  Returns the slot the PCG
// kernels take (block-Jacobi: an empty one); the next solve takes its own inverses.
HostSlot debug_trial_setup(uzl_pgo* h, double& lambda, int ns_steps)
{
    lambda = debug_lambda(h, lambda);
    h->ml_ix = 0;
    debug_reduce(h, lambda);
    set_lambda(h, lambda, tol_factor2(h->cfg));
    if (h->mlp.levels == 0) return HostSlot{};
    const HostSlot hs = host_slot(h);
    ml_setup_numeric(h, hs, h->stream, nullptr);
    kl_ml_trial(hs, h->ml_shape, ns_steps, h->stream, nullptr);
    return hs;
}
}  // namespace

// sizes[4] = {n, nb, nslots, e}.  v2b [n]: vertex -> block row (-1: fixed); row_ptr [nb+1]; col [nslots] (-1: the neighbour is fixed, the
// block is zero); blk [nslots][36]: H_{a, col} row-major for row a, one slot per incident edge (multi-edges give several slots of one
// block); haa [nb][36] (no lambda); b [nb][6] = -J^T Omega' e; scal[2] = {chi2, max |H_jj|}; poses [n][12]: the poses linearised at, as
// uzl_pgo_store writes them.  Structure (sizes) only when blk is null.
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_linearize(uzl_pgo* h, int32_t* sizes, int32_t* v2b, int32_t* row_ptr, int32_t* col,
                                                       double* blk, double* haa, double* b, double* scal, double* poses)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "linearize before add_graph/set_graph");
    if (!sizes) return fail(h, UZL_ERR_BAD_ARG, "sizes is required");
    own_streams(h, true);
    hipStream_t s = h->stream;
    if (!blk) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        prepare_optimize(h);
    } else {
        debug_linearize(h);
    }
    sizes[0] = h->n; sizes[1] = h->nb; sizes[2] = h->nslots; sizes[3] = h->e;
    if (!blk) { UZL_HIP(hipStreamSynchronize(s)); return UZL_OK; }
    const size_t nb = (size_t)h->nb, ns = (size_t)h->nslots;
    if (v2b && h->n) UZL_HIP(hipMemcpyAsync(v2b, h->d_v2b.p, sizeof(int32_t) * (size_t)h->n, hipMemcpyDeviceToHost, s));
    if (row_ptr) UZL_HIP(hipMemcpyAsync(row_ptr, h->sys.row_ptr.p, sizeof(int32_t) * (nb + 1), hipMemcpyDeviceToHost, s));
    if (ns) {
        if (col) UZL_HIP(hipMemcpyAsync(col, h->sys.col.p, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, s));
        UZL_HIP(hipMemcpyAsync(blk, h->D.blk, sizeof(double) * 36 * ns, hipMemcpyDeviceToHost, s));
    }
    if (nb) {
        if (haa) UZL_HIP(hipMemcpyAsync(haa, h->D.hdiag, sizeof(double) * 36 * nb, hipMemcpyDeviceToHost, s));
        if (b) UZL_HIP(hipMemcpyAsync(b, h->D.b, sizeof(double) * 6 * nb, hipMemcpyDeviceToHost, s));
    }
    double sc[16] = {};
    if (nb && h->e) UZL_HIP(hipMemcpyAsync(sc, h->D.scal, sizeof(sc), hipMemcpyDeviceToHost, s));
    if (poses && h->n) {
        h->d_out12.reserve((size_t)h->n * 12);
        k_poses_out(h->cur, h->n, h->d_out12.p, s);
        UZL_HIP(hipMemcpyAsync(poses, h->d_out12.p, sizeof(double) * 12 * (size_t)h->n, hipMemcpyDeviceToHost, s));
    }
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    if (scal) { scal[0] = sc[4]; scal[1] = sc[6]; }
    return UZL_OK;
    UZL_GUARD_END(h)
}

// One linear solve (H + lambda I) dx = b at the current poses, done as the first trial of an LM iteration of the host-driven loop does it
// (do_optimize_host): linearise, Schur reduction for this lambda (when the structure has one), the preconditioner's set-up (numeric part
// and lambda-dependent part; the multiplicative operator and its Newton-Schulz steps where the structure selected them), pcg_solve under the
// handle's cfg (pcg_tol, pcg_stop, pcg_max_iter), back-substitution.  lambda < 0: g2o's lambda_init = 1e-5 max |H_jj|.  No fallback to the
// additive operator: a residual-guard trip is reported (info[3]) and leaves converged = 0.
// dx [n][6]: the step per vertex, zero rows for fixed vertices.  info[8] = {pcg iterations, converged, 0, guard trips, lambda used, |r|^2 / |b|^2 (scal[7]),
// r.M^-1 r at the end (scal[0]), the stop threshold on it (scal[1])}.
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_solve(uzl_pgo* h, double lambda, double* dx, double* info)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "solve before add_graph/set_graph");
    if (!dx || !info) return fail(h, UZL_ERR_BAD_ARG, "dx and info are required");
    own_streams(h, true);
    debug_linearize(h);
    hipStream_t s = h->stream;
    const int n = h->n;
    for (int i = 0; i < 8; i++) info[i] = 0.;
    memset(dx, 0, sizeof(double) * 6 * (size_t)n);
    if (h->nb == 0 || h->e == 0) { info[1] = 1.; return UZL_OK; }
    PgoDev& D = h->D;
    lambda = debug_lambda(h, lambda);
    h->ml_ix = 0;
    debug_reduce(h, lambda);
    if (h->mlp.levels > 0) ml_setup_numeric(h, host_slot(h), s, nullptr);      // (not debug_trial_setup: pcg_solve takes the trial part itself)
    set_lambda(h, lambda, tol_factor2(h->cfg));
    h->prev_pcg_iters = 0;
    const int trips0 = h->guard_trips;
    LmDev L = lm_initial_state(h, 1, true);                   // the first trial of a loop, its trial set-up stamped for this pass
    L.lambda = lambda; L.trial_pass = L.pass;
    const bool conv = pcg_solve(h, L) == kLmSolved;
    const int its = L.flags[1];
    h->prev_pcg_iters = 0;
    if (h->red.on) kl_schur_backsub(host_slot(h), h->ml_shape, s, nullptr);
    const size_t nb = (size_t)h->nb;
    std::vector<double> x(nb * 6);
    std::vector<int32_t> v2b((size_t)n);
    UZL_HIP(hipMemcpyAsync(x.data(), D.x, sizeof(double) * 6 * nb, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(v2b.data(), h->d_v2b.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    for (int v = 0; v < n; v++) {
        const int32_t a = v2b[(size_t)v];
        if (a < 0 || (size_t)a >= nb) continue;
        for (int c = 0; c < 6; c++) dx[(size_t)v * 6 + c] = x[(size_t)a * 6 + c];
    }
    info[0] = its; info[1] = conv ? 1. : 0.; info[3] = h->guard_trips - trips0; info[4] = lambda;
    info[5] = h->h_scal.p->scal[7]; info[6] = h->h_scal.p->scal[0]; info[7] = h->h_scal.p->scal[1];
    h->guard_trips = trips0;
    return UZL_OK;
    UZL_GUARD_END(h)
}

// The system the PCG sees when the structure Schur-eliminates chain interiors, for this lambda (< 0: lambda_init): linearisation, then
// the Schur reduction (kl_schur_reduce).  sizes[3] = {reduced rows nbr, reduced slots, 1 if the structure has a reduction (0: nothing
// else is written)}.  sep_rows [nbr]: full-system block row of every reduced row (-1: an empty row of the strong-aggregate numbering);
// row_ptr [nbr+1], col [slots] (-1: none), blk [slots][36]: off-diagonal blocks (kept and fill); hdiag [nbr][36] and b [nbr][6]: the
// diagonal blocks and the right-hand side.  lambda is NOT in hdiag: the separators' own lambda I is added by the SpMV (as for the full
// system), while the eliminated interiors' lambda is inside the Schur terms.  An empty row has hdiag = I, b = 0 and no slots.
// Structure (sizes) only when blk is null.
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_reduced(uzl_pgo* h, double lambda, int32_t* sizes, int32_t* sep_rows, int32_t* row_ptr,
                                                     int32_t* col, double* blk, double* hdiag, double* b)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "reduced before add_graph/set_graph");
    if (!sizes) return fail(h, UZL_ERR_BAD_ARG, "sizes is required");
    own_streams(h, true);
    hipStream_t s = h->stream;
    if (!blk) { UZL_HIP(hipSetDevice(h->cfg.device)); prepare_optimize(h); }
    else debug_linearize(h);
    const bool on = h->red.on && h->nb > 0 && h->e > 0;
    sizes[0] = on ? h->Dp.nb : 0; sizes[1] = on ? h->Dp.nslots : 0; sizes[2] = on ? 1 : 0;
    if (!blk || !on) { UZL_HIP(hipStreamSynchronize(s)); return UZL_OK; }
    debug_reduce(h, debug_lambda(h, lambda));
    const PgoDev& R = h->Dp;
    const size_t nr = (size_t)R.nb, ns = (size_t)R.nslots;
    if (sep_rows && nr) UZL_HIP(hipMemcpyAsync(sep_rows, h->red.sep_rows.p, sizeof(int32_t) * nr, hipMemcpyDeviceToHost, s));
    if (row_ptr) UZL_HIP(hipMemcpyAsync(row_ptr, R.row_ptr, sizeof(int32_t) * (nr + 1), hipMemcpyDeviceToHost, s));
    if (ns) {
        if (col) UZL_HIP(hipMemcpyAsync(col, R.col, sizeof(int32_t) * ns, hipMemcpyDeviceToHost, s));
        UZL_HIP(hipMemcpyAsync(blk, R.blk, sizeof(double) * 36 * ns, hipMemcpyDeviceToHost, s));
    }
    if (nr) {
        if (hdiag) UZL_HIP(hipMemcpyAsync(hdiag, R.hdiag, sizeof(double) * 36 * nr, hipMemcpyDeviceToHost, s));
        if (b) UZL_HIP(hipMemcpyAsync(b, R.b, sizeof(double) * 6 * nr, hipMemcpyDeviceToHost, s));
    }
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    return UZL_OK;
    UZL_GUARD_END(h)
}

// One application of the PCG's operators to x, on the system the PCG iterates on (the full one, or the reduced one in its numbering: x, y
// [nb_sys][6]) for this lambda (< 0: lambda_init), after the set-up an LM trial makes (linearisation, Schur reduction, preconditioner
// numeric and lambda-dependent parts, set_lambda).  The fused kernels are driven in a state where their fused part is exact:
//   op 0, y = (A + lambda I) x: the PCG's init kernel (kl_ml_pcg_init / k_precond + k_pcg_init: flags and iteration count cleared, so beta = 0),
//         then x written into z and the iteration kernel run with the zero previous direction the init left: it forms p = z + 0 p_old = x
//         and y = A p (ml_spmv / pcg_spmv, D.ap);
//   op 1, y = M^-1 x: the right-hand side replaced by x (and restored afterwards), then the PCG's first step - kl_ml_pcg_init + kl_ml_cg with
//         init = 1 (block-Jacobi: k_precond + k_pcg_init) - which forms z = M^-1 r0 = M^-1 x.
// info[4] = {operator: 0 block-Jacobi, 1 additive multilevel, 2 multiplicative cycle / Newton-Schulz; aggregates per PCG workgroup (AGG);
// level of the dense operator (0: none); rows of the system}.  x = null: info only (after the set-up).
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_apply(uzl_pgo* h, double lambda, int32_t op, const double* x, double* y, double* info)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "apply before add_graph/set_graph");
    if (!info || (op != 0 && op != 1) || (x && !y)) return fail(h, UZL_ERR_BAD_ARG, "apply: op 0 / 1, info, and y with x");
    own_streams(h, true);
    debug_linearize(h);
    hipStream_t s = h->stream;
    PgoDev& Dp = h->Dp;
    const bool ml = h->mlp.levels > 0;
    info[0] = ml ? ((h->ml_mult || h->ml_ns_steps > 0) ? 2. : 1.) : 0.; info[1] = ml ? h->mlp.agg : 0; info[2] = ml ? h->mlp.cl : 0;
    info[3] = (h->nb > 0 && h->e > 0) ? Dp.nb : 0;
    if (!x || info[3] == 0) { UZL_HIP(hipStreamSynchronize(s)); return UZL_OK; }
    const HostSlot hs = debug_trial_setup(h, lambda, ml_ns_steps_at(h->ml_ns_steps, 0));
    const size_t n6 = (size_t)Dp.nb * 6;
    const double tol2 = h->cfg.pcg_tol * h->cfg.pcg_tol;
    DevBuf<double> saved;
    if (op == 0) {
        if (ml) kl_ml_pcg_init(hs, h->ml_shape, s);
        else { k_precond(Dp, s); k_pcg_init(Dp, h->pbuf[0], h->pbuf[1], s); }
        UZL_HIP(hipMemcpyAsync(Dp.z, x, sizeof(double) * n6, hipMemcpyHostToDevice, s));
        if (ml) kl_ml_spmv(hs, h->ml_shape, 0, s);
        else k_pcg_spmv(Dp, h->pbuf[0], h->pbuf[1], g_pcg_update(Dp.nb), tol2, s);
        UZL_HIP(hipMemcpyAsync(y, Dp.ap, sizeof(double) * n6, hipMemcpyDeviceToHost, s));
    } else {
        saved.reserve(n6);
        UZL_HIP(hipMemcpyAsync(saved.p, Dp.b, sizeof(double) * n6, hipMemcpyDeviceToDevice, s));
        UZL_HIP(hipMemcpyAsync(Dp.b, x, sizeof(double) * n6, hipMemcpyHostToDevice, s));
        if (ml) {
            kl_ml_pcg_init(hs, h->ml_shape, s);
            UZL_HIP(kl_ml_cg(hs, h->ml_shape, 0, 1, s));
        } else {
            k_precond(Dp, s);
            k_pcg_init(Dp, h->pbuf[0], h->pbuf[1], s);
        }
        UZL_HIP(hipMemcpyAsync(y, Dp.z, sizeof(double) * n6, hipMemcpyDeviceToHost, s));
        UZL_HIP(hipMemcpyAsync(Dp.b, saved.p, sizeof(double) * n6, hipMemcpyDeviceToDevice, s));
    }
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    return UZL_OK;
    UZL_GUARD_END(h)
}

// The multilevel hierarchy as its set-up kernels leave it (tests/test_pgo_hierarchy_gpu.py), array by array.  Two kinds of call:
//   what < 0:  the set-up an LM trial of the host-driven loop makes, exactly as uzl_debug_pgo_apply does it (linearisation, Schur reduction,
//              set_lambda, numeric part, lambda-dependent part) into hierarchy copy 0, for this lambda (< 0: lambda_init) and with ns_steps
//              Newton-Schulz steps at the composite level (< 0: what the first trial takes, ml_ns_steps_at(.., 0); otherwise even: the
//              steps ping-pong and an even count ends where MlHot::Cmat points; 0 = the cycle's X_0 as it comes).  Fills
//              info[64] = {levels, cl, agg, mult, steps taken at cl, upper_ns, sibling0, rows of the system, c32_stride, Schur-reduced,
//              strong numbering, strong blocks of 4, the structure's own step count, the ml_cg variant (LmCgVariant), 0..; [16 + l] n_l; [32 + l] fan_l; [48 + l] nslots_l}
//              and *lam_used.  levels = 0 (block-Jacobi): nothing else happens.
//   what >= 0: copies one array of level `level` of that copy, as the last what < 0 call left it (no kernel runs): 0 row_ptr [n_l + 1],
//              1 col [nslots_l] (both i32), 2 blk [nslots_l][36], 3 G [n_l][36] (lambda = 0), 4 M [n_l][36] (levels >= 1), 5 geo (level 0:
//              [n_0][12] = R^T | d, above [n_l][3]), 6 cen [n_l][4] (levels >= 1), 7 Winv [n_{l+1}][(6 fan_{l+1})^2] (levels < L),
//              8 Ydense [(6 n_l)^2] (cl <= l < L), 9 top_inv [(6 n_L)^2], 10 Cmat32 [6 n_cl][c32_stride] (f32), 11 b2v of the system's rows
//              [n_0] (i32, -1: EMPTY row).  *nbytes: in = the room at `out` (ignored when out is null), out = the array's size in bytes
//              (0: that level has no such array).
// The hook only reads what the production kernels wrote.
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_hierarchy(uzl_pgo* h, double lambda, int32_t ns_steps, int32_t level, int32_t what, int32_t* info,
                                                       double* lam_used, void* out, int64_t* nbytes)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "hierarchy before add_graph/set_graph");
    own_streams(h, true);
    hipStream_t s = h->stream;
    if (what < 0) {
        if (!info || (ns_steps > 0 && (ns_steps & 1))) return fail(h, UZL_ERR_BAD_ARG, "hierarchy: info, and an even step count");
        debug_linearize(h);
        for (int i = 0; i < 64; i++) info[i] = 0;
        if (h->mlp.levels == 0 || h->nb == 0 || h->e == 0) { UZL_HIP(hipStreamSynchronize(s)); return UZL_OK; }
        const int steps = !h->ml_mult ? 0 : (ns_steps < 0 ? ml_ns_steps_at(h->ml_ns_steps, 0) : ns_steps);
        debug_trial_setup(h, lambda, steps);
        UZL_HIP(hipGetLastError());
        UZL_HIP(hipStreamSynchronize(s));
        info[0] = h->mlp.levels; info[1] = h->mlp.cl; info[2] = h->mlp.agg; info[3] = h->ml_mult ? 1 : 0; info[4] = steps;
        info[5] = kUpperNs; info[6] = h->Dp.sibling0; info[7] = h->Dp.nb; info[8] = h->mlb[0].hot.c32_stride;
        info[9] = h->red.on ? 1 : 0; info[10] = h->red.strong ? 1 : 0; info[11] = h->red.strong_blocks ? 1 : 0; info[12] = h->ml_ns_steps;
        info[13] = h->ml_shape.cg_variant;
        for (int l = 0; l <= h->mlp.levels; l++) { info[16 + l] = h->mlp.n[l]; info[32 + l] = h->mlp.fan[l]; info[48 + l] = h->mlp.nslots[l]; }
        if (lam_used) *lam_used = lambda;
        return UZL_OK;
    }
    const int L = h->mlp.levels, cl = h->mlp.cl;
    if (!nbytes || !h->structure_ready || L == 0 || level < 0 || level > L) return fail(h, UZL_ERR_BAD_ARG, "hierarchy: no such level (or no set-up yet)");
    MlDev M;
    UZL_HIP(hipMemcpyAsync(&M, h->mlb[0].dml, sizeof(MlDev), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    const MlLevel& X = M.lv[level];
    const size_t n = (size_t)X.n, ns = (size_t)X.nslots;
    const void* src = nullptr;
    size_t bytes = 0;
    switch (what) {
    case 0: src = X.row_ptr; bytes = (n + 1) * 4; break;
    case 1: src = X.col; bytes = ns * 4; break;
    case 2: src = X.blk; bytes = ns * 36 * 8; break;
    case 3: src = X.G; bytes = n * 36 * 8; break;
    case 4: if (level >= 1) { src = X.M; bytes = n * 36 * 8; } break;
    case 5: src = X.geo; bytes = n * (level == 0 ? 12 : 3) * 8; break;
    case 6: if (level >= 1) { src = X.cen; bytes = n * 4 * 8; } break;
    case 7: if (level < L) { const size_t m = (size_t)6 * M.lv[level + 1].fan; src = X.Winv; bytes = (size_t)M.lv[level + 1].n * m * m * 8; } break;
    case 8: if (cl > 0 && level >= cl && level < L) { src = M.Ydense[level]; bytes = 36 * n * n * 8; } break;
    case 9: if (level == L) { src = M.top_inv; bytes = 36 * n * n * 8; } break;
    case 10: if (cl > 0 && level == cl) { src = h->mlb[0].hot.Cmat32; bytes = 6 * n * (size_t)h->mlb[0].hot.c32_stride * 4; } break;
    case 11: if (level == 0) { src = h->Dp.b2v; bytes = n * 4; } break;
    default: return fail(h, UZL_ERR_BAD_ARG, "hierarchy: no such array");
    }
    if (out && bytes) {
        if (*nbytes < (int64_t)bytes || !src) return fail(h, UZL_ERR_BAD_ARG, "hierarchy: the buffer is too small");
        UZL_HIP(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToHost, s));
        UZL_HIP(hipStreamSynchronize(s));
    }
    *nbytes = (int64_t)bytes;
    return UZL_OK;
    UZL_GUARD_END(h)
}

// The PCG's state after k iterations on the system's own right-hand side, for this lambda (< 0: lambda_init): the set-up of
// uzl_debug_pgo_apply, the PCG's init (kl_ml_pcg_init + kl_ml_cg with init = 1), then k times the two launches of an iteration
// (kl_ml_spmv, kl_ml_cg) one by one as the eager solve enqueues them.  Copies x, r, z [rows][6], the direction p the last iteration
// formed (k = 0: the init's), and rg [n_g][6]: the gather-level residual buffer the NEXT ml_cg would read.  The stop test runs as in any
// solve: give the handle a pcg_tol it cannot reach in k iterations (info[3] tells).  Multilevel path only.
// info[6] = {rows, gather level, n_g, done flag, iterations the kernels counted, lambda}.  x = null: info only (no kernel runs).
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_pcg_state(uzl_pgo* h, double lambda, int32_t k, double* x, double* r, double* z, double* p,
                                                       double* rg, double* info)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "pcg_state before add_graph/set_graph");
    if (!info || k < 0 || (x && !(r && z && p && rg))) return fail(h, UZL_ERR_BAD_ARG, "pcg_state: info, k >= 0, and every array with x");
    own_streams(h, true);
    debug_linearize(h);
    hipStream_t s = h->stream;
    PgoDev& Dp = h->Dp;
    const bool ml = h->mlp.levels > 0 && h->nb > 0 && h->e > 0;
    const int gl = !ml ? 0 : h->mlp.gather_level;
    for (int i = 0; i < 6; i++) info[i] = 0.;
    info[0] = ml ? Dp.nb : 0; info[1] = gl; info[2] = ml ? h->mlp.n[gl] : 0;
    if (!x || !ml) { UZL_HIP(hipStreamSynchronize(s)); return UZL_OK; }
    const HostSlot hs = debug_trial_setup(h, lambda, ml_ns_steps_at(h->ml_ns_steps, 0));
    kl_ml_pcg_init(hs, h->ml_shape, s);
    UZL_HIP(kl_ml_cg(hs, h->ml_shape, 0, 1, s));
    for (int i = 0; i < k; i++) {
        kl_ml_spmv(hs, h->ml_shape, i & 1, s);
        UZL_HIP(kl_ml_cg(hs, h->ml_shape, i & 1, 0, s));
    }
    const size_t n6 = (size_t)Dp.nb * 6, g6 = (size_t)h->mlp.n[gl] * 6;
    int32_t fl[4] = {0, 0, 0, 0};
    UZL_HIP(hipMemcpyAsync(x, Dp.x, sizeof(double) * n6, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(r, Dp.r, sizeof(double) * n6, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(z, Dp.z, sizeof(double) * n6, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(p, h->pbuf[k & 1], sizeof(double) * n6, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(rg, h->mlb[0].rg[(k & 1) ^ 1], sizeof(double) * g6, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipMemcpyAsync(fl, Dp.flags, sizeof(fl), hipMemcpyDeviceToHost, s));
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    info[3] = fl[0]; info[4] = fl[1]; info[5] = lambda;
    return UZL_OK;
    UZL_GUARD_END(h)
}

// A handle whose later structures start with the additive dense operator: the state the host-driven loop leaves once the multiplicative
// operator has broken down on one of its graphs (uzl_pgo::mult_banned).  Call before add_graph / set_graph.
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_ban_mult(uzl_pgo* h)
{
    UZL_GUARD_BEGIN(h)
    if (h->have_graph) return fail(h, UZL_ERR_STATE, "ban_mult: before the first graph");
    h->mult_banned = true;
    return UZL_OK;
    UZL_GUARD_END(h)
}

// One LM trial's retraction and evaluation for a step the caller gives (tests/test_pgo_geometry_gpu.py): linearise at the current poses,
// write the free vertices' rows of dx [n][6] into D.x (rows of fixed vertices are ignored), scal[3] = lambda, then the launches of a
// trial of the host-driven loop - oplus_kernel from the current poses into the trial buffer, chi2_trial_kernel on the current poses
// (the in-lane retraction) - and chi2_kernel on the stored trial poses with the same grid.  poses [n][12]: the trial poses as
// uzl_pgo_store would write them; part_inlane / part_stored [sizes[0]]: part_a after chi2_trial_kernel / after chi2_kernel;
// info[4] = {computeScale (sum of part_b), chi2 of the in-lane launch, chi2 of the stored poses, 0}.  sizes[1] = {workgroups of the
// two chi2 launches}; a call with null poses returns sizes only.  The current poses are not touched.
extern "C" UZL_DIAG_EXPORT int uzl_debug_pgo_trial(uzl_pgo* h, const double* dx, double lambda, int32_t* sizes, double* poses,
                                                   double* part_inlane, double* part_stored, double* info)
{
    UZL_GUARD_BEGIN(h)
    if (!h->have_graph) return fail(h, UZL_ERR_STATE, "trial before add_graph/set_graph");
    if (!sizes) return fail(h, UZL_ERR_BAD_ARG, "sizes is required");
    own_streams(h, true);
    hipStream_t s = h->stream;
    if (!poses) {
        UZL_HIP(hipSetDevice(h->cfg.device));
        prepare_optimize(h);
        sizes[0] = (h->nb && h->e) ? g_edges_for(h->D.e_end - h->D.e_begin) : 0;
        UZL_HIP(hipStreamSynchronize(s));
        return UZL_OK;
    }
    if (!dx || !part_inlane || !part_stored || !info) return fail(h, UZL_ERR_BAD_ARG, "dx, the partial arrays and info are required");
    debug_linearize(h);
    const int n = h->n;
    const size_t nb = (size_t)h->nb;
    for (int i = 0; i < 4; i++) info[i] = 0.;
    sizes[0] = 0;
    h->d_out12.reserve((size_t)n * 12);
    if (h->nb == 0 || h->e == 0) {
        k_poses_out(h->cur, n, h->d_out12.p, s);
        UZL_HIP(hipMemcpyAsync(poses, h->d_out12.p, sizeof(double) * 12 * (size_t)n, hipMemcpyDeviceToHost, s));
        UZL_HIP(hipGetLastError());
        UZL_HIP(hipStreamSynchronize(s));
        return UZL_OK;
    }
    PgoDev& D = h->D;
    std::vector<int32_t> v2b((size_t)n);
    UZL_HIP(hipMemcpyAsync(v2b.data(), h->d_v2b.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipStreamSynchronize(s));
    std::vector<double> x(nb * 6, 0.);
    for (int v = 0; v < n; v++) {
        const int32_t a = v2b[(size_t)v];
        if (a < 0 || (size_t)a >= nb) continue;
        for (int c = 0; c < 6; c++) x[(size_t)a * 6 + c] = dx[(size_t)v * 6 + c];
    }
    UZL_HIP(hipMemcpyAsync(D.x, x.data(), sizeof(double) * 6 * nb, hipMemcpyHostToDevice, s));
    k_set_scalar(D.scal + 3, lambda, s);
    const double delta = h->cfg.huber_delta;
    const int go = k_oplus(D, h->cur, h->trial, s);
    const int gc = k_chi2_trial(D, h->cur, delta, s);
    UZL_HIP(hipMemcpyAsync(part_inlane, D.part_a, sizeof(double) * (size_t)gc, hipMemcpyDeviceToHost, s));
    k_finalize(D, gc, go, 0, 1, s);
    double sc[16] = {}, sc2[16] = {};
    UZL_HIP(hipMemcpyAsync(sc, D.scal, sizeof(sc), hipMemcpyDeviceToHost, s));
    const int gs = k_chi2(D, h->trial, delta, s);
    if (gs != gc) { UZL_HIP(hipStreamSynchronize(s)); return fail(h, UZL_ERR_STATE, "trial: the two chi2 launches differ in their grids"); }
    UZL_HIP(hipMemcpyAsync(part_stored, D.part_a, sizeof(double) * (size_t)gs, hipMemcpyDeviceToHost, s));
    k_finalize(D, gs, 0, 0, 0, s);
    UZL_HIP(hipMemcpyAsync(sc2, D.scal, sizeof(sc2), hipMemcpyDeviceToHost, s));
    k_poses_out(h->trial, n, h->d_out12.p, s);
    UZL_HIP(hipMemcpyAsync(poses, h->d_out12.p, sizeof(double) * 12 * (size_t)n, hipMemcpyDeviceToHost, s));
    UZL_HIP(hipGetLastError());
    UZL_HIP(hipStreamSynchronize(s));
    sizes[0] = gc;
    info[0] = sc[5]; info[1] = sc[4]; info[2] = sc2[4];
    return UZL_OK;
    UZL_GUARD_END(h)
}

// ---- the host's pass plan of the device-resident loop without a handle or a device (pgo_lm_pass.hpp; tests/test_lm_pass_plan.py).  One
//      stage per call, one output array per call, stateless (the stage is recomputed per call); *nbytes: in = the room at `out` (ignored
//      when out is null), out = the array's size in bytes.  Arrays a stage does not read may be null.
//   A VIEW (LmPlanView) is one row of vi and one of vd:
//      vi [11] = {phase, need, it, iterations, sync_rebuild, pending, ix, pcg_last, st_lm_trials, max_it, flags[1]}
//      vd [9]  = {last_rel, refresh_rel, rate_ref, rate_last, rate_drop, lambda, lambda_setup[0], lambda_setup[1], tol2}
//   A TRACK (LmSlotTrack) is a row of 8: {job, active, no_history, solve_passes, prev_last, cur_last, seen_trials, n_hist}
//   A PLAN (LmPassPlan) is a row of 7: {flags, want, base, ix, ns_steps, setup_captured, any_start}, its tol2 apart
//   stage 0 lm_plan_pass    iv {nS, first_solve_its, shape_ns_steps, wrong_ix}; vi, vd [nS] views; tr [nS] tracks; hist = the slots' history
//                           rows one after the other (n_hist each).    what 0 plan (i32), 1 tol2 (f64), 2 the tracks afterwards (i32)
//   stage 1 lm_pcg_launches iv {base, want, eager}.                    what 0 {lead, long_first, n_long, rem_first, rem} (i32)
//   stage 2 replay          iv {nS, n_ev, Q, first_solve_its, shape_ns_steps, wrong_ix}; tr [Q][2] = {no_history, n_hist} per job; hist = the
//                           jobs' history rows; ev [n_ev][3] = {kind, slot, job}; vi, vd [n_ev]: the view of event k in row k.
//                           kind 0: plan a pass; 1: slot's look at this view (lm_track_look); 2: load job (-1: idle) into slot, its state this view
//                           what 0 the plans in order (i32), 1 their tol2 (f64), 2 the tracks at the end (i32),
//                           3 {first_solve_its, then per job: trials recorded, their counts} (i32)
//   stage 3 lm_host_batch   iv {prev_pcg_iters, max_it, end_round}: batches until the solve ends in the look of round end_round or max_it is
//                           reached.                                    what 0 the batch sizes (i32)
//   stage 4 lm_history_begin  iv {Q_old, Q_new}; vi = structure generations: Q_old of the last drive, then Q_new of this one; tr [Q_old][2] =
//                           {n_prev, n_cur}; hist = per old job its trial_its_prev row, then its trial_its_cur row.
//                           what 0 per new job {n, counts} of trial_its_prev afterwards, 1 {sizes of trial_its_cur [Q_new], hist_gen [Q_new]} (i32)
//   stage 5 lm_init_rides   iv {flags, any_start, pcg_args_pass, reduced}: a pass with these segments, of a graph launched by value / whose
//                           PCG solves a Schur complement.             what 0 {1: its PCG init goes out in the head's launch} (i32)
extern "C" UZL_DIAG_EXPORT int uzl_debug_lm_pass_plan(int32_t stage, const int32_t* iv, const int32_t* vi, const double* vd, const int32_t* tr, const int32_t* hist,
                                                     const int32_t* ev, int32_t what, void* out, int64_t* nbytes)
{
    if (!iv || !nbytes || what < 0) return UZL_ERR_BAD_ARG;
    try {
        std::vector<int32_t> oi; std::vector<double> od;
        bool f64 = false;
        auto view = [&](int k) {
            const int32_t* a = vi + (size_t)k * kPlanViewInts; const double* b = vd + (size_t)k * kPlanViewDoubles;
            return LmPlanView{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], b[0], b[1], b[2], b[3], b[4], b[5], {b[6], b[7]}, b[8]};
        };
        auto bad_view = [](const LmPlanView& v) { return v.ix < 0 || v.ix > 1 || v.phase < kLmLin || v.phase > kLmAnomaly; };      // (lambda_setup[ix])
        auto put_tracks = [&](const std::vector<LmSlotTrack>& T) {
            for (const LmSlotTrack& t : T) oi.insert(oi.end(), {t.job, t.active ? 1 : 0, t.no_history ? 1 : 0, t.solve_passes, t.prev_last, t.cur_last, t.seen_trials, t.n_hist});
        };
        auto put_plan = [&](const LmPassPlan& P) { oi.insert(oi.end(), {P.flags, P.want, P.base, P.ix, P.ns_steps, P.setup_captured ? 1 : 0, P.any_start ? 1 : 0}); };
        switch (stage) {
        case 0: {
            const int nS = iv[0];
            if (nS < 1 || !vi || !vd || !tr || what > 2) return UZL_ERR_BAD_ARG;
            std::vector<LmPlanView> V((size_t)nS);
            std::vector<LmSlotTrack> T((size_t)nS);
            const int32_t* row = hist;
            for (int sl = 0; sl < nS; sl++) {
                const int32_t* t = tr + 8 * (size_t)sl;
                V[sl] = view(sl);
                if (bad_view(V[sl]) || t[7] < 0 || (t[7] > 0 && !hist)) return UZL_ERR_BAD_ARG;
                LmSlotTrack& K = T[sl];
                K.job = t[0]; K.active = t[1] != 0; K.no_history = t[2] != 0; K.solve_passes = t[3]; K.prev_last = t[4]; K.cur_last = t[5]; K.seen_trials = t[6];
                K.hist = row; K.n_hist = t[7]; row += t[7];
            }
            const LmPassPlan P = lm_plan_pass(V.data(), T.data(), nS, iv[1], iv[2], iv[3] != 0);
            if (what == 0) put_plan(P); else if (what == 1) { od = {P.tol2}; f64 = true; } else put_tracks(T);
            break;
        }
        case 1: {
            if (iv[1] < 1 || iv[0] < 0 || what > 0) return UZL_ERR_BAD_ARG;
            const LmPcgLaunches L = lm_pcg_launches(iv[0], iv[1], iv[2] != 0);
            oi = {L.lead, L.long_first, L.n_long, L.rem_first, L.rem};
            break;
        }
        case 2: {
            const int nS = iv[0], n_ev = iv[1], Q = iv[2];
            if (nS < 1 || n_ev < 0 || Q < 0 || (n_ev > 0 && (!ev || !vi || !vd)) || (Q > 0 && !tr) || what > 3) return UZL_ERR_BAD_ARG;
            LmPassHistory H;
            H.first_solve_its = iv[3];
            H.trial_its_prev.resize((size_t)Q); H.trial_its_cur.resize((size_t)Q);
            const int32_t* row = hist;
            for (int j = 0; j < Q; j++) {
                const int n = tr[2 * j + 1];
                if (n < 0 || (n > 0 && !hist)) return UZL_ERR_BAD_ARG;
                H.trial_its_prev[(size_t)j].assign(row, row + n); row += n;
            }
            std::vector<LmPlanView> V((size_t)nS, LmPlanView{});
            std::vector<LmSlotTrack> T((size_t)nS);
            for (int sl = 0; sl < nS; sl++) V[sl].phase = kLmDone;          // (an unloaded slot: idle)
            for (int k = 0; k < n_ev; k++) {
                const int kind = ev[3 * k], sl = ev[3 * k + 1], job = ev[3 * k + 2];
                if (kind == 0) {
                    const LmPassPlan P = lm_plan_pass(V.data(), T.data(), nS, H.first_solve_its, iv[4], iv[5] != 0);
                    if (what == 0) put_plan(P); else if (what == 1) od.push_back(P.tol2);
                    continue;
                }
                if (sl < 0 || sl >= nS || bad_view(view(k))) return UZL_ERR_BAD_ARG;
                V[sl] = view(k);
                if (kind == 1) {
                    if (T[sl].job < 0) return UZL_ERR_BAD_ARG;
                    (void)lm_track_look(V[sl], T[sl], H);
                } else if (kind == 2) {
                    if (job < -1 || job >= Q) return UZL_ERR_BAD_ARG;
                    lm_track_load(T[sl], job, job >= 0 && tr[2 * job] != 0, H);
                } else return UZL_ERR_BAD_ARG;
            }
            if (what == 1) f64 = true;
            if (what == 2) put_tracks(T);
            if (what == 3) {
                oi.push_back(H.first_solve_its);
                for (const std::vector<int>& c : H.trial_its_cur) { oi.push_back((int32_t)c.size()); oi.insert(oi.end(), c.begin(), c.end()); }
            }
            break;
        }
        case 3: {
            const int prev = iv[0], max_it = iv[1], end_round = iv[2];
            if (max_it < 1 || what > 0) return UZL_ERR_BAD_ARG;
            for (int round = 0, launched = 0;; round++) {                   // (pcg_solve's loop, the look's answer scripted)
                oi.push_back(lm_host_batch(round, prev, max_it, launched));
                launched += oi.back();
                if (round >= end_round || launched >= max_it) break;
            }
            break;
        }
        case 4: {
            const int Qo = iv[0], Qn = iv[1];
            if (Qo < 0 || Qn < 0 || (Qo + Qn > 0 && !vi) || (Qo > 0 && !tr) || what > 1) return UZL_ERR_BAD_ARG;
            LmPassHistory H;
            const int32_t* row = hist;
            for (int j = 0; j < Qo; j++) {
                const int np = tr[2 * j], nc = tr[2 * j + 1];
                if (np < 0 || nc < 0 || (np + nc > 0 && !hist)) return UZL_ERR_BAD_ARG;
                H.trial_its_prev.emplace_back(row, row + np); row += np;
                H.trial_its_cur.emplace_back(row, row + nc); row += nc;
                H.hist_gen.push_back((uint64_t)vi[j]);
            }
            std::vector<uint64_t> gen;
            for (int j = 0; j < Qn; j++) gen.push_back((uint64_t)vi[Qo + j]);
            lm_history_begin(H, gen.data(), Qn);
            if (what == 0) for (const std::vector<int>& c : H.trial_its_prev) { oi.push_back((int32_t)c.size()); oi.insert(oi.end(), c.begin(), c.end()); }
            else {
                for (const std::vector<int>& c : H.trial_its_cur) oi.push_back((int32_t)c.size());
                for (uint64_t g : H.hist_gen) oi.push_back((int32_t)g);
            }
            break;
        }
        case 5: {
            if (what > 0) return UZL_ERR_BAD_ARG;
            LmPassPlan P;
            P.flags = iv[0]; P.any_start = iv[1] != 0;
            oi = {lm_init_rides(P, iv[2] != 0, iv[3] != 0) ? 1 : 0};
            break;
        }
        default: return UZL_ERR_BAD_ARG;
        }
        const void* src = f64 ? (const void*)od.data() : (const void*)oi.data();
        const int64_t bytes = f64 ? (int64_t)od.size() * 8 : (int64_t)oi.size() * 4;
        if (out && bytes) {
            if (*nbytes < bytes) return UZL_ERR_BAD_ARG;
            memcpy(out, src, (size_t)bytes);
        }
        *nbytes = bytes;
        return UZL_OK;
    } catch (const std::bad_alloc&) {
        return UZL_ERR_OOM;
    }
}

// ---- the LM state machine itself without a handle or a device (pgo_lm.hpp; tests/test_lm_decide.py): one application of the head or of
//      the tail's lane 0 to a state the caller wrote, in place.
//   A STATE (LmDev) is one row of si and one of sd:
//      si [32] = {flags[0..3], phase, cur, ix, pass, init_pass, schur_pass, numeric_pass, trial_pass, build_pass, build_ix, build_cur, need,
//                 it, qmax, iterations, max_it, pending, adopted, fresh, pcg_last, sync_rebuild, guarded, st_pcg_iterations, st_lm_trials,
//                 st_precond_builds, st_iterations_done, st_terminated_early, anomaly_code}
//      sd [17] = {lambda, ni, chi_cur, last_rel, lambda_setup[0], lambda_setup[1], rate_ref, rate_last, chi2_initial, tol_f2, eps_t, eps_r,
//                 refresh_rel, tol2, lambda_retake, scal2[3], rate_drop}
//   scal [16]: the solve's scalars (PgoDev::scal), in place
//   stage 0 lm_head_decide   iv {red, phase, pass_flags}; dv {chi, dmax}
//   stage 1 lm_tail_decide   dv {chi_t, sc, ratio}
constexpr int kLmStateInts = 32, kLmStateDoubles = 17;
extern "C" UZL_DIAG_EXPORT int uzl_debug_lm_decide(int32_t stage, int32_t* si, double* sd, double* scal, const int32_t* iv, const double* dv)
{
    if (!si || !sd || !scal || !dv || (stage == 0 && !iv) || stage < 0 || stage > 1) return UZL_ERR_BAD_ARG;
    LmDev L;
    memset(&L, 0, sizeof(L));
    int32_t* const I[kLmStateInts] = {&L.flags[0], &L.flags[1], &L.flags[2], &L.flags[3], &L.phase, &L.cur, &L.ix, &L.pass, &L.init_pass, &L.schur_pass, &L.numeric_pass,
                                      &L.trial_pass, &L.build_pass, &L.build_ix, &L.build_cur, &L.need, &L.it, &L.qmax, &L.iterations, &L.max_it, &L.pending, &L.adopted,
                                      &L.fresh, &L.pcg_last, &L.sync_rebuild, &L.guarded, &L.st_pcg_iterations, &L.st_lm_trials, &L.st_precond_builds,
                                      &L.st_iterations_done, &L.st_terminated_early, &L.anomaly_code};
    double* const F[kLmStateDoubles] = {&L.lambda, &L.ni, &L.chi_cur, &L.last_rel, &L.lambda_setup[0], &L.lambda_setup[1], &L.rate_ref, &L.rate_last, &L.chi2_initial,
                                        &L.tol_f2, &L.eps_t, &L.eps_r, &L.refresh_rel, &L.tol2, &L.lambda_retake, &L.scal2[3], &L.rate_drop};
    for (int k = 0; k < kLmStateInts; k++) *I[k] = si[k];
    for (int k = 0; k < kLmStateDoubles; k++) *F[k] = sd[k];
    if (L.ix < 0 || L.ix > 1) return UZL_ERR_BAD_ARG;             // (lambda_setup[ix])
    if (stage == 0) lm_head_decide(&L, scal, iv[0], iv[1], dv[0], dv[1], iv[2]);
    else lm_tail_decide(&L, scal, dv[0], dv[1], dv[2]);
    for (int k = 0; k < kLmStateInts; k++) si[k] = *I[k];
    for (int k = 0; k < kLmStateDoubles; k++) sd[k] = *F[k];
    return UZL_OK;
}
#endif  // UZL_DIAG
