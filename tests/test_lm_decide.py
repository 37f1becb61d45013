"""The decisions of the Levenberg-Marquardt loop (csrc/pgo_lm.hpp: lm_head_decide in front of a trial, lm_tail_decide behind its
evaluation) on the CPU, through uzl_debug_lm_decide of the diagnostic library (capi.lm_decide): no handle, no device.  Both LM loops
drive this one state machine - lane 0 of lm_head_kernel / lm_tail_kernel on the device, do_optimize_host on the host - so a slip here
moves both, and tests/test_lm_loops_gpu.py (the two loops agree) cannot see it.  Every expectation is a known answer read off a rule's
statement - g2o's OptimizationAlgorithmLevenberg::solve and DESIGN.md section 5 - with inputs chosen so that the answer is exact."""
import math
import os

import numpy as np
import pytest

from uzliti_slam_amd import capi

PH = capi.LM_PHASES
SETUP, REBUILD = capi.LM_PASS_SETUP, capi.LM_PASS_REBUILD
TOL_F2, EPS_T, EPS_R, TOL2 = 1e-4, 1e-5, 1e-6, 1e-10


@pytest.fixture(autouse=True)
def _needs_the_diagnostic_library():
    if not os.path.exists(capi.DIAG_LIB_PATH):
        pytest.skip("diagnostic library not built")


def state(**kw):
    """a loop's state as it starts (lm_initial_state), with the solve's constants of a default configuration"""
    s = dict(done=1, phase=PH["lin"], init_pass=-1, schur_pass=-1, numeric_pass=-1, trial_pass=-1, build_pass=-1, iterations=10, max_it=100, ni=2., last_rel=1e300,
             rate_ref=-1., rate_last=-1., tol_f2=TOL_F2, eps_t=EPS_T, eps_r=EPS_R, refresh_rel=1e-3, rate_drop=0.6, tol2=TOL2, lambda_retake=32.)
    s.update(kw)
    return s


def head(s, phase=None, pass_flags=SETUP | REBUILD, red=False, chi=0., dmax=0., scal=None):
    return capi.lm_decide("head", s, scal, red=red, phase=s["phase"] if phase is None else phase, pass_flags=pass_flags, chi=chi, dmax=dmax)


def tail(s, chi_t=0., sc=0., ratio=0., scal=None):
    return capi.lm_decide("tail", s, scal, chi_t=chi_t, sc=sc, ratio=ratio)


def full(s):
    """a state with every key, as lm_decide returns it"""
    return {k: s.get(k, 0) for k in capi.LM_STATE_INTS + capi.LM_STATE_DOUBLES}


def changed(before, after):
    b = full(before)
    return {k for k in b if b[k] != after[k]}


# ------------------------------------------------------------------------------------------------------------------------ the head
@pytest.mark.parametrize("red", [False, True])
def test_first_linearisation_with_the_setup_in_the_pass(red):
    chi, dmax = 12.5, 4000.
    a, scal = head(state(), pass_flags=SETUP, red=red, chi=chi, dmax=dmax)
    assert a["lambda"] == 1e-5 * dmax and a["ni"] == 2.                                          # computeLambdaInit: tau * max diag
    assert a["chi_cur"] == chi and a["chi2_initial"] == chi
    assert a["pass"] == 1 and a["numeric_pass"] == 1 and a["trial_pass"] == 1 and a["init_pass"] == 1
    assert a["schur_pass"] == (1 if red else -1) and a["build_pass"] == -1
    assert a["fresh"] == 1 and a["st_precond_builds"] == 1 and a["lambda_setup0"] == a["lambda"] and a["lambda_setup1"] == 0.
    assert (a["done"], a["pcg_its"], a["breakdown"], a["look"]) == (0, 0, 0, 0)
    assert a["phase"] == PH["solve"] and a["need"] == 0 and a["pending"] == 0 and a["adopted"] == 0 and a["ix"] == 0 and a["qmax"] == 0
    assert scal[2] == 1. and scal[3] == a["lambda"] and scal[8] == TOL_F2 and scal[12] == EPS_T and scal[13] == EPS_R
    assert scal[4] == chi and scal[6] == dmax


@pytest.mark.parametrize("red", [False, True])
def test_first_linearisation_without_the_setup_stalls_and_the_next_pass_starts_the_solve(red):
    a, scal = head(state(), pass_flags=0, red=red, chi=3., dmax=200.)
    assert a["phase"] == PH["need_setup"] and a["need"] == capi.LM_NEED_NUMERIC | capi.LM_NEED_TRIAL and a["done"] == 1
    assert a["st_precond_builds"] == 1 and a["pass"] == 1
    assert a["numeric_pass"] == -1 and a["trial_pass"] == -1 and a["init_pass"] == -1 and a["schur_pass"] == (1 if red else -1)
    assert scal[3] == 1e-5 * 200.                                                                 # (its Schur reduction runs in the pass that stalled)
    b, scal = head(a, pass_flags=SETUP, red=red, scal=scal)
    assert b["phase"] == PH["solve"] and b["pass"] == 2 and b["numeric_pass"] == 2 and b["trial_pass"] == 2 and b["init_pass"] == 2
    assert b["st_precond_builds"] == 1 and b["schur_pass"] == (1 if red else -1)                  # neither counted nor reduced again
    assert b["lambda"] == a["lambda"] and b["chi_cur"] == 3. and b["fresh"] == 1 and b["need"] == 0 and b["done"] == 0
    assert b["lambda_setup0"] == b["lambda"]


def _third_iteration(**kw):
    """it = 3 of 10, chi2 still moving (last_rel > refresh_rel), rebuilds ahead, inverses of copy 0 taken at the current lambda"""
    s = state(it=3, cur=1, sync_rebuild=0, last_rel=0.5, lambda_setup0=0.02, lambda_setup1=0.005, chi_cur=9., **{"lambda": 0.02, "pass": 7})
    s.update(kw)
    return s


def test_a_rebuild_ahead_goes_into_the_other_copy_with_this_iterations_lambda():
    a, _ = head(_third_iteration())
    assert a["build_pass"] == 8 and a["build_ix"] == 1 and a["build_cur"] == 1 and a["scal2_3"] == 0.02
    assert a["lambda_setup1"] == 0.02 and a["lambda_setup0"] == 0.02 and a["pending"] == 1 and a["st_precond_builds"] == 1
    assert a["numeric_pass"] == -1 and a["trial_pass"] == -1 and a["init_pass"] == 8 and a["ix"] == 0
    assert a["fresh"] == 0 and a["phase"] == PH["solve"] and a["chi_cur"] == 9. and a["lambda"] == 0.02
    b, _ = head(_third_iteration(), pass_flags=SETUP)                                             # a pass without the rebuild segment
    assert b["phase"] == PH["need_setup"] and b["need"] == capi.LM_NEED_REBUILD and b["pending"] == 0 and b["build_pass"] == -1


def test_no_rebuild_ahead_in_the_last_iteration_a_synchronous_one_runs():
    a, _ = head(_third_iteration(it=9))
    assert a["st_precond_builds"] == 0 and a["pending"] == 0 and a["build_pass"] == -1 and a["numeric_pass"] == -1 and a["phase"] == PH["solve"]
    b, _ = head(_third_iteration(it=9, sync_rebuild=1))
    assert b["st_precond_builds"] == 1 and b["numeric_pass"] == 8 and b["trial_pass"] == 8 and b["build_pass"] == -1 and b["pending"] == 0


def test_adoption_flips_the_copy_and_makes_the_first_trial_fresh():
    s = state(it=2, pending=1, ix=0, last_rel=0., lambda_setup0=0.01, lambda_setup1=0.01, **{"lambda": 0.01, "pass": 4})
    a, _ = head(s)
    assert a["ix"] == 1 and a["adopted"] == 1 and a["pending"] == 0 and a["fresh"] == 1
    assert a["trial_pass"] == -1 and a["numeric_pass"] == -1 and a["st_precond_builds"] == 0
    a["phase"] = PH["retry"]; a["qmax"] = 1                                                        # its second trial is not
    b, _ = head(a)
    assert b["fresh"] == 0 and b["ix"] == 1 and b["adopted"] == 1


@pytest.mark.parametrize("phase,qmax", [("retry", 2), ("lin", 0)])
def test_the_inverses_are_retaken_beyond_32_times_their_lambda(phase, qmax):
    def at(lam):
        return head(state(it=2, phase=PH[phase], qmax=qmax, last_rel=0., lambda_setup0=1., **{"lambda": lam, "pass": 5}))[0]
    a = at(33.)
    assert a["trial_pass"] == 6 and a["numeric_pass"] == -1 and a["lambda_setup0"] == 33. and a["fresh"] == 1 and a["st_precond_builds"] == 0
    b = at(32.)                                                                                    # exactly 32 x: kept
    assert b["trial_pass"] == -1 and b["lambda_setup0"] == 1. and b["fresh"] == 0 and b["phase"] == PH["solve"] and b["init_pass"] == 6


def test_the_rate_rule_alone_triggers_a_refresh():
    def at(rate_last):
        return head(state(it=4, sync_rebuild=1, last_rel=0., rate_ref=1., rate_last=rate_last, lambda_setup0=1., **{"lambda": 1.}))[0]
    a = at(0.59)                                                                                   # below 0.6 of the fresh rate
    assert a["st_precond_builds"] == 1 and a["numeric_pass"] == 1 and a["trial_pass"] == 1 and a["fresh"] == 1
    b = at(0.61)
    assert b["st_precond_builds"] == 0 and b["numeric_pass"] == -1 and b["trial_pass"] == -1 and b["fresh"] == 0


@pytest.mark.parametrize("phase", ["solve", "done", "anomaly"])
def test_a_graph_that_starts_no_trial_only_counts_the_pass(phase):
    s = state(phase=PH[phase], it=2, done=0, pcg_its=14, pending=1, last_rel=0.5, **{"lambda": 0.3, "pass": 3})
    scal0 = np.arange(16, dtype=np.float64)
    a, scal = head(s, red=True, chi=5., dmax=7., scal=scal0)
    assert changed(s, a) == {"pass"} and a["pass"] == 4 and np.array_equal(scal, scal0)


# ------------------------------------------------------------------------------------------------------------------------ the tail
def solved(**kw):
    """a trial whose solve has ended: 20 PCG iterations, chi2 10 at the linearisation point"""
    s = state(phase=PH["solve"], done=1, pcg_its=20, it=2, chi_cur=10., st_pcg_iterations=100, st_lm_trials=4, **{"lambda": 0.3})
    s.update(kw)
    return s


SC = 7.999
assert SC + 1e-3 == 8.                                              # computeScale + 1e-3: the rho of the cases below is exact


def test_a_solve_below_the_cap_goes_on_one_at_the_cap_is_anomaly_1():
    s = solved(done=0, pcg_its=99)
    a, _ = tail(s, chi_t=1., sc=SC)
    assert changed(s, a) == set()
    s = solved(done=0, pcg_its=100)
    a, _ = tail(s, chi_t=1., sc=SC)
    assert changed(s, a) == {"phase", "anomaly_code", "done"} and a["phase"] == PH["anomaly"] and a["anomaly_code"] == 1 and a["done"] == 1


@pytest.mark.parametrize("breakdown,guarded,ratio,code", [(1, 0, 0., 2), (2, 1, 0., 4), (0, 1, 0.3, 3), (0, 1, float("nan"), 3)])
def test_breakdown_wrong_copy_and_residual_guard_are_anomalies(breakdown, guarded, ratio, code):
    s = solved(breakdown=breakdown, guarded=guarded)
    a, scal = tail(s, chi_t=1., sc=SC, ratio=ratio)
    assert changed(s, a) == {"phase", "anomaly_code"} and a["phase"] == PH["anomaly"] and a["anomaly_code"] == code      # the trial is not evaluated
    if not breakdown:
        assert scal[7] == ratio or (math.isnan(ratio) and math.isnan(scal[7]))


@pytest.mark.parametrize("guarded,ratio", [(1, 0.25), (0, 1e6)])
def test_a_ratio_at_the_guard_or_an_unguarded_large_one_passes(guarded, ratio):
    a, scal = tail(solved(guarded=guarded), chi_t=6., sc=SC, ratio=ratio)
    assert a["phase"] == PH["lin"] and a["anomaly_code"] == 0 and a["st_lm_trials"] == 5 and scal[7] == ratio


@pytest.mark.parametrize("chi_t,factor", [(6., 2. / 3.), (2., 1. / 3.)])            # rho = 0.5: 1 - (2 rho - 1)^3 = 1, capped at 2/3; rho = 1: 0, raised to 1/3
def test_an_accepted_step(chi_t, factor):
    s = solved(ni=8., qmax=1, cur=0)
    a, scal = tail(s, chi_t=chi_t, sc=SC)
    assert a["lambda"] == 0.3 * factor and a["ni"] == 2.
    assert a["cur"] == 1 and a["chi_cur"] == chi_t and a["last_rel"] == (10. - chi_t) / chi_t
    assert a["it"] == 3 and a["qmax"] == 0 and a["phase"] == PH["lin"] and a["st_iterations_done"] == 3 and a["st_terminated_early"] == 0
    assert a["st_pcg_iterations"] == 120 and a["st_lm_trials"] == 5 and a["pcg_last"] == 20
    assert scal[4] == chi_t and scal[5] == SC
    b, _ = tail(solved(it=9), chi_t=chi_t, sc=SC)                                 # the last iteration asked for
    assert b["phase"] == PH["done"] and b["it"] == 10 and b["st_iterations_done"] == 10 and b["st_terminated_early"] == 0 and b["cur"] == 1


@pytest.mark.parametrize("ni", [2., 4.])
def test_a_rejected_step_is_tried_again_with_a_larger_lambda(ni):
    s = solved(ni=ni, cur=1)
    a, _ = tail(s, chi_t=12., sc=SC)
    assert a["lambda"] == 0.3 * ni and a["ni"] == 2. * ni and a["phase"] == PH["retry"] and a["qmax"] == 1
    assert a["cur"] == 1 and a["chi_cur"] == 10. and a["it"] == 2 and a["st_iterations_done"] == 0 and a["last_rel"] == 1e300
    assert a["st_lm_trials"] == 5 and a["st_pcg_iterations"] == 120


def test_the_tenth_rejection_and_rho_0_terminate():
    a, _ = tail(solved(qmax=9), chi_t=12., sc=SC)
    assert a["qmax"] == 10 and a["phase"] == PH["done"] and a["st_terminated_early"] == 1 and a["st_iterations_done"] == 3 and a["it"] == 2
    b, _ = tail(solved(), chi_t=10., sc=SC)                                        # rho == 0: no step, Terminate
    assert b["phase"] == PH["done"] and b["st_terminated_early"] == 1 and b["st_iterations_done"] == 3 and b["it"] == 2
    assert b["cur"] == 0 and b["lambda"] == 0.3 * 2. and b["ni"] == 4.


@pytest.mark.parametrize("chi_t,phase", [(float("inf"), "retry"), (float("nan"), "lin"), (float("-inf"), "lin")])
def test_a_non_finite_trial_chi2_is_a_rejection(chi_t, phase):
    a, _ = tail(solved(), chi_t=chi_t, sc=SC)
    assert a["cur"] == 0 and a["chi_cur"] == 10. and a["lambda"] == 0.3 * 2. and a["ni"] == 4. and a["last_rel"] == 1e300
    assert a["phase"] == PH[phase] and a["st_terminated_early"] == 0          # (rho = -inf: another trial; rho not < 0: g2o's trial loop ends)


RZ_STOP, RZ_END = 5e-14, 5e-9                                                    # r.M^-1 r: the stop threshold (scal[1]) and the value at the end (scal[0])


def _rates(its, **kw):
    scal = np.zeros(16)
    scal[0], scal[1] = RZ_END, RZ_STOP
    return tail(solved(pcg_its=its, **kw), chi_t=6., sc=SC, scal=scal)[0]


def test_fewer_than_16_iterations_leave_the_rates_alone():
    a = _rates(15, fresh=1)
    assert a["rate_last"] == -1. and a["rate_ref"] == -1.
    b = _rates(15, rate_last=0.4, rate_ref=0.7)
    assert b["rate_last"] == 0.4 and b["rate_ref"] == 0.7


def test_the_rate_is_the_contraction_per_iteration_and_the_reference_follows_fresh_operators_only():
    rz0 = RZ_STOP / (TOL2 * TOL_F2)                                             # scal[1] = pcg_tol^2 * tol_f2 * (r_0.M^-1 r_0)
    want = math.log(rz0 / RZ_END) / 16
    a = _rates(16, fresh=1, rate_ref=0.7)
    assert abs(a["rate_last"] - want) <= 1e-12 * want and a["rate_ref"] == a["rate_last"]
    b = _rates(16, fresh=0)                                                      # no reference yet
    assert abs(b["rate_last"] - want) <= 1e-12 * want and b["rate_ref"] == b["rate_last"]
    c = _rates(16, fresh=0, rate_ref=0.7)
    assert abs(c["rate_last"] - want) <= 1e-12 * want and c["rate_ref"] == 0.7
