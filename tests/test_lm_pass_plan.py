"""The host's predictions about the passes of the device-resident LM loop (csrc/pgo_lm_pass.hpp) on the CPU, through
uzl_debug_lm_pass_plan of the diagnostic library (capi.lm_pass_plan): host integer work, no device.  Every comparison is exact equality
against lm_pass_reference.py - the rules restated from their comments - and each named case is the smallest input that reaches its
branch, with the number the rule's comment promises beside it.  A slip here is silent on the device: it never changes a result, it
costs passes."""
import itertools
import os

import numpy as np
import pytest

import lm_pass_reference as LR
from lm_pass_reference import view, track
from uzliti_slam_amd import capi

STEP, LONG = LR.STEP, LR.LONG


@pytest.fixture(autouse=True)
def _needs_the_diagnostic_library():
    if not os.path.exists(capi.DIAG_LIB_PATH):
        pytest.skip("diagnostic library not built")


def plan(views, tracks, **kw):
    """one lm_plan_pass against the reference: the plan and the tracks afterwards"""
    got = capi.lm_pass_plan("plan", views=views, tracks=tracks, **kw)
    ref_plan, ref_tracks = LR.plan_pass(views, tracks, **kw)
    assert got["plan"] == ref_plan, (got["plan"], ref_plan)
    for g, r in zip(got["tracks"], ref_tracks):
        assert {k: g[k] for k in capi.LM_TRACK} == {k: r[k] for k in capi.LM_TRACK} and g["n_hist"] == len(r["hist"])
    return got["plan"]


def one(v, t=None, **kw):
    return plan([v], [t or track()], **kw)


def batch2(v, t=None, **kw):
    return plan([v, v], [t or track(0), dict(t or track(0), job=1)], **kw)


# --------------------------------------------------------------------------------------------------------------- the solve's length
def test_a_fresh_solve_starts_with_two_long_replays():
    assert one(view())["want"] == 2 * LONG and batch2(view())["want"] == 2 * LONG


def test_the_last_optimizes_first_solve_stands_in():
    assert one(view(), first_solve_its=10)["want"] == 11
    assert batch2(view(), first_solve_its=10)["want"] == 12


def test_pass_history_1_ignores_both_histories():
    t = track(no_history=1, hist=[50])
    assert one(view(), t, first_solve_its=10)["want"] == 2 * LONG
    assert one(view(), track(hist=[50]), first_solve_its=10)["want"] == 51          # ... which pass_history 0 takes


def test_one_graph_may_launch_an_odd_count_a_batch_keeps_pairs():
    assert one(view(pcg_last=8))["want"] == 9
    assert batch2(view(pcg_last=8))["want"] == 10
    assert one(view(pcg_last=7))["want"] == 8 and batch2(view(pcg_last=7))["want"] == 8


@pytest.mark.parametrize("last,prev,want", [(12, 10, 15), (50, 10, 67), (10, 12, 11), (10, 0, 11)])
def test_a_rise_is_extrapolated_up_to_16(last, prev, want):
    assert one(view(pcg_last=last, st_lm_trials=2), track(prev_last=prev, cur_last=last, seen_trials=2))["want"] == want


@pytest.mark.parametrize("hist,want", [([5, 5, 40], 41), ([5, 40], 11), ([40], 11)])
def test_history_row_longer_equal_shorter_than_the_trials_so_far(hist, want):
    assert one(view(pcg_last=10, st_lm_trials=2), track(hist=hist, seen_trials=2, cur_last=10))["want"] == want


@pytest.mark.parametrize("max_it,want", [(5, 6), (6, 6), (7, 8)])
def test_the_cap_is_max_it_rounded_up_to_even(max_it, want):
    assert one(view(pcg_last=20, max_it=max_it))["want"] == want


def test_a_pass_holds_two_iterations_at_least():
    assert one(view(pcg_last=20, max_it=1))["want"] == 2
    assert plan([view(phase=LR.DONE)], [track(active=0)])["want"] == 2


# --------------------------------------------------------------------------------------------------------------------- continuations
@pytest.mark.parametrize("nth", [0, 1, 4])
@pytest.mark.parametrize("its,later", [(3, STEP), (30, 16), (500, 4 * LONG)])
def test_continuations_start_short_then_take_half_of_what_the_solve_took(nth, its, later):
    p = one(view(phase=LR.SOLVE, pcg_its=its, pcg_last=9), track(solve_passes=nth))
    assert p["want"] == (STEP if nth == 0 else later) and p["any_start"] == 0 and p["flags"] == 0


def test_base_is_odd_for_one_graph_and_zero_in_a_batch():
    v = view(phase=LR.SOLVE, pcg_its=7)
    assert one(v)["base"] == 7 and batch2(v)["base"] == 0
    assert one(view(phase=LR.RETRY, pcg_its=7))["base"] == 0                         # (a trial that starts: its solve starts at 0)


def test_all_slots_continuing_means_no_head():
    p = batch2(view(phase=LR.SOLVE, pcg_its=20))
    assert p["any_start"] == 0 and p["flags"] == 0
    assert plan([view(phase=LR.SOLVE, pcg_its=20), view(phase=LR.RETRY)], [track(0), track(1)])["any_start"] == 1


# -------------------------------------------------------------------------------------------------------------------------- segments
@pytest.mark.parametrize("need,flags", [(LR.NEED_NUMERIC, 1), (LR.NEED_TRIAL, 1), (LR.NEED_REBUILD, 2), (7, 3), (0, 0)])
def test_need_bits(need, flags):
    assert one(view(phase=LR.NEED_SETUP, need=need, it=3))["flags"] == flags


QUIET = dict(last_rel=1e-6, lambda_setup0=1.0, lambda_setup1=1.0, **{"lambda": 1.0})      # no rule asks for anything


@pytest.mark.parametrize("kw,flags", [
    (dict(it=0), 1), (dict(it=0, sync_rebuild=1), 1),
    (dict(it=3, last_rel=1.0), 2), (dict(it=3, last_rel=1.0, sync_rebuild=1), 1),
    (dict(it=3, last_rel=2e-3), 2), (dict(it=3, last_rel=5e-4), 0), (dict(it=3, last_rel=1e-3), 0),
    (dict(it=3, rate_ref=1.0, rate_last=0.5), 2), (dict(it=3, rate_ref=1.0, rate_last=0.7), 0), (dict(it=3, rate_ref=1.0, rate_last=0.7, rate_drop=0.75), 2),
    (dict(it=3, rate_ref=-1.0, rate_last=0.1), 0),
    (dict(it=19, last_rel=1.0), 0), (dict(it=19, last_rel=1.0, sync_rebuild=1), 1), (dict(it=18, last_rel=1.0), 2)])
def test_linearisation_refresh_rule(kw, flags):
    assert one(view(**dict(QUIET, **kw)))["flags"] == flags


@pytest.mark.parametrize("setup,pending,flags", [((1.0, 10.0), 0, 1), ((1.0, 10.0), 1, 0), ((10.0, 1.0), 0, 0), ((10.0, 1.0), 1, 1)])
def test_lambda_retake_reads_the_copy_the_pass_will_apply(setup, pending, flags):
    v = view(**dict(QUIET, it=2, pending=pending, lambda_setup0=setup[0], lambda_setup1=setup[1], **{"lambda": 100.0}))
    assert one(v)["flags"] == flags
    assert one(dict(v, it=0))["flags"] == 1                                          # (the first linearisation sets up anyway)
    assert one(dict(v, **{"lambda": 32.0 * min(setup)}))["flags"] == 0               # 32x exactly is not yet "grown by more"


@pytest.mark.parametrize("ix,flags", [(1, 1), (0, 0)])
def test_retry_retake(ix, flags):
    v = view(phase=LR.RETRY, it=2, ix=ix, pending=1, lambda_setup0=10.0, lambda_setup1=1.0, **{"lambda": 100.0})
    assert one(v)["flags"] == flags


def test_finished_and_idle_slots_are_ignored():
    views = [view(pcg_last=10), view(phase=LR.NEED_SETUP, need=7, pcg_last=60), view(phase=LR.SOLVE, pcg_its=300)]
    p = plan(views, [track(0), track(1, active=0), track(-1)])
    assert (p["want"], p["flags"], p["any_start"]) == (12, 1, 1)
    assert plan(views, [track(0), track(1), track(2, solve_passes=1)])["want"] == 4 * LONG      # ... which they would not be if active


def test_hierarchy_copy_of_the_pass_and_wrong_ix():
    for ph, ix, pending, want in [(LR.LIN, 0, 1, 1), (LR.LIN, 1, 1, 0), (LR.LIN, 1, 0, 1), (LR.RETRY, 0, 1, 0), (LR.SOLVE, 1, 1, 1)]:
        v = view(phase=ph, ix=ix, pending=pending)
        assert one(v)["ix"] == want and one(v, wrong_ix=True)["ix"] == want ^ 1
    assert one(view(tol2=2.5e-11))["tol2"] == 2.5e-11


@pytest.mark.parametrize("structure,steps", [(4, (2, 2, 4)), (2, (2, 2, 2)), (0, (0, 0, 0))])
def test_set_up_steps_of_the_early_iterations(structure, steps):
    for it in range(3):
        p = one(view(it=it), shape_ns_steps=structure)
        assert p["ns_steps"] == steps[it] and p["setup_captured"] == int(steps[it] == structure)
    p = batch2(view(it=0), shape_ns_steps=structure)                                  # a batch always takes the captured sequence
    assert p["ns_steps"] == structure and p["setup_captured"] == 1


# -------------------------------------------------------------------------------------------------------------------- the PCG launches
def test_pcg_launch_split_sweep():
    for base, want, eager in itertools.product(range(41), range(2, 81), (False, True)):
        L = capi.lm_pass_plan("launches", base=base, want=want, eager=eager)
        assert L == LR.pcg_launches(base, want, eager), (base, want, eager)
        assert L["lead"] + L["n_long"] * LONG + L["rem"] == want and L["rem"] >= 0 and L["lead"] in (0, 1)
        assert L["long_first"] == base + L["lead"] and L["rem_first"] == L["long_first"] + L["n_long"] * LONG      # consecutive from base
        if eager:
            assert L["n_long"] == 0 and L["lead"] == 0 and L["rem"] == want
        else:
            assert L["long_first"] % 2 == 0 and L["rem"] < LONG                       # every replay starts at an even iteration


# ------------------------------------------------------------------------------------------------------------------------- the replay
def check_replay(**kw):
    got = capi.lm_pass_plan("replay", **kw)
    ref = LR.replay(**kw)
    assert got["plans"] == ref["plans"]
    assert got["first_solve_its"] == ref["first_solve_its"] and got["trial_its"] == ref["trial_its"]
    for g, r in zip(got["tracks"], ref["tracks"]):
        assert {k: g[k] for k in capi.LM_TRACK} == {k: r[k] for k in capi.LM_TRACK}
    return got


def test_replay_of_a_rising_solve_and_its_history():
    """config 2's shape: 24 iterations in the first trial, 40 in the second, a continuation in between"""
    ev = [("load", 0, 0, view()), ("plan",),
          ("look", 0, view(phase=LR.LIN, it=1, st_lm_trials=1, pcg_last=24, **QUIET)), ("plan",),
          ("look", 0, view(phase=LR.SOLVE, it=1, st_lm_trials=1, pcg_last=24, pcg_its=25)), ("plan",),
          ("look", 0, view(phase=LR.SOLVE, it=1, st_lm_trials=1, pcg_last=24, pcg_its=29)), ("plan",),
          ("look", 0, view(phase=LR.LIN, it=2, st_lm_trials=2, pcg_last=40, **QUIET)), ("plan",),
          ("look", 0, view(phase=LR.DONE, it=3, st_lm_trials=4, pcg_last=41)), ("plan",)]
    got = check_replay(n_slots=1, jobs=[dict(hist=[])], events=ev)
    assert [p["want"] for p in got["plans"]] == [32, 25, 4, 14, 57, 2]
    assert [p["base"] for p in got["plans"]] == [0, 0, 25, 29, 0, 0]
    assert got["first_solve_its"] == 24 and got["trial_its"] == [[24, 40, 41, 41]]
    # the same walk with that record as its history, and with the history switched off
    again = check_replay(n_slots=1, jobs=[dict(hist=[24, 40, 41, 41])], events=ev, first_solve_its=24)
    assert [p["want"] for p in again["plans"]] == [25, 41, 4, 14, 57, 2]
    off = check_replay(n_slots=1, jobs=[dict(hist=[24, 40, 41, 41], no_history=1)], events=ev, first_solve_its=24)
    assert [p["want"] for p in off["plans"]] == [32, 25, 4, 14, 57, 2]


def test_only_job_0_sets_the_first_solve():
    ev = [("load", 0, 0, view()), ("load", 1, 1, view()), ("plan",),
          ("look", 1, view(phase=LR.LIN, it=1, st_lm_trials=1, pcg_last=30, **QUIET)), ("look", 0, view(phase=LR.LIN, it=1, st_lm_trials=2, pcg_last=12, **QUIET)), ("plan",)]
    got = check_replay(n_slots=2, jobs=[{}, {}], events=ev, first_solve_its=7)
    assert got["first_solve_its"] == 7 and got["trial_its"] == [[12, 12], [30]]
    assert [p["want"] for p in got["plans"]] == [8, 32]


def random_view(rng, prev):
    ph = int(rng.choice([LR.LIN, LR.SOLVE, LR.RETRY, LR.NEED_SETUP, LR.DONE, LR.ANOMALY], p=[0.3, 0.3, 0.15, 0.1, 0.1, 0.05]))
    return view(phase=ph, need=int(rng.integers(0, 8)), it=int(rng.integers(0, 6)), iterations=int(rng.integers(1, 7)), sync_rebuild=int(rng.integers(0, 2)),
                pending=int(rng.integers(0, 2)), ix=int(rng.integers(0, 2)), pcg_last=int(rng.choice([0, int(rng.integers(1, 90))])),
                st_lm_trials=prev["st_lm_trials"] + int(rng.integers(0, 3)), max_it=int(rng.choice([5, 6, 40, 600])), pcg_its=int(rng.integers(0, 700)),
                last_rel=float(rng.choice([1e-6, 1e-3, 2e-3, 1.0])), rate_ref=float(rng.choice([-1.0, 1.0])), rate_last=float(rng.choice([-1.0, 0.5, 0.7])),
                rate_drop=float(rng.choice([0.6, 0.75])), lambda_setup0=float(rng.choice([0.0, 1.0, 10.0])), lambda_setup1=float(rng.choice([0.0, 1.0, 10.0])),
                tol2=float(rng.choice([1e-10, 1e-24])), **{"lambda": float(rng.choice([1.0, 32.0, 100.0, 1e4]))})


@pytest.mark.parametrize("n_slots", [1, 2, 3, 4])
def test_randomised_replay(n_slots):
    """a thousand passes per slot count through the driver's own sequence: plan, look at every unfinished slot, refill by cohorts"""
    rng = np.random.default_rng(20260 + n_slots)
    jobs = [dict(no_history=int(rng.integers(0, 4) == 0), hist=[int(x) for x in rng.integers(1, 90, int(rng.integers(0, 9)))]) for _ in range(400)]
    ev, cur, slot_job, active, next_job, passes = [], [None] * n_slots, [-1] * n_slots, [False] * n_slots, 0, 0

    def load(sl):
        nonlocal next_job
        j = next_job if next_job < len(jobs) else -1
        next_job += j >= 0
        cur[sl] = view(max_it=int(rng.choice([5, 40, 600]))) if j >= 0 else view(phase=LR.DONE)
        slot_job[sl], active[sl] = j, j >= 0
        ev.append(("load", sl, j, cur[sl]))

    for sl in range(n_slots):
        load(sl)
    while any(active) and passes < 1000:
        ev.append(("plan",)); passes += 1
        through = False
        for sl in range(n_slots):
            if active[sl]:
                cur[sl] = random_view(rng, cur[sl])
                ev.append(("look", sl, cur[sl]))
                if cur[sl]["phase"] in (LR.DONE, LR.ANOMALY):
                    active[sl] = False; through = True
        if through and (not any(active) or n_slots == 1):
            for sl in range(n_slots):
                if slot_job[sl] >= 0 and not active[sl]:
                    load(sl)
    got = check_replay(n_slots=n_slots, jobs=jobs, events=ev, first_solve_its=int(rng.integers(0, 30)), shape_ns_steps=4, wrong_ix=False)
    assert len(got["plans"]) == passes == 1000 and next_job > 20
    assert len({(p["flags"], p["any_start"]) for p in got["plans"]}) >= 5 and len({p["want"] for p in got["plans"]}) > 20


# ------------------------------------------------------------------------------------------------------------------------ the hand-over
def test_history_hand_over():
    old = [dict(gen=5, prev=[1, 2], cur=[10, 11, 12]), dict(gen=9, prev=[], cur=[20])]
    for new in ([5, 9], [5, 10], [5], [5, 9, 9], []):
        got = capi.lm_pass_plan("handover", old=old, new_gens=new)
        assert got == LR.handover(old, new), new
    assert capi.lm_pass_plan("handover", old=old, new_gens=[5, 9])["prev"] == [[10, 11, 12], [20]]
    assert capi.lm_pass_plan("handover", old=old, new_gens=[9, 5])["prev"] == [[], []]
    assert capi.lm_pass_plan("handover", old=[], new_gens=[3]) == dict(prev=[[]], cur_sizes=[0], hist_gen=[3])


# ------------------------------------------------------------------------------------------------------- the host-driven loop's batches
@pytest.mark.parametrize("prev", [0, 1, 3, 4, 40, 41])
@pytest.mark.parametrize("max_it", [1, 4, 7, 600])
@pytest.mark.parametrize("end_round", [0, 2, 5])
def test_host_driven_batches(prev, max_it, end_round):
    got = capi.lm_pass_plan("host_batches", prev=prev, max_it=max_it, end_round=end_round)
    assert got == LR.host_batches(prev, max_it, end_round)
    assert all(b > 0 and b % STEP == 0 for b in got) and sum(got[:-1]) < max_it


def test_host_driven_batches_by_hand():
    assert capi.lm_pass_plan("host_batches", prev=0, max_it=600, end_round=5) == [16, 4, 4, 16, 16, 16]
    assert capi.lm_pass_plan("host_batches", prev=40, max_it=600, end_round=2) == [40, 4, 4]           # 38 + 1, in fours
    assert capi.lm_pass_plan("host_batches", prev=41, max_it=600, end_round=0) == [40]                 # 38.95 -> 38, + 1
    assert capi.lm_pass_plan("host_batches", prev=1, max_it=600, end_round=0) == [4]
    assert capi.lm_pass_plan("host_batches", prev=40, max_it=7, end_round=5) == [8]                    # clipped to max_it, rounded to a replay
