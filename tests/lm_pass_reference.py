"""What the host predicts about the passes of the device-resident LM loop (csrc/pgo_lm_pass.hpp), restated from the rules' comments:
the reference of tests/test_lm_pass_plan.py.  Views, tracks and plans are the dicts of capi.lm_pass_plan."""
LIN, SOLVE, RETRY, NEED_SETUP, DONE, ANOMALY = range(6)              # LmPhase
NEED_NUMERIC, NEED_TRIAL, NEED_REBUILD = 1, 2, 4                     # LmNeed
PASS_SETUP, PASS_REBUILD = 1, 2                                      # LmPassFlags
STEP, LONG = 4, 16                                                   # a short / a long PCG replay, in iterations
RETAKE = 32.0                                                        # lambda grown by this much since the inverses were taken
MAX_RISE = 16


def view(**kw):
    """a snapshot as the host reads it; what is not given is what a fresh graph has"""
    v = dict(phase=LIN, need=0, it=0, iterations=20, sync_rebuild=0, pending=0, ix=0, pcg_last=0, st_lm_trials=0, max_it=600, pcg_its=0,
             last_rel=1e300, refresh_rel=1e-3, rate_ref=-1.0, rate_last=-1.0, rate_drop=0.6, lambda_setup0=0.0, lambda_setup1=0.0, tol2=1e-10)
    v["lambda"] = 0.0
    v.update(kw)
    return v


def track(job=0, active=None, no_history=0, solve_passes=0, prev_last=0, cur_last=0, seen_trials=0, hist=()):
    return dict(job=job, active=int(job >= 0 if active is None else active), no_history=int(no_history), solve_passes=solve_passes, prev_last=prev_last,
                cur_last=cur_last, seen_trials=seen_trials, hist=list(hist))


def wants_refresh(v):
    """lazy refresh: always at the first linearisation; later when the last step still moved chi2 or the PCG rate has fallen - but a
    rebuild that runs ahead is for the NEXT iteration, so none in the last one"""
    if v["it"] == 0:
        return True
    stale = v["last_rel"] > v["refresh_rel"] or (v["rate_ref"] > 0 and v["rate_last"] > 0 and v["rate_last"] < v["rate_drop"] * v["rate_ref"])
    return stale and (bool(v["sync_rebuild"]) or v["it"] + 1 < v["iterations"])


def ns_steps_at(structure_steps, it):
    """two Newton-Schulz steps in the first two linearisations where the structure asks for more"""
    return 2 if (structure_steps > 2 and it < 2) else structure_steps


def segments(v):
    lam_setup = (v["lambda_setup0"], v["lambda_setup1"])
    f = 0
    if v["phase"] == NEED_SETUP:
        if v["need"] & (NEED_NUMERIC | NEED_TRIAL):
            f |= PASS_SETUP
        if v["need"] & NEED_REBUILD:
            f |= PASS_REBUILD
    elif v["phase"] == LIN:
        if wants_refresh(v):
            f |= PASS_SETUP if (v["it"] == 0 or v["sync_rebuild"]) else PASS_REBUILD
        in_use = v["ix"] ^ 1 if v["pending"] else v["ix"]            # a copy rebuilt ahead is adopted by this linearisation
        if v["it"] > 0 and v["lambda"] > RETAKE * lam_setup[in_use]:
            f |= PASS_SETUP
    elif v["phase"] == RETRY:
        if v["lambda"] > RETAKE * lam_setup[v["ix"]]:
            f |= PASS_SETUP
    return f


def launches_for(count, n_slots):
    """a solve of `count` iterations is declared done by launch count + 1; a batch keeps whole pairs"""
    return count + 1 if n_slots == 1 else 2 * (count // 2 + 1)


def solve_length(v, t, n_slots, first_solve_its):
    hist_ok = not t["no_history"]
    if v["pcg_last"] > 0:
        expect = v["pcg_last"]
        if 0 < t["prev_last"] < expect:                              # the counts rise: so will the next
            expect += min(expect - t["prev_last"], MAX_RISE)
        w = launches_for(expect, n_slots)
    elif first_solve_its > 0 and hist_ok:
        w = launches_for(first_solve_its, n_slots)
    else:
        w = 2 * LONG
    if hist_ok and 0 <= v["st_lm_trials"] < len(t["hist"]):
        w = max(w, launches_for(t["hist"][v["st_lm_trials"]], n_slots))
    return min(w, v["max_it"] + v["max_it"] % 2)


def continuation_length(v, t):
    if t["solve_passes"] == 0:
        return STEP
    half = (v["pcg_its"] // 2 + 1) // 2 * 2
    return min(max(STEP, half), 4 * LONG)


def plan_pass(views, tracks, first_solve_its=0, shape_ns_steps=0, wrong_ix=False):
    """-> (plan, tracks afterwards)"""
    n = len(views)
    tracks = [dict(t) for t in tracks]
    flags, want, any_start = 0, 0, False
    for v, t in zip(views, tracks):
        if not t["active"]:
            continue
        if v["phase"] == SOLVE:
            w = continuation_length(v, t)
            t["solve_passes"] += 1
        else:
            any_start = True
            t["solve_passes"] = 0
            flags |= segments(v)
            w = solve_length(v, t, n, first_solve_its)
        want = max(want, w)
    v0 = views[0]
    steps = ns_steps_at(shape_ns_steps, v0["it"]) if n == 1 else shape_ns_steps
    ix = (v0["ix"] ^ 1) if (v0["phase"] == LIN and v0["pending"]) else v0["ix"]
    plan = dict(flags=flags, want=max(2, want), base=v0["pcg_its"] if (n == 1 and tracks[0]["job"] >= 0 and v0["phase"] == SOLVE) else 0,
                ix=ix ^ (1 if wrong_ix else 0), ns_steps=steps, setup_captured=int(steps == shape_ns_steps), any_start=int(any_start), tol2=v0["tol2"])
    return plan, tracks


def look(v, t, state):
    """a slot's new snapshot: state = dict(first_solve_its, trial_its [job])"""
    if v["st_lm_trials"] > t["seen_trials"]:
        t["seen_trials"] = v["st_lm_trials"]
        t["prev_last"], t["cur_last"] = t["cur_last"], v["pcg_last"]
    if t["job"] == 0 and v["st_lm_trials"] == 1 and v["pcg_last"] > 0:
        state["first_solve_its"] = v["pcg_last"]
    row = state["trial_its"][t["job"]]
    row.extend([v["pcg_last"]] * (v["st_lm_trials"] - len(row)))     # trials that ended since the last look, at the count the host saw
    if v["phase"] in (DONE, ANOMALY):
        t["active"] = 0


def replay(n_slots, jobs, events, first_solve_its=0, shape_ns_steps=0, wrong_ix=False):
    state = dict(first_solve_its=first_solve_its, trial_its=[[] for _ in jobs])
    views = [view(phase=DONE) for _ in range(n_slots)]
    tracks = [track(job=-1) for _ in range(n_slots)]
    plans = []
    for e in events:
        if e[0] == "plan":
            p, tracks = plan_pass(views, tracks, state["first_solve_its"], shape_ns_steps, wrong_ix)
            plans.append(p)
        elif e[0] == "look":
            views[e[1]] = e[2]
            look(e[2], tracks[e[1]], state)
        else:
            _, sl, job, v = e
            views[sl] = v
            tracks[sl] = track(job=job, no_history=jobs[job].get("no_history", 0) if job >= 0 else 0, hist=jobs[job].get("hist", ()) if job >= 0 else ())
    return dict(plans=plans, tracks=tracks, first_solve_its=state["first_solve_its"], trial_its=state["trial_its"])


def pcg_launches(base, want, eager):
    """captured replays hold LONG iterations and start at an even one; everything else goes out launch by launch"""
    if eager:
        return dict(lead=0, long_first=base, n_long=0, rem_first=base, rem=want)
    lead = base % 2
    n_long = (want - lead) // LONG
    return dict(lead=lead, long_first=base + lead, n_long=n_long, rem_first=base + lead + n_long * LONG, rem=want - lead - n_long * LONG)


def host_batches(prev, max_it, end_round):
    """the host-driven solve: 95 % of the previous solve + 1 in whole short replays (no predecessor: one long), two short, then long;
    clipped to what max_it leaves, in whole short replays"""
    whole = lambda k: -(-k // STEP) * STEP
    out, launched, r = [], 0, 0
    while True:
        ask = (max(STEP, whole(prev * 95 // 100 + 1)) if prev > 0 else LONG) if r == 0 else (STEP if r <= 2 else LONG)
        out.append(whole(max(1, min(ask, max_it - launched))))
        launched += out[-1]
        if r >= end_round or launched >= max_it:
            return out
        r += 1


def handover(old, new_gens):
    """the counts the last drive recorded are this drive's history iff every job is the same structure generation again"""
    same = [j["gen"] for j in old] == list(new_gens)
    prev = [list(j["cur"]) for j in old] if same else [[] for _ in new_gens]
    return dict(prev=prev, cur_sizes=[0] * len(new_gens), hist_gen=list(new_gens))
