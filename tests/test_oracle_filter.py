"""CPU tests of the edge-filter oracle (oracle/uzl_oracle_filter.c) against the hand-made known answers of
filter_cases.py (the cases this file held first; test_filter_cases_reference.py runs all of them, on FilterRef too) and against the
pure-Python restatement in np_reference.FilterRef (TransformationFilter, transformation_filter.cpp:43-350)."""
import numpy as np

from uzliti_slam_amd import synth
import filter_cases
from filter_cases import E, S, _line_edges          # noqa: F401  (test_filter_gpu.py imports them from here)
from filter_common import assert_same_state, play
from np_reference import FilterRef


def test_cluster_window_and_bounds(oracle):
    filter_cases.CASES["cluster_window_and_bounds"](oracle.Filter, oracle)


def test_merge_and_max_cluster_size(oracle):
    filter_cases.CASES["merge_and_max_cluster_size"](oracle.Filter, oracle)


def test_consensus_counter_and_remove(oracle):
    filter_cases.CASES["consensus_counter_and_remove"](oracle.Filter, oracle)


def test_update_keeps_validity_and_stamps(oracle):
    filter_cases.CASES["update_keeps_validity_and_stamps"](oracle.Filter, oracle)


def test_calc_valid_edges_gates_and_verdict(oracle):
    filter_cases.CASES["calc_valid_edges_gates_and_verdict"](oracle.Filter, oracle)


def test_valid_edges_thinning(oracle):
    filter_cases.CASES["valid_edges_thinning"](oracle.Filter, oracle)


def test_failed_ransac_falls_back_to_identity_count(oracle):
    filter_cases.CASES["failed_ransac_falls_back_to_identity_count"](oracle.Filter, oracle)


def test_oracle_equals_python_restatement(oracle):
    scn = synth.make_filter_scenario(160, 420, seed=11)
    cfg = dict(max_dt=5.0, min_size=6.0, max_cluster_size=30, ransac_iterations=60, max_error=0.3, seed=9)
    o = oracle.Filter(**cfg)
    r = FilterRef(**cfg)
    o.set_sensors(scn["sensors"]); r.set_sensors(scn["sensors"])

    def ransac(P, Q, job_id):
        res = oracle.prosac(P.T, Q.T, cfg["max_error"], cfg["ransac_iterations"], 1.0, do_prosac=False, seed=cfg["seed"], job_id=job_id)
        _, s = oracle.consensus3d(P.T, Q.T, res["T"], cfg["max_error"])
        return res["T"], s

    def check(rnd, stage):
        assert_same_state(o.clusters(), r.state(), with_eval=False, tag=(rnd, stage))
        assert np.array_equal(o.all_edges(), r.all_edges())
        if stage == "calc":
            assert np.array_equal(o.valid_edges(), r.valid_edges())
            for co, cr in zip(o.clusters(with_eval=True), r.clusters):
                if co["evaluations"] and hasattr(cr, "lastP") and len(cr.lastP) == len(co["P"]):
                    assert co["P"].tobytes() == cr.lastP.tobytes() and co["Q"].tobytes() == cr.lastQ.tobytes()

    play([o, r], scn, rounds=5, seed=2, check=check, calc=lambda f: f.calc_valid_edges(ransac) if isinstance(f, FilterRef) else f.calc_valid_edges())
    st = o.clusters()
    assert max(c["size"] for c in st) >= 12 and sum(c["evaluations"] for c in st) >= 5      # the scenario exercises the path
    assert len(o.valid_edges()) > 0
