"""The estimator's RANSAC core (stages M6-M9 of estimate_kernel) on the device at the inputs of tests/ransac_cases.py: degenerate
geometry, clouds far from the origin and at extreme scales, non-finite operands, exceptional thresholds and break percentages,
stops at the edges of the 256-hypothesis rounds, and the edge between the LDS tile and HBM scratch.  tests/test_ransac_cases_cpu.py
shows that each case reaches what it is named after.

The device is compared with the CPU oracle bit for bit in T, consensus, iterations_run, mask and mse.  A NaN equals a NaN
whatever its sign and payload; that is the only relaxation (ransac_cases.canonical).  Every small case runs twice: next to a filler
problem of the largest size that still fits the LDS tile at the case's iteration count (2716 points at 200 iterations), and next
to one two points larger, which moves every problem of the call to HBM scratch.  Both must give the oracle's bytes.  The same
calls are repeated in a child process on the diagnostic library with UZL_VOTE_VALU=1 (votes on the vector ALU); its digests must
equal those of the matrix-core votes, which tells a fault of the MFMA identity from a fault of the recipe.

Measured on an MI355X: every class equals the oracle in both placements and in both vote configurations, the estimator case and
the odd-stride call included; no class needed a change to the kernel or to the oracle.  In particular the device returns, like the
oracle, consensus 0 with mse = NaN, a finite T and the identity information matrix where the float refit loses the consensus
(cloud offset by 1e6), T = I and consensus 0 where every float pose is NaN (2^500, offset 1e9), and all points as inliers at distance 0
where the coordinates are f64 denormals (2^-1040, 2^-1070: every squared distance underflows to zero)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ransac_cases as RC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def matcher(capi):
    m = capi.Match(seed=RC.SEED)
    yield m
    m.close()


@pytest.fixture(scope="module")
def device(matcher):
    """Every case in both placements, once for the whole module."""
    return RC.device_results(matcher)


@pytest.fixture(scope="module")
def wanted(oracle):
    return {c.name: RC.run_on_oracle(oracle, c) for c in RC.all_cases()}


def _describe(r):
    return dict(consensus=r["consensus"], iterations_run=r["iterations_run"], mse=r["mse"], inliers=int(np.sum(r["mask"])),
                T=np.asarray(r["T"]).reshape(-1).tolist())


@pytest.mark.parametrize("cls", RC.SMALL_CLASSES)
def test_class_matches_oracle_in_both_placements(device, wanted, cls):
    bad = []
    for c in RC.CLASSES[cls]():
        for place in ("lds", "hbm"):
            diff = RC.differing_fields(device[c.name, place], wanted[c.name])
            if diff:
                bad.append((c.name, place, diff, _describe(device[c.name, place]), _describe(wanted[c.name])))
        if RC.canonical(device[c.name, "lds"]) != RC.canonical(device[c.name, "hbm"]):
            bad.append((c.name, "lds != hbm", RC.differing_fields(device[c.name, "lds"], device[c.name, "hbm"])))
    assert not bad, bad


def test_path_edge_matches_oracle(device, wanted):
    """2716 points at 200 iterations without PROSAC is the last size in the LDS tile; 2717 and 2718 take HBM scratch."""
    assert sorted(k for k in device if k[0].startswith("path_")) == [("path_2716", "lds"), ("path_2717", "hbm"), ("path_2718", "hbm")]
    bad = [(k, RC.differing_fields(r, wanted[k[0]])) for k, r in device.items()
           if k[0].startswith("path_") and RC.differing_fields(r, wanted[k[0]])]
    assert not bad, bad


def test_second_problem_of_an_odd_stride_hbm_call(device, wanted):
    """Rows of the HBM scratch are max-problem-size elements apart: after a 2717-point problem the second problem's rows start at
    odd element offsets."""
    assert RC.path_cases()[1].P.shape[1] % 2 == 1
    diff = RC.differing_fields(device["odd_stride_second", "hbm"], wanted["odd_stride_second"])
    assert not diff, (diff, _describe(device["odd_stride_second", "hbm"]), _describe(wanted["odd_stride_second"]))


def test_estimate_with_positions_at_1e6(capi, oracle):
    """The whole estimator on two node pairs whose keypoint positions carry an offset of 1e6: in the first the float refit loses the
    consensus the hypotheses found (ok = 1, consensus 0, mse = 0 / 0 = NaN, finite T, identity information)."""
    pairs = RC.estimate_offset_pairs()
    m = capi.Match(**RC.ESTIMATE_CFG)
    ids = [(m.add_frame(f["desc"], f["pos"], f["valid"]), m.add_frame(t["desc"], t["pos"], t["valid"])) for f, t in pairs]
    res, diag = m.estimate(ids, job_ids=list(RC.ESTIMATE_JOBS), max_corr=200)
    m.close()
    for j, (f, t) in enumerate(pairs):
        w = RC.estimate_on_oracle(oracle, f, t, RC.ESTIMATE_JOBS[j])
        k = w["n_corr"]
        got = dict(T=res[j]["T"], consensus=int(res[j]["consensus"]), iterations_run=int(res[j]["iterations_run"]),
                   mask=diag["mask"][j, :k], mse=float(res[j]["mse"]))
        assert res[j]["ok"] == w["ok"] and res[j]["n_corr"] == k and res[j]["best_iteration"] == w["best_iteration"]
        assert not RC.differing_fields(got, w), (j, RC.differing_fields(got, w), _describe(got), _describe(w))
        assert np.array_equal(np.asarray(res[j]["information"]).reshape(6, 6), w["information"])
    assert res[0]["consensus"] == 0 and np.isnan(res[0]["mse"]) and res[0]["ok"] == 1


def test_vector_alu_votes_give_the_same_digests(device):
    # the switch only exists in the diagnostic build of the library (csrc/Makefile target `diag`, -DUZL_DIAG)
    diag = os.path.join(os.path.dirname(HERE), "uzliti_slam_amd", "libuzl_mi355x_diag.so")
    assert os.path.exists(diag), "build the diagnostic library: make -C uzliti_slam_amd/csrc diag"
    e = dict(os.environ, UZL_LIB=diag, UZL_VOTE_VALU="1")
    out = subprocess.run([sys.executable, os.path.join(HERE, "_ransac_cases_worker.py")], env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    valu = json.loads(out.stdout.strip().splitlines()[-1])
    mfma = {"%s/%s" % k: RC.digest(r) for k, r in device.items()}
    assert sorted(valu) == sorted(mfma)
    bad = [k for k in mfma if mfma[k] != valu[k]]
    assert not bad, "matrix-core votes differ from the vector-ALU votes: %s" % bad
