"""The one-graph PCG kernels of the small-graph class read what their first loads need from PRELOADED kernel arguments
(csrc/pgo_ml_kernels.hip: ml_spmv_pcg_kernel's leading pointer and integer parameters; csrc/Makefile: -amdgpu-kernarg-preload-count) and
the rest from the kernel-argument segment, beside the first round trip.  Nothing of the arithmetic changed, so on every shape at which
such a prologue can go wrong the device-resident loop (lm_loop = 0: captured PCG segments, PcgArgs of an LmSlot) and the host-driven
loop (lm_loop = 1: the same kernels, PcgArgs of a HostSlot, no LM state behind them) must agree to the bit - poses, chi2, lambda, every
counter - and both sit within tests/test_pgo_gpu.py's tolerances of the CPU oracle.

Shapes (node 0 of a synthetic graph is fixed: n nodes = n - 1 free vertices; a workgroup of ml_spmv holds 8 rows = one level-1
aggregate, one r.z partial per aggregate, 64 partials per group):
    7 free vertices    one partial aggregate, alone (no hierarchy: block-Jacobi, the host-driven loop either way)
    9                  one row into a second workgroup (one coarse level: the walked hierarchy's kernels)
    64, 65             eight whole workgroups, and one row past them: 65 is the smallest graph with the dense level-1 operator, i.e.
                       the smallest that runs the PcgArgs kernels at all
    512, 513           a full group of 64 r.z partials, and one past it
    a hub              one vertex with 25 neighbours: the slot walk beyond the row header's 20 columns (PcgArgs::col)
    a moving chi2      three and more LM iterations that change chi2: both hierarchy copies take their turn (PcgArgs::ix, Winv0 / Cmat32 / rg)
    a long first solve pass_history = 1 at a tight pcg_tol: the first solve outlasts its pass, continuation passes start where the solve
                       stands - at odd iteration counts too (parity)"""
import numpy as np
import pytest

from uzliti_slam_amd import synth
from test_lm_loops_gpu import KEYS, _solve
from test_pgo_gpu import _check

pytestmark = pytest.mark.gpu


def _both_loops_and_oracle(capi, oracle, g, its, device_loop=True, **cfg):
    a = _solve(capi, g, its, 0, **cfg)
    b = _solve(capi, g, its, 1, **cfg)
    assert a[0]["status"] == 0 and b[0]["status"] == 0, (a[0], b[0])
    assert (a[0]["lm_passes"] > 0) == device_loop and b[0]["lm_passes"] == 0, (a[0], b[0])
    for k in KEYS:
        assert a[0][k] == b[0][k], (k, a[0], b[0])
    assert np.array_equal(a[1], b[1])
    assert np.array_equal(a[2], b[2], equal_nan=True)
    if a[3] is not None:                                  # the second optimize on the same handle (it goes on from the result)
        for k in KEYS:
            assert a[3][k] == b[3][k], (k, a[3], b[3])
    assert np.array_equal(a[4], b[4])
    p = capi.Pgo(**cfg)
    try:
        _check(p, oracle, g, iterations=its)
    finally:
        p.close()
    return a[0]


@pytest.mark.parametrize("free,loops", [(7, 5), (9, 7), (64, 70), (65, 70), (512, 900), (513, 900)])
def test_row_and_partial_boundaries(capi, oracle, free, loops):
    n = free + 1
    g = synth.make_pose_graph(n, (n - 1) + loops, seed=100 + free)
    assert int(np.asarray(g["nodes_fixed"]).sum()) == 1
    # (up to 8 free vertices there is no hierarchy - block-Jacobi - and lm_loop = 0 solves on the host-driven loop as well)
    st = _both_loops_and_oracle(capi, oracle, g, 6, device_loop=free > 8)
    assert st["n_vertices"] == n and st["n_eliminated"] == 0, st


def _hub_graph():
    """make_pose_graph(120, 300) plus 24 loop closures from node 60 to nodes 61 .. 84, taken from the ground truth"""
    g = synth.make_pose_graph(120, 300, seed=4)
    e = g["edges"]
    gt = g["gt_pose"].reshape(-1, 3, 4)
    k = 24
    to = np.arange(61, 61 + k)
    T = synth.se3_mul(synth.se3_inv(gt[[60] * k]), gt[to]).reshape(-1, 12)
    ident = np.tile(np.eye(3, 4).reshape(1, 12), (k, 1))
    extra = {"from": np.full(k, 60, np.int32), "to": to.astype(np.int32), "type": np.ones(k, np.int32),
             "sensor_from": np.full(k, -1, np.int32), "sensor_to": np.full(k, -1, np.int32), "valid": np.ones(k, np.int32),
             "transform": T, "displacement_from": ident, "displacement_to": ident,
             "information": np.tile((np.eye(6) * 50.0).reshape(1, 36), (k, 1)), "diff_time": np.zeros(k)}
    e2 = {f: np.concatenate([np.asarray(e[f]), np.asarray(extra[f]).astype(np.asarray(e[f]).dtype)]) for f in extra}
    out = dict(g)
    out["edges"] = e2
    fr, t2 = np.asarray(e2["from"]), np.asarray(e2["to"])
    nbrs = set(t2[fr == 60].tolist()) | set(fr[t2 == 60].tolist())
    assert len(nbrs) >= 21, len(nbrs)
    return out


def test_row_beyond_twenty_slots(capi, oracle):
    _both_loops_and_oracle(capi, oracle, _hub_graph(), 6)


def test_both_hierarchy_copies(capi, oracle):
    g = synth.make_pose_graph(200, 700, seed=9)
    st = _both_loops_and_oracle(capi, oracle, g, 12)
    assert st["iterations_done"] >= 3 and st["chi2_final"] < st["chi2_initial"], st
    assert st["precond_builds"] >= 2, st                  # a rebuild goes into the copy the PCG is not applying


def test_first_solve_outlasts_its_pass(capi, oracle):
    g = synth.make_pose_graph(600, 2600, seed=1500)
    st = _both_loops_and_oracle(capi, oracle, g, 5, pass_history=1, pcg_tol=1e-12)
    assert st["lm_passes"] > st["lm_trials"], st          # more passes than trials: some solve went on in a continuation pass
