"""CPU tests (no GPU needed): uzl_laser_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp:
HandleBase, UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_laserline_handles_cpu.py.  Nothing
here needs a handle on a device, so the tests pass with or without one."""
import ctypes as C
import math
import subprocess

import pytest

SYMBOLS = ["uzl_laser_cfg_default", "uzl_laser_create", "uzl_laser_destroy", "uzl_laser_last_error", "uzl_laser_set_config",
           "uzl_laser_add_scans", "uzl_laser_scan_count", "uzl_laser_estimate", "uzl_laser_correspondences", "uzl_laserline_to_laser"]


def test_null_handle(capi):
    L = capi.lib()
    assert L.uzl_laser_last_error(None) == b"null handle"
    assert L.uzl_laser_destroy(None) is None
    cfg = capi.LaserCfg()
    assert L.uzl_laser_set_config(None, C.byref(cfg)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laser_add_scans(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laser_scan_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laser_estimate(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laser_correspondences(None, None, None, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laserline_to_laser(None, None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_laser_create(None, None) == capi.UZL_ERR_BAD_ARG


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_laser" in capi._MORE_HANDLES and "uzl_laser" not in capi._HANDLES


def test_defaults_and_sizes(capi):
    """laser_transformation_estimator.cpp:35-124, :364, :371, :383"""
    c = capi.LaserCfg()
    capi.lib().uzl_laser_cfg_default(C.byref(c))
    assert (c.max_iterations, c.epsilon_xy, c.epsilon_theta, c.max_correspondence_dist, c.outliers_max_perc, c.outliers_adaptive_order,
            c.outliers_adaptive_mult, c.max_angular_correction_deg, c.max_linear_correction, c.min_valid_fraction, c.fail_fraction,
            c.goal_trace, c.other_information, c.device) == (10, 0.01, 0.02, 0.3, 0.80, 0.7, 2.0, 45.0, 1.5, 0.25, 0.05, 10000.0, 100.0, 0)
    assert C.sizeof(capi.LaserCfg) == 104 and C.sizeof(capi.LaserScanIn) == 32 and C.sizeof(capi.LaserPair) == 104
    assert C.sizeof(capi.LaserEdge) == capi.LASER_EDGE_DTYPE.itemsize == 424
    assert (capi.LASER_OK, capi.LASER_FEW_CORR, capi.LASER_VIEWPOINT, capi.LASER_FEW_MATCHES, capi.LASER_TOO_FAR,
            capi.LASER_DEGENERATE) == (0, 1, 2, 3, 4, 5)


THRESHOLDS = ["epsilon_xy", "epsilon_theta", "max_correspondence_dist", "outliers_adaptive_mult", "max_angular_correction_deg",
              "max_linear_correction", "goal_trace", "other_information"]
FRACTIONS = ["outliers_max_perc", "outliers_adaptive_order", "min_valid_fraction", "fail_fraction"]
BAD = ([{k: math.nan} for k in THRESHOLDS + FRACTIONS] + [{k: -0.5} for k in THRESHOLDS + FRACTIONS] + [{k: 1.5} for k in FRACTIONS] +
       [dict(max_iterations=0), dict(max_iterations=-3)])


@pytest.mark.parametrize("bad", BAD, ids=[f"{k}={v}" for b in BAD for k, v in b.items()])
def test_argument_errors_come_before_the_device_check(capi, bad):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        capi.Laser(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_the_edges_of_the_ranges_are_allowed(capi):
    """fractions 0 and 1, thresholds 0, one iteration: not BAD_ARG (without a GPU they fail at the device check)"""
    for ok in ({k: 0.0 for k in THRESHOLDS + FRACTIONS}, {k: 1.0 for k in FRACTIONS}, dict(max_iterations=1)):
        try:
            capi.Laser(**ok).close()
            status = capi.UZL_OK
        except capi.UzlError as e:
            status = e.status
        assert status != capi.UZL_ERR_BAD_ARG


def test_every_new_symbol_is_exported(capi):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert not [s for s in SYMBOLS if s not in exported]
    assert sorted(s for s in exported if s.startswith("uzl_laser_") or s == "uzl_laserline_to_laser") == sorted(SYMBOLS)


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        h = capi.Laser()
        h.close()
        with pytest.raises(capi.UzlError) as e:
            capi.Laser(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Laser()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
