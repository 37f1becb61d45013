"""CPU tests (no GPU needed): uzl_cloud_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp:
HandleBase, UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_laser_handles_cpu.py.  Nothing
here needs a handle on a device, so the tests pass with or without one."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

SYMBOLS = ["uzl_cloud_cfg_default", "uzl_cloud_create", "uzl_cloud_destroy", "uzl_cloud_last_error", "uzl_cloud_set_config",
           "uzl_cloud_add_images", "uzl_cloud_add_points", "uzl_cloud_count", "uzl_cloud_read", "uzl_cloud_estimate",
           "uzl_cloud_correspondences", "uzl_depthfilter_to_cloud"]


def test_null_handle(capi):
    L = capi.lib()
    assert L.uzl_cloud_last_error(None) == b"null handle"
    assert L.uzl_cloud_destroy(None) is None
    cfg = capi.CloudCfg()
    assert L.uzl_cloud_set_config(None, C.byref(cfg)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_add_images(None, 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_add_points(None, 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_count(None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_read(None, 0, 0, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_estimate(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_correspondences(None, None, None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_depthfilter_to_cloud(None, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_create(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_cloud_cfg_default(None) is None


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_cloud" in capi._MORE_HANDLES and "uzl_cloud" not in capi._HANDLES


def test_defaults_and_sizes(capi):
    """cloud_transformation_estimator.cpp:66-70, :119-121, :145-149; PCL's GICP defaults (k_correspondences 20, gicp_epsilon 0.001,
    rotation_epsilon 2e-3, transformation_epsilon 5e-4)"""
    c = capi.CloudCfg()
    capi.lib().uzl_cloud_cfg_default(C.byref(c))
    assert (c.leaf_size, c.z_min, c.z_max, c.lab_weight) == tuple(float(np.float32(v)) for v in (0.05, 0.0, 5.0, 0.024))
    assert (c.k_neighbours, c.max_iterations, c.inner_iterations, c.device) == (20, 20, 10, 0)
    assert (c.gicp_epsilon, c.max_correspondence_dist, c.rotation_epsilon, c.transformation_epsilon, c.min_score, c.max_translation,
            c.max_rotation_deg) == (0.001, 0.2, 2e-3, 5e-4, 0.3, 1.0, 30.0)
    assert C.sizeof(capi.CloudCfg) == 88 and C.sizeof(capi.CloudPair) == 104 and C.sizeof(capi.ColorImage) == 24
    assert C.sizeof(capi.CloudEdge) == capi.CLOUD_EDGE_DTYPE.itemsize == 680
    assert (capi.CLOUD_OK, capi.CLOUD_NO_CORR, capi.CLOUD_LOW_SCORE, capi.CLOUD_TOO_FAR) == (0, 1, 2, 3)
    assert (capi.CLOUD_MAX_POINTS, capi.CLOUD_MAX_ITERATIONS) == (32768, 64)


def test_the_restatement_has_the_same_defaults(capi):
    import cloud_reference as LR
    c = capi.CloudCfg()
    capi.lib().uzl_cloud_cfg_default(C.byref(c))
    d = LR.DEFAULTS
    for k in ("leaf_size", "z_min", "z_max", "lab_weight"):
        assert np.float32(getattr(c, k)) == d[k] and d[k].dtype == np.float32
    assert c.k_neighbours == d["k"]
    for k in ("max_iterations", "inner_iterations", "gicp_epsilon", "max_correspondence_dist", "rotation_epsilon",
              "transformation_epsilon", "min_score", "max_translation", "max_rotation_deg"):
        assert getattr(c, k) == d[k], k
    assert LR.MAX_POINTS == capi.CLOUD_MAX_POINTS


POSITIVE = ["leaf_size", "gicp_epsilon", "max_correspondence_dist", "rotation_epsilon", "transformation_epsilon"]
NONNEG = ["lab_weight", "min_score", "max_translation", "max_rotation_deg"]
BAD = ([{k: math.nan} for k in POSITIVE + NONNEG] + [{k: -0.5} for k in POSITIVE + NONNEG] + [{k: 0.0} for k in POSITIVE] +
       [{k: math.inf} for k in POSITIVE + NONNEG] +
       [dict(gicp_epsilon=1.5), dict(gicp_epsilon=2.0 ** -54), dict(gicp_epsilon=5e-324), dict(z_min=2.0, z_max=1.0), dict(z_min=math.nan), dict(k_neighbours=2), dict(k_neighbours=21),
        dict(max_iterations=0), dict(max_iterations=65), dict(inner_iterations=0), dict(inner_iterations=101)])


@pytest.mark.parametrize("bad", BAD, ids=["-".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_argument_errors_come_before_the_device_check(capi, bad):
    """A bad config is UZL_ERR_BAD_ARG whether or not a GPU is visible: the create checks it before it looks for a device."""
    with pytest.raises(capi.UzlError) as e:
        capi.Cloud(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_the_edges_of_the_ranges_are_allowed(capi):
    """zero weights and limits, gicp_epsilon 1 and 2^-53 (the least for which 1.0 - gicp_epsilon < 1.0), k 3 and 20, 1 and 64 iterations: not BAD_ARG (without a GPU they fail at the device
    check)"""
    for ok in ({k: 0.0 for k in NONNEG}, dict(gicp_epsilon=1.0), dict(gicp_epsilon=2.0 ** -53), dict(gicp_epsilon=1.5 * 2.0 ** -54), dict(k_neighbours=3), dict(k_neighbours=20), dict(max_iterations=1),
               dict(max_iterations=64), dict(inner_iterations=1), dict(inner_iterations=100), dict(z_min=1.0, z_max=1.0)):
        try:
            capi.Cloud(**ok).close()
            status = capi.UZL_OK
        except capi.UzlError as e:
            status = e.status
        assert status != capi.UZL_ERR_BAD_ARG


def test_every_new_symbol_is_exported(capi):
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    assert not [s for s in SYMBOLS if s not in exported]
    assert sorted(s for s in exported if s.startswith("uzl_cloud_") or s == "uzl_depthfilter_to_cloud") == sorted(SYMBOLS)
    assert "uzl_wire_sensor_color" in exported


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        h = capi.Cloud()
        h.close()
        with pytest.raises(capi.UzlError) as e:
            capi.Cloud(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Cloud()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
