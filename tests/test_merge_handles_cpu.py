"""CPU tests (no GPU needed): uzl_merge_* through the lifecycle and error path every uzl_* handle shares (uzl_common.hpp: HandleBase,
UZL_GUARD_*, last_error_of, check_device; capi._Handle), in the manner of tests/test_scope_handles_cpu.py.  What needs a handle runs on
the device when there is one and is skipped over inside the test otherwise, so the tests pass with or without a GPU."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

EXPORTS = ["uzl_merge_cfg_default", "uzl_merge_create", "uzl_merge_destroy", "uzl_merge_last_error", "uzl_merge_max_nodes",
           "uzl_merge_set_graph", "uzl_merge_set_poses", "uzl_merge_poses_from_pgo", "uzl_merge_set_valid", "uzl_merge_search",
           "uzl_merge_partners", "uzl_merge_stats", "uzl_merge_plan"]


def test_exports_present(capi):
    L = capi.lib()
    for name in EXPORTS:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    found = set(re.findall(r"\b(uzl_merge_[a-z0-9_]+)\b", out))
    assert found == set(EXPORTS)                     # neither the solver's pose accessor nor the pure plan leaks out
    assert "uzl_debug_merge_plan" not in out
    diag = subprocess.run(["nm", "-D", "--defined-only", capi.DIAG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "uzl_debug_merge_plan" in diag


def test_null_handle(capi):
    L = capi.lib()
    n = C.c_int32(); r = C.c_int64(); c3 = (C.c_double * 3)(); out = capi.MergePlanOut()
    assert L.uzl_merge_last_error(None) == b"null handle"
    assert L.uzl_merge_destroy(None) is None
    assert L.uzl_merge_cfg_default(None) is None
    assert L.uzl_merge_create(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_set_graph(None, 0, None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_set_poses(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_poses_from_pgo(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_set_valid(None, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_search(None, 1, c3, C.c_double(1.0), C.byref(n), C.byref(n), C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_partners(None, c3, C.c_double(1.0), 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_stats(None, C.byref(r), C.byref(r)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_merge_plan(None, 1, 0, 1, 1, C.byref(out), 0, None) == capi.UZL_ERR_BAD_ARG


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_merge" in capi._MORE_HANDLES and "uzl_merge" not in capi._HANDLES


def test_defaults_and_the_mirrored_bound(capi):
    c = capi.MergeCfg()
    capi.lib().uzl_merge_cfg_default(C.byref(c))
    assert (c.max_distance, c.max_rotation_deg, c.scope_margin, c.max_hops, c.device) == (0.25, 15.0, 6.0, 10, 0)
    assert C.sizeof(capi.MergeCfg) == 32
    assert (capi.MergeCfg.max_distance.offset, capi.MergeCfg.max_rotation_deg.offset, capi.MergeCfg.scope_margin.offset,
            capi.MergeCfg.max_hops.offset, capi.MergeCfg.device.offset) == (0, 8, 16, 24, 28)
    assert C.sizeof(capi.MergePlanOut) == 8 + 3 * 96 + 16 and capi.MergePlanOut.n_touched.offset == 296
    capi.lib().uzl_merge_max_nodes.restype = C.c_int32
    assert capi.lib().uzl_merge_max_nodes() == capi.MERGE_MAX_NODES == 262144
    # the visited bitmaps of a workgroup's four waves fit the 160 KiB of a CU; a walk's stack is one frame per lane of a wave
    assert 4 * capi.MERGE_MAX_NODES // 8 <= 160 * 1024 and capi.MERGE_MAX_HOPS <= 64
    src = open(capi.LIB_PATH.replace("uzliti_slam_amd/libuzl_mi355x.so", "include/uzl_mi355x.h")).read()
    assert "#define UZL_MERGE_MAX_HOPS %d" % capi.MERGE_MAX_HOPS in src
    for k, name in enumerate(("UNTOUCHED", "KEEP_FROM", "KEEP_TO", "RETARGET_FROM", "RETARGET_TO", "DELETE")):
        assert getattr(capi, "MERGE_EDGE_" + name) == k and re.search(r"#define UZL_MERGE_EDGE_%s\s+%d\b" % (name, k), src)


BAD = [dict(max_distance=math.nan), dict(max_rotation_deg=math.nan), dict(scope_margin=math.nan), dict(max_hops=-1), dict(max_hops=65)]


@pytest.mark.parametrize("bad", BAD, ids=["%s=%s" % (k, v) for b in BAD for k, v in b.items()])
def test_argument_errors_come_before_the_device_check(capi, bad):
    with pytest.raises(capi.UzlError) as e:
        capi.Merge(**bad)
    assert e.value.status == capi.UZL_ERR_BAD_ARG


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        capi.Merge().close()
        capi.Merge(max_hops=0).close(); capi.Merge(max_hops=64).close()
        with pytest.raises(capi.UzlError) as e:
            capi.Merge(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.Merge()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
    with pytest.raises(capi.UzlError) as e:
        capi.Merge(device=-1)
    assert e.value.status == capi.UZL_ERR_NO_DEVICE


def test_lifecycle_and_argument_errors_on_a_handle(capi):
    """with a device: NULL arguments, a cap too small, nodes out of range, the plan's argument errors, close twice; the handle stays
    usable after every refusal"""
    if capi.device_count() <= 0:
        with pytest.raises(capi.UzlError):
            capi.Merge()
        return
    import merge_scenes as S
    L = capi.lib()
    sc = S.two_ticks()
    n = C.c_int32(-5); k = C.c_int32(-5); d = C.c_int32(-5)
    far = np.array(S.FAR); c3 = far.ctypes.data_as(capi.c_f64p)
    out = capi.MergePlanOut(); act = np.zeros(64, np.int8); actp = act.ctypes.data_as(C.c_void_p)
    with capi.Merge() as h:
        assert L.uzl_merge_search(h._h, 1, c3, C.c_double(0.0), C.byref(k), C.byref(d), C.byref(n)) == capi.UZL_OK
        assert (k.value, d.value, n.value) == (-1, -1, 1)                  # empty graph: nothing runs
        assert h.stats() == dict(starts_walked=0, nodes_visited=0)
        assert L.uzl_merge_set_graph(h._h, 2, None, 0, None) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_set_graph(h._h, 0, None, 1, None) == capi.UZL_ERR_BAD_ARG
        h.set_graph(sc["poses"], sc["edges"])
        with pytest.raises(capi.UzlError) as e:
            h.set_graph(sc["poses"], S.edges_of([(0, 11)]))
        assert e.value.status == capi.UZL_ERR_BAD_ARG and "outside" in str(e.value)
        assert h.search(1, far, 0.0) == (7, 2, 2)                          # ... and nothing changed
        assert L.uzl_merge_search(h._h, -1, c3, C.c_double(0.0), C.byref(k), C.byref(d), C.byref(n)) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_search(h._h, 1, None, C.c_double(0.0), C.byref(k), C.byref(d), C.byref(n)) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_search(h._h, 1, c3, C.c_double(0.0), None, C.byref(d), C.byref(n)) == capi.UZL_ERR_BAD_ARG
        buf = np.zeros(11, np.int32)
        assert L.uzl_merge_partners(h._h, c3, C.c_double(0.0), 10, buf.ctypes.data_as(capi.c_i32p)) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_partners(h._h, c3, C.c_double(0.0), 11, None) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_partners(h._h, None, C.c_double(0.0), 11, buf.ctypes.data_as(capi.c_i32p)) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_partners(h._h, c3, C.c_double(0.0), 11, buf.ctypes.data_as(capi.c_i32p)) == 11
        assert L.uzl_merge_set_poses(h._h, 10, sc["poses"].ctypes.data_as(capi.c_f64p)) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_set_poses(h._h, 11, None) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_poses_from_pgo(h._h, None) == capi.UZL_ERR_BAD_ARG
        one = np.array([len(sc["edges"])], np.int32); flag = np.array([1], np.uint8)
        assert L.uzl_merge_set_valid(h._h, 1, None, None) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_set_valid(h._h, 1, one.ctypes.data_as(capi.c_i32p), flag.ctypes.data_as(capi.c_u8p)) == capi.UZL_ERR_BAD_ARG
        assert b"no such edge" in L.uzl_merge_last_error(h._h)
        ne = len(sc["edges"])
        assert L.uzl_merge_plan(h._h, 7, 2, 1, 1, None, ne, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, 7, 1, 1, C.byref(out), ne, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 11, 2, 1, 1, C.byref(out), ne, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, -1, 1, 1, C.byref(out), ne, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, 2, 0, 0, C.byref(out), ne, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, 2, -1, 3, C.byref(out), ne, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, 2, 1, 1, C.byref(out), ne - 1, actp) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, 2, 1, 1, C.byref(out), ne, None) == capi.UZL_ERR_BAD_ARG
        assert L.uzl_merge_plan(h._h, 7, 2, 1, 1, C.byref(out), ne, actp) == ne and out.ratio == 0.5
        assert h.search(1, far, 0.0) == (7, 2, 2)                          # still usable
        h.close()
    h.close()
