"""CPU tests (no GPU needed): uzl_scanmerge_* and uzl_grid_renumber_scans through the lifecycle and error path every uzl_* handle
shares, in the manner of tests/test_merge_handles_cpu.py.  What needs a handle runs on the device when there is one and is skipped
over inside the test otherwise, so the tests pass with or without a GPU."""
import contextlib
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

EXPORTS = ["uzl_scanmerge_cfg_default", "uzl_scanmerge_create", "uzl_scanmerge_destroy", "uzl_scanmerge_last_error", "uzl_scanmerge_run",
           "uzl_scanmerge_read", "uzl_scanmerge_points", "uzl_scanmerge_to_grid", "uzl_scanmerge_to_laser"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports_present(capi):
    L = capi.lib()
    for name in EXPORTS + ["uzl_grid_renumber_scans"]:
        assert hasattr(L, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(uzl_scanmerge_[a-z0-9_]+)\b", out)) == set(EXPORTS)
    assert "uzl_grid_renumber_scans" in out
    assert capi.lib().uzl_abi_version() == 3


def test_the_header_documents_the_stage_entry_and_the_contract():
    src = open(os.path.join(ROOT, "include", "uzl_mi355x.h")).read()
    comment = src[:src.index("int  uzl_scanmerge_points(")].rsplit("/*", 1)[1]
    assert comment.lstrip().startswith("Stage entry:")
    assert "#define UZL_ABI_VERSION 3" in src
    for word in ("UZL_ERR_UNSUPPORTED", "tests/scanmerge_reference.py", "a full build is the caller's next step"):
        assert word in src, word


def test_null_handle(capi):
    L = capi.lib()
    n = C.c_int32()
    assert L.uzl_scanmerge_last_error(None) == b"null handle"
    assert L.uzl_scanmerge_destroy(None) is None
    assert L.uzl_scanmerge_cfg_default(None) is None
    assert L.uzl_scanmerge_create(None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scanmerge_run(None, 0, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scanmerge_read(None, 0, 0, None, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scanmerge_points(None, 0, 0, 0, None, None) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scanmerge_to_grid(None, None, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_scanmerge_to_laser(None, None, 0, C.byref(n)) == capi.UZL_ERR_BAD_ARG
    assert L.uzl_grid_renumber_scans(None, 0, None, None) == capi.UZL_ERR_BAD_ARG


def test_the_prefix_is_registered_apart_from_the_first_eight(capi):
    assert "uzl_scanmerge" in capi._MORE_HANDLES and "uzl_scanmerge" not in capi._HANDLES


def test_struct_sizes_and_offsets(capi):
    c = capi.ScanMergeCfg(device=7, _pad=7)
    capi.lib().uzl_scanmerge_cfg_default(C.byref(c))
    assert (c.device, c._pad) == (0, 0) and C.sizeof(capi.ScanMergeCfg) == 8
    S, P = capi.ScanMergeScan, capi.ScanMergePair
    assert C.sizeof(S) == 144
    assert [getattr(S, f).offset for f, _ in S._fields_] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 136]
    assert C.sizeof(P) == 208 and [getattr(P, f).offset for f, _ in P._fields_] == [0, 8, 16, 112]
    src = open(os.path.join(ROOT, "include", "uzl_mi355x.h")).read()
    body = src[src.index("typedef struct uzl_scanmerge_scan {"):src.index("} uzl_scanmerge_scan;")]
    order = [body.index(w) for w in ("ranges;", "intensities;", "n_beams;", "angle_min,", "_pad;", "displacement[12]", "stamp_ns;")]
    assert order == sorted(order)
    assert (capi.SCANMERGE_KEEP_RANGES, capi.SCANMERGE_KEEP_INTENSITIES, capi.SCANMERGE_DROP_RANGES, capi.SCANMERGE_DROP_INTENSITIES) == (0, 1, 2, 3)


def test_no_device_is_an_error_not_a_fallback(capi):
    if capi.device_count() > 0:
        capi.ScanMerge().close()
        with pytest.raises(capi.UzlError) as e:
            capi.ScanMerge(device=capi.device_count())
        assert e.value.status == capi.UZL_ERR_NO_DEVICE
        return
    with pytest.raises(capi.UzlError) as e:
        capi.ScanMerge()
    assert e.value.status == capi.UZL_ERR_NO_DEVICE
    with pytest.raises(capi.UzlError) as e:
        capi.ScanMerge(device=-1)
    assert e.value.status == capi.UZL_ERR_NO_DEVICE


def _refused(capi, h, a, b, Dk=None, Dd=None):
    eye = np.eye(3, 4)
    with pytest.raises(capi.UzlError) as e:
        h.run([(a, b, eye if Dk is None else Dk, eye if Dd is None else Dd)])
    return e.value.status


def test_lifecycle_and_every_refusal_on_a_handle(capi):
    """with a device: every refusal of uzl_scanmerge_run leaves the resident result as it was; read, points and the hand-overs
    refuse what the header says; renumber refuses indices outside the store; close twice"""
    if capi.device_count() <= 0:
        with pytest.raises(capi.UzlError):
            capi.ScanMerge()
        return
    import scanmerge_scenes as S
    L = capi.lib()
    UNSUPPORTED = -10
    a, b, Dk, Dd = S.scenes()["n64"]
    exp = S.expected("n64")
    f32p = C.POINTER(C.c_float)
    with capi.ScanMerge() as h:
        n = C.c_int32(-5)
        assert L.uzl_scanmerge_read(h._h, 0, 64, None, None, None) == capi.UZL_ERR_STATE
        assert L.uzl_scanmerge_points(h._h, 0, 0, 64, None, None) == capi.UZL_ERR_STATE
        with contextlib.closing(capi.Grid()) as g, contextlib.closing(capi.Laser()) as las:
            assert L.uzl_scanmerge_to_grid(h._h, g._h, None, C.byref(n)) == capi.UZL_ERR_STATE
            assert L.uzl_scanmerge_to_laser(h._h, las._h, 0, C.byref(n)) == capi.UZL_ERR_STATE
            assert L.uzl_scanmerge_run(h._h, -1, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_run(h._h, 1, None) == capi.UZL_ERR_BAD_ARG
            assert h.run([]) == 0                                   # n_pairs = 0 is valid ...
            assert L.uzl_scanmerge_read(h._h, 0, 64, None, None, None) == capi.UZL_ERR_BAD_ARG     # ... and holds no pair
            assert h.to_grid(g, []) == 0 and g.scan_count() == 0
            h.run([(a, b, Dk, Dd)])

            def still_there():
                r, it, ce = h.read(0)
                return np.array_equal(r, exp["ranges"]) and np.array_equal(it, exp["intensities"]) and np.array_equal(ce, exp["center"])

            assert still_there()
            # NULL arrays
            arr, keep, shape = h.pack_pairs([(a, b, Dk, Dd)])
            arr[0].drop = None
            assert L.uzl_scanmerge_run(h._h, 1, arr) == capi.UZL_ERR_BAD_ARG
            arr, keep, shape = h.pack_pairs([(a, b, Dk, Dd)])
            keep[0][0].intensities = None
            assert L.uzl_scanmerge_run(h._h, 1, arr) == capi.UZL_ERR_BAD_ARG
            arr, keep, shape = h.pack_pairs([(a, b, Dk, Dd)])
            keep[0][2].ranges = None
            assert L.uzl_scanmerge_run(h._h, 1, arr) == capi.UZL_ERR_BAD_ARG
            # n_beams out of range (b may lie on any grid, so only its count is wrong)
            for nb in (7, 4097):
                short = dict(b, ranges=np.ones(nb, np.float32), intensities=np.ones(nb, np.float32))
                assert _refused(capi, h, a, short) == capi.UZL_ERR_BAD_ARG
            # a non-finite grid, limit or displacement entry; range_min < 0; range_max < range_min
            bad = [dict(angle_min=math.nan), dict(angle_min=math.inf), dict(angle_increment=math.nan), dict(angle_increment=-math.inf),
                   dict(range_min=math.nan), dict(range_max=math.inf), dict(range_max=math.nan), dict(range_min=-0.5),
                   dict(range_min=2.0, range_max=1.0)]
            for kw in bad:
                assert _refused(capi, h, a, dict(b, **kw)) == capi.UZL_ERR_BAD_ARG, kw
                assert _refused(capi, h, dict(a, **kw), b) == capi.UZL_ERR_BAD_ARG, kw
            for k in (0, 3, 11):
                D = np.eye(3, 4).reshape(12); D[k] = math.nan
                assert _refused(capi, h, a, dict(b, displacement=D)) == capi.UZL_ERR_BAD_ARG
                assert _refused(capi, h, dict(a, displacement=D), b) == capi.UZL_ERR_BAD_ARG
                assert _refused(capi, h, a, b, Dk=D) == capi.UZL_ERR_BAD_ARG
                D[k] = math.inf
                assert _refused(capi, h, a, b, Dd=D) == capi.UZL_ERR_BAD_ARG
            # the scope: keep off the laser-line grid
            assert _refused(capi, h, dict(a, angle_min=-3.0), b) == UNSUPPORTED
            assert "laser-line grid" in L.uzl_scanmerge_last_error(h._h).decode()
            assert _refused(capi, h, dict(a, angle_increment=float(a["angle_increment"]) * 1.5), b) == UNSUPPORTED
            assert _refused(capi, h, dict(a, angle_increment=0.0), b) == UNSUPPORTED
            assert _refused(capi, h, dict(a, angle_increment=-float(a["angle_increment"])), b) == UNSUPPORTED
            assert _refused(capi, h, S.scenes()["seam_pos_zero"][1], b) == UNSUPPORTED
            # a good pair in front of a bad one: nothing of the call is kept
            eye = np.eye(3, 4)
            with pytest.raises(capi.UzlError):
                h.run([(a, b, Dk, Dd), (dict(a, angle_min=-3.0), b, eye, eye)])
            assert still_there() and len(h._pairs) == 1
            # read / points
            buf = np.zeros(64, np.float32)
            assert L.uzl_scanmerge_read(h._h, 1, 64, None, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_read(h._h, -1, 64, None, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_read(h._h, 0, -1, None, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_read(h._h, 0, 63, buf.ctypes.data_as(f32p), None, None) == capi.UZL_ERR_TRUNCATED
            assert L.uzl_scanmerge_read(h._h, 0, 64, None, None, None) == 64
            ib = np.zeros(64, np.int32)
            assert L.uzl_scanmerge_points(h._h, 0, 4, 64, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_points(h._h, 0, -1, 64, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_points(h._h, 1, 0, 64, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_points(h._h, 0, 2, 63, ib.ctypes.data_as(capi.c_i32p), None) == capi.UZL_ERR_TRUNCATED
            assert L.uzl_scanmerge_points(h._h, 0, 2, 64, ib.ctypes.data_as(capi.c_i32p), None) == 64
            assert np.array_equal(ib, exp["bin"][2]) and still_there()
            # the hand-overs
            node = np.array([-1], np.int32)
            assert L.uzl_scanmerge_to_grid(h._h, None, node.ctypes.data_as(capi.c_i32p), C.byref(n)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_to_grid(h._h, g._h, None, C.byref(n)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_scanmerge_to_grid(h._h, g._h, node.ctypes.data_as(capi.c_i32p), C.byref(n)) == capi.UZL_ERR_BAD_ARG
            assert b"grid handle refused" in L.uzl_scanmerge_last_error(h._h) and g.scan_count() == 0
            assert L.uzl_scanmerge_to_laser(h._h, None, 0, C.byref(n)) == capi.UZL_ERR_BAD_ARG
            assert h.to_grid(g, [3]) == 0 and g.scan_count() == 1 and h.to_laser(las) == 0 and las.scan_count() == 1
            # renumber
            one = np.array([1], np.int32); zero = np.array([0], np.int32); low = np.array([-2], np.int32)
            p = lambda v: v.ctypes.data_as(capi.c_i32p)
            assert L.uzl_grid_renumber_scans(g._h, -1, None, None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_grid_renumber_scans(g._h, 1, None, p(zero)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_grid_renumber_scans(g._h, 1, p(zero), None) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_grid_renumber_scans(g._h, 1, p(one), p(zero)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_grid_renumber_scans(g._h, 1, p(low), p(zero)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_grid_renumber_scans(g._h, 1, p(zero), p(low)) == capi.UZL_ERR_BAD_ARG
            assert L.uzl_grid_renumber_scans(g._h, 0, None, None) == capi.UZL_OK
            g.renumber_scans([0], [-1]); g.renumber_scans([0], [5])
            with pytest.raises(capi.UzlError) as e:                 # add_scans still refuses a negative node
                g.add_scans([dict(node=-1, ranges=np.ones(8, np.float32), angle_min=0.0, angle_increment=0.1, range_min=0.1)])
            assert e.value.status == capi.UZL_ERR_BAD_ARG and g.scan_count() == 1
        h.close()
    h.close()
