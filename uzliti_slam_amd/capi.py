"""ctypes binding of libuzl_mi355x.so (include/uzl_mi355x.h) — the only way Python reaches the HIP path.

There is no fallback: if the shared library has not been built, or no HIP device is visible when a
handle is created, the calls raise.  Tests and bench.py drive the product exclusively through this C ABI.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("UZL_LIB", os.path.join(_HERE, "libuzl_mi355x.so"))   # UZL_LIB: diagnostic builds only
CSRC = os.path.join(_HERE, "csrc")

c_f64p = C.POINTER(C.c_double)
c_i32p = C.POINTER(C.c_int32)
c_u8p = C.POINTER(C.c_uint8)
c_u64p = C.POINTER(C.c_uint64)
c_i64p = C.POINTER(C.c_int64)

UZL_OK = 0
UZL_ERR_BAD_ARG = -1
UZL_ERR_NO_DEVICE = -2
UZL_ERR_HIP = -3
UZL_ERR_NOT_CONVERGED = -4
UZL_ERR_BUSY = -5
UZL_ERR_OOM = -6
UZL_ERR_NOT_FOUND = -7
UZL_ERR_STATE = -8
UZL_ERR_TRUNCATED = -9


class UzlError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__(f"uzl status {status}: {msg}")
        self.status = status


class MatchCfg(C.Structure):
    _fields_ = [("ransac_threshold", C.c_double), ("link_covariance", C.c_double),
                ("ransac_iteration", C.c_int32), ("ransac_break_percentage", C.c_double),
                ("use_epnp", C.c_int32), ("do_prosac", C.c_int32), ("device", C.c_int32),
                ("seed", C.c_uint64)]


class Frame(C.Structure):
    _fields_ = [("desc", c_u8p), ("n", C.c_int32), ("bytes_per_desc", C.c_int32),
                ("pos_xyz", c_f64p), ("valid3d", c_u8p), ("feature_type", C.c_int32),
                ("sensor_frame", C.c_int32), ("displacement", C.c_double * 12)]


class PairJob(C.Structure):
    _fields_ = [("job_id", C.c_uint64), ("from_begin", C.c_int32), ("from_count", C.c_int32),
                ("to_begin", C.c_int32), ("to_count", C.c_int32)]


class EdgeResult(C.Structure):
    _fields_ = [("job_id", C.c_uint64), ("ok", C.c_int32), ("consensus", C.c_int32),
                ("n_matches", C.c_int32), ("n_corr", C.c_int32), ("frame_from", C.c_int32),
                ("frame_to", C.c_int32), ("iterations_run", C.c_int32), ("best_iteration", C.c_int32),
                ("mse", C.c_double), ("T", C.c_double * 12), ("information", C.c_double * 36)]


EDGE_RESULT_DTYPE = np.dtype([("job_id", "<u8"), ("ok", "<i4"), ("consensus", "<i4"), ("n_matches", "<i4"),
                              ("n_corr", "<i4"), ("frame_from", "<i4"), ("frame_to", "<i4"),
                              ("iterations_run", "<i4"), ("best_iteration", "<i4"), ("mse", "<f8"),
                              ("T", "<f8", (12,)), ("information", "<f8", (36,))], align=True)
FRAME_DTYPE = np.dtype([("desc", "<u8"), ("n", "<i4"), ("bytes_per_desc", "<i4"), ("pos_xyz", "<u8"), ("valid3d", "<u8"),
                        ("feature_type", "<i4"), ("sensor_frame", "<i4"), ("displacement", "<f8", (12,))], align=True)      # = Frame / uzl_frame
PAIR_JOB_DTYPE = np.dtype([("job_id", "<u8"), ("from_begin", "<i4"), ("from_count", "<i4"),
                           ("to_begin", "<i4"), ("to_count", "<i4")], align=True)


class PgoCfg(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("use_odometry_parameters", C.c_int32),
                ("optimize_xy_only", C.c_int32), ("device", C.c_int32), ("pcg_tol", C.c_double),
                ("pcg_max_iter", C.c_int32), ("schur_reduce", C.c_int32), ("huber_delta", C.c_double), ("verbose", C.c_int32),
                ("preconditioner", C.c_int32), ("pcg_stop", C.c_int32), ("lm_loop", C.c_int32), ("reduced_numbering", C.c_int32), ("pass_history", C.c_int32)]


class PgoStats(C.Structure):
    _fields_ = [("iterations_done", C.c_int32), ("lm_trials", C.c_int32), ("pcg_iterations", C.c_int32),
                ("terminated_early", C.c_int32), ("n_vertices", C.c_int32), ("n_edges", C.c_int32),
                ("n_gauge_fixed", C.c_int32), ("pcg_not_converged", C.c_int32),
                ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("lambda_final", C.c_double),
                ("solve_ms", C.c_double), ("precond_builds", C.c_int32), ("exchange_calls", C.c_int32),
                ("structure_ms", C.c_double), ("exchange_ms", C.c_double), ("structure_reused", C.c_int32), ("n_eliminated", C.c_int32),
                ("lm_passes", C.c_int32), ("reduced_strong", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


NODE_DTYPE = np.dtype([("pose", "<f8", (12,)), ("fixed", "<i4")], align=True)
EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("type", "<i4"), ("sensor_from", "<i4"),
                       ("sensor_to", "<i4"), ("valid", "<i4"), ("transform", "<f8", (12,)),
                       ("displacement_from", "<f8", (12,)), ("displacement_to", "<f8", (12,)),
                       ("information", "<f8", (36,)), ("diff_time", "<f8")], align=True)
PGO_EDGE_OP_DTYPE = np.dtype([("edge", "<i4"), ("action", "<i4"), ("xf", "<i4"), ("node", "<i4")])      # uzl_pgo_edge_op


class PgoRewrite(C.Structure):
    """uzl_pgo_rewrite"""
    _fields_ = [("n_drop", C.c_int32), ("drop_nodes", c_i32p), ("n_pose", C.c_int32), ("pose_nodes", c_i32p), ("poses", c_f64p),
                ("n_xf", C.c_int32), ("xf", c_f64p), ("n_ops", C.c_int32), ("ops", C.c_void_p)]

class FilterCfg(C.Structure):
    _fields_ = [("max_dt", C.c_double), ("min_size", C.c_double), ("max_cluster_size", C.c_int32),
                ("ransac_iterations", C.c_int32), ("max_error", C.c_double), ("min_time_span", C.c_double),
                ("max_edges", C.c_int32), ("device", C.c_int32), ("seed", C.c_uint64)]


class FilterEdge(C.Structure):
    _fields_ = [("key", C.c_uint64), ("matching_score", C.c_double), ("valid", C.c_int32),
                ("sensor_from", C.c_int32), ("sensor_to", C.c_int32), ("n_stamps_from", C.c_int32),
                ("n_stamps_to", C.c_int32), ("_pad", C.c_int32),
                ("stamps_from_ns", C.POINTER(C.c_int64)), ("stamps_to_ns", C.POINTER(C.c_int64)),
                ("transform", C.c_double * 12), ("displacement_from", C.c_double * 12),
                ("displacement_to", C.c_double * 12), ("pose_from", C.c_double * 12), ("pose_to", C.c_double * 12)]


# numpy mirror of uzl_filter_edge (pointers as addresses): batches of thousands of edges are packed without a Python loop
FILTER_EDGE_DTYPE = np.dtype([("key", "<u8"), ("matching_score", "<f8"), ("valid", "<i4"), ("sensor_from", "<i4"), ("sensor_to", "<i4"),
                              ("n_stamps_from", "<i4"), ("n_stamps_to", "<i4"), ("_pad", "<i4"), ("stamps_from_ns", "<u8"),
                              ("stamps_to_ns", "<u8"), ("transform", "<f8", (12,)), ("displacement_from", "<f8", (12,)),
                              ("displacement_to", "<f8", (12,)), ("pose_from", "<f8", (12,)), ("pose_to", "<f8", (12,))], align=True)
assert FILTER_EDGE_DTYPE.itemsize == C.sizeof(FilterEdge)


class ClusterInfo(C.Structure):
    _fields_ = [("uid", C.c_uint64), ("from_start_ns", C.c_int64), ("from_end_ns", C.c_int64),
                ("to_start_ns", C.c_int64), ("to_end_ns", C.c_int64), ("size", C.c_int32),
                ("consensus", C.c_int32), ("changed", C.c_int32), ("evaluations", C.c_int32)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_IDENT12 = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)


def pack_filter_edges(edges, struct=None):
    """list of dicts (key, matching_score, valid, sensor_from, sensor_to, stamps_from, stamps_to, transform,
    displacement_from, displacement_to, pose_from, pose_to) -> (ctypes array, keep-alive list).  3x4 row-major
    transforms (12 doubles); stamps are int64 nanoseconds."""
    struct = struct or FilterEdge
    arr = (struct * max(len(edges), 1))()
    keep = []
    for i, e in enumerate(edges):
        a = arr[i]
        a.key = int(e["key"]); a.matching_score = float(e.get("matching_score", 0.0)); a.valid = int(e.get("valid", 0))
        a.sensor_from = int(e.get("sensor_from", -1)); a.sensor_to = int(e.get("sensor_to", -1))
        sf = np.ascontiguousarray(e.get("stamps_from", ()), np.int64); st = np.ascontiguousarray(e.get("stamps_to", ()), np.int64)
        keep += [sf, st]
        a.n_stamps_from = len(sf); a.n_stamps_to = len(st)
        a.stamps_from_ns = sf.ctypes.data_as(C.POINTER(C.c_int64)); a.stamps_to_ns = st.ctypes.data_as(C.POINTER(C.c_int64))
        for f in ("transform", "displacement_from", "displacement_to", "pose_from", "pose_to"):
            v = e.get(f)
            getattr(a, f)[:] = _IDENT12 if v is None else tuple(np.asarray(v, np.float64).reshape(-1)[:12])
    return arr, keep


class GateCfg(C.Structure):
    _fields_ = [("min_matching_score", C.c_double), ("max_edge_distance_T", C.c_double), ("max_edge_distance_R", C.c_double),
                ("scope_size_factor", C.c_double), ("min_accept_valid", C.c_double), ("device", C.c_int32), ("_pad", C.c_int32)]


GATE_EDGE_DTYPE = np.dtype([("from", "<i4"), ("to", "<i4"), ("type", "<i4"), ("valid", "<i4"), ("matching_score", "<f8"),
                            ("transform", "<f8", (12,))], align=True)


def gate_edges(frm, to, typ, valid=None, score=None, transform=None):
    n = len(frm)
    a = np.zeros(max(n, 1), GATE_EDGE_DTYPE)
    a["from"][:n] = frm; a["to"][:n] = to; a["type"][:n] = typ
    if valid is not None:
        a["valid"][:n] = valid
    if score is not None:
        a["matching_score"][:n] = score
    a["transform"][:n] = np.eye(3, 4).reshape(12) if transform is None else np.asarray(transform, np.float64).reshape(n, 12)
    return a[:n] if n else a[:0]


class RadiusCfg(C.Structure):
    _fields_ = [("radius", C.c_double), ("new_edge_time", C.c_double), ("max_rotation_deg", C.c_double),
                ("device", C.c_int32), ("_pad", C.c_int32)]


class PlacesCfg(C.Structure):
    _fields_ = [("key_width", C.c_int32), ("min_rows_to_add", C.c_int32), ("T", C.c_double), ("k_nearest_neighbors", C.c_int32),
                ("device", C.c_int32), ("min_time_gap", C.c_double)]


class GistCfg(C.Structure):
    _fields_ = [("T", C.c_double), ("k_nearest_neighbors", C.c_int32), ("device", C.c_int32), ("min_time_gap", C.c_double)]


class GfrCfg(C.Structure):
    _fields_ = [("T", C.c_double), ("k_nearest_neighbors", C.c_int32), ("max_distance", C.c_int32), ("device", C.c_int32),
                ("min_time_gap", C.c_double), ("initial_features", C.c_int32)]


class ScopeCfg(C.Structure):
    _fields_ = [("scope_size_min", C.c_double), ("scope_size_factor", C.c_double), ("out_margin", C.c_double),
                ("device", C.c_int32), ("_pad", C.c_int32)]


SCOPE_LDS_NODES = 16384         # scope_types.hpp kScopeLdsNodes = uzl_scope_lds_nodes(): the on-chip bound of a pass


class MergeCfg(C.Structure):
    _fields_ = [("max_distance", C.c_double), ("max_rotation_deg", C.c_double), ("scope_margin", C.c_double),
                ("max_hops", C.c_int32), ("device", C.c_int32)]


class MergePlanOut(C.Structure):
    _fields_ = [("ratio", C.c_double), ("new_pose", C.c_double * 12), ("keep_displacement", C.c_double * 12),
                ("drop_displacement", C.c_double * 12), ("n_touched", C.c_int32), ("n_retargeted", C.c_int32),
                ("n_deleted", C.c_int32), ("_pad", C.c_int32)]


MERGE_MAX_NODES = 262144        # merge_types.hpp kMergeMaxNodes = uzl_merge_max_nodes(): a visited bitmap of 32 KiB per wave
MERGE_MAX_HOPS = 64             # UZL_MERGE_MAX_HOPS
(MERGE_EDGE_UNTOUCHED, MERGE_EDGE_KEEP_FROM, MERGE_EDGE_KEEP_TO, MERGE_EDGE_RETARGET_FROM, MERGE_EDGE_RETARGET_TO,
 MERGE_EDGE_DELETE) = range(6)


class ScanMergeCfg(C.Structure):
    _fields_ = [("device", C.c_int32), ("_pad", C.c_int32)]


class ScanMergeScan(C.Structure):
    _fields_ = [("ranges", C.POINTER(C.c_float)), ("intensities", C.POINTER(C.c_float)), ("n_beams", C.c_int32),
                ("angle_min", C.c_float), ("angle_increment", C.c_float), ("range_min", C.c_float), ("range_max", C.c_float),
                ("_pad", C.c_int32), ("displacement", C.c_double * 12), ("stamp_ns", C.c_int64)]


class ScanMergePair(C.Structure):
    _fields_ = [("keep", C.POINTER(ScanMergeScan)), ("drop", C.POINTER(ScanMergeScan)), ("keep_displacement", C.c_double * 12),
                ("drop_displacement", C.c_double * 12)]


SCANMERGE_KEEP_RANGES, SCANMERGE_KEEP_INTENSITIES, SCANMERGE_DROP_RANGES, SCANMERGE_DROP_INTENSITIES = range(4)


class GridCfg(C.Structure):
    _fields_ = [("resolution", C.c_double), ("range_max", C.c_double), ("occupancy_threshold", C.c_double), ("max_distance", C.c_double),
                ("known_free_radius", C.c_double), ("min_pass_through", C.c_int32), ("device", C.c_int32), ("max_cells", C.c_int64)]


class GridScan(C.Structure):
    _fields_ = [("node", C.c_int32), ("n_ranges", C.c_int32), ("displacement", C.c_double * 12), ("angle_min", C.c_float),
                ("angle_increment", C.c_float), ("range_min", C.c_float), ("ranges", C.POINTER(C.c_float))]


class GridInfo(C.Structure):
    _fields_ = [("origin_x", C.c_double), ("origin_y", C.c_double), ("resolution", C.c_double), ("width", C.c_uint32),
                ("height", C.c_uint32), ("valid_beams", C.c_int64), ("hits", C.c_int64), ("scans", C.c_int32), ("off_grid", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LaserlineCfg(C.Structure):
    _fields_ = [("min_height", C.c_double), ("max_height", C.c_double), ("angle_increment", C.c_double), ("range_min", C.c_double),
                ("range_max", C.c_double), ("depth_scale", C.c_double), ("device", C.c_int32), ("_pad", C.c_int32)]


DEPTH_F32_M, DEPTH_U16_MM = 0, 1


class DepthImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("encoding", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("camera_transform", C.c_double * 12), ("group", C.c_int32), ("_pad", C.c_int32)]


class DepthFilterCfg(C.Structure):
    _fields_ = [("radius", C.c_int32), ("nearest_radius", C.c_int32), ("sigma_space", C.c_double), ("sigma_color", C.c_double),
                ("depth_scale", C.c_double), ("use_bilateral_filter", C.c_int32), ("device", C.c_int32)]


class GuideImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int32), ("_pad", C.c_int32)]


class OrbCfg(C.Structure):
    _fields_ = [("number_of_features", C.c_int32), ("grid_rows", C.c_int32), ("grid_cols", C.c_int32), ("n_levels", C.c_int32),
                ("scale_factor", C.c_float), ("edge_threshold", C.c_int32), ("patch_size", C.c_int32), ("fast_threshold", C.c_int32),
                ("gist_size", C.c_int32), ("device", C.c_int32)]


ORB_STAGE_LEVEL, ORB_STAGE_MASK, ORB_STAGE_BLUR, ORB_STAGE_GIST, ORB_STAGE_GIST_BLUR = range(5)


class LaserCfg(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("device", C.c_int32), ("epsilon_xy", C.c_double), ("epsilon_theta", C.c_double),
                ("max_correspondence_dist", C.c_double), ("outliers_max_perc", C.c_double), ("outliers_adaptive_order", C.c_double),
                ("outliers_adaptive_mult", C.c_double), ("max_angular_correction_deg", C.c_double), ("max_linear_correction", C.c_double),
                ("min_valid_fraction", C.c_double), ("fail_fraction", C.c_double), ("goal_trace", C.c_double),
                ("other_information", C.c_double)]


class LaserScanIn(C.Structure):
    _fields_ = [("values", C.POINTER(C.c_float)), ("n_beams", C.c_int32), ("angle_min", C.c_float), ("angle_increment", C.c_float),
                ("range_min", C.c_float), ("range_max", C.c_float), ("_pad", C.c_int32)]


class LaserPair(C.Structure):
    _fields_ = [("scan_from", C.c_int32), ("scan_to", C.c_int32), ("first_guess", C.c_double * 12)]


class LaserEdge(C.Structure):
    _fields_ = [("status", C.c_int32), ("nvalid", C.c_int32), ("scan_valid", C.c_int32), ("deg_count", C.c_int32),
                ("iterations", C.c_int32), ("_pad", C.c_int32), ("matching_score", C.c_double), ("error", C.c_double),
                ("transform", C.c_double * 12), ("information", C.c_double * 36)]


LASER_OK, LASER_FEW_CORR, LASER_VIEWPOINT, LASER_FEW_MATCHES, LASER_TOO_FAR, LASER_DEGENERATE = range(6)
LASER_EDGE_DTYPE = np.dtype([("status", "<i4"), ("nvalid", "<i4"), ("scan_valid", "<i4"), ("deg_count", "<i4"), ("iterations", "<i4"),
                             ("_pad", "<i4"), ("matching_score", "<f8"), ("error", "<f8"), ("transform", "<f8", (12,)),
                             ("information", "<f8", (36,))])

class CloudCfg(C.Structure):
    _fields_ = [("leaf_size", C.c_float), ("z_min", C.c_float), ("z_max", C.c_float), ("lab_weight", C.c_float),
                ("k_neighbours", C.c_int32), ("max_iterations", C.c_int32), ("inner_iterations", C.c_int32), ("device", C.c_int32),
                ("gicp_epsilon", C.c_double), ("max_correspondence_dist", C.c_double), ("rotation_epsilon", C.c_double),
                ("transformation_epsilon", C.c_double), ("min_score", C.c_double), ("max_translation", C.c_double),
                ("max_rotation_deg", C.c_double)]


COLOR_BGR8, COLOR_RGB8 = 0, 1


class ColorImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int32), ("encoding", C.c_int32)]


class CloudPair(C.Structure):
    _fields_ = [("cloud_from", C.c_int32), ("cloud_to", C.c_int32), ("first_guess", C.c_double * 12)]


CLOUD_MAX_POINTS, CLOUD_MAX_ITERATIONS = 32768, 64


class CloudEdge(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("num_corr", C.c_int32), ("n_from", C.c_int32), ("n_to", C.c_int32),
                ("_pad", C.c_int32), ("num_corr_iter", C.c_int32 * CLOUD_MAX_ITERATIONS), ("match_score", C.c_double),
                ("matching_score", C.c_double), ("transform", C.c_double * 12), ("information", C.c_double * 36)]


CLOUD_OK, CLOUD_NO_CORR, CLOUD_LOW_SCORE, CLOUD_TOO_FAR = range(4)
CLOUD_EDGE_DTYPE = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("num_corr", "<i4"), ("n_from", "<i4"), ("n_to", "<i4"),
                             ("_pad", "<i4"), ("num_corr_iter", "<i4", (CLOUD_MAX_ITERATIONS,)), ("match_score", "<f8"),
                             ("matching_score", "<f8"), ("transform", "<f8", (12,)), ("information", "<f8", (36,))])

ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p)

_lib = None


def build(force=False):
    """hipcc --offload-arch=gfx950 build of the in-tree shared library (csrc/Makefile)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", CSRC, "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", CSRC])
    return LIB_PATH


def lib():
    """Load libuzl_mi355x.so; raises (never falls back) when it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise UzlError(UZL_ERR_STATE, f"{LIB_PATH} is missing: run __graft_entry__.build() / make -C {CSRC}; "
                                          "there is no CPU fallback")
        _lib = _declare(C.CDLL(LIB_PATH))
    return _lib


_HANDLES = ("uzl_match", "uzl_pgo", "uzl_pgo_batch", "uzl_filter", "uzl_gate", "uzl_radius", "uzl_places", "uzl_gist")
_MORE_HANDLES = ("uzl_grid", "uzl_laserline", "uzl_gfr", "uzl_laser", "uzl_depthfilter", "uzl_cloud", "uzl_orb", "uzl_scope", "uzl_merge", "uzl_scanmerge")    # declared like _HANDLES; kept apart because tests pin _HANDLES to the first eight


def _declare(L):
    """The prototypes ctypes cannot guess: every handle's last_error / destroy / cfg_default, and the calls that take only a handle."""
    L.uzl_status_string.restype = C.c_char_p
    for p in _HANDLES + _MORE_HANDLES:
        getattr(L, p + "_last_error").restype = C.c_char_p
        getattr(L, p + "_last_error").argtypes = [C.c_void_p]
        getattr(L, p + "_destroy").restype = None
        getattr(L, p + "_destroy").argtypes = [C.c_void_p]
        if hasattr(L, p + "_cfg_default"):          # (a batch takes uzl_pgo_cfg)
            getattr(L, p + "_cfg_default").restype = None
    for f in ("uzl_places_count", "uzl_gist_count", "uzl_grid_scan_count", "uzl_gate_edge_count", "uzl_filter_cluster_count",
              "uzl_gfr_count", "uzl_gfr_feature_count", "uzl_gfr_link_count", "uzl_laser_scan_count", "uzl_depthfilter_image_count",
              "uzl_cloud_count", "uzl_orb_image_count"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.uzl_pgo_batch_graph.restype = C.c_void_p
    L.uzl_pgo_batch_graph.argtypes = [C.c_void_p, C.c_int32]
    return L


def _p(a, t):
    return a.ctypes.data_as(t) if a is not None else None


def device_count():
    return lib().uzl_device_count()


DIAG_LIB_PATH = os.path.join(_HERE, "libuzl_mi355x_diag.so")
_diag = None


def diag_lib():
    """The diagnostic twin (same sources, -DUZL_DIAG): the only place the uzl_debug_* test hooks exist - the product library exports
    include/uzl_mi355x.h and nothing else.  Loaded beside the product library (both keep their symbols to themselves)."""
    global _diag
    if _diag is None:
        if not os.path.exists(DIAG_LIB_PATH):
            raise UzlError(UZL_ERR_STATE, f"{DIAG_LIB_PATH} is missing: make -C {CSRC} diag")
        _diag = _declare(C.CDLL(DIAG_LIB_PATH))
    return _diag


def stream_stats(device=0):
    """uzl_stream_stats: the device's stream pool (uzl_streams.hip)"""
    v = [C.c_int32() for _ in range(6)]
    ms = C.c_double()
    rc = lib().uzl_stream_stats(C.c_int32(device), *[C.byref(x) for x in v], C.byref(ms))
    if rc != UZL_OK:
        raise UzlError(rc, "uzl_stream_stats")
    return dict(zip(("pooled", "leased", "registered", "pairs_measured", "pairs_independent", "fallbacks"), [x.value for x in v]), probe_ms=ms.value)


RCCL_UNIQUE_ID_BYTES = 128


def rccl_unique_id():
    """ncclGetUniqueId through the library (rank 0); the bytes go to the other ranks by any channel."""
    buf = (C.c_char * RCCL_UNIQUE_ID_BYTES)()
    rc = lib().uzl_rccl_unique_id(buf, C.c_int32(RCCL_UNIQUE_ID_BYTES))
    if rc != UZL_OK:
        raise UzlError(rc, "uzl_rccl_unique_id")
    return bytes(buf.raw)


# --------------------------------------------------------------------------------------- handles
class _Handle:
    """One uzl_<name>_* handle: `cfg` is <prefix>_cfg_default's config with the keyword arguments set on it, `_h` the handle."""

    _prefix = None                  # "uzl_gist", ...
    _cfg_type = None                # its config struct
    _cfg_default = None             # the function that fills it, when not <prefix>_cfg_default
    _lib = staticmethod(lambda: lib())

    def __init__(self, *args, **cfg):
        """args: what <prefix>_create takes between the config and the handle (a batch's n_graphs)."""
        L = self._lib()
        c = self._cfg_type()
        getattr(L, self._cfg_default or self._prefix + "_cfg_default")(C.byref(c))
        for k, v in cfg.items():
            setattr(c, k, v)
        self.cfg = c
        self._h = C.c_void_p()
        rc = getattr(L, self._prefix + "_create")(C.byref(c), *args, C.byref(self._h))
        if rc != UZL_OK:
            raise UzlError(rc, L.uzl_status_string(rc).decode())

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib(), self._prefix + "_destroy")(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, allow=()):
        """Raises with the handle's last_error for a failure status (< 0) not in `allow`; returns rc (counts are >= 0)."""
        if rc < 0 and rc not in allow:
            raise UzlError(rc, getattr(self._lib(), self._prefix + "_last_error")(self._h).decode())
        return rc

    def _set_config(self, **cfg):
        """set_config of the handles with a <prefix>_set_config (match and pgo)"""
        for k, v in cfg.items():
            setattr(self.cfg, k, v)
        self._check(getattr(self._lib(), self._prefix + "_set_config")(self._h, C.byref(self.cfg)))


# --------------------------------------------------------------------------------------- estimator
class Match(_Handle):
    """Thin object wrapper over the uzl_match_* C ABI."""

    _prefix, _cfg_type = "uzl_match", MatchCfg
    set_config = _Handle._set_config

    def add_frame(self, desc, pos, valid, feature_type=2, sensor_frame=0):
        """desc (n,bytes) u8; pos (3,n) f64; valid (n) u8 -> frame id."""
        d = np.ascontiguousarray(desc, np.uint8)
        p = np.ascontiguousarray(np.asarray(pos, np.float64).T)   # (n,3) row-major == 3 x n column-major
        v = np.ascontiguousarray(valid, np.uint8)
        f = Frame()
        f.desc = _p(d, c_u8p); f.n = d.shape[0]; f.bytes_per_desc = d.shape[1] if d.ndim == 2 else 0
        f.pos_xyz = _p(p, c_f64p); f.valid3d = _p(v, c_u8p)
        f.feature_type = int(feature_type); f.sensor_frame = int(sensor_frame)
        f.displacement[:] = np.eye(3, 4).reshape(12).tolist()
        fid = C.c_int32(-1)
        self._check(lib().uzl_match_add_frame(self._h, C.byref(f), C.byref(fid)))
        return fid.value

    @staticmethod
    def pack_frames(frames, feature_type=2, sensor_frame=0):
        """[(desc, pos, valid), ...] -> (array of uzl_frame, keep-alive list): the marshalling a C++ caller does not have.  The structs are
        filled column by column through a numpy view of the same layout (field-by-field ctypes assignment was 18 us per frame)."""
        n = len(frames)
        arr = np.zeros(max(n, 1), FRAME_DTYPE)
        keep = []
        dp = np.empty(n, np.uint64); pp = np.empty(n, np.uint64); vp = np.empty(n, np.uint64); nn = np.empty(n, np.int32); bb = np.empty(n, np.int32)
        for k, (desc, pos, valid) in enumerate(frames):
            d = np.ascontiguousarray(desc, np.uint8)
            p = np.ascontiguousarray(np.asarray(pos, np.float64).T)
            v = np.ascontiguousarray(valid, np.uint8)
            keep.append((d, p, v))
            dp[k] = d.__array_interface__["data"][0]; pp[k] = p.__array_interface__["data"][0]; vp[k] = v.__array_interface__["data"][0]
            nn[k] = d.shape[0]; bb[k] = d.shape[1] if d.ndim == 2 else 0
        a = arr[:n]
        a["desc"] = dp; a["pos_xyz"] = pp; a["valid3d"] = vp; a["n"] = nn; a["bytes_per_desc"] = bb
        a["feature_type"] = int(feature_type); a["sensor_frame"] = int(sensor_frame); a["displacement"] = np.eye(3, 4).reshape(12)
        return a, keep

    def add_frames(self, packed):
        """uzl_match_add_frames over the array pack_frames built -> list of frame ids."""
        arr = packed[0] if isinstance(packed, tuple) else packed
        n = len(arr)
        ids = (C.c_int32 * max(n, 1))()
        self._check(lib().uzl_match_add_frames(self._h, C.c_int32(n), _p(arr, C.c_void_p) if isinstance(arr, np.ndarray) else arr, ids))
        return list(ids[:n])

    def arena_bytes(self):
        live = C.c_uint64(); hw = C.c_uint64(); cap = C.c_uint64()
        self._check(lib().uzl_match_arena_bytes(self._h, C.byref(live), C.byref(hw), C.byref(cap)))
        return dict(live=live.value, high_water=hw.value, capacity=cap.value)

    def remove_frame(self, fid):
        self._check(lib().uzl_match_remove_frame(self._h, C.c_int32(fid)))

    def compact(self):
        """uzl_match_compact: the live frames close up in a new allocation sized to them, ids unchanged -> bytes moved (0: no hole)"""
        moved = C.c_uint64()
        self._check(lib().uzl_match_compact(self._h, C.byref(moved)))
        return moved.value

    def frame_count(self):
        return lib().uzl_match_frame_count(self._h)

    @staticmethod
    def _jobs(pairs, job_ids):
        """pairs: list of (from_frame_ids, to_frame_ids) (ints or lists)."""
        n = len(pairs)
        jobs = np.zeros(n, PAIR_JOB_DTYPE)
        ids = []
        for j, (fr, to) in enumerate(pairs):
            fr = [fr] if np.isscalar(fr) else list(fr)
            to = [to] if np.isscalar(to) else list(to)
            jobs[j]["job_id"] = job_ids[j] if job_ids is not None else j
            jobs[j]["from_begin"] = len(ids); jobs[j]["from_count"] = len(fr); ids += fr
            jobs[j]["to_begin"] = len(ids); jobs[j]["to_count"] = len(to); ids += to
        return jobs, np.asarray(ids, np.int32)

    def estimate(self, pairs, job_ids=None, max_corr=0):
        """Batched estimateEdgeImpl. Returns (results structured array, diag dict or None)."""
        jobs, ids = self._jobs(pairs, job_ids)
        n = len(pairs)
        res = np.zeros(n, EDGE_RESULT_DTYPE)
        diag = None
        cq = ct = cd = mk = None
        if max_corr > 0:
            cq = np.empty((n, max_corr), np.int32); ct = np.empty((n, max_corr), np.int32)
            cd = np.empty((n, max_corr), np.int32); mk = np.empty((n, max_corr), np.uint8)
            diag = dict(corr_query=cq, corr_train=ct, corr_dist=cd, mask=mk)
        self._check(lib().uzl_match_estimate(self._h, C.c_int32(n), _p(jobs, C.c_void_p), _p(ids, c_i32p),
                                             C.c_int32(len(ids)), _p(res, C.c_void_p), C.c_int32(max_corr),
                                             _p(cq, c_i32p), _p(ct, c_i32p), _p(cd, c_i32p), _p(mk, c_u8p)))
        return res, diag

    def launch(self, pairs, job_ids=None):
        jobs, ids = self._jobs(pairs, job_ids)
        self._n_launched = len(pairs)
        self._check(lib().uzl_match_launch(self._h, C.c_int32(len(pairs)), _p(jobs, C.c_void_p), _p(ids, c_i32p),
                                           C.c_int32(len(ids)), C.c_int32(0)))

    def launch_raw(self, jobs, ids):
        """Pre-built PAIR_JOB_DTYPE array + frame id array (no Python work inside a timed region)."""
        self._n_launched = len(jobs)
        self._check(lib().uzl_match_launch(self._h, C.c_int32(len(jobs)), _p(jobs, C.c_void_p), _p(ids, c_i32p),
                                           C.c_int32(len(ids)), C.c_int32(0)))

    def collect(self, out=None):
        res = out if out is not None else np.zeros(self._n_launched, EDGE_RESULT_DTYPE)
        self._check(lib().uzl_match_collect(self._h, _p(res, C.c_void_p), None, None, None, None))
        return res

    def knn2(self, frame_from, frame_to, nq):
        out = [np.empty(nq, np.int32) for _ in range(4)]
        self._check(lib().uzl_match_knn2(self._h, C.c_int32(frame_from), C.c_int32(frame_to),
                                         *[_p(o, c_i32p) for o in out]))
        return tuple(out)

    def ransac_points(self, problems, max_error, iterations, break_percentage, do_prosac=True, job_ids=None):
        """problems: list of (P (3,M), Q (3,M)). Returns one dict per problem (T, consensus, mse, iterations_run, mask)."""
        nb = len(problems)
        offs = np.zeros(nb + 1, np.int32)
        for b, (P, _) in enumerate(problems):
            offs[b + 1] = offs[b] + np.asarray(P).shape[1]
        tot = int(offs[-1])
        Pc = np.empty((max(tot, 1), 3)); Qc = np.empty((max(tot, 1), 3))
        for b, (P, Q) in enumerate(problems):
            Pc[offs[b]:offs[b + 1]] = np.asarray(P).T; Qc[offs[b]:offs[b + 1]] = np.asarray(Q).T
        T = np.empty((nb, 12)); cons = np.empty(nb, np.int32); mse = np.empty(nb); itr = np.empty(nb, np.int32)
        mask = np.zeros(max(tot, 1), np.uint8)
        jid = np.asarray(job_ids if job_ids is not None else np.arange(nb), np.uint64)
        self._check(lib().uzl_ransac_points(self._h, C.c_int32(nb), _p(offs, c_i32p), _p(Pc, c_f64p), _p(Qc, c_f64p),
                                            C.c_double(max_error), C.c_int32(iterations), C.c_double(break_percentage),
                                            C.c_int32(1 if do_prosac else 0), _p(jid, c_u64p), _p(T, c_f64p),
                                            _p(cons, c_i32p), _p(mse, c_f64p), _p(itr, c_i32p), _p(mask, c_u8p)))
        return [dict(T=T[b].reshape(3, 4), consensus=int(cons[b]), mse=float(mse[b]), iterations_run=int(itr[b]),
                     mask=mask[offs[b]:offs[b + 1]].copy()) for b in range(nb)]

    def set_profiling(self, on):
        self._check(lib().uzl_match_set_profiling(self._h, C.c_int32(1 if on else 0)))

    def kernel_times(self):
        cap = 32
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); ln = (C.c_int32 * cap)()
        n = lib().uzl_match_kernel_times(self._h, C.c_int32(cap), names, ms, ln)
        return {names[i].decode(): dict(ms=ms[i], launches=ln[i]) for i in range(max(n, 0))}


# --------------------------------------------------------------------------------------- optimizer
class Pgo(_Handle):
    """Thin object wrapper over the uzl_pgo_* C ABI."""

    _prefix, _cfg_type = "uzl_pgo", PgoCfg
    set_config = _Handle._set_config

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.n = 0
        self.e_in = 0

    def add_graph(self, nodes_pose, nodes_fixed, edges, sensors=None):
        """Reference-shaped input (SlamNode / SlamEdge arrays, see synth.make_pose_graph)."""
        n = len(nodes_fixed); ne = len(edges["from"])
        na = np.zeros(max(n, 1), NODE_DTYPE)
        na["pose"][:n] = np.asarray(nodes_pose, np.float64).reshape(n, 12); na["fixed"][:n] = nodes_fixed
        ea = np.zeros(max(ne, 1), EDGE_DTYPE)
        for k in ("from", "to", "type", "sensor_from", "sensor_to", "valid"):
            ea[k][:ne] = edges[k]
        for k, w in (("transform", 12), ("displacement_from", 12), ("displacement_to", 12), ("information", 36)):
            ea[k][:ne] = np.asarray(edges[k], np.float64).reshape(ne, w)
        if "diff_time" in edges:
            ea["diff_time"][:ne] = edges["diff_time"]
        S = np.ascontiguousarray(sensors, np.float64).reshape(-1, 12) if sensors is not None and len(sensors) else None
        self._check(self._lib().uzl_pgo_add_graph(self._h, C.c_int32(n), _p(na, C.c_void_p), C.c_int32(ne), _p(ea, C.c_void_p),
                                            C.c_int32(0 if S is None else S.shape[0]), _p(S, c_f64p)))
        self.n = n; self.e_in = ne

    @staticmethod
    def pack_edges(edges, lo=0, hi=None):
        """SlamEdge dict-of-arrays (synth.make_pose_graph) -> EDGE_DTYPE array of edges [lo, hi)."""
        hi = len(edges["from"]) if hi is None else hi
        ne = hi - lo
        ea = np.zeros(max(ne, 1), EDGE_DTYPE)
        for k in ("from", "to", "type", "sensor_from", "sensor_to", "valid"):
            ea[k][:ne] = edges[k][lo:hi]
        for k, w in (("transform", 12), ("displacement_from", 12), ("displacement_to", 12), ("information", 36)):
            ea[k][:ne] = np.asarray(edges[k][lo:hi], np.float64).reshape(ne, w)
        if "diff_time" in edges:
            ea["diff_time"][:ne] = edges["diff_time"][lo:hi]
        return ea, ne

    def append_graph(self, new_pose, new_fixed, new_edges, flag_index=None, flag_valid=None):
        """uzl_pgo_append_graph: the resident graph grown by new nodes / edges (`new_edges`: dict like add_graph's, or a packed EDGE_DTYPE
        array), the valid flag of old input edges flag_index set to flag_valid.  Old nodes keep the handle's current estimates."""
        n = len(new_fixed)
        na = np.zeros(max(n, 1), NODE_DTYPE)
        na["pose"][:n] = np.asarray(new_pose, np.float64).reshape(n, 12); na["fixed"][:n] = new_fixed
        if isinstance(new_edges, np.ndarray):
            ea, ne = np.ascontiguousarray(new_edges), len(new_edges)
            if ne == 0:
                ea = np.zeros(1, EDGE_DTYPE)
        else:
            ea, ne = self.pack_edges(new_edges)
        fi = np.ascontiguousarray(flag_index if flag_index is not None else [], np.int32)
        fv = np.ascontiguousarray(flag_valid if flag_valid is not None else [], np.uint8)
        assert fi.shape == fv.shape
        self._check(self._lib().uzl_pgo_append_graph(self._h, C.c_int32(n), _p(na, C.c_void_p), C.c_int32(ne), _p(ea, C.c_void_p),
                                               C.c_int32(len(fi)), _p(fi, c_i32p), _p(fv, c_u8p)))
        self.n += n; self.e_in += ne

    def rewrite_graph(self, drop_nodes=(), pose_nodes=(), poses=None, xf=None, ops=()):
        """uzl_pgo_rewrite_graph: the resident graph shrunk in place.  drop_nodes / pose_nodes: old node indices; poses (n_pose, 12);
        xf (n_xf, 12); ops: rows (edge, action, xf, node) or a PGO_EDGE_OP_DTYPE array.  merge.pgo_rewrite_of_plan / _of_drops make the
        arguments.  -> (old_to_new_node, old_to_new_edge), -1 = gone."""
        drop = np.ascontiguousarray(drop_nodes, np.int32).reshape(-1)
        pn = np.ascontiguousarray(pose_nodes, np.int32).reshape(-1)
        P = np.ascontiguousarray(poses if poses is not None else [], np.float64).reshape(-1, 12)
        X = np.ascontiguousarray(xf if xf is not None else [], np.float64).reshape(-1, 12)
        assert len(P) == len(pn)
        if isinstance(ops, np.ndarray) and ops.dtype == PGO_EDGE_OP_DTYPE:
            oa = np.ascontiguousarray(ops)
        else:
            rows = np.ascontiguousarray(ops, np.int32).reshape(-1, 4)
            oa = np.zeros(len(rows), PGO_EDGE_OP_DTYPE)
            for j, k in enumerate(("edge", "action", "xf", "node")):
                oa[k] = rows[:, j]
        rw = PgoRewrite(len(drop), _p(drop, c_i32p), len(pn), _p(pn, c_i32p), _p(P, c_f64p), len(X), _p(X, c_f64p), len(oa), _p(oa, C.c_void_p))
        node_map = np.empty(max(self.n, 1), np.int32); edge_map = np.empty(max(self.e_in, 1), np.int32)
        self._check(self._lib().uzl_pgo_rewrite_graph(self._h, C.byref(rw), C.c_int32(self.n), _p(node_map, c_i32p), C.c_int32(self.e_in), _p(edge_map, c_i32p)))
        node_map, edge_map = node_map[:self.n], edge_map[:self.e_in]
        self.n = int((node_map >= 0).sum()); self.e_in = int((edge_map >= 0).sum())
        return node_map, edge_map

    def set_graph(self, poses, fixed, ij, meas, info, robust):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12); f = np.ascontiguousarray(fixed, np.uint8)
        ijc = np.ascontiguousarray(ij, np.int32).reshape(-1, 2)
        Z = np.ascontiguousarray(meas, np.float64).reshape(-1, 12)
        Om = np.ascontiguousarray(info, np.float64).reshape(-1, 36); rb = np.ascontiguousarray(robust, np.uint8)
        self._check(self._lib().uzl_pgo_set_graph(self._h, C.c_int32(P.shape[0]), _p(P, c_f64p), _p(f, c_u8p),
                                            C.c_int32(ijc.shape[0]), _p(ijc, c_i32p), _p(Z, c_f64p), _p(Om, c_f64p),
                                            _p(rb, c_u8p)))
        self.n = P.shape[0]; self.e_in = ijc.shape[0]

    def reset(self):
        self._check(self._lib().uzl_pgo_reset(self._h))

    def set_shard(self, rank, world, allreduce=None):
        """Sharded single-graph solve (BASELINE config 4).  allreduce(dev_ptr:int, count:int, stream:int) -> int must sum
        `count` doubles at dev_ptr in place over all ranks (0 = ok).  See uzliti_slam_amd/sharded.py for the RCCL one."""
        if allreduce is None:
            self._shard_cb = ALLREDUCE_FN()
        else:
            def _cb(ptr, count, stream, user):
                try:
                    return int(allreduce(int(ptr or 0), int(count), int(stream or 0)))
                except Exception:      # never let an exception cross the C ABI
                    import traceback
                    traceback.print_exc()
                    return -1
            self._shard_cb = ALLREDUCE_FN(_cb)
        self._check(self._lib().uzl_pgo_set_shard(self._h, C.c_int32(rank), C.c_int32(world), self._shard_cb, None))

    def set_shard_rccl(self, rank, world, unique_id):
        """Native exchange: the handle owns the RCCL communicator (collective call: every rank, same id from rccl_unique_id())."""
        buf = (C.c_char * RCCL_UNIQUE_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(self._lib().uzl_pgo_set_shard_rccl(self._h, C.c_int32(rank), C.c_int32(world), buf, C.c_int32(RCCL_UNIQUE_ID_BYTES)))

    def rccl_ranks(self):
        """ncclCommCount of the handle's communicator (0: none)."""
        return int(self._lib().uzl_pgo_rccl_ranks(self._h))

    def optimize(self, iterations=0):
        st = PgoStats()
        rc = self._check(self._lib().uzl_pgo_optimize(self._h, C.c_int32(iterations), C.byref(st)),
                         allow=(UZL_ERR_NOT_CONVERGED,))
        d = st.as_dict(); d["status"] = rc
        return d

    def store(self):
        poses = np.empty((self.n, 12)); err = np.empty(max(self.e_in, 1)); used = np.empty(max(self.e_in, 1), np.uint8)
        self._check(self._lib().uzl_pgo_store(self._h, _p(poses, c_f64p), _p(err, c_f64p), _p(used, c_u8p)))
        return poses, err[:self.e_in], used[:self.e_in]

    def get_fixed(self):
        f = np.empty(self.n, np.uint8)
        self._check(self._lib().uzl_pgo_get_fixed(self._h, _p(f, c_u8p)))
        return f

    def set_profiling(self, on):
        self._check(self._lib().uzl_pgo_set_profiling(self._h, C.c_int32(1 if on else 0)))

    def kernel_times(self):
        cap = 64
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); ln = (C.c_int32 * cap)()
        n = self._lib().uzl_pgo_kernel_times(self._h, C.c_int32(cap), names, ms, ln)
        return {names[i].decode(): dict(ms=ms[i], launches=ln[i]) for i in range(max(n, 0))}


class DiagPgo(Pgo):
    """A Pgo handle of the diagnostic library (diag_lib), with its stage-level hooks of the linear system (uzl_pgo_debug.hip, UZL_DIAG): the
    handle is created and fed by that library's own uzl_pgo_* - a handle of the product library must never reach a uzl_debug_* hook."""

    _lib = staticmethod(lambda: diag_lib())

    def linearize(self):
        """One linearisation at the handle's current poses (after gauge + structure, as optimize): dict of v2b [n], row_ptr [nb+1],
        col [nslots] (-1: fixed neighbour), blk [nslots,6,6] (H_{a,col} of row a, one slot per incident edge), haa [nb,6,6], b [nb,6],
        chi2, diagmax, poses [n,12] (the linearisation point as store() writes it)."""
        L = self._lib()
        sz = np.zeros(4, np.int32)
        self._check(L.uzl_debug_pgo_linearize(self._h, _p(sz, c_i32p), None, None, None, None, None, None, None, None))
        n, nb, ns, _ = (int(v) for v in sz)
        v2b = np.zeros(max(n, 1), np.int32); rp = np.zeros(nb + 1, np.int32); col = np.zeros(max(ns, 1), np.int32)
        blk = np.zeros((max(ns, 1), 6, 6)); haa = np.zeros((max(nb, 1), 6, 6)); b = np.zeros((max(nb, 1), 6))
        sc = np.zeros(2); P = np.zeros((max(n, 1), 12))
        self._check(L.uzl_debug_pgo_linearize(self._h, _p(sz, c_i32p), _p(v2b, c_i32p), _p(rp, c_i32p), _p(col, c_i32p), _p(blk, c_f64p),
                                              _p(haa, c_f64p), _p(b, c_f64p), _p(sc, c_f64p), _p(P, c_f64p)))
        assert tuple(int(v) for v in sz[:3]) == (n, nb, ns), "the structure changed between the two calls"
        return dict(v2b=v2b[:n], row_ptr=rp, col=col[:ns], blk=blk[:ns], haa=haa[:nb], b=b[:nb], chi2=float(sc[0]), diagmax=float(sc[1]),
                    poses=P[:n])

    def solve(self, lam=-1.0):
        """One linear solve (H + lam I) dx = b at the current poses as an LM trial does it (lam < 0: lambda_init = 1e-5 max |H_jj|):
        dict of dx [n,6] (zero rows for fixed vertices), its, converged, guard_trips, lam, res_ratio (|r|^2 / |b|^2), rz_end, rz_stop."""
        n = self.n
        dx = np.zeros((max(n, 1), 6)); info = np.zeros(8)
        self._check(self._lib().uzl_debug_pgo_solve(self._h, C.c_double(lam), _p(dx, c_f64p), _p(info, c_f64p)))
        return dict(dx=dx[:n], its=int(info[0]), converged=bool(info[1]), guard_trips=int(info[3]), lam=float(info[4]),
                    res_ratio=float(info[5]), rz_end=float(info[6]), rz_stop=float(info[7]))

    def reduced(self, lam=-1.0):
        """The Schur-reduced system for lam (< 0: lambda_init), as the PCG sees it, or None when the structure has no reduction: dict of
        sep_rows [nbr] (full-system row per reduced row, -1: empty row), row_ptr, col, blk [slots,6,6], hdiag [nbr,6,6] (without the
        separators' lambda I, which the SpMV adds), b [nbr,6]."""
        L = self._lib()
        sz = np.zeros(3, np.int32)
        self._check(L.uzl_debug_pgo_reduced(self._h, C.c_double(lam), _p(sz, c_i32p), None, None, None, None, None, None))
        if not sz[2]:
            return None
        nr, ns = int(sz[0]), int(sz[1])
        sep = np.zeros(max(nr, 1), np.int32); rp = np.zeros(nr + 1, np.int32); col = np.zeros(max(ns, 1), np.int32)
        blk = np.zeros((max(ns, 1), 6, 6)); hd = np.zeros((max(nr, 1), 6, 6)); b = np.zeros((max(nr, 1), 6))
        self._check(L.uzl_debug_pgo_reduced(self._h, C.c_double(lam), _p(sz, c_i32p), _p(sep, c_i32p), _p(rp, c_i32p), _p(col, c_i32p),
                                            _p(blk, c_f64p), _p(hd, c_f64p), _p(b, c_f64p)))
        assert (int(sz[0]), int(sz[1])) == (nr, ns), "the structure changed between the two calls"
        return dict(sep_rows=sep[:nr], row_ptr=rp, col=col[:ns], blk=blk[:ns], hdiag=hd[:nr], b=b[:nr])

    def apply_info(self):
        """What the handle's PCG applies: dict(op = 0 block-Jacobi / 1 additive multilevel / 2 multiplicative, agg, cl, rows)."""
        info = np.zeros(4)
        self._check(self._lib().uzl_debug_pgo_apply(self._h, C.c_double(-1.0), C.c_int32(0), None, None, _p(info, c_f64p)))
        return dict(op=int(info[0]), agg=int(info[1]), cl=int(info[2]), rows=int(info[3]))

    def apply(self, op, x, lam=-1.0):
        """op 0: (A + lam I) x with the PCG's own SpMV; op 1: M^-1 x with the preconditioner the PCG applies for lam (< 0: lambda_init).
        x, result: [rows, 6] in the numbering of the system the PCG iterates on (reduced() when the structure has a reduction)."""
        xx = np.ascontiguousarray(x, np.float64).reshape(-1, 6)
        y = np.zeros_like(xx); info = np.zeros(4)
        self._check(self._lib().uzl_debug_pgo_apply(self._h, C.c_double(lam), C.c_int32(op), _p(xx, c_f64p), _p(y, c_f64p), _p(info, c_f64p)))
        assert int(info[3]) == xx.shape[0], "x has %d rows, the system %d" % (xx.shape[0], int(info[3]))
        return y

    def pcg_state(self, k, lam=-1.0):
        """The PCG's state after k iterations on the system's own right-hand side (uzl_debug_pgo_pcg_state): dict of x, r, z, p [rows,6],
        rg [n_g,6] (the gather-level residual the next ml_cg would read), gather_level, done, its, lam."""
        L = self._lib()
        info = np.zeros(6)
        self._check(L.uzl_debug_pgo_pcg_state(self._h, C.c_double(lam), C.c_int32(k), None, None, None, None, None, _p(info, c_f64p)))
        rows, ng = int(info[0]), int(info[2])
        if rows == 0:
            return None
        x, r, z, pp = (np.zeros((rows, 6)) for _ in range(4))
        rg = np.zeros((ng, 6))
        self._check(L.uzl_debug_pgo_pcg_state(self._h, C.c_double(lam), C.c_int32(k), _p(x, c_f64p), _p(r, c_f64p), _p(z, c_f64p), _p(pp, c_f64p),
                                              _p(rg, c_f64p), _p(info, c_f64p)))
        return dict(x=x, r=r, z=z, p=pp, rg=rg, gather_level=int(info[1]), done=int(info[3]), its=int(info[4]), lam=float(info[5]))

    def ban_mult(self):
        """Before the first graph: the handle's structures start with the additive dense operator (what a handle does once the
        multiplicative operator has broken down on one of its graphs)."""
        self._check(self._lib().uzl_debug_pgo_ban_mult(self._h))

    def trial(self, dx, lam=0.0):
        """One LM trial's retraction and evaluation for the step dx [n,6] (rows of fixed vertices are ignored), from the current poses,
        which stay as they are (uzl_debug_pgo_trial): dict of poses [n,12] (what oplus_kernel stored, as store() writes poses),
        part_inlane / part_stored (the per-workgroup chi2 partials of chi2_trial_kernel - poses retracted in the edge lane - and of
        chi2_kernel on the stored trial poses, same grid), scale (computeScale = sum dx (lam dx + b)), chi2_inlane, chi2_stored."""
        L = self._lib()
        n = self.n
        d = np.ascontiguousarray(dx, np.float64).reshape(-1, 6)
        assert d.shape[0] == n, "dx has %d rows, the graph %d vertices" % (d.shape[0], n)
        sz = np.zeros(1, np.int32)
        self._check(L.uzl_debug_pgo_trial(self._h, None, C.c_double(lam), _p(sz, c_i32p), None, None, None, None))
        g = int(sz[0])
        P = np.zeros((max(n, 1), 12)); pa = np.zeros(max(g, 1)); pb = np.zeros(max(g, 1)); info = np.zeros(4)
        self._check(L.uzl_debug_pgo_trial(self._h, _p(d, c_f64p), C.c_double(lam), _p(sz, c_i32p), _p(P, c_f64p), _p(pa, c_f64p),
                                          _p(pb, c_f64p), _p(info, c_f64p)))
        assert int(sz[0]) == g, "the structure changed between the two calls"
        return dict(poses=P[:n], part_inlane=pa[:g], part_stored=pb[:g], scale=float(info[0]), chi2_inlane=float(info[1]),
                    chi2_stored=float(info[2]))

    def _hier_array(self, level, what, dtype, shape):
        L = self._lib()
        nbytes = C.c_int64(0)
        self._check(L.uzl_debug_pgo_hierarchy(self._h, C.c_double(0.0), C.c_int32(0), C.c_int32(level), C.c_int32(what), None, None, None,
                                              C.byref(nbytes)))
        out = np.zeros(max(nbytes.value // np.dtype(dtype).itemsize, 1), dtype)
        if nbytes.value:
            room = C.c_int64(out.nbytes)
            self._check(L.uzl_debug_pgo_hierarchy(self._h, C.c_double(0.0), C.c_int32(0), C.c_int32(level), C.c_int32(what), None, None,
                                                  out.ctypes.data_as(C.c_void_p), C.byref(room)))
            assert room.value == nbytes.value, "the structure changed between the two calls"
        out = out[:nbytes.value // np.dtype(dtype).itemsize]
        return out.reshape(shape) if nbytes.value else None

    def hierarchy(self, lam=-1.0, ns_steps=-1):
        """The multilevel hierarchy after the set-up an LM trial makes for lam (< 0: lambda_init), with ns_steps Newton-Schulz steps at
        the composite level (< 0: what the first trial takes; 0: the cycle's X_0), as the set-up kernels left it (uzl_debug_pgo_hierarchy):
        dict(levels, cl, agg, mult, ns_steps, upper_ns, sibling0, rows, c32_stride, reduced, strong, strong_blocks, structure_ns_steps,
        cg_variant (LmCgVariant: 0 plain1, 1 comp1, 2 plain4, 3 comp4, 4 comp4 Ypre, 5 comp4 Vpre), lam,
        b2v [rows] (-1: EMPTY row), top_inv, Cmat32 [6 n_cl, c32_stride] (None without a dense operator), lv = one dict per level of
        n, fan, nslots, row_ptr, col, blk [nslots,6,6], G [n,6,6], M (levels >= 1), geo ([n,12] at level 0, [n,3] above), cen [n,4]
        (levels >= 1), Winv [n_{l+1}, 6 fan, 6 fan] (levels < L), Y [(6 n)^2] (cl <= l < L)).  levels = 0: block-Jacobi, nothing else."""
        info = np.zeros(64, np.int32)
        lam_used = C.c_double(0.0)
        self._check(self._lib().uzl_debug_pgo_hierarchy(self._h, C.c_double(lam), C.c_int32(ns_steps), C.c_int32(0), C.c_int32(-1),
                                                        _p(info, c_i32p), C.byref(lam_used), None, None))
        keys = ("levels", "cl", "agg", "mult", "ns_steps", "upper_ns", "sibling0", "rows", "c32_stride", "reduced", "strong", "strong_blocks",
                "structure_ns_steps", "cg_variant")
        out = dict(zip(keys, (int(v) for v in info[:len(keys)])), lam=lam_used.value, lv=[])
        L, cl = out["levels"], out["cl"]
        if L == 0:
            return out
        for l in range(L + 1):
            n, fan, ns = int(info[16 + l]), int(info[32 + l]), int(info[48 + l])
            m = 6 * int(info[32 + l + 1]) if l < L else 0
            lv = dict(n=n, fan=fan, nslots=ns, row_ptr=self._hier_array(l, 0, np.int32, (n + 1,)))
            lv["col"] = self._hier_array(l, 1, np.int32, (ns,)) if ns else np.zeros(0, np.int32)
            lv["blk"] = self._hier_array(l, 2, np.float64, (ns, 6, 6)) if ns else np.zeros((0, 6, 6))
            lv["G"] = self._hier_array(l, 3, np.float64, (n, 6, 6))
            lv["M"] = self._hier_array(l, 4, np.float64, (n, 6, 6))
            lv["geo"] = self._hier_array(l, 5, np.float64, (n, 12 if l == 0 else 3))
            lv["cen"] = self._hier_array(l, 6, np.float64, (n, 4))
            lv["Winv"] = self._hier_array(l, 7, np.float64, (int(info[16 + l + 1]), m, m)) if l < L else None
            lv["Y"] = self._hier_array(l, 8, np.float64, (6 * n, 6 * n)) if (cl and cl <= l < L) else None
            out["lv"].append(lv)
        nt = out["lv"][L]["n"]
        out["top_inv"] = self._hier_array(L, 9, np.float64, (6 * nt, 6 * nt))
        out["Cmat32"] = self._hier_array(cl, 10, np.float32, (6 * out["lv"][cl]["n"], out["c32_stride"])) if cl else None
        out["b2v"] = self._hier_array(0, 11, np.int32, (out["rows"],))
        return out


class _BorrowedPgo(Pgo):
    """A Pgo over a handle the batch owns: neither close() nor the finaliser may destroy it."""

    def close(self):
        self._h = None

    __del__ = close


class PgoBatch(_Handle):
    """uzl_pgo_batch_*: n independent graphs solved through shared launches.  `graphs[i]` is an ordinary Pgo over handle i
    (add_graph / set_graph / reset / store); optimize() solves them all and returns one stats dict per graph."""

    _prefix, _cfg_type, _cfg_default = "uzl_pgo_batch", PgoCfg, "uzl_pgo_cfg_default"

    def __init__(self, n_graphs, **cfg):
        super().__init__(C.c_int32(n_graphs), **cfg)
        self.graphs = []
        for i in range(n_graphs):
            p = _BorrowedPgo.__new__(_BorrowedPgo)
            p.cfg = self.cfg; p._h = C.c_void_p(lib().uzl_pgo_batch_graph(self._h, i)); p.n = 0; p.e_in = 0
            self.graphs.append(p)
        self.n_batched = 0

    def optimize(self, iterations=0):
        n = len(self.graphs)
        st = (PgoStats * n)(); nb = C.c_int32()
        rc = self._check(lib().uzl_pgo_batch_optimize(self._h, C.c_int32(iterations), st, C.byref(nb)), allow=(UZL_ERR_NOT_CONVERGED,))
        self.n_batched = nb.value
        out = []
        for i in range(n):
            d = st[i].as_dict(); d["status"] = rc
            out.append(d)
        return out

    def set_resident(self, n):
        """graphs solved at a time (0 = all); the rest of the batch waits in a queue and takes the slots of finished graphs"""
        rc = lib().uzl_pgo_batch_set_resident(self._h, C.c_int32(n))
        if rc != UZL_OK:
            raise UzlError(rc, "uzl_pgo_batch_set_resident")

    def set_profiling(self, on):
        lib().uzl_pgo_batch_set_profiling(self._h, C.c_int32(1 if on else 0))

    def kernel_times(self):
        cap = 16
        names = (C.c_char_p * cap)(); ms = (C.c_double * cap)(); ln = (C.c_int32 * cap)()
        n = lib().uzl_pgo_batch_kernel_times(self._h, C.c_int32(cap), names, ms, ln)
        return {names[i].decode(): dict(ms=ms[i], launches=ln[i]) for i in range(max(n, 0))}

    def close(self):
        if getattr(self, "_h", None):
            for p in self.graphs:
                p._h = None
        super().close()

    __del__ = close


# --------------------------------------------------------------------------------------- edge filter
class Filter(_Handle):
    """uzl_filter_* (TransformationFilter / EdgeCluster, transformation_filter.cpp:43-350)."""

    _prefix, _cfg_type = "uzl_filter", FilterCfg

    def set_sensors(self, sensors):
        s = np.ascontiguousarray(sensors, np.float64).reshape(-1, 12)
        self._check(lib().uzl_filter_set_sensors(self._h, C.c_int32(len(s)), _p(s, c_f64p)))

    def add(self, edges):
        arr, keep = pack_filter_edges(edges)
        self._check(lib().uzl_filter_add(self._h, C.c_int32(len(edges)), arr))

    def add_packed(self, arr):
        """arr: FILTER_EDGE_DTYPE array; the stamp arrays its pointer fields address must stay alive for the call."""
        a = np.ascontiguousarray(arr, FILTER_EDGE_DTYPE)
        if len(a):
            self._check(lib().uzl_filter_add(self._h, C.c_int32(len(a)), _p(a, C.c_void_p)))

    def remove(self, keys):
        k = np.ascontiguousarray(keys, np.uint64)
        self._check(lib().uzl_filter_remove(self._h, C.c_int32(len(k)), _p(k, c_u64p)))

    def _keys(self, fn):
        n = C.c_int32()
        self._check(fn(self._h, C.c_int32(0), None, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint64)
        self._check(fn(self._h, C.c_int32(len(out)), _p(out, c_u64p), C.byref(n)))
        return out[:n.value]

    def all_edges(self):
        return self._keys(lib().uzl_filter_all_edges)

    def valid_edges(self):
        return self._keys(lib().uzl_filter_valid_edges)

    def calc_valid_edges(self):
        n = C.c_int32()
        self._check(lib().uzl_filter_calc_valid_edges(self._h, C.byref(n)))
        return n.value

    def clusters(self, with_eval=False):
        """clusters_ in order: list of dicts (info + keys + valid [+ P, Q, T, ransac_consensus of the last evaluation])."""
        out = []
        for i in range(self._check(lib().uzl_filter_cluster_count(self._h))):
            ci = ClusterInfo()
            self._check(lib().uzl_filter_cluster_info(self._h, C.c_int32(i), C.byref(ci)))
            d = ci.as_dict()
            keys = np.zeros(max(ci.size, 1), np.uint64); valid = np.zeros(max(ci.size, 1), np.uint8)
            self._check(lib().uzl_filter_cluster_edges(self._h, C.c_int32(i), C.c_int32(len(keys)), _p(keys, c_u64p), _p(valid, c_u8p)))
            d["keys"] = keys[:ci.size]; d["valid"] = valid[:ci.size]
            if with_eval:
                cap = max(ci.size + 128, 256)
                P = np.zeros((cap, 3)); Q = np.zeros((cap, 3)); T = np.zeros(12); rc = C.c_int32()
                m = self._check(lib().uzl_filter_cluster_last_eval(self._h, C.c_int32(i), C.c_int32(cap), _p(P, c_f64p), _p(Q, c_f64p),
                                                                   _p(T, c_f64p), C.byref(rc)))
                d.update(P=P[:m].copy(), Q=Q[:m].copy(), T=T, ransac_consensus=rc.value)
            out.append(d)
        return out


# --------------------------------------------------------------------------------------- edge acceptance gate
class Gate(_Handle):
    """uzl_gate_* (GraphSlamNode::newEdgeCallback / checkEdgeHeuristic / SlamGraph::astar)."""

    _prefix, _cfg_type = "uzl_gate", GateCfg

    def set_graph(self, poses, edges, merged=None):
        """poses (n,12); edges: GATE_EDGE_DTYPE array (from, to, type, valid); merged (n) u8 or None."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        E = np.ascontiguousarray(edges, GATE_EDGE_DTYPE)
        m = None if merged is None else np.ascontiguousarray(merged, np.uint8)
        self._check(self._lib().uzl_gate_set_graph(self._h, C.c_int32(len(P)), _p(P, c_f64p), _p(m, c_u8p), C.c_int32(len(E)),
                                             _p(E, C.c_void_p) if len(E) else None))

    def check(self, cand, want_dist=True):
        """-> (accept u8, valid u8, astar_dist f64 or None) per candidate, in order.  want_dist=False passes astar_dist = NULL: the verdicts
        are the same, and the searches whose verdict the straight-line distance between the nodes already decides are not run."""
        Cn = np.ascontiguousarray(cand, GATE_EDGE_DTYPE)
        n = len(Cn)
        acc = np.zeros(max(n, 1), np.uint8); val = np.zeros(max(n, 1), np.uint8); dist = np.zeros(max(n, 1)) if want_dist else None
        self._check(self._lib().uzl_gate_check(self._h, C.c_int32(n), _p(Cn, C.c_void_p) if n else None, _p(acc, c_u8p), _p(val, c_u8p),
                                         _p(dist, c_f64p) if want_dist else None))
        return acc[:n], val[:n], (dist[:n] if want_dist else None)

    def edge_count(self):
        return self._check(self._lib().uzl_gate_edge_count(self._h))


class DiagGate(Gate):
    """A Gate handle of the diagnostic library (diag_lib), the only one stages() works on: created and fed by that library's own
    uzl_gate_* - a handle of the product library must never reach a uzl_debug_* hook."""

    _lib = staticmethod(lambda: diag_lib())

    def stages(self):
        """uzl_debug_gate_stages: per candidate of the last check(), the launch that wrote its final outputs - 0 none (refused by the
        host's index checks), 1 settled without the reference's search (straight line or ball), 2 gate_reg_kernel<2>,
        3 gate_reg_kernel<4>, 4 gate_wave_kernel, 5 gate_kernel."""
        L = self._lib()
        L.uzl_debug_gate_stages.argtypes = [C.c_void_p, c_u8p, C.c_int32]
        cap = 1 << 16
        while True:
            out = np.zeros(cap, np.uint8)
            n = self._check(L.uzl_debug_gate_stages(self._h, _p(out, c_u8p), C.c_int32(cap)))
            if n < cap:
                return out[:n].copy()
            cap *= 4


def schur_plan(row_ptr, col, cap=24):
    """uzl_pgo_schur_plan (host only) -> dict(red_row, run_id, run_pos, row_ptr, col, n_reduced, n_runs)."""
    rp = np.ascontiguousarray(row_ptr, np.int32); cl = np.ascontiguousarray(col, np.int32)
    nb = len(rp) - 1
    red_row = np.empty(max(nb, 1), np.int32); run_id = np.empty(max(nb, 1), np.int32); run_pos = np.empty(max(nb, 1), np.int32)
    rrp = np.zeros(nb + 1, np.int32); cap_slots = len(cl) + 2 * nb + 2; rcol = np.empty(cap_slots, np.int32)
    nr = C.c_int32(); nruns = C.c_int32()
    i32 = C.POINTER(C.c_int32)
    rc = lib().uzl_pgo_schur_plan(C.c_int32(nb), rp.ctypes.data_as(i32), cl.ctypes.data_as(i32), C.c_int32(cap), red_row.ctypes.data_as(i32),
                                  run_id.ctypes.data_as(i32), run_pos.ctypes.data_as(i32), rrp.ctypes.data_as(i32), rcol.ctypes.data_as(i32),
                                  C.c_int32(cap_slots), C.byref(nr), C.byref(nruns))
    if rc != UZL_OK:
        raise UzlError(rc, lib().uzl_status_string(rc).decode())
    return dict(red_row=red_row[:nb], run_id=run_id[:nb], run_pos=run_pos[:nb], row_ptr=rrp[:nr.value + 1], col=rcol[:rrp[nr.value]],
                n_reduced=nr.value, n_runs=nruns.value)


def schur_plan_strong(row_ptr, col, slot_w, cap=24, strong_min=1, theta=0.25, one_level_max=0):
    """uzl_pgo_schur_plan_strong (host only) -> dict(red_row, sep_rows, n_reduced, n_sep, n_groups, n_blocks)."""
    rp = np.ascontiguousarray(row_ptr, np.int32); cl = np.ascontiguousarray(col, np.int32); w = np.ascontiguousarray(slot_w, np.float64)
    nb = len(rp) - 1
    assert len(w) == len(cl)
    red_row = np.empty(max(nb, 1), np.int32); cap_rows = 32 * nb + 32; sep = np.empty(cap_rows, np.int32); counts = np.zeros(5, np.int32)
    i32 = C.POINTER(C.c_int32)
    rc = lib().uzl_pgo_schur_plan_strong(C.c_int32(nb), rp.ctypes.data_as(i32), cl.ctypes.data_as(i32), C.c_int32(cap), w.ctypes.data_as(c_f64p),
                                         C.c_int32(strong_min), C.c_double(theta), C.c_int32(one_level_max), red_row.ctypes.data_as(i32), sep.ctypes.data_as(i32),
                                         C.c_int32(cap_rows), counts.ctypes.data_as(i32))
    if rc != UZL_OK:
        raise UzlError(rc, lib().uzl_status_string(rc).decode())
    return dict(red_row=red_row[:nb], sep_rows=sep[:counts[0]].copy(), n_reduced=int(counts[0]), n_sep=int(counts[1]), n_groups=int(counts[2]),
                n_blocks=int(counts[3]), contiguous=counts[4] / 1000.)


def ml_plan(row_ptr, col, precond_on=True, strong_blocks=False, mult_banned=False, comp4_off=False, arrays=True):
    """uzl_debug_ml_plan (diagnostic library, host only): the hierarchy plan of the block system row_ptr / col ->
    dict(levels, cl, agg, mult, ns_steps (the structure's), gather_level, lds, rows, lv = one dict per level of n, fan, nslots and - with
    arrays - row_ptr, col), the part of DiagPgo.hierarchy()'s dict that hierarchy_checks.check_structure reads.  levels = 0: block-Jacobi."""
    rp = np.ascontiguousarray(row_ptr, np.int32); cl = np.ascontiguousarray(col, np.int32)
    nb = len(rp) - 1
    flags = C.c_int32((1 if precond_on else 0) | (2 if strong_blocks else 0) | (4 if mult_banned else 0) | (8 if comp4_off else 0))
    L = diag_lib()

    def call(level, what, info, out, nbytes):
        rc = L.uzl_debug_ml_plan(C.c_int32(nb), _p(rp, c_i32p), _p(cl, c_i32p), flags, C.c_int32(level), C.c_int32(what), _p(info, c_i32p),
                                 out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(nbytes) if nbytes is not None else None)
        if rc != UZL_OK:
            raise UzlError(rc, "uzl_debug_ml_plan")

    def array(level, what):
        nbytes = C.c_int64(0)
        call(level, what, None, None, nbytes)
        out = np.zeros(nbytes.value // 4, np.int32)
        if nbytes.value:
            call(level, what, None, out, nbytes)
        return out

    info = np.zeros(64, np.int32)
    call(0, -1, info, None, None)
    out = dict(levels=int(info[0]), cl=int(info[1]), agg=int(info[2]), mult=int(info[3]), ns_steps=int(info[12]), gather_level=int(info[14]),
               lds=int(info[15]), rows=nb, lv=[])
    for l in range(out["levels"] + 1):
        lv = dict(n=int(info[16 + l]), fan=int(info[32 + l]), nslots=int(info[48 + l]))
        if arrays:
            lv["row_ptr"] = rp if l == 0 else array(l, 0)
            lv["col"] = cl if l == 0 else array(l, 1)
        out["lv"].append(lv)
    return out


_STRUCTURE_STAGES = dict(flatten=0, gauge=1, order=2, system=3, row_blocks=4, numbering=5, admission=6, shard=7, exchange=8, grown=9)


def pgo_structure_plan(stage, **kw):
    """uzl_debug_pgo_structure_plan (diagnostic library, host only): one stage of the structure of a pose graph (csrc/pgo_structure.hpp)
    -> dict of everything the stage decides.  Stages and their keyword arguments:
      flatten    n, fixed [n], in_edges [e_in, 4] = (from, to, odom, valid), in_w [e_in]            -> ij [e, 2], src, robust, edge_w
      gauge      n, fixed, ij                                                                       -> fixed_eff, n_gauge
      order      n, fixed (effective), ij, edge_w (None: every edge weighs 1)                       -> b2v
      system     n, ij, robust, b2v                      -> nb, nslots, n_rb, v2b, row_ptr, col, slot_edge, smeta [nslots, 4], rb_ptr, rowhdr [rows, 24]
      row_blocks row_ptr                                                                            -> rb_ptr, cap_slots, cap_rows, max_partials
      numbering  cfg_numbering, preconditioner, may_shard, num_its (2)                              -> strong_min, max_contig
      admission  nb, n_int                                                                          -> min_int, admitted
      shard      e, rank, world                                                                     -> e_begin, e_end, diag_owner
      exchange   row_ptr, col of the system the PCG solves (+ ml_plan's flags)                      -> sg, part_a, iter_span, gather_level, n_gather
      grown      old = (n, fixed, ij), new = (n, fixed, ij), window                                 -> survive, grown"""
    L = diag_lib()
    i32 = lambda a: np.ascontiguousarray(a if a is not None else [], np.int32).reshape(-1)
    u8 = lambda a: np.ascontiguousarray(a if a is not None else [], np.uint8).reshape(-1)

    def run(iv, what, dtype, dv=None, fixed=None, ij=None, robust=None, edge_w=None, aux=None):
        iv = i32(iv); dv = None if dv is None else np.ascontiguousarray(dv, np.float64)
        arrs = [None if a is None or len(a) == 0 else a for a in (fixed, ij, robust, edge_w, aux)]

        def call(out, nbytes):
            rc = L.uzl_debug_pgo_structure_plan(C.c_int32(_STRUCTURE_STAGES[stage]), _p(iv, c_i32p), _p(dv, c_f64p), _p(arrs[0], c_u8p), _p(arrs[1], c_i32p),
                                                _p(arrs[2], c_u8p), _p(arrs[3], c_f64p), _p(arrs[4], c_i32p), C.c_int32(what),
                                                out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(nbytes))
            if rc != UZL_OK:
                raise UzlError(rc, "uzl_debug_pgo_structure_plan(%s, %d)" % (stage, what))

        nbytes = C.c_int64(0)
        call(None, nbytes)
        out = np.zeros(nbytes.value // np.dtype(dtype).itemsize, dtype)
        if nbytes.value:
            call(out, nbytes)
        return out

    if stage == "flatten":
        ie = i32(kw["in_edges"]); a = dict(iv=[kw["n"], len(ie) // 4], fixed=u8(kw["fixed"]), aux=ie, edge_w=np.ascontiguousarray(kw["in_w"], np.float64))
        return dict(ij=run(what=0, dtype=np.int32, **a).reshape(-1, 2), src=run(what=1, dtype=np.int32, **a), robust=run(what=2, dtype=np.uint8, **a),
                    edge_w=run(what=3, dtype=np.float64, **a))
    if stage in ("gauge", "order"):
        ij = i32(kw["ij"]); a = dict(iv=[kw["n"], len(ij) // 2], fixed=u8(kw["fixed"]), ij=ij)
        if stage == "gauge":
            return dict(fixed_eff=run(what=0, dtype=np.uint8, **a), n_gauge=int(run(what=1, dtype=np.int32, **a)[0]))
        w = kw.get("edge_w")
        return dict(b2v=run(what=0, dtype=np.int32, edge_w=None if w is None else np.ascontiguousarray(w, np.float64), **a))
    if stage == "system":
        ij = i32(kw["ij"]); b2v = i32(kw["b2v"]); a = dict(iv=[kw["n"], len(ij) // 2, len(b2v)], ij=ij, robust=u8(kw["robust"]), aux=b2v)
        sz = run(what=0, dtype=np.int32, **a)
        out = dict(nb=int(sz[0]), nslots=int(sz[1]), n_rb=int(sz[2]))
        for what, k in enumerate(("v2b", "row_ptr", "col", "slot_edge", "smeta", "rb_ptr", "rowhdr"), 1):
            out[k] = run(what=what, dtype=np.int32, **a)
        out["smeta"] = out["smeta"].reshape(-1, 4); out["rowhdr"] = out["rowhdr"].reshape(-1, 24)
        return out
    if stage == "row_blocks":
        rp = i32(kw["row_ptr"]); a = dict(iv=[len(rp) - 1], aux=rp)
        caps = run(what=1, dtype=np.int32, **a)
        return dict(rb_ptr=run(what=0, dtype=np.int32, **a), cap_slots=int(caps[0]), cap_rows=int(caps[1]), max_partials=int(caps[2]))
    if stage == "numbering":
        r = run(iv=[kw["cfg_numbering"], kw["preconditioner"], 1 if kw["may_shard"] else 0], dv=kw["num_its"], what=0, dtype=np.float64)
        return dict(strong_min=int(r[0]), max_contig=float(r[1]))
    if stage == "admission":
        r = run(iv=[kw["nb"], kw["n_int"]], what=0, dtype=np.int32)
        return dict(min_int=int(r[0]), admitted=bool(r[1]))
    if stage == "shard":
        r = run(iv=[kw["e"], kw["rank"], kw["world"]], what=0, dtype=np.int32)
        return dict(e_begin=int(r[0]), e_end=int(r[1]), diag_owner=int(r[2]))
    if stage == "exchange":
        rp = i32(kw["row_ptr"])
        flags = ((1 if kw.get("precond_on", True) else 0) | (2 if kw.get("strong_blocks") else 0) | (4 if kw.get("mult_banned") else 0) |
                 (8 if kw.get("comp4_off") else 0))
        r = run(iv=[len(rp) - 1, flags], aux=rp, ij=i32(kw["col"]), what=0, dtype=np.int64)
        return dict(zip(("sg", "part_a", "iter_span", "gather_level", "n_gather"), (int(v) for v in r)))
    if stage == "grown":
        (n0, f0, ij0), (n1, f1, ij1) = kw["old"], kw["new"]
        ij0, ij1 = i32(ij0), i32(ij1)
        r = run(iv=[n0, n1, len(ij0) // 2, len(ij1) // 2, kw.get("window", 4096)], fixed=np.concatenate([u8(f0)[:n0], u8(f1)[:n1]]), aux=ij0, ij=ij1, what=0,
                dtype=np.int32)
        return dict(survive=bool(r[0]), grown=bool(r[1]))
    raise ValueError(stage)


def pgo_rewrite_plan(n, fixed, in_edges, drop_nodes=(), pose_nodes=(), n_xf=0, ops=()):
    """uzl_debug_pgo_rewrite_plan (diagnostic library, host only): rewrite_plan of csrc/pgo_structure.hpp, what uzl_pgo_rewrite_graph
    decides before it touches the device.  fixed [n]; in_edges [e_in, 4] = (from, to, odom, valid); ops rows (edge, action, xf, node).
    -> dict(n_new, e_new, old_to_new_node, new_to_old_node, old_to_new_edge, new_to_old_edge, rec [e_new, 4] = (from_new, to_new, xf_from,
    xf_to), in_edges [e_new, 4], fixed); raises UzlError(UZL_ERR_BAD_ARG) for a rewrite the plan refuses."""
    L = diag_lib()
    i32 = lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)
    fx = np.ascontiguousarray(fixed, np.uint8).reshape(-1); ie = i32(in_edges); dr = i32(drop_nodes); pn = i32(pose_nodes); op = i32(ops)
    iv = i32([n, len(ie) // 4, len(dr), len(pn), n_xf, len(op) // 4])
    ptr = lambda a, t: _p(a, t) if len(a) else None

    def run(what, dtype):
        def call(out, nbytes):
            rc = L.uzl_debug_pgo_rewrite_plan(_p(iv, c_i32p), ptr(fx, c_u8p), ptr(ie, c_i32p), ptr(dr, c_i32p), ptr(pn, c_i32p), ptr(op, c_i32p), C.c_int32(what),
                                              out.ctypes.data_as(C.c_void_p) if out is not None else None, C.byref(nbytes))
            if rc != UZL_OK:
                raise UzlError(rc, "uzl_debug_pgo_rewrite_plan(%d)" % what)

        nbytes = C.c_int64(0)
        call(None, nbytes)
        out = np.zeros(nbytes.value // np.dtype(dtype).itemsize, dtype)
        if nbytes.value:
            call(out, nbytes)
        return out

    sz = run(0, np.int32)
    out = dict(n_new=int(sz[0]), e_new=int(sz[1]))
    for what, k in enumerate(("old_to_new_node", "new_to_old_node", "old_to_new_edge", "new_to_old_edge", "rec", "in_edges"), 1):
        out[k] = run(what, np.int32)
    out["rec"] = out["rec"].reshape(-1, 4); out["in_edges"] = out["in_edges"].reshape(-1, 4)
    out["fixed"] = run(7, np.uint8)
    return out


# the rows uzl_debug_lm_pass_plan reads and writes (csrc/uzl_pgo_debug.hip): a view of a snapshot, a slot's track, a pass's plan
LM_VIEW_INTS = ("phase", "need", "it", "iterations", "sync_rebuild", "pending", "ix", "pcg_last", "st_lm_trials", "max_it", "pcg_its")
LM_VIEW_DOUBLES = ("last_rel", "refresh_rel", "rate_ref", "rate_last", "rate_drop", "lambda", "lambda_setup0", "lambda_setup1", "tol2")
LM_TRACK = ("job", "active", "no_history", "solve_passes", "prev_last", "cur_last", "seen_trials")
LM_PLAN = ("flags", "want", "base", "ix", "ns_steps", "setup_captured", "any_start")
_LM_PASS_STAGES = dict(plan=0, launches=1, replay=2, host_batches=3, handover=4, init_rides=5)


def lm_pass_plan(stage, **kw):
    """uzl_debug_lm_pass_plan (diagnostic library, host only): the host's predictions about the passes of the device-resident LM loop
    (csrc/pgo_lm_pass.hpp).  A view is a dict over LM_VIEW_INTS + LM_VIEW_DOUBLES (missing keys: 0), a track one over LM_TRACK plus
    `hist`, the job's per-trial PCG counts of the last optimize; a plan comes back as a dict over LM_PLAN plus `tol2`.  Stages:
      plan         views, tracks (one per slot), first_solve_its, shape_ns_steps, wrong_ix              -> plan, tracks (afterwards)
      launches     base, want, eager                                                              -> lead, long_first, n_long, rem_first, rem
      replay       n_slots, jobs = [dict(no_history, hist)], events = ("plan",) | ("look", slot, view) | ("load", slot, job or -1, view),
                   first_solve_its, shape_ns_steps, wrong_ix                          -> plans, tracks, first_solve_its, trial_its (per job)
      host_batches prev, max_it, end_round                                                        -> the host-driven solve's batch sizes
      handover     old = [dict(gen, prev, cur)] (the last drive's jobs), new_gens                 -> prev (per new job), cur_sizes, hist_gen
      init_rides   flags, any_start, pcg_args_pass, reduced                   -> True: the pass's PCG init goes out in the head's launch"""
    L = diag_lib()
    i32 = lambda a: np.ascontiguousarray(a if a is not None else [], np.int32).reshape(-1)

    def run(iv, what, dtype=np.int32, vi=None, vd=None, tr=None, hist=None, ev=None):
        iv = i32(iv)
        arrs = [None if a is None or len(a) == 0 else a for a in (vi, vd, tr, hist, ev)]

        def call(out, nbytes):
            rc = L.uzl_debug_lm_pass_plan(C.c_int32(_LM_PASS_STAGES[stage]), _p(iv, c_i32p), _p(arrs[0], c_i32p), _p(arrs[1], c_f64p), _p(arrs[2], c_i32p),
                                          _p(arrs[3], c_i32p), _p(arrs[4], c_i32p), C.c_int32(what), out.ctypes.data_as(C.c_void_p) if out is not None else None,
                                          C.byref(nbytes))
            if rc != UZL_OK:
                raise UzlError(rc, "uzl_debug_lm_pass_plan(%s, %d)" % (stage, what))

        nbytes = C.c_int64(0)
        call(None, nbytes)
        out = np.zeros(nbytes.value // np.dtype(dtype).itemsize, dtype)
        if nbytes.value:
            call(out, nbytes)
        return out

    def views(vs):
        return (i32([[int(v.get(k, 0)) for k in LM_VIEW_INTS] for v in vs]),
                np.ascontiguousarray([[float(v.get(k, 0.)) for k in LM_VIEW_DOUBLES] for v in vs], np.float64).reshape(-1))

    def tracks_out(rows):
        return [dict(zip(LM_TRACK + ("n_hist",), (int(x) for x in r))) for r in rows.reshape(-1, 8)]

    def plans_out(rows, tol2):
        return [dict(zip(LM_PLAN, (int(x) for x in r)), tol2=float(t)) for r, t in zip(rows.reshape(-1, 7), tol2)]

    def rows_out(flat, n):                       # n rows of {length, values}
        out, k = [], 0
        for _ in range(n):
            out.append([int(x) for x in flat[k + 1:k + 1 + flat[k]]]); k += 1 + int(flat[k])
        return out

    if stage == "plan":
        vi, vd = views(kw["views"])
        tr = i32([[int(t.get(k, 0)) for k in LM_TRACK] + [len(t.get("hist", ()))] for t in kw["tracks"]])
        hist = i32([c for t in kw["tracks"] for c in t.get("hist", ())])
        a = dict(iv=[len(kw["views"]), kw.get("first_solve_its", 0), kw.get("shape_ns_steps", 0), 1 if kw.get("wrong_ix") else 0], vi=vi, vd=vd, tr=tr, hist=hist)
        return dict(plan=plans_out(run(what=0, **a), run(what=1, dtype=np.float64, **a))[0], tracks=tracks_out(run(what=2, **a)))
    if stage == "launches":
        return dict(zip(("lead", "long_first", "n_long", "rem_first", "rem"), (int(x) for x in run([kw["base"], kw["want"], 1 if kw["eager"] else 0], 0))))
    if stage == "replay":
        jobs, events = kw["jobs"], kw["events"]
        kinds = dict(plan=0, look=1, load=2)
        ev = i32([[kinds[e[0]], e[1] if len(e) > 1 else 0, e[2] if e[0] == "load" else 0] for e in events])
        vi, vd = views([e[-1] if len(e) > 1 else {} for e in events])
        a = dict(iv=[kw["n_slots"], len(events), len(jobs), kw.get("first_solve_its", 0), kw.get("shape_ns_steps", 0), 1 if kw.get("wrong_ix") else 0], vi=vi, vd=vd,
                 tr=i32([[1 if j.get("no_history") else 0, len(j.get("hist", ()))] for j in jobs]), hist=i32([c for j in jobs for c in j.get("hist", ())]), ev=ev)
        h = run(what=3, **a)
        return dict(plans=plans_out(run(what=0, **a), run(what=1, dtype=np.float64, **a)), tracks=tracks_out(run(what=2, **a)), first_solve_its=int(h[0]),
                    trial_its=rows_out(h[1:], len(jobs)))
    if stage == "host_batches":
        return [int(x) for x in run([kw["prev"], kw["max_it"], kw["end_round"]], 0)]
    if stage == "handover":
        old, new = kw["old"], list(kw["new_gens"])
        a = dict(iv=[len(old), len(new)], vi=i32([j["gen"] for j in old] + new), tr=i32([[len(j["prev"]), len(j["cur"])] for j in old]),
                 hist=i32([c for j in old for c in list(j["prev"]) + list(j["cur"])]))
        r = run(what=1, **a)
        return dict(prev=rows_out(run(what=0, **a), len(new)), cur_sizes=[int(x) for x in r[:len(new)]], hist_gen=[int(x) for x in r[len(new):]])
    if stage == "init_rides":
        return bool(run([kw["flags"], 1 if kw["any_start"] else 0, 1 if kw["pcg_args_pass"] else 0, 1 if kw["reduced"] else 0], 0)[0])
    raise ValueError(stage)


# the rows uzl_debug_lm_decide reads and writes (csrc/uzl_pgo_debug.hip): an LM state (LmDev, csrc/pgo_types.hpp)
LM_STATE_INTS = ("done", "pcg_its", "breakdown", "look", "phase", "cur", "ix", "pass", "init_pass", "schur_pass", "numeric_pass", "trial_pass", "build_pass",
                 "build_ix", "build_cur", "need", "it", "qmax", "iterations", "max_it", "pending", "adopted", "fresh", "pcg_last", "sync_rebuild", "guarded",
                 "st_pcg_iterations", "st_lm_trials", "st_precond_builds", "st_iterations_done", "st_terminated_early", "anomaly_code")
LM_STATE_DOUBLES = ("lambda", "ni", "chi_cur", "last_rel", "lambda_setup0", "lambda_setup1", "rate_ref", "rate_last", "chi2_initial", "tol_f2", "eps_t", "eps_r",
                    "refresh_rel", "tol2", "lambda_retake", "scal2_3", "rate_drop")
LM_PHASES = dict(lin=0, solve=1, retry=2, need_setup=3, done=4, anomaly=5)
LM_NEED_NUMERIC, LM_NEED_TRIAL, LM_NEED_REBUILD = 1, 2, 4
LM_PASS_SETUP, LM_PASS_REBUILD = 1, 2


def lm_decide(stage, state, scal=None, **kw):
    """uzl_debug_lm_decide (diagnostic library, host only): one application of the LM loop's state machine (csrc/pgo_lm.hpp) to `state`, a
    dict over LM_STATE_INTS + LM_STATE_DOUBLES (missing keys: 0), and the solve's scalars `scal` [16] (default: zeros).
      head   red, phase (LM_PHASES), pass_flags, chi, dmax     lm_head_decide, in front of a trial
      tail   chi_t, sc, ratio                                  lm_tail_decide, lane 0 of lm_tail_kernel behind an evaluated trial
    -> (the state afterwards, scal afterwards)"""
    L = diag_lib()
    si = np.ascontiguousarray([int(state.get(k, 0)) for k in LM_STATE_INTS], np.int32)
    sd = np.ascontiguousarray([float(state.get(k, 0.)) for k in LM_STATE_DOUBLES], np.float64)
    sc = np.zeros(16, np.float64)
    if scal is not None:
        sc[:] = scal
    if stage == "head":
        iv = np.ascontiguousarray([1 if kw.get("red") else 0, int(kw["phase"]), int(kw.get("pass_flags", 0))], np.int32)
        dv = np.ascontiguousarray([kw.get("chi", 0.), kw.get("dmax", 0.)], np.float64)
    elif stage == "tail":
        iv = np.zeros(1, np.int32)
        dv = np.ascontiguousarray([kw.get("chi_t", 0.), kw.get("sc", 0.), kw.get("ratio", 0.)], np.float64)
    else:
        raise ValueError(stage)
    rc = L.uzl_debug_lm_decide(C.c_int32(dict(head=0, tail=1)[stage]), _p(si, c_i32p), _p(sd, c_f64p), _p(sc, c_f64p), _p(iv, c_i32p), _p(dv, c_f64p))
    if rc != UZL_OK:
        raise UzlError(rc, "uzl_debug_lm_decide(%s)" % stage)
    out = dict(zip(LM_STATE_INTS, (int(x) for x in si)))
    out.update(zip(LM_STATE_DOUBLES, (float(x) for x in sd)))
    return out, sc


# --------------------------------------------------------------------------------------- distance loop-closure candidates
class Radius(_Handle):
    """uzl_radius_* (SlamGraph::getNodesWithinRadius + the caller's filters, graph_slam_node.cpp:272-289)."""

    _prefix, _cfg_type = "uzl_radius", RadiusCfg

    def set_nodes(self, poses, stamps_front_ns):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12); st = np.ascontiguousarray(stamps_front_ns, np.int64)
        self.n = len(P)
        self._check(lib().uzl_radius_set_nodes(self._h, C.c_int32(len(P)), _p(P, c_f64p), st.ctypes.data_as(C.POINTER(C.c_int64))))

    def query(self, queries, cap=None):
        q = np.ascontiguousarray(queries, np.int32)
        cap = int(cap if cap is not None else max(1, self.n * max(len(q), 1)))
        f = np.zeros(max(cap, 1), np.int32); t = np.zeros(max(cap, 1), np.int32); cnt = np.zeros(max(len(q), 1), np.int32)
        tot = C.c_int64()
        self._check(lib().uzl_radius_query(self._h, C.c_int32(len(q)), _p(q, c_i32p), C.c_int64(cap), _p(f, c_i32p), _p(t, c_i32p),
                                           _p(cnt, c_i32p), C.byref(tot)))
        w = min(tot.value, cap)
        return f[:w].copy(), t[:w].copy(), cnt[:len(q)].copy(), tot.value


# --------------------------------------------------------------------------------------- appearance-based candidates
class Places(_Handle):
    """uzl_places_* (FastLshSet / LshSetRecognizer / PlaceRecognizer, place_recognition/src)."""

    _prefix, _cfg_type = "uzl_places", PlacesCfg

    @staticmethod
    def _d(desc):
        d = np.ascontiguousarray(desc, np.uint8)
        return d, (d.shape[0] if d.ndim == 2 else 0), (d.shape[1] if d.ndim == 2 else 32)

    def search_and_add(self, desc, stamp_ns, cap=64):
        d, rows, nb = self._d(desc)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32(); idx = C.c_int32()
        self._check(lib().uzl_places_search_and_add(self._h, _p(d, c_u8p) if rows else None, C.c_int32(rows), C.c_int32(nb), C.c_int64(int(stamp_ns)),
                                                    C.c_int32(cap), _p(out, c_i32p), C.byref(n), C.byref(idx)))
        return out[:min(n.value, cap)].copy(), idx.value

    def add(self, desc, stamp_ns):
        d, rows, nb = self._d(desc)
        idx = C.c_int32()
        self._check(lib().uzl_places_add(self._h, _p(d, c_u8p) if rows else None, C.c_int32(rows), C.c_int32(nb), C.c_int64(int(stamp_ns)), C.byref(idx)))
        return idx.value

    def search(self, desc, stamp_ns, query_place=-1, cap=64):
        d, rows, nb = self._d(desc)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32()
        self._check(lib().uzl_places_search(self._h, _p(d, c_u8p) if rows else None, C.c_int32(rows), C.c_int32(nb), C.c_int64(int(stamp_ns)),
                                            C.c_int32(query_place), C.c_int32(cap), _p(out, c_i32p), C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def remove(self, place, desc):
        d, rows, nb = self._d(desc)
        self._check(lib().uzl_places_remove(self._h, C.c_int32(place), _p(d, c_u8p) if rows else None, C.c_int32(rows), C.c_int32(nb)))

    def count(self):
        return self._check(lib().uzl_places_count(self._h))

    def last_counts(self):
        n = self._check(lib().uzl_places_last_counts(self._h, C.c_int32(0), None))
        out = np.zeros(max(n, 1), np.int32)
        self._check(lib().uzl_places_last_counts(self._h, C.c_int32(len(out)), _p(out, c_i32p)))
        return out[:n]


class Gist(_Handle):
    """uzl_gist_* (BinaryGistRecognizer / PlaceRecognizer, place_recognition/src): exact k-NN under the Hamming distance over one
    binary GIST descriptor per node.  desc=None stands for a node without a GIST sensor."""

    _prefix, _cfg_type = "uzl_gist", GistCfg

    @staticmethod
    def _d(desc):
        if desc is None:
            return None, None, 0
        d = np.ascontiguousarray(desc, np.uint8).reshape(-1)
        return d, _p(d, c_u8p), len(d)

    def _cap(self, cap, n=1):
        return n * max(self.cfg.k_nearest_neighbors, 1) if cap is None else cap

    def search_and_add(self, desc, stamp_ns, cap=None):
        d, dp, nb = self._d(desc)
        cap = self._cap(cap)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32(); idx = C.c_int32()
        self._check(lib().uzl_gist_search_and_add(self._h, dp, C.c_int32(nb), C.c_int64(int(stamp_ns)), C.c_int32(cap), _p(out, c_i32p),
                                                  C.byref(n), C.byref(idx)))
        return out[:min(n.value, cap)].copy(), idx.value

    def add(self, desc, stamp_ns):
        d, dp, nb = self._d(desc)
        idx = C.c_int32()
        self._check(lib().uzl_gist_add(self._h, dp, C.c_int32(nb), C.c_int64(int(stamp_ns)), C.byref(idx)))
        return idx.value

    def search(self, desc, stamp_ns, query_place=-1, cap=None):
        d, dp, nb = self._d(desc)
        cap = self._cap(cap)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32()
        self._check(lib().uzl_gist_search(self._h, dp, C.c_int32(nb), C.c_int64(int(stamp_ns)), C.c_int32(query_place), C.c_int32(cap),
                                          _p(out, c_i32p), C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def remove(self, place):
        self._check(lib().uzl_gist_remove(self._h, C.c_int32(place)))

    def count(self):
        return self._check(lib().uzl_gist_count(self._h))

    @staticmethod
    def _batch(desc, has_gist, n):
        if desc is None:
            return None, None, None, None, 0
        d = np.ascontiguousarray(desc, np.uint8).reshape(n, -1)
        hg = None if has_gist is None else np.ascontiguousarray(has_gist, np.uint8).reshape(n)
        return d, _p(d, c_u8p), hg, _p(hg, c_u8p), d.shape[1]

    def search_and_add_batch(self, desc, stamps_ns, has_gist=None, cap=None):
        """n successive search_and_add calls; returns (neighbour lists per node, first place index, total found).  With a cap
        below the total, the lists hold what was written (the first cap neighbours in node order)."""
        st = np.ascontiguousarray(stamps_ns, np.int64).reshape(-1)
        n = len(st)
        d, dp, hg, hp, nb = self._batch(desc, has_gist, n)
        cap = self._cap(cap, n)
        out = np.zeros(max(cap, 1), np.int32); cnt = np.zeros(max(n, 1), np.int32)
        total = C.c_int64(); first = C.c_int32()
        self._check(lib().uzl_gist_search_and_add_batch(self._h, C.c_int32(n), dp, hp, C.c_int32(nb), _p(st, c_i64p), C.c_int64(cap),
                                                        _p(out, c_i32p), _p(cnt, c_i32p), C.byref(total), C.byref(first)))
        offs = np.concatenate([[0], np.cumsum(cnt[:n])]).astype(np.int64)
        lists = [out[min(offs[i], cap):min(offs[i + 1], cap)].copy() for i in range(n)]
        return lists, first.value, total.value

    def add_batch(self, desc, stamps_ns, has_gist=None):
        st = np.ascontiguousarray(stamps_ns, np.int64).reshape(-1)
        n = len(st)
        d, dp, hg, hp, nb = self._batch(desc, has_gist, n)
        first = C.c_int32()
        self._check(lib().uzl_gist_add_batch(self._h, C.c_int32(n), dp, hp, C.c_int32(nb), _p(st, c_i64p), C.byref(first)))
        return first.value

    def last_knn(self):
        """(place, distance) of the last single search / search_and_add before the time and reported-once filters"""
        n = self._check(lib().uzl_gist_last_knn(self._h, C.c_int32(0), None, None))
        pl = np.zeros(max(n, 1), np.int32); di = np.zeros(max(n, 1), np.int32)
        self._check(lib().uzl_gist_last_knn(self._h, C.c_int32(n), _p(pl, c_i32p), _p(di, c_i32p)))
        return pl[:n], di[:n]


class Gfr(_Handle):
    """uzl_gfr_* (GlobalFeatureRepositoryRecognizer / PlaceRecognizer, place_recognition/src): every row of a node finds its nearest
    feature in a repository of all distinct features seen so far, matched rows vote for the places linked to their feature.
    desc = (rows, bytes) u8, or None for a node without a FeatureData."""

    _prefix, _cfg_type = "uzl_gfr", GfrCfg

    @staticmethod
    def _d(desc):
        if desc is None:
            return None, None, 0, 0
        d = np.ascontiguousarray(desc, np.uint8)
        d = d.reshape(d.shape[0], -1) if d.ndim >= 2 else d.reshape(1, -1)
        return d, _p(d, c_u8p), d.shape[0], d.shape[1]

    def _cap(self, cap):
        return self.count() + 1 if cap is None else cap

    def search_and_add(self, desc, stamp_ns, feature_type=2, cap=None):
        d, dp, rows, nb = self._d(desc)
        cap = self._cap(cap)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32(); idx = C.c_int32()
        self._check(lib().uzl_gfr_search_and_add(self._h, dp, C.c_int32(rows), C.c_int32(nb), C.c_int32(feature_type), C.c_int64(int(stamp_ns)),
                                                 C.c_int32(cap), _p(out, c_i32p), C.byref(n), C.byref(idx)))
        return out[:min(n.value, cap)].copy(), idx.value

    def add(self, desc, stamp_ns, feature_type=2):
        d, dp, rows, nb = self._d(desc)
        idx = C.c_int32()
        self._check(lib().uzl_gfr_add(self._h, dp, C.c_int32(rows), C.c_int32(nb), C.c_int32(feature_type), C.c_int64(int(stamp_ns)),
                                      C.byref(idx)))
        return idx.value

    def search(self, desc, stamp_ns, feature_type=2, query_place=-1, cap=None):
        d, dp, rows, nb = self._d(desc)
        cap = self._cap(cap)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32()
        self._check(lib().uzl_gfr_search(self._h, dp, C.c_int32(rows), C.c_int32(nb), C.c_int32(feature_type), C.c_int64(int(stamp_ns)),
                                         C.c_int32(query_place), C.c_int32(cap), _p(out, c_i32p), C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def remove(self, place):
        self._check(lib().uzl_gfr_remove(self._h, C.c_int32(place)))

    def count(self):
        return self._check(lib().uzl_gfr_count(self._h))

    def feature_count(self):
        return self._check(lib().uzl_gfr_feature_count(self._h))

    def link_count(self):
        return self._check(lib().uzl_gfr_link_count(self._h))

    def last_matches(self):
        """(matched feature or -1, nearest distance or -1) per row of the last call that matched rows"""
        n = self._check(lib().uzl_gfr_last_matches(self._h, C.c_int32(0), None, None))
        ft = np.zeros(max(n, 1), np.int32); di = np.zeros(max(n, 1), np.int32)
        self._check(lib().uzl_gfr_last_matches(self._h, C.c_int32(n), _p(ft, c_i32p), _p(di, c_i32p)))
        return ft[:n], di[:n]

    def last_votes(self):
        """votes per place index of the last search / search_and_add that matched rows"""
        n = self._check(lib().uzl_gfr_last_votes(self._h, C.c_int32(0), None))
        v = np.zeros(max(n, 1), np.int32)
        self._check(lib().uzl_gfr_last_votes(self._h, C.c_int32(n), _p(v, c_i32p)))
        return v[:n]

    def get_feature(self, feature, nbytes=64):
        """(stored bytes, links in ascending place order with duplicates); nbytes = the repository's byte length (the library
        writes that many; the default returns them zero-padded to 64)"""
        d = np.zeros(64, np.uint8); n = C.c_int32()
        self._check(lib().uzl_gfr_get_feature(self._h, C.c_int32(feature), _p(d, c_u8p), C.c_int32(0), None, C.byref(n)))
        pl = np.zeros(max(n.value, 1), np.int32)
        self._check(lib().uzl_gfr_get_feature(self._h, C.c_int32(feature), _p(d, c_u8p), C.c_int32(n.value), _p(pl, c_i32p), C.byref(n)))
        return d[:nbytes], pl[:n.value]


class Scope(_Handle):
    """uzl_scope_* (SlamGraph::reevaluateUncertainty / getOutOfScopeNodes, GraphSlamNode::scopeRequestTimerCallback /
    scopeRequestCallback): uncertainty_ of every node as its shortest-path distance from the oldest node, and the scope lists drawn
    from it.  Node and edge ids are indices in the reference's std::map id order."""

    _prefix, _cfg_type = "uzl_scope", ScopeCfg

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.n = 0

    @staticmethod
    def _graph(poses, uncertainty, edges):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        u = None if uncertainty is None else np.ascontiguousarray(uncertainty, np.float64).reshape(len(P))
        E = np.zeros(0, GATE_EDGE_DTYPE) if edges is None else np.ascontiguousarray(edges, GATE_EDGE_DTYPE)
        return P, u, E

    def set_graph(self, poses, uncertainty, edges):
        """poses (n,12); uncertainty (n) or None; edges: GATE_EDGE_DTYPE array (from, to, type, valid)."""
        P, u, E = self._graph(poses, uncertainty, edges)
        self._check(self._lib().uzl_scope_set_graph(self._h, C.c_int32(len(P)), _p(P, c_f64p) if len(P) else None, _p(u, c_f64p),
                                                    C.c_int32(len(E)), _p(E, C.c_void_p) if len(E) else None))
        self.n = len(P)

    def add(self, poses, uncertainty, edges):
        """new nodes (k,12) with their uncertainty (k) or None, and new edges, appended"""
        P, u, E = self._graph(poses, uncertainty, edges)
        self._check(self._lib().uzl_scope_add(self._h, C.c_int32(len(P)), _p(P, c_f64p) if len(P) else None, _p(u, c_f64p),
                                              C.c_int32(len(E)), _p(E, C.c_void_p) if len(E) else None))
        self.n += len(P)

    def set_poses(self, poses):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        self._check(self._lib().uzl_scope_set_poses(self._h, C.c_int32(len(P)), _p(P, c_f64p) if len(P) else None))

    def poses_from_pgo(self, pgo):
        """the current estimates of a Pgo handle on the same device, read where they lie"""
        self._check(self._lib().uzl_scope_poses_from_pgo(self._h, pgo._h))

    def set_valid(self, edge_index, valid):
        i = np.ascontiguousarray(edge_index, np.int32); v = np.ascontiguousarray(valid, np.uint8)
        assert i.shape == v.shape
        self._check(self._lib().uzl_scope_set_valid(self._h, C.c_int32(len(i)), _p(i, c_i32p), _p(v, c_u8p)))

    def set_uncertainty(self, node, value):
        self._check(self._lib().uzl_scope_set_uncertainty(self._h, C.c_int32(node), C.c_double(value)))

    def reevaluate(self, node=-1):
        """-> (start, n_reached): node < 0 is reevaluateUncertainty(), node >= 0 reevaluateUncertainty(id)"""
        start = C.c_int32(); reached = C.c_int32()
        self._check(self._lib().uzl_scope_reevaluate(self._h, C.c_int32(node), C.byref(start), C.byref(reached)))
        return start.value, reached.value

    def _doubles(self, fn):
        out = np.zeros(max(self.n, 1))
        n = self._check(fn(self._h, C.c_int32(self.n), _p(out, c_f64p)))
        return out[:n]

    def uncertainty(self):
        return self._doubles(self._lib().uzl_scope_uncertainty)

    def distance(self):
        """distance_ of the last pass; DBL_MAX = not reached"""
        return self._doubles(self._lib().uzl_scope_distance)

    def request(self, current, cap=None):
        """-> (current_scope_, ids out of scope, ascending); with a cap below their number only the first cap ids"""
        cap = self.n if cap is None else cap
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32(); radius = C.c_double()
        self._check(self._lib().uzl_scope_request(self._h, C.c_int32(current), C.byref(radius), C.c_int32(cap), _p(out, c_i32p), C.byref(n)))
        self.last_total = n.value
        return radius.value, out[:min(n.value, cap)].copy()

    def select(self, center, radius, have, cap=None):
        """-> ids within radius of center that are not among have, ascending"""
        cap = self.n if cap is None else cap
        c = np.ascontiguousarray(center, np.float64).reshape(3); hv = np.ascontiguousarray(have, np.int32).reshape(-1)
        out = np.zeros(max(cap, 1), np.int32); n = C.c_int32()
        self._check(self._lib().uzl_scope_select(self._h, _p(c, c_f64p), C.c_double(radius), C.c_int32(len(hv)), _p(hv, c_i32p) if len(hv) else None,
                                                 C.c_int32(cap), _p(out, c_i32p), C.byref(n)))
        self.last_total = n.value
        return out[:min(n.value, cap)].copy()

    def stats(self):
        """barrier rounds and strict improvements of the last pass, and whether its distances lived in LDS"""
        r = C.c_int64(); x = C.c_int64(); l = C.c_int32()
        self._check(self._lib().uzl_scope_stats(self._h, C.byref(r), C.byref(x), C.byref(l)))
        return dict(rounds=r.value, relaxations=x.value, in_lds=l.value)


def _plan_dict(out, action):
    return dict(ratio=out.ratio, new_pose=np.array(out.new_pose), keep_displacement=np.array(out.keep_displacement),
                drop_displacement=np.array(out.drop_displacement), action=action, touched=out.n_touched, retargeted=out.n_retargeted,
                deleted=out.n_deleted)


class Merge(_Handle):
    """uzl_merge_* (GraphSlamNode::mergeTimerCallback over SlamGraph::getNodesWithinHops, and mergeNodes): which node the merge
    timer would fold into which, searched on the device, and the rewrite of the graph as a host-side plan.  Node and edge ids are
    indices in the reference's std::map id order."""

    _prefix, _cfg_type = "uzl_merge", MergeCfg

    def __init__(self, **cfg):
        super().__init__(**cfg)
        self.n = self.n_edges = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_graph(self, poses, edges):
        """poses (n,12); edges: GATE_EDGE_DTYPE array (from, to, type, valid) or None."""
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        E = np.zeros(0, GATE_EDGE_DTYPE) if edges is None else np.ascontiguousarray(edges, GATE_EDGE_DTYPE)
        self._check(self._lib().uzl_merge_set_graph(self._h, C.c_int32(len(P)), _p(P, c_f64p) if len(P) else None, C.c_int32(len(E)),
                                                    _p(E, C.c_void_p) if len(E) else None))
        self.n, self.n_edges = len(P), len(E)

    def set_poses(self, poses):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        self._check(self._lib().uzl_merge_set_poses(self._h, C.c_int32(len(P)), _p(P, c_f64p) if len(P) else None))

    def poses_from_pgo(self, pgo):
        """the current estimates of a Pgo handle on the same device, read where they lie"""
        self._check(self._lib().uzl_merge_poses_from_pgo(self._h, pgo._h))

    def set_valid(self, edge_index, valid):
        i = np.ascontiguousarray(edge_index, np.int32); v = np.ascontiguousarray(valid, np.uint8)
        assert i.shape == v.shape
        self._check(self._lib().uzl_merge_set_valid(self._h, C.c_int32(len(i)), _p(i, c_i32p), _p(v, c_u8p)))

    def search(self, first_index, center, radius):
        """one tick -> (keep, drop, next_index); keep = drop = -1: nothing to merge"""
        c = np.ascontiguousarray(center, np.float64).reshape(3)
        k = C.c_int32(); d = C.c_int32(); nx = C.c_int32()
        self._check(self._lib().uzl_merge_search(self._h, C.c_int32(first_index), _p(c, c_f64p), C.c_double(radius), C.byref(k), C.byref(d),
                                                 C.byref(nx)))
        return k.value, d.value, nx.value

    def partners(self, center, radius):
        """partner(i) of every node, -1 for a node the start test rejects or one without a partner"""
        c = np.ascontiguousarray(center, np.float64).reshape(3)
        out = np.full(max(self.n, 1), -1, np.int32)
        n = self._check(self._lib().uzl_merge_partners(self._h, _p(c, c_f64p), C.c_double(radius), C.c_int32(self.n), _p(out, c_i32p)))
        return out[:n]

    def stats(self):
        """the starts the last search walked from and the nodes those walks marked"""
        a = C.c_int64(); b = C.c_int64()
        self._check(self._lib().uzl_merge_stats(self._h, C.byref(a), C.byref(b)))
        return dict(starts_walked=a.value, nodes_visited=b.value)

    def plan(self, keep, drop, n_stamps_keep=1, n_stamps_drop=1):
        """mergeNodes for (keep, drop) over the current graph -> dict(ratio, new_pose, keep_displacement, drop_displacement, action
        [n_edges] int8 of MERGE_EDGE_*, touched, retargeted, deleted, keep, drop)"""
        out = MergePlanOut(); action = np.zeros(max(self.n_edges, 1), np.int8)
        ne = self._check(self._lib().uzl_merge_plan(self._h, C.c_int32(keep), C.c_int32(drop), C.c_int32(n_stamps_keep),
                                                    C.c_int32(n_stamps_drop), C.byref(out), C.c_int32(self.n_edges),
                                                    action.ctypes.data_as(C.c_void_p)))
        return dict(_plan_dict(out, action[:ne]), keep=keep, drop=drop)


def merge_plan(n_nodes, pose_keep, pose_drop, edges, keep, drop, n_stamps_keep=1, n_stamps_drop=1):
    """uzl_debug_merge_plan (diagnostic library, host only): the plan of Merge.plan for two poses and an edge list given, without a
    handle or a device."""
    L = diag_lib()
    Tk = np.ascontiguousarray(pose_keep, np.float64).reshape(12); Td = np.ascontiguousarray(pose_drop, np.float64).reshape(12)
    E = np.zeros(0, GATE_EDGE_DTYPE) if edges is None else np.ascontiguousarray(edges, GATE_EDGE_DTYPE)
    out = MergePlanOut(); action = np.zeros(max(len(E), 1), np.int8)
    L.uzl_debug_merge_plan.argtypes = [C.c_int32, c_f64p, c_f64p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       C.POINTER(MergePlanOut), C.c_void_p]
    rc = L.uzl_debug_merge_plan(n_nodes, _p(Tk, c_f64p), _p(Td, c_f64p), len(E), _p(E, C.c_void_p) if len(E) else None, keep, drop,
                                n_stamps_keep, n_stamps_drop, C.byref(out), action.ctypes.data_as(C.c_void_p))
    if rc < 0:
        raise UzlError(rc, "uzl_debug_merge_plan")
    return dict(_plan_dict(out, action[:rc]), keep=keep, drop=drop)


def _store_compact(handle, fn, count):
    """uzl_grid_compact -> (old_to_new [old count] int32 with -1 for a retired item, n_new)"""
    m = np.full(max(count, 1), -1, np.int32)
    n_new = C.c_int32(-1)
    handle._check(fn(handle._h, C.c_int32(count), _p(m, c_i32p), C.byref(n_new)))
    return m[:count], n_new.value


def _store_bytes(handle, fn):
    """uzl_grid_store_bytes -> dict(live, allocated), bytes of device memory"""
    live = C.c_uint64(); alloc = C.c_uint64()
    handle._check(fn(handle._h, C.byref(live), C.byref(alloc)))
    return dict(live=live.value, allocated=alloc.value)


def store_compact_plan(off, size, live=None, retire=(), align=1, trig_off=None, cap=None, want_map=True):
    """uzl_debug_store_compact_plan (diagnostic library, host only): the plan of a store compaction (csrc/store_compact.hpp).  Segment
    i = (off[i], size[i]) in elements, live unless live[i] == 0 or `retire` names it.  trig_off = None: one arena closed up at
    `align`; else a scan store (scan i has size[i] values at off[i] and the table (trig_off[i], size[i])).  cap: the capacity
    handed in for the map (default: the count).  -> dict(moves [m, 3] = (src, dst, size), new_off [n] (-1: retired), used,
    old_to_new, n_new, and for a scan store trig_moves, new_trig_off, trig_used); raises UzlError(UZL_ERR_BAD_ARG) for a retire
    list with an index outside the store or listed twice and for a cap below the count."""
    L = diag_lib()
    c_i64p = C.POINTER(C.c_int64)
    o = np.ascontiguousarray(off, np.int64).reshape(-1); z = np.ascontiguousarray(size, np.int64).reshape(-1)
    n = len(o)
    assert len(z) == n
    t = None if trig_off is None else np.ascontiguousarray(trig_off, np.int64).reshape(n)
    lv = None if live is None else np.ascontiguousarray(live, np.uint8).reshape(n)
    rt = np.ascontiguousarray(retire, np.int32).reshape(-1)
    cap = n if cap is None else int(cap)
    sizes = np.zeros(4, np.int64)
    mv_a = np.zeros((max(n, 1), 3), np.int64); mv_b = np.zeros((max(n, 1), 3), np.int64)
    no_a = np.zeros(max(n, 1), np.int64); no_b = np.zeros(max(n, 1), np.int64)
    m = np.full(max(cap, 1), -1, np.int32) if want_map else None
    n_new = C.c_int32(-1)
    L.uzl_debug_store_compact_plan.argtypes = [C.c_int32, C.c_int32, c_i64p, c_i64p, c_i64p, c_u8p, C.c_int32, c_i32p, C.c_int64, C.c_int32,
                                               c_i64p, c_i64p, c_i64p, c_i64p, c_i64p, c_i32p, C.POINTER(C.c_int32)]
    rc = L.uzl_debug_store_compact_plan(0 if t is None else 1, n, _p(o, c_i64p), _p(z, c_i64p), _p(t, c_i64p), _p(lv, c_u8p), len(rt),
                                        _p(rt, c_i32p) if len(rt) else None, int(align), cap, _p(sizes, c_i64p), _p(mv_a, c_i64p),
                                        _p(no_a, c_i64p), _p(mv_b, c_i64p), _p(no_b, c_i64p), _p(m, c_i32p), C.byref(n_new))
    if rc != UZL_OK:
        raise UzlError(rc, "uzl_debug_store_compact_plan")
    out = dict(moves=mv_a[:sizes[0]].copy(), new_off=no_a[:n].copy(), used=int(sizes[1]), n_new=n_new.value,
               old_to_new=None if m is None else m[:n].copy())
    if t is not None:
        out.update(trig_moves=mv_b[:sizes[2]].copy(), new_trig_off=no_b[:n].copy(), trig_used=int(sizes[3]))
    return out


def store_compact(src, dst, moves, device=0):
    """uzl_debug_store_compact (diagnostic library): store_compact_kernel alone, ONE launch over the moves [m, 3] = (src, dst, size)
    in bytes from the uint8 array src into a copy of the uint8 array dst -> (dst after the launch, chunk bytes, kernel ms)"""
    L = diag_lib()
    c_i64p = C.POINTER(C.c_int64)
    s = np.ascontiguousarray(src, np.uint8).reshape(-1)
    d = np.array(dst, np.uint8).reshape(-1)
    mv = np.ascontiguousarray(moves, np.int64).reshape(-1, 3)
    chunk = C.c_int64(0); ms = C.c_double(0.0)
    L.uzl_debug_store_compact.argtypes = [C.c_int32, c_u8p, C.c_int64, c_u8p, C.c_int64, C.c_int32, c_i64p, c_i64p, C.POINTER(C.c_double)]
    rc = L.uzl_debug_store_compact(device, _p(s, c_u8p) if len(s) else None, len(s), _p(d, c_u8p) if len(d) else None, len(d), len(mv),
                                   _p(mv, c_i64p) if len(mv) else None, C.byref(chunk), C.byref(ms))
    if rc != UZL_OK:
        raise UzlError(rc, "uzl_debug_store_compact")
    return d, chunk.value, ms.value


class Grid(_Handle):
    """uzl_grid_* (GraphGridMapper::convertLaserScans2Map, map_projection/src/graph_grid_mapper.cpp:295-400): stored laser scans
    ray-traced into an occupancy grid at caller-given poses, fully (build) or for the nodes after the last map (extend)."""

    _prefix, _cfg_type = "uzl_grid", GridCfg
    set_config = _Handle._set_config

    @staticmethod
    def pack_scans(scans):
        """scans: dicts with node, ranges (f32), angle_min, angle_increment, range_min and optionally displacement (12 or 3x4,
        default identity) -> (GridScan array, the ranges it points into)"""
        arr = (GridScan * max(len(scans), 1))()
        keep = []
        for i, s in enumerate(scans):
            r = np.ascontiguousarray(s["ranges"], np.float32).reshape(-1)
            keep.append(r)
            g = arr[i]
            g.node = int(s["node"]); g.n_ranges = len(r)
            g.displacement[:] = np.asarray(s.get("displacement", np.eye(3, 4)), np.float64).reshape(12).tolist()
            g.angle_min = float(s["angle_min"]); g.angle_increment = float(s["angle_increment"]); g.range_min = float(s["range_min"])
            g.ranges = r.ctypes.data_as(C.POINTER(C.c_float)) if len(r) else None
        return arr, keep

    def add_scans(self, scans):
        """-> index of the first scan added"""
        arr, keep = self.pack_scans(scans)
        first = C.c_int32(-1)
        self._check(lib().uzl_grid_add_scans(self._h, C.c_int32(len(scans)), arr, C.byref(first)))
        return first.value

    def scan_count(self):
        return self._check(lib().uzl_grid_scan_count(self._h))

    def renumber_scans(self, scan_index, node):
        """stored scan scan_index[i] now belongs to node[i]; -1 retires it (every later build or extend skips it)"""
        si = np.ascontiguousarray(scan_index, np.int32).reshape(-1); nd = np.ascontiguousarray(node, np.int32).reshape(-1)
        assert si.shape == nd.shape
        self._check(lib().uzl_grid_renumber_scans(self._h, C.c_int32(len(si)), _p(si, c_i32p) if len(si) else None,
                                                  _p(nd, c_i32p) if len(nd) else None))

    def compact(self):
        """uzl_grid_compact: the scans retired with renumber_scans(.., -1) leave the device store -> (old_to_new int32, -1 = retired; n_new)"""
        return _store_compact(self, lib().uzl_grid_compact, self.scan_count())

    def store_bytes(self):
        return _store_bytes(self, lib().uzl_grid_store_bytes)

    @staticmethod
    def _poses(poses, present):
        P = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        pr = None if present is None else np.ascontiguousarray(present, np.uint8).reshape(len(P))
        return P, pr

    def build(self, poses, present=None):
        P, pr = self._poses(poses, present)
        info = GridInfo()
        self._check(lib().uzl_grid_build(self._h, C.c_int32(len(P)), _p(P, c_f64p), _p(pr, c_u8p), C.byref(info)))
        return info.as_dict()

    def extend(self, poses, first_node, present=None):
        P, pr = self._poses(poses, present)
        info = GridInfo()
        self._check(lib().uzl_grid_extend(self._h, C.c_int32(len(P)), _p(P, c_f64p), _p(pr, c_u8p), C.c_int32(first_node), C.byref(info)))
        return info.as_dict()

    def info(self):
        info = GridInfo()
        self._check(lib().uzl_grid_get_info(self._h, C.byref(info)))
        return info.as_dict()

    def read(self):
        """OccupancyGrid.data as an int8 (height, width) array"""
        i = self.info()
        out = np.zeros(i["width"] * i["height"], np.int8)
        self._check(lib().uzl_grid_read(self._h, C.c_int64(out.size), out.ctypes.data_as(C.POINTER(C.c_int8))))
        return out.reshape(i["height"], i["width"])

    def counts(self):
        """(hits, passes), uint32 (height, width) each"""
        i = self.info()
        n = i["width"] * i["height"]
        hits = np.zeros(n, np.uint32); passes = np.zeros(n, np.uint32)
        u32p = C.POINTER(C.c_uint32)
        self._check(lib().uzl_grid_counts(self._h, C.c_int64(n), hits.ctypes.data_as(u32p), passes.ctypes.data_as(u32p)))
        return hits.reshape(i["height"], i["width"]), passes.reshape(i["height"], i["width"])


def grid_ray_clip(rays, cap):
    """uzl_debug_grid_ray_clip (diagnostic library, host only): rays [n, 8] = x0, y0, x1, y1, ux0, uy0, ux1, uy1 ->
    (count [n] int64, cells [n, cap, 2] int32: the first min(count, cap) cells of each ray inside its rectangle, in walk order)"""
    q = np.ascontiguousarray(rays, np.int32).reshape(-1, 8)
    count = np.zeros(len(q), np.int64)
    cells = np.zeros((len(q), cap, 2), np.int32)
    L = diag_lib()
    L.uzl_debug_grid_ray_clip.argtypes = [C.c_int32, c_i32p, C.c_int32, C.POINTER(C.c_int64), c_i32p]
    rc = L.uzl_debug_grid_ray_clip(len(q), _p(q, c_i32p), cap, _p(count, C.POINTER(C.c_int64)), _p(cells, c_i32p))
    if rc != UZL_OK:
        raise UzlError(rc, "uzl_debug_grid_ray_clip")
    return count, cells


def grid_plan(cfg, geom, poses, scans, present=None, first_node=0):
    """uzl_debug_grid_plan (diagnostic library, host only): the bins of a build (first_node = 0) or an extend on the geometry
    geom = (origin_x, origin_y, width, height) for cfg (keywords of GridCfg over the defaults), poses [n, 12] and scans (dicts with
    node, n or ranges, range_min and optionally displacement) -> dict of tiles, ent_start, ent_scan, ent_beam, kf_start,
    kf_rect [rects, 4], ocx, ocy (per projected scan).  A refusal raises UzlError with plan()'s reason."""
    L = diag_lib()
    c = GridCfg()
    L.uzl_grid_cfg_default(C.byref(c))
    for k, v in cfg.items():
        setattr(c, k, v)
    P, pr = Grid._poses(poses, present)
    node = np.array([int(s["node"]) for s in scans], np.int32)
    n = np.array([int(s["n"]) if "n" in s else len(s["ranges"]) for s in scans], np.int32)
    rmin = np.array([float(s["range_min"]) for s in scans], np.float32)
    D = np.array([np.asarray(s.get("displacement", np.eye(3, 4)), np.float64).reshape(12) for s in scans], np.float64).reshape(-1, 12)
    origin = np.array([geom[0], geom[1]], np.float64)
    sizes = np.zeros(4, np.int64)
    err = C.create_string_buffer(256)
    c_i64p, c_f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    L.uzl_debug_grid_plan.argtypes = [C.POINTER(GridCfg), c_f64p, C.c_uint32, C.c_uint32, C.c_int32, c_f64p, c_u8p, C.c_int32, C.c_int32, c_i32p,
                                      c_f64p, c_i32p, c_f32p, c_i64p, c_i32p, c_i32p, c_i32p, c_i64p, c_i32p, c_i32p, c_i32p, c_i32p,
                                      C.c_char_p, C.c_int32]

    def call(*out):
        rc = L.uzl_debug_grid_plan(C.byref(c), _p(origin, c_f64p), int(geom[2]), int(geom[3]), len(P), _p(P, c_f64p), _p(pr, c_u8p),
                                   int(first_node), len(scans), _p(node, c_i32p), _p(D, c_f64p), _p(n, c_i32p), _p(rmin, c_f32p),
                                   _p(sizes, c_i64p), *out, err, len(err))
        if rc != UZL_OK:
            raise UzlError(rc, err.value.decode() or "uzl_debug_grid_plan")

    call(*([None] * 8))
    nr, nt, ne, nk = (int(v) for v in sizes)
    o = dict(tiles=np.zeros(nt, np.int32), ent_start=np.zeros(nt + 1, np.int32), ent_scan=np.zeros(ne, np.int32),
             ent_beam=np.zeros(ne, np.int64), kf_start=np.zeros(nt + 1, np.int32), kf_rect=np.zeros((nk, 4), np.int32),
             ocx=np.zeros(nr, np.int32), ocy=np.zeros(nr, np.int32))
    call(*[_p(o[k], c_i64p if k == "ent_beam" else c_i32p) for k in ("tiles", "ent_start", "ent_scan", "ent_beam", "kf_start", "kf_rect",
                                                                     "ocx", "ocy")])
    return o


class Laserline(_Handle):
    """uzl_laserline_* (GraphGridMapper::extractImageLaserLine + mergeLaserScans + scanMean, map_projection/src/graph_grid_mapper.cpp:
    420-468, 135-212, 605-621): depth images binned by bearing into the laser scans the occupancy grid ray-traces."""

    _prefix, _cfg_type = "uzl_laserline", LaserlineCfg
    set_config = _Handle._set_config

    @staticmethod
    def pack_images(images):
        """images: dicts with depth (2-D float32 = 32FC1 metres, or uint16 = 16UC1 millimetres; rows may be strided), fx, fy, cx, cy,
        camera_transform (12 or 3x4) and optionally group (default: the image's index, one scan per image)
        -> (DepthImage array, the pixel arrays it points into)"""
        arr = (DepthImage * max(len(images), 1))()
        keep = []
        for i, im in enumerate(images):
            d = np.asarray(im["depth"])
            if d.ndim != 2 or d.dtype not in (np.float32, np.uint16):
                raise ValueError("a depth image is a 2-D float32 or uint16 array")
            if d.size and (d.strides[1] != d.itemsize or d.strides[0] < d.shape[1] * d.itemsize):
                d = np.ascontiguousarray(d)
            keep.append(d)
            g = arr[i]
            g.encoding = DEPTH_F32_M if d.dtype == np.float32 else DEPTH_U16_MM
            if d.size:
                g.data = d.ctypes.data; g.height, g.width = d.shape; g.step = d.strides[0]
            g.fx, g.fy, g.cx, g.cy = float(im["fx"]), float(im["fy"]), float(im["cx"]), float(im["cy"])
            g.camera_transform[:] = np.asarray(im["camera_transform"], np.float64).reshape(12).tolist()
            g.group = int(im.get("group", i))
        return arr, keep

    _shape = (0, 0)                   # (scans, beams) of the resident result

    def extract(self, images):
        """-> (ranges, intensities: float32 (n_scans, n_beams); scan centres: float64 (n_scans, 3)); the scans stay on the device.
        images: a list of dicts, or what pack_images made of one"""
        arr, keep = images if isinstance(images, tuple) else self.pack_images(images)
        ns, nb = C.c_int32(0), C.c_int32(0)
        self._check(lib().uzl_laserline_extract(self._h, C.c_int32(len(keep)), arr, C.byref(ns), C.byref(nb)))
        self._shape = (ns.value, nb.value)
        return self.read()

    def read(self):
        """the resident scans, as extract returns them"""
        ns, nb = self._shape
        f32p = C.POINTER(C.c_float)
        r = np.zeros((ns, nb), np.float32); it = np.zeros((ns, nb), np.float32); ce = np.zeros((ns, 3), np.float64)
        self._check(lib().uzl_laserline_read(self._h, C.c_int32(ns), _p(r, f32p), _p(it, f32p), _p(ce, c_f64p)))
        return r, it, ce

    def to_grid(self, grid, nodes):
        """append the resident scans to a Grid's store on the device (scan i at node nodes[i]) -> index of the first scan added"""
        nd = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        first = C.c_int32(-1)
        self._check(lib().uzl_laserline_to_grid(self._h, grid._h, _p(nd, c_i32p) if len(nd) else None, C.byref(first)))
        return first.value

    def to_laser(self, laser, use_near=False):
        """append the resident scans (intensities, or ranges with use_near) to a Laser's store on the device -> index of the first"""
        first = C.c_int32(-1)
        self._check(lib().uzl_laserline_to_laser(self._h, laser._h, C.c_int32(1 if use_near else 0), C.byref(first)))
        return first.value


class ScanMerge(_Handle):
    """uzl_scanmerge_* (the LaserscanDataPtr overload of GraphGridMapper::mergeLaserScans, map_projection/src/graph_grid_mapper.cpp:
    45-133, as GraphSlamNode::mergeNodes calls it): the laser scans of (keep, drop) node pairs re-projected, re-binned on keep's grid
    and folded into one scan per pair, all pairs of a call in one launch."""

    _prefix, _cfg_type = "uzl_scanmerge", ScanMergeCfg

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @staticmethod
    def pack_scan(s):
        """s: dict with ranges, intensities (f32, one length), angle_min, angle_increment, range_min, range_max and optionally
        displacement (12 or 3x4, default identity) and stamp_ns (default 0) -> (ScanMergeScan, the arrays it points into)"""
        r = np.ascontiguousarray(s["ranges"], np.float32).reshape(-1)
        it = np.ascontiguousarray(s["intensities"], np.float32).reshape(-1)
        if len(r) != len(it):
            raise ValueError("ranges and intensities of a scan have one length")
        f32p = C.POINTER(C.c_float)
        g = ScanMergeScan()
        g.ranges = r.ctypes.data_as(f32p); g.intensities = it.ctypes.data_as(f32p); g.n_beams = len(r)
        g.angle_min = float(s["angle_min"]); g.angle_increment = float(s["angle_increment"])
        g.range_min = float(s["range_min"]); g.range_max = float(s["range_max"])
        g.displacement[:] = np.asarray(s.get("displacement", np.eye(3, 4)), np.float64).reshape(12).tolist()
        g.stamp_ns = int(s.get("stamp_ns", 0))
        return g, (r, it)

    @classmethod
    def pack_pairs(cls, pairs):
        """pairs: (keep scan, drop scan, keep_displacement, drop_displacement) with the scans as pack_scan takes them
        -> (ScanMergePair array, what it points into, [(n_beams(keep), n_beams(drop))])"""
        arr = (ScanMergePair * max(len(pairs), 1))()
        keep, shape = [], []
        for i, (a, b, Dk, Dd) in enumerate(pairs):
            ga, ka = cls.pack_scan(a); gb, kb = cls.pack_scan(b)
            keep.append((ga, ka, gb, kb))
            arr[i].keep = C.pointer(ga); arr[i].drop = C.pointer(gb)
            arr[i].keep_displacement[:] = np.asarray(Dk, np.float64).reshape(12).tolist()
            arr[i].drop_displacement[:] = np.asarray(Dd, np.float64).reshape(12).tolist()
            shape.append((ga.n_beams, gb.n_beams))
        return arr, keep, shape

    _pairs = ()                       # (n_beams(keep), n_beams(drop)) per pair of the resident result

    def run(self, pairs):
        """merge every pair; the merged scans stay on the device.  pairs: a list as pack_pairs takes it, or what it made of one"""
        arr, keep, shape = pairs if isinstance(pairs, tuple) else self.pack_pairs(pairs)
        self._check(lib().uzl_scanmerge_run(self._h, C.c_int32(len(shape)), arr))
        self._pairs = tuple(shape)
        return len(shape)

    def read(self, pair):
        """-> (ranges, intensities: float32 (n_beams(keep),); scan centre: float64 (3,)) of one pair"""
        n = self._pairs[pair][0] if 0 <= pair < len(self._pairs) else 0
        f32p = C.POINTER(C.c_float)
        r = np.zeros(max(n, 1), np.float32); it = np.zeros(max(n, 1), np.float32); ce = np.zeros(3, np.float64)
        m = self._check(lib().uzl_scanmerge_read(self._h, C.c_int32(pair), C.c_int32(n), _p(r, f32p), _p(it, f32p), _p(ce, c_f64p)))
        return r[:m], it[:m], ce

    def points(self, pair, which):
        """stage entry: per beam of list `which` (SCANMERGE_*) of one pair -> (bin int32, -1 = unused or dropped; rho float32)"""
        n = self._pairs[pair][0 if which < 2 else 1] if 0 <= pair < len(self._pairs) else 0
        b = np.zeros(max(n, 1), np.int32); rho = np.zeros(max(n, 1), np.float32)
        m = self._check(lib().uzl_scanmerge_points(self._h, C.c_int32(pair), C.c_int32(which), C.c_int32(n), _p(b, c_i32p),
                                                   _p(rho, C.POINTER(C.c_float))))
        return b[:m], rho[:m]

    def to_grid(self, grid, nodes):
        """append the merged scans to a Grid's store on the device (pair i at node nodes[i]) -> index of the first scan added"""
        nd = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        first = C.c_int32(-1)
        self._check(lib().uzl_scanmerge_to_grid(self._h, grid._h, _p(nd, c_i32p) if len(nd) else None, C.byref(first)))
        return first.value

    def to_laser(self, laser, use_near=False):
        """append the merged scans (intensities, or ranges with use_near) to a Laser's store on the device -> index of the first"""
        first = C.c_int32(-1)
        self._check(lib().uzl_scanmerge_to_laser(self._h, laser._h, C.c_int32(1 if use_near else 0), C.byref(first)))
        return first.value


class DepthFilter(_Handle):
    """uzl_depthfilter_* (feature_extraction_service_node.cpp:120-149: depth scaling, jointBilateralFilter, jointNearestFilter;
    FeatureExtractionCore::extract3dFeatures, feature_extraction_core.cpp:254-295): depth images refined against their grey images
    into the images the front end stores, bins into laser scans and lifts its keypoints with; they stay on the device."""

    _prefix, _cfg_type = "uzl_depthfilter", DepthFilterCfg
    set_config = _Handle._set_config

    @staticmethod
    def pack_guides(guides):
        """guides: 2-D uint8 arrays (rows may be strided) -> (GuideImage array, the pixel arrays it points into)"""
        arr = (GuideImage * max(len(guides), 1))()
        keep = []
        for i, g in enumerate(guides):
            g = np.asarray(g)
            if g.ndim != 2 or g.dtype != np.uint8:
                raise ValueError("a guide image is a 2-D uint8 array")
            if g.size and (g.strides[1] != 1 or g.strides[0] < g.shape[1]):
                g = np.ascontiguousarray(g)
            keep.append(g)
            if g.size:
                arr[i].data = g.ctypes.data; arr[i].height, arr[i].width = g.shape; arr[i].step = g.strides[0]
        return arr, keep

    _sizes = ()                       # (height, width) of the resident images

    def refine(self, images, guides=None):
        """images: what Laserline.pack_images takes (the intrinsics, transform and group stay with the refined image); guides: one
        2-D uint8 array per image (None only with use_bilateral_filter = 0).  The refined images stay on the device."""
        arr, keep = Laserline.pack_images(images)
        garr, gkeep = self.pack_guides(guides) if guides is not None else (None, None)
        if guides is not None and len(gkeep) != len(keep):
            raise ValueError("one guide per depth image")
        self._check(lib().uzl_depthfilter_refine(self._h, C.c_int32(len(keep)), arr, garr))
        self._sizes = tuple(d.shape for d in keep)

    def image_count(self):
        return self._check(lib().uzl_depthfilter_image_count(self._h))

    def read(self, image):
        """resident image `image` -> float32 (height, width)"""
        h, w = self._sizes[image]
        out = np.zeros((h, w), np.float32)
        n = self._check(lib().uzl_depthfilter_read(self._h, C.c_int32(image), _p(out, C.POINTER(C.c_float)), C.c_int64(out.size)))
        assert n == out.size, (n, out.shape)
        return out

    def lift(self, image, u, v, max_depth=0.0):
        """keypoints (u, v: int32) on resident image `image` -> (pos (3, n) float64, valid (n) uint8), as Match.add_frame takes them"""
        u = np.ascontiguousarray(u, np.int32).reshape(-1); v = np.ascontiguousarray(v, np.int32).reshape(-1)
        if len(u) != len(v):
            raise ValueError("u and v differ in length")
        pos = np.zeros((len(u), 3), np.float64); valid = np.zeros(len(u), np.uint8)
        self._check(lib().uzl_depthfilter_lift(self._h, C.c_int32(image), C.c_int32(len(u)), _p(u, c_i32p), _p(v, c_i32p),
                                               C.c_double(max_depth), _p(pos, c_f64p), _p(valid, c_u8p)))
        return pos.T, valid

    def to_laserline(self, laserline):
        """the laser-line handle extracts from the resident images on the device -> what Laserline.extract returns"""
        ns, nb = C.c_int32(0), C.c_int32(0)
        self._check(lib().uzl_depthfilter_to_laserline(self._h, laserline._h, C.byref(ns), C.byref(nb)))
        laserline._shape = (ns.value, nb.value)
        return laserline.read()


def _depthfilter_to_cloud(self, cloud, colors, encoding=COLOR_BGR8):
    """the cloud handle voxelises the resident images on the device with one (h, w, 3) uint8 colour image each -> index of the
    first cloud added"""
    carr, ckeep = Cloud.pack_colors(colors, encoding)
    first = C.c_int32(-1)
    self._check(lib().uzl_depthfilter_to_cloud(self._h, cloud._h, carr if len(ckeep) else None, C.byref(first)))
    return first.value


DepthFilter.to_cloud = _depthfilter_to_cloud


class Orb(_Handle):
    """uzl_orb_* (FeatureExtractionCore::extractFeatures and ::extractBinaryGist, feature_extraction_core.cpp:93-102, 119-162, over
    cv::AORB, feature_extraction/external/aorb/aorb.cpp): ORB keypoints, descriptors and the binary GIST of many mono8 images per
    call; they stay on the device.  The pattern (512 x (x, y) int8) is the caller's: the library ships none."""

    _prefix, _cfg_type = "uzl_orb", OrbCfg
    set_config = _Handle._set_config

    def __init__(self, pattern, **cfg):
        pat = None
        if pattern is not None:
            pat = np.ascontiguousarray(pattern, np.int8)
            if pat.shape != (512, 2):
                raise ValueError("the pattern is 512 points (x, y)")
        super().__init__(_p(pat, C.POINTER(C.c_int8)), **cfg)

    def extract(self, images, masks=None, gist_angles=None):
        """images, masks: 2-D uint8 arrays (rows may be strided), one mask per image or None; gist_angles: one angle in degrees per
        image, or None for no GIST.  Replaces the resident results."""
        arr, keep = DepthFilter.pack_guides(images)
        marr, mkeep = DepthFilter.pack_guides(masks) if masks is not None else (None, None)
        if masks is not None and len(mkeep) != len(keep):
            raise ValueError("one mask per image")
        ang = None
        if gist_angles is not None:
            ang = np.ascontiguousarray(gist_angles, np.float32).reshape(-1)
            if len(ang) != len(keep):
                raise ValueError("one gist angle per image")
            ang = np.concatenate([ang, np.zeros(1, np.float32)])          # never an empty array: NULL means no GIST
        self._check(lib().uzl_orb_extract(self._h, C.c_int32(len(keep)), arr, marr, _p(ang, C.POINTER(C.c_float))))

    def image_count(self):
        return self._check(lib().uzl_orb_image_count(self._h))

    def count(self, image):
        return self._check(lib().uzl_orb_count(self._h, C.c_int32(image)))

    def read(self, image):
        """-> dict(u, v, response, angle: float32 (n); octave: int32 (n); desc: uint8 (n, 32)) in the contract's order"""
        n = self.count(image)
        f32p = C.POINTER(C.c_float)
        o = dict(u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), response=np.zeros(n, np.float32), angle=np.zeros(n, np.float32),
                 octave=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8))
        m = self._check(lib().uzl_orb_read(self._h, C.c_int32(image), C.c_int32(n), _p(o["u"], f32p), _p(o["v"], f32p), _p(o["response"], f32p),
                                           _p(o["angle"], f32p), _p(o["octave"], c_i32p), _p(o["desc"], c_u8p)))
        assert m == n, (m, n)
        return o

    def gist(self, image):
        """-> uint8 (32), as Gist.search_and_add takes it"""
        out = np.zeros(32, np.uint8)
        self._check(lib().uzl_orb_gist(self._h, C.c_int32(image), _p(out, c_u8p)))
        return out

    def lift(self, image, depthfilter, df_image, max_depth=0.0):
        """the keypoints of `image` lifted on the device with resident image df_image of a DepthFilter
        -> (pos (3, n) float64, valid (n) uint8), as Match.add_frame takes them"""
        n = self.count(image)
        pos = np.zeros((n, 3), np.float64); valid = np.zeros(n, np.uint8)
        m = self._check(lib().uzl_orb_lift(self._h, C.c_int32(image), depthfilter._h, C.c_int32(df_image), C.c_double(max_depth),
                                           _p(pos, c_f64p), _p(valid, c_u8p)))
        assert m == n, (m, n)
        return pos.T, valid

    def stage_image(self, image, what, cell=-1, level=0):
        """Stage entry: one intermediate image of the last extract (what: ORB_STAGE_*; cell -1 = the whole image) -> uint8 (h, w)"""
        w, h = C.c_int32(0), C.c_int32(0)
        args = (self._h, C.c_int32(image), C.c_int32(what), C.c_int32(cell), C.c_int32(level))
        self._check(lib().uzl_orb_stage_image(*args, C.c_int64(0), None, C.byref(w), C.byref(h)))
        out = np.zeros((h.value, w.value), np.uint8)
        self._check(lib().uzl_orb_stage_image(*args, C.c_int64(out.size), _p(out, c_u8p), C.byref(w), C.byref(h)))
        assert (h.value, w.value) == out.shape
        return out

    def stage_candidates(self, image, cell, level):
        """Stage entry: the candidates of one (cell, level) before the cuts -> (x, y: int32 (n); score: uint8 (n); thr) in the
        device's arrival order"""
        args = (self._h, C.c_int32(image), C.c_int32(cell), C.c_int32(level))
        n = self._check(lib().uzl_orb_stage_candidates(*args, C.c_int32(0), None, None, None, None))
        x, y, s, thr = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), C.c_int32(-1)
        m = self._check(lib().uzl_orb_stage_candidates(*args, C.c_int32(n), _p(x, c_i32p), _p(y, c_i32p), _p(s, c_u8p), C.byref(thr)))
        assert m == n, (m, n)
        return x, y, s, thr.value


class Laser(_Handle):
    """uzl_laser_* (LaserTransformationEstimator, transformation_estimation/src/laser_transformation_estimator.cpp:134-443): stored
    laser scans aligned pair by pair with point-to-line ICP into TYPE_2D_LASER edges, all pairs of a call in one launch."""

    _prefix, _cfg_type = "uzl_laser", LaserCfg
    set_config = _Handle._set_config

    @staticmethod
    def pack_scans(scans):
        """scans: dicts with values (f32: intensities, or ranges for do_near_), angle_min, angle_increment, range_min, range_max
        -> (LaserScanIn array, the values it points into)"""
        arr = (LaserScanIn * max(len(scans), 1))()
        keep = []
        for i, s in enumerate(scans):
            v = np.ascontiguousarray(s["values"], np.float32).reshape(-1)
            keep.append(v)
            g = arr[i]
            g.n_beams = len(v)
            g.angle_min = float(s["angle_min"]); g.angle_increment = float(s["angle_increment"])
            g.range_min = float(s["range_min"]); g.range_max = float(s["range_max"])
            g.values = v.ctypes.data_as(C.POINTER(C.c_float)) if len(v) else None
        return arr, keep

    def add_scans(self, scans):
        """-> index of the first scan added"""
        arr, keep = self.pack_scans(scans)
        first = C.c_int32(-1)
        self._check(lib().uzl_laser_add_scans(self._h, C.c_int32(len(scans)), arr, C.byref(first)))
        return first.value

    def scan_count(self):
        return self._check(lib().uzl_laser_scan_count(self._h))

    @staticmethod
    def pack_pairs(pairs):
        """pairs: (scan_from, scan_to, first_guess as 12 or 3x4) -> LaserPair array"""
        arr = (LaserPair * max(len(pairs), 1))()
        for i, (f, t, guess) in enumerate(pairs):
            arr[i].scan_from = int(f); arr[i].scan_to = int(t)
            arr[i].first_guess[:] = np.asarray(guess, np.float64).reshape(12).tolist()
        return arr

    def estimate(self, pairs):
        """-> one LASER_EDGE_DTYPE record per pair.  pairs: a list of (scan_from, scan_to, first_guess), or what pack_pairs made of one"""
        arr = pairs if isinstance(pairs, C.Array) else self.pack_pairs(pairs)
        n = len(pairs) if not isinstance(pairs, C.Array) else len(arr)
        out = np.zeros(max(n, 1), LASER_EDGE_DTYPE)
        self._check(lib().uzl_laser_estimate(self._h, C.c_int32(n), arr, out.ctypes.data_as(C.POINTER(LaserEdge))))
        return out[:n]

    def correspondences(self, scan_from, scan_to, x, n_beams):
        """steps 2-4 once at x = (tx, ty, theta) -> (j1, j2, valid: int32; dist: float64), one entry per beam of scan_to"""
        pair = self.pack_pairs([(scan_from, scan_to, np.eye(3, 4))])
        xx = (C.c_double * 3)(*[float(v) for v in x])
        j1 = np.zeros(n_beams, np.int32); j2 = np.zeros(n_beams, np.int32); valid = np.zeros(n_beams, np.int32)
        dist = np.zeros(n_beams, np.float64)
        n = self._check(lib().uzl_laser_correspondences(self._h, pair, xx, _p(j1, c_i32p), _p(j2, c_i32p), _p(valid, c_i32p), _p(dist, c_f64p)))
        assert n == n_beams, (n, n_beams)
        return j1, j2, valid, dist


class Cloud(_Handle):
    """uzl_cloud_* (CloudTransformationEstimator, transformation_estimation/src/cloud_transformation_estimator.cpp:40-161, with
    GeneralizedIterativeClosestPoint6D, external/gicp6d/gicp6d.cpp): stored colour point clouds registered pair by pair into
    TYPE_3D_FULL edges, all pairs of a call without a host round trip between the outer iterations."""

    _prefix, _cfg_type = "uzl_cloud", CloudCfg
    set_config = _Handle._set_config

    @staticmethod
    def pack_colors(colors, encoding=COLOR_BGR8):
        """colors: (h, w, 3) uint8 arrays (rows may be strided) -> (ColorImage array, the pixel arrays it points into)"""
        arr = (ColorImage * max(len(colors), 1))()
        keep = []
        for i, c in enumerate(colors):
            c = np.asarray(c)
            if c.ndim != 3 or c.shape[2] != 3 or c.dtype != np.uint8:
                raise ValueError("a colour image is an (h, w, 3) uint8 array")
            if c.size and (c.strides[2] != 1 or c.strides[1] != 3 or c.strides[0] < 3 * c.shape[1]):
                c = np.ascontiguousarray(c)
            keep.append(c)
            arr[i].encoding = encoding
            if c.size:
                arr[i].data = c.ctypes.data; arr[i].height, arr[i].width = c.shape[:2]; arr[i].step = c.strides[0]
        return arr, keep

    def add_images(self, images, colors, encoding=COLOR_BGR8):
        """images: what Laserline.pack_images takes; colors: one (h, w, 3) uint8 array per image -> index of the first cloud added"""
        arr, keep = Laserline.pack_images(images)
        carr, ckeep = self.pack_colors(colors, encoding)
        if len(keep) != len(ckeep):
            raise ValueError("one colour image per depth image")
        first = C.c_int32(-1)
        self._check(self._lib().uzl_cloud_add_images(self._h, C.c_int32(len(keep)), arr, carr, C.byref(first)))
        return first.value

    def add_points(self, xyz, bgr):
        """an already-downsampled cloud: xyz (n, 3) float32, bgr (n, 3) uint8 -> its index in the store"""
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        bgr = np.ascontiguousarray(bgr, np.uint8).reshape(-1, 3)
        if len(xyz) != len(bgr):
            raise ValueError("one colour per point")
        idx = C.c_int32(-1)
        self._check(self._lib().uzl_cloud_add_points(self._h, C.c_int32(len(xyz)), _p(xyz, C.POINTER(C.c_float)), _p(bgr, c_u8p), C.byref(idx)))
        return idx.value

    def count(self):
        return self._check(self._lib().uzl_cloud_count(self._h))

    def point_count(self, cloud):
        return self._check(self._lib().uzl_cloud_read(self._h, C.c_int32(cloud), C.c_int32(0), None, None, None, None))

    def read(self, cloud):
        """-> dict(xyz (n, 3) f32, bgr (n, 3) u8, lab (n, 3) f32, cov (n, 3, 3) f64)"""
        n = self.point_count(cloud)
        xyz = np.zeros((n, 3), np.float32); bgr = np.zeros((n, 3), np.uint8); lab = np.zeros((n, 3), np.float32)
        cov = np.zeros((n, 3, 3), np.float64)
        m = self._check(self._lib().uzl_cloud_read(self._h, C.c_int32(cloud), C.c_int32(n), _p(xyz, C.POINTER(C.c_float)), _p(bgr, c_u8p),
                                             _p(lab, C.POINTER(C.c_float)), _p(cov, c_f64p)))
        assert m == n, (m, n)
        return dict(xyz=xyz, bgr=bgr, lab=lab, cov=cov)

    @staticmethod
    def pack_pairs(pairs):
        """pairs: (cloud_from, cloud_to, first_guess as 12 or 3x4) -> CloudPair array"""
        arr = (CloudPair * max(len(pairs), 1))()
        for i, (f, t, guess) in enumerate(pairs):
            arr[i].cloud_from = int(f); arr[i].cloud_to = int(t)
            arr[i].first_guess[:] = np.asarray(guess, np.float64).reshape(12).tolist()
        return arr

    def estimate(self, pairs):
        """-> one CLOUD_EDGE_DTYPE record per pair.  pairs: a list of (cloud_from, cloud_to, first_guess)"""
        arr = self.pack_pairs(pairs)
        n = len(pairs)
        out = np.zeros(max(n, 1), CLOUD_EDGE_DTYPE)
        self._check(self._lib().uzl_cloud_estimate(self._h, C.c_int32(n), arr, out.ctypes.data_as(C.POINTER(CloudEdge))))
        return out[:n]

    def correspondences(self, cloud_from, cloud_to, first_guess, T):
        """step 6 once at the estimate T (3x4) with the target moved by first_guess -> (j int32, dist2 float32, kept int32), one
        entry per point of cloud_from"""
        n = self.point_count(cloud_from)
        pair = self.pack_pairs([(cloud_from, cloud_to, first_guess)])
        TT = (C.c_double * 12)(*np.asarray(T, np.float64).reshape(12).tolist())
        j = np.zeros(n, np.int32); d = np.zeros(n, np.float32); kept = np.zeros(n, np.int32)
        m = self._check(self._lib().uzl_cloud_correspondences(self._h, pair, TT, _p(j, c_i32p), _p(d, C.POINTER(C.c_float)), _p(kept, c_i32p)))
        assert m == n, (m, n)
        return j, d, kept

    def debug_step(self, cloud_from, cloud_to, first_guess, T):
        """uzl_debug_cloud_step (the diagnostic library only: call it on a DiagCloud): one outer iteration at the estimate T through
        the kernels estimate runs -> dict(M (n, 6) f64, zero rows where not kept; sums (28): H, g, f at T; T (3, 4) after the inner
        loop; status, done, num_corr; log: one dict(mu, outcome 0 refused / 1 accepted / 2 rejected, delta (6), f) per trial)"""
        L = self._lib()
        if not hasattr(L, "uzl_debug_cloud_step"):
            raise UzlError(UZL_ERR_STATE, "uzl_debug_cloud_step exists in the diagnostic library only: use DiagCloud")
        n = self.point_count(cloud_from)
        pair = self.pack_pairs([(cloud_from, cloud_to, first_guess)])
        TT = (C.c_double * 12)(*np.asarray(T, np.float64).reshape(12).tolist())
        M = np.zeros((n, 6)); sums = np.zeros(28); Tn = np.zeros((3, 4)); state = np.zeros(4, np.int32); trials = np.zeros((100, 9))
        m = self._check(L.uzl_debug_cloud_step(self._h, pair, TT, _p(M, c_f64p), _p(sums, c_f64p), _p(Tn, c_f64p), _p(state, c_i32p),
                                               _p(trials, c_f64p)))
        assert m == n, (m, n)
        log = [dict(mu=float(t[0]), outcome=int(t[1]), delta=t[2:8].copy(), f=float(t[8])) for t in trials[:int(state[3])]]
        assert not trials[int(state[3]):].any()
        return dict(M=M, sums=sums, T=Tn, status=int(state[0]), done=int(state[1]), num_corr=int(state[2]), log=log)


class DiagCloud(Cloud):
    """A Cloud handle of the diagnostic library (diag_lib), the only one debug_step works on: created and fed by that library's own
    uzl_cloud_* - a handle of the product library must never reach a uzl_debug_* hook."""

    _lib = staticmethod(lambda: diag_lib())
