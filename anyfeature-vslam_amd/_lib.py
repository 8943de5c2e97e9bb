"""ctypes binding of libafv_hip.so (the C-ABI declared in include/afv_hip.h).

Plumbing only: no arithmetic happens here.  The library is the hand-written HIP path; if it is missing the import
fails loudly — there is no CPU fallback anywhere in this package.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libafv_hip.so")


def use_library(path):
    """measurement tooling only (bench.py --lib, tools/experiments.py): bind a variant build of the library instead of the in-tree
    one.  Must be called before the first load(); nothing in the environment can redirect the loader."""
    global LIB_PATH
    if _lib is not None:
        raise RuntimeError("the library is already loaded")
    LIB_PATH = os.path.abspath(path)


ABI_VERSION = 6  # include/afv_hip.h AFV_ABI_VERSION this mirror was written against
MAX_LEVELS = 8
DESC_BYTES = 32
OK, EINVAL, ENODEV, ENOMEM, EHIP, ECAPACITY, EUNSUPPORTED, ETIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
MATCH_KF_KF, MATCH_KF_FRAME = 0, 1
MATCH_FLOAT32 = 0x100  # OR-ed into MatchJob.mode: float rows, L2^2 distances (include/afv_hip.h AFV_MATCH_FLOAT32)
PROJ_LOCALMAP, PROJ_LASTFRAME = 0, 1
STAGES = ("pyramid", "fast_nms", "select_quadtree", "describe", "match_topk", "match_resolve", "retain_harris")

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                     ("octave", "<i4"), ("class_id", "<i4")])
assert KP_DTYPE.itemsize == 28


class OrbParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int32), ("nlevels", C.c_int32), ("scale_factor", C.c_float),
                ("fast_threshold", C.c_int32), ("max_width", C.c_int32), ("max_height", C.c_int32),
                ("max_batch", C.c_int32)]


class Geometry(C.Structure):
    _fields_ = [("nlevels", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("lw", C.c_int32 * MAX_LEVELS), ("lh", C.c_int32 * MAX_LEVELS), ("lscale", C.c_float * MAX_LEVELS),
                ("quota", C.c_int32 * MAX_LEVELS), ("cv_quota", C.c_int32 * MAX_LEVELS),
                ("cand_cap", C.c_int32 * MAX_LEVELS)]


class MatchJob(C.Structure):
    _fields_ = [("desc1", C.c_void_p), ("n1", C.c_int32), ("desc2", C.c_void_p), ("n2", C.c_int32),
                ("desc_bytes", C.c_int32),
                ("node_id1", C.c_void_p), ("seg_ptr1", C.c_void_p), ("seg_idx1", C.c_void_p), ("nnodes1", C.c_int32),
                ("node_id2", C.c_void_p), ("seg_ptr2", C.c_void_p), ("seg_idx2", C.c_void_p), ("nnodes2", C.c_int32),
                ("valid1", C.c_void_p), ("valid2", C.c_void_p), ("angle1", C.c_void_p), ("angle2", C.c_void_p),
                ("th_low", C.c_float), ("nnratio", C.c_float), ("check_orientation", C.c_int32), ("mode", C.c_int32)]


class TriJob(C.Structure):
    """struct_size first: the runtime strides the array by it and reads only what it covers (include/afv_hip.h)"""
    _fields_ = [("struct_size", C.c_uint32), ("bow", MatchJob), ("x1", C.c_void_p), ("y1", C.c_void_p), ("x2", C.c_void_p), ("y2", C.c_void_p),
                ("sigma2_2", C.c_void_p), ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float),
                ("u_right1", C.c_void_p), ("u_right2", C.c_void_p), ("only_stereo", C.c_int32)]


class TableTriJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("F12", C.c_float * 9), ("ex", C.c_float), ("ey", C.c_float), ("has_mp1", C.c_void_p), ("has_mp2", C.c_void_p),
                ("th_low", C.c_float), ("only_stereo", C.c_int32)]


class FrameView(C.Structure):
    _fields_ = [("desc32", C.c_void_p), ("n", C.c_int32), ("angle", C.c_void_p), ("node_id", C.c_void_p), ("seg_ptr", C.c_void_p),
                ("seg_idx", C.c_void_p), ("nnodes", C.c_int32)]


class ProjJob(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("desc", C.c_void_p), ("n", C.c_int32), ("desc_bytes", C.c_int32),
                ("x", C.c_void_p), ("y", C.c_void_p), ("size", C.c_void_p), ("angle", C.c_void_p), ("occupied", C.c_void_p),
                ("inf", C.c_void_p), ("min_x", C.c_float), ("min_y", C.c_float), ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("nq", C.c_int32),
                ("qdesc", C.c_void_p), ("qvalid", C.c_void_p), ("qu", C.c_void_p), ("qv", C.c_void_p), ("qr", C.c_void_p),
                ("qmin_size", C.c_void_p), ("qmax_size", C.c_void_p), ("qangle", C.c_void_p), ("qoccupies", C.c_void_p),
                ("th_high", C.c_float), ("nnratio", C.c_float), ("size_tol", C.c_float), ("inv_size_tol", C.c_float),
                ("check_orientation", C.c_int32), ("mode", C.c_int32),
                ("u_right", C.c_void_p), ("q_ur", C.c_void_p), ("q_er_max", C.c_void_p), ("float_dim", C.c_int32)]


class FrameParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("distorted", C.c_int32), ("cap", C.c_int32), ("desc_bytes", C.c_int32),
                ("float_dim", C.c_int32), ("keep_pyramid", C.c_int32)]


class StereoParams(C.Structure):
    """afv_stereo_params: the scalars of Frame::ComputeStereoMatches"""
    _fields_ = [("struct_size", C.c_uint32), ("mbf", C.c_float), ("fx", C.c_float), ("th_high", C.c_float), ("th_low", C.c_float)]


class ProjQueries(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nq", C.c_int32), ("qdesc", C.c_void_p), ("desc_bytes", C.c_int32),
                ("qvalid", C.c_void_p), ("qu", C.c_void_p), ("qv", C.c_void_p), ("qr", C.c_void_p), ("qmin_size", C.c_void_p),
                ("qmax_size", C.c_void_p), ("qangle", C.c_void_p), ("qoccupies", C.c_void_p), ("q_ur", C.c_void_p), ("q_er_max", C.c_void_p),
                ("occupied", C.c_void_p), ("th_high", C.c_float), ("nnratio", C.c_float), ("check_orientation", C.c_int32), ("mode", C.c_int32),
                ("qref_table", C.c_void_p), ("qref_slot", C.c_void_p), ("qref_idx", C.c_void_p)]


class TableCamera(C.Structure):
    """afv_table_camera: the image bounds and the grid of KeyFrame::GetFeaturesInArea for every slot of a table"""
    _fields_ = [("struct_size", C.c_uint32), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("grid_inv_w", C.c_float), ("grid_inv_h", C.c_float)]


class TableFusePose(C.Structure):
    """afv_table_fuse_pose: the decomposed Scw of Fuse(pKF, Scw, ...)"""
    _fields_ = [("R", C.c_float * 9), ("t", C.c_float * 3), ("Ow", C.c_float * 3)]


class TableFuseJob(C.Structure):
    """afv_table_fuse_job: one target keyframe of afv_table_fuse_points"""
    _fields_ = [("struct_size", C.c_uint32), ("slot", C.c_int32), ("ids", C.c_void_p), ("nq", C.c_int32), ("radius_th", C.c_float),
                ("radius_scale", C.c_float), ("th_low", C.c_float), ("use_inf_gate", C.c_int32), ("pose_override", C.POINTER(TableFusePose))]


KFFUSE_MAX_TARGETS, KFFUSE_MAX_QUERIES = 64, 1 << 20
# status of a (target, query) of afv_table_fuse_points
KFFUSE_STATUS = {"invalid": 0, "in_keyframe": 1, "not_in_view": 2, "no_feature": 3, "free": 4, "occupant_bad": 5, "replace": 6}


class PointSearch(C.Structure):
    """afv_point_search: a projection search through the ids of resident map points"""
    _fields_ = [("struct_size", C.c_uint32), ("flavour", C.c_int32), ("points", C.c_void_p), ("ids", C.c_void_p), ("nq", C.c_int32),
                ("radius_th", C.c_float), ("radius_scale", C.c_float), ("viewing_cos_limit", C.c_float), ("qframe", C.c_void_p),
                ("qangle", C.c_void_p), ("occupied", C.c_void_p), ("th_high", C.c_float), ("nnratio", C.c_float),
                ("check_orientation", C.c_int32)]


class PointProjection(C.Structure):
    """afv_point_projection: host outputs of afv_frame_project_points"""
    _fields_ = [("struct_size", C.c_uint32), ("n_in_view", C.c_int32), ("in_view", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p),
                ("ur", C.c_void_p), ("size", C.c_void_p), ("sigma", C.c_void_p), ("view_cos", C.c_void_p), ("r", C.c_void_p),
                ("qmin", C.c_void_p), ("qmax", C.c_void_p), ("er", C.c_void_p)]


PT_FRUSTUM, PT_LASTFRAME, PT_RELOC, PT_FUSE = 0, 1, 2, 3


class PoseJob(C.Structure):
    """afv_pose_job: one Optimizer::PoseOptimization on a resident frame"""
    _fields_ = [("struct_size", C.c_uint32), ("pts", C.c_void_p), ("Rcw", C.c_void_p), ("tcw", C.c_void_p)]


class PoseResult(C.Structure):
    """afv_pose_result: the pose, the counts, mvbOutlier and the per-round trace of afv_frame_pose_optimize"""
    _fields_ = [("struct_size", C.c_uint32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("n_good", C.c_int32), ("n_edges", C.c_int32),
                ("rounds", C.c_int32), ("outlier", C.c_void_p), ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4),
                ("chi2", C.c_double * 4), ("lambda_", C.c_double * 4)]


class TriPointsJob(C.Structure):
    """afv_tri_points_job: one (current keyframe, neighbour) pair of afv_table_triangulate"""
    _fields_ = ([("struct_size", C.c_uint32)] +
                [(k, C.c_float * n) for k, n in (("Rcw1", 9), ("tcw1", 3), ("Ow1", 3), ("Rcw2", 9), ("tcw2", 3), ("Ow2", 3))] +
                [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "invfx1", "invfy1", "fx2", "fy2", "cx2", "cy2", "invfx2", "invfy2",
                                          "mb1", "mb2", "mbf1", "ratio_factor", "max_size1")])


class Sim3Job(C.Structure):
    """afv_sim3_job: one (current keyframe, candidate) pair of afv_table_sim3_hypotheses"""
    _fields_ = ([("struct_size", C.c_uint32), ("fix_scale", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)] +
                [(k, C.c_float * n) for k, n in (("Rcw1", 9), ("tcw1", 3), ("Rcw2", 9), ("tcw2", 3))] +
                [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")])


SIM3_MAX_CANDIDATES, SIM3_MAX_HYPOTHESES, SIM3_MAX_MASK_WORDS = 64, 1024, 256


class Sim3OptJob(C.Structure):
    """afv_sim3opt_job: one (current keyframe, candidate) pair of afv_table_optimize_sim3"""
    _fields_ = ([("struct_size", C.c_uint32), ("fix_scale", C.c_int32), ("th2", C.c_float)] +
                [(k, C.c_float * n) for k, n in (("Rcw1", 9), ("tcw1", 3), ("Rcw2", 9), ("tcw2", 3))] +
                [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2")] +
                [("R12", C.c_float * 9), ("t12", C.c_float * 3), ("s12", C.c_float)])


class Sim3OptResult(C.Structure):
    """afv_sim3opt_result: what Optimizer::OptimizeSim3 answers for one job, and the trace of its two optimize() calls"""
    _fields_ = [("n_in", C.c_int32), ("n_corr", C.c_int32), ("n_bad", C.c_int32), ("more_iterations", C.c_int32), ("early", C.c_int32),
                ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("reserved", C.c_int32),
                ("R12", C.c_double * 9), ("t12", C.c_double * 3), ("s12", C.c_double), ("chi2", C.c_double * 2), ("lam", C.c_double * 2)]


SIM3OPT_NO_MATCH, SIM3OPT_NOT_EDGE, SIM3OPT_KEPT, SIM3OPT_REMOVED_FIRST, SIM3OPT_REMOVED_SECOND = 0, 1, 2, 3, 4


class LbaCam(C.Structure):
    """afv_lba_cam: pose and intrinsics of one keyframe of afv_table_bundle_adjust"""
    _fields_ = ([("struct_size", C.c_uint32), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3)] +
                [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "bf")])


class LbaParams(C.Structure):
    """afv_lba_params: the driver of afv_table_bundle_adjust (checks = 1: LocalBundleAdjustment, 0: BundleAdjustment)"""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32 * 2), ("robust", C.c_int32 * 2), ("checks", C.c_int32),
                ("write_points", C.c_int32), ("trial_budget", C.c_int32)]


class LbaResult(C.Structure):
    """afv_lba_result: the trace of the two optimize() calls and the counts of the two checks"""
    _fields_ = [("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("n_edges", C.c_int32), ("n_removed_first", C.c_int32),
                ("n_erase", C.c_int32), ("stopped", C.c_int32), ("chi2", C.c_double * 2), ("lam", C.c_double * 2)]


LBA_MAX_FREE, LBA_MAX_KF, LBA_MAX_POINTS, LBA_MAX_EDGES = 64, 256, 32768, 262144
LBA_EDGE_DROPPED, LBA_EDGE_KEPT, LBA_EDGE_REMOVED_KEPT, LBA_EDGE_ERASE = 0, 1, 2, 3
# afv_table_global_bundle_adjust: the same records, caps of its own
GBA_MAX_KF, GBA_MAX_POINTS, GBA_MAX_EDGES, GBA_MAX_L_BLOCKS = 4096, 524288, 2097152, 1048576


class Sim3d(C.Structure):
    """afv_sim3d: a Sim3 in double, R row-major; 13 doubles, the rows of a float64 [n, 13] array"""
    _fields_ = [("R", C.c_double * 9), ("t", C.c_double * 3), ("s", C.c_double)]


class EssParams(C.Structure):
    """afv_ess_params: the driver of afv_essential_graph"""
    _fields_ = [("struct_size", C.c_uint32), ("iterations", C.c_int32), ("lambda_init", C.c_double), ("fix_scale", C.c_int32),
                ("write_points", C.c_int32)]


class EssResult(C.Structure):
    """afv_ess_result: the trace of the one optimize() call"""
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("chi2_first", C.c_double), ("chi2_last", C.c_double), ("lam", C.c_double),
                ("l_blocks", C.c_int32), ("status", C.c_int32)]


ESS_MAX_KF, ESS_MAX_EDGES, ESS_MAX_L_BLOCKS, ESS_MAX_UPDATES = 4096, 65536, 131072, 2097152
ESS_OK, ESS_NOT_FINITE, ESS_EMPTY = 0, 1, 2
POINT_MOVED, POINT_BAD_OR_UNSET, POINT_NO_PAIR = 0, 1, 2


class RefreshParams(C.Structure):
    """afv_refresh_params: which parts afv_table_refresh_points runs"""
    _fields_ = [("struct_size", C.c_uint32), ("descriptors", C.c_int32), ("normals", C.c_int32)]


class RefreshOut(C.Structure):
    """afv_refresh_out: the host outputs of afv_table_refresh_points, any of which may be NULL"""
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_int32), ("status", C.c_void_p), ("best_obs", C.c_void_p), ("best_median", C.c_void_p)]


REFRESH_DONE, REFRESH_SKIPPED, REFRESH_NO_OBSERVATIONS, REFRESH_NO_REF, REFRESH_BAD_DISTANCE = 0, 1, 2, 3, 4


class PnpJob(C.Structure):
    """afv_pnp_job: one candidate of afv_frame_pnp_hypotheses"""
    _fields_ = [("struct_size", C.c_uint32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("min_inliers", C.c_int32),
                ("epsilon", C.c_float), ("th2", C.c_float)]


PNP_MAX_CANDIDATES, PNP_MAX_HYPOTHESES, PNP_MAX_MASK_WORDS = 64, 1024, 256


class InitJob(C.Structure):
    """afv_init_job: the constants of one afv_frame_initializer call"""
    _fields_ = ([("struct_size", C.c_uint32), ("iterations", C.c_int32), ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32)] +
                [(k, C.c_float) for k in ("fx", "fy", "cx", "cy", "sigma")])


INIT_MAX_ITERATIONS, INIT_MAX_MOTIONS, INIT_MAX_MASK_WORDS = 1024, 8, 256
INIT_ROUTE_H, INIT_ROUTE_F = 0, 1
INIT_REASON = ("ok", "too_few_matches", "d_ratio", "ambiguous", "parallax", "min_triangulated", "min_good")


class InitTrace(C.Structure):
    """afv_init_trace: what afv_frame_initializer decided on the way"""
    _fields_ = [("struct_size", C.c_uint32), ("n", C.c_int32), ("sh", C.c_float), ("sf", C.c_float), ("rh", C.c_float),
                ("best_h", C.c_int32), ("best_f", C.c_int32), ("h21", C.c_float * 9), ("f21", C.c_float * 9), ("route", C.c_int32),
                ("n_inliers", C.c_int32), ("n_motion", C.c_int32), ("best_motion", C.c_int32), ("reason", C.c_int32),
                ("n_good", C.c_int32 * INIT_MAX_MOTIONS), ("cos_parallax", C.c_float * INIT_MAX_MOTIONS),
                ("R", (C.c_float * 9) * INIT_MAX_MOTIONS), ("t", (C.c_float * 3) * INIT_MAX_MOTIONS), ("T1", C.c_float * 9), ("T2", C.c_float * 9)]


TRI_MAX_PAIRS = 64
TRI_STATUS = ("no_match", "accepted", "low_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "scale_ratio", "not_finite")
TRI_ROUTE = ("triangulated", "unproject_a", "unproject_b")
POSE_MAX_JOBS = 64
POINTS_MAX_CAPACITY = 1 << 22
PTF_SET, PTF_BAD, PTF_OBSERVED = 1, 2, 4   # afv_points_get's flag bits


class BowQuery(C.Structure):
    """afv_bow_query: the query BowVector of afv_table_score_bow - a table slot, a resident frame or host arrays"""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("slot", C.c_int32), ("n", C.c_int32), ("frame", C.c_void_p),
                ("word", C.c_void_p), ("value", C.c_void_p)]


BOW_QUERY_SLOT, BOW_QUERY_FRAME, BOW_QUERY_HOST = 0, 1, 2


class VocabTrainParams(C.Structure):
    """afv_vocab_train_params: DBoW2 Vocabulary::create on the device (binary descriptors)"""
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_int32), ("L", C.c_int32), ("desc_bytes", C.c_int32), ("seed", C.c_uint64),
                ("max_iters", C.c_int32), ("n_init", C.c_int32), ("init_centres", C.c_void_p)]


VOCAB_TRAIN_MAX_ROWS = 1 << 26


def sized(struct):
    """a job record with its struct_size filled in"""
    obj = struct()
    obj.struct_size = C.sizeof(struct)
    return obj


# every symbol include/afv_hip.h declares: (name, restype, argtypes)
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
SYMBOLS = {
    "afv_abi_version": (_i, []),
    "afv_default_orb_params": (None, [C.POINTER(OrbParams)]),
    "afv_create": (_i, [_i, C.POINTER(OrbParams), C.POINTER(_vp)]),
    "afv_destroy": (None, [_vp]),
    "afv_strerror": (C.c_char_p, [_i]),
    "afv_last_error": (C.c_char_p, [_vp]),
    "afv_max_keypoints_per_frame": (_i, [_vp]),
    "afv_stream": (_vp, [_vp]),
    "afv_orb_extract": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, C.POINTER(_i)]),
    "afv_orb_detect": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, C.POINTER(_i)]),
    "afv_orb_compute": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "afv_orb_extract_batch": (_i, [_vp, C.POINTER(_vp), _i, _i, _i, _i, _vp, _vp, _i, _vp]),
    "afv_orb_extract_batch_device": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _vp, _vp, _i, _vp, _vp, _vp]),
    "afv_orb_size_sigma": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "afv_match_bow": (_i, [_vp, C.POINTER(MatchJob), _i, _vp, _vp]),
    "afv_match_triangulation": (_i, [_vp, C.POINTER(TriJob), _i, _vp, _vp]),
    "afv_match_bruteforce_pairs_device": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _i, _vp, _vp, _vp]),
    "afv_table_create": (_i, [_vp, _i, _i, C.POINTER(_vp)]),
    "afv_table_create_bytes": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "afv_table_create_f32": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "afv_table_destroy": (None, [_vp]),
    "afv_table_set": (_i, [_vp, _i, _vp, _vp, _i]),
    "afv_table_set_featvec": (_i, [_vp, _i, _vp, _vp, _vp, _i]),
    "afv_table_set_geometry": (_i, [_vp, _i, _vp, _vp, _vp]),
    "afv_table_set_u_right": (_i, [_vp, _i, _vp]),
    "afv_table_set_valid": (_i, [_vp, _i, _vp]),
    "afv_table_device_ptrs": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp)]),
    "afv_table_sync_counts": (_i, [_vp]),
    "afv_table_match_pairs": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp]),
    "afv_table_match_pairs_device": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp, _vp]),
    "afv_table_match_bow": (_i, [_vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp]),
    "afv_table_match_triangulation": (_i, [_vp, _vp, _vp, C.POINTER(TableTriJob), _i, _vp, _vp]),
    "afv_table_match_bow_frame": (_i, [_vp, _vp, _i, C.POINTER(FrameView), _f, _f, _i, _vp, _vp]),
    "afv_table_broadcast": (_i, [_vp, _vp, _i, C.POINTER(_f)]),
    "afv_table_clone": (_i, [_vp, _vp]),
    "afv_comm_unique_id": (_i, [_vp]),
    "afv_comm_create": (_i, [_vp, _vp, _i, _i, C.POINTER(_vp)]),
    "afv_comm_destroy": (None, [_vp]),
    "afv_comm_rank": (_i, [_vp]),
    "afv_comm_size": (_i, [_vp]),
    "afv_comm_broadcast": (_i, [_vp, _vp, _sz, _i, _vp]),
    "afv_comm_allgather": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "afv_shard_range": (None, [C.c_long, _i, _i, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
    "afv_match_l2": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, _vp, _f, _f, _vp, _vp]),
    "afv_match_l2_pairs_device": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _i, _f, _f, _vp, _vp, _vp]),
    "afv_match_projection": (_i, [_vp, C.POINTER(ProjJob), _i, _vp, _vp]),
    "afv_match_fuse": (_i, [_vp, C.POINTER(ProjJob), _i, _vp, _vp]),
    "afv_match_sim3": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "afv_match_initialization": (_i, [_vp, _vp, _i, _vp, _vp]),
    "afv_vocab_create": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_vp)]),
    "afv_distinctive_descriptors": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "afv_distinctive_descriptors_f32": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp]),
    "afv_vocab_create_f32": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_vp)]),
    "afv_bow_transform_f32": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "afv_vocab_destroy": (None, [_vp, _vp]),
    "afv_bow_transform": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "afv_vocab_set_stopped": (_i, [_vp, _vp, _vp]),
    "afv_frame_create": (_i, [_vp, C.POINTER(FrameParams), C.POINTER(_vp)]),
    "afv_frame_destroy": (None, [_vp]),
    "afv_frame_extract": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, C.POINTER(_i)]),
    "afv_frame_set_features": (_i, [_vp, _vp, _vp, _i, _vp, _vp]),
    "afv_frame_set_undistorted": (_i, [_vp, _vp, _vp]),
    "afv_frame_count": (_i, [_vp]),
    "afv_frame_device_ptrs": (_i, [_vp] + [C.POINTER(_vp)] * 7),
    "afv_frame_get_grid": (_i, [_vp, _vp, _vp]),
    "afv_frame_bow_transform": (_i, [_vp, _vp, _i, _vp, _vp, C.POINTER(C.c_int32)]),
    "afv_frame_get_featvec": (_i, [_vp, _vp, _vp, _vp]),
    "afv_frame_match_projection": (_i, [_vp, C.POINTER(ProjQueries), _vp, _vp]),
    "afv_frame_match_fuse": (_i, [_vp, C.POINTER(ProjQueries), _i, _vp, _vp]),
    "afv_frame_match_initialization": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _i, _vp, _vp]),
    "afv_pyramid_level_sizes": (_i, [_vp, _i, _i, C.POINTER(C.c_int32), _vp, _vp]),
    "afv_frame_set_pyramid": (_i, [_vp, _i, _i, C.POINTER(_vp), _i]),
    "afv_frame_get_pyramid_level": (_i, [_vp, _i, _vp]),
    "afv_frame_stereo_match": (_i, [_vp, _vp, C.POINTER(StereoParams), C.POINTER(C.c_int32)]),
    "afv_frame_set_depth": (_i, [_vp, _vp, _i, _i, _i, _f]),
    "afv_frame_get_stereo": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "afv_table_set_from_frame": (_i, [_vp, _i, _vp]),
    "afv_table_match_bow_frame_h": (_i, [_vp, _vp, _i, _vp, _f, _f, _i, _vp, _vp]),
    "afv_set_projection_resolve": (_i, [_vp, _i]),
    "afv_points_create": (_i, [_vp, _i, _i, _i, C.POINTER(_vp)]),
    "afv_points_destroy": (None, [_vp]),
    "afv_points_set": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "afv_points_set_flags": (_i, [_vp, _vp, _i, _vp, _vp]),
    "afv_points_set_descriptors": (_i, [_vp, _vp, _i, _vp]),
    "afv_points_set_descriptors_from_table": (_i, [_vp, _vp, _i, _vp, _vp, _vp]),
    "afv_points_get": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "afv_frame_set_pose": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _f, _f]),
    "afv_frame_search_points": (_i, [_vp, C.POINTER(PointSearch), _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "afv_frame_fuse_points": (_i, [_vp, C.POINTER(PointSearch), _i, _vp, _vp]),
    "afv_frame_project_points": (_i, [_vp, C.POINTER(PointSearch), C.POINTER(PointProjection)]),
    "afv_frame_pose_optimize": (_i, [_vp, _vp, C.POINTER(PoseJob), _i, C.POINTER(PoseResult)]),
    "afv_table_set_scale": (_i, [_vp, _i, _vp, _vp, _vp, _vp]),
    "afv_table_triangulate": (_i, [_vp, _vp, _vp, C.POINTER(TriPointsJob), _i, _vp, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "afv_table_create_new_points": (_i, [_vp, C.c_int32, _vp, _i, C.POINTER(TableTriJob), C.POINTER(TriPointsJob), _vp, _vp, _vp, C.c_int32,
                                         _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "afv_table_sim3_hypotheses": (_i, [_vp, _vp, _vp, _vp, C.POINTER(Sim3Job), _i, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp]),
    "afv_table_optimize_sim3": (_i, [_vp, _vp, _vp, _vp, C.POINTER(Sim3OptJob), _i, _vp, _vp, _vp, C.POINTER(Sim3OptResult), _vp]),
    "afv_table_bundle_adjust": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(LbaCam), _vp, _i, _vp, _vp, _vp, _i, C.POINTER(LbaParams), _vp,
                                     C.POINTER(LbaResult), _vp, _vp, _vp]),
    "afv_table_global_bundle_adjust": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(LbaCam), _vp, _i, _vp, _vp, _vp, _i, C.POINTER(LbaParams), _vp,
                                            C.POINTER(LbaResult), _vp, _vp, _vp]),
    "afv_gba_plan_probe": (_i, [_i, _i, _vp, _vp, _i, C.c_longlong, _vp]),
    "afv_points_correct_se3": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "afv_table_refresh_points": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, C.POINTER(RefreshParams),
                                      C.POINTER(RefreshOut)]),
    "afv_table_set_inf": (_i, [_vp, _i, _vp]),
    "afv_table_set_camera": (_i, [_vp, C.POINTER(TableCamera)]),
    "afv_table_set_pose": (_i, [_vp, _i, _vp, _vp, _vp, _f, _f, _f, _f, _f]),
    "afv_table_set_map_points": (_i, [_vp, _i, _vp]),
    "afv_table_get_map_points": (_i, [_vp, _i, _vp]),
    "afv_table_fuse_points": (_i, [_vp, _vp, C.POINTER(TableFuseJob), _i, _vp, _vp, _vp, _vp]),
    "afv_essential_graph": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i, C.POINTER(EssParams), _vp, _vp, _i, C.POINTER(EssResult), _vp, _vp, _vp,
                                 _vp]),
    "afv_points_correct_sim3": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp]),
    "afv_frame_initializer": (_i, [_vp, _vp, C.POINTER(InitJob), _vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _vp, _vp, _vp, _vp,
                                   C.POINTER(InitTrace), _vp, _vp, _vp, _vp, _i]),
    "afv_frame_pnp_hypotheses": (_i, [_vp, _vp, C.POINTER(PnpJob), _i, _vp, _i, _i] + [_vp] * 13),
    "afv_vocab_set_weights": (_i, [_vp, _vp, _vp, _vp]),
    "afv_bow_vector": (_i, [_vp, _vp, _vp, _i, _vp, _vp, C.POINTER(C.c_int32)]),
    "afv_frame_get_bowvec": (_i, [_vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "afv_table_set_bowvec": (_i, [_vp, _i, _vp, _vp, _i]),
    "afv_table_score_bow": (_i, [_vp, C.POINTER(BowQuery), _i, _vp, _vp, _vp, _vp]),
    "afv_vocab_train": (_i, [_vp, C.POINTER(VocabTrainParams), _vp, C.c_int64, _vp, _i, C.POINTER(_vp)]),
    "afv_vocab_train_device": (_i, [_vp, C.POINTER(VocabTrainParams), _vp, _sz, C.c_int64, _vp, _i, C.POINTER(_vp)]),
    "afv_vocab_tree_nnodes": (_i, [_vp]),
    "afv_vocab_tree_get": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "afv_vocab_tree_stats": (_i, [_vp, _vp, _vp, _vp, C.POINTER(C.c_int32)]),
    "afv_vocab_tree_destroy": (None, [_vp]),
    "afv_hamming256": (_i, [_vp, _vp]),
    # include/afv_akaze.h
    "afv_akaze_default_params": (None, [_vp]),
    "afv_akaze_create": (_i, [_i, _vp, C.POINTER(_vp)]),
    "afv_akaze_destroy": (None, [_vp]),
    "afv_akaze_last_error": (C.c_char_p, [_vp]),
    "afv_akaze_plan_for": (_i, [_vp, _i, _i, _vp]),
    "afv_akaze_scale_space": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_size_t]),
    "afv_akaze_scale_space_device": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_size_t]),
    "afv_akaze_synchronize": (_i, [_vp]),
    "afv_akaze_get_plane": (_i, [_vp, _i, _i, _i, _vp]),
    "afv_akaze_get_kcontrast": (_i, [_vp, _i, _vp]),
    "afv_akaze_detect": (_i, [_vp]),
    "afv_akaze_get_keypoints": (_i, [_vp, _i, _vp, _i, _vp]),
    "afv_akaze_get_candidates": (_i, [_vp, _i, _i, _vp, _i, _vp]),
    "afv_akaze_describe": (_i, [_vp]),
    "afv_akaze_get_features": (_i, [_vp, _i, _vp, _vp, _i, _vp]),
    "afv_akaze_extract": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_size_t, _vp, _vp, _i, _vp]),
    "afv_akaze_extract_device": (_i, [_vp, _vp, _i, _i, _i, _i, C.c_size_t]),
    "afv_akaze_get_quotas": (_i, [_vp, _vp]),
    "afv_akaze_set_step_by_step": (_i, [_vp, _i]),
    "afv_akaze_set_suppress_engine": (_i, [_vp, _i, _i]),
    "afv_akaze_debug_neighbour_cap": (_i, [_vp, _i]),
    "afv_akaze_profile_enable": (_i, [_vp, _i]),
    "afv_akaze_profile_read": (_i, [_vp, _vp, _vp, _vp]),
    "afv_profile_enable": (_i, [_vp, _i]),
    "afv_profile_read": (_i, [_vp, _vp, _vp, _vp]),
    "afv_set_split_threshold": (_i, [_vp, _i]),
    "afv_set_split_chunks": (_i, [_vp, _i]),
    "afv_set_split_schedule": (_i, [_vp, _i]),
    "afv_set_match_engine": (_i, [_vp, _i]),
    "afv_set_small_batch_path": (_i, [_vp, _i, _i]),
    "afv_set_match_resolve": (_i, [_vp, _i]),
    "afv_set_l2_chunk_pairs": (_i, [_vp, _i]),
    "afv_debug_pyramid_plan": (_i, [C.POINTER(OrbParams), _i, _i, _i, _i, _vp, _i, _vp, _vp, _i]),
    "afv_debug_fast_tiles": (_i, [C.POINTER(OrbParams), _i, _i, _vp, _i, _vp, C.POINTER(_i)]),
    "afv_debug_describe_reach": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "afv_set_pipeline_chunk": (_i, [_vp, _i, _i]),
    "afv_get_geometry": (_i, [_vp, C.POINTER(Geometry)]),
    "afv_debug_get_level": (_i, [_vp, _i, _i, _vp]),
    "afv_debug_get_candidates": (_i, [_vp, _i, _i, _vp, _vp, _i, C.POINTER(_i)]),
    "afv_debug_get_selected": (_i, [_vp, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_i)]),
    "afv_debug_blur_level": (_i, [_vp, _i, _i, _vp]),
    "afv_debug_scratch_bytes": (_i, [_vp, _vp, _i]),
    "afv_debug_paint_scratch": (_i, [_vp, _i]),
    "afv_debug_rest_words": (_i, [_vp, C.POINTER(C.c_int32)]),
    "afv_debug_scratch_read": (_i, [_vp, _i, C.c_size_t, _vp, C.c_size_t]),
    "afv_num_stages": (_i, []),
}

_lib = None


def load():
    """dlopen libafv_hip.so and bind every declared symbol.  Raises if the HIP extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # Load order matters: PyTorch ships its own libamdhip64; if libafv_hip.so pulled in /opt/rocm's copy first, a
    # later `import torch` would bring a SECOND HIP runtime into the process and one of the two fails to see the
    # GPU.  Importing torch first makes libafv_hip.so bind to the runtime that is already loaded.
    try:
        import torch  # noqa: F401  (plumbing only: device memory, streams, torch.distributed)
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: build the HIP extension first (python __graft_entry__.py or "
                          "anyfeature-vslam_amd/build.py); there is no CPU fallback" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    # the profile getters write afv_num_stages() entries: a (variant) build with more stages than this mirror knows would overrun the
    # arrays the wrapper hands it
    if lib.afv_abi_version() != ABI_VERSION:
        raise ImportError("%s speaks ABI revision %d, this mirror %d" % (LIB_PATH, lib.afv_abi_version(), ABI_VERSION))
    if lib.afv_num_stages() > len(STAGES):
        raise ImportError("%s reports %d profile stages, this mirror knows %d" % (LIB_PATH, lib.afv_num_stages(), len(STAGES)))
    _lib = lib
    return lib


class AfvError(RuntimeError):
    def __init__(self, code, detail=""):
        self.code = code
        msg = load().afv_strerror(code).decode()
        super().__init__("afv error %d (%s)%s" % (code, msg, (": " + detail) if detail else ""))


def strerror(code):
    return load().afv_strerror(int(code)).decode()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def launch_ordered(ctx, device, stream, fn, tensors=()):
    """Call fn(hipStream_t) so that the work is ordered with torch's CURRENT stream.
    An explicit `stream` or a non-default torch stream is handed to the library as is.  torch reports its default stream
    as handle 0, which the C-ABI reads as "the context's own non-blocking stream" (not ordered with torch): in that case
    the context's stream is bridged with events through torch.cuda.ExternalStream: wait for torch's stream before, make
    torch's stream wait after."""
    if stream is not None:
        return fn(stream)
    import torch
    cur = torch.cuda.current_stream(device)
    if cur.cuda_stream:
        return fn(cur.cuda_stream)
    ext = getattr(ctx, "_ext_stream", None)
    if ext is None:
        ext = torch.cuda.ExternalStream(ctx.stream, device=device)
        ctx._ext_stream = ext
    ext.wait_stream(cur)
    rc = fn(None)
    cur.wait_stream(ext)
    # no tensor.record_stream(ext): everything torch does with these tensors later (including freeing and reusing their
    # memory) is enqueued on `cur` AFTER the wait above, and the allocator must never touch the context's stream — it is
    # destroyed with the context while cached blocks live on
    return rc
