"""Optimizer::LocalBundleAdjustment (src/Optimizer.cc:450-768) and Optimizer::BundleAdjustment (:61-243) over slots of the keyframe table
and ids of the map-point store: afv_table_bundle_adjust (csrc/k_lba.hip).  Normative semantics, the quirk L-Q1 and the deviations L1-L9:
tests/_lba_ref.py and include/afv_hip.h ("Bundle adjustment").

What stays with the host's map after a call: EraseMapPointMatch / EraseObservation for every pair in to_erase and SetPose from the
returned poses.  UpdateNormalAndDepth of the moved points is refresh.RefreshAfterBundleAdjustment, on the device, over the same observations.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LbaCam, LbaParams, LbaResult, ptr


def lba_cams(cams):
    """afv_lba_cam records from camera dicts {Rcw, tcw, fx, fy, cx, cy[, mbf]}"""
    out = (LbaCam * max(len(cams), 1))()
    for k, cam in enumerate(cams):
        c = out[k]
        c.struct_size = C.sizeof(LbaCam)
        R, t = np.asarray(cam["Rcw"], np.float32).reshape(9), np.asarray(cam["tcw"], np.float32).reshape(3)
        for q in range(9):
            c.Rcw[q] = float(R[q])
        for q in range(3):
            c.tcw[q] = float(t[q])
        for key in ("fx", "fy", "cx", "cy"):
            setattr(c, key, float(np.float32(cam[key])))
        c.bf = float(np.float32(cam.get("mbf", cam.get("bf", 0.0))))
    return out


def edge_arrays(point_ids, kf_slots, observations):
    """observations [(point id, keyframe slot, feature index), ...] -> (obs_point, obs_kf, obs_idx, order): the edges grouped by point in
    the order of point_ids (a stable sort: the observations of a point keep their order); order[e] = the observation edge e came from"""
    where_p = {int(p): i for i, p in enumerate(point_ids)}
    where_k = {int(s): i for i, s in enumerate(kf_slots)}
    if len(where_p) != len(point_ids) or len(where_k) != len(kf_slots):
        raise ValueError("bundle adjustment: a point id or a keyframe slot is named twice")
    try:
        pk = np.array([(where_p[int(p)], where_k[int(k)], int(i)) for p, k, i in observations], np.int32).reshape(-1, 3)
    except KeyError as e:
        raise ValueError("bundle adjustment: an observation names point / keyframe %s, which is not in the problem" % e)
    order = np.argsort(pk[:, 0], kind="stable")
    pk = pk[order]
    return (np.ascontiguousarray(pk[:, 0]), np.ascontiguousarray(pk[:, 1]), np.ascontiguousarray(pk[:, 2]), order)


def bundle_adjust(table, points, slots, n_free, cams, point_ids, obs_point, obs_kf, obs_idx, iterations, robust, checks, write_points=True,
                  trial_budget=0, stop=None, entry="afv_table_bundle_adjust"):
    """afv_table_bundle_adjust (or, with entry="afv_table_global_bundle_adjust", the block-sparse route with its own caps) as it is.  stop: None, or a ctypes.c_int32 the caller (another thread) raises.  Returns (result: LbaResult,
    kf [n_free, 12] float64, xyz [np, 3] float64, edge_state [ne] uint8)"""
    slots, point_ids = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (slots, point_ids))
    obs_point, obs_kf, obs_idx = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (obs_point, obs_kf, obs_idx))
    nk, npts, ne = len(slots), len(point_ids), len(obs_point)
    if len(obs_kf) != ne or len(obs_idx) != ne or len(cams) < nk:
        raise ValueError("bundle adjustment: the edge arrays / camera records do not match the counts")
    prm = LbaParams()
    prm.struct_size = C.sizeof(LbaParams)
    for r in range(2):
        prm.iterations[r], prm.robust[r] = int(iterations[r]), int(bool(robust[r]))
    prm.checks, prm.write_points, prm.trial_budget = int(bool(checks)), int(bool(write_points)), int(trial_budget)
    res = LbaResult()
    kf, xyz, state = np.zeros((max(n_free, 1), 12), np.float64), np.zeros((max(npts, 1), 3), np.float64), np.zeros(max(ne, 1), np.uint8)
    pad = lambda a: a if len(a) else np.zeros(1, np.int32)
    table.ctx.check(getattr(table.lib, entry)(table.handle, points.handle, ptr(pad(slots)), nk, int(n_free), cams, ptr(pad(point_ids)), npts,
                                             ptr(pad(obs_point)), ptr(pad(obs_kf)), ptr(pad(obs_idx)), ne, C.byref(prm),
                                             None if stop is None else C.byref(stop), C.byref(res), ptr(kf), ptr(xyz), ptr(state)), entry)
    return res, kf[:n_free], xyz[:npts], state[:ne]


def _trace(res):
    return dict(iterations=list(res.iterations), trials=list(res.trials), chi2=list(res.chi2), lam=list(res.lam), n_edges=res.n_edges,
                n_removed_first=res.n_removed_first, n_erase=res.n_erase, stopped=res.stopped)


def _run(table, points, kfs, fixed_flags, cams, point_ids, observations, iterations, robust, checks, write_points, stop,
         entry="afv_table_bundle_adjust"):
    kfs = [int(s) for s in kfs]
    free = [s for s, f in zip(kfs, fixed_flags) if not f]
    order_kf = free + [s for s, f in zip(kfs, fixed_flags) if f]
    op, ok, oi, order = edge_arrays(point_ids, order_kf, observations)
    recs = lba_cams([cams[s] for s in order_kf])
    res, kf, xyz, state = bundle_adjust(table, points, order_kf, len(free), recs, point_ids, op, ok, oi, iterations, robust, checks, write_points, 0, stop, entry)
    poses = {s: (kf[i, :9].reshape(3, 3).copy(), kf[i, 9:].copy()) for i, s in enumerate(free)} if res.stopped != 1 else {}
    st = np.zeros(len(order), np.uint8)
    st[order] = state
    return res, poses, xyz, st


def LocalBundleAdjustment(table, points, local, fixed, cams, point_ids, observations, stop=None):
    """Optimizer::LocalBundleAdjustment in one call.  local: [(slot, is_fixed), ...] or slots - lLocalKeyFrames, the entry with keyId == 0
    flagged fixed; fixed: the slots of lFixedCameras; cams: {slot: {Rcw, tcw, fx, fy, cx, cy, mbf}}; point_ids: lLocalMapPoints as store
    ids; observations: [(point id, slot, feature index), ...] in the reference's order.  Returns (poses {slot: (Rcw [3, 3], tcw [3])
    float64} of the optimised keyframes, xyz [np, 3] float64 (the store already holds the float cast), to_erase [(slot, point id), ...] =
    vToErase, trace).  A stop flag raised before the call: ({}, None, [], trace) and nothing was written."""
    entries = [(e, False) if np.isscalar(e) else (e[0], bool(e[1])) for e in local] + [(s, True) for s in fixed]
    res, poses, xyz, st = _run(table, points, [e[0] for e in entries], [e[1] for e in entries], cams, point_ids, observations, (5, 10), (1, 0), 1, True, stop)
    trace = _trace(res)
    trace["edge_state"] = st
    if res.stopped == 1:
        return {}, None, [], trace
    erase = [(int(observations[i][1]), int(observations[i][0])) for i in np.nonzero(st == _lib.LBA_EDGE_ERASE)[0]]
    return poses, xyz, erase, trace


def BundleAdjustment(table, points, kfs, cams, point_ids, observations, nIterations=5, robust=True, stop=None, write_points=True):
    """Optimizer::BundleAdjustment: kfs [(slot, is_fixed), ...] (keyId == 0 flagged fixed); write_points=False is the nLoopKF != 0 path (the
    caller keeps xyz as mPosGBA, the store stays).  Returns (poses, xyz, trace)."""
    entries = [(e, False) if np.isscalar(e) else (e[0], bool(e[1])) for e in kfs]
    res, poses, xyz, st = _run(table, points, [e[0] for e in entries], [e[1] for e in entries], cams, point_ids, observations, (nIterations, 0),
                               (robust, 0), 0, write_points, stop)
    trace = _trace(res)
    trace["edge_state"] = st
    return poses, xyz, trace


def GlobalBundleAdjustment(table, points, kfs, cams, point_ids, observations, nIterations=5, robust=True, stop=None, write_points=True):
    """Optimizer::GlobalBundleAdjustemnt (Optimizer.cc:53-58; the defaults are Optimizer.h:42-43) over the whole map, on the block-sparse
    route (afv_table_global_bundle_adjust: up to _lib.GBA_MAX_KF keyframes, deviation L7' of include/afv_hip.h).  The arguments and the
    answer are BundleAdjustment's: kfs [(slot, is_fixed), ...] with keyId == 0 flagged fixed.  LoopClosing::RunGlobalBundleAdjustment
    passes nIterations=10, robust=False, write_points=False and keeps xyz as mPosGBA; the points the BA did not optimise are then moved
    by MapPoints.correct_se3.  Returns (poses, xyz, trace)."""
    entries = [(e, False) if np.isscalar(e) else (e[0], bool(e[1])) for e in kfs]
    res, poses, xyz, st = _run(table, points, [e[0] for e in entries], [e[1] for e in entries], cams, point_ids, observations, (nIterations, 0),
                               (robust, 0), 0, write_points, stop, "afv_table_global_bundle_adjust")
    trace = _trace(res)
    trace["edge_state"] = st
    return poses, xyz, trace
