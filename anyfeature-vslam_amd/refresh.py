"""MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:279-349) and MapPoint::UpdateNormalAndDepth (:372-418) for a batch of resident
map points: afv_table_refresh_points (csrc/k_refresh.hip).  Normative semantics and the deviations R1-R3: tests/_refresh_ref.py and
include/afv_hip.h ("Refresh of resident map points").

The observations are those of the bundle adjustment (lba.edge_arrays): a caller that has just run LocalBundleAdjustment passes the same
list again.  What stays with the host's map after a call: refKeyframe / refIndex of every point, from best_obs.
"""
import ctypes as C

import numpy as np

from . import _lib, matcher
from ._lib import RefreshOut, RefreshParams, ptr
from .lba import edge_arrays
from .table import DescriptorTable


def camera_centre(Rcw, tcw):
    """twc = -Rwc * tcw as KeyFrame::SetPose computes it (src/KeyFrame.cc:81-84), in float32 from the float32 casts of Rcw and tcw: the
    rule of Frame.set_pose for Ow.  (GetCameraCenter returns twc; Cw, the stereo centre, is another member.)"""
    R, t = np.asarray(Rcw, np.float32).reshape(3, 3), np.asarray(tcw, np.float32).reshape(3)
    return np.array([-R[0, k] * t[0] + (-R[1, k] * t[1] + -R[2, k] * t[2]) for k in range(3)], np.float32)


def refresh_points(table, points, slots, centres, max_size, kf_bad, point_ids, ref_kf, obs_point, obs_kf, obs_idx, descriptors=True, normals=True):
    """afv_table_refresh_points as it is.  Returns (status [np] int32, best_obs [np] int32: an index into the obs arrays | -1, best_median
    [np]: int32 for a binary table, float32 for a float table)"""
    slots, point_ids, ref_kf = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (slots, point_ids, ref_kf))
    obs_point, obs_kf, obs_idx = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (obs_point, obs_kf, obs_idx))
    centres, max_size = np.ascontiguousarray(centres, np.float32).reshape(-1), np.ascontiguousarray(max_size, np.float32).reshape(-1)
    nk, npts, ne = len(slots), len(point_ids), len(obs_point)
    if len(obs_kf) != ne or len(obs_idx) != ne or len(ref_kf) != npts or len(centres) != 3 * nk or len(max_size) != nk:
        raise ValueError("refresh: the observation / keyframe / point arrays do not match the counts")
    bad = None
    if kf_bad is not None:
        bad = np.ascontiguousarray(np.asarray(kf_bad) != 0, np.uint8).reshape(-1)
        if len(bad) != nk:
            raise ValueError("refresh: one bad flag per keyframe is expected")
    prm = _lib.sized(RefreshParams)
    prm.descriptors, prm.normals = int(bool(descriptors)), int(bool(normals))
    status, best, med = (np.zeros(max(npts, 1), np.int32) for _ in range(3))
    out = _lib.sized(RefreshOut)
    out.status, out.best_obs, out.best_median = (a.ctypes.data for a in (status, best, med))
    pad = lambda a, dt=np.int32: a if len(a) else np.zeros(1, dt)
    table.ctx.check(table.lib.afv_table_refresh_points(table.handle, points.handle, ptr(pad(slots)), nk, ptr(pad(centres, np.float32)),
                                                       ptr(pad(max_size, np.float32)), ptr(bad), ptr(pad(point_ids)), npts, ptr(pad(ref_kf)),
                                                       ptr(pad(obs_point)), ptr(pad(obs_kf)), ptr(pad(obs_idx)), ne, C.byref(prm), C.byref(out)),
                    "afv_table_refresh_points")
    med = med[:npts]
    return status[:npts], best[:npts], med.view(np.float32) if table.float_dim else med


def RefreshMapPoints(table, points, kfs, centres, max_size, point_ids, ref_kf, observations, kf_bad=None, descriptors=True, normals=True):
    """Both routines for point_ids in one call.  kfs: the slots of every keyframe an observation names; centres {slot: GetCameraCenter()},
    max_size {slot: maxKeyPtSize}, kf_bad: the slots whose keyframe isBad() (None: none); ref_kf {point id: slot of mpRefKF} (a point
    without an entry: -1); observations [(point id, slot, feature index), ...] in the reference's order, as LocalBundleAdjustment takes
    them.  Returns (status [np], best_obs [np]: the index into `observations` of the winning row | -1, best_median [np])."""
    kfs = [int(s) for s in kfs]
    point_ids = [int(p) for p in point_ids]
    op, ok, oi, order = edge_arrays(point_ids, kfs, observations)
    where_k = {s: i for i, s in enumerate(kfs)}
    cen = np.array([np.asarray(centres[s], np.float32).reshape(3) for s in kfs], np.float32).reshape(-1)
    mx = np.array([max_size[s] for s in kfs], np.float32)
    bad_slots = set() if kf_bad is None else set(int(b) for b in kf_bad)
    bad = None if kf_bad is None else np.array([s in bad_slots for s in kfs], np.uint8)
    ref = np.array([where_k.get(ref_kf.get(p, -1), -1) for p in point_ids], np.int32)
    status, best, med = refresh_points(table, points, kfs, cen, mx, bad, point_ids, ref, op, ok, oi, descriptors, normals)
    if len(order):
        best = np.where(best >= 0, order[np.maximum(best, 0)], -1).astype(np.int32)
    return status, best, med


def UpdateNormalAndDepth(table, points, kfs, centres, max_size, point_ids, ref_kf, observations):
    """MapPoint::UpdateNormalAndDepth of point_ids: RefreshMapPoints, the normal part alone.  Returns status [np]"""
    return RefreshMapPoints(table, points, kfs, centres, max_size, point_ids, ref_kf, observations, None, False, True)[0]


def ComputeDistinctiveDescriptors(table, *args, **kw):
    """MapPoint::ComputeDistinctiveDescriptors of resident points: (table, points, kfs, point_ids, observations, kf_bad=None) ->
    (status, best_obs, best_median), RefreshMapPoints with the descriptor part alone.  With a Context in front - (ctx, descriptor_sets) -
    it is the form over host rows (matcher.ComputeDistinctiveDescriptors)."""
    if not isinstance(table, DescriptorTable):
        return matcher.ComputeDistinctiveDescriptors(table, *args, **kw)
    return _distinctive_resident(table, *args, **kw)


def _distinctive_resident(table, points, kfs, point_ids, observations, kf_bad=None):
    zero3, one = np.zeros(3, np.float32), np.float32(1.0)
    return RefreshMapPoints(table, points, kfs, {int(s): zero3 for s in kfs}, {int(s): one for s in kfs}, point_ids, {}, observations, kf_bad, True, False)


def RefreshAfterBundleAdjustment(table, points, poses, fixed_cams, max_size, point_ids, ref_kf, observations, kf_bad=None, descriptors=False,
                                 normals=True):
    """What Optimizer::LocalBundleAdjustment does after its write-back (Optimizer.cc:753-767): poses is the first answer of
    lba.LocalBundleAdjustment / BundleAdjustment, {slot: (Rcw, tcw) float64} of the optimised keyframes; fixed_cams {slot: {Rcw, tcw, ...}}
    the cameras that did not move.  The centres are formed in float32 from the float32 casts of the poses, as KeyFrame::SetPose does after
    Converter::toMatrix4f; then RefreshMapPoints runs over the observations the adjustment was given."""
    centres = {int(s): camera_centre(R, t) for s, (R, t) in poses.items()}
    for s, cam in fixed_cams.items():
        if int(s) not in centres:
            centres[int(s)] = camera_centre(cam["Rcw"], cam["tcw"])
    return RefreshMapPoints(table, points, list(centres), centres, max_size, point_ids, ref_kf, observations, kf_bad, descriptors, normals)
