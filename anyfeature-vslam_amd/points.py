"""Host-side mirror of the reference's MapPoint as far as the projection searches read it (include/MapPoint.h, src/MapPoint.cc): the
device-resident map-point store of the C-ABI (afv_points_*).

Per point id the store keeps XYZ, normalVector, minDistance / maxDistance (the raw members: the device applies 0.8f / 1.2f as the getters
do, MapPoint.cc:420-430), refSize / refDistance / refSigma, isBad(), NumberOfObservations() > 0 and the descriptor of
ComputeDistinctiveDescriptors.  LocalMapping writes it where it calls SetWorldPos / UpdateNormalAndDepth / ComputeDistinctiveDescriptors;
a resident Frame with a pose (Frame.set_pose) then searches it by point id (Frame.SearchLocalPoints and the like).
Plumbing only: every method is one C-ABI call.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr


class MapPoints:
    def __init__(self, ctx, capacity, desc_bytes=32, float_dim=0):
        """desc_bytes / float_dim: the kind of descriptor row, as for Frame"""
        self.ctx, self.lib = ctx, ctx.lib
        self.capacity = int(capacity)
        self.float_dim = int(float_dim)
        self.desc_bytes = 4 * self.float_dim if self.float_dim else int(desc_bytes)
        h = C.c_void_p()
        ctx.check(self.lib.afv_points_create(ctx.handle, self.capacity, int(desc_bytes), self.float_dim, C.byref(h)), "afv_points_create")
        self.handle = h

    def close(self):
        if getattr(self, "handle", None) and getattr(self.ctx, "handle", None):
            self.lib.afv_points_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _ids(ids):
        return np.ascontiguousarray(ids, np.int32).reshape(-1)

    def set(self, ids, pos=None, normal=None, min_distance=None, max_distance=None, ref_size=None, ref_distance=None, ref_sigma=None):
        """SetWorldPos / UpdateNormalAndDepth: pos, normal [n, 3]; the others [n]; None leaves the field as it is.  Marks the ids as set."""
        ids = self._ids(ids)
        n = len(ids)

        def f(a, cols):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float32).reshape(-1)
            if len(a) != n * cols:
                raise ValueError("an array of %d x %d floats is expected" % (n, cols))
            return a
        arrs = [f(pos, 3), f(normal, 3)] + [f(a, 1) for a in (min_distance, max_distance, ref_size, ref_distance, ref_sigma)]
        self.ctx.check(self.lib.afv_points_set(self.handle, ptr(ids), n, *[ptr(a) for a in arrs]), "afv_points_set")

    def set_flags(self, ids, bad=None, observed=None):
        """isBad() / NumberOfObservations() > 0 per id; None leaves the flag as it is"""
        ids = self._ids(ids)
        b = None if bad is None else np.ascontiguousarray(np.asarray(bad) != 0, np.uint8).reshape(-1)
        o = None if observed is None else np.ascontiguousarray(np.asarray(observed) != 0, np.uint8).reshape(-1)
        if (b is not None and len(b) != len(ids)) or (o is not None and len(o) != len(ids)):
            raise ValueError("one flag per id is expected")
        self.ctx.check(self.lib.afv_points_set_flags(self.handle, ptr(ids), len(ids), ptr(b), ptr(o)), "afv_points_set_flags")

    def _rows(self, rows, n):
        if self.float_dim:
            rows = np.ascontiguousarray(rows, np.float32).reshape(-1, self.float_dim)
        else:
            rows = np.ascontiguousarray(rows, np.uint8).reshape(-1, self.desc_bytes)
        if len(rows) != n:
            raise ValueError("one descriptor row per id is expected")
        return rows

    def set_descriptors(self, ids, rows):
        """ComputeDistinctiveDescriptors' result as host rows [n, desc_bytes] (float store: [n, float_dim] float32)"""
        ids = self._ids(ids)
        rows = self._rows(rows, len(ids))
        self.ctx.check(self.lib.afv_points_set_descriptors(self.handle, ptr(ids), len(ids), ptr(rows)), "afv_points_set_descriptors")

    def set_descriptors_from_table(self, ids, table, slots, idx):
        """... as rows (slot, feature index) of a keyframe table, copied device to device now"""
        ids = self._ids(ids)
        sl, ix = self._ids(slots), self._ids(idx)
        if len(sl) != len(ids) or len(ix) != len(ids):
            raise ValueError("one (slot, index) per id is expected")
        self.ctx.check(self.lib.afv_points_set_descriptors_from_table(self.handle, ptr(ids), len(ids), table.handle, ptr(sl), ptr(ix)),
                       "afv_points_set_descriptors_from_table")

    def correct_sim3(self, ids, pair_of_point, S_from, S_to):
        """The point correction of LoopClosing::CorrectLoop (LoopClosing.cc:487-516) in place: point ids[i] moves to
        float(S_to[q].map(S_from[q].map(double(P)))), q = pair_of_point[i] (-1: no pair).  S_from / S_to: m Sim3 as (R, t, s) or [m, 13]
        doubles.  Returns status [n] (_lib.POINT_MOVED / POINT_BAD_OR_UNSET / POINT_NO_PAIR)"""
        from .essgraph import sim3_records
        ids, pair = self._ids(ids), self._ids(pair_of_point)
        A, B = sim3_records(S_from), sim3_records(S_to)
        if len(pair) != len(ids) or len(A) != len(B):
            raise ValueError("one pair per id and as many S_to as S_from are expected")
        st = np.zeros(max(len(ids), 1), np.uint8)
        pad = lambda a: a if len(a) else np.zeros((4,) + a.shape[1:], a.dtype)
        self.ctx.check(self.lib.afv_points_correct_sim3(self.handle, ptr(pad(ids)), len(ids), ptr(pad(pair)), ptr(pad(A)), ptr(pad(B)), len(A), ptr(st)),
                       "afv_points_correct_sim3")
        return st[:len(ids)]

    def correct_se3(self, ids, pair_of_point, Tcw_before, Twc_after):
        """The point correction of LoopClosing::RunGlobalBundleAdjustment (LoopClosing.cc:731-750) for points the BA did not optimise, in
        place and IN FLOAT: point ids[i] moves to Rwc * (Rcw_bef * X + tcw_bef) + twc with q = pair_of_point[i] (-1: no pair).
        Tcw_before [m]: mTcwBefGBA of the reference keyframes; Twc_after [m]: their GetPoseInverse() after SetPose(TcwGBA) - nothing is
        inverted here.  Each as [m, 4, 4] / [m, 3, 4] matrices or [m, 12] (R row-major, then t), float32.  Returns status [n]
        (_lib.POINT_MOVED / POINT_BAD_OR_UNSET / POINT_NO_PAIR)"""
        def records(T):
            T = np.asarray(T, np.float32)
            if T.ndim == 3:
                T = np.concatenate([T[:, :3, :3].reshape(-1, 9), T[:, :3, 3]], 1)
            return np.ascontiguousarray(T.reshape(-1, 12))
        ids, pair = self._ids(ids), self._ids(pair_of_point)
        A, B = records(Tcw_before), records(Twc_after)
        if len(pair) != len(ids) or len(A) != len(B):
            raise ValueError("one pair per id and as many Twc_after as Tcw_before are expected")
        st = np.zeros(max(len(ids), 1), np.uint8)
        pad = lambda a: a if len(a) else np.zeros((4,) + a.shape[1:], a.dtype)
        self.ctx.check(self.lib.afv_points_correct_se3(self.handle, ptr(pad(ids)), len(ids), ptr(pad(pair)), ptr(pad(A)), ptr(pad(B)), len(A), ptr(st)),
                       "afv_points_correct_se3")
        return st[:len(ids)]

    def get(self, ids):
        """what the store holds for `ids` (tests): dict of pos, normal, min_distance, max_distance, ref_size, ref_distance, ref_sigma, flags
        (_lib.PTF_* bits), descriptors"""
        ids = self._ids(ids)
        n = len(ids)
        m = max(n, 1)
        out = {"pos": np.zeros((m, 3), np.float32), "normal": np.zeros((m, 3), np.float32)}
        for k in ("min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma"):
            out[k] = np.zeros(m, np.float32)
        out["flags"] = np.zeros(m, np.uint8)
        out["descriptors"] = np.zeros((m, self.float_dim), np.float32) if self.float_dim else np.zeros((m, self.desc_bytes), np.uint8)
        self.ctx.check(self.lib.afv_points_get(self.handle, ptr(ids), n, *[ptr(out[k]) for k in (
            "pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma", "flags", "descriptors")]), "afv_points_get")
        return {k: v[:n] for k, v in out.items()}
