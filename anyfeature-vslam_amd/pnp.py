"""Host-side mirror of the reference's PnPsolver (include/PnPsolver.h, src/PnPsolver.cc) as Tracking::Relocalization uses it
(src/Tracking.cc:1190-1216): one solver per candidate keyframe, iterated round-robin, five hypotheses at a time.

PnPsolver.batch makes ONE device call (afv_frame_pnp_hypotheses: the constructor of every solver, every EPnP RANSAC hypothesis of every
candidate and the Refine of every record, csrc/k_pnp.hip) and returns one PnPsolver per candidate.  iterate / find are host code over the
per-hypothesis counts, poses and inlier words: hypothesis h depends on (seed, h) alone and Refine reads only the best set, which changes
only at a record, so the reference's sequential rule is a scan.  The normative semantics, the quirks Q1-Q6 and the deviations E1-E10 are
tests/_pnp_ref.py's and include/afv_hip.h's ("PnPsolver").
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import PnpJob, ptr

INT_MAX = 2 ** 31 - 1


def pnp_jobs(seeds, min_inliers, epsilon, th2):
    """afv_pnp_job records, one per seed"""
    jobs = (PnpJob * max(len(seeds), 1))()
    for c, seed in enumerate(seeds):
        j = jobs[c]
        j.struct_size = C.sizeof(PnpJob)
        seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        j.seed_lo, j.seed_hi = seed & 0xFFFFFFFF, seed >> 32
        j.min_inliers, j.epsilon, j.th2 = int(min_inliers), float(epsilon), float(th2)
    return jobs


def hypotheses(frame, points, jobs, pts_rows, nhyp=300, mask_words=None, extras=False):
    """afv_frame_pnp_hypotheses as it is: pts rows [nc, NF] in, a dict of n / min_inliers [nc], index [nc, NF], count / degenerate / refined /
    refined_count [nc, nhyp], pose / refined_pose [nc, nhyp, 12], inliers / refined_inliers [nc, nhyp, mask_words] out; extras: max_err
    [nc, NF] and p3dw [nc, NF, 3] as well.  mask_words None: what the frame's feature count needs"""
    nf = frame.N
    pts = np.ascontiguousarray(pts_rows, np.int32)
    if pts.ndim == 1:
        pts = pts.reshape(1, -1)
    if pts.ndim != 2 or pts.shape[1] != nf:
        raise ValueError("PnPsolver: rows of %d point ids (the frame's features) are expected, got %s" % (nf, pts.shape))
    nc = pts.shape[0]
    if len(jobs) < nc:
        raise ValueError("PnPsolver: %d candidates need %d jobs" % (nc, nc))
    if mask_words is None:
        mask_words = (nf + 31) // 32
    nhyp, mask_words = int(nhyp), int(mask_words)
    ok_shape = 1 <= nhyp <= _lib.PNP_MAX_HYPOTHESES and 0 <= mask_words <= _lib.PNP_MAX_MASK_WORDS
    h, w = (nhyp, mask_words) if ok_shape else (1, 1)  # an absurd size is the library's to refuse: no array of that size is made for it
    m, cells = max(nc, 1), max(nf, 1)
    out = dict(n=np.zeros(m, np.int32), min_inliers=np.zeros(m, np.int32), index=np.full((m, cells), -1, np.int32),
               count=np.zeros((m, h), np.int32), degenerate=np.zeros((m, h), np.uint8), pose=np.zeros((m, h, 12), np.float32),
               inliers=np.zeros((m, h, w), np.uint32), refined=np.zeros((m, h), np.uint8), refined_count=np.zeros((m, h), np.int32),
               refined_pose=np.zeros((m, h, 12), np.float32), refined_inliers=np.zeros((m, h, w), np.uint32))
    if extras:
        out.update(max_err=np.zeros((m, cells), np.float32), p3dw=np.zeros((m, cells, 3), np.float32))
    frame.ctx.check(frame.lib.afv_frame_pnp_hypotheses(
        frame.handle, points.handle, jobs, nc, ptr(pts), nhyp, mask_words, ptr(out["n"]), ptr(out["min_inliers"]), ptr(out["index"]),
        ptr(out["count"]), ptr(out["degenerate"]), ptr(out["pose"]), ptr(out["inliers"]), ptr(out["refined"]), ptr(out["refined_count"]),
        ptr(out["refined_pose"]), ptr(out["refined_inliers"]), ptr(out.get("max_err")), ptr(out.get("p3dw"))), "afv_frame_pnp_hypotheses")
    return out


def min_inliers_rule(N, min_inliers, epsilon):
    """:134-139 with minSet = 4: the product in float, truncated (saturating)"""
    with np.errstate(over="ignore"):
        prod = np.float32(N) * np.float32(epsilon)
    n_min = INT_MAX if not prod < np.float32(2147483648.0) else int(prod)
    return max(n_min, int(min_inliers), 4)


def _Tcw(pose):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = np.asarray(pose[:9], np.float32).reshape(3, 3)
    T[:3, 3] = pose[9:12]
    return T


class PnPsolver:
    """the reference's interface over the device's answer for one candidate"""

    @classmethod
    def batch(cls, frame, points, pts_rows, seed=0, nhyp=300, minInliers=10, epsilon=0.5, th2=5.991, mask_words=None):
        """one device call for all candidates of a relocalisation (Tracking.cc:1190-1216 creates all solvers before it iterates any).
        frame: the resident current frame (features and a pose: the intrinsics are the frame's); points: the MapPoints store; pts_rows
        [nc, N]: vvpMapPointMatches of every candidate as point ids (what SearchByBoW(KF, F) answers, mapped to ids), -1 = none; seed: an
        int (candidate c draws from seed + c) or one per candidate; minInliers / epsilon / th2: what SetRansacParameters will be given
        (the defaults are Tracking's, include/Tracking.h:323-328).  Returns a list of PnPsolver."""
        rows = np.ascontiguousarray(pts_rows, np.int32)
        if rows.ndim == 1:
            rows = rows.reshape(1, -1)
        nc = rows.shape[0]
        seeds = [int(seed) + c for c in range(nc)] if np.ndim(seed) == 0 else [int(s) for s in seed]
        if len(seeds) != nc:
            raise ValueError("PnPsolver.batch: one seed per candidate is expected")
        out = hypotheses(frame, points, pnp_jobs(seeds, minInliers, epsilon, th2), rows, nhyp, mask_words)
        return [cls(int(out["n"][c]), int(out["min_inliers"][c]), out["index"][c], out["count"][c], out["degenerate"][c], out["pose"][c],
                    out["inliers"][c], out["refined"][c], out["refined_count"][c], out["refined_pose"][c], out["refined_inliers"][c],
                    rows.shape[1], (minInliers, epsilon, th2)) for c in range(nc)]

    def __init__(self, n, min_inliers, index, count, degenerate, pose, inliers, refined, refined_count, refined_pose, refined_inliers,
                 n_features, given):
        """n = N, min_inliers = the device's mRansacMinInliers, index = mvKeyPointIndices, the rest = the rows of one candidate, n_features =
        the frame's feature count, given = (minInliers, epsilon, th2) of the device call"""
        self.N, self.n_features = int(n), int(n_features)
        self.index, self.count, self.degenerate, self.pose, self.inliers = index, count, degenerate, pose, inliers
        self.refined, self.refined_count, self.refined_pose, self.refined_inliers = refined, refined_count, refined_pose, refined_inliers
        self.device_min_inliers = int(min_inliers)
        self.given = (int(given[0]), np.float32(given[1]), np.float32(given[2]))
        self.nhyp = len(count)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = None       # the hypothesis mBestTcw / mvbBestInliers come from: the current record
        self.SetRansacParameters(maxIterations=min(300, self.nhyp), minInliers=self.given[0], epsilon=self.given[1], th2=self.given[2])

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        """:121-157 (Q2): host mathematics only.  minInliers, epsilon and th2 must be what the device call was given and minSet 4;
        maxIterations beyond the evaluated hypotheses raises"""
        if (int(minInliers), np.float32(epsilon), np.float32(th2)) != self.given:
            raise ValueError("PnPsolver: minInliers, epsilon and th2 must be what the device call was given: %r" % (self.given,))
        if minSet != 4:
            raise ValueError("PnPsolver: minSet must be 4")
        if maxIterations > self.nhyp:
            raise ValueError("PnPsolver: maxIterations %d exceeds the %d hypotheses the device evaluated" % (maxIterations, self.nhyp))
        n_min = min_inliers_rule(self.N, minInliers, epsilon)
        if n_min != self.device_min_inliers:
            raise ValueError("PnPsolver: the device's mRansacMinInliers %d is not the host's %d" % (self.device_min_inliers, n_min))
        self.mRansacProb, self.mRansacMinInliers = float(probability), n_min
        eps = np.float32(epsilon)
        with np.errstate(all="ignore"):
            ratio = np.float32(n_min) / np.float32(self.N)
        if eps < ratio:
            eps = ratio
        self.mRansacEpsilon = eps
        if n_min == self.N:
            n_it = 1
        else:
            e3 = float(eps) ** 3 if math.isfinite(float(eps)) else float("inf")
            arg = 1.0 - e3
            den = math.log(arg) if arg > 0 else (float("-inf") if arg == 0 else float("nan"))
            num = math.log(1.0 - self.mRansacProb) if self.mRansacProb < 1 else float("-inf")
            if den == 0:
                v = float("nan") if num == 0 or num != num else math.copysign(float("inf"), -num)
            else:
                v = num / den
            # a double outside int's range is undefined in the reference: here it saturates and a NaN reads maxIterations
            n_it = int(maxIterations) if math.isnan(v) else int(min(max(math.ceil(v) if math.isfinite(v) else v, -2 ** 31), INT_MAX))
        self.nIterations = n_it
        self.mRansacMaxIts = max(1, min(n_it, int(maxIterations)))

    def _vb(self, words):
        """mvbInliersi as vbInliers over the frame's features"""
        k = np.arange(self.N)
        flags = ((words[k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool) if self.N else np.zeros(0, bool)
        vb = np.zeros(self.n_features, bool)
        vb[self.index[:self.N][flags]] = True
        return vb

    def iterate(self, nIterations):
        """:165-258 -> (Tcw [4, 4] float32 or None, bNoMore, vbInliers [frame N] bool, nInliers).  A scan that would visit a hypothesis the
        device did not evaluate raises"""
        none = np.zeros(self.n_features, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, none, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:   # Q1
            h = self.mnIterations
            if h >= self.nhyp:
                raise IndexError("PnPsolver: hypothesis %d was not evaluated (nhyp = %d)" % (h, self.nhyp))
            cur += 1
            self.mnIterations += 1
            c = int(self.count[h])     # a degenerate hypothesis counts 0 and still advances mnIterations
            if c >= self.mRansacMinInliers:
                if c > self.mnBestInliers:   # a record
                    self.mnBestInliers = c
                    self.best = h
                b = self.best              # Q4: Refine on the best set so far; the device evaluated it at the record
                if int(self.refined[b]) == 1 and int(self.refined_count[b]) > self.mRansacMinInliers:
                    return _Tcw(self.refined_pose[b]), False, self._vb(self.refined_inliers[b]), int(self.refined_count[b])
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:   # Q3: the unrefined best
                return _Tcw(self.pose[self.best]), True, self._vb(self.inliers[self.best]), self.mnBestInliers
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        """:159-163 -> (Tcw or None, vbInliers, nInliers)"""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
