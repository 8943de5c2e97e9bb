"""Host-side mirror of the reference's Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc) as LoopClosing::ComputeSim3 uses it
(src/LoopClosing.cc:247-416): one solver per candidate keyframe, iterated round-robin.

Sim3Solver.batch makes ONE device call (afv_table_sim3_hypotheses: the constructor of every solver and every RANSAC hypothesis of every
candidate, csrc/k_sim3.hip) and returns one Sim3Solver per candidate.  iterate / find are host code over the per-hypothesis counts,
transforms and inlier words: hypothesis h depends on (seed, h) alone, so the reference's sequential rule (running best, return on
> minInliers) is a scan.  The normative semantics, the quirks Q1-Q3 and the deviations S1-S6 are tests/_sim3_ref.py's and
include/afv_hip.h's ("Sim3Solver").

OptimizeSim3 / OptimizeSim3Batch are Optimizer::OptimizeSim3 (src/Optimizer.cc:1033-1226) as LoopClosing::ComputeSim3 calls it after a
solver found a transform (src/LoopClosing.cc:342): ONE device call (afv_table_optimize_sim3, csrc/k_sim3opt.hip) refines the Sim3 of every
candidate.  Normative semantics and the deviations O1-O7: tests/_sim3opt_ref.py and include/afv_hip.h ("OptimizeSim3").
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import Sim3Job, Sim3OptJob, Sim3OptResult, ptr


def _rows(a, nc, cap, what, broadcast=False):
    """host rows as a contiguous (nc, cap) int32 array: shorter rows are padded with -1, one row is repeated when `broadcast`"""
    a = np.asarray(a, np.int32)
    if a.ndim == 1 and broadcast:
        a = np.broadcast_to(a, (nc, a.shape[0]))
    if a.ndim != 2 or a.shape[0] != nc or a.shape[1] > cap:
        raise ValueError("%s: rows of shape (%d, <= %d) are expected, got %s" % (what, nc, cap, a.shape))
    out = np.full((nc, cap), -1, np.int32)
    out[:, :a.shape[1]] = a
    return out


def sim3_jobs(cam_cur, cams_cand, fix_scale, seeds):
    """afv_sim3_job records from camera dicts {Rcw, tcw, fx, fy, cx, cy}: 1 = the current keyframe, 2 = candidate c"""
    jobs = (Sim3Job * len(cams_cand))()
    for c, cam2 in enumerate(cams_cand):
        j = jobs[c]
        j.struct_size = C.sizeof(Sim3Job)
        j.fix_scale = 1 if fix_scale else 0
        seed = int(seeds[c]) & 0xFFFFFFFFFFFFFFFF
        j.seed_lo, j.seed_hi = seed & 0xFFFFFFFF, seed >> 32
        for side, cam in (("1", cam_cur), ("2", cam2)):
            for name, cnt in (("Rcw", 9), ("tcw", 3)):
                v = np.asarray(cam[name], np.float32).reshape(cnt)
                dst = getattr(j, name + side)
                for k in range(cnt):
                    dst[k] = float(v[k])
            for key in ("fx", "fy", "cx", "cy"):
                setattr(j, key + side, float(np.float32(cam[key])))
    return jobs


def hypotheses(table, points, slot_a, slot_b, jobs, mp1, mp2, idx2, idx1=None, nhyp=300, mask_words=None, extras=False):
    """afv_table_sim3_hypotheses as it is: rows [nc, cap] in, a dict of n [nc], index1 [nc, cap], count / degenerate [nc, nhyp], sim3
    [nc, nhyp, 13], inliers [nc, nhyp, mask_words] out; extras: x3dc1 / x3dc2 [nc, cap, 3] and max_err [nc, cap, 2] as well.
    mask_words None: what the table's capacity needs"""
    sa, sb = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (slot_a, slot_b))
    nc, cap = len(sa), table.cap
    if len(sb) != nc or len(jobs) != nc:
        raise ValueError("Sim3Solver: %d candidates need %d slots and jobs" % (nc, nc))
    mp1, mp2, idx2 = _rows(mp1, nc, cap, "mp1", True), _rows(mp2, nc, cap, "mp2"), _rows(idx2, nc, cap, "idx2")
    idx1 = None if idx1 is None else _rows(idx1, nc, cap, "idx1", True)
    if mask_words is None:
        mask_words = (cap + 31) // 32
    nhyp, mask_words = int(nhyp), int(mask_words)
    ok_shape = 1 <= nhyp <= _lib.SIM3_MAX_HYPOTHESES and 0 <= mask_words <= _lib.SIM3_MAX_MASK_WORDS
    h, w = (nhyp, mask_words) if ok_shape else (1, 1)  # an absurd size is the library's to refuse: no array of that size is made for it
    out = dict(n=np.zeros(nc, np.int32), index1=np.full((nc, cap), -1, np.int32), count=np.zeros((nc, h), np.int32),
               degenerate=np.zeros((nc, h), np.uint8), sim3=np.zeros((nc, h, 13), np.float32), inliers=np.zeros((nc, h, w), np.uint32))
    if extras:
        out.update(x3dc1=np.zeros((nc, cap, 3), np.float32), x3dc2=np.zeros((nc, cap, 3), np.float32), max_err=np.zeros((nc, cap, 2), np.float32))
    table.ctx.check(table.lib.afv_table_sim3_hypotheses(
        table.handle, points.handle, ptr(sa), ptr(sb), jobs, nc, ptr(mp1), ptr(mp2), ptr(idx1), ptr(idx2), nhyp, mask_words, ptr(out["n"]),
        ptr(out["index1"]), ptr(out["count"]), ptr(out["degenerate"]), ptr(out["sim3"]), ptr(out["inliers"]), ptr(out.get("x3dc1")),
        ptr(out.get("x3dc2")), ptr(out.get("max_err"))), "afv_table_sim3_hypotheses")
    return out


class Sim3Solver:
    """the reference's interface over the device's answer for one candidate"""

    @classmethod
    def batch(cls, table, points, cur, cands, mp1, mp2, idx2, cams, fix_scale, seed=0, idx1=None, nhyp=300):
        """one device call for all candidates of a loop check (LoopClosing.cc:279-300 creates all solvers before it iterates any).
        table: the keyframe table whose slots hold the keyframes' geometry; points: the MapPoints store; cur: the slot of the current
        keyframe, cands: the candidates' slots; mp1 [n1] (or one row per candidate): the point id of every feature of the current
        keyframe (GetMapPointMatches), -1 = none; mp2 [nc, n1]: vpMatched12 of every candidate as point ids; idx2 [nc, n1]:
        GetIndexInKeyFrame of those points in their candidate; idx1: the same for mp1 in the current keyframe (None: the feature itself);
        cams: {slot: {Rcw, tcw, fx, fy, cx, cy}}; fix_scale: mbFixScale; seed: an int (candidate c draws from seed + c) or one per
        candidate.  Returns a list of Sim3Solver."""
        cands = [int(s) for s in cands]
        nc = len(cands)
        seeds = [int(seed) + c for c in range(nc)] if np.ndim(seed) == 0 else [int(s) for s in seed]
        if len(seeds) != nc:
            raise ValueError("Sim3Solver.batch: one seed per candidate is expected")
        jobs = sim3_jobs(cams[int(cur)], [cams[s] for s in cands], fix_scale, seeds)
        out = hypotheses(table, points, [int(cur)] * nc, cands, jobs, mp1, mp2, idx2, idx1, nhyp)
        n1 = int(np.asarray(mp2).shape[1]) if np.asarray(mp2).ndim == 2 else table.cap
        return [cls(int(out["n"][c]), out["index1"][c], out["count"][c], out["degenerate"][c], out["sim3"][c], out["inliers"][c], n1)
                for c in range(nc)]

    def __init__(self, n, index1, count, degenerate, sim3, inliers, n1):
        """n = N, index1 = mvnIndices1, count / degenerate / sim3 / inliers = the rows of one candidate, n1 = mN1"""
        self.N, self.mN1 = int(n), int(n1)
        self.index1, self.count, self.degenerate, self.sim3, self.inliers = index1, count, degenerate, sim3, inliers
        self.nhyp = len(count)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = None       # the hypothesis bestT12 / mvbBestInliers come from
        self.SetRansacParameters(maxIterations=min(300, self.nhyp))   # :109, within what the device evaluated

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        """:112-136 (Q3).  maxIterations beyond the evaluated hypotheses and minInliers < 3 raise ValueError"""
        if maxIterations > self.nhyp:
            raise ValueError("Sim3Solver: maxIterations %d exceeds the %d hypotheses the device evaluated" % (maxIterations, self.nhyp))
        if minInliers < 3:
            raise ValueError("Sim3Solver: minInliers must be at least 3")
        self.mRansacProb, self.mRansacMinInliers = float(probability), int(minInliers)
        with np.errstate(all="ignore"):
            epsilon = np.float32(minInliers) / np.float32(self.N)
        if minInliers == self.N:
            n_it = 1
        else:
            e3 = float(epsilon) ** 3 if math.isfinite(float(epsilon)) else float("inf")
            arg = 1.0 - e3
            den = math.log(arg) if arg > 0 else (float("-inf") if arg == 0 else float("nan"))
            num = math.log(1.0 - self.mRansacProb) if self.mRansacProb < 1 else float("-inf")
            v = num / den if den != 0 else float("inf")
            # a double outside int's range is undefined in the reference: here it saturates and a NaN reads maxIterations
            n_it = int(maxIterations) if math.isnan(v) else int(min(max(math.ceil(v) if math.isfinite(v) else v, -2 ** 31), 2 ** 31 - 1))
        self.mRansacMaxIts = max(1, min(n_it, int(maxIterations)))
        self.mnIterations = 0

    def _flags(self, h):
        """mvbInliersi of hypothesis h over the N correspondences"""
        k = np.arange(self.N)
        return ((self.inliers[h][k >> 5] >> (k & 31).astype(np.uint32)) & 1).astype(bool)

    def _T12(self, h):
        r = self.sim3[h]
        T = np.zeros((4, 4), np.float32)
        T[:3, :3] = (np.float32(r[12]) * r[:9]).reshape(3, 3)   # mat3f sR = s12i * R12i, one float product per element
        T[:3, 3] = r[9:12]
        T[3, 3] = 1
        return T

    def iterate(self, nIterations):
        """:138-204 -> (T12 [4, 4] float32 or None, bNoMore, vbInliers [mN1] bool, nInliers)"""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            c = int(self.count[h])     # a degenerate hypothesis counts 0 and still advances mnIterations
            if c >= self.mnBestInliers:
                self.mnBestInliers = c
                self.best = h
                if c > self.mRansacMinInliers:
                    vb[self.index1[:self.N][self._flags(h)]] = True
                    return self._T12(h), False, vb, c
        return None, self.mnIterations >= self.mRansacMaxIts, vb, 0

    def find(self):
        """:206-210 -> (T12 or None, vbInliers12, nInliers)"""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def GetEstimatedRotation(self):
        return None if self.best is None else self.sim3[self.best][:9].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return None if self.best is None else self.sim3[self.best][9:12].copy()

    def GetEstimatedScale(self):
        return None if self.best is None else float(self.sim3[self.best][12])


def sim3opt_jobs(cam_cur, cams_cand, S12s, th2, fix_scale):
    """afv_sim3opt_job records from camera dicts {Rcw, tcw, fx, fy, cx, cy} and starts (R12, t12, s12): 1 = the current keyframe, 2 = candidate c"""
    jobs = (Sim3OptJob * len(cams_cand))()
    for c, (cam2, S12) in enumerate(zip(cams_cand, S12s)):
        j = jobs[c]
        j.struct_size = C.sizeof(Sim3OptJob)
        j.fix_scale = 1 if fix_scale else 0
        j.th2 = float(np.float32(th2))
        for side, cam in (("1", cam_cur), ("2", cam2)):
            for name, cnt in (("Rcw", 9), ("tcw", 3)):
                v = np.asarray(cam[name], np.float32).reshape(cnt)
                dst = getattr(j, name + side)
                for k in range(cnt):
                    dst[k] = float(v[k])
            for key in ("fx", "fy", "cx", "cy"):
                setattr(j, key + side, float(np.float32(cam[key])))
        R12, t12 = np.asarray(S12[0], np.float32).reshape(9), np.asarray(S12[1], np.float32).reshape(3)
        for k in range(9):
            j.R12[k] = float(R12[k])
        for k in range(3):
            j.t12[k] = float(t12[k])
        j.s12 = float(np.float32(S12[2]))
    return jobs


def optimize_sim3(table, points, slot_a, slot_b, jobs, mp1, mp2, idx2):
    """afv_table_optimize_sim3 as it is: rows [nc, cap] in; (results: a ctypes array of Sim3OptResult, state [nc, cap] uint8) out"""
    sa, sb = (np.ascontiguousarray(v, np.int32).reshape(-1) for v in (slot_a, slot_b))
    nc, cap = len(sa), table.cap
    if len(sb) != nc or len(jobs) != nc:
        raise ValueError("OptimizeSim3: %d candidates need %d slots and jobs" % (nc, nc))
    mp1, mp2, idx2 = _rows(mp1, nc, cap, "mp1", True), _rows(mp2, nc, cap, "mp2"), _rows(idx2, nc, cap, "idx2")
    results = (Sim3OptResult * nc)()
    state = np.zeros((nc, cap), np.uint8)
    table.ctx.check(table.lib.afv_table_optimize_sim3(table.handle, points.handle, ptr(sa), ptr(sb), jobs, nc, ptr(mp1), ptr(mp2), ptr(idx2), results,
                                                      ptr(state)), "afv_table_optimize_sim3")
    return results, state


def OptimizeSim3Batch(table, points, cur, cands, mp1, mp2, idx2, cams, S12s, th2=10, fix_scale=False):
    """Optimizer::OptimizeSim3 for every candidate of a loop check in one device call.  table / points / cur / cands / mp1 / mp2 / idx2 / cams:
    as Sim3Solver.batch takes them (the slots also need their information plane: DescriptorTable.set_inf or a promoted frame); S12s: per
    candidate (R12 [3, 3], t12 [3], s12), what the solver's GetEstimatedRotation / Translation / Scale return; th2, fix_scale: the
    reference's arguments.  Returns per candidate (nInliers, mp2_out, (R12 [3, 3], t12 [3], s12)) with mp2_out = vpMatches1 after the call
    (-1 where the reference writes NULL) and the Sim3 in double (the start itself when the call answers 0 for want of correspondences)."""
    cands = [int(s) for s in cands]
    nc = len(cands)
    if len(S12s) != nc:
        raise ValueError("OptimizeSim3Batch: one start per candidate is expected")
    jobs = sim3opt_jobs(cams[int(cur)], [cams[s] for s in cands], S12s, th2, fix_scale)
    results, state = optimize_sim3(table, points, [int(cur)] * nc, cands, jobs, mp1, mp2, idx2)
    mp2 = np.asarray(mp2, np.int32)
    out = []
    for c in range(nc):
        r = results[c]
        row = mp2[c].copy()
        st = state[c, :len(row)]
        row[(st == _lib.SIM3OPT_REMOVED_FIRST) | (st == _lib.SIM3OPT_REMOVED_SECOND)] = -1
        out.append((int(r.n_in), row, (np.array(r.R12[:], np.float64).reshape(3, 3), np.array(r.t12[:], np.float64), float(r.s12))))
    return out


def OptimizeSim3(table, points, cur, cand, mp1, mp2, idx2, cams, S12, th2=10, fix_scale=False):
    """one candidate: mp2 / idx2 [n1].  Returns (nInliers, mp2_out, (R12, t12, s12))"""
    return OptimizeSim3Batch(table, points, cur, [cand], mp1, np.asarray(mp2, np.int32)[None], np.asarray(idx2, np.int32)[None], cams, [S12], th2,
                             fix_scale)[0]
