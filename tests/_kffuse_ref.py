"""Plain-Python restatement of Fuse into keyframes of the table (afv_table_fuse_points, include/afv_hip.h).  TEST INFRASTRUCTURE ONLY.

The NORMATIVE semantics of the call, which the device is held to bit for bit on best, occupant, status and nfused:

  geometry   tests/_points_ref.project(..., FUSE) with the camera of the job (the slot's pose, or the decomposed Scw)
  search     tests/_proj_ref._fuse over the queries the geometry leaves (use_inf_gate: the 5.99 / 7.8 gates of Fuse no. 1)
  plane      status 1 when the id occurs in the slot's plane of point ids (IsInKeyFrame / spAlreadyFound), ahead of the geometry;
             occupant = plane[best]; 4 free, 5 occupant bad in the store, 6 occupant good - an occupant id outside [0, capacity) or never
             set counts as good and the store is not read for it

Restated from FeatureMatcher::Fuse(pKF, vpMapPoints, th) (FeatureMatcher.cc:794-940), Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)
(:942-1064) - whose decomposition of Scw (:954-958) keeps tcw UNDIVIDED by scw, a quirk that is restated, not repaired - and, on a toy map,
LocalMapping::SearchInNeighbors (LocalMapping.cc:503-535) and LoopClosing::SearchAndFuse (LoopClosing.cc:601-628) in their sequential order.
"""
import numpy as np

import _points_ref as R
import _proj_ref as PR

f32 = np.float32
INVALID, IN_KEYFRAME, NOT_IN_VIEW, NO_FEATURE, FREE, OCCUPANT_BAD, REPLACE = range(7)
TH_LOW = 50.0


class Grid:
    """the camera of a table: image bounds and the grid of KeyFrame::GetFeaturesInArea"""

    def __init__(self, min_x=0.0, max_x=96.0, min_y=0.0, max_y=64.0, cols=64, rows=48):
        self.min_x, self.max_x, self.min_y, self.max_y = f32(min_x), f32(max_x), f32(min_y), f32(max_y)
        self.cols, self.rows = int(cols), int(rows)
        self.inv_w = f32(cols) / (self.max_x - self.min_x)
        self.inv_h = f32(rows) / (self.max_y - self.min_y)


class Keyframe:
    """what a slot holds: mvKeysUn, keyPtsSize, descriptors, mvuRight (None: monocular), keyPtsInf (None: 1 / size^2 as a frame derives
    it), mvpMapPoints (point id | -1) and the pose with its intrinsics (an _points_ref.Camera; its bounds and tol are overridden by the
    grid and the context)"""

    def __init__(self, x, y, sizes, desc, plane=None, u_right=None, inf=None, cam=None):
        self.x, self.y, self.sizes = (np.ascontiguousarray(a, np.float32).reshape(-1) for a in (x, y, sizes))
        self.n = len(self.x)
        self.desc = np.ascontiguousarray(desc)
        self.plane = np.full(self.n, -1, np.int32) if plane is None else np.array(plane, np.int32).reshape(-1)
        self.u_right = None if u_right is None else np.ascontiguousarray(u_right, np.float32)
        with np.errstate(all="ignore"):
            self.inf = (f32(1.0) / (self.sizes * self.sizes)) if inf is None else np.ascontiguousarray(inf, np.float32)
        self.cam = cam


class _View:
    """the feature side tests/_proj_ref.py reads"""

    def __init__(self, kf, grid, with_inf):
        self.N, self.x, self.y, self.sizes, self.descriptors = kf.n, kf.x, kf.y, kf.sizes, kf.desc
        self.u_right = kf.u_right
        self.inf = kf.inf if with_inf else None
        self.min_x, self.min_y, self.grid_inv_w, self.grid_inv_h = grid.min_x, grid.min_y, grid.inv_w, grid.inv_h
        self.grid_cols, self.grid_rows = grid.cols, grid.rows


def decompose_scw(Scw):
    """:954-958 in float, one rounding per operator, three-term sums in _points_ref's order: scw = |row 0 of sRcw|, Rcw = sRcw / scw,
    tcw = the translation of Scw AS IT STANDS (the kept quirk), Ow = -Rcw^T tcw"""
    S = np.asarray(Scw, np.float32).reshape(4, 4)
    sR = S[:3, :3]
    scw = np.sqrt(R.sum3(sR[0, 0] * sR[0, 0], sR[0, 1] * sR[0, 1], sR[0, 2] * sR[0, 2]))
    Rcw = (sR / f32(scw)).astype(np.float32)
    tcw = S[:3, 3].copy()
    return Rcw, tcw, R.twc(Rcw, tcw)


def camera_for(kf, grid, tol, pose=None):
    """the camera of a job: the slot's intrinsics, the table's bounds, the context's sizeTolerance and the slot's pose or the override"""
    c = kf.cam
    Rcw, tcw, Ow = (c.Rcw, c.tcw, c.Ow) if pose is None else pose
    return R.Camera(Rcw=Rcw, tcw=tcw, Ow=Ow, fx=c.fx, fy=c.fy, cx=c.cx, cy=c.cy, mbf=c.mbf, min_x=grid.min_x, max_x=grid.max_x, min_y=grid.min_y,
                    max_y=grid.max_y, tol=tol)


def fuse_target(P, kf, grid, ids, radius_th=3.0, th_low=TH_LOW, use_inf_gate=True, pose=None, tol=1.2, radius_scale=R.RADIUS_SCALE, flip=None,
                proj_flip=None):
    """one job -> best, occupant (int32 [nq]), status (uint8 [nq]), nfused, detail {"o": project()'s dict, "tr": _fuse's trace}"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    nq = len(ids)
    cam = camera_for(kf, grid, tol, pose)
    Q, o = R.queries(P, cam, ids, R.FUSE, radius_th=radius_th, radius_scale=radius_scale, flip=flip)
    flags = P.flags[np.clip(ids, 0, P.capacity - 1)]
    valid = (ids >= 0) & ((flags & R.SET) != 0) & ((flags & R.BAD) == 0)
    held = set(int(v) for v in kf.plane[:kf.n] if v >= 0)
    member = np.array([bool(valid[q]) and int(ids[q]) in held for q in range(nq)], bool)
    search = valid & ~member & o["in_view"]
    Q.valid = search.astype(np.uint8)
    best, _, tr = PR._fuse(_View(kf, grid, use_inf_gate), Q, th_low, proj_flip)
    status = np.zeros(nq, np.uint8)
    occupant = np.full(nq, -1, np.int32)
    for q in range(nq):
        if not valid[q]:
            status[q] = INVALID
        elif member[q]:
            status[q] = IN_KEYFRAME
        elif not o["in_view"][q]:
            status[q] = NOT_IN_VIEW
        elif best[q] < 0:
            status[q] = NO_FEATURE
        else:
            occ = int(kf.plane[best[q]])
            occupant[q] = occ
            if occ < 0:
                status[q] = FREE
            else:
                fl = int(P.flags[occ]) if occ < P.capacity else R.SET   # out of range: good, the store is not read
                status[q] = OCCUPANT_BAD if (fl & R.SET and fl & R.BAD) else REPLACE
    return best.astype(np.int32), occupant, status, int((status >= FREE).sum()), {"o": o, "tr": tr}


def fuse_batch(P, kfs, grid, jobs, tol=1.2):
    """the call: jobs = dicts (slot, ids, radius_th, th_low, use_inf_gate, pose) answered against ONE snapshot -> lists per job + nfused"""
    out = [fuse_target(P, kfs[j["slot"]], grid, j["ids"], j.get("radius_th", 3.0), j.get("th_low", TH_LOW), j.get("use_inf_gate", True),
                       j.get("pose"), tol) for j in jobs]
    return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out], np.array([o[3] for o in out], np.int32)


# ---- a toy map: observations, counts, Replace ----
class ToyMap:
    """points of a store P seen by keyframes kfs (dict slot -> Keyframe): obs[id] = {slot: feature}; the planes of the keyframes and the
    BAD flags of P are kept in step, as AddObservation / AddMapPoint / Replace / SetBadFlag keep them in the reference"""

    def __init__(self, P, kfs):
        self.P, self.kfs = P, kfs
        self.obs = {}
        for s, kf in kfs.items():
            for i, pid in enumerate(kf.plane):
                if pid >= 0:
                    self.obs.setdefault(int(pid), {})[s] = i

    def n_obs(self, pid):
        return len(self.obs.get(pid, {}))

    def is_bad(self, pid):
        return bool(self.P.flags[pid] & R.BAD)

    def in_keyframe(self, pid, s):
        return s in self.obs.get(pid, {})

    def add(self, pid, s, i):
        self.obs.setdefault(pid, {})[s] = i
        self.kfs[s].plane[i] = pid

    def replace(self, old, new):
        """old->Replace(new) (MapPoint.cc:204-249)"""
        if old == new:
            return
        for s, i in list(self.obs.get(old, {}).items()):
            if not self.in_keyframe(new, s):
                self.add(new, s, i)
            else:
                self.kfs[s].plane[i] = -1
        self.obs[old] = {}
        self.P.flags[old] |= R.BAD

    def lists(self):
        return {pid: sorted(o.items()) for pid, o in self.obs.items() if o and not self.is_bad(pid)}

    # the surgery of one answered target, queries in order; a query whose feature or point changed under an earlier query of the same
    # answer is judged against the map as it stands now
    def apply(self, s, ids, best, status, sim3=False):
        for q in range(len(ids)):
            pid, st = int(ids[q]), int(status[q])
            if st < FREE or self.is_bad(pid) or self.in_keyframe(pid, s):
                continue
            self._settle(pid, s, int(best[q]), sim3)

    def _settle(self, pid, s, i, sim3):
        occ = int(self.kfs[s].plane[i])
        if occ < 0:
            self.add(pid, s, i)
        elif occ != pid and not self.is_bad(occ):
            if sim3:
                self.replace(occ, pid)                     # LoopClosing.cc:623: pRep->Replace(loop point)
            elif self.n_obs(occ) > self.n_obs(pid):
                self.replace(pid, occ)                     # FeatureMatcher.cc:924-927
            else:
                self.replace(occ, pid)


def _best_of(P, kf, grid, pid, **kw):
    """the feature one point wins in a keyframe whatever its plane holds (the search does not read the plane)"""
    bare = Keyframe(kf.x, kf.y, kf.sizes, kf.desc, None, kf.u_right, kf.inf, kf.cam)
    best, _, status, _, _ = fuse_target(P, bare, grid, [pid], **kw)
    return int(best[0]), int(status[0])


def fuse_sequential(M, grid, s, ids, sim3_pose=None, **kw):
    """Fuse no. 1 (sim3_pose None) / no. 2 as the reference runs it: query by query against the LIVE map.  -> nFused.  Fuse no. 2 collects
    vpReplacePoint and SearchAndFuse replaces after the loop (LoopClosing.cc:616-624)"""
    kf = M.kfs[s]
    n, later = 0, []
    if sim3_pose is not None:
        kw = dict(kw, use_inf_gate=False, pose=sim3_pose)
    for pid in ids:
        pid = int(pid)
        if pid < 0 or not M.P.flags[pid] & R.SET or M.is_bad(pid) or M.in_keyframe(pid, s):
            continue
        i, st = _best_of(M.P, kf, grid, pid, **kw)
        if st < FREE:
            continue
        n += 1
        if sim3_pose is None:
            M._settle(pid, s, i, False)
        else:
            occ = int(kf.plane[i])
            if occ < 0:
                M.add(pid, s, i)
            elif not M.is_bad(occ):
                later.append((occ, pid))
    for occ, pid in later:
        M.replace(occ, pid)
    return n


def fuse_candidates(M, targets):
    """vpFuseCandidates of :517-533: the points of the targets in order, each once (mnFuseCandidateForKF), bad ones skipped"""
    out, seen = [], set()
    for s in targets:
        for pid in M.kfs[s].plane:
            pid = int(pid)
            if pid < 0 or M.is_bad(pid) or pid in seen:
                continue
            seen.add(pid)
            out.append(pid)
    return out


def search_in_neighbors(M, grid, cur, targets, **kw):
    """LocalMapping.cc:503-535 -> (nFused per target, nFused of the second half)"""
    first = [int(v) for v in M.kfs[cur].plane]   # vpMapPointMatches, taken once (:505)
    nf = [fuse_sequential(M, grid, s, first, **kw) for s in targets]
    return nf, fuse_sequential(M, grid, cur, fuse_candidates(M, targets), **kw)


def search_and_fuse(M, grid, corrected, Scw, loop_ids, **kw):
    """LoopClosing.cc:601-628 -> nFused per corrected keyframe"""
    kw.setdefault("radius_th", 4.0)
    return [fuse_sequential(M, grid, s, loop_ids, sim3_pose=decompose_scw(S), **kw) for s, S in zip(corrected, Scw)]
