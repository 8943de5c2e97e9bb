"""Plain-Python restatement of the covisibility count and the local map (include/afv_covis.h), the normative semantics.

Reference: KeyFrame::UpdateConnections (KeyFrame.cc:329-418), Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:1040-1104), the
skip of SearchLocalPoints (Tracking.cc:1003-1005).  A map here is: planes[slot] = list of point ids (-1 = none) of a table slot, and a store
given as (capacity, set_ids, bad_ids).  `wrong=` switches on ONE deliberately wrong reading; the scene tests show each scene is moved by its
variant (tests/test_covis_ref_cpu.py).

Also here: the toy map of objects with observation maps, written after the reference's text, which the plane reading is shown equal to.
"""
WRONG = ("q_dup_once", "plane_dup_twice", "self_counted", "ties_ascending", "best_tie_highest", "th_strict", "no_fallback",
         "last_occurrence", "bad_kf_best")


class Store:
    def __init__(self, capacity, set_ids, bad_ids=()):
        self.capacity, self.set_ids, self.bad_ids = int(capacity), set(int(i) for i in set_ids), set(int(i) for i in bad_ids)

    def good(self, i):  # V1
        return 0 <= i < self.capacity and i in self.set_ids and i not in self.bad_ids


def votes(planes, store, slots, queries, wrong=None):
    """queries: ("slot", position) | ("ids", [ids]).  Returns votes[q][k]."""
    out = []
    member_sets = {s: set(planes[s]) for s in slots}  # the observations are a map: an id stands in it once
    for kind, arg in queries:
        Q = list(planes[slots[arg]]) if kind == "slot" else list(arg)
        Q = [i for i in Q if store.good(i)]
        if wrong == "q_dup_once":
            Q = sorted(set(Q))
        row = []
        for k, s in enumerate(slots):
            if kind == "slot" and k == arg and wrong != "self_counted":
                row.append(0)
                continue
            if wrong == "plane_dup_twice":
                plane = list(planes[s])
                row.append(sum(plane.count(i) for i in Q))
            else:
                members = member_sets[s]
                row.append(sum(1 for i in Q if i in members))
        out.append(row)
    return out


def connect(row, key_id, th, skip_bad=False, kf_bad=None, wrong=None):
    """The connection rule over one row of votes.  Returns (order, best, n_nonzero)."""
    nk = len(row)
    stands = [row[p] > 0 and not (skip_bad and kf_bad[p] and wrong != "bad_kf_best") for p in range(nk)]
    best, nmax = -1, 0
    walk = sorted(range(nk), key=lambda p: key_id[p])  # the map is walked in ascending keyId
    for p in walk:
        if not stands[p]:
            continue
        if row[p] > nmax or (wrong == "best_tie_highest" and row[p] == nmax):
            nmax, best = row[p], p
    members = [p for p in walk if stands[p] and (row[p] > th if wrong == "th_strict" else row[p] >= th)]
    if not members and best >= 0 and wrong != "no_fallback":
        members = [best]
    # sort ascending by (votes, keyId), then push_front: descending in both
    members.sort(key=lambda p: (row[p], key_id[p]))
    if wrong == "ties_ascending":
        members.sort(key=lambda p: (row[p], -key_id[p]))
    order = members[::-1]
    return order, best, sum(1 for v in row if v > 0)


def local_points(planes, store, local, frame_pts=None, wrong=None):
    """Returns (ids, seen)."""
    ids, have = [], set()
    cand = [i for s in local for i in planes[s]]
    if wrong == "last_occurrence":
        keep = {}
        for c, i in enumerate(cand):
            if store.good(i):
                keep[i] = c
        ids = [i for c, i in enumerate(cand) if store.good(i) and keep[i] == c]
    else:
        for i in cand:
            if store.good(i) and i not in have:
                have.add(i)
                ids.append(i)
    mine = set(i for i in (frame_pts or []) if store.good(i))
    return ids, [1 if i in mine else 0 for i in ids]


# ---- the toy map: objects with observation maps, after the reference's text ----
class ToyPoint:
    def __init__(self, pt_id):
        self.ptId, self.bad, self.observations = pt_id, False, {}  # keyId -> ToyKeyFrame

    def isBad(self):
        return self.bad


class ToyKeyFrame:
    def __init__(self, key_id, n):
        self.keyId, self.bad = key_id, False
        self.mvpMapPoints = [None] * n
        self.connectedKeyFrameWeights, self.connectedKeyFrames = {}, {}
        self.orderedConnectedKeyFrames, self.orderedWeights = [], []
        self.mbFirstConnection, self.mpParent, self.mspChildrens = True, None, set()

    def isBad(self):
        return self.bad

    def AddMapPoint(self, pt, idx):
        self.mvpMapPoints[idx] = pt
        pt.observations[self.keyId] = self

    # KeyFrame.cc:131-168
    def AddConnection(self, kf, weight):
        if kf.keyId not in self.connectedKeyFrameWeights:
            self.connectedKeyFrameWeights[kf.keyId] = weight
            self.connectedKeyFrames[kf.keyId] = kf
        elif self.connectedKeyFrameWeights[kf.keyId] != weight:
            self.connectedKeyFrameWeights[kf.keyId] = weight
        else:
            return
        self.UpdateBestCovisibles()

    def UpdateBestCovisibles(self):
        pairs = [(w, self.connectedKeyFrames[k]) for k, w in sorted(self.connectedKeyFrameWeights.items())]
        pairs.sort(key=lambda a: (a[0], a[1].keyId))
        self.orderedConnectedKeyFrames = [kf for _, kf in pairs][::-1]
        self.orderedWeights = [w for w, _ in pairs][::-1]

    # KeyFrame.cc:329-418
    def UpdateConnections(self, th=15):
        counter, kfs = {}, {}
        for pt in list(self.mvpMapPoints):
            if pt is None:
                continue
            if pt.isBad():
                continue
            for key_id, kf in sorted(pt.observations.items()):
                if key_id == self.keyId:
                    continue
                counter[key_id] = counter.get(key_id, 0) + 1
                kfs[key_id] = kf
        if not kfs:
            return
        nmax, kf_max = 0, None
        pairs = []
        for key_id in sorted(counter):
            w = counter[key_id]
            if w > nmax:
                nmax, kf_max = w, kfs[key_id]
            if w >= th:
                pairs.append((w, kfs[key_id]))
                kfs[key_id].AddConnection(self, w)
        if not pairs:
            pairs.append((nmax, kf_max))
            kf_max.AddConnection(self, nmax)
        pairs.sort(key=lambda a: (a[0], a[1].keyId))
        self.connectedKeyFrameWeights = dict(counter)
        self.connectedKeyFrames = dict(kfs)
        self.orderedConnectedKeyFrames = [kf for _, kf in pairs][::-1]
        self.orderedWeights = [w for w, _ in pairs][::-1]
        if self.mbFirstConnection and self.keyId != 0:
            self.mpParent = self.orderedConnectedKeyFrames[0]
            self.mpParent.mspChildrens.add(self)
            self.mbFirstConnection = False

    def GetBestCovisibilityKeyFrames(self, N):
        return list(self.orderedConnectedKeyFrames[:N])


def toy_update_local_map(frame_pts, max_keyframes=80, best_cov=10):
    """Tracking.cc:1040-1144 on toy objects: frame_pts is a list of ToyPoint | None.  Returns (localKeyframes, refKeyframe, localPts, seen)
    or None where the reference returns early (no keyframe observes a point of the frame)."""
    counter, kfs = {}, {}
    for pt in frame_pts:
        if pt is not None and not pt.isBad():
            for key_id, kf in pt.observations.items():
                counter[key_id] = counter.get(key_id, 0) + 1
                kfs[key_id] = kf
    if not counter:
        return None
    local, ids, max_obs, ref = [], set(), 0, None
    for key_id in sorted(kfs):
        kf = kfs[key_id]
        if kf.isBad():
            continue
        if counter[key_id] > max_obs:
            max_obs, ref = counter[key_id], kf
        local.append(kf)
        ids.add(key_id)
    for kf in list(local):  # the range-for reads end() once: keyframes pushed below are not walked
        if len(local) > max_keyframes:
            break
        for nb in kf.GetBestCovisibilityKeyFrames(best_cov):
            if not nb.isBad() and nb.keyId not in ids:
                local.append(nb)
                ids.add(nb.keyId)
                break
        for child in sorted(kf.mspChildrens, key=lambda c: c.keyId):
            if not child.isBad() and child.keyId not in ids:
                local.append(child)
                ids.add(child.keyId)
                break
        parent = kf.mpParent
        if parent is not None and not parent.isBad() and parent.keyId not in ids:
            local.append(parent)
            ids.add(parent.keyId)
            break
    pts, have = [], set()
    for kf in local:
        for pt in kf.mvpMapPoints:
            if pt is None:
                continue
            if pt.ptId in have:
                continue
            if not pt.isBad():
                pts.append(pt)
                have.add(pt.ptId)
    mine = set(pt.ptId for pt in frame_pts if pt is not None and not pt.isBad())
    return local, ref, pts, [1 if pt.ptId in mine else 0 for pt in pts]
