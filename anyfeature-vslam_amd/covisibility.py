"""The covisibility count and the local map over the keyframe table's map-point planes (include/afv_covis.h), and a host mirror of the
reference's covisibility graph on top of them.

Reference: KeyFrame::UpdateConnections, AddConnection, UpdateBestCovisibles and the getters (KeyFrame.cc:131-219, :329-418),
Tracking::UpdateLocalKeyFrames / UpdateLocalPoints (Tracking.cc:1040-1144).  The reference walks MapPoint::GetObservations(); the device reads
the planes DescriptorTable.set_map_points stored and the flags of the MapPoints store.  What stays on the host is the bookkeeping of who is
connected to whom - dictionaries, no counting.

The entry points of afv_covis.h are bound by this module's own table (SYMBOLS), beside _lib.SYMBOLS as afv_akaze.h's stand beside it.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ptr

MAX_IDS, MAX_QUERIES, MAX_LOCAL, MAX_KF, MAX_CAP = 65536, 64, 256, 4096, 4096
QUERY_SLOT, QUERY_IDS = 0, 1


class CovisQuery(C.Structure):
    """afv_covis_query"""
    _fields_ = [("struct_size", C.c_uint32), ("kind", C.c_int32), ("position", C.c_int32), ("n", C.c_int32), ("ids", C.c_void_p),
                ("th", C.c_int32), ("skip_bad", C.c_int32)]


_vp, _i = C.c_void_p, C.c_int
SYMBOLS = {
    "afv_table_covis_votes": (_i, [_vp, _vp, _vp, _vp, _vp, _i, C.POINTER(CovisQuery), _i, _vp, _vp, _vp, _vp, _vp]),
    "afv_table_local_points": (_i, [_vp, _vp, _vp, _i, _vp, _i, _i, _vp, _vp, _vp]),
}
_bound = None


def bind():
    """the library with this module's symbols bound (AttributeError if it does not export one)"""
    global _bound
    if _bound is None:
        lib = _lib.load()
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _bound = lib
    return _bound


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1))


def covisibility_votes(table, points, slots, key_ids, queries, kf_bad=None, want_votes=True, want_order=True):
    """votes of the listed keyframes for up to 64 queries in one device call.
    slots / key_ids: the live keyframes (table slots, their keyIds).  queries: a list of dicts, {"slot": position in `slots`} or
    {"ids": point ids}, each with "th" (default 15) and "skip_bad" (default False).
    Returns (votes [nq, nk] | None, order: list of arrays of positions, best [nq], n_nonzero [nq])."""
    lib = bind()
    slots, key_ids = _i32(slots), _i32(key_ids)
    nk, nq = len(slots), len(queries)
    if len(key_ids) != nk:
        raise ValueError("covisibility_votes: %d slots, %d key ids" % (nk, len(key_ids)))
    bad = None if kf_bad is None else np.ascontiguousarray(np.asarray(kf_bad, np.uint8).reshape(-1))
    if bad is not None and len(bad) != nk:
        raise ValueError("covisibility_votes: kf_bad must have one entry per keyframe")
    recs = (CovisQuery * max(nq, 1))()
    keep = []
    for r, q in zip(recs, queries):
        r.struct_size = C.sizeof(CovisQuery)
        r.th, r.skip_bad = int(q.get("th", 15)), int(bool(q.get("skip_bad", False)))
        if "slot" in q:
            r.kind, r.position = QUERY_SLOT, int(q["slot"])
        else:
            ids = _i32(q["ids"])
            keep.append(ids)
            r.kind, r.n, r.ids = QUERY_IDS, len(ids), ids.ctypes.data if len(ids) else None
    cells = max(nq * nk, 1)
    votes = np.zeros(cells, np.int32) if want_votes else None
    order = np.full(cells, -1, np.int32) if want_order else None
    n_order, best, nz = np.zeros(max(nq, 1), np.int32), np.full(max(nq, 1), -1, np.int32), np.zeros(max(nq, 1), np.int32)
    table.ctx.check(lib.afv_table_covis_votes(table.handle, points.handle, ptr(slots), ptr(key_ids), ptr(bad), nk, recs, nq, ptr(votes), ptr(order),
                                              ptr(n_order), ptr(best), ptr(nz)), "afv_table_covis_votes")
    orders = None
    if want_order:
        order = order[:nq * nk].reshape(nq, nk)
        orders = [order[q, :n_order[q]].copy() for q in range(nq)]
    return (votes[:nq * nk].reshape(nq, nk) if want_votes else None), orders, best[:nq].copy(), nz[:nq].copy()


def local_points(table, points, local, frame_pts=None, max_out=None):
    """Tracking::UpdateLocalPoints over the slots `local` (the order of localKeyframes): the good ids of their planes at their first
    occurrence.  frame_pts: the frame's point ids; seen[j] = 1 where local point j is one of them (SearchLocalPoints skips those).
    max_out: room of the answer (default: every feature of the listed slots could be a point).  The call brings back as many entries as
    the answer can have - min(max_out, features of the listed slots) - in its one transfer, whatever the total turns out to be; a caller
    who knows a bound passes it.  Returns (ids, seen | None)."""
    lib = bind()
    local = _i32(local)
    nl = len(local)
    if max_out is None:
        max_out = nl * table.cap
    pts = None if frame_pts is None else _i32(frame_pts)
    ids = np.full(max(int(max_out), 1), -1, np.int32)
    seen = None if pts is None else np.zeros(max(int(max_out), 1), np.uint8)
    n = C.c_int32(0)
    table.ctx.check(lib.afv_table_local_points(table.handle, points.handle, ptr(local) if nl else None, nl, ptr(pts) if pts is not None and len(pts) else None,
                                               0 if pts is None else len(pts), int(max_out), ptr(ids), ptr(seen), C.byref(n)), "afv_table_local_points")
    return ids[:n.value].copy(), (None if seen is None else seen[:n.value].copy())


class _Node:
    """the connection members of one KeyFrame"""
    __slots__ = ("slot", "key_id", "bad", "weights", "ordered", "ordered_w", "first", "parent", "children", "loop_edges")

    def __init__(self, slot, key_id):
        self.slot, self.key_id, self.bad = slot, key_id, False
        self.weights = {}      # connectedKeyFrameWeights: slot -> weight
        self.ordered, self.ordered_w = [], []
        self.first, self.parent, self.children, self.loop_edges = True, None, set(), set()


class CovisibilityGraph:
    """Host mirror of the covisibility graph over a keyframe table: keyframes are named by their table slot, ordered by their keyId.
    votes_fn / local_fn stand in for the two device calls (tests)."""

    TH = 15  # KeyFrame.cc:369

    def __init__(self, table, points, votes_fn=None, local_fn=None):
        self.table, self.points = table, points
        self._votes = votes_fn or (lambda slots, key_ids, queries, kf_bad: covisibility_votes(table, points, slots, key_ids, queries, kf_bad))
        self._local = local_fn or (lambda local, frame_pts: local_points(table, points, local, frame_pts))
        self.kf = {}  # slot -> _Node, in insertion order

    def add_keyframe(self, slot, key_id):
        slot, key_id = int(slot), int(key_id)
        if slot in self.kf:
            raise ValueError("CovisibilityGraph.add_keyframe: slot %d is listed" % slot)
        if any(n.key_id == key_id for n in self.kf.values()):
            raise ValueError("CovisibilityGraph.add_keyframe: keyId %d is listed" % key_id)
        self.kf[slot] = _Node(slot, key_id)

    def set_bad(self, slot, bad=True):
        self.kf[int(slot)].bad = bool(bad)

    def _lists(self):
        slots = list(self.kf)
        return slots, [self.kf[s].key_id for s in slots], np.array([self.kf[s].bad for s in slots], np.uint8)

    def _sorted(self, pairs):
        """[(weight, slot)] as KeyframeComparison and push_front leave it: weight descending, ties by keyId descending"""
        pairs = sorted(pairs, key=lambda a: (a[0], self.kf[a[1]].key_id), reverse=True)
        return [s for _, s in pairs], [w for w, _ in pairs]

    # KeyFrame.cc:131-168
    def _add_connection(self, node, other, weight):
        if node.weights.get(other) == weight:
            return
        node.weights[other] = weight
        node.ordered, node.ordered_w = self._sorted([(w, s) for s, w in node.weights.items()])

    def _apply(self, slot, slots, row, order):
        """the side effects of UpdateConnections of `slot` from its row of votes (KeyFrame.cc:361-417)"""
        node = self.kf[slot]
        counter = {slots[p]: int(row[p]) for p in range(len(slots)) if row[p] > 0}
        if not counter:
            return
        for p in order:  # the keyframes at the threshold, or the best one alone
            self._add_connection(self.kf[slots[p]], slot, int(row[p]))
        node.weights = counter  # the whole counter, not only the entries at the threshold (KeyFrame.cc:405)
        node.ordered, node.ordered_w = [slots[p] for p in order], [int(row[p]) for p in order]
        if node.first and node.key_id != 0:
            node.parent = node.ordered[0]
            self.kf[node.parent].children.add(slot)
            node.first = False

    def UpdateConnections(self, slot):
        self.UpdateConnectionsBatch([slot])

    def UpdateConnectionsBatch(self, batch):
        """UpdateConnections of every slot of `batch`, one device call per 64: the planes are read as they stand at the call, the host side
        effects are applied in list order"""
        batch = [int(s) for s in batch]
        slots, key_ids, bad = self._lists()
        pos = {s: p for p, s in enumerate(slots)}
        for at in range(0, len(batch), MAX_QUERIES):
            part = batch[at:at + MAX_QUERIES]
            votes, order, _, _ = self._votes(slots, key_ids, [{"slot": pos[s], "th": self.TH} for s in part], None)
            for q, s in enumerate(part):
                self._apply(s, slots, votes[q], order[q])

    # ---- the getters (KeyFrame.cc:170-219) ----
    def GetVectorCovisibleKeyFrames(self, slot):
        return list(self.kf[int(slot)].ordered)

    def GetBestCovisibilityKeyFrames(self, slot, N=10):
        return list(self.kf[int(slot)].ordered[:int(N)])

    def GetCovisiblesByWeight(self, slot, w):
        node = self.kf[int(slot)]
        n = sum(1 for x in node.ordered_w if x >= w)  # upper_bound with weightComp
        if n == len(node.ordered_w):
            return []  # it == end(): the reference answers an empty vector when every weight reaches w
        return list(node.ordered[:n])

    def GetWeight(self, slot, other):
        return self.kf[int(slot)].weights.get(int(other), 0)

    def GetConnectedKeyFrames(self, slot):
        """ascending keyId, as the reference's map"""
        return sorted(self.kf[int(slot)].weights, key=lambda s: self.kf[s].key_id)

    def EraseConnection(self, slot, other):
        node = self.kf[int(slot)]
        if int(other) in node.weights:
            del node.weights[int(other)]
            node.ordered, node.ordered_w = self._sorted([(w, s) for s, w in node.weights.items()])

    def GetParent(self, slot):
        return self.kf[int(slot)].parent

    def GetChilds(self, slot):
        return sorted(self.kf[int(slot)].children, key=lambda s: self.kf[s].key_id)

    def AddLoopEdge(self, slot, other):
        self.kf[int(slot)].loop_edges.add(int(other))

    def essential_graph_dict(self, min_feat=100):
        """the {parent, loop_edges, covisibles} pieces OptimizeEssentialGraph(graph=...) takes, keyed by keyId, over the keyframes not bad"""
        key = lambda s: self.kf[s].key_id
        live = [n for n in self.kf.values() if not n.bad]
        return {"parent": {n.key_id: (None if n.parent is None else key(n.parent)) for n in live},
                "loop_edges": {n.key_id: sorted(key(s) for s in n.loop_edges) for n in live},
                "covisibles": {n.key_id: [key(s) for s in self.GetCovisiblesByWeight(n.slot, min_feat)] for n in live}}

    def connected(self, slot):
        """the list KeyFrameDatabase.DetectLoopCandidates(slot, minScore, connected, ...) and min_score_to_connected take: they want the
        keyframes themselves, not a callable"""
        return self.GetConnectedKeyFrames(slot)

    def best_covisibles(self, slot):
        """the callable KeyFrameDatabase.DetectLoopCandidates / DetectRelocalizationCandidates take as best_covisibles: pass the bound
        method, g.best_covisibles"""
        return self.GetBestCovisibilityKeyFrames(slot, 10)

    # ---- Tracking::UpdateLocalMap (Tracking.cc:1030-1144) ----
    def UpdateLocalMap(self, frame_pts, max_keyframes=80, best_cov=10):
        """frame_pts: the point ids of the current frame (-1 = none).  Returns (localKeyframes, refKeyframe, local_ids, seen) - slots, a
        slot, the point ids in the order of localPts, and seen[j] = 1 for the local points SearchLocalPoints skips - or None where the
        reference returns before it touches the local map (no keyframe observes a point of the frame).
        The children of a keyframe are walked in ascending keyId (the reference's set is ordered by pointer)."""
        slots, key_ids, bad = self._lists()
        if not slots:
            return None
        votes, order, best, nz = self._votes(slots, key_ids, [{"ids": frame_pts, "th": 1, "skip_bad": True}], bad)
        if int(nz[0]) == 0:
            return None
        local = sorted((slots[p] for p in order[0]), key=lambda s: self.kf[s].key_id)  # the map iteration: ascending keyId
        ref = slots[int(best[0])] if int(best[0]) >= 0 else None
        have = set(local)
        for s in list(local):  # the range-for reads end() once: keyframes pushed below are not walked
            if len(local) > max_keyframes:
                break
            node = self.kf[s]
            for nb in node.ordered[:best_cov]:
                if not self.kf[nb].bad and nb not in have:
                    local.append(nb)
                    have.add(nb)
                    break
            for ch in self.GetChilds(s):
                if not self.kf[ch].bad and ch not in have:
                    local.append(ch)
                    have.add(ch)
                    break
            pa = node.parent
            if pa is not None and not self.kf[pa].bad and pa not in have:
                local.append(pa)
                have.add(pa)
                break
        ids, seen = self._local(local, frame_pts)
        return local, ref, ids, seen
