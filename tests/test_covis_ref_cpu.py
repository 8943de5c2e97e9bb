"""CPU: the restatement of the covisibility count and the local map (tests/_covis_ref.py) - every constructed scene reaches the rule it is
named after and is moved by the matching wrong reading; the plane reading equals the reference's observation maps on toy maps; the scalar
host program tools/covis_host.cpp answers every scene with the restatement's integers; the host mirror CovisibilityGraph equals the literal
toy-map routines with a stand-in for the two device calls."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _covis_ref as R
import _covis_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- every scene reaches its rule, and the wrong reading moves it ----
@pytest.mark.parametrize("make", S.RULE_SCENES, ids=lambda f: f.__name__)
def test_scene_is_moved_by_its_wrong_variant(make):
    sc = make()
    assert sc["variant"] in R.WRONG
    right, wrong = S.answer(sc), S.answer(sc, sc["variant"])
    assert right != wrong, "scene %s does not tell %s apart" % (sc["name"], sc["variant"])
    for other in R.WRONG:  # (a scene may be moved by other variants too; the restatement itself must be deterministic)
        S.answer(sc, other)
    assert S.answer(sc) == right


def test_scenes_reach_their_rules():
    a = S.answer(S.q_duplicate())
    assert a["votes"] == [[3, 2]]                       # 5, 5, 6 in slot 0; 5, 5 in slot 1
    a = S.answer(S.plane_duplicate())
    assert a["votes"] == [[0, 2], [1, 1]]               # slot 1 holds 5 twice: one vote per query entry
    a = S.answer(S.self_excluded())
    assert a["votes"][0][0] == 0 and a["votes"][1][1] == 0 and a["votes"][0][1] == 2
    a = S.answer(S.order_ties())
    assert a["votes"] == [[0, 16, 16, 17, 1]] and a["order"] == [[3, 2, 1]] and a["best"] == [3] and a["nz"] == [4]  # keyIds 9; 30 before 7
    a = S.answer(S.best_tie())
    assert a["votes"] == [[0, 3, 3, 1]] and a["best"] == [2] and a["order"] == [[2]]     # keyId 3 < 9
    a = S.answer(S.fallback())
    assert a["order"] == [[1]] and a["best"] == [1]
    a = S.answer(S.th_edge())
    assert a["votes"][0] == [0, 14, 15, 15] and a["order"][0] == [3, 2] and a["votes"][1] == [15, 14, 15, 10] and a["order"][1] == [2, 0]
    a = S.answer(S.skip_bad())
    assert a["votes"][0] == [2, 4, 1, 0] and a["best"] == [0, 1] and a["order"][0] == [0, 2] and a["order"][1] == [1, 0, 2]
    a = S.answer(S.first_occurrence())
    assert a["local_ids"] == [4, 7, 2, 1, 3] and a["seen"] == [0, 1, 0, 0, 1]
    a = S.answer(S.all_zero())
    assert a["best"] == [-1, -1, -1] and a["order"] == [[], [], []] and a["nz"] == [0, 0, 0]
    a = S.answer(S.good_filter())
    assert a["votes"] == [[0, 3, 0], [3, 3, 0], [0, 0, 0]] and a["local_ids"] == [15, 0, 2] and a["seen"] == [1, 1, 0]


# ---- the plane reading equals the observation maps ----
def _toy_map(seed, nk, n_feat, n_pts, bad_pt=0.1, bad_kf=0.0, dup=True):
    """a seeded toy map and the planes that agree with it: an id stands in plane(kf) exactly where kf.mvpMapPoints holds the point, and the
    point's observations are the keyframes that hold it.  keyIds ascend with the slot but are not the slots."""
    rng = np.random.RandomState(seed)
    pts = [R.ToyPoint(i) for i in range(n_pts)]
    kfs = [R.ToyKeyFrame(2 * s + (0 if s == 0 else 1), n_feat) for s in range(nk)]
    for kf in kfs:
        for idx in range(n_feat):
            if rng.rand() < 0.7:
                kf.AddMapPoint(pts[rng.randint(0, n_pts)], idx)  # the same point at two features: a duplicate in the plane
    for p in pts:
        p.bad = rng.rand() < bad_pt
    for kf in kfs:
        kf.bad = rng.rand() < bad_kf
    planes = {s: [(-1 if p is None else p.ptId) for p in kf.mvpMapPoints] for s, kf in enumerate(kfs)}
    store = R.Store(n_pts, range(n_pts), [p.ptId for p in pts if p.bad])
    return kfs, pts, planes, store


@pytest.mark.parametrize("seed", range(6))
def test_planes_equal_observation_maps(seed):
    kfs, pts, planes, store = _toy_map(seed, nk=9, n_feat=40, n_pts=60)
    slots, key_ids = list(range(len(kfs))), [kf.keyId for kf in kfs]
    votes = R.votes(planes, store, slots, [("slot", p) for p in slots])
    for p, kf in enumerate(kfs):
        kf.UpdateConnections(th=4)
        order, best, nz = R.connect(votes[p], key_ids, 4)
        counter = {key_ids[k]: v for k, v in enumerate(votes[p]) if v > 0}
        if not counter:
            continue
        assert kf.connectedKeyFrameWeights == counter
        assert [o.keyId for o in kf.orderedConnectedKeyFrames] == [key_ids[k] for k in order]
        assert kf.orderedWeights == [votes[p][k] for k in order]
    # an ids query against the frame's vote (Tracking.cc:1069-1079)
    rng = np.random.RandomState(100 + seed)
    frame = [None if rng.rand() < 0.2 else pts[rng.randint(0, len(pts))] for _ in range(50)]
    row = R.votes(planes, store, slots, [("ids", [-1 if p is None else p.ptId for p in frame])])[0]
    counter = {}
    for p in frame:
        if p is not None and not p.isBad():
            for k in p.observations:
                counter[k] = counter.get(k, 0) + 1
    assert {key_ids[k]: v for k, v in enumerate(row) if v > 0} == counter


# ---- the scalar host program ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("covis_host") / "libcovis_host.so")
    subprocess.run(["g++", "-O3", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tools", "covis_host.cpp"), "-o", out],
                   check=True, timeout=300)
    lib = C.CDLL(out)
    lib.covis_host_create.restype = C.c_void_p
    lib.covis_host_create.argtypes = [C.c_int]
    lib.covis_host_destroy.argtypes = [C.c_void_p]
    lib.covis_host_votes.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 11
    lib.covis_host_local.restype = C.c_int
    lib.covis_host_local.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    return lib


def host_answer(lib, sc, handle=None):
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    planes, n, flags = S.dense(sc)
    h = handle or lib.covis_host_create(sc["capacity"])
    out = {}
    if sc["queries"]:
        nk, nq = len(sc["slots"]), len(sc["queries"])
        slots, keys = np.array(sc["slots"], np.int32), np.array(sc["key_ids"], np.int32)
        bad = np.array(sc["kf_bad"] if sc["kf_bad"] is not None else [0] * nk, np.uint8)
        kind = np.array([0 if "slot" in q else 1 for q in sc["queries"]], np.int32)
        pos = np.array([q.get("slot", -1) for q in sc["queries"]], np.int32)
        lists = [np.array(q.get("ids", []), np.int32) for q in sc["queries"]]
        qptr = np.cumsum([0] + [len(a) for a in lists]).astype(np.int32)
        qids = np.concatenate(lists + [np.zeros(1, np.int32)]).astype(np.int32)
        th = np.array([q.get("th", 15) for q in sc["queries"]], np.int32)
        skip = np.array([int(q.get("skip_bad", False)) for q in sc["queries"]], np.int32)
        votes, order = np.zeros((nq, nk), np.int32), np.zeros((nq, nk), np.int32)
        no, best, nz = np.zeros(nq, np.int32), np.zeros(nq, np.int32), np.zeros(nq, np.int32)
        lib.covis_host_votes(h, p(planes), p(n), sc["cap"], p(flags), p(slots), p(keys), p(bad), nk, nq, p(kind), p(pos), p(qptr), p(qids), p(th), p(skip),
                             p(votes), p(order), p(no), p(best), p(nz))
        out.update(votes=votes.tolist(), order=[order[q, :no[q]].tolist() for q in range(nq)], best=best.tolist(), nz=nz.tolist())
        for q in range(nq):
            assert (order[q, no[q]:] == -1).all()
    if sc["local"] is not None:
        local = np.array(sc["local"] + [0], np.int32)
        pts = np.array((sc["frame_pts"] or []) + [0], np.int32)
        room = max(int(n.sum()), 1)
        ids, seen = np.zeros(room, np.int32), np.zeros(room, np.uint8)
        total = lib.covis_host_local(h, p(planes), p(n), sc["cap"], p(flags), p(local), len(sc["local"]), p(pts), len(sc["frame_pts"] or []), p(ids), p(seen))
        out.update(local_ids=ids[:total].tolist(), seen=seen[:total].tolist())
    if handle is None:
        lib.covis_host_destroy(h)
    return out


SWEEPS = [dict(seed=1, counts=[0, 1, 63, 64, 65, 130], cap=130, capacity=500, nq_slot=6, id_lengths=(0, 1, 64, 65), local=[5, 0, 3, 4], n_frame=40),
          dict(seed=2, counts=[40] * 65, cap=64, capacity=300, nq_slot=20, id_lengths=(200, 30), with_bad_kf=True, local=list(range(64, 0, -3)), n_frame=100),
          dict(seed=3, counts=[25, 30], cap=32, capacity=40, nq_slot=2, id_lengths=(5000,), th=3, local=[1, 0], n_frame=10)]


@pytest.mark.parametrize("make", S.RULE_SCENES + S.PLAIN_SCENES, ids=lambda f: f.__name__)
def test_host_program_answers_the_scenes(host, make):
    sc = make()
    assert host_answer(host, sc) == S.answer(sc)


@pytest.mark.parametrize("kw", SWEEPS, ids=lambda kw: "seed%d" % kw["seed"])
def test_host_program_answers_the_sweeps(host, kw):
    sc = S.random_scene(**kw)
    h = host.covis_host_create(sc["capacity"])
    want = S.answer(sc)
    assert host_answer(host, sc, h) == want
    assert host_answer(host, sc, h) == want  # the stamps of the first pass do not leak into the second
    host.covis_host_destroy(h)
    for total, nl in ((0, 2), (1, 1), (65, 2), (257, 80)):
        sc = S.survivors_scene(total, nl)
        want = S.answer(sc)
        assert len(want["local_ids"]) == total and host_answer(host, sc) == want


# ---- the mirror against the literal toy-map routines ----
def _stand_ins(planes, store):
    def votes_fn(slots, key_ids, queries, kf_bad):
        qs = [("slot", q["slot"]) if "slot" in q else ("ids", list(q["ids"])) for q in queries]
        votes = R.votes(planes, store, slots, qs)
        res = [R.connect(row, key_ids, q.get("th", 15), q.get("skip_bad", False), kf_bad) for q, row in zip(queries, votes)]
        return np.array(votes, np.int32).reshape(len(queries), len(slots)), [np.array(r[0], np.int32) for r in res], [r[1] for r in res], [r[2] for r in res]

    def local_fn(local, frame_pts):
        ids, seen = R.local_points(planes, store, local, frame_pts)
        return np.array(ids, np.int32), np.array(seen, np.uint8)
    return votes_fn, local_fn


def _mirror_of(afv, kfs, planes, store, th):
    class _T:  # the mirror only keeps them
        nsets, cap = len(kfs), 0
    g = afv.CovisibilityGraph(_T(), None, *_stand_ins(planes, store))
    g.TH = th
    for s, kf in enumerate(kfs):
        g.add_keyframe(s, kf.keyId)
        if kf.bad:
            g.set_bad(s)
    return g


@pytest.mark.parametrize("seed", range(8))
def test_mirror_equals_the_toy_map(afv, seed):
    nk = 4 + 3 * seed
    kfs, pts, planes, store = _toy_map(40 + seed, nk=nk, n_feat=30, n_pts=25 * nk // 4, bad_kf=0.15 if seed % 2 else 0.0)
    slot_of = {kf.keyId: s for s, kf in enumerate(kfs)}
    th = 3
    g = _mirror_of(afv, kfs, planes, store, th)
    order = np.random.RandomState(seed).permutation(nk).tolist()
    for s in order[:nk // 2]:  # one by one ...
        kfs[s].UpdateConnections(th)
        g.UpdateConnections(s)
    # ... and as a batch: the planes do not change between the keyframes of a batch, so the snapshot answers as the sequence does
    for s in order[nk // 2:]:
        kfs[s].UpdateConnections(th)
    g.UpdateConnectionsBatch(order[nk // 2:])
    for s, kf in enumerate(kfs):
        assert g.GetVectorCovisibleKeyFrames(s) == [slot_of[o.keyId] for o in kf.orderedConnectedKeyFrames], s
        assert g.kf[s].ordered_w == kf.orderedWeights
        assert {g.kf[o].key_id: w for o, w in g.kf[s].weights.items()} == kf.connectedKeyFrameWeights
        assert g.GetConnectedKeyFrames(s) == [slot_of[k] for k in sorted(kf.connectedKeyFrameWeights)]
        assert g.GetParent(s) == (None if kf.mpParent is None else slot_of[kf.mpParent.keyId])
        assert g.GetChilds(s) == sorted(slot_of[c.keyId] for c in kf.mspChildrens)
        assert g.GetBestCovisibilityKeyFrames(s, 3) == [slot_of[o.keyId] for o in kf.GetBestCovisibilityKeyFrames(3)]
        for o in range(nk):
            assert g.GetWeight(s, o) == kf.connectedKeyFrameWeights.get(kfs[o].keyId, 0)
    assert g.kf[0].parent is None  # keyId 0 never takes a parent
    d = g.essential_graph_dict(min_feat=4)
    for s, kf in enumerate(kfs):
        if kf.bad:
            assert kf.keyId not in d["parent"]
            continue
        assert d["parent"][kf.keyId] == (None if kf.mpParent is None else kf.mpParent.keyId)
        n = sum(1 for w in kf.orderedWeights if w >= 4)
        assert d["covisibles"][kf.keyId] == ([] if n == len(kf.orderedWeights) else [o.keyId for o in kf.orderedConnectedKeyFrames[:n]])
    # the local map of a few frames, with a small keyframe limit so that the size test and the breaks are met
    rng = np.random.RandomState(900 + seed)
    for trial in range(6):
        frame = [None if rng.rand() < 0.3 else pts[rng.randint(0, len(pts))] for _ in range(12)]
        frame_ids = [-1 if p is None else p.ptId for p in frame]
        limit = [80, 3, 1][trial % 3]
        want = R.toy_update_local_map(frame, max_keyframes=limit, best_cov=2)
        got = g.UpdateLocalMap(frame_ids, max_keyframes=limit, best_cov=2)
        if want is None:
            assert got is None
            continue
        local, ref, lpts, seen = want
        assert got[0] == [slot_of[kf.keyId] for kf in local]
        assert got[1] == (None if ref is None else slot_of[ref.keyId])
        assert got[2].tolist() == [p.ptId for p in lpts] and got[3].tolist() == seen


def test_erase_connection_and_quirks(afv):
    kfs, pts, planes, store = _toy_map(7, nk=6, n_feat=30, n_pts=30)
    g = _mirror_of(afv, kfs, planes, store, 2)
    g.UpdateConnectionsBatch(range(6))
    s = 1
    full = g.GetVectorCovisibleKeyFrames(s)
    assert len(full) >= 2
    # GetWeight answers from the whole counter, GetVectorCovisibleKeyFrames from the entries at the threshold
    assert set(full) <= set(g.GetConnectedKeyFrames(s))
    g.EraseConnection(s, full[0])
    assert full[0] not in g.GetConnectedKeyFrames(s) and g.GetWeight(s, full[0]) == 0
    # upper_bound's end(): every weight reaches w -> empty
    assert g.GetCovisiblesByWeight(s, 0) == []
    with pytest.raises(ValueError):
        g.add_keyframe(1, 99)
    with pytest.raises(ValueError):
        g.add_keyframe(17, g.kf[2].key_id)


def test_essential_graph_dict_feeds_the_edge_list(afv):
    """essential_graph_dict -> essgraph.essential_graph_edges: the edge list equals the one built from the toy map's own members"""
    kfs, pts, planes, store = _toy_map(11, nk=10, n_feat=40, n_pts=45, bad_kf=0.0)
    kfs[4].bad = True
    g = _mirror_of(afv, kfs, planes, store, 3)
    for kf in kfs:
        kf.UpdateConnections(3)
    g.UpdateConnectionsBatch(range(len(kfs)))
    g.AddLoopEdge(9, 1)
    g.AddLoopEdge(1, 9)
    live = [kf for kf in kfs if not kf.bad]
    ident = (np.eye(3), np.zeros(3), 1.0)
    Scw = {kf.keyId: ident for kf in live}
    min_feat = 12

    def by_weight(kf):
        n = sum(1 for w in kf.orderedWeights if w >= min_feat)
        return [] if n == len(kf.orderedWeights) else [o.keyId for o in kf.orderedConnectedKeyFrames[:n]]
    want = afv.essgraph.essential_graph_edges([kf.keyId for kf in live], {kf.keyId: None if kf.mpParent is None else kf.mpParent.keyId for kf in live},
                                              {kfs[9].keyId: [kfs[1].keyId], kfs[1].keyId: [kfs[9].keyId]}, {kf.keyId: by_weight(kf) for kf in live}, {}, Scw, {},
                                              kfs[1].keyId, kfs[9].keyId, min_feat)
    d = g.essential_graph_dict(min_feat)
    got = afv.essgraph.essential_graph_edges(sorted(d["parent"]), d["parent"], d["loop_edges"], d["covisibles"], {}, Scw, {}, kfs[1].keyId, kfs[9].keyId,
                                             min_feat)
    assert [(i, j) for i, j, _ in got] == [(i, j) for i, j, _ in want] and len(got) >= len(live)
    assert kfs[4].keyId not in d["parent"] and any(d["covisibles"].values())
