"""-m gpu: afv_table_covis_votes and afv_table_local_points (include/afv_covis.h) against the restatement tests/_covis_ref.py, integer for
integer: the constructed scenes, the sizes at the wavefront / workgroup / chunk edges, every refusal with outputs and store unchanged, a
cloned table, a fresh context and painted scratch (this file carries that coverage for the two entry points: they are declared outside
afv_hip.h, so tests/_scratch_cases.py has no row for them), and the chain UpdateConnections -> UpdateLocalMap -> SearchLocalPoints."""
import ctypes as C

import numpy as np
import pytest

import _covis_ref as R
import _covis_scenes as S

pytestmark = pytest.mark.gpu


class Rig:
    """a scene on the device: a table whose slots hold the planes (their rows are zeros: nothing here reads them) and the store's flags"""

    def __init__(self, afv, ctx, sc):
        self.table = afv.table.DescriptorTable(ctx, sc["nsets"], sc["cap"])
        self.points = afv.MapPoints(ctx, sc["capacity"])
        for s, plane in sc["planes"].items():
            self.table.set(s, np.zeros((len(plane), 32), np.uint8))
            self.table.set_map_points(s, plane)
        if sc["set"]:
            self.points.set(sc["set"], pos=np.zeros((len(sc["set"]), 3), np.float32))
        if sc["bad"]:
            self.points.set_flags(sc["bad"], bad=np.ones(len(sc["bad"]), np.uint8))

    def close(self):
        self.table.close()
        self.points.close()


def device_answer(afv, rig, sc, table=None):
    t = table or rig.table
    out = {}
    if sc["queries"]:
        votes, order, best, nz = afv.covisibility_votes(t, rig.points, sc["slots"], sc["key_ids"], sc["queries"], sc["kf_bad"])
        out.update(votes=votes.tolist(), order=[o.tolist() for o in order], best=best.tolist(), nz=nz.tolist())
    if sc["local"] is not None:
        ids, seen = afv.local_points(t, rig.points, sc["local"], sc["frame_pts"])
        out.update(local_ids=ids.tolist(), seen=[0] * len(ids) if seen is None else seen.tolist())
    return out


def check_scene(afv, ctx, sc, twice=False):
    want = S.answer(sc)
    rig = Rig(afv, ctx, sc)
    try:
        got = device_answer(afv, rig, sc)
        assert got == want, sc["name"]
        if twice:
            assert device_answer(afv, rig, sc) == want, (sc["name"], "second call")
    finally:
        rig.close()
    return want


@pytest.mark.parametrize("make", S.RULE_SCENES + S.PLAIN_SCENES, ids=lambda f: f.__name__)
def test_constructed_scene(afv, gpu_ctx, make):
    check_scene(afv, gpu_ctx, make(), twice=True)


def test_features_per_slot_at_the_edges(afv, gpu_ctx):
    """0, 1, 63, 64, 65 and cap features; ids queries of 0, 1, 64, 65 and 5000 entries (longer than cap) beside slot queries"""
    sc = S.random_scene(11, counts=[0, 1, 63, 64, 65, 130], cap=130, capacity=700, nq_slot=6, id_lengths=(0, 1, 64, 65, 5000), th=15, with_bad_kf=True,
                        local=[5, 0, 1, 4, 2, 3], n_frame=200)
    want = check_scene(afv, gpu_ctx, sc, twice=True)
    assert max(max(r) for r in want["votes"]) >= 15 and len(sc["queries"]) == 11


@pytest.mark.parametrize("nk,nq_slot,id_lengths", [(1, 1, ()), (2, 2, (3, 70, 0, 130, 9)), (63, 40, (100,) * 24), (64, 3, (64, 65, 1, 300)), (65, 0, (257,)),
                                                    (300, 32, (5000, 10) + (130,) * 30)], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_keyframe_and_query_counts(afv, gpu_ctx, nk, nq_slot, id_lengths):
    """nk 1, 2, 63, 64, 65, 300 with nq 1, 7, 64, 7, 1, 64; slot and ids queries mixed, slots listed against the order of the keyIds"""
    rng = np.random.RandomState(nk)
    sc = S.random_scene(20 + nk, counts=rng.randint(0, 131, nk).tolist(), cap=130, capacity=900, nq_slot=nq_slot, id_lengths=id_lengths, th=15,
                        with_bad_kf=nk > 2, pool=400)
    assert len(sc["queries"]) in (1, 7, 64)
    want = check_scene(afv, gpu_ctx, sc)
    if nk >= 63:
        assert any(len(o) > 1 for o in want["order"])
        assert any(len(set(r[p] for p in o)) < len(o) for r, o in zip(want["votes"], want["order"]) if len(o) > 1)  # tied votes in an order


def test_table_of_4096_features_and_a_query_of_65536(afv, gpu_ctx):
    """a plane of 4096 distinct ids fills the set of k_covis_votes to its design load; the ids share their low four bits"""
    capacity = 70000
    rng = np.random.RandomState(5)
    p0 = (rng.permutation(4096) * 16 + 3).tolist()
    p1 = list(range(4000))
    sc = S._scene("cap4096", {0: p0, 1: p1, 2: [capacity - 1, 0, 3]}, capacity, set(p0) | set(p1) | {capacity - 1}, bad=p0[:50] + p1[100:140],
                  queries=[{"slot": 0, "th": 15}, {"slot": 1, "th": 15}, {"ids": rng.randint(-1, capacity, 65536).tolist(), "th": 15}],
                  local=[2, 1, 0], frame_pts=rng.randint(-1, capacity, 3000).tolist(), cap=4096)
    want = check_scene(afv, gpu_ctx, sc)
    assert want["votes"][0][1] > 100 and len(want["local_ids"]) > 7000


@pytest.mark.parametrize("total,nl", [(0, 0), (0, 2), (1, 1), (64, 1), (65, 2), (256, 80), (257, 80), (1024, 256), (1025, 256)])
def test_local_points_totals(afv, gpu_ctx, total, nl):
    sc = S.survivors_scene(total, nl)
    want = check_scene(afv, gpu_ctx, sc, twice=True)
    assert len(want["local_ids"]) == total


def _raw_local(afv, rig, local, pts, max_out, paint=77):
    lib = afv.covisibility.bind()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    local = np.asarray(local, np.int32)
    pts = None if pts is None else np.asarray(pts, np.int32)
    ids, seen = np.full(max(max_out, 1) + 8, paint, np.int32), np.full(max(max_out, 1) + 8, paint, np.uint8)
    n = C.c_int32(paint)
    rc = lib.afv_table_local_points(rig.table.handle, rig.points.handle, p(local), len(local), p(pts), 0 if pts is None else len(pts), max_out, p(ids), p(seen),
                                    C.byref(n))
    return rc, ids, seen, n.value


def test_local_points_capacity(afv, gpu_ctx):
    """a total beyond max_out: AFV_ECAPACITY, the painted outputs unchanged; the words are at rest: the same call with room answers as the
    restatement, twice, and so does a call after a refused one"""
    sc = S.survivors_scene(257, 80)
    want = S.answer(sc)
    rig = Rig(afv, gpu_ctx, sc)
    L = afv._lib
    try:
        for max_out in (256, 0, 100):
            rc, ids, seen, n = _raw_local(afv, rig, sc["local"], sc["frame_pts"], max_out)
            assert rc == L.ECAPACITY and (ids == 77).all() and (seen == 77).all() and n == 77, max_out
        for max_out in (257, 300):
            rc, ids, seen, n = _raw_local(afv, rig, sc["local"], sc["frame_pts"], max_out)
            assert rc == 0 and n == 257 and ids[:n].tolist() == want["local_ids"] and seen[:n].tolist() == want["seen"]
            assert (ids[n:] == 77).all() and (seen[n:] == 77).all()
        rc, ids, seen, n = _raw_local(afv, rig, [0, 0], None, 300)  # refused: a slot listed twice
        assert rc == L.EINVAL and (ids == 77).all() and n == 77
        assert device_answer(afv, rig, sc) == want
    finally:
        rig.close()


def _raw_votes(afv, rig, slots, keys, bad, queries, nk=None, nq=None, struct_size=None, points=None, table=None, null=()):
    cv = afv.covisibility
    lib = cv.bind()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    slots, keys = np.asarray(slots, np.int32), np.asarray(keys, np.int32)
    bad = None if bad is None else np.asarray(bad, np.uint8)
    recs = (cv.CovisQuery * max(len(queries), 1))()
    keep = []
    for r, q in zip(recs, queries):
        r.struct_size = C.sizeof(cv.CovisQuery) if struct_size is None else struct_size
        r.th, r.skip_bad = q.get("th", 15), q.get("skip_bad", 0)
        r.kind = q.get("kind", cv.QUERY_SLOT if "slot" in q else cv.QUERY_IDS)
        if "slot" in q:
            r.position = q["slot"]
        else:
            a = np.asarray(q["ids"], np.int32)
            keep.append(a)
            r.n, r.ids = q.get("n", len(a)), a.ctypes.data
    nk, nq = len(slots) if nk is None else nk, len(queries) if nq is None else nq
    cells = max(len(slots) * len(queries), 1) + 4
    outs = {k: np.full(cells, 77, np.int32) for k in ("votes", "order", "n_order", "best", "n_nonzero")}
    args = {k: (None if k in null else p(v)) for k, v in outs.items()}
    rc = lib.afv_table_covis_votes((table or rig.table).handle, (points or rig.points).handle, None if "slots" in null else p(slots),
                                   None if "key_id" in null else p(keys), p(bad), nk, None if "queries" in null else recs, nq, args["votes"], args["order"],
                                   args["n_order"], args["best"], args["n_nonzero"])
    return rc, outs


def test_refusals_leave_outputs_and_store_unchanged(afv, gpu_ctx):
    sc = S.good_filter()
    want = S.answer(sc)
    rig = Rig(afv, gpu_ctx, sc)
    L = afv._lib
    other_ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = afv.MapPoints(other_ctx, sc["capacity"])
    no_plane = afv.table.DescriptorTable(gpu_ctx, 3, 8)
    try:
        for s in range(3):
            no_plane.set(s, np.zeros((2, 32), np.uint8))
        no_plane.set_map_points(0, [1, 2])  # slots 1 and 2 have no plane
        ok = dict(slots=[0, 1, 2], keys=[5, 6, 7], bad=None, queries=[{"slot": 0}, {"ids": [1, 2, -1]}])
        rc, outs = _raw_votes(afv, rig, **ok)
        assert rc == 0 and (outs["votes"][:6] != 77).all() and (outs["votes"][6:] == 77).all()
        rc, outs = _raw_votes(afv, rig, **dict(ok, null=("votes", "order")))
        assert rc == 0 and (outs["best"][:2] != 77).all()
        refused = [dict(ok, null=("slots",)), dict(ok, null=("key_id",)), dict(ok, null=("queries",)), dict(ok, null=("n_order",)), dict(ok, null=("best",)),
                   dict(ok, null=("n_nonzero",)), dict(ok, nk=0), dict(ok, nk=4097), dict(ok, nq=0), dict(ok, nq=65),
                   dict(ok, slots=[0, 1, 3]), dict(ok, slots=[0, -1, 2]), dict(ok, slots=[0, 1, 1]), dict(ok, keys=[5, 6, 5]),
                   dict(ok, queries=[{"slot": 3}]), dict(ok, queries=[{"slot": -1}]), dict(ok, queries=[{"ids": [16]}]), dict(ok, queries=[{"ids": [-2]}]),
                   dict(ok, queries=[{"ids": [1], "n": 65537}]), dict(ok, queries=[{"ids": [1], "n": -1}]), dict(ok, queries=[{"ids": [1], "kind": 2}]),
                   dict(ok, struct_size=0), dict(ok, struct_size=16), dict(ok, struct_size=30), dict(ok, queries=[{"ids": [1], "skip_bad": 1}]),
                   dict(ok, queries=[{"ids": [1], "skip_bad": 2}], bad=[0, 0, 0]), dict(ok, points=foreign), dict(ok, table=no_plane)]
        for kw in refused:
            rc, outs = _raw_votes(afv, rig, **kw)
            assert rc == L.EINVAL, kw
            for k, a in outs.items():
                assert (a == 77).all(), (kw, k)
        # local points
        for local, pts, max_out, kw in (([0, 3], None, 50, {}), ([0, -1], None, 50, {}), ([1, 1], None, 50, {}), ([0], [16], 50, {}), ([0], [-2], 50, {}),
                                        ([0], None, -1, {}), ([0], [1] * 65537, 50, {})):
            rc, ids, seen, n = _raw_local(afv, rig, local, pts, max_out)
            assert rc == L.EINVAL and (ids == 77).all() and (seen == 77).all() and n == 77, (local, pts, max_out)
        lib = afv.covisibility.bind()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        one, ids, n = np.zeros(1, np.int32), np.full(8, 77, np.int32), C.c_int32(77)
        assert lib.afv_table_local_points(rig.table.handle, rig.points.handle, p(one), 1, None, 0, 8, p(ids), None, None) == L.EINVAL          # n_out
        assert lib.afv_table_local_points(rig.table.handle, rig.points.handle, None, 1, None, 0, 8, p(ids), None, C.byref(n)) == L.EINVAL       # local
        assert lib.afv_table_local_points(rig.table.handle, rig.points.handle, p(one), 1, None, 0, 8, None, None, C.byref(n)) == L.EINVAL       # ids_out
        assert lib.afv_table_local_points(rig.table.handle, rig.points.handle, p(one), 1, None, 3, 8, p(ids), None, C.byref(n)) == L.EINVAL     # frame_pts
        assert lib.afv_table_local_points(rig.table.handle, foreign.handle, p(one), 1, None, 0, 8, p(ids), None, C.byref(n)) == L.EINVAL
        assert lib.afv_table_local_points(no_plane.handle, rig.points.handle, p(np.array([1], np.int32)), 1, None, 0, 8, p(ids), None, C.byref(n)) == L.EINVAL
        assert (ids == 77).all() and n.value == 77
        assert lib.afv_table_local_points(rig.table.handle, rig.points.handle, None, 0, None, 0, 0, None, None, C.byref(n)) == 0 and n.value == 0  # nl = 0
        # nl beyond AFV_COVIS_MAX_LOCAL: 257 distinct slots that all hold a plane, so nothing else refuses the call; 256 of them pass
        wide = afv.table.DescriptorTable(gpu_ctx, 257, 2)
        try:
            for s in range(257):
                wide.set(s, np.zeros((1, 32), np.uint8))
                wide.set_map_points(s, [s % 3])
            many = np.arange(257, dtype=np.int32)
            ids = np.full(300, 77, np.int32)
            assert lib.afv_table_local_points(wide.handle, rig.points.handle, p(many), 257, None, 0, 300, p(ids), None, C.byref(n)) == L.EINVAL
            assert (ids == 77).all() and n.value == 0
            assert lib.afv_table_local_points(wide.handle, rig.points.handle, p(many), 256, None, 0, 300, p(ids), None, C.byref(n)) == 0
            assert n.value == 3 and ids[:3].tolist() == [0, 1, 2] and (ids[3:] == 77).all()
        finally:
            wide.close()
        # the store and the planes are as they were: every answer again
        assert device_answer(afv, rig, sc) == want
    finally:
        no_plane.close()
        foreign.close()
        other_ctx.close()
        rig.close()


def test_cloned_table(afv, gpu_ctx):
    sc = S.random_scene(31, counts=[50, 0, 64, 20, 33], cap=64, capacity=200, nq_slot=5, id_lengths=(40,), th=3, local=[4, 2, 0], n_frame=30)
    want = S.answer(sc)
    rig = Rig(afv, gpu_ctx, sc)
    other = afv.table.DescriptorTable(gpu_ctx, sc["nsets"], sc["cap"])
    try:
        rig.table.clone_into(other)
        assert device_answer(afv, rig, sc, table=other) == want
        other.set_map_points(2, [-1] * 64)  # the clone has planes of its own
        assert device_answer(afv, rig, sc) == want
        assert device_answer(afv, rig, sc, table=other) != want
    finally:
        other.close()
        rig.close()


def test_fresh_context_and_painted_scratch(afv):
    """both entry points on a context of their own: the first call (the buffers grow inside it, the store's words are made), then after the
    scratch is painted 0xA5 and 0x5A - as ints neither -1 nor 0 nor an id - with the sizes unchanged and the zero-at-rest words zero"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sc = S.random_scene(41, counts=[130, 0, 65, 64, 1, 90, 130, 17], cap=130, capacity=600, nq_slot=8, id_lengths=(0, 300, 64), th=15, with_bad_kf=True,
                        local=[6, 0, 2, 5, 7], n_frame=150)
    want = S.answer(sc)
    ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    rig = Rig(afv, ctx, sc)
    try:
        sizes = None
        for what, byte in (("fresh", None), ("painted 0xA5", 0xA5), ("painted 0x5A", 0x5A)):
            if byte is not None:
                sizes = ctx.scratch_bytes()
                assert sizes[0] > 0 and sizes[1] > 0
                ctx.paint_scratch(byte)
            assert device_answer(afv, rig, sc) == want, what
            assert ctx.rest_words() == 0, what
            if byte is not None:
                assert ctx.scratch_bytes() == sizes, what
        # the local points first on another fresh context: nothing of the votes call is needed by it
        ctx2 = afv.Context(max_width=640, max_height=480, max_batch=1)
        rig2 = Rig(afv, ctx2, sc)
        try:
            ids, seen = afv.local_points(rig2.table, rig2.points, sc["local"], sc["frame_pts"])
            assert ids.tolist() == want["local_ids"] and seen.tolist() == want["seen"]
        finally:
            rig2.close()
            ctx2.close()
    finally:
        rig.close()
        ctx.close()


def test_raw_order_rows_end_in_minus_one(afv, gpu_ctx):
    sc = S.order_ties()
    rig = Rig(afv, gpu_ctx, sc)
    try:
        rc, outs = _raw_votes(afv, rig, sc["slots"], sc["key_ids"], None, sc["queries"])
        assert rc == 0 and outs["order"][:5].tolist() == [3, 2, 1, -1, -1] and outs["n_order"][0] == 3 and outs["n_nonzero"][0] == 4
    finally:
        rig.close()


def test_chain_connections_local_map_search(afv, gpu_ctx):
    """a small seeded map: UpdateConnections of every keyframe, UpdateLocalMap of a frame, Frame.SearchLocalPoints over the local ids - against
    the literal toy-map routines and the search over the list they build"""
    import _points_ref as PR
    import _points_scenes as PS
    ps = PS.random_scene(1, PR.FRUSTUM)
    P, cam, f = ps.P, ps.cam, ps.feat
    set_ids = np.flatnonzero(P.flags & PR.SET)
    rng = np.random.RandomState(3)
    nk, n_feat = 12, 60
    # the toy map and the planes that agree with it
    toy_pts = {int(i): R.ToyPoint(int(i)) for i in set_ids}
    for i, pt in toy_pts.items():
        pt.bad = bool(P.flags[i] & PR.BAD)
    kfs = [R.ToyKeyFrame(0 if s == 0 else 3 * s + 1, n_feat) for s in range(nk)]
    for s, kf in enumerate(kfs):
        near = set_ids[(np.arange(len(set_ids)) + s * len(set_ids) // nk) % len(set_ids)][:len(set_ids) // 2]  # neighbours share points
        for idx in range(n_feat):
            if rng.rand() < 0.8:
                kf.AddMapPoint(toy_pts[int(near[rng.randint(0, len(near))])], idx)
    kfs[5].bad = True
    table = afv.table.DescriptorTable(gpu_ctx, nk, n_feat)
    points = afv.MapPoints(gpu_ctx, P.capacity, desc_bytes=P.desc_bytes)
    points.set(set_ids, pos=P.pos[set_ids], normal=P.normal[set_ids], min_distance=P.min_distance[set_ids], max_distance=P.max_distance[set_ids],
               ref_size=P.ref_size[set_ids], ref_distance=P.ref_distance[set_ids], ref_sigma=P.ref_sigma[set_ids])
    points.set_flags(set_ids, bad=(P.flags[set_ids] & PR.BAD) != 0, observed=(P.flags[set_ids] & PR.OBSERVED) != 0)
    points.set_descriptors(set_ids, P.descriptors[set_ids])
    frame = afv.Frame(gpu_ctx, max_x=PS.W, max_y=PS.H, cap=f.n)
    afv.FeatureMatcher.setDescriptorDistanceThresholds(ps.th)
    try:
        for s, kf in enumerate(kfs):
            table.set(s, np.zeros((n_feat, 32), np.uint8))
            table.set_map_points(s, [-1 if p is None else p.ptId for p in kf.mvpMapPoints])
        g = afv.CovisibilityGraph(table, points)
        g.TH = 6
        for s, kf in enumerate(kfs):
            g.add_keyframe(s, kf.keyId)
        g.set_bad(5)
        for kf in kfs:
            kf.UpdateConnections(6)
        g.UpdateConnectionsBatch(range(nk))
        slot_of = {kf.keyId: s for s, kf in enumerate(kfs)}
        for s, kf in enumerate(kfs):
            assert g.GetVectorCovisibleKeyFrames(s) == [slot_of[o.keyId] for o in kf.orderedConnectedKeyFrames]
            assert g.kf[s].ordered_w == kf.orderedWeights and g.GetParent(s) == (None if kf.mpParent is None else slot_of[kf.mpParent.keyId])
        assert sum(len(kf.orderedConnectedKeyFrames) for kf in kfs) > nk
        frame_ids = [int(i) if rng.rand() < 0.7 else -1 for i in set_ids[rng.randint(0, len(set_ids), 40)]]
        want = R.toy_update_local_map([toy_pts.get(i) for i in frame_ids], max_keyframes=80, best_cov=3)
        local, ref, ids, seen = g.UpdateLocalMap(frame_ids, max_keyframes=80, best_cov=3)
        assert local == [slot_of[kf.keyId] for kf in want[0]] and ref == slot_of[want[1].keyId] and 5 not in local
        want_ids = [p.ptId for p in want[2]]
        assert ids.tolist() == want_ids and seen.tolist() == want[3] and 0 < sum(want[3]) < len(want_ids)
        kps = np.zeros(f.n, afv.KP_DTYPE)
        kps["x"], kps["y"], kps["angle"] = f.x, f.y, f.angles
        frame.set_features(kps, f.desc, sizes=f.sizes, u_right=f.u_right)
        frame.set_pose(cam.Rcw, cam.tcw, cam.Ow, cam.fx, cam.fy, cam.cx, cam.cy, cam.mbf)
        m = afv.FeatureMatcher(ps.nnratio, False, ctx=gpu_ctx)
        a = frame.SearchLocalPoints(m, points, ids, ps.radius_th, ps.cos_limit)
        b = frame.SearchLocalPoints(m, points, np.array(want_ids, np.int32), ps.radius_th, ps.cos_limit)
        assert np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        frame.close()
        table.close()
        points.close()


def test_graph_feeds_the_keyframe_database(afv, gpu_ctx):
    """KeyFrameDatabase.DetectLoopCandidates / DetectRelocalizationCandidates take the graph's answers as they come: connected(slot) as the
    list, best_covisibles as the callable - the same candidates as with lists and a function made from the literal toy map"""
    rng = np.random.RandomState(9)
    nk, n_feat = 10, 40
    pts = [R.ToyPoint(i) for i in range(60)]
    kfs = [R.ToyKeyFrame(0 if s == 0 else 2 * s + 1, n_feat) for s in range(nk)]
    for s, kf in enumerate(kfs):
        for idx in range(n_feat):  # keyframes 0 .. 4 and 5 .. 9 share points among themselves only: the far half holds the loop candidates
            kf.AddMapPoint(pts[(0 if s < 5 else 30) + rng.randint(0, 30)], idx)
    table = afv.table.DescriptorTable(gpu_ctx, nk, n_feat)
    points = afv.MapPoints(gpu_ctx, 60)
    try:
        points.set(np.arange(60), pos=np.zeros((60, 3), np.float32))
        for s, kf in enumerate(kfs):
            table.set(s, np.zeros((n_feat, 32), np.uint8))
            table.set_map_points(s, [p.ptId for p in kf.mvpMapPoints])
            words = np.unique(rng.randint(0, 50, 30))  # every keyframe shares words with every other
            value = rng.rand(len(words))
            if s == 2:
                twin = (words, value)
            if s == 7:  # the BowVector of keyframe 2 again: the one score no connected keyframe can beat
                words, value = twin
            table.set_bowvec(s, words, value / value.sum())
        g = afv.CovisibilityGraph(table, points)
        g.TH = 5
        db = afv.KeyFrameDatabase(table)
        for s, kf in enumerate(kfs):
            g.add_keyframe(s, kf.keyId)
            db.add(s)
            kf.UpdateConnections(5)
        g.UpdateConnectionsBatch(range(nk))
        slot_of = {kf.keyId: s for s, kf in enumerate(kfs)}
        toy_connected = lambda s: [slot_of[k] for k in sorted(kfs[s].connectedKeyFrameWeights)]
        toy_best = lambda s: [slot_of[o.keyId] for o in kfs[s].GetBestCovisibilityKeyFrames(10)]
        assert g.connected(2) == toy_connected(2) and set(g.connected(2)) == {0, 1, 3, 4}
        min_score = db.min_score_to_connected(2, g.connected(2))
        got = db.DetectLoopCandidates(2, min_score, g.connected(2), g.best_covisibles)
        want = db.DetectLoopCandidates(2, min_score, toy_connected(2), toy_best)
        assert got == want and 7 in got and not set(got) & set(g.connected(2))  # (the database masks the connected list, nothing else)
        assert db.DetectRelocalizationCandidates(7, g.best_covisibles) == db.DetectRelocalizationCandidates(7, toy_best)
    finally:
        table.close()
        points.close()
