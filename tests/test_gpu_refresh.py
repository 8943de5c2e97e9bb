"""-m gpu: afv_table_refresh_points (csrc/k_refresh.hip) against the restatement (tests/_refresh_ref.py), bit for bit: the status, the
winning observation and its median, and every plane and row of the store read back through afv_points_get - of the points the call
names and of those it does not.  Every rule of tests/_refresh_scenes.py on tables of 32 and 61 bytes and of 128 and 36 floats, the
three combinations of the two parts, observation counts around the chunk of 64 rows and the LDS limit, point counts around the
workgroup of four, afv_distinctive_descriptors on the same rows from the host, points written by DescriptorTable.triangulate as a
fixed point, the chain LocalBundleAdjustment -> RefreshAfterBundleAdjustment -> SearchLocalPoints, and every refusal that needs a table
and a store.  Nothing here provokes a fault: every input is handled by rule."""
import ctypes as C
import functools

import numpy as np
import pytest

import _refresh_ref as R
import _refresh_scenes as S

pytestmark = pytest.mark.gpu
FIELDS = ("pos", "normal", "min_distance", "max_distance", "ref_size", "ref_distance", "ref_sigma", "flags", "descriptors")
PARTS = {"both": (True, True), "descriptors": (True, False), "normals": (False, True)}


@functools.lru_cache(maxsize=None)
def reference(maker, kind, args=(), parts=(True, True)):
    """a scene and the restatement's answer, computed once and shared"""
    sc = getattr(S, maker)(kind, *args)
    return sc, R.refresh(sc, *parts)


class Rig:
    """a scene installed in a table (slot = the scene's slot) and a store (id = the scene's id; an id the scene leaves unset is not written)"""

    def __init__(self, afv, ctx, sc):
        kind = {"float_dim": sc.float_dim} if sc.float_dim else {"desc_bytes": sc.desc_bytes}
        self.sc = sc
        self.table = afv.table.DescriptorTable(ctx, sc.nslots, sc.cap, **kind)
        self.points = afv.MapPoints(ctx, max(sc.store) + 2, **kind)
        for s in range(sc.nslots):
            self.table.set(s, sc.table_rows(s))
            self.table.set_geometry(s, sc.x[s], sc.y[s], sc.sigma2[s])
            self.table.set_scale(s, sc.size[s])
        if not sc.float_dim and sc.pitch != sc.desc_bytes:
            # afv_table_set zero-pads: the scene's pad bytes are written into the device rows themselves, through the table's own view
            import torch
            torch.cuda.synchronize()
            rows = self.table.device_views()[0]
            for s in range(sc.nslots):
                rows[s, :sc.cap].copy_(torch.from_numpy(sc.rows[s]))
            torch.cuda.synchronize()
        ids = np.array([i for i in sorted(sc.store) if sc.store[i]["flags"] & R.SET], np.int32)
        a = sc.store_arrays(ids)
        self.points.set(ids, **{k: a[k] for k in FIELDS[:7]})
        self.points.set_flags(ids, bad=(a["flags"] & R.BAD) != 0, observed=(a["flags"] & R.OBSERVED) != 0)
        self.points.set_descriptors(ids, a["descriptors"])
        self.set_ids = ids
        self.all_ids = np.arange(self.points.capacity, dtype=np.int32)
        self.before = self.points.get(self.all_ids)

    def close(self):
        self.points.close()
        self.table.close()

    def refresh(self, afv, descriptors=True, normals=True):
        sc = self.sc
        return afv.RefreshMapPoints(self.table, self.points, sc.kfs, sc.centres, sc.max_size, sc.point_ids, sc.ref_kf, sc.observations,
                                    kf_bad=sc.kf_bad, descriptors=descriptors, normals=normals)

    def assert_store(self, want_store, what):
        """every set id of the scene holds the restatement's fields; every other id of the store is as it was"""
        after = self.points.get(self.all_ids)
        named = np.zeros(self.points.capacity, bool)
        for i in self.set_ids:
            named[i] = True
            for k in FIELDS:
                got, want = after[k][i], np.asarray(want_store[int(i)][k])
                assert np.asarray(got, want.dtype).tobytes() == want.tobytes(), (what, int(i), k, got, want)
        for k in FIELDS:
            assert after[k][~named].tobytes() == self.before[k][~named].tobytes(), (what, k, "an id the scene does not hold changed")


def check(afv, ctx, sc, want, parts, what):
    rig = Rig(afv, ctx, sc)
    try:
        status, best, med = rig.refresh(afv, *parts)
        w_status, w_best, w_med, w_store = want
        for i, pid in enumerate(sc.point_ids):   # a failure names its point
            assert status[i] == w_status[i] and best[i] == w_best[i], (what, pid, status[i], w_status[i], best[i], w_best[i])
        assert med.tobytes() == w_med.tobytes(), (what, med, w_med)
        rig.assert_store(w_store, what)
    finally:
        rig.close()


@pytest.mark.parametrize("parts", sorted(PARTS))
@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_every_rule_against_the_restatement(afv, gpu_ctx, kind, parts):
    """... the ids 100 - 102 of the store, which the call does not name, included"""
    sc, want = reference("rule_scene", kind, (), PARTS[parts])
    check(afv, gpu_ctx, sc, want, PARTS[parts], (kind, parts))


def test_pad_bytes_that_differ_on_the_device_are_not_counted(afv, gpu_ctx):
    """the 61-byte table holds rows whose bytes 61 .. 63 differ ON THE DEVICE (the Rig writes them through the table's view): the call
    still picks row 0 with the restatement's median, and the store receives that row; the same 64 bytes counted in full - the host-rows
    form on rows of 64 bytes - pick row 1"""
    kind = ("bytes", 61)
    sc, want = reference("rule_scene", kind, (), PARTS["descriptors"])
    pid = sc.rule["pad_bytes_differ"]
    at = sc.point_ids.index(pid)
    mine = [(e, o) for e, o in enumerate(sc.observations) if o[0] == pid]
    rig = Rig(afv, gpu_ctx, sc)
    try:
        on_device = rig.table.device_views()[0].cpu().numpy()
        pads = [on_device[s, i, 61:].tolist() for _, (_, s, i) in mine]
        assert pads == [[255] * 3, [0] * 3, [0] * 3, [0x0f] * 3]
        status, best, med = rig.refresh(afv, True, False)
        assert best[at] == mine[0][0] == want[1][at] and med[at] == want[2][at] == 0
        s0, i0 = mine[0][1][1:]
        assert rig.points.get([pid])["descriptors"][0].tobytes() == sc.rows[s0][i0, :61].tobytes()
        counted, _ = afv.ComputeDistinctiveDescriptors(gpu_ctx, [np.stack([on_device[s, i] for _, (_, s, i) in mine])])
        assert counted[0] == 1
    finally:
        rig.close()


COUNTS = (1, 2, 3, 4, 63, 64, 65, 129)


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_observation_counts_around_the_row_chunk_and_the_lds_limit(afv, gpu_ctx, kind):
    """1, 2, 3, 4, 63, 64, 65 and 129 observations: that many terms of the normal and, every fourth keyframe of a long list being bad,
    three quarters as many rows; then without a bad keyframe, that many rows"""
    sc, want = reference("sized_scene", kind, (COUNTS,))
    check(afv, gpu_ctx, sc, want, (True, True), kind)
    sc2 = S.sized_scene(kind, COUNTS)
    sc2.kf_bad = []                               # ... and 63, 64, 65 and 129 good rows
    check(afv, gpu_ctx, sc2, R.refresh(sc2, True, False), (True, False), (kind, "no bad keyframe"))


@pytest.mark.parametrize("npts,kind", [(1, S.KINDS[0]), (4, S.KINDS[0]), (5, S.KINDS[0]), (257, S.KINDS[0]), (5, S.KINDS[3]), (257, S.KINDS[1])])
def test_point_counts_with_a_ragged_last_workgroup(afv, gpu_ctx, npts, kind):
    sc, want = reference("sized_scene", kind, (tuple(1 + (p * 7) % 6 for p in range(npts)), 13))
    check(afv, gpu_ctx, sc, want, (True, True), (npts, kind))


@pytest.mark.parametrize("kind", S.KINDS, ids=S.KIND_IDS)
def test_best_obs_agrees_with_the_distinctive_descriptors_of_host_rows(afv, gpu_ctx, kind):
    sc = S.sized_scene(kind, (1, 2, 3, 5, 8, 13, 21, 64, 65, 70), seed=17)
    sc.kf_bad = []
    rig = Rig(afv, gpu_ctx, sc)
    try:
        status, best, med = afv.ComputeDistinctiveDescriptors(rig.table, rig.points, sc.kfs, sc.point_ids, sc.observations)
        sets, first = [], []
        for pid in sc.point_ids:
            mine = [(e, o) for e, o in enumerate(sc.observations) if o[0] == pid]
            first.append(mine[0][0])
            sets.append(np.stack([sc.table_rows(s)[i] for _, (_, s, i) in mine]))
        h_best, h_med = afv.ComputeDistinctiveDescriptors(gpu_ctx, sets)
        assert np.array_equal(best - np.array(first), h_best) and np.all(status == R.DONE)
        assert med.tobytes() == np.asarray(h_med, med.dtype).tobytes()
    finally:
        rig.close()


def test_points_of_the_triangulation_are_a_fixed_point_of_the_normal_part(afv, gpu_ctx):
    """DescriptorTable.triangulate writes what UpdateNormalAndDepth would: refreshed with the observations (current, neighbour) and
    mpRefKF = current, every plane of the store stays bit-identical"""
    import _tri_scenes as TS
    from test_gpu_triangulate import c_jobs, fill_slot, make_table, pad, prefilled_store, rows_for
    job, a, b, m = TS.random_scene("mono", TS.SEEDS[0])
    t = make_table(afv, gpu_ctx, 2)
    pts, _ = prefilled_store(afv, gpu_ctx, 80)
    try:
        fill_slot(t, 0, a, rows_for(a.n, 1)); fill_slot(t, 1, b, rows_for(b.n, 2))
        got = t.triangulate([0], [1], c_jobs(afv, [job]), pad(m), points=pts, first_id=11)
        new_id = got[3][0]
        obs, ids = [], []
        for i in np.nonzero(new_id >= 0)[0]:
            ids.append(int(new_id[i]))
            obs += [(int(new_id[i]), 0, int(i)), (int(new_id[i]), 1, int(m[i]))]
        assert len(ids) >= 8
        everything = np.arange(pts.capacity, dtype=np.int32)
        before = pts.get(everything)
        status = afv.UpdateNormalAndDepth(t, pts, [0, 1], {0: job.Ow1, 1: job.Ow2}, {0: job.max_size1, 1: np.float32(1.0)}, ids, {i: 0 for i in ids}, obs)
        assert np.all(status == R.DONE)
        after = pts.get(everything)
        for k in before:
            assert after[k].tobytes() == before[k].tobytes(), k
        # ... and it is not a no-op: with the neighbour as mpRefKF the distances change
        afv.UpdateNormalAndDepth(t, pts, [0, 1], {0: job.Ow1, 1: job.Ow2}, {0: job.max_size1, 1: np.float32(1.0)}, ids, {i: 1 for i in ids}, obs)
        moved = pts.get(everything)
        assert moved["ref_distance"].tobytes() != before["ref_distance"].tobytes() and moved["normal"].tobytes() == before["normal"].tobytes()
    finally:
        pts.close(); t.close()


def test_the_chain_local_ba_refresh_search_local_points(afv, gpu_ctx):
    """LocalBundleAdjustment -> RefreshAfterBundleAdjustment -> SearchLocalPoints with nothing uploaded in between, against the same chain
    with the host's UpdateNormalAndDepth (the restatement) uploaded through afv_points_set"""
    import _lba_scenes as LS
    sc = LS.make(nk=4, nf=2, npts=30, seed=5)
    rng = np.random.default_rng(8)
    n = [len(f["x"]) for f in sc.feats]
    rows = [rng.integers(0, 256, (k, 32), dtype=np.uint8) for k in n]
    of_point = rng.integers(0, 256, (sc.np, 32), dtype=np.uint8)   # every observation of a point shows the point's own row
    for e in range(sc.ne):
        rows[sc.e_kf[e]][sc.e_idx[e]] = of_point[sc.e_pt[e]]
    size =[(np.float32(31.0) * np.float32(1.2) ** rng.integers(0, 4, k)).astype(np.float32) for k in n]
    sigma2 = [np.ones(k, np.float32) for k in n]
    table = afv.table.DescriptorTable(gpu_ctx, sc.nk, max(n) + 2)
    dev, host = afv.MapPoints(gpu_ctx, sc.store_cap), afv.MapPoints(gpu_ctx, sc.store_cap)
    fr = afv.Frame(gpu_ctx, max_x=640.0, max_y=480.0, cap=max(n) + 2)
    try:
        for k, f in enumerate(sc.feats):
            table.set(k, rows[k])
            table.set_geometry(k, f["x"], f["y"], sigma2[k], u_right=f["ur"])
            table.set_inf(k, f["inf"])
            table.set_scale(k, size[k])
        cams = {k: dict(Rcw=sc.cams[k, :9], tcw=sc.cams[k, 9:12], fx=sc.cams[k, 12], fy=sc.cams[k, 13], cx=sc.cams[k, 14], cy=sc.cams[k, 15],
                        mbf=sc.cams[k, 16]) for k in range(sc.nk)}
        obs = [(int(sc.ids[sc.e_pt[e]]), int(sc.e_kf[e]), int(sc.e_idx[e])) for e in range(sc.ne)]
        ids = [int(i) for i in sc.ids]
        first = {p: [o for o in obs if o[0] == p][0] for p in ids}
        for store in (dev, host):   # the map before the adjustment: positions, descriptors of the first observation, stale view geometry
            store.set(sc.ids, pos=sc.pos, normal=np.tile(np.float32([0, 0, 1]), (sc.np, 1)), min_distance=np.full(sc.np, 0.1), max_distance=np.full(sc.np, 0.2),
                      ref_size=np.full(sc.np, 31.0), ref_distance=np.full(sc.np, 0.15), ref_sigma=np.ones(sc.np))
            store.set_flags(sc.ids, bad=np.zeros(sc.np), observed=np.ones(sc.np))
            store.set_descriptors(sc.ids, np.stack([rows[first[p][1]][first[p][2]] for p in ids]))
        ref_kf = {p: first[p][1] for p in ids}
        max_size = {k: np.float32(31.0) * np.float32(1.2) ** 7 for k in range(sc.nk)}
        fixed = {k: cams[k] for k in range(sc.nf, sc.nk)}
        # the device chain
        poses, xyz, _, _ = afv.LocalBundleAdjustment(table, dev, list(range(sc.nf)), list(range(sc.nf, sc.nk)), cams, sc.ids, obs)
        status, _, _ = afv.RefreshAfterBundleAdjustment(table, dev, poses, fixed, max_size, ids, ref_kf, obs)
        assert np.all(status == R.DONE)
        # the host chain: the same adjustment, UpdateNormalAndDepth by the restatement, afv_points_set
        poses_h, xyz_h, _, _ = afv.LocalBundleAdjustment(table, host, list(range(sc.nf)), list(range(sc.nf, sc.nk)), cams, sc.ids, obs)
        assert xyz_h.tobytes() == xyz.tobytes()
        centres = [afv.refresh.camera_centre(*poses_h[k]) if k in poses_h else afv.refresh.camera_centre(cams[k]["Rcw"], cams[k]["tcw"]) for k in range(sc.nk)]
        moved = host.get(sc.ids)["pos"]
        fields = []
        for i, p in enumerate(ids):
            st, f = R.normal_and_depth(moved[i], [(k, j) for q, k, j in obs if q == p], centres, ref_kf[p], lambda k, j: size[k][j],
                                       lambda k, j: sigma2[k][j], [max_size[k] for k in range(sc.nk)])
            assert st == R.DONE
            fields.append(f)
        host.set(sc.ids, **{k: np.stack([f[k] for f in fields]) for k in R.PLANES})
        a, b = dev.get(sc.ids), host.get(sc.ids)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a["ref_distance"].tobytes() != np.full(sc.np, 0.15, np.float32).tobytes()
        # SearchLocalPoints from the last (fixed) keyframe's view: the same answer from both stores
        k = sc.nk - 1
        kps = np.zeros(n[k], afv.KP_DTYPE)
        kps["x"], kps["y"] = sc.feats[k]["x"], sc.feats[k]["y"]
        fr.set_features(kps, rows[k], sizes=size[k])
        c = cams[k]
        fr.set_pose(c["Rcw"], c["tcw"], centres[k], c["fx"], c["fy"], c["cx"], c["cy"], 0.0)
        afv.FeatureMatcher.setDescriptorDistanceThresholds(100.0)
        try:
            m = afv.FeatureMatcher(0.8, False, ctx=gpu_ctx)
            ga = fr.SearchLocalPoints(m, dev, sc.ids, 3.0)
            gb = fr.SearchLocalPoints(m, host, sc.ids, 3.0)
        finally:
            afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        assert ga[1] == gb[1] and np.array_equal(ga[0], gb[0]) and np.array_equal(ga[2], gb[2])
        assert ga[1] > 0   # the refreshed distances put the points into the search: the stale ones (0.1 .. 0.2) would reject every one
    finally:
        dev.close(); host.close(); fr.close(); table.close()


def test_every_refusal_leaves_the_store_and_the_outputs_untouched(afv, gpu_ctx):
    L = afv._lib
    sc = S.rule_scene(S.KINDS[0])
    rig = Rig(afv, gpu_ctx, sc)
    other_ctx = afv.Context(max_width=640, max_height=480, max_batch=1)
    foreign = afv.MapPoints(other_ctx, 16)
    foreign_table = afv.table.DescriptorTable(other_ctx, 2, 4)
    wide = afv.MapPoints(gpu_ctx, rig.points.capacity, desc_bytes=61)
    floats = afv.MapPoints(gpu_ctx, rig.points.capacity, float_dim=36)
    bare = afv.table.DescriptorTable(gpu_ctx, sc.nslots, sc.cap)
    try:
        op, ok, oi, _ = S.edge_arrays(sc)
        where_k = {s: i for i, s in enumerate(sc.kfs)}
        base = dict(slots=np.array(sc.kfs, np.int32), cen=np.array([sc.centres[s] for s in sc.kfs], np.float32).reshape(-1),
                    mx=np.array([sc.max_size[s] for s in sc.kfs], np.float32), bad=np.zeros(len(sc.kfs), np.uint8),
                    ids=np.array(sc.point_ids, np.int32), ref=np.array([where_k.get(sc.ref_kf.get(p, -1), -1) for p in sc.point_ids], np.int32),
                    op=op, ok=ok, oi=oi)
        nk, npts, ne = len(sc.kfs), len(sc.point_ids), len(op)

        def refused(table=None, points=None, descriptors=1, normals=1, struct_size=None, out_size=None, **over):
            a = dict(base, nk=nk, npts=npts, ne=ne)
            a.update(over)
            prm = L.sized(L.RefreshParams)
            prm.descriptors, prm.normals = descriptors, normals
            if struct_size is not None:
                prm.struct_size = struct_size
            status, best, med = (np.full(npts + 1, 0x5A5A5A5A, np.int32) for _ in range(3))
            out = L.sized(L.RefreshOut)
            out.status, out.best_obs, out.best_median = status.ctypes.data, best.ctypes.data, med.ctypes.data
            if out_size is not None:
                out.struct_size = out_size
            p = lambda v: L.ptr(v) if isinstance(v, np.ndarray) else v
            code = rig.table.lib.afv_table_refresh_points((table or rig.table).handle, (points or rig.points).handle, p(a["slots"]), a["nk"], p(a["cen"]),
                                                          p(a["mx"]), p(a["bad"]), p(a["ids"]), a["npts"], p(a["ref"]), p(a["op"]), p(a["ok"]), p(a["oi"]),
                                                          a["ne"], C.byref(prm), C.byref(out))
            assert all(np.all(v == 0x5A5A5A5A) for v in (status, best, med)), over.keys()
            after = rig.points.get(rig.all_ids)
            for k in after:
                assert after[k].tobytes() == rig.before[k].tobytes(), (over.keys(), k)
            return code

        def changed(a, i, v):
            b = np.array(a)
            b[i] = v
            return b

        for name in ("slots", "cen", "mx", "ids", "ref", "op", "ok", "oi"):
            assert refused(**{name: None}) == L.EINVAL, name
        assert refused(struct_size=8) == L.EINVAL and refused(struct_size=0) == L.EINVAL and refused(out_size=6) == L.EINVAL
        assert refused(descriptors=2) == L.EINVAL and refused(normals=-1) == L.EINVAL
        assert refused(points=foreign) == L.EINVAL and refused(table=foreign_table) == L.EINVAL   # a store / a table of another context
        assert refused(points=wide) == L.EUNSUPPORTED and refused(points=floats) == L.EUNSUPPORTED
        assert refused(nk=L.LBA_MAX_KF + 1) == L.EINVAL and refused(npts=L.LBA_MAX_POINTS + 1) == L.EINVAL and refused(ne=L.LBA_MAX_EDGES + 1) == L.EINVAL
        assert refused(nk=-1) == L.EINVAL and refused(npts=-1) == L.EINVAL and refused(ne=-1) == L.EINVAL
        assert refused(slots=changed(base["slots"], 1, sc.nslots)) == L.EINVAL and refused(slots=changed(base["slots"], 0, -1)) == L.EINVAL
        assert refused(ids=changed(base["ids"], 3, rig.points.capacity)) == L.EINVAL and refused(ids=changed(base["ids"], 3, -1)) == L.EINVAL
        assert refused(ids=changed(base["ids"], 3, base["ids"][4])) == L.EINVAL      # named twice
        assert refused(ref=changed(base["ref"], 0, nk)) == L.EINVAL and refused(ref=changed(base["ref"], 0, -2)) == L.EINVAL
        assert refused(op=changed(op, 9, npts)) == L.EINVAL and refused(op=changed(op, 9, -1)) == L.EINVAL
        assert refused(op=changed(op, 9, 0)) == L.EINVAL                             # not grouped by point
        assert refused(ok=changed(ok, 9, nk)) == L.EINVAL and refused(ok=changed(ok, 9, -1)) == L.EINVAL
        assert op[1] == op[2] and refused(ok=changed(ok, 2, ok[1])) == L.EINVAL      # a point observed twice by one keyframe
        assert refused(oi=changed(oi, 9, sc.cap)) == L.EINVAL and refused(oi=changed(oi, 9, -1)) == L.EINVAL
        # a table whose slots hold rows without geometry, then with geometry but without the scale plane
        for s in range(sc.nslots):
            bare.set(s, sc.table_rows(s))
        assert refused(table=bare) == L.EINVAL
        for s in range(sc.nslots):
            bare.set_geometry(s, sc.x[s], sc.y[s], sc.sigma2[s])
        assert refused(table=bare) == L.EINVAL
        assert b"scale" in bare.lib.afv_last_error(gpu_ctx.handle)
        # ... which the descriptor part alone does not need: the same table is accepted without the normals and answers as the full one
        want = reference("rule_scene", S.KINDS[0], (), PARTS["descriptors"])[1]
        status, best, med = afv.RefreshMapPoints(bare, rig.points, sc.kfs, sc.centres, sc.max_size, sc.point_ids, sc.ref_kf, sc.observations,
                                                 kf_bad=sc.kf_bad, descriptors=True, normals=False)
        assert np.array_equal(status, want[0]) and np.array_equal(best, want[1]) and med.tobytes() == want[2].tobytes()
        rig.assert_store(want[3], "descriptors alone, a table without the scale plane")
        # and the call as it stands is accepted
        status = rig.refresh(afv)[0]
        assert np.array_equal(status, reference("rule_scene", S.KINDS[0])[1][0])
    finally:
        bare.close(); floats.close(); wide.close(); foreign.close(); foreign_table.close(); rig.close(); other_ctx.close()

