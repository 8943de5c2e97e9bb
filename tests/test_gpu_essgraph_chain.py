"""-m gpu: a loop closure on a small map, every step on the device and nothing uploaded in between but what the host's map owns:
OptimizeSim3 (the Sim3 of the loop candidate) -> MapPoints.correct_sim3 (CorrectLoop's correction of the current keyframe's neighbourhood)
-> FusePoints (the loop keyframe's points into the corrected current keyframe) -> OptimizeEssentialGraph (poses and every point of the
store) -> RefreshMapPoints(normals) -> SearchLocalPoints.  After it a frame at the corrected pose of the current keyframe finds the
corrected points: each of its features gets the point it shows, the loop keyframe's copy where Fuse replaced the duplicate.

The map: six keyframes on a path that returns to its start, monocular drift that grows with the keyId (a rotation, a translation and a
scale per keyframe: keyframe k holds its part of the world through the similarity D_k, D_0 = identity), 20 loop points that the map holds
twice (an old copy seen by keyframes 0 and 1, a drifted new copy seen by 4 and 5), 20 points of the middle, 15 recent points.  Pixels do
not drift: every keyframe observes the true projections."""
import importlib

import numpy as np
import pytest

import _essgraph_scenes as SC

pytestmark = pytest.mark.gpu
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
SIZE = np.float32(2.0)        # keyPtsSize of every feature: the search radius of SearchLocalPoints is th * 4 * size = 24 px at th = 3
F64 = np.float64


class World:
    def __init__(self, seed=3):
        E = importlib.import_module("anyfeature-vslam_amd").essgraph
        self.E = E
        rng = np.random.default_rng(seed)
        self.nk = 6
        centres = [(0.0, 0.0, 0.0), (0.5, 0.1, 0.0), (0.9, 0.5, 0.1), (0.7, 0.9, 0.0), (0.3, 0.6, -0.1), (0.1, 0.1, 0.05)]
        self.true = []                                      # (R_k, t_k): camera = R X + t
        for k, c in enumerate(centres):
            R = SC.rot([0.02 * np.sin(k), 0.03 * np.cos(2 * k), 0.01 * k])
            self.true.append((R, -R @ np.array(c, F64)))
        self.scale = [1.0 + 0.02 * k for k in range(self.nk)]
        self.D = [(SC.rot(np.array([0.3, 1.0, 0.2]) * 0.01 * k), np.array([0.04, 0.02, -0.02]) * k, self.scale[k]) for k in range(self.nk)]
        # C_k = (R_k, s_k t_k, s_k): the Sim3 the essential graph should end at; the stored pose is C_k * D_k^-1 (scale 1)
        self.C = [(R, self.scale[k] * t, self.scale[k]) for k, (R, t) in enumerate(self.true)]
        self.stored = [E.sim3_mul(self.C[k], E.sim3_inverse(self.D[k])) for k in range(self.nk)]
        self.cams = {k: dict(Rcw=self.stored[k][0].astype(np.float32), tcw=self.stored[k][1].astype(np.float32), fx=FX, fy=FY, cx=CX, cy=CY)
                     for k in range(self.nk)}
        nl, nm, nr = 20, 20, 15
        X = np.stack([rng.uniform(-1.6, 2.2, nl + nm + nr), rng.uniform(-1.2, 1.8, nl + nm + nr), rng.uniform(4.0, 8.0, nl + nm + nr)], 1)
        # store ids: old copies 0 .. 19 (ref 0, seen by 0, 1), new copies 20 .. 39 (ref 5, seen by 4, 5), middle 40 .. 59 (ref 2, seen by 1, 2, 3),
        # recent 60 .. 74 (ref 4 for even ids, 5 for odd, seen by 3, 4, 5)
        self.phys = np.concatenate([np.arange(nl), np.arange(nl), nl + np.arange(nm), nl + nm + np.arange(nr)])
        self.ref = np.concatenate([np.zeros(nl, int), np.full(nl, 5), np.full(nm, 2), np.where(np.arange(nr) % 2 == 0, 4, 5)])
        seen = [(0, 1)] * nl + [(4, 5)] * nl + [(1, 2, 3)] * nm + [(3, 4, 5)] * nr
        self.npts = len(self.phys)
        self.X = X
        self.rows_of_phys = rng.integers(0, 256, (len(X), 32), dtype=np.uint8)
        self.pos = np.stack([self.map_point(self.D[self.ref[p]], X[self.phys[p]]) for p in range(self.npts)]).astype(np.float32)
        self.feats = [[] for _ in range(self.nk)]           # per keyframe the store ids its features show, in feature order
        self.obs = []                                       # (point id, keyframe, feature index), by point
        for p in range(self.npts):
            for k in seen[p]:
                self.obs.append((p, k, len(self.feats[k])))
                self.feats[k].append(p)
        self.xy = []
        for k in range(self.nk):
            R, t = self.true[k]
            c = (R @ X[self.phys[self.feats[k]]].T).T + t
            self.xy.append((np.float32(FX * c[:, 0] / c[:, 2] + CX), np.float32(FY * c[:, 1] / c[:, 2] + CY)))
            assert np.all(c[:, 2] > 1) and np.all((self.xy[k][0] > 5) & (self.xy[k][0] < 635) & (self.xy[k][1] > 5) & (self.xy[k][1] < 475))

    @staticmethod
    def map_point(S, X):
        return S[2] * (S[0] @ X) + S[1]

    def rows(self, k):
        return self.rows_of_phys[self.phys[self.feats[k]]]


def centre_of(afv, R, t):
    return afv.refresh.camera_centre(np.asarray(R, np.float32), np.asarray(t, np.float32))


def frame_at(afv, ctx, w, k, R, t):
    """a frame with keyframe k's features at the pose (R, t)"""
    fr = afv.Frame(ctx, max_x=640.0, max_y=480.0, cap=len(w.feats[k]) + 2)
    kps = np.zeros(len(w.feats[k]), afv.KP_DTYPE)
    kps["x"], kps["y"] = w.xy[k]
    fr.set_features(kps, w.rows(k), sizes=np.full(len(kps), SIZE))
    fr.set_pose(np.float32(R), np.float32(t), centre_of(afv, R, t), FX, FY, CX, CY, 0.0)
    return fr


def correct_matches(w, k, assign, ids, replaced):
    """features of keyframe k that were given the point they show (the old copy where the duplicate was replaced)"""
    want = np.array([replaced.get(p, p) for p in w.feats[k]])
    got = np.where(assign >= 0, np.asarray(ids)[np.clip(assign, 0, None)], -1)
    return int(np.sum(got == want)), got, want


def test_the_chain_of_a_loop_closure(afv, gpu_ctx):
    E = afv.essgraph
    w = World()
    nk, cur, loop = w.nk, 5, 0
    n = [len(f) for f in w.feats]
    table = afv.table.DescriptorTable(gpu_ctx, nk, max(n) + 2)
    store = afv.MapPoints(gpu_ctx, w.npts + 5)
    frames = []
    afv.FeatureMatcher.setDescriptorDistanceThresholds(100.0)
    try:
        matcher = afv.FeatureMatcher(0.8, False, ctx=gpu_ctx)
        for k in range(nk):
            table.set(k, w.rows(k))
            table.set_geometry(k, w.xy[k][0], w.xy[k][1], np.ones(n[k], np.float32))
            table.set_inf(k, np.ones(n[k], np.float32))
            table.set_scale(k, np.full(n[k], SIZE))
        ids = np.arange(w.npts, dtype=np.int32)
        store.set(ids, pos=w.pos)
        store.set_flags(ids, bad=np.zeros(w.npts), observed=np.ones(w.npts))
        store.set_descriptors(ids, w.rows_of_phys[w.phys])
        kfs = list(range(nk))
        max_size = {k: SIZE * np.float32(1.2) ** 7 for k in kfs}
        ref_kf = {int(p): int(w.ref[p]) for p in ids}
        centres = {k: centre_of(afv, w.cams[k]["Rcw"], w.cams[k]["tcw"]) for k in kfs}
        st = afv.UpdateNormalAndDepth(table, store, kfs, centres, max_size, ids, ref_kf, w.obs)       # the map as LocalMapping left it
        assert not st.any()
        # before the loop is closed: a frame at the TRUE pose of the current keyframe finds the old copies, not the drifted recent points
        fr = frame_at(afv, gpu_ctx, w, cur, *w.true[cur])
        frames.append(fr)
        a0, n0, _ = fr.SearchLocalPoints(matcher, store, ids, 3.0)
        before, _, _ = correct_matches(w, cur, a0, ids, {p: p - 20 for p in range(20, 40)})

        # 1. OptimizeSim3: the current keyframe's new copies against the loop keyframe's old copies, from a perturbed start
        mp1 = np.array(w.feats[cur], np.int32)
        mp2 = np.where((mp1 >= 20) & (mp1 < 40), mp1 - 20, -1).astype(np.int32)
        idx_in_loop = {p: i for i, p in enumerate(w.feats[loop])}
        idx2 = np.array([idx_in_loop.get(int(b), -1) for b in mp2], np.int32)
        S12 = E.sim3_mul(w.C[cur], E.sim3_inverse((w.true[loop][0], w.true[loop][1], 1.0)))
        start = (np.float32(SC.rot([0.004, -0.003, 0.002]) @ S12[0]), np.float32(S12[1] + [0.01, -0.01, 0.02]), np.float32(S12[2] * 1.01))
        n_in, _, (R12, t12, s12) = afv.OptimizeSim3(table, store, cur, loop, mp1, mp2, idx2, w.cams, start, th2=10, fix_scale=False)
        assert n_in == 20 and abs(s12 - w.scale[cur]) < 2e-3

        # 2. CorrectLoop: the corrected Sim3 of the current keyframe and of its neighbour 4; their points move in the store
        Scw = E.sim3_mul((np.asarray(R12, F64).reshape(3, 3), np.asarray(t12, F64), F64(s12)),
                         (w.cams[loop]["Rcw"].astype(F64), w.cams[loop]["tcw"].astype(F64), F64(1.0)))
        siw = lambda k: (w.cams[k]["Rcw"].astype(F64), w.cams[k]["tcw"].astype(F64), F64(1.0))
        non_corrected = {k: siw(k) for k in (4, cur)}
        corrected = {cur: Scw, 4: E.sim3_mul(E.sim3_mul(siw(4), E.sim3_inverse(siw(cur))), Scw)}
        near = [int(p) for p in ids if w.ref[p] in (4, cur)]
        st = store.correct_sim3(near, [0 if w.ref[p] == 4 else 1 for p in near], [non_corrected[4], non_corrected[cur]],
                                [E.sim3_inverse(corrected[4]), E.sim3_inverse(corrected[cur])])
        assert not st.any()

        # 3. SearchAndFuse: the loop keyframe's points into the current keyframe at its corrected pose; a found duplicate is replaced
        Rc, tc = corrected[cur][0], corrected[cur][1] / corrected[cur][2]
        fr = frame_at(afv, gpu_ctx, w, cur, Rc, tc)
        frames.append(fr)
        old = np.arange(20, dtype=np.int32)
        best, found = fr.FusePoints(matcher, store, old, 4.0, use_inf_gate=False)
        assert found == 20 and np.array_equal(np.asarray(w.feats[cur])[best], old + 20)     # each old copy lands on the feature of its duplicate
        replaced = {int(p) + 20: int(p) for p in old}
        store.set_flags(old + 20, bad=np.ones(20), observed=np.zeros(20))
        obs = [o for o in w.obs if o[0] not in replaced] + [(replaced[p], k, i) for p, k, i in w.obs if p in replaced]
        alive = np.array([p for p in ids if p not in replaced], np.int32)

        # 4. OptimizeEssentialGraph: every keyframe, every point of the map
        kf_list = [dict(id=k, Rcw=w.cams[k]["Rcw"].reshape(3, 3), tcw=w.cams[k]["tcw"]) for k in kfs]
        graph = dict(parent={k: (k - 1 if k else None) for k in kfs}, loop_edges={},
                     covisibles={k: [j for j in (k - 1, k + 1) if 0 <= j < nk] for k in kfs})
        out = afv.OptimizeEssentialGraph(gpu_ctx, store, kf_list, loop, cur, non_corrected, corrected, {cur: [(loop, 20)]}, graph, False, ids, w.ref)
        res = out["result"]
        assert res.status == 0 and res.iterations >= 2 and res.chi2_last < 0.2 * res.chi2_first
        assert [(e[0], e[1]) for e in out["edges"]] == [(5, 0), (1, 0), (2, 1), (3, 2), (4, 3), (5, 4)]
        assert np.array_equal(out["point_status"], np.where(np.isin(ids, old + 20), 1, 0))       # the replaced duplicates are bad: skipped
        # six edges of equal weight share the drift of the cycle, so no pose ends AT the truth; each ends at least twice as near as it was
        err = lambda R, t, k: (np.abs(np.asarray(R, F64).reshape(3, 3) - w.true[k][0]).max(), np.abs(np.asarray(t, F64) - w.true[k][1]).max())
        was = np.array([err(w.cams[k]["Rcw"], w.cams[k]["tcw"], k) for k in kfs]).max(0)
        now = np.array([err(out["Tiw_double"][k, :9], out["Tiw_double"][k, 9:], k) for k in kfs]).max(0)
        assert np.all(now < 0.5 * was), (now, was)
        moved = store.get(alive)["pos"]
        assert np.abs(moved - w.X[w.phys[alive]]).max() < 0.5 * np.abs(w.pos[alive] - w.X[w.phys[alive]]).max()

        # 5. UpdateNormalAndDepth of the moved points from the corrected poses
        Tiw = out["Tiw"]
        centres = {k: centre_of(afv, Tiw[k, :9], Tiw[k, 9:]) for k in kfs}
        st = afv.UpdateNormalAndDepth(table, store, kfs, centres, max_size, alive, ref_kf, obs)
        assert not st.any()

        # 6. a frame at the corrected pose of the current keyframe finds the corrected points
        fr = frame_at(afv, gpu_ctx, w, cur, Tiw[cur, :9].reshape(3, 3), Tiw[cur, 9:])
        frames.append(fr)
        a1, n1, in_view = fr.SearchLocalPoints(matcher, store, alive, 3.0)
        after, got, want = correct_matches(w, cur, a1, alive, replaced)
        assert after == n[cur] == 35, (after, got, want)
        assert before <= 24 < after, before                    # before the closure the drifted recent points were out of reach
        assert in_view[np.isin(alive, w.feats[cur]) | np.isin(alive, old)].all()
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        for fr in frames:
            fr.close()
        store.close()
        table.close()
