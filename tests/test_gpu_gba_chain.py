"""-m gpu: what follows a loop closure on a map with MORE than 64 keyframes, every step on the device: OptimizeEssentialGraph (poses and every
point of the store) -> GlobalBundleAdjustment(write_points=False) over all 70 keyframes (69 free: past the old cap, the block-sparse
route) -> the host sets the store from xyz for the optimised points (mPosGBA) -> MapPoints.correct_se3 moves the few points that were
left out of the BA (LoopClosing.cc:731-750) -> UpdateNormalAndDepth over the observations -> a frame at an optimised pose finds its
points with SearchLocalPoints.  This is tests/test_gpu_essgraph_chain.py's map at 70 keyframes with 10 points each, the step the
reference runs next included.

The map: 70 keyframes on a closed path, monocular drift that grows with the keyId (keyframe k holds its part of the world through the
similarity D_k, D_0 = identity), ten points per keyframe seen by that keyframe and its two neighbours on the path (the loop is fused:
keyframes 69 and 0 share points).  Pixels do not drift: every keyframe observes the true projections."""
import importlib

import numpy as np
import pytest

import _essgraph_scenes as SC
import _gba_ref as G
from test_gpu_essgraph_chain import CX, CY, FX, FY, SIZE, centre_of, frame_at

pytestmark = pytest.mark.gpu
F64 = np.float64
NK, PER, LEFT_OUT = 70, 10, (7, 203, 318, 455, 611, 699)     # the points no keyframe's BA edge names (the BA "did not optimise" them)


class World:
    def __init__(self, seed=5):
        E = importlib.import_module("anyfeature-vslam_amd").essgraph
        rng = np.random.default_rng(seed)
        self.nk = NK
        self.true = []
        for k in range(NK):
            a = 2 * np.pi * k / NK
            R = SC.rot([0.02 * np.sin(k), 0.03 * np.cos(2 * k), 0.0])
            self.true.append((R, -R @ np.array([0.5 * np.cos(a), 0.5 * np.sin(a), 0.0], F64)))
        self.scale = [1.0 + 0.0015 * k for k in range(NK)]
        self.D = [(SC.rot(np.array([0.3, 1.0, 0.2]) * 0.0008 * k), np.array([0.04, 0.02, -0.02]) * 0.08 * k, self.scale[k]) for k in range(NK)]
        self.C = [(R, self.scale[k] * t, self.scale[k]) for k, (R, t) in enumerate(self.true)]
        self.stored = [E.sim3_mul(self.C[k], E.sim3_inverse(self.D[k])) for k in range(NK)]
        self.cams = {k: dict(Rcw=self.stored[k][0].astype(np.float32), tcw=self.stored[k][1].astype(np.float32), fx=FX, fy=FY, cx=CX, cy=CY)
                     for k in range(NK)}
        self.npts = NK * PER
        self.X = np.stack([rng.uniform(-1.0, 1.0, self.npts), rng.uniform(-1.0, 1.0, self.npts), rng.uniform(4.0, 8.0, self.npts)], 1)
        self.ref = np.arange(self.npts) // PER
        self.rows_of_point = rng.integers(0, 256, (self.npts, 32), dtype=np.uint8)
        self.pos = np.stack([self.D[self.ref[p]][2] * (self.D[self.ref[p]][0] @ self.X[p]) + self.D[self.ref[p]][1] for p in range(self.npts)]).astype(np.float32)
        self.feats = [[] for _ in range(NK)]
        self.obs = []
        for p in range(self.npts):
            for k in sorted({(self.ref[p] - 1) % NK, self.ref[p], (self.ref[p] + 1) % NK}):
                self.obs.append((p, int(k), len(self.feats[k])))
                self.feats[k].append(p)
        self.xy = []
        for k in range(NK):
            R, t = self.true[k]
            c = (R @ self.X[self.feats[k]].T).T + t
            self.xy.append((np.float32(FX * c[:, 0] / c[:, 2] + CX), np.float32(FY * c[:, 1] / c[:, 2] + CY)))
            assert np.all(c[:, 2] > 1) and np.all((self.xy[k][0] > 5) & (self.xy[k][0] < 635) & (self.xy[k][1] > 5) & (self.xy[k][1] < 475))

    def rows(self, k):
        return self.rows_of_point[self.feats[k]]


def pixel_error(w, poses, X_of):
    """sum of squared reprojection errors of every observation that X_of names, at poses {k: (R, t)}"""
    s = 0.0
    for p, k, i in w.obs:
        if p in X_of:
            R, t = poses[k]
            c = np.asarray(R, F64).reshape(3, 3) @ np.asarray(X_of[p], F64) + np.asarray(t, F64)
            s += (FX * c[0] / c[2] + CX - w.xy[k][0][i]) ** 2 + (FY * c[1] / c[2] + CY - w.xy[k][1][i]) ** 2
    return s


def test_the_chain_after_a_loop_closure_on_seventy_keyframes(afv, gpu_ctx):
    E = afv.essgraph
    w = World()
    nk, cur, loop = w.nk, NK - 1, 0
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
        store.set_descriptors(ids, w.rows_of_point)
        kfs = list(range(nk))

        # 1. OptimizeEssentialGraph: the corrected Sim3 of the current keyframe (and of its neighbour) closes the loop
        siw = lambda k: (w.cams[k]["Rcw"].astype(F64), w.cams[k]["tcw"].astype(F64), F64(1.0))
        Scw = (w.C[cur][0], w.C[cur][1], F64(w.C[cur][2]))
        non_corrected = {k: siw(k) for k in (cur - 1, cur)}
        corrected = {cur: Scw, cur - 1: E.sim3_mul(E.sim3_mul(siw(cur - 1), E.sim3_inverse(siw(cur))), Scw)}
        kf_list = [dict(id=k, Rcw=w.cams[k]["Rcw"].reshape(3, 3), tcw=w.cams[k]["tcw"]) for k in kfs]
        graph = dict(parent={k: (k - 1 if k else None) for k in kfs}, loop_edges={},
                     covisibles={k: [j for j in (k - 1, k + 1) if 0 <= j < nk] for k in kfs})
        out = afv.OptimizeEssentialGraph(gpu_ctx, store, kf_list, loop, cur, non_corrected, corrected, {cur: [(loop, 20)]}, graph, False, ids, w.ref)
        assert out["result"].status == 0 and out["result"].iterations >= 2
        Tiw = np.asarray(out["Tiw"], np.float32).reshape(nk, 12)
        after_ess = store.get(ids)["pos"].copy()

        # 2. GlobalBundleAdjustment as LoopClosing::RunGlobalBundleAdjustment calls it: 69 free keyframes, the store stays
        in_ba = np.array([p for p in ids if p not in LEFT_OUT], np.int32)
        obs = [o for o in w.obs if o[0] not in LEFT_OUT]
        cams = {k: dict(Rcw=Tiw[k, :9], tcw=Tiw[k, 9:], fx=FX, fy=FY, cx=CX, cy=CY) for k in kfs}
        poses, xyz, trace = afv.GlobalBundleAdjustment(table, store, [(k, k == 0) for k in kfs], cams, in_ba, obs, 10, robust=False, write_points=False)
        assert len(poses) == nk - 1 > afv._lib.LBA_MAX_FREE and trace["iterations"][0] >= 1 and trace["n_edges"] == len(obs) and trace["stopped"] == 0
        assert store.get(ids)["pos"].tobytes() == after_ess.tobytes()                     # write_points = False
        # Levenberg accepts a trial only when the chi2 falls: the adjusted map explains the pixels better than the essential graph's
        start = {k: (Tiw[k, :9], Tiw[k, 9:]) for k in kfs}
        end = dict(poses)
        end[0] = start[0]                                                                   # keyId 0 is fixed
        e0 = pixel_error(w, start, {int(p): after_ess[p] for p in in_ba})
        e1 = pixel_error(w, end, {int(p): xyz[i] for i, p in enumerate(in_ba)})
        assert e1 < e0 and np.isfinite(trace["chi2"][0]), (e0, e1)
        assert abs(trace["chi2"][0] - e1) <= 1e-6 * e1                                      # information 1 everywhere: the chi2 IS that sum

        # 3. the host: SetWorldPos(mPosGBA) for the optimised points, SetPose(TcwGBA) for the keyframes
        store.set(in_ba, pos=xyz.astype(np.float32))
        Tcw = {k: (np.float32(end[k][0]).reshape(3, 3), np.float32(end[k][1])) for k in kfs}

        # 4. the points the BA left out follow their reference keyframe: Twc is GetPoseInverse() after SetPose, formed by the host in float
        left = np.array(LEFT_OUT, np.int32)
        refs = sorted({int(w.ref[p]) for p in left})
        T_before = np.stack([Tiw[k] for k in refs])
        T_after = np.stack([np.concatenate([Tcw[k][0].T.reshape(9), -(Tcw[k][0].T @ Tcw[k][1])]).astype(np.float32) for k in refs])
        pair = [refs.index(int(w.ref[p])) for p in left]
        st = store.correct_se3(left, pair, T_before, T_after)
        want, want_st = G.correct_se3(after_ess[left], np.ones(len(left), bool), pair, T_before, T_after)
        assert not st.any() and np.array_equal(st, want_st)
        moved = store.get(left)["pos"]
        assert moved.tobytes() == want.tobytes() and moved.tobytes() != after_ess[left].tobytes()

        # 5. UpdateNormalAndDepth of every point from the adjusted poses
        max_size = {k: SIZE * np.float32(1.2) ** 7 for k in kfs}
        ref_kf = {int(p): int(w.ref[p]) for p in ids}
        centres = {k: centre_of(afv, Tcw[k][0], Tcw[k][1]) for k in kfs}
        assert not afv.UpdateNormalAndDepth(table, store, kfs, centres, max_size, ids, ref_kf, w.obs).any()

        # 6. a frame at an adjusted pose finds its points, a left-out one among them
        k = int(w.ref[LEFT_OUT[2]])
        fr = frame_at(afv, gpu_ctx, w, k, Tcw[k][0], Tcw[k][1])
        frames.append(fr)
        assign, n_found, in_view = fr.SearchLocalPoints(matcher, store, ids, 3.0)
        got = np.where(assign >= 0, ids[np.clip(assign, 0, None)], -1)
        assert np.array_equal(got, np.asarray(w.feats[k])), (got, w.feats[k])
        assert LEFT_OUT[2] in got and n_found >= len(w.feats[k]) == 3 * PER
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        for fr in frames:
            fr.close()
        store.close()
        table.close()
