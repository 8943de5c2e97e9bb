"""Constructed scenes for LocalBundleAdjustment / BundleAdjustment (tests/_lba_ref.py): cameras on an arc looking at points in front of
them, seeded pixel noise, planted gross outliers.  A Scene holds what the device entry point takes (keyframe features, store ids and
positions, the edge list by point) and the same problem as the restatement and the host program take it (one observation per edge).
tests/test_lba_ref_cpu.py proves that every named scene reaches the rule it is named for."""
import numpy as np

import _lba_ref as L

F32 = np.float32


class Scene:
    def problem(self):
        return L.Problem(self.cams, self.nf, self.pos, self.p_ok, self.e_pt, self.e_kf, self.obs)

    def solve(self, log=None, stop_at="scene"):
        return L.bundle_adjust(self.problem(), self.iterations, self.robust, self.checks, self.stop_at if stop_at == "scene" else stop_at, log)


def make(nk=6, nf=3, npts=40, seed=1, views=None, stereo_kfs=(), noise=0.5, outliers=(), shake=0.02, pose_shake=0.01, behind=(), dropped=(),
         iterations=(5, 10), robust=(True, False), checks=True, stop_at=None, extra_features=3, centers=None, truth=None, start=None,
         obs_truth=None, inf_of=None, inf_scale=None):
    """views: per point the keyframes that see it (default: all).  outliers: (point, kf, du) pixel offsets.  behind: (point, kf) edges whose
    point is mirrored behind that keyframe with an observation that projects exactly.  dropped: points whose id is unset in the store.  centers {k: C}: a keyframe placed elsewhere
    (same orientation rule); truth {p: X}; start {p: X}: the position in the store; obs_truth {(p, k): X}: that edge observes X exactly;
    inf_of {(p, k): inf}; inf_scale {k: s}: every information of keyframe k times s."""
    centers, truth, start, obs_truth, inf_of, inf_scale = (v or {} for v in (centers, truth, start, obs_truth, inf_of, inf_scale))
    rng = np.random.RandomState(seed)
    sc = Scene()
    sc.nk, sc.nf, sc.np = nk, nf, npts
    sc.iterations, sc.robust, sc.checks, sc.stop_at = iterations, robust, checks, stop_at
    cams = np.zeros((nk, 17), np.float64)
    spread = min(1.0, 6.0 / max(nk - 1, 1))               # many keyframes share the arc of seven
    for k in range(nk):
        a = 0.06 * spread * (k - (nk - 1) / 2.0)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        C = np.asarray(centers.get(k, [0.35 * spread * (k - (nk - 1) / 2.0), 0.02 * spread * k, 0.0]), np.float64)
        cams[k, :9], cams[k, 9:12] = R.reshape(9), -R @ C
        cams[k, 12:17] = (500.0, 505.0, 320.0, 240.0, 40.0)
    true_cams = cams.astype(F32)
    X = np.stack([rng.uniform(-2, 2, npts), rng.uniform(-1, 1, npts), rng.uniform(4, 8, npts)], 1)
    for p, v in truth.items():
        X[p] = v
    for p, k in behind:                                     # a point behind keyframe k, on its optical axis side
        Rk, tk = true_cams[k, :9].reshape(3, 3).astype(np.float64), true_cams[k, 9:12].astype(np.float64)
        X[p] = Rk.T @ (np.array([0.3, 0.2, -3.0]) - tk)
    views = views if views is not None else [list(range(nk))] * npts
    feats = [dict(x=[], y=[], ur=[], inf=[]) for _ in range(nk)]
    for k in range(nk):                                     # decoy features that no edge names
        for _ in range(extra_features):
            feats[k]["x"].append(rng.uniform(0, 640)); feats[k]["y"].append(rng.uniform(0, 480)); feats[k]["ur"].append(-1.0); feats[k]["inf"].append(1.0)
    e_pt, e_kf, e_idx = [], [], []
    off = {(p, k): du for p, k, du in outliers}
    for p in range(npts):
        for k in views[p]:
            c = true_cams[k].astype(np.float64)
            q = c[:9].reshape(3, 3) @ np.asarray(obs_truth.get((p, k), X[p]), np.float64) + c[9:12]
            u, v = c[12] * q[0] / q[2] + c[14], c[13] * q[1] / q[2] + c[15]
            exact = (p, k) in [tuple(b) for b in behind] or (p, k) in obs_truth
            n = (0.0, 0.0) if exact else rng.normal(0, noise, 2)
            u, v = u + n[0] + off.get((p, k), 0.0), v + n[1]
            ur = (u - c[16] / q[2] + (0.0 if exact else rng.normal(0, noise))) if k in stereo_kfs else -1.0
            if k in stereo_kfs and ur < 0:
                ur = 0.0
            f = feats[k]
            e_pt.append(p); e_kf.append(k); e_idx.append(len(f["x"]))
            f["x"].append(u); f["y"].append(v); f["ur"].append(ur); f["inf"].append(inf_of.get((p, k), inf_scale.get(k, 1.0) / 1.2 ** (2 * ((p + k) % 4))))
    sc.feats = [{n: np.asarray(v, F32) for n, v in f.items()} for f in feats]
    sc.e_pt, sc.e_kf, sc.e_idx = (np.asarray(v, np.int32) for v in (e_pt, e_kf, e_idx))
    sc.ne = len(e_pt)
    # the start: shaken free poses and points
    shaken = true_cams.copy()
    for k in range(nf):
        shaken[k, 9:12] += rng.normal(0, pose_shake, 3).astype(F32)
    sc.cams = shaken
    sc.pos = (X + rng.normal(0, shake, X.shape)).astype(F32)
    for p, k in behind:
        sc.pos[p] = X[p].astype(F32)
    for p, v in start.items():
        sc.pos[p] = np.asarray(v, F32)
    sc.ids = (3 + 2 * np.arange(npts)).astype(np.int32)     # ids in the store
    sc.store_cap = 3 + 2 * max(npts, 1) + 5
    sc.p_ok = np.ones(npts, np.uint8)
    sc.p_ok[list(dropped)] = 0
    sc.obs = np.zeros((sc.ne, 4), F32)
    for e in range(sc.ne):
        f = sc.feats[sc.e_kf[e]]
        sc.obs[e] = (f["x"][sc.e_idx[e]], f["y"][sc.e_idx[e]], f["ur"][sc.e_idx[e]], f["inf"][sc.e_idx[e]])
    return sc


def sized(n_free=2, n_fixed=1, npts=20, obs_per_point=None, seed=7, kf_edges=None, **kw):
    """a scene at the edges of the sum shapes: obs_per_point keyframes see each point (round robin); kf_edges: keyframe 0 sees exactly that
    many points"""
    nk = n_free + n_fixed
    per = nk if obs_per_point is None else obs_per_point
    views = [[(p + q) % nk for q in range(per)] for p in range(npts)]
    if kf_edges is not None:
        views = [sorted(set([0] if p < kf_edges else []) | {1 + (p + q) % (nk - 1) for q in range(min(per, nk - 1))}) for p in range(npts)]
    else:
        views = [sorted(v) for v in views]
    return make(nk=nk, nf=n_free, npts=npts, seed=seed, views=views, **kw)


def lq1_scene():
    """L-Q1: fixed keyframe 6 stands at z = 6 and sees point 0 alone, which starts BEHIND it (z = -0.1) with an observation that projects
    exactly; keyframes 0 .. 2 observe point 0 where it truly is, IN FRONT of keyframe 6 (z = +0.1).  Point 1 carries two inconsistent edges
    of information 1e30 to fixed keyframes, so lambda of the first optimize() is huge and nothing else moves: the first check removes the
    edge of keyframe 6 for depth alone; the second optimize() carries point 0 through the plane and the final check keeps the edge."""
    nk, npts = 7, 40
    views = [[0, 1, 2, 6], [0, 1, 2, 3, 4]] + [list(range(6))] * (npts - 2)
    p1, p0 = [0.0, 0.05, 6.1], [0.0, 0.05, 5.9]
    return make(nk=nk, nf=3, npts=npts, seed=31, views=views, centers={6: [0.0, 0.0, 6.0]}, truth={0: p1}, start={0: p0}, shake=0.002, pose_shake=0.001,
                obs_truth={(0, 6): p0, (0, 0): p1, (0, 1): p1, (0, 2): p1}, inf_of={(0, 0): 1.0, (0, 1): 1.0, (0, 2): 1.0, (1, 3): 1e30, (1, 4): 1e30},
                outliers=[(1, 3, 5.0), (1, 4, -5.0)])


def every_scene():
    """(name, scene) for each rule"""
    out = []
    out.append(("chi2_first_mono", make(seed=2, outliers=[(5, 1, 40.0)])))
    out.append(("chi2_first_stereo", make(seed=3, stereo_kfs=(1, 4), outliers=[(7, 1, 40.0)])))
    out.append(("depth_alone_erased", make(seed=4, behind=[(9, 4)])))
    out.append(("depth_alone_survives", lq1_scene()))
    out.append(("bad_pivot", make(nk=3, nf=3, npts=12, seed=21, checks=False, iterations=(20, 0), robust=(False, False), inf_scale={0: 1e10})))
    out.append(("singular_point_block_ten_trials", make(seed=22, inf_scale={k: 0.0 for k in range(6)})))
    out.append(("mixed_mono_stereo", make(seed=5, stereo_kfs=(0, 2, 5), outliers=[(3, 0, -30.0), (11, 5, 25.0)])))
    out.append(("failed_trial_lambda_growth", make(seed=6, shake=0.6, pose_shake=0.15, noise=1.0)))
    out.append(("startup_two_keyframes", make(nk=2, nf=1, npts=60, seed=8, iterations=(20, 0), robust=(False, False), checks=False, shake=0.05)))
    out.append(("no_fixed_keyframe", make(nk=4, nf=4, seed=9)))
    out.append(("single_edge_point", make(seed=10, views=[[0]] + [list(range(6))] * 39)))
    out.append(("point_seen_by_fixed_only", make(seed=11, views=[[3, 4, 5]] + [list(range(6))] * 39)))
    out.append(("dropped_points", make(seed=12, dropped=(0, 17, 39))))
    out.append(("stop_before", make(seed=13, stop_at=0)))
    out.append(("stop_in_first", make(seed=13, stop_at=2)))
    out.append(("stop_in_second", make(seed=13, outliers=[(5, 1, 40.0)], stop_at=7)))
    out.append(("stop_global_ba", make(seed=13, checks=False, iterations=(10, 0), stop_at=3)))
    out.append(("empty_no_free", make(nk=3, nf=0, seed=14)))
    out.append(("empty_no_points", make(npts=0, seed=15)))
    out.append(("empty_all_dropped", make(npts=4, seed=16, dropped=(0, 1, 2, 3))))
    return out


def small_sized():
    """the sized scenes that the restatement itself solves"""
    out = {}
    for n in (63, 64, 65, 129):
        out["kf_edges_%d" % n] = sized(2, 2, n + 3, obs_per_point=2, kf_edges=n)
    for n in (1, 63, 64, 65):
        out["points_%d" % n] = sized(2, 1, n)
    for n in (1, 2):
        out["obs_per_point_%d" % n] = sized(2, 2, 30, obs_per_point=n)
    for n in (1, 2, 10, 11):
        out["free_%d" % n] = sized(n, 2, 30, obs_per_point=min(4, n + 2))
    return out


def large_sized():
    """device against the host program only"""
    return {"free_64": sized(64, 4, 200, obs_per_point=6), "obs_per_point_65": sized(3, 62, 8, obs_per_point=65),
            "kf_edges_129_stereo": sized(2, 2, 140, obs_per_point=2, kf_edges=129, stereo_kfs=(0, 2))}
