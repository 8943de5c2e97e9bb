"""Seeded worlds and constructed scenes for Sim3Solver (tests/_sim3_ref.py is what they are judged by).  TEST INFRASTRUCTURE ONLY.

A scene is what one candidate of afv_table_sim3_hypotheses reads: the two keyframes (poses, intrinsics, the sigma2 planes of their table
slots), the store (positions and flags per point id) and the rows mp1 / mp2 / idx1 / idx2 over the features of keyframe 1.

World: two keyframe poses, points in front of both, a planted Sim3 (X3Dc1 = s * R12 * X3Dc2 + t12), a share of outliers, pixel noise on
or off.  Feature i of keyframe 1 carries point id i; its match is point id n1 + i, which keyframe 2 sees as feature idx2[i] (a
permutation).  The constructed scenes (one per rule) are functions below; each says in its docstring which rule it reaches and
tests/test_sim3_ref_cpu.py checks that it does.
"""
import numpy as np

import _sim3_ref as R

f32 = np.float32


def _rot(rng, max_angle):
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    a = rng.uniform(-max_angle, max_angle)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K


class Scene:
    """one candidate.  n1 / n2: features of the two keyframes; P: the store's capacity"""

    def __init__(self, cam1, cam2, pos, flags, sigma2_1, sigma2_2, mp1, mp2, idx2, idx1=None, fix_scale=False, seed=0):
        self.cam1, self.cam2 = cam1, cam2
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self.flags = np.ascontiguousarray(flags, np.uint8)
        self.sigma2_1, self.sigma2_2 = np.ascontiguousarray(sigma2_1, np.float32), np.ascontiguousarray(sigma2_2, np.float32)
        self.mp1, self.mp2, self.idx2 = (np.ascontiguousarray(v, np.int32) for v in (mp1, mp2, idx2))
        self.idx1 = None if idx1 is None else np.ascontiguousarray(idx1, np.int32)
        self.n1, self.n2 = len(self.sigma2_1), len(self.sigma2_2)
        self.fix_scale, self.seed = bool(fix_scale), int(seed)
        assert len(self.mp1) == len(self.mp2) == len(self.idx2) == self.n1

    def gather(self):
        return R.gather(self.cam1, self.cam2, self.pos, self.flags, self.sigma2_1, self.sigma2_2, self.mp1, self.mp2, self.idx1, self.idx2, self.n1)

    def hypothesis(self, h, G=None):
        return R.hypothesis(G or self.gather(), self.cam1, self.cam2, self.fix_scale, self.seed, h)

    def candidate(self, cap, nhyp, mask_words):
        return R.candidate(self.cam1, self.cam2, self.pos, self.flags, self.sigma2_1, self.sigma2_2, self.mp1, self.mp2, self.idx1, self.idx2,
                           self.n1, cap, self.fix_scale, self.seed, nhyp, mask_words)

    def solver(self, ref, nhyp):
        """the restated class over a `candidate` answer"""
        fl = lambda h: [bool((int(ref["inliers"][h][k >> 5]) >> (k & 31)) & 1) for k in range(ref["n"])]
        return R.Solver(ref["n"], ref["index1"], ref["count"], ref["sim3"], fl, self.n1, nhyp)


def identity_cam(fx=500.0, fy=500.0, cx=320.0, cy=240.0):
    return R.Cam(np.eye(3), np.zeros(3), fx, fy, cx, cy)


def world(seed, n=40, s=1.0, outliers=0.0, noise=0.0, fix_scale=False, extra2=5, levels=True):
    """a seeded world of n correspondences (all valid).  outliers: share whose point of map 2 is somewhere else; noise: sigma of the
    pixel noise on the point of map 2 as keyframe 1 sees it (0 = none)"""
    rng = np.random.default_rng(seed)
    R1, R2 = _rot(rng, 0.4), _rot(rng, 0.4)
    t1, t2 = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3)
    cam1 = R.Cam(R1, t1, 520.0, 515.0, 318.5, 241.25)
    cam2 = R.Cam(R2, t2, 480.0, 485.0, 322.0, 238.5)
    X1 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    R12, t12 = _rot(rng, 0.5), rng.uniform(-0.5, 0.5, 3)
    if fix_scale:
        s = 1.0
    X1n = X1.copy()
    if noise:
        X1n[:, :2] += rng.normal(0, noise, (n, 2)) * X1[:, 2:3] / 500.0
    X2 = ((X1n - t12) @ R12) / s                                   # R12^T (X1 - t12) / s
    bad = rng.permutation(n)[:int(round(outliers * n))]
    X2[bad] = np.stack([rng.uniform(-2, 2, len(bad)), rng.uniform(-1.5, 1.5, len(bad)), rng.uniform(3, 9, len(bad)) / s], 1)
    Xw1 = (X1 - t1) @ R1                                           # Rcw^T (Xc - tcw), in double, then the store's floats
    Xw2 = (X2 - t2) @ R2
    n2 = n + extra2
    lev1, lev2 = (rng.integers(0, 8, n), rng.integers(0, 8, n2)) if levels else (np.zeros(n, int), np.zeros(n2, int))
    sc = Scene(cam1, cam2, np.concatenate([Xw1, Xw2]), np.full(2 * n, R.SET, np.uint8), f32(1.2) ** (2 * lev1), f32(1.2) ** (2 * lev2),
               np.arange(n), n + np.arange(n), rng.permutation(n2)[:n], fix_scale=fix_scale, seed=seed * 7919 + 11)
    sc.planted = dict(R12=R12, t12=t12, s=s, outliers=set(int(b) for b in bad))
    return sc


def skip_reasons(seed=3, n=24):
    """every skip reason of the constructor once, plus an id the store holds no point for.  sc.skipped: {feature: reason}"""
    sc = world(seed, n)
    sc.idx1 = np.arange(n, dtype=np.int32)
    sc.skipped = {2: "no mp2", 5: "no mp1", 7: "bad 1", 11: "bad 2", 13: "idx1 < 0", 17: "idx2 < 0", 19: "never set 2"}
    sc.mp2[2] = -1
    sc.mp1[5] = -1
    sc.flags[sc.mp1[7]] |= R.BAD
    sc.flags[sc.mp2[11]] |= R.BAD
    sc.idx1[13] = -1
    sc.idx2[17] = -1
    sc.flags[sc.mp2[19]] = 0
    return sc


def q1_bound(above):
    """Q1: correspondence K sits d = sqrt(13.5) px from its partner in keyframe 1; 9.210 * sigma2 is 13.999 (bound 13: outlier although
    13.5 < 13.999) or, `above`, 14.001 (bound 14: inlier).  Its second bound is wide.  Noise-free otherwise."""
    n, K = 12, 5
    sc = world(21, n, levels=False)
    G = sc.gather()
    x1 = np.array(G["x1"][K], np.float64)
    x1[0] += np.sqrt(13.5) * x1[2] / float(sc.cam1.fx)
    P = sc.planted
    X2 = ((x1 - P["t12"]) @ P["R12"]) / P["s"]
    sc.pos[sc.mp2[K]] = ((X2 - sc.cam2.tcw.astype(np.float64)) @ sc.cam2.Rcw.reshape(3, 3).astype(np.float64)).astype(np.float32)
    sc.idx1 = np.arange(n, dtype=np.int32)
    sc.sigma2_1[K] = f32((14.001 if above else 13.999) / 9.210)
    sc.sigma2_2[sc.idx2[K]] = f32(100.0)
    sc.K = K
    return sc


def dyadic(points1, t12, fix_scale=True, seed=5):
    """identity poses, map 2 = map 1 - t12, coordinates that are exact in float: every X3Dc is its stored position"""
    p1 = np.array(points1, np.float32)
    p2 = p1 - np.array(t12, np.float32)
    n = len(p1)
    return Scene(identity_cam(), identity_cam(), np.concatenate([p1, p2]), np.full(2 * n, R.SET, np.uint8), np.ones(n, np.float32),
                 np.ones(n, np.float32), np.arange(n), n + np.arange(n), np.arange(n), fix_scale=fix_scale, seed=seed)


def coincident(fix_scale):
    """S5: N = 3 and the three points coincide: Pr1 = Pr2 = 0, N = 0, R12 = I, den == 0: degenerate when the scale is estimated; with the
    scale fixed the hypothesis is a translation and counts all three"""
    return dyadic([[0.5, -0.25, 4.0]] * 3, [0.25, 0.0, 0.5], fix_scale)


def collinear():
    """three collinear sample points (N = 3): Horn's N has a double largest eigenvalue; the answer is finite, the rotation about the line
    is whatever S2's fixed order gives, the hypothesis is NOT flagged and counts the three points"""
    return dyadic([[-1.0, 0.5, 4.0], [0.0, 0.5, 5.0], [1.0, 0.5, 6.0]], [0.25, -0.5, 0.5], False)


def z_zero(under_t21):
    """z = 0 under T12 (or, `under_t21`, T21) for correspondence K of hypothesis 0: invz = inf, the error is not finite, no inlier.
    Identity poses, a pure translation, fixed scale, coordinates in 64ths whose sums over the three sample points divide by 3: the
    centroids, Pr1 = Pr2 and M are exact, M is symmetric, R12 = I exactly, so z = Z + t[2] and Z = -t[2] makes it +0"""
    rng = np.random.default_rng(8)
    n, seed = 10, 5
    picks = R.sample3(seed, 0, n)
    ints = np.stack([rng.integers(-128, 128, n), rng.integers(-64, 64, n), rng.integers(192, 512, n)], 1)
    ints[picks[2]] -= ints[picks].sum(0) % 3
    sc = dyadic(ints / 64.0, [0.25, -0.125, 0.5], seed=seed)
    K = [k for k in range(n) if k not in picks][0]
    S = sc.hypothesis(0)["solve"]
    assert S["R"] == [1, 0, 0, 0, 1, 0, 0, 0, 1]
    if under_t21:
        sc.pos[sc.mp1[K], 2] = -S["ti"][2]
    else:
        sc.pos[sc.mp2[K], 2] = -S["t"][2]
    sc.K = K
    return sc


def counted(m, n_out=2, seed=31):
    """Q2: exactly m correspondences agree with the planted transform, n_out are far off: every hypothesis counts at most m"""
    sc = world(seed, m + n_out, levels=False)
    rng = np.random.default_rng(seed + 1)
    for k in range(m, m + n_out):
        sc.pos[sc.mp2[k]] += rng.uniform(1.0, 2.0, 3).astype(np.float32)
    return sc
