"""Constructed scenes for the Initializer tests (tests/test_init_ref_cpu.py, tests/test_gpu_init.py, tests/test_gpu_init_adapter.py): 3D
points projected by a known motion into two frames, with unmatched features in both, a permuted second frame, optional pixel noise and
gross outliers.  TEST INFRASTRUCTURE ONLY.  Every scene is named for the rule of tests/_init_ref.py it reaches; test_init_ref_cpu.py proves
that from the restatement's trace.  The seeds below were found by a seeded search with the restatement; the search is not kept."""
import functools

import numpy as np

import _init_ref as R

FX, FY, CX, CY = 500.0, 510.0, 320.0, 240.0


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def project(P):
    return FX * P[:, 0] / P[:, 2] + CX, FY * P[:, 1] / P[:, 2] + CY


def cloud(rng, n, z0=3.0, z1=8.0):
    z = rng.uniform(z0, z1, n)
    return np.stack([rng.uniform(-0.55, 0.55, n) * z, rng.uniform(-0.4, 0.4, n) * z, z], 1)


def plane(rng, n, depth=5.0, tilt=(0.15, -0.1)):
    x, y = rng.uniform(-2.5, 2.5, n), rng.uniform(-1.8, 1.8, n)
    return np.stack([x, y, depth + tilt[0] * x + tilt[1] * y], 1)


def build(P, Rm, t, seed, extra=(17, 23), noise=0.0, outliers=0, iterations=24, sigma=1.0, call_seed=7, repeat=0):
    """P [n][3] in camera 1; camera 2 sees Rm P + t.  extra: unmatched features of frame 1 / frame 2; outliers: that many matches get a
    random partner position; repeat: that many further matches copy the positions of match 0 exactly."""
    rng = np.random.default_rng(seed + 1000)
    n = len(P)
    u1, v1 = project(P)
    u2, v2 = project(P @ Rm.T + t)
    if noise:
        u1, v1, u2, v2 = (a + rng.normal(0, noise, n) for a in (u1, v1, u2, v2))
    for k in rng.choice(n, outliers, replace=False) if outliers else ():
        u2[k], v2[k] = rng.uniform(20, 620), rng.uniform(20, 460)
    if repeat:
        u1, v1, u2, v2 = (np.concatenate([a, np.full(repeat, a[0])]) for a in (u1, v1, u2, v2))
        n += repeat
    n1, n2 = n + extra[0], n + extra[1]
    x1, y1 = np.concatenate([u1, rng.uniform(0, 640, extra[0])]), np.concatenate([v1, rng.uniform(0, 480, extra[0])])
    x2, y2 = np.concatenate([u2, rng.uniform(0, 640, extra[1])]), np.concatenate([v2, rng.uniform(0, 480, extra[1])])
    p1, p2 = rng.permutation(n1), rng.permutation(n2)          # feature k of the construction is feature p1[k] / p2[k] of its frame
    X1, Y1, X2, Y2 = np.zeros(n1), np.zeros(n1), np.zeros(n2), np.zeros(n2)
    X1[p1], Y1[p1], X2[p2], Y2[p2] = x1, y1, x2, y2
    m = np.full(n1, -1, np.int32)
    m[p1[:n]] = p2[:n]
    sc = R.Scene(X1, Y1, X2, Y2, m, FX, FY, CX, CY, sigma=sigma, iterations=iterations, seed=call_seed)
    sc.true_R, sc.true_t = Rm, np.asarray(t, float)
    return sc


R_SMALL = rot(0.02, -0.03, 0.01)
T_SIDE = np.array([0.4, 0.05, 0.03])


def _cloud_n(n, iterations=8, seed=3):
    return build(cloud(np.random.default_rng(seed), n), R_SMALL, T_SIDE, seed, iterations=iterations)


def _garbage(n, seed):
    """matches between unrelated positions: whatever model 8 of them define, few points triangulate well"""
    rng = np.random.default_rng(seed)
    x1, y1, x2, y2 = rng.uniform(0, 640, n), rng.uniform(0, 480, n), rng.uniform(0, 640, n), rng.uniform(0, 480, n)
    return R.Scene(x1, y1, x2, y2, np.arange(n, dtype=np.int32), FX, FY, CX, CY, iterations=4, seed=seed)


def _mixed(seed, n_plane, n_off):
    rng = np.random.default_rng(seed)
    P = np.concatenate([plane(rng, n_plane), cloud(rng, n_off, 4.0, 6.5)])
    return build(P, R_SMALL, T_SIDE, seed, noise=0.5, iterations=16)


SCENES = {
    # RH > 0.40 and ReconstructH succeeds: the mirror solution of the plane puts enough points behind a camera
    "plane": lambda: build(plane(np.random.default_rng(1), 120, 5.0, (-0.58, 0.35)), rot(0.078, 0.087, -0.028), np.array([0.05, -0.38, -0.03]), 1,
                           noise=0.2, iterations=16),
    "cloud": lambda: build(cloud(np.random.default_rng(2), 120), R_SMALL, T_SIDE, 2, noise=0.2),
    # a unique winner whose 50th smallest cosine is above cos(1 degree): parallax about 0.6 degrees, so the depth tests still apply
    "low_parallax": lambda: build(cloud(np.random.default_rng(12), 100, 3.0, 7.0), np.eye(3), np.array([0.06, 0.0, 0.0]), 12, sigma=0.2),
    # a pure rotation never reaches the parallax rule as the rules are written: every point has cosParallax >= minCos, the depth tests
    # are skipped, nGood counts the points for several hypotheses and the call is rejected as ambiguous first
    "pure_rotation": lambda: build(cloud(np.random.default_rng(4), 100), rot(0.03, 0.05, -0.02), np.zeros(3), 4, noise=0.3),
    "few_good": lambda: build(cloud(np.random.default_rng(5), 40), R_SMALL, T_SIDE, 5),
    # both solutions of the homography decomposition triangulate the plane in front of both cameras
    "ambiguous": lambda: build(plane(np.random.default_rng(1), 120), R_SMALL, T_SIDE, 1, noise=0.2),
    "d_ratio": lambda: build(cloud(np.random.default_rng(8), 80), rot(0.03, 0.05, -0.02), np.zeros(3), 8),
    "outliers": lambda: build(cloud(np.random.default_rng(9), 120), R_SMALL, T_SIDE, 9, noise=0.1, outliers=30, iterations=60),
    # 6 further matches repeat match 0: an 8-set that draws two of the 7 equal pairs leaves ComputeF21's system rank deficient
    "repeated": lambda: build(cloud(np.random.default_rng(10), 24), R_SMALL, T_SIDE, 10, repeat=6, iterations=40),
    "all_repeated": lambda: build(cloud(np.random.default_rng(11), 1), R_SMALL, T_SIDE, 11, repeat=7, iterations=3),
    "rh_above": lambda: _mixed(67, 60, 40),    # RH = 0.40012
    "rh_below": lambda: _mixed(40, 60, 40),    # RH = 0.39820
    "iter200": lambda: _cloud_n(30, 200),
}
for _n in (7, 8, 9, 63, 64, 65, 129):
    SCENES["n%d" % _n] = functools.partial(_cloud_n, _n)
for _it in (1, 63, 64, 65):
    SCENES["iter%d" % _it] = functools.partial(_cloud_n, 30, _it)
for _k in (50, 51, 52):
    SCENES["cos%d" % _k] = functools.partial(_cloud_n, _k, 8, 30 + _k)
SCENES["cos1"] = lambda: _garbage(8, 103)   # the winning motion hypothesis pushes exactly one cosine


@functools.lru_cache(maxsize=None)
def scene(name):
    return SCENES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's answer, computed once per process and shared by the tests; treat it as read-only"""
    return R.initialize(scene(name))


def motion_error(Rm, t, true_R, true_t):
    """(rotation angle between Rm and true_R, angle between the translation directions), radians, float64"""
    Rm, t = np.asarray(Rm, float).reshape(3, 3), np.asarray(t, float).reshape(3)
    c = (np.trace(Rm.T @ true_R) - 1.0) / 2.0
    ct = float(t @ true_t) / (np.linalg.norm(t) * np.linalg.norm(true_t))
    return float(np.arccos(np.clip(c, -1, 1))), float(np.arccos(np.clip(ct, -1, 1)))
