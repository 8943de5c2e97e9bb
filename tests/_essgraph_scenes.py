"""Constructed essential graphs for tests/_essgraph_ref.py, each named for the rule it reaches; tests/test_essgraph_ref_cpu.py proves from
the restatement's branch counter or trace that it does.  A scene is a dict: S_init (R [nk, 3, 3], t [nk, 3], s [nk]), fixed, v0, v1, meas (R, t,
s over the edges), fix_scale, iterations, and, where one exists, truth: the estimate the measurements are consistent with.
Scene construction may use libm: the scene is data, not arithmetic under test."""
import numpy as np

import _essgraph_ref as G

F64 = np.float64


def rot(w):
    w = np.asarray(w, F64)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], F64)
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def pack(lst):
    """[(R, t, s)] -> (R [n, 3, 3], t [n, 3], s [n])"""
    return (np.array([e[0] for e in lst], F64).reshape(-1, 3, 3), np.array([e[1] for e in lst], F64).reshape(-1, 3),
            np.array([e[2] for e in lst], F64).reshape(-1))


def scene(S_init, fixed, edges, meas_from, fix_scale=False, iterations=20, truth=None, meas=None):
    """edges [(v0, v1)]; the measurement of an edge is S(v1) * S(v0)^-1 over meas_from (a list of Sim3) unless meas gives it"""
    v0 = np.array([e[0] for e in edges], np.int32)
    v1 = np.array([e[1] for e in edges], np.int32)
    if meas is None:
        meas = [G.relative(meas_from[b], meas_from[a]) for a, b in edges]
    return dict(S_init=pack(S_init), fixed=int(fixed), v0=v0, v1=v1, meas=pack(meas), fix_scale=bool(fix_scale), iterations=int(iterations),
                truth=None if truth is None else pack(truth))


def problem(sc):
    return G.Problem(sc["S_init"], sc["fixed"], sc["v0"], sc["v1"], sc["meas"], sc["fix_scale"])


def circle(n, scale_end=1.0, tilt=0.02):
    """n keyframes looking along a circle: the truth of the chain scenes; the scale grows linearly to scale_end"""
    out = []
    for k in range(n):
        a = 2.0 * np.pi * k / n
        R = rot([tilt * np.sin(a), 0.1 * np.cos(3 * a), a])
        t = np.array([2.0 * np.cos(a), 2.0 * np.sin(a), 0.1 * k])
        s = 1.0 + (scale_end - 1.0) * k / max(n - 1, 1)
        out.append((R, s * (-R @ t), s))
    return out


def band_edges(n, band, loop=True, order=1):
    """the chain: keyframe i is joined with i - 1 .. i - 1 - band (v0 = the later one, as the reference's spanning tree and covisibility
    edges are), then the loop edge from the last to the first"""
    e = [(i, j) if order else (j, i) for i in range(n) for j in range(i - 1, max(i - 2 - band, -1), -1)]
    if loop and n > 2:
        e = [(n - 1, 0)] + e
    return e


def drifted(n=12, band=1, fixed=0, fix_scale=False, drift=0.01, iterations=20, edges=None, scale_end=1.1):
    """a drifted loop: the measurements are those of the truth; the initial estimates drift away from it at scale 1, and the last keyframe
    carries its CorrectedSim3 (the truth: scale 1.1 and its rotation)"""
    truth = circle(n, scale_end)
    init = []
    for k, (R, t, s) in enumerate(truth):
        if k in (fixed, n - 1):
            init.append((R, t, s))
        else:
            D = rot([drift * k, -0.5 * drift * k, 0.3 * drift * k])
            init.append((D @ R, t / s + drift * k * np.array([0.3, -0.2, 0.1]), 1.0))
    return scene(init, fixed, band_edges(n, band) if edges is None else edges, truth, fix_scale, iterations, truth)


def log_branches():
    """four edges from the fixed vertex 0, the error of edge b in branch b of Sim3::log at the initial estimate"""
    I = (np.eye(3), np.zeros(3), 1.0)
    us = [([1e-6, 0, 0], 1e-6), ([0.3, -0.2, 0.5], 2e-6), ([0, 2e-6, 0], 0.2), ([0.4, 0.1, -0.3], -0.3)]
    meas = [(rot(w), np.array([0.5, -0.25, 0.125]), float(np.exp(sg))) for w, sg in us]
    return scene([I] * 5, 0, [(k + 1, 0) for k in range(4)], None, meas=meas)


def consistent():
    """dyadic translations, no rotation, scale 1: every product is exact, chi2 is exactly 0 and the step exactly zero (G-Q1)"""
    S = [(np.eye(3), np.array([0.5 * k, -0.25 * k, 2.0 * k]), 1.0) for k in range(6)]
    return scene(S, 0, band_edges(6, 1), S, truth=S)


def rejected():
    """initial estimates far from the truth (rotations off by more than a radian): a Gauss-Newton-sized first step overshoots"""
    return drifted(8, 1, drift=0.35)


def floating():
    """vertices 4 and 5 are joined with each other but with nothing else: their 14 x 14 system is singular but for lambda"""
    truth = circle(6, 1.05)
    init = [(rot([0.02 * k, 0, 0]) @ R, t, 1.0) if k else (R, t, s) for k, (R, t, s) in enumerate(truth)]
    return scene(init, 0, [(1, 0), (2, 1), (3, 2), (3, 0), (5, 4)], truth, truth=None)


def isolated():
    """vertex 3 has no edge: its block holds lambda alone and its step is 0"""
    truth = circle(6, 1.05)
    init = [(rot([0.02 * k, 0, 0]) @ R, t, 1.0) if k else (R, t, s) for k, (R, t, s) in enumerate(truth)]
    return scene(init, 0, [(1, 0), (2, 1), (4, 2), (5, 4), (5, 0)], truth)


def double_edges():
    """the pair (2, 1) is joined by three edges, in both orientations; the pair (3, 0) by two onto the fixed vertex"""
    truth = circle(5, 1.05)
    init = [(rot([0.02 * k, 0.01, 0]) @ R, t, 1.0) if k else (R, t, s) for k, (R, t, s) in enumerate(truth)]
    return scene(init, 0, [(4, 0), (1, 0), (2, 1), (1, 2), (2, 1), (3, 2), (4, 3), (3, 0), (0, 3)], truth, truth=truth)


def onto_fixed():
    """every edge has the fixed vertex at one end, on either side"""
    truth = circle(5, 1.1)
    init = [(rot([0.0, 0.03 * k, 0]) @ R, t * 1.01, 1.0) if k != 2 else (R, t, s) for k, (R, t, s) in enumerate(truth)]
    return scene(init, 2, [(0, 2), (2, 1), (3, 2), (2, 4)], truth, truth=truth)


def not_finite():
    """the error of the one edge is a rotation by exactly pi: theta / (2 sqrt(1 - d d)) is a division by zero (G5)"""
    I = (np.eye(3), np.zeros(3), 1.0)
    return scene([I, I], 0, [(1, 0)], None, meas=[(np.diag([1.0, -1.0, -1.0]), np.zeros(3), 1.0)])


SCENES = {
    "log_branches": log_branches,
    "consistent": consistent,
    "drifted_loop": lambda: drifted(12, 3),
    "drifted_stall": lambda: drifted(12, 1),
    "fix_scale_on": lambda: drifted(8, 1, fix_scale=True),
    "fixed_first": lambda: drifted(7, 1, fixed=0),
    "fixed_middle": lambda: drifted(7, 1, fixed=3),
    "fixed_last": lambda: drifted(7, 1, fixed=6),
    "rejected": rejected,
    "floating": floating,
    "isolated": isolated,
    "double_edges": double_edges,
    "onto_fixed": onto_fixed,
    "not_finite": not_finite,
}

_cache = {}


def solved(name):
    """the scene, its problem and the restatement's answer with its trace, computed once and shared"""
    if name not in _cache:
        sc = SCENES[name]()
        pr = problem(sc)
        log = []
        _cache[name] = (sc, pr, G.essential_graph(pr, sc["iterations"], log=log), log)
    return _cache[name]


def points_for(sc, n=40, seed=5, cap=64):
    """a small store beside a scene: pos [cap, 3] float32, flags [cap], ids [n], ref [n] (a position in the keyframe list, -1 for some), with
    bad and unset points among them"""
    rng = np.random.default_rng(seed)
    nk = len(sc["S_init"][2])
    pos = rng.uniform(-3, 3, (cap, 3)).astype(np.float32)
    flags = np.full(cap, G.SET, np.uint8)
    ids = rng.permutation(cap)[:n].astype(np.int32)
    ref = rng.integers(0, nk, n).astype(np.int32)
    if n >= 6:
        flags[ids[1]] |= G.BAD
        flags[ids[3]] = 0
        ref[4] = -1
    return pos, flags, ids, ref
