"""constructed scenes for the projection-guided searches (test data; no extractor, no GPU)

Every generator is deterministic (LCG of afv.synth, no global RNG state) and returns a list of Case(name, kind, F, Q, kw, rule): F / Q are the
FrameGridView / ProjectionQueries the searches take, kw the arguments of oracle.match_projection / match_initialization, `rule` the name
of the comparison (a key of _proj_ref.FLIPS) the scene sits on.  tests/test_proj_ref_cpu.py proves on the CPU that each scene reaches its
rule at equality and that its outcome depends on it; tests/test_gpu_proj_scenes.py runs them through the kernels.

Descriptors are built from DISTANCES: a query is the `base` row, a feature is the base with `d` bits flipped (binary rows) or with an
integer offset vector whose squares sum to `d` (float rows: every L2^2 is a small integer, exact in any summation order).  `variant`
moves the flipped bits / permutes the offset, so that several features can sit at the same distance without being equal.
(The summation order of the float distance is tested in tests/_l2_scenes.py, on rows that tell orders apart.)
Coordinates that must sit exactly on an edge are found with np.nextafter against the expression the reference evaluates, in float32.
"""
import collections
import importlib
import math
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)
afv = importlib.import_module("anyfeature-vslam_amd")
S = afv.synth
f32 = np.float32
Case = collections.namedtuple("Case", "name kind F Q kw rule")

DESCS = ("b32", "b61", "f8", "f64")
TH = 75.0


def _four_squares(d):
    for a in range(int(math.isqrt(d)), -1, -1):
        for b in range(int(math.isqrt(d - a * a)), -1, -1):
            for c in range(int(math.isqrt(d - a * a - b * b)), -1, -1):
                e = d - a * a - b * b - c * c
                r = math.isqrt(e)
                if r * r == e:
                    return [a, b, c, r]
    raise ValueError(d)


def base_row(desc):
    if desc[0] == "b":
        return S.lcg_bytes(4242, int(desc[1:])).copy()
    return (S.lcg_states(4243, int(desc[1:])) % 7).astype(np.float32)


def row_at(desc, d, variant=0):
    """a row at distance d (Hamming / L2^2) from base_row(desc)"""
    b = base_row(desc).copy()
    if desc[0] == "b":
        nbits = 8 * len(b)
        for k in range(int(d)):
            bit = (variant * 37 + k) % nbits
            b[bit >> 3] ^= np.uint8(1 << (bit & 7))
        return b
    off = _four_squares(int(d))
    for k, o in enumerate(off):
        b[(variant + 2 * k) % len(b)] += f32(o if (variant >> k) & 1 == 0 else -o)
    return b


def rows(desc, dists, variants=None):
    variants = variants if variants is not None else list(range(len(dists)))
    return np.stack([row_at(desc, d, v) for d, v in zip(dists, variants)]) if len(dists) else np.zeros((0, len(base_row(desc))), base_row(desc).dtype)


GRIDS = {
    "default": dict(min_x=0.0, min_y=0.0, max_x=640.0, max_y=480.0, grid_cols=64, grid_rows=48),
    # an "undistorted" frame: bounds outside the image, non-integer cells (tests/test_gpu_frame.py::test_undistorted_keypoints_rebuild_the_grid)
    # (x: 64 / 660 per pixel, no float32 x lands on a half cell left of min_x; y: 48 / 480 with min_y < 0, where one does)
    "undist": dict(min_x=-8.0, min_y=-6.0, max_x=652.0, max_y=474.0, grid_cols=64, grid_rows=48),
    "coarse": dict(min_x=0.0, min_y=0.0, max_x=640.0, max_y=480.0, grid_cols=8, grid_rows=6),
}


def _frame(desc, feats, grid="default", **extra):
    """feats: list of dicts x, y, d, and optionally v (variant), size, angle, occ, ur, inf"""
    n = len(feats)
    g = lambda k, dflt: np.array([f.get(k, dflt) for f in feats], np.float32) if n else np.zeros(0, np.float32)
    D = rows(desc, [f["d"] for f in feats], [f.get("v", i) for i, f in enumerate(feats)])
    kw = dict(GRIDS[grid])
    kw.update(extra)
    F = afv.FrameGridView(D, np.stack([g("x", 0), g("y", 0)], 1) if n else np.zeros((0, 2), np.float32), g("size", 1.0), angles=g("angle", 0.0), **kw)
    if any("occ" in f for f in feats):
        F.occupied = np.array([f.get("occ", 0) for f in feats], np.uint8)
    if any("ur" in f for f in feats):
        F.u_right = g("ur", -1.0)
    if any("inf" in f for f in feats):
        F.inf = g("inf", 1.0)
    return F


def _queries(desc, qs):
    """qs: list of dicts u, v, r and optionally min, max, angle, occupies, valid, ur, er, d / dv (the query's own distance from the base)"""
    n = len(qs)
    g = lambda k, dflt: np.array([q.get(k, dflt) for q in qs], np.float32)
    D = rows(desc, [q.get("d", 0) for q in qs], [q.get("dv", 0) for q in qs])
    Q = afv.ProjectionQueries(D, g("u", 0), g("v", 0), g("r", 5), g("min", 0.5), g("max", 2.0), angles=g("angle", 0.0))
    if any("occupies" in q for q in qs):
        Q.occupies = np.array([q.get("occupies", 1) for q in qs], np.uint8)
    if any("valid" in q for q in qs):
        Q.valid = np.array([q.get("valid", 1) for q in qs], np.uint8)
    if any("ur" in q for q in qs):
        Q.ur, Q.er_max = g("ur", 0.0), g("er", 0.0)
    return Q


def _kinds(kinds, name, desc, F, Q, rule, **kw):
    """one Case per search kind the scene applies to: L = local map, T = last frame (tracking), U = Fuse, I = initialization"""
    out = []
    for k in kinds:
        if k == "L":
            out.append(Case("%s-%s-localmap" % (name, desc), "proj", F, Q, dict(dict(th_high=TH, nnratio=0.8, last_frame=False), **kw), rule))
        elif k == "T":
            out.append(Case("%s-%s-lastframe" % (name, desc), "proj", F, Q, dict(dict(th_high=TH, nnratio=0.9, last_frame=True), **kw), rule))
        elif k == "U":
            out.append(Case("%s-%s-fuse" % (name, desc), "proj", F, Q, dict(th_high=TH, fuse=True), rule))
        else:
            ikw = {a: b for a, b in kw.items() if a in ("nnratio", "check_orientation")}
            out.append(Case("%s-%s-init" % (name, desc), "init", F, Q, dict(dict(th_low=TH, nnratio=0.9, check_orientation=False), **ikw), rule))
    return out


def _below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def _above(v):
    return np.nextafter(f32(v), f32(np.inf))


def solve(expr, target, x0, steps=4096):
    """the float32 x nearest x0 with expr(x) == target (expr monotonic non-decreasing), or None"""
    x = f32(x0)
    for _ in range(steps):
        v = expr(x)
        if v == target:
            return x
        x = _above(x) if v < target else _below(x)
    return None


# ---- item 3: exact edges of the geometric filters ----
def geometric_edges(desc="b32", grid="default"):
    G = GRIDS[grid]
    Fp = afv.FrameGridView(np.zeros((0, 32), np.uint8), np.zeros((0, 2), np.float32), [], **G)
    mnx, mny, iw, ih = Fp.min_x, Fp.min_y, Fp.grid_inv_w, Fp.grid_inv_h
    cols, rws = G["grid_cols"], G["grid_rows"]
    out = []
    ox = 0.25 if grid == "undist" else 0.0   # non-integer but exactly representable coordinates
    # |dx| == r / |dy| == r: the edge feature (distance 0) is out, the decoy (distance 10) wins; one ulp inside it is in
    for rule, ax in (("dx_lt_r", 0), ("dy_lt_r", 1)):
        feats, qs = [], []
        for j, (inside, sign) in enumerate([(False, 1), (False, -1), (True, 1), (True, -1)]):
            u, v, r = 100.0 + 60 * j + ox, 100.0 + ox, 5.5
            e = (u if ax == 0 else v) + sign * r
            if inside:
                e = _below(e) if sign > 0 else _above(e)
            feats.append(dict(x=e if ax == 0 else u, y=v if ax == 0 else e, d=0))
            feats.append(dict(x=u + 1, y=v + 1, d=10))
            qs.append(dict(u=u, v=v, r=r))
        out += _kinds("LTUI", rule, desc, _frame(desc, feats, grid), _queries(desc, qs), rule)
    # size == min / max is in; one ulp outside is out
    for rule, key in (("size_lt_min", "min"), ("size_gt_max", "max")):
        feats, qs = [], []
        for j, outside in enumerate([False, True]):
            u, v = 100.0 + 60 * j + ox, 200.0 + ox
            lim = f32(0.8333333) if key == "min" else f32(1.2)
            sz = lim if not outside else (_below(lim) if key == "min" else _above(lim))
            feats.append(dict(x=u, y=v, d=0, size=sz))
            feats.append(dict(x=u + 1, y=v + 1, d=10, size=1.0))
            qs.append(dict(u=u, v=v, r=5.0, **{key: lim}))
        out += _kinds("LTUI", rule, desc, _frame(desc, feats, grid), _queries(desc, qs), rule)
    # PosInGrid at k + 0.5 (half away from zero).  Inside the grid the cell decides the visiting order, so two features at the same
    # distance: the lower index sits squarely in cell k + 1, the half-way one lands in k + 1 as well (visited second) - rounded towards
    # zero it would land in cell k and be visited first.  Left of min_x the same rule decides whether the feature is in the grid at all.
    feats, qs = [], []
    k = 20
    xh = solve(lambda x: (x - mnx) * iw, f32(k + 0.5), (k + 0.5) / float(iw) + float(mnx))
    yh = solve(lambda y: (y - mny) * ih, f32(k + 0.5), (k + 0.5) / float(ih) + float(mny))
    assert xh is not None and yh is not None
    feats += [dict(x=xh + f32(3), y=100.0, d=5, v=1), dict(x=xh, y=100.0, d=5, v=2)]
    qs.append(dict(u=xh + f32(1), v=100.0, r=6.0))
    feats += [dict(x=300.0, y=yh + f32(3), d=5, v=1), dict(x=300.0, y=yh, d=5, v=2)]
    qs.append(dict(u=300.0, v=yh + f32(1), r=6.0))
    xn = solve(lambda x: (x - mnx) * iw, f32(-0.5), -0.5 / float(iw) + float(mnx))
    yn = solve(lambda y: (y - mny) * ih, f32(-0.5), -0.5 / float(ih) + float(mny))
    assert yn is not None   # (the x side exists where 1 / inv_w is friendly)
    if xn is not None:
        feats.append(dict(x=xn, y=400.0, d=0)); qs.append(dict(u=xn + f32(1), v=400.0, r=6.0))
    feats.append(dict(x=500.0, y=yn, d=0)); qs.append(dict(u=500.0, v=yn + f32(1), r=6.0))
    out += _kinds("LTUI", "pos_round", desc, _frame(desc, feats, grid), _queries(desc, qs), "pos_round")
    # floor / ceil of the window exactly on a cell border: the border cell k is in the window; the feature just inside it would be lost if it
    # were not
    for rule, sign in (("win_floor", -1), ("win_ceil", 1)):
        feats, qs = [], []
        k, r = 30, f32(7.0)
        u = solve(lambda x: (x - mnx + f32(sign) * r) * iw, f32(k), (k / float(iw)) + float(mnx) - sign * 7.0)
        v = solve(lambda y: (y - mny + f32(sign) * r) * ih, f32(k), (k / float(ih)) + float(mny) - sign * 7.0)
        assert u is not None and v is not None
        e = u + f32(sign) * r
        feats.append(dict(x=e - f32(sign) * f32(0.5), y=50.0, d=0)); qs.append(dict(u=u, v=50.0, r=r))
        e = v + f32(sign) * r
        feats.append(dict(x=50.0, y=e - f32(sign) * f32(0.5), d=0)); qs.append(dict(u=50.0, v=v, r=r))
        out += _kinds("LTUI", rule, desc, _frame(desc, feats, grid), _queries(desc, qs), rule)
    # windows clipped on each side (matching a feature in the border cell) and windows just outside each side (skipped)
    W, H = cols / float(iw), rws / float(ih)
    x_last = float(mnx) + (cols - 1) / float(iw)   # centre of the last column of cells
    y_last = float(mny) + (rws - 1) / float(ih)
    sides = {
        "skip_cx0": [dict(u=x_last + 2, v=200.0, r=1.0, fx=x_last + 2.5, fy=200.0), dict(u=float(mnx) + W + 30, v=200.0, r=5.0)],
        "skip_cx1": [dict(u=float(mnx) - 4, v=200.0, r=4.0, fx=float(mnx) - 1, fy=200.0), dict(u=float(mnx) - 60, v=200.0, r=5.0)],
        "skip_cy0": [dict(u=200.0, v=y_last + 2, r=1.0, fx=200.0, fy=y_last + 2.5), dict(u=200.0, v=float(mny) + H + 30, r=5.0)],
        "skip_cy1": [dict(u=200.0, v=float(mny) - 4, r=4.0, fx=200.0, fy=float(mny) - 1), dict(u=200.0, v=float(mny) - 60, r=5.0)],
    }
    for rule, (hit, miss) in sides.items():
        feats = [dict(x=hit["fx"], y=hit["fy"], d=0), dict(x=320.0, y=240.0, d=3)]
        qs = [dict(u=hit["u"], v=hit["v"], r=hit["r"]), dict(u=miss["u"], v=miss["v"], r=miss["r"]), dict(u=320.0, v=240.0, r=5.0)]
        out += _kinds("LTUI", rule, desc, _frame(desc, feats, grid), _queries(desc, qs), rule)
    # stereo: mvuRight == 0 exactly (projection: no gate, Fuse: the 3-dof gate) and |ur - mvuRight| == gate (kept)
    feats = [dict(x=100.0, y=300.0, d=0, ur=0.0), dict(x=101.0, y=301.0, d=10, ur=-1.0),
             dict(x=200.0, y=300.0, d=0, ur=150.0), dict(x=201.0, y=301.0, d=10, ur=-1.0)]
    feats += [dict(x=300.0, y=300.0, d=0, ur=150.0), dict(x=301.0, y=301.0, d=10, ur=-1.0)]
    qs = [dict(u=100.0, v=300.0, r=5.0, ur=80.0, er=4.0), dict(u=200.0, v=300.0, r=5.0, ur=154.0, er=4.0),
          dict(u=300.0, v=300.0, r=5.0, ur=155.0, er=4.0)]
    out += _kinds("LT", "uright_gt0", desc, _frame(desc, feats, grid), _queries(desc, qs), "uright_gt0")
    out += _kinds("LT", "er_gt_max", desc, _frame(desc, feats, grid), _queries(desc, qs), "er_gt_max")
    for f in feats:
        f["inf"] = 0.5
    qs = [dict(u=100.0, v=300.0, r=5.0, ur=3.0), dict(u=200.0, v=300.0, r=5.0, ur=151.0), dict(u=300.0, v=300.0, r=5.0, ur=190.0)]
    feats[0]["x"] = 103.0  # 2-dof: 9 * 0.5 = 4.5 passes; 3-dof with er = 3: (9 + 9) * 0.5 = 9 > 7.8 fails - which gate applies decides
    out += _kinds("U", "uright_ge0", desc, _frame(desc, feats, grid), _queries(desc, qs), "uright_ge0")
    return out


# ---- item 4: exact edges of the decision rules ----
def decision_edges(desc="b32", grid="default"):
    out = []
    slot = lambda j: (80.0 + 50 * (j % 10), 80.0 + 50 * (j // 10))
    # best == th_high is accepted
    feats, qs = [], []
    for j, d in enumerate([75, 74]):
        u, v = slot(j)
        feats.append(dict(x=u, y=v, d=d)); qs.append(dict(u=u, v=v, r=5.0))
    out += _kinds("LTUI", "best_le_th", desc, _frame(desc, feats, grid), _queries(desc, qs), "best_le_th")
    # best == nnratio * best2: local map accepts (only > rejects), initialization rejects (strict <).  nnratio = 0.5, distances 8 / 16
    feats, qs = [], []
    for j, (d1, d2) in enumerate([(8, 16), (8, 15), (8, 17)]):
        u, v = slot(j)
        feats += [dict(x=u, y=v, d=d1, v=1), dict(x=u + 1, y=v, d=d2, v=2)]
        qs.append(dict(u=u, v=v, r=5.0))
    F, Q = _frame(desc, feats, grid), _queries(desc, qs)
    out += _kinds("L", "ratio_gt", desc, F, Q, "ratio_gt", nnratio=0.5)
    out += _kinds("I", "init_ratio_lt", desc, F, Q, "init_ratio_lt", nnratio=0.5)
    # best_size / best_size2 exactly at size_tol / inv_size_tol: the band is open, so the ratio test is skipped and the match stands
    tol = f32(1.2)
    inv = f32(1.0) / tol
    for rule, lim in (("size_ratio_lt_tol", tol), ("size_ratio_gt_inv", inv)):
        feats, qs = [], []
        s2 = f32(1.0)
        s1 = solve(lambda s: s / s2, lim, float(lim))
        assert s1 is not None
        for j, sz in enumerate([s1, (_below(s1) if rule == "size_ratio_lt_tol" else _above(s1))]):
            u, v = slot(j)
            feats += [dict(x=u, y=v, d=10, v=1, size=sz), dict(x=u + 1, y=v, d=11, v=2, size=s2)]  # 10 > 0.8 * 11: rejected if tested
            qs.append(dict(u=u, v=v, r=5.0, min=0.5, max=2.0))
        out += _kinds("L", rule, desc, _frame(desc, feats, grid), _queries(desc, qs), rule)
    # equal distances: inside one cell the lower index wins; across cells the first in ix-outer / iy-inner order wins, which is NOT index order
    feats, qs = [], []
    u, v = 105.0, 105.0
    feats += [dict(x=u + 1, y=v, d=6, v=1), dict(x=u + 2, y=v, d=6, v=2)]; qs.append(dict(u=u, v=v, r=4.0))
    u, v = 205.0, 205.0   # index order: (ix + 1, iy), (ix, iy + 1), (ix, iy): the reference visits the last one first
    feats += [dict(x=u + 10, y=v, d=6, v=3), dict(x=u, y=v + 10, d=6, v=4), dict(x=u, y=v, d=6, v=5)]; qs.append(dict(u=u + 3, v=v + 3, r=12.0))
    out += _kinds("LTUI", "tie_first", desc, _frame(desc, feats, grid), _queries(desc, qs), "tie_first", nnratio=2.0)
    # d == best2: the second-best stays the FIRST of the equal ones, and with it best_size2 (in the band: the ratio test rejects; flipped, the
    # later one's size is outside the band and the match would stand)
    feats, qs = [], []
    u, v = slot(0)
    feats += [dict(x=u, y=v, d=10, v=1, size=1.0), dict(x=u + 1, y=v, d=11, v=2, size=1.0), dict(x=u + 2, y=v, d=11, v=3, size=1.9)]
    qs.append(dict(u=u, v=v, r=5.0, min=0.5, max=2.0))
    out += _kinds("L", "d_lt_best2", desc, _frame(desc, feats, grid), _queries(desc, qs), "d_lt_best2")
    # initialization: mdist[idx] <= d at equality - the second query at the same distance does not steal
    feats, qs = [], []
    u, v = slot(0)
    feats.append(dict(x=u, y=v, d=7))
    qs += [dict(u=u, v=v, r=5.0, d=0), dict(u=u, v=v, r=5.0, d=0), dict(u=u, v=v, r=5.0, d=2, dv=3)]  # distances 7, 7, 9
    out += _kinds("I", "mdist_le", desc, _frame(desc, feats, grid), _queries(desc, qs), "mdist_le", nnratio=1.0)
    return out


# ---- item 5: ordered-phase stress by construction ----
def chain(desc="b32", nrow=300, rows_=3, grid="default", every_nonocc=0):
    """query i sees features i - 1 and i, both at distance 1: the first visited (i - 1) would win the tie, but query i - 1 holds it (occupied
    in the projection searches; held at a distance <= 1 in SearchForInitialization), because query i - 2 holds ITS first choice ... down to
    query 0, which is feature 0 itself: a dependency chain of nrow - 1 per row - without query 0 every query would end one feature to the
    left.  every_nonocc > 0: every k-th query does not occupy (the next one lands on the same feature and the chain restarts)"""
    feats, qs = [], []
    base = base_row(desc)
    D, QD = [], []
    for rr in range(rows_):
        for i in range(nrow):
            x, y = 20.0 + 2 * i, 40.0 + 100 * rr
            feats.append(dict(x=x, y=y, d=0))
            f = base.copy()
            if desc[0] == "b":
                bit = i % (8 * len(base))
                f[bit >> 3] ^= np.uint8(1 << (bit & 7))
            else:
                f[i % len(base)] += f32(1)
            D.append(f)
            qd = f.copy()
            if i:  # base ^ bit(i - 1) ^ bit(i) / base + e(i - 1) + e(i): distance 1 to both neighbours
                qd = qd ^ (D[-2] ^ base) if desc[0] == "b" else qd + (D[-2] - base)
            QD.append(qd)
            q = dict(u=x - 1.0, v=y, r=1.5)   # the window holds features i - 1 and i only
            if every_nonocc and i % every_nonocc == every_nonocc - 1:
                q["occupies"] = 0
            qs.append(q)
    F, Q = _frame(desc, feats, grid), _queries(desc, qs)
    F.descriptors = np.ascontiguousarray(np.stack(D)); Q.descriptors = np.ascontiguousarray(np.stack(QD))
    tag = "chain%s" % ("-nonocc" if every_nonocc else "")
    return _kinds("LT", tag, desc, F, Q, None, nnratio=1.0) + (_kinds("I", tag, desc, F, Q, None, nnratio=1.0) if not every_nonocc else [])


def behind_keys(desc="b32", nq=120, grid="default", nonocc=False):
    """82 features in one window at distances 0 .. 81 from the base, nq identical queries: query j ends on the feature of rank j (+ 6 in the
    projection searches, where the first 6 features are occupied before the call), far behind the key list of 4 (8); the late queries
    find every candidate within the threshold taken.  nonocc: every third query does not occupy, so the next one lands on the same
    feature."""
    feats = []
    for k in range(82):
        feats.append(dict(x=300.0 + (k % 9) * 2, y=200.0 + (k // 9) * 2, d=k, v=k, occ=int(k < 6)))
    qs = [dict(u=308.0, v=209.0, r=30.0, **({"occupies": int(j % 3 != 1)} if nonocc else {})) for j in range(nq)]
    F, Q = _frame(desc, feats, grid), _queries(desc, qs)
    tag = "behind%s" % ("-nonocc" if nonocc else "")
    return _kinds("LT", tag, desc, F, Q, None, nnratio=1.0) + (_kinds("I", tag, desc, F, Q, None, nnratio=1.0) if not nonocc else [])


def steals(desc="b32", grid="default"):
    """initialization: 40 first-comers take 40 features at distances 1 .. 40; then 30 late queries that ARE features 10 .. 39 (distance 0)
    rob them.  The robbed queries' histogram entries stay (bin 3: 30 of 40 entries), and decide the three maxima."""
    feats = [dict(x=100.0 + 12 * (k % 20), y=100.0 + 12 * (k // 20), d=k + 1, v=k, angle=0.0) for k in range(40)]
    qs = [dict(u=f["x"], v=f["y"], r=3.0, angle=90.0 if k >= 10 else 30.0) for k, f in enumerate(feats)]
    for k in range(10, 40):
        qs.append(dict(u=feats[k]["x"], v=feats[k]["y"], r=3.0, d=k + 1, dv=k, angle=150.0 + 30.0 * (k % 3)))
    return _kinds("I", "steals", desc, _frame(desc, feats, grid), _queries(desc, qs), "steal_hist_stays", nnratio=1.0, check_orientation=True)


# ---- item 6: rotation histogram edges ----
def _rot_scene(desc, pairs, grid="default"):
    """pairs: (query angle, feature angle, copies): isolated query / feature pairs at distance 0"""
    feats, qs = [], []
    j = 0
    for qa, fa, copies in pairs:
        for _ in range(copies):
            u, v = 15.0 + 12 * (j % 50), 15.0 + 12 * (j // 50)
            feats.append(dict(x=u, y=v, d=0, angle=fa)); qs.append(dict(u=u, v=v, r=3.0, angle=qa))
            j += 1
    return _frame(desc, feats, grid), _queries(desc, qs)


def rotation_edges(desc="b32", grid="default"):
    out = []

    def both(name, rule, pairs):
        F, Q = _rot_scene(desc, pairs, grid)
        return (_kinds("T", name, desc, F, Q, rule, check_orientation=True) +
                _kinds("I", name, desc, F, Q, rule, check_orientation=True, nnratio=0.9))
    filler = [(0.0, 0.0, 40), (30.0, 0.0, 30), (60.0, 0.0, 20)]  # bins 0, 1, 2 are the maxima; whatever else is dropped
    # rot * (1 / 30) exactly k + 0.5 goes to bin k + 1: 45 degrees -> 1.5 -> 2 (kept); towards zero it would be bin 1 ... use a dropped bin:
    half = [a for a in (105.0, 135.0, 165.0, 195.0) if abs(float(f32(a) * (f32(1.0) / f32(30.0)))) % 1.0 == 0.5]
    assert half
    a = half[0]
    k = int(float(f32(a) * (f32(1.0) / f32(30.0))))  # lands in bin k + 1; bin k is made a maximum, bin k + 1 is not
    out += both("rot_round", "rot_round", [(0.0, 0.0, 40), (30.0, 0.0, 30), (30.0 * k, 0.0, 20), (a, 0.0, 3)])
    # rot that rounds to bin 30 wraps to bin 0 (a maximum); without the wrap the matches would sit in a dropped bin
    out += both("rot_wrap", "rot_wrap", filler + [(900.0, 0.0, 3), (1000.0, 110.0, 2)])
    # a1 - a2 == 0 exactly stays at 0 (bin 0, kept); just below zero wraps to 360 -> bin 12 (dropped)
    out += both("rot_lt0", "rot_lt0", [(30.0, 0.0, 40), (60.0, 0.0, 30), (90.0, 0.0, 20), (77.0, 77.0, 5), (_below(77.0), 77.0, 4), (200.0, 200.0, 3)]
                + [(0.0, 0.0, 12)])
    # equal counts among the maxima: the first index wins the better rank, the fourth equal bin is dropped
    out += both("max_first", "max_first", [(0.0, 0.0, 9), (30.0, 0.0, 9), (60.0, 0.0, 9), (90.0, 0.0, 9), (120.0, 0.0, 2)])
    # max2 / max3 exactly at 0.1f * (float)max1
    for m1, m in ((100, 10), (30, 3), (70, 7)):
        out += both("max2_lt-%d" % m1, "max2_lt", [(0.0, 0.0, m1), (30.0, 0.0, m), (60.0, 0.0, max(m - 1, 1))])
        out += both("max3_lt-%d" % m1, "max3_lt", [(0.0, 0.0, m1), (30.0, 0.0, m + 5), (60.0, 0.0, m), (90.0, 0.0, 1)])
    return out


def constructed(desc="b32", grid="default"):
    """every scene of items 3-6 for one descriptor kind and grid"""
    out = geometric_edges(desc, grid) + decision_edges(desc, grid) + rotation_edges(desc, grid) + steals(desc, grid)
    out += chain(desc, grid=grid) + chain(desc, 120, 2, grid, every_nonocc=7) + behind_keys(desc, grid=grid) + behind_keys(desc, grid=grid, nonocc=True)
    return out


def all_constructed():
    """32-byte rows on the default, the undistorted and a coarse grid; the scenes whose rule involves distances also with 61-byte and
    float rows (dim 8 and 64)"""
    out = constructed("b32", "default") + [c._replace(name=c.name + "-undist") for c in constructed("b32", "undist")]
    out += [c._replace(name=c.name + "-coarse") for c in decision_edges("b32", "coarse") + behind_keys("b32", grid="coarse")]
    for desc in ("b61", "f8", "f64"):
        out += decision_edges(desc) + steals(desc) + chain(desc, 280, 1) + behind_keys(desc) + rotation_edges(desc)[:2]
    return out


# ---- the random scenes of tests/test_gpu_projection.py::_scene, from the oracle's extractor ----
def random_scene(oracle, seed, shift, radius_scale):
    img = S.corners_frame(seed)
    k1, d1 = oracle.orb_extract(img)
    k2, d2 = oracle.orb_extract(np.roll(img, shift, axis=1))
    size1 = oracle.size_sigma(k1)[0]; size2 = oracle.size_sigma(k2)[0]
    occ = (S.lcg_bytes(seed + 9, len(k1)) < 30).astype(np.uint8)
    F = afv.FrameGridView(d1, np.stack([k1["x"], k1["y"]], 1), size1, angles=k1["angle"], occupied=occ)
    order = np.argsort(S.lcg_states(seed + 5, len(k2)), kind="stable")
    k2, d2, size2 = k2[order], d2[order], size2[order]
    u = k2["x"] - np.float32(shift) + ((S.lcg_states(seed + 6, len(k2)) % 5).astype(np.float32) - 2)
    v = k2["y"] + ((S.lcg_states(seed + 7, len(k2)) % 5).astype(np.float32) - 2)
    valid = (S.lcg_bytes(seed + 8, len(k2)) > 20).astype(np.uint8)
    occupies = (S.lcg_bytes(seed + 10, len(k2)) > 10).astype(np.uint8)
    Q = afv.ProjectionQueries(d2, u, v, np.float32(radius_scale) * size2, size2 / np.float32(1.2), size2 * np.float32(1.2), valid=valid,
                              angles=k2["angle"], occupies=occupies)
    return F, Q


# ---- item 2: size regimes ----
def synthetic(n, nq, seed, desc="b32", grid="default", r=8.0, cluster=None, nonocc=False, protos=16, **gridkw):
    """n features spread over the image (or, cluster=(x, y, w, h), inside that box), nq queries aimed at features, descriptors a few bits
    from a small set of prototypes so that neighbours compete"""
    G = dict(GRIDS[grid]); G.update(gridkw)
    w, h = G["max_x"] - G["min_x"], G["max_y"] - G["min_y"]
    bx, by, bw, bh = cluster if cluster else (G["min_x"] + 2, G["min_y"] + 2, w - 4, h - 4)
    x = (bx + (S.lcg_states(seed, n) % 4096).astype(np.float32) * np.float32(bw / 4096.0)).astype(np.float32)
    y = (by + (S.lcg_states(seed + 1, n) % 4096).astype(np.float32) * np.float32(bh / 4096.0)).astype(np.float32)
    nb = int(desc[1:])
    proto = S.random_descriptors(seed + 2, 16, nb)
    rb = lambda sd, m: S.lcg_bytes(sd, max(m, 1) * nb).reshape(max(m, 1), nb)[:m]
    D = proto[S.lcg_states(seed + 3, n) % protos] ^ (rb(seed + 4, n) & rb(seed + 5, n) & rb(seed + 18, n))   # each bit of the prototype flipped w.p. 1 / 8
    if protos == 1:  # one prototype, bits flipped w.p. 1 / 16: every neighbour is within the threshold, queries compete for all of them
        D = D ^ (rb(seed + 4, n) & rb(seed + 5, n) & rb(seed + 18, n) & ~rb(seed + 21, n))
    sizes = np.float32(1.2) ** (S.lcg_states(seed + 6, n) % 3).astype(np.float32)
    ang = (S.lcg_states(seed + 7, n) % 360).astype(np.float32)
    F = afv.FrameGridView(D, np.stack([x, y], 1), sizes, angles=ang, occupied=(S.lcg_bytes(seed + 8, n) < 20).astype(np.uint8), **G)
    t = S.lcg_states(seed + 9, nq) % max(n, 1)
    QD = (D[t] if n else proto[t % 16]) ^ (rb(seed + 10, nq) & rb(seed + 11, nq) & rb(seed + 12, nq) & rb(seed + 19, nq) & rb(seed + 20, nq))
    qu = (x[t] if n else np.zeros(nq, np.float32)) + ((S.lcg_states(seed + 13, nq) % 7).astype(np.float32) - 3)
    qv = (y[t] if n else np.zeros(nq, np.float32)) + ((S.lcg_states(seed + 14, nq) % 7).astype(np.float32) - 3)
    qs = sizes[t] if n else np.ones(nq, np.float32)
    Q = afv.ProjectionQueries(QD, qu, qv, np.full(nq, r, np.float32), qs / np.float32(1.2), qs * np.float32(1.2),
                              valid=(S.lcg_bytes(seed + 15, nq) > 12).astype(np.uint8), angles=(ang[t] if n else np.zeros(nq, np.float32)) +
                              (S.lcg_states(seed + 16, nq) % 3).astype(np.float32),
                              occupies=(S.lcg_bytes(seed + 17, nq) > (90 if nonocc else 8)).astype(np.uint8))
    return F, Q


def size_regimes():
    """name -> (F, Q): see tests/test_proj_ref_cpu.py for which side of which limit each lies on"""
    out = collections.OrderedDict()
    for nq in (1, 1500, 9000, 65535):
        out["n8192-nq%d" % nq] = synthetic(8192, nq, 100 + nq % 97, r=6.0)
    out["n3000-cluster-64x48"] = synthetic(3000, 8, 211, r=40.0, cluster=(250.0, 180.0, 60.0, 60.0))
    out["n3000-cluster-coarse"] = synthetic(3000, 8, 223, grid="coarse", r=40.0, cluster=(250.0, 180.0, 120.0, 120.0))
    # one chunk of cells holding exactly PW_LIST = 256 entries (the dense list is full) and one holding 257 (the first that falls back)
    out["chunk-256"] = synthetic(256, 8, 227, grid="coarse", r=30.0, cluster=(250.0, 180.0, 40.0, 40.0))
    out["chunk-257"] = synthetic(257, 8, 229, grid="coarse", r=30.0, cluster=(250.0, 180.0, 40.0, 40.0))
    out["live2500-rescans"] = synthetic(2200, 2500, 233, r=14.0, cluster=(100.0, 100.0, 400.0, 300.0), protos=1)
    out["grid-8192-cells"] = synthetic(2000, 1500, 241, r=9.0, grid_cols=128, grid_rows=64)
    out["grid-1x1"] = synthetic(150, 300, 251, r=30.0, grid_cols=1, grid_rows=1)
    return out


# ---- one scene for every route into the projection searches (tests/test_gpu_proj_scenes.py::test_one_scene_through_every_projection_route) ----
INIT_MAX_SIZE = 3.5831808   # 1.2^7: the size band 0 .. F1.maxKeyPtSize a SearchForInitialization between resident frames applies


def every_route_scene(desc="b32"):
    """70 features on the default grid, clustered in a 50 x 40 box around one descriptor prototype so that neighbours are contested, and 65
    queries (a wavefront and one lane) with holes in qvalid, angles, non-occupying queries and an occupancy mask on a few features.
    desc "f64": the same scene with rows of 64 floats - twice the first 64 bits of the binary rows, so that every L2^2 is four times a
    Hamming distance, exact in any summation order.  Returns a dict:
      F, Q      the scene (F.occupied set; F.u_right None)
      Fs, Qs    its stereo twin: mvuRight on two features in three, the queries' ur / er_max placed so that some candidates fail the gate
      Qi        the queries as a SearchForInitialization between resident frames states them: one window, band 0 .. 1.2^7, no mask
      F1, Q2    the reverse direction of a SearchBySim3 pair: the queries as 65 features, the features as 70 queries"""
    F, Q = synthetic(70, 65, 977, r=14.0, cluster=(280.0, 200.0, 50.0, 40.0), protos=1)
    Q.valid[:] = 1
    Q.valid[[3, 17, 40, 63]] = 0          # (query 64, the one-lane tail, searches)
    F.occupied[:] = 0
    F.occupied[[5, 22, 41, 58]] = 1
    if desc == "f64":
        fl = lambda D: np.ascontiguousarray(np.unpackbits(D[:, :8], axis=1).astype(np.float32) * f32(2))
        F.descriptors, Q.descriptors = fl(F.descriptors), fl(Q.descriptors)
    else:
        assert desc == "b32"
    G = GRIDS["default"]
    pts = np.stack([F.x, F.y], 1)
    ur = np.where(np.arange(F.N) % 3 == 2, f32(-1), F.x - f32(20)).astype(np.float32)
    Fs = afv.FrameGridView(F.descriptors, pts, F.sizes, angles=F.angles, occupied=F.occupied, u_right=ur, **G)
    qur = (Q.u - f32(20) + (S.lcg_states(991, Q.n) % 13).astype(np.float32) - f32(6)).astype(np.float32)
    Qs = afv.ProjectionQueries(Q.descriptors, Q.u, Q.v, Q.r, Q.min_size, Q.max_size, valid=Q.valid, angles=Q.angles, occupies=Q.occupies,
                               ur=qur, er_max=np.full(Q.n, 4.0, np.float32))
    Qi = afv.ProjectionQueries(Q.descriptors, Q.u, Q.v, Q.r, np.zeros(Q.n, np.float32), np.full(Q.n, INIT_MAX_SIZE, np.float32), angles=Q.angles)
    F1 = afv.FrameGridView(Q.descriptors, np.stack([Q.u, Q.v], 1), (Q.min_size * f32(1.2)).astype(np.float32), angles=Q.angles, **G)
    Q2 = afv.ProjectionQueries(F.descriptors, F.x, F.y, np.full(F.N, 14.0, np.float32), F.sizes / f32(1.3), F.sizes * f32(1.3), angles=F.angles)
    return dict(F=F, Q=Q, Fs=Fs, Qs=Qs, Qi=Qi, F1=F1, Q2=Q2)
