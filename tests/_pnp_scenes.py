"""Constructed scenes for PnPsolver (tests/_pnp_ref.py; afv_frame_pnp_hypotheses).  TEST INFRASTRUCTURE ONLY.

A scene is a camera with a pose, 3-D points of a map-point store, a frame whose features are the exact projections of some of them rounded
to float32, planted outliers (features displaced by tens of pixels), and one row of point ids per candidate.  Each constructed scene is
named for the rule it reaches; tests/test_pnp_ref_cpu.py proves that it does."""
import numpy as np

import _pnp_ref as R

W, H = 640, 480
CAM = (520.0, 515.0, 318.5, 242.25)
f32 = np.float32


def rot(w):
    """Rodrigues in float64"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


class Scene:
    def __init__(self, name, x, y, octave, store_pos, store_flags, rows, Rcw, tcw, seed=1, min_inliers=10, epsilon=0.5, th2=5.991, nhyp=35,
                 cam=CAM):
        self.name, self.cam = name, tuple(float(f32(v)) for v in cam)
        self.x, self.y, self.octave = np.asarray(x, f32), np.asarray(y, f32), np.asarray(octave, np.int32)
        self.N = len(self.x)
        self.store_pos, self.store_flags = np.asarray(store_pos, f32).reshape(-1, 3), np.asarray(store_flags, np.uint8)
        self.rows = np.asarray(rows, np.int32).reshape(-1, self.N)
        self.nc = self.rows.shape[0]
        self.Rcw, self.tcw = np.asarray(Rcw, np.float64), np.asarray(tcw, np.float64)
        self.seed, self.min_inliers, self.epsilon, self.th2, self.nhyp = seed, min_inliers, epsilon, th2, nhyp

    def sigma2_host(self):
        """sigma2 of the octaves at scale factor 1.2 (the CPU tests; the GPU tests read the plane from the device)"""
        s = f32(1.0)
        table = []
        for _ in range(16):
            table.append(s * s)
            s = s * f32(1.2)
        return np.asarray(table, f32)[self.octave]

    def problem(self, c=0, sigma2=None):
        sigma2 = self.sigma2_host() if sigma2 is None else sigma2
        return R.gather(self.x, self.y, sigma2, self.store_pos, self.store_flags, self.rows[c], self.min_inliers, self.epsilon, self.th2)

    def run(self, c=0, sigma2=None, nhyp=None, mask_words=None, trace=None):
        P = self.problem(c, sigma2)
        mask_words = (self.N + 31) // 32 if mask_words is None else mask_words
        return R.device_outputs(P, R.camera(*self.cam), self.seed + c, self.nhyp if nhyp is None else nhyp, mask_words, cap=self.N, trace=trace)

    def solver(self, c=0, sigma2=None):
        s = R.Solver(self.problem(c, sigma2), R.camera(*self.cam), self.seed + c, self.N)
        s.SetRansacParameters(0.99, self.min_inliers, min(300, self.nhyp), 4, self.epsilon, self.th2)
        return s


def build(name, n, n_match, n_out, rs_seed, nc=1, planar=False, bad=0, unset=0, octaves=False, false_rows=(), depth=(4.0, 8.0),
          identical=False, noise=0.0, **kw):
    """n features of which n_match carry a point id (n_out of those displaced: outliers), `bad` more name a bad point and `unset` more a
    point that was never set; noise: sigma of Gaussian pixel noise on every feature; false_rows: candidates whose ids are shuffled among
    the matched features (every match false); planar: every point at depth 6 in the camera; identical: every point the same"""
    rs = np.random.RandomState(rs_seed)
    fx, fy, cx, cy = (float(f32(v)) for v in CAM)
    Rcw = rot(rs.normal(0, 0.2, 3))
    tcw = rs.normal(0, 0.3, 3)
    u = rs.uniform(20, W - 20, n)
    v = rs.uniform(20, H - 20, n)
    z = np.full(n, 6.0) if planar else rs.uniform(depth[0], depth[1], n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    Xw = ((Xc - tcw) @ Rcw).astype(f32)          # Rcw^T (Xc - tcw)
    if identical:
        Xw[:] = Xw[0]
    Xc = Xw.astype(np.float64) @ Rcw.T + tcw
    x = (fx * Xc[:, 0] / Xc[:, 2] + cx).astype(f32)
    y = (fy * Xc[:, 1] / Xc[:, 2] + cy).astype(f32)
    if noise:
        x = (x + rs.normal(0, noise, n)).astype(f32)
        y = (y + rs.normal(0, noise, n)).astype(f32)
    feats = rs.permutation(n)
    matched, badf, unsetf = feats[:n_match], feats[n_match:n_match + bad], feats[n_match + bad:n_match + bad + unset]
    for i in matched[:n_out]:
        x[i] = f32(np.clip(x[i] + rs.choice([-1, 1]) * rs.uniform(30, 90), 1, W - 2))
        y[i] = f32(np.clip(y[i] + rs.choice([-1, 1]) * rs.uniform(30, 90), 1, H - 2))
    P = n + 5
    ids = rs.permutation(P)
    pos = rs.normal(0, 50, (P, 3)).astype(f32)
    flags = np.full(P, R.SET, np.uint8)
    row = np.full(n, -1, np.int32)
    for i in list(matched) + list(badf) + list(unsetf):
        row[i] = ids[i]
        pos[ids[i]] = Xw[i]
    for i in badf:
        flags[ids[i]] = R.SET | R.BAD
    for i in unsetf:
        flags[ids[i]] = 0
    rows = np.tile(row, (nc, 1))
    for c in range(nc):
        if c in false_rows:
            rows[c, matched] = row[matched][rs.permutation(n_match)]
        elif c > 0:
            rows[c, matched[rs.rand(n_match) < 0.15]] = -1
    octave = rs.randint(0, 8, n) if octaves else np.zeros(n, np.int32)
    return Scene(name, x, y, octave, pos, flags, rows, Rcw, tcw, **kw)


def clean(n, rs_seed, **kw):
    """noise-free, every feature matched, no outliers, well spread, not coplanar"""
    return build("clean_%d_%d" % (n, rs_seed), n, n, 0, rs_seed, **kw)


def rules_of(trace):
    """the rules the EPnP runs of a trace reached (tests/_pnp_ref.py, epnp's info)"""
    out = set()
    for _, _, info in trace:
        if "winner" not in info:
            continue
        out.add("winner%d" % info["winner"])
        out.add("flip" if any(info["flips"]) else "noflip")
        if not all(info["flips"]):
            out.add("noflip")
        if any(info["detfix"]):
            out.add("detfix")
        out.add("b1_neg%s" % info["b1"])
        for tag in ("b2", "b3"):
            neg, second, flip = info[tag]
            out.update(("%s_neg%s" % (tag, neg), "%s_neg%s_second%s" % (tag, neg, second), "%s_flip%s" % (tag, flip)))
    return out


def constructed():
    """(scene, the rules it is named for).  Rules of rules_of, and of the run: degenerate (E8, R or t not finite), record_refine_fails_then_
    succeeds, ends_on_unrefined_best (Q3), n_below_min_inliers, n_below_four (E9), min_inliers_equals_n, bad_and_unset_ids"""
    mk = lambda name, rs, planar: build(name, 24, 20, 8, rs, planar=planar, min_inliers=8, epsilon=0.4, nhyp=20)
    return [
        (mk("every_approximation_wins", 1, False),
         {"winner1", "winner2", "winner3", "flip", "noflip", "detfix", "b1_negTrue", "b1_negFalse", "b2_negFalse", "b2_negFalse_secondTrue",
          "b2_flipFalse", "b2_flipTrue", "b3_negFalse", "b3_negFalse_secondTrue", "b3_negFalse_secondFalse", "b3_flipFalse", "b3_flipTrue"}),
        (mk("coplanar_negative_b0", 1, True), {"b2_negTrue", "b2_negTrue_secondFalse", "b3_negTrue", "b3_negTrue_secondFalse"}),
        (mk("coplanar_negative_b0_b2", 2, True), {"b3_negTrue_secondTrue"}),
        (build("coplanar_approximation_2_negative_b0_b2", 16, 14, 7, 20, planar=True, min_inliers=8, epsilon=0.4, nhyp=30), {"b2_negTrue_secondTrue"}),
        (mk("coplanar_not_finite", 3, True), {"b2_negFalse_secondFalse", "degenerate"}),
        (build("identical_points", 6, 6, 0, 51, identical=True, min_inliers=4, nhyp=6), {"degenerate"}),
        (build("record_refine_fails_then_succeeds", 30, 26, 8, 2, noise=1.5, min_inliers=8, epsilon=0.3, nhyp=35),
         {"record_refine_fails_then_succeeds"}),
        (build("ends_on_unrefined_best", 30, 26, 8, 1, noise=2.5, min_inliers=8, epsilon=0.3, nhyp=35), {"ends_on_unrefined_best"}),
        (build("n_below_min_inliers", 20, 8, 0, 53, min_inliers=10, nhyp=6), {"n_below_min_inliers"}),
        (build("n_below_four", 20, 3, 0, 54, min_inliers=4, nhyp=6), {"n_below_four"}),
        (build("min_inliers_equals_n", 14, 10, 0, 5, min_inliers=10, epsilon=0.5, nhyp=35), {"min_inliers_equals_n"}),
        (build("bad_and_unset_ids", 30, 20, 5, 9, bad=3, unset=3, octaves=True, min_inliers=8, epsilon=0.4, nhyp=12), {"bad_and_unset_ids"}),
    ]
