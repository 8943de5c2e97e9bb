"""Scenes for Optimizer::PoseOptimization on a resident frame: seeded random frames and constructed ones, each named after the rule of
tests/_poseopt_ref.py it reaches.  `reaches(scene)` is the proof, checked on the CPU (tests/test_poseopt_ref_cpu.py): it runs the
restatement with its log and answers whether the rule was met.  The GPU test holds the device to the restatement on every one of them."""
import numpy as np

import _poseopt_ref as R

W, H = 640.0, 480.0
FX, FY, CX, CY, MBF = 517.3, 516.5, 318.6, 255.3, 40.0
SCALE_FACTOR = np.float32(1.2)


def octave_inf(octave):
    """keyPtsInf of an octave as the CPU tests take it (the GPU tests read the device's own values): 1 / (1.2^octave)^2 in float"""
    s = np.ones(8, np.float32)
    for k in range(1, 8):
        s[k] = s[k - 1] * SCALE_FACTOR
    return (np.float32(1.0) / (s * s))[np.asarray(octave)]


def rot(w):
    """a rotation matrix from a rotation vector, float64 (scene construction only: not part of any semantics)"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


class Scene:
    def __init__(self, name, x, y, u_right, octave, pts, store_pos, store_set, Rcw, tcw, cam=(FX, FY, CX, CY, MBF), planted=None, rule=None):
        self.name, self.rule = name, rule
        self.x, self.y, self.u_right = (np.asarray(a, np.float32) for a in (x, y, u_right))
        self.octave = np.asarray(octave, np.int32)
        self.pts = np.asarray(pts, np.int32)
        self.store_pos = np.asarray(store_pos, np.float32).reshape(-1, 3)
        self.store_set = np.asarray(store_set, bool)
        self.Rcw, self.tcw = np.asarray(Rcw, np.float32).reshape(3, 3), np.asarray(tcw, np.float32).reshape(3)
        self.cam = tuple(float(np.float32(v)) for v in cam)
        self.planted = planted
        self.N = len(self.x)

    def problem(self, inf=None, pts=None, store_pos=None, store_set=None):
        return R.Problem(self.x, self.y, self.u_right, octave_inf(self.octave) if inf is None else inf, self.pts if pts is None else pts,
                         self.store_pos if store_pos is None else store_pos, self.store_set if store_set is None else store_set, *self.cam)

    def run(self, log=None, **kw):
        return R.pose_optimization(self.problem(**kw), self.Rcw, self.tcw, log)


def make(name, seed, n, n_edges=None, stereo="mixed", outliers=0.1, noise=0.0, rot_err=0.02, trans_err=0.05, never_set=0.05, out_px=50.0,
         depth=(2.0, 10.0), rule=None):
    """a frame of n features seen from a true pose; the initial pose is the true one perturbed.  n_edges: how many features have a point
    (default: about 85 %).  stereo: "mono" | "stereo" | "mixed".  outliers: fraction of the edges whose observation is moved by out_px."""
    rs = np.random.RandomState(seed)
    Rt = rot(rs.normal(0, 0.2, 3))
    tt = rs.normal(0, 0.5, 3)
    u, v = rs.uniform(10, W - 10, n), rs.uniform(10, H - 10, n)
    z = rs.uniform(depth[0], depth[1], n)
    pc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
    pw = ((pc - tt) @ Rt).astype(np.float32)                      # Rt^T (pc - tt)
    pc = pw.astype(np.float64) @ Rt.T + tt
    x = FX * pc[:, 0] / pc[:, 2] + CX + rs.normal(0, 1, n) * noise
    y = FY * pc[:, 1] / pc[:, 2] + CY + rs.normal(0, 1, n) * noise
    ur = x - MBF / pc[:, 2] + rs.normal(0, 1, n) * noise
    is_stereo = {"mono": np.zeros(n, bool), "stereo": np.ones(n, bool), "mixed": rs.rand(n) < 0.5}[stereo]
    ur = np.where(is_stereo, ur, -1.0)
    cap = 2 * n + 8
    ids = rs.permutation(cap)[:n]
    has = rs.rand(n) < 0.85
    if n_edges is not None:
        has = np.zeros(n, bool)
        has[rs.permutation(n)[:n_edges]] = True
    pts = np.where(has, ids, -1)
    unset = has & (rs.rand(n) < never_set) if n_edges is None else np.zeros(n, bool)
    store_pos = rs.normal(0, 1, (cap, 3)).astype(np.float32)
    store_set = np.zeros(cap, bool)
    store_pos[ids] = pw
    store_set[ids[has & ~unset]] = True
    edge = has & ~unset
    planted = edge & (rs.rand(n) < outliers)
    ang = rs.uniform(0, 2 * np.pi, n)
    x = np.where(planted, x + out_px * np.cos(ang), x)
    y = np.where(planted, y + out_px * np.sin(ang), y)
    R0 = rot(rs.normal(0, 1, 3) * rot_err) @ Rt
    t0 = tt + rs.normal(0, 1, 3) * trans_err
    return Scene(name, x, y, ur, rs.randint(0, 8, n), pts, store_pos, store_set, R0, t0, planted=planted, rule=rule)


_random_cache = {}


def random_scene(seed, n, stereo="mixed"):
    key = (seed, n, stereo)
    if key not in _random_cache:
        _random_cache[key] = make("random-%d-%d-%s" % (seed, n, stereo), seed, n, stereo=stereo, noise=0.7)
    return _random_cache[key]


def exact_scene(special=None):
    """identity pose, fx = fy = 256, dyadic points: every residual is exactly 0, so b = 0, x = 0, the trial leaves chi2 as it is and
    rho == 0 ends the call.  special(x, y, pos) may edit the arrays (in place) before the scene is built."""
    n = 12
    k = np.arange(n)
    Z = np.full(n, 4.0)
    X, Y = (k % 4 - 1.5) * 0.5, (k // 4 - 1.0) * 0.5
    cam = (256.0, 256.0, 320.0, 240.0, 32.0)
    x, y = 256.0 * X / Z + 320.0, 256.0 * Y / Z + 240.0
    ur = np.where(k % 2 == 0, x - 32.0 / Z, -1.0)
    pos = np.stack([X, Y, Z], 1).astype(np.float32)
    if special:
        special(x, y, pos)
    return Scene("exact", x, y, ur, np.zeros(n, np.int32), k, pos, np.ones(n, bool), np.eye(3), np.zeros(3), cam=cam)


def _z_cases(x, y, pos):
    pos[0, 2] = 0.0     # z == 0 exactly: a chi2 that is not finite (P2), and ten failed trials in round 0 (its H is not finite)
    pos[1, 2] = -4.0    # z < 0: projects like any point (isDepthPositive is not consulted), here far from its observation


# (stereo, side) -> (d, Y): found by bisection against the restatement, see threshold_scene
_THRESHOLD = {(False, "equal"): (3.05328369140625, "-0x1.4a78840000000p-15"), (False, "above"): (3.05328369140625, "-0x1.4a8f060000000p-15"),
              (True, "equal"): (2.947967529296875, "-0x1.07ca8a0000000p-16"), (True, "above"): (2.947967529296875, "-0x1.07e2040000000p-16")}


def threshold_scene(stereo, side):
    """(float)chi2 > 5.991f / 7.815f at the boundary.  Eight of the exact edges and one tuned edge (index 8), so one round.  The tuned
    edge's x observation is its exact projection + d, which leaves its chi2 at the round's final pose about 1e-3 under the threshold; its
    point's Y (about -4e-5: 2e-11 of chi2 per float of Y) then raises it, by bisection against the restatement, to
      "equal": a double ABOVE (double)th that the cast rounds down to th - not flagged, though a comparison in double would flag it;
      "above": the next float after th - flagged."""
    d, Y = _THRESHOLD[(stereo, side)]
    e = exact_scene()
    n, k = 9, 8
    x, y, ur, pos = e.x[:n].copy(), e.y[:n].copy(), e.u_right[:n].copy(), e.store_pos[:n].copy()
    pos[k] = (0.25, np.float32(float.fromhex(Y)), 4.0)
    px = 256.0 * 0.25 / 4.0 + 320.0
    x[k], y[k] = np.float32(px + d), 240.0
    ur[k] = np.float32(px + d - 32.0 / 4.0) if stereo else -1.0
    return Scene("threshold-%s-%s" % ("stereo" if stereo else "mono", side), x, y, ur, np.zeros(n, np.int32), np.arange(n), pos, np.ones(n, bool),
                 np.eye(3), np.zeros(3), cam=e.cam)


def constructed():
    """[(scene, rule)]: rule is what `reaches` checks"""
    out = []
    out.append((make("huber-both-sides", 11, 200, noise=1.0, outliers=0.2, out_px=6.0), "huber_both"))
    out.append((make("taken-back", 1, 120, noise=1.6, outliers=0.3, out_px=4.0, rot_err=0.05), "taken_back"))
    out.append((make("rejected-trial", 5, 80, noise=0.5, rot_err=0.3, trans_err=0.8, outliers=0.3), "rejected"))
    out.append((make("ten-rejections", 88, 30, noise=2.0, outliers=0.3, out_px=5.0), "qmax_real"))
    s = exact_scene()
    s.name = "rho-zero"
    out.append((s, "rho0"))
    s = exact_scene(_z_cases)
    s.name = "z-not-positive"
    out.append((s, "nonfinite"))
    for k in (2, 3, 9, 10):
        out.append((make("edges-%d" % k, 20 + k, 40, n_edges=k, noise=0.5, outliers=0.0), "edges_%d" % k))
    out.append((make("all-flagged", 31, 64, outliers=1.0, noise=0.0), "all_flagged"))
    out.append((make("beyond-pi", 6, 30, n_edges=3, stereo="mono", noise=0.0, outliers=1.0, out_px=300.0, depth=(40.0, 41.0)), "theta"))
    out.append((make("never-set", 41, 100, never_set=0.5, noise=0.5), "never_set"))
    for kind in ("mono", "stereo", "mixed"):
        out.append((make("kind-" + kind, 50, 150, stereo=kind, noise=0.7), "kind_" + kind))
    for stereo in (False, True):
        for side in ("equal", "above"):
            out.append((threshold_scene(stereo, side), "th_" + side))
    return out


def reaches(scene, rule):
    """the proof that `scene` reaches `rule`: runs the restatement (and, where the rule is about dependence, a variant) and returns a bool"""
    log = []
    pr = scene.problem()
    res = R.pose_optimization(pr, scene.Rcw, scene.tcw, log)
    trials = [e for rl in log for e in rl if "trial" in e]
    ends = [e for rl in log for e in rl if "terminate" in e]
    if rule == "huber_both":   # at the initial pose, active edges on both sides of delta^2, of both kinds where the frame has both
        _, chi2 = R.edge_error(pr, scene.Rcw.astype(np.float64), scene.tcw.astype(np.float64))
        inside = pr.edge & (chi2 <= pr.delta * pr.delta)
        outside = pr.edge & (chi2 > pr.delta * pr.delta)
        return all((inside & k).any() and (outside & k).any() for k in (pr.stereo, ~pr.stereo))
    if rule == "taken_back":
        f = res.flags_by_round
        return res.rounds == 4 and bool((f[0] & ~f[2]).any()) and bool((f[0] & ~f[3]).any())
    if rule == "rejected":
        return any(not e["accepted"] and not e["failed"] and e["rho"] < 0 for e in trials) and any(e["accepted"] for e in trials)
    if rule == "qmax_real":    # a call that ends on qmax == 10 through ten solved, evaluated and rejected trials: the whole lambda *= ni, ni *= 2 ladder
        for rl in log:
            t = [e for e in rl if "trial" in e]
            if rl and rl[-1].get("terminate") == "qmax" and len(t) >= 10 and all(not e["failed"] and not e["accepted"] and e["rho"] < 0 for e in t[-10:]):
                lams = [e["lam"] for e in t[-10:]]
                return all(lams[i + 1] == lams[i] * 2.0 ** (i + 1) for i in range(9))
        return False
    if rule == "rho0":
        return any(e["terminate"] == "rho0" for e in ends) and res.n_good == res.n_edges and np.array_equal(res.Rcw, scene.Rcw.reshape(9))
    if rule == "nonfinite":
        _, chi2 = R.edge_error(pr, scene.Rcw.astype(np.float64), scene.tcw.astype(np.float64))
        return (not np.isfinite(chi2[0]) and bool(res.outlier[0]) and bool(res.outlier[1]) and log[0][-1].get("terminate") == "qmax" and
                sum(e["why"] == "pivot" for e in log[0] if "trial" in e) == 10 and res.n_good == res.n_edges - 2)
    if rule.startswith("edges_"):
        k = int(rule[6:])
        return res.n_edges == k and res.rounds == (0 if k < 3 else 1 if k < 10 else 4) and (k >= 3 or res.n_good == 0)
    if rule == "all_flagged":
        return (res.rounds == 4 and bool(res.flags_by_round[0][pr.edge].all()) and int(res.iterations[1]) == 0 and
                np.array_equal(res.Rcw, scene.Rcw.reshape(9)) and np.array_equal(res.tcw, scene.tcw))
    if rule in ("th_equal", "th_above"):
        k = 8
        th = pr.th[k]
        c = res.chi2_edges[k]
        others_in = not res.outlier[:k].any() and res.rounds == 1 and res.n_edges == 9
        if rule == "th_equal":   # above the threshold as a double, equal to it after the cast: `>` in float is false
            return others_in and c > np.float64(th) and np.float32(c) == th and not res.outlier[k] and res.n_good == 9
        return others_in and np.float32(c) == np.nextafter(th, np.float32(np.inf)) and bool(res.outlier[k]) and res.n_good == 8
    if rule == "theta":
        return any(e["why"] == "theta" for e in trials)
    if rule == "never_set":    # the never-set ids are no edges, and setting them would change the answer
        named = scene.pts >= 0
        other = scene.run(store_set=np.ones_like(scene.store_set))
        return res.n_edges < int(named.sum()) == other.n_edges and not np.array_equal(other.Rcw, res.Rcw)
    if rule.startswith("kind_"):
        want = {"mono": (False, True), "stereo": (True, False), "mixed": (True, True)}[rule[5:]]
        return (bool((pr.edge & pr.stereo).any()), bool((pr.edge & ~pr.stereo).any())) == want and res.rounds == 4
    raise KeyError(rule)
