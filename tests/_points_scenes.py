"""Constructed scenes for the resident map points (tests/_points_ref.py; -m gpu: tests/test_gpu_points.py).  TEST INFRASTRUCTURE ONLY.

Each scene is named after the ONE rule that decides it: tests/test_points_ref_cpu.py proves on the CPU that the restatement reaches that
rule on the scene (its trace) and that flipping the rule changes the scene's outcome.  Scenes are small: 3 to 40 points, a feature side of
at most 130 features on a 96 x 64 frame.  The default camera looks down +z from the origin with fx = fy = 32, cx = 48, cy = 32, so that
u = 32 X / Z + 48 is exact for small integers and a bound, a band end or a cosine can be met exactly.
"""
import numpy as np

import _points_ref as R

f32 = np.float32
W, H = 96.0, 64.0


def up(v, n=1):
    v = f32(v)
    for _ in range(n):
        v = np.nextafter(v, f32(np.inf))
    return v


def down(v, n=1):
    v = f32(v)
    for _ in range(n):
        v = np.nextafter(v, f32(-np.inf))
    return v


def rows_for(n, nbytes, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, nbytes)).astype(np.uint8)


class Features:
    """the feature side of a search scene: what a resident frame is filled with (Frame.set_features)"""

    def __init__(self, x, y, sizes, desc, angles=None, u_right=None):
        self.x, self.y, self.sizes = (np.ascontiguousarray(a, np.float32) for a in (x, y, sizes))
        self.desc = np.ascontiguousarray(desc)
        self.n = len(self.x)
        self.angles = np.zeros(self.n, np.float32) if angles is None else np.ascontiguousarray(angles, np.float32)
        self.u_right = None if u_right is None else np.ascontiguousarray(u_right, np.float32)


class Scene:
    def __init__(self, name, rule, flavour, P, cam, ids, reached, radius_th=1.0, radius_scale=R.RADIUS_SCALE, cos_limit=0.5, last_sizes=None,
                 last_angles=None, feat=None, th=64.0, nnratio=0.9, check_orientation=False, occupied=None, inf_gate=False):
        self.name, self.rule, self.flavour, self.P, self.cam = name, rule, flavour, P, cam
        self.ids = np.asarray(ids, np.int32)
        self.reached = reached  # trace -> bool: the scene reaches its rule
        self.radius_th, self.radius_scale, self.cos_limit = f32(radius_th), f32(radius_scale), f32(cos_limit)
        self.last_sizes = None if last_sizes is None else np.ascontiguousarray(last_sizes, np.float32)
        self.last_angles = None if last_angles is None else np.ascontiguousarray(last_angles, np.float32)
        self.feat, self.th, self.nnratio, self.check_orientation, self.occupied = feat, th, nnratio, check_orientation, occupied
        self.inf_gate = inf_gate  # FUSE: the chi-square gate on the reprojection error (Fuse(pKF, vpMapPoints)) applies

    def kw(self):
        return dict(radius_th=self.radius_th, radius_scale=self.radius_scale, cos_limit=self.cos_limit, last_sizes=self.last_sizes)

    def project(self, flip=None):
        return R.project(self.P, self.cam, self.ids, self.flavour, flip=flip, **self.kw())

    def queries(self, flip=None):
        return R.queries(self.P, self.cam, self.ids, self.flavour, angles=self.last_angles, flip=flip, **self.kw())


def outcome(o):
    """what a flipped rule must change: the answer per query, bit for bit, and which rules rejected how many queries"""
    keys = ("in_view", "occ", "u", "v", "ur", "size", "sigma", "view_cos", "r", "qmin", "qmax", "er")
    return b"".join(np.ascontiguousarray(o[k]).tobytes() for k in keys) + repr(sorted(o["trace"]["rej"].items())).encode()


def store(points, cap=64, desc_seed=1, desc_bytes=32):
    """points: list of dicts (pos, normal, min, max, ref_size, ref_dist, ref_sigma; bad / observed / unset optional) -> Points, ids 0 .."""
    P = R.Points(cap, desc_bytes)
    n = len(points)
    g = lambda k, d: np.array([p.get(k, d) for p in points], np.float32)
    ids = np.arange(n)
    P.set(ids, pos=g("pos", (0, 0, 4)), normal=g("normal", (0, 0, 1)), min_distance=g("min", 0.5), max_distance=g("max", 100.0),
          ref_size=g("ref_size", 1.0), ref_distance=g("ref_dist", 4.0), ref_sigma=g("ref_sigma", 0.5))
    P.set_flags(ids, bad=[p.get("bad", 0) for p in points], observed=[p.get("observed", 1) for p in points])
    P.set_descriptors(ids, rows_for(n, desc_bytes, desc_seed))
    for i, p in enumerate(points):
        if p.get("unset"):
            P.flags[i] &= ~np.uint8(R.SET)
    return P


def _eq(rule):
    return lambda tr: tr["eq"].get(rule, 0) > 0


def _first_x_beyond(cam, flavour, z, x0, bound, step):
    """the float next to x0 (stepping by `step` = +-1 ulp) at which u leaves `bound`; the scene asserts what it gets"""
    x = f32(x0)
    for _ in range(64):
        x = up(x) if step > 0 else down(x)
        P = store([{"pos": (x, 0, z)}])
        o = R.project(P, cam, [0], flavour, last_sizes=[1.0])
        if not o["in_view"][0]:
            return x
    raise AssertionError("no float beyond the bound within 64 ulps")


def bound_scenes():
    out = []
    cam = R.Camera()
    for fname in ("frustum", "lastframe", "reloc"):
        fl = R.FLAVOURS[fname]
        last = np.ones(8, np.float32) if fl == R.LASTFRAME else None
        # u == max, v == max: inside (inclusive); one float beyond: outside
        xb = _first_x_beyond(cam, fl, 2, 3, W, +1)
        pts = [{"pos": (3, 0, 2)}, {"pos": (0, 2, 2)}, {"pos": (xb, 0, 2)}, {"pos": (0, 0, 4)}]
        out.append(Scene("bound_max_" + fname, "bound_max", fl, store(pts), cam, range(4), _eq("bound_max"), last_sizes=last))
        xb = _first_x_beyond(cam, fl, 2, -3, 0.0, -1)
        pts = [{"pos": (-3, 0, 2)}, {"pos": (0, -2, 2)}, {"pos": (xb, 0, 2)}, {"pos": (0, 0, 4)}]
        out.append(Scene("bound_min_" + fname, "bound_min", fl, store(pts), cam, range(4), _eq("bound_min"), last_sizes=last))
    # KeyFrame::IsInImage is half-open: u == max is outside, u == min inside
    xi = f32(3)
    while not R.project(store([{"pos": (xi, 0, 2)}]), cam, [0], R.FUSE)["in_view"][0]:   # the first float below 3 whose u lies below max
        xi = down(xi)
    pts = [{"pos": (3, 0, 2)}, {"pos": (0, 2, 2)}, {"pos": (xi, 0, 2)}, {"pos": (0, 0, 4)}, {"pos": (up(xi), 0, 2)}]
    out.append(Scene("fuse_bound_max", "fuse_bound_max", R.FUSE, store(pts), cam, range(5), _eq("fuse_bound_max")))
    pts = [{"pos": (-3, 0, 2)}, {"pos": (0, -2, 2)}, {"pos": (down(-3), 0, 2)}, {"pos": (0, 0, 4)}]
    out.append(Scene("fuse_bound_min", "fuse_bound_min", R.FUSE, store(pts), cam, range(4), _eq("fuse_bound_min")))
    return out


def band_scenes():
    out = []
    cam = R.Camera()
    z7 = f32(0.8) * f32(7.0)   # 0.8f * 7 rounds DOWN to 5.5999999: the double product 0.8 * 7 lies above it
    for fname in ("frustum", "reloc", "fuse"):
        fl = R.FLAVOURS[fname]
        # dist == 0.8f * min: inside; min one float up: outside
        pts = [{"pos": (0, 0, 4), "min": 5.0}, {"pos": (0, 0, 4), "min": up(5.0)}, {"pos": (0, 0, 4), "min": down(5.0)}]
        out.append(Scene("band_lo_" + fname, "band_lo", fl, store(pts), cam, range(3), _eq("band_lo")))
        # dist == 1.2f * max (1.2f * 2.5 rounds to 3): inside; max one float down: outside
        pts = [{"pos": (0, 0, 3), "max": 2.5}, {"pos": (0, 0, 3), "max": down(2.5)}, {"pos": (0, 0, 3), "max": up(2.5)}]
        out.append(Scene("band_hi_" + fname, "band_hi", fl, store(pts), cam, range(3), _eq("band_hi")))
        pts = [{"pos": (0, 0, z7), "min": 7.0}, {"pos": (0, 0, 4)}, {"pos": (0, 0, down(z7)), "min": 7.0}]
        out.append(Scene("band_factor_" + fname, "band_factor", fl, store(pts), cam, range(3), _eq("band_lo")))
    # the last-frame search has no band: a point far outside its band is searched
    pts = [{"pos": (0, 0, 4), "min": 50.0}, {"pos": (1, 1, 4), "max": 1.0}, {"pos": (0, 0, 4)}]
    out.append(Scene("lastframe_no_band", "lastframe_no_band", R.LASTFRAME, store(pts), cam, range(3), lambda tr: not tr["rej"],
                     last_sizes=[1.0, 1.5, 2.0]))
    out.append(Scene("size_last", "size_last", R.LASTFRAME, store(pts), cam, range(3), lambda tr: not tr["rej"], last_sizes=[1.0, 1.5, 2.0]))
    return out


def angle_scenes():
    out = []
    cam = R.Camera()
    # PO = (0, 0, 4), normal (0, 0, n): dot = 4 n, viewCos = n exactly
    pts = [{"normal": (0, 0, 0.5)}, {"normal": (0, 0, down(0.5))}, {"normal": (0, 0, up(0.5))}]
    out.append(Scene("view_cos_lt", "view_cos_lt", R.FRUSTUM, store(pts), cam, range(3), _eq("view_cos_lt")))
    out.append(Scene("view_cos_limit_0.75", "view_cos_lt", R.FRUSTUM, store([{"normal": (0, 0, 0.75)}, {"normal": (0, 0, down(0.75))}, {"normal": (0, 0, up(0.75))}]),
                     cam, range(3), _eq("view_cos_lt"), cos_limit=0.75))
    c = f32(0.998)   # the float 0.998f lies above the double 0.998; the float below it lies below
    pts = [{"normal": (0, 0, c)}, {"normal": (0, 0, down(c))}, {"normal": (0, 0, up(c))}, {"normal": (0, 0, 1)}]
    out.append(Scene("cos998_double", "cos998_double", R.FRUSTUM, store(pts), cam, range(4), _eq("cos998_double"), radius_th=3.0))
    pts = [{"normal": (0, 0, 0.5)}, {"normal": (0, 0, down(0.5))}, {"normal": (0, 0, up(0.5))}]
    out.append(Scene("fuse_dot", "fuse_dot", R.FUSE, store(pts), cam, range(3), _eq("fuse_dot")))
    # the relocalisation search has no viewing-angle test: a point seen from behind its normal is searched
    pts = [{"normal": (0, 0, -1)}, {"normal": (0, 0, 0.25)}, {"normal": (0, 0, 1)}]
    out.append(Scene("reloc_no_cos", "reloc_no_cos", R.RELOC, store(pts), cam, range(3), _eq("reloc_no_cos")))
    # a radius whose two product orders differ in the last bit
    for seed in range(200):
        rs = np.random.RandomState(seed)
        pts = [{"pos": (0, 0, f32(rs.uniform(3, 5))), "ref_size": f32(rs.uniform(1, 2)), "ref_dist": f32(rs.uniform(3, 5))} for _ in range(6)]
        s = Scene("radius_order", "radius_order", R.FRUSTUM, store(pts), cam, range(6), lambda tr: True, radius_th=f32(rs.uniform(1, 4)))
        if outcome(s.project()) != outcome(s.project("radius_order")):
            out.append(s)
            break
    else:
        raise AssertionError("no radius whose product orders differ")
    return out


def depth_scenes():
    out = []
    # pcz = -0.0f needs every term of the sum and tcw(2) at -0: X, Y < 0 under a zero coefficient
    cam_m0 = R.Camera(tcw=(0.0, 0.0, -0.0), Ow=(0, 0, 0))
    cam = R.Camera()
    neg0 = {"pos": (-1.0, -1.0, -0.0)}
    pos0 = {"pos": (1.0, 1.0, 0.0)}
    tiny = {"pos": (0.0, 0.0, -1e-30)}
    good = {"pos": (0, 0, 4)}
    side = {"pos": (1, 0.5, 4)}
    for fname in ("frustum", "lastframe", "reloc", "fuse"):
        fl = R.FLAVOURS[fname]
        last = np.ones(4, np.float32) if fl == R.LASTFRAME else None
        rule = {"frustum": "depth_pcz", "fuse": "depth_pcz", "lastframe": "depth_invz", "reloc": "d1"}[fname]
        out.append(Scene("z_minus_zero_" + fname, rule, fl, store([neg0, good, side]), cam_m0, range(3),
                         (lambda tr: tr["eq"].get("d1", 0) > 0) if fname == "reloc" else _eq(rule), last_sizes=last))
        out.append(Scene("z_plus_zero_" + fname, "d1", fl, store([pos0, good, side]), cam, range(3), _eq("d1"), last_sizes=last))
        rule = {"frustum": "depth_pcz", "fuse": "depth_pcz", "lastframe": "depth_invz", "reloc": "reloc_no_depth"}[fname]
        reached = (lambda tr: tr["rej"].get("depth", 0) > 0) if fname != "reloc" else _eq("reloc_no_depth")
        if fname != "reloc":   # (a tiny negative z is rejected by either form of the depth test: the scene pins the rejection itself)
            out.append(Scene("z_tiny_negative_" + fname, None, fl, store([tiny, good, neg0]), cam, range(3), reached, last_sizes=last))
        else:                  # no depth test: with a band that starts at 0 the point is searched, at u = 48 with an enormous radius
            out.append(Scene("z_tiny_negative_reloc", rule, fl, store([dict(tiny, min=0.0), good, tiny]), cam, range(3), reached))
    # a point behind the camera that the relocalisation search lets through: u = 32 * 1 / -4 + 48 = 40
    pts = [{"pos": (1, 1, -4)}, {"pos": (0, 0, 4)}, {"pos": (0.0, 0.0, -1e-30)}]
    out.append(Scene("reloc_behind_camera", "reloc_no_depth", R.RELOC, store(pts), cam, range(3), _eq("reloc_no_depth")))
    # NaN coordinates and a zero distance: D1
    pts = [{"pos": (np.nan, 0, 4)}, {"pos": (0, 0, 0)}, {"pos": (0, 0, 4)}]
    out.append(Scene("d1_nan_and_zero_dist", "d1", R.RELOC, store(pts), cam, range(3), _eq("d1")))
    return out


def rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def order_scenes():
    """a three-term sum whose two orders differ in the last bit, and a projection whose two forms do"""
    out = []
    cam = R.Camera(Rcw=rotation(0.05, -0.08, 0.03), tcw=(0.1, -0.05, 0.2), mbf=8.0)
    for name, flavour in (("sum_order_frustum", R.FRUSTUM), ("sum_order_fuse", R.FUSE)):
        for seed in range(200):
            rs = np.random.RandomState(seed)
            pts = [{"pos": (f32(rs.uniform(-2, 2)), f32(rs.uniform(-1.5, 1.5)), f32(rs.uniform(3, 6)))} for _ in range(8)]
            for p in pts:
                p["normal"] = tuple(np.asarray(p["pos"], np.float32) / np.linalg.norm(p["pos"]))   # seen head-on
            s = Scene(name, "sum_order", flavour, store(pts), cam, range(8), lambda tr: tr["sum_order_matters"] > 0)
            o = s.project()
            if o["trace"]["sum_order_matters"] and o["in_view"].all() and outcome(o) != outcome(s.project("sum_order")):
                out.append(s)
                break
        else:
            raise AssertionError("no sum whose orders differ")
    for name, flavour, rule in (("proj_order_frustum", R.FRUSTUM, "proj_order"), ("proj_order_fuse", R.FUSE, "fuse_proj_order")):
        for seed in range(200):
            rs = np.random.RandomState(seed)
            pts = [{"pos": (f32(rs.uniform(-2, 2)), f32(rs.uniform(-1.5, 1.5)), f32(rs.uniform(3, 6)))} for _ in range(8)]
            s = Scene(name, rule, flavour, store(pts), R.Camera(fx=31.7, fy=33.1, cx=47.3, cy=31.9), range(8), lambda tr: tr["proj_order_matters"] > 0)
            if outcome(s.project()) != outcome(s.project(rule)):
                out.append(s)
                break
        else:
            raise AssertionError("no projection whose forms differ")
    return out


def _features_at(o, P, ids, extra=20, seed=5, jitter=0.4, flips=6, u_right=None):
    """a feature near every in-view query (its descriptor the point's with a few bits flipped, its size the predicted one) plus `extra`
    features elsewhere"""
    rs = np.random.RandomState(seed)
    x, y, sz, rows = [], [], [], []
    nb = P.descriptors.shape[1]
    for q in np.flatnonzero(o["in_view"]):
        x.append(f32(o["u"][q] + rs.uniform(-jitter, jitter)))
        y.append(f32(o["v"][q] + rs.uniform(-jitter, jitter)))
        sz.append(o["size"][q])
        d = P.descriptors[ids[q]].copy()
        for b in rs.randint(0, 8 * nb, flips):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        rows.append(d)
    for _ in range(extra):
        x.append(f32(rs.uniform(0, W))); y.append(f32(rs.uniform(0, H))); sz.append(f32(rs.uniform(0.8, 2.5)))
        rows.append(rs.randint(0, 256, nb).astype(np.uint8))
    n = len(x)
    return Features(x, y, sz, np.array(rows, np.uint8).reshape(n, nb), angles=rs.uniform(0, 360, n), u_right=u_right)


def search_scenes():
    out = []
    cam = R.Camera(mbf=8.0)
    # the stereo gate of SearchByProjection(F, vpMapPoints) is r * trackSigma: radius_scale 1 and th 1 make r = 2.5 * size = 2.5 exactly,
    # the gate 2.5 * 0.5 = 1.25; ur = 48 - 8 / 4 = 46.  Feature 0 sits at the gate (er == gate passes), feature 1 is the better match
    # beyond it (er = 2)
    P = store([{"pos": (0, 0, 4), "ref_size": 1.0, "ref_dist": 4.0, "ref_sigma": 0.5}, {"pos": (1, 0.75, 4)}, {"pos": (-1, -0.75, 4)}])
    d = P.descriptors[0]
    d1 = d.copy(); d1[0] ^= 0x0f
    feat = Features([48.5, 47.5], [32.0, 32.0], [1.0, 1.0], np.stack([d1, d]), u_right=[47.25, 48.0])
    out.append(Scene("er_sigma_gate", "er_sigma", R.FRUSTUM, P, cam, [0, 1, 2], lambda tr: True, radius_scale=1.0, radius_th=1.0, feat=feat))
    # the last-frame search gates |ur - mvuRight| by the window radius itself: size 1, th 2, radius_scale 1 make r = 2; ur = 46.
    # Feature 0 sits at the gate (er == 2 passes), feature 1 is the better match beyond it (er = 2.5)
    feat = Features([48.5, 47.5], [32.0, 32.0], [1.0, 1.0], np.stack([d1, d]), u_right=[48.0, 48.5])
    out.append(Scene("stereo_gate_lastframe", None, R.LASTFRAME, P, cam, [0, 1, 2], lambda tr: True, radius_scale=1.0, radius_th=2.0, feat=feat,
                     last_sizes=[1.0, 1.0, 1.0], last_angles=[0, 0, 0]))
    # Fuse with the chi-square gate on a stereo keyframe (keyPtsInf = 1 / size^2 = 1): point 0 projects to (48, 32), ur = 46.  Feature 0
    # (ex = -1, er = -1: e2 = 2) passes the 3-dof gate, feature 1 is the better match with er = -4 (e2 = 16.25 > 7.8).  Point 1 projects to
    # (56, 38): feature 2, monocular and the better match, fails the 2-dof gate (ex = -2.5: 6.25 > 5.99), feature 3 (ex = -1) passes
    d2 = P.descriptors[1]
    d3 = d2.copy(); d3[0] ^= 0x0f
    feat = Features([49.0, 48.5, 58.5, 57.0], [32.0, 32.0, 38.0, 38.0], [1.0, 1.0, 1.0, 1.0], np.stack([d1, d, d2, d3]), u_right=[47.0, 50.0, -1.0, -1.0])
    out.append(Scene("stereo_fuse_inf_gate", None, R.FUSE, P, cam, [0, 1, 2], lambda tr: True, radius_th=3.0, feat=feat, inf_gate=True))
    # validity: -1, an unset id, a bad point and an unobserved one among good ones
    pts = [{"pos": (0, 0, 4)}, {"pos": (1, 0, 4), "bad": 1}, {"pos": (0, 1, 4), "unset": 1}, {"pos": (-1, 0, 4), "observed": 0},
           {"pos": (0, -1, 4)}, {"pos": (-1, -0.75, 4), "observed": 0}]
    P = store(pts)
    ids = [0, -1, 1, 2, 3, -1, 4, 5, 3]
    for rule, what in (("bad_invalid", "bad"), ("unset_invalid", "unset"), ("occ_observed", "minus1")):
        for fname in ("frustum", "fuse"):
            fl = R.FLAVOURS[fname]
            s = Scene("validity_%s_%s" % (rule, fname), rule, fl, P, cam, ids, (lambda w: lambda tr: tr["invalid"][w] > 0)(what), radius_th=3.0)
            s.feat = _features_at(s.project(), P, s.ids, extra=10)
            out.append(s)
    # two points contest one feature: the ordered phase follows the order of ids.  Both project next to the one feature; the second is
    # the better match but the first comes first and occupies it
    pts = [{"pos": (0, 0, 4)}, {"pos": (0.01, 0, 4)}, {"pos": (1.5, 1, 4)}]
    P = store(pts)
    P.descriptors[1] = P.descriptors[0]
    P.descriptors[0, 0] ^= 0x03
    feat = Features([48.0, 60.2], [32.0, 40.1], [1.0, 1.0], np.stack([P.descriptors[1], P.descriptors[2]]))
    for name, order in (("contest_order_01", [0, 1, 2]), ("contest_order_10", [1, 0, 2])):
        out.append(Scene(name, None, R.FRUSTUM, P, cam, order, lambda tr: True, radius_th=2.0, feat=feat))
    # the last-frame search: query q takes size and angle of the last frame's feature q
    pts = [{"pos": (f32(x), f32(y), 4)} for x, y in ((0, 0), (1, 0.5), (-1, -0.5), (2, 1), (-2, 1), (0.5, -1.5))]
    P = store(pts)
    s = Scene("lastframe_search", None, R.LASTFRAME, P, cam, [0, 1, -1, 2, 3, 4, 5], lambda tr: True, radius_th=7.0,
              last_sizes=[1.0, 1.2, 1.0, 1.44, 1.0, 1.2, 1.0], last_angles=[10, 20, 30, 40, 50, 60, 70], check_orientation=True)
    o = s.project()
    s.feat = _features_at(o, P, s.ids, extra=12)
    s.feat.sizes[:int(o["in_view"].sum())] = o["size"][o["in_view"]]
    s.feat.angles[:int(o["in_view"].sum())] = np.asarray(s.last_angles)[o["in_view"]] + f32(3.0)
    out.append(s)
    r = Scene("reloc_search", None, R.RELOC, P, cam, [0, 1, -1, 2, 3, 4, 5], lambda tr: True, radius_th=7.0,
              last_angles=[10, 20, 30, 40, 50, 60, 70], check_orientation=True)
    r.feat = _features_at(r.project(), P, r.ids, extra=12)
    out.append(r)
    return out


def all_constructed():
    return bound_scenes() + band_scenes() + angle_scenes() + depth_scenes() + order_scenes() + search_scenes()


# ---- seeded random scenes: 300 points around the frustum ----
REJECTS = {R.FRUSTUM: ("depth", "bounds", "band_lo", "band_hi", "view_cos"), R.LASTFRAME: ("depth", "bounds"),
           R.RELOC: ("bounds", "band_lo", "band_hi"), R.FUSE: ("depth", "bounds", "band_lo", "band_hi", "fuse_dot")}


def random_scene(seed, flavour, n=300, desc_bytes=32, cap=512):
    rs = np.random.RandomState(1000 + seed)
    cam = R.Camera(Rcw=rotation(*rs.uniform(-0.06, 0.06, 3)), tcw=rs.uniform(-0.2, 0.2, 3), mbf=8.0)
    z = rs.uniform(2.0, 9.0, n)
    z[rs.rand(n) < 0.08] *= -1                       # behind the camera
    x = rs.uniform(-1.9, 1.9, n) * np.abs(z)         # the image spans |X / Z| <= 1.5
    y = rs.uniform(-1.25, 1.25, n) * np.abs(z)
    pos = np.stack([x, y, z], 1).astype(np.float32)
    dist = np.linalg.norm(pos - cam.Ow, axis=1)
    # the normal points from where the point was seen towards the point: PO . Pn > 0 from the front; viewing angles around the 60 degree limit
    nrm = (pos - cam.Ow) / dist[:, None] + rs.normal(0, 0.45, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    P = R.Points(cap, desc_bytes)
    ids = rs.permutation(cap)[:n]                     # shuffled ids
    P.set(ids, pos=pos, normal=nrm, min_distance=dist * rs.uniform(0.6, 1.45, n),
          max_distance=dist * rs.uniform(0.7, 1.6, n), ref_size=rs.uniform(1.0, 2.0, n), ref_distance=dist * rs.uniform(0.7, 1.4, n),
          ref_sigma=rs.uniform(0.3, 1.0, n))
    P.set_flags(ids, bad=rs.rand(n) < 0.05, observed=rs.rand(n) < 0.7)
    P.set_descriptors(ids, rows_for(n, desc_bytes, 77 + seed))
    q = ids.astype(np.int32).copy()
    q[rs.rand(n) < 0.04] = -1
    never = rs.permutation(cap)                       # ... and ids nobody ever set
    never = never[~np.isin(never, ids)]
    hole = np.flatnonzero(rs.rand(n) < 0.03)
    q[hole] = never[:len(hole)]
    last = rs.choice([1.0, 1.2, 1.44, 1.728], n).astype(np.float32) if flavour == R.LASTFRAME else None
    ang = rs.uniform(0, 360, n).astype(np.float32) if flavour in (R.LASTFRAME, R.RELOC) else None
    s = Scene("random_%d_%s" % (seed, [k for k, v in R.FLAVOURS.items() if v == flavour][0]), None, flavour, P, cam, q, lambda tr: True,
              radius_th=3.0, last_sizes=last, last_angles=ang, check_orientation=ang is not None)
    o = s.project()
    keep = np.flatnonzero(o["in_view"])[:100]
    sub = {k: (v[keep] if isinstance(v, np.ndarray) else v) for k, v in o.items()}
    sub["in_view"] = np.ones(len(keep), bool)
    s.feat = _features_at(sub, P, q[keep], extra=30, seed=seed, u_right=None)
    return s


def grid_view(afv, s):
    """the scene's feature side as the FrameGridView tests/_proj_ref.py reads (the 96 x 64 frame, the default 64 x 48 grid)"""
    f = s.feat
    inf = None
    if s.inf_gate:   # keyPtsInf as a frame derives it from keyPtsSize: 1 / size^2 (FeatureExtractor.cpp:160-170), in float
        inf = f32(1.0) / (f.sizes * f.sizes)
    return afv.FrameGridView(f.desc, np.stack([f.x, f.y], 1), f.sizes, angles=f.angles, occupied=s.occupied, max_x=W, max_y=H,
                             size_tolerance=float(s.cam.tol), inf=inf, u_right=f.u_right)


def expected_search(afv, PR, s, flip=None, proj_flip=None):
    """the restatement composed with tests/_proj_ref.py: (assign | best, count, project()'s dict)"""
    Q, o = s.queries(flip)
    F = grid_view(afv, s)
    if s.flavour == R.FUSE:
        got, n, _ = PR.match_projection(F, Q, th_high=s.th, fuse=True, flip=proj_flip)
    else:
        got, n, _ = PR.match_projection(F, Q, th_high=s.th, nnratio=s.nnratio, check_orientation=s.check_orientation and s.flavour != R.FRUSTUM,
                                        last_frame=s.flavour != R.FRUSTUM, flip=proj_flip)
    return got, n, o
