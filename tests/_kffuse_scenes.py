"""Constructed scenes and seeded random maps for Fuse into keyframes of the table (tests/_kffuse_ref.py; -m gpu: tests/test_gpu_kffuse.py).
TEST INFRASTRUCTURE ONLY.

Each constructed scene is named after the rule it reaches; tests/test_kffuse_ref_cpu.py proves on the CPU that the restatement reaches it
(`reached`, over the per-job results of Scene.run) and, where a rule can be turned around, that doing so changes the answer.  The geometric
edges are the FUSE scenes of tests/_points_scenes.py with a feature side and a plane added.  The default camera looks down +z from the origin
with fx = fy = 32, cx = 48, cy = 32 on a 96 x 64 image and a 64 x 48 grid: a point at (X, Y, 4) with ref_size 1 and ref_distance 4 projects
to (48 + 8 X, 32 + 8 Y) with predicted size 1, window radius 1.15 * 3 = 3.45 and size band 1 / 1.2 .. 1.2.
"""
import numpy as np

import _kffuse_ref as K
import _points_ref as R
import _points_scenes as S

f32 = np.float32
TH = 64.0
# the rules of _points_ref whose turning around moves a status (a last bit of u, or a point every other test rejects too, does not)
TURNABLE = ("fuse_bound_max", "fuse_bound_min", "band_lo", "band_hi", "band_factor", "fuse_dot")


class Scene:
    def __init__(self, name, rule, P, kfs, jobs, reached, grid=None, flip=None, proj_flip=None):
        self.name, self.rule, self.P, self.kfs, self.jobs, self.reached = name, rule, P, kfs, jobs, reached
        self.grid = K.Grid() if grid is None else grid
        self.flip, self.proj_flip = flip, proj_flip   # the rule of _points_ref / _proj_ref that, turned around, changes the answer

    def run(self, flip=None, proj_flip=None):
        return [K.fuse_target(self.P, self.kfs[j["slot"]], self.grid, j["ids"], j.get("radius_th", 3.0), j.get("th_low", TH),
                              j.get("use_inf_gate", True), j.get("pose"), flip=flip, proj_flip=proj_flip) for j in self.jobs]


def answer(res):
    return b"".join(np.ascontiguousarray(a).tobytes() for r in res for a in r[:3])


def near(d, flips, seed=0):
    """a row `flips` bits away from d"""
    d = d.copy()
    for b in np.random.RandomState(seed).permutation(8 * len(d))[:flips]:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def kf_of(feats, plane=None, cam=None, u_right=None):
    """feats: list of (x, y, size, row)"""
    x, y, sz, rows = zip(*feats)
    return K.Keyframe(x, y, sz, np.stack(rows), plane, u_right, None, R.Camera() if cam is None else cam)


def status_scene():
    pts = [{"pos": (0, 0, 4)}, {"pos": (0.5, 0.5, 4), "bad": 1}, {"pos": (1, 0, 4)}, {"pos": (0, 0, -4)}, {"pos": (-1, 0, 4)}, {"pos": (0, 1, 4)},
           {"pos": (3, 3, 4), "bad": 1}, {"pos": (0, -1, 4)}, {"pos": (-3, -3, 4)}]
    P = S.store(pts)
    d = P.descriptors
    feats = [(48.5, 32.0, 1.0, near(d[0], 3)), (48.0, 40.3, 1.0, near(d[5], 4)), (48.2, 24.0, 1.0, near(d[7], 2)), (80.0, 50.0, 1.0, near(d[2], 1))]
    kf = kf_of(feats, plane=[-1, 6, 8, 2])
    want = [K.FREE, K.INVALID, K.IN_KEYFRAME, K.NOT_IN_VIEW, K.NO_FEATURE, K.OCCUPANT_BAD, K.REPLACE, K.INVALID]
    return Scene("every_status", None, P, {0: kf}, [dict(slot=0, ids=[0, 1, 2, 3, 4, 5, 7, -1])],
                 lambda res: list(res[0][2]) == want and res[0][3] == 3 and list(res[0][1]) == [-1, -1, -1, -1, -1, 6, 8, -1])


def plane_scenes():
    out = [status_scene()]
    # already in the keyframe at a feature OTHER than the one it would win: the rule is membership, not "the winning feature holds me"
    P = S.store([{"pos": (0, 0, 4)}, {"pos": (1, 1, 4)}])
    d = P.descriptors
    kf = kf_of([(48.3, 32.0, 1.0, near(d[0], 2)), (70.0, 20.0, 1.0, near(d[1], 30))], plane=[-1, 0])
    out.append(Scene("member_elsewhere", "member", P, {0: kf}, [dict(slot=0, ids=[0, 1])],
                     lambda res: res[0][2][0] == K.IN_KEYFRAME and res[0][0][0] == -1 and K._best_of(P, kf, K.Grid(), 0, th_low=TH)[0] == 0))
    # two queries win one free feature: the snapshot answers both with status 4
    P2 = S.store([{"pos": (0, 0, 4)}, {"pos": (0.01, 0, 4)}, {"pos": (2, 1, 4)}])
    P2.descriptors[1] = near(P2.descriptors[0], 2, 1)
    kf2 = kf_of([(48.0, 32.0, 1.0, P2.descriptors[0]), (10.0, 10.0, 1.0, P2.descriptors[2])])
    out.append(Scene("two_win_one_free", "snapshot", P2, {0: kf2}, [dict(slot=0, ids=[0, 1, 2])],
                     lambda res: list(res[0][0][:2]) == [0, 0] and list(res[0][2][:2]) == [K.FREE, K.FREE]))
    # the occupant is bad in the store
    P3 = S.store([{"pos": (0, 0, 4)}, {"pos": (2, 2, 4), "bad": 1}])
    kf3 = kf_of([(48.0, 32.0, 1.0, near(P3.descriptors[0], 1))], plane=[1])
    out.append(Scene("occupant_bad", "occupant_bad", P3, {0: kf3}, [dict(slot=0, ids=[0])],
                     lambda res: res[0][2][0] == K.OCCUPANT_BAD and res[0][1][0] == 1 and res[0][3] == 1))
    # occupants the store never saw: an id never set, one never set whose BAD bit is on, one beyond the capacity - all good (6)
    P4 = S.store([{"pos": (0, 0, 4)}, {"pos": (1, 0, 4)}, {"pos": (0, 1, 4)}])
    P4.flags[41] |= R.BAD
    d = P4.descriptors
    kf4 = kf_of([(48.0, 32.0, 1.0, near(d[0], 1)), (56.0, 32.0, 1.0, near(d[1], 1)), (48.0, 40.0, 1.0, near(d[2], 1))], plane=[40, 41, 1000])
    out.append(Scene("occupant_never_set", "occupant_unset_good", P4, {0: kf4}, [dict(slot=0, ids=[0, 1, 2])],
                     lambda res: list(res[0][2]) == [K.REPLACE] * 3 and list(res[0][1]) == [40, 41, 1000]))
    return out


def tie_scenes():
    out = []
    P = S.store([{"pos": (0, 0, 4)}])
    row = near(P.descriptors[0], 5)
    # two features at one distance in different cells: the cell with the smaller ix is visited first, though it holds the larger index
    kf = kf_of([(49.6, 32.0, 1.0, row), (46.9, 32.0, 1.0, row)])
    out.append(Scene("tie_across_cells", "tie_first", P, {0: kf}, [dict(slot=0, ids=[0])],
                     lambda res: res[0][4]["tr"]["eq"]["tie_first"] > 0 and res[0][0][0] == 1, proj_flip="tie_first"))
    # ... and inside one cell: ascending feature index
    kf = kf_of([(48.2, 32.0, 1.0, row), (48.1, 32.1, 1.0, row)])
    out.append(Scene("tie_inside_cell", "tie_first", P, {0: kf}, [dict(slot=0, ids=[0])],
                     lambda res: res[0][4]["tr"]["eq"]["tie_first"] > 0 and res[0][0][0] == 0, proj_flip="tie_first"))
    return out


def size_scene():
    P = S.store([{"pos": (0, 0, 4)}, {"pos": (0, 0, 4)}])   # (two points at one place: their random rows are far apart)
    d = P.descriptors
    qmin, qmax = f32(1.0) / f32(1.2), f32(1.0) * f32(1.2)
    # the band is closed at both ends: size == qmin and size == qmax are candidates, one float outside they are not - and those are the
    # better matches
    feats = [(48.3, 32.0, qmin, near(d[0], 6)), (47.8, 32.0, S.down(qmin), d[0]), (48.2, 33.0, S.up(qmax), d[1]), (47.9, 31.0, qmax, near(d[1], 6))]
    kf = kf_of(feats)
    reach = lambda res: (res[0][4]["tr"]["eq"]["size_lt_min"] > 0 and res[0][4]["tr"]["eq"]["size_gt_max"] > 0 and list(res[0][0]) == [0, 3])
    return [Scene("size_band_lo", "size_lt_min", P, {0: kf}, [dict(slot=0, ids=[0, 1])], reach, proj_flip="size_lt_min"),
            Scene("size_band_hi", "size_gt_max", P, {0: kf}, [dict(slot=0, ids=[0, 1])], reach, proj_flip="size_gt_max")]


def gate_scenes():
    out = []
    cam = R.Camera(mbf=8.0)
    # keyPtsInf = 1 / size^2 = 1.  Mono: e2 = ex^2 around 5.99 (2.447^2 = 5.9878, 2.448^2 = 5.9927); the gated feature is the better match
    P = S.store([{"pos": (0, 0, 4)}, {"pos": (0, 1, 4)}])
    d = P.descriptors
    # stereo: the query's ur = 48 - 8 / 4 = 46; ex = 2, e2 = 4 + er^2 around 7.8 (er = 1.949: 7.7986, er = 1.950: 7.8025)
    feats = [(48.0 + 2.448, 32.0, 1.0, d[0]), (48.0 - 2.447, 32.0, 1.0, near(d[0], 6)),
             (50.0, 40.0, 1.0, d[1]), (46.0, 40.0, 1.0, near(d[1], 6))]
    kf = kf_of(feats, cam=cam, u_right=[-1.0, -1.0, 46.0 - 1.950, 46.0 + 1.949])

    def reach(res):
        tr = res[0][4]["tr"]
        return tr["drop"]["chi2_2dof"] == 1 and tr["drop"]["chi2_3dof"] == 1 and list(res[0][0]) == [1, 3]
    out.append(Scene("gates_599_and_78_both_sides", "inf_gate", P, {0: kf}, [dict(slot=0, ids=[0, 1], use_inf_gate=True)], reach))
    # the same slot through Fuse no. 2: no gate, the better matches win
    out.append(Scene("no_gate_sim3_flavour", "no_gate", P, {0: kf}, [dict(slot=0, ids=[0, 1], use_inf_gate=False)],
                     lambda res: list(res[0][0]) == [0, 2]))
    return out


def sim3_scene():
    """Scw = [2 R | t]: the reference divides the rotation by scw = 2 and leaves t as it stands.  The point projects to u = 52 (t kept) or
    u = 50 (t / 2); the exact match at 47.0 lies inside the window only in the second case"""
    P = S.store([{"pos": (0, 0, 4)}])
    d = P.descriptors
    kf = kf_of([(52.3, 32.0, 1.0, near(d[0], 5)), (47.0, 32.0, 1.0, d[0])])
    Scw = np.eye(4, dtype=np.float32)
    Scw[:3, :3] *= f32(2.0)
    Scw[:3, 3] = (0.5, 0.0, 0.0)
    Rcw, tcw, Ow = K.decompose_scw(Scw)
    fixed = (Rcw, tcw / f32(2.0), R.twc(Rcw, tcw / f32(2.0)))
    job = dict(slot=0, ids=[0], radius_th=4.0, use_inf_gate=False, pose=(Rcw, tcw, Ow))

    def reach(res):
        other = K.fuse_target(P, kf, K.Grid(), [0], 4.0, TH, False, fixed)
        return np.array_equal(tcw, Scw[:3, 3]) and res[0][0][0] == 0 and other[0][0] == 1
    s = Scene("scw_scale_2_translation_kept", "sim3_quirk", P, {0: kf}, [job], reach)
    s.Scw = Scw
    return [s]


def geometry_scenes():
    """the FUSE scenes of tests/_points_scenes.py: half-open IsInImage, z = -0.0f / +0.0f, both ends of the distance band, the viewing
    angle, the sum and projection orders, validity, the stereo gate scene with mixed mvuRight"""
    out = []
    for s in S.all_constructed():
        if s.flavour != R.FUSE:
            continue
        o = s.project()
        feat = s.feat if s.feat is not None else S._features_at(o, s.P, s.ids, extra=8, seed=3)
        kf = K.Keyframe(feat.x, feat.y, feat.sizes, feat.desc, None, feat.u_right, None, s.cam)
        job = dict(slot=0, ids=s.ids, radius_th=float(s.radius_th), th_low=s.th, use_inf_gate=bool(s.inf_gate))
        out.append(Scene("points_" + s.name, s.rule, s.P, {0: kf}, [job], (lambda sc: lambda res: sc.reached(res[0][4]["o"]["trace"]))(s),
                         flip=s.rule if s.rule in TURNABLE else None))
    return out


def all_constructed():
    return plane_scenes() + tie_scenes() + size_scene() + gate_scenes() + sim3_scene() + geometry_scenes()


# ---- a small map for the sequential loops ----
def small_map(seed=0):
    """three keyframes that see a handful of points, some of them twice under two ids (the duplicates CreateNewMapPoints leaves)"""
    rs = np.random.RandomState(300 + seed)
    n = 12
    pts = [{"pos": (f32(rs.uniform(-1.5, 1.5)), f32(rs.uniform(-1, 1)), 4)} for _ in range(n)]
    pts += [dict(p) for p in pts[:5]]            # ids 12..16 duplicate ids 0..4
    P = S.store(pts, cap=64, desc_seed=9 + seed)
    for k in range(5):
        P.descriptors[n + k] = near(P.descriptors[k], 2, k)
    kfs = {}
    for s in range(3):
        cam = R.Camera(tcw=(0.05 * s, 0, 0))
        o = R.project(P, cam, np.arange(n), R.FUSE, radius_th=3.0)
        feats, plane = [], []
        for q in range(n):
            feats.append((f32(o["u"][q] + rs.uniform(-0.3, 0.3)), f32(o["v"][q] + rs.uniform(-0.3, 0.3)), o["size"][q],
                          near(P.descriptors[q], 3, 50 * s + q)))
            # keyframe 0 holds the originals, keyframe 1 the duplicates of 0..4 and nothing else, keyframe 2 points 5..8
            plane.append(q if s == 0 else (n + q if s == 1 and q < 5 else (q if s == 2 and 5 <= q < 9 else -1)))
        kfs[s] = kf_of(feats, plane=plane, cam=cam)
    return P, kfs


# ---- seeded random maps ----
class Map:
    def __init__(self, name, P, kfs, lists, grid, th_low):
        self.name, self.P, self.kfs, self.lists, self.grid, self.th_low = name, P, kfs, lists, grid, th_low


def random_map(seed, nq, nfeat, ntargets, desc_bytes=32, float_dim=0, stereo=False, per_target=False, cap=None):
    """ntargets keyframes around the origin looking down +z, nq points in front of them (some behind, some bad, some never set, some -1),
    nfeat features per keyframe: near the projections of points (rows a few bits / a little noise away) and elsewhere; the planes hold
    query points (status 1), other good points, bad ones and ids the store never saw"""
    rs = np.random.RandomState(7000 + seed)
    cap = max(2 * nq + 16, 64) if cap is None else cap
    P = R.Points(cap, desc_bytes, float_dim)
    n = max(nq, 1)
    ids = rs.permutation(cap)[:n]
    z = rs.uniform(2.5, 8.0, n)
    z[rs.rand(n) < 0.06] *= -1
    pos = np.stack([rs.uniform(-1.4, 1.4, n) * np.abs(z), rs.uniform(-0.95, 0.95, n) * np.abs(z), z], 1).astype(np.float32)
    dist = np.linalg.norm(pos, axis=1)
    nrm = pos / dist[:, None] + rs.normal(0, 0.35, (n, 3))
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    P.set(ids, pos=pos, normal=nrm, min_distance=dist * rs.uniform(0.5, 1.3, n), max_distance=dist * rs.uniform(0.8, 1.8, n),
          ref_size=rs.uniform(1.0, 2.0, n), ref_distance=dist * rs.uniform(0.8, 1.25, n), ref_sigma=rs.uniform(0.3, 1.0, n))
    P.set_flags(ids, bad=rs.rand(n) < 0.06, observed=rs.rand(n) < 0.7)
    if float_dim:
        rows = rs.uniform(0, 1, (n, float_dim)).astype(np.float32)
    else:
        rows = rs.randint(0, 256, (n, desc_bytes)).astype(np.uint8)
    P.set_descriptors(ids, rows)
    never = np.setdiff1d(np.arange(cap), ids)
    grid = K.Grid()
    kfs = {}
    for s in range(ntargets):
        cam = R.Camera(Rcw=S.rotation(*rs.uniform(-0.05, 0.05, 3)), tcw=rs.uniform(-0.15, 0.15, 3), mbf=8.0 if stereo else 0.0)
        o = R.project(P, cam, ids, R.FUSE, radius_th=3.0)
        seen = np.flatnonzero(o["in_view"])
        x, y, sz, dr, owner = [], [], [], [], []
        for k in range(nfeat):
            if len(seen) and rs.rand() < 0.7:
                q = int(seen[rs.randint(len(seen))])
                x.append(f32(o["u"][q] + rs.uniform(-1.5, 1.5))); y.append(f32(o["v"][q] + rs.uniform(-1.5, 1.5)))
                sz.append(f32(o["size"][q] * rs.choice([1.0, 1.0, 1.1, 1.25, 0.8])))
                if float_dim:
                    dr.append((rows[q] + rs.normal(0, 0.05, float_dim)).astype(np.float32))
                else:
                    dr.append(near(rows[q], int(rs.randint(0, 12)), int(rs.randint(1 << 30))))
                owner.append(q)
            else:
                x.append(f32(rs.uniform(0, 96))); y.append(f32(rs.uniform(0, 64))); sz.append(f32(rs.uniform(0.8, 2.5)))
                dr.append(rs.uniform(0, 1, float_dim).astype(np.float32) if float_dim else rs.randint(0, 256, desc_bytes).astype(np.uint8))
                owner.append(-1)
        plane = np.full(nfeat, -1, np.int32)
        for k in range(nfeat):
            r = rs.rand()
            if r < 0.25:
                plane[k] = ids[rs.randint(n)]        # a point of the store: good, bad, maybe a query of the call
            elif r < 0.30 and len(never):
                plane[k] = never[rs.randint(len(never))]
            elif r < 0.32:
                plane[k] = cap + rs.randint(100)
        ur = None
        if stereo:
            ur = np.where(rs.rand(nfeat) < 0.5, np.asarray(x, np.float32) - f32(2.0) + rs.uniform(-1, 1, nfeat).astype(np.float32), f32(-1.0))
        kfs[s] = K.Keyframe(x, y, sz, np.stack(dr) if nfeat else np.zeros((0, float_dim or desc_bytes), np.float32 if float_dim else np.uint8),
                            plane, ur, None, cam)

    def qlist(r):
        q = ids[:nq].astype(np.int32).copy()
        r.shuffle(q)
        q[r.rand(nq) < 0.04] = -1
        hole = np.flatnonzero(r.rand(nq) < 0.03)
        if len(never):
            q[hole] = never[r.randint(len(never), size=len(hole))]
        return q
    lists = [qlist(np.random.RandomState(seed * 131 + s)) for s in range(ntargets)] if per_target else [qlist(rs)] * ntargets
    th = 0.6 if float_dim else 50.0
    return Map("random_%d_q%d_f%d_t%d" % (seed, nq, nfeat, ntargets), P, kfs, lists, grid, th)


def expected(m, use_inf_gate=True, poses=None):
    jobs = [dict(slot=s, ids=m.lists[s], th_low=m.th_low, use_inf_gate=use_inf_gate, pose=None if poses is None else poses[s]) for s in sorted(m.kfs)]
    return K.fuse_batch(m.P, m.kfs, m.grid, jobs)
