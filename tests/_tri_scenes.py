"""Scenes for the match loop of CreateNewMapPoints (tests/_tri_ref.py).  TEST INFRASTRUCTURE ONLY.

A scene is ONE match: a job record, a feature of keyframe a and a feature of keyframe b.  Every constructed scene sits on one comparison of
the routine and has a twin on the other side of it.  Where the comparison has a free input (a sigma2, a size, a depth, a keypoint
coordinate, a pose entry) the pair is found by bisection over the float grid of that input: the two scenes differ by ONE ulp of it and end on
different sides.  The job records of some scenes are not poses of a camera (a zero column, an Ow that is not -R^T t): the routine takes the
record as numbers, and the comparison is what the scene is about.

SCENES: name -> Scene (with .twin).  pack() lays any list of scenes out as two keyframes (scene k = feature k of each) with one pair per
scene, which is how the GPU test sends them: one call, one pair per scene.
"""
import numpy as np

import _tri_ref as R
from _points_ref import twc

f32 = np.float32
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
TOL = 1.2


def feat(x, y, sigma2=1.0, size=1.2, u_right=-1.0, depth=-1.0, x_dist=None, y_dist=None):
    return {"x": f32(x), "y": f32(y), "sigma2": f32(sigma2), "size": f32(size), "u_right": f32(u_right), "depth": f32(depth),
            "x_dist": f32(x if x_dist is None else x_dist), "y_dist": f32(y if y_dist is None else y_dist)}


def kf_of(feats):
    g = lambda k: np.array([f[k] for f in feats], np.float32)
    return R.KF(g("x"), g("y"), g("sigma2"), g("size"), g("u_right"), g("depth"), g("x_dist"), g("y_dist"))


def make_job(R1=None, t1=(0, 0, 0), R2=None, C2=(0.5, 0, 0), mb1=0.1, mb2=0.1, mbf1=50.0, **over):
    R1 = np.eye(3) if R1 is None else np.asarray(R1, np.float64).reshape(3, 3)
    R2 = np.eye(3) if R2 is None else np.asarray(R2, np.float64).reshape(3, 3)
    t1 = np.asarray(t1, np.float32)
    t2 = (-R2 @ np.asarray(C2, np.float64)).astype(np.float32)
    kw = dict(fx1=FX, fy1=FY, cx1=CX, cy1=CY, invfx1=f32(1) / f32(FX), invfy1=f32(1) / f32(FY), fx2=FX, fy2=FY, cx2=CX, cy2=CY,
              invfx2=f32(1) / f32(FX), invfy2=f32(1) / f32(FY), mb1=mb1, mb2=mb2, mbf1=mbf1, ratio_factor=f32(1.5) * f32(TOL), max_size1=f32(TOL) ** 7)
    geo = dict(Rcw1=R1, tcw1=t1, Ow1=twc(R1, t1), Rcw2=R2, tcw2=t2, Ow2=twc(R2, t2))
    for k in list(over):
        if k in geo:
            geo[k] = over.pop(k)
    kw.update(over)
    return R.Job(geo["Rcw1"], geo["tcw1"], geo["Ow1"], geo["Rcw2"], geo["tcw2"], geo["Ow2"], **kw)


def project(Rcw, tcw, P):
    """pinhole projection in float64 -> (u, v, z)"""
    pc = np.asarray(Rcw, np.float64).reshape(3, 3) @ np.asarray(P, np.float64) + np.asarray(tcw, np.float64)
    return FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY, pc[2]


class Scene:
    def __init__(self, name, job, fa, fb, on=""):
        self.name, self.job, self.fa, self.fb, self.on = name, job, fa, fb, on
        self.twin = None
        self.status, self.route, self.x3d = R.triangulate_match(job, kf_of([fa]), 0, kf_of([fb]), 0)

    def cos_rays(self):
        return R.cos_parallax_rays(self.job, kf_of([self.fa]), 0, kf_of([self.fb]), 0)


def _ord(v):
    v = f32(v)
    assert v > 0
    return int(v.view(np.int32))


def straddle(make, lo, hi, pred):
    """two scenes whose free input differs by one ulp (both positive floats) and on which pred differs: (the one where pred holds, its twin)"""
    a, b = _ord(lo), _ord(hi)
    pa = pred(make(np.int32(a).view(f32)))
    assert pa != pred(make(np.int32(b).view(f32))), "the ends of the bisection agree"
    while b - a > 1:
        m = (a + b) // 2
        if pred(make(np.int32(m).view(f32))) == pa:
            a = m
        else:
            b = m
    sa, sb = make(np.int32(a).view(f32)), make(np.int32(b).view(f32))
    return (sa, sb) if pa else (sb, sa)


def _pair(s, t):
    s.twin, t.twin = t, s
    return s


def mono_match(P=(0.3, -0.2, 4.0), C2=(0.5, 0, 0), noise=(0.2, -0.1, -0.15, 0.1), job=None, **fkw):
    """an accepted monocular match of point P: (job, fa, fb)"""
    job = job or make_job(C2=C2)
    u1, v1, _ = project(job.Rcw1, job.tcw1, P)
    u2, v2, _ = project(job.Rcw2, job.tcw2, P)
    return job, feat(u1 + noise[0], v1 + noise[1], **fkw), feat(u2 + noise[2], v2 + noise[3], **fkw)


def stereo_feat(job_R, job_t, P, mbf, noise=(0.0, 0.0, 0.0), **kw):
    u, v, z = project(job_R, job_t, P)
    return feat(u + noise[0], v + noise[1], u_right=u - mbf / z + noise[2], depth=z, **kw)


def _with(d, **kw):
    d = dict(d)
    for k, v in kw.items():
        d[k] = f32(v)
    return d


ROT_Y90 = np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]], np.float64)   # Rcw of a camera that looks along world +x


def build():
    S = {}

    def add(name, pair, on):
        s, t = pair
        s.name, t.name, s.on, t.on = name, name + "_twin", on, on
        S[name] = _pair(s, t)

    # cosParallaxRays > 0: camera b looks along world +x at a point on a's optical axis, the rays are perpendicular
    jb = make_job(R2=ROT_Y90, C2=(-5, 0, 5))
    fb0 = feat(CX, CY)
    add("cos_rays_zero", straddle(lambda v: Scene("", jb, feat(v, CY), fb0), CX - 40, CX + 40, lambda s: not s.cos_rays() > 0),
        "cosParallaxRays > 0 (:348): the scene has cos <= 0 and ends as low parallax, the twin's cos is the next float up")
    # cosParallaxRays < 0.9998 (double): a short baseline and a far point
    job, fa, fb = mono_match(P=(0.0, 1.6, 4.0), C2=(0.08, 0, 0), noise=(0, 0, 0, 0))
    add("cos_rays_9998", straddle(lambda v: Scene("", job, fa, _with(fb, x=v, x_dist=v)), fb["x"] - 6, fb["x"] + 6,
                                  lambda s: not float(s.cos_rays()) < 0.9998),
        "(double)cosParallaxRays < 0.9998 (:348), both monocular: cos is the float above the literal | the float below it")
    s9 = S["cos_rays_9998"]   # (the point's height was chosen so that the quotient's rounding does not step over the float below)
    assert s9.cos_rays() == f32(0.9998) and s9.twin.cos_rays() == np.nextafter(f32(0.9998), f32(0))
    # cosParallaxRays against cosParallaxStereo, from either stereo side: the baseline mb of the stereo keyframe decides between the routes
    P = (0.3, -0.2, 4.0)
    jmb = lambda **kw: make_job(C2=(0.5, 0, 0), mbf1=300.0, **kw)
    job = jmb()
    fa_s, fb_m = stereo_feat(job.Rcw1, job.tcw1, P, 300.0), mono_match(P, job=job, noise=(0, 0, 0, 0))[2]
    add("stereo_a_cos", straddle(lambda v: Scene("", jmb(mb1=v, mb2=0.1), fa_s, fb_m), 0.01, 4.0, lambda s: s.route == R.UNPROJECT_A),
        "cosParallaxRays < cosParallaxStereo1 (:348, :373): unprojected from a | triangulated")
    fa_m, fb_s = mono_match(P, job=job, noise=(0, 0, 0, 0))[1], stereo_feat(job.Rcw2, job.tcw2, P, 300.0)
    add("stereo_b_cos", straddle(lambda v: Scene("", jmb(mb1=0.1, mb2=v), fa_m, fb_s), 0.01, 4.0, lambda s: s.route == R.UNPROJECT_B),
        "cosParallaxRays < cosParallaxStereo2 (:348, :377): unprojected from b | triangulated")
    # equal stereo cosines: perpendicular rays (cos = 0 exactly) and mb1 = 0 give cosParallaxStereo1 == cosParallaxStereo2 == 1
    je, jt = make_job(R2=ROT_Y90, C2=(-5, 0, 5), mb1=0.0), make_job(R2=ROT_Y90, C2=(-5, 0, 5), mb1=0.5)
    fs = feat(CX, CY, u_right=CX - 10.0, depth=5.0)
    add("stereo_cos_equal", (Scene("", je, fs, fb0), Scene("", jt, fs, fb0)),
        "cosParallaxStereo1 < cosParallaxStereo2 (:373) at equality: neither unprojection is chosen | mb1 > 0: unprojected from a")
    # w == 0: the first column of A is exactly zero (both `rotations` have a zero first column), vt.row(3) is (1, 0, 0, 0)
    Z = lambda e: np.array([[e, 0.6, 0.8], [0, 0.8, -0.6], [0, 0.0, 1.0]], np.float64)
    Z2 = np.array([[0, 0.8, 0.6], [0, -0.6, 0.8], [0, 0.1, 1.0]], np.float64)
    mk = lambda e: Scene("", make_job(Rcw1=Z(e), tcw1=np.array([0.1, 0.2, 1], np.float32), Rcw2=Z2, tcw2=np.array([0.3, -0.1, 1], np.float32),
                                      Ow1=np.zeros(3, np.float32), Ow2=np.zeros(3, np.float32)), feat(CX + 50, CY + 20), feat(CX - 30, CY + 10))
    add("w_zero", (mk(0.0), mk(1e-3)), "x3D_tmp.at<float>(3) == 0 (:366) | a first column that is not zero")
    # z1 / z2 at +0 and -0, through UnprojectStereo's (0, 0, -1) (depth <= 0; mb1 = 2 makes cosParallaxStereo1 = 0 <= cosParallaxRays)
    fu = feat(CX, CY, u_right=CX - 10.0, depth=-1.0)
    fm = feat(CX + 5, CY)
    mz = lambda t1z, r8=1.0, r67=0.0, t2z=2.0, r8b=1.0, r67b=0.0: Scene("", make_job(
        Rcw1=np.array([[1, 0, 0], [0, 1, 0], [r67, r67, r8]], np.float32), tcw1=np.array([0, 0, t1z], np.float32), Ow1=np.zeros(3, np.float32),
        Rcw2=np.array([[1, 0, 0], [0, 1, 0], [r67b, r67b, r8b]], np.float32), tcw2=np.array([0.1, 0, t2z], np.float32),
        Ow2=np.array([-0.1, 0, 0], np.float32), mb1=2.0), fu, fm)
    tiny = np.finfo(np.float32).tiny
    add("z1_plus_zero", (mz(1.0), mz(np.nextafter(f32(1), f32(2)))), "z1 <= 0 (:387) at z1 = +0 | the next float up")
    add("z1_minus_zero", (mz(-0.0, r8=0.0, r67=-1.0), mz(tiny, r8=0.0, r67=-1.0)), "z1 <= 0 (:387) at z1 = -0 | the smallest normal float")
    add("z2_plus_zero", (mz(2.0, t2z=1.0), mz(2.0, t2z=np.nextafter(f32(1), f32(2)))), "z2 <= 0 (:391) at z2 = +0 | the next float up")
    add("z2_minus_zero", (mz(2.0, t2z=-0.0, r8b=0.0, r67b=-1.0), mz(2.0, t2z=tiny, r8b=0.0, r67b=-1.0)), "z2 <= 0 (:391) at z2 = -0 | the smallest normal float")
    # the reprojection gates: sigma2 of the feature is the free input
    job = make_job(C2=(0.5, 0, 0), mb1=0.1, mb2=0.1, mbf1=50.0)
    _, fa, fb = mono_match(P, job=job)
    add("reproj1_mono", straddle(lambda v: Scene("", job, _with(fa, sigma2=v), fb), 1e-4, 4.0, lambda s: s.status == R.REPROJ1),
        "err2 > 5.991 * sigmaSquare1 (:406)")
    add("reproj2_mono", straddle(lambda v: Scene("", job, fa, _with(fb, sigma2=v)), 1e-4, 4.0, lambda s: s.status == R.REPROJ2),
        "err2 > 5.991 * sigmaSquare2 (:432)")
    fas = stereo_feat(job.Rcw1, job.tcw1, P, 50.0, noise=(0.2, -0.1, 0.15))
    fbs = stereo_feat(job.Rcw2, job.tcw2, P, 50.0, noise=(-0.15, 0.1, 0.2))
    add("reproj1_stereo", straddle(lambda v: Scene("", job, _with(fas, sigma2=v), fb), 1e-4, 4.0, lambda s: s.status == R.REPROJ1),
        "err2 > 7.8 * sigmaSquare1 (:417)")
    add("reproj2_stereo", straddle(lambda v: Scene("", job, fa, _with(fbs, sigma2=v)), 1e-4, 4.0, lambda s: s.status == R.REPROJ2),
        "err2 > 7.8 * sigmaSquare2 with a's mbf (:438, :443)")
    # dist == 0: Ow is the triangulated point itself, to the bit
    base = Scene("", job, fa, fb)
    assert base.status == R.ACCEPTED and base.route == R.TRIANGULATED
    for which in (1, 2):
        key = "Ow%d" % which
        near = base.x3d.copy()
        near[0] = np.nextafter(near[0], f32(10))
        add("dist%d_zero" % which, (Scene("", make_job(C2=(0.5, 0, 0), **{key: base.x3d}), fa, fb), Scene("", make_job(C2=(0.5, 0, 0), **{key: near}), fa, fb)),
            "dist%d == 0 (:454) | Ow one ulp away" % which)
    # the ratio test: size1 is the free input
    add("ratio_low", straddle(lambda v: Scene("", job, _with(fa, size=v), fb), 1.2, 12.0, lambda s: s.status == R.SCALE_RATIO),
        "ratioDist * ratioFactor < ratioOctave (:460)")
    add("ratio_high", straddle(lambda v: Scene("", job, _with(fa, size=v), fb), 0.05, 1.2, lambda s: s.status == R.SCALE_RATIO),
        "ratioDist > ratioOctave * ratioFactor (:460)")
    # a depth <= 0 in UnprojectStereo (KeyFrame.cc:662): (0, 0, -1) comes back | the smallest normal depth is unprojected
    ju = make_job(mb1=2.0)
    add("unproject_depth_zero", (Scene("", ju, _with(fu, depth=0.0), fm), Scene("", ju, _with(fu, depth=tiny), fm)),
        "z > 0 in UnprojectStereo (KeyFrame.cc:662)")
    # T3: a NaN in the distorted keypoint reaches x3D through UnprojectStereo
    jn = make_job(C2=(0.5, 0, 0), mb1=2.0, mbf1=300.0)
    fn = stereo_feat(jn.Rcw1, jn.tcw1, P, 300.0)
    add("x3d_nan", (Scene("", jn, _with(fn, x_dist=np.nan), fb_m), Scene("", jn, fn, fb_m)), "T3: x3D not finite | the same match with a finite keypoint")
    return S


EXPECT = {  # name -> (status, route) of the scene; the twin must differ in the named respect
    "cos_rays_zero": (R.LOW_PARALLAX, R.TRIANGULATED), "cos_rays_9998": (R.LOW_PARALLAX, R.TRIANGULATED),
    "stereo_a_cos": (R.ACCEPTED, R.UNPROJECT_A), "stereo_b_cos": (R.ACCEPTED, R.UNPROJECT_B),
    "stereo_cos_equal": (R.LOW_PARALLAX, R.TRIANGULATED), "w_zero": (R.W_ZERO, R.TRIANGULATED),
    "z1_plus_zero": (R.Z1_NEG, R.UNPROJECT_A), "z1_minus_zero": (R.Z1_NEG, R.UNPROJECT_A),
    "z2_plus_zero": (R.Z2_NEG, R.UNPROJECT_A), "z2_minus_zero": (R.Z2_NEG, R.UNPROJECT_A),
    "reproj1_mono": (R.REPROJ1, R.TRIANGULATED), "reproj2_mono": (R.REPROJ2, R.TRIANGULATED),
    "reproj1_stereo": (R.REPROJ1, R.TRIANGULATED), "reproj2_stereo": (R.REPROJ2, R.TRIANGULATED),
    "dist1_zero": (R.ZERO_DIST, R.TRIANGULATED), "dist2_zero": (R.ZERO_DIST, R.TRIANGULATED),
    "ratio_low": (R.SCALE_RATIO, R.TRIANGULATED), "ratio_high": (R.SCALE_RATIO, R.TRIANGULATED),
    "unproject_depth_zero": (R.Z1_NEG, R.UNPROJECT_A), "x3d_nan": (R.NOT_FINITE, R.UNPROJECT_A),
}

_SCENES = None


def scenes():
    global _SCENES
    if _SCENES is None:
        _SCENES = build()
    return _SCENES


def all_constructed():
    """every constructed scene followed by its twin"""
    out = []
    for s in scenes().values():
        out += [s, s.twin]
    return out


def pack(scene_list, cap):
    """-> (KF a, KF b, jobs, match12 [len, cap]): scene k is feature k of each keyframe and pair k of the call"""
    a, b = kf_of([s.fa for s in scene_list]), kf_of([s.fb for s in scene_list])
    m = np.full((len(scene_list), cap), -1, np.int32)
    for k in range(len(scene_list)):
        m[k, k] = k
    return a, b, [s.job for s in scene_list], m


KINDS = ("mono", "a_stereo", "b_stereo", "both_stereo")
SEEDS = (0, 1, 2)


def random_scene(kind, seed, n=48, noise=0.6, clean=False):
    """a pair of keyframes that see n points: (job, KF a, KF b, match12 over n).  Keyframe b is rotated and displaced; pixel noise makes
    some matches miss a gate, some sizes miss the ratio test, a few depths are off (the stereo routes), a few matches are absent.
    clean: no noise, every feature monocular, well-conditioned rays (the Jacobi check against numpy.linalg.svd)"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + seed)
    ang = rng.uniform(-0.15, 0.15, 3)
    cx_, sx = np.cos(ang[0]), np.sin(ang[0]); cy_, sy = np.cos(ang[1]), np.sin(ang[1]); cz, sz = np.cos(ang[2]), np.sin(ang[2])
    R2 = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy_, 0, sy], [0, 1, 0], [-sy, 0, cy_]]) @ np.array([[1, 0, 0], [0, cx_, -sx], [0, sx, cx_]]))
    C2 = np.array([rng.uniform(0.3, 0.8), rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2)])
    mbf = 250.0
    job = make_job(R2=R2, C2=C2, mb1=mbf / FX, mb2=mbf / FX, mbf1=mbf)
    fa, fb = [], []
    for _ in range(n):
        P = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(2.0, 5.0) if clean else (rng.uniform(30.0, 80.0) if rng.random() < 0.15 else rng.uniform(2.0, 9.0))])
        ns = (lambda: 0.0) if clean else (lambda: rng.normal(0, noise) * (4.0 if rng.random() < 0.15 else 1.0))
        size = lambda: TOL ** int(rng.integers(0, 4)) if not clean else 1.0
        sa = kind in ("a_stereo", "both_stereo") and not clean and rng.random() < 0.8
        sb = kind in ("b_stereo", "both_stereo") and not clean and rng.random() < 0.8
        for feats, Rc, tc, st in ((fa, job.Rcw1, job.tcw1, sa), (fb, job.Rcw2, job.tcw2, sb)):
            u, v, z = project(Rc, tc, P)
            sg = f32(TOL ** int(rng.integers(0, 3))) ** 2 if not clean else 1.0
            if st:
                zn = z * (rng.uniform(0.5, 1.5) if rng.random() < 0.2 else 1.0 + rng.normal(0, 0.01))
                f = feat(u + ns(), v + ns(), sigma2=sg, size=size(), u_right=u - mbf / z + ns(), depth=zn, x_dist=u + rng.normal(0, 0.3), y_dist=v + rng.normal(0, 0.3))
            else:
                f = feat(u + ns(), v + ns(), sigma2=sg, size=size())
            feats.append(f)
    m = np.arange(n, dtype=np.int32)
    if not clean:
        perm = rng.permutation(n)
        fb = [fb[k] for k in perm]
        inv = np.empty(n, np.int32); inv[perm] = np.arange(n, dtype=np.int32)
        m = inv
        m[rng.random(n) < 0.1] = -1
    return job, kf_of(fa), kf_of(fb), m


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]], np.float64)


class World:
    """a current keyframe and nn neighbours that see the same n points: what CreateNewMapPoints gets from its caller.  kfs[0] is the current
    keyframe; desc[k] the descriptor rows of keyframe k (uint8 [n, desc_bytes] or float32 [n, float_dim]); jobs[k - 1], F12[k - 1],
    epipoles[k - 1] belong to the pair (0, k) (ComputeF12, LocalMapping.cc:474-494, and the epipole of FeatureMatcher.cc:669-677, made in
    float64 and handed over as float32: inputs, not results under test); cams[k]: what DescriptorTable.tri_points_jobs takes"""

    def __init__(self, seed, nn=3, n=40, desc_bytes=32, float_dim=0):
        rng = np.random.default_rng(7000 + seed)
        self.n, self.nn, self.desc_bytes, self.float_dim = n, nn, desc_bytes, float_dim
        Pw = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1, 1, n), rng.uniform(2.5, 8, n)], 1)
        poses = [(np.eye(3), np.zeros(3))]
        for k in range(nn):
            a = rng.uniform(-0.1, 0.1)
            Rk = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
            poses.append((Rk, np.array([0.4 + 0.3 * k, rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])))
        if float_dim:
            base = rng.normal(0, 1, (n, float_dim)).astype(np.float32)
        else:
            base = rng.integers(0, 256, (n, desc_bytes), dtype=np.uint8)
        self.kfs, self.desc, self.cams = [], [], []
        K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1]], np.float64)
        for k, (Rk, Ck) in enumerate(poses):
            tk = (-Rk @ Ck).astype(np.float32)
            Rk32 = Rk.astype(np.float32)
            feats = []
            for i in range(n):
                u, v, _ = project(Rk32, tk, Pw[i])
                feats.append(feat(u + rng.normal(0, 0.3), v + rng.normal(0, 0.3), sigma2=1.0, size=TOL ** int(rng.integers(0, 2))))
            self.kfs.append(kf_of(feats))
            if float_dim:
                self.desc.append((base + rng.normal(0, 0.02, base.shape)).astype(np.float32))
            else:
                d = base.copy()
                flip = rng.integers(0, desc_bytes, n)
                d[np.arange(n), flip] ^= np.uint8(1) << rng.integers(0, 8, n).astype(np.uint8)
                self.desc.append(d)
            self.cams.append({"Rcw": Rk32.reshape(9), "tcw": tk, "Ow": twc(Rk32, tk), "fx": f32(FX), "fy": f32(FY), "cx": f32(CX), "cy": f32(CY),
                              "invfx": f32(1) / f32(FX), "invfy": f32(1) / f32(FY), "mb": f32(0.1), "mbf": f32(50.0)})
        self.cams[0]["ratio_factor"] = f32(1.5) * f32(TOL)
        self.cams[0]["max_size"] = f32(TOL) ** 7
        self.jobs, self.F12, self.epipoles = [], [], []
        R1, t1 = poses[0][0], np.zeros(3)
        for k in range(1, nn + 1):
            c0, ck = self.cams[0], self.cams[k]
            self.jobs.append(R.Job(c0["Rcw"], c0["tcw"], c0["Ow"], ck["Rcw"], ck["tcw"], ck["Ow"], fx1=FX, fy1=FY, cx1=CX, cy1=CY, invfx1=c0["invfx"],
                                   invfy1=c0["invfy"], fx2=FX, fy2=FY, cx2=CX, cy2=CY, invfx2=ck["invfx"], invfy2=ck["invfy"], mb1=c0["mb"], mb2=ck["mb"],
                                   mbf1=c0["mbf"], ratio_factor=c0["ratio_factor"], max_size1=c0["max_size"]))
            R2, t2 = poses[k][0], -poses[k][0] @ poses[k][1]
            R12 = R1 @ R2.T
            t12 = -R12 @ t2 + t1
            self.F12.append((np.linalg.inv(K).T @ _skew(t12) @ R12 @ np.linalg.inv(K)).astype(np.float32).reshape(9))
            c2 = R2 @ poses[0][1] + t2
            self.epipoles.append(np.array([FX * c2[0] / c2[2] + CX, FY * c2[1] / c2[2] + CY], np.float32))

    def search(self, th_low):
        """the SearchForTriangulation of the restatement for create_new_map_points (brute force: no vocabulary)"""
        import _bow_ref as B

        def run(k, has_cur, has_nb):
            a, b = self.kfs[0], self.kfs[k + 1]
            out, _, _ = B.search_for_triangulation(self.desc[0], self.desc[k + 1], np.stack([a.x, a.y], 1), np.stack([b.x, b.y], 1), b.sigma2,
                                                   self.F12[k], self.epipoles[k], has_mp1=has_cur, has_mp2=has_nb, th_low=th_low)
            return out
        return run
