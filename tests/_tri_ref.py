"""Plain-Python restatement of the per-match body of LocalMapping::CreateNewMapPoints.  TEST INFRASTRUCTURE ONLY.

This file is the NORMATIVE semantics of k_tri_points / k_tri_store (afv_table_triangulate, include/afv_hip.h): the device is held to it
bit for bit.  It follows tests/_points_ref.py: np.float32 scalars, one operation per statement, no fused multiply-add.  Parity with a build
of the reference is unpinned: the reference is built -O3 -march=native and links an OpenCV that is not part of this project.

Restated from the reference's source:

  the body of the match loop      LocalMapping.cc:315-461   triangulate_match
  KeyFrame::UnprojectStereo       KeyFrame.cc:659-675       unproject_stereo
  MapPoint::MapPoint + UpdateNormalAndDepth for a point with these two observations, the current keyframe as reference
                                  MapPoint.cc:372-418       new_point
  cv::SVD::compute on a 4 x 4 CV_32F matrix, vt.row(3)      jacobi_null_vector, after OpenCV 4.x's JacobiSVDImpl_<float> as published
                                  (modules/core/src/lapack.cpp) - PARITY UNPINNED: OpenCV is not available to this project
  the neighbour loop              LocalMapping.cc:265-472   create_new_map_points (with _bow_ref.search_for_triangulation)

Conventions, written down once more (they are those of tests/_points_ref.py):
  * every float operator rounds once; a * b + c is two roundings
  * a three-term sum (a dot product, a squared norm, a row of a 3 x 3 matrix times a vector) is a0 + (a1 + a2)   (SUM_ORDER)
  * a norm is sqrt of that sum; fx * x * invz + cx is ((fx * x) * invz) + cx as written; err2 is (ex * ex + ey * ey) [+ er * er]
  * Rwc * v is the transposed access of Rcw: component k = sum3(Rcw[0][k] * v0, Rcw[1][k] * v1, Rcw[2][k] * v2)
  * Twc's translation is Ow as the host computed it (the job record carries it)
  * x3D = vt.row(3)[0..2] / vt.row(3)[3] is a float division per component
  * comparisons the reference evaluates in double are evaluated in double: err2 > 5.991 * sigma2, err2 > 7.8 * sigma2 (double products of
    the double literal and the promoted float) and cosParallaxRays < 0.9998 (the float promoted against the double literal)

The Jacobi (one-sided, on the rows of At = A^T, i.e. the columns of A): W[i] = sum of squares of row i in double; at most 30 sweeps over the
pairs (i, j), i < j; p = sum of products in double; skipped when |p| <= eps * sqrt(a * b) with eps = 2 * FLT_EPSILON (a float, promoted);
p *= 2, beta = a - b, gamma = hypot(p, beta); beta < 0: s = (float)sqrt((gamma - beta) * 0.5 / gamma), c = (float)(p / (gamma * s * 2));
else c = (float)sqrt((gamma + beta) / (gamma * 2)), s = (float)(p / (gamma * c * 2)); rows rotated in float (t0 = c * ai + s * aj,
t1 = -s * ai + c * aj), their norms re-accumulated in double; Vt rotated the same way; afterwards W[i] = sqrt(sum of squares) in double and
a selection sort, descending, strict (W[j] < W[k]), that swaps the rows of Vt along.  vt.row(3) is row 3 after the sort.

Two quirks of the reference, restated as written:
  Q1  the stereo reprojection gate of the SECOND keyframe uses the CURRENT keyframe's mbf (:438)
  Q2  UnprojectStereo reads the DISTORTED keypoint mvKeys[i].pt (KeyFrame.cc:664-665)

Three deliberate deviations:
  T1  cos(2 * atan2(mb / 2, depth)) is (d * d - h * h) / (d * d + h * h) in float, h = mb / 2: no library cos / atan2 (the reference's value
      depends on its libm)
  T2  the rotation's hypot(p, beta) is sqrt(p * p + beta * beta) in double, correctly rounded
  T3  a match whose x3D has a component that is not finite is rejected (in the reference every comparison against a NaN is false: the
      point would pass every gate and enter the map).  It is tested as soon as x3D exists.

Outputs per match: status, route, x3D (zeros where no x3D was made: no match, low parallax, w == 0).
"""
import numpy as np

from _points_ref import OBSERVED, SET, SUM_ORDER

assert SUM_ORDER == "a0+(a1+a2)"
f32 = np.float32
f64 = np.float64

NO_MATCH, ACCEPTED, LOW_PARALLAX, W_ZERO, Z1_NEG, Z2_NEG, REPROJ1, REPROJ2, ZERO_DIST, SCALE_RATIO, NOT_FINITE = range(11)
STATUS_NAMES = ("no_match", "accepted", "low_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "zero_dist", "scale_ratio", "not_finite")
TRIANGULATED, UNPROJECT_A, UNPROJECT_B = 0, 1, 2
JACOBI_EPS = f32(np.finfo(np.float32).eps * 2)   # FLT_EPSILON * 2
JACOBI_SWEEPS = 30                               # max(m, 30), m = 4


def sum3(a0, a1, a2):
    return a0 + (a1 + a2)


class KF:
    """what the table holds per feature of a keyframe slot: geometry planes (x, y, sigma2, u_right) and scale planes (size, depth, x_dist,
    y_dist); depth None = -1 everywhere, x_dist / y_dist None = the undistorted points (afv_table_set_scale)"""

    def __init__(self, x, y, sigma2, size, u_right=None, depth=None, x_dist=None, y_dist=None):
        a = lambda v: np.ascontiguousarray(v, np.float32).reshape(-1)
        self.x, self.y, self.sigma2, self.size = a(x), a(y), a(sigma2), a(size)
        n = len(self.x)
        self.n = n
        self.u_right = np.full(n, -1, np.float32) if u_right is None else a(u_right)
        self.depth = np.full(n, -1, np.float32) if depth is None else a(depth)
        self.x_dist = self.x.copy() if x_dist is None else a(x_dist)
        self.y_dist = self.y.copy() if y_dist is None else a(y_dist)


class Job:
    """afv_tri_points_job: poses (Rcw row-major, tcw, Ow as the host computes GetCameraCenter), intrinsics, mb of a and b, mbf of a,
    ratio_factor = 1.5f * sizeTolerance, max_size1 = maxKeyPtSize of a"""
    FIELDS = ("fx1", "fy1", "cx1", "cy1", "invfx1", "invfy1", "fx2", "fy2", "cx2", "cy2", "invfx2", "invfy2", "mb1", "mb2", "mbf1",
              "ratio_factor", "max_size1")

    def __init__(self, Rcw1, tcw1, Ow1, Rcw2, tcw2, Ow2, **kw):
        v = lambda a, n: np.ascontiguousarray(a, np.float32).reshape(n)
        self.Rcw1, self.tcw1, self.Ow1 = v(Rcw1, 9), v(tcw1, 3), v(Ow1, 3)
        self.Rcw2, self.tcw2, self.Ow2 = v(Rcw2, 9), v(tcw2, 3), v(Ow2, 3)
        for k in self.FIELDS:
            setattr(self, k, f32(kw.pop(k)))
        assert not kw, kw


def jacobi_null_vector(A):
    """A: 4 x 4 float32.  -> (vt row 3 as 4 float32, sweeps run).  See the module text."""
    n = 4
    At = [[f32(A[k][i]) for k in range(n)] for i in range(n)]       # transpose(src, temp_a)
    Vt = [[f32(1.0) if i == k else f32(0.0) for k in range(n)] for i in range(n)]
    W = []
    for i in range(n):
        sd = f64(0.0)
        for k in range(n):
            t = f64(At[i][k])
            sd = sd + t * t
        W.append(sd)
    sweeps = 0
    for _ in range(JACOBI_SWEEPS):
        sweeps += 1
        changed = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                Ai, Aj = At[i], At[j]
                a, b = W[i], W[j]
                p = f64(0.0)
                for k in range(n):
                    p = p + f64(Ai[k]) * f64(Aj[k])
                if abs(p) <= f64(JACOBI_EPS) * np.sqrt(a * b):
                    continue
                p = p * f64(2.0)
                beta = a - b
                gamma = np.sqrt(p * p + beta * beta)               # T2
                if beta < 0:
                    delta = (gamma - beta) * f64(0.5)
                    s = f32(np.sqrt(delta / gamma))
                    c = f32(p / (gamma * f64(s) * f64(2.0)))
                else:
                    c = f32(np.sqrt((gamma + beta) / (gamma * f64(2.0))))
                    s = f32(p / (gamma * f64(c) * f64(2.0)))
                a = f64(0.0)
                b = f64(0.0)
                ms = -s
                for k in range(n):
                    t0 = c * Ai[k] + s * Aj[k]
                    t1 = ms * Ai[k] + c * Aj[k]
                    Ai[k], Aj[k] = t0, t1
                    a = a + f64(t0) * f64(t0)
                    b = b + f64(t1) * f64(t1)
                W[i], W[j] = a, b
                changed = True
                Vi, Vj = Vt[i], Vt[j]
                for k in range(n):
                    t0 = c * Vi[k] + s * Vj[k]
                    t1 = ms * Vi[k] + c * Vj[k]
                    Vi[k], Vj[k] = t0, t1
        if not changed:
            break
    for i in range(n):
        sd = f64(0.0)
        for k in range(n):
            t = f64(At[i][k])
            sd = sd + t * t
        W[i] = np.sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    return np.array(Vt[3], np.float32), sweeps


def triangulation_matrix(job, xn1, xn2):
    """A (:352-355): row = xn(k) * Tcw.row(2) - Tcw.row(k), Tcw = [Rcw | tcw]"""
    A = np.zeros((4, 4), np.float32)
    for r, (xn, R, t) in enumerate(((xn1[0], job.Rcw1, job.tcw1), (xn1[1], job.Rcw1, job.tcw1), (xn2[0], job.Rcw2, job.tcw2),
                                    (xn2[1], job.Rcw2, job.tcw2))):
        k = r & 1
        for col in range(4):
            t2 = f32(R[6 + col]) if col < 3 else f32(t[2])
            tk = f32(R[3 * k + col]) if col < 3 else f32(t[k])
            A[r, col] = xn * t2 - tk
    return A


def _rays(job, a, i, b, j):
    xn1 = (f32(a.x[i]) - job.cx1) * job.invfx1, (f32(a.y[i]) - job.cy1) * job.invfy1, f32(1.0)
    xn2 = (f32(b.x[j]) - job.cx2) * job.invfx2, (f32(b.y[j]) - job.cy2) * job.invfy2, f32(1.0)
    R1, R2 = job.Rcw1, job.Rcw2
    ray1 = [sum3(f32(R1[k]) * xn1[0], f32(R1[3 + k]) * xn1[1], f32(R1[6 + k]) * xn1[2]) for k in range(3)]
    ray2 = [sum3(f32(R2[k]) * xn2[0], f32(R2[3 + k]) * xn2[1], f32(R2[6 + k]) * xn2[2]) for k in range(3)]
    return xn1, xn2, ray1, ray2


def cos_parallax_rays(job, a, i, b, j):
    _, _, r1, r2 = _rays(job, a, i, b, j)
    dot = sum3(r1[0] * r2[0], r1[1] * r2[1], r1[2] * r2[2])
    n1 = np.sqrt(sum3(r1[0] * r1[0], r1[1] * r1[1], r1[2] * r1[2]))
    n2 = np.sqrt(sum3(r2[0] * r2[0], r2[1] * r2[1], r2[2] * r2[2]))
    return dot / (n1 * n2)


def cos_stereo(mb, depth):
    """T1"""
    h = f32(mb) / f32(2.0)
    d = f32(depth)
    dd = d * d
    hh = h * h
    return (dd - hh) / (dd + hh)


def unproject_stereo(kf, i, cx, cy, invfx, invfy, Rcw, Ow):
    z = f32(kf.depth[i])
    if not z > 0:
        return [f32(0.0), f32(0.0), f32(-1.0)]
    u, v = f32(kf.x_dist[i]), f32(kf.y_dist[i])          # Q2
    x = ((u - cx) * z) * invfx
    y = ((v - cy) * z) * invfy
    return [sum3(f32(Rcw[k]) * x, f32(Rcw[3 + k]) * y, f32(Rcw[6 + k]) * z) + f32(Ow[k]) for k in range(3)]


def _cam(R, t, X, row):
    return sum3(f32(R[3 * row]) * X[0], f32(R[3 * row + 1]) * X[1], f32(R[3 * row + 2]) * X[2]) + f32(t[row])


def _reproj_fails(fx, fy, cx, cy, mbf, x, y, invz, kx, ky, kur, stereo, sigma2):
    u = (fx * x) * invz + cx
    v = (fy * y) * invz + cy
    ex = u - kx
    ey = v - ky
    e2 = ex * ex + ey * ey
    if not stereo:
        return bool(float(e2) > 5.991 * float(sigma2))
    u_r = u - mbf * invz
    er = u_r - kur
    e2 = e2 + er * er
    return bool(float(e2) > 7.8 * float(sigma2))


def triangulate_match(job, a, i, b, j):
    """-> (status, route, x3D as 3 float32)"""
    zero = np.zeros(3, np.float32)
    if j < 0:
        return NO_MATCH, TRIANGULATED, zero
    with np.errstate(all="ignore"):
        ur1, ur2 = f32(a.u_right[i]), f32(b.u_right[j])
        st1, st2 = bool(ur1 >= 0), bool(ur2 >= 0)
        xn1, xn2, r1, r2 = _rays(job, a, i, b, j)
        cos_rays = cos_parallax_rays(job, a, i, b, j)
        cs = cos_rays + f32(1.0)
        cs1 = cs2 = cs
        if st1:
            cs1 = cos_stereo(job.mb1, a.depth[i])
        elif st2:
            cs2 = cos_stereo(job.mb2, b.depth[j])
        cs = cs2 if cs2 < cs1 else cs1                    # std::min(cs1, cs2)
        route = TRIANGULATED
        if cos_rays < cs and cos_rays > 0 and (st1 or st2 or float(cos_rays) < 0.9998):
            v, _ = jacobi_null_vector(triangulation_matrix(job, xn1, xn2))
            if v[3] == 0:
                return W_ZERO, TRIANGULATED, zero
            X = [v[0] / v[3], v[1] / v[3], v[2] / v[3]]
        elif st1 and cs1 < cs2:
            route = UNPROJECT_A
            X = unproject_stereo(a, i, job.cx1, job.cy1, job.invfx1, job.invfy1, job.Rcw1, job.Ow1)
        elif st2 and cs2 < cs1:
            route = UNPROJECT_B
            X = unproject_stereo(b, j, job.cx2, job.cy2, job.invfx2, job.invfy2, job.Rcw2, job.Ow2)
        else:
            return LOW_PARALLAX, TRIANGULATED, zero
        x3d = np.array(X, np.float32)
        if not np.all(np.isfinite(x3d)):                  # T3
            return NOT_FINITE, route, x3d
        z1 = _cam(job.Rcw1, job.tcw1, X, 2)
        if z1 <= 0:
            return Z1_NEG, route, x3d
        z2 = _cam(job.Rcw2, job.tcw2, X, 2)
        if z2 <= 0:
            return Z2_NEG, route, x3d
        x1, y1 = _cam(job.Rcw1, job.tcw1, X, 0), _cam(job.Rcw1, job.tcw1, X, 1)
        invz1 = f32(1.0) / z1
        if _reproj_fails(job.fx1, job.fy1, job.cx1, job.cy1, job.mbf1, x1, y1, invz1, f32(a.x[i]), f32(a.y[i]), ur1, st1, f32(a.sigma2[i])):
            return REPROJ1, route, x3d
        x2, y2 = _cam(job.Rcw2, job.tcw2, X, 0), _cam(job.Rcw2, job.tcw2, X, 1)
        invz2 = f32(1.0) / z2
        if _reproj_fails(job.fx2, job.fy2, job.cx2, job.cy2, job.mbf1, x2, y2, invz2, f32(b.x[j]), f32(b.y[j]), ur2, st2, f32(b.sigma2[j])):   # Q1
            return REPROJ2, route, x3d
        d1 = _dist(X, job.Ow1)
        d2 = _dist(X, job.Ow2)
        if d1 == 0 or d2 == 0:
            return ZERO_DIST, route, x3d
        ratio_dist = d2 / d1
        ratio_octave = f32(a.size[i]) / f32(b.size[j])
        if ratio_dist * job.ratio_factor < ratio_octave or ratio_dist > ratio_octave * job.ratio_factor:
            return SCALE_RATIO, route, x3d
        return ACCEPTED, route, x3d


def _dist(X, O):
    n = [X[k] - f32(O[k]) for k in range(3)]
    return np.sqrt(sum3(n[0] * n[0], n[1] * n[1], n[2] * n[2]))


def new_point(job, a, i, x3d):
    """the fields of the store for an accepted match: dict of pos, normal, min_distance, max_distance, ref_size, ref_distance, ref_sigma,
    flags (MapPoint.cc:372-418; the sum over the two observations starts from zero, :390-397)"""
    with np.errstate(all="ignore"):
        X = [f32(v) for v in x3d]
        n1 = [X[k] - f32(job.Ow1[k]) for k in range(3)]
        n2 = [X[k] - f32(job.Ow2[k]) for k in range(3)]
        d1 = np.sqrt(sum3(n1[0] * n1[0], n1[1] * n1[1], n1[2] * n1[2]))
        d2 = np.sqrt(sum3(n2[0] * n2[0], n2[1] * n2[1], n2[2] * n2[2]))
        normal = [((f32(0.0) + n1[k] / d1) + n2[k] / d2) / f32(2.0) for k in range(3)]
        size = f32(a.size[i])
        max_d = d1 * size
        return {"pos": np.array(X, np.float32), "normal": np.array(normal, np.float32), "ref_distance": d1, "ref_size": size,
                "ref_sigma": np.sqrt(f32(a.sigma2[i])), "max_distance": max_d, "min_distance": max_d / job.max_size1,
                "flags": np.uint8(SET | OBSERVED)}


def triangulate(jobs, kfs_a, kfs_b, match12, first_id=0):
    """afv_table_triangulate: pairs p with keyframes kfs_a[p], kfs_b[p], match12[p] over the cap of the table.
    -> status [P, cap] u8, route [P, cap] u8, x3d [P, cap, 3] f32, new_id [P, cap] i32, n_new [P] i32, points: list of (id, p, i, fields)"""
    match12 = np.asarray(match12, np.int32)
    P, cap = match12.shape
    status = np.zeros((P, cap), np.uint8)
    route = np.zeros((P, cap), np.uint8)
    x3d = np.zeros((P, cap, 3), np.float32)
    new_id = np.full((P, cap), -1, np.int32)
    n_new = np.zeros(P, np.int32)
    points = []
    nid = int(first_id)
    for p in range(P):
        for i in range(kfs_a[p].n):
            s, r, X = triangulate_match(jobs[p], kfs_a[p], i, kfs_b[p], int(match12[p, i]))
            status[p, i], route[p, i], x3d[p, i] = s, r, X
            if s == ACCEPTED:
                new_id[p, i] = nid
                points.append((nid, p, i, new_point(jobs[p], kfs_a[p], i, X)))
                nid += 1
                n_new[p] += 1
    return status, route, x3d, new_id, n_new, points


def create_new_map_points(cur, neighbours, jobs, search, has_mp_cur, has_mp_nb, first_id=0):
    """the neighbour loop (:265-472): per neighbour one SearchForTriangulation (search(k, has_mp_cur, has_mp_nb[k]) -> match12 over cur's
    features) and the triangulation of its matches; the features of cur and of that neighbour that received a point are marked in the
    masks before the next neighbour.  -> list of (id, k, i, j, fields)"""
    has_mp_cur = np.array(has_mp_cur, np.uint8)
    has_mp_nb = [np.array(m, np.uint8) for m in has_mp_nb]
    out = []
    nid = int(first_id)
    for k, nb in enumerate(neighbours):
        m = np.asarray(search(k, has_mp_cur, has_mp_nb[k]), np.int32)
        for i in range(cur.n):
            j = int(m[i])
            s, _, X = triangulate_match(jobs[k], cur, i, nb, j)
            if s == ACCEPTED:
                out.append((nid, k, i, j, new_point(jobs[k], cur, i, X)))
                nid += 1
                has_mp_cur[i] = 1
                has_mp_nb[k][j] = 1
    return out
