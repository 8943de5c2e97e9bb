"""Plain-Python restatement of Sim3Solver (src/Sim3Solver.cc:38-411).  TEST INFRASTRUCTURE ONLY.

This file is the NORMATIVE semantics of k_sim3_gather / k_sim3_hypotheses (afv_table_sim3_hypotheses, include/afv_hip.h) and of the host
scan of the adapters (Sim3Solver.iterate): the device is held to it bit for bit.  It follows tests/_tri_ref.py: np.float32 scalars, one
operation per statement, no fused multiply-add.  Parity with a build of the reference is unpinned: the reference is built -O3
-march=native and links an Eigen and an OpenCV that are not part of this project.

Restated from the reference's source:

  the constructor                 Sim3Solver.cc:38-110      gather
  SetRansacParameters             :112-136                  Solver.SetRansacParameters
  iterate / find                  :138-210                  Solver.iterate / Solver.find
  ComputeCentroid, ComputeSim3    :212-325                  centroid, compute_sim3
  CheckInliers, Project           :328-391                  check_inliers, project
  FromCameraToImage               :393-411                  (in gather)

Conventions (those of tests/_tri_ref.py):
  * every float operator rounds once; a * b + c is two roundings
  * a three-term sum (a row of a 3 x 3 matrix times a vector or a matrix, a row sum) is a0 + (a1 + a2)   (SUM_ORDER)
  * scalar expressions are evaluated left to right as written: M00 + M11 + M22 is (M00 + M11) + M22; fx * x + cx is (fx * x) + cx
  * double where the reference accumulates in double: cv::Mat::dot (nom; err1 and err2: both products and their sum in double, the result
    rounded to float), den (a double sum of the float squares), s12i = (float)(nom / den); nom and den run over the 3 x 3 in row-major order
  * C / P.cols() is a float division by 3.0f; s12i * R12i * O2 is (s12i * R12i) * O2: the matrix sR that T12 takes

Quirks restated as written:
  Q1  mvnMaxError1/2 are vector<size_t> (include/Sim3Solver.h:79-80): the bound is (size_t)(9.210 * sigmaSquare), the product in double,
      truncated, and err < bound compares in float (the integer converted to float)
  Q2  the best hypothesis is updated on mnInliersi >= mnBestInliers, iterate returns on mnInliersi > mRansacMinInliers (strict)
  Q3  SetRansacParameters: epsilon in float, ceil(log(1 - p) / log(1 - pow(epsilon, 3))) in double, max(1, min(nIterations,
      maxIterations)); host mathematics only

Deliberate deviations:
  S1  the reference assigns N(0..2,3) from row 3, which was never written (:254-256); here N is Horn's symmetric matrix:
      N(3,0..2) = N(0..2,3) as computed at :242, :247, :252
  S2  the eigenvector of the largest eigenvalue comes from a cyclic Jacobi on the symmetric 4 x 4 in double: pairs (0,1) (0,2) (0,3)
      (1,2) (1,3) (2,3); only + - * / and sqrt; at most JACOBI_SWEEPS = 12 sweeps, a pair is skipped when a_pq == 0 or |a_pp| + |a_pq| ==
      |a_pp| and |a_qq| + |a_pq| == |a_qq|, a sweep that rotates nothing ends it; ties on the maximum go to the lowest index.  It
      replaces Eigen::EigenSolver.  The rotation: theta = (a_qq - a_pp) / (2 a_pq), t = 1 / (|theta| + sqrt(theta theta + 1)) with the
      sign of theta, c = 1 / sqrt(t t + 1), s = t c; a_kp' = c a_kp - s a_kq, a_kq' = s a_kp + c a_kq (k other than p, q, mirrored),
      a_pp' = a_pp - t a_pq, a_qq' = a_qq + t a_pq, a_pq' = 0; the columns p, q of V turn the same way
  S3  R12 is built directly from the normalised quaternion (w, x, y, z) = column / sqrt(w w + x x + y y + z z), in double, then rounded
      to float; it replaces atan2 + cv::Rodrigues: the same mathematics, no libm, insensitive to the eigenvector's sign
  S4  draws come from the counter-based generator of the vocabulary trainer (sm = splitmix64 and DRAW_STEP of tests/_voctrain_ref.py):
      key_h = sm(sm(seed) ^ (h + 1)), draw d in {0, 1, 2} = sm(key_h + (d + 1) * DRAW_STEP) % (N - d), applied to vAvailableIndices with
      the reference's swap-with-back removal (:166-173)
  S5  a hypothesis is degenerate if den (when the scale is estimated), s12i, R12 or t12 is not finite, or den == 0: it counts 0
      inliers, is flagged, and its sim3 record and inlier words read 0.  A correspondence whose error is not finite is not an inlier
      (the comparisons as written).  A sigma2 that is negative or not finite gives bound 0
  S6  N < 3 evaluates no hypothesis: all counts 0, no flag (callers reach bNoMore first: min_inliers >= 3 is required)
"""
import math

import numpy as np

from _points_ref import SUM_ORDER
from _voctrain_ref import DRAW_STEP, M64, sm

assert SUM_ORDER == "a0+(a1+a2)"
f32 = np.float32
f64 = np.float64
SET, BAD = 1, 2
JACOBI_SWEEPS = 12
JACOBI_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def sum3(a0, a1, a2):
    return a0 + (a1 + a2)


def finite(v):
    return bool(np.isfinite(v))


class Cam:
    """one keyframe of a job: Rcw row-major, tcw, the intrinsics"""

    def __init__(self, Rcw, tcw, fx, fy, cx, cy):
        self.Rcw = np.ascontiguousarray(Rcw, np.float32).reshape(9)
        self.tcw = np.ascontiguousarray(tcw, np.float32).reshape(3)
        self.fx, self.fy, self.cx, self.cy = f32(fx), f32(fy), f32(cx), f32(cy)


def rigid(R, t, X):
    """R * X + t, R row-major 9 floats"""
    return [sum3(f32(R[3 * r]) * X[0], f32(R[3 * r + 1]) * X[1], f32(R[3 * r + 2]) * X[2]) + f32(t[r]) for r in range(3)]


def to_image(cam, P):
    """FromCameraToImage (:393-411) / the tail of Project (:385-389)"""
    invz = f32(1.0) / P[2]
    x = P[0] * invz
    y = P[1] * invz
    return [cam.fx * x + cam.cx, cam.fy * y + cam.cy]


def max_error(sigma2):
    """Q1 / S5: (size_t)(9.210 * sigmaSquare) as the float the comparison converts it to"""
    s = f32(sigma2)
    if not finite(s) or not s >= 0:
        return f32(0.0)
    with np.errstate(over="ignore"):
        return f32(np.trunc(f64(9.210) * f64(s)))


def gather(cam1, cam2, pos, flags, sigma2_1, sigma2_2, mp1, mp2, idx1, idx2, n1):
    """the constructor (:38-110).  pos [P][3] float32 and flags [P] (SET | BAD) are the store; sigma2_1 / sigma2_2 the tables' planes of the
    two slots; mp1 / mp2 / idx1 / idx2 rows over i1 (idx1 None: i1).  -> dict(n, index1, x1, x2, im1, im2, max_err)"""
    out = dict(index1=[], x1=[], x2=[], im1=[], im2=[], max_err=[])
    with np.errstate(all="ignore"):
        for i1 in range(n1):
            p2 = int(mp2[i1])
            if p2 < 0:
                continue
            p1 = int(mp1[i1])
            if p1 < 0:
                continue
            bad1 = not (int(flags[p1]) & SET) or bool(int(flags[p1]) & BAD)
            bad2 = not (int(flags[p2]) & SET) or bool(int(flags[p2]) & BAD)
            if bad1 or bad2:
                continue
            k1 = i1 if idx1 is None else int(idx1[i1])
            k2 = int(idx2[i1])
            if k1 < 0 or k2 < 0:
                continue
            out["max_err"].append([max_error(sigma2_1[k1]), max_error(sigma2_2[k2])])
            out["index1"].append(i1)
            X1 = rigid(cam1.Rcw, cam1.tcw, [f32(v) for v in pos[p1]])
            X2 = rigid(cam2.Rcw, cam2.tcw, [f32(v) for v in pos[p2]])
            out["x1"].append(X1)
            out["x2"].append(X2)
            out["im1"].append(to_image(cam1, X1))
            out["im2"].append(to_image(cam2, X2))
    out["n"] = len(out["index1"])
    return out


def draws(seed, h, N):
    """S4: the three raw draws of hypothesis h"""
    key = sm(sm(seed & M64) ^ (h + 1))
    return [sm((key + (d + 1) * DRAW_STEP) & M64) % (N - d) for d in range(3)]


def sample3(seed, h, N):
    """S4 on vAvailableIndices (:161-174), literally: the list, the pick, the swap with the back, the pop"""
    avail = list(range(N))
    picks = []
    for r in draws(seed, h, N):
        picks.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return picks


def sample3_closed(seed, h, N):
    """the same three indices without the list (what the kernel computes)"""
    r0, r1, r2 = draws(seed, h, N)
    i0 = r0
    i1 = N - 1 if r1 == r0 else r1
    back1 = N - 1 if N - 2 == r0 else N - 2
    i2 = back1 if r2 == r1 else (N - 1 if r2 == r0 else r2)
    return [i0, i1, i2]


def centroid(P):
    """ComputeCentroid (:212-218): P[r][i] = component r of point i -> (Pr, C)"""
    C = [sum3(P[r][0], P[r][1], P[r][2]) / f32(3.0) for r in range(3)]
    return [[P[r][i] - C[r] for i in range(3)] for r in range(3)], C


def horn_matrix(M):
    """Step 3 with S1: the symmetric N as 4 x 4 float32"""
    n00 = M[0][0] + M[1][1] + M[2][2]
    n01 = M[1][2] - M[2][1]
    n02 = M[2][0] - M[0][2]
    n03 = M[0][1] - M[1][0]
    n11 = M[0][0] - M[1][1] - M[2][2]
    n12 = M[0][1] + M[1][0]
    n13 = M[2][0] + M[0][2]
    n22 = -M[0][0] + M[1][1] - M[2][2]
    n23 = M[1][2] + M[2][1]
    n33 = -M[0][0] - M[1][1] + M[2][2]
    return [[n00, n01, n02, n03], [n01, n11, n12, n13], [n02, n12, n22, n23], [n03, n13, n23, n33]]


def jacobi_max_eigenvector(Nm):
    """S2.  Nm: symmetric 4 x 4 (any float type).  -> ((w, x, y, z) as float64, sweeps that rotated, the eigenvalue)"""
    a = [[f64(Nm[r][c]) for c in range(4)] for r in range(4)]
    v = [[f64(1.0) if r == c else f64(0.0) for c in range(4)] for r in range(4)]
    sweeps = 0
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for p, q in JACOBI_PAIRS:
            apq, app, aqq = a[p][q], a[p][p], a[q][q]
            if apq == 0:
                continue
            g = abs(apq)
            if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                continue
            theta = (aqq - app) / (f64(2.0) * apq)
            t = f64(1.0) / (abs(theta) + np.sqrt(theta * theta + f64(1.0)))
            if theta < 0:
                t = -t
            c = f64(1.0) / np.sqrt(t * t + f64(1.0))
            s = t * c
            for k in range(4):
                if k == p or k == q:
                    continue
                akp, akq = a[k][p], a[k][q]
                np_ = c * akp - s * akq
                nq_ = s * akp + c * akq
                a[k][p] = a[p][k] = np_
                a[k][q] = a[q][k] = nq_
            a[p][p] = app - t * apq
            a[q][q] = aqq + t * apq
            a[p][q] = a[q][p] = f64(0.0)
            for k in range(4):
                vkp, vkq = v[k][p], v[k][q]
                v[k][p] = c * vkp - s * vkq
                v[k][q] = s * vkp + c * vkq
            rotated = True
        if not rotated:
            break
        sweeps += 1
    best = 0
    for k in range(1, 4):
        if a[k][k] > a[best][best]:
            best = k
    return [v[r][best] for r in range(4)], sweeps, a[best][best]


def quaternion_rotation(q):
    """S3: the rotation of the normalised quaternion, 9 float64 row-major (before the rounding to float)"""
    q0, q1, q2, q3 = q
    nrm = np.sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3)
    w, x, y, z = q0 / nrm, q1 / nrm, q2 / nrm, q3 / nrm
    one, two = f64(1.0), f64(2.0)
    return [one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y),
            two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x),
            two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]


def compute_sim3(P1, P2, fix_scale):
    """ComputeSim3 (:220-325).  P1 / P2 [r][i] float32.  -> dict(ok, R, t, s, sR, sRi, ti, N, sweeps): R12i, t12i, s12i, the blocks of
    T12i and T21i; ok False = degenerate (S5)"""
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = [[sum3(Pr2[r][0] * Pr1[c][0], Pr2[r][1] * Pr1[c][1], Pr2[r][2] * Pr1[c][2]) for c in range(3)] for r in range(3)]
        Nm = horn_matrix(M)
        q, sweeps, _ = jacobi_max_eigenvector(Nm)
        R = [f32(v) for v in quaternion_rotation(q)]
        ok = all(finite(v) for v in R)
        den = None
        if not fix_scale:
            nom = f64(0.0)
            den = f64(0.0)
            for r in range(3):
                for c in range(3):
                    p3 = sum3(R[3 * r] * Pr2[0][c], R[3 * r + 1] * Pr2[1][c], R[3 * r + 2] * Pr2[2][c])
                    nom = nom + f64(Pr1[r][c]) * f64(p3)
                    sq = p3 * p3
                    den = den + f64(sq)
            ok = ok and finite(den) and den != 0
            s = f32(nom / den)
        else:
            s = f32(1.0)
        ok = ok and finite(s)
        inv_s = f32(1.0) / s
        sR = [s * R[k] for k in range(9)]
        t = [O1[r] - sum3(sR[3 * r] * O2[0], sR[3 * r + 1] * O2[1], sR[3 * r + 2] * O2[2]) for r in range(3)]
        ok = ok and all(finite(v) for v in t)
        sRi = [inv_s * R[3 * c + r] for r in range(3) for c in range(3)]
        ti = [sum3(-sRi[3 * r] * t[0], -sRi[3 * r + 1] * t[1], -sRi[3 * r + 2] * t[2]) for r in range(3)]
    return dict(ok=bool(ok), R=R, t=t, s=s, sR=sR, sRi=sRi, ti=ti, N=Nm, sweeps=sweeps, den=den)


def project(R, t, cam, X):
    """Project (:370-391) of one point"""
    return to_image(cam, rigid(R, t, X))


def dot2(d0, d1):
    """cv::Mat::dot of a 2 x 1 CV_32F with itself: double products, double sum, the result to float"""
    return f32(f64(d0) * f64(d0) + f64(d1) * f64(d1))


def check_inliers(G, S, cam1, cam2):
    """CheckInliers (:328-352) -> (flags over the N correspondences, count, [(err1, err2)])"""
    flags, errs = [], []
    with np.errstate(all="ignore"):
        for k in range(G["n"]):
            p2im1 = project(S["sR"], S["t"], cam1, G["x2"][k])
            p1im2 = project(S["sRi"], S["ti"], cam2, G["x1"][k])
            err1 = dot2(G["im1"][k][0] - p2im1[0], G["im1"][k][1] - p2im1[1])
            err2 = dot2(p1im2[0] - G["im2"][k][0], p1im2[1] - G["im2"][k][1])
            errs.append((err1, err2))
            flags.append(bool(err1 < G["max_err"][k][0] and err2 < G["max_err"][k][1]))
    return flags, sum(flags), errs


def hypothesis(G, cam1, cam2, fix_scale, seed, h):
    """hypothesis h of a gathered candidate -> dict(count, degenerate, sim3 [13] float32, flags [N], picks, solve, errs)"""
    N = G["n"]
    zero = np.zeros(13, np.float32)
    if N < 3:                                                     # S6
        return dict(count=0, degenerate=0, sim3=zero, flags=[False] * N, picks=None, solve=None, errs=None)
    picks = sample3(seed, h, N)
    P1 = [[G["x1"][i][r] for i in picks] for r in range(3)]
    P2 = [[G["x2"][i][r] for i in picks] for r in range(3)]
    S = compute_sim3(P1, P2, fix_scale)
    if not S["ok"]:                                               # S5
        return dict(count=0, degenerate=1, sim3=zero, flags=[False] * N, picks=picks, solve=S, errs=None)
    flags, count, errs = check_inliers(G, S, cam1, cam2)
    return dict(count=count, degenerate=0, sim3=np.array(S["R"] + S["t"] + [S["s"]], np.float32), flags=flags, picks=picks, solve=S, errs=errs)


def pack_words(flags, mask_words):
    w = np.zeros(mask_words, np.uint32)
    for k, f in enumerate(flags):
        if f:
            w[k >> 5] |= np.uint32(1 << (k & 31))
    return w


def candidate(cam1, cam2, pos, flags, sigma2_1, sigma2_2, mp1, mp2, idx1, idx2, n1, cap, fix_scale, seed, nhyp, mask_words):
    """everything afv_table_sim3_hypotheses returns for one candidate, as arrays of the C-ABI's shapes"""
    G = gather(cam1, cam2, pos, flags, sigma2_1, sigma2_2, mp1, mp2, idx1, idx2, n1)
    N = G["n"]
    out = dict(n=N, index1=np.full(cap, -1, np.int32), x3dc1=np.zeros((cap, 3), np.float32), x3dc2=np.zeros((cap, 3), np.float32),
               max_err=np.zeros((cap, 2), np.float32), count=np.zeros(nhyp, np.int32), degenerate=np.zeros(nhyp, np.uint8),
               sim3=np.zeros((nhyp, 13), np.float32), inliers=np.zeros((nhyp, mask_words), np.uint32), gathered=G)
    if N:
        out["index1"][:N] = G["index1"]
        out["x3dc1"][:N] = np.array(G["x1"], np.float32)
        out["x3dc2"][:N] = np.array(G["x2"], np.float32)
        out["max_err"][:N] = np.array(G["max_err"], np.float32)
    for h in range(nhyp):
        H = hypothesis(G, cam1, cam2, fix_scale, seed, h)
        out["count"][h] = H["count"]
        out["degenerate"][h] = H["degenerate"]
        out["sim3"][h] = H["sim3"]
        out["inliers"][h] = pack_words(H["flags"], mask_words)
    return out


def ransac_iterations(probability, min_inliers, max_iterations, N):
    """Q3: SetRansacParameters (:112-136) -> mRansacMaxIts"""
    with np.errstate(all="ignore"):
        epsilon = f32(min_inliers) / f32(N)
        if min_inliers == N:
            n_it = 1
        else:
            e3 = float(epsilon) ** 3 if math.isfinite(float(epsilon)) else float("inf")   # pow(float, int) promotes to double
            arg = 1.0 - e3
            den = math.log(arg) if arg > 0 else (float("-inf") if arg == 0 else float("nan"))
            num = math.log(1.0 - probability) if probability < 1 else float("-inf")
            v = num / den if den != 0 else float("inf")
            # the conversion of a double outside int's range is undefined in the reference; here it saturates, a NaN reads max_iterations
            n_it = max_iterations if math.isnan(v) else int(min(max(math.ceil(v) if math.isfinite(v) else v, -2 ** 31), 2 ** 31 - 1))
    return max(1, min(n_it, max_iterations))


class Solver:
    """the reference's class over the outputs of one candidate (count [H], sim3 [H][13], inlier flags per hypothesis, index1, mN1):
    iterate (:138-204) as a scan over the hypotheses"""

    def __init__(self, n, index1, count, sim3, flags_of, n1, nhyp):
        self.N, self.index1, self.count, self.sim3, self.flags_of, self.mN1, self.nhyp = int(n), index1, count, sim3, flags_of, int(n1), nhyp
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best = None
        self.SetRansacParameters(maxIterations=min(300, nhyp))    # :109, within what was evaluated

    def SetRansacParameters(self, probability=0.99, minInliers=6, maxIterations=300):
        if maxIterations > self.nhyp or minInliers < 3:
            raise ValueError("maxIterations beyond the evaluated hypotheses, or minInliers < 3")
        self.mRansacMinInliers = minInliers
        self.mRansacMaxIts = ransac_iterations(probability, minInliers, maxIterations, self.N)
        self.mnIterations = 0

    def T12(self, h):
        r = self.sim3[h]
        T = np.zeros((4, 4), np.float32)
        T[3, 3] = 1
        for i in range(3):
            for j in range(3):
                T[i, j] = f32(r[12]) * f32(r[3 * i + j])
            T[i, 3] = r[9 + i]
        return T

    def iterate(self, nIterations):
        """-> (T12 or None, bNoMore, vbInliers [mN1], nInliers)"""
        vb = np.zeros(self.mN1, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, vb, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            c = int(self.count[h])
            if c >= self.mnBestInliers:                           # Q2
                self.mnBestInliers = c
                self.best = h
                if c > self.mRansacMinInliers:                    # Q2
                    fl = self.flags_of(h)
                    for k in range(self.N):
                        if fl[k]:
                            vb[self.index1[k]] = True
                    return self.T12(h), False, vb, c
        return None, self.mnIterations >= self.mRansacMaxIts, vb, 0

    def find(self):
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
