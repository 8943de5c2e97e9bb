"""Plain-Python restatement of Initializer::Initialize (src/Initializer.cc:41-908).  TEST INFRASTRUCTURE ONLY.

This file is the NORMATIVE semantics of k_init_prepare / k_init_hypotheses / k_init_reconstruct (afv_frame_initializer,
include/afv_hip.h): the device is held to it bit for bit.  It follows tests/_sim3_ref.py and tests/_tri_ref.py: float32 with one rounding
per operator, no fused multiply-add.  Where a loop over the matches is written with numpy float32 arrays, every element sees the same
single-rounded operators as the scalar statement (numpy has no fused operations); the double parts are Python floats (IEEE binary64,
math.sqrt correctly rounded).  Parity with a build of the reference is unpinned: it uses Eigen::JacobiSVD<float> and its own random
generator, and Eigen is not restated here.

Restated from the reference's source:

  Initialize                      Initializer.cc:41-114      initialize, compact, draw_set
  FindHomography / FindFundamental :117-214                  hypothesis (one (model, iteration)), select
  ComputeH21 / ComputeF21         :217-293                   dlt_h, dlt_f, null_vector9, rank2 (svd3)
  CheckHomography / CheckFundamental :295-451                check_homography, check_fundamental
  ReconstructF, DecomposeE        :453-548, :886-908         reconstruct_f, decompose_e
  ReconstructH                    :550-704                   reconstruct_h
  Triangulate                     :706-726                   tests/_tri_ref.py jacobi_null_vector (not restated a third time)
  Normalize                       :728-770                   normalize
  CheckRT                         :773-884                   check_rt

Conventions:
  * every float operator rounds once; a three-term sum (a row times a column, a squared norm, h31 u + h32 v + h33) is a0 + (a1 + a2);
    other scalar expressions run left to right as written: fx * x * invz + cx is ((fx * x) * invz) + cx
  * A * B * C of 3 x 3 matrices is (A * B) * C
  * det3(m) = m00 c00 + (m01 c01 + m02 c02) with c00 = m11 m22 - m12 m21, c01 = m12 m20 - m10 m22, c02 = m10 m21 - m11 m20;
    inv3(m) = adjugate * (1 / det3(m)), every cofactor a b - c d: it stands for Eigen's inverse() and determinant()
  * double sums (A^T A, A v, squared norms in svd3) run left to right from the first term

Quirks restated as written:
  * CheckFundamental gates on 3.841 and scores with 5.991
  * CheckRT counts in nGood (and writes p3d for) points that fail cosParallax < minCos, while isGood stays false for them
  * ReconstructF's else-if chain on maxGood == nGoodK tests only the first equal hypothesis
  * RH is NaN when both scores are 0, and NaN > 0.40 is false: ReconstructF
  * ReconstructF counts its inliers in a float, ReconstructH in an int

Deliberate deviations:
  I1  null vector of the DLT system (ComputeH21 16 x 9, ComputeF21 8 x 9): M = A^T A in double (the float entries of A converted, a
      running sum over the rows), then a cyclic Jacobi on the symmetric 9 x 9 in double: pairs (0,1) (0,2) .. (0,8) (1,2) .. (7,8); only
      + - * / and sqrt; at most JACOBI_SWEEPS = 30 sweeps; a pair is skipped when a_pq == 0 or |a_pp| + |a_pq| == |a_pp| and |a_qq| +
      |a_pq| == |a_qq|; a sweep that rotates nothing ends it.  The rotation is S2's of tests/_sim3_ref.py.  The null vector is the
      column of V of the smallest diagonal entry, ties to the lowest index, rounded to float.  It replaces Eigen::JacobiSVD.
  I2  svd3 (ComputeF21's rank-2 step, DecomposeE, ReconstructH): the same Jacobi on the 3 x 3 M = A^T A in double gives V; its columns
      are ordered by descending eigenvalue (for i in 0, 1: for k in i + 1 .. 2: entries i and k are swapped when d_i < d_k);
      b_k = A v_k, w_k = |b_k|, u_0 = b_0 / w_0, u_1 = b_1 / w_1, u_2 = u_0 x u_1, and v_2 is negated when b_2 . u_2 < 0; U, w and V are
      then rounded to float.  det U = +1 by construction.  -A gives (-u_0, -u_1, u_2) and (v_0, v_1, -v_2) exactly.
  I3  ReconstructH negates A = K^-1 H21 K when det3(A) < 0, so the eight hypotheses do not depend on the sign of H21 (then s = det U *
      det Vt = 1 up to rounding).  DecomposeE needs no such rule: R1, R2 and t come out the same for E and -E (I2 and the det < 0 flips).
  I4  draws: key_h = sm(sm(seed) ^ (h + 1)), draw d in 0..7 = sm(key_h + (d + 1) * DRAW_STEP) % (N - d), applied to availableIndices
      with the reference's swap-with-back (:83-89).  H and F share the sets.
  I5  sums are fixed-shape trees, not running sums in index order.  Normalize: 256 partial sums (partial t adds the elements t, t + 256,
      .. in ascending order, starting from 0), then p[t] = p[t] + p[t + s] for s = 128, 64 .. 1.  The two scores: a match contributes
      e = c1 + c2 (c = th - chiSquare where the gate passes, else 0); 64 partial sums over the matches l, l + 64, .. and the same
      halving tree from s = 32.
  I6  no acosf: parallax > minParallax is cos < COS_MIN_PARALLAX, parallax >= minParallax is cos <= COS_MIN_PARALLAX, with
      COS_MIN_PARALLAX = float(cos(1 degree)); nGood == 0 gives cosine 1 (parallax 0); ReconstructH starts from bestParallax = -1, here
      cosine 2.  The selected cosine is the min(50, n - 1)-th smallest of the pushed ones.
  I7  N < 8: nothing is evaluated, ok = 0, reason TOO_FEW_MATCHES; every per-hypothesis output reads 0.
  I8  a hypothesis is degenerate when the second-smallest diagonal entry of the converged 9 x 9 is <= 1e-12 times the largest (the
      null vector is not defined by the 8 pairs: repeated or collinear points), or when an entry of H21, H12 or F21 is not finite
      (det(H21) == 0 makes H12 not finite): it scores 0, is flagged, and its model record and inlier words read 0.  A match whose
      chiSquare is not finite fails that gate and contributes 0.
  I9  no hypothesis of a model scores above 0: the model is all zeros with no inliers and its winning index is -1.
  I10 CheckRT: a point with x3Dh(3) == 0 (the reference ignores Triangulate's false and reads an unwritten vector) or with a
      cosParallax that is not finite is skipped like a point that is not finite.
  I11 on ok = 0, R21, t21, p3d and triangulated read 0; on ok = 1, the p3d rows CheckRT did not write read 0.
"""
import math

import numpy as np

from _points_ref import SUM_ORDER
from _tri_ref import jacobi_null_vector
from _voctrain_ref import DRAW_STEP, M64, sm

assert SUM_ORDER == "a0+(a1+a2)"
f32 = np.float32
JACOBI_SWEEPS = 30
RANK_GAP = 1e-12
MIN_RH = f32(0.4)
MIN_TRIANGULATED = 50
PERC_MAX_GOOD, PERC_MIN_GOOD, X_SIGMA2 = f32(0.7), f32(0.9), f32(4.0)
D_RATIO, PERC_BEST_GOOD, PERC_SECOND_BEST_GOOD = f32(1.00001), f32(0.9), f32(0.75)
MIN_COS, PARALLAX_IDX = f32(0.99998), 50
CHI_H, CHI_F_GATE, CHI_F_SCORE = f32(5.991), f32(3.841), f32(5.991)
COS_MIN_PARALLAX = f32(math.cos(math.pi / 180.0))   # I6: 0.9998477f
ROUTE_H, ROUTE_F = 0, 1
REASONS = ("ok", "too_few_matches", "d_ratio", "ambiguous", "parallax", "min_triangulated", "min_good")
OK, TOO_FEW_MATCHES, DRATIO, AMBIGUOUS, PARALLAX, MIN_TRI, MIN_GOOD = range(7)
ZERO, ONE = f32(0.0), f32(1.0)


def sum3(a0, a1, a2):
    return a0 + (a1 + a2)


def finite(v):
    return bool(np.all(np.isfinite(v)))


def mat(rows):
    return [[f32(v) for v in r] for r in rows]


def mm(A, B):
    return [[sum3(A[r][0] * B[0][c], A[r][1] * B[1][c], A[r][2] * B[2][c]) for c in range(3)] for r in range(3)]


def transpose(A):
    return [[A[c][r] for c in range(3)] for r in range(3)]


def neg(A):
    return [[-v for v in r] for r in A]


def cof0(m):
    return (m[1][1] * m[2][2] - m[1][2] * m[2][1], m[1][2] * m[2][0] - m[1][0] * m[2][2], m[1][0] * m[2][1] - m[1][1] * m[2][0])


def det3(m):
    c = cof0(m)
    return sum3(m[0][0] * c[0], m[0][1] * c[1], m[0][2] * c[2])


def inv3(m):
    c = cof0(m)
    i = ONE / sum3(m[0][0] * c[0], m[0][1] * c[1], m[0][2] * c[2])
    return [[c[0] * i, (m[0][2] * m[2][1] - m[0][1] * m[2][2]) * i, (m[0][1] * m[1][2] - m[0][2] * m[1][1]) * i],
            [c[1] * i, (m[0][0] * m[2][2] - m[0][2] * m[2][0]) * i, (m[0][2] * m[1][0] - m[0][0] * m[1][2]) * i],
            [c[2] * i, (m[0][1] * m[2][0] - m[0][0] * m[2][1]) * i, (m[0][0] * m[1][1] - m[0][1] * m[1][0]) * i]]


def flat(m):
    return np.array([v for r in m for v in r], np.float32)


def tree_sum(e, width):
    """I5: `width` strided running partial sums, then the halving tree"""
    e = np.asarray(e, np.float32)
    rows = (len(e) + width - 1) // width
    pad = np.zeros(max(rows, 1) * width, np.float32)
    pad[:len(e)] = e
    pad = pad.reshape(-1, width)
    acc = np.zeros(width, np.float32)
    for r in range(rows):
        acc = acc + pad[r]
    s = width // 2
    while s >= 1:
        acc = acc[:s] + acc[s:2 * s]
        s //= 2
    return f32(acc[0])


# ---- I1 / I2: the Jacobi in double (Python floats) ----
def jacobi_sym(a, n):
    """a: symmetric n x n list of Python floats, changed in place.  -> (V as n x n list, sweeps that rotated)"""
    v = [[1.0 if r == c else 0.0 for c in range(n)] for r in range(n)]
    sweeps = 0
    for _ in range(JACOBI_SWEEPS):
        rotated = False
        for p in range(n - 1):
            for q in range(p + 1, n):
                apq, app, aqq = a[p][q], a[p][p], a[q][q]
                if apq == 0.0:
                    continue
                g = abs(apq)
                if abs(app) + g == abs(app) and abs(aqq) + g == abs(aqq):
                    continue
                theta = (aqq - app) / (2.0 * apq)
                t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(n):
                    if k == p or k == q:
                        continue
                    akp, akq = a[k][p], a[k][q]
                    np_, nq = c * akp - s * akq, s * akp + c * akq
                    a[k][p] = np_
                    a[p][k] = np_
                    a[k][q] = nq
                    a[q][k] = nq
                a[p][p] = app - t * apq
                a[q][q] = aqq + t * apq
                a[p][q] = 0.0
                a[q][p] = 0.0
                for k in range(n):
                    vkp, vkq = v[k][p], v[k][q]
                    v[k][p] = c * vkp - s * vkq
                    v[k][q] = s * vkp + c * vkq
                rotated = True
        if not rotated:
            break
        sweeps += 1
    return v, sweeps


def gram(A, n):
    """M = A^T A in double: running sums over the rows"""
    M = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(n):
            s = 0.0
            for row in A:
                s = s + float(row[i]) * float(row[j])
            M[i][j] = s
    return M


def null_vector9(A):
    """I1, I8.  A: rows of 9 float32.  -> (the null vector as 9 Python floats (before the float rounding), rank deficient?, sweeps)"""
    a = gram(A, 9)
    v, sweeps = jacobi_sym(a, 9)
    d = [a[k][k] for k in range(9)]
    lo = 0
    for k in range(1, 9):
        if d[k] < d[lo]:
            lo = k
    second, largest = None, d[0]
    for k in range(9):
        if d[k] > largest:
            largest = d[k]
        if k != lo and (second is None or d[k] < second):
            second = d[k]
    deficient = not (second > RANK_GAP * largest)
    return [v[k][lo] for k in range(9)], deficient, sweeps


def svd3(A):
    """I2.  A: 3 x 3 float32.  -> (U, w, V) float32, U and V as 3 x 3 lists whose COLUMNS are the vectors"""
    Ad = [[float(v) for v in r] for r in A]
    a = gram(Ad, 3)
    v, _ = jacobi_sym(a, 3)
    d = [a[0][0], a[1][1], a[2][2]]
    order = [0, 1, 2]
    for i in range(2):
        for k in range(i + 1, 3):
            if d[i] < d[k]:
                d[i], d[k] = d[k], d[i]
                order[i], order[k] = order[k], order[i]
    vc = [[v[r][order[k]] for r in range(3)] for k in range(3)]          # vc[k] = v_k
    b = [[(Ad[r][0] * vc[k][0] + Ad[r][1] * vc[k][1]) + Ad[r][2] * vc[k][2] for r in range(3)] for k in range(3)]
    with np.errstate(all="ignore"):
        w = [math.sqrt((b[k][0] * b[k][0] + b[k][1] * b[k][1]) + b[k][2] * b[k][2]) for k in range(3)]
        u0 = [float(np.float64(b[0][r]) / np.float64(w[0])) for r in range(3)]
        u1 = [float(np.float64(b[1][r]) / np.float64(w[1])) for r in range(3)]
    u2 = [u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]]
    if (b[2][0] * u2[0] + b[2][1] * u2[1]) + b[2][2] * u2[2] < 0.0:
        vc[2] = [-x for x in vc[2]]
    uc = [u0, u1, u2]
    U = [[f32(uc[c][r]) for c in range(3)] for r in range(3)]
    V = [[f32(vc[c][r]) for c in range(3)] for r in range(3)]
    return U, [f32(x) for x in w], V


# ---- Initialize :41-91 ----
def compact(matches12):
    return [(i, int(m)) for i, m in enumerate(matches12) if int(m) >= 0]


def draws(seed, h, N):
    key = sm(sm(seed & M64) ^ (h + 1))
    return [sm((key + (d + 1) * DRAW_STEP) & M64) % (N - d) for d in range(8)]


def draw_set(seed, h, N):
    """I4 on availableIndices (:78-90), literally"""
    avail = list(range(N))
    out = []
    for r in draws(seed, h, N):
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def draw_set_closed(seed, h, N):
    """the same eight indices without the N-sized list (what the kernel computes): at most 8 positions are disturbed"""
    pos, val, out = [], [], []

    def look(p):
        return val[pos.index(p)] if p in pos else p

    for d, r in enumerate(draws(seed, h, N)):
        out.append(look(r))
        back = look(N - 1 - d)
        if r in pos:
            val[pos.index(r)] = back
        else:
            pos.append(r)
            val.append(back)
    return out


# ---- Normalize :728-770 ----
def normalize(x, y):
    """-> (meanX, meanY, sX, sY) float32 over ALL keypoints of a frame; T = [[sX, 0, -meanX sX], [0, sY, -meanY sY], [0, 0, 1]]"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    with np.errstate(all="ignore"):
        n = f32(len(x))
        mx, my = tree_sum(x, 256) / n, tree_sum(y, 256) / n
        dx, dy = tree_sum(np.abs(x - mx), 256) / n, tree_sum(np.abs(y - my), 256) / n
        return mx, my, ONE / dx, ONE / dy


def t_matrix(nrm):
    mx, my, sx, sy = nrm
    return [[sx, ZERO, -mx * sx], [ZERO, sy, -my * sy], [ZERO, ZERO, ONE]]


# ---- ComputeH21 / ComputeF21 :217-293 ----
def dlt_h(P1, P2):
    A = []
    for (u1, v1), (u2, v2) in zip(P1, P2):
        A.append([ZERO, ZERO, ZERO, -u1, -v1, -ONE, v2 * u1, v2 * v1, v2])
        A.append([u1, v1, ONE, ZERO, ZERO, ZERO, -u2 * u1, -u2 * v1, -u2])
    return A


def dlt_f(P1, P2):
    return [[u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, ONE] for (u1, v1), (u2, v2) in zip(P1, P2)]


def as3(vec):
    return [[f32(vec[3 * r + c]) for c in range(3)] for r in range(3)]


def rank2(Fpre):
    U, w, V = svd3(Fpre)
    UD = [[U[r][0] * w[0], U[r][1] * w[1], U[r][2] * ZERO] for r in range(3)]
    return mm(UD, transpose(V))


# ---- CheckHomography / CheckFundamental :295-451 over all matches at once ----
def _gate(chi, th):
    with np.errstate(all="ignore"):
        return np.isfinite(chi) & ~(chi > th)


def check_homography(H21, H12, u1, v1, u2, v2, sigma):
    """-> (score, inlier mask)"""
    with np.errstate(all="ignore"):
        inv_s2 = ONE / (sigma * sigma)
        h, g = H21, H12
        w = ONE / sum3(g[2][0] * u2, g[2][1] * v2, g[2][2])
        a = sum3(g[0][0] * u2, g[0][1] * v2, g[0][2]) * w
        b = sum3(g[1][0] * u2, g[1][1] * v2, g[1][2]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w = ONE / sum3(h[2][0] * u1, h[2][1] * v1, h[2][2])
        a = sum3(h[0][0] * u1, h[0][1] * v1, h[0][2]) * w
        b = sum3(h[1][0] * u1, h[1][1] * v1, h[1][2]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
        in1, in2 = _gate(chi1, CHI_H), _gate(chi2, CHI_H)
        e = np.where(in1, CHI_H - chi1, ZERO).astype(np.float32) + np.where(in2, CHI_H - chi2, ZERO).astype(np.float32)
        return tree_sum(e, 64), in1 & in2


def check_fundamental(F, u1, v1, u2, v2, sigma):
    with np.errstate(all="ignore"):
        inv_s2 = ONE / (sigma * sigma)
        a2 = sum3(F[0][0] * u1, F[0][1] * v1, F[0][2])
        b2 = sum3(F[1][0] * u1, F[1][1] * v1, F[1][2])
        c2 = sum3(F[2][0] * u1, F[2][1] * v1, F[2][2])
        num2 = sum3(a2 * u2, b2 * v2, c2)
        chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_s2
        a1 = sum3(F[0][0] * u2, F[1][0] * v2, F[2][0])
        b1 = sum3(F[0][1] * u2, F[1][1] * v2, F[2][1])
        c1 = sum3(F[0][2] * u2, F[1][2] * v2, F[2][2])
        num1 = sum3(a1 * u1, b1 * v1, c1)
        chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_s2
        in1, in2 = _gate(chi1, CHI_F_GATE), _gate(chi2, CHI_F_GATE)
        e = np.where(in1, CHI_F_SCORE - chi1, ZERO).astype(np.float32) + np.where(in2, CHI_F_SCORE - chi2, ZERO).astype(np.float32)
        return tree_sum(e, 64), in1 & in2


class Scene:
    """what a call reads: the mvKeysUn planes of both frames, matches12, K, sigma, iterations, seed"""

    def __init__(self, x1, y1, x2, y2, matches12, fx, fy, cx, cy, sigma=1.0, iterations=200, seed=0):
        a = lambda v: np.ascontiguousarray(v, np.float32).reshape(-1)
        self.x1, self.y1, self.x2, self.y2 = a(x1), a(y1), a(x2), a(y2)
        self.matches12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
        assert len(self.matches12) == len(self.x1)
        self.fx, self.fy, self.cx, self.cy, self.sigma = f32(fx), f32(fy), f32(cx), f32(cy), f32(sigma)
        self.iterations, self.seed = int(iterations), int(seed)

    @property
    def K(self):
        return [[self.fx, ZERO, self.cx], [ZERO, self.fy, self.cy], [ZERO, ZERO, ONE]]


def hypothesis(sc, pairs, nrm1, nrm2, model, idx8, uv):
    """one (model, iteration): -> dict(score, model[9], degenerate, inliers (bool [N]), null (Python floats), deficient)"""
    N = len(pairs)
    zero = dict(score=ZERO, model=np.zeros(9, np.float32), degenerate=1, inliers=np.zeros(N, bool))
    with np.errstate(all="ignore"):
        P1 = [((sc.x1[pairs[k][0]] - nrm1[0]) * nrm1[2], (sc.y1[pairs[k][0]] - nrm1[1]) * nrm1[3]) for k in idx8]
        P2 = [((sc.x2[pairs[k][1]] - nrm2[0]) * nrm2[2], (sc.y2[pairs[k][1]] - nrm2[1]) * nrm2[3]) for k in idx8]
        A = dlt_h(P1, P2) if model == ROUTE_H else dlt_f(P1, P2)
        nv, deficient, _ = null_vector9(A)
        zero.update(null=nv, deficient=deficient, A=A)
        T1, T2 = t_matrix(nrm1), t_matrix(nrm2)
        if model == ROUTE_H:
            H21 = mm(mm(inv3(T2), as3(nv)), T1)
            H12 = inv3(H21)
            if deficient or not finite(flat(H21)) or not finite(flat(H12)):
                return zero
            score, inl = check_homography(H21, H12, *uv, sc.sigma)
            M = H21
        else:
            F21 = mm(mm(transpose(T2), rank2(as3(nv))), T1)
            if deficient or not finite(flat(F21)):
                return zero
            score, inl = check_fundamental(F21, *uv, sc.sigma)
            M = F21
    return dict(score=score, model=flat(M), degenerate=0, inliers=inl, null=nv, deficient=deficient, A=A)


def select(hyps):
    """:157 / :207: the strict > keeps the lowest index that holds the maximum; I9"""
    best, score = -1, ZERO
    for h, r in enumerate(hyps):
        if r["score"] > score:
            best, score = h, r["score"]
    return best, score


# ---- CheckRT :773-884 ----
def check_rt(sc, pairs, inliers, R, t, th2):
    """-> dict(n_good, cos, p3d [N1][3], good [N1]); cos is I6's selected cosine"""
    n1 = len(sc.x1)
    p3d, good, cosv = np.zeros((n1, 3), np.float32), np.zeros(n1, np.uint8), []
    K = sc.K
    with np.errstate(all="ignore"):
        Rt = [[R[r][0], R[r][1], R[r][2], t[r]] for r in range(3)]
        P1 = [[sc.fx, ZERO, sc.cx, ZERO], [ZERO, sc.fy, sc.cy, ZERO], [ZERO, ZERO, ONE, ZERO]]
        P2 = [[sum3(K[r][0] * Rt[0][c], K[r][1] * Rt[1][c], K[r][2] * Rt[2][c]) for c in range(4)] for r in range(3)]
        O2 = [sum3(-R[0][r] * t[0], -R[1][r] * t[1], -R[2][r] * t[2]) for r in range(3)]
        n_good = 0
        for k, (i1, i2) in enumerate(pairs):
            if not inliers[k]:
                continue
            kx1, ky1, kx2, ky2 = sc.x1[i1], sc.y1[i1], sc.x2[i2], sc.y2[i2]
            A = [[kx1 * P1[2][c] - P1[0][c] for c in range(4)], [ky1 * P1[2][c] - P1[1][c] for c in range(4)],
                 [kx2 * P2[2][c] - P2[0][c] for c in range(4)], [ky2 * P2[2][c] - P2[1][c] for c in range(4)]]
            v, _ = jacobi_null_vector(A)
            if v[3] == 0:                                             # I10
                continue
            p = [v[0] / v[3], v[1] / v[3], v[2] / v[3]]
            if not finite(p):
                continue
            dist1 = np.sqrt(sum3(p[0] * p[0], p[1] * p[1], p[2] * p[2]))
            n2 = [p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]]
            dist2 = np.sqrt(sum3(n2[0] * n2[0], n2[1] * n2[1], n2[2] * n2[2]))
            cosp = sum3(p[0] * n2[0], p[1] * n2[1], p[2] * n2[2]) / (dist1 * dist2)
            if not finite(cosp):                                      # I10
                continue
            if p[2] <= 0 and cosp < MIN_COS:
                continue
            q = [sum3(R[r][0] * p[0], R[r][1] * p[1], R[r][2] * p[2]) + t[r] for r in range(3)]
            if q[2] <= 0 and cosp < MIN_COS:
                continue
            iz = ONE / p[2]
            ex, ey = (sc.fx * p[0] * iz + sc.cx) - kx1, (sc.fy * p[1] * iz + sc.cy) - ky1
            if ex * ex + ey * ey > th2:
                continue
            iz = ONE / q[2]
            ex, ey = (sc.fx * q[0] * iz + sc.cx) - kx2, (sc.fy * q[1] * iz + sc.cy) - ky2
            if ex * ex + ey * ey > th2:
                continue
            cosv.append(cosp)
            p3d[i1] = p
            n_good += 1
            if cosp < MIN_COS:
                good[i1] = 1
    cos = sorted(cosv)[min(PARALLAX_IDX, len(cosv) - 1)] if n_good > 0 else ONE
    return dict(n_good=n_good, cos=f32(cos), p3d=p3d, good=good, n_cos=len(cosv))


def decompose_e(E):
    """:886-908 -> (R1, R2, t)"""
    U, _, V = svd3(E)
    with np.errstate(all="ignore"):
        t = [U[0][2], U[1][2], U[2][2]]
        nrm = np.sqrt(sum3(t[0] * t[0], t[1] * t[1], t[2] * t[2]))
        t = [t[0] / nrm, t[1] / nrm, t[2] / nrm]
        Vt = transpose(V)
        R1 = mm([[U[r][1], -U[r][0], U[r][2]] for r in range(3)], Vt)   # U * W
        if det3(R1) < 0:
            R1 = neg(R1)
        R2 = mm([[-U[r][1], U[r][0], U[r][2]] for r in range(3)], Vt)   # U * W^T
        if det3(R2) < 0:
            R2 = neg(R2)
    return R1, R2, t


def reconstruct_f(sc, pairs, inliers, F21, tr):
    with np.errstate(all="ignore"):
        N = ZERO
        for b in inliers:
            if b:
                N = N + ONE
        K = sc.K
        E21 = mm(mm(transpose(K), F21), K)
        R1, R2, t = decompose_e(E21)
        t2 = [-t[0], -t[1], -t[2]]
        motions = [(R1, t), (R2, t), (R1, t2), (R2, t2)]
        th2 = X_SIGMA2 * (sc.sigma * sc.sigma)
        res = [check_rt(sc, pairs, inliers, R, tt, th2) for R, tt in motions]
        tr.update(motions=motions, checks=res)
        g = [r["n_good"] for r in res]
        max_good = max(g)
        n_min_good = max(int(PERC_MIN_GOOD * N), MIN_TRIANGULATED)
        nsimilar = sum(1 for k in range(4) if f32(g[k]) > PERC_MAX_GOOD * f32(max_good))
        if max_good < n_min_good:
            return MIN_TRI if max_good < MIN_TRIANGULATED else MIN_GOOD, -1
        if nsimilar > 1:
            return AMBIGUOUS, -1
        k = g.index(max_good)                                          # the else-if chain: the first equal one only
        if res[k]["cos"] < COS_MIN_PARALLAX:
            return OK, k
        return PARALLAX, -1


def reconstruct_h(sc, pairs, inliers, H21, tr):
    with np.errstate(all="ignore"):
        N = sum(1 for b in inliers if b)
        K = sc.K
        A = mm(mm(inv3(K), H21), K)
        if det3(A) < 0:                                                # I3
            A = neg(A)
        U, w, V = svd3(A)
        Vt = transpose(V)
        s = det3(U) * det3(Vt)
        d1, d2, d3 = w
        tr.update(d=(d1, d2, d3))
        if d1 / d2 < D_RATIO or d2 / d3 < D_RATIO:
            return DRATIO, -1
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [aux_st, -aux_st, -aux_st, aux_st]
        sU = [[s * U[r][c] for c in range(3)] for r in range(3)]
        motions = []

        def unit(U, tp):
            t = [sum3(U[r][0] * tp[0], U[r][1] * tp[1], U[r][2] * tp[2]) for r in range(3)]
            nrm = np.sqrt(sum3(t[0] * t[0], t[1] * t[1], t[2] * t[2]))
            return [t[0] / nrm, t[1] / nrm, t[2] / nrm]

        for i in range(4):
            Rp = [[ct, ZERO, -st[i]], [ZERO, ONE, ZERO], [st[i], ZERO, ct]]
            R = mm(mm(sU, Rp), Vt)
            m = d1 - d3
            motions.append((R, unit(U, [x1[i] * m, ZERO * m, -x3[i] * m])))
        aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
        for i in range(4):
            Rp = [[cp, ZERO, sp[i]], [ZERO, -ONE, ZERO], [sp[i], ZERO, -cp]]
            R = mm(mm(sU, Rp), Vt)
            m = d1 + d3
            motions.append((R, unit(U, [x1[i] * m, ZERO * m, x3[i] * m])))
        th2 = X_SIGMA2 * (sc.sigma * sc.sigma)
        res = [check_rt(sc, pairs, inliers, R, tt, th2) for R, tt in motions]
        tr.update(motions=motions, checks=res)
        best_good, second, best, best_cos = 0, 0, -1, f32(2.0)
        for i, r in enumerate(res):
            if r["n_good"] > best_good:
                second, best_good, best, best_cos = best_good, r["n_good"], i, r["cos"]
            elif r["n_good"] > second:
                second = r["n_good"]
        tr.update(best_good=best_good, second_best_good=second)
        if not f32(second) < PERC_SECOND_BEST_GOOD * f32(best_good):
            return AMBIGUOUS, -1
        if not best_cos <= COS_MIN_PARALLAX:
            return PARALLAX, -1
        if not f32(best_good) > f32(MIN_TRIANGULATED):
            return MIN_TRI, -1
        if not f32(best_good) > PERC_BEST_GOOD * f32(N):
            return MIN_GOOD, -1
        return OK, best


def mask_words(inl, words):
    out = np.zeros(words, np.uint32)
    for k, b in enumerate(inl):
        if b:
            out[k >> 5] |= np.uint32(1 << (k & 31))
    return out


def initialize(sc, negate_models=False, keep_hypotheses=True):
    """Initialize (:41-114).  -> dict(ok, route, R21 [9], t21 [3], p3d [N1][3], triangulated [N1], trace, hyp).  negate_models: hand -H21
    and -F21 to the reconstruction (the sign must not reach any output)"""
    n1 = len(sc.x1)
    pairs = compact(sc.matches12)
    N = len(pairs)
    out = dict(ok=0, route=ROUTE_F, R21=np.zeros(9, np.float32), t21=np.zeros(3, np.float32), p3d=np.zeros((n1, 3), np.float32),
               triangulated=np.zeros(n1, np.uint8))
    tr = dict(N=N, SH=ZERO, SF=ZERO, RH=ZERO, best=[-1, -1], model=[np.zeros(9, np.float32), np.zeros(9, np.float32)], n_motion=0,
              reason=TOO_FEW_MATCHES, motions=[], checks=[], best_motion=-1, n_inliers=0, T1=np.zeros(9, np.float32), T2=np.zeros(9, np.float32))
    out["trace"] = tr
    out["hyp"] = [[], []]
    if N < 8:                                                          # I7
        return out
    nrm1, nrm2 = normalize(sc.x1, sc.y1), normalize(sc.x2, sc.y2)
    tr["T1"], tr["T2"] = flat(t_matrix(nrm1)), flat(t_matrix(nrm2))
    i1 = np.array([p[0] for p in pairs])
    i2 = np.array([p[1] for p in pairs])
    uv = (sc.x1[i1], sc.y1[i1], sc.x2[i2], sc.y2[i2])
    sets = [draw_set(sc.seed, h, N) for h in range(sc.iterations)]
    tr["sets"] = sets
    hyps = [[hypothesis(sc, pairs, nrm1, nrm2, m, sets[h], uv) for h in range(sc.iterations)] for m in (ROUTE_H, ROUTE_F)]
    out["hyp"] = hyps
    with np.errstate(all="ignore"):
        (bh, SH), (bf, SF) = select(hyps[0]), select(hyps[1])
        RH = SH / (SH + SF)
    models, inls = [], []
    for m, b in ((0, bh), (1, bf)):
        models.append(hyps[m][b]["model"] if b >= 0 else np.zeros(9, np.float32))
        inls.append(hyps[m][b]["inliers"] if b >= 0 else np.zeros(N, bool))
    route = ROUTE_H if RH > MIN_RH else ROUTE_F
    tr.update(SH=SH, SF=SF, RH=RH, best=[bh, bf], model=models, n_inliers=int(np.sum(inls[route])))
    M = as3(models[route])
    if negate_models:
        M = neg(M)
    reason, k = (reconstruct_h if route == ROUTE_H else reconstruct_f)(sc, pairs, inls[route], M, tr)
    tr.update(reason=reason, best_motion=k, n_motion=len(tr["motions"]))
    out["route"] = route
    if reason == OK:
        R, t = tr["motions"][k]
        out.update(ok=1, R21=flat(R), t21=np.array(t, np.float32), p3d=tr["checks"][k]["p3d"], triangulated=tr["checks"][k]["good"])
    return out
