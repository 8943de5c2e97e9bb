"""Plain-Python restatement of PnPsolver (src/PnPsolver.cc:67-950).  TEST INFRASTRUCTURE ONLY.

This file is the NORMATIVE semantics of k_pnp_gather / k_pnp_hypotheses / k_pnp_refine (afv_frame_pnp_hypotheses, include/afv_hip.h) and
of the host scan of the Python class (PnPsolver.iterate): the device is held to it bit for bit.  Doubles are Python floats (IEEE binary64,
one rounding per operator, math.sqrt correctly rounded), floats are np.float32; no fused multiply-add anywhere.  Parity with a build of
the reference is unpinned: the reference links OpenCV's legacy cvSVD / cvSolve / cvInvert, which are not part of this project.

Restated from the reference's source:

  the constructor                 PnPsolver.cc:67-110       gather
  SetRansacParameters             :121-157                  ransac_parameters, Solver.SetRansacParameters
  iterate / find / Refine         :159-305                  Solver.iterate / Solver.find / Solver.Refine (the sequential loop, Q4 literal)
  CheckInliers                    :308-339                  check_inliers
  compute_pose and what it calls  :375-950                  epnp

Conventions:
  * scalar expressions are evaluated left to right as written: a + b + c is (a + b) + c; dot(a, b) is (a0 b0 + a1 b1) + a2 b2
  * an accumulation `x = 0; x += t_i` is ((0 + t_0) + t_1) + ...
  * a float literal in a double expression (1.0f, 2.0f) is that value as a double: exact

Quirks restated as written:
  Q1  the `||` of iterate's loop (:182): a call runs until mnIterations >= mRansacMaxIts AND its own count >= nIterations
  Q2  pow(epsilon, 3) with a minimal set of 4 (:150)
  Q3  the best is updated on >, the early answer is given on refined count > min, the final answer on best >= min: the UNREFINED best pose
  Q4  Refine runs at every qualifying hypothesis, on the best set so far, not on the current one
  Q5  CheckInliers: Xc, Yc, invZc are floats of double expressions, ue / ve double, distX / distY / error2 float, error2 < mvMaxError[i]
  Q6  solve_for_sign looks at the first selected correspondence only

Deliberate deviations:
  E1  eigenvectors of M^T M: cyclic Jacobi on the symmetric 12 x 12 in double, pairs (0,1) (0,2) ... (10,11), the rotation, skip and
      stop rules of S2 (tests/_sim3_ref.py), at most JACOBI_SWEEPS sweeps; columns ordered by descending diagonal entry, ties to the
      lowest index (rank_i = #{j: d_j > d_i or (d_j == d_i and j < i)}); ut row k = that column; signs as the Jacobi leaves them
  E2  PCA of the points: the same Jacobi on the 3 x 3, descending order
  E3  cvInvert(CC, CV_SVD): the inverse by cofactors in double: c0 = m4 m8 - m5 m7, c1 = m5 m6 - m3 m8, c2 = m3 m7 - m4 m6,
      i = 1 / (m0 c0 + m1 c1 + m2 c2), every cofactor times i (the layout of the Initializer's inv3)
  E4  the three cvSolve(CV_SVD) least-squares systems go through qr_solve (:860-950), restated as written, on copies of L's columns and rho
  E5  estimate_R_and_t's SVD of ABt: V from the Jacobi on A^T A (descending), u_k = A v_k / |A v_k| for k = 0, 1, u_2 = u_0 x u_1, v_2
      negated when (A v_2) . u_2 < 0; R = U V^T, then the reference's det < 0 fix
  E6  draws: key_h = sm(sm(seed) ^ (h + 1)), draw d = sm(key_h + (d + 1) * DRAW_STEP) % (N - d) on vAvailableIndices, swap-with-back
  E7  every sum over the selected correspondences has a fixed shape: 64 partial sums (partial l starts at 0.0 and adds the selected
      elements l, l + 64, ... in ascending order), then p[l] += p[l + s] for s = 32 .. 1
  E8  degenerate: qr_solve meets eta == 0, a betas[0] that is divided by is 0, or an entry of R / t of the chosen approximation is not
      finite: 0 inliers, flagged, pose and words 0.  A reprojection error that is not finite loses the comparison of the approximations;
      a correspondence whose error2 is not finite is no inlier.  A coplanar or collinear 4-set has NO rule of its own: CC is (nearly)
      singular, the pose is whatever the arithmetic gives (few inliers) or not finite (this clause) - the reference has no rank test either
  E9  N < 4 evaluates nothing: counts 0, no flag
  E10 what is not written reads 0; the refined rows of a hypothesis that is not a record read 0 with refined = 0
"""
import math

import numpy as np

from _voctrain_ref import DRAW_STEP, M64, sm

f32 = np.float32
SET, BAD = 1, 2
JACOBI_SWEEPS = 30
INT_MAX = 2 ** 31 - 1


def finite(v):
    return math.isfinite(v)


def fsum(vals):
    """E7"""
    p = [0.0] * 64
    for j, v in enumerate(vals):
        p[j & 63] = p[j & 63] + v
    s = 32
    while s >= 1:
        for l in range(s):
            p[l] = p[l] + p[l + s]
        s >>= 1
    return p[0]


def div(a, b):
    """IEEE division (Python raises on a zero divisor)"""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        neg = (math.copysign(1.0, a) < 0) != (math.copysign(1.0, b) < 0)
        return -math.inf if neg else math.inf
    return a / b


def sqrt(a):
    if a != a or a < 0.0:
        return math.nan
    return math.sqrt(a)


def jacobi(A, n):
    """E1 / E2.  A: symmetric n x n of doubles -> (diagonal, V as rows [k][column], sweeps that rotated)"""
    a = [[float(A[r][c]) for c in range(n)] for r in range(n)]
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
                theta = div(aqq - app, 2.0 * apq)
                t = div(1.0, abs(theta) + sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = div(1.0, sqrt(t * t + 1.0))
                s = t * c
                for k in range(n):
                    if k == p or k == q:
                        continue
                    akp, akq = a[k][p], a[k][q]
                    np_ = c * akp - s * akq
                    nq = s * akp + c * akq
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
    return [a[k][k] for k in range(n)], v, sweeps


def order_desc(d):
    """the column of every rank: descending, ties to the lowest index; a rank nobody takes (NaN) reads column 0, the last writer wins"""
    n = len(d)
    col = [0] * n
    for i in range(n):
        rank = 0
        for j in range(n):
            if d[j] > d[i] or (d[j] == d[i] and j < i):
                rank += 1
        col[rank] = i
    return col


def inv3(m):
    """E3"""
    c0 = m[4] * m[8] - m[5] * m[7]
    c1 = m[5] * m[6] - m[3] * m[8]
    c2 = m[3] * m[7] - m[4] * m[6]
    i = div(1.0, m[0] * c0 + m[1] * c1 + m[2] * c2)
    return [c0 * i, (m[2] * m[7] - m[1] * m[8]) * i, (m[1] * m[5] - m[2] * m[4]) * i,
            c1 * i, (m[0] * m[8] - m[2] * m[6]) * i, (m[2] * m[3] - m[0] * m[5]) * i,
            c2 * i, (m[1] * m[6] - m[0] * m[7]) * i, (m[0] * m[4] - m[1] * m[3]) * i]


def dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(p1, p2):
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2])


def qr_solve(A, b, nr, nc, info):
    """:860-950 as written, on copies.  A: nr x nc row-major list, b: nr.  eta == 0: E8 (X reads 0)"""
    A = list(A)
    b = list(b)
    A1 = [0.0] * nc
    A2 = [0.0] * nc
    for k in range(nc):
        eta = abs(A[k * nc + k])
        for i in range(k + 1, nr):
            elt = abs(A[i * nc + k])
            if eta < elt:
                eta = elt
        if eta == 0.0:
            info["eta0"] = True
            return [0.0] * nc
        inv_eta = div(1.0, eta)
        ssum = 0.0
        for i in range(k, nr):
            A[i * nc + k] = A[i * nc + k] * inv_eta
            ssum = ssum + A[i * nc + k] * A[i * nc + k]
        sigma = sqrt(ssum)
        if A[k * nc + k] < 0.0:
            sigma = -sigma
        A[k * nc + k] = A[k * nc + k] + sigma
        A1[k] = sigma * A[k * nc + k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            ssum = 0.0
            for i in range(k, nr):
                ssum = ssum + A[i * nc + k] * A[i * nc + j]
            tau = div(ssum, A1[k])
            for i in range(k, nr):
                A[i * nc + j] = A[i * nc + j] - tau * A[i * nc + k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau = tau + A[i * nc + j] * b[i]
        tau = div(tau, A1[j])
        for i in range(j, nr):
            b[i] = b[i] - tau * A[i * nc + j]
    X = [0.0] * nc
    X[nc - 1] = div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        ssum = 0.0
        for j in range(i + 1, nc):
            ssum = ssum + A[i * nc + j] * X[j]
        X[i] = div(b[i] - ssum, A2[i])
    return X


def l_columns(L, cols):
    return [L[10 * i + c] for i in range(6) for c in cols]


def betas_approx_1(L, rho, info):
    b4 = qr_solve(l_columns(L, (0, 1, 3, 6)), rho, 6, 4, info)
    neg = b4[0] < 0
    info["b1"] = neg
    b0 = sqrt(-b4[0]) if neg else sqrt(b4[0])
    if b0 == 0.0:
        info["beta0"] = True
    if neg:
        return [b0, div(-b4[1], b0), div(-b4[2], b0), div(-b4[3], b0)]
    return [b0, div(b4[1], b0), div(b4[2], b0), div(b4[3], b0)]


def _b01(b, tag, info):
    neg = b[0] < 0
    if neg:
        b0 = sqrt(-b[0])
        b1 = sqrt(-b[2]) if b[2] < 0 else 0.0
        second = b[2] < 0
    else:
        b0 = sqrt(b[0])
        b1 = sqrt(b[2]) if b[2] > 0 else 0.0
        second = b[2] > 0
    flip = b[1] < 0
    if flip:
        b0 = -b0
    info[tag] = (neg, second, flip)
    return b0, b1


def betas_approx_2(L, rho, info):
    b3 = qr_solve(l_columns(L, (0, 1, 2)), rho, 6, 3, info)
    b0, b1 = _b01(b3, "b2", info)
    return [b0, b1, 0.0, 0.0]


def betas_approx_3(L, rho, info):
    b5 = qr_solve(l_columns(L, (0, 1, 2, 3, 4)), rho, 6, 5, info)
    b0, b1 = _b01(b5, "b3", info)
    if b0 == 0.0:
        info["beta0"] = True
    return [b0, b1, div(b5[3], b0), 0.0]


def gauss_newton(L, rho, betas, info):
    betas = list(betas)
    for _ in range(5):
        A = [0.0] * 24
        b = [0.0] * 6
        b0, b1, b2, b3 = betas
        for i in range(6):
            r = L[10 * i:10 * i + 10]
            A[4 * i] = 2 * r[0] * b0 + r[1] * b1 + r[3] * b2 + r[6] * b3
            A[4 * i + 1] = r[1] * b0 + 2 * r[2] * b1 + r[4] * b2 + r[7] * b3
            A[4 * i + 2] = r[3] * b0 + r[4] * b1 + 2 * r[5] * b2 + r[8] * b3
            A[4 * i + 3] = r[6] * b0 + r[7] * b1 + r[8] * b2 + 2 * r[9] * b3
            b[i] = rho[i] - (r[0] * b0 * b0 + r[1] * b0 * b1 + r[2] * b1 * b1 + r[3] * b0 * b2 + r[4] * b1 * b2 + r[5] * b2 * b2 +
                             r[6] * b0 * b3 + r[7] * b1 * b3 + r[8] * b2 * b3 + r[9] * b3 * b3)
        x = qr_solve(A, b, 6, 4, info)
        betas = [betas[i] + x[i] for i in range(4)]
    return betas


def epnp(pw, us, cam, info=None):
    """compute_pose (:477-525) over the selected correspondences: pw [n][3], us [n][2] doubles, cam = (fu, fv, uc, vc) doubles.
    -> (R [3][3], t [3], error, bad); bad: E8's first two clauses.  info collects which rule was reached (the scenes' tests)"""
    info = {} if info is None else info
    n = len(pw)
    fn = float(n)
    fu, fv, uc, vc = cam
    # choose_control_points (:375-409)
    c0 = [div(fsum([p[j] for p in pw]), fn) for j in range(3)]
    S = [[0.0] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(a, 3):
            S[a][b] = fsum([(p[a] - c0[a]) * (p[b] - c0[b]) for p in pw])
            S[b][a] = S[a][b]
    dc, V3, sw3 = jacobi(S, 3)
    col = order_desc(dc)
    cws = [c0]
    for i in range(1, 4):
        k = sqrt(div(dc[col[i - 1]], fn))
        cws.append([c0[j] + k * V3[j][col[i - 1]] for j in range(3)])
    # compute_barycentric_coordinates (:411-434)
    cc = [cws[j][i] - cws[0][i] for i in range(3) for j in range(1, 4)]
    ci = inv3(cc)

    def alphas(p):
        d0, d1, d2 = p[0] - c0[0], p[1] - c0[1], p[2] - c0[2]
        a = [0.0] + [ci[3 * j] * d0 + ci[3 * j + 1] * d1 + ci[3 * j + 2] * d2 for j in range(3)]
        a[0] = 1.0 - a[1] - a[2] - a[3]
        return a
    al = [alphas(p) for p in pw]   # recomputed where used on the device: the same bits
    # M^T M (:482-492), one pass per pair of alpha indices
    M = [[0.0] * 12 for _ in range(12)]
    du = [uc - u[0] for u in us]
    dv = [vc - u[1] for u in us]
    for i in range(4):
        for k in range(i, 4):
            Ai = [a[i] * fu for a in al]; Ak = [a[k] * fu for a in al]
            Bi = [a[i] * fv for a in al]; Bk = [a[k] * fv for a in al]
            Ci = [al[j][i] * du[j] for j in range(n)]; Ck = [al[j][k] * du[j] for j in range(n)]
            Di = [al[j][i] * dv[j] for j in range(n)]; Dk = [al[j][k] * dv[j] for j in range(n)]
            e = {(0, 0): fsum([Ai[j] * Ak[j] for j in range(n)]), (0, 2): fsum([Ai[j] * Ck[j] for j in range(n)]),
                 (1, 1): fsum([Bi[j] * Bk[j] for j in range(n)]), (1, 2): fsum([Bi[j] * Dk[j] for j in range(n)]),
                 (2, 2): fsum([Ci[j] * Ck[j] + Di[j] * Dk[j] for j in range(n)])}
            if i < k:
                e[(2, 0)] = fsum([Ci[j] * Ak[j] for j in range(n)])
                e[(2, 1)] = fsum([Di[j] * Bk[j] for j in range(n)])
            for (x, y), val in e.items():
                M[3 * i + x][3 * k + y] = val
                M[3 * k + y][3 * i + x] = val
    d12, V12, sw12 = jacobi(M, 12)
    info["mtm"], info["d12"], info["v12"], info["sweeps12"], info["sweeps3"], info["s3"], info["d3"], info["v3"] = M, d12, V12, sw12, sw3, S, dc, V3
    col12 = order_desc(d12)
    info["col12"] = col12
    v = [[V12[r][col12[11 - i]] for r in range(12)] for i in range(4)]   # v[i] = ut row 11 - i
    # compute_L_6x10 (:760-800), compute_rho (:802-810)
    dvv = [[None] * 6 for _ in range(4)]
    for i in range(4):
        a, b = 0, 1
        for j in range(6):
            dvv[i][j] = [v[i][3 * a] - v[i][3 * b], v[i][3 * a + 1] - v[i][3 * b + 1], v[i][3 * a + 2] - v[i][3 * b + 2]]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
    L = [0.0] * 60
    for i in range(6):
        d = [dvv[k][i] for k in range(4)]
        L[10 * i:10 * i + 10] = [dot3(d[0], d[0]), 2.0 * dot3(d[0], d[1]), dot3(d[1], d[1]), 2.0 * dot3(d[0], d[2]), 2.0 * dot3(d[1], d[2]),
                                 dot3(d[2], d[2]), 2.0 * dot3(d[0], d[3]), 2.0 * dot3(d[1], d[3]), 2.0 * dot3(d[2], d[3]), dot3(d[3], d[3])]
    rho = [dist2(cws[0], cws[1]), dist2(cws[0], cws[2]), dist2(cws[0], cws[3]), dist2(cws[1], cws[2]), dist2(cws[1], cws[3]),
           dist2(cws[2], cws[3])]

    def R_and_t(betas):
        """compute_R_and_t (:651-662)"""
        ccs = [[0.0] * 3 for _ in range(4)]
        for i in range(4):
            for j in range(4):
                for k in range(3):
                    ccs[j][k] = ccs[j][k] + betas[i] * v[i][3 * j + k]

        def pc_of(a):
            return [a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)]
        flip = pc_of(al[0])[2] < 0.0   # Q6
        if flip:
            ccs = [[-x for x in r] for r in ccs]
        pcs = [pc_of(a) for a in al]
        pc0 = [div(fsum([p[j] for p in pcs]), fn) for j in range(3)]
        pw0 = c0   # the same sum of the same shape
        A = [fsum([(pcs[q][j] - pc0[j]) * (pw[q][k] - pw0[k]) for q in range(n)]) for j in range(3) for k in range(3)]
        AtA = [[0.0] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(i, 3):
                AtA[i][j] = A[i] * A[j] + A[3 + i] * A[3 + j] + A[6 + i] * A[6 + j]
                AtA[j][i] = AtA[i][j]
        dd, VV, _ = jacobi(AtA, 3)
        cl = order_desc(dd)
        vk = [[VV[r][cl[k]] for r in range(3)] for k in range(3)]
        Av = [[A[3 * i] * w[0] + A[3 * i + 1] * w[1] + A[3 * i + 2] * w[2] for i in range(3)] for w in vk]
        uk = []
        for k in range(2):
            nrm = sqrt(Av[k][0] * Av[k][0] + Av[k][1] * Av[k][1] + Av[k][2] * Av[k][2])
            uk.append([div(Av[k][i], nrm) for i in range(3)])
        u0, u1 = uk
        u2 = [u0[1] * u1[2] - u0[2] * u1[1], u0[2] * u1[0] - u0[0] * u1[2], u0[0] * u1[1] - u0[1] * u1[0]]
        if dot3(Av[2], u2) < 0.0:
            vk[2] = [-x for x in vk[2]]
        U = [[u0[i], u1[i], u2[i]] for i in range(3)]
        Vr = [[vk[0][j], vk[1][j], vk[2][j]] for j in range(3)]
        R = [[dot3(U[i], Vr[j]) for j in range(3)] for i in range(3)]
        det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
               R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
        detfix = det < 0
        if detfix:
            R[2] = [-x for x in R[2]]
        t = [pc0[i] - dot3(R[i], pw0) for i in range(3)]
        errs = []
        for q in range(n):
            Xc = dot3(R[0], pw[q]) + t[0]
            Yc = dot3(R[1], pw[q]) + t[1]
            inv_Zc = div(1.0, dot3(R[2], pw[q]) + t[2])
            ue = uc + fu * Xc * inv_Zc
            ve = vc + fv * Yc * inv_Zc
            u, w = us[q]
            errs.append(sqrt((u - ue) * (u - ue) + (w - ve) * (w - ve)))
        return R, t, div(fsum(errs), fn), flip, detfix

    sols = []
    for approx in (betas_approx_1, betas_approx_2, betas_approx_3):
        sols.append(R_and_t(gauss_newton(L, rho, approx(L, rho, info), info)))
    win = 0
    for k in (1, 2):   # E8: an error that is not finite loses
        if finite(sols[k][2]) and (not finite(sols[win][2]) or sols[k][2] < sols[win][2]):
            win = k
    info["winner"], info["flips"], info["detfix"], info["errors"] = win + 1, [s[3] for s in sols], [s[4] for s in sols], [s[2] for s in sols]
    R, t, err = sols[win][:3]
    bad = bool(info.get("eta0") or info.get("beta0"))
    return R, t, err, bad


# ---- the constructor, SetRansacParameters ----

def min_inliers_rule(N, min_inliers, epsilon):
    """:134-139 with minSet = 4: the product in float, truncated (saturating at INT_MAX)"""
    with np.errstate(over="ignore"):
        prod = f32(N) * f32(epsilon)
    n_min = INT_MAX if not prod < f32(2147483648.0) else int(prod)
    return max(n_min, int(min_inliers), 4)


def gather(x, y, sigma2, pos, flags, pts, min_inliers, epsilon, th2):
    """the constructor (:67-110) + mvMaxError and mRansacMinInliers of SetRansacParameters.  x / y / sigma2: the frame's planes over its
    features; pos [P][3] float32 and flags [P] (SET | BAD): the store; pts: one id | -1 per feature"""
    idx = [i for i in range(len(pts)) if int(pts[i]) >= 0 and (int(flags[int(pts[i])]) & SET) and not (int(flags[int(pts[i])]) & BAD)]
    ids = [int(pts[i]) for i in idx]
    with np.errstate(all="ignore"):
        P = dict(n=len(idx), index=np.asarray(idx, np.int32).reshape(-1),
                 p2d=np.stack([np.asarray(x, f32)[idx], np.asarray(y, f32)[idx]], 1).reshape(-1, 2),
                 p3dw=np.asarray(pos, f32).reshape(-1, 3)[ids].reshape(-1, 3),
                 sigma2=np.asarray(sigma2, f32)[idx].reshape(-1))
        P["max_err"] = (P["sigma2"] * f32(th2)).astype(f32)
    P["min_inliers"] = min_inliers_rule(P["n"], min_inliers, epsilon)
    return P


def ransac_parameters(N, probability=0.99, minInliers=10, maxIterations=300, minSet=4, epsilon=0.5, th2=5.991):
    """:121-152 -> (mRansacMinInliers, mRansacEpsilon, nIterations as computed, mRansacMaxIts)"""
    n_min = max(min_inliers_rule(N, minInliers, epsilon), minSet)
    eps = f32(epsilon)
    with np.errstate(all="ignore"):
        ratio = f32(n_min) / f32(N)
    if eps < ratio:
        eps = ratio
    if n_min == N:
        n_it = 1
    else:
        e3 = float(eps) ** 3 if finite(float(eps)) else math.inf   # Q2
        arg = 1.0 - e3
        den = math.log(arg) if arg > 0 else (-math.inf if arg == 0 else math.nan)
        num = math.log(1.0 - probability) if probability < 1 else -math.inf
        val = div(num, den)
        # a double outside int's range is undefined in the reference: here it saturates and a NaN reads maxIterations
        n_it = int(maxIterations) if val != val else int(min(max(math.ceil(val) if finite(val) else val, -2 ** 31), INT_MAX))
    return n_min, eps, n_it, max(1, min(n_it, int(maxIterations)))


# ---- hypotheses ----

def sample4(seed, h, N):
    """E6 on vAvailableIndices (:188-201), literally"""
    key = sm(sm(seed & M64) ^ (h + 1))
    avail = list(range(N))
    picks = []
    for d in range(4):
        r = sm((key + (d + 1) * DRAW_STEP) & M64) % (N - d)
        picks.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return picks


def camera(fx, fy, cx, cy):
    return (float(f32(fx)), float(f32(fy)), float(f32(cx)), float(f32(cy)))


def check_inliers(R, t, P, cam):
    """:308-339 (Q5) -> bool [N]"""
    fu, fv, uc, vc = cam
    X = P["p3dw"].astype(np.float64)
    with np.errstate(all="ignore"):
        Xc = (R[0][0] * X[:, 0] + R[0][1] * X[:, 1] + R[0][2] * X[:, 2] + t[0]).astype(f32)
        Yc = (R[1][0] * X[:, 0] + R[1][1] * X[:, 1] + R[1][2] * X[:, 2] + t[1]).astype(f32)
        invZ = (1.0 / (R[2][0] * X[:, 0] + R[2][1] * X[:, 1] + R[2][2] * X[:, 2] + t[2])).astype(f32)
        ue = uc + fu * Xc.astype(np.float64) * invZ.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * invZ.astype(np.float64)
        dx = (P["p2d"][:, 0].astype(np.float64) - ue).astype(f32)
        dy = (P["p2d"][:, 1].astype(np.float64) - ve).astype(f32)
        e2 = dx * dx + dy * dy
        return e2 < P["max_err"]


def solve(P, sel, cam, info=None):
    """compute_pose on the selected correspondences + CheckInliers -> (count, degenerate, pose float32 [12], mask bool [N])"""
    pw = [[float(v) for v in P["p3dw"][i]] for i in sel]
    us = [[float(v) for v in P["p2d"][i]] for i in sel]
    R, t, _, bad = epnp(pw, us, cam, info)
    flat = [R[i][j] for i in range(3) for j in range(3)] + list(t)
    if bad or not all(finite(v) for v in flat):
        return 0, 1, np.zeros(12, f32), np.zeros(P["n"], bool)
    mask = check_inliers(R, t, P, cam)
    with np.errstate(over="ignore"):
        return int(mask.sum()), 0, np.asarray(flat, np.float64).astype(f32), mask


def pack(mask, mask_words):
    w = np.zeros(mask_words, np.uint32)
    for k in np.nonzero(mask)[0]:
        w[k >> 5] |= np.uint32(1 << (int(k) & 31))
    return w


def device_outputs(P, cam, seed, nhyp, mask_words, cap=None, trace=None):
    """what afv_frame_pnp_hypotheses answers for one candidate, from its gathered correspondences.  trace: a list that receives
    (h, "hyp" | "refine", info of epnp) per EPnP run"""
    N = P["n"]
    cap = N if cap is None else cap
    out = dict(n=N, min_inliers=P["min_inliers"], index=np.full(cap, -1, np.int32), count=np.zeros(nhyp, np.int32),
               degenerate=np.zeros(nhyp, np.uint8), pose=np.zeros((nhyp, 12), f32), inliers=np.zeros((nhyp, mask_words), np.uint32),
               refined=np.zeros(nhyp, np.uint8), refined_count=np.zeros(nhyp, np.int32), refined_pose=np.zeros((nhyp, 12), f32),
               refined_inliers=np.zeros((nhyp, mask_words), np.uint32), max_err=np.zeros(cap, f32), p3dw=np.zeros((cap, 3), f32))
    out["index"][:N] = P["index"]
    out["max_err"][:N] = P["max_err"]
    out["p3dw"][:N] = P["p3dw"]
    if N < 4:   # E9
        return out
    best = 0
    for h in range(nhyp):
        info = {}
        c, deg, pose, mask = solve(P, sample4(seed, h, N), cam, info)
        if trace is not None:
            trace.append((h, "hyp", info))
        out["count"][h], out["degenerate"][h], out["pose"][h], out["inliers"][h] = c, deg, pose, pack(mask, mask_words)
        if c >= P["min_inliers"] and c > best:   # a record
            best = c
            info = {}
            rc, rdeg, rpose, rmask = solve(P, list(np.nonzero(mask)[0]), cam, info)
            if trace is not None:
                trace.append((h, "refine", info))
            out["refined"][h] = 2 if rdeg else 1
            out["refined_count"][h], out["refined_pose"][h], out["refined_inliers"][h] = rc, rpose, pack(rmask, mask_words)
    return out


def Tcw(pose):
    T = np.eye(4, dtype=f32)
    T[:3, :3] = np.asarray(pose[:9], f32).reshape(3, 3)
    T[:3, 3] = pose[9:12]
    return T


class Solver:
    """PnPsolver as the reference writes it: the sequential loop, Refine at every qualifying hypothesis (Q4)"""

    def __init__(self, P, cam, seed, n_features):
        self.P, self.cam, self.seed, self.n_features = P, cam, seed, n_features
        self.N = P["n"]
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.best_mask = None
        self.best_T = None
        self.refines = 0
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        self.mRansacMinInliers, self.mRansacEpsilon, self.nIterations, self.mRansacMaxIts = ransac_parameters(
            self.N, probability, minInliers, maxIterations, minSet, epsilon, th2)
        with np.errstate(all="ignore"):
            self.P = dict(self.P, min_inliers=self.mRansacMinInliers, max_err=(self.P["sigma2"] * f32(th2)).astype(f32))

    def _vb(self, mask):
        vb = np.zeros(self.n_features, bool)
        vb[self.P["index"][:self.N][mask]] = True
        return vb

    def Refine(self):
        """:260-305"""
        self.refines += 1
        c, deg, pose, mask = solve(self.P, list(np.nonzero(self.best_mask)[0]), self.cam)
        self.mnRefinedInliers, self.refined_mask = c, mask
        if c > self.mRansacMinInliers:
            self.refined_T = Tcw(pose)
            return True
        return False

    def iterate(self, nIterations):
        """:165-258 -> (Tcw or None, bNoMore, vbInliers, nInliers)"""
        none = np.zeros(self.n_features, bool)
        if self.N < self.mRansacMinInliers:
            return None, True, none, 0
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:   # Q1
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            c, deg, pose, mask = solve(self.P, sample4(self.seed, h, self.N), self.cam)
            if c >= self.mRansacMinInliers:
                if c > self.mnBestInliers:
                    self.best_mask, self.mnBestInliers, self.best_T = mask, c, Tcw(pose)
                if self.Refine():
                    return self.refined_T.copy(), False, self._vb(self.refined_mask), self.mnRefinedInliers
        if self.mnIterations >= self.mRansacMaxIts:
            if self.mnBestInliers >= self.mRansacMinInliers:
                return self.best_T.copy(), True, self._vb(self.best_mask), self.mnBestInliers
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
