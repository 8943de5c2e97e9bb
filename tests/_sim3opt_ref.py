"""Normative restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1033-1226) and of the parts of g2o it runs, over slots of the keyframe
table and ids of the map-point store (afv_table_optimize_sim3, csrc/k_sim3opt.hip).  numpy float64, ONE rounding per operator (the
library is built with -ffp-contract=off; division and square root are correctly rounded on both sides), every operator order fixed here;
three-term sums are a0 + (a1 + a2).  The Levenberg pieces whose text is PoseOptimization's are imported from tests/_poseopt_ref.py.

g2o is an empty directory in the reference, so its arithmetic is restated after upstream g2o as bundled with ORB-SLAM2 - parity with a real
g2o is UNPINNED.  What is restated, by class and function:
  EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ :: computeError (types_seven_dof_expmap)                       -> edge_errors
  Sim3::map, Sim3::inverse, Sim3::operator*, Sim3::Sim3(Vector7) (the exponential, its four branches) (sim3.h)   -> sim3_map via project_error, inverse, compose, sim3_exp
  VertexSim3Expmap::oplusImpl (update[6] = 0 under _fix_scale), cam_map1 / cam_map2                               -> step, project_error
  BaseBinaryEdge::linearizeOplus (central differences, delta 1e-9, the non-fixed vertex only)                    -> perturbed, linearise
  BaseBinaryEdge::constructQuadraticForm, BaseEdge::chi2, RobustKernelHuber::robustify                           -> linearise, _poseopt_ref.huber
  OptimizationAlgorithmLevenberg::solve, computeLambdaInit, computeScale; SparseOptimizer::optimize              -> optimize
  LinearSolverDense (the 7 x 7 block)                                                                            -> solve_llt

The edge set (:1084-1163): feature i of keyframe 1 is a correspondence when mp2[i] >= 0 and mp1[i] >= 0, both ids are set in the store and
not bad, and idx2[i] >= 0.  P3D1c = R1w X1 + t1w and P3D2c = R2w X2 + t2w in float (a row as a0 + (a1 + a2), then + t), then cast to
double.  The observations are mvKeysUn[i] of slot 1 and mvKeysUn[idx2[i]] of slot 2, the informations inf1[i] * I and inf2[idx2[i]] * I,
the Huber delta (double)sqrtf(th2).  Quirk kept: a match that fails the filter is NOT removed from vpMatches1 - it is no edge.

The call: optimize(5); first classification, e12.chi2() > th2 || e21.chi2() > th2 removes both edges and the match; nMoreIterations = 10
if nBad > 0 else 5; nCorrespondences - nBad < 10 returns 0 (g2oS12 is not written back, the removals stand); optimize(nMoreIterations);
second classification removes matches only; nIn.  Each optimize() call starts its own Levenberg (lambda from computeLambdaInit at its
iteration 0); the Huber kernel is never removed.

The Jacobians are numeric, as BaseBinaryEdge leaves them: per linearisation 14 perturbed estimates Sim3(+-1e-9 e_d) * estimate, shared by
all edges; column d of an edge is (1 / (2 * 1e-9)) * (e(+d) - e(-d)).

Deliberate deviations from upstream:
  (O1) both classifications are made at the accepted estimate (upstream leaves an edge with the error of the last trial, rejected or not,
       when optimize() ends on a rejection) - P1 of PoseOptimization.
  (O2) a chi2 that is not finite is an outlier (upstream: NaN > th2 is false) - P2.
  (O3) the state is R (3 x 3), t and s in double; a step is R <- dR R, t <- ds (dR t) + dt, s <- ds s, no quaternion in between; the
       caller's R12 is taken as given, not re-normalised through a quaternion - P3.
  (O4) no library sin / cos / exp on either side.  sin(th)/th, (1 - cos th)/th^2, (th - sin th)/th^3 are PoseOptimization's EXP_A / EXP_B /
       EXP_C (16-term Horner polynomials in th^2; accuracy: P4 there); sin th = th * A(th^2), cos th = 1 - th^2 * B(th^2), th = sqrt(th^2).
       exp(sigma) = 2^k * P(r): k = floor(sigma * LOG2E + 0.5), r = (sigma - k * LN2_HI) - k * LN2_LO (|r| <= 0.347), P = the Taylor
       polynomial of degree 13 by Horner (EXP_T[n] = 1 / n! correctly rounded; the first dropped term is < 2^-57), the power of two applied
       exactly (ldexp).  Measured against math.exp over |sigma| <= 64 (the range a step can take, below): at most 1 ulp
       (tests/test_sim3opt_ref_cpu.py measures it and asserts 2).  A step with th^2 > pi^2 (or not comparable), or a sigma that is not
       finite or beyond 64 in magnitude, is a failed trial.
  (O5) every sum over the correspondences (28 + 7 + 1 values per linearisation, 1 per trial) has one fixed shape - PnPsolver's E7: 64
       partial sums, partial l starts at +0.0 and adds the terms of the correspondences l, l + 64, ... (positions in the edge list) in
       ascending order, the term of a correspondence being e12's term + e21's term, a removed correspondence adding nothing; then
       p[l] += p[l + s] for s = 32 .. 1.  One wavefront evaluates it without a barrier.
  (O6) the 7 x 7 solve is an unpivoted L L^T in a fixed loop order; a pivot that is not positive and finite is a failed trial.  Under
       fix_scale the two perturbed estimates of the scale are the estimate itself (exp(0) is exact), the scale column of every Jacobian is
       exactly zero, row 6 of H holds lambda alone, x[6] = 0 and the scale's bits never change.
  (O7) a problem without (remaining) edges evaluates nothing: optimize() returns the estimate with 0 iterations, chi2 0 and lambda 0.
A failed trial (O4, O6) is a rejected trial whatever rho would have been: the estimate is restored, lambda *= ni, ni *= 2, and the trial
loop goes on as for rho < 0.
"""
import math
from fractions import Fraction

import numpy as np

import _sim3_ref as S3
from _poseopt_ref import DBL_MAX, EXP_A, EXP_B, EXP_C, F64, GOOD_LOW, GOOD_UP, MAX_TRIALS, PI2, TAU, horner, huber

SET, BAD = S3.SET, S3.BAD
EPS = F64(0.00001)                                    # Sim3(Vector7): the branches on |sigma| < eps and theta < eps
DELTA = F64(1e-9)                                     # BaseBinaryEdge::linearizeOplus
SCALAR = F64(1.0) / (F64(2.0) * DELTA)
SIGMA_MAX = F64(64.0)
LOG2E = F64(float.fromhex("0x1.71547652b82fep+0"))
LN2_HI = F64(float.fromhex("0x1.62e42fee00000p-1"))
LN2_LO = F64(float.fromhex("0x1.a39ef35793c76p-33"))
EXP_T = [float(Fraction(1, math.factorial(n))) for n in range(14)]  # the kernel holds them as hexadecimal literals, digit for digit
MIN_CORRESPONDENCES, ITERATIONS_FIRST, MORE_HIGH, MORE_LOW = 10, 5, 10, 5
NO_MATCH, NOT_EDGE, KEPT, REMOVED_FIRST, REMOVED_SECOND = 0, 1, 2, 3, 4


def exp_sigma(x):
    """O4: exp of a finite |x| <= 64"""
    x = F64(x)
    kf = np.floor(x * LOG2E + F64(0.5))
    r = (x - kf * LN2_HI) - kf * LN2_LO
    p = F64(EXP_T[13])
    for c in EXP_T[12::-1]:
        p = p * r + F64(c)
    return F64(np.ldexp(p, int(kf)))


def sim3_exp(u):
    """Sim3::Sim3(const Vector7 &update), update = (omega, upsilon, sigma); O3, O4.  Returns (dR, dt, ds) or None for a failed trial"""
    w0, w1, w2, u0, u1, u2, sg = (F64(v) for v in u)
    with np.errstate(all="ignore"):
        if not (np.abs(sg) <= SIGMA_MAX):
            return None
        t2 = w0 * w0 + (w1 * w1 + w2 * w2)
        if not (t2 <= PI2):
            return None
        theta = np.sqrt(t2)
        s = exp_sigma(sg)
        hA, hB, hC = horner(EXP_A, t2), horner(EXP_B, t2), horner(EXP_C, t2)
        one = F64(1.0)
        if np.abs(sg) < EPS:
            C = one
            if theta < EPS:
                A, B, ra, rb = F64(0.5), one / F64(6.0), one, one    # R = I + Omega + Omega2, as written upstream
            else:
                A, B, ra, rb = hB, hC, hA, hB
        else:
            C = (s - one) / sg
            sg2 = sg * sg
            if theta < EPS:
                A = ((sg - one) * s + one) / sg2
                B = (((F64(0.5) * sg2 - sg) + one) * s) / (sg2 * sg)  # as written upstream (no "- 1")
                ra, rb = one, one
            else:
                ra, rb = hA, hB
                a = s * (theta * hA)                                   # s sin(theta)
                b = s * (one - t2 * hB)                                # s cos(theta)
                c = t2 + sg2
                A = (a * sg + (one - b) * theta) / (theta * c)
                B = (C - ((b - one) * sg + a * theta) / c) * (one / t2)
        Z = F64(0.0)
        W = [[Z, -w2, w1], [w2, Z, -w0], [-w1, w0, Z]]
        W2 = [[-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2],
              [w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2],
              [w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)]]
        dR = [[(one + rb * W2[i][j]) if i == j else (ra * W[i][j] + rb * W2[i][j]) for j in range(3)] for i in range(3)]
        Wm = [[(C + B * W2[i][j]) if i == j else (A * W[i][j] + B * W2[i][j]) for j in range(3)] for i in range(3)]
        dt = [Wm[i][0] * u0 + (Wm[i][1] * u1 + Wm[i][2] * u2) for i in range(3)]
    return dR, dt, s


def compose(dR, dt, ds, E):
    """Sim3::operator*: (dR, dt, ds) * E"""
    R, t, s = E
    Rn, tn = np.empty((3, 3), F64), np.empty(3, F64)
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(3):
                Rn[i, j] = dR[i][0] * R[0, j] + (dR[i][1] * R[1, j] + dR[i][2] * R[2, j])
            tn[i] = ds * (dR[i][0] * t[0] + (dR[i][1] * t[1] + dR[i][2] * t[2])) + dt[i]
        sn = ds * s
    return Rn, tn, F64(sn)


def inverse(E):
    """Sim3::inverse: (R^T, R^T (t * (-1 / s)), 1 / s)"""
    R, t, s = E
    with np.errstate(all="ignore"):
        m = F64(-1.0) / s
        tm = [t[0] * m, t[1] * m, t[2] * m]
        ti = np.array([R[0, i] * tm[0] + (R[1, i] * tm[1] + R[2, i] * tm[2]) for i in range(3)], F64)
        si = F64(1.0) / s
    return np.ascontiguousarray(R.T), ti, F64(si)


def step(E, x, fix_scale):
    """VertexSim3Expmap::oplusImpl: Sim3(update) * estimate, update[6] = 0 under fix_scale.  None: a failed trial"""
    u = [F64(v) for v in x]
    if fix_scale:
        u[6] = F64(0.0)
    d = sim3_exp(u)
    return None if d is None else compose(d[0], d[1], d[2], E)


class Problem:
    """the edges of one call as float64 arrays over the n correspondences, in ascending feature order"""

    def __init__(self, cam1, cam2, pos, flags, x1, y1, inf1, x2, y2, inf2, mp1, mp2, idx2, th2, fix_scale):
        f32 = np.float32
        self.n1 = n1 = len(mp1)
        self.mp2 = np.asarray(mp2, np.int64)
        idx, p1, p2, o1, o2, i1, i2 = [], [], [], [], [], [], []
        for i in range(n1):
            a, b, k2 = int(mp1[i]), int(mp2[i]), int(idx2[i])
            if b < 0 or a < 0:
                continue
            if not (int(flags[a]) & SET) or (int(flags[a]) & BAD) or not (int(flags[b]) & SET) or (int(flags[b]) & BAD) or k2 < 0:
                continue
            idx.append(i)
            with np.errstate(all="ignore"):
                p1.append(S3.rigid(cam1.Rcw, cam1.tcw, [f32(v) for v in pos[a]]))
                p2.append(S3.rigid(cam2.Rcw, cam2.tcw, [f32(v) for v in pos[b]]))
            o1.append([f32(x1[i]), f32(y1[i])])
            o2.append([f32(x2[k2]), f32(y2[k2])])
            i1.append(f32(inf1[i]))
            i2.append(f32(inf2[k2]))
        self.index1 = np.array(idx, np.int64)
        self.n = n = len(idx)
        self.p1 = np.array(p1, np.float32).reshape(n, 3).astype(F64)
        self.p2 = np.array(p2, np.float32).reshape(n, 3).astype(F64)
        self.obs1 = np.array(o1, np.float32).reshape(n, 2).astype(F64)
        self.obs2 = np.array(o2, np.float32).reshape(n, 2).astype(F64)
        self.inf1, self.inf2 = np.array(i1, np.float32).astype(F64), np.array(i2, np.float32).astype(F64)
        self.K1 = tuple(F64(f32(getattr(cam1, k))) for k in ("fx", "fy", "cx", "cy"))
        self.K2 = tuple(F64(f32(getattr(cam2, k))) for k in ("fx", "fy", "cx", "cy"))
        self.th2 = F64(f32(th2))                               # chi2 > th2 promotes the float
        self.delta = F64(np.sqrt(f32(th2)))                   # const float deltaHuber = sqrt(th2); setDelta takes a double
        self.fix_scale = bool(fix_scale)


def lane_sum(v, active):
    """O5"""
    n = len(v)
    rows = (n + 63) // 64
    a = np.zeros(max(rows, 1) * 64, F64)
    with np.errstate(all="ignore"):
        a[:n] = np.where(active, v, F64(0.0))                 # + 0.0 is exactly neutral: no partial is ever -0.0
        a = a.reshape(-1, 64)
        p = np.zeros(64, F64)
        for r in range(a.shape[0]):
            p = p + a[r]
        s = 32
        while s >= 1:
            p[:s] = p[:s] + p[s:2 * s]
            s >>= 1
    return F64(p[0])


def project_error(R, t, s, X, obs, K):
    """obs - cam_map(project(Sim3(R, t, s).map(X))), Sim3::map = s (R x) + t"""
    fx, fy, cx, cy = K
    with np.errstate(all="ignore"):
        q = [s * (R[r, 0] * X[:, 0] + (R[r, 1] * X[:, 1] + R[r, 2] * X[:, 2])) + t[r] for r in range(3)]
        u = fx * (q[0] / q[2]) + cx
        v = fy * (q[1] / q[2]) + cy
        return obs[:, 0] - u, obs[:, 1] - v


def edge_errors(pr, E):
    """computeError of both edges of every correspondence: (e12, e21), each (e0, e1)"""
    Ri, ti, si = inverse(E)
    return project_error(E[0], E[1], E[2], pr.p2, pr.obs1, pr.K1), project_error(Ri, ti, si, pr.p1, pr.obs2, pr.K2)


def chi2_of(e, inf):
    with np.errstate(all="ignore"):
        return e[0] * (inf * e[0]) + e[1] * (inf * e[1])


def edge_chi2(pr, E):
    e12, e21 = edge_errors(pr, E)
    return chi2_of(e12, pr.inf1), chi2_of(e21, pr.inf2)


def robust_chi2(pr, E, active):
    c12, c21 = edge_chi2(pr, E)
    with np.errstate(all="ignore"):
        return lane_sum(huber(pr, c12, True)[0] + huber(pr, c21, True)[0], active)


def perturbed(E, fix_scale):
    """the 14 estimates of a linearisation: [(plus_d, minus_d) for d in 0 .. 6]"""
    out = []
    for d in range(7):
        pair = []
        for sign in (DELTA, -DELTA):
            u = [F64(0.0)] * 7
            u[d] = sign
            pair.append(step(E, u, fix_scale))
        out.append(tuple(pair))
    return out


def jacobians(pr, E):
    """J12[r][d], J21[r][d] over the correspondences (r = 0, 1; d = 0 .. 6)"""
    J12 = [[None] * 7 for _ in range(2)]
    J21 = [[None] * 7 for _ in range(2)]
    for d, (Ep, Em) in enumerate(perturbed(E, pr.fix_scale)):
        p12, p21 = edge_errors(pr, Ep)
        m12, m21 = edge_errors(pr, Em)
        with np.errstate(all="ignore"):
            for r in range(2):
                J12[r][d] = SCALAR * (p12[r] - m12[r])
                J21[r][d] = SCALAR * (p21[r] - m21[r])
    return J12, J21


def linearise(pr, E, active):
    """computeActiveErrors + activeRobustChi2 + buildSystem: H (upper triangle mirrored), b, the robust chi2"""
    e12, e21 = edge_errors(pr, E)
    c12, c21 = chi2_of(e12, pr.inf1), chi2_of(e21, pr.inf2)
    r12, r21 = huber(pr, c12, True), huber(pr, c21, True)
    J12, J21 = jacobians(pr, E)
    H, b = np.zeros((7, 7), F64), np.zeros(7, F64)
    with np.errstate(all="ignore"):
        w12, w21 = r12[1] * pr.inf1, r21[1] * pr.inf2                 # robustInformation: rho[1] * Omega
        g12 = [r12[1] * -(pr.inf1 * e12[k]) for k in range(2)]        # rho[1] * (-Omega e)
        g21 = [r21[1] * -(pr.inf2 * e21[k]) for k in range(2)]
        for i in range(7):
            for j in range(i, 7):
                h12 = J12[0][i] * (w12 * J12[0][j]) + J12[1][i] * (w12 * J12[1][j])
                h21 = J21[0][i] * (w21 * J21[0][j]) + J21[1][i] * (w21 * J21[1][j])
                H[i, j] = H[j, i] = lane_sum(h12 + h21, active)
        for j in range(7):
            b[j] = lane_sum((J12[0][j] * g12[0] + J12[1][j] * g12[1]) + (J21[0][j] * g21[0] + J21[1][j] * g21[1]), active)
        chi = lane_sum(r12[0] + r21[0], active)
    return H, b, chi


def solve_llt(H, b, lam, n=7):
    """(H + lam I) x = b by an unpivoted L L^T in a fixed loop order (O6); None when a pivot is not positive and finite"""
    L = np.zeros((n, n), F64)
    with np.errstate(all="ignore"):
        for j in range(n):
            s = H[j, j] + lam
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0.0 and np.isfinite(s)):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                s = H[j, i]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        yv = np.zeros(n, F64)
        for i in range(n):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * yv[k]
            yv[i] = s / L[i, i]
        x = np.zeros(n, F64)
        for i in range(n - 1, -1, -1):
            s = yv[i]
            for k in range(i + 1, n):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x


def optimize(pr, E0, active, iterations, log=None):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve.  Returns (E, iterations, trials, chi2, lambda).
    log (a list) receives one dict per trial: what the CPU tests assert on."""
    E = (E0[0].copy(), E0[1].copy(), F64(E0[2]))
    if not active.any():                                               # O7
        return E, 0, 0, F64(0.0), F64(0.0)
    lam, ni = F64(0.0), F64(2.0)
    done = trials = 0
    cur = F64(0.0)
    for it in range(iterations):
        H, b, cur = linearise(pr, E, active)
        if it == 0:
            m = np.abs(H[0, 0])                                        # computeLambdaInit: tau * max |H_jj|
            for j in range(1, 7):
                a = np.abs(H[j, j])
                m = a if a > m else m
            lam, ni = TAU * m, F64(2.0)
        done += 1
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            x = solve_llt(H, b, lam)
            st = step(E, x, pr.fix_scale) if x is not None else None
            failed = st is None
            why = "pivot" if x is None else ("exp" if failed else "")
            accepted = False
            with np.errstate(all="ignore"):
                if failed:
                    rho, temp = F64(-1.0), F64(DBL_MAX)
                else:
                    temp = robust_chi2(pr, st, active)
                    scale = F64(0.0)
                    for j in range(7):
                        scale = scale + x[j] * (lam * x[j] + b[j])     # computeScale
                    scale = scale + F64(1e-3)
                    rho = (cur - temp) / scale
                    accepted = bool(rho > 0.0 and np.isfinite(temp))
                if log is not None:
                    log.append(dict(iteration=it, trial=qmax, failed=failed, why=why, accepted=accepted, rho=rho, before=cur, after=temp, lam=lam))
                if accepted:
                    q = F64(2.0) * rho - F64(1.0)
                    alpha = F64(1.0) - (q * q) * q
                    alpha = GOOD_UP if GOOD_UP < alpha else alpha
                    factor = alpha if GOOD_LOW < alpha else GOOD_LOW
                    lam = lam * factor
                    ni = F64(2.0)
                    cur = temp
                    E = st
                else:
                    lam = lam * ni
                    ni = ni * F64(2.0)
            qmax += 1
            if not (rho < 0.0 and qmax < MAX_TRIALS):
                break
        if qmax == MAX_TRIALS or rho == 0.0:
            if log is not None:
                log.append(dict(terminate="qmax" if qmax == MAX_TRIALS else "rho0", iteration=it))
            break
    return E, done, trials, cur, lam


def outliers(pr, E):
    """O1, O2: e12.chi2() > th2 || e21.chi2() > th2 at the accepted estimate; not finite counts as an outlier"""
    c12, c21 = edge_chi2(pr, E)
    with np.errstate(all="ignore"):
        return ~np.isfinite(c12) | (c12 > pr.th2) | ~np.isfinite(c21) | (c21 > pr.th2), c12, c21


class Result:
    pass


def optimize_sim3(pr, R12, t12, s12, log=None):
    """Optimizer::OptimizeSim3.  R12 [9], t12 [3], s12 float32 (what Sim3Solver::GetEstimated* return).  Returns a Result: n_in, n_corr,
    n_bad, more_iterations, early, R12 [9] / t12 [3] / s12 float64, iterations[2], trials[2] int32, chi2[2], lam[2] float64, state[n1] uint8,
    mp2_out[n1] (vpMatches1 after the call, -1 = NULL)."""
    f32 = np.float32
    E0 = (np.asarray(R12, f32).reshape(3, 3).astype(F64), np.asarray(t12, f32).reshape(3).astype(F64), F64(f32(s12)))
    res = Result()
    res.n_corr, res.n_bad, res.n_in, res.early, res.more_iterations = pr.n, 0, 0, 0, 0
    res.iterations, res.trials = np.zeros(2, np.int32), np.zeros(2, np.int32)
    res.chi2, res.lam = np.zeros(2, F64), np.zeros(2, F64)
    state = np.where(pr.mp2 >= 0, NOT_EDGE, NO_MATCH).astype(np.uint8)
    state[pr.index1] = KEPT
    active = np.ones(pr.n, bool)
    logs = [[], []]
    E1, res.iterations[0], res.trials[0], res.chi2[0], res.lam[0] = optimize(pr, E0, active, ITERATIONS_FIRST, logs[0])
    bad, c12, c21 = outliers(pr, E1)
    res.first_chi2 = (c12, c21)                                        # (for the CPU tests: what the first classification compared)
    res.n_bad = int(bad.sum())
    state[pr.index1[bad]] = REMOVED_FIRST
    active = active & ~bad
    res.more_iterations = MORE_HIGH if res.n_bad > 0 else MORE_LOW
    E = E0
    if pr.n - res.n_bad < MIN_CORRESPONDENCES:
        res.early = 1
    else:
        E, res.iterations[1], res.trials[1], res.chi2[1], res.lam[1] = optimize(pr, E1, active, res.more_iterations, logs[1])
        bad2, c12, c21 = outliers(pr, E)
        res.second_chi2 = (c12, c21)
        bad2 = bad2 & active
        state[pr.index1[bad2]] = REMOVED_SECOND
        res.n_in = int((active & ~bad2).sum())
    if log is not None:
        log.extend(logs)
    res.R12, res.t12, res.s12 = E[0].reshape(9).copy(), E[1].copy(), F64(E[2])
    res.state = state
    res.mp2_out = np.where((state == REMOVED_FIRST) | (state == REMOVED_SECOND), -1, pr.mp2).astype(np.int32)
    return res
