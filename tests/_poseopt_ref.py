"""Normative restatement of Optimizer::PoseOptimization (src/Optimizer.cc:245-448) and of the parts of g2o it runs, for a resident frame
(afv_frame_pose_optimize, csrc/k_poseopt.hip).  numpy float64, ONE rounding per operator (the library is built with -ffp-contract=off;
division and square root are correctly rounded on both sides), every operator order fixed here; three-term sums are a0 + (a1 + a2).

g2o is an empty directory in the reference, so its arithmetic is restated after upstream g2o as bundled with ORB-SLAM2 - parity with a real
g2o is UNPINNED.  What is restated, by class and function:
  EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose :: computeError, linearizeOplus (types_six_dof_expmap) -> edge_error, edge_jacobian
  BaseUnaryEdge::constructQuadraticForm, BaseEdge::chi2, RobustKernelHuber::robustify                                -> huber, linearise
  OptimizationAlgorithmLevenberg::solve, computeLambdaInit, computeScale; SparseOptimizer::optimize                  -> optimize_round
  LinearSolverDense (the 6 x 6 pose block), VertexSE3Expmap::oplusImpl, SE3Quat::exp                                 -> solve6, exp_step

Edges (Optimizer.cc:279-358): feature i is an edge when pts[i] >= 0 and that id was set in the store (a never-set id is no point; isBad is
not consulted, :282).  mvuRight[i] < 0: a mono edge, 2 residuals, delta = sqrtf(5.991f), threshold 5.991f; else stereo, 3 residuals,
bf = mbf, sqrtf(7.815f), 7.815f.  The information is keyPtsInf[i] * I (Frame.cc:709-725).  nInitialCorrespondences < 3: returns 0, the pose
stays, no flag is set (:362).  The error is evaluated in double throughout: e = obs - (fx * (x / z) + cx, fy * (y / z) + cy [, u - bf / z]).
A mono edge's third terms are +0.0 in every three-term sum.

Rounds (:372-440): four, each from the frame's INITIAL pose (:375) over the edges not flagged by the round before; after each, every edge
is classified with (float)chi2 > threshold (:386-403); the Huber kernel is removed after the classification of round 2 (:405-406); fewer
than 10 edges: one round (:438).  Output: the last round's pose as 12 floats, mvbOutlier, nInitialCorrespondences - nBad.

Deliberate deviations from upstream:
  (P1) every edge is classified at the round's final ACCEPTED pose (upstream leaves an inlier edge with the error of the last trial,
       rejected or not, when the call ends on a rejection).
  (P2) a chi2 that is not finite is an outlier (upstream: NaN > th is false).
  (P3) the state is R (3 x 3) and t in double; a step is R <- dR R, t <- dR t + V upsilon, no quaternion in between.
  (P4) the coefficients of the exponential map, sin(th)/th, (1 - cos th)/th^2, (th - sin th)/th^3, are fixed-length Horner polynomials in
       th^2 (EXP_A / EXP_B / EXP_C below, 16 terms: the first dropped term is < 2^-59 at th = pi; the kernel copies the tables digit for
       digit); neither side calls a library sin or cos.  A step with th^2 > pi^2 is a failed trial.  Accuracy, measured against the exact
       series in ulps of the value: (1 - cos th)/th^2 2.9 and (th - sin th)/th^3 1.6 over [0, pi] - within 4 ulp; sin(th)/th 2.3 up to
       th = 2 - within 4 ulp - but 5.8 at 2.5, 29 at 3.0, 88 at 3.1 and unbounded at pi, where it crosses zero while its alternating series
       still has terms of size 1.6: beyond th = 2 it is within 2^-52 ABSOLUTE (measured 1.9e-16), not within 4 ulp of its value.
  (P5) every sum over the edges (21 + 6 + 1 values per linearisation, 1 per trial) is a perfect binary tree over the feature index with
       P leaves, P the smallest power of two >= max(N, 1); a feature that is no active edge is +0.0, and every leaf is its value + 0.0 (no
       leaf is -0.0, so zero padding of the tree to any larger power of two is exactly neutral).  The 6 x 6 solve is an unpivoted L L^T in a
       fixed loop order; a pivot that is not positive and finite is a failed trial.  A round with no active edge leaves the pose as it is.
A failed trial (P4, P5) is a rejected trial whatever rho would have been: the pose is restored, lambda *= ni, ni *= 2, and the trial loop
goes on as for rho < 0.
"""
import numpy as np

F64 = np.float64
TH_MONO, TH_STEREO = np.float32(5.991), np.float32(7.815)            # chi2_2dof, chi2_3dof
DELTA_MONO, DELTA_STEREO = F64(np.sqrt(TH_MONO)), F64(np.sqrt(TH_STEREO))  # thHuber_2dof / _3dof: sqrtf in float, then a double (setDelta)
TAU = F64(1e-5)
PI2 = F64(float.fromhex("0x1.3bd3cc9be45dep+3"))  # (double)pi * (double)pi
GOOD_LOW, GOOD_UP = F64(1.0) / F64(3.0), F64(2.0) / F64(3.0)
MAX_TRIALS, ITERATIONS, ROUNDS = 10, 10, 4
DBL_MAX = np.finfo(np.float64).max

_h = float.fromhex
EXP_A = [_h(s) for s in ("0x1.0000000000000p+0", "-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19",
                         "-0x1.ae64567f544e4p-26", "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41", "0x1.952c77030ad4ap-49", "-0x1.2f49b46814157p-57",
                         "0x1.71b8ef6dcf572p-66", "-0x1.761b41316381ap-75", "0x1.3f3ccdd165fa9p-84", "-0x1.d1ab1c2dccea3p-94", "0x1.259f98b4358adp-103",
                         "-0x1.434d2e783f5bcp-113")]
EXP_B = [_h(s) for s in ("0x1.0000000000000p-1", "-0x1.5555555555555p-5", "0x1.6c16c16c16c17p-10", "-0x1.a01a01a01a01ap-16", "0x1.27e4fb7789f5cp-22",
                         "-0x1.1eed8eff8d898p-29", "0x1.93974a8c07c9dp-37", "-0x1.ae7f3e733b81fp-45", "0x1.6827863b97d97p-53", "-0x1.e542ba4020225p-62",
                         "0x1.0ce396db7f853p-70", "-0x1.f2cf01972f578p-80", "0x1.88e85fc6a4e5ap-89", "-0x1.0a18a2635085dp-98", "0x1.3932c5047d60ep-108",
                         "-0x1.434d2e783f5bcp-118")]
EXP_C = [_h(s) for s in ("0x1.5555555555555p-3", "-0x1.1111111111111p-7", "0x1.a01a01a01a01ap-13", "-0x1.71de3a556c734p-19", "0x1.ae64567f544e4p-26",
                         "-0x1.6124613a86d09p-33", "0x1.ae7f3e733b81fp-41", "-0x1.952c77030ad4ap-49", "0x1.2f49b46814157p-57", "-0x1.71b8ef6dcf572p-66",
                         "0x1.761b41316381ap-75", "-0x1.3f3ccdd165fa9p-84", "0x1.d1ab1c2dccea3p-94", "-0x1.259f98b4358adp-103", "0x1.434d2e783f5bcp-113",
                         "-0x1.3981254dd0d52p-123")]


def horner(table, t2):
    r = F64(table[-1])
    for c in table[-2::-1]:
        r = r * t2 + F64(c)
    return r


def exp_step(R, t, x):
    """VertexSE3Expmap::oplusImpl: setEstimate(SE3Quat::exp(update) * estimate()), update = (omega, upsilon); P3, P4.
    Returns (R', t') or None for a failed trial (th^2 > pi^2)."""
    w0, w1, w2, u0, u1, u2 = (F64(v) for v in x)
    t2 = w0 * w0 + (w1 * w1 + w2 * w2)
    if t2 > PI2:
        return None
    A, B, Cc = horner(EXP_A, t2), horner(EXP_B, t2), horner(EXP_C, t2)
    Z = F64(0.0)
    W = [[Z, -w2, w1], [w2, Z, -w0], [-w1, w0, Z]]                 # skew(omega)
    W2 = [[-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2],                 # skew(omega)^2
          [w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2],
          [w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)]]
    dR = [[(F64(1.0) + B * W2[i][j]) if i == j else (A * W[i][j] + B * W2[i][j]) for j in range(3)] for i in range(3)]
    V = [[(F64(1.0) + Cc * W2[i][j]) if i == j else (B * W[i][j] + Cc * W2[i][j]) for j in range(3)] for i in range(3)]
    u = (u0, u1, u2)
    Rn = np.empty((3, 3), F64)
    tn = np.empty(3, F64)
    for i in range(3):
        for j in range(3):
            Rn[i, j] = dR[i][0] * R[0, j] + (dR[i][1] * R[1, j] + dR[i][2] * R[2, j])
        tn[i] = (dR[i][0] * t[0] + (dR[i][1] * t[1] + dR[i][2] * t[2])) + (V[i][0] * u[0] + (V[i][1] * u[1] + V[i][2] * u[2]))
    return Rn, tn


class Problem:
    """the edges of one call, as float64 arrays over the N features"""

    def __init__(self, x, y, u_right, inf, pts, store_pos, store_set, fx, fy, cx, cy, mbf):
        pts = np.asarray(pts, np.int64).reshape(-1)
        self.N = N = len(pts)
        cap = len(store_set)
        assert np.all(pts < cap)
        safe = np.clip(pts, 0, None)
        self.edge = (pts >= 0) & (np.asarray(store_set, bool)[safe] if cap else np.zeros(N, bool))
        ur = np.asarray(u_right, np.float32).reshape(-1)
        self.stereo = ~(ur < np.float32(0.0))                     # mvuRight[i] < 0: mono (:285)
        pos = np.asarray(store_pos, np.float32).reshape(-1, 3)[safe] if cap else np.zeros((N, 3), np.float32)
        self.X, self.Y, self.Z = (pos[:, k].astype(F64) for k in range(3))
        self.ox, self.oy, self.our = np.asarray(x, np.float32).astype(F64), np.asarray(y, np.float32).astype(F64), ur.astype(F64)
        self.inf = np.asarray(inf, np.float32).astype(F64)
        self.fx, self.fy, self.cx, self.cy, self.bf = (F64(np.float32(v)) for v in (fx, fy, cx, cy, mbf))
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.th = np.where(self.stereo, TH_STEREO, TH_MONO).astype(np.float32)
        self.P = 1
        while self.P < max(N, 1):
            self.P *= 2


def tree_sum(pr, leaf, active):
    """P5: leaf[i] + 0.0 for an active edge, +0.0 otherwise, summed as a perfect binary tree over the feature index"""
    a = np.zeros(pr.P, F64)
    with np.errstate(all="ignore"):
        a[:pr.N] = np.where(active, leaf + F64(0.0), F64(0.0))
        while len(a) > 1:
            a = a[0::2] + a[1::2]
    return F64(a[0])


def camera_point(pr, R, t):
    x = (R[0, 0] * pr.X + (R[0, 1] * pr.Y + R[0, 2] * pr.Z)) + t[0]
    y = (R[1, 0] * pr.X + (R[1, 1] * pr.Y + R[1, 2] * pr.Z)) + t[1]
    z = (R[2, 0] * pr.X + (R[2, 1] * pr.Y + R[2, 2] * pr.Z)) + t[2]
    return x, y, z


def edge_error(pr, R, t):
    """computeError of both edge types: (e0, e1, e2) with e2 = +0.0 on a mono edge, and chi2 = e^T (inf I) e (BaseEdge::chi2)"""
    with np.errstate(all="ignore"):
        x, y, z = camera_point(pr, R, t)
        px = pr.fx * (x / z) + pr.cx
        py = pr.fy * (y / z) + pr.cy
        e0 = pr.ox - px
        e1 = pr.oy - py
        e2 = np.where(pr.stereo, pr.our - (px - pr.bf / z), F64(0.0))
        c2 = np.where(pr.stereo, e2 * (pr.inf * e2), F64(0.0))
        chi2 = e0 * (pr.inf * e0) + (e1 * (pr.inf * e1) + c2)
    return (e0, e1, e2), chi2


def huber(pr, chi2, robust):
    """RobustKernelHuber::robustify: (rho[0], rho[1]); without a kernel (chi2, 1)"""
    if not robust:
        return chi2, np.ones_like(chi2)
    with np.errstate(all="ignore"):
        dsqr = pr.delta * pr.delta
        s = np.sqrt(chi2)
        inl = chi2 <= dsqr
        rho0 = np.where(inl, chi2, (F64(2.0) * s) * pr.delta - dsqr)
        rho1 = np.where(inl, F64(1.0), pr.delta / s)
    return rho0, rho1


def edge_jacobian(pr, R, t):
    """linearizeOplus of both edge types: J[k][j], rotation columns first; row 2 is read on stereo edges only"""
    with np.errstate(all="ignore"):
        x, y, z = camera_point(pr, R, t)
        invz = F64(1.0) / z
        invz2 = invz * invz
        fx, fy, bf = pr.fx, pr.fy, pr.bf
        zero = np.zeros_like(x)
        J0 = [((x * y) * invz2) * fx, -((F64(1.0) + (x * x) * invz2) * fx), (y * invz) * fx, -(invz * fx), zero, (x * invz2) * fx]
        J1 = [(F64(1.0) + (y * y) * invz2) * fy, -(((x * y) * invz2) * fy), -((x * invz) * fy), zero, -(invz * fy), (y * invz2) * fy]
        J2 = [J0[0] - (bf * y) * invz2, J0[1] + (bf * x) * invz2, J0[2], J0[3], zero, J0[5] - bf * invz2]
    return [J0, J1, J2]


def linearise(pr, R, t, active, robust):
    """computeActiveErrors + activeRobustChi2 + buildSystem: H (upper triangle mirrored), b, the robust chi2"""
    e, chi2 = edge_error(pr, R, t)
    rho0, rho1 = huber(pr, chi2, robust)
    J = edge_jacobian(pr, R, t)
    H = np.zeros((6, 6), F64)
    b = np.zeros(6, F64)
    with np.errstate(all="ignore"):
        w = rho1 * pr.inf if robust else pr.inf                       # robustInformation: rho[1] * Omega
        g = [-(pr.inf * e[k]) for k in range(3)]                      # -Omega e
        if robust:
            g = [rho1 * g[k] for k in range(3)]
        for i in range(6):
            for j in range(i, 6):
                a2 = np.where(pr.stereo, J[2][i] * (w * J[2][j]), F64(0.0))
                H[i, j] = H[j, i] = tree_sum(pr, J[0][i] * (w * J[0][j]) + (J[1][i] * (w * J[1][j]) + a2), active)
        for j in range(6):
            a2 = np.where(pr.stereo, J[2][j] * g[2], F64(0.0))
            b[j] = tree_sum(pr, J[0][j] * g[0] + (J[1][j] * g[1] + a2), active)
    return H, b, tree_sum(pr, rho0, active)


def robust_chi2(pr, R, t, active, robust):
    _, chi2 = edge_error(pr, R, t)
    return tree_sum(pr, huber(pr, chi2, robust)[0], active)


def solve6(H, b, lam):
    """(H + lam I) x = b by an unpivoted L L^T in a fixed loop order (P5); None when a pivot is not positive and finite"""
    L = np.zeros((6, 6), F64)
    with np.errstate(all="ignore"):
        for j in range(6):
            s = H[j, j] + lam
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0.0 and np.isfinite(s)):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, 6):
                s = H[j, i]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        yv = np.zeros(6, F64)
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * yv[k]
            yv[i] = s / L[i, i]
        x = np.zeros(6, F64)
        for i in range(5, -1, -1):
            s = yv[i]
            for k in range(i + 1, 6):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x


def optimize_round(pr, R0, t0, active, robust, log=None):
    """SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg::solve.  Returns (R, t, iterations, trials, chi2, lambda).
    log (a list) receives one dict per trial: what the CPU tests assert on."""
    R, t = R0.copy(), t0.copy()
    if not active.any():
        return R, t, 0, 0, F64(0.0), F64(0.0)
    lam, ni = F64(0.0), F64(2.0)
    iterations = trials = 0
    cur = F64(0.0)
    for it in range(ITERATIONS):
        H, b, cur = linearise(pr, R, t, active, robust)
        if it == 0:
            m = np.abs(H[0, 0])                                        # computeLambdaInit: tau * max |H_jj|
            for j in range(1, 6):
                a = np.abs(H[j, j])
                m = a if a > m else m
            lam, ni = TAU * m, F64(2.0)
        iterations += 1
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            x = solve6(H, b, lam)
            step = exp_step(R, t, x) if x is not None else None
            failed = step is None
            why = "pivot" if x is None else ("theta" if failed else "")
            accepted = False
            with np.errstate(all="ignore"):
                if failed:
                    rho, temp = F64(-1.0), F64(DBL_MAX)
                else:
                    temp = robust_chi2(pr, step[0], step[1], active, robust)
                    scale = F64(0.0)
                    for j in range(6):
                        scale = scale + x[j] * (lam * x[j] + b[j])     # computeScale
                    scale = scale + F64(1e-3)
                    rho = (cur - temp) / scale
                    accepted = bool(rho > 0.0 and np.isfinite(temp))
                if log is not None:
                    log.append(dict(iteration=it, trial=qmax, failed=failed, why=why, accepted=accepted, rho=rho, before=cur, after=temp, lam=lam))
                if accepted:
                    q = F64(2.0) * rho - F64(1.0)
                    alpha = F64(1.0) - (q * q) * q
                    alpha = GOOD_UP if GOOD_UP < alpha else alpha       # std::min(alpha, 2/3)
                    factor = alpha if GOOD_LOW < alpha else GOOD_LOW    # std::max(1/3, alpha)
                    lam = lam * factor
                    ni = F64(2.0)
                    cur = temp
                    R, t = step
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
    return R, t, iterations, trials, cur, lam


class Result:
    pass


def pose_optimization(pr, Rcw, tcw, log=None):
    """Optimizer::PoseOptimization.  Rcw [3, 3], tcw [3] float32.  Returns a Result: Rcw[9], tcw[3] float32, outlier[N] uint8, n_good, n_edges,
    rounds, iterations[4], trials[4] int32, chi2[4], lam[4] float64."""
    R0 = np.asarray(Rcw, np.float32).reshape(3, 3).astype(F64)
    t0 = np.asarray(tcw, np.float32).reshape(3).astype(F64)
    res = Result()
    res.n_edges = int(pr.edge.sum())
    res.iterations, res.trials = np.zeros(4, np.int32), np.zeros(4, np.int32)
    res.chi2, res.lam = np.zeros(4, F64), np.zeros(4, F64)
    res.outlier = np.zeros(pr.N, np.uint8)
    res.rounds, res.n_good = 0, 0
    res.flags_by_round = []                                             # (for the CPU tests: mvbOutlier after each round)
    R, t = R0, t0
    if res.n_edges >= 3:
        flagged = np.zeros(pr.N, bool)
        for r in range(ROUNDS):
            rl = None if log is None else []
            R, t, res.iterations[r], res.trials[r], res.chi2[r], res.lam[r] = optimize_round(pr, R0, t0, pr.edge & ~flagged, r < 3, rl)
            if log is not None:
                log.append(rl)
            _, chi2 = edge_error(pr, R, t)                              # P1: at the round's final accepted pose
            with np.errstate(all="ignore"):
                flagged = pr.edge & (~np.isfinite(chi2) | (chi2.astype(np.float32) > pr.th))  # P2
            res.flags_by_round.append(flagged.copy())
            res.chi2_edges = chi2                                       # (for the CPU tests: what the last classification compared)
            res.rounds = r + 1
            if res.n_edges < 10:
                break
        res.outlier = flagged.astype(np.uint8)
        res.n_good = res.n_edges - int(flagged.sum())
    res.Rcw = R.reshape(9).astype(np.float32)                           # Converter::toMatrix4f
    res.tcw = t.astype(np.float32)
    return res
