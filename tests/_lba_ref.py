"""Normative restatement of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:450-768) and Optimizer::BundleAdjustment (:61-243) and of
the parts of g2o they run, over slots of the keyframe table and ids of the map-point store (afv_table_bundle_adjust, csrc/k_lba.hip).
numpy float64, ONE rounding per operator (the library is built with -ffp-contract=off; division and square root are correctly rounded on
both sides), every operator order fixed here; three-term sums are a0 + (a1 + a2).  The pieces whose text is PoseOptimization's (the
exponential map, the Huber kernel, the error and the pose Jacobian of the projection edges) are imported from tests/_poseopt_ref.py.

g2o is an empty directory in the reference, so its arithmetic is restated after upstream g2o as bundled with ORB-SLAM2 - parity with a real
g2o is UNPINNED.  What is restated, by class and function:
  EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ :: computeError, linearizeOplus (both vertices), isDepthPositive   -> edges_at, jacobians
  BaseBinaryEdge::constructQuadraticForm, BaseEdge::chi2, RobustKernelHuber::robustify                           -> linearise
  BlockSolver_6_3 with the points marginalised (buildSystem, setLambda, solve)                                   -> linearise, schur_step
  OptimizationAlgorithmLevenberg::solve, computeLambdaInit, computeScale; SparseOptimizer::optimize, terminate   -> optimize
  VertexSE3Expmap::oplusImpl, VertexSBAPointXYZ::oplusImpl                                                       -> _poseopt_ref.exp_step, x + dx

The problem: nk keyframes, the first nf free, the others fixed (the host puts keyId == 0 and lFixedCameras there); np points; ne edges in
the order in which the reference adds them (per point, per observation), so obs_point is ascending.  A point whose id is unset or bad in
the store is DROPPED with its edges (:475-476).  A feature is a stereo edge when its u_right >= 0.  The information of a mono edge is
inf * I2 (GetKeyPt2DInf); of a stereo edge diag(inf, inf, inf3) with inf3 = 0.5f * (inf + inf) in float (GetKeyPt3DInf / GetKeyPt1DInf,
Frame.cc:709-725).  Huber deltas (double)sqrtf(5.991f) / (double)sqrtf(7.815f); thresholds the floats 5.991f / 7.815f promoted.

The edge: e = obs - (fx * (x / z) + cx, fy * (y / z) + cy [, u - bf / z]) at (x, y, z) = R X + t, as _poseopt_ref.edge_error.  The pose
Jacobian (2 x 6 / 3 x 6, rotation columns first) is _poseopt_ref.edge_jacobian's text (invz = 1 / z, invz2 = invz * invz).  The point
Jacobian is -1 / z * tmp * R with tmp = [fx 0 -(x / z) fx; 0 fy -(y / z) fy]: J[0][c] = m * (fx * R[0][c] + t02 * R[2][c]), m = -invz,
t02 = -((x * invz) * fx); row 1 alike; the stereo row is J[0][c] - (bf * R[2][c]) * invz2.  A fixed keyframe contributes no Jacobian.
Every product J^T (w Omega) J' of an edge is u0 * (w0 * v0) + (u1 * (w0 * v1) + a2), a2 = u2 * (w2 * v2) on a stereo edge and +0.0 on
a mono edge; w = rho[1] * Omega under the kernel; the right-hand side is J^T g with g = rho[1] * (-(Omega e)).

The system: Hpp (6 x 6 per free keyframe), Hll (3 x 3 per point), Hpl = W (6 x 3 per edge to a free keyframe), bp, bl.  A trial with
lambda: Hinv = (Hll + lambda I)^-1, z = Hinv bl; S(i, j) = [Hpp_i + lambda I if i == j] - sum_e (W_e Hinv) W_e'^T over the edges e of
keyframe i whose point has an edge e' to keyframe j; bS_i = bp_i - sum_e W_e z; S dxp = bS; dxl = Hinv (bl - sum_e W_e^T dxp), the sum
subtracted edge by edge from bl, each W^T dxp summed in ascending row; poses step through exp_step, points by addition.

The drivers.  LocalBundleAdjustment: optimize(5) under the kernel; the first check (:662-692: level 1 on chi2 > 5.991 / 7.815 ||
!isDepthPositive, the kernel off for every edge); optimize(10); the final check (:705-733) that fills vToErase.  BundleAdjustment: one
optimize(nIterations), under the kernel or not, no checks.  Each optimize() starts its own Levenberg.
Quirk kept (L-Q1): the final check visits the edges removed by the first check too; as upstream caches _error, a removed edge keeps the
chi2 of the first check while its depth test is made at the final estimate - an edge removed for depth alone can survive.

The stop flag (pbStopFlag; g2o reads it before every iteration and after every trial) is the index stop_at: raised from the moment
stop_at trials have run (None: never; 0: before the call).  Raised before the call: LocalBundleAdjustment returns at :645-647, nothing
is written.  Raised during the first optimize: bDoMore = false, the first check and the second optimize are skipped, the final check
and the write-back run.  BundleAdjustment has no early return: a raised flag ends its optimize().

Deliberate deviations from upstream:
  (L1) both checks are made at the accepted estimate (P1 / O1).
  (L2) a chi2 that is not finite is an outlier (P2 / O2).
  (L3) the state is R, t in double, no quaternion (P3).
  (L4) no libm: PoseOptimization's Horner tables (P4); a step beyond pi is a failed trial.
  (L5) every sum has one fixed shape.  Per keyframe (Hpp, bp, the Schur sums of block row i), over that keyframe's edges in list order: 64
       partial sums, partial l starts at +0.0 and adds the terms at positions l, l + 64, ... of the keyframe's list in ascending order, an
       edge that is not active adding nothing; then p[l] += p[l + s] for s = 32 .. 1 (O5 / E7).  Per point (Hll, bl, the back
       substitution), over its active edges in list order, one after the other from +0.0 (from bl).  The chi2 sums: the same 64-partial
       tree over positions in the edge list.  The scale sum: the same tree over the unknowns, poses first (6 per free keyframe), then
       points (3 per point, a dropped point adding nothing).  computeLambdaInit's maximum starts at +0.0, so a NaN never enters.
  (L6) Hinv by cofactors in the order of point_inverse; a determinant that is 0 or not finite is a failed trial.
  (L7) the reduced system is solved by a dense, unpivoted L L^T in the order of the free-keyframe list; element (i, j) subtracts its
       products in ascending k; the forward substitution subtracts in ascending k, the back substitution in descending k (both are column
       sweeps on a device).  The reference uses Eigen's sparse Cholesky with a fill-reducing ordering.  A pivot that is not positive
       and finite is a failed trial (O6).  A vertex without active edges stays in the system: its block holds lambda alone, its step is 0.
  (L8) a problem without free keyframes, without points or without (active) edges evaluates nothing.
  (L9) what is not written reads 0: the position of a dropped point, the trace of a round that did not run.
A failed trial (L4, L6, L7) is a rejected trial whatever rho would have been: lambda *= ni, ni *= 2, the trial loop goes on as for rho < 0.
A point observed twice by one keyframe is outside the contract (GetObservations is a map keyed by the keyframe); the C-ABI refuses it.
"""
import numpy as np

from _poseopt_ref import DBL_MAX, DELTA_MONO, DELTA_STEREO, F64, GOOD_LOW, GOOD_UP, MAX_TRIALS, TAU, TH_MONO, TH_STEREO, exp_step

DROPPED, KEPT, REMOVED_KEPT, ERASE = 0, 1, 2, 3
F32 = np.float32


class Problem:
    """cams[k]: (Rcw[9], tcw[3], fx, fy, cx, cy, bf) as 17 floats; pos [np][3] float32; p_ok [np]; e_pt, e_kf [ne]; obs [ne][4] float32:
    x, y, u_right, inf"""

    def __init__(self, cams, nf, pos, p_ok, e_pt, e_kf, obs):
        cams = np.asarray(cams, F32).reshape(-1, 17)
        self.nk, self.nf = len(cams), int(nf)
        self.R0 = cams[:, :9].astype(F64).reshape(-1, 3, 3)
        self.t0 = cams[:, 9:12].astype(F64)
        self.K = cams[:, 12:17].astype(F64)
        pos = np.asarray(pos, F32).reshape(-1, 3)
        self.np = len(pos)
        self.p_on = np.asarray(p_ok, bool).reshape(-1).copy()
        self.X0 = np.where(self.p_on[:, None], pos.astype(F64), F64(0.0))
        self.e_pt, self.e_kf = np.asarray(e_pt, np.int64).reshape(-1), np.asarray(e_kf, np.int64).reshape(-1)
        self.ne = len(self.e_pt)
        assert np.all(np.diff(self.e_pt) >= 0)
        obs = np.asarray(obs, F32).reshape(-1, 4)
        self.ox, self.oy, self.our, self.inf = (obs[:, k].astype(F64) for k in range(4))
        with np.errstate(all="ignore"):
            self.inf3 = (F32(0.5) * (obs[:, 3] + obs[:, 3])).astype(F64)   # GetKeyPt1DInf, in float
        self.stereo = obs[:, 2] >= F32(0.0)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.th = np.where(self.stereo, F64(TH_STEREO), F64(TH_MONO))
        self.free = self.e_kf < self.nf
        self.pt_edges = [np.nonzero(self.e_pt == p)[0] for p in range(self.np)]
        self.kf_edges = [np.nonzero(self.e_kf == i)[0] for i in range(self.nf)]
        self.fx, self.fy, self.cx, self.cy, self.bf = (self.K[self.e_kf, k] if self.ne else np.zeros(0, F64) for k in range(5))


def lane_sum(v, active):
    """L5: v [m] or [m, q] over the positions of a list"""
    v = np.asarray(v, F64)
    v2 = v.reshape(len(v), -1)
    m, q = v2.shape
    rows = max((m + 63) // 64, 1)
    a = np.zeros((rows * 64, q), F64)
    with np.errstate(all="ignore"):
        a[:m] = np.where(np.asarray(active, bool)[:, None], v2, F64(0.0))   # + 0.0 is exactly neutral: no partial is ever -0.0
        a = a.reshape(rows, 64, q)
        p = np.zeros((64, q), F64)
        for r in range(rows):
            p = p + a[r]
        s = 32
        while s >= 1:
            p[:s] = p[:s] + p[s:2 * s]
            s >>= 1
    return p[0] if v.ndim > 1 else F64(p[0, 0])


def edges_at(pr, R, t, X):
    """computeError + chi2 of every edge at an estimate: (x, y, z), (e0, e1, e2), chi2"""
    Re, te, Xe = R[pr.e_kf], t[pr.e_kf], X[pr.e_pt]
    with np.errstate(all="ignore"):
        c = [(Re[:, r, 0] * Xe[:, 0] + (Re[:, r, 1] * Xe[:, 1] + Re[:, r, 2] * Xe[:, 2])) + te[:, r] for r in range(3)]
        x, y, z = c
        px = pr.fx * (x / z) + pr.cx
        py = pr.fy * (y / z) + pr.cy
        e0 = pr.ox - px
        e1 = pr.oy - py
        e2 = np.where(pr.stereo, pr.our - (px - pr.bf / z), F64(0.0))
        c2 = np.where(pr.stereo, e2 * (pr.inf3 * e2), F64(0.0))
        chi2 = e0 * (pr.inf * e0) + (e1 * (pr.inf * e1) + c2)
    return (x, y, z), (e0, e1, e2), chi2


def huber(pr, chi2, robust):
    if not robust:
        return chi2, np.ones_like(chi2)
    with np.errstate(all="ignore"):
        dsqr = pr.delta * pr.delta
        s = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, (F64(2.0) * s) * pr.delta - dsqr), np.where(inl, F64(1.0), pr.delta / s)


def jacobians(pr, R, xyz):
    """linearizeOplus: Jl[r][c] (the point), Jp[r][j] (the pose)"""
    x, y, z = xyz
    Re = R[pr.e_kf]
    fx, fy, bf = pr.fx, pr.fy, pr.bf
    with np.errstate(all="ignore"):
        invz = F64(1.0) / z
        invz2 = invz * invz
        m, t02, t12 = -invz, -((x * invz) * fx), -((y * invz) * fy)
        Jl = [[None] * 3 for _ in range(3)]
        for c in range(3):
            Jl[0][c] = m * (fx * Re[:, 0, c] + t02 * Re[:, 2, c])
            Jl[1][c] = m * (fy * Re[:, 1, c] + t12 * Re[:, 2, c])
            Jl[2][c] = Jl[0][c] - (bf * Re[:, 2, c]) * invz2
        zero = np.zeros_like(x)
        J0 = [((x * y) * invz2) * fx, -((F64(1.0) + (x * x) * invz2) * fx), (y * invz) * fx, -(invz * fx), zero, (x * invz2) * fx]
        J1 = [(F64(1.0) + (y * y) * invz2) * fy, -(((x * y) * invz2) * fy), -((x * invz) * fy), zero, -(invz * fy), (y * invz2) * fy]
        J2 = [J0[0] - (bf * y) * invz2, J0[1] + (bf * x) * invz2, J0[2], J0[3], zero, J0[5] - bf * invz2]
    return Jl, [J0, J1, J2]


class System:
    pass


def linearise(pr, R, t, X, on, robust):
    """computeActiveErrors + activeRobustChi2 + buildSystem"""
    xyz, e, chi2 = edges_at(pr, R, t, X)
    rho0, rho1 = huber(pr, chi2, robust)
    Jl, Jp = jacobians(pr, R, xyz)
    sy = System()
    with np.errstate(all="ignore"):
        w0 = rho1 * pr.inf if robust else pr.inf
        w2 = rho1 * pr.inf3 if robust else pr.inf3
        g = [-(pr.inf * e[0]), -(pr.inf * e[1]), -(pr.inf3 * e[2])]
        if robust:
            g = [rho1 * v for v in g]

        def w3(u, v):
            a2 = np.where(pr.stereo, u[2] * (w2 * v[2]), F64(0.0))
            return u[0] * (w0 * v[0]) + (u[1] * (w0 * v[1]) + a2)

        def g3(u):
            a2 = np.where(pr.stereo, u[2] * g[2], F64(0.0))
            return u[0] * g[0] + (u[1] * g[1] + a2)

        col = lambda J, c: (J[0][c], J[1][c], J[2][c])
        Al = {(c, d): w3(col(Jl, c), col(Jl, d)) for c in range(3) for d in range(c, 3)}
        gl = [g3(col(Jl, c)) for c in range(3)]
        sy.W = np.stack([np.stack([w3(col(Jp, a), col(Jl, c)) for c in range(3)], 1) for a in range(6)], 1) if pr.ne else np.zeros((0, 6, 3))
        Ap = [w3(col(Jp, i), col(Jp, j)) for i in range(6) for j in range(i, 6)]
        gp = [g3(col(Jp, i)) for i in range(6)]
        # per point, one after the other
        sy.Hll, sy.bl = np.zeros((pr.np, 3, 3), F64), np.zeros((pr.np, 3), F64)
        for p in range(pr.np):
            if not pr.p_on[p]:
                continue
            for ed in pr.pt_edges[p]:
                if not on[ed]:
                    continue
                for c in range(3):
                    for d in range(c, 3):
                        sy.Hll[p, c, d] = sy.Hll[p, c, d] + Al[(c, d)][ed]
                    sy.bl[p, c] = sy.bl[p, c] + gl[c][ed]
            for c in range(3):
                for d in range(c):
                    sy.Hll[p, c, d] = sy.Hll[p, d, c]
        # per free keyframe, the 64-partial tree
        sy.Hpp, sy.bp = np.zeros((pr.nf, 6, 6), F64), np.zeros((pr.nf, 6), F64)
        for i in range(pr.nf):
            ke = pr.kf_edges[i]
            s = lane_sum(np.stack([a[ke] for a in Ap] + [a[ke] for a in gp], 1), on[ke])
            q = 0
            for a in range(6):
                for b in range(a, 6):
                    sy.Hpp[i, a, b] = sy.Hpp[i, b, a] = s[q]
                    q += 1
            sy.bp[i] = s[21:27]
        sy.chi2 = lane_sum(rho0, on)
    return sy


def robust_chi2(pr, R, t, X, on, robust):
    _, _, chi2 = edges_at(pr, R, t, X)
    return lane_sum(huber(pr, chi2, robust)[0], on)


def lambda_init(pr, sy):
    m = F64(0.0)
    for i in range(pr.nf):
        for a in range(6):
            v = np.abs(sy.Hpp[i, a, a])
            m = v if v > m else m
    for p in range(pr.np):
        if pr.p_on[p]:
            for c in range(3):
                v = np.abs(sy.Hll[p, c, c])
                m = v if v > m else m
    return TAU * m


def point_inverse(H, lam):
    """L6: the inverse of the symmetric H + lam I by cofactors; None when the determinant is 0 or not finite"""
    with np.errstate(all="ignore"):
        a, b, c, d, e, f = H[0, 0] + lam, H[0, 1], H[0, 2], H[1, 1] + lam, H[1, 2], H[2, 2] + lam
        c00, c01, c02, c11, c12, c22 = d * f - e * e, c * e - b * f, b * e - c * d, a * f - c * c, b * c - a * e, a * d - b * b
        det = a * c00 + (b * c01 + c * c02)
        bad = bool(det == 0.0 or not np.isfinite(det))
        r = F64(1.0) / det
        I = np.array([[c00 * r, c01 * r, c02 * r], [c01 * r, c11 * r, c12 * r], [c02 * r, c12 * r, c22 * r]], F64)
    return I, bad


def mat3(M, v):
    return np.array([M[r, 0] * v[0] + (M[r, 1] * v[1] + M[r, 2] * v[2]) for r in range(3)], F64)


def solve_dense(S, b):
    """L7 on the upper triangle of S; None on a bad pivot"""
    n = len(b)
    L = np.zeros((n, n), F64)
    with np.errstate(all="ignore"):
        for j in range(n):
            s = S[j, j]
            for k in range(j):
                s = s - L[j, k] * L[j, k]
            if not (s > 0.0 and np.isfinite(s)):
                return None
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                s = S[j, i]
                for k in range(j):
                    s = s - L[i, k] * L[j, k]
                L[i, j] = s / L[j, j]
        x = np.zeros(n, F64)
        for i in range(n):
            s = b[i]
            for k in range(i):
                s = s - L[i, k] * x[k]
            x[i] = s / L[i, i]
        for i in range(n - 1, -1, -1):
            s = x[i]
            for k in range(n - 1, i, -1):
                s = s - L[k, i] * x[k]
            x[i] = s / L[i, i]
    return x


def reduced_system(pr, sy, on, lam):
    """Hinv, z per point; S (upper triangle), bS.  Returns (S, bS, Hinv, z, failed)"""
    n = 6 * pr.nf
    Hinv, z = np.zeros((pr.np, 3, 3), F64), np.zeros((pr.np, 3), F64)
    failed = False
    with np.errstate(all="ignore"):
        for p in range(pr.np):
            if pr.p_on[p]:
                Hinv[p], bad = point_inverse(sy.Hll[p], lam)
                failed = failed or bad
                z[p] = mat3(Hinv[p], sy.bl[p])
        S, bS = np.zeros((n, n), F64), np.zeros(n, F64)
        partner = {(int(pr.e_pt[e]), int(pr.e_kf[e])): e for e in range(pr.ne - 1, -1, -1) if on[e] and pr.free[e]}
        for i in range(pr.nf):
            ke = pr.kf_edges[i]
            F = Hinv[pr.e_pt[ke]]
            W = sy.W[ke]
            Y = [[W[:, a, 0] * F[:, 0, c] + (W[:, a, 1] * F[:, 1, c] + W[:, a, 2] * F[:, 2, c]) for c in range(3)] for a in range(6)]
            for j in range(i, pr.nf):
                e2 = np.array([partner.get((int(pr.e_pt[e]), j), -1) for e in ke], np.int64)
                act = on[ke] & (e2 >= 0)
                W2 = sy.W[np.clip(e2, 0, None)] if pr.ne else W
                cols = [Y[a][0] * W2[:, b, 0] + (Y[a][1] * W2[:, b, 1] + Y[a][2] * W2[:, b, 2]) for a in range(6) for b in range(6)]
                if j == i:
                    zz = z[pr.e_pt[ke]]
                    cols += [W[:, a, 0] * zz[:, 0] + (W[:, a, 1] * zz[:, 1] + W[:, a, 2] * zz[:, 2]) for a in range(6)]
                s = lane_sum(np.stack(cols, 1), act)
                for a in range(6):
                    for b in range(6):
                        if j == i and b < a:
                            continue
                        h = F64(0.0)
                        if j == i:
                            h = sy.Hpp[i, a, b]
                            if a == b:
                                h = h + lam
                        S[6 * i + a, 6 * j + b] = h - s[6 * a + b]
                if j == i:
                    bS[6 * i:6 * i + 6] = sy.bp[i] - s[36:42]
    return S, bS, Hinv, z, failed


def schur_step(pr, sy, on, lam):
    """one solve of the damped system with the points marginalised: (dxp [nf, 6], dxl [np, 3]) or (None, why)"""
    S, bS, Hinv, z, failed = reduced_system(pr, sy, on, lam)
    if failed:
        return None, "det"
    x = solve_dense(S, bS)
    if x is None:
        return None, "pivot"
    dxp = x.reshape(pr.nf, 6)
    dxl = np.zeros((pr.np, 3), F64)
    with np.errstate(all="ignore"):
        for p in range(pr.np):
            if not pr.p_on[p]:
                continue
            r = sy.bl[p].copy()
            for e in pr.pt_edges[p]:
                if not on[e] or not pr.free[e]:
                    continue
                d = dxp[pr.e_kf[e]]
                for c in range(3):
                    s = sy.W[e, 0, c] * d[0]
                    for a in range(1, 6):
                        s = s + sy.W[e, a, c] * d[a]
                    r[c] = r[c] - s
            dxl[p] = mat3(Hinv[p], r)
    return (dxp, dxl), ""


class Clock:
    """the stop flag as an index: raised from the moment stop_at trials have run"""

    def __init__(self, stop_at):
        self.stop_at, self.trials = stop_at, 0

    def raised(self):
        return self.stop_at is not None and self.trials >= self.stop_at


def optimize(pr, est, on, iterations, robust, clock, log=None):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve.  est = (R [nk, 3, 3], t [nk, 3], X [np, 3]).
    Returns (est, iterations, trials, chi2, lambda)"""
    R, t, X = est
    if not on.any() or pr.nf == 0 or iterations <= 0 or clock.raised():                # L8; terminate() before the first iteration
        return est, 0, 0, F64(0.0), F64(0.0)
    lam, ni, cur = F64(0.0), F64(2.0), F64(0.0)
    done = trials = 0
    for it in range(iterations):
        if clock.raised():
            break
        sy = linearise(pr, R, t, X, on, robust)
        cur = sy.chi2
        if it == 0:
            lam, ni = lambda_init(pr, sy), F64(2.0)
        done += 1
        rho, qmax = F64(0.0), 0
        while True:
            trials += 1
            clock.trials += 1
            step, why = schur_step(pr, sy, on, lam)
            new = None
            if step is not None:
                dxp, dxl = step
                Rn, tn = R.copy(), t.copy()
                for i in range(pr.nf):
                    st = exp_step(R[i], t[i], dxp[i])
                    if st is None:
                        why = "theta"
                        break
                    Rn[i], tn[i] = st
                else:
                    with np.errstate(all="ignore"):
                        new = (Rn, tn, np.where(pr.p_on[:, None], X + dxl, X))
            failed = new is None
            accepted = False
            with np.errstate(all="ignore"):
                if failed:
                    rho, temp = F64(-1.0), F64(DBL_MAX)
                else:
                    temp = robust_chi2(pr, new[0], new[1], new[2], on, robust)
                    xs = np.concatenate([dxp.reshape(-1), dxl.reshape(-1)])
                    bs = np.concatenate([sy.bp.reshape(-1), sy.bl.reshape(-1)])
                    takes = np.concatenate([np.ones(6 * pr.nf, bool), np.repeat(pr.p_on, 3)])
                    scale = lane_sum(xs * (lam * xs + bs), takes) + F64(1e-3)                # computeScale
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
                    R, t, X = new
                else:
                    lam = lam * ni
                    ni = ni * F64(2.0)
            qmax += 1
            if not (rho < 0.0 and qmax < MAX_TRIALS and not clock.raised()):
                break
        if qmax == MAX_TRIALS or rho == 0.0:
            if log is not None:
                log.append(dict(terminate="qmax" if qmax == MAX_TRIALS else "rho0", iteration=it))
            break
    return (R, t, X), done, trials, cur, lam


def outliers(pr, est, cached=None, use_cached=None):
    """L1, L2: chi2 > th || !isDepthPositive at the estimate; with use_cached the chi2 is the cached one (L-Q1)"""
    xyz, _, chi2 = edges_at(pr, *est)
    if cached is not None:
        chi2 = np.where(use_cached, cached, chi2)
    with np.errstate(all="ignore"):
        return ~np.isfinite(chi2) | (chi2 > pr.th) | ~(xyz[2] > 0.0), chi2, ~(xyz[2] > 0.0)


class Result:
    pass


def bundle_adjust(pr, iterations=(5, 10), robust=(True, False), checks=True, stop_at=None, log=None):
    """checks=True: LocalBundleAdjustment; False: BundleAdjustment with iterations[0], robust[0].  Returns a Result: stopped (0 no, 1 before
    the call - nothing written, 2 in the first optimize, 3 in the second), iterations[2], trials[2] int32, chi2[2], lam[2], n_edges,
    n_removed_first, n_erase, R [nf, 9], t [nf, 3], xyz [np, 3] float64 (L9: 0 for a dropped point), state[ne] uint8"""
    res = Result()
    res.iterations, res.trials = np.zeros(2, np.int32), np.zeros(2, np.int32)
    res.chi2, res.lam = np.zeros(2, F64), np.zeros(2, F64)
    on = pr.p_on[pr.e_pt] if pr.ne else np.zeros(0, bool)
    res.n_edges, res.n_removed_first, res.n_erase, res.stopped = int(on.sum()), 0, 0, 0
    state = np.where(on, KEPT, DROPPED).astype(np.uint8)
    clock = Clock(stop_at)
    res.state, res.R, res.t, res.xyz = state, None, None, None
    if checks and clock.raised():
        res.stopped = 1
        return res
    logs = [[], []]
    est = (pr.R0.copy(), pr.t0.copy(), pr.X0.copy())
    est, res.iterations[0], res.trials[0], res.chi2[0], res.lam[0] = optimize(pr, est, on, iterations[0], robust[0], clock, logs[0])
    if clock.raised():
        res.stopped = 2
    if checks:
        first_chi2 = np.zeros(pr.ne, F64)
        if not res.stopped:
            bad, first_chi2, res.first_depth_bad = outliers(pr, est)
            bad = bad & on
            res.first_chi2 = first_chi2
            res.n_removed_first = int(bad.sum())
            state[bad] = REMOVED_KEPT
            on = on & ~bad
            est, res.iterations[1], res.trials[1], res.chi2[1], res.lam[1] = optimize(pr, est, on, iterations[1], robust[1], clock, logs[1])
            if clock.raised():
                res.stopped = 3
        bad, res.final_chi2, res.final_depth_bad = outliers(pr, est, first_chi2, state == REMOVED_KEPT)
        bad = bad & (state != DROPPED)
        state[bad] = ERASE
        res.n_erase = int(bad.sum())
    if log is not None:
        log.extend(logs)
    res.R, res.t = est[0][:pr.nf].reshape(-1, 9).copy(), est[1][:pr.nf].copy()
    res.xyz = np.where(pr.p_on[:, None], est[2], F64(0.0))
    return res
