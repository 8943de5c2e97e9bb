"""Normative restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:771-1031) and of the parts of g2o it runs, over plain
arrays (afv_essential_graph, csrc/k_essgraph.hip) and of the point correction of LoopClosing::CorrectLoop (LoopClosing.cc:487-516,
afv_points_correct_sim3).  numpy float64, ONE rounding per operator (the library is built with -ffp-contract=off; division and square
root are correctly rounded on both sides), every operator order fixed here; three-term sums are a0 + (a1 + a2).  What OptimizeSim3 and
the bundle adjustment already state is imported: sim3_exp, exp_sigma, compose, inverse, step (tests/_sim3opt_ref.py), the Horner
tables and the Levenberg constants (tests/_poseopt_ref.py), the 64-partial halving tree lane_sum (tests/_lba_ref.py).

g2o is an empty directory in the reference, so its arithmetic is restated after upstream g2o as bundled with ORB-SLAM2 - parity with a real
g2o is UNPINNED.  What is restated, by class and function:
  VertexSim3Expmap::oplusImpl (update[6] = 0 under _fix_scale)                                                   -> _sim3opt_ref.step
  EdgeSim3::computeError: log(C * S(v0) * S(v1)^-1), v0 the vertex of setVertex(0, ...)                          -> edge_error
  Sim3::log (its four branches), Sim3::operator*, Sim3::inverse, Sim3::map                                       -> sim3_log, vcompose, vinverse, sim3_map
  BaseBinaryEdge::linearizeOplus (central differences, delta 1e-9, a fixed vertex skipped)                       -> jacobians
  BaseBinaryEdge::constructQuadraticForm, BaseEdge::chi2 (information I7, no robust kernel)                      -> build_system
  BlockSolver_7_3 / LinearSolverEigen (the block-sparse system over the free vertices)                           -> symbolic, factor_solve
  OptimizationAlgorithmLevenberg::solve with userLambdaInit, computeScale; SparseOptimizer::optimize             -> optimize
  the recovery (:979-998) and the point correction (:1000-1030)                                                  -> recover, correct_points
  the edge list (:835-971)                                                                                       -> essential_graph_edges

The problem: nk vertices in the order of the caller's keyframe list, vertex `fixed` (pLoopKF) fixed, the others free; system position of
a free vertex = its rank among the free ones.  ne edges (v0, v1, measurement) in the order in which the reference adds them.  One
optimize(iterations) call (20 in the reference), lambda at iteration 0 = lambda_init (userLambdaInit, 1e-16 in the reference), at most
10 trials per iteration, accept on rho > 0 and a finite chi2; a rejected trial: lambda *= ni, ni *= 2.

The edge: T = C * S0, U = T * S1^-1, e = log(U) = (omega, upsilon, sigma).  chi2 = e0 e0 + e1 e1 + ... one after the other.  The
Jacobians are numeric: per vertex 14 perturbed estimates Sim3(+-1e-9 e_d) * estimate; column d of J0 is (1 / (2 * 1e-9)) * (e(S0 +d) -
e(S0 -d)), of J1 alike with S1 perturbed: 28 perturbed errors per edge.  The terms of an edge: A00 = J0^T J0, A11 = J1^T J1, A01 = J0^T
J1, each entry its seven products one after the other in ascending row, g0 = J0^T (-e), g1 = J1^T (-e).

Sim3::log.  sigma = log(s); d = 0.5 * ((R00 + (R11 + R22)) - 1); dR = (R21 - R12, R02 - R20, R10 - R01).
  d > 1 - eps: omega = 0.5 dR; else theta = acos(d), omega = (theta / (2 sqrt(1 - d d))) dR.
  |sigma| < eps: C = 1, (A, B) = (1/2, 1/6) near the identity, else (EXP_B(theta^2), EXP_C(theta^2)) (G3).
  else C = (s - 1) / sigma and A, B as Sim3(Vector7) writes them (_sim3opt_ref.sim3_exp, the same text), but for G10.
  W = A Omega + B Omega^2 + C I; upsilon = W^-1 t by cofactors (G4).
The branch of an evaluation is 2 * (|sigma| >= eps) + (d <= 1 - eps): 0 .. 3.

Deliberate deviations from upstream:
  (G1) the linear system is block-sparse in 7 x 7 blocks over the free vertices IN THE ORDER OF THE CALLER'S KEYFRAME LIST, factorised
       by an unpivoted block L L^T whose pattern is the symbolic fill of that order (the reference lets Eigen's sparse Cholesky choose a
       fill-reducing order).  Block column j is finished before column j + 1: L_jj the unpivoted 7 x 7 L L^T of A_jj (L7's loops), L_ij =
       A_ij L_jj^-T by forward substitution (ascending k), then every later block A_ik -= L_ij L_kj^T, the seven products of an entry
       subtracted one after the other in ascending order, the columns j in ascending order.  The forward substitution runs ascending
       (column sweep: after y_j, every row i of column j subtracts L_ij y_j, products in ascending order), the back substitution
       descending (row j subtracts L_ij^T x_i over the rows i of column j in descending i, products in descending order, then the block's
       own back substitution in descending k).  A pivot that is not positive and finite is a failed trial (O6 / L7).  A vertex without
       edges stays in the system: its block holds lambda alone, its step is 0.
  (G2) the state is R, t, s in double, no quaternion; the caller's rotations are taken as given (O3).
  (G3) no libm.  sin / cos of theta: PoseOptimization's Horner tables (sin th = th * A(th^2), cos th = 1 - th^2 * B(th^2)); (1 - cos th) /
       th^2 and (th - sin th) / th^3 are the tables EXP_B and EXP_C themselves (upstream forms the differences, which cancel).  log(x)
       = k LN2_HI + (2 f P(f^2) + k LN2_LO): x = m 2^k with m in [sqrt(1/2), sqrt(2)) (frexp, exact), f = (m - 1) / (m + 1), P(z) = sum_n
       z^n / (2 n + 1), n = 0 .. 11, by Horner; x <= 0 or not finite: NaN.  acos(x): the rational approximation of fdlibm's e_acos.c (the
       three ranges |x| < 0.5, x <= -0.5, x >= 0.5; the square root is IEEE's), |x| > 1: NaN.  Measured on this file's sweeps
       (tests/test_essgraph_ref_cpu.py measures them again and asserts the bounds): log against math.log at most 3 ulp (LOG_ULP = 4 is
       asserted; the 3 are met for x near 1, where the result is 2 f P alone), acos against math.acos at most 1 ulp (ACOS_ULP = 2),
       log(exp(u)) against u, relative to |u|_inf, per branch at most 5.1e-16, 8.4e-14, 1.04e-10 and 8.9e-14 for theta up to 3 (LOGEXP_REL
       asserts 8 times each).  Branch 2 (near the identity, |sigma| >= eps) is swept over |sigma| >= 0.5 and measures the constructor, not
       the log: O4 keeps upstream's B there (wrong by 1 / sigma^3, times theta^2 < 1e-10), G10 does not.
  (G4) W^-1 t by cofactors in a fixed order (E3 / L6), not by LU: a zero determinant gives an error that is not finite.
  (G5) an error that is not finite (theta at pi, s <= 0, a zero determinant) makes the trial fail.  If it is not finite at the initial
       estimate the call evaluates nothing: status NOT_FINITE, 0 iterations, the outputs hold the initial estimate.
  (G6) every sum has one fixed shape (L5).  Per free vertex (H_ii, b_i): 64 partial sums over that vertex's edges (as v0 or as v1) in
       edge-list order, partial l adding positions l, l + 64, ..., then p[l] += p[l + s], s = 32 .. 1.  Per off-diagonal block: its edges
       one after the other in list order from +0.0 (several edges may join one pair: the reference does not deduplicate).  chi2: the
       64-partial tree over the edge list.  computeScale: the tree over the unknowns in system order.
  (G7) under fix_scale the scale column of every Jacobian is exactly zero, row 6 of every block holds lambda alone, the scale's bits never
       change (O6).
  (G8) a problem without free vertices or without edges evaluates nothing: status EMPTY (L8).
  (G9) the caller lists only keyframes that are not bad (the reference would look up a null vertex for a bad one); an edge from a
       vertex to itself is refused.
  (G10) near the identity with |sigma| >= eps, B = (((0.5 sigma^2 - sigma) + 1) s - 1) / sigma^3.  Upstream's text lacks the "- 1" (in the
       constructor too, where theta < 1e-5 hides it: O4 keeps it there); in log this branch reaches theta = 4.5e-3, B grows as 1 /
       sigma^3, W degenerates to B Omega^2 and Levenberg stalls a few iterations before the optimum of every monocular loop.
  (G11) the edge list walks the loop edges of a keyframe (GetLoopEdges) in ascending keyId.  The reference's set<Keyframe> is ordered by
       pointer, an order no restatement can have; the order of the edge list fixes the bits of every sum over it (G6).
A failed trial (G1, G5, O4's step limits) is a rejected trial whatever rho would have been.
Quirk kept (G-Q1): a step of exactly zero on a graph whose chi2 is exactly 0 has rho == 0: the rule rho > 0 rejects it and optimize()
terminates on rho == 0 - the estimate is what it was either way.
"""
import numpy as np

import _sim3opt_ref as SO
from _lba_ref import lane_sum
from _poseopt_ref import DBL_MAX, EXP_A, EXP_B, EXP_C, F64, GOOD_LOW, GOOD_UP, MAX_TRIALS, horner

EPS = SO.EPS
ONE_M_EPS = F64(1.0) - EPS
DELTA, SCALAR = SO.DELTA, SO.SCALAR
LN2_HI, LN2_LO = SO.LN2_HI, SO.LN2_LO
SQRT_HALF = F64(float.fromhex("0x1.6a09e667f3bcdp-1"))
LOG_C = [float.fromhex(h) for h in ("0x1.0000000000000p+0", "0x1.5555555555555p-2", "0x1.999999999999ap-3", "0x1.2492492492492p-3",
                                    "0x1.c71c71c71c71cp-4", "0x1.745d1745d1746p-4", "0x1.3b13b13b13b14p-4", "0x1.1111111111111p-4",
                                    "0x1.e1e1e1e1e1e1ep-5", "0x1.af286bca1af28p-5", "0x1.8618618618618p-5", "0x1.642c8590b2164p-5")]  # 1 / (2 n + 1)
PIO2_HI, PIO2_LO = F64(1.57079632679489655800e+00), F64(6.12323399573676603587e-17)
ACOS_P = [F64(v) for v in (1.66666666666666657415e-01, -3.25565818622400915405e-01, 2.01212532134862925881e-01, -4.00555345006794114027e-02,
                           7.91534994289814532176e-04, 3.47933107596021167570e-05)]
ACOS_Q = [F64(v) for v in (-2.40339491173441421878e+00, 2.02094576023350569471e+00, -6.88283971605453293030e-01, 7.70381505559019352791e-02)]
LOG_ULP, ACOS_ULP = 4, 2                              # G3: asserted; measured 3, 1
LOGEXP_REL = (4.1e-15, 6.8e-13, 8.4e-10, 7.2e-13)    # ... per branch, 8 times the measured 5.1e-16, 8.4e-14, 1.04e-10, 8.9e-14
OK, NOT_FINITE, EMPTY = 0, 1, 2                      # the status of a call
MOVED, BAD_OR_UNSET, NO_PAIR = 0, 1, 2              # the status of a point
SET, BAD = SO.SET, SO.BAD
NAN = F64("nan")


def log_f64(x):
    """G3; x an array"""
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        ok = (x > 0.0) & (x <= DBL_MAX)
        m, k = np.frexp(np.where(ok, x, F64(1.0)))
        low = m < SQRT_HALF
        m = np.where(low, m * F64(2.0), m)
        kf = (k - low).astype(F64)
        f = (m - F64(1.0)) / (m + F64(1.0))
        z = f * f
        p = F64(LOG_C[11])
        for c in LOG_C[10::-1]:
            p = p * z + F64(c)
        r = kf * LN2_HI + ((F64(2.0) * f) * p + kf * LN2_LO)
        return np.where(ok, r, NAN)


def _acos_r(z):
    p = z * (ACOS_P[0] + z * (ACOS_P[1] + z * (ACOS_P[2] + z * (ACOS_P[3] + z * (ACOS_P[4] + z * ACOS_P[5])))))
    q = F64(1.0) + z * (ACOS_Q[0] + z * (ACOS_Q[1] + z * (ACOS_Q[2] + z * ACOS_Q[3])))
    return p / q


def acos_f64(x):
    """G3; x an array"""
    x = np.asarray(x, F64)
    with np.errstate(all="ignore"):
        ok = np.abs(x) <= F64(1.0)
        xs = np.where(ok, x, F64(0.0))
        z0 = xs * xs                                              # |x| < 0.5
        a0 = PIO2_HI - (xs - (PIO2_LO - xs * _acos_r(z0)))
        z1 = (F64(1.0) + xs) * F64(0.5)                          # x <= -0.5
        s1 = np.sqrt(z1)
        w1 = _acos_r(z1) * s1 - PIO2_LO
        a1 = F64(2.0) * (PIO2_HI - (s1 + w1))
        z2 = (F64(1.0) - xs) * F64(0.5)                          # x >= 0.5
        s2 = np.sqrt(z2)
        df = (s2.view(np.uint64) & np.uint64(0xFFFFFFFF00000000)).view(F64)
        c = (z2 - df * df) / (s2 + df)
        w2 = _acos_r(z2) * s2 + c
        a2 = F64(2.0) * (df + w2)
        r = np.where(np.abs(xs) < F64(0.5), a0, np.where(xs < 0.0, a1, np.where(xs == F64(1.0), F64(0.0), a2)))
        return np.where(ok, r, NAN)


def vcompose(A, B):
    """Sim3::operator*: A * B, over arrays of Sim3 (R [n, 3, 3], t [n, 3], s [n]); the text of _sim3opt_ref.compose"""
    Ra, ta, sa = A
    Rb, tb, sb = B
    with np.errstate(all="ignore"):
        Rn = np.stack([np.stack([Ra[:, i, 0] * Rb[:, 0, j] + (Ra[:, i, 1] * Rb[:, 1, j] + Ra[:, i, 2] * Rb[:, 2, j]) for j in range(3)], 1)
                       for i in range(3)], 1)
        tn = np.stack([sa * (Ra[:, i, 0] * tb[:, 0] + (Ra[:, i, 1] * tb[:, 1] + Ra[:, i, 2] * tb[:, 2])) + ta[:, i] for i in range(3)], 1)
        return Rn, tn, sa * sb


def vinverse(E):
    """Sim3::inverse; the text of _sim3opt_ref.inverse"""
    R, t, s = E
    with np.errstate(all="ignore"):
        m = F64(-1.0) / s
        tm = [t[:, 0] * m, t[:, 1] * m, t[:, 2] * m]
        ti = np.stack([R[:, 0, i] * tm[0] + (R[:, 1, i] * tm[1] + R[:, 2, i] * tm[2]) for i in range(3)], 1)
        return np.ascontiguousarray(np.swapaxes(R, 1, 2)), ti, F64(1.0) / s


def sim3_log(E):
    """Sim3::log over an array of Sim3: (e [n, 7] = (omega, upsilon, sigma), branch [n])"""
    R, t, s = E
    one, half = F64(1.0), F64(0.5)
    with np.errstate(all="ignore"):
        sg = log_f64(s)
        d = half * ((R[:, 0, 0] + (R[:, 1, 1] + R[:, 2, 2])) - one)
        dr = [R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]]
        near = d > ONE_M_EPS
        small = np.abs(sg) < EPS
        theta = np.where(near, F64(0.0), acos_f64(np.where(near, F64(0.0), d)))
        t2 = theta * theta
        k = np.where(near, half, theta / (F64(2.0) * np.sqrt(one - d * d)))
        w0, w1, w2 = k * dr[0], k * dr[1], k * dr[2]
        hA, hB, hC = horner(EXP_A, t2), horner(EXP_B, t2), horner(EXP_C, t2)
        sg2 = sg * sg
        C = np.where(small, one, (s - one) / sg)
        A_ss = np.where(near, half, hB)                                     # |sigma| < eps
        B_ss = np.where(near, one / F64(6.0), hC)
        A_n = ((sg - one) * s + one) / sg2                                  # near the identity
        B_n = ((((half * sg2 - sg) + one) * s) - one) / (sg2 * sg)         # G10
        a = s * (theta * hA)                                                # s sin(theta)
        b = s * (one - t2 * hB)                                             # s cos(theta)
        c = t2 + sg2
        A_g = (a * sg + (one - b) * theta) / (theta * c)
        B_g = (C - ((b - one) * sg + a * theta) / c) * (one / t2)
        A = np.where(small, A_ss, np.where(near, A_n, A_g))
        B = np.where(small, B_ss, np.where(near, B_n, B_g))
        Z = np.zeros_like(w0)
        W = [[Z, -w2, w1], [w2, Z, -w0], [-w1, w0, Z]]
        W2 = [[-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2],
              [w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2],
              [w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)]]
        M = [[(C + B * W2[i][j]) if i == j else (A * W[i][j] + B * W2[i][j]) for j in range(3)] for i in range(3)]
        # G4: the cofactors cof[i][j] of M, the determinant along row 0, M^-1 = cof^T / det
        cof = [[M[(i + 1) % 3][(j + 1) % 3] * M[(i + 2) % 3][(j + 2) % 3] - M[(i + 1) % 3][(j + 2) % 3] * M[(i + 2) % 3][(j + 1) % 3]
                for j in range(3)] for i in range(3)]
        det = M[0][0] * cof[0][0] + (M[0][1] * cof[0][1] + M[0][2] * cof[0][2])
        r = one / det
        ups = [(cof[0][i] * r) * t[:, 0] + ((cof[1][i] * r) * t[:, 1] + (cof[2][i] * r) * t[:, 2]) for i in range(3)]
        e = np.stack([w0, w1, w2, ups[0], ups[1], ups[2], sg], 1)
        return e, 2 * (~small).astype(np.int64) + (~near).astype(np.int64)


def edge_error(meas, S0, S1):
    """EdgeSim3::computeError over the edges: log((C * S0) * S1^-1)"""
    return sim3_log(vcompose(vcompose(meas, S0), vinverse(S1)))


def sim3_map(E, X):
    """Sim3::map over arrays: s (R x) + t"""
    R, t, s = E
    with np.errstate(all="ignore"):
        return np.stack([s * (R[:, r, 0] * X[:, 0] + (R[:, r, 1] * X[:, 1] + R[:, r, 2] * X[:, 2])) + t[:, r] for r in range(3)], 1)


def chi2_of(e):
    with np.errstate(all="ignore"):
        c = e[:, 0] * e[:, 0]
        for r in range(1, 7):
            c = c + e[:, r] * e[:, r]
    return c


class Problem:
    """S_init: (R [nk, 3, 3], t [nk, 3], s [nk]) double; fixed: a position; v0, v1 [ne]; meas: (R, t, s) over the edges"""

    def __init__(self, S_init, fixed, v0, v1, meas, fix_scale):
        self.S0 = (np.asarray(S_init[0], F64).reshape(-1, 3, 3).copy(), np.asarray(S_init[1], F64).reshape(-1, 3).copy(),
                   np.asarray(S_init[2], F64).reshape(-1).copy())
        self.nk, self.fixed, self.fix_scale = len(self.S0[2]), int(fixed), bool(fix_scale)
        self.v0, self.v1 = np.asarray(v0, np.int64).reshape(-1), np.asarray(v1, np.int64).reshape(-1)
        self.ne = len(self.v0)
        self.meas = (np.asarray(meas[0], F64).reshape(-1, 3, 3), np.asarray(meas[1], F64).reshape(-1, 3), np.asarray(meas[2], F64).reshape(-1))
        assert 0 <= self.fixed < self.nk and np.all(self.v0 != self.v1)
        self.nf = self.nk - 1
        self.sys_of = np.array([k - (k > self.fixed) if k != self.fixed else -1 for k in range(self.nk)], np.int64)
        self.vertex_of = np.array([k for k in range(self.nk) if k != self.fixed], np.int64)
        # by vertex: the edges in list order and the side the vertex is on
        self.v_edges = [np.nonzero((self.v0 == k) | (self.v1 == k))[0] for k in self.vertex_of]
        self.pairs = {}                                   # (hi, lo) system positions -> [(edge, v0 is lo)]
        for e in range(self.ne):
            a, b = int(self.sys_of[self.v0[e]]), int(self.sys_of[self.v1[e]])
            if a >= 0 and b >= 0:
                self.pairs.setdefault((max(a, b), min(a, b)), []).append((e, a < b))
        self.cols = symbolic(self.nf, self.pairs.keys())
        self.l_blocks = self.nf + sum(len(c) for c in self.cols)
        self.n_updates = sum(len(c) * (len(c) + 1) // 2 for c in self.cols)


def symbolic(nf, pairs):
    """G1: the rows below the diagonal of every block column of L, ascending; struct(parent) receives struct(j) minus the parent"""
    struct = [set() for _ in range(nf)]
    for hi, lo in pairs:
        struct[lo].add(hi)
    cols = []
    for j in range(nf):
        rows = sorted(struct[j])
        cols.append(rows)
        if rows:
            struct[rows[0]].update(rows[1:])
    return cols


def take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


def errors_at(pr, S):
    return edge_error(pr.meas, take(S, pr.v0), take(S, pr.v1))


def perturbed(S, fix_scale):
    """per vertex the 14 estimates of a linearisation: out[d][sign] = Sim3(+-delta e_d) * S over the vertices"""
    out = []
    n = len(S[2])
    for d in range(7):
        pair = []
        for sign in (DELTA, -DELTA):
            u = [F64(0.0)] * 7
            u[d] = sign
            if fix_scale:
                u[6] = F64(0.0)
            dR, dt, ds = SO.sim3_exp(u)
            D = (np.broadcast_to(np.array(dR, F64), (n, 3, 3)), np.broadcast_to(np.array(dt, F64), (n, 3)), np.broadcast_to(F64(ds), (n,)))
            pair.append(vcompose(D, S))
        out.append(pair)
    return out


def jacobians(pr, S):
    """J0, J1 [ne, 7 (row), 7 (column d)]; the Jacobian of a fixed vertex stays 0 and is never read"""
    P = perturbed(S, pr.fix_scale)
    J0, J1 = np.zeros((pr.ne, 7, 7), F64), np.zeros((pr.ne, 7, 7), F64)
    Sa, Sb = take(S, pr.v0), take(S, pr.v1)
    with np.errstate(all="ignore"):
        for d in range(7):
            ep, _ = edge_error(pr.meas, take(P[d][0], pr.v0), Sb)
            em, _ = edge_error(pr.meas, take(P[d][1], pr.v0), Sb)
            J0[:, :, d] = SCALAR * (ep - em)
            ep, _ = edge_error(pr.meas, Sa, take(P[d][0], pr.v1))
            em, _ = edge_error(pr.meas, Sa, take(P[d][1], pr.v1))
            J1[:, :, d] = SCALAR * (ep - em)
    return J0, J1


def _jtj(Ja, Jb):
    """[ne, 7, 7]: entry (a, b) = sum_r Ja[r][a] Jb[r][b], one after the other in ascending r"""
    with np.errstate(all="ignore"):
        s = Ja[:, 0, :, None] * Jb[:, 0, None, :]
        for r in range(1, 7):
            s = s + Ja[:, r, :, None] * Jb[:, r, None, :]
    return s


class System:
    pass


def build_system(pr, S):
    """computeActiveErrors + buildSystem: H_ii [nf, 7, 7], b [nf, 7], the off-diagonal blocks {(hi, lo): [7, 7]}, chi2, finite"""
    e, _ = errors_at(pr, S)
    J0, J1 = jacobians(pr, S)
    sy = System()
    with np.errstate(all="ignore"):
        g = -e
        A00, A11, A01 = _jtj(J0, J0), _jtj(J1, J1), _jtj(J0, J1)
        g0, g1 = _jtj(J0, g[:, :, None])[:, :, 0], _jtj(J1, g[:, :, None])[:, :, 0]
        sy.Hd, sy.b = np.zeros((pr.nf, 7, 7), F64), np.zeros((pr.nf, 7), F64)
        for i, k in enumerate(pr.vertex_of):
            ed = pr.v_edges[i]
            if len(ed) == 0:
                continue
            first = (pr.v0[ed] == k)
            terms = np.concatenate([np.where(first[:, None, None], A00[ed], A11[ed]).reshape(len(ed), 49), np.where(first[:, None], g0[ed], g1[ed])], 1)
            s = lane_sum(terms, np.ones(len(ed), bool))
            sy.Hd[i], sy.b[i] = s[:49].reshape(7, 7), s[49:]
        sy.off = {}
        for key, lst in pr.pairs.items():
            blk = np.zeros((7, 7), F64)
            for ed, v0_is_lo in lst:
                blk = blk + (A01[ed].T if v0_is_lo else A01[ed])           # rows: the later vertex (hi)
            sy.off[key] = blk
        c = chi2_of(e)
        sy.chi2 = lane_sum(c, np.ones(pr.ne, bool))
        sy.finite = bool(np.all(np.isfinite(e)))
    return sy


def chol7(A):
    """the unpivoted L L^T of the lower triangle of a 7 x 7 block (L7's loops); None on a bad pivot"""
    L = np.zeros((7, 7), F64)
    with np.errstate(all="ignore"):
        for c in range(7):
            s = A[c, c]
            for k in range(c):
                s = s - L[c, k] * L[c, k]
            if not (s > 0.0 and np.isfinite(s)):
                return None
            L[c, c] = np.sqrt(s)
            for r in range(c + 1, 7):
                s = A[r, c]
                for k in range(c):
                    s = s - L[r, k] * L[c, k]
                L[r, c] = s / L[c, c]
    return L


def factor_solve(pr, sy, lam):
    """G1: x [nf, 7] or None on a bad pivot"""
    nf, cols = pr.nf, pr.cols
    with np.errstate(all="ignore"):
        D = [sy.Hd[j].copy() for j in range(nf)]
        for j in range(nf):
            for a in range(7):
                D[j][a, a] = D[j][a, a] + lam
        B = [{i: sy.off.get((i, j), np.zeros((7, 7), F64)).copy() for i in cols[j]} for j in range(nf)]
        for j in range(nf):
            Ljj = chol7(D[j])
            if Ljj is None:
                return None
            D[j] = Ljj
            for i in cols[j]:
                A, X = B[j][i], np.zeros((7, 7), F64)
                for c in range(7):
                    s = A[:, c].copy()
                    for k in range(c):
                        s = s - X[:, k] * Ljj[c, k]
                    X[:, c] = s / Ljj[c, c]
                B[j][i] = X
            for qi, i in enumerate(cols[j]):
                for k in cols[j][:qi + 1]:
                    T = D[i] if i == k else B[k][i]
                    for c in range(7):
                        T -= B[j][i][:, c, None] * B[j][k][None, :, c]
        r = sy.b.copy()
        for j in range(nf):                                                # forward, ascending
            for c in range(7):
                s = r[j, c]
                for k in range(c):
                    s = s - D[j][c, k] * r[j, k]
                r[j, c] = s / D[j][c, c]
            for i in cols[j]:
                for c in range(7):
                    r[i] = r[i] - B[j][i][:, c] * r[j, c]
        for j in range(nf - 1, -1, -1):                                    # back, descending
            s = r[j].copy()
            for i in cols[j][::-1]:
                for c in range(6, -1, -1):
                    s = s - B[j][i][c, :] * r[i, c]
            for a in range(6, -1, -1):
                v = s[a]
                for k in range(6, a, -1):
                    v = v - D[j][k, a] * r[j, k]
                r[j, a] = v / D[j][a, a]
    return r


def dense_system(pr, sy, lam):
    """the assembled dense H + lam I and b (for the dense twin)"""
    n = 7 * pr.nf
    H = np.zeros((n, n), F64)
    for j in range(pr.nf):
        H[7 * j:7 * j + 7, 7 * j:7 * j + 7] = sy.Hd[j]
    for (hi, lo), blk in sy.off.items():
        H[7 * hi:7 * hi + 7, 7 * lo:7 * lo + 7] = blk
        H[7 * lo:7 * lo + 7, 7 * hi:7 * hi + 7] = blk.T
    return H + lam * np.eye(n), sy.b.reshape(-1).copy()


def dense_solve(pr, sy, lam):
    """the dense twin of factor_solve: numpy.linalg on the assembled system; None when it is not positive definite"""
    H, b = dense_system(pr, sy, lam)
    try:
        with np.errstate(all="ignore"):
            if not np.all(np.isfinite(H)):
                return None
            np.linalg.cholesky(H)
            return np.linalg.solve(H, b).reshape(pr.nf, 7)
    except np.linalg.LinAlgError:
        return None


class Result:
    pass


def optimize(pr, iterations=20, lambda_init=1e-16, log=None, solver=factor_solve):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg::solve.  Returns a Result: S (R, t, s), iterations,
    trials, chi2_first, chi2_last, lam, l_blocks, status.  log (a list) receives one dict per trial"""
    res = Result()
    S = tuple(a.copy() for a in pr.S0)
    res.iterations = res.trials = 0
    res.chi2_first = res.chi2_last = res.lam = F64(0.0)
    res.l_blocks, res.status = pr.l_blocks, OK
    res.S = S
    if pr.nf == 0 or pr.ne == 0 or iterations <= 0:                         # G8
        res.status = EMPTY
        return res
    lam, ni, cur = F64(lambda_init), F64(2.0), F64(0.0)
    for it in range(iterations):
        sy = build_system(pr, S)
        cur = sy.chi2
        if it == 0:
            if not sy.finite:                                               # G5
                res.status = NOT_FINITE
                return res
            res.chi2_first = cur
        res.iterations += 1
        rho, qmax = F64(0.0), 0
        while True:
            res.trials += 1
            x = solver(pr, sy, lam)
            why, new = ("pivot" if x is None else ""), None
            if x is not None:
                Rn, tn, sn = S[0].copy(), S[1].copy(), S[2].copy()
                for i, k in enumerate(pr.vertex_of):
                    st = SO.step((S[0][k], S[1][k], S[2][k]), x[i], pr.fix_scale)
                    if st is None:
                        why = "exp"
                        break
                    Rn[k], tn[k], sn[k] = st
                else:
                    new = (Rn, tn, sn)
                    en, _ = errors_at(pr, new)
                    if not np.all(np.isfinite(en)):
                        why, new = "error", None
            failed = new is None
            accepted = False
            with np.errstate(all="ignore"):
                if failed:
                    rho, temp = F64(-1.0), F64(DBL_MAX)
                else:
                    temp = lane_sum(chi2_of(en), np.ones(pr.ne, bool))
                    xs, bs = x.reshape(-1), sy.b.reshape(-1)
                    scale = lane_sum(xs * (lam * xs + bs), np.ones(len(xs), bool)) + F64(1e-3)   # computeScale
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
                    S = new
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
    res.S, res.chi2_last, res.lam = S, cur, lam
    return res


def recover(S):
    """:979-998: Tiw [nk, 12] = [R | t * (1 / s)] in double, its float cast, correctedSwc = S^-1"""
    R, t, s = S
    with np.errstate(all="ignore"):
        inv_s = F64(1.0) / s
        Tiw = np.concatenate([R.reshape(-1, 9), t * inv_s[:, None]], 1)
    return Tiw, Tiw.astype(np.float32), vinverse(S)


def correct_points(pos, flags, ids, pair_of_point, S_from, S_to):
    """:1000-1030 / LoopClosing.cc:487-516 over a store (pos [cap, 3] float32, flags [cap]): P' = float(S_to.map(S_from.map(double(P)))) of
    point ids[i] with pair pair_of_point[i].  Returns (xyz [n, 3] float64, 0 where nothing moved; status [n]); pos is updated in place"""
    n = len(ids)
    xyz, status = np.zeros((n, 3), F64), np.zeros(n, np.uint8)
    for i in range(n):
        f, q = int(flags[ids[i]]), int(pair_of_point[i])
        if not (f & SET) or (f & BAD):
            status[i] = BAD_OR_UNSET
        elif q < 0:
            status[i] = NO_PAIR
    mv = np.nonzero(status == MOVED)[0]
    if len(mv):
        q = np.asarray(pair_of_point, np.int64)[mv]
        P = pos[np.asarray(ids, np.int64)[mv]].astype(F64)
        out = sim3_map(take(S_to, q), sim3_map(take(S_from, q), P))
        xyz[mv] = out
        with np.errstate(all="ignore"):
            pos[np.asarray(ids, np.int64)[mv]] = out.astype(np.float32)
    return xyz, status


def essential_graph(pr, iterations=20, lambda_init=1e-16, log=None):
    """the whole call without the store: optimize, recover"""
    res = optimize(pr, iterations, lambda_init, log)
    res.Tiw, res.Tiw_f, res.Swc = recover(res.S)
    return res


def _one(E):
    return E[0][None], E[1][None], np.asarray(E[2], F64).reshape(1)


def relative(Sjw, Siw):
    """Sji = Sjw * Siw^-1 of two single Sim3 (R [3, 3], t [3], s)"""
    R, t, s = vcompose(_one(Sjw), vinverse(_one(Siw)))
    return R[0], t[0], F64(s[0])


def essential_graph_edges(key_ids, parent, loop_edges, covisibles, loop_connections, Scw, non_corrected, loop_id, cur_id, min_feat=100, rules=None):
    """:835-971 over plain inputs.  key_ids: the keyIds of the keyframes that are not bad, ascending (vpKFs; G9); parent {id: id or None};
    loop_edges {id: set of ids}; covisibles {id: [ids]} = GetCovisiblesByWeight(minFeat) in its order; loop_connections {id: [(id_j, weight
    of the pair)]}, walked in ascending id as the reference's maps are; Scw {id: Sim3} = vScw; non_corrected {id: Sim3}.  Returns [(id_i, id_j,
    measurement)] with id_i the vertex of setVertex(0, ...).  rules: a set of rule names a twin switches OFF (the tests flip each rule)"""
    off = rules or set()
    ids = set(key_ids)
    out, inserted = [], set()
    for i in sorted(loop_connections):                                      # :839-868
        for j, w in sorted(loop_connections[i], key=lambda c: c[0]):
            if "min_feat" not in off and (i != cur_id or j != loop_id) and w < min_feat:
                continue
            out.append((i, j, relative(Scw[j], Scw[i])))
            inserted.add((min(i, j), max(i, j)))
    for i in key_ids:                                                       # :870-971
        Siw = non_corrected[i] if i in non_corrected else Scw[i]
        pick = lambda j: non_corrected[j] if j in non_corrected else Scw[j]
        p = parent.get(i)
        if p is not None:                                                   # the spanning tree
            out.append((i, p, relative(pick(p), Siw)))
        le = loop_edges.get(i, ())
        for j in sorted(le):                                                # G11
            if "loop_lower" in off or j < i:
                out.append((i, j, relative(pick(j), Siw)))
        for n in covisibles.get(i, ()):
            if "not_parent" not in off and n == p:
                continue
            if "not_child" not in off and parent.get(n) == i:
                continue
            if "not_loop_edge" not in off and n in le:
                continue
            if n not in ids or not ("cov_lower" in off or n < i):
                continue
            if "inserted" not in off and (min(i, n), max(i, n)) in inserted:
                continue
            out.append((i, n, relative(pick(n), Siw)))
    return out
