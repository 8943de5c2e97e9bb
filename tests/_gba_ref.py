"""Normative restatement of afv_table_global_bundle_adjust (csrc/k_gba.hip) and afv_points_correct_se3: Optimizer::GlobalBundleAdjustemnt
(src/Optimizer.cc:53-58) as LoopClosing::RunGlobalBundleAdjustment calls it, and the float point correction that follows it
(LoopClosing.cc:731-750).

Everything is tests/_lba_ref.py - L-Q1, L1 to L6, L8, L9, the order of every sum - with ONE amendment:

  (L7') the reduced system is block-sparse in 6 x 6 blocks over the free keyframes, in the order of the caller's list.  Block (i, j) is
        STRUCTURAL when some listed point has an edge to both keyframes, taken from the edge list as given: before points are dropped and
        before a check removes edges.  The pattern is therefore a superset, and a block that became empty holds exact zeros.  The
        factorisation is the unpivoted L L^T of L7 restricted to the SYMBOLIC FILL of that order (struct(parent) receives struct(j)
        without the parent, parent = the first row below the diagonal of column j): every scalar element subtracts its products one after
        the other in ascending k, exactly as solve_dense does; a product with a factor in a block outside the fill is skipped.  The forward
        substitution ascends, the back substitution descends, each product by product.  A pivot that is not positive and finite is a
        failed trial.  A free keyframe without active edges stays in the system with lambda on its diagonal.

On finite data L7' gives the doubles of L7: a skipped product is s - (+-0), which changes nothing unless s is -0.0.
tests/test_gba_ref_cpu.py proves the equality, byte for byte, at every solve of every small scene; where a zero sign ever differed, this
file would be normative for the new entry point.

correct_se3 is numpy.float32 with one rounding per operator: each row ((R[r][0] * x + R[r][1] * y) + R[r][2] * z) + t[r]; first with
(Rcw, tcw) before the BA, then with (Rwc, twc) after it, as the host's GetPoseInverse() holds them.  Parity with the reference's cv::Mat
product is UNPINNED.
"""
import numpy as np

import _lba_ref as L

F64, F32 = np.float64, np.float32
MOVED, BAD_OR_UNSET, NO_PAIR = 0, 1, 2


class Plan:
    """nf; structural {(lo, hi)}; rows[j]: the rows below the diagonal of column j of L, ascending; the block list by columns: col_ptr
    [nf + 1], blk_row, blk_col, blk_kind [nb] (1: a structural block of S, the diagonal blocks included; 0: fill)"""


def make_plan(nf, npts, e_pt, e_kf):
    pl = Plan()
    pl.nf = nf
    by_point = [[] for _ in range(npts)]
    for p, k in zip(e_pt, e_kf):
        if k < nf:
            by_point[int(p)].append(int(k))
    pl.structural = set()
    for ks in by_point:
        for x in range(len(ks)):
            for y in range(x + 1, len(ks)):
                pl.structural.add((min(ks[x], ks[y]), max(ks[x], ks[y])))
    rows = [sorted(hi for lo, hi in pl.structural if lo == j) for j in range(nf)]
    for j in range(nf):                                 # the symbolic factorisation in list order
        r = rows[j]
        if len(r) > 1:
            rows[r[0]] = sorted(set(rows[r[0]]) | set(r[1:]))
    pl.rows = rows
    pl.col_ptr, pl.blk_row, pl.blk_col, pl.blk_kind = [0], [], [], []
    for j in range(nf):
        pl.blk_row.append(j); pl.blk_col.append(j); pl.blk_kind.append(1)
        for i in rows[j]:
            pl.blk_row.append(i); pl.blk_col.append(j); pl.blk_kind.append(1 if (j, i) in pl.structural else 0)
        pl.col_ptr.append(len(pl.blk_row))
    pl.nb, pl.ns = len(pl.blk_row), int(sum(pl.blk_kind))
    pl.fill = {(i, j) for j in range(nf) for i in rows[j]} | {(j, j) for j in range(nf)}   # (row block, column block) of L
    return pl


def plan_of(pr):
    return make_plan(pr.nf, pr.np, pr.e_pt, pr.e_kf)


def solve_block_sparse(S, b, pl):
    """L7' on the upper triangle of S; None on a bad pivot.  The loops are solve_dense's; a product is formed only when both factors lie
    in a block of the fill, an element of L only when its block does"""
    n = len(b)
    inside = pl.fill
    L_ = np.zeros((n, n), F64)
    cols = [[k for k in range(i + 1) if (i, k) in inside] for i in range(pl.nf)]            # the column blocks of row block i
    common = {}

    def ks(bi, bj, upto):
        """the scalar k < upto at which both L[6 bi + ., k] and L[6 bj + ., k] lie in the fill, ascending"""
        if (bi, bj) not in common:
            sj = set(cols[bj])
            common[(bi, bj)] = [K for K in cols[bi] if K in sj]
        out = []
        for K in common[(bi, bj)]:
            out.extend(range(6 * K, min(6 * K + 6, upto)))
        return out

    with np.errstate(all="ignore"):
        for j in range(n):
            bj = j // 6
            s = S[j, j]
            for k in ks(bj, bj, j):
                s = s - L_[j, k] * L_[j, k]
            if not (s > 0.0 and np.isfinite(s)):
                return None
            L_[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                bi = i // 6
                if (bi, bj) not in inside:
                    continue
                s = S[j, i]
                for k in ks(bi, bj, j):
                    s = s - L_[i, k] * L_[j, k]
                L_[i, j] = s / L_[j, j]
        x = np.zeros(n, F64)
        for i in range(n):
            bi = i // 6
            s = b[i]
            for K in cols[bi]:
                for k in range(6 * K, min(6 * K + 6, i)):
                    s = s - L_[i, k] * x[k]
            x[i] = s / L_[i, i]
        below = [[i for i in range(j, pl.nf) if (i, j) in inside] for j in range(pl.nf)]     # the row blocks of column block j
        for i in range(n - 1, -1, -1):
            bi = i // 6
            s = x[i]
            for K in reversed(below[bi]):
                for k in range(6 * K + 5, max(6 * K - 1, i), -1):
                    s = s - L_[k, i] * x[k]
            x[i] = s / L_[i, i]
    return x


def bundle_adjust(pr, iterations=(5, 10), robust=(True, False), checks=True, stop_at=None, log=None, solves=None):
    """_lba_ref.bundle_adjust with every solve of the reduced system routed to solve_block_sparse: the module's solve_dense is swapped for
    the duration of the call.  solves: a list that receives (sparse answer, dense answer) of every solve (None: a bad pivot)"""
    pl = plan_of(pr)
    dense = L.solve_dense

    def routed(S, b):
        x = solve_block_sparse(S, b, pl)
        if solves is not None:
            solves.append((x, dense(S, b)))
        return x

    L.solve_dense = routed
    try:
        return L.bundle_adjust(pr, iterations, robust, checks, stop_at, log)
    finally:
        L.solve_dense = dense


def se3_apply(T, X):
    """T [12] float32 (R row-major, t), X [3] float32: one rounding per operator"""
    T, X = np.asarray(T, F32), np.asarray(X, F32)
    with np.errstate(all="ignore"):
        return np.array([((T[3 * r] * X[0] + T[3 * r + 1] * X[1]) + T[3 * r + 2] * X[2]) + T[9 + r] for r in range(3)], F32)


def correct_se3(pos, ok, pair, T_before, T_after):
    """pos [n, 3] float32, ok [n] (set and not bad), pair [n]; T_before / T_after [m, 12] float32 -> (pos', status [n])"""
    pos = np.asarray(pos, F32).reshape(-1, 3).copy()
    T_before, T_after = np.asarray(T_before, F32).reshape(-1, 12), np.asarray(T_after, F32).reshape(-1, 12)
    st = np.zeros(len(pos), np.uint8)
    for i in range(len(pos)):
        if not ok[i]:
            st[i] = BAD_OR_UNSET
        elif pair[i] < 0:
            st[i] = NO_PAIR
        else:
            pos[i] = se3_apply(T_after[pair[i]], se3_apply(T_before[pair[i]], pos[i]))
    return pos, st
