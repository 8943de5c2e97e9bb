"""Plain-Python restatement of the reference's projection-guided searches, with a trace.  TEST INFRASTRUCTURE ONLY.

A second opinion next to oracle/afvo.c (written by the same hand as the kernels), as _kfdb_ref.py is for place recognition.  Restated from
the reference's source, not from the oracle:

  SearchByProjection(F, vpMapPoints, th)             FeatureMatcher.cc:73-154      match_projection(..., last_frame=False)
  SearchByProjection(pKF, Scw, vpPoints, vpMatched)  :287-397                      match_projection(..., last_frame=True), no stereo
  SearchForInitialization                            :399-557 (active code :479-)  match_initialization
  Fuse(pKF, vpMapPoints, th)                         :794-940                      match_projection(..., fuse=True), F.inf set
  Fuse(pKF, Scw, ...)                                :944-1064                     match_projection(..., fuse=True), F.inf None
  SearchBySim3                                       :1066-1287                    match_sim3
  SearchByProjection(CurrentFrame, LastFrame)        :1291-1402                    match_projection(..., last_frame=True)
  SearchByProjection(CurrentFrame, pKF, sAlready..)  :1406-1506                    match_projection(..., last_frame=True), no stereo
  rotation histogram                                 :1579-1668
  Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea   Frame.cc:225-240, :384-394, :333-382
  KeyFrame::GetFeaturesInArea                        KeyFrame.cc:613-652

Inputs are the FrameGridView / ProjectionQueries objects oracle.match_projection takes; outputs are the same arrays and counts plus a
trace dict.  Every product and difference the reference does in `float` is done on np.float32 scalars; the comparisons against the double
literals 5.99 / 7.8 are done in double.

`flip="rule"` turns ONE comparison of the restatement around (FLIPS below).  tests/test_proj_ref_cpu.py uses it to prove that a scene's outcome
depends on the rule the scene is named after.
"""
import math

import numpy as np

f32 = np.float32
HISTO_LENGTH = 30  # FeatureMatcher.cc:64

# rule -> what the flipped restatement does instead
FLIPS = {
    "dx_lt_r": "|dx| < r  ->  |dx| <= r (Frame.cc:375)",
    "dy_lt_r": "|dy| < r  ->  |dy| <= r",
    "size_lt_min": "size < minSize  ->  size <= minSize (Frame.cc:367)",
    "size_gt_max": "size > maxSize  ->  size >= maxSize (Frame.cc:369)",
    "pos_round": "round() half away from zero  ->  half towards zero (Frame.cc:386-387)",
    "win_floor": "floor() that lands on a cell border  ->  the cell after it (Frame.cc:339, :347)",
    "win_ceil": "ceil() that lands on a cell border  ->  the cell before it (Frame.cc:343, :351)",
    "skip_cx0": "nMinCellX >= COLS  ->  >= COLS - 1", "skip_cx1": "nMaxCellX < 0  ->  <= 0",
    "skip_cy0": "nMinCellY >= ROWS  ->  >= ROWS - 1", "skip_cy1": "nMaxCellY < 0  ->  <= 0",
    "uright_gt0": "mvuRight > 0  ->  >= 0 (FeatureMatcher.cc:114, :1367)",
    "uright_ge0": "mvuRight >= 0  ->  > 0 (Fuse, :880)",
    "er_gt_max": "er > gate  ->  er >= gate (:117, :1371)",
    "best_le_th": "bestDist <= TH  ->  < TH",
    "ratio_gt": "bestDist > ratio * bestDist2 rejects  ->  >= rejects (:143)",
    "init_ratio_lt": "bestDist < bestDist2 * ratio accepts  ->  <= accepts (:528)",
    "size_ratio_lt_tol": "bestSize / bestSize2 < sizeTolerance  ->  <= (:142)",
    "size_ratio_gt_inv": "bestSize / bestSize2 > invSizeTolerance  ->  >= (:142)",
    "tie_first": "descDist < bestDist  ->  <= (the last of equals wins)",
    "d_lt_best2": "descDist < bestDist2  ->  <= (:132, :520)",
    "mdist_le": "vMatchedDistance <= descDist skips  ->  < skips (:511)",
    "steal_hist_stays": "a robbed query's histogram entry stays  ->  is removed (:530-541)",
    "rot_round": "round(rot * rotFactor) half away from zero  ->  half towards zero (:1594)",
    "rot_wrap": "bin == 30 -> 0  ->  29 (:1595)",
    "rot_lt0": "rot < 0 adds 360  ->  rot <= 0 adds 360 (:1592)",
    "max_first": "s > max: the first of equal bins wins  ->  >= : the last wins (:1636-1652)",
    "max2_lt": "max2 < 0.1f * max1 drops  ->  <= drops (:1659)",
    "max3_lt": "max3 < 0.1f * max1 drops  ->  <= drops (:1664)",
}


def _round_half_away(v):
    """C round() of a float: halves go away from zero"""
    v = float(v)
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def _round_half_toward(v):
    v = float(v)
    return int(math.ceil(abs(v) - 0.5)) * (1 if v >= 0 else -1)


def hamming(a, rows):
    """cv::norm(a, b, NORM_HAMMING) / the SWAR popcount of Feature_orb32.cpp:67-84: the number of differing bits"""
    if len(rows) == 0:
        return np.zeros(0, np.float32)
    return np.unpackbits(np.bitwise_xor(rows, a[None, :]), axis=1).sum(axis=1).astype(np.float32)


def l2sqr(a, rows):
    """cv::norm(a, b, NORM_L2SQR) of CV_32F rows as oracle.l2sqr documents it (normL2Sqr<float, double>): float differences, squares in
    double, four squares at a time added left to right, each group of four added to ONE double accumulator in order, the remainder one by
    one, narrowed to Descriptor_Distance_Type = float at the end.  The order is part of the result, so it is kept: np.cumsum walks an axis
    sequentially (np.sum adds pairwise)."""
    if len(rows) == 0:
        return np.zeros(0, np.float32)
    v = (a[None, :] - rows).astype(np.float64)
    n4 = v.shape[1] // 4 * 4
    q = v[:, :n4].reshape(len(rows), -1, 4) ** 2
    groups = ((q[:, :, 0] + q[:, :, 1]) + q[:, :, 2]) + q[:, :, 3]
    terms = np.concatenate([groups, v[:, n4:] ** 2], axis=1)
    s = np.cumsum(terms, axis=1)[:, -1] if terms.shape[1] else np.zeros(len(rows))
    return s.astype(np.float32)


# the float distance every restatement built on this file evaluates (_bow_ref, _stereo_ref): tests/_l2_scenes.arithmetic() puts a wrong
# arithmetic here to prove that a scene's outcome depends on the right one
DISTANCE = {"l2sqr": l2sqr}


def _distances(F, Q, q, idxs):
    rows = F.descriptors[np.asarray(idxs, np.int64)] if len(idxs) else F.descriptors[:0]
    if F.descriptors.dtype.kind == "f":
        return DISTANCE["l2sqr"](Q.descriptors[q], rows)
    return hamming(Q.descriptors[q], rows)


def build_grid(F, flip=None):
    """Frame::AssignFeaturesToGrid with PosInGrid: mGrid[ix][iy] = feature indices in ascending order"""
    cols, rows = int(F.grid_cols), int(F.grid_rows)
    grid = [[[] for _ in range(rows)] for _ in range(cols)]
    rnd = _round_half_toward if flip == "pos_round" else _round_half_away
    half = 0
    for i in range(F.N):
        vx = (f32(F.x[i]) - F.min_x) * F.grid_inv_w
        vy = (f32(F.y[i]) - F.min_y) * F.grid_inv_h
        if abs(float(vx)) % 1.0 == 0.5 or abs(float(vy)) % 1.0 == 0.5:
            half += 1
        px, py = rnd(vx), rnd(vy)
        if px < 0 or px >= cols or py < 0 or py >= rows:
            continue
        grid[px][py].append(i)
    return grid, half


def _window(F, x, y, r, tr, flip):
    """the four cell bounds of GetFeaturesInArea, or None when one of its four early returns fires"""
    cols, rows = int(F.grid_cols), int(F.grid_rows)

    def lo(v):
        fl = math.floor(float(v))
        if float(v) == fl:
            tr["eq"]["win_floor"] += 1
            if flip == "win_floor":
                fl += 1
        return int(fl)

    def hi(v):
        ce = math.ceil(float(v))
        if float(v) == ce:
            tr["eq"]["win_ceil"] += 1
            if flip == "win_ceil":
                ce -= 1
        return int(ce)

    raw = lo((x - F.min_x - r) * F.grid_inv_w)
    cx0 = max(0, raw)
    tr["clip"]["left"] += raw < 0
    tr["eq"]["skip_cx0"] += cx0 == cols - 1   # the last column that is still searched
    if cx0 >= (cols - 1 if flip == "skip_cx0" else cols):
        tr["skip"]["cx0"] += 1
        return None
    raw = hi((x - F.min_x + r) * F.grid_inv_w)
    cx1 = min(cols - 1, raw)
    tr["clip"]["right"] += raw > cols - 1
    tr["eq"]["skip_cx1"] += cx1 == 0
    if (cx1 <= 0) if flip == "skip_cx1" else (cx1 < 0):
        tr["skip"]["cx1"] += 1
        return None
    raw = lo((y - F.min_y - r) * F.grid_inv_h)
    cy0 = max(0, raw)
    tr["clip"]["top"] += raw < 0
    tr["eq"]["skip_cy0"] += cy0 == rows - 1
    if cy0 >= (rows - 1 if flip == "skip_cy0" else rows):
        tr["skip"]["cy0"] += 1
        return None
    raw = hi((y - F.min_y + r) * F.grid_inv_h)
    cy1 = min(rows - 1, raw)
    tr["clip"]["bottom"] += raw > rows - 1
    tr["eq"]["skip_cy1"] += cy1 == 0
    if (cy1 <= 0) if flip == "skip_cy1" else (cy1 < 0):
        tr["skip"]["cy1"] += 1
        return None
    return cx0, cx1, cy0, cy1


def _area(F, grid, q, Q, tr, flip, with_size):
    """Frame::GetFeaturesInArea (with_size) / KeyFrame::GetFeaturesInArea: vIndices in the reference's visiting order (ix outer, iy inner,
    cell order), or None for an early return"""
    x, y, r = f32(Q.u[q]), f32(Q.v[q]), f32(Q.r[q])
    w = _window(F, x, y, r, tr, flip)
    if w is None:
        return None
    cx0, cx1, cy0, cy1 = w
    mn, mx = f32(Q.min_size[q]), f32(Q.max_size[q])
    out = []
    chunk_cells, chunk_n, chunk_max = 0, 0, 0
    for ix in range(cx0, cx1 + 1):
        for iy in range(cy0, cy1 + 1):
            cell = grid[ix][iy]
            chunk_n += len(cell)
            chunk_cells += 1
            if chunk_cells == 256:  # candidates of 256 cells in visiting order (see test_proj_ref_cpu.PW_LIST)
                chunk_max = max(chunk_max, chunk_n)
                tr["chunk_counts"].add(chunk_n)
                chunk_cells = chunk_n = 0
            for i in cell:
                tr["visits"] += 1
                if with_size:
                    sz = f32(F.sizes[i])
                    if sz == mn:
                        tr["eq"]["size_lt_min"] += 1
                    if (sz <= mn) if flip == "size_lt_min" else (sz < mn):
                        tr["drop"]["size_low"] += 1
                        continue
                    if sz == mx:
                        tr["eq"]["size_gt_max"] += 1
                    if (sz >= mx) if flip == "size_gt_max" else (sz > mx):
                        tr["drop"]["size_high"] += 1
                        continue
                dx = abs(f32(F.x[i]) - x)
                dy = abs(f32(F.y[i]) - y)
                if dx == r:
                    tr["eq"]["dx_lt_r"] += 1
                if not ((dx <= r) if flip == "dx_lt_r" else (dx < r)):
                    tr["drop"]["dx"] += 1
                    continue
                if dy == r:
                    tr["eq"]["dy_lt_r"] += 1
                if not ((dy <= r) if flip == "dy_lt_r" else (dy < r)):
                    tr["drop"]["dy"] += 1
                    continue
                out.append(i)
    tr["chunk_max"] = max(tr["chunk_max"], chunk_max, chunk_n)
    tr["chunk_counts"].add(chunk_n)
    return out


def _new_trace(nq):
    return {"ncand": np.zeros(nq, np.int64), "rank": np.full(nq, -1, np.int64), "live": np.zeros(nq, bool),
            "key_rank": np.full(nq, -1, np.int64), "visits": 0, "chunk_max": 0, "chunk_counts": set(), "half_cells": 0,
            "skip": dict(cx0=0, cx1=0, cy0=0, cy1=0), "clip": dict(left=0, right=0, top=0, bottom=0),
            "drop": dict(size_low=0, size_high=0, dx=0, dy=0, occupied=0, stereo=0, chi2_2dof=0, chi2_3dof=0, mdist=0),
            "eq": {k: 0 for k in FLIPS}, "ratio_skipped": 0, "steals": 0, "hist": [0] * HISTO_LENGTH, "maxima": (-1, -1, -1),
            "rule01": 0, "wraps": 0, "longest_chain": 0, "starved": 0, "accepted": 0}


def _rank(d_all, pos):
    """rank of candidate `pos` among all filtered candidates by (distance, visiting order)"""
    d = d_all[pos]
    return int(np.sum(d_all < d) + np.sum(d_all[:pos] == d))


# ---- rotation histogram (FeatureMatcher.cc:1579-1668) ----
def rotation_bin(a1, a2, tr, flip=None):
    rot_factor = f32(1.0) / f32(HISTO_LENGTH)
    rot = f32(a1) - f32(a2)
    if rot == 0:
        tr["eq"]["rot_lt0"] += 1
    if (rot <= 0.0) if flip == "rot_lt0" else (rot < 0.0):
        rot = rot + f32(360.0)
    v = rot * rot_factor
    if abs(float(v)) % 1.0 == 0.5:
        tr["eq"]["rot_round"] += 1
    b = (_round_half_toward if flip == "rot_round" else _round_half_away)(v)
    if b == HISTO_LENGTH:
        tr["wraps"] += 1
        tr["eq"]["rot_wrap"] += 1
        b = HISTO_LENGTH - 1 if flip == "rot_wrap" else 0
    assert 0 <= b < HISTO_LENGTH, "rotation bin %d: the reference asserts here (:1597)" % b
    return b


def three_maxima(sizes, tr, flip=None):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    gt = (lambda a, b: a >= b and a > 0) if flip == "max_first" else (lambda a, b: a > b)
    for i, s in enumerate(sizes):
        if s > 0 and s in (max1, max2, max3):
            tr["eq"]["max_first"] += 1
        if gt(s, max1):
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif gt(s, max2):
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif gt(s, max3):
            max3, ind3 = s, i
    lim = f32(0.1) * f32(max1)  # 0.1f * (float)max1; the int on the left is converted to float for the comparison
    if f32(max2) == lim and max1 > 0:
        tr["eq"]["max2_lt"] += 1
    if (f32(max2) <= lim) if flip == "max2_lt" else (f32(max2) < lim):
        ind2 = ind3 = -1
        tr["rule01"] = 1
    else:
        if f32(max3) == lim and max1 > 0:
            tr["eq"]["max3_lt"] += 1
        if (f32(max3) <= lim) if flip == "max3_lt" else (f32(max3) < lim):
            ind3 = -1
            tr["rule01"] = 2
    tr["hist"] = list(sizes)
    tr["maxima"] = (ind1, ind2, ind3)
    return ind1, ind2, ind3


def _stereo_ok(F, Q, q, idx, flip):
    """the stereo gate of the projection searches alone (no counters): True when feature idx is not dropped by it"""
    u_right = getattr(F, "u_right", None)
    if u_right is None:
        return True
    ur = f32(u_right[idx])
    if not ((ur >= 0) if flip == "uright_gt0" else (ur > 0)):
        return True
    er, gate = abs(f32(Q.ur[q]) - ur), f32(Q.er_max[q])
    return not ((er >= gate) if flip == "er_gt_max" else (er > gate))


def match_projection(F, Q, th_high=75.0, nnratio=0.8, check_orientation=False, last_frame=False, fuse=False, flip=None):
    """-> (assign[F.N] = query now stored in F.pts[i] | -1, nmatches, trace); fuse: (bestIdx[Q.n] | -1, nFused, trace)"""
    assert flip is None or flip in FLIPS, flip
    if fuse:
        return _fuse(F, Q, th_high, flip)
    tr = _new_trace(Q.n)
    grid, tr["half_cells"] = build_grid(F, flip)
    tr["eq"]["pos_round"] = tr["half_cells"]
    th, ratio = f32(th_high), f32(nnratio)
    tol, inv_tol = f32(F.sizeTolerance), f32(F.invSizeTolerance)
    occ = np.zeros(F.N, bool) if F.occupied is None else (np.asarray(F.occupied) != 0)
    before = occ.copy()
    taker = np.full(F.N, -1, np.int64)   # the query of this call that occupies feature i
    depth = np.zeros(Q.n, np.int64)      # dependency chain behind query q
    assign = np.full(F.N, -1, np.int32)
    nmatches = 0
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    u_right = getattr(F, "u_right", None)
    stereo = u_right is not None
    for q in range(Q.n):
        if Q.valid is not None and not Q.valid[q]:
            continue
        cand = _area(F, grid, q, Q, tr, flip, True)
        if cand is None or not cand:
            continue
        tr["ncand"][q] = len(cand)
        d_all = _distances(F, Q, q, cand)
        # what the kernels' key lists are drawn from: the candidates that were free before the call and pass the stereo gate; a query is
        # "live" in the ordered phase when the best of them is within the threshold (k_project.hip, "live queries")
        keyset = [p for p, i in enumerate(cand) if not before[i] and _stereo_ok(F, Q, q, i, flip)]
        tr["live"][q] = bool(keyset) and bool(d_all[keyset].min() <= th)
        best = best2 = f32(np.finfo(np.float32).max)
        best_size = best_size2 = f32(-1.0)
        best_pos = -1
        nfree = 0
        for pos, idx in enumerate(cand):
            if occ[idx]:
                tr["drop"]["occupied"] += 1
                continue
            if stereo:
                ur = f32(u_right[idx])
                if ur == 0:
                    tr["eq"]["uright_gt0"] += 1
                if (ur >= 0) if flip == "uright_gt0" else (ur > 0):
                    er = abs(f32(Q.ur[q]) - ur)
                    gate = f32(Q.er_max[q])
                    if er == gate:
                        tr["eq"]["er_gt_max"] += 1
                    if (er >= gate) if flip == "er_gt_max" else (er > gate):
                        tr["drop"]["stereo"] += 1
                        continue
            nfree += 1
            d = d_all[pos]
            if d == best:
                tr["eq"]["tie_first"] += 1
            if (d <= best) if flip == "tie_first" else (d < best):
                best2, best, best_pos = best, d, pos
                best_size2, best_size = best_size, f32(F.sizes[idx])
            elif not last_frame:
                if d == best2:
                    tr["eq"]["d_lt_best2"] += 1
                if (d <= best2) if flip == "d_lt_best2" else (d < best2):
                    best2, best_size2 = d, f32(F.sizes[idx])
        # the chain behind q: the earlier query of this call that holds the feature q would have liked most
        # (features occupied before the call never take part)
        order = [p for p in np.lexsort((np.arange(len(cand)), d_all)) if not before[cand[p]]]
        if order and taker[cand[order[0]]] >= 0 and occ[cand[order[0]]]:
            depth[q] = depth[taker[cand[order[0]]]] + 1
        if (best_pos < 0 or best > th) and len(cand) > 4 and any(taker[i] >= 0 and d_all[p] <= th for p, i in enumerate(cand)):
            tr["starved"] += 1  # unmatched only because earlier queries of this call hold every candidate within the threshold
        if best_pos < 0:
            continue
        if best == th:
            tr["eq"]["best_le_th"] += 1
        if not ((best < th) if flip == "best_le_th" else (best <= th)):
            continue
        if not last_frame:
            with np.errstate(all="ignore"):
                sr = best_size / best_size2
            if sr == tol:
                tr["eq"]["size_ratio_lt_tol"] += 1
            if sr == inv_tol:
                tr["eq"]["size_ratio_gt_inv"] += 1
            c1 = (sr <= tol) if flip == "size_ratio_lt_tol" else (sr < tol)
            c2 = (sr >= inv_tol) if flip == "size_ratio_gt_inv" else (sr > inv_tol)
            if c1 and c2 and best_size2 > 0.0:
                lim = ratio * best2
                if best == lim:
                    tr["eq"]["ratio_gt"] += 1
                if (best >= lim) if flip == "ratio_gt" else (best > lim):
                    continue
            else:
                tr["ratio_skipped"] += 1
        idx = cand[best_pos]
        tr["rank"][q] = _rank(d_all, best_pos)
        tr["key_rank"][q] = _rank(d_all[keyset], keyset.index(best_pos))   # its place in a key list of unlimited length
        tr["accepted"] += 1
        assign[idx] = q
        nmatches += 1
        if Q.occupies is None or Q.occupies[q]:
            occ[idx] = True
            taker[idx] = q
        if last_frame and check_orientation:
            rot_hist[rotation_bin(Q.angles[q], F.angles[idx], tr, flip)].append(idx)
    if last_frame and check_orientation:
        i1, i2, i3 = three_maxima([len(b) for b in rot_hist], tr, flip)
        for i in range(HISTO_LENGTH):
            if i in (i1, i2, i3):
                continue
            for j in rot_hist[i]:
                assign[j] = -1
                nmatches -= 1
    tr["longest_chain"] = int(depth.max()) if Q.n else 0
    return assign, nmatches, tr


def _fuse(F, Q, th_low, flip):
    tr = _new_trace(Q.n)
    grid, tr["half_cells"] = build_grid(F, flip)
    tr["eq"]["pos_round"] = tr["half_cells"]
    th = f32(th_low)
    out = np.full(Q.n, -1, np.int32)
    nfused = 0
    inf = getattr(F, "inf", None)
    u_right = getattr(F, "u_right", None)
    for q in range(Q.n):
        if Q.valid is not None and not Q.valid[q]:
            continue
        area = _area(F, grid, q, Q, tr, flip, False)  # KeyFrame::GetFeaturesInArea has no size band ...
        if area is None or not area:
            continue
        u, v = f32(Q.u[q]), f32(Q.v[q])
        mn, mx = f32(Q.min_size[q]), f32(Q.max_size[q])
        cand = []
        for idx in area:
            sz = f32(F.sizes[idx])  # ... the matching loop applies it (:877, :1032, :1171)
            if sz == mn:
                tr["eq"]["size_lt_min"] += 1
            if sz == mx:
                tr["eq"]["size_gt_max"] += 1
            if (sz <= mn) if flip == "size_lt_min" else (sz < mn):
                tr["drop"]["size_low"] += 1
                continue
            if (sz >= mx) if flip == "size_gt_max" else (sz > mx):
                tr["drop"]["size_high"] += 1
                continue
            if inf is not None:  # Fuse(pKF, vpMapPoints): the chi-square gate; Fuse(Sim3) / SearchBySim3 have none
                ex, ey = u - f32(F.x[idx]), v - f32(F.y[idx])
                ur = f32(u_right[idx]) if u_right is not None else f32(-1.0)
                if u_right is not None and ur == 0:
                    tr["eq"]["uright_ge0"] += 1
                if (ur > 0) if flip == "uright_ge0" else (ur >= 0):
                    er = f32(Q.ur[q]) - ur
                    e2 = ex * ex + ey * ey + er * er
                    if float(e2 * f32(inf[idx])) > 7.8:
                        tr["drop"]["chi2_3dof"] += 1
                        continue
                else:
                    e2 = ex * ex + ey * ey
                    if float(e2 * f32(inf[idx])) > 5.99:
                        tr["drop"]["chi2_2dof"] += 1
                        continue
            cand.append(idx)
        tr["ncand"][q] = len(cand)
        if not cand:
            continue
        d_all = _distances(F, Q, q, cand)
        best = f32(np.finfo(np.float32).max)
        best_pos = -1
        for pos in range(len(cand)):
            d = d_all[pos]
            if d == best:
                tr["eq"]["tie_first"] += 1
            if (d <= best) if flip == "tie_first" else (d < best):
                best, best_pos = d, pos
        if best == th:
            tr["eq"]["best_le_th"] += 1
        if (best < th) if flip == "best_le_th" else (best <= th):
            out[q] = cand[best_pos]
            tr["rank"][q] = _rank(d_all, best_pos)
            tr["accepted"] += 1
            nfused += 1
    return out, nfused, tr


def match_sim3(F2, Q1, F1, Q2, th_high=75.0, flip=None):
    """SearchBySim3: both directed searches are the gate-less matching loop of :1159-1187 / :1237-1265, then the agreement check"""
    class _NoGate:  # a view of F without the chi-square gate and without mvuRight
        def __init__(self, F):
            self.__dict__.update(F.__dict__)
            self.inf = None
            self.u_right = None
    m1, _, t1 = _fuse(_NoGate(F2), Q1, th_high, flip)
    m2, _, t2 = _fuse(_NoGate(F1), Q2, th_high, flip)
    out = np.full(Q1.n, -1, np.int32)
    found = 0
    for i1 in range(Q1.n):
        idx2 = m1[i1]
        if idx2 >= 0 and idx2 < Q2.n and m2[idx2] == i1:
            out[i1] = idx2
            found += 1
    return out, found, {"j12": t1, "j21": t2}


def match_initialization(F2, Q1, th_low=75.0, nnratio=0.9, check_orientation=True, flip=None):
    """SearchForInitialization, active code (:479-556): -> (vnMatches12[Q1.n], nMatches, trace)"""
    assert flip is None or flip in FLIPS, flip
    tr = _new_trace(Q1.n)
    grid, tr["half_cells"] = build_grid(F2, flip)
    tr["eq"]["pos_round"] = tr["half_cells"]
    th, ratio = f32(th_low), f32(nnratio)
    big = f32(np.finfo(np.float32).max)
    mdist = np.full(F2.N, big, np.float32)
    m21 = np.full(F2.N, -1, np.int64)
    m12 = np.full(Q1.n, -1, np.int32)
    depth = np.zeros(Q1.n, np.int64)
    nmatches = 0
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    for q in range(Q1.n):
        if Q1.valid is not None and not Q1.valid[q]:
            continue
        cand = _area(F2, grid, q, Q1, tr, flip, True)
        if cand is None or not cand:
            continue
        tr["ncand"][q] = len(cand)
        d_all = _distances(F2, Q1, q, cand)
        best = best2 = big
        best_pos = -1
        held = False
        for pos, idx in enumerate(cand):
            d = d_all[pos]
            if mdist[idx] == d:
                tr["eq"]["mdist_le"] += 1
            if (mdist[idx] < d) if flip == "mdist_le" else (mdist[idx] <= d):
                tr["drop"]["mdist"] += 1
                held = held or d <= th
                continue
            if d == best:
                tr["eq"]["tie_first"] += 1
            if (d <= best) if flip == "tie_first" else (d < best):
                best2, best, best_pos = best, d, pos
            else:
                if d == best2:
                    tr["eq"]["d_lt_best2"] += 1
                if (d <= best2) if flip == "d_lt_best2" else (d < best2):
                    best2 = d
        top = int(np.lexsort((np.arange(len(cand)), d_all))[0])
        if m21[cand[top]] >= 0:
            depth[q] = depth[m21[cand[top]]] + 1
        if (best_pos < 0 or best > th) and held and len(cand) > 8:
            tr["starved"] += 1  # unmatched only because earlier queries hold every candidate within the threshold at a distance <= its own
        if best_pos < 0:
            continue
        if best == th:
            tr["eq"]["best_le_th"] += 1
        if not ((best < th) if flip == "best_le_th" else (best <= th)):
            continue
        lim = best2 * ratio
        if best == lim:
            tr["eq"]["init_ratio_lt"] += 1
        if not ((best <= lim) if flip == "init_ratio_lt" else (best < lim)):
            continue
        idx = cand[best_pos]
        if m21[idx] >= 0:
            robbed = int(m21[idx])
            m12[robbed] = -1
            nmatches -= 1
            tr["steals"] += 1
            if flip == "steal_hist_stays":
                for b in rot_hist:
                    if robbed in b:
                        b.remove(robbed)
        m12[q] = idx
        m21[idx] = q
        mdist[idx] = best
        nmatches += 1
        tr["rank"][q] = _rank(d_all, best_pos)
        tr["accepted"] += 1
        if check_orientation:
            rot_hist[rotation_bin(Q1.angles[q], F2.angles[idx], tr, flip)].append(q)
    if check_orientation:
        i1, i2, i3 = three_maxima([len(b) for b in rot_hist], tr, flip)
        for i in range(HISTO_LENGTH):
            if i in (i1, i2, i3):
                continue
            for q in rot_hist[i]:
                if m12[q] >= 0:
                    nmatches -= 1
                    m12[q] = -1
    tr["longest_chain"] = int(depth.max()) if Q1.n else 0
    return m12, nmatches, tr


# ---- the LDS budgets of the ordered phase, restated from csrc/k_project.hip (tests compare them with afv_project_wg_lds) ----
WG_LDS_MAX = 150 * 1024 - 32 * 1024 - 2 * 1024   # k_project.hip afv_project_prepare: what the fixed point may use
WALK_FIXED, WALK_REC, WALK_MAX = 8192 * 4 + 8192 // 8 + 32 * 4, 64, 128 * 1024   # PR_LDS_FIXED, PR_REC_BYTES, the stage_cap rule


def proj_wg_lds(n, nq, float_rows=False):
    """k_project.hip proj_wg_lds_bytes"""
    nr, qr = (n + 63) & ~63, (nq + 63) & ~63
    return 3 * nr * 4 + qr * 16 + qr * 4 + qr * 4 + 3 * qr * 2 + qr * 2 + qr + 64 + (qr * 8 if float_rows else 0)


def init_wg_lds(n, nq):
    """k_project.hip init_wg_lds_bytes"""
    nr, qr = (n + 63) & ~63, (nq + 63) & ~63
    return 9 * nr * 4 + qr * 32 + qr * 4 + 4 * qr * 2 + 2 * qr * 2 + qr * 2 + qr + 64


def candidate_visits(F, Q):
    """cheap upper estimate of the features the restatement would look at (the rule for leaving a size-regime scene to the oracle alone):
    features per cell x cells per window, vectorised"""
    cols, rows = int(F.grid_cols), int(F.grid_rows)
    vx = (F.x - F.min_x) * F.grid_inv_w
    vy = (F.y - F.min_y) * F.grid_inv_h
    px = (np.sign(vx) * np.floor(np.abs(vx.astype(np.float64)) + 0.5)).astype(np.int64)
    py = (np.sign(vy) * np.floor(np.abs(vy.astype(np.float64)) + 0.5)).astype(np.int64)
    ok = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
    cnt = np.zeros((cols + 1, rows + 1), np.int64)
    np.add.at(cnt, (px[ok] + 1, py[ok] + 1), 1)
    S = cnt.cumsum(0).cumsum(1)
    x0 = np.clip(np.floor((Q.u - F.min_x - Q.r) * F.grid_inv_w).astype(np.int64), 0, cols)
    x1 = np.clip(np.ceil((Q.u - F.min_x + Q.r) * F.grid_inv_w).astype(np.int64) + 1, 0, cols)
    y0 = np.clip(np.floor((Q.v - F.min_y - Q.r) * F.grid_inv_h).astype(np.int64), 0, rows)
    y1 = np.clip(np.ceil((Q.v - F.min_y + Q.r) * F.grid_inv_h).astype(np.int64) + 1, 0, rows)
    x1 = np.maximum(x1, x0); y1 = np.maximum(y1, y0)
    tot = S[x1, y1] - S[x0, y1] - S[x1, y0] + S[x0, y0]
    if Q.valid is not None:
        tot = tot * (np.asarray(Q.valid) != 0)
    return int(tot.sum())
