"""Plain-Python restatement of the reference's BoW-guided matchers, with a trace.  TEST INFRASTRUCTURE ONLY.

A second opinion next to oracle/afvo.c (written by the same hand as the kernels), as _proj_ref.py is for the projection searches.  Restated
from the reference's source, not from the oracle:

  SearchByBoW(KF, F)          FeatureMatcher.cc:186-283   search_by_bow_kf_frame
  SearchByBoW(KF, KF)         :561-660                    search_by_bow_kf_kf
  SearchForTriangulation      :662-790                    search_for_triangulation
  CheckDistEpipolarLine       :165-182
  rotation histogram          :1579-1668                  (rotation_bin / three_maxima of _proj_ref.py)

Signatures and outputs are those of oracle/binding.py, plus a trace dict.  A FeatureVector is a list of (node id, [feature indices])
ascending by node id; None on either side means "no vocabulary": one node that holds every feature of both sides in index order (the
project's brute-force convention, not the reference's).  Everything the reference computes in `float` is done on np.float32 scalars: the
ratio product (:252 / :632), 3.84f * sigma2 (:181), 100.0f * sqrtf(sigma2) (:746) and a, b, c, num, den, dsqr of the epipolar line.

`flip="rule"` turns ONE rule of the restatement around (FLIPS below).  tests/test_match_ref_cpu.py uses it to prove that a scene's outcome
depends on the rule the scene is named after.  The issue's `rule01` is the pair max2_lt / max3_lt, under the names _proj_ref.FLIPS gives them.
"""
import numpy as np

from _proj_ref import DISTANCE, HISTO_LENGTH, hamming, l2sqr, rotation_bin, three_maxima  # noqa: F401  (l2sqr: used by the scene files)

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max   # highestPossibleDistance (FeatureMatcher.h:116)

# rule -> what the flipped restatement does instead
FLIPS = {
    "th_lt_kfkf": "bestDist1 < TH_LOW  ->  <= (:630)",
    "th_le_kff": "bestDist1 <= TH_LOW  ->  < (:250)",
    "ratio_lt": "(float)bestDist1 < mfNNratio * (float)bestDist2  ->  <= (:252, :632)",
    "ratio_f32": "the ratio product in float  ->  in double (0.6f * 50 = 30.000002 accepts 30; 0.6 * 50 = 30.0 does not)",
    "best_first": "descDist < bestDist1: the first listed of equal columns wins  ->  <= : the last wins (:238, :618)",
    "second_lt": "else if (descDist < bestDist2) bestDist2 = descDist  ->  the else branch never moves bestDist2 (:244, :624)",
    "taken": "a taken column is skipped (:609 vbMatched2, :232 vpMapPointMatches)  ->  it stays visible",
    "valid1": "a row without a good map point is skipped (:216-222, :593-597)  ->  it is matched",
    "valid2": "a KF2 column without a good map point is skipped (:607-613)  ->  it is a candidate",
    "node_order": "a node is walked in the listed order of its indices  ->  in ascending feature index",
    "merge_lower_bound": "the side with the smaller node id jumps to lower_bound of the other's (:268-275, :646-653)  ->  both sides step",
    "rot_lt0": "rot < 0 adds 360  ->  rot <= 0 adds 360 (:1592)",
    "rot_round": "round(rot * rotFactor) half away from zero  ->  half towards zero (:1594)",
    "rot_wrap": "bin == 30 -> 0  ->  29 (:1595)",
    "max_first": "s > max: the first of equal bins wins  ->  >= : the last wins (:1636-1652)",
    "max2_lt": "max2 < 0.1f * max1 drops  ->  <= drops (:1659)",
    "max3_lt": "max3 < 0.1f * max1 drops  ->  <= drops (:1664)",
    "hist_key": "the histogram entry is the FRAME feature in (KF, F) (:259) and idx1 in (KF, KF) (:638)  ->  the other side's index",
    "tri_th": "descDist > TH_LOW skips  ->  >= skips (:736)",
    "tri_last_wins": "descDist > bestDist skips: an equal distance later in the node replaces  ->  it does not (:736)",
    "tri_geom_before_best": "bestDist moves only when the geometry passes (:751-755)  ->  as soon as the distance test passes",
    "tri_has_mp1": "a KF1 feature that has a map point is skipped (:702)  ->  one that has none is",
    "tri_has_mp2": "a KF2 feature that has a map point is skipped (:724)  ->  one that has none is",
    "tri_stereo_ge0": "mvuRight >= 0 is stereo  ->  > 0 (:705, :727)",
    "tri_only_stereo": "bOnlyStereo skips monocular features (:707-709, :729-731)  ->  it does not",
    "tri_epipole_lt": "distance^2 to the epipole < 100.0f * sqrtf(sigma2) skips  ->  <= skips (:746)",
    "tri_epipole_mono": "the epipole test applies when BOTH sides are monocular (:741)  ->  always",
    "tri_epiline_lt": "dsqr < 3.84f * sigma2 passes  ->  <= passes (:181)",
    "tri_den0": "den == 0 fails (:176)  ->  passes",
    "tri_not_taken": "vbMatched2 is never set: two rows may take one column (:681, :724, :758-763)  ->  a matched column is taken",
}


def _new_trace(n1):
    return {"eq": {k: 0 for k in FLIPS}, "shared_nodes": 0, "jumps": 0, "empty_nodes": 0, "max_node": (0, 0),
            # per KF1 feature: taken columns ahead of the answer in (distance, position) order; length of the dependency chain that ends in it
            "behind": np.full(n1, -1, np.int64), "chain": np.zeros(n1, np.int64), "longest_chain": 0, "starved": 0,
            "hist": [0] * HISTO_LENGTH, "maxima": (-1, -1, -1), "rule01": 0, "wraps": 0, "accepted": 0, "rows_walked": 0,
            "rows_outside_shared_nodes": 0, "geometry_failed": 0}


def _dist(D1, i, D2, idxs):
    rows = D2[np.asarray(idxs, np.int64)] if len(idxs) else D2[:0]
    return DISTANCE["l2sqr"](D1[i], rows) if D1.dtype.kind == "f" else hamming(D1[i], rows)


def _rows(desc):
    d = np.asarray(desc)
    return np.ascontiguousarray(d, np.float32 if d.dtype.kind == "f" else np.uint8)


def shared_nodes(nodes1, nodes2, n1, n2, tr, flip=None):
    """the merge of the two FeatureVectors: [(indices1, indices2)] of the node ids both sides hold, in id order"""
    if nodes1 is None or nodes2 is None:
        tr["shared_nodes"] = 1
        tr["max_node"] = (n1, n2)
        return [(list(range(n1)), list(range(n2)))]
    out = []
    a = b = 0
    ids1 = [n for n, _ in nodes1]; ids2 = [n for n, _ in nodes2]
    assert ids1 == sorted(set(ids1)) and ids2 == sorted(set(ids2)), "a std::map holds every node id once, ascending"

    def lower_bound(ids, key):
        k = 0
        while k < len(ids) and ids[k] < key:
            k += 1
        return k

    while a < len(nodes1) and b < len(nodes2):
        if ids1[a] == ids2[b]:
            l1, l2 = list(nodes1[a][1]), list(nodes2[b][1])
            if sorted(l1) != l1 or sorted(l2) != l2:
                tr["eq"]["node_order"] += 1
            if flip == "node_order":
                l1, l2 = sorted(l1), sorted(l2)
            tr["empty_nodes"] += (not l1) + (not l2)
            tr["max_node"] = max(tr["max_node"], (len(l1), len(l2)), key=lambda t: max(t))
            out.append((l1, l2))
            a += 1; b += 1
            continue
        tr["jumps"] += 1
        tr["eq"]["merge_lower_bound"] += 1
        if flip == "merge_lower_bound":
            a += 1; b += 1
        elif ids1[a] < ids2[b]:
            a = lower_bound(ids1, ids2[b])
        else:
            b = lower_bound(ids2, ids1[a])
    tr["shared_nodes"] = len(out)
    return out


def _best_two(d, visible, tr, flip):
    """:228-248 / :603-628 over the node's columns: (position of the best | -1, bestDist1, bestDist2)"""
    best1 = best2 = FLT_MAX
    pos = -1
    for p in range(len(d)):
        if not visible[p]:
            continue
        v = f32(d[p])
        if v == best1 and pos >= 0:
            tr["eq"]["best_first"] += 1
        if (v <= best1) if flip == "best_first" else (v < best1):
            best2, best1, pos = best1, v, p
        elif v < best2:
            tr["eq"]["second_lt"] += 1
            if flip != "second_lt":
                best2 = v
    return pos, best1, best2


def _ratio_ok(best1, best2, nnratio, tr, flip):
    prod = f32(nnratio) * f32(best2)          # mfNNratio is a float member; static_cast<float>(bestDist2)
    with np.errstate(over="ignore"):
        dbl = float(nnratio) * float(best2)   # what a reading in decimal / double arithmetic gives
    if f32(best1) == prod:
        tr["eq"]["ratio_lt"] += 1
    if (float(best1) < dbl) != bool(f32(best1) < prod):
        tr["eq"]["ratio_f32"] += 1
    if flip == "ratio_f32":
        return float(best1) < dbl
    return bool(f32(best1) <= prod) if flip == "ratio_lt" else bool(f32(best1) < prod)


def _search_by_bow(D1, D2, nodes1, nodes2, valid1, valid2, angle1, angle2, th_low, nnratio, check_orientation, frame, flip):
    D1, D2 = _rows(D1), _rows(D2)
    n1, n2 = len(D1), len(D2)
    tr = _new_trace(n1)
    out = np.full(n2 if frame else n1, -1, np.int32)
    taken2 = np.zeros(n2, bool)      # vbMatched2 (:574) / vpMapPointMatches[idx] != NULL (:232)
    taker = np.full(n2, -1, np.int64)
    hist = [[] for _ in range(HISTO_LENGTH)]
    th = f32(th_low)
    nm = 0
    for l1, l2 in shared_nodes(nodes1, nodes2, n1, n2, tr, flip):
        for idx1 in l1:
            tr["rows_walked"] += 1
            if valid1 is not None and not valid1[idx1]:
                tr["eq"]["valid1"] += 1
                if flip != "valid1":
                    continue
            d = _dist(D1, idx1, D2, l2)
            visible = np.ones(len(l2), bool)
            usable = np.ones(len(l2), bool)   # what the row could ever see: everything but the masked columns
            for p, idx2 in enumerate(l2):
                if not frame and valid2 is not None and not valid2[idx2]:
                    tr["eq"]["valid2"] += 1
                    if flip != "valid2":
                        visible[p] = usable[p] = False
                        continue
                if taken2[idx2]:
                    tr["eq"]["taken"] += 1
                    if flip != "taken":
                        visible[p] = False
            pos, best1, best2 = _best_two(d, visible, tr, flip)
            # the row's first choice had nothing been taken: when another row holds it, this row's answer depends on that row's
            free_pos = _best_two(d, usable, {"eq": {"best_first": 0, "second_lt": 0}}, None)[0]
            if free_pos >= 0 and taken2[l2[free_pos]] and flip is None:
                tr["chain"][idx1] = tr["chain"][taker[l2[free_pos]]] + 1
                tr["longest_chain"] = max(tr["longest_chain"], int(tr["chain"][idx1]))
            if pos < 0:
                tr["starved"] += int(usable.any())
                continue
            if best1 == th:
                tr["eq"]["th_le_kff" if frame else "th_lt_kfkf"] += 1
            if frame:
                under = (best1 < th) if flip == "th_le_kff" else (best1 <= th)
            else:
                under = (best1 <= th) if flip == "th_lt_kfkf" else (best1 < th)
            if not under:
                continue
            if not _ratio_ok(best1, best2, nnratio, tr, flip):
                continue
            idx2 = l2[pos]
            tr["behind"][idx1] = int(sum(1 for p in range(len(l2)) if usable[p] and not visible[p] and (d[p], p) < (d[pos], pos)))
            if frame:
                out[idx2] = idx1
            else:
                out[idx1] = idx2
            taken2[idx2] = True
            taker[idx2] = idx1
            nm += 1
            tr["accepted"] += 1
            if check_orientation:
                b = rotation_bin(angle1[idx1], angle2[idx2], tr, flip)   # keyPt = the keyframe's (KF1's), refKeyPt = the other side's
                tr["eq"]["hist_key"] += 1
                key = idx2 if frame else idx1
                if flip == "hist_key":
                    key = idx1 if frame else idx2
                hist[b].append(key)
    if check_orientation:
        i1, i2, i3 = three_maxima([len(h) for h in hist], tr, flip)
        for b in range(HISTO_LENGTH):
            if b in (i1, i2, i3):
                continue
            for key in hist[b]:     # filterMatchesWithOrientation over vector<Pt>: the entry is cleared, the count drops (:1605-1612)
                if key < len(out):
                    out[key] = -1
                nm -= 1
    return out, nm, tr


def search_by_bow_kf_kf(desc1, desc2, nodes1=None, nodes2=None, valid1=None, valid2=None, angle1=None, angle2=None,
                        th_low=75.0, nnratio=0.6, check_orientation=False, flip=None):
    return _search_by_bow(desc1, desc2, nodes1, nodes2, valid1, valid2, angle1, angle2, th_low, nnratio, check_orientation, False, flip)


def search_by_bow_kf_frame(desc_kf, desc_f, nodes_kf=None, nodes_f=None, valid_kf=None, angle_kf=None, angle_f=None,
                           th_low=75.0, nnratio=0.7, check_orientation=False, flip=None):
    """(the frame side has no mask: a frame feature is free until this very search fills it, :190)"""
    return _search_by_bow(desc_kf, desc_f, nodes_kf, nodes_f, valid_kf, None, angle_kf, angle_f, th_low, nnratio, check_orientation, True, flip)


def check_dist_epipolar_line(x1, y1, x2, y2, F, sigma2, tr, flip=None):
    """:165-182; F is F12 row-major"""
    x1, y1, x2, y2 = f32(x1), f32(y1), f32(x2), f32(y2)
    F = [f32(v) for v in F]
    with np.errstate(all="ignore"):
        a = x1 * F[0] + y1 * F[3] + F[6]
        b = x1 * F[1] + y1 * F[4] + F[7]
        c = x1 * F[2] + y1 * F[5] + F[8]
        num = a * x2 + b * y2 + c
        den = a * a + b * b
        if den == 0:
            tr["eq"]["tri_den0"] += 1
            return flip == "tri_den0"
        dsqr = num * num / den
        lim = f32(3.84) * f32(sigma2)
    if dsqr == lim:
        tr["eq"]["tri_epiline_lt"] += 1
    return bool(dsqr <= lim) if flip == "tri_epiline_lt" else bool(dsqr < lim)


def search_for_triangulation(desc1, desc2, pts1, pts2, sigma2_2, F12, epipole, nodes1=None, nodes2=None, has_mp1=None, has_mp2=None,
                             th_low=75.0, u_right1=None, u_right2=None, only_stereo=False, flip=None):
    D1, D2 = _rows(desc1), _rows(desc2)
    n1, n2 = len(D1), len(D2)
    tr = _new_trace(n1)
    pts1 = np.asarray(pts1, np.float32).reshape(-1, 2); pts2 = np.asarray(pts2, np.float32).reshape(-1, 2)
    F = np.asarray(F12, np.float32).reshape(9)
    ex, ey = f32(epipole[0]), f32(epipole[1])
    th = f32(th_low)
    out = np.full(n1, -1, np.int32)
    matched2 = np.zeros(n2, bool)
    chosen2 = np.zeros(n2, bool)
    nm = 0

    def stereo(u, i):
        if u is None:
            return False     # a monocular keyframe: mvuRight is -1 everywhere
        v = f32(u[i])
        if v == 0:
            tr["eq"]["tri_stereo_ge0"] += 1
        return bool(v > 0) if flip == "tri_stereo_ge0" else bool(v >= 0)

    def skipped_by_mask(mask, i, rule):
        if mask is None:
            return False
        tr["eq"][rule] += int(bool(mask[i]))
        return (not mask[i]) if flip == rule else bool(mask[i])

    seen1 = np.zeros(n1, bool)
    for l1, l2 in shared_nodes(nodes1, nodes2, n1, n2, tr, flip):
        for idx1 in l1:
            seen1[idx1] = True
            tr["rows_walked"] += 1
            if skipped_by_mask(has_mp1, idx1, "tri_has_mp1"):
                continue
            st1 = stereo(u_right1, idx1)
            if only_stereo and not st1:
                tr["eq"]["tri_only_stereo"] += 1
                if flip != "tri_only_stereo":
                    continue
            d = _dist(D1, idx1, D2, l2)
            best = th
            best_idx2 = -1
            for p, idx2 in enumerate(l2):
                if matched2[idx2] or skipped_by_mask(has_mp2, idx2, "tri_has_mp2"):
                    continue
                st2 = stereo(u_right2, idx2)
                if only_stereo and not st2:
                    tr["eq"]["tri_only_stereo"] += 1
                    if flip != "tri_only_stereo":
                        continue
                v = f32(d[p])
                if v == th:
                    tr["eq"]["tri_th"] += 1
                if (v >= th) if flip == "tri_th" else (v > th):
                    continue
                if v == best and best_idx2 >= 0:
                    tr["eq"]["tri_last_wins"] += 1
                    if flip == "tri_last_wins":
                        continue
                if v > best:
                    continue
                if flip == "tri_geom_before_best":
                    best = v
                s2 = f32(sigma2_2[idx2])
                ok = True
                dex, dey = ex - f32(pts2[idx2, 0]), ey - f32(pts2[idx2, 1])
                near = dex * dex + dey * dey
                lim = f32(100.0) * np.sqrt(s2, dtype=np.float32)
                if not st1 and not st2:
                    if near == lim:
                        tr["eq"]["tri_epipole_lt"] += 1
                    if (near <= lim) if flip == "tri_epipole_lt" else (near < lim):
                        ok = False
                elif near < lim:
                    tr["eq"]["tri_epipole_mono"] += 1
                    if flip == "tri_epipole_mono":
                        ok = False
                if ok:
                    ok = check_dist_epipolar_line(pts1[idx1, 0], pts1[idx1, 1], pts2[idx2, 0], pts2[idx2, 1], F, s2, tr, flip)
                if not ok:
                    tr["geometry_failed"] += 1
                    tr["eq"]["tri_geom_before_best"] += 1
                    continue
                best_idx2, best = idx2, v
            if best_idx2 >= 0:
                if chosen2[best_idx2]:
                    tr["eq"]["tri_not_taken"] += 1
                chosen2[best_idx2] = True
                if flip == "tri_not_taken":
                    matched2[best_idx2] = True
                out[idx1] = best_idx2
                nm += 1
                tr["accepted"] += 1
    tr["rows_outside_shared_nodes"] = int((~seen1).sum())
    return out, nm, tr
