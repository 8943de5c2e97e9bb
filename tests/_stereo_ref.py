"""Plain-Python restatement of Frame::ComputeStereoMatches / ComputeStereoFromRGBD, with a trace.  TEST INFRASTRUCTURE ONLY.

This file is the NORMATIVE semantics of afv_frame_stereo_match / afv_frame_set_depth (include/afv_hip.h): the device is held to it bit
for bit (u_right and depth as float bits, the SAD as an int).  It follows tests/_proj_ref.py and tests/_voctrain_ref.py: np.float32
scalars, one operation per statement, no fused multiply-add.  Parity with a real build of the reference is unpinned: the reference's
function prints "has not been modified yet to work with AnyFeature-VSLAM" and its stereo constructor has the extraction commented out
(Frame.cc:76-80), so there is no build to compare with.

Restated from the reference's source (src/Frame.cc:465-669, ORB-SLAM2's routine), with three deviations:

  A  the row table reads the RIGHT keypoint's own size.  The reference reads GetKeyPtSize(iR) of the LEFT frame (:491, its own comment
     "GetKeyPtSizeRight(iR) !!!" marks it): an out-of-bounds read when Nr > N.
  B  rows outside [0, nRows) are dropped, for the table (:496-497 indexes vRowIndices[yi] unchecked) and for the left keypoint's own row
     (:516).
  C  a keypoint is skipped when any pixel either SAD window reads lies outside its level (sv +- 5, su +- 5, su0 +- 10), or when its
     octave is no level of the pyramid.  The reference would assert inside OpenCV (rowRange / colRange, :568, :585); with
     edgeThreshold = 0 keypoints 3 px from the border are legal in this project.  The same holds for a scaled coordinate
     round(u / size), round(v / size), round(uR0 / size) that is not finite or beyond +-2^20 (a zero, denormal or NaN size, a huge
     coordinate: the reference converts it to int, which is undefined): the keypoint is skipped.  A left keypoint whose y is NaN or outside
     (-1, nRows) has no row (B), and the ends of a right keypoint's row band are clamped to +-2^30, a NaN end emptying the band.

Kept as written, although it looks like a fourth defect: bestIdxR starts at 0 (:528).  A left keypoint whose row is not empty but none of
whose candidates passes the octave / u gates keeps bestDist1 = TH_HIGH, and goes on with right keypoint 0 whenever TH_HIGH < thOrbDist
(that is, TH_LOW > TH_HIGH).  With the reference's settings (TH_HIGH == TH_LOW) it cannot happen.

Inputs: `Side` objects (distorted mvKeys x / y / octave, keyPtsSize, descriptor rows uint8 [n, bytes] or float32 [n, dim]), the two
pyramids as lists of uint8 [h, w] levels (the detector's unblurred levels), the scalars mbf, fx, th_high, th_low.
Outputs: u_right[N], depth[N] (float32, -1 where none), sad[N] (the SAD of an accepted pair BEFORE the median filter, -1 where none),
best_r[N] (the right index the descriptor search chose and `best < thOrbDist` let through, -1 where none), trace.

`flip="rule"` turns ONE rule of the restatement around (FLIPS below); tests/test_stereo_ref_cpu.py uses it to prove that a scene's outcome
depends on the rule the scene is named after.
"""
import math

import numpy as np

from _proj_ref import DISTANCE, hamming, l2sqr  # noqa: F401

f32 = np.float32
W = 5  # :567 const int w = 5
L = 5  # :574 const int L = 5

FLIPS = {
    "band_max": "yi <= maxr  ->  yi < maxr (:496)",
    "band_min": "yi >= minr  ->  yi > minr (:496)",
    "row_trunc": "vRowIndices[(int)vL]  ->  the nearest row (:516)",
    "row_clip": "deviation B: rows outside [0, nRows) dropped  ->  clamped into the table",
    "right_size": "deviation A: the right keypoint's own size  ->  GetKeyPtSize(iR) of the left frame where it exists (:491)",
    "oct_lo": "kpR.octave < levelL - 1 rejects  ->  <= rejects (:538)",
    "oct_hi": "kpR.octave > levelL + 1 rejects  ->  >= rejects (:538)",
    "u_min": "uR >= minU  ->  uR > minU (:543)",
    "u_max": "uR <= maxU  ->  uR < maxU (:543)",
    "maxu_neg": "maxU < 0 skips  ->  never skips (:524)",
    "tie_first": "descDist < bestDist1  ->  <= (the last of equals wins; dist == TH_HIGH matches) (:548)",
    "orb_lt": "bestDist1 < thOrbDist  ->  <= (:557)",
    "th_sep": "thOrbDist = (TH_HIGH + TH_LOW) / 2  ->  TH_HIGH (:473)",
    "best0": "bestIdxR starts at 0 (:528)  ->  a keypoint none of whose candidates passed is skipped",
    "inc_lo": "bestincR == -L skips  ->  goes on, dist1 = dist2 (:599)",
    "inc_hi": "bestincR == +L skips  ->  goes on, dist3 = dist2 (:599)",
    "sad_tie_first": "dist < bestDist  ->  <= (the last of equal offsets wins) (:590)",
    "centre_sub": "the windows minus their centre pixels  ->  the raw windows (:570, :587)",
    "gate_iniu": "iniu < 0 skips  ->  does not (:580)",
    "gate_endu": "endu >= cols skips  ->  endu > cols skips (:580)",
    "c_top": "deviation C: sv - 5 < 0 skips  ->  reads clamped rows",
    "c_bottom": "deviation C: sv + 5 >= rows skips  ->  reads clamped rows",
    "c_left": "deviation C: su - 5 < 0 skips  ->  reads clamped columns",
    "c_right": "deviation C: su + 5 >= cols skips  ->  reads clamped columns",
    "c_r0_left": "deviation C: su0 - 10 < 0 skips  ->  reads clamped columns",
    "disp_ge0": "disparity >= minD  ->  > minD (:617)",
    "disp_neg": "disparity >= minD  ->  >= minD - 1 (:617)",
    "disp_lt_max": "disparity < maxD  ->  <= maxD (:617)",
    "median_index": "vDistIdx[size / 2]  ->  [(size - 1) / 2] (:632)",
    "median_ge": "first >= thDist is removed  ->  first > thDist (:637)",
}


class Side:
    """one eye: mvKeys (distorted), keyPtsSize, descriptors"""

    def __init__(self, x, y, octave, size, desc):
        self.x = np.ascontiguousarray(x, np.float32)
        self.y = np.ascontiguousarray(y, np.float32)
        self.octave = np.ascontiguousarray(octave, np.int32)
        self.size = np.ascontiguousarray(size, np.float32)
        d = np.asarray(desc)
        self.desc = np.ascontiguousarray(d, np.float32 if d.dtype.kind == "f" else np.uint8)
        self.n = len(self.x)
        assert len(self.y) == self.n and len(self.octave) == self.n and len(self.size) == self.n and self.desc.shape[0] == self.n


def c_round(v):
    """C round() of a float: halves go away from zero; the result as the float the reference keeps it in"""
    v = float(v)
    if not math.isfinite(v):
        return f32(v)
    return f32(math.floor(abs(v) + 0.5) * (1.0 if v >= 0 else -1.0))


def distance(a, b):
    """FeatureMatcher::DescriptorDistance (FeatureMatcher.cc:1508-1531) as Descriptor_Distance_Type = float"""
    if a.dtype.kind == "f":
        return f32(DISTANCE["l2sqr"](a, b[None, :])[0])
    return f32(hamming(a, b[None, :])[0])


def _px(img, y, x):
    """a pixel as int; clamped, which only a flipped deviation-C rule can make matter"""
    h, w = img.shape
    return int(img[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])


def window_sad(imL, imR, sv, su, cu, centre=True):
    """cv::norm(IL, IR, NORM_L1) of the two 11 x 11 windows around (sv, su) of imL and (sv, cu) of imR, each minus its own centre pixel
    (:568-570, :585-589).  The values are integers of magnitude <= 510, the sum <= 121 * 510 = 61 710: exact in the reference's floats."""
    lc = _px(imL, sv, su) if centre else 0
    rc = _px(imR, sv, cu) if centre else 0
    h, w = imL.shape
    if sv - W >= 0 and sv + W < h and min(su, cu) - W >= 0 and max(su, cu) + W < w:   # both windows inside: the same sum on slices
        a = imL[sv - W:sv + W + 1, su - W:su + W + 1].astype(np.int64) - lc
        b = imR[sv - W:sv + W + 1, cu - W:cu + W + 1].astype(np.int64) - rc
        return int(np.abs(a - b).sum())
    s = 0
    for dy in range(-W, W + 1):
        for dx in range(-W, W + 1):
            a = _px(imL, sv + dy, su + dx) - lc
            b = _px(imR, sv + dy, cu + dx) - rc
            s += abs(a - b)
    return s


def parabola(d1, d2, d3):
    """:607 deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2)) on the float values of the three SADs"""
    d1, d2, d3 = f32(d1), f32(d2), f32(d3)
    num = f32(d1 - d3)
    s13 = f32(d1 + d3)
    two_d2 = f32(f32(2.0) * d2)
    den = f32(s13 - two_d2)
    den2 = f32(f32(2.0) * den)
    with np.errstate(divide="ignore", invalid="ignore"):
        return f32(num / den2)


COORD_MAX = 1 << 20  # a scaled window coordinate beyond it (or not finite) skips the keypoint: no level is that wide
BAND_MAX = 1 << 30   # the ends of a row band are clamped to it before they become ints


def band_end(v):
    """an end of a row band as an int.  The reference converts any float (undefined for NaN and beyond int); here the end is clamped to
    +-2^30 and a NaN end becomes -2^30, which empties the band"""
    v = float(v)
    if v != v:
        return -BAND_MAX
    return int(min(max(v, -float(BAND_MAX)), float(BAND_MAX)))


def row_table(Lside, R, n_rows, flip=None, trace=None):
    """:485-498 with deviations A and B: per row the right keypoints in ascending iR"""
    rows = [[] for _ in range(n_rows)]
    for iR in range(R.n):
        size = R.size[iR]                                   # deviation A
        if flip == "right_size" and iR < Lside.n:
            size = Lside.size[iR]                           # :491 const float r = 2.0f * GetKeyPtSize(iR)
        r = f32(f32(2.0) * size)
        maxr = band_end(np.ceil(f32(R.y[iR] + r)))          # :493 const int maxr = ceil(kpY + r)
        minr = band_end(np.floor(f32(R.y[iR] - r)))         # :494 const int minr = floor(kpY - r)
        lo = minr + 1 if flip == "band_min" else minr
        hi = maxr - 1 if flip == "band_max" else maxr
        for yi in range(max(lo, -1), min(hi, n_rows) + 1):  # :496 for (int yi = minr; yi <= maxr; yi++) (rows beyond -1 / nRows: dropped unseen)
            if yi < 0 or yi >= n_rows:                      # deviation B
                if trace is not None:
                    trace["rows_dropped"] += 1
                if flip != "row_clip":
                    continue
                yi = min(max(yi, 0), n_rows - 1)
                if iR in rows[yi]:
                    continue
            rows[yi].append(iR)
    return rows


def _new_trace():
    keys = ("rows_dropped", "row_outside", "row_empty", "maxu_neg", "oct_lo", "oct_hi", "u_lo", "u_hi", "dist_evals", "dist_ties", "dist_eq_th",
            "best0_used", "orb_reject", "orb_equal", "coord_range", "level_missing", "gate_iniu", "gate_endu", "c_top", "c_bottom", "c_left", "c_right", "c_r0_left",
            "inc_lo", "inc_hi", "sad_ties", "sad_flat", "parabola_gate", "disp_zero", "disp_neg", "disp_ge_max", "accepted", "median_removed",
            "median_on_th")
    t = {k: 0 for k in keys}
    t["median"] = None
    t["th_dist"] = None
    t["sads"] = {}       # iL -> the 11 SADs
    t["delta"] = {}      # iL -> deltaR
    return t


def compute_stereo_matches(Lside, R, pyrL, pyrR, mbf, fx, th_high, th_low, flip=None):
    assert flip is None or flip in FLIPS, flip
    tr = _new_trace()
    N = Lside.n
    u_right = np.full(N, -1.0, np.float32)                  # :470
    depth = np.full(N, -1.0, np.float32)                    # :471
    sad = np.full(N, -1, np.int32)
    best_r = np.full(N, -1, np.int32)
    mbf, fx, th_high, th_low = f32(mbf), f32(fx), f32(th_high), f32(th_low)
    th_sum = f32(th_high + th_low)
    th_orb = f32(th_sum / f32(2.0))                         # :473
    if flip == "th_sep":
        th_orb = th_high
    n_rows = pyrL[0].shape[0]                               # :475
    rows = row_table(Lside, R, n_rows, flip, tr)
    mb = f32(mbf / fx)                                      # Frame.cc:213 mb = mbf / fx
    min_d = f32(0.0)                                        # :502
    max_d = f32(mbf / mb)                                   # :503
    pairs = []                                              # :506 vDistIdx
    for iL in range(N):
        levelL = int(Lside.octave[iL])
        vL, uL = Lside.y[iL], Lside.x[iL]
        if not (vL > f32(-1.0) and vL < f32(n_rows)):       # deviation B; also NaN: only such a y is converted (it truncates into the table)
            tr["row_outside"] += 1
            continue
        row = int(vL)                                       # :516 vRowIndices[vL]: float -> size_t truncates
        if flip == "row_trunc":
            row = int(c_round(vL))
        if row < 0 or row >= n_rows:                        # deviation B
            tr["row_outside"] += 1
            continue
        cand = rows[row]
        if not cand:                                        # :518
            tr["row_empty"] += 1
            continue
        min_u = f32(uL - max_d)                             # :521
        max_u = f32(uL - min_d)                             # :522
        if max_u < 0:                                       # :524
            tr["maxu_neg"] += 1
            if flip != "maxu_neg":
                continue
        best = th_high                                      # :527
        best_idx = 0                                        # :528
        found = False
        for iR in cand:                                     # :533
            o = int(R.octave[iR])
            if (o <= levelL - 1) if flip == "oct_lo" else (o < levelL - 1):   # :538
                tr["oct_lo"] += 1
                continue
            if (o >= levelL + 1) if flip == "oct_hi" else (o > levelL + 1):
                tr["oct_hi"] += 1
                continue
            uR = R.x[iR]
            if not ((uR > min_u) if flip == "u_min" else (uR >= min_u)):      # :543
                tr["u_lo"] += 1
                continue
            if not ((uR < max_u) if flip == "u_max" else (uR <= max_u)):
                tr["u_hi"] += 1
                continue
            d = distance(Lside.desc[iL], R.desc[iR])        # :546
            tr["dist_evals"] += 1
            if d == best:
                tr["dist_eq_th" if not found else "dist_ties"] += 1
            if (d <= best) if flip == "tie_first" else (d < best):           # :548
                best = d
                best_idx = iR
                found = True
        if not ((best <= th_orb) if flip == "orb_lt" else (best < th_orb)):   # :557
            tr["orb_reject"] += 1
            if best == th_orb:
                tr["orb_equal"] += 1
            continue
        if not found:
            tr["best0_used"] += 1
            if flip == "best0":
                continue
        best_r[iL] = best_idx
        uR0 = R.x[best_idx]                                 # :560
        with np.errstate(all="ignore"):
            s = f32(f32(1.0) / Lside.size[iL])              # :561
        with np.errstate(all="ignore"):
            fu = c_round(f32(uL * s))                       # :562
            fv = c_round(f32(vL * s))                       # :563
            fu0 = c_round(f32(uR0 * s))                     # :564
        # a zero / denormal / NaN size or a huge coordinate: such a scaled coordinate lies on no level.  The reference converts it to int
        # (undefined); here it skips the keypoint, as deviation C would
        if not all(-COORD_MAX <= float(c) <= COORD_MAX for c in (fu, fv, fu0)):
            tr["coord_range"] += 1
            continue
        su, sv, su0 = int(fu), int(fv), int(fu0)
        if levelL < 0 or levelL >= len(pyrL):               # deviation C: the octave is no level of the pyramid
            tr["level_missing"] += 1
            continue
        imL, imR = pyrL[levelL], pyrR[levelL]
        h, w = imL.shape
        iniu = su0 + L - W                                  # :578
        endu = su0 + L + W + 1                              # :579
        skip = False
        if iniu < 0:                                        # :580
            tr["gate_iniu"] += 1
            skip = skip or flip != "gate_iniu"
        if (endu > w) if flip == "gate_endu" else (endu >= w):
            tr["gate_endu"] += 1
            skip = True
        for rule, out in (("c_top", sv - W < 0), ("c_bottom", sv + W >= h), ("c_left", su - W < 0), ("c_right", su + W >= w),
                          ("c_r0_left", su0 - L - W < 0)):  # deviation C (su0 + L + W >= cols is inside the endu gate)
            if out:
                tr[rule] += 1
                skip = skip or flip != rule
        if skip:
            continue
        dists = []
        best_sad, best_inc = None, 0                        # :572-573 (INT_MAX)
        for inc in range(-L, L + 1):                        # :583
            d = window_sad(imL, imR, sv, su, su0 + inc, centre=flip != "centre_sub")
            if best_sad is not None and d == best_sad:
                tr["sad_ties"] += 1
            if best_sad is None or ((d <= best_sad) if flip == "sad_tie_first" else (d < best_sad)):   # :590
                best_sad, best_inc = d, inc
            dists.append(d)
        tr["sads"][iL] = dists
        if len(set(dists)) == 1:
            tr["sad_flat"] += 1
        k = L + best_inc
        d2 = dists[k]
        if best_inc == -L:                                  # :599
            tr["inc_lo"] += 1
            if flip != "inc_lo":
                continue
            d1, d3 = d2, dists[k + 1]
        elif best_inc == L:
            tr["inc_hi"] += 1
            if flip != "inc_hi":
                continue
            d1, d3 = dists[k - 1], d2
        else:
            d1, d3 = dists[k - 1], dists[k + 1]             # :603-605
        delta = parabola(d1, d2, d3)                        # :607
        tr["delta"][iL] = delta
        if delta < -1 or delta > 1:                         # :609 (a first minimum cannot trigger it; kept)
            tr["parabola_gate"] += 1
            continue
        t0 = f32(f32(su0) + f32(best_inc))
        t1 = f32(t0 + delta)
        best_u = f32(Lside.size[iL] * t1)                   # :613
        disparity = f32(uL - best_u)                        # :615
        if flip == "disp_ge0":
            lo_ok = disparity > min_d
        elif flip == "disp_neg":
            lo_ok = disparity >= f32(min_d - f32(1.0))
        else:
            lo_ok = disparity >= min_d                      # :617
        hi_ok = (disparity <= max_d) if flip == "disp_lt_max" else (disparity < max_d)
        if not lo_ok:
            tr["disp_neg"] += 1
        if disparity == min_d:
            tr["disp_zero"] += 1
        if not hi_ok:
            tr["disp_ge_max"] += 1
        if not (lo_ok and hi_ok):
            continue
        if disparity <= 0:                                  # :619
            disparity = f32(0.01)                           # :621 disparity = 0.01 (a double literal narrowed)
            best_u = f32(float(uL) - 0.01)                  # :622 bestuR = uL - 0.01 (in double, narrowed)
        depth[iL] = f32(mbf / disparity)                    # :624
        u_right[iL] = best_u                                # :625
        sad[iL] = best_sad
        pairs.append((best_sad, iL))                        # :626
        tr["accepted"] += 1
    if pairs:                                               # (the reference indexes an empty vector at :632)
        pairs.sort()                                        # :631
        mid = (len(pairs) - 1) // 2 if flip == "median_index" else len(pairs) // 2
        median = f32(pairs[mid][0])                         # :632
        k21 = f32(f32(1.5) * f32(1.4))
        th_dist = f32(k21 * median)                         # :633 1.5f * 1.4f * median
        tr["median"], tr["th_dist"] = float(median), float(th_dist)
        for s_, iL in pairs:                                # :635-644: the walk from the top stops at the first pair below thDist
            if f32(s_) == th_dist:
                tr["median_on_th"] += 1
            if (f32(s_) > th_dist) if flip == "median_ge" else (f32(s_) >= th_dist):
                u_right[iL] = f32(-1.0)
                depth[iL] = f32(-1.0)
                tr["median_removed"] += 1
    return u_right, depth, sad, best_r, tr


def compute_stereo_from_rgbd(x, y, x_un, depth_image, mbf):
    """Frame::ComputeStereoFromRGBD (:648-669): x / y the distorted mvKeys, x_un = mvKeysUn.x"""
    n = len(x)
    u_right = np.full(n, -1.0, np.float32)                  # :650
    depth = np.full(n, -1.0, np.float32)                    # :651
    mbf = f32(mbf)
    img = np.asarray(depth_image, np.float32)
    for i in range(n):
        v, u = f32(y[i]), f32(x[i])                         # :658-659
        r, c = int(v), int(u)                               # :661 imDepth.at<float>(v, u): float -> int truncates
        if r < 0 or r >= img.shape[0] or c < 0 or c >= img.shape[1]:
            continue                                        # (outside the depth image: the reference reads out of bounds; here no depth)
        d = img[r, c]
        if d > 0:                                           # :663
            depth[i] = d                                    # :665
            q = f32(mbf / d)
            u_right[i] = f32(f32(x_un[i]) - q)              # :666
    return u_right, depth
