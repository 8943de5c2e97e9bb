"""plain restatement of the front of the ORB32 pipeline (test data): cv::ORB's level sizes, resize(..., INTER_LINEAR_EXACT) for 8-bit images, the FAST-9/16
corner score and the 3 x 3 non-maximum suppression of FastFeatureDetector(t, true) - each written from its definition, with numpy and plain loops.

Nothing is imported from oracle/ or from the library.  There is no pre-test, no early exit and no packed arithmetic here: the score of a pixel is the
maximum over all 16 windows and both polarities of the minimum over the 9 ring pixels of the window, evaluated in full for every pixel.  The whole-image
functions evaluate that same expression for all pixels at once on shifted integer planes (one numpy operation per ring pixel and window); the scalar
functions evaluate it for one pixel in Python integers and say which window, polarity and ring pixel decided, which is what the scene proofs of
tests/test_detect_ref_cpu.py need.  The test module holds the whole-image forms to the scalar ones."""
import fractions

import numpy as np

f32 = np.float32
# OpenCV fast_score.cpp makeOffsets(pixel, rowStride, 16): (dx, dy), clockwise from (0, 3)
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
NEIGHBOURS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]


# ---------------------------------------------------------------- level sizes ----------------------------------------------------------------
def level_geometry(w, h, nlevels=8, scale_factor=1.2):
    """cv::ORB (orb.cpp, detectAndCompute): scale_l = (float)pow((double)scaleFactor, l) with scaleFactor the float the extractor was created with,
    size_l = cvRound(size * (1.f / scale_l)) - float32 reciprocal, float32 product, round half to even.  Returns (lw, lh, lscale)."""
    sf = float(f32(scale_factor))
    lw, lh, ls = [], [], []
    for l in range(nlevels):
        scale = f32(sf ** l)           # double pow, rounded to float
        inv = f32(1) / scale           # float32 division
        ls.append(scale)
        lw.append(int(np.rint(f32(w) * inv)))   # float32 product; rint = half to even = cvRound
        lh.append(int(np.rint(f32(h) * inv)))
    return lw, lh, ls


# ---------------------------------------------------------------- resize ----------------------------------------------------------------
def _cv_round(v):
    """cvRound of a double: to nearest, halves to even"""
    fl = int(np.floor(v))
    d = v - fl
    if d > 0.5 or (d == 0.5 and fl & 1):
        return fl + 1
    return fl


def resize_coeffs(src, dst, scale_as="1/(dst/src)"):
    """interpolation_linear<uchar>::getCoeffs of resize.cpp per destination index: (offset of the left tap, weight of the right tap in 1 / 256).
    IEEE double in OpenCV's order: inv = dst / src; scale = 1 / inv; f = scale * (d + 0.5) - 0.5; i = floor(f); weight = cvRound((f - i) * 256).
    i < 0 (or a one-pixel source) gives (0, 0): the first pixel alone; i >= src - 1 gives (src - 1, 0): the last pixel alone.
    scale_as = 'src/dst' evaluates the scale as the single division src / dst instead (the alternative OpenCV does NOT use)."""
    if scale_as == "1/(dst/src)":
        inv = float(dst) / float(src)
        scale = 1.0 / inv
    else:
        assert scale_as == "src/dst"
        scale = float(src) / float(dst)
    ofs, c1 = [], []
    for d in range(dst):
        f = scale * (float(d) + 0.5) - 0.5
        i = int(np.floor(f))
        if i < 0 or src <= 1:
            ofs.append(0)
            c1.append(0)
        elif i >= src - 1:
            ofs.append(src - 1)
            c1.append(0)
        else:
            ofs.append(i)
            c1.append(_cv_round((f - float(i)) * 256.0))
    return ofs, c1


def resize_coeffs_exact(src, dst):
    """the same table with exact rationals: f = src / dst * (d + 1/2) - 1/2 without any rounding, weight = round half to even of (f - i) * 256"""
    F = fractions.Fraction
    ofs, c1 = [], []
    for d in range(dst):
        f = F(src, dst) * (d + F(1, 2)) - F(1, 2)
        i = f.numerator // f.denominator
        if i < 0 or src <= 1:
            ofs.append(0)
            c1.append(0)
        elif i >= src - 1:
            ofs.append(src - 1)
            c1.append(0)
        else:
            ofs.append(i)
            c1.append(round((f - i) * 256))    # Fraction.__round__: half to even
    return ofs, c1


def coeff_differences(src, dst):
    """destination indices at which the table of 'src/dst' and the exact table differ from the table OpenCV computes: (src/dst indices, exact indices)"""
    a = list(zip(*resize_coeffs(src, dst)))
    b = list(zip(*resize_coeffs(src, dst, "src/dst")))
    c = list(zip(*resize_coeffs_exact(src, dst)))
    return [d for d in range(dst) if a[d] != b[d]], [d for d in range(dst) if a[d] != c[d]]


def coeff_tables_np(src, dst):
    """the three tables of coeff_differences for all indices at once (numpy float64 = IEEE double, one rounding per operation, np.rint = half to even;
    the exact table in int64: f = (src (2d + 1) - dst) / (2 dst)).  Returns [(ofs, c1)] * 3: OpenCV's, 'src/dst', exact.  Used by the search over every
    (src, dst) pair; tests/test_detect_ref_cpu.py holds it to the plain loops above."""
    d = np.arange(dst, dtype=np.float64)
    out = []
    for scale in (np.float64(1.0) / (np.float64(dst) / np.float64(src)), np.float64(src) / np.float64(dst)):
        f = scale * (d + 0.5) - 0.5
        i = np.floor(f)
        c = np.rint((f - i) * 256.0).astype(np.int64)
        i = i.astype(np.int64)
        lo, hi = (i < 0) | (src <= 1), (i >= src - 1)
        out.append((np.where(lo, 0, np.where(hi, src - 1, i)), np.where(lo | hi, 0, c)))
    di = np.arange(dst, dtype=np.int64)
    num, den = src * (2 * di + 1) - dst, 2 * dst
    i = num // den                              # floor division
    r = (num - i * den) * 256                   # (f - i) * 256 = r / den
    q, rem = r // den, r % den
    c = q + ((2 * rem > den) | ((2 * rem == den) & (q & 1 == 1)))
    lo, hi = (i < 0) | (src <= 1), (i >= src - 1)
    out.append((np.where(lo, 0, np.where(hi, src - 1, i)), np.where(lo | hi, 0, c)))
    return out


def resize_pixel(src, xo, xc, yo, yc, x, y):
    """one destination pixel from its four source bytes in Python integers: (byte, low 16 bits of the vertical sum before rounding).
    Horizontal pass in 8.8 fixed point (<= 65280), vertical pass (+ 2^15) >> 16; a right / lower tap past the last column / row is the last one."""
    sh, sw = src.shape
    o, o1 = xo[x], min(xo[x] + 1, sw - 1)
    r, r1 = yo[y], min(yo[y] + 1, sh - 1)
    cx, cy = int(xc[x]), int(yc[y])
    h0 = (256 - cx) * int(src[r, o]) + cx * int(src[r, o1])
    h1 = (256 - cx) * int(src[r1, o]) + cx * int(src[r1, o1])
    v = h0 * (256 - cy) + h1 * cy
    return (v + (1 << 15)) >> 16, v & 0xffff


def resize_linear_exact(src, dw, dh, scale_as="1/(dst/src)", half=1 << 15):
    """resize(src, dst, Size(dw, dh), 0, 0, INTER_LINEAR_EXACT) for CV_8UC1: (dst, low 16 bits of every vertical sum, maximum of the horizontal sums).
    The expression of resize_pixel for all pixels at once, in int64.  `half` and `scale_as` exist for the scene proofs: the wrong alternatives (+ 32767,
    the scale as src / dst) must change the result on the scenes built for them.  (The clamp of the right / lower tap to the last column / row has no
    alternative that results could show: a tap is clamped only where its weight is 0, see resize_coeffs.)"""
    src = np.asarray(src, np.uint8)
    sh, sw = src.shape
    xo, xc = (np.array(t, np.int64) for t in resize_coeffs(sw, dw, scale_as))
    yo, yc = (np.array(t, np.int64) for t in resize_coeffs(sh, dh, scale_as))
    xo1, yo1 = np.minimum(xo + 1, sw - 1), np.minimum(yo + 1, sh - 1)
    s = src.astype(np.int64)
    hrow = (256 - xc)[None, :] * s[:, xo] + xc[None, :] * s[:, xo1]     # every source row filtered horizontally
    v = hrow[yo, :] * (256 - yc)[:, None] + hrow[yo1, :] * yc[:, None]
    return ((v + half) >> 16).astype(np.uint8), (v & 0xffff).astype(np.int64), int(hrow.max())


def pyramid(img, nlevels=8, scale_factor=1.2, **rules):
    """level l resized from level l - 1 (cv::ORB).  Returns (levels, low-16 planes of levels >= 1 [None for level 0], largest horizontal sum)"""
    lw, lh, _ = level_geometry(img.shape[1], img.shape[0], nlevels, scale_factor)
    levels, lows, hmax = [np.asarray(img, np.uint8)], [None], 0
    for l in range(1, nlevels):
        d, low, hm = resize_linear_exact(levels[-1], lw[l], lh[l], **rules)
        levels.append(d)
        lows.append(low)
        hmax = max(hmax, hm)
    return levels, lows, hmax


# ---------------------------------------------------------------- FAST-9/16 ----------------------------------------------------------------
def ring_values(img, x, y, ring=RING):
    return [int(img[y + dy, x + dx]) for dx, dy in ring]


def fast_score_info(img, x, y, ring=RING):
    """The FAST-9/16 score of pixel (x, y) from its definition, and what decided it.

    With v the centre and r_k the 16 ring pixels, a window is 9 contiguous ring indices w .. w + 8 (mod 16).  Its bright strength is min_k (r_k - v), its
    dark strength min_k (v - r_k); M is the largest strength over the 16 windows and the two polarities.  All 9 pixels of a window are > v + t (or all
    < v - t) iff its strength is > t, so the largest t for which the pixel is a 9-arc corner is M - 1.
    OpenCV: FAST_t<16> (fast.cpp) makes (x, y) a corner at threshold t iff some window has all 9 pixels > v + t or all < v - t, i.e. iff M > t; it then
    stores cornerScore<16>(ptr, pixel, t) (fast_score.cpp) = max(t, M) - 1 = M - 1.  So: corner at t  <=>  M - 1 >= t, and its score is M - 1 whatever
    t was.  At t = 0 a pixel with M = 1 is a corner with score 0; the non-maximum suppression compares scores with strict '>' against neighbours that
    are >= 0, so a score of 0 is never reported (and 0 is also what a non-corner holds in the score plane).
    Returns (M - 1, polarity [+1 bright, -1 dark, 0 if M <= 0], windows that reach M, per such window the positions 0..8 of the pixels that equal M)."""
    v = int(img[y, x])
    r = ring_values(img, x, y, ring)
    best, pol, wins = None, 0, []
    for s in (1, -1):
        for w in range(16):
            d = [s * (r[(w + j) % 16] - v) for j in range(9)]
            m = min(d)
            if best is None or m > best:
                best, pol, wins = m, s, []
            if m == best and s == pol:
                wins.append((w, [j for j in range(9) if d[j] == m]))
    if best <= 0:
        return best - 1, 0, [], []
    return best - 1, pol, [w for w, _ in wins], [p for _, p in wins]


def fast_score(img, x, y):
    """largest t in 0 .. 254 for which (x, y) is a 9-arc corner, -1 (or less) if there is none"""
    return fast_score_info(img, x, y)[0]


def pretest(img, x, y, t):
    """FAST_t's necessary test on the four even antipodal ring pairs (0, 8), (2, 10), (4, 12), (6, 14): (every pair holds a pixel > v + t, every pair holds
    a pixel < v - t).  NOT used by the score above; the scenes are classified with it."""
    v = int(img[y, x])
    r = ring_values(img, x, y)
    return (all(r[k] > v + t or r[k + 8] > v + t for k in (0, 2, 4, 6)), all(r[k] < v - t or r[k + 8] < v - t for k in (0, 2, 4, 6)))


def longest_arc(img, x, y, t):
    """(longest circular run of ring pixels > v + t, of ring pixels < v - t)"""
    v = int(img[y, x])
    r = ring_values(img, x, y)
    out = []
    for flags in ([q > v + t for q in r], [q < v - t for q in r]):
        if all(flags):
            out.append(16)
            continue
        best = run = 0
        for f in flags + flags:
            run = run + 1 if f else 0
            best = max(best, run)
        out.append(best)
    return tuple(out)


def fast_strength_map(img, ring=RING):
    """M - 1 of fast_score_info for every pixel with a full ring (rows and columns [3, dim - 4]) as an int16 plane, -1 elsewhere"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    out = np.full((h, w), -1, np.int16)
    if w < 7 or h < 7:
        return out
    s = img.astype(np.int16)
    c = s[3:h - 3, 3:w - 3]
    d = [s[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in ring]
    best = np.full(c.shape, -256, np.int16)
    for sign in (1, -1):
        for k in range(16):
            m = sign * d[k]
            for j in range(1, 9):
                m = np.minimum(m, sign * d[(k + j) % 16])
            best = np.maximum(best, m)
    out[3:h - 3, 3:w - 3] = np.maximum(best, 0) - 1
    return out


def fast_score_map(img, t, ring=RING, border=3, strength=None):
    """the score plane FAST_t fills before non-maximum suppression: M - 1 where M - 1 >= t (t clamped to 0 .. 255), 0 elsewhere and on the rows and columns
    without a full ring.  `border` = 2 is the wrong alternative 'score row 2 / column w - 3' for the scene proofs (the ring then wraps by reflection)."""
    t = min(max(int(t), 0), 255)
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    if border != 3:
        pad = np.pad(img, 3 - border, mode="reflect")
        return fast_score_map(pad, t, ring)[3 - border:3 - border + h, 3 - border:3 - border + w]
    st = fast_strength_map(img, ring) if strength is None else strength
    return np.where(st >= t, np.maximum(st, 0), 0).astype(np.uint8)


def fast_nms(img, t, dropped=None, ge_neighbour=None, **rules):
    """FastFeatureDetector(t, nonmaxSuppression = true, TYPE_9_16): [(x, y, score)] in raster order.  A pixel is kept iff its score is non-zero and
    strictly greater than the scores of all 8 neighbours; the score plane is zero outside [3, dim - 4]; nothing for w < 7 or h < 7.
    dropped: a dict that receives, per corner that is not kept, [(dx, dy, 'tie' | 'beat')] of the neighbours that stopped it.
    ge_neighbour: the wrong alternative for the scene proofs - '>=' instead of '>' against that one neighbour (dx, dy)."""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    if w < 7 or h < 7:
        return []
    sc = fast_score_map(img, t, **rules).astype(np.int32)
    out = []
    ys, xs = np.nonzero(sc)
    for y, x in zip(ys.tolist(), xs.tolist()):
        if not (3 <= x < w - 3 and 3 <= y < h - 3):
            continue                      # (only the wrong alternative `border` scores such a pixel: FAST_t never visits it as a centre)
        s = sc[y, x]
        why = []
        for dx, dy in NEIGHBOURS:
            n = sc[y + dy, x + dx]
            if n > s:
                why.append((dx, dy, "beat"))
            elif n == s and (dx, dy) != ge_neighbour:
                why.append((dx, dy, "tie"))
        if not why:
            out.append((x, y, int(s)))
        elif dropped is not None:
            dropped[(x, y)] = why
    return out


def candidates(img, t, nlevels=8, scale_factor=1.2, **rules):
    """FAST + NMS on every level of the pyramid: sorted [(level, y, x, score)] - the candidate set of the extraction"""
    levels = pyramid(img, nlevels, scale_factor)[0]
    return sorted((l, y, x, s) for l, lv in enumerate(levels) for x, y, s in fast_nms(lv, t, **rules))
