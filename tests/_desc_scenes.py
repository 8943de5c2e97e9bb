"""constructed scenes for the numeric half of the ORB32 extractor (test data): Harris response, intensity-centroid angle, 7 x 7 blur, rotated BRIEF

DETECT scenes are frames that go through the whole extraction.  They reuse the isolated dot of tests/_scenes.py: one pixel well above a constant patch is a
FAST corner whose moments vanish by symmetry; probe pixels at most 20 grey levels from the background (no corner of their own) then set the moments at will.
The motifs of a family walk through all four residues of x mod 4 (the patch alignment a = px0 & 3 of k_describe) and both parities of y.
COMPUTE scenes are a frame plus caller-given keypoints (afv_orb_compute): their angle is free, so they carry the rotation, apron, tie and comparison cases.
tests/test_orb_ref_cpu.py proves on the CPU that every scene reaches the rule it names.  numpy only, no global RNG state: the same call gives the same bytes;
the searches use tests/_orb_ref.py (the restatement), never the library or the oracle."""
import functools

import numpy as np

import _orb_ref as R

f32 = np.float32
W, H = 320, 240
BG, DOT, PROBE = 60, 160, 16       # background, dot height above it (a FAST corner at any threshold < 160), probe height (<= 20)
PITCH, MARGIN = 34, 22             # a cell holds the radius-15 disc, the column beyond it and a gap: 8 x 6 cells per frame, every one of them interior
KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def interior(x, y, w=W, h=H):
    """k_describe stages the patch of a keypoint at (x, y) of a w x h level with aligned dword loads (column offset a = (x - 21) & 3) iff the 43 rows and
    48 columns that start at (x - 21, y - 21) lie inside the level; every other keypoint takes the border path with a = 0"""
    return x - 21 >= 0 and y - 21 >= 0 and x - 21 + 48 <= w and y - 21 + 43 <= h


def alignments(centres, w=W, h=H):
    """the (a, parity of y) combinations the interior centres cover"""
    return {((x - 21) & 3, y & 1) for x, y in centres if interior(x, y, w, h)}


def _cells():
    """cell centres, all of them interior(); cell i is shifted so that x = i (mod 4) and y = i div 4 (mod 2): any 8 consecutive cells cover every
    residue of x mod 4 (every patch alignment a) with both parities of y"""
    out = []
    for row in range((H - 23 - MARGIN) // PITCH + 1):
        for col in range((W - 30 - MARGIN) // PITCH + 1):
            i = len(out)
            out.append((MARGIN + PITCH * col + (i - MARGIN - PITCH * col) % 4, MARGIN + PITCH * row + (i // 4) % 2))
    assert all(interior(x, y) for x, y in out)
    return out


def _dots(motifs):
    """motifs: one list of (u, v, delta) probes per dot -> (frame, [(x, y)] of the dots)"""
    cells = _cells()
    assert len(motifs) <= len(cells), (len(motifs), len(cells))
    img = np.full((H, W), BG, np.uint8)
    centres = []
    for (x, y), probes in zip(cells, motifs):
        img[y, x] = BG + DOT
        for u, v, d in probes:
            img[y + v, x + u] = BG + d
        centres.append((x, y))
    return img, centres


def _edge_motifs():
    """a probe on the last disc column of every row, on both sides, and one a column further out (angle 0 = empty moments)"""
    inside, outside = [], []
    for v in range(-15, 16):
        for s in (1, -1):
            inside.append([(s * R.UMAX[abs(v)], v, PROBE)])
            outside.append([(s * (R.UMAX[abs(v)] + 1), v, PROBE)])
    return inside, outside


def disc_edge(part):
    """part 0 / 1 / 2: a third of the 62 last-column probes interleaved with a third of the 62 probes one column outside.  Returns frame, centres, kinds"""
    inside, outside = _edge_motifs()
    motifs, kinds = [], []
    for i in range(part, 62, 3):
        motifs += [inside[i], outside[i]]
        kinds += ["inside", "outside"]
    img, centres = _dots(motifs)
    return img, centres, kinds


ATAN_PROBES = [("axis+x", [(9, 0, PROBE)]), ("axis-x", [(-9, 0, PROBE)]), ("axis+y", [(0, 9, PROBE)]), ("axis-y", [(0, -9, PROBE)]),
               ("diag++", [(7, 7, PROBE)]), ("diag-+", [(-7, 7, PROBE)]), ("diag--", [(-7, -7, PROBE)]), ("diag+-", [(7, -7, PROBE)]),
               ("zero", []), ("diag++", [(10, 10, 20)]), ("diag--", [(-5, -5, 3)]), ("diag+-", [(6, -6, 11), (1, -1, 7)]),
               ("axis-x", [(-15, 0, 1)]), ("axis-y", [(0, -15, 20), (0, -6, 5)]), ("zero", [(6, 2, 9), (-6, -2, 9)]), ("diag-+", [(-10, 10, 1)])]


def atan_cases():
    """the four axes (m01 = 0 with m10 < 0 and m10 = 0 with m01 < 0 among them), the four diagonals (|m01| == |m10|: the branch test decides the float
    bits) and empty moments, each kind more than once; the list is laid out twice so that every motif meets two alignments"""
    motifs = [p for _, p in ATAN_PROBES] + [p for _, p in ATAN_PROBES[5:] + ATAN_PROBES[:5]]
    kinds = [k for k, _ in ATAN_PROBES] + [k for k, _ in ATAN_PROBES[5:] + ATAN_PROBES[:5]]
    img, centres = _dots(motifs)
    return img, centres, kinds


def half_planes(direction):
    """0 / 255 stripes 40 px wide (a disc sees one step only) with a dot of 128 on the dark and on the bright side of every step: exactly 9 ring pixels
    differ from it by more than the threshold.  Half discs of 0 / 255 are the largest moments there are, and a step through the 7 x 7 block the largest
    Sobel sums: direction 'v' (vertical steps: m10 = +-max, Harris a), 'h' (m01, Harris b), 'd+' / 'd-' (both diagonals: Harris c of either sign, and
    a * b next to c * c).  The steps sit at 41 k (vertical) so that they walk through the residues of x mod 4."""
    yy, xx = np.mgrid[0:H, 0:W]
    t = {"v": xx, "h": yy, "d+": xx + yy, "d-": xx - yy + H}[direction]
    period = 41 if direction in "vh" else 58
    band = t // period
    img = np.where(band % 2 == 1, 255, 0).astype(np.uint8)
    centres = []
    n = 0
    for k in range(1, int(t.max()) // period + 1):
        for side in (0, 1):                    # last coordinate of band k - 1 / first coordinate of band k
            tc = k * period - 1 + side
            for along in range(20 + 7 * (k % 3) + 18 * side, 300, 37):
                if direction == "v":
                    x, y = tc, along
                elif direction == "h":
                    x, y = along, tc
                elif direction == "d+":
                    x, y = along, tc - along
                else:
                    x, y = along, along + H - tc
                if interior(x, y):
                    img[y, x] = 128
                    centres.append((x, y))
                    n += 1
    return img, centres, [direction] * n


def checker():
    """one-pixel 0 / 255 checkerboard patches (every sample that moves by a pixel flips; Sobel sums of a pure checkerboard vanish, the ring breaks that) with
    the 16 ring pixels at 0 and the centre at 255, on the constant background"""
    ring = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
    img = np.full((H, W), BG, np.uint8)
    centres = []
    for i, (x, y) in enumerate(_cells()[20:28]):
        r = 8 + i % 3
        yy, xx = np.mgrid[y - r:y + r + 1, x - r:x + r + 1]
        img[y - r:y + r + 1, x - r:x + r + 1] = np.where((xx + yy + i) % 2 == 0, 255, 0)
        for dx, dy in ring:
            img[y + dy, x + dx] = 0
        img[y, x] = 255
        centres.append((x, y))
    return img, centres, ["checker"] * len(centres)


def _lcg(seed, n):
    out = np.empty(n, np.int64)
    s = seed
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out[i] = s >> 40
    return out


def saturation():
    """patches of 250 .. 255 (4 x 4 px blocks, and whole patches of 254 / 255) with a dark dot: S / 65536 >= 255.5 from a flat 254 on (q = 256: saturated, 0
    if it wrapped) and S >= 2^24 where everything under the taps is 255 (the taps sum to 257: 257^2 * 255 > 2^24, beyond the exact u32 -> f32 range)"""
    img = np.full((H, W), BG, np.uint8)
    centres = []
    r = _lcg(7, 16 * 121)
    for i, (x, y) in enumerate(_cells()[:16]):
        blocks = 250 + (r[i * 121:(i + 1) * 121] % 6).reshape(11, 11)
        if i % 4 == 1:
            blocks[:] = 255
        elif i % 4 == 3:
            blocks[:, :6] = 254
            blocks[:, 6:] = 252
        patch = np.kron(blocks, np.ones((3, 3), np.int64))[:33, :33]
        img[y - 16:y + 17, x - 16:x + 17] = patch
        img[y, x] = 0
        centres.append((x, y))
    return img, centres, ["saturation"] * len(centres)


DETECT = {"disc_edge0": lambda: disc_edge(0), "disc_edge1": lambda: disc_edge(1), "disc_edge2": lambda: disc_edge(2), "atan": atan_cases, "half_v": lambda: half_planes("v"),
          "half_h": lambda: half_planes("h"), "half_d+": lambda: half_planes("d+"), "half_d-": lambda: half_planes("d-"), "checker": checker,
          "saturation": saturation}


@functools.lru_cache(maxsize=None)
def detect_scene(name):
    """(frame, [(x, y)] of the intended level-0 keypoints, kind of each)"""
    img, centres, kinds = DETECT[name]()
    img.setflags(write=False)
    return img, centres, kinds


# ---------------------------------------------------------------- compute scenes ----------------------------------------------------------------
def keypoints(rows):
    """rows of (x, y, angle, octave) -> KP_DTYPE"""
    k = np.zeros(len(rows), KP_DTYPE)
    for i, (x, y, a, l) in enumerate(rows):
        k[i] = (x, y, 31.0, a, 0.0, l, -1)
    return k


def _weights():
    t = np.array(R.TAPS, np.int64)
    return np.outer(t, t)


@functools.lru_cache(maxsize=None)
def _tie_deltas(target):
    """non-negative additions d[7][7] to a flat 7 x 7 window with sum(w * d) == target, w = products of two taps (gcd 1): unbounded coin change over the
    distinct weights (one prefix-or per residue class and weight), the count of a weight spread over the positions that carry it"""
    w = _weights()
    coins = sorted(set(w.ravel().tolist()), reverse=True)
    n = target + 1
    reach = np.zeros(n, bool)
    reach[0] = True
    stages = []
    for c in coins:
        stages.append(reach)
        pad = (-n) % c
        m = np.concatenate([reach, np.zeros(pad, bool)]).reshape(-1, c)
        reach = np.logical_or.accumulate(m, axis=0).ravel()[:n]
    assert reach[target], target
    d = np.zeros((7, 7), np.int64)
    s = target
    for c, before in zip(coins[::-1], stages[::-1]):
        cnt = 0
        while not before[s]:
            s -= c
            cnt += 1
        pos = np.argwhere(w == c)
        for j in range(cnt):
            i0, j0 = pos[j % len(pos)]
            d[i0, j0] += 1
    assert s == 0 and int((w * d).sum()) == target
    return d


def tie_window(q):
    """a 7 x 7 window whose filter sum is exactly q * 65536 + 32768: flat q plus the additions"""
    win = q + _tie_deltas(q * 65536 + 32768 - int(_weights().sum()) * q)
    assert win.max() <= 255 and int((_weights() * win).sum()) == q * 65536 + 32768
    return win.astype(np.uint8)


def far_pairs():
    """test pairs whose two points are at least 8 px apart along an axis (their 7 x 7 windows are disjoint), both at least 4 px from the centre"""
    p = R.PATTERN
    d = np.abs(p[:, 0] - p[:, 1]).max(1)
    return [int(i) for i in np.flatnonzero((d >= 8) & (np.abs(p).max(2).min(1) >= 4))]


TIE_Q = {"even": 40, "odd": 41}   # flat values <= 63 blur to themselves under every rounding rule (513 v < 32768)


def ties():
    """angle 0: the sample positions are the pattern itself.  Keypoint i uses test pair far_pairs()[3 i]: the window under one of its points sums to
    q * 65536 + 32768 (q even / odd), the window under the other is flat.  Tie first: partner q + 1, bit = blurred < q + 1; tie second: partner q,
    bit = q < blurred.  half-even gives q for the even and q + 1 for the odd tie; half-up lifts the even one, truncation drops the odd one.
    Keypoints 0..7 are interior (all four patch alignments, both parities of y); 8..15 repeat them on the rows next to the lower frame edge, where
    the patch leaves the level (the border path).  Returns frame, keypoints, [(pair, parity of q, tie_first)]"""
    img = np.full((H, W), 50, np.uint8)
    rows, meta = [], []
    pairs = far_pairs()
    cells = _cells()[:8] + [(x, H - 18 + y % 2) for x, y in _cells()[:8]]
    for i in range(16):
        x, y = cells[i]
        pair = pairs[3 * (i % 8)]
        parity, first = ("even", "odd")[i % 2], (i // 2) % 2 == 0
        q = TIE_Q[parity]
        (tx, ty), (px, py) = (R.PATTERN[pair][0], R.PATTERN[pair][1]) if first else (R.PATTERN[pair][1], R.PATTERN[pair][0])
        img[y + py - 3:y + py + 4, x + px - 3:x + px + 4] = q + 1 if first else q
        img[y + ty - 3:y + ty + 4, x + tx - 3:x + tx + 4] = tie_window(q)
        rows.append((x, y, 0.0, 0))
        meta.append((pair, parity, first))
    img.setflags(write=False)
    return img, keypoints(rows), meta


def comparisons():
    """angle 0 on a constant frame (all 256 bits are 0: no value is below itself), and keypoints where the windows under the two points of three pairs are
    flat (v, v), (v, v + 1) and (v + 1, v): equal, and one apart in each direction.  Keypoints 0..7 are interior (all four patch alignments, both
    parities of y), 8..15 repeat them next to the lower frame edge (the border path).  Returns frame, keypoints, [[(pair, t0, t1)]]"""
    img = np.full((H, W), 50, np.uint8)
    rows, meta = [], []
    pairs = far_pairs()
    cells = _cells()[:8] + [(x, H - 18 + y % 2) for x, y in _cells()[:8]]
    for i in range(16):
        x, y = cells[i]
        mine = []
        if i % 8 >= 2:                      # keypoints 0, 1, 8 and 9 stay on the constant frame
            for j, (a, b) in enumerate(((0, 0), (0, 1), (1, 0))):
                pair = pairs[(7 * (i % 8) + 5 * j) % len(pairs)]
                v = 20 + 2 * i
                ok = all(np.abs(R.PATTERN[pair][:, None] - R.PATTERN[p][None]).max(2).min() >= 7 for p, _, _ in mine)
                if not ok:
                    continue
                for (sx, sy), val in zip(R.PATTERN[pair], (v + a, v + b)):
                    img[y + sy - 3:y + sy + 4, x + sx - 3:x + sx + 4] = val
                mine.append((pair, v + a, v + b))
        rows.append((x, y, 0.0, 0))
        meta.append(mine)
    img.setflags(write=False)
    return img, keypoints(rows), meta


def _rotated(angles, sincos):
    """float32 rotated pattern coordinates [A, 1024] of every angle"""
    a, b = sincos(angles)
    x, y = R.PATTERN[..., 0].astype(f32).ravel(), R.PATTERN[..., 1].astype(f32).ravel()
    a, b = a[:, None], b[:, None]
    return np.concatenate([x * a - y * b, x * b + y * a], 1)


@functools.lru_cache(maxsize=None)
def searched_angles(n_half=64, n_moved=16):
    """(angles for which some rotated pattern coordinate lies within 2 float32 ulps of n + 0.5, angles for which cos / sin evaluated in float32 put a sample
    on another pixel than the double-then-float ones): candidates are the float32 neighbours of the solutions of x cos t - y sin t = k + 0.5 for the
    pattern's points, evaluated with the restatement's arithmetic"""
    pts = np.unique(R.PATTERN.reshape(-1, 2), axis=0).astype(np.float64)[::5]
    r, phi = np.hypot(pts[:, 0], pts[:, 1]), np.arctan2(pts[:, 1], pts[:, 0])
    cand = []
    for k in range(-14, 14):
        hk = k + 0.5
        ok = r > abs(hk) + 0.05
        t0 = np.arccos(hk / r[ok])
        for t in (t0 - phi[ok], -t0 - phi[ok]):
            cand.append(np.degrees(t) % 360.0)
    base = np.concatenate(cand).astype(f32)
    base = base[(base > 1) & (base < 359)]
    nb, up, down = [base], base, base
    for _ in range(3):
        up, down = np.nextafter(up, f32(400)), np.nextafter(down, f32(-400))
        nb += [up, down]
    angles = np.unique(np.concatenate(nb))
    half, moved = [], []
    for chunk in np.array_split(angles, max(1, len(angles) // 2048)):
        c = _rotated(chunk, R.sincos_f64)
        frac = np.abs(c - np.floor(c) - f32(0.5))
        near = (frac <= 2 * np.spacing(np.abs(c))).any(1)
        half += chunk[near].tolist()
        c32 = _rotated(chunk, lambda a: R._sincos_f32(np.asarray(a, f32) * R.FACTOR_PI))
        moved += chunk[(np.rint(c) != np.rint(c32)).any(1)].tolist()
    assert len(half) >= n_half and len(moved) >= n_moved, (len(half), len(moved))
    pick = lambda v, n: [v[i * len(v) // n] for i in range(n)]  # spread over the circle
    return tuple(pick(half, n_half)), tuple(pick(moved, n_moved))


def fixed_angles():
    return (0.0, 90.0, 180.0, 270.0, float(np.nextafter(f32(360), f32(0))), 360.0, -0.0, -45.3, -359.5, -90.0, 405.3, 725.0, 45.0, 135.0)


def rotation_angles():
    half, moved = searched_angles()
    return fixed_angles() + half + moved


def rotation(kind):
    """caller-given angles on a noise frame ('noise') or a one-pixel checkerboard ('checker': a sample that lands one pixel off reads the other colour, 129
    against 128 after the blur), every angle at four keypoints that cover the four patch alignments and both parities"""
    if kind == "noise":
        img = (_lcg(11, W * H) % 256).astype(np.uint8).reshape(H, W)
    else:
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.where((xx + yy) % 2 == 0, 255, 0).astype(np.uint8)
    rows = []
    for i, a in enumerate(rotation_angles()):
        for j in range(4):
            rows.append((40.0 + 23 * (i % 11) + j, 30.0 + 17 * (i // 11) + (j // 2) % 2, a, 0))
    img.setflags(write=False)
    return img, keypoints(rows)


APRON_W = APRON_H = 115


def apron(lscale, lw, lh):
    """115 x 115 noise; keypoints whose patch leaves level 0 and the top level on each side and in each corner (centres on the first / last row and column
    and one beyond), and interior ones at the four alignments, each under every one of the rotation angles.  lscale / lw / lh: the level geometry"""
    img = (_lcg(13, APRON_W * APRON_H) % 256).astype(np.uint8).reshape(APRON_H, APRON_W)
    angles = rotation_angles()
    rows = []
    top = len(lscale) - 1
    for l in (0, top):
        w, h, s = lw[l], lh[l], f32(lscale[l])
        centres = [(0, 0), (w, 0), (0, h), (w, h), (w // 2, 0), (w // 2, h), (0, h // 2), (w, h // 2), (w - 1, h - 1), (5, 7), (w - 6, h - 4), (3, h - 9)]
        if l == 0:
            centres += [(57, 57), (58, 56), (59, 57), (60, 56)]
        for a in angles:
            for cx, cy in centres:
                rows.append((f32(cx) * s, f32(cy) * s, a, l))
    img.setflags(write=False)
    return img, keypoints(rows)
