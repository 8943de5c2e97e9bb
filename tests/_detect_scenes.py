"""constructed scenes for the front of the ORB32 pipeline (test data): the pyramid (k_pyramid.hip) and FAST-9 score + NMS (k_fast.hip)

Every generator returns frames together with the facts it was built for; tests/test_detect_ref_cpu.py proves the facts with the plain restatement
tests/_detect_ref.py (and holds the CPU oracle to it on every frame), tests/test_gpu_detect_scenes.py runs the frames through the kernels.

A FAST motif is a 9 x 9 patch of the centre value v (radius 4: the ring of every NMS neighbour of the centre lies inside it, see EDGE_CELL in
tests/_scenes.py) whose ring pixels k carry v + s d_k.  No NMS neighbour of the centre can be a corner (a ring of radius 3 around a neighbour meets the
centre's ring in at most 4 pixels), so the centre's fate is the motif's alone.  The altered ring pixels may well be corners themselves (a bright pixel on a
flat patch is one): they are content like any other and are compared with the oracle, but they are not designed facts.
k_fast_nms works on 64 x 32 tiles; `rx`, `ry` below are x % 64 and y % 32.
numpy only, seeded generators only: the same arguments give the same bytes."""
import functools

import numpy as np

import _detect_ref as R

RING = R.RING
BG = 128
TILE_W, TILE_H = 64, 32
THRESHOLDS = (1, 7, 20, 254)


def motif(img, x, y, v, s, diffs):
    """9 x 9 patch of v around (x, y); ring pixel k = v + s * diffs[k]"""
    img[y - 4:y + 5, x - 4:x + 5] = v
    for k, d in diffs.items():
        dx, dy = RING[k % 16]
        val = v + s * d
        assert 0 <= val <= 255, (v, s, d)
        img[y + dy, x + dx] = val


def _centre(rng, s, dmax):
    """a centre value that leaves room for v + s * dmax"""
    return int(rng.integers(0, 256 - dmax)) if s > 0 else int(rng.integers(dmax, 256))


class Canvas:
    """a frame that hands out free square regions: place() returns the first position in raster order (on a lattice of the region size where a coordinate
    is free, at every x with x % 64 == rx / y with y % 32 == ry where it is not) whose (2 half + 1)^2 region is unused and inside the frame"""

    def __init__(self, w, h, bg=BG):
        self.img = np.full((h, w), bg, np.uint8)
        self.used = np.zeros((h, w), bool)
        self.facts = []

    def place(self, half, rx=None, ry=None):
        h, w = self.img.shape
        step = 2 * half + 1
        xs = range(half, w - half, step) if rx is None else [x for x in range(half, w - half) if x % TILE_W == rx]
        ys = range(half, h - half, step) if ry is None else [y for y in range(half, h - half) if y % TILE_H == ry]
        for y in ys:
            for x in xs:
                if not self.used[y - half:y + half + 1, x - half:x + half + 1].any():
                    self.used[y - half:y + half + 1, x - half:x + half + 1] = True
                    return x, y
        return None


def _pack(w, h, jobs, bg=BG):
    """jobs: [(half, rx, ry, draw(img, x, y) -> [facts])], the constrained ones first on every frame.  Returns [(image, facts)]: as many frames as the jobs need."""
    jobs = sorted(jobs, key=lambda j: (j[1] is None) + (j[2] is None))   # stable: both residues given, one given, free
    frames = []
    while jobs:
        c = Canvas(w, h, bg)
        rest = []
        for job in jobs:
            at = c.place(*job[:3])
            if at is None:
                rest.append(job)
            else:
                c.facts += job[3](c.img, *at)
        assert len(rest) < len(jobs), "a job fits no empty %d x %d frame" % (w, h)
        frames.append((c.img, c.facts))
        jobs = rest
    return frames


# ---------------------------------------------------------------- FAST score and tile position ----------------------------------------------------------------
SWEEP_PITCH = 13      # coprime with 64 and 32, >= 12 (EDGE_CELL)
SWEEP_FRAMES = 4


def tile_sweep(f, t=20, w=640, h=480):
    """frame f of 4: isolated motifs on a 13 x 13 lattice.  x = 8 + ox + 13 i, y = 8 + 13 j: the 36 rows reach every y % 32, the columns of frames 0, 1
    (ox = 0, i = 0 .. 47) and of frames 2, 3 (ox = 48 = 13 * 48 mod 64: the same progression continued) every x % 64 between them.  The polarity of a cell is
    the parity of i + j + f, so frames f and f + 1 give every position both polarities and every tile holds both.  Centre, arc start 0..15, arc
    length 9..16 and the per-pixel differences (t + 1 .. t + 1 + spread) are drawn from the frame's generator, independently of the position.
    Facts: dict(x, y, pol, score, start, length) - every one a kept corner."""
    rng = np.random.default_rng(1000 + f)
    ox = 0 if f < 2 else SWEEP_PITCH * len(range(8, w - 8, SWEEP_PITCH)) % TILE_W
    img = np.full((h, w), BG, np.uint8)
    facts = []
    for j in range((h - 16) // SWEEP_PITCH + 1):
        y = 8 + SWEEP_PITCH * j
        for i in range(w):
            x = 8 + ox + SWEEP_PITCH * i
            if x > w - 9:
                break
            s = 1 if (i + j + f) % 2 == 0 else -1
            L, a = int(rng.integers(9, 17)), int(rng.integers(0, 16))
            d = (t + 1 + rng.integers(0, int(rng.integers(0, 60)) + 1, L)).tolist()
            motif(img, x, y, _centre(rng, s, max(d)), s, {a + k: d[k] for k in range(L)})
            ring = [0] * 16
            for k in range(L):
                ring[(a + k) % 16] = d[k]
            score = max(min(ring[(win + j) % 16] for j in range(9)) for win in range(16)) - 1      # the best 9-window of the arc
            facts.append(dict(x=x, y=y, pol=s, score=score, start=a, length=L))
    return img, facts


def score_network(t, w=320, h=240):
    """one motif per (polarity, window start 0..15, position 0..8): a 9-arc whose unique weakest pixel (difference m) sits at that position of that window, the
    other eight stronger by 1..30 - the score m - 1 is decided by that pixel alone; arcs of length 10..16 in which each possible window in turn is the
    unique best one (the arc pixels next to it are weaker than its weakest); centres 0 and 255 with rings at 255 and 0 (score 254), scores of exactly t,
    centres within t of 0 (bright arcs) and of 255 (dark arcs), arcs whose strongest pixel is 255 / 0.
    Facts: dict(x, y, pol, score, windows, positions [None: every pixel of the window ties], length of the arc, q [index of the best window inside a longer
    arc]) - every one a kept corner."""
    assert 1 <= t <= 100
    rng = np.random.default_rng(2000 + t)
    jobs = []

    def job(v, s, diffs, score, windows, positions, q=None):
        def draw(img, x, y):
            motif(img, x, y, v, s, diffs)
            return [dict(x=x, y=y, pol=s, score=score, windows=windows, positions=positions, length=len(diffs), q=q)]
        jobs.append((6, None, None, draw))

    for s in (1, -1):
        for win in range(16):
            for pos in range(9):
                m = t + 1 + int(rng.integers(0, 41))
                d = {win + j: m + int(rng.integers(1, 31)) for j in range(9)}
                d[win + pos] = m
                job(_centre(rng, s, max(d.values())), s, d, m - 1, [win], [[pos]])
        for L in range(10, 17):
            for q in range(16 if L == 16 else L - 8):
                a, pos = int(rng.integers(0, 16)), int(rng.integers(0, 9))
                m = t + 2 + int(rng.integers(0, 41))
                d = {(a + k) % 16: t + 1 + int(rng.integers(0, m - t + 20)) for k in range(L)}
                for j in range(9):
                    d[(a + q + j) % 16] = m + int(rng.integers(1, 21))
                d[(a + q + pos) % 16] = m
                for k in ((q - 1, q + 9) if L == 16 else [k for k in (q - 1, q + 9) if 0 <= k < L]):
                    d[(a + k) % 16] = t + 1 + int(rng.integers(0, m - t - 1))      # t + 1 .. m - 1: every other window of the arc holds one of them
                assert len(d) == L
                job(_centre(rng, s, max(d.values())), s, d, m - 1, [(a + q) % 16], [[pos]], q)
        v0 = 0 if s > 0 else 255
        job(v0, s, {k: 255 for k in range(16)}, 254, list(range(16)), None)                 # full ring at the other end of the range
        for a in (3, 12):
            job(v0, s, {a + k: 255 for k in range(9)}, 254, [a], None)
            job(100, s, {a + k: t + 1 for k in range(9)}, t, [a], None)                      # the smallest reportable score
        for v in ((0, 1, t - 1, t) if s > 0 else (255 - t, 256 - t, 254, 255)):             # v - t < 0 / v + t > 255
            a, m = int(rng.integers(0, 16)), t + 1 + int(rng.integers(0, 41))
            d = {(a + j) % 16: m + int(rng.integers(1, 31)) for j in range(9)}
            d[(a + 4) % 16] = m
            job(v, s, d, m - 1, [a], [[4]])
        for pos in (0, 8):                                                                  # the strongest ring pixel is 255 / 0
            a, m = int(rng.integers(0, 16)), t + 1 + int(rng.integers(0, 41))
            d = {(a + j) % 16: m + int(rng.integers(1, 31)) for j in range(9)}
            d[(a + pos) % 16] = m
            job(255 - max(d.values()) if s > 0 else max(d.values()), s, d, m - 1, [a], [[pos]])
    return _pack(w, h, jobs)


def pretest_traps(t, w=320, h=240):
    """rings that pass FAST_t's necessary test on the four even antipodal pairs and are decided by the 9-arc test alone:
      'arc8'      8 contiguous pixels beyond the threshold (one of every antipodal pair), in every rotation and both polarities: no corner;
      'arc8+6'    8 beyond, one exactly on the threshold, 6 beyond, one on the threshold: no corner;
      'both_none' every even pair holds a brighter AND a darker pixel (the pixel enters both lists), odd ring pixels at v: a corner in neither polarity;
      'both_one'  9 brighter + 7 darker pixels (the 9-arc starts at an odd index: an arc from an even index holds a whole even pair) and the mirror: both
                  lists, a corner in one polarity.
    Facts: dict(x, y, kind, pol, score [None: not a corner])."""
    assert 1 <= t <= 100
    rng = np.random.default_rng(3000 + t)
    jobs = []

    def job(kind, v, pol, score, values):
        def draw(img, x, y):
            img[y - 4:y + 5, x - 4:x + 5] = v
            for k, val in values.items():
                img[y + RING[k % 16][1], x + RING[k % 16][0]] = val
            return [dict(x=x, y=y, kind=kind, pol=pol, score=score)]
        jobs.append((6, None, None, draw))

    def beyond():
        return t + 1 + int(rng.integers(0, 40))

    for s in (1, -1):
        for r in range(16):
            v = _centre(rng, s, t + 40)
            job("arc8", v, s, None, {r + k: v + s * beyond() for k in range(8)})
            vals = {r + k: v + s * beyond() for k in range(16)}
            vals[r + 8] = vals[r + 15] = v + s * t
            job("arc8+6", v, s, None, vals)
            v = int(rng.integers(t + 40, 216 - t))
            job("both_none", v, 0, None, {k: v + (s if (k - r) % 16 < 8 else -s) * beyond() for k in range(0, 16, 2)})
        for r in range(1, 16, 2):
            v = int(rng.integers(t + 40, 216 - t))
            d = [beyond() for _ in range(16)]
            job("both_one", v, s, min(d[:9]) - 1, {r + k: v + (s if k < 9 else -s) * d[k] for k in range(16)})
    return _pack(w, h, jobs)


# ---------------------------------------------------------------- NMS and the FAST border ----------------------------------------------------------------
DIRS = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
NMS_P, NMS_C = 60, 101     # flat patches of 60, bright single pixels from 60 + 101 upwards: a lone pixel p + c scores c - 1 (its 16 ring pixels are all c darker)


def _nms_anchors(dx, dy):
    """(placement, rx, ry) of the first pixel P of a pair whose second pixel is P + (dx, dy): inside a tile; with the pair across (or, for a pair parallel to
    it, on either side of) a vertical seam x % 64 = 63 | 0; the same for a horizontal seam y % 32 = 31 | 0; across a tile corner"""
    xs = [63 if dx > 0 else 0] if dx else [63, 0]
    ys = [31 if dy > 0 else 0] if dy else [31, 0]
    out = [("inside", 20, 12)] + [("vseam", rx, 12) for rx in xs] + [("hseam", 20, ry) for ry in ys]
    return out + [("corner", rx, ry) for rx in ((xs if dx else [63, 0])) for ry in (ys if dy else [31, 0])]


def nms_pairs(w=320, h=240):
    """adjacent bright single pixels on flat patches (independent scores, as the pairs of tests/_scenes.py::fast_edges):
      pairs in each of the 8 directions, equal (neither is kept) and one apart (the higher is kept), at every placement of _nms_anchors;
      chains of three with rising scores (horizontal, vertical, both diagonals, L-shaped): the middle one is dropped and still suppresses the lowest;
      2 x 2 and 3 x 3 blocks of equal corners: none is kept - chains and blocks inside a tile and over a tile corner.
    Facts: dict(kind, place, dir, kept [(x, y, score)], dropped [(x, y, 'tie' | 'beat')])."""
    jobs = []

    def job(kind, place, d, rx, ry, pixels):
        """pixels: [(dx, dy, c)] around the anchor, |dx|, |dy| <= 1"""
        def draw(img, x, y):
            img[y - 5:y + 6, x - 5:x + 6] = NMS_P
            for dx, dy, c in pixels:
                img[y + dy, x + dx] = NMS_P + c
            top = max(c for _, _, c in pixels)
            tops = [(x + dx, y + dy, c - 1) for dx, dy, c in pixels if c == top]
            kept = tops if len(tops) == 1 else []
            dropped = [(x + dx, y + dy, "beat" if c < top else "tie") for dx, dy, c in pixels if (x + dx, y + dy, c - 1) not in kept]
            return [dict(kind=kind, place=place, dir=d, kept=kept, dropped=dropped)]
        jobs.append((7, rx, ry, draw))

    for d in DIRS:
        for place, rx, ry in _nms_anchors(*d):
            job("equal", place, d, rx, ry, [(0, 0, NMS_C), (d[0], d[1], NMS_C)])
            job("above", place, d, rx, ry, [(0, 0, NMS_C), (d[0], d[1], NMS_C + 1)])
    chains = {"h": [(-1, 0), (0, 0), (1, 0)], "v": [(0, -1), (0, 0), (0, 1)], "d": [(-1, -1), (0, 0), (1, 1)], "a": [(1, -1), (0, 0), (-1, 1)],
              "L": [(-1, 0), (0, 0), (0, 1)], "h-": [(1, 0), (0, 0), (-1, 0)], "v-": [(0, 1), (0, 0), (0, -1)]}
    for place, rx, ry in (("inside", 21, 13), ("corner", 63, 31), ("corner", 0, 0), ("vseam", 0, 14), ("hseam", 22, 31)):
        for name, offs in chains.items():
            job("chain", place, name, rx, ry, [(dx, dy, NMS_C + i) for i, (dx, dy) in enumerate(offs)])
        job("block2", place, None, rx, ry, [(dx, dy, NMS_C) for dx in (0, 1) for dy in (0, 1)])
        job("block3", place, None, rx, ry, [(dx, dy, NMS_C) for dx in (-1, 0, 1) for dy in (-1, 0, 1)])
    return _pack(w, h, jobs)


BORDER_SIZES = [(193, 97), (194, 98), (195, 99), (196, 100), (255, 127), (256, 128), (203, 150)]   # last tile column 1, 2, 3, 4, 63, 64, 11 wide; row 1, 2, 3, 4, 31, 32, 22
BORDER_LEVELS = 4          # 97 / 1.2^3 = 56: every level of every size stays >= 32 px
BORDER_VARIANTS = 4
BORDER_P, BORDER_C = 60, 100


def border(w, h, variant):
    """bright single pixels on a flat frame at the FAST border: line 3 from an edge (rows / columns 3 and dim - 4) is the last one with a score, line 2
    (2 and dim - 3) the first without.  Along each side, 12 px apart, in turn (the turn starts at `variant`):
      0 a pixel on line 3: kept;  1 a pixel on line 2: nothing;  2 a pixel on line 3 and a stronger one next to it on line 2: the scored one is kept (a
      stronger pixel on the unscored line must not suppress it);  3 the same with the stronger one diagonally next to it;  4 two equal pixels on line 3: a tie.
    In corner k (0 top left, 1 top right, 2 bottom left, 3 bottom right) configuration (variant + k) % 4:
      0 a pixel on (3, 3): kept;  1 a pixel on (2, 2): nothing;  2 (3, 3) with stronger pixels on (2, 2), (2, 3), (3, 2): kept;  3 a pixel on (2, 3): nothing.
    Facts: dict(kept [(x, y, score)], nothing [(x, y)], lines {(side, line)} the frame touches)."""
    img = np.full((h, w), BORDER_P, np.uint8)
    kept, nothing, lines = [], [], set()
    c = BORDER_C

    def put(side, u, q, val):
        """position u along the side, line q from the edge"""
        x, y = {"top": (u, q), "bottom": (u, h - 1 - q), "left": (q, u), "right": (w - 1 - q, u)}[side]
        img[y, x] = BORDER_P + val
        lines.add((side, q))
        return x, y

    for side in ("top", "bottom", "left", "right"):
        n = w if side in ("top", "bottom") else h
        for k, u in enumerate(range(15, n - 15, 12)):
            turn = (k + variant) % 5
            if turn == 0:
                kept.append(put(side, u, 3, c) + (c - 1,))
            elif turn == 1:
                nothing.append(put(side, u, 2, c))
            elif turn in (2, 3):
                kept.append(put(side, u, 3, c) + (c - 1,))
                nothing.append(put(side, u + (turn == 3), 2, c + 40))
            else:
                nothing += [put(side, u, 3, c), put(side, u + 1, 3, c)]
    for k in range(4):
        fx = (lambda q: q) if k % 2 == 0 else (lambda q: w - 1 - q)
        fy = (lambda q: q) if k < 2 else (lambda q: h - 1 - q)
        cfg = (variant + k) % 4

        def put2(qx, qy, val):
            img[fy(qy), fx(qx)] = BORDER_P + val
            return fx(qx), fy(qy)
        if cfg == 0:
            kept.append(put2(3, 3, c) + (c - 1,))
        elif cfg == 1:
            nothing.append(put2(2, 2, c))
        elif cfg == 2:
            kept.append(put2(3, 3, c) + (c - 1,))
            nothing += [put2(2, 2, c + 40), put2(2, 3, c + 40), put2(3, 2, c + 40)]
        else:
            nothing.append(put2(2, 3, c))
    return img, dict(kept=kept, nothing=nothing, lines=lines)


# ---------------------------------------------------------------- levels >= 1 ----------------------------------------------------------------
TWO_LEVELS, TWO_SCALE = 3, 2.0
D_W, D_H = 160, 120                                    # the designed image of two_to_one: level 0 is 640 x 480
D_BORDER_SIZES = [(129, 65), (132, 100), (160, 96)]    # last tile column 1, 4, 32 wide; last tile row 1, 4, 32 high


def two_to_one(D):
    """D replicated in 4 x 4 blocks: with scale factor 2.0 and 3 levels, level l is D replicated 2^(2 - l) times exactly (every 2 : 1 resize averages a
    constant 2 x 2 block: offsets 2 d, weights 128) - designed content reaches k_fast_nms through the pyramid buffer at levels 1 and 2"""
    return np.repeat(np.repeat(D, 4, axis=0), 4, axis=1)


@functools.lru_cache(maxsize=None)
def designed_images():
    """{name: (D, facts, kind)}: score_network(20), nms_pairs and border as 160 x 120 (and odd-sized) images for two_to_one"""
    out = {}
    for i, (img, facts) in enumerate(score_network(20, D_W, D_H)):
        out["score_network/%d" % i] = (img, facts, "score_network")
    for i, (img, facts) in enumerate(nms_pairs(D_W, D_H)):
        out["nms_pairs/%d" % i] = (img, facts, "nms_pairs")
    for w, h in D_BORDER_SIZES:
        for v in range(BORDER_VARIANTS):
            img, facts = border(w, h, v)
            out["border/%dx%d/%d" % (w, h, v)] = (img, facts, "border")
    return out


# ---------------------------------------------------------------- pyramid ----------------------------------------------------------------
RESIZE_SIZES = [(640, 480), (600, 480), (203, 150), (333, 251), (115, 115)]    # 600 -> 500: level 1 at exactly 1.2


def resize_extremes(w, h):
    """{name: image}: one-pixel checkerboard of 0 / 255, constant 255 (every horizontal sum is 65280 = 255 * 256, the largest) and constant 0, single 255
    pixels on 0 along the first and last two columns and rows (16 apart, staggered) and the inverse, and a noise frame"""
    yy, xx = np.mgrid[0:h, 0:w]
    dots = np.zeros((h, w), np.uint8)
    for k, x in enumerate((0, 1, w - 2, w - 1)):
        dots[5 + 4 * k:h - 3:16, x] = 255
    for k, y in enumerate((0, 1, h - 2, h - 1)):
        dots[y, 7 + 4 * k:w - 3:16] = 255
    return {"checker": (((xx + yy) & 1) * 255).astype(np.uint8), "ones": np.full((h, w), 255, np.uint8), "zeros": np.zeros((h, w), np.uint8),
            "dots": dots, "inverse": 255 - dots, "noise": np.random.default_rng(w * 1000 + h).integers(0, 256, (h, w), dtype=np.uint8)}


TIE_VALUES = (0x7fff, 0x8000, 0x8001)
TIE_SEEDS = (0, 1, 3, 4, 5, 6, 8, 17)        # found by search_tie_seeds()


def tie_frame(seed, w=640, h=480):
    return np.random.default_rng(4000 + seed).integers(0, 256, (h, w), dtype=np.uint8)


def tie_counts(img, nlevels=8, scale_factor=1.2):
    """per level >= 1: how many pixels have exactly 0x7fff, 0x8000, 0x8001 in the low 16 bits of their vertical sum (the rounding tie and its neighbours)"""
    lows = R.pyramid(img, nlevels, scale_factor)[1]
    return [tuple(int((low == v).sum()) for v in TIE_VALUES) for low in lows[1:]]


def search_tie_seeds(limit=200):
    """the greedy search that produced TIE_SEEDS: noise frames in seed order, a frame is kept if it brings a (level, value) no earlier one had"""
    have, seeds = set(), []
    for seed in range(limit):
        new = {(l, k) for l, c in enumerate(tie_counts(tie_frame(seed))) for k in range(3) if c[k]} - have
        if new:
            have |= new
            seeds.append(seed)
        if len(have) == 21:
            break
    return seeds, have


def resize_ties():
    """[(name, image, nlevels, scale factor)]: frames on which, between them, every level >= 1 of the 1.2 pyramid has pixels whose vertical sum ends in
    exactly 0x8000 (the tie: rounds up), 0x7fff (the last value that rounds down) and 0x8001.
      * 640 x 480 noise frames TIE_SEEDS: generic weights, each value is hit about once in 65536 pixels (the frames were found by search_tie_seeds);
      * a 600 x 480 noise frame: 600 -> 500 is exactly 1.2, every fifth column and row has weight 128 and a pixel with both has the sum 16384 (a + b + c + d):
        0x8000 for every such pixel whose four sources add up to 2 mod 4.  Such sums are multiples of 16384: 0x7fff and 0x8001 cannot occur THERE;
      * a 320 x 240 noise frame for the 3-level 2.0 pyramid: every sum is 16384 (a + b + c + d), the tie is every 2 x 2 block whose sum is 2 mod 4, and a
        2.0 level cannot reach 0x7fff or 0x8001 at all."""
    out = [("noise%d" % s, tie_frame(s), 8, 1.2) for s in TIE_SEEDS]
    out.append(("exact1.2", np.random.default_rng(4600).integers(0, 256, (480, 600), dtype=np.uint8), 8, 1.2))
    out.append(("two", np.random.default_rng(4320).integers(0, 256, (240, 320), dtype=np.uint8), TWO_LEVELS, TWO_SCALE))
    return out


# the source windows of k_resize_level (afv_launch_resize / afv_resize_window_ok): 88 x 44, 96 x 48, 160 x 80 bytes for a 64 x 32 output tile
WINDOWS = [(88, 44), (96, 48), (160, 80)]


def resize_window(sw, sh, dw, dh):
    """index into WINDOWS of the instantiation afv_launch_resize picks for one level step, None if afv_resize_window_ok refuses it"""
    fx, fy = sw / dw, sh / dh
    for i, (ww, wh) in enumerate(WINDOWS):
        if 64 * fx + 8 <= ww and 32 * fy + 3 <= wh:
            return i
    return None


def level_windows(w, h, nlevels, scale_factor):
    lw, lh, _ = R.level_geometry(w, h, nlevels, scale_factor)
    return [resize_window(lw[l - 1], lh[l - 1], lw[l], lh[l]) for l in range(1, nlevels)], lw, lh


@functools.lru_cache(maxsize=None)
def ratio_limits():
    """[(w, h, scale factor, nlevels, windows per level step)]: for each of the limits 64 fx + 8 <= 88 | 96 (fx <= 1.25 | 1.375) the largest 4 : 3 frame up to
    640 wide whose pyramid at that scale factor has level steps on BOTH sides of it (the widths round: 640 -> 512 is exactly 1.25, 328 -> 262 is above);
    for the last limit (fx <= 2.375) a pyramid whose steps stay below with one as close as the search finds, and the first one found with a step beyond,
    which the library must refuse (windows holds None there).  The y limits 32 fy + 3 <= 44 | 48 | 80 (fy <= 1.28125 | 1.40625 | 2.40625) are wider than the
    x limits for every level of at least 32 px and never decide."""
    out = []
    for i, sf in ((0, 1.25), (1, 1.375)):
        for w in range(640, 200, -1):
            h = (3 * w + 2) // 4
            n = max(n for n in range(2, 9) if min(R.level_geometry(w, h, n, sf)[0][-1], R.level_geometry(w, h, n, sf)[1][-1]) >= 32)
            win = level_windows(w, h, n, sf)[0]
            if i in win and i + 1 in win and None not in win:
                out.append((w, h, sf, n, win))
                break
    best = None
    for w in range(640, 200, -1):
        h = (3 * w + 2) // 4
        win, lw, lh = level_windows(w, h, 3, 2.375)
        if None not in win and min(lw[-1], lh[-1]) >= 32:
            r = max(lw[l - 1] / lw[l] for l in (1, 2))
            if best is None or r > best[0]:
                best = (r, (w, h, 2.375, 3, win))
    out.append(best[1])
    for w in range(640, 200, -1):
        h = (3 * w + 2) // 4
        win, lw, lh = level_windows(w, h, 3, 2.375)
        if None in win and min(lw[-1], lh[-1]) >= 32:
            out.append((w, h, 2.375, 3, win))
            break
    return out


def ratio_frame(w, h):
    return np.random.default_rng(6000 + w).integers(0, 256, (h, w), dtype=np.uint8)


SCALE_FACTORS = (1.2, 1.1892, 1.25, 1.5, 2.0)
SCALE_MAX = 4095


@functools.lru_cache(maxsize=None)
def scale_pairs():
    """{(src, dst): (base, scale factor, level)}: every level step of cv::ORB - base sizes 32 .. 4095, the five scale factors, 8 levels while a level is >= 32 -
    with the smallest base size (and the first scale factor) whose level `level` is dst and whose level `level - 1` is src"""
    pairs = {}
    base = np.arange(32, SCALE_MAX + 1, dtype=np.float32)
    for sf in SCALE_FACTORS:
        sfd = float(np.float32(sf))
        sizes = [np.rint(base * (np.float32(1) / np.float32(sfd ** l))).astype(np.int64) for l in range(8)]     # level_geometry for all bases at once
        for l in range(1, 8):
            for b, s, d in zip(base.tolist(), sizes[l - 1].tolist(), sizes[l].tolist()):
                if d >= 32:
                    pairs.setdefault((s, d), (int(b), sf, l))
    return pairs


@functools.lru_cache(maxsize=None)
def scale_evaluation():
    """[(src, dst, indices where the table of src / dst differs from OpenCV's 1 / (dst / src), indices where the exact table differs)] over scale_pairs(),
    only the pairs where one of the two lists is not empty"""
    out = []
    for src, dst in sorted(scale_pairs()):
        a, b, c = R.coeff_tables_np(src, dst)
        nb = np.flatnonzero((a[0] != b[0]) | (a[1] != b[1]))
        nc = np.flatnonzero((a[0] != c[0]) | (a[1] != c[1]))
        if len(nb) or len(nc):
            out.append((src, dst, nb.tolist(), nc.tolist()))
    return out


SCALE_GPU_MAX_WIDTH = 2048


def scale_scenes():
    """[(w, h, scale factor, nlevels, src, dst)]: one black-and-white noise frame (scale_frame) per pair of scale_evaluation() whose 'src / dst' table differs
    in effect (not same_taps): w is the smallest base width whose level step nlevels - 2 -> nlevels - 1 is src -> dst in x, h = 9 / 16 w.  All of them are wider than 640 (the first is 961 -> 768 from a 1876 wide frame: the exact weight is a half
    there, dst is a multiple of 256): no smaller frame shows the difference.  Pairs that differ from the exact table only are no scenes: every implementation evaluates the table in double, the exact
    table is a fact about OpenCV, not an alternative the kernels could take."""
    prov = scale_pairs()
    out = []
    for src, dst, nb, _ in scale_evaluation():
        b, sf, l = prov[(src, dst)]
        if nb and not same_taps(src, dst):
            out.append((b, (9 * b + 8) // 16, sf, l + 1, src, dst))
    return out


def same_taps(src, dst):
    """whether the tables of 1 / (dst / src) and src / dst, where they differ, only name the same tap twice: (o, 256) is (o + 1, 0) - where the exact position
    is an integer, one order of evaluation lands just below it (all the weight on the right tap) and the other on it"""
    a, b, _ = R.coeff_tables_np(src, dst)
    ea, eb = (np.where(t[1] == 256, t[0] + 1, t[0]) * 256 + t[1] % 256 for t in (a, b))
    return bool((ea == eb).all())


def scale_frame(w, h):
    """black and white noise: the largest differences between neighbours, so that a weight that is off by 1 / 256 shows"""
    return (np.random.default_rng(5000 + w).integers(0, 2, (h, w)) * 255).astype(np.uint8)
