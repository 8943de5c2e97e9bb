"""adversarial scenes for the ORB32 selection stages (test data): isolated copies of a few motifs on a constant background

Every copy sits alone in its cell, so its FAST ring, 3 x 3 NMS neighbourhood and 9 x 9 Harris window at level 0 are the same bytes as
every other copy's: n copies of a motif are n candidates with exactly equal scores and responses.  The motifs:
  * a dot: one pixel `c` above the background.  FAST score c - 1, Harris response > 0 (grows like c^4);
  * a bar: a vertical 9 px line of value `b` whose middle pixel is `d` brighter.  Only the middle pixel is a corner (score d - 1,
    the two ends see 7 px arcs); the gradient across the line dominates the Harris window, so the response is < 0.
Which 12-bit key bin (float_key(r) >> 20, the bins of the select kernels) a motif falls in is a constant of the motif; the numbers below
were read off the CPU oracle and tests/test_oracle_scenes.py checks them there.
numpy only, no global RNG state: the same arguments give the same bytes."""
import numpy as np

W, H = 1280, 720
BG = 50
PITCH_X, PITCH_Y, MARGIN = 10, 14, 16   # a bar spans rows y-4..y+4: 14 rows leave 5 background rows between two bars

# level 0, default parameters (1000 features x 10 for cv::ORB, 8 levels, 1.2): afvo_quotas_cvorb(10000)[0]
CV_QUOTA0 = 2172

# motifs: ("dot", c) or ("bar", b, d), listed in descending response order inside each tier
POS_FILL = [("dot", 200)]                                   # bin 0xb89
POS_BIN = [("dot", 141), ("dot", 140), ("dot", 139)]        # bin 0xb79
POS_LOW = [("dot", 80)]                                     # bin 0xb5f
NEG_FILL = [("dot", 200)]                                   # any positive response is above a negative bin
NEG_BIN = [("bar", 211, 25), ("bar", 211, 30), ("bar", 212, 21)]  # bin 0x45e
NEG_LOW = [("bar", 234, 21)]                                # bin 0x458


def slots(w=W, h=H):
    """(x, y) of every motif cell centre, column by column (x, then y ascending)"""
    xs = np.arange(MARGIN, w - MARGIN + 1, PITCH_X)
    ys = np.arange(MARGIN, h - MARGIN + 1, PITCH_Y)
    gx, gy = np.meshgrid(xs, ys, indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], 1)


def draw(img, x, y, motif):
    if motif[0] == "dot":
        img[y, x] = BG + motif[1]
    else:
        _, b, d = motif
        img[y - 4:y + 5, x] = b
        img[y, x] = b + d


def place(groups, low=(), w=W, h=H, seed=0):
    """groups: [(motif, count)] spread over the left part of the frame in a fixed shuffled order; low: [(motif, count)] packed into the
    rightmost columns (a region of its own).  Returns the image and the level-0 centre of every copy with its group index
    (low groups follow the upper ones)."""
    s = slots(w, h)
    n_low = sum(c for _, c in low)
    n_up = sum(c for _, c in groups)
    assert n_low + n_up <= len(s), "scene needs %d cells, the frame has %d" % (n_low + n_up, len(s))
    up_cells = s[:len(s) - n_low]
    up_cells = up_cells[np.random.default_rng(seed).permutation(len(up_cells))[:n_up]]
    low_cells = s[len(s) - n_low:]
    img = np.full((h, w), BG, np.uint8)
    centres, tags = [], []
    for cells, gs, t0 in ((up_cells, groups, 0), (low_cells, low, len(groups))):
        i = 0
        for g, (motif, count) in enumerate(gs):
            for x, y in cells[i:i + count]:
                draw(img, int(x), int(y), motif)
                centres.append((int(x), int(y)))
                tags.append(t0 + g)
            i += count
    return img, np.array(centres, np.int32).reshape(-1, 2), np.array(tags, np.int32)


def threshold_bin(sign, n_bin, k=CV_QUOTA0, n_low=400):
    """retainBest #2 at level 0: F = k - 400 fillers above the threshold bin, n_bin keys in the one 12-bit bin that holds the k-th largest key
    (three motif variants: 300, 400, n_bin - 700 copies, so the (k - F)-th key of the bin is inside the second group of equal keys), and
    n_low keys below it in the rightmost columns.  n_bin = 1024: the exact ranking of the 1024-thread kernel; 1025: its radix passes.
    sign '-': the bin is a negative one (bins < 2048 of the 4096-bin pass)."""
    fill, binm, lowm = (POS_FILL, POS_BIN, POS_LOW) if sign == "+" else (NEG_FILL, NEG_BIN, NEG_LOW)
    F = k - 400
    groups = [(fill[0], F), (binm[0], 300), (binm[1], 400), (binm[2], n_bin - 700)]
    return place(groups, [(lowm[0], n_low)], seed=11 if sign == "+" else 12)


def tie_flood(sign, n=3200, n_low=500):
    """n > 3072 copies of one motif (the k-th largest key is one of them, so retainBest keeps all of them: more survivors than the quadtree's
    LDS holds at either thread count) and a sparser motif below them"""
    top, lowm = (POS_BIN[1], POS_LOW[0]) if sign == "+" else (NEG_BIN[0], NEG_LOW[0])
    return place([(top, n), (lowm, n_low)], seed=21 if sign == "+" else 22)


def score_threshold_ties(k2=2 * CV_QUOTA0):
    """retainBest #1 (FAST score) at level 0: 3000 fillers with higher scores (two groups: 199 and 189), 1800 with score 139 (the k2-th
    score falls inside them: ranks 3001..4800) and 600 with score 79 below.  5400 candidates, 4800 kept."""
    assert 3000 < k2 < 4800
    return place([(("dot", 200), 1500), (("dot", 190), 1500), (("dot", 140), 1800)], [(("dot", 80), 600)], seed=31)


# ---- FAST: ring pixels exactly on the threshold ----
RING = list(zip([0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1],
                [3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3]))  # (dx, dy), clockwise from (0, 3): OpenCV's makeOffsets
EDGE_CELL = 12    # a 9 x 9 patch of the centre value per motif (radius 4: the ring of every NMS neighbour of the centre) + 3 px of background
EDGE_BG = 128


def _edge_centres(t):
    lo = [0, 1, t // 2, t - 1, t]
    hi = [255 - t, 256 - t, 255 - t // 2, 254, 255]
    return sorted({v for v in lo + [100, 127, 128] + hi if 0 <= v <= 255})


def fast_edges(t, w=640, h=480):
    """one centre per motif: a 9 x 9 patch of value v, an arc of L ring pixels at v + s*d (s = +1 brighter, -1 darker, d in {t, t + 1},
    L in {8, 9, 10}, starting at a ring index that walks round the ring so that arcs wrap past index 15), the rest of the ring at v.
    A FAST-9 corner at threshold t iff d = t + 1 and L >= 9.  Centres v in 0..t, mid-range, 255 - t..255.  Then maximum-contrast motifs
    (255 on 0 and 0 on 255, full ring and 9-arc) and pairs of horizontally adjacent corners: equal (NMS keeps neither) and one level apart.
    Returns the image and a list of (x, y, kind) where kind is 'corner', 'flat' (designed non-corner) or 'tie' (a corner that NMS drops)."""
    img = np.full((h, w), EDGE_BG, np.uint8)
    cells = [(x, y) for y in range(8, h - 8, EDGE_CELL) for x in range(8, w - 8, EDGE_CELL)]
    out = []
    it = iter(cells)

    def patch(v):
        x, y = next(it)
        img[y - 4:y + 5, x - 4:x + 5] = v
        return x, y

    start = 0
    for v in _edge_centres(t):
        for s in (1, -1):
            for d in (t, t + 1):
                if not 0 <= v + s * d <= 255:
                    continue
                for L in (8, 9, 10):
                    x, y = patch(v)
                    for j in range(L):
                        dx, dy = RING[(start + j) % 16]
                        img[y + dy, x + dx] = v + s * d
                    start = (start + 5) % 16
                    out.append((x, y, "corner" if d == t + 1 and L >= 9 else "flat"))
    for v, c in ((0, 255), (255, 0)):
        x, y = patch(v)
        img[y, x] = c
        out.append((x, y, "corner"))
        x, y = patch(c)
        for j in range(9):
            dx, dy = RING[(start + j) % 16]
            img[y + dy, x + dx] = v
        start = (start + 7) % 16
        out.append((x, y, "corner"))
    # adjacent pairs: a bright pixel pair on a patch of value p, the left one a, the right one b
    p = 0 if t > 200 else 60
    for a, b in ((255, 255), (254, 255), (p + t + 40, p + t + 40), (p + t + 40, p + t + 41)):
        if max(a, b) > 255 or min(a, b) - p <= t:
            continue
        x, y = patch(p)
        img[y, x] = a
        img[y, x + 1] = b
        if a == b:
            out += [(x, y, "tie"), (x + 1, y, "tie")]
        else:
            out.append((x + 1, y, "corner"))
    return img, out
