"""the CPU oracle against the plain restatement tests/_detect_ref.py on the scenes of tests/_detect_scenes.py (pyramid levels, FAST score planes, FAST + NMS lists
and the candidate sets of the extraction trace: every one an equality), and the proof that each scene reaches the rule it was built for, from the
restatement's own account of what decided every designed pixel.  With a rule's wrong alternative (a swapped ring table, '>=' against one NMS neighbour, a
score on row 2 / column w - 3, + 32767, the scale as src / dst) the restatement's result on the scene built for that rule changes.  Without these checks a
change to a generator or to the oracle could leave tests/test_gpu_detect_scenes.py green without testing anything."""
import itertools

import numpy as np
import pytest

import _detect_ref as R
import _detect_scenes as S


def _params(oracle, nlevels, sf, t):
    return oracle.default_params(nlevels=nlevels, scale_factor=sf, fast_threshold=t)


def _hold(oracle, img, what, nlevels=8, sf=1.2, thresholds=(20,), fast=True):
    """the oracle's pyramid, score planes, FAST lists and trace candidates on `img` are the restatement's; returns the restatement's (levels, low-16 planes)"""
    levels, lows, _ = R.pyramid(img, nlevels, sf)
    if not fast:      # the pyramid alone (frames too large for the Python score planes)
        for l in range(1, nlevels):
            assert np.array_equal(oracle.resize_linear_exact(levels[l - 1], levels[l].shape[1], levels[l].shape[0]), levels[l]), (what, "resize_linear_exact", l)
        return levels, lows
    strength = [R.fast_strength_map(lv) for lv in levels]
    if nlevels > 1:
        assert np.array_equal(oracle.resize_linear_exact(img, levels[1].shape[1], levels[1].shape[0]), levels[1]), (what, "resize_linear_exact")
    for i, t in enumerate(thresholds):
        tr = oracle.orb_extract_trace(img, _params(oracle, nlevels, sf, t), cap=4000)[2]
        want = []
        for l, lv in enumerate(levels):
            if i == 0:
                assert np.array_equal(tr["level"][l], lv), (what, "pyramid level", l, np.argwhere(tr["level"][l] != lv)[:4] if tr["level"][l].shape == lv.shape else lv.shape)
            assert np.array_equal(oracle.fast_score_map(lv, t), R.fast_score_map(lv, t, strength=strength[l])), (what, "fast_score_map", l, t)
            kept = R.fast_nms(lv, t, strength=strength[l])
            x, y, s = oracle.fast9_16(lv, t)
            assert list(zip(x.tolist(), y.tolist(), s.tolist())) == kept, (what, "fast9_16", l, t)
            want += [(l, y, x, s) for x, y, s in kept]
        c = tr["cand"]
        assert sorted(zip(c["level"].tolist(), c["y"].tolist(), c["x"].tolist(), c["fast_score"].tolist())) == sorted(want), (what, "candidates", t)
    return levels, lows


# ---------------------------------------------------------------- tables ----------------------------------------------------------------
def test_level_geometry(oracle):
    """afvo_level_geometry is cv::ORB's rule, for every scale factor of the scenes"""
    for sf in S.SCALE_FACTORS + (1.375, 2.375, 1.0905):
        for w in itertools.chain(range(32, 700), range(700, 4096, 37)):
            h = (3 * w + 2) // 4
            n = 8 if w >= 300 else 3
            lw, lh, ls = R.level_geometry(w, h, n, sf)
            ow, oh, os_ = oracle.level_geometry(w, h, n, sf)
            assert lw == ow.tolist() and lh == oh.tolist() and [float(v) for v in ls] == os_.tolist(), (w, h, sf)


def test_coefficient_tables_three_ways():
    """the vectorised tables of the search over every (src, dst) pair are the plain loops: IEEE double in OpenCV's order, as src / dst, and exact rationals"""
    ev = S.scale_evaluation()
    pairs = [(e[0], e[1]) for e in ev[:40]] + [(640, 533), (600, 500), (640, 320), (33, 32), (640, 269), (1280, 1067)]
    for src, dst in pairs:
        a, b, c = R.coeff_tables_np(src, dst)
        for got, want in ((a, R.resize_coeffs(src, dst)), (b, R.resize_coeffs(src, dst, "src/dst")), (c, R.resize_coeffs_exact(src, dst))):
            assert got[0].tolist() == want[0] and got[1].tolist() == want[1], (src, dst)
    nb, nc = R.coeff_differences(44, 36)
    assert (44, 36, nb, nc) == next(e for e in ev if e[:2] == (44, 36)) and nb


def test_resize_and_score_planes_are_the_scalar_definitions():
    """the whole-image forms of the restatement against its one-pixel forms in Python integers, on a small noise frame"""
    img = np.random.default_rng(7).integers(0, 256, (41, 53), dtype=np.uint8)
    dw, dh = 44, 34
    dst, low, _ = R.resize_linear_exact(img, dw, dh)
    xo, xc = R.resize_coeffs(53, dw)
    yo, yc = R.resize_coeffs(41, dh)
    for y in range(dh):
        for x in range(dw):
            assert R.resize_pixel(img, xo, xc, yo, yc, x, y) == (dst[y, x], low[y, x])
    img[10:30, 10:40] //= 8      # a flatter region: more corners
    st = R.fast_strength_map(img)
    for y in range(3, 38):
        for x in range(3, 50):
            assert R.fast_score(img, x, y) == st[y, x] or (st[y, x] == -1 and R.fast_score(img, x, y) < 0)
    assert (st[:3] == -1).all() and (st[:, -3:] == -1).all() and R.fast_nms(img[:6], 1) == [] and R.fast_nms(img[:, :6], 1) == []


# ---------------------------------------------------------------- the oracle's score on an exhaustive small domain ----------------------------------------------------------------
def _rings_to_image(rings, v):
    """one 7 x 7 cell per ring, side by side: the centre of cell i is (7 i + 3, 3)"""
    n = len(rings)
    img = np.full((7, 7 * n), v, np.uint8)
    for k, (dx, dy) in enumerate(R.RING):
        img[3 + dy, 3 + dx + 7 * np.arange(n)] = rings[:, k]
    return img


def _ring_strength(rings, v):
    """M - 1 of R.fast_score_info for an [n, 16] array of rings around the centre value v: the same loops over polarity, window and position"""
    d = rings.astype(np.int16) - np.int16(v)
    best = np.full(len(rings), -256, np.int16)
    for s in (1, -1):
        for w in range(16):
            m = s * d[:, w]
            for j in range(1, 9):
                m = np.minimum(m, s * d[:, (w + j) % 16])
            best = np.maximum(best, m)
    return np.maximum(best, 0) - 1


@pytest.mark.parametrize("v,t,rest", [(100, 20, 0), (1, 2, 0), (100, 20, 1), (254, 3, -1)])
def test_oracle_score_on_every_ring_of_a_small_domain(oracle, v, t, rest):
    """every ring that takes the values v - t - 1, v - t, v, v + t, v + t + 1 (clipped to 0 .. 255) on 5 of its pixels, in every choice of the 5, the other 11
    at v (rest = 0: no 9-window holds fewer than 4 pixels at v, the oracle's shortcuts must not invent a corner) or all beyond the threshold (rest = +-1:
    at v +- (t + 1), so that whether a 9-arc is left depends on the 5): fast_corner_score steps by 2 and leaves its loops early, the restatement does neither"""
    vals = np.clip(np.array([v - t - 1, v - t, v, v + t, v + t + 1]), 0, 255).astype(np.uint8)
    combos = vals[np.array(list(itertools.product(range(5), repeat=5)), np.int64)]            # 3125 x 5
    sets = list(itertools.combinations(range(16), 5))
    assert len(sets) == 4368
    for i in range(0, len(sets), 48):
        chunk = sets[i:i + 48]
        rings = np.full((len(chunk), len(combos), 16), int(np.clip(v + rest * (t + 1), 0, 255)), np.uint8)
        for k, pos in enumerate(chunk):
            rings[k][:, pos] = combos
        rings = rings.reshape(-1, 16)
        want = _ring_strength(rings, v)
        got = oracle.fast_score_map(_rings_to_image(rings, v), t)[3, 3::7]
        bad = np.flatnonzero(got != np.where(want >= t, np.maximum(want, 0), 0))
        assert len(bad) == 0, (v, t, rest, rings[bad[0]].tolist(), int(got[bad[0]]), int(want[bad[0]]))
        assert rest != 0 or not got.any()


def test_oracle_score_on_random_rings(oracle):
    rng = np.random.default_rng(11)
    for t in S.THRESHOLDS + (0, 100):
        rings = rng.integers(0, 256, (40000, 16), dtype=np.uint8)
        rings[:20000] = np.where(rng.random((20000, 16)) < 0.7, rng.integers(0, 2, (20000, 1)) * 255, rings[:20000])   # long arcs at the ends of the range
        for v in (0, 1, 127, 254, 255):
            want = _ring_strength(rings, v)
            got = oracle.fast_score_map(_rings_to_image(rings, v), t)[3, 3::7]
            assert np.array_equal(got, np.where(want >= t, np.maximum(want, 0), 0)), (v, t)
    img = _rings_to_image(rings[:500], 9)
    assert np.array_equal(R.fast_strength_map(img)[3, 3::7], _ring_strength(rings[:500], 9))


# ---------------------------------------------------------------- FAST score and tile position ----------------------------------------------------------------
def _prove_corners(img, facts, t, what):
    """every designed corner is kept with its designed score and polarity, decided by the designed window and pixel"""
    kept = {(x, y): s for x, y, s in R.fast_nms(img, t)}
    for f in facts:
        at = (f["x"], f["y"])
        assert kept.get(at) == f["score"], (what, f, kept.get(at))
        score, pol, wins, poss = R.fast_score_info(img, *at)
        assert (score, pol) == (f["score"], f["pol"]), (what, f)
        if "windows" in f:
            assert wins == f["windows"] and (f["positions"] is None or poss == f["positions"]), (what, f, wins, poss)


def test_tile_sweep(oracle):
    seen = {1: set(), -1: set()}
    for i in range(S.SWEEP_FRAMES):
        img, facts = S.tile_sweep(i)
        _hold(oracle, img, "tile_sweep/%d" % i, thresholds=S.THRESHOLDS)
        _prove_corners(img, facts, 20, "tile_sweep/%d" % i)
        pts = np.array([(f["x"], f["y"]) for f in facts])
        d = np.abs(pts[:, None, :] - pts[None, :, :]).max(2)
        assert d[d > 0].min() >= 12
        for f in facts:
            seen[f["pol"]].add((f["x"] % 64, f["y"] % 32))
        assert {f["start"] for f in facts} == set(range(16)) and {f["length"] for f in facts} == set(range(9, 17))
    assert len(seen[1]) == 2048 and len(seen[-1]) == 2048


@pytest.mark.parametrize("t", [1, 7, 20])
def test_score_network(oracle, t):
    frames = S.score_network(t)
    facts = [f for _, fs in frames for f in fs]
    for i, (img, fs) in enumerate(frames):
        _hold(oracle, img, "score_network(%d)/%d" % (t, i), thresholds=S.THRESHOLDS)
        _prove_corners(img, fs, t, "score_network(%d)/%d" % (t, i))
        swapped = list(R.RING)
        swapped[5], swapped[6] = swapped[6], swapped[5]
        assert R.fast_nms(img, t, ring=swapped) != R.fast_nms(img, t), "two swapped ring entries go unnoticed"
    nine = {(f["pol"], f["windows"][0], f["positions"][0][0]) for f in facts if f["length"] == 9 and f["positions"] and f["q"] is None}
    assert nine >= set(itertools.product((1, -1), range(16), range(9)))
    for L in range(10, 17):
        for s in (1, -1):
            assert {f["q"] for f in facts if f["length"] == L and f["pol"] == s and f["q"] is not None} == set(range(16 if L == 16 else L - 8)), (L, s)
    assert {f["score"] for f in facts} >= {t, 254}
    centres = {int(frames[0][0][f["y"], f["x"]]) for f in facts} if len(frames) == 1 else None
    assert centres is None or centres >= {0, 1, t - 1, t, 255 - t, 256 - t, 254, 255}
    assert all(len(np.unique(img)) > 200 and img.min() == 0 and img.max() == 255 for img, _ in frames)


@pytest.mark.parametrize("t", [1, 7, 20])
def test_pretest_traps(oracle, t):
    kinds = set()
    for i, (img, facts) in enumerate(S.pretest_traps(t)):
        what = "pretest_traps(%d)/%d" % (t, i)
        _hold(oracle, img, what, thresholds=S.THRESHOLDS)
        kept = {(x, y): s for x, y, s in R.fast_nms(img, t)}
        for f in facts:
            at = (f["x"], f["y"])
            pre, arcs = R.pretest(img, *at, t), R.longest_arc(img, *at, t)
            if f["kind"] in ("arc8", "arc8+6"):
                assert pre[f["pol"] < 0] and arcs[f["pol"] < 0] == 8 and max(arcs) == 8 and at not in kept and R.fast_score(img, *at) < t, (what, f)
            elif f["kind"] == "both_none":
                assert pre == (True, True) and max(arcs) < 9 and at not in kept and R.fast_score(img, *at) < t, (what, f)
            else:
                assert pre == (True, True) and sorted(arcs) == [7, 9] and kept.get(at) == f["score"] and R.fast_score_info(img, *at)[1] == f["pol"], (what, f)
            kinds.add((f["kind"], f["pol"]))
    assert kinds == {(k, s) for k in ("arc8", "arc8+6", "both_one") for s in (1, -1)} | {("both_none", 0)}


# ---------------------------------------------------------------- NMS and the FAST border ----------------------------------------------------------------
def _prove_nms(img, facts, t, what):
    dropped = {}
    kept = {(x, y): s for x, y, s in R.fast_nms(img, t, dropped=dropped)}
    for f in facts:
        for x, y, s in f["kept"]:
            assert kept.get((x, y)) == s, (what, f)
        for x, y, why in f["dropped"]:
            assert (x, y) not in kept and why in {r for _, _, r in dropped[(x, y)]}, (what, f, dropped.get((x, y)))
        pts = [(x, y) for x, y, _ in f["kept"] + f["dropped"]]
        rx, ry = {x % 64 for x, _ in pts}, {y % 32 for _, y in pts}
        if f["kind"] in ("equal", "above"):
            dx, dy = f["dir"]
            seam_x, seam_y = rx == {63, 0}, ry == {31, 0}
            want = {"inside": (False, False), "vseam": (dx != 0, False), "hseam": (False, dy != 0), "corner": (dx != 0, dy != 0)}[f["place"]]
            assert (seam_x, seam_y) == want and (f["place"] == "inside" or rx & {63, 0} or ry & {31, 0}), (what, f)
            assert len(f["kept"]) == (f["kind"] == "above")
        else:
            assert len(f["kept"]) == (f["kind"] == "chain") and (f["place"] != "corner" or (rx & {63, 0} and ry & {31, 0})), (what, f)
        if f["kind"] == "chain":          # 1 < 2 < 3: the lowest is beaten by the middle one only, which is itself dropped
            lowest = min(f["dropped"], key=lambda p: img[p[1], p[0]])
            beaters = [(lowest[0] + dx, lowest[1] + dy) for dx, dy, _ in dropped[lowest[:2]]]
            assert len(beaters) == (2 if f["dir"] == "L" else 1) and any(b not in kept for b in beaters), (what, f)
    for n in R.NEIGHBOURS:                # '>=' against any one neighbour keeps one pixel of an equal pair in that direction
        assert R.fast_nms(img, t, ge_neighbour=n) != R.fast_nms(img, t) or not any(f["kind"] == "equal" and f["dir"] in (n, (-n[0], -n[1])) for f in facts), (what, n)


def test_nms_pairs(oracle):
    facts = []
    for i, (img, fs) in enumerate(S.nms_pairs()):
        _hold(oracle, img, "nms_pairs/%d" % i, thresholds=S.THRESHOLDS)
        _prove_nms(img, fs, 20, "nms_pairs/%d" % i)
        facts += fs
    want = {(k, p, d) for d in S.DIRS for p, _, _ in S._nms_anchors(*d) for k in ("equal", "above")}
    assert {(f["kind"], f["place"], f["dir"]) for f in facts if f["kind"] in ("equal", "above")} == want and len(want) == 64
    for n in R.NEIGHBOURS:
        assert any(R.fast_nms(img, 20, ge_neighbour=n) != R.fast_nms(img, 20) for img, _ in S.nms_pairs()), n
    for kind, names in (("chain", {"h", "v", "d", "a", "L", "h-", "v-"}), ("block2", {None}), ("block3", {None})):
        for place in ("inside", "corner", "vseam", "hseam"):
            assert {f["dir"] for f in facts if f["kind"] == kind and f["place"] == place} == names


def _prove_border(img, facts, t, what):
    kept = {(x, y): s for x, y, s in R.fast_nms(img, t)}
    h, w = img.shape
    for x, y, s in facts["kept"]:
        assert kept.get((x, y)) == s and (x in (3, w - 4) or y in (3, h - 4)), (what, x, y)
    for x, y in facts["nothing"]:
        assert (x, y) not in kept, (what, x, y)
    assert len(kept) == len(facts["kept"]) and facts["lines"] == {(s, q) for s in ("top", "bottom", "left", "right") for q in (2, 3)}, what
    wrong = R.fast_nms(img, t, border=2)
    assert wrong != R.fast_nms(img, t), (what, "a score on line 2 goes unnoticed")


@pytest.mark.parametrize("size", S.BORDER_SIZES)
def test_border(oracle, size):
    w, h = size
    assert min(R.level_geometry(w, h, S.BORDER_LEVELS)[1]) >= 32
    for v in range(S.BORDER_VARIANTS):
        img, facts = S.border(w, h, v)
        _hold(oracle, img, "border %s/%d" % (size, v), nlevels=S.BORDER_LEVELS, thresholds=S.THRESHOLDS)
        _prove_border(img, facts, 20, "border %s/%d" % (size, v))
    assert {(w - 1) % 64 + 1 for w, _ in S.BORDER_SIZES} >= {1, 2, 3, 4, 63, 64} and {(h - 1) % 32 + 1 for _, h in S.BORDER_SIZES} >= {1, 2, 3, 4, 31, 32}


# ---------------------------------------------------------------- levels >= 1 ----------------------------------------------------------------
@pytest.mark.parametrize("family", ["score_network", "nms_pairs", "border"])
def test_two_to_one(oracle, family):
    """level l of the 2.0 pyramid of two_to_one(D) is D replicated 2^(2 - l) times - on the oracle's levels - and D's designed facts hold at level 2"""
    n = total = 0
    for name, (D, facts, kind) in S.designed_images().items():
        if kind != family:
            continue
        n += 1
        img = S.two_to_one(D)
        assert img.shape[0] <= 480 and img.shape[1] <= 640
        tr = oracle.orb_extract_trace(img, _params(oracle, S.TWO_LEVELS, S.TWO_SCALE, 20))[2]
        for l in range(3):
            k = 4 >> l
            assert np.array_equal(tr["level"][l], np.repeat(np.repeat(D, k, 0), k, 1)), (name, l)
        _hold(oracle, img, name, nlevels=S.TWO_LEVELS, sf=S.TWO_SCALE, thresholds=(7, 20))
        {"score_network": _prove_corners, "nms_pairs": _prove_nms, "border": _prove_border}[kind](D, facts, 20, name)
        got = {(c["x"], c["y"], c["fast_score"]) for c in tr["cand"][tr["cand"]["level"] == 2]}
        designed = facts["kept"] if kind == "border" else [k for f in facts for k in f["kept"]] if kind == "nms_pairs" else [(f["x"], f["y"], f["score"]) for f in facts]
        assert set(designed) <= got, name
        total += len(designed)
    assert n >= 4 and total > 20


# ---------------------------------------------------------------- pyramid ----------------------------------------------------------------
@pytest.mark.parametrize("size", S.RESIZE_SIZES)
def test_resize_extremes(oracle, size):
    w, h = size
    for name, img in S.resize_extremes(w, h).items():
        levels, lows = _hold(oracle, img, "resize_extremes %s %s" % (size, name))
        if name in ("ones", "zeros"):
            assert all((lv == img[0, 0]).all() for lv in levels)
        if name == "ones":
            assert R.pyramid(img)[2] == 65280
        if name == "checker":
            assert len(np.unique(levels[1])) > 2
    lw = R.level_geometry(w, h)[0]
    assert size != (600, 480) or (lw[1] == 500 and R.resize_coeffs(600, 500)[1][:5] == [26, 77, 128, 179, 230])
    xo, xc = R.resize_coeffs(lw[0], lw[1])
    assert (xo[0], xo[-1] + 1) == (0, lw[0] - 1) and xc[0] > 0 and xc[-1] > 0      # first and last column: offset 0, and the right tap of the last one is the last source column


def test_right_tap_clamp_never_decides():
    """a right / lower tap is clamped to the last column / row only where its weight is 0 (getCoeffs gives (src - 1, 0) there), and at the level steps of a
    pyramid (dst < src) not even that happens: the last offset is at most src - 2.  Dropping the clamp cannot change a result; it guards the read alone."""
    for src, dst in S.scale_pairs():
        a = R.coeff_tables_np(src, dst)[0]
        assert a[0].max() <= src - 2 and a[0].min() == 0


def test_resize_ties(oracle):
    seen = set()
    for name, img, nlevels, sf in S.resize_ties():
        levels, lows = _hold(oracle, img, "resize_ties " + name, nlevels=nlevels, sf=sf)
        counts = [tuple(int((low == v).sum()) for v in S.TIE_VALUES) for low in lows[1:]]
        assert counts == S.tie_counts(img, nlevels, sf)
        wrong = R.pyramid(img, nlevels, sf, half=32767)[0]
        for l in range(1, nlevels):
            if counts[l - 1][1] and np.array_equal(levels[l - 1], wrong[l - 1]):     # same source level: exactly the ties round the other way
                assert int((wrong[l] != levels[l]).sum()) == counts[l - 1][1], (name, l)
        if name == "two":
            for l in (1, 2):
                s = levels[l - 1].astype(np.int64)
                blocks = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
                assert counts[l - 1] == (0, int((blocks % 4 == 2).sum()), 0) and counts[l - 1][1] > 100 and (lows[l] % 16384 == 0).all(), (name, l)
        elif name == "exact1.2":
            cols = np.flatnonzero(np.array(R.resize_coeffs(600, 500)[1]) == 128)
            rows = np.flatnonzero(np.array(R.resize_coeffs(480, 400)[1]) == 128)
            sub = lows[1][np.ix_(rows, cols)]
            assert len(cols) == 100 and len(rows) == 80 and (sub % 16384 == 0).all() and int((sub == 0x8000).sum()) > 1000
        else:
            seen |= {(l, k) for l, c in enumerate(counts) for k in range(3) if c[k]}
    assert seen == set(itertools.product(range(7), range(3))), "every level >= 1 of the 1.2 pyramid reaches 0x7fff, 0x8000 and 0x8001"
    assert S.search_tie_seeds(max(S.TIE_SEEDS) + 1)[0] == list(S.TIE_SEEDS)


def test_ratio_limits(oracle):
    """level steps on both sides of each window limit of afv_launch_resize; what afv_resize_window_ok says about each is recorded here, tests/test_gpu_detect_scenes.py
    asserts what the library does with it"""
    lim = S.ratio_limits()
    assert [(t[0], t[1], t[2], t[3]) for t in lim] == [(640, 480, 1.25, 8), (640, 480, 1.375, 8), (631, 473, 2.375, 3), (640, 480, 2.375, 3)]
    assert set(lim[0][4]) == {0, 1} and set(lim[1][4]) == {1, 2} and set(lim[2][4]) == {2} and None in lim[3][4]
    for (w, h, sf, n, win), limit in zip(lim, (1.25, 1.375, 2.375, 2.375)):
        lw, lh, _ = R.level_geometry(w, h, n, sf)
        fx = [lw[l - 1] / lw[l] for l in range(1, n)]
        fy = [lh[l - 1] / lh[l] for l in range(1, n)]
        assert min(abs(f - limit) for f in fx) < 0.005 and min(lw[-1], lh[-1]) >= 32
        assert all((64 * a + 8 <= S.WINDOWS[i][0]) == (32 * b + 3 <= S.WINDOWS[i][1]) or 64 * a + 8 > S.WINDOWS[i][0] for a, b in zip(fx, fy) for i in range(3)), "a y limit decides"
        if None not in win:
            assert any(f <= limit for f in fx) and (limit == 2.375 or any(f > limit for f in fx))
            _hold(oracle, S.ratio_frame(w, h), "ratio_limits %s" % ((w, h, sf),), nlevels=n, sf=sf)
        else:
            assert any(f > limit for f in fx)


def test_scale_evaluation(oracle):
    """recorded facts of the search over every level step up to 4095 at 1.2, 1.1892, 1.25, 1.5, 2.0: the scale OpenCV uses, 1 / (dst / src) in double, gives
    another coefficient table than src / dst for 975 of the 27869 steps and another than exact rationals for 1089.  In 966 of the 975 the two tables name the same
    taps ((o, 256) and (o + 1, 0): the exact position is an integer); 9 steps, the narrowest 961 -> 768, really differ (the exact weight is a half).  On a frame
    of each of the 9 the restatement with src / dst produces another last level, and the oracle agrees with OpenCV's order."""
    ev = S.scale_evaluation()
    assert (len(S.scale_pairs()), len(ev), sum(1 for e in ev if e[2]), sum(1 for e in ev if e[3])) == (27869, 1355, 975, 1089)
    assert sum(1 for e in ev if e[2] and S.same_taps(e[0], e[1])) == 966
    scenes = S.scale_scenes()
    assert [(s[4], s[5]) for s in scenes] == [(961, 768), (1151, 768), (1523, 1280), (1535, 768), (1601, 1280), (2689, 1792), (3349, 2816), (3583, 1792), (3993, 3328)]
    assert sum(1 for s in scenes if s[0] <= S.SCALE_GPU_MAX_WIDTH) == 3
    for w, h, sf, n, src, dst in scenes:
        img = S.scale_frame(w, h)
        levels, _ = _hold(oracle, img, "scale_evaluation %s" % ((w, h, sf, n),), nlevels=n, sf=sf, fast=w <= S.SCALE_GPU_MAX_WIDTH)
        assert levels[-1].shape[1] == dst and levels[-2].shape[1] == src
        assert not np.array_equal(R.resize_linear_exact(levels[-2], dst, levels[-1].shape[0], scale_as="src/dst")[0], levels[-1]), (w, h, sf, n)
