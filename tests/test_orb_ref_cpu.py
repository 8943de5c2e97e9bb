"""the CPU oracle against the plain restatement tests/_orb_ref.py on the scenes of tests/_desc_scenes.py (angles, Harris bits, blurred planes, descriptors:
every one an equality of bits), and the proof that each scene reaches the rule it was built for: with the rule's wrong alternative the restatement's
result on that scene changes.  Without these checks a change to a generator or to the oracle could leave tests/test_gpu_desc_scenes.py green without
testing anything.  mpmath gives the cos / sin of the restatement (exact value -> double -> float)."""
import functools

import numpy as np
import pytest

import _desc_scenes as D
import _orb_ref as R

f32 = np.float32
COMPUTE = ["ties", "comparisons", "rotation_noise", "rotation_checker", "apron"]


def bits(v):
    return np.asarray(v, f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _trace_of(name):
    import oracle
    return oracle.orb_extract_trace(D.detect_scene(name)[0])


def _level_coords(kps, tr):
    """level coordinates of the oracle's keypoints, through the candidates that survived retainBest (pt = level coordinate * scale in float32)"""
    c = tr["cand"][tr["keep2"]]
    lut = {}
    for e in c:
        s = f32(tr["lscale"][e["level"]])
        lut[(int(e["level"]), float(f32(e["x"]) * s), float(f32(e["y"]) * s))] = e
    return [lut[(int(k["octave"]), float(k["x"]), float(k["y"]))] for k in kps]


def _compute_scene(oracle, name):
    if name == "ties":
        return D.ties()[:2]
    if name == "comparisons":
        return D.comparisons()[:2]
    if name.startswith("rotation"):
        return D.rotation(name[9:])
    lw, lh, ls = oracle.level_geometry(D.APRON_W, D.APRON_H)
    return D.apron(ls.tolist(), lw.tolist(), lh.tolist())


def _ref_compute(oracle, img, kps, rules=R.RIGHT, only=None):
    """the restatement of afv_orb_compute on the oracle's pyramid levels (the resize is not restated here): centre = cvRound(pt * (1 / scale))"""
    _, _, tr = oracle.orb_extract_trace(img)
    blurred = {}
    out = np.zeros((len(kps), 32), np.uint8)
    for i in (range(len(kps)) if only is None else only):
        k = kps[i]
        l = int(k["octave"])
        if l not in blurred:
            blurred[l] = R.blur(tr["level"][l], rules)
        inv = f32(1) / f32(tr["lscale"][l])
        cx, cy = int(np.rint(f32(k["x"] * inv))), int(np.rint(f32(k["y"] * inv)))
        out[i] = R.descriptor(tr["level"][l], blurred[l], cx, cy, k["angle"], rules)
    return out


# ---------------------------------------------------------------- oracle == restatement ----------------------------------------------------------------
def test_tables(oracle):
    assert R.UMAX == oracle.umax().tolist()
    assert R.TAPS == oracle.gauss7_taps().tolist() and sum(R.TAPS) == 257
    assert np.array_equal(R.PATTERN.ravel(), oracle.brief_pattern())


@pytest.mark.parametrize("name", list(D.DETECT))
def test_oracle_equals_restatement_on_detect_scene(oracle, name):
    img, centres, kinds = D.detect_scene(name)
    assert img.shape[0] <= 240 and img.shape[1] <= 320
    kps, desc, tr = _trace_of(name)
    blurred = [R.blur(lv) for lv in tr["level"]]
    for l, b in enumerate(blurred):
        assert np.array_equal(b, tr["blurred"][l]), ("blurred plane", l)
    k0 = kps[kps["octave"] == 0]
    assert set(centres) <= {(int(x), int(y)) for x, y in zip(k0["x"], k0["y"])}, "every motif must be a level-0 keypoint"
    assert all(D.interior(x, y) for x, y in centres) and len(D.alignments(centres)) == 8, "motifs on the aligned path, at every a = (x - 21) & 3 with both parities of y"
    for k, d, e in zip(kps, desc, _level_coords(kps, tr)):
        l, x, y = int(e["level"]), int(e["x"]), int(e["y"])
        lv = tr["level"][l]
        a, b, c = R.harris_sums(lv, x, y)
        assert (a, b, c) == (e["ha"], e["hb"], e["hc"]), (l, x, y)
        want = R.harris_response(a, b, c)
        assert bits(want) == bits(e["response"]) == bits(k["response"]) == bits(oracle.harris_response(a, b, c)), (l, x, y, a, b, c)
        m10, m01 = R.moments(lv, x, y)
        ang = R.fast_atan2(f32(m01), f32(m10))
        assert bits(ang) == bits(k["angle"]) == bits(oracle.fast_atan2(f32(m01), f32(m10))), (l, x, y, m10, m01)
        assert np.array_equal(R.descriptor(lv, blurred[l], x, y, k["angle"]), d), (l, x, y)


@pytest.mark.parametrize("name", COMPUTE)
def test_oracle_equals_restatement_on_compute_scene(oracle, name):
    img, kps = _compute_scene(oracle, name)
    assert img.shape[0] <= 240 and img.shape[1] <= 320
    want = _ref_compute(oracle, img, kps)
    got = oracle.orb_compute(img, kps)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(1))[:8]


def test_oracle_sincos_is_the_double_then_float_one_at_every_scene_angle(oracle):
    """the oracle's explicit Cody-Waite routine is the correctly rounded float 'except for ~1e-9 of inputs': none of the angles the scenes use is one"""
    for a in D.rotation_angles():
        c, s = R.sincos(a)
        oc, os_ = oracle.sincos_deg(a)
        assert bits(c) == bits(oc) and bits(s) == bits(os_), a


# ---------------------------------------------------------------- every scene reaches its rule ----------------------------------------------------------------
def _angles(name, rules):
    img, centres, kinds = D.detect_scene(name)
    return np.array([R.ic_angle(img, x, y, rules) for x, y in centres], f32), np.array(kinds)


@pytest.mark.parametrize("part", [0, 1, 2])
def test_disc_edge_scene_bites_on_the_disc_radius(part):
    name = "disc_edge%d" % part
    right, kinds = _angles(name, R.RIGHT)
    wide, _ = _angles(name, R.RIGHT._replace(disc=1))
    narrow, _ = _angles(name, R.RIGHT._replace(disc=-1))
    ins, outs = kinds == "inside", kinds == "outside"
    n = int(ins.sum())
    assert n == outs.sum() == len(range(part, 62, 3))
    assert np.all(bits(right[outs]) == 0) and (right[ins] != 0).sum() >= n - 1
    # a probe on the last column of its row counts, one column further out it does not: umax + 1 picks up every outside probe, umax - 1 loses every
    # inside one (a probe at v = 0, u = +umax has angle 0 either way: one motif of the 62)
    assert (bits(wide[outs]) != bits(right[outs])).sum() >= n - 1 and np.array_equal(bits(wide[ins]), bits(right[ins]))
    assert (bits(narrow[ins]) != bits(right[ins])).sum() >= n - 1 and np.array_equal(bits(narrow[outs]), bits(right[outs]))


def test_disc_edge_scenes_cover_every_row_and_side():
    seen = set()
    for part in (0, 1, 2):
        img, centres, kinds = D.detect_scene("disc_edge%d" % part)
        for (x, y), k in zip(centres, kinds):
            yy, xx = np.nonzero(img[y - 15:y + 16, x - 16:x + 17] == D.BG + D.PROBE)
            assert len(xx) == 1
            u, v = int(xx[0]) - 16, int(yy[0]) - 15
            assert abs(u) == R.UMAX[abs(v)] + (k == "outside")
            seen.add((v, u > 0, k))
    assert len(seen) == 31 * 2 * 2


def test_atan_scene_bites_on_the_branch_test():
    right, kinds = _angles("atan", R.RIGHT)
    wrong, _ = _angles("atan", R.RIGHT._replace(atan_branch=">"))
    img, centres, _ = D.detect_scene("atan")
    for kind in ("diag++", "diag-+", "diag--", "diag+-", "zero"):   # |m01| == |m10|: the other branch gives other float bits (90 for empty moments)
        m = kinds == kind
        assert m.sum() >= 2 and np.all(bits(right[m]) != bits(wrong[m])), kind
        for (x, y) in np.array(centres)[m]:
            m10, m01 = R.moments(img, int(x), int(y))
            assert abs(m10) == abs(m01) and (m10 != 0) == (kind != "zero")
    for kind, sign in (("axis+x", (1, 0)), ("axis-x", (-1, 0)), ("axis+y", (0, 1)), ("axis-y", (0, -1))):
        m = kinds == kind
        assert m.sum() >= 2 and np.array_equal(bits(right[m]), bits(wrong[m]))
        for (x, y) in np.array(centres)[m]:
            m10, m01 = R.moments(img, int(x), int(y))
            assert (np.sign(m10), np.sign(m01)) == sign
    assert set(right[kinds == "axis-x"].tolist()) == {180.0} and set(right[kinds == "axis-y"].tolist()) == {270.0}
    assert set(right[kinds == "zero"].tolist()) == {0.0} and set(wrong[kinds == "zero"].tolist()) == {90.0}


@pytest.mark.parametrize("direction", ["v", "h"])
def test_half_plane_scenes_reach_the_largest_moments(direction):
    img, centres, _ = D.detect_scene("half_" + direction)
    full = 255 * sum(u for v in range(-15, 16) for u in range(1, R.UMAX[abs(v)] + 1))
    seen = set()
    for x, y in centres:
        m10, m01 = R.moments(img, x, y)
        big, small = (m10, m01) if direction == "v" else (m01, m10)
        assert small == 0 and abs(big) >= full - 255 * 120   # a half disc less at most its centre line (the dot's column is dark on one side)
        seen.add(np.sign(big))
    assert seen == {1, -1}


def test_harris_scenes_reach_the_largest_sums_and_the_cancellation():
    top = {}
    for name in ("half_v", "half_h", "half_d+", "half_d-", "checker"):
        img, centres, _ = D.detect_scene(name)
        top[name] = np.array([R.harris_sums(img, x, y) for x, y in centres], np.int64)
    # a step through the block: 7 rows x 2 columns of |Ix| = 4 * 255 (14 * 1020^2 = 14.6 M, the largest a single step gives); the dot touches the
    # entries next to it, 12 of the 14 are whole at least
    a, b, c = top["half_v"].T
    assert a.min() >= 12 * 1020 ** 2 and np.all(a > 20 * b)                # one gradient direction only
    a, b, c = top["half_h"].T
    assert b.min() >= 12 * 1020 ** 2 and np.all(b > 20 * a)
    # a diagonal step: |Ix| = |Iy| = 3 * 255 along the step (7 block entries at least), Ix Iy of one sign: |c| large with either sign, a * b next to c * c
    cp, cm = top["half_d+"][:, 2], top["half_d-"][:, 2]
    assert cp.min() >= 7 * 765 ** 2 and cm.max() <= -7 * 765 ** 2
    for name in ("half_d+", "half_d-"):
        a, b, c = top[name].T.astype(object)
        assert np.all(abs(a * b - c * c) * 4 < a * b)                      # the two float products nearly cancel
    a, b, c = top["checker"].T                                             # the ring of zeros beside 255s: mixed gradients in both directions
    assert a.min() > 2 ** 20 and b.min() > 2 ** 20


def test_saturation_scene_reaches_the_clamp_and_2_to_the_24():
    img, centres, _ = D.detect_scene("saturation")
    S = R.blur_sums(img)
    assert S.max() == 257 * 257 * 255 >= 2 ** 24
    on, off = R.blur(img), R.blur(img, R.RIGHT._replace(saturate=False))
    assert ((S >> 16) >= 256).sum() > 100 and (on != off).sum() > 100
    kps, desc, tr = _trace_of("saturation")
    k0 = np.flatnonzero(kps["octave"] == 0)
    changed = beyond = 0
    for i in k0:
        x, y = int(kps["x"][i]), int(kps["y"][i])
        pos = R.sample_positions(kps["angle"][i])
        s = S[y + pos[..., 1], x + pos[..., 0]]
        if (x, y) in centres:
            assert (s >= 255 * 65536 + 32768).any()                        # S / 65536 >= 255.5 under a sample point
            if centres.index((x, y)) % 4 == 1:                             # the all-255 patches: S >= 2^24 under sample points
                assert (s >= 2 ** 24).any(), (x, y)
                beyond += 1
        changed += not np.array_equal(R.descriptor(img, off, x, y, kps["angle"][i]), desc[i])
    assert changed >= 8, "descriptors must depend on the clamp"
    assert beyond == 4


def test_tie_scene_bites_on_the_rounding_rule(oracle):
    img, kps, meta = D.ties()
    S = R.blur_sums(img)
    right = _ref_compute(oracle, img, kps)
    up = _ref_compute(oracle, img, kps, R.RIGHT._replace(blur_round="half_up"))
    down = _ref_compute(oracle, img, kps, R.RIGHT._replace(blur_round="truncate"))
    xy = [(int(k["x"]), int(k["y"])) for k in kps]
    assert len(D.alignments(xy[:8])) == 8 and all(D.interior(x, y) for x, y in xy[:8]), "the aligned path at every a, both parities of y"
    assert not any(D.interior(x, y) for x, y in xy[8:]) and len({(x % 4, y % 2) for x, y in xy[8:]}) == 8, "and the border path"
    seen = set()
    for i, (k, (pair, parity, first)) in enumerate(zip(kps, meta)):
        x, y = int(k["x"]), int(k["y"])
        (tx, ty), (px, py) = (R.PATTERN[pair][0], R.PATTERN[pair][1]) if first else (R.PATTERN[pair][1], R.PATTERN[pair][0])
        s = int(S[y + ty, x + tx])
        q = s >> 16
        assert s & 0xFFFF == 32768 and q % 2 == (parity == "odd")
        assert max(abs(tx - px), abs(ty - py)) >= 8
        win = img[y + py - 3:y + py + 4, x + px - 3:x + px + 4]
        assert win.min() == win.max() == (q + 1 if first else q)
        bit = lambda d: int(d[i][pair // 8] >> (pair % 8)) & 1
        # half-even gives q for the even tie and q + 1 for the odd one: half-up moves the even tie's bit, truncation the odd tie's
        assert bit(right) == (1 if (parity == "even") == first else 0)
        assert (bit(up) != bit(right)) == (parity == "even") and (bit(down) != bit(right)) == (parity == "odd"), (i, pair, parity, first)
        seen.add((parity, first, i < 8))
    assert len(seen) == 8


def test_comparison_scene_bites_on_the_strictness(oracle):
    img, kps, meta = D.comparisons()
    right = _ref_compute(oracle, img, kps)
    loose = _ref_compute(oracle, img, kps, R.RIGHT._replace(compare="<="))
    got = oracle.orb_compute(img, kps)
    flat = [0, 1, 8, 9]
    assert not got[flat].any() and not right[flat].any() and np.all(loose[flat] == 255)   # a constant patch: all 256 bits are 0, all 1 under <=
    xy = [(int(k["x"]), int(k["y"])) for k in kps]
    assert len(D.alignments(xy[:8])) == 8 and all(D.interior(x, y) for x, y in xy[:8]) and not any(D.interior(x, y) for x, y in xy[8:])
    blurred = R.blur(img)
    kinds = set()
    for i, (k, mine) in enumerate(zip(kps, meta)):
        x, y = int(k["x"]), int(k["y"])
        for pair, v0, v1 in mine:
            (x0, y0), (x1, y1) = R.PATTERN[pair]
            assert (int(blurred[y + y0, x + x0]), int(blurred[y + y1, x + x1])) == (v0, v1)
            bit = lambda d: int(d[i][pair // 8] >> (pair % 8)) & 1
            assert bit(right) == bit(got) == (v0 < v1) and bit(loose) == (v0 <= v1)
            kinds.add((int(np.sign(v1 - v0)), i < 8))
    assert kinds == {(d, part) for d in (-1, 0, 1) for part in (True, False)}


def test_searched_angles_have_their_properties():
    half, moved = D.searched_angles()
    assert len(set(half)) >= 64 and len(set(moved)) >= 16
    for a in half:   # some rotated coordinate within 2 float32 ulps of n + 0.5, with the restatement's own cos / sin
        c = R.rotate_pattern(*R.sincos(a)).ravel()
        assert (np.abs(c - np.floor(c) - f32(0.5)) <= 2 * np.spacing(np.abs(c))).any(), a
    wrong = R.RIGHT._replace(sincos="float32")
    for a in moved:  # cos / sin evaluated in float32 differ from the double-then-float ones AND a sample lands on another pixel
        assert R.sincos(a) != R.sincos(a, wrong) and not np.array_equal(R.sample_positions(a), R.sample_positions(a, wrong)), a
    fixed = D.fixed_angles()
    assert {0.0, 90.0, 180.0, 270.0, 360.0} <= set(fixed) and min(fixed) < 0 and max(fixed) > 360 and any(359.9999 < a < 360 for a in fixed)


def test_rotation_scene_bites_on_the_sincos_precision(oracle):
    """on the one-pixel checkerboard a sample that moves by a pixel reads the other colour: every 'moved' angle changes a descriptor"""
    img, kps = D.rotation("checker")
    blurred = R.blur(img)
    assert set(np.unique(blurred[8:-8, 8:-8]).tolist()) == {128, 129}
    moved = set(f32(a) for a in D.searched_angles()[1])
    idx = [i for i in range(len(kps)) if kps["angle"][i] in moved]
    xy = [(int(k["x"]), int(k["y"])) for k in kps]
    assert all(D.interior(x, y) for x, y in xy) and len(D.alignments(xy)) == 8
    assert len(idx) == 4 * len(moved) and len(D.alignments([xy[i] for i in idx])) == 8
    right = _ref_compute(oracle, img, kps, only=idx)
    wrong = _ref_compute(oracle, img, kps, R.RIGHT._replace(sincos="float32"), only=idx)
    for a in moved:
        mine = [i for i in idx if kps["angle"][i] == a]
        assert any(not np.array_equal(right[i], wrong[i]) for i in mine), a


def test_apron_scene_leaves_the_level_on_every_side(oracle):
    lw, lh, ls = oracle.level_geometry(D.APRON_W, D.APRON_H)
    img, kps = D.apron(ls.tolist(), lw.tolist(), lh.tolist())
    assert lw[7] == 32 and set(kps["octave"].tolist()) == {0, 7}
    want_angles = sorted(bits(a).item() for a in D.rotation_angles())
    for l in (0, 7):     # every centre under every rotation angle
        m = kps[kps["octave"] == l]
        for xy in {(float(x), float(y)) for x, y in zip(m["x"], m["y"])}:
            assert sorted(bits(m["angle"][(m["x"] == xy[0]) & (m["y"] == xy[1])]).tolist()) == want_angles, (l, xy)
    for l in (0, 7):
        sides = set()
        interior = 0
        for k in kps[kps["octave"] == l]:
            inv = f32(1) / ls[l]
            cx, cy = int(np.rint(f32(k["x"] * inv))), int(np.rint(f32(k["y"] * inv)))
            pos = R.sample_positions(k["angle"])
            gx, gy = cx + pos[..., 0], cy + pos[..., 1]
            out = ((gx < 0).any(), (gx >= lw[l]).any(), (gy < 0).any(), (gy >= lh[l]).any())
            sides.add(out)
            interior += not any(out)
        for want in ((1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 0), (0, 1, 1, 0), (1, 0, 0, 1), (0, 1, 0, 1)):
            assert tuple(bool(v) for v in want) in sides, (l, want)
        assert l == 7 or interior >= 4
    k0 = kps[kps["octave"] == 0]
    assert len(D.alignments([(int(x), int(y)) for x, y in zip(k0["x"], k0["y"])], D.APRON_W, D.APRON_H)) == 4


def test_scenes_are_deterministic():
    for name in ("disc_edge2", "saturation", "half_d-"):
        assert np.array_equal(D.DETECT[name]()[0], D.DETECT[name]()[0])
    assert D.ties()[0].tobytes() == D.ties()[0].tobytes() and D.rotation("noise")[1].tobytes() == D.rotation("noise")[1].tobytes()
