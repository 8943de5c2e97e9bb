"""Constructed stereo scenes for afv_frame_stereo_match: keypoints, descriptors and pyramid levels built by hand.  TEST INFRASTRUCTURE ONLY.

Every scene lives on a 96 x 64 image with 3 levels at scale 1.2 (level sizes 96 x 64, 80 x 53, 67 x 44) and at most 130 features a side; it is
fed to the device through set_features + set_pyramid (tests/test_gpu_stereo.py) and to the restatement tests/_stereo_ref.py as it stands.
A scene names the rule it aims at (`rule`: a key of _stereo_ref.FLIPS that must change its outcome when flipped; `reach`: trace counters
that must be positive).  tests/test_stereo_ref_cpu.py proves both on the CPU.

The levels are NOT a real pyramid: each level is its own random texture (values 20 .. 200), and the right eye's level is the left one moved
`d` pixels (right[y, x] = left[y, x + d]), so a left window at column su has SAD 0 against the right window at su - d and a large SAD
elsewhere.  Pixels are then patched by hand where a scene needs particular SADs.
"""
import math

import numpy as np

import _stereo_ref as SR

f32 = np.float32
WIDTH, HEIGHT, NLEVELS, SCALE = 96, 64, 3, 1.2


def level_sizes(w=WIDTH, h=HEIGHT, nlevels=NLEVELS, scale=SCALE):
    """the extractor's level sizes: round(w * (1.0f / (float)pow(scale, l))) in float, halves to even"""
    out = []
    for l in range(nlevels):
        s = f32(math.pow(float(f32(scale)), float(l)))
        inv = f32(f32(1.0) / s)
        out.append((int(np.rint(f32(f32(w) * inv))), int(np.rint(f32(f32(h) * inv)))))
    return out


SIZES = level_sizes()
LEVEL_SIZE = [f32(math.pow(float(f32(SCALE)), float(l))) for l in range(NLEVELS)]  # keyPtsSize of an octave in these scenes


class Scene:
    def __init__(self, name, rule, reach, L, R, pyrL, pyrR, mbf, fx, th_high, th_low):
        self.name, self.rule, self.reach = name, rule, tuple(reach)
        self.L, self.R, self.pyrL, self.pyrR = L, R, pyrL, pyrR
        self.mbf, self.fx, self.th_high, self.th_low = f32(mbf), f32(fx), f32(th_high), f32(th_low)

    def run(self, flip=None):
        return SR.compute_stereo_matches(self.L, self.R, self.pyrL, self.pyrR, self.mbf, self.fx, self.th_high, self.th_low, flip=flip)


def same_outcome(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a[:4], b[:4]))


class Builder:
    """left / right keypoint lists over a textured pair of pyramids"""

    def __init__(self, seed, d=4, desc_bytes=32, float_dim=0, brightness=0):
        self.rng = np.random.default_rng(seed)
        self.d, self.desc_bytes, self.float_dim = d, desc_bytes, float_dim
        self.pl = [self.rng.integers(20, 201, (h, w)).astype(np.uint8) for (w, h) in SIZES]
        self.pr = []
        for im in self.pl:
            r = self.rng.integers(20, 201, im.shape).astype(np.uint8)
            if d >= 0:
                r[:, :im.shape[1] - d] = im[:, d:]
            self.pr.append((r.astype(np.int32) + brightness).astype(np.uint8))
        self.kl, self.kr = [], []

    def desc(self):
        if self.float_dim:
            return self.rng.normal(0, 1, self.float_dim).astype(np.float32)
        return self.rng.integers(0, 256, self.desc_bytes).astype(np.uint8)

    def flipped(self, desc, bits, first=0):
        """desc at Hamming distance `bits` (bits first .. first + bits - 1 turned); float rows: L2^2 grows with `bits`"""
        d = desc.copy()
        if self.float_dim:
            d[first % self.float_dim] += f32(0.125) * f32(bits)
            return d
        for b in range(first, first + bits):
            d[b // 8] ^= np.uint8(1 << (b % 8))
        return d

    @staticmethod
    def _coord(c, size):
        v = f32(f32(c) * size)
        assert int(SR.c_round(f32(v * f32(f32(1.0) / size)))) == c, (c, size)
        return v

    def left(self, cx, cy, level=0, desc=None, x=None, y=None, size=None):
        """a left keypoint whose window centre on `level` is (cx, cy); x / y / size override the values derived from it"""
        size = LEVEL_SIZE[level] if size is None else f32(size)
        desc = self.desc() if desc is None else desc
        self.kl.append((self._coord(cx, size) if x is None else f32(x), self._coord(cy, size) if y is None else f32(y), level, size, desc))
        return desc

    def right(self, cx, cy, level=0, desc=None, x=None, y=None, size=None, octave=None):
        """size: the keypoint's own keyPtsSize (2 x size is its row band); level only places it"""
        lsize = LEVEL_SIZE[level]
        desc = self.desc() if desc is None else desc
        self.kr.append((self._coord(cx, lsize) if x is None else f32(x), self._coord(cy, lsize) if y is None else f32(y),
                        level if octave is None else octave, f32(lsize if size is None else size), desc))
        return len(self.kr) - 1

    def pair(self, cx, cy, level=0, bits=0, sad=0, **kw):
        """a left keypoint and its true right counterpart (d columns to the left); `sad`: their SAD at the true offset"""
        desc = self.left(cx, cy, level)
        iR = self.right(cx - self.d, cy, level, desc=self.flipped(desc, bits), **kw)
        if sad:
            self.bump(level, cy - 3, cx - 3, sad)
        return len(self.kl) - 1, iR

    def bump(self, level, y, x, v):
        """one window pixel: left = right + v, so the window around it has SAD v where it had 0"""
        self.pr[level][y, x - self.d] = 100
        self.pl[level][y, x] = 100 + v

    def ballast(self, sad=10):
        """two accepted pairs of SAD `sad` far from the scene's rows, so that the median filter's threshold is positive"""
        self.pair(40, 10, 0, sad=sad)
        self.pair(60, 54, 0, sad=sad)

    def symmetric(self, level, cy, cx, half=16):
        """make the left level mirror-symmetric about column cx on the window's rows, and the right level its copy d columns to the left:
        then SAD(inc = -1) == SAD(inc = +1) around the true offset and the parabola's deltaR is exactly 0"""
        im, r = self.pl[level], self.pr[level]
        for k in range(1, half + 1):
            if cx + k < im.shape[1] and cx - k >= 0:
                im[cy - 5:cy + 6, cx + k] = im[cy - 5:cy + 6, cx - k]
        lo, hi = max(cx - half, self.d), min(cx + half + 1, im.shape[1])
        r[cy - 5:cy + 6, lo - self.d:hi - self.d] = im[cy - 5:cy + 6, lo:hi]

    def scene(self, name, rule=None, reach=(), mbf=40.0, fx=30.0, th_high=50.0, th_low=50.0):
        def side(k):
            dim = self.float_dim or self.desc_bytes
            dt = np.float32 if self.float_dim else np.uint8
            desc = np.stack([e[4] for e in k]) if k else np.zeros((0, dim), dt)
            return SR.Side([e[0] for e in k], [e[1] for e in k], [e[2] for e in k], [e[3] for e in k], desc)
        return Scene(name, rule, reach, side(self.kl), side(self.kr), self.pl, self.pr, mbf, fx, th_high, th_low)


def _max_d(mbf, fx):
    mbf, fx = f32(mbf), f32(fx)
    return f32(mbf / f32(mbf / fx))


# ---- the row band ----
def s_band_max():
    b = Builder(1)
    b.ballast()
    d0 = b.left(50, 30)                       # row 30
    b.left(50, 31, desc=d0)                   # one row beyond: nothing
    b.right(46, 0, y=27.5, desc=d0)           # size 1: r = 2, maxr = ceil(29.5) = 30 == (int)vL exactly
    return b.scene("band_max", "band_max", ("dist_evals", "row_empty"))


def s_band_min():
    b = Builder(2)
    b.ballast()
    d0 = b.left(50, 30)
    b.left(50, 29, desc=d0)                   # one row beyond
    b.right(46, 0, y=32.5, desc=d0)           # minr = floor(30.5) = 30
    return b.scene("band_min", "band_min", ("dist_evals", "row_empty"))


def s_row_trunc():
    b = Builder(3)
    b.ballast()
    d0 = b.left(50, 31, y=30.9)               # vL = 30.9: row 30 (sv = round(30.9) = 31)
    b.right(46, 0, y=28.0, desc=d0)           # band 26 .. 30: holds row 30, not 31
    return b.scene("row_trunc", "row_trunc", ("accepted",))


def s_row_clip():
    b = Builder(4)
    b.ballast()
    d0 = b.left(50, 5)                        # row 5
    b.right(46, 5, desc=d0, size=3.0)         # r = 6: band -1 .. 11 crosses row 0
    d1 = b.left(50, 58)                       # row 58 (rows = 64)
    b.right(46, 58, desc=d1, size=3.0)        # band 52 .. 64 crosses row 63
    d2 = b.left(30, 0, y=0.5)                 # row 0; its window leaves the level (deviation C)
    b.right(26, 0, y=-1.5, desc=d2, size=0.2) # band -2 .. -1: wholly above the image
    d3 = b.left(30, 63, y=63.2)               # row 63
    b.right(26, 0, y=64.5, desc=d3, size=0.2) # band 64 .. 65: wholly below
    return b.scene("row_clip", "row_clip", ("rows_dropped", "accepted"))


def s_right_size():
    b = Builder(5)
    b.ballast()                               # left 0, 1 / right 0, 1
    d0 = b.left(50, 30)                       # left 2
    b.left(20, 30, size=3.0, level=0, x=20.0, y=40.0)  # left 3: size 3 at the index of right 3
    b.right(46, 30, desc=b.flipped(d0, 3))    # right 2: in the band by its own size
    b.right(46, 0, y=34.5, desc=d0)           # right 3: own size 1: band 32 .. 37, not row 30; the left size 3 at index 3 would make it 28 .. 41
    return b.scene("right_size_deviation_A", "right_size", ("accepted",))


def s_nr_gt_n():
    b = Builder(6)
    b.pair(50, 30, sad=10)
    for k in range(4):
        b.right(20 + 5 * k, 12 + 10 * k)
    return b.scene("nr_gt_n", None, ("accepted",))


# ---- the octave and u gates ----
def _octaves(seed, name, rule, bits_lo, bits_hi):
    b = Builder(seed)
    b.ballast()
    d0 = b.left(40, 20, level=2)
    for octave, bits in ((0, 0), (1, bits_lo), (3, bits_hi), (4, 1)):
        b.right(36, 20, level=2, octave=octave, size=1.0, desc=b.flipped(d0, bits))
    return b.scene(name, rule, ("oct_lo", "oct_hi", "accepted"))


def s_oct_lo():
    return _octaves(7, "octave_minus_1_and_minus_2", "oct_lo", 2, 3)


def s_oct_hi():
    return _octaves(8, "octave_plus_1_and_plus_2", "oct_hi", 3, 2)


def _u_edge(seed, name, rule, reach, which, ulps):
    b = Builder(seed)
    b.ballast()
    d0 = b.left(50, 30)
    uL = b.kl[-1][0]
    edge = f32(uL - _max_d(40.0, 30.0)) if which == "min" else uL
    for _ in range(ulps):
        edge = np.nextafter(edge, f32(-np.inf) if which == "min" else f32(np.inf))
    b.right(0, 30, x=edge, desc=d0)
    return b.scene(name, rule, reach)


def s_u_min_edge():
    return _u_edge(9, "uR_at_uL_minus_maxD", "u_min", ("dist_evals",), "min", 0)


def s_u_min_out():
    return _u_edge(10, "uR_one_ulp_below_uL_minus_maxD", None, ("u_lo",), "min", 1)


def s_u_max_edge():
    return _u_edge(11, "uR_at_uL", "u_max", ("dist_evals",), "max", 0)


def s_u_max_out():
    return _u_edge(12, "uR_one_ulp_above_uL", None, ("u_hi",), "max", 1)


def s_maxu_neg():
    b = Builder(13)
    b.ballast()
    d0 = b.left(0, 30, x=-0.5)
    b.right(0, 30, x=-1.5, desc=d0)
    return b.scene("uL_minus_minD_negative", "maxu_neg", ("maxu_neg",))


# ---- the descriptor decision ----
def s_dist_tie():
    b = Builder(14)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(44, 30, desc=b.flipped(d0, 2, first=8))
    b.right(46, 30, desc=b.flipped(d0, 2, first=40))
    return b.scene("distance_tie_lower_iR_wins", "tie_first", ("dist_ties",))


def s_dist_eq_th_high():
    b = Builder(15, d=4)
    b.right(90, 30)                            # right 0: same row, outside the u range; what bestIdxR = 0 falls back to
    d0 = b.left(50, 30)
    b.right(46, 30, desc=b.flipped(d0, 40))    # dist == th_high: never matches
    return b.scene("dist_equals_th_high", "tie_first", ("dist_eq_th", "best0_used"), th_high=40.0, th_low=60.0)


def s_best0():
    b = Builder(16)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(46, 30, desc=d0, octave=2)         # in the row, fails the octave gate: bestDist1 stays th_high = 40 < thOrbDist = 50
    return b.scene("bestIdxR_starts_at_0", "best0", ("best0_used",), th_high=40.0, th_low=60.0)


def s_orb_equal():
    b = Builder(17)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(46, 30, desc=b.flipped(d0, 50))
    return b.scene("best_equals_thOrbDist", "orb_lt", ("orb_equal",), th_high=60.0, th_low=40.0)


def s_th_sep():
    b = Builder(18)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(46, 30, desc=b.flipped(d0, 55))    # < th_high = 60, not < thOrbDist = 50
    return b.scene("th_high_differs_from_th_low", "th_sep", ("orb_reject",), th_high=60.0, th_low=40.0)


# ---- the SAD window ----
def s_inc_lo():
    b = Builder(19, d=10)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(45, 30, desc=d0)                   # su0 = 45: the true column 40 is offset -5
    return b.scene("sad_minimum_at_minus_5", "inc_lo", ("inc_lo",))


def s_inc_hi():
    b = Builder(20)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(41, 30, desc=d0)                   # the true column is offset +5
    return b.scene("sad_minimum_at_plus_5", "inc_hi", ("inc_hi",))


def s_sad_tie():
    b = Builder(21)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(46, 30, desc=d0)
    su, su0, sv = 50, 46, 30
    P = b.rng.permuted(np.tile(np.array([30, 90, 150]), (11, 1)), axis=1)  # per row three distinct values: period 3 in x
    for j in range(11):
        b.pl[0][sv - 5:sv + 6, su - 5 + j] = P[:, j % 3]
    for x in range(su0 - 10, su0 + 11):
        b.pr[0][sv - 5:sv + 6, x] = P[:, (x - (su0 - 7)) % 3]            # SAD 0 at offsets -5, -2, +1, +4
    b.pr[0][sv - 4, su0 - 9] = 200                                        # breaks -5 (and -4, -3)
    b.pr[0][sv - 4, su0 + 8] = 200                                        # breaks +4 (and +3, +5)
    return b.scene("equal_sad_at_two_offsets", "sad_tie_first", ("sad_ties", "accepted"))


def s_sad_flat():
    b = Builder(22)
    b.ballast()
    d0 = b.left(50, 30)
    b.right(46, 30, desc=d0)
    b.pl[0][25:36, 45:56] = 77
    b.pr[0][25:36, 36:57] = 140
    return b.scene("flat_strip_all_sads_equal", None, ("sad_flat", "inc_lo"))  # (all equal: the first offset, -5, keeps the minimum)


def s_centre_sub():
    b = Builder(23, brightness=30)             # the right eye is 30 brighter everywhere
    b.ballast()
    b.pair(50, 30)
    return b.scene("brightness_offset_between_the_eyes", "centre_sub", ("accepted",))


def s_gate_endu():
    b = Builder(24)
    b.ballast()
    b.pair(WIDTH - 11 + 4, 30)                 # su0 = cols - 11: endu = cols
    return b.scene("endu_equals_cols", "gate_endu", ("gate_endu",))


def s_gate_endu_in():
    b = Builder(25)
    b.ballast()
    b.pair(WIDTH - 12 + 4, 30)                 # su0 = cols - 12: the last column the gate lets through
    return b.scene("endu_one_below_cols", None, ("accepted",))


def s_gate_iniu():
    b = Builder(26)
    b.ballast()
    d0 = b.left(3, 30)
    b.right(0, 30, x=-1.0, desc=d0)            # su0 = -1: iniu < 0 (deviation C's su0 - 10 < 0 holds too)
    return b.scene("iniu_negative", None, ("gate_iniu", "c_r0_left", "c_left"))


def _edge_c(seed, name, rule, level, cx, cy, d=4, reach=()):
    b = Builder(seed, d=d)
    b.ballast()
    b.pair(cx, cy, level)
    return b.scene(name, rule, reach or (rule,))


def s_c_top():
    return _edge_c(27, "window_above_level_2", "c_top", 2, 40, 4)


def s_c_top_in():
    return _edge_c(28, "window_touches_top_of_level_2", None, 2, 40, 5, reach=("accepted",))


def s_c_bottom():
    return _edge_c(29, "window_below_level_1", "c_bottom", 1, 40, SIZES[1][1] - 5)


def s_c_bottom_in():
    return _edge_c(30, "window_touches_bottom_of_level_1", None, 1, 40, SIZES[1][1] - 6, reach=("accepted",))


def s_c_right():
    return _edge_c(31, "left_window_beyond_right_edge", "c_right", 0, WIDTH - 5, 30, d=20)


def s_c_right_in():
    return _edge_c(32, "left_window_touches_right_edge", None, 0, WIDTH - 6, 30, d=20, reach=("accepted",))


def s_c_r0_left():
    return _edge_c(33, "strip_beyond_left_edge_level_2", "c_r0_left", 2, 9 + 4, 20)


def s_c_r0_left_in():
    return _edge_c(34, "strip_touches_left_edge_level_2", None, 2, 10 + 4, 20, reach=("accepted",))


def s_c_left():
    b = Builder(35)                            # su - 5 < 0 implies su0 - 10 < 0 (uR <= uL): reached, never alone
    b.ballast()
    d0 = b.left(4, 30)
    b.right(2, 30, desc=d0)
    return b.scene("left_window_beyond_left_edge", None, ("c_left", "c_r0_left"))


def s_level_missing():
    b = Builder(36)
    b.ballast()
    d0 = b.left(30, 20, level=2, size=LEVEL_SIZE[2])
    b.kl[-1] = b.kl[-1][:2] + (3,) + b.kl[-1][3:]   # octave 3 of a 3-level pyramid
    b.right(26, 20, level=2, octave=3, size=1.0, desc=d0)
    return b.scene("octave_is_no_level", None, ("level_missing",))


def s_coord_range():
    """keyPtsSize 0 (a zero-initialised sizes array), a denormal and a tiny size: 1 / size is inf or huge, the scaled coordinates are inf,
    NaN (0 * inf) or beyond any level, and the keypoint is skipped before any int gate sees them"""
    b = Builder(46)
    b.ballast()
    for k, (size, x) in enumerate(((0.0, 50.0), (1e-40, 50.0), (1e-30, 50.0), (0.0, 0.0), (float("nan"), 50.0))):
        d0 = b.left(0, 0, x=x, y=24.0 + 3 * k, size=size)
        b.right(46, 24 + 3 * k, desc=d0, x=min(x, 46.0))
    return b.scene("left_size_zero_denormal_tiny_nan", None, ("coord_range",))


# ---- the sub-pixel step and the disparity gates ----
def s_disp_zero():
    b = Builder(37, d=0)
    b.ballast()
    b.pair(50, 30)
    b.symmetric(0, 30, 50)
    return b.scene("disparity_exactly_zero", "disp_ge0", ("disp_zero", "accepted"))


def s_disp_neg():
    b = Builder(38, d=0)
    b.ballast()
    x = np.nextafter(f32(50.0), f32(-np.inf))
    d0 = b.left(50, 30, x=x)
    b.right(50, 30, x=x, desc=d0)
    b.symmetric(0, 30, 50)
    return b.scene("disparity_slightly_negative", "disp_neg", ("disp_neg",))


def s_disp_max():
    b = Builder(39, d=8)
    b.pair(40, 10, 0, sad=10)                  # (ballast of this d)
    b.pair(50, 30)
    b.symmetric(0, 30, 50)
    assert _max_d(8.0, 8.0) == f32(8.0)
    return b.scene("disparity_equals_maxD", "disp_lt_max", ("disp_ge_max",), mbf=8.0, fx=8.0)


# ---- the median filter ----
def s_median_0():
    b = Builder(40, d=10)
    d0 = b.left(50, 30)
    b.right(45, 30, desc=d0)                   # offset -5: rejected; nothing is accepted
    return b.scene("median_of_no_pairs", None, ("inc_lo",))


def s_median_1():
    b = Builder(41)
    b.pair(50, 30, sad=10)
    return b.scene("median_of_one_pair", None, ("accepted",))


def s_median_1_zero():
    b = Builder(42)
    b.pair(50, 30)                             # SAD 0 alone: thDist = 0 and 0 >= 0 removes it, as the reference's walk does
    return b.scene("median_of_one_pair_sad_0", "median_ge", ("accepted", "median_removed"))


def s_median_2():
    b = Builder(43)
    b.pair(50, 20, sad=10)
    b.pair(50, 40, sad=30)                     # size / 2 = 1: median 30, thDist 63; index 0 would give 21 and remove this pair
    return b.scene("median_of_two_pairs", "median_index", ("accepted",))


def s_median_3():
    b = Builder(44)
    b.pair(30, 12)
    b.pair(50, 30, sad=10)
    b.pair(60, 50, sad=40)                     # median 10, thDist 21: removed
    return b.scene("median_of_three_pairs", None, ("median_removed",))


def s_median_on_th():
    b = Builder(45)
    b.pair(30, 12, sad=10)
    b.pair(50, 30, sad=10)
    b.pair(60, 50, sad=21)                     # 1.5f * 1.4f * 10 rounds to 21 exactly
    assert f32(f32(f32(1.5) * f32(1.4)) * f32(10.0)) == f32(21.0)
    return b.scene("pair_exactly_on_thDist", "median_ge", ("median_on_th",))


# ---- sizes and descriptor kinds ----
def random_scene(name, seed, n_l, n_r, desc_bytes=32, float_dim=0, th=50.0):
    """min(n_l, n_r) true pairs spread over the three levels (some a few bits / a little noise apart, SADs 0 .. 40), the rest unrelated
    keypoints; windows may overlap, which only makes the SADs less tidy"""
    b = Builder(seed, desc_bytes=desc_bytes, float_dim=float_dim)
    rng = b.rng
    m = min(n_l, n_r)
    for i in range(max(n_l, n_r)):
        level = int(rng.integers(0, NLEVELS))
        w, h = SIZES[level]
        cx, cy = int(rng.integers(3, w - 3)), int(rng.integers(3, h - 3))
        if i < m:
            sad = int(rng.integers(0, 41))
            ok = 8 <= cy < h - 8 and 16 <= cx < w - 8
            b.pair(cx, cy, level, bits=int(rng.integers(0, 12)), sad=sad if ok and rng.random() < 0.7 else 0)
        elif i < n_l:
            b.left(cx, cy, level)
        else:
            b.right(cx, cy, level)
    return b.scene(name, None, (), th_high=th, th_low=th)


def size_scenes():
    out = []
    for k, (n_l, n_r) in enumerate(((0, 5), (5, 0), (0, 0), (1, 1), (63, 65), (64, 64), (65, 63), (129, 129), (129, 1), (1, 129))):
        out.append(random_scene("sizes_N%d_Nr%d" % (n_l, n_r), 100 + k, n_l, n_r))
    return out


def kind_scenes():
    return [random_scene("rows_32_bytes", 200, 40, 44, desc_bytes=32),
            random_scene("rows_61_bytes", 201, 40, 44, desc_bytes=61),
            random_scene("rows_20_bytes", 202, 40, 44, desc_bytes=20, th=40.0),
            random_scene("rows_64_floats", 203, 40, 44, float_dim=64, th=0.5)]


CONSTRUCTED = (s_band_max, s_band_min, s_row_trunc, s_row_clip, s_right_size, s_nr_gt_n, s_oct_lo, s_oct_hi, s_u_min_edge, s_u_min_out,
               s_u_max_edge, s_u_max_out, s_maxu_neg, s_dist_tie, s_dist_eq_th_high, s_best0, s_orb_equal, s_th_sep, s_inc_lo, s_inc_hi,
               s_sad_tie, s_sad_flat, s_centre_sub, s_gate_endu, s_gate_endu_in, s_gate_iniu, s_c_top, s_c_top_in, s_c_bottom, s_c_bottom_in,
               s_c_right, s_c_right_in, s_c_r0_left, s_c_r0_left_in, s_c_left, s_level_missing, s_coord_range, s_disp_zero, s_disp_neg, s_disp_max,
               s_median_0, s_median_1, s_median_1_zero, s_median_2, s_median_3, s_median_on_th)

_cache = {}


def all_scenes():
    """every scene, built once and shared (the restatement's answer is cached with it: Scene.expected)"""
    if "all" not in _cache:
        scenes = [f() for f in CONSTRUCTED] + size_scenes() + kind_scenes()
        for s in scenes:
            s.expected = s.run()
        _cache["all"] = scenes
    return _cache["all"]
