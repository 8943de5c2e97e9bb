"""frame sizes whose AKAZE61 level planes end in ragged tiles (test data, numpy only)

The kernels of the AKAZE61 path cut each level into tiles whose size depends on the level (its FED step count N, its derivative
sigma_size S).  A tile-tail bug shows only where a level's width or height leaves a remainder of 0, 1 or tile - 1 against that tile.
SIZES below was picked so that, counted over the levels of every size, each kernel family meets each of those three remainders on
both axes; tests/test_oracle_akaze_scenes.py::test_shape_list_covers_every_tail recomputes the claim from the evolution plan, so the
list cannot go stale silently when a tile constant or the plan changes.

Tile constants (anyfeature-vslam_amd/csrc/):
  * k_akaze.hip:16-17     AT_W x AT_H = 64 x 32: k_akz_gauss, k_akz_contrast_modg / k_akz_modg, k_akz_flow, k_akz_nld_step,
                          k_akz_deriv1, k_akz_hessian (the step-by-step path and every level-0 Gaussian);
  * k_akaze.hip:503       k_akz_fed_gauss<N> writes (62 - 2N) x (64 - 2N) outputs per tile (the fused level kernel, N = FED steps);
  * k_akaze.hip:788,802   k_akz_dhess<S> writes 64 - 4S columns in strips of AKZ_DH_ROWS = 64 rows (16 rows for a batch of fewer
                          than 8 frames: the remainders 0, 1, 63 of 64 are 0, 1, 15 of 16 as well);
  * k_akaze.hip:911       k_akz_halfsample: 64 x 4 destination pixels per workgroup;
  * k_akaze_detect.hip:47-49  k_akz_cand_mask: 64-column chunks (at most AKD_MAXCHUNKS = 32: levels up to 2048 wide) x AKM_ROWS = 32 rows.
Extractor limits: akaze_api.hip akz_frames_ok (w >= 80, h >= 40, stride >= w), akz_detect_enqueue (a level wider than 2048 is refused with
AFV_EUNSUPPORTED), akz_describe_enqueue (round(w / h) quadtree roots, 1 .. 16); akaze_plan.hip afv_akaze_plan_for (every halved level even:
exact 2x INTER_AREA; 2 <= sigma_size <= 8)."""
import numpy as np

AT_W, AT_H = 64, 32
DH_ROWS = 64
HALF_W, HALF_H = 64, 4
MASK_W, MASK_ROWS, MASK_MAXCHUNKS = 64, 32, 32
MIN_W, MIN_H = 80, 40
MAX_LEVEL_W = MASK_W * MASK_MAXCHUNKS          # 2048
FED_FUSED_MAX = 8                               # k_akaze.hip:468 AKZ_FED_MAX


def fed_tile(n):
    return 62 - 2 * n, 64 - 2 * n


def dhess_tile(s):
    return 64 - 4 * s, DH_ROWS


def level_families(nsteps, sigma_size, octave, first_of_octave):
    """[(family, tile_w, tile_h)] of the kernels that tile one level"""
    out = [("tile64x32", AT_W, AT_H), ("cand_mask", MASK_W, MASK_ROWS)]
    if 1 <= nsteps <= FED_FUSED_MAX:
        out.append(("fed_gauss<%d>" % nsteps,) + fed_tile(nsteps))
    if 2 <= sigma_size <= 4:
        out.append(("dhess<%d>" % sigma_size,) + dhess_tile(sigma_size))
    if octave > 0 and first_of_octave:
        out.append(("halfsample", HALF_W, HALF_H))
    return out


def plan_levels(plan):
    """(w, h, octave, nsteps, sigma_size, first_of_octave) per level of an evolution plan (oracle or product layout)"""
    out = []
    for i in range(plan.nlevels):
        L = plan.lv[i]
        first = i > 0 and plan.lv[i - 1].octave != L.octave
        out.append((L.w, L.h, L.octave, L.nsteps, L.sigma_size, first))
    return out


def accepted(plan):
    """the extractor's own acceptance rules for a frame whose plan this is (afv_akaze_plan_for, akz_frames_ok, akz_detect_enqueue)"""
    lv = plan_levels(plan)
    if plan.w < MIN_W or plan.h < MIN_H or plan.w > MAX_LEVEL_W or not 1 <= int(np.round(np.float32(plan.w) / np.float32(plan.h))) <= 16:
        return False
    for i, (w, h, o, n, s, first) in enumerate(lv):
        if not 2 <= s <= 8:
            return False
        if first and (lv[i - 1][0] % 2 or lv[i - 1][1] % 2):
            return False
    return True


def tails(plan):
    """{(family, axis, tile, remainder)} of the remainders 0, 1 and tile - 1 that this plan's levels reach"""
    got = set()
    for (w, h, o, n, s, first) in plan_levels(plan):
        for fam, tw, th in level_families(n, s, o, first):
            for axis, d, t in ((0, w, tw), (1, h, th)):
                r = d % t
                if r in (0, 1, t - 1):
                    got.add((fam, axis, t, r))
    return got


def wanted(plans):
    """every (family, axis, tile, remainder in {0, 1, tile - 1}) for the families that occur in the given plans"""
    want = set()
    for plan in plans:
        for (w, h, o, n, s, first) in plan_levels(plan):
            for fam, tw, th in level_families(n, s, o, first):
                for axis, t in ((0, tw), (1, th)):
                    for r in (0, 1, t - 1):
                        want.add((fam, axis, t, r))
    return want


SMALLEST = (80, 40)              # the smallest frame akz_check accepts
ONE_OCTAVE = (126, 62)           # w < 160: the plan stops after octave 0 (and 126 = 64 + 62: remainder 62 of 64, 30 of 32)
WIDEST = (2048, 128)             # level 0 fills all 32 mask chunks; w / h = 16 is the most quadtree roots k_akz_select takes
FIRST_REFUSED = (2049, 40)       # one octave (h < 80): plan_for accepts it, detection refuses it (AFV_EUNSUPPORTED).  Any 2049-wide frame is
                                 # refused somewhere (h >= 80: odd level 0; h < 80: round(w / h) > 16 quadtree roots), so only the direct
                                 # afv_akaze_detect call pins the 2048-column limit itself
CONFIG5 = (1280, 720)

# ragged sizes, picked greedily (smallest area per newly covered tail) until every tail of every family is reached; the odd ones stay
# below 160 x 80 (one octave), which is the only way to reach the odd remainders of the octave-0 fed_gauss<3> tile
RAGGED = [(191, 63), (193, 64), (111, 65), (168, 102), (113, 57), (192, 106), (206, 110), (208, 98), (210, 100), (107, 56), (108, 58),
          (109, 59), (382, 104), (386, 108), (198, 80), (200, 80), (202, 80)]

SIZES = [SMALLEST, ONE_OCTAVE] + RAGGED + [WIDEST, CONFIG5]


def size_id(wh):
    return "%dx%d" % wh
