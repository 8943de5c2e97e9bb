"""geometries and scenes for the ragged tiles of k_fast_nms (test data): levels whose last tile column / row holds few reportable pixels or none

k_fast_nms cuts every level into 64 x 32 tiles from (0, 0); FAST reports 3 <= x < w - 3, 3 <= y < h - 3 only.  A tile without a reportable pixel leaves
at once, and in a bottom tile the wavefronts whose rows lie past the last reportable row skip the pre-test and the NMS (csrc/k_fast.hip).  The sizes below
are the smallest at which each of these decisions can go wrong; every level of every one is at least 32 px.
tests/test_fast_ragged_cpu.py holds the kernel's rule (afv_debug_fast_tiles: compiled from the kernel's own expressions) to the rectangles computed here;
tests/test_gpu_fast_ragged.py runs the scenes.  numpy only, seeded generators only."""
import functools

import numpy as np

import _detect_ref as R
import _detect_scenes as S

TILE_W, TILE_H = S.TILE_W, S.TILE_H
SCALE = 1.2
T = 20

# (w, h, nlevels): what the last tile column / row of a level holds
CASES = [
    (67, 40, 1),      # last tile column: x = 64 .. 66, none reportable; last tile row: 5 reportable rows
    (131, 70, 2),     # the same in the third tile column, 3 reportable rows in the third tile row; level 1 is 109 x 58
    (96, 35, 1),      # last tile row: y = 32 .. 34, none reportable
    (68, 36, 1),      # exactly one reportable column (x = 64) and one reportable row (y = 32)
    (100, 45, 1),     # last tile column 33 reportable columns wide, 10 reportable rows in the bottom tiles
    (101, 45, 1),     # 34
    (102, 45, 2),     # 35; level 1 is 85 x 38: a last tile column of 18 columns that is also a bottom tile of 3 rows
    (85, 58, 1),      # 18 columns (the width of the last tile column of level 1 of 640 x 480), 23 rows
]
FULL = (640, 480, 8)


def reportable(w, h, tx, ty):
    """the pixels of tile (tx, ty) FAST can report, in LEVEL coordinates: (x0, y0, x1, y1) with exclusive ends, None if there are none"""
    x0, x1 = max(3, tx * TILE_W), min(w - 3, tx * TILE_W + TILE_W)
    y0, y1 = max(3, ty * TILE_H), min(h - 3, ty * TILE_H + TILE_H)
    return (x0, y0, x1, y1) if x0 < x1 and y0 < y1 else None


def tiles_of(w, h):
    return [(tx, ty) for ty in range((h + TILE_H - 1) // TILE_H) for tx in range((w + TILE_W - 1) // TILE_W)]


def dense(w, h, seed):
    """random 5 x 5 blocks over the whole range plus +- 12 of noise: corners at the block junctions of every level of the pyramid"""
    rng = np.random.default_rng(7000 + seed)
    base = rng.integers(0, 256, (h // 5 + 2, w // 5 + 2))
    img = np.repeat(np.repeat(base, 5, axis=0), 5, axis=1)[:h, :w] + rng.integers(-12, 13, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def scene(w, h, variant):
    """S.border(w, h, variant) - bright single pixels on the last scored line of every side (rows / columns 3 and dim - 4) and on the first unscored
    one (2 and dim - 3), alone and next to each other - with everything farther than 5 px from such a pixel replaced by dense(): the designed pixels keep
    their flat 11 x 11 surroundings (clipped at the edge), so S.border's facts still hold, and every tile is full of other corners.
    Returns (image, facts)."""
    img, facts = S.border(w, h, variant)
    img = img.copy()
    marks = np.argwhere(img != S.BORDER_P)
    keep = np.zeros((h, w), bool)
    for y, x in marks:
        keep[max(y - 5, 0):y + 6, max(x - 5, 0):x + 6] = True
    d = dense(w, h, 10 * variant + (w * 31 + h) % 7)
    img[~keep] = d[~keep]
    img.setflags(write=False)
    return img, facts


def noise(w, h):
    """the frame a context sees before the test frame: full-range noise, corners everywhere (edge rows and columns included)"""
    return np.random.default_rng(7900 + w + h).integers(0, 2, (h, w), dtype=np.uint8) * 255


@functools.lru_cache(maxsize=None)
def reference(w, h, nlevels, variant):
    """the candidate sets of scene(w, h, variant) from the plain restatement: [set of (x, y, score)] per level"""
    img = scene(w, h, variant)[0]
    out = [set() for _ in range(nlevels)]
    for l, y, x, s in R.candidates(img, T, nlevels, SCALE):
        out[l].add((x, y, s))
    return out
