"""the rule by which k_fast_nms drops work outside the level (csrc/k_fast.hip: empty tiles leave at once, wavefronts of a bottom tile whose rows lie past
the last reportable row skip the pre-test and the NMS) against rectangles computed here, without a GPU.  afv_debug_fast_tiles is compiled from the
expressions the kernel itself uses and decodes the flat tile index as the kernel does, so this test cannot drift from the kernel.  The scenes of
tests/test_gpu_fast_ragged.py are proved here as well: their designed border pixels behave in the plain restatement as S.border says."""
import ctypes as C

import numpy as np
import pytest

import _detect_ref as R
import _fast_ragged as F

PRE_PAIRS, PRE_ITERS, PRE_GROUPS = 34, 5, 7      # step 2a: thread tid -> row group tid // 34, which computes the tile rows 5 g - 1 .. 5 g + 3
NMS_ROWS = 8                                      # step 3: wavefront w owns the tile rows 8 w .. 8 w + 7


def _tiles(afv, w, h, nlevels):
    lib = afv._lib.load()
    p = afv._lib.OrbParams(1000, nlevels, F.SCALE, F.T, w, h, 1)
    tiles = np.zeros((4096, 12), np.int32)
    wh = np.zeros((afv._lib.MAX_LEVELS, 2), np.int32)
    n = C.c_int(0)
    rc = lib.afv_debug_fast_tiles(C.byref(p), w, h, afv._lib.ptr(tiles), tiles.size, afv._lib.ptr(wh), C.byref(n))
    assert rc == 0, rc
    return tiles[:n.value], wh[:nlevels]


@pytest.mark.parametrize("case", F.CASES + [F.FULL])
def test_tile_rule_matches_the_reportable_rectangles(afv, case):
    w, h, nlevels = case
    tiles, wh = _tiles(afv, w, h, nlevels)
    lw, lh, _ = R.level_geometry(w, h, nlevels, F.SCALE)
    assert wh[:, 0].tolist() == lw and wh[:, 1].tolist() == lh and min(lw + lh) >= 32
    want = [(l, tx, ty) for l in range(nlevels) for tx, ty in F.tiles_of(lw[l], lh[l])]
    assert [tuple(t[:3]) for t in tiles.tolist()] == want, "the flat tile index enumerates every tile of every level once, level by level, row by row"
    empty_rule, empty_rect = set(), set()
    for l, tx, ty, x0, y0, x1, y1, empty, row_hi, g_last, pre_idle, nms_idle in tiles.tolist():
        rect = F.reportable(lw[l], lh[l], tx, ty)
        if empty:
            empty_rule.add((l, tx, ty))
        if rect is None:
            empty_rect.add((l, tx, ty))
            assert x1 <= x0 or y1 <= y0
            continue
        assert (tx * 64 + x0, ty * 32 + y0, tx * 64 + x1, ty * 32 + y1) == rect, (case, l, tx, ty)
        # the score rows of the tile's plane that can be non-zero: the reportable rows and, where they are reportable rows of the level, the neighbour
        # rows -1 and 32 - each one computed by a live row group in a wavefront that runs the pre-test, each reportable row by a wavefront that runs the NMS
        rows = [y for y in range(-1, 33) if 3 <= ty * 32 + y < lh[l] - 3]
        assert rows and max(rows) == row_hi and 0 <= g_last < PRE_GROUPS
        for y in rows:
            g = (y + 1) // PRE_ITERS
            assert g <= g_last, (case, l, tx, ty, y)
            waves = {tid // 64 for tid in range(g * PRE_PAIRS, (g + 1) * PRE_PAIRS)}
            assert not any(pre_idle >> wv & 1 for wv in waves), (case, l, tx, ty, y)
            if 0 <= y < 32:
                assert not nms_idle >> (y // NMS_ROWS) & 1, (case, l, tx, ty, y)
        # and no more than that: an idle wavefront is one with no such row
        for wv in range(4):
            groups = {tid // PRE_PAIRS for tid in range(64 * wv, 64 * wv + 64)} & set(range(PRE_GROUPS))
            assert bool(pre_idle >> wv & 1) == (min(groups) > g_last), (case, l, tx, ty, wv)
            assert bool(nms_idle >> wv & 1) == (not any(NMS_ROWS * wv <= y < NMS_ROWS * wv + NMS_ROWS for y in rows)), (case, l, tx, ty, wv)
    assert empty_rule == empty_rect, (case, sorted(empty_rule ^ empty_rect))


def test_empty_tiles_of_the_benchmark_geometry(afv):
    """640 x 480, 8 levels, 1.2: 15 of the 512 tiles of a frame (150 + 117 + 77 + 54 + 40 + 35 + 24 + 15; they cover 512 * 2048 = 1 048 576 pixels) hold no
    reportable pixel - tile column 4 and tile row 6 of level 5 (257 x 193), tile row 5 of
    level 6 (214 x 161)"""
    tiles, wh = _tiles(afv, *F.FULL)
    assert wh.tolist() == [[640, 480], [533, 400], [444, 333], [370, 278], [309, 231], [257, 193], [214, 161], [179, 134]]
    empty = [tuple(t[:3]) for t in tiles.tolist() if t[7]]
    assert len(tiles) == 512 and len(empty) == 15
    assert sorted(empty) == sorted({(5, 4, ty) for ty in range(7)} | {(5, tx, 6) for tx in range(5)} | {(6, tx, 5) for tx in range(4)})
    per_level = [sum(1 for t in tiles.tolist() if t[0] == l) for l in range(8)]
    assert per_level == [150, 117, 77, 54, 40, 35, 24, 15]
    # the bottom tile rows that are cut short: reportable rows of 32
    cut = {l: int(t[6] - t[4]) for t in tiles.tolist() for l in [t[0]] if not t[7] and t[2] == (wh[l][1] + 31) // 32 - 1 and t[6] - t[4] < 32}
    assert cut == {0: 29, 1: 13, 2: 10, 3: 19, 4: 4, 7: 3}
    cols = {l: int(t[5] - t[3]) for t in tiles.tolist() for l in [t[0]] if not t[7] and t[1] == (wh[l][0] + 63) // 64 - 1 and t[5] - t[3] < 64}
    assert cols == {0: 61, 1: 18, 2: 57, 3: 47, 4: 50, 6: 19, 7: 48}


def test_cases_reach_every_branch(afv):
    """between them the small geometries hold: a last tile column and a last tile row without a reportable pixel, exactly one reportable column, exactly
    one reportable row, last tile columns 18, 33, 34 and 35 wide, a narrow tile that is also a cut bottom tile, and bottom tiles in which 1, 2 and 3 of
    the 4 wavefronts skip the pre-test and the NMS"""
    seen_cols, seen_rows, pre, nms, narrow_bottom, empty_col, empty_row = set(), set(), set(), set(), False, False, False
    for w, h, nlevels in F.CASES:
        tiles, wh = _tiles(afv, w, h, nlevels)
        for l, tx, ty, x0, y0, x1, y1, empty, row_hi, g_last, pre_idle, nms_idle in tiles.tolist():
            last_col, last_row = tx == (wh[l][0] + 63) // 64 - 1, ty == (wh[l][1] + 31) // 32 - 1
            if empty:
                empty_col |= bool(last_col and x1 <= x0)
                empty_row |= bool(last_row and y1 <= y0)
                continue
            if last_col:
                seen_cols.add(x1 - x0)
            if last_row:
                seen_rows.add(y1 - y0)
            narrow_bottom |= bool(last_col and last_row and x1 - x0 <= 18 and y1 - y0 < 32)
            pre.add(bin(pre_idle).count("1"))
            nms.add(bin(nms_idle).count("1"))
    assert empty_col and empty_row and narrow_bottom
    assert seen_cols >= {1, 18, 33, 34, 35} and seen_rows >= {1, 3, 5, 10, 23}
    assert pre >= {0, 1, 2, 3} and nms >= {0, 1, 2, 3}


@pytest.mark.parametrize("case", F.CASES)
def test_scenes_hold_their_border_facts(case):
    """in the restatement's candidates of level 0: every designed pixel on the last scored line is kept with its score, none on the first unscored line
    appears (nor a pixel tied with its neighbour), and the scene is dense - corners in every tile that has a reportable pixel"""
    w, h, nlevels = case
    lines = set()
    for variant in (0, 1):
        img, facts = F.scene(w, h, variant)
        lines |= facts["lines"]
        ref = F.reference(w, h, nlevels, variant)
        at = {(x, y): s for x, y, s in ref[0]}
        for x, y, s in facts["kept"]:
            assert at.get((x, y)) == s and (x in (3, w - 4) or y in (3, h - 4)), (case, variant, x, y)
        for x, y in facts["nothing"]:
            assert (x, y) not in at, (case, variant, x, y)
        assert all(3 <= x < w - 3 and 3 <= y < h - 3 for x, y in at)
    assert lines == {(s, q) for s in ("top", "bottom", "left", "right") for q in (2, 3)}, "between them the two variants put a pixel on both lines of every side"
    lw, lh, _ = R.level_geometry(w, h, nlevels, F.SCALE)
    for l in range(nlevels):
        both = F.reference(w, h, nlevels, 0)[l] | F.reference(w, h, nlevels, 1)[l]
        for tx, ty in F.tiles_of(lw[l], lh[l]):
            rect = F.reportable(lw[l], lh[l], tx, ty)
            if rect is not None and (rect[2] - rect[0]) * (rect[3] - rect[1]) >= 64:
                assert any(rect[0] <= x < rect[2] and rect[1] <= y < rect[3] for x, y, _ in both), (case, l, tx, ty)
