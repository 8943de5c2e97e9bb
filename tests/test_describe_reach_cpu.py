"""what k_describe stages and row-filters of a keypoint's patch (csrc/k_describe.hip: the reach tables, built at compile time from the BRIEF
pattern) against an angle sweep done here, without a GPU.  afv_debug_describe_reach returns the tables the library was compiled with: the
set R of positions a rotated test can land on, the (pair-row, dword group) items of the row pass and the staged dwords, per patch alignment
a = px0 & 3, in the order of the kernel's schedule.  The sweep rotates every pattern point in 0.01 degree steps with fp32 products, one
rounding per operator, and rounds half to even - the kernel's arithmetic."""
import numpy as np
import pytest

import _describe_reach as D

PR, PS, REACH = 21, 43, D.REACH
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]   # the radius-15 disc of IC_Angle (orb.cpp), row |v| -> last column


def tables(afv):
    lib = afv._lib.load()
    R = np.zeros((37, 37), np.uint8)
    items = np.zeros((4, 192), np.uint16)
    dwords = np.zeros((4, 448), np.uint16)
    counts = np.zeros(8, np.int32)
    layout = np.zeros(8, np.int32)
    p = afv._lib.ptr
    assert lib.afv_debug_describe_reach(p(R), p(items), p(dwords), p(counts), p(layout)) == 0
    return R.astype(bool), items, dwords, counts, layout


@pytest.fixture(scope="module")
def swept():
    return D.sweep()


def test_reach_set_is_the_sweep(afv, swept):
    R, _, _, _, _ = tables(afv)
    Rs, rim, angles = swept
    assert Rs.sum() == 1124 and np.array_equal(R, Rs)
    assert rim.sum() == 64 and len(angles) == 64 and not (rim & ~Rs).any()


def test_row_items_hold_every_sampled_column(afv, swept):
    """a sample at (ix, iy) reads the plane rows 18 + iy .. 24 + iy of plane column 18 + a + ix, as the four pair-row dwords (18 + iy) >> 1 .. + 3"""
    _, items, _, counts, layout = tables(afv)
    Rs, _, _ = swept
    assert layout[0] == 3 and layout[6] in (0, 1)
    for a in range(4):
        n = int(counts[a])
        assert 128 < n <= 64 * layout[0]
        lst = items[a].tolist()
        assert lst[:n] == sorted(set(lst[:n])), "sorted by pair-row, no item twice"
        assert all(v == lst[n - 1] for v in lst[n:]), "padding repeats the last item"
        have = {(v >> 8, v & 255) for v in lst[:n]}
        assert all(j < 22 and g < 10 for j, g in have)
        for y, x in zip(*np.nonzero(Rs)):
            col = x + a   # = 18 + a + ix
            for r in range(y, y + 7):
                assert (r >> 1, col >> 2) in have, (a, x - REACH, y - REACH, r)
            assert ((y >> 1) + 3, col >> 2) in have, "the fourth dword is read whole, weight 0 or not"


def test_staged_dwords_hold_every_needed_byte(afv, swept):
    _, _, dwords, counts, layout = tables(afv)
    Rs, _, _ = swept
    assert layout[1] == 7
    H = np.zeros((PS, 37), bool)
    for y, x in zip(*np.nonzero(Rs)):
        H[y:y + 7, x] = True
    assert H.sum() == 1347
    for a in range(4):
        n = int(counts[4 + a])
        assert 0 < n <= 64 * layout[1]
        lst = dwords[a].tolist()
        assert lst[:n] == sorted(set(lst[:n])) and all(v == lst[n - 1] for v in lst[n:])
        have = {(v >> 8, v & 255) for v in lst[:n]}
        assert all(r < PS and q < 12 for r, q in have), "inside the twelve dwords of a patch row"
        for r, c in zip(*np.nonzero(H)):
            for k in range(7):   # H[r][xh] = taps over LDS bytes xh .. xh + 6, xh = c + a
                assert (r, (c + a + k) >> 2) in have, (a, r, c, k)
        for v in range(-15, 16):
            for u in range(-UMAX[abs(v)], UMAX[abs(v)] + 1):
                assert (PR + v, (PR + a + u) >> 2) in have, (a, u, v)


def test_row_pass_never_overwrites_a_patch_byte_it_still_needs(afv):
    """the plane overlays the patch: every plane byte stored in steps 0 .. k lies below the first patch byte loaded in step k + 1"""
    _, items, _, counts, layout = tables(afv)
    steps, p_off, pp, gp, slice_bytes = int(layout[0]), int(layout[2]), int(layout[3]), int(layout[4]), int(layout[5])
    assert p_off + PS * pp == slice_bytes and 22 * gp == slice_bytes
    for a in range(4):
        store_end = 0
        for k in range(steps):
            step = [(v >> 8, v & 255) for v in items[a][64 * k:64 * k + 64].tolist()]
            load_lo = min(p_off + 2 * j * pp + 4 * g for j, g in step)
            if k:
                assert store_end <= load_lo, (a, k, store_end, load_lo)
            store_end = max([store_end] + [j * gp + 16 * g + 16 for j, g in step])
            # the pair-row without an upper patch row: the kernel skips that row's loads in the last step only
            assert k == steps - 1 or all(j < 21 for j, _ in step)
            # nothing past the slice is read or written
            assert all(p_off + (2 * j + (1 if j < 21 else 0)) * pp + 4 * g + 12 <= slice_bytes and j * gp + 16 * g + 16 <= slice_bytes for j, g in step)
