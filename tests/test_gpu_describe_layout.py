"""-m gpu: the LDS layout of k_describe (row pass with a fixed lane mapping, row-filtered plane of interleaved row pairs, sample addresses taken
from the float bits) on one noise image, byte for byte against the CPU oracle

One LCG-noise image of 160 x 120 (second level 133 x 100), through compute (caller-given keypoints: k_describe_given) and through extract (k_describe).
The keypoints are the product of: patch origin (cx - 21) & 3 in 0..3 (the alignment of the staged patch inside its LDS rows), cy even and odd, octaves
0 and 1, the angles below, and six positions - interior, the patch leaving the level on each of the four sides, and a corner.  All of them go in one
launch; a second launch has a keypoint count that is no multiple of the keypoints per workgroup.

The plane is relative to the patch: a sample at rotated offset (ix, iy) reads plane rows yy .. yy + 6 with yy = 18 + iy, columns 18 + a + ix, so what
the layout puts at risk is reached through the ANGLES, and test_inputs_reach_the_layout_edges proves on the CPU, with the oracle's pattern and
sincos_deg, that the chosen angles reach it: the smallest and largest ix and iy a scan of all angles in 0.25 degree steps reaches (-18 and 18: plane
rows 0 and 42, the unpaired last row, and both ends of a plane row), both parities of yy, both parities among the samples whose four dwords start at
pair-row 0 (yy = 0 and 1), the samples that start at the last pair-row a sample can start at (18: yy = 36, which ends in pair-row 21 = (row 42, 0)) and
the last odd row (yy = 35).  yy = 37 would need an offset of 19, which no rotation of the pattern has (its largest radius is 18.38)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H = 160, 120
ANGLES = (0.0, 28.0, 35.0, 40.0, 90.0, 130.0, 180.0, 213.75, 270.0, 305.5, 359.75, -45.3)
KP_PER_BLOCK = 4  # AFV_KP_PER_BLOCK (csrc/afv_device.h)


def _lcg(seed, n):
    out = np.empty(n, np.int64)
    s = seed
    for i in range(n):
        s = (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out[i] = s >> 40
    return out


@functools.lru_cache(maxsize=None)
def _image():
    img = (_lcg(17, W * H) % 256).astype(np.uint8).reshape(H, W)
    img.setflags(write=False)
    return img


def _offsets(oracle, angle):
    """(ix, iy) of the 512 sample points under `angle`: the arithmetic of computeOrbDescriptor (one float32 rounding per operator, cvRound)"""
    pat = oracle.brief_pattern().astype(f32).reshape(-1, 2)
    c, s = (f32(v) for v in oracle.sincos_deg(angle))
    x, y = pat[:, 0], pat[:, 1]
    return np.rint(x * c - y * s).astype(np.int64), np.rint(x * s + y * c).astype(np.int64)


def _positions(w, h):
    """name -> base centre (cx, cy) on a level of w x h; cx + 0..3 and cy + 0..1 are used.  Interior: the 48 x 43 staged window lies inside the level
    (cx - 21 >= 0, cx + 27 <= w, cy - 21 >= 0, cy + 22 <= h)"""
    return {"interior": (44, 40), "left": (4, 40), "right": (w - 12, 40), "top": (44, 3), "bottom": (44, h - 9), "corner": (w - 8, h - 6)}


@functools.lru_cache(maxsize=None)
def _rows(oracle):
    """[(x, y, angle, octave)], [(position, cx, cy, octave, angle)]"""
    lw, lh, ls = oracle.level_geometry(W, H)
    rows, meta = [], []
    for l in (0, 1):
        s = f32(ls[l])
        for name, (bx, by) in _positions(int(lw[l]), int(lh[l])).items():
            for dx in range(4):
                for dy in range(2):
                    for a in ANGLES:
                        cx, cy = bx + dx, by + dy
                        rows.append((f32(cx) * s, f32(cy) * s, a, l))
                        meta.append((name, cx, cy, l, a))
    return rows, meta


def _keypoints(oracle, rows):
    k = np.zeros(len(rows), oracle.KP_DTYPE)
    for i, (x, y, a, l) in enumerate(rows):
        k[i] = (x, y, 31.0, a, 0.0, l, -1)
    return k


@functools.lru_cache(maxsize=None)
def _reference(oracle):
    """computed once, shared by the two launches"""
    rows, _ = _rows(oracle)
    kps = _keypoints(oracle, rows)
    want = oracle.orb_compute(_image(), kps)
    want.setflags(write=False)
    return kps, want


def test_inputs_reach_the_layout_edges(oracle):
    """conditions on the INPUTS, proved before any GPU call (the module is marked gpu as a whole; this test itself needs none)"""
    lo_x = hi_x = lo_y = hi_y = 0
    for a in np.arange(0.0, 360.0, 0.25):
        ix, iy = _offsets(oracle, float(a))
        lo_x, hi_x, lo_y, hi_y = min(lo_x, ix.min()), max(hi_x, ix.max()), min(lo_y, iy.min()), max(hi_y, iy.max())
    assert (lo_x, hi_x, lo_y, hi_y) == (-18, 18, -18, 18)  # what the patch of 43 = 2 (18 + 3) + 1 is sized for
    ix, iy = (np.concatenate(v) for v in zip(*[_offsets(oracle, a) for a in ANGLES]))
    assert (ix.min(), ix.max(), iy.min(), iy.max()) == (lo_x, hi_x, lo_y, hi_y)
    yy = 18 + iy  # first plane row of a sample; its four dwords start at pair-row yy >> 1
    assert yy.min() == 0 and yy.max() + 6 == 42  # plane row 0 and the unpaired last row
    assert set(np.unique(yy & 1)) == {0, 1}
    assert set(np.unique(yy[(yy >> 1) == 0])) == {0, 1}  # both parities at pair-row 0
    assert 36 in yy and 35 in yy  # pair-row 18 (the last a sample starts at: its fourth dword is the half-filled pair-row 21) and the last odd row
    # the keypoints: every (alignment, parity of cy, octave, position) under every angle, interior / border as named
    rows, meta = _rows(oracle)
    lw, lh, ls = oracle.level_geometry(W, H)
    assert (int(lw[1]), int(lh[1])) == (133, 100)
    seen = set()
    for (x, y, a, l), (name, cx, cy, ll, aa) in zip(rows, meta):
        inv = f32(1.0) / f32(ls[l])
        assert (int(np.rint(f32(x) * inv)), int(np.rint(f32(y) * inv))) == (cx, cy)  # the centre the kernel derives is the intended one
        w, h = int(lw[l]), int(lh[l])
        inside = cx - 21 >= 0 and cy - 21 >= 0 and cx + 27 <= w and cy + 22 <= h
        assert inside == (name == "interior"), (name, cx, cy, l)
        left, right, top, bottom = cx - 18 < 0, cx + 18 >= w, cy - 18 < 0, cy + 18 >= h  # the 37 x 37 sampled window leaves the level
        assert {"interior": not (left or right or top or bottom), "left": left and not (top or bottom), "right": right and not (top or bottom),
                "top": top and not (left or right), "bottom": bottom and not (left or right), "corner": right and bottom}[name], (name, cx, cy, l)
        seen.add(((cx - 21) & 3, cy & 1, l, name))
    assert len(seen) == 4 * 2 * 2 * 6 and len(rows) == len(seen) * len(ANGLES)
    assert len(rows) % KP_PER_BLOCK == 0 and (len(rows) - 1) % KP_PER_BLOCK != 0


@pytest.fixture(scope="module")
def ctx(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context(max_width=W, max_height=H, max_batch=1)
    yield c
    c.close()


def test_compute_whole_set_in_one_launch(ctx, oracle):
    kps, want = _reference(oracle)
    got = ctx.compute(_image(), kps)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (len(bad), [_rows(oracle)[1][i] for i in bad[:8]])


def test_compute_count_not_a_multiple_of_the_block(ctx, oracle):
    kps, want = _reference(oracle)
    n = len(kps) - 1
    got = ctx.compute(_image(), kps[:n])
    assert got.shape == (n, 32) and np.array_equal(got, want[:n]), np.flatnonzero((got != want[:n]).any(1))[:8]


def test_extract_keypoints_and_descriptors(ctx, oracle):
    okps, odesc = oracle.orb_extract(_image())
    kps, desc = ctx.extract(_image())
    assert len(okps) > 100 and {0, 1} <= set(okps["octave"].tolist())
    assert kps.tobytes() == okps.tobytes()
    assert np.array_equal(desc, odesc), np.flatnonzero((desc != odesc).any(1))[:8]
