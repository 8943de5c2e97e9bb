"""-m gpu: k_describe stages and row-filters only the part of a keypoint's patch that a BRIEF test can reach (csrc/k_describe.hip, the reach
tables); whatever it leaves out keeps stale LDS bytes.  On a noise image a stale byte read as a filtered value changes a descriptor bit with
near certainty, so descriptors equal to the oracle's, byte for byte, at every angle and patch alignment say that nothing stale is read.
Bar: 0 mismatching descriptors."""
import numpy as np
import pytest

import _describe_reach as D

pytestmark = pytest.mark.gpu

W, H, NLEVELS = 160, 120, 4


@pytest.fixture(scope="module")
def ctx(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context(nlevels=NLEVELS, max_width=W, max_height=H, max_batch=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def img(afv):
    return np.ascontiguousarray(afv.synth.noise_frame(29, W, H))


def _angles():
    _, rim, rim_angles = D.sweep()
    assert rim.sum() == 64 and len(rim_angles) == 64
    return [float(d) for d in range(360)] + rim_angles


def _centres(lw, lh):
    """(cx, cy, interior) in level coordinates.  The kernel's interior rule: the 43 rows and the twelve aligned dwords of every patch row lie
    inside the level (cx >= 21, cx + 27 <= lw, cy >= 21, cy + 22 <= lh)"""
    mx, my = 40, 40
    c = [(x, my) for x in (40, 41, 42, 43)]                              # patch alignment (cx - 21) & 3 = 3, 0, 1, 2
    c += [(x, my) for x in (20, 21, 22)] + [(x, my) for x in (lw - 21, lw - 22, lw - 26, lw - 27)]
    c += [(mx, y) for y in (20, 21, 22)] + [(mx, y) for y in (lh - 21, lh - 22)]
    c += [(21, 21), (lw - 27, lh - 22), (22, lh - 22), (lw - 27, 21)]    # the four interior corners, alignments 0, 0 / 1 / 2 / 3 by level width
    return [(x, y, x >= 21 and x + 27 <= lw and y >= 21 and y + 22 <= lh) for x, y in c]


def _keypoints(afv, geo):
    angles = _angles()
    rows, interior, aligns = [], 0, set()
    for l in (0, NLEVELS - 1):
        lw, lh, scale = geo["lw"][l], geo["lh"][l], np.float32(geo["lscale"][l])
        assert lw >= 70 and lh >= 64, "room for interior patches on the top level"
        inv = np.float32(1) / scale
        for cx, cy, inside in _centres(lw, lh):
            x, y = np.float32(cx * scale), np.float32(cy * scale)
            assert np.rint(np.float32(x * inv)) == cx and np.rint(np.float32(y * inv)) == cy
            for ang in angles:
                rows.append((x, y, 31.0 * scale, ang, 0.0, l, -1))
            if inside:
                interior += 1
                aligns.add((l, (cx - 21) & 3))
    assert aligns == {(l, a) for l in (0, NLEVELS - 1) for a in range(4)}, "every patch alignment on both levels"
    assert interior >= 16
    return np.array(rows, afv._lib.KP_DTYPE)


def test_given_keypoints_at_every_angle_and_alignment(ctx, oracle, afv, img):
    """afv_orb_compute against afvo_orb_compute: octaves 0 and the top level; the four alignments px0 & 3; interior centres and centres 20, 21
    and 22 px from each edge and on both sides of the right-hand interior / border switch (cx + 27 <= lw); every whole degree and the 64
    angles at which a sample lies on the rim of the reach set"""
    k = _keypoints(afv, ctx.geometry())
    want = oracle.orb_compute(img, k, oracle.default_params(nlevels=NLEVELS))
    got = ctx.compute(img, k)
    bad = np.nonzero((got != want).any(1))[0]
    print("describe reach: %d keypoints, %d mismatching descriptors" % (len(k), len(bad)))
    assert len(bad) == 0, [(int(i), k[i].tolist()) for i in bad[:8]]
    # the noise does what it is there for: neighbouring angles give different descriptors
    assert len(np.unique(want, axis=0)) > len(want) // 2


def test_extraction_on_the_same_image(ctx, oracle, img):
    """the normal path (the kernel finds the angle itself) against the oracle, keypoints and descriptors"""
    k, d = ctx.extract(img)
    ok, od = oracle.orb_extract(img, oracle.default_params(nlevels=NLEVELS))
    assert len(k) == len(ok) and len(k) > 200
    for f in ("x", "y", "angle", "octave"):
        assert np.array_equal(k[f], ok[f]), f
    bad = np.nonzero((d != od).any(1))[0]
    print("describe reach: %d extracted keypoints, %d mismatching descriptors" % (len(k), len(bad)))
    assert len(bad) == 0, bad[:8].tolist()
