"""CPU: the frame sizes of tests/_akaze_shapes.py cover every tile tail, and the scenes of tests/_akaze_scenes.py reach the branches
they exist for, read off the oracle's stage functions (oracle/akaze.c).  Without these checks a change to a generator, a tile constant or
the oracle could leave tests/test_gpu_akaze_edges.py green without testing anything."""
import numpy as np
import pytest

import _akaze_f64 as F
import _akaze_scenes as SC
import _akaze_shapes as SH


@pytest.fixture(scope="module")
def akz():
    from oracle import akaze_binding
    return akaze_binding


def test_shape_list_covers_every_tail(akz):
    plans = [akz.make_plan(w, h) for (w, h) in SH.SIZES]
    for (w, h), p in zip(SH.SIZES, plans):
        assert SH.accepted(p), (w, h)
    want = SH.wanted(plans)
    got = set().union(*[SH.tails(p) for p in plans])
    assert want - got == set(), sorted(want - got)
    fams = {f for f, _, _, _ in want}
    assert {"tile64x32", "cand_mask", "halfsample"} <= fams
    assert {"fed_gauss<%d>" % n for n in range(3, 8)} <= fams and {"dhess<%d>" % s for s in range(2, 5)} <= fams
    # the named limits
    assert SH.SMALLEST == (SH.MIN_W, SH.MIN_H)
    assert akz.make_plan(*SH.ONE_OCTAVE).nlevels == 4 and SH.ONE_OCTAVE[0] < 2 * SH.MIN_W
    assert akz.make_plan(*SH.WIDEST).lv[0].w == SH.MAX_LEVEL_W and akz.make_plan(*SH.WIDEST).nlevels == 8
    assert SH.FIRST_REFUSED[0] == SH.MAX_LEVEL_W + 1 and not SH.accepted(akz.make_plan(*SH.FIRST_REFUSED))
    assert SH.CONFIG5 in SH.SIZES


def _evolve(akz, name):
    f = SC.scene(name)
    h, w = f.shape
    p = akz.make_plan(w, h)
    lv, k0 = akz.full_evolution(f, p)
    return f, p, lv, k0


def _raw_maxima(ldet, th=0.0005):
    """strict 3 x 3 maxima above the threshold, before the descriptor-border test"""
    c = ldet[1:-1, 1:-1]
    m = c > th
    for dy in range(3):
        for dx in range(3):
            if (dy, dx) != (1, 1):
                m &= c > ldet[dy:dy + c.shape[0], dx:dx + c.shape[1]]
    ys, xs = np.nonzero(m)
    return set(zip((ys + 1).tolist(), (xs + 1).tolist()))


def _border_stats(akz, p, lv, level):
    L = p.lv[level]
    cand = {(int(v) // L.w, int(v) % L.w) for v in akz.level_candidates(p, level, lv[level]["Ldet"])}
    dropped = _raw_maxima(lv[level]["Ldet"]) - cand
    M = SC.MARGIN[L.sigma_size]
    dist = lambda q: min(q[1], L.w - 1 - q[1], q[0], L.h - 1 - q[0])
    return sum(dist(q) == M - 1 for q in dropped), sum(dist(q) == M for q in cand), sum(dist(q) < M - 1 for q in dropped)


def test_border_scene_straddles_the_descriptor_margin(akz):
    """maxima one pixel outside the margin are dropped and maxima on it are kept, at octave 0 and at octave 1"""
    _, p, lv, _ = _evolve(akz, "border")
    out0, in0, _ = _border_stats(akz, p, lv, 0)
    assert out0 > 0 and in0 > 0, (out0, in0)
    _, in1, _ = _border_stats(akz, p, lv, 4)
    assert in1 > 0
    _, pm, lvm, _ = _evolve(akz, "mirror")
    out1, in1m, _ = _border_stats(akz, pm, lvm, 4)
    assert out1 > 0 and in1m > 0
    # the margin constant is the oracle's rule: no kept candidate is closer to the border than MARGIN
    for i in range(p.nlevels):
        L = p.lv[i]
        for v in akz.level_candidates(p, i, lv[i]["Ldet"]):
            y, x = divmod(int(v), L.w)
            assert min(x, L.w - 1 - x, y, L.h - 1 - y) >= SC.MARGIN[L.sigma_size], (i, x, y)


def test_mirror_scene_has_bit_equal_responses(akz):
    """both sides of the axis: bit-equal Ldet at every level, so every candidate has a partner with exactly its response"""
    f, p, lv, _ = _evolve(akz, "mirror")
    assert np.array_equal(f, f[:, ::-1])
    pairs = 0
    for i in range(p.nlevels):
        L = p.lv[i]
        d = lv[i]["Ldet"]
        assert np.array_equal(d, d[:, ::-1]), i          # the chain is exactly mirror symmetric
        c = akz.level_candidates(p, i, d)
        ys, xs = np.divmod(c, L.w)
        mirrored = np.sort(ys * L.w + (L.w - 1 - xs))
        assert np.array_equal(np.sort(c), mirrored), i   # the candidate set is its own mirror image
        pairs += int(np.count_nonzero(L.w - 1 - xs > xs))
    assert pairs > 500
    kp = akz.find_extrema(p, lv)
    assert len(kp) > 100


@pytest.mark.parametrize("name", ["constant", "saturated"])
def test_flat_scenes_take_the_contrast_fallback(akz, name):
    f, p, lv, k0 = _evolve(akz, name)
    assert F.kcontrast(np.asarray(f, np.float64) / 255.0)[2] == 0.0     # hmax == 0
    assert np.float32(k0) == np.float32(0.03)
    assert len(akz.find_extrema(p, lv)) == 0


def test_two_level_scene_puts_the_percentile_on_a_bin_boundary(akz):
    """the 70th percentile lands on magnitudes that are exactly hmax / 2 (a bin boundary: 300 * m / hmax == 150 exactly), so the
    contrast factor is hmax * 151 / 300; the magnitudes equal to hmax reach bin nbins and are folded into the last bin"""
    f, p, lv, k0 = _evolve(akz, "two_level")
    k64, m, hmax = F.kcontrast(np.asarray(f, np.float64) / 255.0)
    nz = np.sort(m[m != 0])
    nth = int(len(nz) * 0.7)
    assert nz[nth - 1] == hmax / 2 and np.count_nonzero(nz == hmax / 2) > 100    # the nth magnitude sits exactly on the boundary
    assert np.count_nonzero(nz == hmax) > 100                                      # the fold nbins -> nbins - 1
    assert k64 == hmax * 151 / 300
    assert abs(k0 - k64) <= F.BOUND_KCONTRAST * hmax, (k0, k64)                    # the oracle takes the same bin


def _flat_mask(lv, level):
    d = lv[level]
    lt = d["Lt"]
    vals, counts = np.unique(lt, return_counts=True)
    return (d["Lx"] == 0) & (d["Ly"] == 0) & (lt == vals[np.argmax(counts)])


def test_plateau_scene_has_descriptor_cells_on_exactly_flat_planes(akz):
    """cells of the MLDB grids that sample only exactly flat pixels (constant Lt, Lx == Ly == 0) average to bit-equal values: their bits
    are 0 both ways, and the oracle's descriptors show it"""
    f, p, lv, _ = _evolve(akz, "plateau")
    kp, desc = akz.compute_descriptors(p, lv, akz.subpixel(p, lv, akz.find_extrema(p, lv)))
    assert len(kp) >= 4
    flat_pairs = 0
    for k, d in zip(kp, desc):
        L = p.lv[k["class_id"]]
        mask = _flat_mask(lv, k["class_id"])
        r = float(1 << L.octave)
        sc = float(int(0.5 * k["size"] / r + 0.5))
        xf, yf, co, si = k["x"] / r, k["y"] / r, np.cos(k["angle"]), np.sin(k["angle"])
        bits = np.unpackbits(d, bitorder="little")
        dpos = 0
        for step in (10, 7, 5):      # the 2 x 2, 3 x 3 and 4 x 4 grids of MLDB
            flat = []
            for i0 in range(-10, 10, step):
                for j0 in range(-10, 10, step):
                    kk, ll = np.meshgrid(np.arange(i0, i0 + step), np.arange(j0, j0 + step), indexing="ij")
                    sy = yf + (ll * co * sc + kk * si * sc)
                    sx = xf + (-ll * si * sc + kk * co * sc)
                    ok = True
                    for ddx in (-1, 0, 1):   # one pixel of slack around every sample: float64 positions, float32 rounding
                        for ddy in (-1, 0, 1):
                            qx = np.clip(np.trunc(sx + 0.5).astype(int) + ddx, 0, L.w - 1)
                            qy = np.clip(np.trunc(sy + 0.5).astype(int) + ddy, 0, L.h - 1)
                            ok &= bool(mask[qy, qx].all())
                    flat.append(ok)
            n = len(flat)
            for c in range(3):
                for i in range(n):
                    for j in range(i + 1, n):
                        if flat[i] and flat[j]:
                            assert bits[dpos] == 0, (float(k["x"]), float(k["y"]), step, c, i, j)
                            flat_pairs += 1
                        dpos += 1
    assert flat_pairs >= 30, flat_pairs


def test_symmetric_scene_ties_orientation_windows(akz):
    """isotropic blobs: windows with different samples reach the largest |sum|^2 to within rounding for most keypoints"""
    f, p, lv, k0 = _evolve(akz, "symmetric")
    kp = akz.subpixel(p, lv, akz.find_extrema(p, lv))
    assert len(kp) >= 6
    ref = F.scale_space(f, p, k0=np.float32(k0))
    ties = 0
    for k in kp:
        L = p.lv[k["class_id"]]
        r = float(1 << L.octave)
        s = int(np.floor(0.5 * float(k["size"]) / r + 0.5))
        P = ref[k["class_id"]]
        ties += F.orientation(P["Lx"], P["Ly"], float(k["x"]) / r, float(k["y"]) / r, s)[2]
    assert ties >= 3, ties
