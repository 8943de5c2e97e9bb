"""Constructed scenes for the block-sparse global bundle adjustment (tests/_gba_ref.py, deviation L7'): the scenes of tests/_lba_scenes.py
(make, by import) with covisibility patterns chosen per rule.  The small ones have at most 12 free keyframes, so the dense restatement
solves them in seconds; tests/test_gba_ref_cpu.py proves that each reaches what it is named for.  The large ones lie past the old cap of
64 free keyframes and are held against the host program only; their sizes come from what the kernels stride over."""
import numpy as np

import _gba_ref as G
import _lba_scenes as S


def _solve(sc, log=None, stop_at="scene", solves=None):
    return G.bundle_adjust(sc.problem(), sc.iterations, sc.robust, sc.checks, sc.stop_at if stop_at == "scene" else stop_at, log, solves)


def _finish(sc):
    sc.solve_sparse = lambda **kw: _solve(sc, **kw)
    return sc


def band_views(n_free, fixed, npts, width):
    """point p is seen by `width` consecutive free keyframes (round robin over the starts) and by the fixed keyframes"""
    starts = max(n_free - width + 1, 1)
    return [sorted({(p % starts) + q for q in range(min(width, n_free))} | set(fixed)) for p in range(npts)]


def band(n_free=9, n_fixed=1, width=3, npts=54, seed=41, loop=0, **kw):
    """covisibility width `width`: block (i, j) is structural when |i - j| < width; loop: that many extra points seen by the first and the
    last free keyframe (fill)"""
    nk = n_free + n_fixed
    fixed = list(range(n_free, nk))
    views = band_views(n_free, fixed, npts, width) + [sorted({0, n_free - 1} | set(fixed))] * loop
    return _finish(S.make(nk=nk, nf=n_free, npts=npts + loop, seed=seed, views=views, **kw))


def hub(n_free, n_fixed=1, shared=1, own=6, seed=43, **kw):
    """keyframe 0 shares `shared` points with each other free keyframe (its column of L is full, the elimination makes L dense); every
    other keyframe also has `own` points that it shares with the fixed keyframes only"""
    nk = n_free + n_fixed
    fixed = list(range(n_free, nk))
    views = []
    for k in range(1, n_free):
        views += [sorted({0, k} | set(fixed))] * shared + [sorted({k} | set(fixed))] * own
    return _finish(S.make(nk=nk, nf=n_free, npts=len(views), seed=seed, views=views, **kw))


def small():
    """(name, scene) for each rule of L7'"""
    out = []
    out.append(("band", band()))
    ring = [sorted({k, k + 1, 12}) for k in range(11)] * 4 + [[0, 11, 12]] * 4
    out.append(("arrow_fill", _finish(S.make(nk=13, nf=12, npts=len(ring), seed=42, views=ring))))
    two = [[0, 1, 2, 3, 8]] * 14 + [[4, 5, 6, 7, 8]] * 14
    out.append(("two_components", _finish(S.make(nk=9, nf=8, npts=len(two), seed=44, views=two))))
    iso = [[0, 3]] * 3 + [[0, 1, 2, 4]] * 30
    out.append(("isolated_keyframe", _finish(S.make(nk=5, nf=4, npts=len(iso), seed=45, views=iso, dropped=(0, 1, 2)))))
    out.append(("first_is_hub", hub(10, shared=2, own=5)))
    # point 7 alone joins keyframes 1 and 4; its edge to keyframe 1 is a gross outlier that the first check removes
    pat = [[0, 1, 2, 6]] * 7 + [[1, 4, 5, 6]] +[[2, 3, 4, 5, 6]] * 12 + [[0, 1, 6]] * 6 + [[4, 5, 6]] * 6
    out.append(("pattern_empties", _finish(S.make(nk=7, nf=6, npts=len(pat), seed=46, views=pat, outliers=[(7, 1, 200.0)]))))
    bp = [[0, 1]] * 6 + [[1, 2]] * 6 + [[2, 3]] * 6
    out.append(("bad_pivot", _finish(S.make(nk=4, nf=4, npts=len(bp), seed=21, views=bp, checks=False, iterations=(20, 0), robust=(False, False),
                                            inf_scale={0: 1e10}))))
    out.append(("stop_in_first", band(seed=47, stop_at=2)))
    out.append(("startup_two_keyframes", _finish(S.make(nk=2, nf=1, npts=60, seed=8, iterations=(20, 0), robust=(False, False), checks=False,
                                                        shake=0.05))))
    out.append(("no_fixed_keyframe", band(n_free=6, n_fixed=0, width=3, npts=48, seed=48)))
    out.append(("mixed_mono_stereo", band(seed=49, stereo_kfs=(0, 2, 5, 9), outliers=[(3, 0, -30.0), (11, 5, 25.0)])))
    return out


FAILURE_SCENES = ("bad_pivot",)          # named for a failure: no accepted trial is asked of them
LOOP = dict(iterations=(10, 0), robust=(False, False), checks=False)   # the call of LoopClosing::RunGlobalBundleAdjustment


def large():
    """past the old cap: the device against the host program only.  8 to 12 points per keyframe: the scenes are about the pattern"""
    out = {}
    out["band_65"] = band(n_free=65, n_fixed=1, width=4, npts=65 * 9, seed=51, **LOOP)
    out["band_130"] = band(n_free=130, n_fixed=2, width=4, npts=130 * 9, seed=52, loop=3, **LOOP)
    # keyframe 0's column holds 180 sub-diagonal blocks: 1080 rows, more than the 1024 lanes of the factor workgroup, 16290 update pairs
    out["hub_180"] = hub(181, n_fixed=1, shared=8, own=2, seed=53, **LOOP)
    return out


def band_65_with_checks():
    return band(n_free=65, n_fixed=1, width=4, npts=65 * 9, seed=51)
