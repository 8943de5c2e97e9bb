"""-m gpu: k_fast_nms on levels whose last tile column / row holds few reportable pixels or none (tests/_fast_ragged.py), candidate sets of every level as
sets of (x, y, score) against the plain restatement tests/_detect_ref.py

The kernel leaves a tile without a reportable pixel at once and, in a bottom tile, lets the wavefronts past the last reportable row skip the pre-test and the
NMS.  Each geometry runs two dense scenes with designed pixels on the last scored and the first unscored line of every side; every scene is extracted by a
context that has just extracted a noise frame of the same size (whatever the workgroups of that call left in LDS must not show) and by a fresh one.
tests/test_fast_ragged_cpu.py proves that the geometries reach every branch and that the scenes hold their facts."""
import numpy as np
import pytest

import _fast_ragged as F

pytestmark = pytest.mark.gpu


def _candidates(ctx, frame, nlevels):
    out = []
    for l in range(nlevels):
        x, y, s, _ = ctx.debug_candidates(frame, l)
        got = list(zip(x.tolist(), y.tolist(), s.tolist()))
        assert len(set(got)) == len(got), ("a candidate twice", l)
        out.append(set(got))
    return out


def _check(got, want, facts, what):
    for l, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, "level", l, sorted(g ^ w)[:8])
    at = {(x, y): s for x, y, s in got[0]}
    for x, y, s in facts["kept"]:
        assert at.get((x, y)) == s, (what, "a pixel on the last scored line", x, y)
    for x, y in facts["nothing"]:
        assert (x, y) not in at, (what, "a pixel on the first unscored line", x, y)


@pytest.mark.parametrize("case", F.CASES)
def test_ragged_geometry(afv, case):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    w, h, nlevels = case
    used = afv.Context(nlevels=nlevels, scale_factor=F.SCALE, fast_threshold=F.T, max_width=w, max_height=h, max_batch=2)
    try:
        g = used.geometry()
        assert min(g["lw"] + g["lh"]) >= 32
        for variant in (0, 1):
            img, facts = F.scene(w, h, variant)
            want = F.reference(w, h, nlevels, variant)
            used.extract(F.noise(w, h))
            used.extract(img)
            _check(_candidates(used, 0, nlevels), want, facts, (case, variant, "after a noise frame"))
            fresh = afv.Context(nlevels=nlevels, scale_factor=F.SCALE, fast_threshold=F.T, max_width=w, max_height=h, max_batch=2)
            try:
                fresh.extract(img)
                _check(_candidates(fresh, 0, nlevels), want, facts, (case, variant, "fresh context"))
            finally:
                fresh.close()
    finally:
        used.close()


def test_benchmark_geometry_two_frames(afv):
    """640 x 480, 8 levels: 15 empty tiles and cut bottom tiles at levels 1, 2, 3, 4 and 7; two different frames in one call, after a call on two noise frames"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    w, h, nlevels = F.FULL
    frames = [F.scene(w, h, 0), F.scene(w, h, 1)]
    want = [F.reference(w, h, nlevels, v) for v in (0, 1)]
    used = afv.Context(nlevels=nlevels, scale_factor=F.SCALE, fast_threshold=F.T, max_width=w, max_height=h, max_batch=2)
    fresh = afv.Context(nlevels=nlevels, scale_factor=F.SCALE, fast_threshold=F.T, max_width=w, max_height=h, max_batch=2)
    try:
        used.extract_batch([F.noise(w, h), np.ascontiguousarray(F.noise(w, h)[::-1])])
        for ctx, what in ((used, "after noise frames"), (fresh, "fresh context")):
            ctx.extract_batch([f[0] for f in frames])
            for i in (0, 1):
                _check(_candidates(ctx, i, nlevels), want[i], frames[i][1], (what, "frame", i))
    finally:
        used.close()
        fresh.close()
