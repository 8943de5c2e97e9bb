"""-m gpu: AKAZE61 at ragged tiles, at the extractor's size limits, on the edge scenes of tests/_akaze_scenes.py and through one context
that sees many frame shapes.  HIP against the oracle (oracle/akaze.c) bit for bit, stage by stage (kcontrast, the five planes of every
level, candidates per level, keypoints, features), fused and step by step; HIP against the float64 restatement (tests/_akaze_f64.py)
within the bounds that tests/test_oracle_akaze_f64.py measures the oracle against.  Every case runs through both suppression engines."""
import ctypes as C

import numpy as np
import pytest

import _akaze_scenes as SC
import _akaze_shapes as SH
from test_gpu_akaze import _oracle_plan, akz, suppress_engine  # noqa: F401  (fixtures: both suppression engines, the oracle binding)

pytestmark = pytest.mark.gpu

PLANES = (("Lt", 0), ("Lsmooth", 1), ("Lx", 2), ("Ly", 3), ("Ldet", 4))
_ORACLE = {}  # oracle results per frame (the two engine runs of a case see the same frame)


def _oracle_all(akz, oracle, op, frame, quotas):
    """every stage of the oracle for one frame, with the product's plan (sizes, FED steps, taps) and quotas"""
    key = (frame.shape, frame.tobytes(), tuple(int(q) for q in quotas[:op.nlevels]))
    if key in _ORACLE:
        return _ORACLE[key]
    h, w = frame.shape
    levels, k0 = akz.full_evolution(frame, op)
    cands = [akz.level_candidates(op, i, levels[i]["Ldet"]) for i in range(op.nlevels)]
    kp = akz.subpixel(op, levels, akz.find_extrema(op, levels))
    chosen = []
    for lvl in range(op.nlevels):
        idx = np.nonzero(kp["class_id"] == lvl)[0]
        if len(idx):
            chosen.append(idx[oracle.quadtree(kp["x"][idx], kp["y"][idx], kp["response"][idx], int(quotas[lvl]), w, h, tiebreak=np.arange(len(idx)))])
    chosen = np.concatenate(chosen) if chosen else np.zeros(0, np.int64)
    fk, fd = akz.compute_descriptors(op, levels, kp[chosen])
    out = dict(levels=levels, k0=k0, cands=cands, kp=kp, fk=fk, fd=fd)
    _ORACLE[key] = out
    return out


def _check_features(gk, gd, want, what):
    assert len(gk) == len(want["fk"]), (what, len(gk), len(want["fk"]))
    assert gk.tobytes() == want["fk"].tobytes(), what          # keypoints incl. the angle bits
    assert np.array_equal(gd, want["fd"]), what                 # 61-byte descriptors


def _check_stages(afv, akz, oracle, ctx, frame, what):
    """extract on ctx, fused and then step by step; every stage against the oracle.  Returns the oracle record."""
    h, w = frame.shape
    want = None
    for step in (False, True):
        ctx.set_step_by_step(step)
        gk, gd = ctx.extract(frame)
        plan = ctx.plan
        assert (plan.w, plan.h) == (w, h)
        op = _oracle_plan(akz, plan)
        want = _oracle_all(akz, oracle, op, frame, ctx.quotas())
        tag = (what, "step" if step else "fused")
        assert ctx.kcontrast(0) == np.float32(want["k0"]), tag
        for i in range(plan.nlevels):
            for name, which in PLANES:
                assert np.array_equal(ctx.plane(0, i, which), want["levels"][i][name]), tag + (i, name)
        for i in range(plan.nlevels):
            assert np.array_equal(ctx.candidates(0, i), want["cands"][i]), tag + (i, "candidates")
        assert ctx.keypoints(0).tobytes() == want["kp"].tobytes(), tag + ("keypoints",)
        _check_features(gk, gd, want, tag)
    ctx.set_step_by_step(False)
    return want


def test_plans_match_the_oracle_at_every_size(afv, akz):
    prm = afv.akaze.default_params()
    for (w, h) in SH.SIZES + [SH.FIRST_REFUSED]:
        a, b = afv.akaze.plan_for(prm, w, h), akz.make_plan(w, h)
        assert C.string_at(C.addressof(a), C.sizeof(a)) == C.string_at(C.addressof(b), C.sizeof(b)), (w, h)


@pytest.mark.parametrize("wh", SH.SIZES, ids=SH.size_id)
def test_ragged_sizes_match_oracle(afv, akz, oracle, wh):
    w, h = wh
    ctx = afv.AkazeContext(afv.akaze.default_params(max_width=w, max_height=h, max_batch=1))
    frame = afv.synth.corners_frame(40 + w % 7, w, h)
    want = _check_stages(afv, akz, oracle, ctx, frame, wh)
    # below about 60 rows the descriptor margin (29 pixels at sigma_size 2) leaves no candidate: there the candidate, keypoint and feature
    # comparisons compare empty lists, and only the scale-space stages are tested at that size
    if min(w, h) >= 100:
        assert len(want["kp"]) > 0, "the frame gives the detector nothing to compare"
    ctx.close()


@pytest.mark.parametrize("name", SC.NAMES)
def test_scenes_match_oracle(afv, akz, oracle, name):
    frame = SC.scene(name)
    h, w = frame.shape
    ctx = afv.AkazeContext(afv.akaze.default_params(max_width=w, max_height=h, max_batch=1))
    _check_stages(afv, akz, oracle, ctx, frame, name)
    ctx.close()


@pytest.mark.parametrize("name", SC.NAMES + ["ragged"])
def test_hip_within_float64_bounds(afv, akz, name):
    """the HIP planes and kcontrast against the float64 restatement, with the bounds the oracle is held to on the CPU"""
    import _akaze_f64 as F
    frame = SC.scene(name) if name != "ragged" else afv.synth.corners_frame(7, 206, 110)
    h, w = frame.shape
    ctx = afv.AkazeContext(afv.akaze.default_params(max_width=w, max_height=h, max_batch=1))
    fk, fd = ctx.extract(frame)
    plan = ctx.plan
    op = _oracle_plan(akz, plan)
    got = [{n: ctx.plane(0, i, which) for n, which in PLANES} for i in range(plan.nlevels)]
    F.check_against_f64(frame, op, got, ctx.kcontrast(0))
    # detection and descriptors: HIP candidates and keypoints (the unrefined list is the oracle's suppression on the HIP planes), HIP
    # angles and descriptors, against the float64 detection / orientation / MLDB wherever the float64 margin exceeds the bound
    ref = F.scale_space(frame, op, k0=np.float32(ctx.kcontrast(0)))
    cands = [ctx.candidates(0, i) for i in range(plan.nlevels)]
    d_cmp, d_exc = F.check_detection_f64(frame, op, ref, cands, akz.find_extrema(op, got), ctx.keypoints(0))
    a_cmp, a_exc, a_tie, b_cmp, b_exc = F.check_descriptors_f64(op, ref, fk, fd)
    assert d_exc <= 0.02 * max(d_cmp, 1)
    print("%s: detection %d / %d excluded, angles %d / %d, bits %d / %d" % (name, d_cmp, d_exc, a_cmp, a_exc, b_cmp, b_exc))
    ctx.close()


def test_one_context_many_shapes(afv, akz, oracle):
    """a context made for 1280 x 720 extracts large -> small -> large frames and a strided view: each result is the oracle's for that frame
    alone and what a fresh context returns (buffers sized for the largest frame hold stale data past a smaller frame's width)"""
    W, H = SH.CONFIG5
    prm = afv.akaze.default_params(max_width=W, max_height=H, max_batch=1)
    ctx = afv.AkazeContext(prm)
    seq = [afv.synth.corners_frame(12, W, H), afv.synth.corners_frame(13, 193, 64), afv.synth.corners_frame(14, 382, 104),
           afv.synth.corners_frame(15, W, H)]
    for i, frame in enumerate(seq):
        h, w = frame.shape
        gk, gd = ctx.extract(frame)
        op = _oracle_plan(akz, ctx.plan)
        want = _oracle_all(akz, oracle, op, frame, ctx.quotas())
        _check_features(gk, gd, want, (i, w, h))
        if w * h < W * H:   # the planes of a small frame after a large one: nothing stale leaks in
            for lvl in range(ctx.plan.nlevels):
                for name, which in PLANES:
                    assert np.array_equal(ctx.plane(0, lvl, which), want["levels"][lvl][name]), (i, lvl, name)
        fresh = afv.AkazeContext(afv.akaze.default_params(max_width=w, max_height=h, max_batch=1))
        fk, fd = fresh.extract(frame)
        fresh.close()
        assert fk.tobytes() == gk.tobytes() and np.array_equal(fd, gd), (i, "fresh context")
    # a strided view (stride > w) of a small frame, after the large one
    frame = seq[2]
    h, w = frame.shape
    big = np.full((h + 6, w + 37), 255, np.uint8)
    big[3:3 + h, 5:5 + w] = frame
    roi = big[3:3 + h, 5:5 + w]
    cap = prm.nfeatures + 3 * 16
    kps = np.zeros(cap, afv.KP_DTYPE); desc = np.zeros((cap, 61), np.uint8); n = np.zeros(1, np.int32)
    rc = ctx.lib.afv_akaze_extract(ctx.handle, roi.ctypes.data, 1, w, h, big.strides[0], 0, kps.ctypes.data, desc.ctypes.data, cap, n.ctypes.data)
    assert rc == 0
    want = _oracle_all(akz, oracle, _oracle_plan(akz, afv.akaze.plan_for(prm, w, h)), frame, ctx.quotas())
    _check_features(kps[:n[0]], desc[:n[0]], want, "strided")
    ctx.close()


def test_widest_level_and_first_refused_width(afv, akz, oracle):
    """2048 columns fill the 32 mask chunks of the candidate kernels and are extracted; one more column is refused with
    AFV_EUNSUPPORTED, not answered"""
    from importlib import import_module
    lib = import_module("anyfeature-vslam_amd")._lib
    w, h = SH.WIDEST
    ctx = afv.AkazeContext(afv.akaze.default_params(max_width=w + 2, max_height=h, max_batch=1))
    frame = afv.synth.corners_frame(16, w, h)
    gk, gd = ctx.extract(frame)
    want = _oracle_all(akz, oracle, _oracle_plan(akz, ctx.plan), frame, ctx.quotas())
    _check_features(gk, gd, want, SH.WIDEST)
    assert len(gk) > 100
    rw, rh = SH.FIRST_REFUSED
    bad = afv.synth.corners_frame(17, rw, rh)
    ctx.scale_space(bad)
    assert ctx.lib.afv_akaze_detect(ctx.handle) == lib.EUNSUPPORTED   # the check that pins the 2048-column limit (see _akaze_shapes.py)
    cap = 1064
    kps = np.zeros(cap, afv.KP_DTYPE); desc = np.zeros((cap, 61), np.uint8); n = np.full(1, -1, np.int32)
    rc = ctx.lib.afv_akaze_extract(ctx.handle, bad.ctypes.data, 1, rw, rh, rw, 0, kps.ctypes.data, desc.ctypes.data, cap, n.ctypes.data)
    assert rc == lib.EUNSUPPORTED
    # the context still works after the refusal
    gk2, gd2 = ctx.extract(frame)
    assert gk2.tobytes() == gk.tobytes() and np.array_equal(gd2, gd)
    ctx.close()
