"""-m gpu: k_pyramid.hip and k_fast.hip on the constructed scenes of tests/_detect_scenes.py, bit for bit against the CPU oracle

Same bar and the same checker as tests/test_gpu_desc_scenes.py - pyramid levels, candidate sets with integer scores, Harris float bits of the kept candidates,
selected positions, keypoint bytes, descriptors - on frames built for the front of the pipeline: designed corners of both polarities on every (x % 64, y % 32)
of a FAST tile, scores decided by one chosen ring pixel of one chosen window, rings that pass the pre-test and fail the arc test, NMS pairs, chains and blocks
inside tiles and over their seams and corners, pixels on the last scored and the first unscored line of levels whose last tile is 1 .. 64 px wide, the same
content at levels 1 and 2 of a 2.0 pyramid, and pyramids of extreme images, rounding ties, level ratios on both sides of every source-window limit and the
level steps where the order of evaluating the scale shows.  Every scene runs on the three kernel sets.  The expected values are the oracle's;
tests/test_detect_ref_cpu.py checks the oracle against a plain restatement on the same scenes and proves that every scene reaches its rule."""
import numpy as np
import pytest

import _detect_scenes as S

pytestmark = pytest.mark.gpu

MODES = {"auto": 1, "batch-kernels": 0, "small-batch-kernels": 2}
_traces = {}


def _oracle(oracle, img, nlevels=8, sf=1.2, t=20):
    key = (img.tobytes(), img.shape, nlevels, sf, t)
    if key not in _traces:
        _traces[key] = oracle.orb_extract_trace(img, oracle.default_params(nlevels=nlevels, scale_factor=sf, fast_threshold=t), cap=4000)
    return _traces[key]


_contexts = {}


@pytest.fixture(scope="module", params=list(MODES))
def mode(request):
    """the three kernel sets of tests/test_gpu_extract.py; the contexts of one set are closed before the next set starts"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    yield MODES[request.param]
    for c in _contexts.values():
        c.close()
    _contexts.clear()


def _ctx(afv, mode, w=640, h=480, nlevels=8, sf=1.2, t=20, batch=8):
    """one context per (kernel set, size, pyramid, threshold), kept while the kernel set is under test"""
    key = (mode, w, h, nlevels, sf, t, batch)
    if key not in _contexts:
        c = afv.Context(nlevels=nlevels, scale_factor=sf, fast_threshold=t, max_width=w, max_height=h, max_batch=batch)
        c.set_small_batch_path(mode)
        _contexts[key] = c
    return _contexts[key]


def _check_frame(ctx, frame, trace, kps, desc, what):
    """every stage of frame `frame` of the context's last call against the oracle's trace (tests/test_gpu_desc_scenes.py::_check_frame + the pyramid levels)"""
    okps, odesc, tr = trace
    o = 0
    for l in range(len(tr["lw"])):
        lv = ctx.debug_level(frame, l)
        assert np.array_equal(lv, tr["level"][l]), (what, "level", l, np.argwhere(lv != tr["level"][l])[:4] if lv.shape == tr["level"][l].shape else lv.shape)
        x, y, s, r = ctx.debug_candidates(frame, l)
        got = sorted(zip(y.tolist(), x.tolist(), s.tolist(), r.view(np.uint32).tolist()))
        m = tr["cand"]["level"] == l
        oc, keep1 = tr["cand"][m], tr["keep1"][m]
        want = sorted(zip(oc["y"].tolist(), oc["x"].tolist(), oc["fast_score"].tolist()))
        assert [g[:3] for g in got] == want, (what, "candidates", l, sorted(set(want) ^ {g[:3] for g in got})[:6])
        gmap = {(g[0], g[1]): g[3] for g in got}
        for c in oc[keep1]:
            assert gmap[(int(c["y"]), int(c["x"]))] == int(np.float32(c["response"]).view(np.uint32)), (what, l, c)
        sx, sy, sr = ctx.debug_selected(frame, l)
        n = tr["t_counts"][l]
        assert len(sx) == n, (what, l, len(sx), n)
        ok = okps[o:o + n]
        o += n
        ls = np.float32(tr["lscale"][l])
        assert np.array_equal(sx.astype(np.float32) * ls, ok["x"]) and np.array_equal(sy.astype(np.float32) * ls, ok["y"]), (what, l)
        assert np.array_equal(sr.view(np.uint32), ok["response"].view(np.uint32)), (what, l)
    assert o == len(okps)
    assert kps.tobytes() == okps.tobytes(), what
    assert np.array_equal(desc, odesc), (what, np.flatnonzero((desc != odesc).any(1))[:8])


def _run(afv, oracle, mode, img, what, nlevels=8, sf=1.2, t=20, size=None, entries=False, batch=8):
    """extract, stage by stage; with `entries` also detect + compute and afv.Frame.extract"""
    w, h = size or (img.shape[1], img.shape[0])
    ctx = _ctx(afv, mode, w, h, nlevels, sf, t, batch)
    trace = _oracle(oracle, img, nlevels, sf, t)
    kps, desc = ctx.extract(img)
    _check_frame(ctx, 0, trace, kps, desc, what)
    if entries:
        kd = ctx.detect(img)
        assert kd.tobytes() == trace[0].tobytes(), (what, "detect")
        assert np.array_equal(ctx.compute(img, kd), trace[1]), (what, "compute")
        fr = afv.Frame(ctx)
        try:
            k, d = fr.extract(img)
            assert k.tobytes() == trace[0].tobytes() and np.array_equal(d, trace[1]) and fr.N == len(trace[0]), (what, "Frame.extract")
        finally:
            fr.close()


# ---------------------------------------------------------------- FAST score, tile position, pre-test, NMS ----------------------------------------------------------------
@pytest.mark.parametrize("t", S.THRESHOLDS)
@pytest.mark.parametrize("f", range(S.SWEEP_FRAMES))
def test_tile_sweep(afv, oracle, mode, f, t):
    _run(afv, oracle, mode, S.tile_sweep(f)[0], "tile_sweep/%d t=%d" % (f, t), t=t, entries=t == 20)


def _generic(name, t):
    """the frames of a threshold-generic scene for a context with threshold t (the scene is built for min(t, 20): at 254 only its 0 / 255 motifs are corners)"""
    ts = min(t, 20)
    return {"score_network": lambda: S.score_network(ts), "pretest_traps": lambda: S.pretest_traps(ts), "nms_pairs": S.nms_pairs}[name]()


@pytest.mark.parametrize("t", S.THRESHOLDS)
@pytest.mark.parametrize("name", ["score_network", "pretest_traps", "nms_pairs"])
def test_fast_scene(afv, oracle, mode, name, t):
    for i, (img, _) in enumerate(_generic(name, t)):
        _run(afv, oracle, mode, img, "%s/%d t=%d" % (name, i, t), t=t, size=(320, 240), entries=t == 20)


@pytest.mark.parametrize("size", S.BORDER_SIZES)
def test_border(afv, oracle, mode, size):
    """one context per odd size; thresholds 1 and 20"""
    for t in (20, 1):
        for v in range(S.BORDER_VARIANTS):
            _run(afv, oracle, mode, S.border(size[0], size[1], v)[0], "border %s/%d t=%d" % (size, v, t), nlevels=S.BORDER_LEVELS, t=t, entries=v == 0 and t == 20)


@pytest.mark.parametrize("family", ["score_network", "nms_pairs", "border"])
def test_two_to_one(afv, oracle, mode, family):
    """the designed images at levels 1 and 2 of a 3-level 2.0 pyramid: k_fast_nms reads them from the pyramid buffer with the level's own pitch"""
    for name, (D, _, kind) in S.designed_images().items():
        if kind == family:
            img = S.two_to_one(D)
            _run(afv, oracle, mode, img, "two_to_one " + name, nlevels=S.TWO_LEVELS, sf=S.TWO_SCALE, size=(640, 480), entries=name.endswith("/0") and img.shape == (480, 640))


# ---------------------------------------------------------------- pyramid ----------------------------------------------------------------
@pytest.mark.parametrize("size", S.RESIZE_SIZES)
def test_resize_extremes(afv, oracle, mode, size):
    for name, img in S.resize_extremes(*size).items():
        _run(afv, oracle, mode, img, "resize_extremes %s %s" % (size, name), entries=name == "noise")


def test_resize_ties(afv, oracle, mode):
    for name, img, nlevels, sf in S.resize_ties():
        _run(afv, oracle, mode, img, "resize_ties " + name, nlevels=nlevels, sf=sf, size=(640, 480))


def test_ratio_limits(afv, oracle, mode):
    """level steps on both sides of the 88 x 44 / 96 x 48 and 96 x 48 / 160 x 80 window limits and just below the last one; a step beyond the last limit is
    refused when the context is created (AFV_EUNSUPPORTED from build_geometry), nothing is launched"""
    for w, h, sf, n, win in S.ratio_limits():
        if None in win:
            with pytest.raises(afv._lib.AfvError) as e:
                afv.Context(nlevels=n, scale_factor=sf, max_width=w, max_height=h)
            assert "unsupported" in str(e.value)
        else:
            _run(afv, oracle, mode, S.ratio_frame(w, h), "ratio_limits %s" % ((w, h, sf),), nlevels=n, sf=sf, entries=True)


def test_scale_evaluation(afv, oracle, mode):
    """the level steps where 1 / (dst / src) and src / dst give different taps (frames up to 2048 wide; the wider ones are held on the CPU only)"""
    for w, h, sf, n, src, dst in S.scale_scenes():
        if w <= S.SCALE_GPU_MAX_WIDTH:
            _run(afv, oracle, mode, S.scale_frame(w, h), "scale_evaluation %d -> %d" % (src, dst), nlevels=n, sf=sf, batch=1)


# ---------------------------------------------------------------- batches ----------------------------------------------------------------
def test_mixed_scene_batch(afv, oracle, mode):
    """six different scenes in a single call"""
    frames = [S.score_network(20)[0][0], S.pretest_traps(20)[0][0], S.nms_pairs()[0][0], S.nms_pairs()[1][0], S.score_network(7)[0][0], S.pretest_traps(1)[0][0]]
    ctx = _ctx(afv, mode, 320, 240)
    res = ctx.extract_batch(frames)
    assert len(res) == 6
    for i, (f, (k, d)) in enumerate(zip(frames, res)):
        _check_frame(ctx, i, _oracle(oracle, f), k, d, "mixed batch %d" % i)


def test_same_frame_at_two_batch_indices(afv, oracle, mode):
    a, b = S.tile_sweep(0)[0], S.tile_sweep(3)[0]
    frames = [a, b, a, S.tile_sweep(1)[0]]
    ctx = _ctx(afv, mode)
    res = ctx.extract_batch(frames)
    for i, (f, (k, d)) in enumerate(zip(frames, res)):
        _check_frame(ctx, i, _oracle(oracle, f), k, d, "tile_sweep batch %d" % i)
    assert res[0][0].tobytes() == res[2][0].tobytes() and np.array_equal(res[0][1], res[2][1])
