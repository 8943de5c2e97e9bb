"""-m gpu: k_harris and k_describe on the constructed scenes of tests/_desc_scenes.py, bit for bit against the CPU oracle

Same bar as tests/test_gpu_extract_scenes.py (candidate sets with integer scores, Harris float bits, selected positions, keypoint bytes - the IC angle among
them - and descriptors), on frames built for the edges of the numeric stages: probes on the last column of every disc row and one beyond, moments on the axes
and diagonals, half discs, blur sums on exact halves and beyond 2^24, equal and adjacent blurred values, rotated coordinates a few ulps from n + 0.5, patches
that leave the level on every side, Sobel sums at their largest.  Every scene runs on the three kernel sets, through extract, detect + compute and
afv.Frame.extract, and six of them in one batch; the caller-angle scenes run through compute.  The expected values are the oracle's;
tests/test_orb_ref_cpu.py checks the oracle against a plain restatement on the same scenes and proves that every scene reaches its rule."""
import numpy as np
import pytest

import _desc_scenes as D

pytestmark = pytest.mark.gpu

DETECT = list(D.DETECT)
MIXED = ["disc_edge0", "atan", "half_v", "half_d-", "checker", "saturation"]

_traces = {}


def _oracle(oracle, img):
    key = img.tobytes()
    if key not in _traces:
        _traces[key] = oracle.orb_extract_trace(img)
    return _traces[key]


@pytest.fixture(scope="module", params=["auto", "batch-kernels", "small-batch-kernels"])
def ctx(afv, request):
    """the three kernel sets of tests/test_gpu_extract.py, on a context sized to the scenes"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context(max_width=D.W, max_height=D.H, max_batch=8)
    c.set_small_batch_path({"auto": 1, "batch-kernels": 0, "small-batch-kernels": 2}[request.param])
    yield c
    c.close()


def _check_frame(ctx, frame, trace, kps, desc, what):
    """every stage of frame `frame` of the context's last call against the oracle's trace (as tests/test_gpu_extract_scenes.py does)"""
    okps, odesc, tr = trace
    o = 0
    for l in range(len(tr["lw"])):
        x, y, s, r = ctx.debug_candidates(frame, l)
        got = sorted(zip(y.tolist(), x.tolist(), s.tolist(), r.view(np.uint32).tolist()))
        m = tr["cand"]["level"] == l
        oc, keep1 = tr["cand"][m], tr["keep1"][m]
        assert [g[:3] for g in got] == sorted(zip(oc["y"].tolist(), oc["x"].tolist(), oc["fast_score"].tolist())), (what, l)
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
    bad = np.flatnonzero(kps["angle"].view(np.uint32) != okps["angle"].view(np.uint32)) if len(kps) == len(okps) else []
    assert len(bad) == 0, (what, "angles", kps[bad[:4]], okps[bad[:4]])
    assert kps.tobytes() == okps.tobytes(), what
    assert np.array_equal(desc, odesc), (what, np.flatnonzero((desc != odesc).any(1))[:8])


@pytest.mark.parametrize("name", DETECT)
def test_scene_stage_by_stage(ctx, oracle, name):
    """extract, stage by stage; then detect alone gives the same keypoints and compute at them the same descriptors"""
    img = D.detect_scene(name)[0]
    trace = _oracle(oracle, img)
    kps, desc = ctx.extract(img)
    _check_frame(ctx, 0, trace, kps, desc, name)
    kd = ctx.detect(img)
    assert kd.tobytes() == trace[0].tobytes(), name
    assert np.array_equal(ctx.compute(img, kd), trace[1]), name


@pytest.mark.parametrize("name", DETECT)
def test_scene_into_a_resident_frame(ctx, oracle, afv, name):
    """afv.Frame.extract: the launch that also mirrors keypoints and descriptors into the frame's device copy returns the oracle's bytes, and the mirror
    holds them too: the grid built on the device from the mirrored positions is the host's, and a projection search of the frame's own features against
    the resident copy (positions, sizes, angles and descriptors read from the mirror) gives the oracle's matches on the oracle's outputs"""
    img = D.detect_scene(name)[0]
    okps, odesc, _ = _oracle(oracle, img)
    fr = afv.Frame(ctx)
    try:
        k, d = fr.extract(img)
        assert k.tobytes() == okps.tobytes() and np.array_equal(d, odesc) and fr.N == len(okps), name
        cp, ci = fr.grid()
        assert cp[-1] == len(okps)   # every keypoint of a 320 x 240 frame lies inside the 640 x 480 grid
        cells = np.repeat(np.arange(len(cp) - 1), np.diff(cp))
        px = np.floor((okps["x"] * fr.grid_inv_w).astype(np.float64) + 0.5).astype(np.int64)   # PosInGrid: round((x - 0) * inv), float32 product
        py = np.floor((okps["y"] * fr.grid_inv_h).astype(np.float64) + 0.5).astype(np.int64)
        assert np.array_equal(np.sort(ci), np.arange(len(okps))) and np.array_equal(cells, (px * 48 + py)[ci]), name
        size = ctx.size_sigma(okps)[0]
        q = afv.ProjectionQueries(odesc, okps["x"], okps["y"], np.float32(15.0) * size, size / np.float32(1.2), size * np.float32(1.2), angles=okps["angle"])
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        got, n = fr.SearchByProjection(afv.FeatureMatcher(0.9, True, ctx=ctx), q, last_frame=True)
        view = afv.FrameGridView(odesc, np.stack([okps["x"], okps["y"]], 1), size, angles=okps["angle"])
        want, wn = oracle.match_projection(view, q, th_high=75.0, nnratio=0.9, check_orientation=True, last_frame=True)
        assert n == wn > 0 and np.array_equal(got, want), name
    finally:
        fr.close()


def test_mixed_scene_batch(ctx, oracle):
    """six different scenes in a single call"""
    frames = [D.detect_scene(n)[0] for n in MIXED]
    res = ctx.extract_batch(frames)
    assert len(res) == 6
    for i, (f, (k, d)) in enumerate(zip(frames, res)):
        _check_frame(ctx, i, _oracle(oracle, f), k, d, MIXED[i])


def _compute_scene(oracle, name):
    if name == "ties":
        return D.ties()[:2]
    if name == "comparisons":
        return D.comparisons()[:2]
    if name.startswith("rotation"):
        return D.rotation(name[9:])
    lw, lh, ls = oracle.level_geometry(D.APRON_W, D.APRON_H)
    return D.apron(ls.tolist(), lw.tolist(), lh.tolist())


@pytest.mark.parametrize("name", ["ties", "comparisons", "rotation_noise", "rotation_checker", "apron"])
def test_compute_scene(ctx, oracle, name):
    """caller-given keypoints and angles: blur ties, equal and adjacent values, rotated coordinates next to n + 0.5, patches that leave the level"""
    img, kps = _compute_scene(oracle, name)
    want = oracle.orb_compute(img, kps)
    got = ctx.compute(img, kps)
    assert np.array_equal(got, want), (name, np.flatnonzero((got != want).any(1))[:8])


@pytest.mark.parametrize("name", ["saturation", "ties"])
def test_level_blur_kernel(ctx, oracle, name):
    """the whole-level blur kernel (another code path than the blur inside k_describe) on the sums beyond 2^24 and the exact halves"""
    img = D.detect_scene(name)[0] if name == "saturation" else D.ties()[0]
    ctx.extract(img)
    tr = _oracle(oracle, img)[2]
    for l in range(len(tr["lw"])):
        assert np.array_equal(ctx.debug_blur_level(0, l), tr["blurred"][l]), (name, l)
