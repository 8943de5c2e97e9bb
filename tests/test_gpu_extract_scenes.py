"""-m gpu: the extraction kernels on the adversarial scenes of tests/_scenes.py, stage by stage against the CPU oracle

Same bar as tests/test_gpu_extract.py (FAST + NMS sets with integer scores, Harris float bits, selected positions and response bits per
level, keypoint bytes and descriptors end to end), on frames where the select kernels' hardest branches run: a threshold bin of exactly
1024 / 1025 equal-valued keys (positive and negative responses), more equal survivors than the quadtree's LDS holds, the 2k-th FAST score
inside a group of ties, and ring pixels exactly t and t + 1 away from the FAST centre.  tests/test_oracle_scenes.py checks on the CPU that
every scene reaches its branch."""
import functools

import numpy as np
import pytest

import _scenes as S

pytestmark = pytest.mark.gpu

SCENES = ["bin+1024", "bin+1025", "bin-1024", "bin-1025", "flood+", "flood-", "score_ties", "fast_edges20"]


@functools.lru_cache(maxsize=None)
def _scene(name):
    if name.startswith("bin"):
        return S.threshold_bin(name[3], int(name[4:]))[0]
    if name.startswith("flood"):
        return S.tie_flood(name[5])[0]
    if name == "score_ties":
        return S.score_threshold_ties()[0]
    if name.startswith("fast_edges"):
        return S.fast_edges(int(name[10:]))[0]
    raise KeyError(name)


_traces = {}


def _oracle(oracle, img, t=20):
    key = (img.tobytes(), t)
    if key not in _traces:
        _traces[key] = oracle.orb_extract_trace(img, oracle.default_params(1000, 8, 1.2, t))
    return _traces[key]


@pytest.fixture(scope="module", params=["auto", "batch-kernels", "small-batch-kernels"])
def gpu_ctx(afv, request):
    """the three kernel sets of tests/test_gpu_extract.py: the library's choice (<= 4 frames: small-batch kernels, 1024-thread select),
    the batch kernels (256-thread select) for every call, the small-batch kernels for every call (the 6-frame batch included)"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = afv.Context(max_width=1280, max_height=720, max_batch=8)
    ctx.set_small_batch_path({"auto": 1, "batch-kernels": 0, "small-batch-kernels": 2}[request.param])
    yield ctx
    ctx.close()


def _check_frame(ctx, frame, trace, kps, desc, what):
    """every stage of frame `frame` of the context's last call against the oracle's trace"""
    okps, odesc, tr = trace
    nl = len(tr["lw"])
    o = 0
    for l in range(nl):
        # FAST + NMS: the candidate set with integer scores; Harris: float bits of every candidate the oracle scored
        x, y, s, r = ctx.debug_candidates(frame, l)
        got = sorted(zip(y.tolist(), x.tolist(), s.tolist(), r.view(np.uint32).tolist()))
        m = tr["cand"]["level"] == l
        oc, keep1 = tr["cand"][m], tr["keep1"][m]
        assert [g[:3] for g in got] == sorted(zip(oc["y"].tolist(), oc["x"].tolist(), oc["fast_score"].tolist())), (what, l)
        gmap = {(g[0], g[1]): g[3] for g in got}
        for c in oc[keep1]:
            assert gmap[(int(c["y"]), int(c["x"]))] == int(np.float32(c["response"]).view(np.uint32)), (what, l, c)
        # retainBest x 2 + DistributeOctTree: positions and response bits of the selected keypoints
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
    assert np.array_equal(desc, odesc), what


@pytest.mark.parametrize("name", SCENES)
def test_scene_stage_by_stage(gpu_ctx, oracle, name):
    img = _scene(name)
    kps, desc = gpu_ctx.extract(img)
    _check_frame(gpu_ctx, 0, _oracle(oracle, img), kps, desc, name)


def test_mixed_scene_batch(gpu_ctx, oracle, afv):
    """six frames of different kinds in one call: the (frame, level) workgroups of one launch take different branches"""
    frames = [S.threshold_bin("-", 1025)[0], S.tie_flood("+")[0], S.score_threshold_ties()[0], S.fast_edges(20, S.W, S.H)[0],
              afv.synth.corners_frame(5, S.W, S.H), S.threshold_bin("+", 1024)[0]]
    res = gpu_ctx.extract_batch(frames)
    assert len(res) == 6
    for i, (f, (k, d)) in enumerate(zip(frames, res)):
        _check_frame(gpu_ctx, i, _oracle(oracle, f), k, d, "frame %d" % i)


@pytest.mark.parametrize("t", [1, 7, 20, 30, 254])
def test_fast_edges_at_their_threshold(afv, oracle, t):
    """ring pixels exactly t and t + 1 from the centre, with a context whose FAST threshold is t, on both kernel sets"""
    img = S.fast_edges(t)[0]
    ctx = afv.Context(fast_threshold=t)
    trace = _oracle(oracle, img, t)
    for path in (1, 0, 2):
        ctx.set_small_batch_path(path)
        kps, desc = ctx.extract(img)
        _check_frame(ctx, 0, trace, kps, desc, (t, path))
    ctx.close()


@pytest.mark.parametrize("t", [1, 7, 30, 254])
def test_fast_edges_at_the_default_threshold(gpu_ctx, oracle, t):
    img = S.fast_edges(t)[0]
    kps, desc = gpu_ctx.extract(img)
    _check_frame(gpu_ctx, 0, _oracle(oracle, img), kps, desc, t)
