"""-m gpu: the host runtime of the AKAZE61 path (csrc/akaze_api.hip) where no stage comparison reaches it: the fallback from the fixed-point
suppression to the ordered rounds INSIDE afv_akaze_extract, what that call reports when engine 1 is forced and gives up, and the upload
branches of afv_akaze_scale_space (pageable, strided, page-locked source through one staging function)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 320, 200   # the two-frame scene of test_gpu_akaze.py::test_fixed_point_gives_up_loudly_or_falls_back


def _frames(afv, w, h, seeds):
    return np.stack([afv.synth.corners_batch(s, 1, w, h)[0] for s in seeds])


def _context(afv, w=W, h=H, batch=2):
    return afv.AkazeContext(afv.akaze.default_params(max_width=w, max_height=h, max_batch=batch))


def _give_up(ctx, mode, reason):
    """make the fixed point give up on an ordinary frame: a pass bound of 1 (status 7) or records that hold one earlier neighbour (status 6)"""
    if reason == "pass_bound":
        ctx.set_suppress_engine(mode, pass_cap=1)
    else:
        ctx.set_suppress_engine(mode)
        ctx.debug_neighbour_cap(1)


@pytest.fixture(scope="module")
def scene(afv):
    """the frames and what the ordered rounds (engine 0) extract from them: computed once, read by every test"""
    frames = _frames(afv, W, H, (4, 5))
    ctx = _context(afv)
    ctx.set_suppress_engine(0)
    want = [(k.tobytes(), d.copy()) for k, d in ctx.extract(frames)]
    ctx.close()
    assert all(len(d) > 100 for _, d in want)
    return frames, want


@pytest.mark.parametrize("reason", ["pass_bound", "neighbour_cap"])
def test_extract_falls_back_inside_the_call(afv, scene, reason):
    """engine 2 with a fixed point that must give up: afv_akaze_extract repeats the batch through the ordered rounds within the call and returns
    their result, byte for byte - and again on the next call, which builds a new scale space and so has to fall back once more"""
    frames, want = scene
    ctx = _context(afv)
    _give_up(ctx, 2, reason)
    for rep in range(2):
        got = ctx.extract(frames)
        for f in range(2):
            assert got[f][0].tobytes() == want[f][0], (rep, f)
            assert np.array_equal(got[f][1], want[f][1]), (rep, f)
    ctx.close()


@pytest.mark.parametrize("reason,names", [("pass_bound", b"pass bound"), ("neighbour_cap", b"earlier in-range candidates")])
def test_extract_reports_a_forced_engine_that_gives_up(afv, scene, reason, names):
    """engine 1 forced (no fallback): the raw C call returns AFV_ECAPACITY and afv_akaze_last_error names the limit.  What the call copies out
    beside the error is deliberately not asserted (the status rule in csrc/akaze_api.hip documents it)"""
    frames, _ = scene
    ctx = _context(afv)
    _give_up(ctx, 1, reason)
    cap = 1064
    kps = np.zeros((2, cap), afv.KP_DTYPE); desc = np.zeros((2, cap, 61), np.uint8); n = np.zeros(2, np.int32)
    rc = ctx.lib.afv_akaze_extract(ctx.handle, frames.ctypes.data, 2, W, H, W, W * H, kps.ctypes.data, desc.ctypes.data, cap, n.ctypes.data)
    assert rc == afv._lib.ECAPACITY
    assert names in ctx.lib.afv_akaze_last_error(ctx.handle)
    ctx.close()


def test_scale_space_upload_branches_agree(afv):
    """afv_akaze_scale_space from a contiguous pageable frame, from a strided view (a ROI of a larger array) and from page-locked memory, on one
    context in that order (the device image and the pinned arena grow on the first call and are reused): identical Lt planes at the first and
    the last level"""
    import torch
    w, h = 97, 61
    frame = _frames(afv, w, h, (8,))[0]
    ctx = _context(afv, w, h, 1)
    plan = ctx.scale_space(frame)
    levels = (0, plan.nlevels - 1)
    want = [ctx.plane(0, i, afv.akaze.LT) for i in levels]
    assert all(np.isfinite(p).all() and p.std() > 0 for p in want)
    big = np.full((h + 8, w + 16), 255, np.uint8)
    big[4:4 + h, 8:8 + w] = frame
    roi = big[4:4 + h, 8:8 + w]
    pinned = torch.from_numpy(frame.copy()).pin_memory()
    for name, address, stride in (("strided", roi.ctypes.data, big.strides[0]), ("pinned", pinned.data_ptr(), w)):
        ctx.check(ctx.lib.afv_akaze_scale_space(ctx.handle, address, 1, w, h, stride, 0), "afv_akaze_scale_space")
        for i, p in zip(levels, want):
            assert np.array_equal(ctx.plane(0, i, afv.akaze.LT), p), (name, i)
    ctx.close()
