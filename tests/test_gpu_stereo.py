"""-m gpu: Frame::ComputeStereoMatches / ComputeStereoFromRGBD on the device (afv_frame_stereo_match, afv_frame_set_depth) against the plain
restatement tests/_stereo_ref.py, bit for bit: u_right and depth as float bits, the SAD and the chosen right index as ints.

Every constructed scene of tests/_stereo_scenes.py goes through set_features + set_pyramid on a 96 x 64, 3-level context
(tests/test_stereo_ref_cpu.py proves on the CPU that each scene reaches the rule it names and that the rule decides its outcome); one
end-to-end case runs on two extracted keep_pyramid frames; the mvuRight the device made is followed into the keyframe table and
SearchForTriangulation(bOnlyStereo)."""
import ctypes

import numpy as np
import pytest

import _stereo_ref as SR
import _stereo_scenes as SS

pytestmark = pytest.mark.gpu

f32 = np.float32
SCENES = SS.all_scenes()
EINVAL, EUNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def sctx(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context(nfeatures=300, nlevels=SS.NLEVELS, scale_factor=SS.SCALE, max_width=SS.WIDTH, max_height=SS.HEIGHT)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ectx(afv):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = afv.Context(nfeatures=300, max_width=160, max_height=120)
    yield c
    c.close()


def _frame(afv, ctx, side, pyr, cap=130):
    """a resident frame holding one eye of a scene"""
    fl = side.desc.dtype.kind == "f"
    fr = afv.Frame(ctx, max_x=float(SS.WIDTH), max_y=float(SS.HEIGHT), cap=cap, desc_bytes=32 if fl else side.desc.shape[1],
                   float_dim=side.desc.shape[1] if fl else 0)
    kps = np.zeros(side.n, afv.KP_DTYPE)
    kps["x"], kps["y"], kps["octave"] = side.x, side.y, side.octave
    fr.set_features(kps, side.desc, sizes=side.size)
    if pyr is not None:
        fr.set_pyramid(pyr)
    return fr


def _same_bits(got, want):
    return got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _check(fr, n_stereo, want):
    ur, dp, sad, br = fr.stereo()
    w_ur, w_dp, w_sad, w_br = want[:4]
    assert np.array_equal(br, w_br), "best_r"
    assert np.array_equal(sad, w_sad), "sad"
    assert _same_bits(ur, w_ur), "u_right bits: %r vs %r" % (ur, w_ur)
    assert _same_bits(dp, w_dp), "depth bits"
    assert n_stereo == int((w_ur >= 0).sum())


@pytest.mark.parametrize("s", SCENES, ids=[s.name for s in SCENES])
def test_scene_against_the_restatement(afv, sctx, s):
    left, right = _frame(afv, sctx, s.L, s.pyrL), _frame(afv, sctx, s.R, s.pyrR)
    try:
        assert left.pyramid()[2].tobytes() == s.pyrL[2].tobytes()
        n = left.ComputeStereoMatches(right, s.mbf, s.fx, th_high=s.th_high, th_low=s.th_low)
        _check(left, n, s.expected)
    finally:
        left.close(); right.close()


def test_default_thresholds_are_the_matchers(afv, sctx):
    s = next(x for x in SCENES if x.name == "rows_32_bytes")
    left, right = _frame(afv, sctx, s.L, s.pyrL), _frame(afv, sctx, s.R, s.pyrR)
    try:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(50.0)
        n = left.ComputeStereoMatches(right, s.mbf, s.fx)
        _check(left, n, s.expected)
    finally:
        afv.FeatureMatcher.setDescriptorDistanceThresholds(75.0)
        left.close(); right.close()


@pytest.fixture(scope="module")
def extracted(afv, ectx):
    """two keep_pyramid frames extracted from a 160 x 120 synthetic image and its copy moved 4 px, everything of them downloaded, and the
    restatement's answer on the downloaded data"""
    img = afv.synth.corners_frame(5, 160, 120)
    eyes = []
    for im in (img, np.roll(img, -4, axis=1)):
        fr = afv.Frame(ectx, max_x=160.0, max_y=120.0, keep_pyramid=True)
        k, d = fr.extract(im)
        g = ectx.geometry()
        levels = [ectx.debug_level(0, l) for l in range(g["nlevels"])]   # afv_debug_get_level of the extraction that just ran
        eyes.append((fr, k, d, levels, ectx.size_sigma(k)[0]))
    (fl, kl, dl, pl, sl), (fr_, kr, dr, pr, sr) = eyes
    L = SR.Side(kl["x"], kl["y"], kl["octave"], sl, dl)
    R = SR.Side(kr["x"], kr["y"], kr["octave"], sr, dr)
    want = SR.compute_stereo_matches(L, R, pl, pr, 40.0, 100.0, 75.0, 75.0)
    yield eyes, want
    fl.close(); fr_.close()


def test_keep_pyramid_levels_equal_debug_get_level(extracted):
    eyes, _ = extracted
    for fr, _, _, levels, _ in eyes:
        kept = fr.pyramid()
        assert len(kept) == len(levels) == 8
        for a, b in zip(kept, levels):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_end_to_end_on_extracted_frames(extracted):
    eyes, want = extracted
    left, right = eyes[0][0], eyes[1][0]
    n = left.ComputeStereoMatches(right, 40.0, 100.0, th_high=75.0, th_low=75.0)
    _check(left, n, want)
    assert n >= 1 and want[4]["accepted"] >= n
    assert left.mvuRight.tobytes() == want[0].tobytes() and left.mvDepth.tobytes() == want[1].tobytes()


def test_a_frame_without_keep_pyramid_keeps_none(afv, ectx, extracted):
    eyes, _ = extracted
    fr = afv.Frame(ectx, max_x=160.0, max_y=120.0)
    try:
        fr.extract(afv.synth.corners_frame(5, 160, 120))
        with pytest.raises(afv._lib.AfvError) as e:
            fr.ComputeStereoMatches(eyes[1][0], 40.0, 100.0)
        assert e.value.code == EINVAL
        assert np.all(fr.mvDepth == -1) and np.all(fr.mvuRight == -1)
    finally:
        fr.close()


def test_rgbd_gather(afv, sctx):
    h, w = 40, 50
    depth = np.zeros((h, w), np.float32)
    rng = np.random.default_rng(7)
    depth[:] = rng.uniform(0.5, 8.0, (h, w)).astype(np.float32)
    x = np.array([10.2, 49.9, 0.0, 20.7, 30.0, 49.0, 50.0, 12.0, -0.5], np.float32)   # last column 49; 50.0 is outside; -0.5 truncates to 0
    y = np.array([5.9, 39.9, 0.0, 11.1, 39.0, 20.0, 10.0, 40.0, 3.0], np.float32)     # last row 39; 40.0 is outside
    depth[11, 20] = 0.0
    depth[39, 30] = -2.0
    kps = np.zeros(len(x), afv.KP_DTYPE)
    kps["x"], kps["y"] = x, y
    fr = afv.Frame(sctx, max_x=float(SS.WIDTH), max_y=float(SS.HEIGHT), cap=16)
    try:
        fr.set_features(kps, np.zeros((len(x), 32), np.uint8), sizes=np.ones(len(x), np.float32))
        padded = np.zeros((h, w + 3), np.float32)       # a strided image
        padded[:, :w] = depth
        fr.ComputeStereoFromRGBD(padded[:, :w], 40.0)
        w_ur, w_dp = SR.compute_stereo_from_rgbd(x, y, x, depth, 40.0)
        assert w_dp[3] == -1 and w_dp[4] == -1 and w_dp[6] == -1 and w_dp[7] == -1 and w_dp[1] == depth[39, 49] and w_dp[8] == depth[3, 0]
        ur, dp, sad, br = fr.stereo()
        assert _same_bits(ur, w_ur) and _same_bits(dp, w_dp)
        assert np.all(sad == -1) and np.all(br == -1)
    finally:
        fr.close()


def test_device_made_u_right_reaches_the_keyframe_table(afv, ectx, extracted):
    """device-made mvuRight -> afv_table_set_from_frame -> afv_table_match_triangulation(only_stereo = 1), equal to the same chain with the
    restatement's u_right uploaded through set_features"""
    eyes, want = extracted
    (left, kl, dl, _, sl), (right, kr, dr, _, sr) = eyes
    left.ComputeStereoMatches(right, 40.0, 100.0, th_high=75.0, th_low=75.0)
    # the second keyframe: the right eye's features with a u_right of their own (uploaded: this test is about the left frame's plane)
    ur2 = np.where(np.arange(len(kr)) % 3 != 0, kr["x"] - f32(4.0), f32(-1.0)).astype(np.float32)
    voc = afv.Vocabulary.random(3, k=8, L=3, ctx=ectx)
    kf2 = afv.Frame(ectx, max_x=160.0, max_y=120.0)
    ref = afv.Frame(ectx, max_x=160.0, max_y=120.0)
    table = afv.table.DescriptorTable(ectx, 3, ectx.cap)
    try:
        kf2.set_features(kr, dr, sizes=sr, u_right=ur2)
        ref.set_features(kl, dl, sizes=sl, u_right=want[0])
        for fr in (left, kf2, ref):
            fr.ComputeBoW(voc, levelsup=2)
        table.set_from_frame(0, left)
        table.set_from_frame(1, kf2)
        table.set_from_frame(2, ref)
        F12 = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0]] * 2, np.float32)
        ep = np.array([[-1000.0, -1000.0]] * 2, np.float32)
        for only in (True, False):
            m, nm = table.match_triangulation([0, 2], [1, 1], F12, ep, 75.0, only_stereo=only)
            assert nm[0] == nm[1] and np.array_equal(m[0], m[1]), only
            if only:
                n_only = int(nm[0])
                matched = np.nonzero(m[0, :len(kl)] >= 0)[0]
                assert n_only >= 1 and np.all(want[0][matched] >= 0)   # bOnlyStereo keeps stereo-stereo pairs only
            else:
                assert nm[0] >= n_only
    finally:
        table.close(); voc.close(); kf2.close(); ref.close()


def test_more_than_1024_accepted_pairs(afv):
    """k_stereo_median strides over the features 1024 at a time and k_stereo_match stages the right side 128 at a time: 1600 pairs on a
    320 x 240 image (beyond the 130 features of the constructed scenes), SADs spread over both bytes of the radix select"""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ctx = afv.Context(nfeatures=300, nlevels=2, max_width=320, max_height=240)
    rng = np.random.default_rng(11)
    w, h, d = 320, 240, 4
    (w1, h1) = SS.level_sizes(w, h, 2)[1]
    left0 = rng.integers(20, 201, (h, w)).astype(np.uint8)
    right0 = rng.integers(20, 201, (h, w)).astype(np.uint8)
    right0[:, :w - d] = left0[:, d:]
    right0 = (right0.astype(np.int32) + rng.integers(0, 2, (h, w)) * rng.integers(0, 40, (h, 1))).astype(np.uint8)   # rows of growing noise
    pl, pr = [left0, np.zeros((h1, w1), np.uint8)], [right0, np.zeros((h1, w1), np.uint8)]
    cy, cx = np.meshgrid(np.arange(8, 232, 5), np.arange(20, 308, 8), indexing="ij")
    cx, cy = cx.ravel()[:1600].astype(np.float32), cy.ravel()[:1600].astype(np.float32)
    n = len(cx)
    assert n == 1600
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    L = SR.Side(cx, cy, np.zeros(n, np.int32), np.ones(n, np.float32), desc)
    R = SR.Side(cx - f32(d), cy, np.zeros(n, np.int32), np.ones(n, np.float32), desc)
    want = SR.compute_stereo_matches(L, R, pl, pr, 40.0, 30.0, 50.0, 50.0)
    assert want[4]["accepted"] > 1024 and want[4]["median_removed"] > 0 and want[4]["median"] > 255
    frames = []
    try:
        for side, pyr in ((L, pl), (R, pr)):
            fr = afv.Frame(ctx, max_x=float(w), max_y=float(h), cap=n)
            frames.append(fr)
            kps = np.zeros(n, afv.KP_DTYPE)
            kps["x"], kps["y"], kps["octave"] = side.x, side.y, side.octave
            fr.set_features(kps, side.desc, sizes=side.size)
            fr.set_pyramid(pyr)
        got = frames[0].ComputeStereoMatches(frames[1], 40.0, 30.0, th_high=50.0, th_low=50.0)
        _check(frames[0], got, want)
    finally:
        for fr in frames:
            fr.close()
        ctx.close()


def test_error_codes(afv, sctx, ectx):
    s = next(x for x in SCENES if x.name == "rows_32_bytes")
    s61 = next(x for x in SCENES if x.name == "rows_61_bytes")
    sf = next(x for x in SCENES if x.name == "rows_64_floats")
    left, right = _frame(afv, sctx, s.L, s.pyrL), _frame(afv, sctx, s.R, s.pyrR)
    other_ctx = _frame(afv, ectx, s.R, None, cap=0)
    no_pyr = _frame(afv, sctx, s.R, None)
    r61, rf = _frame(afv, sctx, s61.R, s61.pyrR), _frame(afv, sctx, sf.R, sf.pyrR)
    small = _frame(afv, sctx, s.R, None)
    frames = [left, right, other_ctx, no_pyr, r61, rf, small]

    def code(fn):
        with pytest.raises(afv._lib.AfvError) as e:
            fn()
        return e.value.code
    try:
        assert code(lambda: left.ComputeStereoMatches(other_ctx, 40.0, 30.0)) == EINVAL        # two contexts
        assert code(lambda: left.ComputeStereoMatches(no_pyr, 40.0, 30.0)) == EINVAL           # a missing pyramid
        assert code(lambda: no_pyr.ComputeStereoMatches(right, 40.0, 30.0)) == EINVAL
        assert code(lambda: left.ComputeStereoMatches(r61, 40.0, 30.0)) == EUNSUPPORTED        # another row width
        assert code(lambda: left.ComputeStereoMatches(rf, 40.0, 30.0)) == EUNSUPPORTED         # another kind
        lv = [np.zeros((h, w), np.uint8) for (w, h) in SS.level_sizes(64, 48)]
        small.set_pyramid(lv)                                                                   # a 64 x 48 image's levels
        assert code(lambda: left.ComputeStereoMatches(small, 40.0, 30.0)) == EUNSUPPORTED      # another geometry
        assert code(lambda: small.set_pyramid(lv[:2])) == EINVAL                               # not the context's level count
        assert code(lambda: small.set_pyramid([lv[0], lv[1], lv[2][:-1]])) == EINVAL           # not the context's level size
        # the C side's own checks (Frame.set_pyramid answers the two above before the library is called)
        set_pyr = sctx.lib.afv_frame_set_pyramid
        arr = lambda lvs: (ctypes.c_void_p * len(lvs))(*[None if a is None else a.ctypes.data for a in lvs])
        assert set_pyr(small.handle, 64, 48, arr(lv[:2]), 2) == EINVAL                          # another level count
        assert set_pyr(small.handle, 64, 48, arr([lv[0], None, lv[2]]), 3) == EINVAL            # a NULL level
        assert set_pyr(small.handle, SS.WIDTH + 1, 48, arr(lv), 3) == EINVAL                    # wider than the context
        assert set_pyr(small.handle, 64, 48, arr(lv), 3) == 0
        p = afv._lib.sized(afv._lib.StereoParams)
        p.struct_size = 8
        assert sctx.lib.afv_frame_stereo_match(left.handle, right.handle, ctypes.byref(p), None) == EINVAL
        assert left.ComputeStereoMatches(right, s.mbf, s.fx, th_high=s.th_high, th_low=s.th_low) == int((s.expected[0] >= 0).sum())
    finally:
        for fr in frames:
            fr.close()
