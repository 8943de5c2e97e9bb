"""-m "not gpu": the restatement tests/_stereo_ref.py (the normative semantics of afv_frame_stereo_match / afv_frame_set_depth) and the
constructed scenes of tests/_stereo_scenes.py.  For every scene that names a rule: the restatement's trace shows the rule was reached, and
turning that one rule around changes the scene's outcome - so a device that gets the rule wrong cannot pass tests/test_gpu_stereo.py.
Plus a few answers computed by hand, and the new symbols of the built library."""
import ctypes
import os

import numpy as np
import pytest

import _stereo_ref as SR
import _stereo_scenes as SS

f32 = np.float32
SCENES = SS.all_scenes()
RULED = [s for s in SCENES if s.rule]


def test_level_sizes_of_the_scene_geometry():
    assert SS.SIZES == [(96, 64), (80, 53), (67, 44)]


@pytest.mark.parametrize("s", SCENES, ids=[s.name for s in SCENES])
def test_scene_reaches_what_it_names(s):
    tr = s.expected[4]
    for key in s.reach:
        assert tr[key] > 0, "%s: the trace never counted %s" % (s.name, key)
    assert s.L.n <= 130 and s.R.n <= 130


@pytest.mark.parametrize("s", RULED, ids=[s.name + "-" + s.rule for s in RULED])
def test_rule_changes_the_outcome(s):
    assert s.rule in SR.FLIPS
    assert not SS.same_outcome(s.expected, s.run(flip=s.rule)), "%s: flipping %s (%s) changes nothing" % (s.name, s.rule, SR.FLIPS[s.rule])


def test_every_flip_but_the_unreachable_ones_has_a_scene():
    # c_left / gate_iniu: uR <= uL makes su0 - 10 < 0 hold whenever they do (scenes reach them, never alone)
    assert set(SR.FLIPS) - {s.rule for s in RULED} == {"c_left", "gate_iniu"}


def test_accepted_counts_of_the_median_scenes():
    by = {s.name: s for s in SCENES}
    for name, acc, kept in (("median_of_no_pairs", 0, 0), ("median_of_one_pair", 1, 1), ("median_of_one_pair_sad_0", 1, 0), ("median_of_two_pairs", 2, 2),
                            ("median_of_three_pairs", 3, 2), ("pair_exactly_on_thDist", 3, 2)):
        e = by[name].expected
        assert e[4]["accepted"] == acc and int((e[0] >= 0).sum()) == kept, name
    assert by["pair_exactly_on_thDist"].expected[4]["th_dist"] == 21.0


def test_disparity_scenes_take_the_branches_they_name():
    by = {s.name: s for s in SCENES}
    e = by["disparity_exactly_zero"].expected
    assert e[0][2] == f32(50.0 - 0.01) and e[1][2] == f32(f32(40.0) / f32(0.01)) and e[4]["delta"][2] == 0.0
    assert by["disparity_slightly_negative"].expected[0][2] == -1.0
    e = by["brightness_offset_between_the_eyes"].expected
    assert e[2][2] == 0 and e[0][2] >= 0


def test_window_sad_by_hand():
    imL = np.full((11, 11), 50, np.uint8)
    imL[5, 5] = 60                      # minus its centre: 120 pixels of -10
    imR = np.full((11, 11), 80, np.uint8)
    assert SR.window_sad(imL, imR, 5, 5, 5) == 1200
    assert SR.window_sad(imL, imR, 5, 5, 5, centre=False) == 120 * 30 + 20
    imR[0, 0] = 83                      # one pixel of +3 against -10
    imR[10, 10] = 60                    # one of -20 against -10
    assert SR.window_sad(imL, imR, 5, 5, 5) == 1200 + 3 + 0
    assert 121 * 510 == 61710


def test_parabola_by_hand():
    assert SR.parabola(30, 10, 20) == f32(f32(10.0) / f32(60.0))
    assert SR.parabola(20, 10, 20) == 0.0
    assert SR.parabola(11, 10, 10) == f32(0.5)        # d3 == d2: the first minimum keeps the lower offset
    assert f32(f32(1.5) * f32(1.4)) * f32(10.0) == f32(21.0)


def test_c_round_is_half_away_from_zero():
    assert [int(SR.c_round(v)) for v in (0.5, 1.5, 2.5, -0.5, -1.5, 0.49999997)] == [1, 2, 3, -1, -2, 0]


def test_rgbd_restatement():
    img = np.zeros((4, 6), np.float32)
    img[3, 5] = 2.0
    img[1, 2] = -1.0
    x = np.array([5.9, 2.2, 0.0, 6.0], np.float32)
    y = np.array([3.9, 1.7, 0.0, 1.0], np.float32)
    ur, dp = SR.compute_stereo_from_rgbd(x, y, x + f32(0.25), img, 40.0)
    assert dp.tolist() == [2.0, -1.0, -1.0, -1.0]
    assert ur[0] == f32(f32(6.15) - f32(20.0)) and ur[1:].tolist() == [-1.0, -1.0, -1.0]


def test_library_exports_the_stereo_symbols(afv):
    lib = ctypes.CDLL(afv._lib.LIB_PATH)
    for name in ("afv_frame_stereo_match", "afv_frame_set_depth", "afv_frame_get_stereo", "afv_frame_set_pyramid", "afv_frame_get_pyramid_level",
                 "afv_pyramid_level_sizes"):
        assert hasattr(lib, name), name
    assert ctypes.sizeof(afv._lib.StereoParams) == 20
    assert afv._lib.FrameParams.keep_pyramid.offset == 44 and lib.afv_abi_version() == afv._lib.ABI_VERSION
    assert os.path.exists(afv._lib.LIB_PATH)
