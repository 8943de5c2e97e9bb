"""CPU: the restatement of the resident map points' geometry (tests/_points_ref.py) on the constructed scenes of tests/_points_scenes.py:
every scene reaches the rule it is named after, and flipping that rule changes its outcome; the seeded random scenes exercise every
rejection rule of every flavour.  The device is held to the same restatement in tests/test_gpu_points.py."""
import numpy as np
import pytest

import _points_ref as R
import _points_scenes as S
import _proj_ref as PR

CASES = S.all_constructed()
RULED = [c for c in CASES if c.rule is not None]
SEARCH = [c for c in CASES if c.feat is not None]


def test_scene_sizes_and_names():
    assert len({c.name for c in CASES}) == len(CASES)
    for c in CASES:
        assert 3 <= len(c.ids) <= 40, c.name
        assert c.feat is None or c.feat.n <= 130, c.name
        assert c.rule is None or c.rule in R.FLIPS, c.name
    covered = {c.rule for c in RULED}
    assert covered == set(R.FLIPS), sorted(set(R.FLIPS) - covered)


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_scene_reaches_its_rule(c):
    o = c.project()
    assert c.reached(o["trace"]), o["trace"]
    assert o["n_in_view"] == int(o["in_view"].sum())
    dead = ~o["in_view"]
    for k in ("u", "v", "ur", "size", "sigma", "view_cos", "r", "qmin", "qmax", "er"):
        assert not o[k][dead].view(np.uint32).any(), k   # 0 where not in view


@pytest.mark.parametrize("c", RULED, ids=[c.name for c in RULED])
def test_flipping_the_rule_changes_the_outcome(c):
    assert S.outcome(c.project()) != S.outcome(c.project(c.rule))


def test_exact_edges_are_met():
    by = {c.name: c.project() for c in CASES}
    cam = R.Camera()
    o = by["bound_max_frustum"]
    assert o["u"][0] == cam.max_x and o["v"][1] == cam.max_y and o["in_view"].tolist() == [True, True, False, True]
    o = by["fuse_bound_max"]
    assert o["in_view"].tolist() == [False, False, True, True, False]   # u == max, v == max: outside; the first u below max: inside
    assert o["u"][2] == np.nextafter(cam.max_x, np.float32(0))
    o = by["bound_min_reloc"]
    assert o["u"][0] == 0 and o["v"][1] == 0
    o = by["cos998_double"]
    assert o["view_cos"][0] == np.float32(0.998) and float(o["view_cos"][0]) > 0.998 > float(o["view_cos"][1])
    assert o["r"][0] == o["r"][2] == o["r"][3] and o["r"][1] > o["r"][0]     # 2.5 against 4.0
    o = by["reloc_behind_camera"]
    assert o["in_view"][0] and o["u"][0] == 40.0
    for f in ("frustum", "lastframe", "reloc", "fuse"):
        assert not by["z_minus_zero_" + f]["in_view"][0] and not by["z_plus_zero_" + f]["in_view"][0]
    assert by["z_minus_zero_lastframe"]["trace"]["rej"].get("depth") == 1 and "depth" not in by["z_plus_zero_lastframe"]["trace"]["rej"]
    assert "depth" not in by["z_minus_zero_frustum"]["trace"]["rej"] and "depth" not in by["z_minus_zero_fuse"]["trace"]["rej"]


def test_lastframe_takes_size_of_feature_q():
    c = next(c for c in CASES if c.name == "size_last")
    o = c.project()
    assert o["size"].tolist() == [1.0, 1.5, 2.0] and np.array_equal(o["er"], o["r"])


@pytest.mark.parametrize("c", SEARCH, ids=[c.name for c in SEARCH])
def test_search_scene_matches_something(afv, c):
    got, n, o = S.expected_search(afv, PR, c)
    assert n >= 1 and n == int((got >= 0).sum())


def test_stereo_gate_at_equality(afv):
    c = next(c for c in CASES if c.name == "er_sigma_gate")
    Q, o = c.queries()
    assert o["r"][0] == 2.5 and o["er"][0] == 1.25 and o["ur"][0] == 46.0
    got, n, tr = PR.match_projection(S.grid_view(afv, c), Q, th_high=c.th, nnratio=c.nnratio)
    assert tr["eq"]["er_gt_max"] == 1 and got.tolist() == [0, -1]        # the feature AT the gate; the better one beyond it is skipped
    got, n, _ = PR.match_projection(S.grid_view(afv, c), Q, th_high=c.th, nnratio=c.nnratio, flip="er_gt_max")
    assert got.tolist() == [-1, -1]
    got, n, _ = S.expected_search(afv, PR, c, flip="er_sigma")
    assert got.tolist() == [-1, 0]


def test_stereo_gates_of_the_last_frame_search_and_of_fuse(afv):
    c = next(c for c in CASES if c.name == "stereo_gate_lastframe")
    Q, o = c.queries()
    assert o["r"][0] == 2.0 and o["er"][0] == 2.0 and o["ur"][0] == 46.0
    got, n, tr = PR.match_projection(S.grid_view(afv, c), Q, th_high=c.th, nnratio=c.nnratio, last_frame=True)
    assert tr["eq"]["er_gt_max"] == 1 and got.tolist() == [0, -1]        # the feature at the gate; the better one beyond it is skipped
    c = next(c for c in CASES if c.name == "stereo_fuse_inf_gate")
    got, n, o = S.expected_search(afv, PR, c)
    assert got.tolist() == [0, 3, -1]
    c.inf_gate = False
    try:
        assert S.expected_search(afv, PR, c)[0].tolist() == [1, 2, -1]  # without the gate the better matches win
    finally:
        c.inf_gate = True


def test_contested_feature_follows_the_id_order(afv):
    a, b = (next(c for c in CASES if c.name == n) for n in ("contest_order_01", "contest_order_10"))
    ga, na, _ = S.expected_search(afv, PR, a)
    gb, nb, _ = S.expected_search(afv, PR, b)
    assert ga[0] == 0 and gb[0] == 0 and na == nb == 2                  # the FIRST query takes the contested feature ...
    assert a.ids[ga[0]] == 0 and b.ids[gb[0]] == 1                       # ... which is another point in the two orders


RANDOM = [(seed, fl) for seed in range(3) for fl in (R.FRUSTUM, R.LASTFRAME, R.RELOC, R.FUSE)]


@pytest.mark.parametrize("seed,fl", RANDOM, ids=["seed%d_flavour%d" % sf for sf in RANDOM])
def test_random_scenes_exercise_every_rejection(seed, fl):
    s = S.random_scene(seed, fl)
    assert len(s.ids) == 300 and s.feat.n <= 130
    o = s.project()
    share = o["n_in_view"] / 300.0
    assert 0.2 <= share <= 0.8, share
    for rule in S.REJECTS[fl]:
        assert o["trace"]["rej"].get(rule, 0) > 0, rule
    for what in ("minus1", "unset", "bad"):
        assert o["trace"]["invalid"][what] > 0, what
