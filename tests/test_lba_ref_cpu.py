"""CPU: the restatement of LocalBundleAdjustment / BundleAdjustment (tests/_lba_ref.py) on the constructed scenes (tests/_lba_scenes.py):
every scene reaches the rule it is named for; the restated Schur step equals a dense solve of the FULL damped system; each analytic
Jacobian equals a central difference of the error."""
import numpy as np
import pytest

import _lba_ref as L
import _lba_scenes as S
from _poseopt_ref import exp_step

F64 = np.float64
SCENES = dict(S.every_scene())
_cache = {}


def solved(name):
    if name not in _cache:
        log = []
        _cache[name] = (SCENES[name].solve(log), log)
    return _cache[name]


def trials(log):
    return [t for rnd in log for t in rnd if "trial" in t]


def edge_of(sc, p, k):
    return int(np.nonzero((sc.e_pt == p) & (sc.e_kf == k))[0][0])


def test_every_rule_has_its_scene():
    want = {"chi2_first_mono", "chi2_first_stereo", "depth_alone_erased", "depth_alone_survives", "bad_pivot", "singular_point_block_ten_trials",
            "mixed_mono_stereo", "failed_trial_lambda_growth", "startup_two_keyframes", "no_fixed_keyframe", "single_edge_point",
            "point_seen_by_fixed_only", "dropped_points", "stop_before", "stop_in_first", "stop_in_second", "stop_global_ba", "empty_no_free",
            "empty_no_points", "empty_all_dropped"}
    assert want == set(SCENES)


@pytest.mark.parametrize("name,p,k,stereo", [("chi2_first_mono", 5, 1, False), ("chi2_first_stereo", 7, 1, True)])
def test_an_edge_is_removed_by_chi2_at_the_first_check(name, p, k, stereo):
    sc = SCENES[name]
    r, _ = solved(name)
    e = edge_of(sc, p, k)
    pr = sc.problem()
    assert bool(pr.stereo[e]) == stereo
    assert r.first_chi2[e] > pr.th[e] and not r.first_depth_bad[e]
    assert r.state[e] == L.ERASE and r.n_removed_first >= 1 and r.iterations[1] > 0


def test_an_edge_removed_for_depth_alone_is_erased_when_the_point_stays_behind():
    sc = SCENES["depth_alone_erased"]
    r, _ = solved("depth_alone_erased")
    e = edge_of(sc, 9, 4)
    assert r.first_chi2[e] <= sc.problem().th[e] and r.first_depth_bad[e] and r.final_depth_bad[e] and r.state[e] == L.ERASE


def test_an_edge_removed_for_depth_alone_survives_the_final_check():
    """L-Q1"""
    sc = SCENES["depth_alone_survives"]
    r, _ = solved("depth_alone_survives")
    e = edge_of(sc, 0, 6)
    pr = sc.problem()
    assert r.first_chi2[e] <= pr.th[e] and r.first_depth_bad[e]          # removed by the first check, for depth alone
    assert not r.final_depth_bad[e] and r.state[e] == L.REMOVED_KEPT     # in front at the final estimate: not in vToErase
    est = (pr.R0, pr.t0, r.xyz)
    est[0][:pr.nf], est[1][:pr.nf] = r.R.reshape(-1, 3, 3), r.t
    assert L.edges_at(pr, *est)[2][e] > pr.th[e]                         # although its error at the final estimate is gross


def test_failed_trials_grow_lambda():
    _, log = solved("failed_trial_lambda_growth")
    t = trials(log)
    rejected = [i for i, x in enumerate(t) if not x["accepted"]]
    assert rejected
    i = rejected[0]
    assert t[i + 1]["lam"] == t[i]["lam"] * F64(2.0) and t[i + 1]["iteration"] == t[i]["iteration"]


def test_a_bad_pivot_is_a_failed_trial():
    r, log = solved("bad_pivot")
    t = trials(log)
    bad = [i for i, x in enumerate(t) if x["why"] == "pivot"]
    assert bad and all(t[i]["failed"] and not t[i]["accepted"] and t[i]["rho"] == -1.0 for i in bad)
    assert t[bad[0] + 1]["lam"] > t[bad[0]]["lam"]


def test_a_singular_point_block_is_a_failed_trial_and_ten_trials_stop():
    r, log = solved("singular_point_block_ten_trials")
    assert all(x["why"] == "det" and x["failed"] for x in trials(log))
    assert list(r.iterations) == [1, 1] and list(r.trials) == [10, 10]
    assert [x["terminate"] for rnd in log for x in rnd if "terminate" in x] == ["qmax", "qmax"]
    sc = SCENES["singular_point_block_ten_trials"]
    assert np.array_equal(r.xyz, sc.problem().X0)


def test_the_start_up_shape():
    sc = SCENES["startup_two_keyframes"]
    r, _ = solved("startup_two_keyframes")
    assert (sc.nk, sc.nf, sc.checks, sc.robust[0], sc.iterations[0]) == (2, 1, False, False, 20)
    assert r.iterations[0] == 20 and r.iterations[1] == 0 and r.n_erase == 0 and np.all(r.state == L.KEPT)


def test_no_fixed_keyframe_and_mixed_keyframes():
    sc = SCENES["no_fixed_keyframe"]
    r, _ = solved("no_fixed_keyframe")
    assert sc.nf == sc.nk and r.iterations[0] == 5 and r.chi2[1] < r.chi2[0] * 2
    pr = SCENES["mixed_mono_stereo"].problem()
    assert pr.stereo.any() and (~pr.stereo).any()
    for i in range(pr.nf):
        assert len(pr.kf_edges[i])


def test_single_edge_point_and_point_seen_by_fixed_keyframes_only():
    sc = SCENES["single_edge_point"]
    r, _ = solved("single_edge_point")
    assert len(sc.problem().pt_edges[0]) == 1 and not np.array_equal(r.xyz[0], sc.problem().X0[0])
    sc = SCENES["point_seen_by_fixed_only"]
    pr = sc.problem()
    r, _ = solved("point_seen_by_fixed_only")
    assert not pr.free[pr.pt_edges[0]].any() and not np.array_equal(r.xyz[0], pr.X0[0])


def test_dropped_points():
    sc = SCENES["dropped_points"]
    r, _ = solved("dropped_points")
    for p in (0, 17, 39):
        assert np.all(r.state[sc.e_pt == p] == L.DROPPED) and np.all(r.xyz[p] == 0.0)
    assert r.n_edges == sc.ne - 18


def test_each_stop_case():
    r, _ = solved("stop_before")
    assert r.stopped == 1 and r.R is None and r.xyz is None
    r, _ = solved("stop_in_first")
    assert r.stopped == 2 and list(r.trials) == [2, 0] and r.n_removed_first == 0 and r.R is not None
    r, _ = solved("stop_in_second")
    assert r.stopped == 3 and r.trials[0] + r.trials[1] == 7 and r.n_removed_first >= 1
    r, _ = solved("stop_global_ba")
    assert r.stopped == 2 and list(r.trials) == [3, 0]


def test_the_empty_problems_evaluate_nothing():
    for name in ("empty_no_free", "empty_no_points", "empty_all_dropped"):
        r, log = solved(name)
        assert list(r.iterations) == [0, 0] and list(r.trials) == [0, 0] and not trials(log), name
        assert np.array_equal(r.xyz, SCENES[name].problem().X0)


SEEDED = ["chi2_first_mono", "chi2_first_stereo", "mixed_mono_stereo", "no_fixed_keyframe", "startup_two_keyframes", "single_edge_point"]


def full_system(pr, sy, on, lam):
    n, m = 6 * pr.nf, 3 * pr.np
    H, b = np.zeros((n + m, n + m)), np.zeros(n + m)
    for i in range(pr.nf):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = sy.Hpp[i]
        b[6 * i:6 * i + 6] = sy.bp[i]
    for p in range(pr.np):
        H[n + 3 * p:n + 3 * p + 3, n + 3 * p:n + 3 * p + 3] = sy.Hll[p]
        b[n + 3 * p:n + 3 * p + 3] = sy.bl[p]
    for e in range(pr.ne):
        if on[e] and pr.free[e]:
            i, p = pr.e_kf[e], pr.e_pt[e]
            H[6 * i:6 * i + 6, n + 3 * p:n + 3 * p + 3] = sy.W[e]
            H[n + 3 * p:n + 3 * p + 3, 6 * i:6 * i + 6] = sy.W[e].T
    return H + lam * np.eye(n + m), b


@pytest.mark.parametrize("name", SEEDED)
def test_the_schur_step_is_the_dense_solve_of_the_full_damped_system(name):
    pr = SCENES[name].problem()
    on = pr.p_on[pr.e_pt]
    sy = L.linearise(pr, pr.R0, pr.t0, pr.X0, on, True)
    lam = L.lambda_init(pr, sy)
    (dxp, dxl), why = L.schur_step(pr, sy, on, lam)
    H, b = full_system(pr, sy, on, lam)
    x = np.linalg.solve(H, b)
    got = np.concatenate([dxp.reshape(-1), dxl.reshape(-1)])
    rel = np.linalg.norm(got - x) / np.linalg.norm(x)
    print(name, "relative difference", rel)
    # measured over these scenes: at most 9.4e-14 (no_fixed_keyframe, where lambda alone holds the gauge; the others 3e-15 .. 1e-14); a
    # property of their conditioning, asserted with a factor of 10
    assert rel < 9.4e-13


@pytest.mark.parametrize("name", SEEDED)
def test_each_jacobian_is_the_central_difference_of_the_error(name):
    pr = SCENES[name].problem()
    h = F64(1e-6)
    xyz, e0, _ = L.edges_at(pr, pr.R0, pr.t0, pr.X0)
    Jl, Jp = L.jacobians(pr, pr.R0, xyz)
    worst = 0.0
    rows = lambda e: np.stack(e, 1)
    mask = np.stack([np.ones(pr.ne), np.ones(pr.ne), pr.stereo.astype(F64)], 1)   # row 2 is read on stereo edges only
    for c in range(3):
        d = np.zeros(3)
        d[c] = h
        num = (rows(L.edges_at(pr, pr.R0, pr.t0, pr.X0 + d)[1]) - rows(L.edges_at(pr, pr.R0, pr.t0, pr.X0 - d)[1])) / (2 * h)
        ana = np.stack([Jl[r][c] for r in range(3)], 1) * mask
        worst = max(worst, float(np.max(np.abs(num - ana) / (1.0 + np.abs(ana)))))
    for j in range(6):
        out = []
        for sgn in (1.0, -1.0):
            x = np.zeros(6)
            x[j] = sgn * h
            R, t = pr.R0.copy(), pr.t0.copy()
            for k in range(pr.nk):
                R[k], t[k] = exp_step(pr.R0[k], pr.t0[k], x)
            out.append(rows(L.edges_at(pr, R, t, pr.X0)[1]))
        num = (out[0] - out[1]) / (2 * h)
        ana = np.stack([Jp[r][j] for r in range(3)], 1) * mask
        worst = max(worst, float(np.max(np.abs(num - ana) / (1.0 + np.abs(ana)))))
    print(name, "worst |numeric - analytic| / (1 + |analytic|)", worst)
    # measured over these scenes: 2.0e-8 .. 3.4e-8 (the truncation and cancellation error of a central difference at 1e-6), asserted with a
    # factor of 10
    assert worst < 3.4e-7
