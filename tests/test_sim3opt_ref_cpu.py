"""CPU: the restatement of OptimizeSim3 (tests/_sim3opt_ref.py) on the constructed scenes (tests/_sim3opt_scenes.py).  Every scene reaches
the rule it is named after (read from the restatement's trace), the numeric Jacobian is held to an analytic one, exp(sigma) to math.exp,
and noise-free scenes converge with every correspondence an inlier."""
import math

import numpy as np
import pytest

import _sim3opt_ref as R
import _sim3opt_scenes as S

_cache = {}


def solved(name):
    if name not in _cache:
        sc = S.every_scene()[name]
        log = []
        _cache[name] = (sc, sc.problem(), sc.solve(log), log)
    return _cache[name]


def trials(log, stage=None):
    stages = log if stage is None else [log[stage]]
    return [e for L in stages for e in L if "accepted" in e]


def test_clean_set_takes_the_low_branch():
    sc, pr, r, log = solved("clean")
    assert r.n_corr == 40 and r.n_bad == 0 and r.more_iterations == 5 and not r.early and r.n_in == 40
    assert r.iterations[0] == 5 and 1 <= r.iterations[1] <= 5
    assert (r.state == R.KEPT).all() and np.array_equal(r.mp2_out, sc.mp2)


def test_planted_outliers_take_the_high_branch():
    sc, pr, r, log = solved("planted_outliers")
    assert r.n_bad > 0 and r.more_iterations == 10 and not r.early and r.iterations[1] > 5
    removed = set(np.nonzero(r.state == R.REMOVED_FIRST)[0])
    assert removed >= sc.planted["outliers"] or len(removed & sc.planted["outliers"]) >= 6   # the planted ones are what goes
    assert r.n_in == r.n_corr - r.n_bad - int((r.state == R.REMOVED_SECOND).sum())
    assert (r.mp2_out[r.state >= R.REMOVED_FIRST] == -1).all() and (r.mp2_out[r.state == R.KEPT] >= 0).all()


def test_exactly_ten_survivors_proceed_and_nine_return_zero():
    sc, pr, r, log = solved("survivors_10")
    assert r.n_corr == 13 and r.n_bad == 3 and r.n_corr - r.n_bad == 10 and not r.early and r.iterations[1] > 0 and r.n_in == 10
    assert sorted(np.nonzero(r.state == R.REMOVED_FIRST)[0]) == [1, 4, 7]
    sc, pr, r, log = solved("survivors_9")
    assert r.n_corr == 12 and r.n_bad == 3 and r.early == 1 and r.n_in == 0 and r.iterations[1] == 0 and r.trials[1] == 0
    assert r.more_iterations == 10                                     # decided before the return
    start = np.concatenate([sc.R12, sc.t12, [sc.s12]]).astype(np.float64)
    assert np.concatenate([r.R12, r.t12, [r.s12]]).tobytes() == start.tobytes()   # g2oS12 is not written back
    assert sorted(np.nonzero(r.mp2_out == -1)[0]) == [1, 4, 7]       # the first removals stand
    assert (r.state[[0, 2, 3]] == R.KEPT).all()


@pytest.mark.parametrize("which", [1, 2])
def test_one_edge_alone_removes_the_match(which):
    sc, pr, r, log = solved("only_e12" if which == 1 else "only_e21")
    k = list(pr.index1).index(sc.K)
    c12, c21 = r.first_chi2
    over = (c12[k] > pr.th2, c21[k] > pr.th2)
    assert over == ((True, False) if which == 1 else (False, True))
    assert r.state[sc.K] == R.REMOVED_FIRST and r.n_bad == 1 and r.mp2_out[sc.K] == -1


def test_second_classification_removes_a_match_the_first_passed():
    sc, pr, r, log = solved("second_removal")
    second = np.nonzero(r.state == R.REMOVED_SECOND)[0]
    assert len(second) >= 1 and not r.early
    for i in second:
        k = list(pr.index1).index(i)
        assert r.first_chi2[0][k] <= pr.th2 and r.first_chi2[1][k] <= pr.th2
        assert r.second_chi2[0][k] > pr.th2 or r.second_chi2[1][k] > pr.th2
        assert r.mp2_out[i] == -1
    assert r.n_in == r.n_corr - r.n_bad - len(second)


def test_fix_scale_leaves_the_bits_of_the_scale():
    sc, pr, r, log = solved("fixed_scale")
    assert not r.early and r.iterations[1] > 0 and any(e["accepted"] for e in trials(log))
    assert np.float64(r.s12).tobytes() == np.float64(sc.s12).tobytes()
    assert r.R12.tobytes() != sc.R12.astype(np.float64).tobytes()      # ... while the rest moved
    H, b, _ = R.linearise(pr, (sc.R12.reshape(3, 3).astype(np.float64), sc.t12.astype(np.float64), np.float64(sc.s12)), np.ones(pr.n, bool))
    assert not H[6].any() and not H[:, 6].any() and b[6] == 0.0         # O6: row 6 holds lambda alone


def test_every_filter_clause_is_no_edge_and_stays_in_the_list():
    sc, pr, r, log = solved("filter_clauses")
    assert r.n_corr == 32 - len(S.FILTER_CLAUSES)
    for i, why in S.FILTER_CLAUSES.items():
        assert i not in pr.index1, why
        if why == "mp2 < 0":
            assert r.state[i] == R.NO_MATCH and r.mp2_out[i] == -1
        else:
            assert r.state[i] == R.NOT_EDGE and r.mp2_out[i] == sc.mp2[i] >= 0, why   # the quirk: the match is kept


def test_a_point_behind_the_camera_is_a_finite_outlier():
    sc, pr, r, log = solved("behind_camera")
    k = list(pr.index1).index(sc.K)
    E0 = (sc.R12.reshape(3, 3).astype(np.float64), sc.t12.astype(np.float64), np.float64(sc.s12))
    q2 = E0[2] * (E0[0][2, 0] * pr.p2[k, 0] + (E0[0][2, 1] * pr.p2[k, 1] + E0[0][2, 2] * pr.p2[k, 2])) + E0[1][2]
    assert q2 < 0                                                       # z <= 0 in camera 1
    assert np.isfinite(r.first_chi2[0][k]) and r.first_chi2[0][k] > pr.th2 and r.state[sc.K] == R.REMOVED_FIRST
    assert np.isfinite(r.chi2).all() and np.isfinite(r.R12).all()


def test_a_far_start_has_a_rejected_trial():
    sc, pr, r, log = solved("rejected_trial")
    t = trials(log)
    assert any(not e["accepted"] for e in t) and any(e["accepted"] for e in t) and not r.early
    assert r.trials[0] + r.trials[1] == len(t) and r.trials[0] + r.trials[1] > r.iterations[0] + r.iterations[1]


def test_no_edges_and_few_edges():
    sc, pr, r, log = solved("no_edges")
    assert pr.n == 0 and r.n_corr == 0 and r.early == 1 and r.n_in == 0 and not r.iterations.any() and not r.trials.any()   # O7
    assert (r.state == R.NOT_EDGE).all() and np.array_equal(r.mp2_out, sc.mp2)
    sc, pr, r, log = solved("few_edges")
    assert r.n_corr == 6 and r.iterations[0] > 0 and r.early == 1 and r.n_in == 0 and r.iterations[1] == 0
    assert np.array_equal(r.mp2_out, sc.mp2) and r.s12 == np.float64(sc.s12)


def analytic_jacobians(pr, E):
    """d e12 / d u and d e21 / d u at u = 0 for estimate <- Sim3(u) * estimate, u = (omega, upsilon, sigma)"""
    Rm, t, s = E
    skew = lambda v: np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    J12, J21 = np.zeros((pr.n, 2, 7)), np.zeros((pr.n, 2, 7))
    for k in range(pr.n):
        q = s * (Rm @ pr.p2[k]) + t                                     # exp(u) q = q + omega x q + upsilon + sigma q + O(u^2)
        dq = np.concatenate([-skew(q), np.eye(3), q[:, None]], 1)
        fx, fy = pr.K1[0], pr.K1[1]
        dpi = np.array([[fx / q[2], 0, -fx * q[0] / q[2] ** 2], [0, fy / q[2], -fy * q[1] / q[2] ** 2]])
        J12[k] = -dpi @ dq
        q = (Rm.T @ (pr.p1[k] - t)) / s                                 # (exp(u) S)^-1 X = S^-1 (X - omega x X - upsilon - sigma X) + O(u^2)
        A = Rm.T / s
        dq = np.concatenate([A @ skew(pr.p1[k]), -A, -(A @ pr.p1[k])[:, None]], 1)
        fx, fy = pr.K2[0], pr.K2[1]
        dpi = np.array([[fx / q[2], 0, -fx * q[0] / q[2] ** 2], [0, fy / q[2], -fy * q[1] / q[2] ** 2]])
        J21[k] = -dpi @ dq
    return J12, J21


def test_numeric_jacobian_against_the_analytic_one():
    """Central differences at delta = 1e-9 cannot be better than the rounding noise of the two projections they subtract.  The bound is
    derived from the scene's geometry, not from what the code gives.  A projected coordinate u = f (x / z) + c carries (a) the rounding of
    q = s (R X) + t: at most 10 roundings (3 products, 2 sums, the scale, the translation, and up to 3 more for the perturbed estimate's own
    entries), each at most 2^-53 of the largest magnitude qmax met, so |dq| <= 10 * 2^-53 * qmax per component; through the projection
    that is (fmax / zmin) * (1 + rmax) * |dq| with rmax the largest |x / z|, |y / z|; and (b) 4 roundings of its own (division, product,
    the two sums) of at most ulp(cmax) / 2 each, cmax the largest coordinate.  Two such values are subtracted and divided by 2 * delta, so
    the noise of a Jacobian entry is at most E_u / delta.  The truncation error of the central difference is delta^2 times a third
    derivative of order |J|: below 1e-15, ignored.  Allowed factor over that worst case: 1 - it is a worst-case sum already."""
    for name in ("clean", "planted_outliers", "fixed_scale"):
        sc, pr, r, log = solved(name)
        E = (sc.R12.reshape(3, 3).astype(np.float64), sc.t12.astype(np.float64), np.float64(sc.s12))
        num12, num21 = R.jacobians(pr, E)
        ana12, ana21 = analytic_jacobians(pr, E)
        q12 = np.array([E[2] * (E[0] @ p) + E[1] for p in pr.p2])
        q21 = np.array([(E[0].T @ (p - E[1])) / E[2] for p in pr.p1])
        worst = 0.0
        for q, X, K, obs, num, ana in ((q12, pr.p2, pr.K1, pr.obs1, num12, ana12), (q21, pr.p1, pr.K2, pr.obs2, num21, ana21)):
            qmax = max(np.abs(q).max(), np.abs(X).max() * max(1.0, E[2], 1.0 / E[2]))
            zmin = q[:, 2].min()
            assert zmin > 1.0
            rmax = max(np.abs(q[:, 0] / q[:, 2]).max(), np.abs(q[:, 1] / q[:, 2]).max())
            fmax = max(K[0], K[1])
            u = np.stack([K[0] * q[:, 0] / q[:, 2] + K[2], K[1] * q[:, 1] / q[:, 2] + K[3]], 1)
            cmax = max(np.abs(u).max(), np.abs(obs).max())
            e_u = (fmax / zmin) * (1.0 + rmax) * 10 * 2.0 ** -53 * qmax + 4 * math.ulp(cmax) / 2
            bound = e_u / float(R.DELTA)
            cols = range(6) if pr.fix_scale else range(7)            # under fix_scale the numeric scale column is exactly zero (O6)
            for d in cols:
                diff = max(np.abs(num[0][d] - ana[:, 0, d]).max(), np.abs(num[1][d] - ana[:, 1, d]).max())
                worst = max(worst, diff / bound)
                print("%s column %d: |numeric - analytic| max %.3e, bound %.3e (ulp(cmax) / delta = %.3e)" % (name, d, diff, bound, math.ulp(cmax) / 1e-9))
                assert diff <= bound, (name, d, diff, bound)
            if pr.fix_scale:
                assert not np.any(num[0][6]) and not np.any(num[1][6])
        assert worst > 1e-4                                             # the bound is not vacuous: the noise is within four decades of it


def test_exp_sigma_against_math_exp():
    """O4: the asserted bound is the maximum measured here (1.0 ulp), rounded up to the next whole ulp, plus one: 2 ulp"""
    rng = np.random.default_rng(5)
    xs = np.concatenate([np.linspace(-64.0, 64.0, 40001), rng.uniform(-64, 64, 20000), rng.uniform(-1e-3, 1e-3, 5000),
                         (np.arange(-92, 93) + 0.5) * math.log(2.0), [0.0, 1e-9, -1e-9, 64.0, -64.0]])
    worst = 0.0
    for x in xs:
        want = math.exp(float(x))
        worst = max(worst, abs(float(R.exp_sigma(x)) - want) / math.ulp(want))
    print("exp_sigma: worst error %.3f ulp over %d arguments in [-64, 64]" % (worst, len(xs)))
    assert worst <= 2.0
    assert R.exp_sigma(0.0) == 1.0                                      # exact: what O6 rests on
    assert R.sim3_exp([0, 0, 0, 0, 0, 0, 64.5]) is None and R.sim3_exp([0, 0, 0, 0, 0, 0, float("nan")]) is None
    assert R.sim3_exp([3.2, 0, 0, 0, 0, 0, 0]) is None and R.sim3_exp([3.1, 0, 0, 0, 0, 0, 0]) is not None


def test_sim3_exp_branches_agree_with_the_closed_form():
    """the four branches of Sim3(Vector7) against scipy-free closed forms in numpy: R by Rodrigues, s = e^sigma, t = W upsilon with W summed
    from its series"""
    rng = np.random.default_rng(9)
    for om, sg in ((1e-7, 1e-7), (0.3, 1e-7), (1e-7, 0.2), (0.3, 0.2), (2.5, -0.7)):
        w = rng.normal(size=3)
        w = w / np.linalg.norm(w) * om
        ups = rng.normal(size=3)
        dR, dt, ds = R.sim3_exp(list(w) + list(ups) + [sg])
        K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        M = np.zeros((4, 4))
        M[:3, :3] = K + sg * np.eye(3)
        M[:3, 3] = ups
        term, total = np.eye(4), np.eye(4)
        for n in range(1, 40):
            term = term @ M / n
            total = total + term
        assert abs(ds - math.exp(sg)) <= 4 * math.ulp(math.exp(sg))
        tol = 1e-12 if om > 1e-5 else 2e-14 + om * om                  # theta < eps: R = I + Omega + Omega^2 as written upstream, O(theta^2) off
        assert np.abs(np.array(dR) * ds - total[:3, :3]).max() <= tol + 1e-13
        if not (om < 1e-5 and abs(sg) >= 1e-5):                         # that branch's B is upstream's as written (no "- 1"): only R and s are held
            # a branch taken on |sigma| < eps or theta < eps uses the coefficients AT zero: first order in the small quantity is dropped
            small = (abs(sg) if abs(sg) < 1e-5 else 0.0) + (om if om < 1e-5 else 0.0)
            assert np.abs(np.array(dt) - total[:3, 3]).max() <= 1e-12 + 2 * small * np.abs(ups).sum()


@pytest.mark.parametrize("seed,s", [(11, 1.0), (31, 0.5), (32, 3.0)])
def test_noise_free_scenes_converge(seed, s):
    sc = S.clean(seed, n=40, s=s)
    pr = sc.problem()
    log = []
    r = sc.solve(log)
    E0 = (sc.R12.reshape(3, 3).astype(np.float64), sc.t12.astype(np.float64), np.float64(sc.s12))
    before = sum(float(c.sum()) for c in R.edge_chi2(pr, E0))
    after = sum(float(c.sum()) for c in R.edge_chi2(pr, (r.R12.reshape(3, 3), r.t12, r.s12)))
    print("seed %d: summed chi2 %.6g -> %.6g" % (seed, before, after))
    assert after < before and after < 1e-3
    assert r.n_in == r.n_corr == 40 and r.n_bad == 0 and r.more_iterations == 5 and (r.state == R.KEPT).all()
    P = sc.planted
    assert abs(r.s12 - P["s"]) < 1e-4 * P["s"] and np.abs(r.t12 - P["t12"]).max() < 1e-3
