"""CPU: the restatement of Optimizer::PoseOptimization (tests/_poseopt_ref.py) against what does not depend on it - central differences,
math.sin / math.cos and exact rational series, properties that hold by construction, planted outliers - and the proof that every
constructed scene of tests/_poseopt_scenes.py reaches the rule it is named after."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _poseopt_ref as R
import _poseopt_scenes as S

CONSTRUCTED = S.constructed()
ULP1 = 2.0 ** -52


def test_jacobians_against_central_differences():
    """linearizeOplus against (e(+h) - e(-h)) / 2h of the restated error through exp_step, h = 1e-6, float64, on 18 random scenes of 500
    features (mono, stereo, mixed): the largest deviation of an entry, relative to the largest entry of that edge's Jacobian, measured
    2.2e-10 (rounding of the error, ~1e-16 * 300 px / 1e-6, over entries of ~500).  Asserted: ten times that, plus 1e-10 for the
    truncation term h^2 f''' / 6 of the central difference."""
    h, worst = 1e-6, 0.0
    for seed in range(6):
        for kind in ("mono", "stereo", "mixed"):
            s = S.random_scene(seed, 500, kind)
            pr = s.problem()
            R0, t0 = s.Rcw.astype(np.float64), s.tcw.astype(np.float64)
            J = R.edge_jacobian(pr, R0, t0)
            scale = np.max(np.abs(np.stack([np.stack(J[k]) for k in range(3)])), axis=(0, 1))
            for j in range(6):
                d = np.zeros(6)
                d[j] = h
                ep, _ = R.edge_error(pr, *R.exp_step(R0, t0, d))
                em, _ = R.edge_error(pr, *R.exp_step(R0, t0, -d))
                for k in range(3):
                    ana = np.where(pr.stereo | (k < 2), J[k][j], 0.0)
                    dev = np.abs((ep[k] - em[k]) / (2 * h) - ana)[pr.edge] / scale[pr.edge]
                    worst = max(worst, float(dev.max()))
    print("largest relative deviation: %.3g" % worst)
    assert worst <= 10 * 2.2e-10 + 1e-10


def _series_exact(off, t2, terms=40):
    """sum (-1)^k t2^k / (2k + off)! as a Fraction (40 terms: the remainder is below 1e-60 on [0, pi^2])"""
    t2 = Fraction(t2)
    acc, p, f = Fraction(0), Fraction(1), math.factorial(off)
    for k in range(terms):
        acc += (-1) ** k * p / f
        p *= t2
        f *= (2 * k + off + 1) * (2 * k + off + 2)
    return acc


def _ulps(got, want):
    """|got - want| in ulps of `want` (want: a float, or an exact Fraction rounded for the ulp)"""
    w = float(want)
    return float(abs(Fraction(got) - Fraction(want)) / Fraction(math.ulp(w)))


def test_exponential_map_polynomials():
    """P4: the Horner polynomials against math.sin / math.cos, 4 ulp of the VALUE, over theta in [0, pi], and against the exact rational
    series (what both approximate).  Measured, in ulps of the value, against the series: (1 - cos)/th^2 2.9, (th - sin)/th^3 1.6 over
    [0, pi]; sin/th 0.8 up to th = 1, 2.3 up to 2 - and 5.8 at 2.5, 29 at 3.0, 88 at 3.1, unbounded at pi, where sin/th crosses zero while
    its alternating series still has terms of size 1.6: the polynomial in th^2 does NOT meet 4 ulp of the value beyond th = 2.  That is
    P4's documented accuracy (restatement, kernel header): sin/th within 4 ulp of its value for th <= 2 and within 2^-52
    absolute (measured 1.9e-16) up to pi.  The test holds the table to exactly that.
    References: sin(th)/th; (1 - cos th)/th^2 both as 2 sin^2(th/2)/th^2 (every th) and as written (th >= 1); (th - sin th)/th^3 as written
    for th >= 1 only - below, that expression itself is wrong by 12 ulp at 0.5 and 53 at 0.25 (its subtraction cancels), so the series is
    the reference there."""
    assert len(R.EXP_A) == len(R.EXP_B) == len(R.EXP_C) == 16
    for k in range(16):   # the table is the correctly rounded 1 / n! with alternating signs
        for tab, off in ((R.EXP_A, 1), (R.EXP_B, 2), (R.EXP_C, 3)):
            assert tab[k] == float(Fraction((-1) ** k, math.factorial(2 * k + off)))
    assert R.PI2 == math.pi * math.pi
    rs = np.random.RandomState(0)
    thetas = np.concatenate([np.linspace(0.0, math.pi, 1501), rs.uniform(0, math.pi, 500), [math.pi, 1e-8, 1e-3, 2.0]])
    worst = {"A<=2": 0.0, "A abs": 0.0, "B": 0.0, "C": 0.0}
    for th in thetas:
        th = float(th)
        t2 = np.float64(th) * np.float64(th)
        if t2 > R.PI2:
            continue
        a, b, c = (float(R.horner(t, t2)) for t in (R.EXP_A, R.EXP_B, R.EXP_C))
        ea, eb, ec = (_series_exact(off, float(t2)) for off in (1, 2, 3))
        worst["B"] = max(worst["B"], _ulps(b, eb))
        worst["C"] = max(worst["C"], _ulps(c, ec))
        worst["A abs"] = max(worst["A abs"], abs(a - float(ea)))
        if th <= 2.0:
            worst["A<=2"] = max(worst["A<=2"], _ulps(a, ea))
        if th > 0:
            assert _ulps(b, 2.0 * math.sin(th / 2) ** 2 / (th * th)) <= 4
            if th <= 2.0:
                assert _ulps(a, math.sin(th) / th) <= 4
            else:
                assert abs(a - math.sin(th) / th) <= ULP1       # P4's documented accuracy beyond th = 2
        if th >= 1.0:
            assert _ulps(b, (1.0 - math.cos(th)) / (th * th)) <= 4
            assert _ulps(c, (th - math.sin(th)) / th ** 3) <= 4
    print("against the exact series:", worst)
    assert worst["B"] <= 4 and worst["C"] <= 4 and worst["A<=2"] <= 4 and worst["A abs"] <= ULP1
    assert R.exp_step(np.eye(3), np.zeros(3), [1.8138, 1.8138, 1.8138, 0, 0, 0]) is None      # theta^2 = 9.8699 > pi^2
    assert R.exp_step(np.eye(3), np.zeros(3), [1.8137, 1.8137, 1.8137, 0, 0, 0]) is not None  # theta^2 = 9.8685
    Rn, _ = R.exp_step(np.eye(3), np.zeros(3), [0.3, -0.2, 0.5, 0, 0, 0])
    assert np.abs(Rn @ Rn.T - np.eye(3)).max() < 1e-15


def test_robust_chi2_never_rises_over_an_accepted_step():
    """by construction: a trial is accepted when rho = (before - after) / scale > 0, and scale = x^T (lambda x + b) + 1e-3 is positive"""
    n_acc = 0
    for s in [c[0] for c in CONSTRUCTED] + [S.random_scene(k, 300) for k in range(3)]:
        log = []
        res = s.run(log=log)
        for r, rl in enumerate(log):
            before = None
            for e in rl:
                if "trial" not in e:
                    continue
                if before is not None:
                    assert e["before"] == before      # what the next trial starts from is what the last accepted one left
                if e["accepted"]:
                    assert e["after"] < e["before"]
                    before = e["after"]
                    n_acc += 1
                else:
                    before = e["before"]
            if before is not None:
                assert res.chi2[r] == before
    assert n_acc > 100


@pytest.mark.parametrize("kind", ("mono", "stereo", "mixed"))
def test_planted_outliers_are_exactly_the_flagged_edges(kind):
    for seed in range(4):
        s = S.make("planted", 100 + seed, 400, stereo=kind, noise=0.0, outliers=0.1, out_px=50.0)
        res = s.run()
        assert s.planted.sum() >= 20
        assert np.array_equal(res.outlier != 0, s.planted), (kind, seed)
        assert res.n_good == res.n_edges - int(s.planted.sum()) and res.rounds == 4


def test_padding_the_tree_is_neutral():
    """P5: no leaf is -0.0, so the zero leaves of a larger power of two change no bit (the kernel's tree has at least 1024 leaves)"""
    for s in (S.random_scene(1, 70), CONSTRUCTED[3][0], CONSTRUCTED[4][0]):
        a = s.run()
        pr = s.problem()
        pr.P = 1024
        b = R.pose_optimization(pr, s.Rcw, s.tcw)
        assert a.Rcw.tobytes() == b.Rcw.tobytes() and a.tcw.tobytes() == b.tcw.tobytes() and np.array_equal(a.outlier, b.outlier)
        assert a.chi2.tobytes() == b.chi2.tobytes() or (np.isnan(a.chi2) == np.isnan(b.chi2)).all()
        assert np.array_equal(a.trials, b.trials)
    pr = S.random_scene(1, 70).problem()
    assert math.copysign(1.0, R.tree_sum(pr, np.full(70, -0.0), pr.edge)) == 1.0


@pytest.mark.parametrize("case", CONSTRUCTED, ids=[s.name for s, _ in CONSTRUCTED])
def test_scene_reaches_its_rule(case):
    scene, rule = case
    assert S.reaches(scene, rule), (scene.name, rule)


def test_few_edges_leave_pose_and_flags():
    s = [c[0] for c in CONSTRUCTED if c[0].name == "edges-2"][0]
    res = s.run()
    assert res.n_good == 0 and res.rounds == 0 and not res.outlier.any()
    assert res.Rcw.tobytes() == s.Rcw.tobytes() and res.tcw.tobytes() == s.tcw.tobytes()
