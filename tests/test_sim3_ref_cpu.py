"""CPU: the restatement of Sim3Solver (tests/_sim3_ref.py) and its scenes (tests/_sim3_scenes.py) - every constructed scene reaches the
rule it is named for, the S4 sampler is the literal vAvailableIndices walk, noise-free worlds are solved, and the restated Jacobi agrees
with numpy.linalg.eigh.

The Jacobi check (test_jacobi_rotation_against_eigh): 400 seeded symmetric N matrices built by horn_matrix from random 3 x 3 M (seeds
1000 .. 1399).  Condition: the two largest eigenvalues differ by at least 1e-3 of the largest in magnitude (below that the eigenvector is
ill-conditioned and two correct algorithms may differ by much more than rounding noise); all 400 seeds meet it, which the test asserts.
R12 of S3 is compared in double, before the float rounding, with the R12 built the same way from eigh's eigenvector.  Largest deviation of
an element of R12 found over them: 4.16e-15 (JACOBI_DEV); the bound is 16 x that, since the deviation is the rounding noise of two
different algorithms and moves by small factors with the seeds."""
import numpy as np
import pytest

import _sim3_ref as R
import _sim3_scenes as S

JACOBI_DEV = 4.16e-15
JACOBI_SEEDS = range(400)


def _gap_ok(w):
    return (w[-1] - w[-2]) >= 1e-3 * np.max(np.abs(w))


def test_jacobi_rotation_against_eigh():
    worst, kept = 0.0, 0
    for seed in JACOBI_SEEDS:
        rng = np.random.default_rng(1000 + seed)
        M = (rng.normal(size=(3, 3)) * 10.0 ** rng.uniform(-2, 2)).astype(np.float32)
        Nm = np.array(R.horn_matrix([[np.float32(v) for v in row] for row in M]), np.float64)
        assert np.array_equal(Nm, Nm.T)
        w, v = np.linalg.eigh(Nm)
        assert _gap_ok(w), seed
        kept += 1
        q, sweeps, lam = R.jacobi_max_eigenvector(Nm)
        assert 1 <= sweeps < R.JACOBI_SWEEPS
        assert abs(float(lam) - w[-1]) <= 1e-12 * np.max(np.abs(w))
        got = np.array(R.quaternion_rotation(q), np.float64)
        want = np.array(R.quaternion_rotation([np.float64(x) for x in v[:, -1]]), np.float64)
        worst = max(worst, float(np.max(np.abs(got - want))))
        assert np.allclose(got.reshape(3, 3) @ got.reshape(3, 3).T, np.eye(3), atol=1e-14)
    print("kept %d of %d matrices, largest deviation %.3g" % (kept, len(JACOBI_SEEDS), worst))
    assert kept == len(JACOBI_SEEDS)
    assert worst <= 16 * JACOBI_DEV, worst


def test_jacobi_ties_and_zero_matrix():
    q, sweeps, lam = R.jacobi_max_eigenvector(np.zeros((4, 4)))
    assert [float(x) for x in q] == [1, 0, 0, 0] and sweeps == 0 and lam == 0
    q, _, lam = R.jacobi_max_eigenvector(np.diag([1.0, 3.0, 3.0, -7.0]))
    assert [float(x) for x in q] == [0, 1, 0, 0] and lam == 3            # the lowest index of the tie
    assert [float(x) for x in R.quaternion_rotation([np.float64(-2.0), np.float64(0), np.float64(0), np.float64(0)])] == [1, 0, 0, 0, 1, 0, 0, 0, 1]


def test_sampler_is_the_literal_list_walk():
    for N in list(range(3, 40)) + [63, 64, 65, 257, 4096]:
        for h in range(60 if N < 40 else 8):
            for seed in (0, 1, 2 ** 63 + 12345):
                a, b = R.sample3(seed, h, N), R.sample3_closed(seed, h, N)
                assert a == b, (N, h, seed)
                assert len(set(a)) == 3 and all(0 <= i < N for i in a)
    # small N: every swap case occurs (the pick is the back; a later draw hits a moved entry)
    seen = set()
    for h in range(400):
        r0, r1, r2 = R.draws(7, h, 4)
        seen.add((r0 == 3, r1 == r0, r2 == r1, r2 == r0))
    assert len(seen) >= 6
    assert R.draws(0, 0, 10) != R.draws(0, 1, 10) and R.draws(0, 0, 10) != R.draws(1, 0, 10)


@pytest.mark.parametrize("s,fix", [(1.0, False), (0.5, False), (3.0, False), (1.0, True)])
def test_noise_free_worlds_are_solved_by_every_hypothesis(s, fix):
    sc = S.world(40 + int(s * 2), n=30, s=s, fix_scale=fix)
    ref = sc.candidate(64, 24, 2)
    assert ref["n"] == 30 and not ref["degenerate"].any()
    assert (ref["count"] == 30).all()
    assert (ref["inliers"][:, 0] == (1 << 30) - 1).all() and (ref["inliers"][:, 1] == 0).all()
    P = sc.planted
    for h in range(24):
        r = ref["sim3"][h]
        assert np.allclose(r[:9].reshape(3, 3), P["R12"], atol=2e-4) and np.allclose(r[9:12], P["t12"], atol=2e-3)
        assert abs(r[12] - P["s"]) < 1e-3 * P["s"] and (not fix or r[12] == 1)
    sol = sc.solver(ref, 24)
    sol.SetRansacParameters(0.99, 6, 24)
    T, no_more, vb, n_in = sol.iterate(5)
    assert T is not None and sol.mnIterations == 1 and not no_more and n_in == 30 and vb.all()
    assert np.array_equal(T[:3, :3].ravel(), np.float32(ref["sim3"][0][12]) * ref["sim3"][0][:9])


def test_outliers_and_noise_leave_the_planted_inliers():
    sc = S.world(77, n=40, s=0.5, outliers=0.25, noise=0.5)
    ref = sc.candidate(64, 40, 2)
    good = 40 - len(sc.planted["outliers"])
    assert good == 30 and ref["count"].max() >= good - 3 and ref["count"].min() < good // 2
    sol = sc.solver(ref, 40)
    sol.SetRansacParameters(0.99, 20, 40)
    T, vb, n_in = sol.find()
    assert T is not None and n_in > 20 and not vb[sorted(sc.planted["outliers"])].any()


def test_skip_reasons():
    sc = S.skip_reasons()
    G = sc.gather()
    assert len(sc.skipped) == 7
    assert G["index1"] == [i for i in range(sc.n1) if i not in sc.skipped]
    assert S.world(3, 24).gather()["n"] == 24                             # the same world without the skips keeps every feature


@pytest.mark.parametrize("above", [False, True])
def test_q1_truncated_bound(above):
    sc = S.q1_bound(above)
    G = sc.gather()
    K = sc.K
    assert float(G["max_err"][K][0]) == (14.0 if above else 13.0)
    assert 13.0 < 9.210 * float(sc.sigma2_1[K]) < 14.01
    seen = 0
    for h in range(12):
        H = sc.hypothesis(h, G)
        if K in H["picks"]:
            continue
        seen += 1
        e1, e2 = H["errs"][K]
        assert 13.4 < float(e1) < 13.6 and float(e1) < 9.210 * float(sc.sigma2_1[K]) and float(e2) < float(G["max_err"][K][1])
        assert H["flags"][K] == above and H["count"] == (12 if above else 11)
    assert seen >= 6
    assert float(R.max_error(-1.0)) == 0 and float(R.max_error(np.nan)) == 0 and float(R.max_error(np.inf)) == 0 and float(R.max_error(0.1)) == 0


def test_coincident_and_collinear_samples():
    H = S.coincident(False).hypothesis(0)
    assert H["degenerate"] == 1 and H["count"] == 0 and float(H["solve"]["den"]) == 0 and not H["sim3"].any()
    H = S.coincident(True).hypothesis(0)
    assert H["degenerate"] == 0 and H["count"] == 3 and H["sim3"].tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1, 0.25, 0, 0.5, 1]
    sc = S.collinear()
    for h in range(4):
        H = sc.hypothesis(h)
        Rm = H["sim3"][:9].reshape(3, 3).astype(np.float64)
        assert H["degenerate"] == 0 and np.isfinite(H["sim3"]).all() and np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-6)
        assert H["count"] == 3 and abs(H["sim3"][12] - 1) < 1e-6
        w = np.linalg.eigvalsh(np.array(H["solve"]["N"], np.float64))
        assert abs(w[-1] - w[-2]) < 1e-6 * abs(w[-1])                      # the double largest eigenvalue


@pytest.mark.parametrize("under_t21", [False, True])
def test_z_zero_is_no_inlier(under_t21):
    sc = S.z_zero(under_t21)
    H = sc.hypothesis(0)
    assert sc.K not in H["picks"] and H["degenerate"] == 0
    e = H["errs"][sc.K][1 if under_t21 else 0]
    assert not np.isfinite(e) and not H["flags"][sc.K] and H["count"] == 9
    X = R.rigid(H["solve"]["sRi" if under_t21 else "sR"], H["solve"]["ti" if under_t21 else "t"],
                sc.gather()["x1" if under_t21 else "x2"][sc.K])
    assert float(X[2]) == 0


def test_q2_counts_at_and_above_min_inliers():
    at = S.counted(6)
    ref = at.candidate(32, 60, 1)
    assert ref["n"] == 8 and ref["count"].max() == 6 and (ref["count"] == 6).sum() >= 2
    sol = at.solver(ref, 60)
    sol.SetRansacParameters(0.99, 6, 60)
    its = sol.mRansacMaxIts
    assert 2 < its <= 60
    T, vb, n_in = sol.find()
    assert T is None and n_in == 0 and not vb.any() and sol.mnIterations == its and sol.mnBestInliers == 6
    sixes = [h for h in range(its) if ref["count"][h] == 6]
    assert len(sixes) >= 2 and sol.best == sixes[-1]                       # equal counts in a row: >= keeps the LAST
    above = S.counted(7)
    ref = above.candidate(32, 60, 1)
    assert ref["count"].max() == 7
    sol = above.solver(ref, 60)
    sol.SetRansacParameters(0.99, 6, 60)
    first = int(np.nonzero(ref["count"] == 7)[0][0])
    assert 0 < first < sol.mRansacMaxIts
    T, no_more, vb, n_in = sol.iterate(first)                              # stops one short of it
    assert T is None and not no_more
    T, no_more, vb, n_in = sol.iterate(5)
    assert T is not None and n_in == 7 and vb.sum() == 7 and sol.mnIterations == first + 1 and vb[:7].all()


def test_n_equal_to_and_below_min_inliers():
    sc = S.world(9, n=6, levels=False)
    ref = sc.candidate(16, 8, 1)
    sol = sc.solver(ref, 8)
    sol.SetRansacParameters(0.99, 6, 8)
    assert ref["n"] == 6 and sol.mRansacMaxIts == 1
    T, no_more, vb, n_in = sol.iterate(5)
    assert T is None and no_more and sol.mnIterations == 1 and sol.mnBestInliers == 6   # 6 > 6 is false
    sc = S.world(9, n=5, levels=False)
    sol = sc.solver(sc.candidate(16, 8, 1), 8)
    T, no_more, vb, n_in = sol.iterate(5)
    assert T is None and no_more and sol.mnIterations == 0 and len(vb) == 5
    with pytest.raises(ValueError):
        sol.SetRansacParameters(0.99, 6, 9)
    with pytest.raises(ValueError):
        sol.SetRansacParameters(0.99, 2, 8)


@pytest.mark.parametrize("n", [0, 2, 3])
def test_tiny_n(n):
    sc = S.world(12, n=n, levels=False)
    ref = sc.candidate(8, 5, 1)
    assert ref["n"] == n
    if n < 3:
        assert not ref["count"].any() and not ref["degenerate"].any() and not ref["sim3"].any() and not ref["inliers"].any()
    else:
        assert (ref["count"] == 3).all() and (ref["inliers"] == 7).all()
    assert R.ransac_iterations(0.99, 6, 300, n) >= 1


def test_q3_iteration_counts():
    assert R.ransac_iterations(0.99, 6, 300, 6) == 1
    assert R.ransac_iterations(0.99, 6, 300, 12) == 35                     # eps = 0.5: ceil(log(0.01) / log(0.875))
    assert R.ransac_iterations(0.99, 6, 300, 150) == 300
    assert R.ransac_iterations(0.99, 20, 300, 25) == 7
    assert R.ransac_iterations(0.99, 6, 5, 150) == 5
