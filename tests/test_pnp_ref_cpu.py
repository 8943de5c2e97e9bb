"""CPU: the restatement tests/_pnp_ref.py (the normative semantics of afv_frame_pnp_hypotheses) on the constructed scenes of
tests/_pnp_scenes.py: each scene reaches the rule it is named for; the scan over records (PnPsolver of the package) equals the sequential
loop with Refine at every qualifying hypothesis; the restated Jacobi is held to numpy on the scenes' own matrices; the refined pose of
clean scenes reprojects exactly; SetRansacParameters at the reference's constants."""
import functools

import numpy as np
import pytest

import _pnp_ref as R
import _pnp_scenes as S

CONSTRUCTED = S.constructed()
IDS = [s.name for s, _ in CONSTRUCTED]


@functools.lru_cache(None)
def outputs(k):
    """the restatement's answer for scene k, computed once: (outputs, trace)"""
    trace = []
    return CONSTRUCTED[k][0].run(trace=trace), trace


def run_rules(s, out):
    rules = set()
    rec, m = np.flatnonzero(out["refined"]), out["min_inliers"]
    if out["degenerate"].any():
        rules.add("degenerate")
    if len(rec) >= 2 and out["refined_count"][rec[0]] <= m and (out["refined_count"][rec[1:]] > m).any():
        rules.add("record_refine_fails_then_succeeds")
    if len(rec) and (out["refined_count"][rec] <= m).all():
        T, no_more, vb, n = s.solver().iterate(5)
        if T is not None and no_more and n == out["count"][rec[-1]]:
            rules.add("ends_on_unrefined_best")
    if 4 <= out["n"] < m:
        T, no_more, vb, n = s.solver().iterate(5)
        if T is None and no_more and n == 0:
            rules.add("n_below_min_inliers")
    if out["n"] < 4 and not out["count"].any() and not out["degenerate"].any():
        rules.add("n_below_four")
    if out["n"] == m:
        sol = s.solver()
        if sol.nIterations == 1 and sol.mRansacMaxIts == 1:
            rules.add("min_inliers_equals_n")
    ids = s.rows[0][s.rows[0] >= 0]
    flags = s.store_flags[ids]
    if (flags == 0).any() and (flags & R.BAD).any() and out["n"] == int(((flags & R.SET) != 0).sum() - ((flags & R.BAD) != 0).sum()):
        rules.add("bad_and_unset_ids")
    return rules


@pytest.mark.parametrize("k", range(len(CONSTRUCTED)), ids=IDS)
def test_scene_reaches_its_rule(k):
    s, want = CONSTRUCTED[k]
    out, trace = outputs(k)
    got = S.rules_of(trace) | run_rules(s, out)
    assert want <= got, (s.name, sorted(want - got))


def test_every_rule_has_a_scene():
    need = {"winner1", "winner2", "winner3", "flip", "noflip", "detfix", "b1_negTrue", "b1_negFalse", "degenerate", "record_refine_fails_then_succeeds",
            "ends_on_unrefined_best", "n_below_min_inliers", "n_below_four", "min_inliers_equals_n", "bad_and_unset_ids"}
    for tag in ("b2", "b3"):
        need |= {"%s_neg%s_second%s" % (tag, a, b) for a in (True, False) for b in (True, False)} | {"%s_flip%s" % (tag, a) for a in (True, False)}
    have = set().union(*(w for _, w in CONSTRUCTED))
    assert need <= have, sorted(need - have)


def test_degenerate_by_eta_zero_and_by_beta_zero():
    """E8's first two clauses, at the functions that raise them: no 4-set of finite points was found that reaches them through epnp (a
    zero column of L needs control points that coincide exactly, and those make CC singular and the alphas NaN first: clause 3)"""
    info = {}
    L = [0.0] * 60
    assert R.qr_solve([0.0, 1.0, 0.0, 2.0, 0.0, 3.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0], [1.0] * 6, 6, 2, info) == [0.0, 0.0] and info["eta0"]
    info = {}
    R.betas_approx_1(L, [0.0] * 6, info)
    assert info["eta0"] and info["beta0"]
    info = {}
    for i in range(6):   # a system of full column rank
        L[10 * i:10 * i + 10] = [float(i + 1), float((i * i) % 5 + 1), float(i % 3), float((7 * i) % 4), float(i % 2 + 3), 0, float((3 * i) % 7 - 2), 0, 0, 0]
    rho = [L[10 * i + 1] for i in range(6)]
    R.betas_approx_1(L, rho, info)
    assert "eta0" not in info and "beta0" not in info
    info = {}
    R.betas_approx_1(L, [0.0] * 6, info)   # rho = 0: the least-squares answer is 0 and betas[0] = sqrt(0) is divided by
    assert info.get("beta0") and "eta0" not in info
    info = {}
    R.betas_approx_3(L, [0.0] * 6, info)
    assert info.get("beta0")


@pytest.mark.parametrize("k", range(len(CONSTRUCTED)), ids=IDS)
def test_scan_equals_the_sequential_loop(afv, k):
    """PnPsolver of the package (the scan over the device's arrays, here the restatement's) against Solver (Refine at every qualifying
    hypothesis): Tcw bits, masks, counts, bNoMore and mnIterations after each iterate(5)"""
    s, _ = CONSTRUCTED[k]
    out, _ = outputs(k)
    scan = afv.PnPsolver(out["n"], out["min_inliers"], out["index"], out["count"], out["degenerate"], out["pose"], out["inliers"], out["refined"],
                         out["refined_count"], out["refined_pose"], out["refined_inliers"], s.N, (s.min_inliers, s.epsilon, s.th2))
    seq = s.solver()
    assert (scan.mRansacMaxIts, scan.mRansacMinInliers, scan.nIterations) == (seq.mRansacMaxIts, seq.mRansacMinInliers, seq.nIterations)
    calls, compared = 0, 0
    while True:
        calls += 1
        if max(scan.mnIterations + 5, scan.mRansacMaxIts) > s.nhyp:   # Q1: what the next call would visit
            break
        a, b = scan.iterate(5), seq.iterate(5)
        assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2]), (s.name, calls)
        assert a[0] is None or a[0].tobytes() == b[0].tobytes(), (s.name, calls)
        assert scan.mnIterations == seq.mnIterations
        compared += 1
        if a[1] and calls > 2:
            break
    assert compared >= 1 and (seq.refines == 0 or seq.refines >= np.count_nonzero(out["refined"][:seq.mnIterations]))
    if scan.N >= scan.mRansacMinInliers:   # (a solver that says bNoMore at once visits no hypothesis)
        with pytest.raises(IndexError):    # Q1: every call runs five more hypotheses; one that would pass nhyp is refused
            for _ in range(s.nhyp + 2):
                scan.iterate(5)


def test_jacobi_against_numpy():
    """E1 / E2 on the scenes' own matrices.  12 x 12: every eigenvalue within 1e-12 x the largest of numpy.linalg.eigvalsh; the four used
    vectors orthonormal to 1e-12 with |MtM v| <= 1e-10 x the largest eigenvalue (for four points the null space is four-dimensional:
    single vectors are not comparable, residuals are).  3 x 3: the same two checks.  Double eps is 2.2e-16, 12 rows, a few hundred
    rotations: the bounds are a hundred times the expected error and far below what a wrong rotation produces.
    On the matrices of the 4-point hypotheses |MtM v| <= 1e-10 x the largest eigenvalue is asserted as it stands; on every matrix,
    those of the refinements included (their four smallest eigenvalues are not null), |MtM v - d v| is held to the same bound.
    Largest number of sweeps that rotated, over all finite matrices of the
    scenes: 12 x 12: 10, 3 x 3: 4 (the limit is 30)."""
    seen, sweeps12, sweeps3, null_sets = 0, 0, 0, 0
    for k in range(len(CONSTRUCTED)):
        for _, kind, info in outputs(k)[1]:
            if "mtm" not in info:
                continue
            for M, d, V, cols in ((np.array(info["mtm"]), np.array(info["d12"]), np.array(info["v12"]), info["col12"][8:]),
                                  (np.array(info["s3"]), np.array(info["d3"]), np.array(info["v3"]), [0, 1, 2])):
                if not np.isfinite(M).all():
                    continue
                w = np.linalg.eigvalsh(M)
                top = max(abs(w).max(), 1e-300)
                assert np.abs(np.sort(d) - w).max() <= 1e-12 * top
                U = V[:, cols]
                assert np.abs(U.T @ U - np.eye(len(cols))).max() <= 1e-12
                assert np.abs(M @ U - U * d[cols]).max() <= 1e-10 * top
                if len(d) == 12:
                    if kind == "hyp":   # four points: the four used vectors span the null space
                        assert np.abs(M @ U).max() <= 1e-10 * top
                        null_sets += 1
                    sweeps12 = max(sweeps12, info["sweeps12"])
                else:
                    sweeps3 = max(sweeps3, info["sweeps3"])
                seen += 1
    assert seen > 200 and null_sets > 100 and sweeps12 < R.JACOBI_SWEEPS and sweeps3 < R.JACOBI_SWEEPS
    print("sweeps", sweeps12, sweeps3)


@pytest.mark.parametrize("n,rs", ((20, 1), (33, 2), (64, 3), (129, 4)))
def test_clean_scenes_reproject_exactly(n, rs):
    """noise-free, all inliers, well spread, not coplanar: the refined pose reprojects every point to within 1e-2 px of its exact
    projection.  A condition, not a measurement: inputs are rounded to float32 (about 3e-5 px at 640) and a wrong EPnP misses by pixels.
    Largest value observed: 1.7e-5 px."""
    s = S.clean(n, rs, min_inliers=10, epsilon=0.5, nhyp=12)
    out = s.run()
    rec = np.flatnonzero(out["refined"] == 1)
    assert len(rec) and out["refined_count"][rec[-1]] == n, (out["count"], out["refined_count"])
    pose = out["refined_pose"][rec[-1]].astype(np.float64)
    Rm, t = pose[:9].reshape(3, 3), pose[9:]
    P = s.problem()
    fx, fy, cx, cy = s.cam
    X = P["p3dw"].astype(np.float64)
    Xe = X @ s.Rcw.T + s.tcw
    Xg = X @ Rm.T + t
    exact = np.stack([fx * Xe[:, 0] / Xe[:, 2] + cx, fy * Xe[:, 1] / Xe[:, 2] + cy], 1)
    got = np.stack([fx * Xg[:, 0] / Xg[:, 2] + cx, fy * Xg[:, 1] / Xg[:, 2] + cy], 1)
    worst = np.abs(got - exact).max()
    print("worst", worst)
    assert worst <= 1e-2


def test_ransac_parameters_at_the_references_constants():
    assert R.ransac_parameters(100, 0.99, 10, 300, 4, 0.5, 5.991)[3] == 35
    assert R.ransac_parameters(15, 0.99, 10, 300, 4, 0.5, 5.991)[3] == 14
