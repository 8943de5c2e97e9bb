"""CPU: the restatement tests/_init_ref.py on the constructed scenes of tests/_init_scenes.py.  Every scene reaches the rule it is named
for (read from the restatement's trace); the success scenes return the motion hypothesis closest to the scene's true motion; the restated
Jacobi agrees with numpy.linalg.svd; the sign of H21 / F21 reaches no output; the draws without the N-sized list are the literal ones."""
import numpy as np
import pytest

import _init_ref as R
import _init_scenes as S

H, F = R.ROUTE_H, R.ROUTE_F
# scene -> (ok, route, reason)
EXPECT = {
    "plane": (1, H, R.OK), "cloud": (1, F, R.OK), "outliers": (1, F, R.OK),
    "low_parallax": (0, F, R.PARALLAX), "pure_rotation": (0, H, R.AMBIGUOUS), "ambiguous": (0, H, R.AMBIGUOUS),
    "few_good": (0, F, R.MIN_TRI), "d_ratio": (0, H, R.DRATIO), "repeated": (0, F, R.MIN_TRI), "all_repeated": (0, F, R.MIN_TRI),
    "rh_above": (0, H, R.AMBIGUOUS), "rh_below": (0, F, R.MIN_TRI), "iter200": (0, F, R.MIN_TRI),
    "n7": (0, F, R.TOO_FEW_MATCHES), "n8": (0, F, R.MIN_TRI), "n9": (0, F, R.MIN_TRI), "n63": (1, F, R.OK), "n64": (1, F, R.OK),
    "n65": (1, F, R.OK), "n129": (1, F, R.OK),
    "iter1": (0, F, R.MIN_TRI), "iter63": (0, F, R.MIN_TRI), "iter64": (0, F, R.MIN_TRI), "iter65": (0, F, R.MIN_TRI),
    "cos1": (0, F, R.MIN_TRI), "cos50": (1, F, R.OK), "cos51": (1, F, R.OK), "cos52": (1, F, R.OK),
}
SUCCESS = sorted(k for k, v in EXPECT.items() if v[0])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def test_every_scene_is_listed():
    assert sorted(EXPECT) == sorted(S.SCENES)


@pytest.mark.parametrize("name", sorted(EXPECT))
def test_scene_reaches_its_rule(name):
    out, tr, sc = S.reference(name), S.reference(name)["trace"], S.scene(name)
    assert (out["ok"], out["route"], tr["reason"]) == EXPECT[name], (R.REASONS[tr["reason"]], tr["RH"])
    assert tr["N"] == int(np.sum(sc.matches12 >= 0))
    if tr["N"] >= 8:
        assert len(out["hyp"][0]) == len(out["hyp"][1]) == sc.iterations
        assert (tr["RH"] > R.MIN_RH) == (out["route"] == H)
    if out["ok"]:
        k = tr["best_motion"]
        assert tr["checks"][k]["n_good"] == max(c["n_good"] for c in tr["checks"]) >= R.MIN_TRIANGULATED
        assert out["triangulated"].sum() > 0 and np.all(out["triangulated"] <= (sc.matches12 >= 0))
        assert np.all(out["p3d"][sc.matches12 < 0] == 0) and np.all(out["p3d"][out["triangulated"] == 1][:, 2] > 0)
    else:
        assert not out["R21"].any() and not out["t21"].any() and not out["p3d"].any() and not out["triangulated"].any()


def test_the_rules_behind_the_names():
    ref = lambda n: S.reference(n)["trace"]
    # plane: RH > 0.40, ReconstructH's eight hypotheses; cloud: ReconstructF's four
    assert ref("plane")["RH"] > 0.45 and ref("plane")["n_motion"] == 8 and ref("cloud")["RH"] < 0.2 and ref("cloud")["n_motion"] == 4
    # low_parallax: a unique winner with everything good, refused only because its 50th smallest cosine is above cos(1 degree)
    tr = ref("low_parallax")
    g = [c["n_good"] for c in tr["checks"]]
    assert max(g) == 100 and sorted(g)[-2] == 0 and R.COS_MIN_PARALLAX <= tr["checks"][g.index(100)]["cos"] < R.MIN_COS
    # pure_rotation: every point is seen without parallax, so the depth tests are skipped, several hypotheses count every point and the
    # call is refused as ambiguous BEFORE the parallax rule is reached (the rules as written; see tests/_init_scenes.py)
    tr = ref("pure_rotation")
    g = [c["n_good"] for c in tr["checks"]]
    assert sorted(g)[-2:] == [100, 100] and all(c["cos"] > R.COS_MIN_PARALLAX for c in tr["checks"])
    # few_good: fewer than minTriangulated good points; ambiguous: two hypotheses pass percSecondBestGood
    assert max(c["n_good"] for c in ref("few_good")["checks"]) == 40 < R.MIN_TRIANGULATED
    tr = ref("ambiguous")
    assert tr["second_best_good"] >= 0.75 * tr["best_good"] and tr["best_good"] == 120
    # d_ratio: d1 / d2 or d2 / d3 below dRatio, nothing reconstructed
    d1, d2, d3 = ref("d_ratio")["d"]
    assert (d1 / d2 < R.D_RATIO or d2 / d3 < R.D_RATIO) and ref("d_ratio")["n_motion"] == 0
    # outliers: the inlier masks differ between hypotheses, and the winner leaves the 30 planted outliers out
    out = S.reference("outliers")
    masks = {h["inliers"].tobytes() for h in out["hyp"][F] if not h["degenerate"]}
    assert len(masks) > 20 and 80 <= out["trace"]["n_inliers"] <= 95
    # RH on both sides of 0.40, within 0.002 of it
    assert 0.40 < ref("rh_above")["RH"] < 0.402 and 0.398 < ref("rh_below")["RH"] < 0.40
    # RH is NaN when both scores are 0: ReconstructF
    tr = ref("all_repeated")
    assert np.isnan(tr["RH"]) and tr["best"] == [-1, -1] and not tr["model"][0].any() and not tr["model"][1].any() and tr["n_inliers"] == 0
    # the edge of min(50, n - 1): the winning hypothesis pushed 1, 50, 51, 52 cosines
    for n in (1, 50, 51, 52):
        tr = ref("cos%d" % n)
        g = [c["n_cos"] for c in tr["checks"]]
        assert max(g) == n, (n, g)


def test_the_selected_cosine_is_the_min_50_n_minus_1_th_smallest():
    """recomputed in float64 from the winner's points: entry n - 1 (the largest) for n = 50 and entry 50 for n = 51, 52"""
    for n in (50, 51, 52):
        name = "cos%d" % n
        sc, out = S.scene(name), S.reference(name)
        tr = out["trace"]
        k = tr["best_motion"]
        Rm, t = np.array(R.flat(tr["motions"][k][0]), float).reshape(3, 3), np.array(tr["motions"][k][1], float)
        O2 = -Rm.T @ t
        P = out["p3d"][sc.matches12 >= 0].astype(float)
        cos = np.sort([p @ (p - O2) / (np.linalg.norm(p) * np.linalg.norm(p - O2)) for p in P])
        assert len(cos) == n and abs(cos[min(50, n - 1)] - float(tr["checks"][k]["cos"])) < 1e-6
        if n > 51:
            assert cos[51] - cos[50] > 1e-6 or cos[50] - cos[49] > 1e-6   # a neighbouring entry would have been told apart


@pytest.mark.parametrize("name", SUCCESS)
def test_success_returns_the_hypothesis_closest_to_the_true_motion(name):
    """no tolerance: in rotation angle and in the angle between translation directions the answer is at least as close as every other
    motion hypothesis of the trace, and strictly closer in one of the two"""
    sc, out = S.scene(name), S.reference(name)
    tr = out["trace"]
    errs = [S.motion_error(R.flat(m[0]), m[1], sc.true_R, sc.true_t) for m in tr["motions"]]
    k = tr["best_motion"]
    same(out["R21"], R.flat(tr["motions"][k][0]))
    for j, e in enumerate(errs):
        if j != k:
            assert errs[k][0] <= e[0] and errs[k][1] <= e[1] and (errs[k][0] < e[0] or errs[k][1] < e[1]), (j, errs)
    assert errs[k][0] < 0.02 and errs[k][1] < 0.1


def same(a, b):
    assert np.array_equal(bits(np.asarray(a, np.float32)), bits(np.asarray(b, np.float32)))


def test_match_count_and_mask_word_edges():
    for n, words in ((8, 1), (9, 1), (63, 2), (64, 2), (65, 3), (129, 5)):
        out = S.reference("n%d" % n)
        assert out["trace"]["N"] == n
        for m in (H, F):
            for h in out["hyp"][m]:
                assert len(h["inliers"]) == n
                w = R.mask_words(h["inliers"], words)
                assert sum(bin(int(x)).count("1") for x in w) == int(h["inliers"].sum())
        assert any(h["inliers"][n - 1] for h in out["hyp"][F])   # the last match, bit (n - 1) & 31 of the last word, is an inlier somewhere
    out = S.reference("n7")
    assert out["hyp"] == [[], []] and out["trace"]["n_motion"] == 0 and not out["trace"]["T1"].any()


def test_iteration_counts_share_their_prefix():
    """hypothesis h depends on (seed, h) alone: fewer iterations are a prefix; the winner of 63, 64, 65 and 200 iterations is iteration 25"""
    full = S.reference("iter200")
    for it in (1, 63, 64, 65):
        out = S.reference("iter%d" % it)
        for m in (H, F):
            assert len(out["hyp"][m]) == it
            for a, b in zip(out["hyp"][m], full["hyp"][m]):
                same(a["model"], b["model"])
                same([a["score"]], [b["score"]])
        assert out["trace"]["best"][H] == (0 if it == 1 else 25)


def test_ties_go_to_the_lowest_index():
    """N = 8: every iteration draws the same eight matches (in another order), the models fit all eight and the F scores tie exactly"""
    out = S.reference("n8")
    assert all(sorted(s) == list(range(8)) for s in out["trace"]["sets"]) and len({tuple(s) for s in out["trace"]["sets"]}) > 1
    scores = [h["score"] for h in out["hyp"][F]]
    assert len(set(float(s) for s in scores)) == 1 and scores[0] > 0 and out["trace"]["best"][F] == 0
    # and in general: the first index that holds the maximum
    for name in ("cloud", "iter200", "outliers"):
        o = S.reference(name)
        for m in (H, F):
            s = [float(h["score"]) for h in o["hyp"][m]]
            assert o["trace"]["best"][m] == s.index(max(s))


def test_repeated_matches_flag_their_hypotheses_only():
    """7 matches share their positions: an 8-set that holds two of them leaves ComputeF21's 8 x 9 system rank deficient (I8); ComputeH21's
    16 x 9 system keeps rank 8 as long as four different points remain"""
    sc, out = S.scene("repeated"), S.reference("repeated")
    pairs = R.compact(sc.matches12)
    key = [(float(sc.x1[a]), float(sc.y1[a])) for a, _ in pairs]
    twin = [k for k in range(len(pairs)) if key.count(key[k]) > 1]
    assert len(twin) == 7
    flagged = 0
    for h, s in enumerate(out["trace"]["sets"]):
        doubles = len([k for k in s if k in twin]) >= 2
        f = out["hyp"][F][h]
        assert f["degenerate"] == int(doubles) == int(f["deficient"]), h
        flagged += doubles
        if doubles:
            assert f["score"] == 0 and not f["model"].any() and not f["inliers"].any()
        else:
            assert f["score"] > 0 and f["inliers"].sum() >= 8
        hh = out["hyp"][H][h]
        assert hh["degenerate"] == int(hh["deficient"])
        if not doubles:
            assert hh["degenerate"] == 0 and hh["model"].any()
    assert 10 < flagged < 35
    # the hypotheses without twins are what they are without the planted matches' influence: rebuilt one by one from their own 8 pairs
    assert out["trace"]["best"][F] >= 0 and not out["hyp"][F][out["trace"]["best"][F]]["degenerate"]
    every = S.reference("all_repeated")
    assert all(h["degenerate"] == 1 for m in (H, F) for h in every["hyp"][m])


def test_draws_without_the_list_are_the_literal_ones():
    for N in (8, 9, 10, 15, 16, 17, 100):
        for seed in (0, 7, 1 << 40):
            for h in range(60):
                lit = R.draw_set(seed, h, N)
                assert lit == R.draw_set_closed(seed, h, N) and len(set(lit)) == 8 and all(0 <= k < N for k in lit)
    assert R.draw_set(1, 0, 50) != R.draw_set(2, 0, 50) and R.draw_set(1, 0, 50) != R.draw_set(1, 1, 50)


JACOBI_SETS = (("plane", H), ("cloud", H), ("outliers", H), ("iter200", H), ("outliers", F), ("cloud", F))


def test_jacobi_null_vector_against_numpy_svd():
    """Over the 384 seeded 8-sets of JACOBI_SETS, those with sigma8 / sigma1 >= 1e-3 (the gap condition excludes 11 of the 384, 2.9 %: F
    systems of a near-planar draw).  The sine of the angle between the restated null vector (float64, before the float rounding) and
    numpy's must be <= 1e-6.  Derivation: the restatement goes through A^T A, so the error is of order eps64 * |A^T A| / gap, with
    |A^T A| ~ 1e2 for normalised points and gap >= (1e-3 sigma1)^2 ~ 1e-6 * 1e2: 1e-16 * 1e2 / 1e-4 = 1e-10 .. 1e-8 at the edge of the gap
    condition; 1e-6 leaves a 100x margin.  Measured: 1.9e-11 at worst."""
    total = excluded = 0
    worst = 0.0
    for name, m in JACOBI_SETS:
        for h in S.reference(name)["hyp"][m]:
            A = np.array(h["A"], np.float64)
            total += 1
            _, sv, vt = np.linalg.svd(A, full_matrices=True)
            if sv[7] / sv[0] < 1e-3:
                excluded += 1
                continue
            v = np.array(h["null"], np.float64)
            v = v / np.linalg.norm(v)
            sine = np.linalg.norm(v - (v @ vt[8]) * vt[8])
            worst = max(worst, sine)
            assert sine <= 1e-6, (name, m, sine)
    print("jacobi: %d sets, %d excluded, worst sine %.3g" % (total, excluded, worst))
    assert total == 384 and excluded <= 0.10 * total


def test_svd3_is_a_singular_value_decomposition():
    rng = np.random.default_rng(5)
    for k in range(40):
        A = rng.normal(0, 1, (3, 3)).astype(np.float32)
        if k % 4 == 0:
            A[2] = A[0] + A[1]   # rank 2, as an essential matrix
        U, w, V = (np.array(x, np.float64) for x in R.svd3(R.mat(A)))
        assert np.allclose(U @ np.diag(w) @ V.T, A, atol=2e-6) and w[0] >= w[1] >= w[2] >= 0
        assert np.allclose(U.T @ U, np.eye(3), atol=1e-5) and np.allclose(V.T @ V, np.eye(3), atol=1e-5) and np.linalg.det(U) > 0.99
        assert np.allclose(w, np.linalg.svd(A.astype(np.float64), compute_uv=False), atol=2e-6)
        Un, wn, Vn = R.svd3(R.neg(R.mat(A)))   # I2: -A gives (-u0, -u1, u2), (v0, v1, -v2) exactly
        same(np.array(Un)[:, :2], -np.array(U, np.float32)[:, :2])
        same(np.array(Un)[:, 2], np.array(U, np.float32)[:, 2])
        same(np.array(Vn)[:, 2], -np.array(V, np.float32)[:, 2])
        same(wn, w)


@pytest.mark.parametrize("name", ["plane", "cloud", "ambiguous", "low_parallax", "outliers", "rh_above", "n65"])
def test_the_sign_of_h_and_f_reaches_no_output(name):
    """H and F are homogeneous: the reconstruction from -H21 / -F21 answers bit for bit what it answers from H21 / F21 (I2, I3), down to
    every motion hypothesis of the trace; and -H21 / -F21 score every match alike"""
    a, b = S.reference(name), R.initialize(S.scene(name), negate_models=True)
    for k in ("ok", "route"):
        assert a[k] == b[k]
    for k in ("R21", "t21", "p3d", "triangulated"):
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    ta, tb = a["trace"], b["trace"]
    assert (ta["reason"], ta["best_motion"], ta["n_motion"]) == (tb["reason"], tb["best_motion"], tb["n_motion"])
    for (Ra, t_a), (Rb, t_b), ca, cb in zip(ta["motions"], tb["motions"], ta["checks"], tb["checks"]):
        same(R.flat(Ra), R.flat(Rb))
        same(t_a, t_b)
        assert ca["n_good"] == cb["n_good"]
        same([ca["cos"]], [cb["cos"]])
    sc = S.scene(name)
    pairs = R.compact(sc.matches12)
    i1, i2 = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    uv = (sc.x1[i1], sc.y1[i1], sc.x2[i2], sc.y2[i2])
    Hm, Fm = R.as3(ta["model"][H]), R.as3(ta["model"][F])
    s1, in1 = R.check_homography(Hm, R.inv3(Hm), *uv, sc.sigma)
    s2, in2 = R.check_homography(R.neg(Hm), R.inv3(R.neg(Hm)), *uv, sc.sigma)
    same([s1], [s2])
    assert np.array_equal(in1, in2)
    s1, in1 = R.check_fundamental(Fm, *uv, sc.sigma)
    s2, in2 = R.check_fundamental(R.neg(Fm), *uv, sc.sigma)
    same([s1], [s2])
    assert np.array_equal(in1, in2)


def test_fixed_shape_sums():
    """I5: 64 (or 256) strided partial sums, then the halving tree - not the running sum"""
    e = (np.random.default_rng(3).random(300) * 5).astype(np.float32)
    for width in (64, 256):
        part = [np.float32(0)] * width
        for k, v in enumerate(e):
            part[k % width] = part[k % width] + v
        s = width // 2
        while s:
            part = [part[t] + part[t + s] for t in range(s)]
            s //= 2
        same([R.tree_sum(e, width)], [part[0]])
    run = np.float32(0)
    for v in e:
        run = run + v
    assert abs(float(R.tree_sum(e, 64)) - float(run)) < 1e-2
    assert R.tree_sum(np.zeros(0, np.float32), 64) == 0
