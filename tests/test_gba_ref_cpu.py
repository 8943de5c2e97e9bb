"""CPU: the restatement of the block-sparse global bundle adjustment (tests/_gba_ref.py, L7') against the dense restatement
(tests/_lba_ref.py, L7) on every small scene of tests/_gba_scenes.py: solve_block_sparse equals solve_dense BYTE FOR BYTE at every solve
of the run, and the whole answer of _gba_ref.bundle_adjust equals _lba_ref.bundle_adjust likewise.  Each scene is shown to reach what it
is named for, and every scene that is not named for a failure accepts at least one trial and ends its first round with a finite chi2
below the one it started with - a scene where every trial fails would hide the solve.  correct_se3 in float32 against a float64
evaluation."""
import numpy as np
import pytest

import _gba_ref as G
import _gba_scenes as GS
import _lba_ref as L

SCENES = dict(GS.small())
_runs = {}


def run(name):
    """one sparse and one dense run per scene, shared by the tests"""
    if name not in _runs:
        sc = SCENES[name]
        solves, log = [], []
        sparse = sc.solve_sparse(log=log, solves=solves)
        dense_log = []
        dense = sc.solve(log=dense_log)
        _runs[name] = (sc, G.plan_of(sc.problem()), sparse, dense, solves, log, dense_log)
    return _runs[name]


def same_bytes(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.asarray(a).tobytes() == np.asarray(b).tobytes())


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_solve_and_the_whole_answer_equal_the_dense_restatement(name):
    sc, pl, sparse, dense, solves, log, dense_log = run(name)
    assert len(solves) >= 1
    for q, (xs, xd) in enumerate(solves):
        assert same_bytes(xs, xd), (name, q)
    for f in ("iterations", "trials", "chi2", "lam", "R", "t", "xyz", "state"):
        assert same_bytes(getattr(sparse, f), getattr(dense, f)), (name, f)
    assert (sparse.n_edges, sparse.n_removed_first, sparse.n_erase, sparse.stopped) == (dense.n_edges, dense.n_removed_first, dense.n_erase, dense.stopped)


@pytest.mark.parametrize("name", sorted(n for n in SCENES if n not in GS.FAILURE_SCENES))
def test_the_first_round_accepts_a_trial_and_lowers_the_chi2(name):
    sc, pl, sparse, dense, solves, log, dense_log = run(name)
    first = [r for r in log[0] if "trial" in r]
    assert any(r["accepted"] for r in first), name
    assert np.isfinite(sparse.chi2[0]) and sparse.chi2[0] < first[0]["before"], (name, sparse.chi2[0], first[0]["before"])


def test_band_is_sparse_without_fill():
    sc, pl = run("band")[:2]
    all_blocks = pl.nf * (pl.nf + 1) // 2
    assert pl.structural == {(i, j) for i in range(9) for j in range(i + 1, 9) if j - i < 3}
    assert pl.ns == 9 + len(pl.structural) < all_blocks and pl.nb == pl.ns and all(pl.blk_kind)


def test_arrow_fill_has_more_blocks_of_l_than_structural_blocks():
    sc, pl = run("arrow_fill")[:2]
    assert (0, 11) in pl.structural and pl.nb > pl.ns
    assert [(pl.blk_row[b], pl.blk_col[b]) for b in range(pl.nb) if not pl.blk_kind[b]] == [(11, j) for j in range(1, 10)]


def test_two_components_share_no_block():
    sc, pl = run("two_components")[:2]
    assert all((pl.blk_row[b] < 4) == (pl.blk_col[b] < 4) for b in range(pl.nb)) and pl.nb == 2 * 10


def test_isolated_keyframe_holds_lambda_alone_and_does_not_move():
    sc, pl, sparse = run("isolated_keyframe")[:3]
    pr = sc.problem()
    assert not pr.p_on[pr.e_pt[pr.e_kf == 3]].any() and (0, 3) in pl.structural          # its only points are dropped; the pattern keeps the block
    sy = L.linearise(pr, pr.R0, pr.t0, pr.X0, pr.p_on[pr.e_pt], True)
    S, bS = L.reduced_system(pr, sy, pr.p_on[pr.e_pt], np.float64(0.25))[:2]
    assert np.array_equal(S[18:24, 18:24], 0.25 * np.eye(6)) and not S[:18, 18:24].any() and not bS[18:24].any()
    assert sparse.R[3].tobytes() == pr.R0[3].reshape(9).tobytes() and sparse.t[3].tobytes() == pr.t0[3].tobytes()


def test_first_is_hub_makes_l_dense():
    sc, pl = run("first_is_hub")[:2]
    assert pl.rows[0] == list(range(1, 10)) and pl.nb == 10 * 11 // 2
    assert pl.structural == {(0, k) for k in range(1, 10)} and pl.ns == 10 + 9


def test_pattern_empties_runs_its_second_round_with_an_exact_zero_block():
    sc, pl, sparse = run("pattern_empties")[:3]
    pr = sc.problem()
    assert (1, 4) in pl.structural
    behind = [e for e in range(pr.ne) if pr.e_kf[e] in (1, 4) and sum(1 for q in pr.pt_edges[pr.e_pt[e]] if pr.e_kf[q] in (1, 4)) == 2]
    assert len(behind) == 2 and pr.e_pt[behind[0]] == 7
    with np.errstate(all="ignore"):
        removed = pr.p_on[pr.e_pt] & (~np.isfinite(sparse.first_chi2) | (sparse.first_chi2 > pr.th) | sparse.first_depth_bad)
    # point 7 alone stands behind block (1, 4): a pair contributes while both its edges are active, and the first check removed one of them
    assert removed.sum() == sparse.n_removed_first and removed[behind].any()
    assert sparse.iterations[1] >= 1 and sparse.trials[1] >= 1
    on = pr.p_on[pr.e_pt] & ~removed
    sy = L.linearise(pr, pr.R0, pr.t0, pr.X0, on, False)
    S = L.reduced_system(pr, sy, on, np.float64(1.0))[0]
    assert not S[6:12, 24:30].any() and S[0:6, 6:12].any()


def test_bad_pivot_is_reached_on_a_sparse_pattern():
    sc, pl, sparse, dense, solves, log = run("bad_pivot")[:6]
    assert pl.nb == pl.ns == 4 + 3 < 10
    assert any(r.get("why") == "pivot" for r in log[0]) and any(xs is None for xs, _ in solves)


def test_stop_in_first_and_the_one_column_plan():
    sc, pl, sparse = run("stop_in_first")[:3]
    assert sparse.stopped == 2 and sparse.trials[0] == 2 and sparse.trials[1] == 0
    pl1 = run("startup_two_keyframes")[1]
    assert (pl1.nf, pl1.nb, pl1.col_ptr) == (1, 1, [0, 1])
    assert run("no_fixed_keyframe")[0].nk == run("no_fixed_keyframe")[0].nf == 6
    pr = run("mixed_mono_stereo")[0].problem()
    assert pr.stereo.any() and not pr.stereo.all()


def test_correct_se3_against_a_float64_evaluation():
    rng = np.random.default_rng(5)
    m, n = 7, 300
    T = np.zeros((2, m, 12), np.float32)
    for q in range(m):
        for s in range(2):
            a, ax = rng.uniform(-1, 1), rng.normal(0, 1, 3)
            ax /= np.linalg.norm(ax)
            K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
            T[s, q, :9] = (np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K).reshape(9)
            T[s, q, 9:] = rng.uniform(-3, 3, 3)
    pos = rng.uniform(-8, 8, (n, 3)).astype(np.float32)
    pair = rng.integers(-1, m, n)
    ok = rng.uniform(0, 1, n) > 0.1
    got, st = G.correct_se3(pos, ok, pair, T[0], T[1])
    assert got.dtype == np.float32
    moved = ok & (pair >= 0)
    assert np.array_equal(st, np.where(~ok, G.BAD_OR_UNSET, np.where(pair < 0, G.NO_PAIR, G.MOVED)))
    assert got[~moved].tobytes() == pos[~moved].tobytes()
    A, B = T[0].astype(np.float64)[pair[moved]], T[1].astype(np.float64)[pair[moved]]
    X = pos[moved].astype(np.float64)
    Xc = np.einsum("nrc,nc->nr", A[:, :9].reshape(-1, 3, 3), X) + A[:, 9:]
    want = np.einsum("nrc,nc->nr", B[:, :9].reshape(-1, 3, 3), Xc) + B[:, 9:]
    # float rounding: each of the two steps has 3 products and 3 sums of magnitudes up to |R| |X| + |t| <= 3 * 14 + 3 = 45 (second
    # step: up to 3 * 45 + 3); each operator adds at most half an ulp of its result: 6 * 2^-24 * 140 per step, the first step's error
    # passes through a rotation (norm 1, at most sqrt(3) per row)
    bound = 6 * 2.0 ** -24 * 140 * (1 + np.sqrt(3))
    assert np.abs(got[moved].astype(np.float64) - want).max() <= bound
    # a pure translation by representable numbers is exact
    eye = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], np.float32)
    Tb, Ta = np.concatenate([eye, [0.5, -2.0, 4.0]]).astype(np.float32), np.concatenate([eye, [1.25, 8.0, -0.75]]).astype(np.float32)
    P = np.array([[1.5, 2.25, -3.0], [64.0, 0.125, 7.0]], np.float32)
    got, st = G.correct_se3(P, [True, True], [0, 0], Tb[None], Ta[None])
    assert got.tobytes() == (P + np.float32([1.75, 6.0, 3.25])).tobytes()
