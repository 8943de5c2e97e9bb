"""CPU: the restatement tests/_essgraph_ref.py of Optimizer::OptimizeEssentialGraph on the constructed graphs of tests/_essgraph_scenes.py.
Each scene is named for the rule it reaches, and the restatement's branch counter or trace proves that it reaches it.  The restated log
and acos are held to math.log and math.acos, log(exp(u)) to u, at the bounds measured into the restatement's header.  The block-sparse
solve is held to a dense twin (numpy.linalg on the assembled H), one solve and the whole optimisation.

The bound of the twin: TWIN_MEASURED is the largest relative difference between the two, measured on this file's scenes: one solve
over every scene with a system, the whole optimisation over every such scene BUT floating, drifted_stall and rejected, whose trajectories
turn on the sign of a rounding error (a pivot, a rejected trial) and are not comparable between two solvers; TWIN_BOUND = 8 * TWIN_MEASURED is asserted (the two eliminate in different orders but are both backward stable; the 8 absorbs other
seeds).  The drifted-loop scene must end with every pose within TWIN_BOUND of the truth its measurements are consistent with."""
import math
from fractions import Fraction

import numpy as np
import pytest

import _essgraph_ref as G
import _essgraph_scenes as SC
import _sim3opt_ref as SO

TWIN_MEASURED = 2.92e-8   # one solve 1.93e-10 (all scenes), the whole optimisation 2.92e-08 (all but floating, drifted_stall, rejected: see above)
TWIN_BOUND = 8 * TWIN_MEASURED


def trials(log):
    return [l for l in log if "trial" in l]


def ulp_error(got, want):
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want) + (want == 0))))


def test_log_is_held_to_math_log():
    assert all(G.LOG_C[n] == float(Fraction(1, 2 * n + 1)) for n in range(12))
    rng = np.random.default_rng(7)
    x = np.concatenate([np.exp(rng.uniform(-64, 64, 200000)), 1 + rng.uniform(-1e-3, 1e-3, 100000), rng.uniform(0.5, 2, 100000), [1.0, 0.5, 2.0]])
    got, want = G.log_f64(x), np.array([math.log(v) for v in x])
    worst = ulp_error(got, want)
    print("log: %.1f ulp" % worst)
    assert worst <= G.LOG_ULP and got[-3] == 0.0
    assert np.all(np.isnan(G.log_f64(np.array([0.0, -1.0, np.inf, np.nan]))))


def test_acos_is_held_to_math_acos():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.uniform(-1, 1, 300000), 1 - np.exp(rng.uniform(-30, 0, 50000)), -1 + np.exp(rng.uniform(-30, 0, 50000)), [1.0, -1.0, 0.0, 0.5, -0.5]])
    got, want = G.acos_f64(x), np.array([math.acos(v) for v in x])
    worst = ulp_error(got, want)
    print("acos: %.1f ulp" % worst)
    assert worst <= G.ACOS_ULP and got[-5] == 0.0
    assert np.all(np.isnan(G.acos_f64(np.array([1.0000001, -1.5, np.nan]))))


def test_log_of_exp_returns_the_update_in_all_four_branches():
    rng = np.random.default_rng(11)
    worst = [0.0] * 4
    for k in range(4000):
        br = k % 4
        th = rng.uniform(1e-2, 3.0) if br & 1 else rng.uniform(0, 4e-6)
        sg = rng.choice([-1.0, 1.0]) * rng.uniform(0.5 if br == 2 else 2e-5, 2) if br & 2 else rng.uniform(-9e-6, 9e-6)
        w = rng.normal(size=3)
        u = np.concatenate([w / np.linalg.norm(w) * th, rng.uniform(-5, 5, 3), [sg]])
        dR, dt, ds = SO.sim3_exp(u)
        e, b = G.sim3_log((np.array(dR, np.float64)[None], np.array(dt, np.float64)[None], np.array([ds])))
        assert b[0] == br
        worst[br] = max(worst[br], float(np.abs(e[0] - u).max() / np.abs(u).max()))
    print("log(exp(u)) per branch:", worst)
    for br in range(4):
        assert worst[br] <= G.LOGEXP_REL[br], (br, worst)


def test_four_branches_of_log_are_reached():
    sc, pr, res, log = SC.solved("log_branches")
    e, branch = G.errors_at(pr, pr.S0)
    assert list(branch) == [0, 1, 2, 3] and np.all(np.isfinite(e))
    assert res.status == G.OK and res.chi2_last < 1e-20 * res.chi2_first


def test_consistent_graph_has_zero_chi2_and_a_zero_step():
    sc, pr, res, log = SC.solved("consistent")
    t = trials(log)
    assert res.chi2_first == 0.0 and res.chi2_last == 0.0 and res.iterations == 1 and len(t) == 1
    assert t[0]["rho"] == 0.0 and not t[0]["failed"] and not t[0]["accepted"]      # G-Q1: rho > 0 is the rule; the estimate stands either way
    assert [l["terminate"] for l in log if "terminate" in l] == ["rho0"]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res.S, pr.S0))


def test_rejected_trial_restores_the_estimate_and_grows_lambda():
    sc, pr, res, log = SC.solved("rejected")
    t = trials(log)
    rej = [i for i, l in enumerate(t) if not l["accepted"] and not l["failed"] and i + 1 < len(t) and t[i + 1]["iteration"] == l["iteration"]]
    assert rej, "no trial was rejected on its chi2"
    i = rej[0]
    assert t[i]["rho"] < 0 and t[i + 1]["lam"] > t[i]["lam"] and t[i + 1]["before"].tobytes() == t[i]["before"].tobytes()
    acc = [l for l in t if l["accepted"]]
    assert len(acc) >= 2 and acc[-1]["after"] < acc[0]["before"]


def test_floating_component_fails_on_its_pivot_and_lambda_grows():
    sc, pr, res, log = SC.solved("floating")
    t = trials(log)
    piv = [i for i, l in enumerate(t) if l["why"] == "pivot"]
    assert piv and all(t[i]["failed"] and not t[i]["accepted"] for i in piv)
    i = piv[0]
    assert t[i + 1]["lam"] > t[i]["lam"]
    assert any(l["accepted"] for l in t[i + 1:]), "lambda never grew enough"
    assert res.status == G.OK


def test_isolated_vertex_stays_in_the_system_and_does_not_move():
    sc, pr, res, log = SC.solved("isolated")
    assert len(pr.v_edges[pr.sys_of[3]]) == 0 and pr.cols[pr.sys_of[3]] == []
    sy = G.build_system(pr, pr.S0)
    assert not sy.Hd[pr.sys_of[3]].any() and not sy.b[pr.sys_of[3]].any()
    x = G.factor_solve(pr, sy, np.float64(1e-16))
    assert x is not None and not x[pr.sys_of[3]].any()
    assert all(a[3].tobytes() == b[3].tobytes() for a, b in zip(res.S, pr.S0)) and res.iterations > 1


def test_double_edges_are_summed_not_deduplicated():
    sc, pr, res, log = SC.solved("double_edges")
    assert len(pr.pairs[(pr.sys_of[2], pr.sys_of[1])]) == 3 and {f for _, f in pr.pairs[(pr.sys_of[2], pr.sys_of[1])]} == {True, False}
    once = dict(sc, v0=np.delete(sc["v0"], [3, 4]), v1=np.delete(sc["v1"], [3, 4]), meas=tuple(np.delete(a, [3, 4], 0) for a in sc["meas"]))
    a, b = G.build_system(pr, pr.S0), G.build_system(SC.problem(once), pr.S0)
    key = (pr.sys_of[2], pr.sys_of[1])
    assert np.abs(a.off[key]).max() > 2 * np.abs(b.off[key]).max() * 0.9 and a.chi2 > b.chi2


def test_edge_onto_the_fixed_vertex_contributes_to_one_block_only():
    sc, pr, res, log = SC.solved("onto_fixed")
    assert pr.pairs == {} and all(c == [] for c in pr.cols) and pr.l_blocks == pr.nf
    assert res.chi2_last < 1e-20 * res.chi2_first


@pytest.mark.parametrize("name", ["fixed_first", "fixed_middle", "fixed_last"])
def test_fixed_vertex_first_middle_last(name):
    sc, pr, res, log = SC.solved(name)
    f = sc["fixed"]
    assert all(a[f].tobytes() == b[f].tobytes() for a, b in zip(res.S, pr.S0))
    assert pr.sys_of[f] == -1 and sorted(pr.sys_of[pr.sys_of >= 0]) == list(range(pr.nf))
    assert res.chi2_last < 1e-15 * res.chi2_first


def test_fix_scale_never_changes_the_bits_of_a_scale():
    sc, pr, res, log = SC.solved("fix_scale_on")
    assert res.S[2].tobytes() == pr.S0[2].tobytes() and res.iterations > 1
    sy = G.build_system(pr, pr.S0)
    assert not sy.Hd[:, 6, :].any() and not sy.Hd[:, :, 6].any() and not sy.b[:, 6].any()          # G7
    off = SC.solved("drifted_stall")[2]
    assert off.S[2].tobytes() != SC.solved("drifted_stall")[1].S0[2].tobytes()


def test_error_not_finite_at_the_start_evaluates_nothing():
    sc, pr, res, log = SC.solved("not_finite")
    e, _ = G.errors_at(pr, pr.S0)
    assert not np.all(np.isfinite(e))
    assert res.status == G.NOT_FINITE and res.iterations == 0 and res.trials == 0 and log == []
    assert all(a.tobytes() == b.tobytes() for a, b in zip(res.S, pr.S0))


def test_stall_near_the_threshold_of_sigma_is_upstreams_own():
    """the band-1 loop ends on qmax at a chi2 of 1e-8: with |sigma| of the errors just above eps, upstream's A and B near the identity are
    differences of nearly equal numbers, and the numeric Jacobian divides their noise by 2e-9"""
    sc, pr, res, log = SC.solved("drifted_stall")
    assert [l["terminate"] for l in log if "terminate" in l] == ["qmax"] and 0 < res.chi2_last < 1e-6 * res.chi2_first


def relative(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_block_sparse_solve_against_the_dense_twin():
    worst_solve, worst_run = 0.0, 0.0
    for name in sorted(SC.SCENES):
        sc, pr, res, log = SC.solved(name)
        if res.status != G.OK or pr.nf == 0:
            continue
        sy = G.build_system(pr, pr.S0)
        for lam in (1e-16, 1e-6, 1.0):
            x, xd = G.factor_solve(pr, sy, np.float64(lam)), G.dense_solve(pr, sy, np.float64(lam))
            if x is None or xd is None:
                assert name == "floating"
                continue
            if np.abs(xd).max() > 0:
                worst_solve = max(worst_solve, relative(x, xd))
        if name in ("floating", "drifted_stall", "rejected"):
            continue              # trajectories that turn on the sign of a rounding error (a pivot, a rejected trial) are not comparable
        twin = G.optimize(pr, sc["iterations"], solver=G.dense_solve)
        for a, b in zip(res.S, twin.S):
            worst_run = max(worst_run, relative(a, b))
    print("twin: one solve %.3g, the whole optimisation %.3g" % (worst_solve, worst_run))
    assert max(worst_solve, worst_run) <= TWIN_BOUND


def test_drifted_loop_ends_at_the_truth_its_measurements_are_consistent_with():
    sc, pr, res, log = SC.solved("drifted_loop")
    assert sc["S_init"][2][-1] == 1.1 and sc["S_init"][2][1] == 1.0
    worst = max(relative(a, b) for a, b in zip(res.S, sc["truth"]))
    print("drifted loop: %.3g from the truth" % worst)
    assert worst <= TWIN_BOUND


# ---- the edge list (:835-971) ----
def graph_inputs():
    ids = [0, 2, 3, 5, 7, 8]
    I = lambda k: (SC.rot([0.0, 0.0, 0.1 * k]), np.array([0.5 * k, 0.0, 1.0]), 1.0)
    Scw = {k: I(k) for k in ids}
    Scw[8] = (SC.rot([0.0, 0.0, 0.75]), np.array([3.5, 0.25, 1.0]), 1.1)            # the corrected current keyframe
    non_corrected = {8: I(8), 7: I(7)}
    Scw[7] = (SC.rot([0.0, 0.0, 0.68]), np.array([3.25, 0.125, 1.0]), 1.05)
    parent = {0: None, 2: 0, 3: 2, 5: 3, 7: 5, 8: 7}
    loop_edges = {7: {2, 8}, 2: {7}, 8: {7}}
    covisibles = {0: [2, 3], 2: [0, 3], 3: [5, 2, 0], 5: [7, 3, 2, 9], 7: [8, 5, 3, 2, 0], 8: [7, 5, 0, 2]}
    loop_connections = {8: [(2, 40), (0, 30), (3, 150)], 7: [(0, 99), (3, 100)]}
    return ids, parent, loop_edges, covisibles, loop_connections, Scw, non_corrected


def pairs(edges):
    return [(e[0], e[1]) for e in edges]


def test_edge_list_order_and_measurements():
    ids, parent, le, cov, lc, Scw, nc = graph_inputs()
    edges = G.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, loop_id=0, cur_id=8)
    assert pairs(edges) == [(7, 3), (8, 0), (8, 3),                       # the loop connections in ascending id: weight >= 100, or cur -> loop
                            (2, 0), (3, 2), (3, 0), (5, 3), (5, 2), (7, 5), (7, 2), (7, 0), (8, 7), (8, 7), (8, 5), (8, 2)]     # (8, 7): parent AND loop edge
    m = {(e[0], e[1]): e[2] for e in edges}
    for (i, j), want in (((8, 0), G.relative(Scw[0], Scw[8])), ((8, 7), G.relative(nc[7], nc[8])), ((5, 3), G.relative(Scw[3], Scw[5])),
                         ((7, 2), G.relative(Scw[2], nc[7]))):
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(m[(i, j)], want)), (i, j)


@pytest.mark.parametrize("rule,extra", [("min_feat", []), ("loop_lower", [(2, 7), (7, 8)]), ("not_parent", [(2, 0), (3, 2), (5, 3), (7, 5)]),
                                        ("not_child", []), ("not_loop_edge", [(7, 2)]), ("cov_lower", None), ("inserted", [(7, 3), (8, 0)])])
def test_edge_list_rules_each_against_a_twin_that_flips_it(rule, extra):
    ids, parent, le, cov, lc, Scw, nc = graph_inputs()
    base = pairs(G.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, 0, 8))
    twin = pairs(G.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, 0, 8, rules={rule}))
    assert twin != base or rule == "not_child", rule
    if rule == "not_child":        # a child has a higher id than its parent here, so the rule is shadowed by "lower ids only": flip both
        both = pairs(G.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, 0, 8, rules={"not_child", "cov_lower"}))
        only = pairs(G.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, 0, 8, rules={"cov_lower"}))
        assert (0, 2) in both and (0, 2) not in only
        return
    if rule == "min_feat":         # the weak connections (7, 0) and (8, 2) enter as loop connections and, through sInsertedEdges, leave as covisibility edges
        assert twin[:5] == [(7, 0), (7, 3), (8, 0), (8, 2), (8, 3)] and len(twin) == len(base)
    if extra is not None:
        rest = list(twin)
        for e in base:
            rest.remove(e)
        assert sorted(rest) == sorted(extra), (rule, rest)
    else:
        assert (0, 3) in twin and (0, 3) not in base and 9 not in [b for _, b in twin]       # a bad keyframe (not listed) never enters


def test_package_builds_the_same_list(afv):
    ids, parent, le, cov, lc, Scw, nc = graph_inputs()
    a = G.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, 0, 8)
    b = afv.essential_graph_edges(ids, parent, le, cov, lc, Scw, nc, 0, 8)
    assert pairs(a) == pairs(b)
    for x, y in zip(a, b):
        assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[2], y[2]))
