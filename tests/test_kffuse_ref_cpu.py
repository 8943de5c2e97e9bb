"""CPU: the restatement of Fuse into keyframes of the table (tests/_kffuse_ref.py) on the scenes of tests/_kffuse_scenes.py - every scene
reaches the rule it is named after, a turned-around rule changes its answer, a batch of targets equals the targets one by one, the
one-target-per-call loop with toy-map surgery reproduces the sequential SearchInNeighbors / SearchAndFuse, and a scene in which the snapshot
batch does NOT (a point replaced at target 0 that the batch still fuses into target 1)."""
import copy

import numpy as np
import pytest

import _kffuse_ref as K
import _kffuse_scenes as KS
import _points_ref as R

CASES = KS.all_constructed()


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_scene_reaches_its_rule(c):
    res = c.run()
    assert c.reached(res), c.name
    if c.flip or c.proj_flip:
        assert KS.answer(c.run(flip=c.flip, proj_flip=c.proj_flip)) != KS.answer(res), (c.name, c.flip, c.proj_flip)


def test_the_scenes_cover_every_status_and_named_rule():
    seen = set()
    for c in CASES:
        for r in c.run():
            seen |= set(int(v) for v in r[2])
    assert seen == set(range(7))
    names = " ".join(c.name for c in CASES)
    for need in ("every_status", "member_elsewhere", "two_win_one_free", "occupant_bad", "occupant_never_set", "tie_across_cells", "tie_inside_cell",
                 "fuse_bound_max", "fuse_bound_min", "z_minus_zero_fuse", "z_plus_zero_fuse", "band_lo_fuse", "band_hi_fuse", "fuse_dot",
                 "size_band_lo", "size_band_hi", "gates_599_and_78", "stereo_fuse_inf_gate", "scw_scale_2"):
        assert need in names, need


def test_decomposition_keeps_the_translation():
    S = np.eye(4, dtype=np.float32)
    S[:3, :3] = KS.S.rotation(0.1, -0.2, 0.05) * np.float32(1.7)
    S[:3, 3] = (0.3, -0.4, 0.9)
    Rcw, tcw, Ow = K.decompose_scw(S)
    assert np.array_equal(tcw, S[:3, 3])
    assert np.allclose(Rcw @ Rcw.T, np.eye(3), atol=1e-6)
    assert np.array_equal(Ow, R.twc(Rcw, tcw))


@pytest.mark.parametrize("seed", range(2))
def test_a_batch_equals_its_targets_one_by_one(seed):
    m = KS.random_map(seed, 80, 60, 4, per_target=bool(seed))
    best, occ, st, nf = KS.expected(m)
    for s in sorted(m.kfs):
        b, o, t, n, _ = K.fuse_target(m.P, m.kfs[s], m.grid, m.lists[s], th_low=m.th_low)
        assert np.array_equal(b, best[s]) and np.array_equal(o, occ[s]) and np.array_equal(t, st[s]) and n == nf[s]
    assert sum(int((t >= K.FREE).sum()) for t in st) > 0 and any((t == K.IN_KEYFRAME).any() for t in st)


def loop_with_surgery(P, kfs, grid, cur, targets, **kw):
    """what DescriptorTable.SearchInNeighborsFuse does with ToyMap.apply as its callback: one target per call, surgery in between"""
    M = K.ToyMap(P, kfs)
    first = [int(v) for v in kfs[cur].plane]
    nf = []
    for s in targets:
        b, o, st, n, _ = K.fuse_target(P, kfs[s], grid, first, **kw)
        M.apply(s, first, b, st)
        nf.append(n)
    cand = K.fuse_candidates(M, targets)
    b, o, st, n, _ = K.fuse_target(P, kfs[cur], grid, cand, **kw)
    M.apply(cur, cand, b, st)
    return M, nf, n


@pytest.mark.parametrize("seed", range(3))
def test_one_target_per_call_reproduces_search_in_neighbors(seed):
    grid = K.Grid()
    P1, k1 = KS.small_map(seed)
    P2, k2 = copy.deepcopy((P1, k1))
    Ma = K.ToyMap(P1, k1)
    nf_a, n_a = K.search_in_neighbors(Ma, grid, 0, [1, 2], th_low=KS.TH)
    Mb, nf_b, n_b = loop_with_surgery(P2, k2, grid, 0, [1, 2], th_low=KS.TH)
    assert nf_a == nf_b and n_a == n_b and sum(nf_a) > 0
    assert Ma.lists() == Mb.lists()
    assert all(np.array_equal(k1[s].plane, k2[s].plane) for s in k1) and np.array_equal(P1.flags, P2.flags)
    # the duplicates are gone: one of each pair survives with the observations of both
    assert sum(Ma.is_bad(p) for p in range(17)) == 5


def test_one_target_per_call_reproduces_search_and_fuse():
    grid = K.Grid()
    P1, k1 = KS.small_map(1)
    P2, k2 = copy.deepcopy((P1, k1))
    Scw = []
    for s in (1, 2):
        S = np.eye(4, dtype=np.float32)
        S[:3, 3] = k1[s].cam.tcw
        Scw.append(S)
    loop_ids = list(range(12))
    Ma = K.ToyMap(P1, k1)
    nf_a = K.search_and_fuse(Ma, grid, [1, 2], Scw, loop_ids, th_low=KS.TH)
    Mb = K.ToyMap(P2, k2)
    nf_b = []
    for s, S in zip((1, 2), Scw):
        b, o, st, n, _ = K.fuse_target(P2, k2[s], grid, loop_ids, 4.0, KS.TH, False, K.decompose_scw(S))
        Mb.apply(s, loop_ids, b, st, sim3=True)
        nf_b.append(n)
    assert nf_a == nf_b and sum(nf_a) > 0 and Ma.lists() == Mb.lists()
    assert any(Ma.is_bad(p) for p in range(12, 17))   # duplicates held by keyframe 1 were replaced by the loop points


def test_the_snapshot_batch_differs_where_a_point_is_replaced_mid_loop():
    """point 0 (one observation) meets its duplicate 12 (two observations) at target 1: 0->Replace(12), 0 is bad from then on and the
    loop does not fuse it into target 2.  The batch answers target 2 against the store as it stood: it still fuses point 0 there."""
    grid = K.Grid()
    P = KS.S.store([{"pos": (0, 0, 4)}, {"pos": (1, 1, 4)}] + [{"pos": (3, 3, 4)}] * 10 + [{"pos": (0, 0, 4)}], cap=64)
    P.descriptors[12] = KS.near(P.descriptors[0], 2)
    row = KS.near(P.descriptors[0], 3)
    mk = lambda plane: KS.kf_of([(48.2, 32.1, 1.0, row), (80.0, 10.0, 1.0, P.descriptors[1])], plane=plane)
    kfs = {0: mk([0, -1]), 1: mk([12, -1]), 2: mk([-1, -1]), 3: mk([12, -1])}
    first = [0, -1]
    # the loop
    Pl, kl = copy.deepcopy((P, kfs))
    M = K.ToyMap(Pl, kl)
    nf = [K.fuse_sequential(M, grid, s, first, th_low=KS.TH) for s in (1, 2)]
    assert nf == [1, 0] and M.is_bad(0) and kl[2].plane[0] == -1 and kl[0].plane[0] == 12
    # the batch
    best, occ, st, nfb = K.fuse_batch(P, kfs, grid, [dict(slot=s, ids=first, th_low=KS.TH) for s in (1, 2)])
    assert list(nfb) == [1, 1] and st[0][0] == K.REPLACE and occ[0][0] == 12 and st[1][0] == K.FREE and best[1][0] == 0
