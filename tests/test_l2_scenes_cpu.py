"""The duels of tests/_l2_scenes.py proved on the CPU (no device: nothing here launches).

  - the normative function of _l2_scenes.py is, bit for bit on every row of every scene, the restatements' (_refresh_ref.l2sqr,
    _proj_ref.l2sqr, the distances of _bow_ref and _stereo_ref) and the C oracle's: it is no eighth definition
  - every scene's outcome under the normative distance is the C oracle's, and CHANGES when the wrong arithmetic the scene is named
    after is plugged into the route's restatement: "flipping the rule changes the outcome"
  - every (wrong arithmetic, route) cell has a scene or stands in _l2_scenes.UNREACHABLE, and nothing else does
  - mutation check: each listed wrong arithmetic in a route's restatement makes at least one scene of that route fail; MUTATION_COUNTS
    holds a lower bound of the number of scenes that fail per cell
Without this file an edit to a generator could leave tests/test_gpu_l2_scenes.py green while it tells no arithmetic from another."""
import numpy as np
import pytest

import _bow_ref
import _l2_scenes as L
import _proj_ref
import _refresh_ref
import _stereo_ref

ROUTES = sorted(L.ROUTES)


def _rows_of(s):
    """(query, rows) pairs whose distances the scene's route evaluates"""
    i = s.inputs
    if "d1" in i:
        return [(a, i["d2"]) for a in i["d1"][[0, 1, 4, len(i["d1"]) - 1]]]
    if "rows" in i:
        return [(i["rows"][0], i["rows"]), (i["rows"][2], i["rows"])]
    if "case" in i:
        c = i["case"]
        if hasattr(c, "K1"):
            return [(c.K1.descriptors[0], c.K2.descriptors)]
        return [(c.Q.descriptors[0], c.F.descriptors), (c.Q.descriptors[-1], c.F.descriptors)]
    sc = i["scene"]
    if hasattr(sc, "feat"):
        return [(sc.P.descriptors[0], sc.feat.desc)]
    return [(sc.L.desc[-1], sc.R.desc)]


@pytest.mark.parametrize("route", ROUTES)
def test_the_normative_function_is_the_restatements_and_the_oracles(oracle, route):
    n = 0
    for s in L.scenes(route):
        d = s.duel
        for a, rows in _rows_of(s) + [(d.q, np.stack([d.a, d.b]))]:
            mine = L.l2sqr(a, rows)
            assert mine.dtype == np.float32
            assert mine.tobytes() == _proj_ref.l2sqr(a, rows).tobytes(), s.name
            assert mine.tobytes() == _bow_ref._dist(np.stack([a]), 0, rows, list(range(len(rows)))).tobytes(), s.name
            for k in (0, len(rows) // 2, len(rows) - 1):
                bits = mine[k].tobytes()
                assert np.float32(_refresh_ref.l2sqr(a, rows[k])).tobytes() == bits, s.name
                assert _stereo_ref.distance(a, rows[k]).tobytes() == bits, s.name
                assert np.float32(oracle.l2sqr(a, rows[k])).tobytes() == bits, s.name
                n += 1
    assert n > 20


def _oracle_outcome(oracle, s):
    i = s.inputs
    if "d1" in i:
        got, n = oracle.match_l2_bruteforce(i["d1"], i["d2"], L.TH, 1.0, i.get("valid1"), i.get("valid2"))
        return got, np.int32(n)
    if "rows" in i:
        bi, bm = oracle.distinctive_descriptor(i["rows"])
        return np.int32(bi), np.float32(bm)
    if "scene" in i:     # a point-store scene: the oracle on the restatement's own queries
        import _points_scenes as PSC
        sc = i["scene"]
        Q, o = sc.queries()
        got, n = oracle.match_projection(PSC.grid_view(L._afv(), sc), Q, th_high=sc.th, nnratio=sc.nnratio, check_orientation=False, last_frame=False)
        return np.asarray(got, np.int32), np.int32(n), np.asarray(o["in_view"], bool)
    c = i["case"]
    if hasattr(c, "K1"):
        import _match_scenes as MS
        got, n = MS.run_oracle(oracle, c)
        return np.asarray(got, np.int32), int(n)
    f = oracle.match_initialization if c.kind == "init" else oracle.match_projection
    got, n = f(c.F, c.Q, **c.kw)
    return np.asarray(got, np.int32), np.int32(n)


@pytest.mark.parametrize("route", ROUTES)
def test_every_scene_flips_and_the_oracle_gives_the_normative_outcome(oracle, route):
    scenes = L.scenes(route)
    assert scenes
    for s in scenes:
        assert s.flips(), (s.name, s.duel.how)
        if route != "stereo":        # (the C oracle has no stereo matcher: _stereo_ref.py is that route's only statement)
            assert L.same(_oracle_outcome(oracle, s), s.expected), s.name
    assert len({s.name for s in scenes}) == len(scenes)


def test_the_unreachable_cells_are_exactly_the_listed_ones():
    have = {(s.wrong, s.route) for r in ROUTES for s in L.scenes(r)}
    every = {(w, r) for w in L.WRONG for r in L.ROUTES}
    assert every - have == set(L.UNREACHABLE)
    assert all(isinstance(v, str) and v and "\n" not in v for v in L.UNREACHABLE.values())
    # a route is without a remainder only where an argument check refuses one (tests/test_gpu_l2_scenes.py sees each refusal on the
    # device): the dimensions a route happens to be run at are no reason
    assert {r for (w, r) in L.UNREACHABLE if w == "tail_first"} == set(L.REFUSES_TAIL)
    assert "distinctive" not in L.REFUSES_TAIL and "match_generic" not in L.REFUSES_TAIL   # both take any width: both have a scene of 7 floats
    assert all(any(s.dim % 4 for s in L.scenes(r) if s.wrong == "tail_first") for r in ("distinctive", "match_generic"))
    for (w, r), dims in L.cells().items():
        assert dims, (w, r)
        assert {s.dim for s in L.scenes(r) if s.wrong == w} == set(dims), (w, r)


# (wrong, route) -> scenes of the route whose outcome changes when the route's restatement evaluates the distance that way
MUTATION_COUNTS = {}


@pytest.mark.parametrize("route", ROUTES)
def test_mutating_the_distance_of_a_restatement_fails_a_scene_of_its_route(route):
    scenes = L.scenes(route)
    for w in L.WRONG:
        if (w, route) in L.UNREACHABLE:
            continue
        # (a scene whose duel distances keep their bits under w is not run: every other distance of a scene is far from every
        # threshold and from every other, so such a scene could only add to the count - the counts are lower bounds)
        moved = [s for s in scenes if L.l2sqr(s.duel.q, [s.duel.a, s.duel.b], w).tobytes() != s.duel.norm.tobytes()]
        MUTATION_COUNTS[(w, route)] = sum(not L.same(s.outcome(w), s.expected) for s in moved)
        assert MUTATION_COUNTS[(w, route)] >= 1, (w, route)
    print(route, {w: n for (w, r), n in sorted(MUTATION_COUNTS.items()) if r == route}, "of", len(scenes))


def test_the_hook_is_restored_and_defaults_to_the_normative_distance():
    for ref in (_proj_ref, _refresh_ref):
        assert ref.DISTANCE["l2sqr"] is ref.l2sqr
        with L.arithmetic("f32_sum"):
            assert ref.DISTANCE["l2sqr"] is not ref.l2sqr
        with L.arithmetic(None):
            a, b = np.float32([0.9, 0, 0, 0, 3]), np.float32([1, 0, 0, 0, 1])
            assert np.float32(_refresh_ref.DISTANCE["l2sqr"](a, b)).tobytes() == np.float32(_refresh_ref.l2sqr(a, b)).tobytes()
        assert ref.DISTANCE["l2sqr"] is ref.l2sqr


def test_the_pairs_scene_puts_a_candidate_at_every_column_of_a_staged_chunk():
    """... in the first and in a later chunk, for the chunk of 32 columns and for the one of 8 (1024 floats), and in both row tiles"""
    s = next(x for x in L.scenes("match_pairs") if x.dim == 1024)
    d1, d2 = s.inputs["d1"], s.inputs["d2"]
    assert d1.shape == (L.N1, 1024) and d2.shape == (L.N2, 1024)
    cols = np.flatnonzero(d2[:, -1] < L.FILLER_TAG)
    rows = np.flatnonzero(d1[:, -1] < L.FILLER_TAG)
    assert len(cols) == 2 * L.NDUEL and len(rows) == L.NDUEL and 64 in rows
    assert sum(r < 32 for r in rows) == 16 and sum(32 <= r < 64 for r in rows) == 16     # both halves of the wavefront's lanes
    for chunk in (32, 8):
        first = {c for c in cols if c < chunk}
        later = {c % chunk for c in cols if c >= chunk}
        assert first == set(range(chunk)) and later == set(range(chunk)), chunk
    for r in rows:      # each duel row sees exactly its own two candidates below the threshold
        assert int((L.l2sqr(d1[r], d2) < L.TH).sum()) == 2


def test_the_rescan_scene_uses_up_the_key_list():
    for s in L.scenes("rescan"):
        d1, d2 = s.inputs["d1"], s.inputs["d2"]
        near = np.argsort(L.l2sqr(d1[4], d2), kind="stable")[:4]
        assert set(near) == {0, 1, 2, 3} and all(s.expected[0][:4] == [0, 1, 2, 3]), s.name
        assert len(d2) > 4      # more valid columns than keys: the lists are not complete


def test_the_projection_scenes_use_up_the_key_lists():
    """in a used-up scene the first eight queries take the eight features nearest to the ninth, whose answer is one of the duel pair or none"""
    mine = [s for s in L.scenes("projection") if s.name.endswith("used-up")]
    assert {s.name.split("-")[3] for s in mine} == {"localmap", "lastframe", "init"}
    for s in mine:
        got = s.expected[0]
        if s.inputs["case"].kind == "init":
            assert list(got[:8]) == list(range(8)) and got[8] in (-1, 9, 10), s.name
        else:
            assert list(got[:8]) == list(range(8)) and got[8] == -1 and sorted(got[9:11])[0] == -1 and max(got[9:11]) in (-1, 8), s.name


def test_the_searched_seeds_are_the_ones_a_search_finds():
    """the committed seeds are findings of find_seeds(): a search over the first seeds reproduces one per dimension, and a search that
    finds nothing raises"""
    found = L.find_seeds(dims=(8, 64), nseeds=4)
    for key, val in found.items():
        assert L.SEEDS[key] == val, key
    with pytest.raises(AssertionError, match="no duel found"):
        L.find_seeds(dims=(8,), nseeds=0)
