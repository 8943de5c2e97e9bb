"""the CPU oracle and the host containers against the plain restatement tests/_quant_ref.py on the scenes of tests/_quant_scenes.py (leaf and nid of
every feature, FeatureVector, BowVector: every one an equality), and the proof - from the restatement's own trace - that each scene reaches the rule
it was built for: a tie whose positions lie in different 16-child chunks, the winner on the named lane, four rows of a wavefront at four depths, an id
order that differs from record order on the level used, a key present in two 1024-feature chunks.  With a rule's wrong alternative (the last minimum,
a float32 sum, a reversed sum, nodes in record order, stopped words kept, nid one level off) the restatement's result on the scene built for that
rule changes.  Without these checks an edit to a generator could leave tests/test_gpu_quant_scenes.py green while it tests nothing."""
import numpy as np
import pytest

import _quant_ref as R
import _quant_scenes as S

_VOC = {}


def _voc(afv, tree):
    """the package's host-side Vocabulary of a scene's tree (no device: nothing here launches)"""
    if tree.name not in _VOC:
        _VOC[tree.name] = afv.Vocabulary(tree.k, tree.L, tree.parent, tree.node_desc, tree.weight, tree.is_leaf)
    return _VOC[tree.name]


@pytest.mark.parametrize("kind", S.KINDS)
def test_oracle_and_containers_are_the_restatement(afv, oracle, kind):
    for sc in S.all_scenes(kind):
        leaf, nid, _, fv, bow = S.ref(sc)
        voc = _voc(afv, sc.tree)
        oleaf, onid = oracle.bow_transform(voc, sc.features, sc.levelsup)
        assert np.array_equal(oleaf, leaf) and np.array_equal(onid, nid), sc
        vbow, vfv = voc.vectors_from_nodes(np.asarray(leaf), np.asarray(nid))
        assert vfv == fv and list(vbow.items()) == list(bow.items()), sc
        assert all(sc.tree.ref.is_leaf[v] for v in leaf.tolist()), sc


def _changed(sc, **wrong):
    """(leaf, nid, FeatureVector) of the scene under a wrong alternative"""
    rules = R.Rules(**wrong)
    if set(wrong) <= {"record_order", "keep_stopped"}:      # rules of the FeatureVector alone: the descent is the scene's
        leaf, nid = S.ref(sc)[:2]
    else:
        leaf, nid = R.transform_nodes(sc.tree.ref, sc.features, sc.levelsup, rules)
    return leaf, nid, R.feature_vector(sc.tree.ref, leaf, nid, rules)


# ---------------------------------------------------------------- the descent ----------------------------------------------------------------
@pytest.mark.parametrize("kind", S.KINDS)
def test_chunk_edges_reach_their_lanes(kind):
    sc = S.chunk_edges(kind)
    leaf, nid, trace, _, _ = S.ref(sc)
    seen = set()
    for i, (count, pos) in enumerate(sc.facts["want"]):
        step = trace[i][1]
        assert len(trace[i]) == 2 and (step["count"], step["pos"], step["chunk"]) == (count, pos, pos // 16), (sc, i, step)
        assert leaf[i] == sc.tree.ref.children[int(nid[i])][pos]
        seen.add((count, pos))
    for count in S.CHUNK_COUNTS:
        want = {(count, 0), (count, count - 1)} | {(count, p) for p in (15, 31, 47, 16, 32, 48) if p < count}
        assert want <= seen, (count, want - seen)
    assert {c for c, _ in seen} == set(S.CHUNK_COUNTS)
    level1 = sc.tree.ref.children[0]
    assert sorted(set(nid.tolist())) == level1 and max(level1) in nid                 # every node of the level used, the one of the highest rank among them
    assert {(49, 48), (33, 32), (17, 16), (16, 15), (32, 31), (48, 47)} <= seen      # lane 0 of a last chunk that holds one child; a winner that is lane 15 and the last child


@pytest.mark.parametrize("kind", S.KINDS)
def test_ties_lie_across_chunks_and_the_first_wins(kind):
    sc = S.tie_scene(kind)
    leaf, nid, trace, _, _ = S.ref(sc)
    wleaf, _, _ = _changed(sc, last_minimum=True)
    assert [w for w in sc.facts["want"][:5]] == [list(c) for c in S.TIE_CASES]
    for i, tied in enumerate(sc.facts["want"]):
        step = trace[i][1]
        kids = sc.tree.ref.children[int(nid[i])]
        assert step["count"] == 49 and step["tied"] == tied and step["pos"] == tied[0], (sc, i, step)
        assert len({p // 16 for p in tied}) == len(tied)                               # every tied position in a chunk of its own
        assert leaf[i] == kids[tied[0]] and wleaf[i] == kids[tied[-1]] and wleaf[i] != leaf[i]
        same = all(np.array_equal(sc.tree.node_desc[kids[tied[0]]], sc.tree.node_desc[kids[p]]) for p in tied[1:])
        assert same == (i < len(S.TIE_CASES))                                          # exact copies; binary kinds: also different descriptors at one distance
        assert not np.array_equal(sc.features[i], sc.tree.node_desc[kids[tied[0]]])    # the tie is at a distance > 0
    assert len(sc.facts["want"]) == (5 if S.is_float(kind) else 7)
    assert [17, 35] in sc.facts["want"] and [5, 21, 37] in sc.facts["want"]            # chunk 0 holds only worse children; three chunks


@pytest.mark.parametrize("kind", [k for k in S.KINDS if S.is_float(k)])
def test_float_order_scenes_change_under_the_wrong_sum(kind):
    f32, rev = S.order_scenes(kind)
    for sc, wrong in ((f32, {"float32_sum": True}), (rev, {"reversed_sum": True})):
        leaf, _, trace, _, _ = S.ref(sc)
        wleaf, _, _ = _changed(sc, **wrong)
        assert sc.n == S.ORDER_PAIRS and (wleaf != leaf).all(), (sc, leaf, wleaf)
        for i in range(sc.n):                                                            # the pair built for the query decides, both ways round
            assert {int(leaf[i]), int(wleaf[i])} == {1 + 2 * i, 2 + 2 * i} and trace[i][0]["count"] == 2 * S.ORDER_PAIRS
        rows = sc.tree.node_desc[1:]
        assert (np.frexp(rows)[0] * 2.0 ** 24 % 2 == 1).sum() > rows.size // 16        # full mantissas: the last of the 24 bits is set in many of them


@pytest.mark.parametrize("kind", S.KINDS)
def test_ragged_scenes_reach_their_rules(kind):
    scenes = {s.name: s for s in S.ragged_scenes(kind)}
    assert len(scenes) == 2 * len(S.RAGGED_LEVELSUP) * len(S.N_SMALL)
    assert S.RAGGED_LEVELSUP == (0, 1, S.RAGGED_L - 1, S.RAGGED_L, S.RAGGED_L + 3) and S.N_SMALL == (0, 1, 2, 3, 5, 63, 64, 65)
    for scheme in ("dfs", "perm"):
        tree = S.ragged_tree(kind, scheme).ref
        assert {tree.depth[i] for i in range(len(tree.parent)) if tree.is_leaf[i]} == {1, 2, 3, 4}
        assert tree.record != sorted(tree.record)                                      # ids are not breadth first
        assert max(len(c) for c in tree.children) > 16
        for levelsup in S.RAGGED_LEVELSUP:
            sc = scenes["ragged_%s_%s_up%d_n65" % (scheme, kind, levelsup)]
            leaf, nid, trace, fv, _ = S.ref(sc)
            for w in range(0, 64, 4):                                                  # the four rows of a wavefront stop at four depths
                assert sorted(len(trace[i]) for i in range(w, w + 4)) == [1, 2, 3, 4], (sc, w)
            level = S.RAGGED_L - levelsup
            if level <= 0:
                assert not nid.any() and [n for n, _ in fv] == [0]
                continue
            assert all(tree.depth[v] == level for v in nid.tolist() if v) and (nid == 0).any() == (level > 1) and (nid != 0).any()
            at_level = [v for v in tree.record if tree.depth[v] == level]
            if level == 1:                                                             # (the children of one node are in id order in every tree)
                assert at_level == sorted(at_level)
            elif scheme == "perm":                                                     # id order differs from record order on the level used ...
                assert at_level != sorted(at_level)
                assert _changed(sc, record_order=True)[2] != fv, sc                    # ... and on the nodes this frame reaches
            else:                                                                      # depth-first ids ascend along every level
                assert at_level == sorted(at_level) and at_level != list(range(at_level[0], at_level[0] + len(at_level)))
            assert not np.array_equal(_changed(sc, nid_off=1)[1], nid) and not np.array_equal(_changed(sc, nid_off=-1)[1], nid), sc
            kept = sum(len(v) for _, v in fv)
            assert 0 < kept < sc.n and _changed(sc, keep_stopped=True)[2] != fv, sc     # stopped words among the reached leaves


# ---------------------------------------------------------------- FeatureVector regimes ----------------------------------------------------------------
def _keys(sc):
    leaf, nid, _, fv, _ = S.ref(sc)
    kept = np.array([sc.tree.weight[v] > 0 for v in leaf.tolist()], bool)
    return nid, kept, fv


@pytest.mark.parametrize("kind", S.KINDS)
def test_regime_scenes_reach_their_regimes(kind):
    scenes = {s.name[len("regime_"):-len("_" + kind)]: s for s in S.regime_scenes(kind)}
    assert list(scenes) == S.regime_names(kind) and len(scenes) == 21
    assert {s.n for s in scenes.values()} >= set(S.N_LARGE) and max(s.n for s in scenes.values()) == S.FRAME_CAP
    widths = {}
    for name, sc in scenes.items():
        nid, kept, fv = _keys(sc)
        tree = sc.tree.ref
        level = tree.L - sc.levelsup
        widths[name] = 1 + sum(1 for d in tree.depth if d == level) if level > 0 else 1
        assert sorted(i for _, v in fv for i in v) == np.flatnonzero(kept).tolist()
        stopped = sc.facts["stopped"]
        assert {"none": kept.all(), "all": not kept.any() and fv == [], "half": 0.3 * sc.n < kept.sum() < 0.7 * sc.n,
                "some": 0.7 * sc.n < kept.sum() < sc.n}[stopped], (name, kept.sum())
        layout = sc.facts["layout"]
        if layout == "one_node":
            assert len(set(nid.tolist())) == 1 and nid[0] == max(v for v in range(len(tree.depth)) if tree.depth[v] == level)   # the last key of the level
            if stopped == "none":                                                      # 64 equal keys in a wavefront: the per-wave byte at its maximum
                assert kept[:64].all()
        elif layout == "own_node":
            assert len(set(nid.tolist())) == sc.n
        elif layout == "alternate":
            assert len(set(nid[0::2].tolist())) == 1 and len(set(nid[1::2].tolist())) == 1 and nid[0] != nid[1]
        elif layout in ("waves40", "second_chunk") and level == 2:
            assert 30 <= len(set(nid.tolist())) <= 41
            for w0 in range(0, sc.n - 63, 64):                                          # many distinct repeated keys in every wavefront
                _, cnt = np.unique(nid[w0:w0 + 64][kept[w0:w0 + 64]], return_counts=True)
                assert stopped == "all" or (cnt >= 2).sum() >= (2 if w0 & 64 else 6 if stopped == "none" else 3), (name, w0)
        if sc.n > 1024 and layout in ("one_node", "alternate", "waves40") and stopped != "all" and level == 2:
            first, second = set(nid[:1024][kept[:1024]].tolist()), set(nid[1024:2048][kept[1024:2048]].tolist())
            assert first & second, name                                                # a key in two chunks: its start carries over
            if sc.n > 2048:
                assert first & second & set(nid[2048:][kept[2048:]].tolist()), name
        if layout == "second_chunk":
            special = set(nid[1024:2048][kept[1024:2048]].tolist()) - set(nid[:1024].tolist()) - set(nid[2048:].tolist())
            assert [v for v in special if (nid == v).sum() > 50] != [], name           # a node of many features, all of them in the second chunk
    assert widths["waves40_w4096"] == 4096 and widths["own_node_n3000"] == 4096        # the last width of the counting sort
    assert widths["quad_n1023"] == widths["quad_n2049"] == widths["quad_n3000"] == 4097  # the first width that ranks by comparison
    assert widths["width1_L"] == widths["width1_beyond"] == 1 and widths["width17"] == 17 and widths["waves40_half"] == 257
    q = scenes["quad_n1023"]
    assert q.n % 4 == 3 and q.facts["stopped"] == "half" and len(set(_keys(q)[0].tolist())) < q.n   # not a multiple of 4, stopped words, repeated keys


@pytest.mark.parametrize("kind", S.KINDS)
def test_regime_trees_are_renumbered(kind):
    """on the wide trees too the ids of the level used are not in record order, and the stopped words change the FeatureVector"""
    for sc in S.regime_scenes(kind):
        tree = sc.tree.ref
        level = tree.L - sc.levelsup
        _, _, _, fv, _ = S.ref(sc)
        if level > 1 and len(fv) > 1:                                                  # (the children of the root are in id order in every tree)
            assert _changed(sc, record_order=True)[2] != fv, sc
        if sc.facts["stopped"] != "none":
            assert _changed(sc, keep_stopped=True)[2] != fv, sc
