"""CPU: the plain-Python restatement of DBoW2's BowVector / L1 score and of KeyFrameDatabase.cc:76-309 / LoopClosing.cc:142-155
(tests/_kfdb_ref.py) against answers worked out by hand; the scenes of tests/_bow_scenes.py meet the conditions that keep the GPU tests
from being vacuous (asserted on the restatement alone); the new C-ABI names are declared and exported.  The constructed scenes of tests/_kfdb_scenes.py:
each reaches the rule it names (trace counters) and is moved by the flip it names - a scene that no flip moves fails."""
import ctypes as C
import os

import numpy as np
import pytest

import _bow_scenes as scenes
import _kfdb_ref as ref
import _kfdb_scenes as ks

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("afv_vocab_set_weights", "afv_bow_vector", "afv_frame_get_bowvec", "afv_table_set_bowvec", "afv_table_score_bow")


def test_header_and_library_export_the_new_names(afv):
    header = open(os.path.join(ROOT, "include", "afv_hip.h")).read()
    lib = C.CDLL(afv._lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in afv._lib.SYMBOLS
    assert "afv_bow_query" in header and afv._lib.BowQuery._fields_[0][0] == "struct_size"
    assert afv._lib.ABI_VERSION == 6 and "#define AFV_ABI_VERSION 6" in header      # new symbols and records only
    assert afv.KeyFrameDatabase is not None and hasattr(afv.table.DescriptorTable, "score_bow") and hasattr(afv.Frame, "bowvec")


def test_bow_query_mirror_matches_the_header(tmp_path, afv):
    import subprocess
    st = afv._lib.BowQuery
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "afv_hip.h"', 'int main(void) {', '  printf("%zu\\n", sizeof(afv_bow_query));']
    lines += ['  printf("%%zu\\n", offsetof(afv_bow_query, %s));' % f for f, _ in st._fields_] + ['  return 0;', '}']
    src = tmp_path / "q.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "q"
    r = subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()]
    assert got == [C.sizeof(st)] + [getattr(st, f).offset for f, _ in st._fields_]


def test_score_by_hand():
    """v = {1: 0.5, 4: 0.25, 9: 0.25}, w = {1: 0.25, 5: 0.5, 9: 0.25} (all exact in binary): shared words 1 and 9.
    word 1: |0.5 - 0.25| - 0.5 - 0.25 = -0.5; word 9: |0.25 - 0.25| - 0.25 - 0.25 = -0.5; s = -1.0; score = 0.5"""
    v = {1: 0.5, 4: 0.25, 9: 0.25}
    w = {1: 0.25, 5: 0.5, 9: 0.25}
    assert ref.l1_score(v, w) == (2, 0.5, 1)
    assert ref.l1_score(w, v) == (2, 0.5, 1)
    assert ref.l1_score(v, {2: 1.0}) == (0, 0.0, -1) and ref.l1_score(v, {}) == (0, 0.0, -1)
    assert ref.l1_score({7: 0.5, 9: 0.5}, v) == (1, 0.25, 9)
    # identical vectors: 1.0 up to the rounding the sum really has (thirds do not add up to one exactly in every order)
    assert ref.score(v, v) == 1.0
    third = {k: 1.0 / 3.0 for k in (2, 3, 5)}
    s = 0.0
    for _ in range(3):
        s = s + (0.0 - 1.0 / 3.0 - 1.0 / 3.0)
    assert ref.score(third, third) == -s / 2.0 and abs(ref.score(third, third) - 1.0) < 1e-15


def test_bow_vector_by_hand():
    weight = np.array([0.0, 0.1, 0.0, 2.0, 0.7])
    word_id = np.array([-1, 0, 1, 2, 3])
    # leaves: word 0 six times (repeated addition), the stopped word 1 twice, word 3 once, word 2 never
    b = ref.bow_vector([1, 4, 1, 2, 1, 1, 2, 1, 1], weight, word_id)
    five = 0.1 + 0.1 + 0.1 + 0.1 + 0.1 + 0.1
    assert five != 6 * 0.1                                   # what "repeated addition" is about
    norm = five + 0.7
    assert list(b.items()) == [(0, five / norm), (3, 0.7 / norm)]
    assert ref.bow_vector([2, 2], weight, word_id) == {} and ref.bow_vector([], weight, word_id) == {}


def _db(bows):
    db = ref.KeyFrameDatabaseRef()
    for i, b in enumerate(bows):
        db.add(i, b)
    return db


def test_common_word_gate_by_hand():
    """int(5 * 0.8f) == 4: a keyframe with 5 common words passes (5 > 4), one with 4 does not"""
    assert int(F32(5) * F32(0.8)) == 4
    q = {k: 0.125 for k in range(8)}
    five = {k: 0.2 for k in range(5)}
    four = {k: 0.25 for k in range(4)}
    tr = {}
    out = _db([five, four]).detect_relocalization_candidates(q, lambda s: [], tr)
    assert tr["sharing"] == [0, 1] and tr["min_common"] == 4 and tr["scored"] == [0] and out == [0]


def test_min_score_equality_and_neighbours_by_hand():
    q = {0: 0.5, 1: 0.5}
    a = {0: 0.5, 1: 0.5}          # score 1.0
    b = {0: 0.25, 1: 0.25, 2: 0.5}  # score 0.5
    c = {5: 1.0}                    # shares nothing: never part of the query set
    db = _db([a, b, c])
    assert ref.score(q, b) == 0.5
    tr = {}
    # si >= minScore: equality passes; b alone is below 0.75 * best accumulated score
    assert db.detect_loop_candidates(q, 0.5, [], lambda s: [], tr) == [0]
    assert tr["passed"] == [0, 1] and tr["acc"] == [(1.0, 0), (0.5, 1)]
    assert db.detect_loop_candidates(q, np.nextafter(F32(0.5), F32(1)), [], lambda s: [], tr) == [0] and tr["passed"] == [0]
    # a neighbour outside the query set (c) is skipped, one inside adds its score and takes over when it is better;
    # both entries then name keyframe 0: the duplicate is dropped, the first occurrence stays
    covis = {0: [2, 1], 1: [2, 0]}
    assert db.detect_loop_candidates(q, 0.25, [], lambda s: covis.get(s, []), tr) == [0]
    assert tr["acc"] == [(1.5, 0), (1.5, 0)]
    assert db.detect_relocalization_candidates(q, lambda s: covis.get(s, []), tr) == [0] and tr["acc"] == [(1.5, 0), (1.5, 0)]
    # a connected keyframe never becomes a candidate
    assert db.detect_loop_candidates(q, 0.25, [0], lambda s: covis.get(s, []), tr) == [1] and tr["sharing"] == [1]
    assert ref.min_score_to_connected(q, [a, b]) == F32(0.5) and ref.min_score_to_connected(q, []) == F32(1)
    # order: keyframes are met word by word, inside a word in insertion order; erase + add moves a keyframe to the end of its lists
    db.detect_relocalization_candidates(q, lambda s: [], tr)
    assert tr["sharing"] == [0, 1]
    db.erase(0); db.add(0, a)
    db.detect_relocalization_candidates(q, lambda s: [], tr)
    assert tr["sharing"] == [1, 0]


@pytest.mark.parametrize("kind", ["orb32", "akaze61", "sift128"])
def test_scenes_meet_their_conditions(afv, kind):
    """asserted on the restatement alone: (a) non-empty results, (b) a keyframe shares words but fails > minCommonWords, (c) one passes
    that and fails the score / 0.75f gate, (d) the covisibility accumulation changes the keyframe of an entry, (e) loops: a connected
    keyframe that shares words is excluded.  Also: vocabulary.py's vectors_from_nodes equals the restatement bit for bit."""
    s = scenes.scene(kind)
    voc = scenes.vocabulary(kind)
    assert voc.size() >= 10000 and 64 <= s.nkf <= 200
    bows = [ref.bow_vector(l, s.weight, s.word_id) for l in s.leaves]
    for i in (0, 31, s.nkf - 1):
        merged, _ = voc.vectors_from_nodes(s.leaves[i], np.zeros_like(s.leaves[i]))
        assert list(merged.keys()) == list(bows[i].keys())
        assert np.array(list(merged.values())).tobytes() == np.array(list(bows[i].values())).tobytes()
    db = ref.KeyFrameDatabaseRef()
    for i in range(s.nkf - 1):
        db.add(i, bows[i])
    fbow = ref.bow_vector(s.frame_leaves, s.weight, s.word_id)
    tr = {}
    out = db.detect_relocalization_candidates(fbow, s.best_covisibles, tr)
    _conditions(out, tr)
    ms = ref.min_score_to_connected(bows[s.loop_slot], [bows[j] for j in s.connected])
    assert 0 < ms < 1
    out = db.detect_loop_candidates(bows[s.loop_slot], ms, s.connected, s.best_covisibles, tr)
    _conditions(out, tr)
    assert any(ref.l1_score(bows[s.loop_slot], bows[j])[0] > tr["min_common"] for j in s.connected)   # (e): it would have been scored
    assert not set(s.connected) & set(tr["sharing"])


def _conditions(out, tr):
    assert len(out) >= 1                                                              # (a)
    assert len(tr["scored"]) < len(tr["sharing"])                                     # (b)
    failed = [k for (a, k), kf in zip(tr["acc"], tr["passed"]) if not a > tr["min_retain"]]
    assert len(tr["passed"]) < len(tr["scored"]) or failed                            # (c)
    assert any(k != kf for (a, k), kf in zip(tr["acc"], tr["passed"]) if a > tr["min_retain"])   # (d): a returned entry names another keyframe


# ---------------- the constructed scenes of tests/_kfdb_scenes.py: every rule is reached, every scene is moved by its flip ----------------

def _bits(bow):
    return list(bow.keys()), np.array(list(bow.values()), np.float64).tobytes()


def test_flips_are_named_and_silent_by_default():
    assert len(set(ref.FLIPS)) == 14
    with pytest.raises(ValueError):
        ref.bow_vector([], [], [], flip="common_ge")
    with pytest.raises(ValueError):
        ref.l1_score({}, {}, flip="no_such_flip")
    tr = {}
    assert _db([{0: 1.0}]).detect_relocalization_candidates({0: 1.0}, lambda s: [], tr) == [0]
    assert all(tr[c] == 0 for c in ref.COUNTERS)


def test_bow_scenes_cover_the_sizes_the_issue_names():
    S = {s.name: s for s in ks.bow_scenes()}
    assert len(S) == len(ks.bow_scenes())
    assert {len(s.leaves) for s in S.values()} >= {0, 1, 63, 64, 65, 1023, 1024, 1025, 4097, 8192}
    assert {len(s.want()) for s in S.values()} >= {0, 1, 1024, 1025, 2049, 8192}
    w = ks.weights("mixed")
    pos = w[w > 0]
    assert pos.min() < 2.0 ** -38 and pos.max() > 2.0 ** 9 and len(set(np.frexp(pos)[1].tolist())) >= 50
    _, word_id, is_leaf = ks.tree()
    assert int(is_leaf.sum()) == 10000
    # the descriptor pool reaches every leaf a scene uses, by the CPU descent
    desc, leaf, reach, row_of = ks.pool()
    for s in S.values():
        assert set(s.leaves.tolist()) <= set(reach.tolist())
    assert all(leaf[row_of[int(l)]] == l for l in reach[::97])
    # runs_3_9: in the sorted keys, runs of 3 and of 9 start at every offset modulo the 8 keys of a thread's stretch
    keys = np.sort(word_id[S["runs_3_9"].leaves])
    starts = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1]])
    length = np.diff(np.r_[starts, len(keys)])
    for run in (3, 9):
        assert set((starts[length == run] % 8).tolist()) == set(range(8))
    # heavy_word: one run of 8190 keys; half_stopped: stopped and kept features alternate all through the feature order
    hw = word_id[S["heavy_word"].leaves]
    assert np.bincount(hw).max() == 8190
    for name in ("half_stopped_8192", "half_stopped_4097"):
        kept = S[name].weight[S[name].leaves] > 0
        assert 0.3 < kept.mean() < 0.7 and kept[:64].any() and (~kept[:64]).any() and kept[-64:].any() and (~kept[-64:]).any()
    assert not (S["all_stopped"].weight > 0).any() and S["all_stopped"].want() == {}


@pytest.mark.parametrize("scene", ks.bow_scenes(), ids=lambda s: s.name)
def test_bow_scene_is_moved_by_its_flips(scene):
    want = scene.want()
    assert list(want.keys()) == sorted(want.keys())
    if not scene.flips:
        # a size edge: at most one entry, and then its value is v / v = 1.0: there is no arithmetic a flip could change
        assert len(want) <= 1 and list(want.values()) in ([], [1.0])
        assert all(_bits(scene.want(f)) == _bits(want) for f in ref.BOW_FLIPS)
        return
    for f in scene.flips:
        assert f in ref.BOW_FLIPS
        assert _bits(scene.want(f)) != _bits(want), "%s is not moved by %s" % (scene.name, f)
        assert list(scene.want(f).keys()) == list(want.keys())          # the flips move bits, not words


def test_score_scenes_follow_the_launch_rule():
    S = {s.name: s for s in ks.score_scenes()}
    assert ks.slots_per_wg(5, 99) == 4 and ks.slots_per_wg(1, 1) == 4 and ks.slots_per_wg(65535, 100000) == 64
    for name, per in (("batch_8", 8), ("batch_64", 64)):
        s = S[name]
        assert ks.slots_per_wg(len(s.queries), s.nsets) == per and s.nsets % per and s.cap <= 40
        kinds = [x if isinstance(x, str) else "bow" for x in s.slots]
        assert kinds.count(ks.NO_BOW) >= 3 and kinds.count(ks.EMPTY) >= 3 and 0 < s.mask.sum() < s.nsets
        assert any(isinstance(x, dict) and not x for x in s.slots) and any(isinstance(q, tuple) for q in s.queries)
        assert len({id(s.query_bow(q)) for q in s.queries}) <= 40          # a handful of distinct queries, repeated
        # the slots one wavefront visits in a row never hold the same vector
        assert all(s.slots[i] is not s.slots[i + 4] or isinstance(s.slots[i], str) for i in range(s.nsets - 4))
    for s in S.values():
        if not s.name.startswith("batch"):
            assert ks.slots_per_wg(len(s.queries), s.nsets) == 4
    sizes = {len(x) for x in S["chunk_edges"].slots if isinstance(x, dict)}
    assert sizes >= {0, 1, 63, 64, 65, 129}
    assert {len(S["query_edges"].query_bow(q)) for q in S["query_edges"].queries} >= {0, 1, 8192}


@pytest.mark.parametrize("scene", ks.score_scenes(), ids=lambda s: s.name)
def test_score_scene_is_moved_by_its_flips(scene):
    common, score, first = scene.want()
    for r, s, (c, sc, f) in scene.facts:                                 # the cells worked out by hand
        assert (common[r, s], first[r, s]) == (c, f), (scene.name, r, s)
        if sc is not None:
            assert score[r, s].tobytes() == np.float64(sc).tobytes(), (scene.name, r, s)   # bits: -0.0 is not +0.0
    assert scene.flips
    for f in scene.flips:
        c2, s2, f2 = scene.want(flip=f)
        assert s2.tobytes() != score.tobytes(), "%s is not moved by %s" % (scene.name, f)
        assert np.array_equal(c2, common) and np.array_equal(f2, first)
    masked = scene.want(mask=scene.mask)
    assert (masked[0][:, scene.mask == 0] == -1).all() and np.array_equal(masked[0][:, scene.mask == 1], common[:, scene.mask == 1])


def test_zero_scores_carry_the_sign_the_reference_gives():
    s = [x for x in ks.score_scenes() if x.name == "signed_values"][0]
    _, score, _ = s.want()
    assert score[0, 1] == 0 and np.signbit(score[0, 1])                  # shared words, all terms +0: -(+0) / 2
    assert score[0, 3] == 0 and not np.signbit(score[0, 3])              # nothing shared: the literal 0


@pytest.mark.parametrize("scene", ks.decision_scenes(), ids=lambda s: s.name)
def test_decision_scene_reaches_its_rule_and_is_moved_by_its_flip(scene):
    traces = []
    want = ks.run_ref(scene, traces=traces)
    assert any(isinstance(a, list) and a for a in want)                  # some query returns candidates
    if scene.counter:
        assert sum(t[scene.counter] for t in traces) >= 1, "%s never meets %s" % (scene.name, scene.counter)
    assert scene.flip in ref.DETECT_FLIPS
    flipped = ks.run_ref(scene, flip=scene.flip)
    assert [list(a) if isinstance(a, list) else a.tobytes() for a in flipped] != \
        [list(a) if isinstance(a, list) else a.tobytes() for a in want], "%s is not moved by %s" % (scene.name, scene.flip)
    assert ks.run_ref(scene) == want                                     # a fresh database gives the same answers
    out = ks.parse_script_output("".join("%s: %s\n" % ("minscore" if not isinstance(a, list) else "q", float(a).hex() if not isinstance(a, list)
                                                         else " ".join(map(str, a))) for a in want))
    assert [a if isinstance(a, list) else a.tobytes() for a in out] == [a if isinstance(a, list) else a.tobytes() for a in want]


def test_decision_scenes_cover_every_flip_and_the_edges():
    S = ks.decision_scenes()
    assert {s.flip for s in S} == set(ref.DETECT_FLIPS)
    adds = [[op[1] for op in s.ops if op[0] == "add"] for s in S]
    assert all(a != sorted(a) for a in adds)                             # never in ascending slot order
    covis = [c for s in S for v in s.covis.values() for c in v]
    assert any(c >= 8 for c in covis) and any(c < 0 for c in covis)      # covisibles outside the table
    assert any(op[0] == "erase" and any(op[1] in v for v in s.covis.values()) for s in S for op in s.ops)   # an erased covisible
    assert any(op[0] == "loop" and set(op[3]) & {c for v in s.covis.values() for c in v} for s in S for op in s.ops)   # connected and covisible
    # int(max * 0.8f) in float: 0.8f is above 0.8, the products truncate where the scenes say
    assert [int(F32(m) * F32(0.8)) for m in (2, 5, 7, 8)] == [1, 4, 5, 6]
    assert "script " in ks.script_text(S[0])


class _RestatedTable:
    """DescriptorTable.score_bow answered by the restatement: what database.py needs of a table, without a device"""

    def __init__(self, scene):
        self.nsets, self.bows = scene.nsets, scene.bows

    def score_bow(self, queries, slot_mask=None, want_first=True):
        common = np.full((len(queries), self.nsets), -1, np.int32); score = np.zeros((len(queries), self.nsets)); first = np.full((len(queries), self.nsets), -1, np.int32)
        for r, q in enumerate(queries):
            qb = self.bows[q] if isinstance(q, (int, np.integer)) else dict(zip(q[0].tolist(), q[1].tolist()))
            for s, b in self.bows.items():
                if slot_mask is None or slot_mask[s]:
                    common[r, s], score[r, s], first[r, s] = ref.l1_score(qb, b)
        return common, score, first if want_first else None


@pytest.mark.parametrize("scene", ks.decision_scenes(), ids=lambda s: s.name)
def test_decision_scene_on_the_python_mirror_over_restated_scores(afv, scene):
    """database.py's own float arithmetic, order and bookkeeping, with the scores taken from the restatement (the device route is
    tests/test_gpu_kfdb_scenes.py)"""
    got = ks.run_db(scene, afv.KeyFrameDatabase(_RestatedTable(scene)))
    want = ks.run_ref(scene)
    assert [a if isinstance(a, list) else a.tobytes() for a in got] == [a if isinstance(a, list) else a.tobytes() for a in want]
