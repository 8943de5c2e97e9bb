"""CPU: the plain-Python restatement of DBoW2's BowVector / L1 score and of KeyFrameDatabase.cc:76-309 / LoopClosing.cc:142-155
(tests/_kfdb_ref.py) against answers worked out by hand; the scenes of tests/_bow_scenes.py meet the conditions that keep the GPU tests
from being vacuous (asserted on the restatement alone); the new C-ABI names are declared and exported."""
import ctypes as C
import os

import numpy as np
import pytest

import _bow_scenes as scenes
import _kfdb_ref as ref

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
