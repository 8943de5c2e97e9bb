"""CPU: the restatement of the two-phase brute-force pair matcher (tests/_pairs_ref.py) on the constructed scenes of tests/_pairs_scenes.py.

For every scene and every record model (popcount, matrix cores unsliced, matrix cores sliced):
  (i)   resolve_model on the modelled records + the rotation histogram gives the vector and count of _bow_ref.search_by_bow_kf_kf (no
        nodes: the restated reference, FeatureMatcher.cc:587-641) and of the oracle binding;
  (ii)  the trace holds the class the scene is named for at the named row, the records show the named nk / head / tail;
  (iii) for every flip the scene sits on: a record flip breaks record_contract at the named row, an outcome flip changes the answer, a
        trace flip changes the class of the named row (see _pairs_ref.FLIP_KIND for why those four cannot change an answer);
  (iv)  record_contract accepts every modelled record, per slice too.
Without (ii) and (iii) tests/test_gpu_pairs_scenes.py could stay green without reaching the branches it exists for.  The last test shows
that every entry of FLIPS is caught by at least one scene.

The constants of the kernels the scenes are built around (nothing is imported from the kernels):
  TOPK = 4, RKEYS = 7        csrc/k_match.hip        keys of the popcount engine / slots of a record
  64 columns per tile        csrc/k_match_mfma.hip   T_TILE; lane half of column c = (c % 8) // 4 (the C/D layout of the 32x32 MFMA)
  64 rows per round          csrc/k_match.hip        the walk of k_match_resolve
  128 / 32 / 1024            csrc/afv_wave.h         AFV_FP_WLIST waiting rows per convergence, RW_RPW * AFV_FP_NW per step, AFV_FP_T threads
  1024                       csrc/k_match.hip        PAIR_KEYS_LDS: records of later live rows are read from global memory
  4096                       csrc/afv_api.hip        largest cap afv_match_bruteforce_pairs_device accepts
"""
import numpy as np
import pytest

import _bow_ref as R
import _pairs_ref as P
import _pairs_scenes as PS

SCENES = [s for kind in PS.KINDS for s in PS.small_scenes(kind) + PS.large_scenes(kind)]
IDS = [s.name for s in SCENES]
_CACHE = {}


def dist_of(s):
    if s.name not in _CACHE:
        _CACHE[s.name] = P.hamming(s.D1, s.D2)
    return _CACHE[s.name]


def run(s, model, flip=None):
    return P.match_pair(model, s.D1, s.D2, PS.TH[s.kind], s.ratio, s.ori, s.a1, s.a2, s.cap, flip, dist=dist_of(s))


def test_scene_names_are_unique_and_the_lists_are_paired_one_to_one():
    assert len(set(IDS)) == len(IDS)
    for kind in PS.KINDS:
        sizes = [n for n in IDS if n.startswith("sizes_") and n.endswith(kind)]
        assert len(sizes) == len(PS.N2S)
        assert {int(n.split("_")[1].split("x")[0]) for n in sizes} == set(PS.N1S)


@pytest.mark.parametrize("s", SCENES, ids=IDS)
def test_models_equal_the_restated_reference_and_the_oracle(oracle, s):
    """(i) and (iv)"""
    th = PS.TH[s.kind]
    kw = dict(angle1=s.a1, angle2=s.a2, th_low=th, nnratio=s.ratio, check_orientation=s.ori)
    want, wn = oracle.search_by_bow_kf_kf(s.D1, s.D2, **kw)
    ref, rn, _ = R.search_by_bow_kf_kf(s.D1, s.D2, **kw)
    assert rn == wn and np.array_equal(ref, want), "restated reference != oracle"
    dist = dist_of(s)
    n2 = dist.shape[1]
    for model in P.MODELS:
        got, gn, tr, recs = run(s, model)
        assert gn == wn and np.array_equal(got, want), model
        bad = [(i, msg) for i in range(len(recs)) for msg in [P.record_contract(recs[i], dist[i], n2)] if msg]
        assert bad == [], model
    nsl = P.topk_slices(s.cap, 1)
    _, per = P.records_sliced(dist, nsl)
    cols = P.slice_columns(n2, nsl)
    assert sum(len(c) for c in cols) == n2
    bad = [(i, k, msg) for i in range(len(dist)) for k in range(nsl)
           for msg in [P.record_contract(per[i, k], dist[i, cols[k]], len(cols[k]), cols[k])] if msg]
    assert bad == []


@pytest.mark.parametrize("s", SCENES, ids=IDS)
def test_the_scene_reaches_what_it_is_named_for(s):
    """(ii)"""
    e = s.expect
    for model in P.MODELS:
        got, gn, tr, recs = run(s, model)
        if s.rule is not None and model in s.models:
            assert tr["cls"][s.row] == s.rule, (model, tr["cls"][s.row])
        for row, col in e.get("cols", {}).items():
            assert got[row] == col, (model, row, got[row])
        for row, slot in e.get("slots", {}).items():
            assert tr["slot"][row] == slot, (model, row, tr["slot"][row])
        if "rescans" in e:
            assert len(tr["rescans"]) >= e["rescans"], (model, len(tr["rescans"]))
        if "nk" in e:
            assert recs[s.row][7] == e["nk"][model], (model, recs[s.row])
        if "head" in e:
            h = e["head"][model]
            assert recs[s.row][:len(h)].tolist() == h, (model, recs[s.row])
        if model in e.get("tail", ()):
            nk = int(recs[s.row][7])
            assert nk < P.RKEYS and all(int(k) != P.NO_KEY for k in recs[s.row][nk:P.RKEYS]), (model, recs[s.row])
        if e.get("second_far"):   # the clamped copies of the last column did not enter: the second key is filler
            assert (int(recs[s.row][1]) >> 16) > PS.TH[s.kind] + 5
        if "head_row5" in e:
            h = e["head_row5"][model]
            assert recs[5][:len(h)].tolist() == h, (model, recs[5])
        if "min_live" in e:
            assert int((tr["slot"] >= 0).sum()) >= e["min_live"] and all(tr["slot"][r] >= 1024 for r in e["behind_1024"])
            # contention is confined to the slots behind 1024: every other live row gets its first key's column
            lost = [i for i in range(len(got)) if tr["slot"][i] >= 0 and got[i] != (int(recs[i][0]) & 0xffff)]
            assert lost == [1036, 1037] == tr["rescans"], (model, lost[:5], tr["rescans"][:5])
    if "empty_slices" in e:
        _, per = P.records_sliced(dist_of(s), P.topk_slices(s.cap, 1))
        for k in e["empty_slices"]:
            assert per[s.row, k].tolist() == [P.NO_KEY] * 7 + [7]


def test_the_slices_are_where_the_scenes_put_their_columns():
    assert P.topk_slices(320, 1) == 3 and P.topk_slices(320, 0) == 1 and P.topk_slices(1300, 1) == 11 and P.topk_slices(4096, 1) == 16
    assert [(c[0], c[-1]) for c in P.slice_columns(257, 3)] == [(0, 127), (128, 255), (256, 256)]
    assert [len(c) for c in P.slice_columns(2, 3)] == [2, 0, 0]
    assert [int(c[0]) for c in P.slice_columns(1100, 11)[:9]] == [128 * k for k in range(9)]


def test_each_exact_prefix_length_occurs():
    for kind in PS.KINDS:
        seen = set()
        for s in PS.record_scenes(kind):
            if "nk" in s.expect:
                seen.add(int(run(s, "mfma")[3][s.row][7]))
        assert seen == {4, 5, 6, 7}


def flip_caught(s, flip):
    """does scene s notice the flipped rule?  (model -> what it saw) for the models that do"""
    seen = {}
    dist = dist_of(s)
    for model in P.MODELS:
        base, bn, btr, brecs = run(s, model)
        kind = P.FLIP_KIND[flip]
        if kind == "record":
            if flip == "slice_bound" and model != "sliced":
                continue
            recs = P.records(model, dist, s.cap, flip)
            msg = P.record_contract(recs[s.row], dist[s.row], dist.shape[1])
            if msg:
                seen[model] = msg
        elif kind == "outcome":
            got, gn, _, _ = run(s, model, flip)
            if gn != bn or not np.array_equal(got, base):
                seen[model] = "row %d: %d -> %d" % (s.row, base[s.row], got[s.row])
        else:
            turned = {flip, "guard_dropped"} if flip == "complete_ignored" else flip
            got, gn, tr, _ = run(s, model, turned)
            # a shortcut: the answer must NOT move, only the way to it
            assert gn == bn and np.array_equal(got, base), (s.name, flip, model)
            if flip == "complete_ignored":
                # `complete` and the n2 > nk guard cover for each other on every valid record (a NO_KEY inside the prefix means the list holds
                # all n2 < nk columns): either alone leaves even the classes alone, both together send the row to the last_d test
                for one in ("complete_ignored", "guard_dropped"):
                    assert run(s, model, one)[2]["cls"] == btr["cls"], (s.name, one, model)
            if tr["cls"][s.row] != btr["cls"][s.row] or (flip == "dead_kept_live" and tr["slot"][s.row] != btr["slot"][s.row]):
                seen[model] = "%s -> %s" % (btr["cls"][s.row], tr["cls"][s.row])
    return seen


FLIPPED = [(s, f) for s in SCENES for f in s.flips]


@pytest.mark.parametrize("s,flip", FLIPPED, ids=["%s/%s" % (s.name, f) for s, f in FLIPPED])
def test_the_outcome_depends_on_the_rule_the_scene_sits_on(s, flip):
    """(iii): under every record model the scene names (a record flip of the slice merge: under the sliced model)"""
    seen = flip_caught(s, flip)
    need = {"sliced"} if flip == "slice_bound" else set(s.models)
    assert need <= set(seen), (flip, sorted(need - set(seen)))


def test_every_flip_is_caught_by_at_least_one_scene():
    for kind in PS.KINDS:
        caught = {f for s, f in FLIPPED if s.kind == kind and flip_caught(s, f)}
        assert caught == set(P.FLIPS), (kind, sorted(set(P.FLIPS) - caught))
