"""-m gpu: the constructed place-recognition scenes of tests/_kfdb_scenes.py on the device and through both mirrors of KeyFrameDatabase,
against the plain-Python restatement (tests/_kfdb_ref.py).  tests/test_kfdb_ref_cpu.py shows without a GPU that every scene reaches the
rule it names and is moved by the matching flip of the restatement; here the same scenes run
  (a) through k_bowvec_build: Vocabulary.bow_vector (host leaves) and a resident Frame (bow_transform_nodes + bowvec);
  (b) through k_score_bow: DescriptorTable.score_bow with slot, frame and host queries, with and without mask, in batches that reach
      8 and 64 slots per workgroup;
  (c) through afv.KeyFrameDatabase (database.py) and afv::KeyFrameDatabase (adapter/afv_adapter.hpp, as the kfdb_selftest process).
No tolerance anywhere: word ids, counts, candidate lists in order and the bit pattern of every double / float."""
import os
import subprocess

import numpy as np
import pytest

import _bow_scenes as bs
import _kfdb_ref as ref
import _kfdb_scenes as ks
from test_gpu_bowvec import _frame, _parents, _same
from test_gpu_table_bow import KFDB_BIN, _arrays, _check

pytestmark = pytest.mark.gpu
_vocs = {}


def _voc(afv, ctx, key):
    """the scene tree with the weight array `key` in place of its own (one device vocabulary per array and context)"""
    if (id(ctx), key) not in _vocs:
        v0 = bs.vocabulary(ks.KIND)
        _vocs[(id(ctx), key)] = afv.Vocabulary(v0.k, v0.L, _parents(v0), v0.node_desc, ks.weights(key), v0.is_leaf, ctx)
    return _vocs[(id(ctx), key)]


# ---------------------------------------------------------------- (a) BowVector scenes ----------------------------------------------------------------
@pytest.mark.parametrize("scene", ks.bow_scenes(), ids=lambda s: s.name)
def test_bow_scene_from_host_leaves(afv, gpu_ctx, scene):
    voc = _voc(afv, gpu_ctx, scene.weight_key)
    assert np.array_equal(voc.word_id, ks.tree()[1])
    _same(voc.bow_vector(scene.leaves), scene.want())


def test_small_host_vectors_after_a_large_one(afv, gpu_ctx):
    """the context's arena still holds the 8192 entries of the call before: the 1-feature, empty and all-stopped scenes read none of it"""
    S = {s.name: s for s in ks.bow_scenes()}
    for name in ("words_8192", "n_1", "heavy_word", "n_0", "n_8192", "all_stopped", "n_1", "n_63"):
        _same(_voc(afv, gpu_ctx, S[name].weight_key).bow_vector(S[name].leaves), S[name].want())


def _resident(afv, fr, voc, scene):
    n = len(scene.leaves)
    kps = np.zeros(n, afv.KP_DTYPE)
    kps["x"] = np.arange(n) % 600 + 10
    kps["y"] = np.arange(n) % 400 + 10
    fr.set_features(kps, ks.descriptors_of(scene.leaves))
    leaf, _ = fr.bow_transform_nodes(voc)
    assert np.array_equal(leaf, scene.leaves)             # the pool's CPU descent is the device's
    return fr.bowvec()


def test_bow_scenes_on_a_resident_frame(afv, gpu_ctx):
    """every scene on ONE frame, one after the other: whatever a scene leaves behind in the frame's arrays meets the next one; the
    8192-feature scenes are each followed by the 1-feature scene and by the empty one (stale arena / LDS residue)"""
    S = {s.name: s for s in ks.bow_scenes()}
    fr = _frame(afv, gpu_ctx, ks.KIND, ks.descriptors_of(S["n_65"].leaves), cap=8192)
    order = []
    for s in ks.bow_scenes():
        order.append(s)
        if len(s.leaves) == 8192:
            order += [S["n_1"], S["n_0"], S["n_1"]]
    assert sum(len(s.leaves) == 8192 for s in order) >= 6
    for s in order:
        _same(_resident(afv, fr, _voc(afv, gpu_ctx, s.weight_key), s), s.want())
    fr.close()


# ---------------------------------------------------------------- (b) score scenes ----------------------------------------------------------------
def _score_table(afv, ctx, scene):
    t = afv.table.DescriptorTable(ctx, scene.nsets, scene.cap)
    one = np.full((1, 32), 0x5a, np.uint8)
    for s, b in enumerate(scene.slots):
        if b == ks.EMPTY:
            continue
        t.set(s, one)                                      # a slot scores only when it holds features
        if b != ks.NO_BOW:
            t.set_bowvec(s, *_arrays(b))
    return t


def _queries(scene):
    return [q[1] if isinstance(q, tuple) else _arrays(q) for q in scene.queries]


@pytest.mark.parametrize("scene", ks.score_scenes(), ids=lambda s: s.name)
def test_score_scene_equals_the_restatement(afv, gpu_ctx, scene):
    t = _score_table(afv, gpu_ctx, scene)
    queries = _queries(scene)
    nq = len(queries)
    rows = sorted(set(range(min(nq, 8))) | {nq - 1, nq // 2} | set(range(3, nq, 37)))      # the sample of rows asked one by one
    for m in (None, scene.mask):
        got = t.score_bow(queries, m)
        _check(got, scene.want(mask=m))                    # common, score bits, first_common: every cell
        for r in rows:
            one = t.score_bow([queries[r]], m)
            _check([a[0] for a in one], [a[r] for a in got])
    common, score, _ = got
    assert (common[:, scene.mask == 0] == -1).all() and (score[:, scene.mask == 0] == 0).all()
    assert t.score_bow(queries[:2], None, want_first=False)[2] is None
    t.close()


def test_score_scene_with_a_frame_query(afv, gpu_ctx):
    """the query is the resident BowVector of a frame (k_bowvec_build's output read by k_score_bow in place): slots cut from the same
    vector at the chunk edges, next to the same query as host arrays"""
    S = {s.name: s for s in ks.bow_scenes()}
    scene = S["words_8192"]                                # 8192 entries: the query list fills the LDS
    voc = _voc(afv, gpu_ctx, scene.weight_key)
    fr = _frame(afv, gpu_ctx, ks.KIND, ks.descriptors_of(scene.leaves), cap=8192)
    fbow = scene.want()
    _same(_resident(afv, fr, voc, scene), fbow)
    words, rng = list(fbow.keys()), np.random.RandomState(5)
    slots = []
    for size in (1, 63, 64, 65, 129, 4096):               # 4096: the largest slot a table takes
        pick = sorted(rng.choice(len(words), size, replace=False).tolist())
        slots.append({words[i]: (fbow[words[i]] if k % 3 else float(rng.random_sample() * 2.0 ** -rng.randint(1, 20))) for k, i in enumerate(pick)})
    slots.append({w: fbow[w] for w in words[-4096:]})
    t = afv.table.DescriptorTable(gpu_ctx, len(slots), 4096)
    for s, b in enumerate(slots):
        t.set(s, np.full((1, 32), 0x5a, np.uint8))
        t.set_bowvec(s, *_arrays(b))
    got = t.score_bow([fr, _arrays(fbow)])
    want = [ref.l1_score(fbow, b) for b in slots]
    assert [w[0] for w in want] == [1, 63, 64, 65, 129, 4096, 4096] and want[-1][2] == words[-4096]
    for r in range(2):
        assert got[0][r].tolist() == [w[0] for w in want] and got[2][r].tolist() == [w[2] for w in want]
        assert got[1][r].tobytes() == np.array([w[1] for w in want], np.float64).tobytes()
    t.close(); fr.close()


# ---------------------------------------------------------------- (c) decision scenes ----------------------------------------------------------------
def _plain(answers):
    return [a if isinstance(a, list) else ("f32", np.float32(a).tobytes()) for a in answers]


def _decision_table(afv, ctx, scene):
    t = afv.table.DescriptorTable(ctx, scene.nsets, max(len(b) for b in scene.bows.values()))
    for s, b in scene.bows.items():
        t.set(s, np.full((1, 32), 0x5a, np.uint8))
        t.set_bowvec(s, *_arrays(b))
    return t


@pytest.mark.parametrize("scene", ks.decision_scenes(), ids=lambda s: s.name)
def test_decision_scene_on_the_python_mirror(afv, gpu_ctx, scene):
    t = _decision_table(afv, gpu_ctx, scene)
    got = ks.run_db(scene, afv.KeyFrameDatabase(t))
    assert all(isinstance(a, (list, np.float32)) for a in got)
    assert _plain(got) == _plain(ks.run_ref(scene))
    assert _plain(got) != _plain(ks.run_ref(scene, flip=scene.flip))     # ... and not the flipped rule's answer
    t.close()


def test_decision_scenes_through_the_cpp_adapter(afv, gpu_ctx, tmp_path):
    """afv::KeyFrameDatabase of adapter/afv_adapter.hpp: every scene as an operation script through the kfdb_selftest process"""
    assert os.path.exists(KFDB_BIN), "kfdb_selftest is not built: __graft_entry__.build() compiles it"
    for scene in ks.decision_scenes():
        inp = tmp_path / (scene.name + ".txt")
        inp.write_text(ks.script_text(scene))
        r = subprocess.run([KFDB_BIN, str(inp)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (scene.name, r.stderr)
        assert _plain(ks.parse_script_output(r.stdout)) == _plain(ks.run_ref(scene)), scene.name
