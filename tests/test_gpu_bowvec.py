"""-m gpu: the BowVector built on the device (k_bowvec.hip) against the plain-Python restatement of DBoW2 transform
(tests/_kfdb_ref.py): word ids and the bit pattern of every double, for resident frames (afv_frame_bow_transform + afv_frame_get_bowvec)
and for host leaves (afv_bow_vector)."""
import ctypes as C

import numpy as np
import pytest

import _bow_scenes as scenes
import _kfdb_ref as ref

pytestmark = pytest.mark.gpu


def _same(got, want):
    """(word int32[], value float64[]) == {word: value}: ids and double bits"""
    word, value = got
    assert word.dtype == np.int32 and value.dtype == np.float64
    assert word.tolist() == list(want.keys())
    assert value.tobytes() == np.array(list(want.values()), np.float64).tobytes()


def _frame(afv, ctx, kind, desc, cap=0):
    spec = scenes.KINDS[kind]
    fr = afv.Frame(ctx, float_dim=spec["float_dim"], cap=cap) if spec["float_dim"] else afv.Frame(ctx, desc_bytes=spec["desc_bytes"], cap=cap)
    kps = np.zeros(len(desc), afv.KP_DTYPE)
    kps["x"] = np.arange(len(desc)) % 600 + 10
    kps["y"] = np.arange(len(desc)) % 400 + 10
    fr.set_features(kps, desc)
    return fr


@pytest.mark.parametrize("kind", ["orb32", "akaze61", "sift128"])
def test_frame_bowvec_equals_the_restatement(afv, gpu_ctx, kind):
    s = scenes.scene(kind)
    voc = scenes.vocabulary(kind, gpu_ctx)
    for i in (0, 17, s.nkf - 1):
        fr = _frame(afv, gpu_ctx, kind, s.keyframes[i])
        leaf, _ = fr.bow_transform_nodes(voc)
        assert np.array_equal(leaf, s.leaves[i])          # the scene's CPU descent is the device's
        want = ref.bow_vector(leaf, voc.weight, voc.word_id)
        assert len(want) > 200
        _same(fr.bowvec(), want)
        _same(voc.bow_vector(leaf), want)                 # host leaves through afv_bow_vector
        # ... and the host containers of the merged code agree with both
        bow, _ = voc.vectors_from_nodes(leaf, np.zeros_like(leaf))
        assert list(bow.items()) == list(want.items())
        fr.close()
    voc.close()


def test_stopped_words_and_repeated_addition(afv, gpu_ctx):
    """the small default tree (216 words, some stopped): every word is hit many times, so a value is weight added count times (differs
    from count * weight from the 4th addition on); stopped words do not appear"""
    voc = afv.Vocabulary.random(3, ctx=gpu_ctx)
    desc = afv.synth.random_descriptors(9, 1500)
    fr = _frame(afv, gpu_ctx, "orb32", desc, cap=1500)
    leaf, _ = fr.bow_transform_nodes(voc)
    counts = np.bincount(voc.word_id[leaf[voc.weight[leaf] > 0]])
    assert counts.max() >= 5 and (~(voc.weight[leaf] > 0)).any()
    want = ref.bow_vector(leaf, voc.weight, voc.word_id)
    rep = {}
    for lf in leaf.tolist():
        if voc.weight[lf] > 0:
            rep[int(voc.word_id[lf])] = rep.get(int(voc.word_id[lf]), 0.0) + float(voc.weight[lf])
    by_word = {int(voc.word_id[lf]): float(voc.weight[lf]) for lf in set(leaf.tolist())}
    assert any(rep[k] != int(counts[k]) * by_word[k] for k in rep), "the scene does not tell repeated addition from count * weight"
    _same(fr.bowvec(), want)
    _same(voc.bow_vector(leaf), want)
    stopped_words = set(voc.word_id[(~(voc.weight > 0)) & voc.is_leaf].tolist())
    assert not stopped_words & set(fr.bowvec()[0].tolist())
    fr.close()
    voc.close()


def test_every_leaf_stopped_gives_an_empty_vector(afv, gpu_ctx):
    v0 = afv.Vocabulary.random(3)
    voc = afv.Vocabulary(v0.k, v0.L, _parents(v0), v0.node_desc, np.zeros_like(v0.weight), v0.is_leaf, gpu_ctx)
    desc = afv.synth.random_descriptors(4, 300)
    fr = _frame(afv, gpu_ctx, "orb32", desc)
    leaf, _ = fr.bow_transform_nodes(voc)
    word, value = fr.bowvec()
    assert len(word) == 0 and len(value) == 0             # n = 0: the norm is not > 0, nothing is divided
    word, value = voc.bow_vector(leaf)
    assert len(word) == 0
    assert ref.bow_vector(leaf, voc.weight, voc.word_id) == {}
    fr.close()
    voc.close()


def _parents(v):
    parent = np.zeros(len(v.weight), np.int32)
    for p in range(len(v.weight)):
        parent[v.child_idx[v.child_ptr[p]:v.child_ptr[p + 1]]] = p
    return parent


def test_vocabulary_without_weights_keeps_todays_behaviour(afv, gpu_ctx):
    lib = gpu_ctx.lib
    voc = afv.Vocabulary.random(3, ctx=gpu_ctx)
    h = voc._device()
    desc = afv.synth.random_descriptors(5, 400)
    fr = _frame(afv, gpu_ctx, "orb32", desc)
    leaf_w, nid_w = fr.bow_transform_nodes(voc)
    fv_w = fr.featvec()
    assert lib.afv_vocab_set_weights(gpu_ctx.handle, h, None, None) == 0      # weights removed
    leaf, nid = fr.bow_transform_nodes(voc)
    assert np.array_equal(leaf, leaf_w) and np.array_equal(nid, nid_w) and fr.featvec() == fv_w
    n = C.c_int32(-5)
    assert lib.afv_frame_get_bowvec(fr.handle, None, None, C.byref(n)) == afv._lib.EINVAL
    w = np.zeros(400, np.int32); v = np.zeros(400, np.float64)
    assert lib.afv_bow_vector(gpu_ctx.handle, h, leaf.ctypes.data, len(leaf), w.ctypes.data, v.ctypes.data, C.byref(n)) == afv._lib.EINVAL
    fr.close()
    voc.close()
