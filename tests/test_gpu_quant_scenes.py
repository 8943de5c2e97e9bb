"""-m gpu: BoW quantisation on the device - k_bow_transform<8|16>, k_bow_transform_f32<64|128|256>, k_featvec_build and the tree image
with its per-depth ranks - against the plain restatement tests/_quant_ref.py on the constructed scenes of tests/_quant_scenes.py.  Every
assertion is an equality; no feature, scene or kind is left out of a comparison.  tests/test_quant_ref_cpu.py proves on the CPU that
every scene reaches the rule it was built for.  Nothing here needs the oracle."""
import numpy as np
import pytest

import _quant_scenes as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vocab(afv, gpu_ctx):
    """the device vocabulary of a scene's tree, built once per tree"""
    made = {}

    def get(tree):
        if tree.name not in made:
            made[tree.name] = afv.Vocabulary(tree.k, tree.L, tree.parent, tree.node_desc, tree.weight, tree.is_leaf, ctx=gpu_ctx)
        return made[tree.name]
    yield get
    for v in made.values():
        v.close()


def _frame(afv, ctx, kind, cap):
    if S.is_float(kind):
        return afv.Frame(ctx, cap=cap, float_dim=S.WIDTH[kind])
    return afv.Frame(ctx, cap=cap, desc_bytes=S.WIDTH[kind])


def _hold(afv, fr, voc, sc):
    """host-array descent, resident descent, FeatureVector and BowVector of the scene are the restatement's"""
    leaf, nid, _, fv, bow = S.ref(sc)
    hleaf, hnid = voc.transform_nodes(sc.features, sc.levelsup)
    assert np.array_equal(hleaf, leaf) and np.array_equal(hnid, nid), (sc, "transform_nodes", np.flatnonzero((hleaf != leaf) | (hnid != nid))[:8])
    fr.set_features(np.zeros(sc.n, afv.KP_DTYPE), sc.features)
    fleaf, fnid = fr.bow_transform_nodes(voc, sc.levelsup)
    assert fr.N == sc.n and np.array_equal(fleaf, leaf) and np.array_equal(fnid, nid), (sc, "bow_transform_nodes")
    got = fr.featvec()
    assert got == fv, (sc, "featvec", [n for n, _ in got][:8], [n for n, _ in fv][:8])
    word, value = fr.bowvec()
    assert word.tolist() == list(bow.keys()) and value.tobytes() == np.array(list(bow.values()), np.float64).tobytes(), (sc, "bowvec")


@pytest.mark.parametrize("kind", S.KINDS)
def test_descent_scenes(afv, gpu_ctx, vocab, kind):
    """chunk edges (nodes of 1 .. 49 children, winners on lane 0 / 15 / the last child), ties across chunks, the float summation order, and
    ragged renumbered trees (levelsup 0, 1, L - 1, L, L + 3; n = 0 .. 65; the rows of a wavefront at four depths) through one small frame"""
    fr = _frame(afv, gpu_ctx, kind, 80)
    try:
        for sc in S.descent_scenes(kind):
            _hold(afv, fr, vocab(sc.tree), sc)
    finally:
        fr.close()


@pytest.mark.parametrize("kind,name", [(k, n) for k in S.KINDS for n in S.regime_names(k)])
def test_featvec_regimes(afv, gpu_ctx, vocab, kind, name):
    """the counting sort of k_featvec_build over one, two and three chunks of 1024 features, keys that fill a wavefront, many repeated keys
    in a wavefront, a key of the second chunk only, 0 % / 50 % / 100 % stopped words, widths 1, 17, 257, 4096 and - ranked by comparison -
    4097, on trees whose ids are a seeded permutation"""
    (sc,) = S.regime_scenes(kind, only=name)
    fr = _frame(afv, gpu_ctx, kind, sc.cap)
    try:
        _hold(afv, fr, vocab(sc.tree), sc)
    finally:
        fr.close()


@pytest.mark.parametrize("kind", S.KINDS)
def test_small_frame_after_a_large_one(afv, gpu_ctx, vocab, kind):
    """the same resident frame takes a 3000-feature scene, then scenes of 65 and fewer features on other trees, then a quadratic one: stale
    tails of the sorted body, of the per-feature keys and of the LDS tables must not show"""
    large = S.regime_scenes(kind, only="waves40_half")[0]
    small = [s for s in S.ragged_scenes(kind) if s.name.endswith(("perm_%s_up1_n65" % kind, "perm_%s_up0_n5" % kind, "dfs_%s_up4_n63" % kind))]
    assert len(small) == 3
    fr = _frame(afv, gpu_ctx, kind, S.FRAME_CAP)
    try:
        for sc in [large] + small + [S.tie_scene(kind), S.regime_scenes(kind, only="quad_n1023")[0], small[0], large]:
            _hold(afv, fr, vocab(sc.tree), sc)
    finally:
        fr.close()


def _csr(fv):
    ids = np.array([k for k, _ in fv], np.int32)
    ptr = np.zeros(len(fv) + 1, np.int32)
    ptr[1:] = np.cumsum([len(v) for _, v in fv])
    return ids, ptr, np.array([x for _, v in fv for x in v], np.int32)


@pytest.mark.parametrize("kind", S.KINDS)
def test_promoted_frame_equals_a_slot_filled_from_the_restatement(afv, gpu_ctx, vocab, kind):
    """table.set_from_frame of a frame quantised on the renumbered ragged tree, against a slot filled with set + set_featvec from the
    restatement's FeatureVector: match_bow against a second keyframe gives the same match vectors and counts"""
    a, b = S.table_scenes(kind)
    T = afv.table.DescriptorTable
    table = T(gpu_ctx, 3, 80, float_dim=S.WIDTH[kind]) if S.is_float(kind) else T(gpu_ctx, 3, 80, desc_bytes=S.WIDTH[kind])
    fr = _frame(afv, gpu_ctx, kind, 80)
    try:
        voc = vocab(a.tree)
        _hold(afv, fr, voc, a)
        table.set_from_frame(0, fr)
        table.set(1, a.features)
        table.set_featvec(1, *_csr(S.ref(a)[3]))
        table.set(2, b.features)
        table.set_featvec(2, *_csr(S.ref(b)[3]))
        th = 1.0 if S.is_float(kind) else 40.0
        for ori in (False, True):
            m, nm = table.match_bow(np.array([0, 1, 2, 2], np.int32), np.array([2, 2, 0, 1], np.int32), th, 0.9, ori)
            assert nm[0] == nm[1] and np.array_equal(m[0, :a.n], m[1, :a.n]), (kind, ori)
            assert nm[2] == nm[3] and np.array_equal(m[2, :b.n], m[3, :b.n]), (kind, ori)
            assert nm[0] > 0 and nm[2] > 0, (kind, nm)                   # (the second keyframe holds the first one's descriptors: there is something to match)
    finally:
        fr.close()
        table.close()


def test_lds_refusal_is_out_of_reach(afv, gpu_ctx, vocab):
    """afv_frame_bow_transform refuses a node level whose tables do not fit the LDS of one workgroup.  Through the public API that refusal
    cannot be reached for a width <= 4096: a frame takes at most 8192 features (a larger cap is AFV_EINVAL), and at cap 8192 and width 4096
    the kernel asks for 16 400 + 16 384 + 65 536 + 16 = 98 336 bytes of the 152 576 a launch may use; wider levels rank by comparison in
    4 * cap + 16 bytes.  This holds where the context could raise the kernels' dynamic LDS limit (afv_frame_prepare: hipFuncSetAttribute
    succeeds, as it does on an MI355X); with its 63 KB fallback the refusal would be reachable.  So nothing is forced here: the largest
    accepted frame quantises the widest counting-sort level correctly."""
    with pytest.raises(afv._lib.AfvError) as e:
        afv.Frame(gpu_ctx, cap=8193)
    assert e.value.code == afv._lib.EINVAL
    sc = S.regime_scenes("b32", only="own_node_n3000")[0]
    fr = afv.Frame(gpu_ctx, cap=8192)
    try:
        _hold(afv, fr, vocab(sc.tree), sc)
    finally:
        fr.close()
