"""CPU: the oracle's BoW-guided matchers against the plain-Python restatement of the reference (tests/_bow_ref.py) on the constructed scenes
of tests/_match_scenes.py, and the proof that every scene reaches the branch it exists for: the equality counter of its rule is > 0 AND the
restatement with that one rule flipped gives another answer.  Without these checks tests/test_gpu_match_scenes.py could stay green without
testing anything.

The constants of the kernels the scenes are built to exceed (nothing is imported from the kernels):
  64 x 64        csrc/k_match.hip:357   a node up to this size is walked in registers (bow_segment_small), anything larger in the LDS-bitset form
  TOPK = 4       csrc/k_match.hip:483   keys per row of the top-4 phase of the brute-force path
  RKEYS = 7      csrc/k_match.hip:542   key slots of a resolve record: a row whose answer lies behind more taken columns rescans
  MT = 256       csrc/k_match.hip:25    rows per workgroup of k_match_tri
  4096           csrc/afv_api.hip:1417  largest side of the top-4 path;  AFV_MAX_SIDE = 8192 the largest side afv_match_bow accepts
"""
import numpy as np
import pytest

import _bow_ref as R
import _match_scenes as MS

TOPK, RKEYS, MT, SMALL = 4, 7, 256, 64
CASES = MS.all_constructed()
IDS = [c.name for c in CASES]
_REF = {}


def run_ref(c, flip=None):
    """(the unflipped answers are kept: several tests read the same traces)"""
    if flip is None and c.name in _REF:
        return _REF[c.name]
    r = MS.run_ref(c, flip)
    if flip is None:
        _REF[c.name] = r
    return r


def test_scene_names_are_unique():
    assert len(set(IDS)) == len(IDS)


def test_every_rule_is_named_by_a_scene():
    named = {c.rule for c in CASES if c.rule is not None}
    assert named == set(R.FLIPS), (sorted(set(R.FLIPS) - named), sorted(named - set(R.FLIPS)))
    # ... per descriptor kind, and in each of the three node shapes wherever a rule has more than one
    for desc in MS.DESCS:
        here = {c.rule for c in CASES if ("-%s-" % desc) in c.name}
        assert set(R.FLIPS) <= here, (desc, sorted(set(R.FLIPS) - here))
    for rule in R.FLIPS:
        shapes = {c.name.rsplit("-", 1)[1] for c in CASES if c.rule == rule}
        assert shapes >= ({"small", "large"} if rule == "merge_lower_bound" else set(MS.SHAPES)), (rule, shapes)


def test_only_the_side_scenes_skip_the_restatement():
    for c in CASES:
        if c.name.startswith("side-"):
            assert c.rule is None
        else:
            assert max(c.K1.N, c.K2.N) <= 2100, c.name   # what the Python loops walk in reasonable time


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_oracle_equals_restatement_and_the_scene_reaches_its_rule(oracle, c):
    want, wn = MS.run_oracle(oracle, c)
    assert len(want) == (c.K2.N if c.kind == "kff" else c.K1.N)
    if c.name.startswith("side-"):
        assert wn > 10, "the largest scenes go to the oracle alone; they must at least match something"
        return
    got, n, tr = run_ref(c)
    assert n == wn and np.array_equal(got, want)
    if c.rule is None:
        return
    assert tr["eq"][c.rule] > 0, "the scene never meets its rule"
    flipped, fn, _ = run_ref(c, flip=c.rule)
    assert not (np.array_equal(flipped, got) and fn == n), "the outcome does not depend on the rule: the scene proves nothing"


def _named(prefix):
    return [c for c in CASES if c.name.startswith(prefix)]


def test_the_every_route_scene_needs_its_masks_and_its_histogram(oracle):
    """MS.every_route_scene: the oracle equals the restatement under both rules, and the answer changes when the masks or the
    orientation check are taken away - so a route that drops either one shows"""
    kfkf, kff, _ = MS.every_route_scene()
    for c in (kfkf, kff):
        want, n = MS.run_oracle(oracle, c)
        got, gn = MS.run_ref(c)[:2]
        assert n == gn and np.array_equal(want, got) and n > 30
        assert MS.run_oracle(oracle, c._replace(kw=dict(c.kw, check_orientation=False)))[1] > n
        bare = [MS.afv.FeatureView(K.descriptors, K.featvec, None, K.angles) for K in (c.K1, c.K2)]
        assert MS.run_oracle(oracle, c._replace(K1=bare[0], K2=bare[1]))[1] > n
    assert not np.array_equal(MS.run_oracle(oracle, kfkf)[0][:65], MS.run_oracle(oracle, kff)[0])


def test_node_shapes_land_where_they_are_meant_to():
    for c in CASES:
        if c.rule is None or c.kind == "tri":
            continue
        tr = run_ref(c)[2]
        shape = c.name.rsplit("-", 1)[1]
        if shape == "single":
            assert tr["shared_nodes"] == 1, c.name
        elif shape == "small":
            assert tr["shared_nodes"] > 1 and max(tr["max_node"]) <= SMALL, (c.name, tr["max_node"])
        else:
            assert tr["shared_nodes"] > 1 and min(tr["max_node"]) > SMALL, (c.name, tr["max_node"])


def test_structural_traces():
    for c in _named("chain-"):
        got, n, tr = run_ref(c)
        assert tr["longest_chain"] >= 200, (c.name, tr["longest_chain"])
        assert n == c.K1.N - (0 if "single" in c.name else MS.NFILL + 6)   # every row of the scene matches, no filler row does
        assert run_ref(c, flip="taken")[1] < 3   # without the flags nearly nothing matches: the whole answer hangs on them
    for c in _named("behind-"):
        got, n, tr = run_ref(c)
        b = tr["behind"]
        assert int((b > TOPK).sum()) >= 60 and int((b > RKEYS).sum()) >= 60 and int(b.max()) >= 73, c.name
        assert tr["starved"] + (c.K1.N - tr["accepted"]) > 0
        assert n == (76 if c.kind == "kff" else 75)   # th_low = 75: (KF, F) accepts the column at 75, (KF, KF) does not
    for c in _named("merge-"):
        tr = run_ref(c)[2]
        assert tr["jumps"] >= 5 and tr["empty_nodes"] == 2 and tr["shared_nodes"] == 5, c.name
    sizes = {}
    for c in _named("node6") + _named("bits"):
        tr = run_ref(c)[2]
        sizes[c.name] = tr["max_node"]
    for m1 in (63, 64, 65):
        for m2 in (63, 64, 65):
            assert sizes["node%dx%d-b32-kfkf" % (m1, m2)] == (m1, m2)
    for n2 in (31, 32, 33, 2047, 2048, 2049):
        assert sizes["bits%d-b32-kff" % n2][1] == n2 - 6
    for c in _named("tri-n"):
        got, n, tr = run_ref(c)
        assert tr["rows_outside_shared_nodes"] >= c.K1.N // 5 and n > 20, c.name
        assert {c.K1.N for c in _named("tri-n")} == {MT - 1, MT, MT + 1}


def test_the_largest_sides_lie_on_both_sides_of_the_limits():
    n = {(c.K1.N, c.K2.N) for c in _named("side-")}
    assert (4096, 4096) in n and (4097, 300) in n and (300, 4097) in n and (8192, 500) in n and (500, 8192) in n and (8192, 8192) in n
    (a, _), (_, b) = MS.too_large()
    assert a.N == 8193 and b.N == 8193


def _same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(np.asarray(a), np.asarray(b)))


def test_generators_are_deterministic():
    again = MS.all_constructed()
    assert [c.name for c in again] == IDS
    for a, b in zip(CASES, again):
        assert a.kind == b.kind and a.rule == b.rule and sorted(a.kw) == sorted(b.kw)
        assert all(_same(a.kw[k], b.kw[k]) for k in a.kw)
        for o1, o2 in ((a.K1, b.K1), (a.K2, b.K2)):
            assert o1.featvec == o2.featvec
            for k in ("descriptors", "valid", "angles", "pts", "sigma2", "u_right"):
                assert _same(getattr(o1, k), getattr(o2, k)), (a.name, k)
    b1, b2 = MS.batches(CASES), MS.batches(again)
    assert list(b1) == list(b2) and all([c.name for c in b1[k]] == [c.name for c in b2[k]] for k in b1)


def test_batches_have_the_sizes_and_the_mixtures_asked_for():
    B = MS.batches(CASES)
    assert sorted({len(v) for k, v in B.items() if not k.startswith("tri-")}) == [2, 7, 8, 33]
    assert [len(B[k]) for k in ("tri-two", "tri-seven", "tri-thirty-three")] == [2, 7, 33]
    eligible = lambda c: (c.kind == "kfkf" and c.K1.featvec is None and c.K1.descriptors.dtype == np.uint8 and c.K1.descriptors.shape[1] == 32
                          and c.K1.valid is None and c.K2.valid is None and max(c.K1.N, c.K2.N) <= 4096)
    assert all(eligible(c) for c in B["fast-path-settings"])
    assert len({(c.kw["th_low"], c.kw["nnratio"], c.kw["check_orientation"]) for c in B["fast-path-settings"]}) >= 4
    assert sum(not eligible(c) for c in B["fast-path-but-one"]) == 1
    for k in ("seven-mixed", "thirty-three"):
        kinds = {c.kind for c in B[k]}
        widths = {(c.K1.descriptors.dtype.kind, c.K1.descriptors.shape[1]) for c in B[k]}
        # shared nodes of a job: 0, 1 (no FeatureVector counts as one) or many
        nodes = {1 if c.K1.featvec is None or c.K2.featvec is None else min(len({i for i, _ in c.K1.featvec} & {i for i, _ in c.K2.featvec}), 2)
                 for c in B[k]}
        assert kinds == {"kfkf", "kff"}, k
        assert len(widths) >= 3 and (("f", 8) in widths or ("f", 64) in widths) and {("u", 32), ("u", 61)} <= widths, (k, widths)
        assert nodes == {0, 1, 2}, (k, nodes)


def _vocab_pair(afv, oracle, seed):
    """oracle-extracted descriptors with Vocabulary FeatureVectors, as tests/test_gpu_bow.py::test_extract_transform_match_chain builds them"""
    s = afv.synth
    voc = afv.Vocabulary.random(4 + seed, k=8, L=3)
    sides = []
    for im in (s.corners_frame(10 + seed), np.roll(s.corners_frame(10 + seed), 3 + seed % 3, axis=1)):
        kps, desc = oracle.orb_extract(im)
        _, nid = oracle.bow_transform(voc, desc, 2)
        fv = [(int(k), np.nonzero(nid == k)[0].tolist()) for k in np.unique(nid)]
        sides.append((kps, desc, fv))
    return sides


@pytest.mark.parametrize("seed", [0, 1, 2, 5])
def test_random_scenes_with_vocabulary_featvecs(afv, oracle, seed):
    (k1, d1, fv1), (k2, d2, fv2) = _vocab_pair(afv, oracle, seed)
    v1 = (afv.synth.lcg_bytes(seed + 60, len(d1)) > 30).astype(np.uint8); v2 = (afv.synth.lcg_bytes(seed + 61, len(d2)) > 30).astype(np.uint8)
    want, wn = oracle.search_by_bow_kf_kf(d1, d2, fv1, fv2, v1, v2, k1["angle"], k2["angle"], 75.0, 0.75, True)
    got, n, _ = R.search_by_bow_kf_kf(d1, d2, fv1, fv2, v1, v2, k1["angle"], k2["angle"], 75.0, 0.75, True)
    assert n == wn and np.array_equal(got, want) and wn > 50
    want, wn = oracle.search_by_bow_kf_frame(d1, d2, fv1, fv2, v1, k1["angle"], k2["angle"], 75.0, 0.75, True)
    got, n, _ = R.search_by_bow_kf_frame(d1, d2, fv1, fv2, v1, k1["angle"], k2["angle"], 75.0, 0.75, True)
    assert n == wn and np.array_equal(got, want) and wn > 50
    p1 = np.stack([k1["x"], k1["y"]], 1); p2 = np.stack([k2["x"], k2["y"]], 1)
    s2 = oracle.size_sigma(k2)[1]
    F12 = np.array([0, 0, 0, 0, 0, -1, 0, 1, 0], np.float32)   # a pure shift along x: the epipolar line of (x, y) is y
    mp1 = 1 - v1; mp2 = 1 - v2
    want, wn = oracle.search_for_triangulation(d1, d2, p1, p2, s2, F12, (9000.0, 240.0), fv1, fv2, mp1, mp2, 75.0)
    got, n, _ = R.search_for_triangulation(d1, d2, p1, p2, s2, F12, (9000.0, 240.0), fv1, fv2, mp1, mp2, 75.0)
    assert n == wn and np.array_equal(got, want) and wn > 50


def test_a_feature_listed_twice_is_refused_before_the_library_is_called(afv):
    """FeatureView.csr: the Python layer names the feature; the library's own check (validate_job, afv_table_set_featvec,
    afv_table_match_bow_frame) needs a context, hence a device: tests/test_gpu_match_scenes.py"""
    d = np.zeros((6, 32), np.uint8)
    for fv in ([(1, [0, 1]), (5, [1, 2])], [(1, [3, 3])], [(1, [0]), (2, []), (9, [4, 5, 0])]):
        with pytest.raises(afv._lib.AfvError) as e:
            afv.FeatureView(d, fv).csr()
        assert e.value.code == afv._lib.EINVAL
    ids, ptrs, flat, nn = afv.FeatureView(d, [(1, [5, 0]), (2, []), (9, [4, 3])]).csr()   # a feature may be missing; none may repeat
    assert nn == 3 and flat.tolist() == [5, 0, 4, 3] and ptrs.tolist() == [0, 2, 2, 4]
