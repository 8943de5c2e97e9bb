"""the scenes of tests/_scenes.py reach the branches they exist for (CPU, the oracle's trace): without these checks a change to a generator
or to the oracle could leave tests/test_gpu_extract_scenes.py green without testing anything"""
import numpy as np
import pytest

import _scenes as S

SEL_EXACT = 1024                       # k_select.hip: keys of the threshold bin the exact ranking of the 1024-thread kernel takes
KEPT_LDS = {256: 2304, 1024: 3072}     # k_select.hip SelCfg<ST>::KEPT_LDS: survivors the quadtree keeps in LDS


def float_key(r):
    """k_select.hip float_key: the order-preserving integer image of a float"""
    u = np.asarray(r, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _level(tr, l=0):
    m = tr["cand"]["level"] == l
    return tr["cand"][m], tr["keep1"][m], tr["keep2"][m]


def test_quotas_match_the_scene_constants(oracle):
    assert int(oracle.quotas_cvorb(10000)[0]) == S.CV_QUOTA0


@pytest.mark.parametrize("sign", ["+", "-"])
@pytest.mark.parametrize("n_bin", [1024, 1025])
def test_threshold_bin_scene(oracle, sign, n_bin):
    img, centres, tags = S.threshold_bin(sign, n_bin)
    assert img.shape == (S.H, S.W)
    _, _, tr = oracle.orb_extract_trace(img)
    c, k1, k2 = _level(tr)
    k = S.CV_QUOTA0
    # every copy is a candidate, nothing else is one, and retainBest #1 (2k on the FAST score) cuts nothing
    assert sorted(zip(c["x"].tolist(), c["y"].tolist())) == sorted(map(tuple, centres.tolist()))
    assert len(c) <= 2 * k and k1.all()
    n1 = len(c)
    assert n1 > k
    keys = float_key(c["response"])
    desc = np.sort(keys)[::-1]
    T = desc[k - 1]
    b = int(T) >> 20
    in_bin = keys >> 20 == b
    assert int(in_bin.sum()) == n_bin
    assert (b >= 2048) == (sign == "+") and np.all((c["response"][in_bin] > 0) == (sign == "+"))
    above = int((keys >> 20 > b).sum())
    kk = k - above
    assert 1 < kk < n_bin
    # the kk-th key of the bin is strictly inside a group of equal keys (ties on both sides of the threshold)
    g, ge = int((keys > T).sum()), int((keys >= T).sum())
    assert g < k - 1 and k < ge
    assert len(np.unique(keys[in_bin])) == 3
    # retainBest keeps the ties: more survivors than the quota; the low tier (its own region) is cut entirely
    assert k2.sum() == ge > k
    pos = {(int(x), int(y)): t for (x, y), t in zip(centres.tolist(), tags.tolist())}
    low = np.array([pos[(int(x), int(y))] == 4 for x, y in zip(c["x"], c["y"])])
    assert low.sum() == 400 and not k2[low].any() and int(keys[low].max()) >> 20 < b
    # in the exact branch iff n_bin <= SEL_EXACT: both sides of the edge are covered by the parametrisation
    assert (n_bin <= SEL_EXACT) == (n_bin == 1024)


@pytest.mark.parametrize("sign", ["+", "-"])
def test_tie_flood_scene(oracle, sign):
    img, centres, tags = S.tie_flood(sign)
    _, _, tr = oracle.orb_extract_trace(img)
    c, k1, k2 = _level(tr)
    assert len(c) == len(centres) and k1.all()
    keys = float_key(c["response"])
    assert np.all((c["response"] > 0) == (sign == "+"))
    top = keys == keys.max()
    assert top.sum() == 3200
    # every copy of the top motif survives retainBest #2: more survivors than LDS holds at either thread count
    assert k2.sum() == 3200 and k2[top].all() and not k2[~top].any()
    assert k2.sum() > max(KEPT_LDS.values())
    # and the quadtree selects among exactly equal responses only
    assert tr["t_counts"][0] >= 217
    sel_resp = {float(r) for r in c["response"][k2]}
    assert len(sel_resp) == 1


def test_score_threshold_ties_scene(oracle):
    img, centres, _ = S.score_threshold_ties()
    _, _, tr = oracle.orb_extract_trace(img)
    c, k1, k2 = _level(tr)
    k2n = 2 * S.CV_QUOTA0
    assert len(c) == len(centres) == 5400 > k2n
    s = np.sort(c["fast_score"])[::-1]
    T = s[k2n - 1]
    assert T == 139 and (s > T).sum() < k2n - 1 and k2n < (s >= T).sum()
    # ties kept: more than 2k survive retainBest #1, the low tier does not
    assert k1.sum() == 4800 > k2n and not k1[c["fast_score"] < T].any()
    assert k2.sum() == 3000


@pytest.mark.parametrize("t", [1, 7, 20, 30, 254])
def test_fast_edges_scene(oracle, t):
    img, motifs = S.fast_edges(t)
    _, _, tr = oracle.orb_extract_trace(img, oracle.default_params(1000, 8, 1.2, t))
    c, _, _ = _level(tr)
    cand = {(int(x), int(y)) for x, y in zip(c["x"], c["y"])}
    score = oracle.fast_score_map(img, t)
    kinds = {"corner": 0, "flat": 0, "tie": 0}
    for x, y, kind in motifs:
        kinds[kind] += 1
        if kind == "corner":
            assert score[y, x] > 0 and (x, y) in cand, (x, y, t)
        elif kind == "flat":
            assert score[y, x] == 0 and (x, y) not in cand, (x, y, t)
        else:
            assert score[y, x] > 0 and (x, y) not in cand, (x, y, t)
    # both sides of the threshold, at both ends of the byte range
    assert kinds["corner"] >= 4 and kinds["flat"] >= 4
    if t < 200:
        assert kinds["tie"] == 4
    vs = {int(img[y, x]) for x, y, kind in motifs if kind == "corner"}
    assert min(vs) <= t and max(vs) >= 255 - t


def test_scenes_are_deterministic():
    a = S.threshold_bin("-", 1025)[0]
    assert np.array_equal(a, S.threshold_bin("-", 1025)[0])
    assert np.array_equal(S.fast_edges(7)[0], S.fast_edges(7)[0])
