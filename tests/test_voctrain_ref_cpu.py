"""CPU: the plain-Python restatement of DBoW2's Vocabulary::create (tests/_voctrain_ref.py) on the constructed scenes of
tests/_voctrain_scenes.py: the proof that every scene reaches the rule it exists for (read from the restatement's trace), and the
properties any trained tree has.  Without these checks tests/test_gpu_voctrain.py could stay green without testing anything."""
import numpy as np
import pytest

import _voctrain_ref as R
import _voctrain_scenes as S

CASES = S.all_constructed()


def training_leaf(trace, out):
    """feature -> the node its training clusters end in (the child of the deepest node record that holds it)"""
    leaf = {}
    for rec in sorted(trace["nodes"], key=lambda r: r["level"]):
        for c, g in enumerate(rec["groups"]):
            for f in g:
                leaf[f] = rec["children"][c]
    return leaf


def test_splitmix_known_values():
    # splitmix64 from state 0: the first outputs of the published generator
    assert R.sm(0) == 0xE220A8397B1DCDAF
    assert R.sm(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


def test_mean_value_rule():
    rows = [0b0001, 0b0011, 0b0111, 0b1111]
    sp = [R.spread(r, 1) for r in rows]
    assert R.mean_value([0, 1, 2, 3], sp, rows, 1) == 0b0111       # N = 4: a bit needs 2 of 4; bit 2 has exactly N / 2
    assert R.mean_value([0, 1, 2], sp, rows, 1) == 0b0011          # N = 3: needs 2; bit 1 has exactly 2 = (N + 1) / 2, bit 2 has 1 = (N - 1) / 2
    assert R.mean_value([3], sp, rows, 1) == 0b1111                # one member: a copy


@pytest.mark.parametrize("sc", CASES, ids=repr)
def test_tree_properties(sc):
    out, trace = S.ref(sc)
    parent, leaf, n = out["parent"], out["is_leaf"], len(out["parent"])
    # node ids are a pre-order with consecutive sibling ids: a node's children are consecutive, created right after ... the recursion of
    # its earlier siblings; every child's id is above its parent's; the subtree of a node is an id interval
    for i in range(n):
        ch = out["children"][i]
        assert ch == list(range(ch[0], ch[0] + len(ch))) if ch else True
        assert all(c > i for c in ch)
    for rec in trace["nodes"]:
        ch = rec["children"]
        for a, b in zip(ch, ch[1:]):          # everything below child a is numbered before the children of child b
            below_a = [x for x in range(n) if x != a and _has_ancestor(parent, x, a)]
            kids_b = out["children"][b]
            assert not below_a or not kids_b or max(below_a) < min(kids_b)
    # word ids ascend with node ids (createWords) - the Vocabulary numbers the leaves in node order
    words = [i for i in range(n) if leaf[i]]
    assert words == sorted(words) and not leaf[0]
    # non-trivial nodes: the association is a fixed point unless capped, and every centre is the majority of its final group
    rows = [int.from_bytes(bytes(bytearray(r)), "little") for im in sc.images for r in im]
    sp = [R.spread(r, sc.desc_bytes) for r in rows]
    for rec in trace["nodes"]:
        if rec["trivial"]:
            assert rec["rounds"] == 0 and all(len(g) == 1 for g in rec["groups"])
            continue
        feats = sorted(f for g in rec["groups"] for f in g)
        assoc, groups = R.associate(feats, rows, rec["centres"])
        assert groups == rec["groups"]                               # the centres reproduce the recorded association
        assert all(g == sorted(g) for g in groups)                   # groups keep ascending feature order
        if not rec["capped"]:
            assert rec["rounds"] >= 2
            for c, g in enumerate(groups):
                if g:
                    assert R.mean_value(g, sp, rows, sc.desc_bytes) == rec["centres"][c]
    # depth: no node below level L; weights: log(N / Ni) where Ni > 0, else 0.0
    for i in range(1, n):
        d, x = 0, i
        while x:
            x, d = parent[x], d + 1
        assert d <= sc.L
    assert all(out["ni"][i] == -1 for i in range(n) if not leaf[i])
    assert sum(1 for w in set(out["leaf_of"])) <= len(words)


def _has_ancestor(parent, x, a):
    while x:
        x = parent[x]
        if x == a:
            return True
    return False


def test_scenes_reach_their_rules():
    t = {sc.name: S.ref(sc) for sc in CASES}
    # segment edges / shapes: non-trivial training at every level asked for
    for n in (63, 64, 65, 1025, 4097):
        out, tr = t["edge_n%d" % n]
        assert tr["nodes"][0]["n"] == n and not tr["nodes"][0]["trivial"] and out["rounds"][0] >= 2
    out, tr = t["deep_multi_tile"]
    assert sum(1 for r in tr["nodes"] if r["level"] == 2 and r["n"] > 4096) == 2
    for name in ("trivial_n_eq_k", "trivial_n_eq_k_plus_1", "trivial_n_1"):
        out, tr = t[name]
        assert tr["trivial"] >= 1
    assert t["trivial_n_eq_k"][1]["nodes"][0]["trivial"] and t["trivial_n_1"][1]["nodes"][0]["trivial"]
    assert not t["trivial_n_eq_k_plus_1"][1]["nodes"][0]["trivial"]
    assert len(t["trivial_n_1"][0]["parent"]) == 2
    # unbalanced: child 1 of the root is a leaf, child 2 has grandchildren; depth-first: the ids below child 2 follow it directly
    out, tr = t["unbalanced"]
    assert out["children"][0] == [1, 2, 3] and out["is_leaf"][1] and out["children"][2] == [4, 5, 6]
    assert any(out["children"][c] for c in out["children"][2])       # two more levels below the later child
    assert out["children"][3] and min(out["children"][3]) > max(max(out["children"][c], default=0) for c in out["children"][2])
    level_order = sorted(range(len(out["parent"])), key=lambda i: (_depth(out["parent"], i), i))
    assert level_order != list(range(len(out["parent"])))            # the ids are NOT the level order
    # duplicates: seeding stopped short; three words, each in every image with rows: weight exactly 0.0; empty images count in N
    out, tr = t["duplicates"]
    assert tr["seed_short"] >= 1 and len(out["children"][0]) == 3
    assert [out["weight"][i] for i in range(len(out["parent"])) if out["is_leaf"][i]] != []
    out, tr = t["weights"]
    w = [out["weight"][i] for i in range(len(out["parent"])) if out["is_leaf"][i] and out["ni"][i] > 0]
    assert any(x > 0 for x in w)
    nimg = len(S.by_name("weights").images)
    assert any(len(im) == 0 for im in S.by_name("weights").images[:-1]) and len(S.by_name("weights").images[-1]) == 0
    assert all(out["weight"][i] == np.log(nimg / out["ni"][i]) for i in range(len(out["parent"])) if out["is_leaf"][i] and out["ni"][i] > 0)
    # a word present in every image is a stopped word - only with images that are all non-empty
    out, tr = t["descent_differs"]
    tl = training_leaf(tr, out)
    assert any(out["leaf_of"][f] != tl[f] for f in tl) and any(out["ni"][i] == 0 for i in range(len(out["parent"])) if out["is_leaf"][i])
    assert any(out["weight"][i] == 0.0 and out["ni"][i] == 2 for i in range(len(out["parent"])) if out["is_leaf"][i])   # in both images
    # ties
    assert {(0, 0), (1, 1), (1, -1)} <= t["majority_ties"][1]["majority_edge"]
    assert t["association_ties"][1]["assoc_tie"] > 0
    assert t["seed_cut_boundary"][1]["cut_on_boundary"] > 0 and t["seed_cut_is_sum"][1]["cut_is_sum"] > 0
    # the kept-centre rule
    out, tr = t["empty_cluster"]
    sc = S.by_name("empty_cluster")
    assert tr["empty_cluster"] > 0 and out["ni"][2] == 0 and out["weight"][2] == 0.0 and out["desc"][2] == bytes(bytearray(sc.init_centres[1]))
    # the cap
    out, tr = t["max_iters_1"]
    assert out["capped"] and out["rounds"] == [1, 1]
    sc = S.by_name("max_iters_1")
    free = R.train(sc.images, sc.desc_bytes, sc.k, sc.L, sc.seed, 0)
    assert not free["capped"] and free["rounds"][0] > 1 and free["desc"] != out["desc"]
    for name, (out, tr) in t.items():
        if name != "max_iters_1":
            assert not out["capped"], name


def _depth(parent, i):
    d = 0
    while i:
        i, d = parent[i], d + 1
    return d


def test_duplicates_are_stopped_words():
    out, _ = S.ref(S.by_name("duplicates"))
    sc = S.by_name("duplicates")
    nonempty = sum(1 for im in sc.images if len(im))
    words = [i for i in range(len(out["parent"])) if out["is_leaf"][i]]
    # every word is in every image that has rows - with the empty images counted in N the weight is log(9 / 6), NOT 0: the stopped word needs
    # a scene without empty images, which the same rows give
    assert all(out["ni"][i] == nonempty for i in words)
    full = R.train([im for im in sc.images if len(im)], sc.desc_bytes, sc.k, sc.L, sc.seed)
    assert all(full["weight"][i] == 0.0 and full["ni"][i] == nonempty for i in range(len(full["parent"])) if full["is_leaf"][i])


def test_text_file_round_trip(afv, tmp_path):
    """saveToTextFile -> loadFromTextFile of a trained tree (the Vocabulary class of the package on the restatement's arrays)"""
    sc = S.by_name("shape_k3_L2_b61")
    out, _ = S.ref(sc)
    desc = np.frombuffer(b"".join(out["desc"]), np.uint8).reshape(-1, sc.desc_bytes)
    v = afv.Vocabulary(sc.k, sc.L, out["parent"], desc, out["weight"], out["is_leaf"])
    path = str(tmp_path / "voc.txt")
    v.saveToTextFile(path)
    w = afv.Vocabulary.loadFromTextFile(path)
    assert (w.k, w.L) == (v.k, v.L)
    assert np.array_equal(w.child_ptr, v.child_ptr) and np.array_equal(w.child_idx, v.child_idx)
    assert np.array_equal(w.node_desc[1:], v.node_desc[1:]) and np.array_equal(w.is_leaf, v.is_leaf)
    assert w.weight.tobytes() == v.weight.tobytes() and np.array_equal(w.word_id, v.word_id)


def test_create_is_bound(afv):
    """the feature's public surface exists (fails on a tree without afv_vocab_train)"""
    assert callable(afv.Vocabulary.create)
    assert "afv_vocab_train" in afv._lib.SYMBOLS and "afv_vocab_train_device" in afv._lib.SYMBOLS
    lib = afv._lib.load()
    import ctypes as C
    out = C.c_void_p(1)
    assert lib.afv_vocab_train(None, None, None, 0, None, 0, C.byref(out)) == afv._lib.EINVAL and not out.value
    assert lib.afv_vocab_tree_nnodes(None) == afv._lib.EINVAL
    lib.afv_vocab_tree_destroy(None)
