"""Constructed vocabulary trees and descriptors for BoW quantisation (the descent kernels of csrc/k_bow.hip, k_featvec_build of
csrc/k_frame.hip and the tree image of csrc/afv_api.hip against tests/_quant_ref.py), built from the project's LCG (synth.lcg_*) alone.
Each scene names the rule it exists for; tests/test_quant_ref_cpu.py proves from the restatement's trace that the rule is reached,
tests/test_gpu_quant_scenes.py holds the device to equality on the same scenes.

Sizes the kernels care about (nothing is imported from them): the children of a node are taken 16 at a time (a 16-lane row per
descriptor, four descriptors per wavefront); the FeatureVector is placed in chunks of 1024 features, 64 per wavefront, by a counting sort
over 1 + (nodes of the level) keys while that is <= 4096 and by comparison beyond.

How a tree routes a descriptor: a node at depth d copies its parent's descriptor and replaces segment d (8 bytes, or dim / 4 floats) by
random data of its own.  The descriptor of a node, used as a query, then meets at every depth d one child that equals it in segment d
and siblings that differ there and nowhere else: it descends to that node.  This is how the scenes choose their keys; what the keys ARE is
always taken from the restatement, never assumed.
"""
import importlib

import numpy as np

import _quant_ref as R

KINDS = ("b32", "b61", "f64", "f128", "f256")
WIDTH = {"b32": 32, "b61": 61, "f64": 64, "f128": 128, "f256": 256}
N_SMALL = (0, 1, 2, 3, 5, 63, 64, 65)
N_LARGE = (1023, 1024, 1025, 2049, 3000)
CHUNK_COUNTS = (1, 15, 16, 17, 31, 32, 33, 48, 49)
TIE_CASES = ((3, 19), (15, 16), (0, 32), (17, 35), (5, 21, 37))
FRAME_CAP = 3000      # the largest frame of the issue


def _synth():
    return importlib.import_module("anyfeature-vslam_amd").synth


def is_float(kind):
    return kind[0] == "f"


def _rand(kind, seed, n, width):
    """n x width random descriptor elements: bytes, or floats in [0, 1) with 24 random mantissa bits"""
    s = _synth()
    if is_float(kind):
        return ((s.lcg_states(seed, n * width) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).reshape(n, width)
    return s.lcg_bytes(seed, n * width).reshape(n, width).copy()


def _seg(kind, depth):
    w = WIDTH[kind] // 4 if is_float(kind) else 8
    return slice(w * (depth - 1), w * depth)


class TreeData:
    """arrays in DBoW2 id order, what Vocabulary(k, L, parent, node_desc, weight, is_leaf) and R.Tree take"""

    def __init__(self, name, kind, k, L, parent, node_desc, weight, is_leaf):
        self.name, self.kind, self.k, self.L = name, kind, k, L
        self.parent, self.node_desc, self.weight, self.is_leaf = parent, node_desc, weight, is_leaf
        self._ref = None

    @property
    def ref(self):
        if self._ref is None:
            self._ref = R.Tree(self.k, self.L, self.parent, self.node_desc, self.weight, self.is_leaf)
        return self._ref

    def with_weights(self, tag, weight):
        return TreeData(self.name + "/" + tag, self.kind, self.k, self.L, self.parent, self.node_desc, weight, self.is_leaf)


def _shape(counts_of):
    """abstract tree in breadth-first order: counts_of(node, depth, first_child) -> number of children; returns (parent, depth)"""
    parent, depth, first = [0], [0], [False]
    i = 0
    while i < len(parent):
        for c in range(counts_of(i, depth[i], first[i])):
            parent.append(i)
            depth.append(depth[i] + 1)
            first.append(c == 0)
        i += 1
    return np.array(parent, np.int64), np.array(depth, np.int64)


def _number(parent, scheme, seed):
    """DBoW2 ids of the abstract (breadth-first) nodes: 'bfs' = the same, 'dfs' = depth-first preorder (what a recursive trainer gives),
    'perm' = a seeded permutation (what nothing forbids)"""
    n = len(parent)
    if scheme == "bfs":
        return np.arange(n)
    if scheme == "perm":
        ids = np.zeros(n, np.int64)
        ids[1:] = 1 + np.argsort(_synth().lcg_states(seed, n - 1), kind="stable")
        return ids
    kids = [[] for _ in range(n)]
    for i in range(1, n):
        kids[parent[i]].append(i)
    ids, stack, nxt = np.zeros(n, np.int64), [0], 0
    while stack:
        v = stack.pop()
        ids[v] = nxt
        nxt += 1
        stack.extend(reversed(kids[v]))
    return ids


def _weights(is_leaf, seed, stopped):
    """word weights; stopped: 'none', 'some' (a seventh), 'half', 'all' of the words have weight 0"""
    s = _synth()
    n = len(is_leaf)
    w = 0.5 + (s.lcg_states(seed, n) % 1000).astype(np.float64) / 500.0
    r = s.lcg_states(seed + 1, n) >> np.uint32(9)
    if stopped == "some":
        w[r % 7 == 0] = 0.0
    elif stopped == "half":
        w[r % 2 == 0] = 0.0
    elif stopped == "all":
        w[:] = 0.0
    w[~is_leaf] = 0.0
    return w


_TREES = {}


def routed_tree(name, kind, k, L, counts_of, scheme, seed, stopped="some", edit=None):
    """edit(tree): changes to the node descriptors of the new tree, applied before anybody else sees it (a cached tree is never edited)"""
    key = (name, kind)
    if key not in _TREES:
        ap, ad = _shape(counts_of)
        n = len(ap)
        width = WIDTH[kind]
        desc = np.zeros((n, width), np.float32 if is_float(kind) else np.uint8)
        desc[0] = _rand(kind, seed, 1, width)[0]
        noise = _rand(kind, seed + 1, n, width)
        for d in range(1, int(ad.max()) + 1):          # breadth-first: the parents of depth d are complete
            at = np.flatnonzero(ad == d)
            desc[at] = desc[ap[at]]
            desc[at, _seg(kind, d)] = noise[at, _seg(kind, d)]
        ids = _number(ap, scheme, seed + 2)
        parent = np.zeros(n, np.int32)
        parent[ids] = ids[ap]
        by_id = np.zeros_like(desc)
        by_id[ids] = desc
        by_id[0] = 0                                   # the root carries no descriptor
        leaf = np.ones(n, bool)
        leaf[parent[1:]] = False
        t = TreeData("%s_%s" % (name, kind), kind, k, L, parent, by_id, _weights(leaf, seed + 3, stopped), leaf)
        if edit is not None:
            edit(t)
            t._ref = None                              # (the restatement's view of the tree is built from the edited rows)
        _TREES[key] = t
    return _TREES[key]


class Scene:
    def __init__(self, name, rule, tree, features, levelsup, cap=0, **facts):
        self.name, self.rule, self.tree, self.kind, self.levelsup, self.cap = name, rule, tree, tree.kind, levelsup, cap
        self.features = np.ascontiguousarray(features, np.float32 if is_float(tree.kind) else np.uint8).reshape(-1, WIDTH[tree.kind])
        self.n = len(self.features)
        self.facts = facts

    def __repr__(self):
        return self.name


_REF = {}


def ref(scene):
    """the restatement's (leaf, nid, trace, FeatureVector, BowVector) of a scene, computed once and left unchanged"""
    if scene.name not in _REF:
        trace = []
        leaf, nid = R.transform_nodes(scene.tree.ref, scene.features, scene.levelsup, trace=trace)
        leaf.setflags(write=False)
        nid.setflags(write=False)
        _REF[scene.name] = (leaf, nid, trace, R.feature_vector(scene.tree.ref, leaf, nid), R.bow_vector(scene.tree.ref, leaf))
    return _REF[scene.name]


def _queries(tree, targets):
    return tree.node_desc[np.asarray(targets, np.int64)] if len(targets) else np.zeros((0, WIDTH[tree.kind]), tree.node_desc.dtype)


# ---------------------------------------------------------------- chunk edges ----------------------------------------------------------------
def chunk_tree(kind):
    return routed_tree("chunks", kind, 49, 2, lambda i, d, f: len(CHUNK_COUNTS) if d == 0 else CHUNK_COUNTS[i - 1] if d == 1 else 0, "perm", 11)


def chunk_edges(kind):
    """nodes of 1 .. 49 children; queries whose winner is child 0, the last child, lane 15 of every chunk and lane 0 of every later chunk.
    facts['want']: per feature (child count, position)"""
    t = chunk_tree(kind)
    targets, want = [], []
    for node in t.ref.children[0]:
        kids = t.ref.children[node]
        for pos in sorted({0, len(kids) - 1} | {p for p in (15, 31, 47, 16, 32, 48) if p < len(kids)}):
            targets.append(kids[pos])
            want.append((len(kids), pos))
    return Scene("chunk_edges_" + kind, "winner on a named lane", t, _queries(t, targets), 1, want=want)


# ---------------------------------------------------------------- ties across chunks ----------------------------------------------------------------
def _flip(kind, row, where, amount):
    row = row.copy()
    if is_float(kind):
        row[where] += np.float32(amount) * np.float32(2.0 ** -6)
    else:
        row[where // 8] ^= np.uint8(1 << (where % 8))
    return row


def tie_tree(kind):
    """every depth-1 node has 49 children; case c makes the children at the positions TIE_CASES[c] exact copies of each other.  Binary
    kinds: two more nodes whose tied children are DIFFERENT descriptors at the same distance from the query"""
    ncase = len(TIE_CASES) + (0 if is_float(kind) else 2)

    def tie(t):
        lo = _seg(kind, 2).start * (1 if is_float(kind) else 8)
        for c, node in enumerate(t.ref.children[0]):
            kids = t.ref.children[node]
            if c < len(TIE_CASES):
                for p in TIE_CASES[c][1:]:
                    t.node_desc[kids[p]] = t.node_desc[kids[TIE_CASES[c][0]]]
            else:                                     # X ^ bit a and X ^ bit b: distance 1 from X each, distance 2 from each other
                p, q = ((3, 19), (17, 35))[c - len(TIE_CASES)]
                x = t.node_desc[kids[p]].copy()
                t.node_desc[kids[p]] = _flip(kind, x, lo + 1, 1)
                t.node_desc[kids[q]] = _flip(kind, x, lo + 10, 1)
    return routed_tree("ties", kind, 49, 2, lambda i, d, f: ncase if d == 0 else 49 if d == 1 else 0, "perm", 23, stopped="none", edit=tie)


def tie_scene(kind):
    """one query per case, next to the tied descriptor (three bits / a small step away, so that the tie is at a distance > 0); the binary
    'different descriptors' cases query the X both children are one bit from.  facts['want']: per feature the tied positions"""
    t = tie_tree(kind)
    s2 = _seg(kind, 2)
    lo = s2.start * (1 if is_float(kind) else 8)
    feats, want = [], []
    for c, node in enumerate(t.ref.children[0]):
        kids = t.ref.children[node]
        if c < len(TIE_CASES):
            q = t.node_desc[kids[TIE_CASES[c][0]]]
            for j, w in enumerate((2, 13, 29)):
                q = _flip(kind, q, lo + w if not is_float(kind) else s2.start + j, j + 1)
            feats.append(q)
            want.append(list(TIE_CASES[c]))
        else:
            p, q = ((3, 19), (17, 35))[c - len(TIE_CASES)]
            x = _flip(kind, t.node_desc[kids[p]], lo + 1, 1)      # undo the flip: X
            feats.append(x)
            want.append([p, q])
    return Scene("ties_" + kind, "first minimum across chunks", t, np.stack(feats), 1, want=want)


# ---------------------------------------------------------------- float summation order ----------------------------------------------------------------
ORDER_PAIRS = 3


def _order_rows(dim, seed):
    """q, A = q + d, B = q + reversed(d): element i lies on the grid 2^-g[i], g = 20, 24 .. 44 and symmetric in i, q below 2^24 and d below
    2^18 steps of it (full 24-bit mantissas) - every sum and difference is exact in float32, the squares of A and B are the same numbers in opposite order, and
    they reach from 2^-88 to 2^-4: a float64 sum of them rounds, a float32 sum rounds a lot"""
    s = _synth()
    st = s.lcg_states(seed, 5 * dim).reshape(5, dim) >> np.uint32(8)
    mq = (st[0] % ((1 << 24) - (1 << 19))).astype(np.int64) + (1 << 18)
    e = (st[1] % 19).astype(np.int64)
    md = (1 + st[2] % (np.int64(1) << e)) * np.where(st[3] & 1, 1, -1)
    g = 20 + 4 * (st[4] % 7).astype(np.int64)
    g[dim // 2:] = g[:dim // 2][::-1]
    g = np.ldexp(1.0, -g)
    q, a, b = (mq * g).astype(np.float32), ((mq + md) * g).astype(np.float32), ((mq + md[::-1]) * g).astype(np.float32)
    assert np.array_equal(q.astype(np.float64), mq * g) and np.array_equal(a.astype(np.float64), (mq + md) * g)
    return q, a, b


def _order_scene(kind, wrong, tag):
    """root with 2 * ORDER_PAIRS children (leaves); query j is nearly equidistant from children 2j and 2j + 1 and far from the others.
    Seeds searched on the CPU: the DBoW2 winner (float32 squares, float64 sum, index order) differs from the winner under `wrong`"""
    dim = WIDTH[kind]
    rows, feats, seeds = [], [], []
    seed = 0
    while len(feats) < ORDER_PAIRS:
        if seed >= 4000:
            raise AssertionError("no seed below %d reaches the rule" % seed)
        q, a, b = _order_rows(dim, 7000 + 13 * seed + dim)
        two = np.stack([a, b])
        d_ok, d_bad = R.float_distances(q, two).tolist(), R.float_distances(q, two, wrong).tolist()
        if (d_ok[1] < d_ok[0]) != (d_bad[1] < d_bad[0]):
            rows += [a, b]
            feats.append(q)
            seeds.append(seed)
        seed += 1
    n = 1 + len(rows)
    desc = np.zeros((n, dim), np.float32)
    desc[1:] = np.stack(rows)
    leaf = np.ones(n, bool)
    leaf[0] = False
    t = TreeData("order_%s_%s" % (tag, kind), kind, 2 * ORDER_PAIRS, 1, np.zeros(n, np.int32), desc, _weights(leaf, 5, "none"), leaf)
    return Scene("order_%s_%s" % (tag, kind), "float summation: " + tag, t, np.stack(feats), 0, seeds=seeds)


_ORDER = {}


def order_scenes(kind):
    if kind not in _ORDER:
        _ORDER[kind] = [_order_scene(kind, R.Rules(float32_sum=True), "f32"), _order_scene(kind, R.Rules(reversed_sum=True), "rev")]
    return _ORDER[kind]


# ---------------------------------------------------------------- ragged, renumbered trees ----------------------------------------------------------------
RAGGED_L = 4
_RAGGED_CYCLE = (3, 17, 2, 5, 4, 2, 3, 33, 2, 2)
RAGGED_LEVELSUP = (0, 1, RAGGED_L - 1, RAGGED_L, RAGGED_L + 3)


def ragged_tree(kind, scheme):
    """the first child of every inner node is a leaf: leaves at depths 1 .. 4; 2 .. 33 children per node"""
    def counts(i, d, first):
        if d == 0:
            return 4
        return 0 if d == RAGGED_L or first else _RAGGED_CYCLE[i % len(_RAGGED_CYCLE)]
    return routed_tree("ragged_" + scheme, kind, 33, RAGGED_L, counts, scheme, 31, stopped="half")


def ragged_targets(t, n, seed=41):
    """feature i ends at a leaf of depth 1 + i % 4: the four rows of a wavefront stop at four different depths"""
    r = t.ref
    by_depth = [[i for i in range(1, len(r.parent)) if r.is_leaf[i] and r.depth[i] == d] for d in range(1, RAGGED_L + 1)]
    st = _synth().lcg_states(seed, max(n, 1)) >> np.uint32(8)
    return [by_depth[i % 4][int(st[i]) % len(by_depth[i % 4])] for i in range(n)]


def ragged_scenes(kind):
    out = []
    for scheme in ("dfs", "perm"):
        t = ragged_tree(kind, scheme)
        targets = ragged_targets(t, max(N_SMALL))
        for levelsup in RAGGED_LEVELSUP:
            for n in N_SMALL:
                out.append(Scene("ragged_%s_%s_up%d_n%d" % (scheme, kind, levelsup, n), "ragged renumbered tree", t, _queries(t, targets[:n]), levelsup,
                                 cap=80, scheme=scheme))
    return out


def table_scenes(kind):
    """two keyframes on the renumbered ragged tree: the second holds the first one's descriptors in another order"""
    t = ragged_tree(kind, "perm")
    targets = ragged_targets(t, 65, seed=43)
    order = np.argsort(_synth().lcg_states(47, 65), kind="stable")
    return (Scene("table_a_" + kind, "promotion", t, _queries(t, targets), 1, cap=80),
            Scene("table_b_" + kind, "promotion", t, _queries(t, [targets[i] for i in order]), 1, cap=80))


# ---------------------------------------------------------------- FeatureVector regimes ----------------------------------------------------------------
def wide_tree(kind, leaves, stopped):
    """k = 16, L = 3, ids by a seeded permutation; 4096 leaves, or 4095 (the last depth-2 node has 15 children)"""
    def counts(i, d, first):
        return 0 if d == 3 else 15 if (leaves == 4095 and i == 16 + 256) else 16
    base = routed_tree("wide%d" % leaves, kind, 16, 3, counts, "perm", 53, stopped="some")
    if stopped == "some":
        return base
    key = ("wide%d/%s" % (leaves, stopped), kind)
    if key not in _TREES:
        _TREES[key] = base.with_weights(stopped, _weights(base.is_leaf, 56, stopped))
    return _TREES[key]


def _leaf_under(t, node, j):
    kids = t.ref.children[node]
    return kids[j % len(kids)]


def _regime_targets(t, layout, n, seed):
    r = t.ref
    st = (_synth().lcg_states(seed, 4 * max(n, 64) + 64) >> np.uint32(8)).astype(np.int64)
    level2 = [i for i in range(1, len(r.parent)) if r.depth[i] == 2]
    leaves = [i for i in range(1, len(r.parent)) if r.depth[i] == 3]
    if layout == "one_node":                          # every wave byte at its maximum of 64; the node of the highest id: the last key of the level
        return [_leaf_under(t, max(level2), int(st[i])) for i in range(n)]
    if layout == "own_node":                          # n distinct leaves
        pick = np.argsort(_synth().lcg_states(seed + 1, len(leaves)), kind="stable")
        return [leaves[int(pick[i])] for i in range(n)]
    if layout == "alternate":
        return [_leaf_under(t, level2[(5, 201)[i & 1]], int(st[i])) for i in range(n)]
    if layout == "random_leaves":
        return [leaves[int(st[i]) % len(leaves)] for i in range(n)]
    palette = [level2[(7 * j + 3) % len(level2)] for j in range(40)]
    out = []
    if layout in ("waves40", "second_chunk"):          # per wave of 64: runs of 2 .. 30 equal keys (every other wave: 2 .. 6), shuffled inside the wave
        special = level2[250]
        p = 0
        for w0 in range(0, n, 64):
            wave = []
            while len(wave) < 64:
                node = palette[int(st[p]) % 40]
                wave += [node] * (2 + int(st[p + 1]) % (29 if w0 & 64 else 5))
                p += 2
            wave = wave[:64]
            if layout == "second_chunk" and 1024 <= w0 < 2048:
                for j in range(0, 64, 5):
                    wave[j] = special                  # a node whose features fall only in the second chunk
            order = np.argsort(st[p:p + 64], kind="stable")
            p += 64
            out += [wave[int(j)] for j in order]
        return [_leaf_under(t, node, int(st[i])) for i, node in enumerate(out[:n])]
    raise ValueError(layout)


# (name, leaves of the tree, stopped words, layout, n, levelsup)
_REGIMES_FULL = (
    [("one_node_n%d" % n, 4096, "some" if n in (1023, 1025) else "none", "one_node", n, 1) for n in N_LARGE] +
    [("own_node_n1023", 4095, "none", "own_node", 1023, 0), ("own_node_n1025", 4095, "half", "own_node", 1025, 0),
     ("own_node_n3000", 4095, "some", "own_node", 3000, 0),
     ("alternate_n2049", 4096, "half", "alternate", 2049, 1),
     ("waves40_none", 4096, "none", "waves40", 3000, 1), ("waves40_half", 4096, "half", "waves40", 3000, 1),
     ("waves40_all", 4096, "all", "waves40", 3000, 1),
     ("waves40_w4096", 4095, "half", "waves40", 2049, 0),
     ("second_chunk_n2049", 4096, "none", "second_chunk", 2049, 1), ("second_chunk_n3000", 4096, "some", "second_chunk", 3000, 1),
     ("width1_L", 4096, "some", "waves40", 1025, 3), ("width1_beyond", 4096, "half", "waves40", 1024, 6),
     ("width17", 4096, "some", "waves40", 1023, 2),
     ("quad_n1023", 4096, "half", "random_leaves", 1023, 0), ("quad_n2049", 4096, "none", "own_node", 2049, 0),
     ("quad_n3000", 4096, "some", "waves40", 3000, 0)])


def regime_names(kind):
    """every regime runs on every kind"""
    return [r[0] for r in _REGIMES_FULL]


def regime_scenes(kind, only=None):
    out = []
    for name, leaves, stopped, layout, n, levelsup in _REGIMES_FULL:
        if name not in regime_names(kind) or (only is not None and name != only):
            continue
        t = wide_tree(kind, leaves, stopped)
        out.append(Scene("regime_%s_%s" % (name, kind), "FeatureVector regime: " + layout, t, _queries(t, _regime_targets(t, layout, n, 61 + n + levelsup)),
                         levelsup, cap=FRAME_CAP, layout=layout, leaves=leaves, stopped=stopped))
    return out


# ---------------------------------------------------------------- all ----------------------------------------------------------------
_ALL = {}


def descent_scenes(kind):
    """the scenes about the descent: small frames"""
    return [chunk_edges(kind), tie_scene(kind)] + (order_scenes(kind) if is_float(kind) else []) + ragged_scenes(kind)


def all_scenes(kind):
    if kind not in _ALL:
        _ALL[kind] = descent_scenes(kind) + regime_scenes(kind)
    return _ALL[kind]


def by_name(name):
    return next(s for k in KINDS for s in all_scenes(k) if s.name == name)
