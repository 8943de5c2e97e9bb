"""Plain restatement of BoW quantisation (Frame::ComputeBoW), the checker of tests/test_quant_ref_cpu.py and tests/test_gpu_quant_scenes.py.
It imports nothing from the package, and it is written from DBoW2, not from the kernels and not from oracle/afvo.c.

The reference calls TemplatedVocabulary::transform(features, BowVector, FeatureVector, levelsup = 4) through Vocabulary::transform
(src/Vocabulary.cpp:156-206: one case per descriptor type, binary ones as cv::Mat rows, float ones as vector<float>) from
Frame::ComputeBoW (src/Frame.cc:397-401) and KeyFrame::ComputeBoW (src/KeyFrame.cc:65-73).  DBoW2 is an empty submodule there; what
follows is upstream DBoW2, TemplatedVocabulary.h:

  transform(features, v, fv, levelsup), TF_IDF branch:
      for each feature i:  transform(feature, id, w, &nid, levelsup);  if(w > 0) { v.addWeight(id, w); fv.addFeature(nid, i); }
      then v.normalize(L1)
  transform(feature, word_id, weight, nid, levelsup):
      nid_level = m_L - levelsup;  if(nid_level <= 0 && nid != NULL) *nid = 0;
      final_id = 0; current_level = 0;
      do { ++current_level;  nodes = m_nodes[final_id].children;
           final_id = nodes[0]; best_d = F::distance(feature, m_nodes[final_id].descriptor);
           for(the other children, in order) { d = F::distance(...); if(d < best_d) { best_d = d; final_id = id; } }
           if(nid != NULL && current_level == nid_level) *nid = final_id;
      } while(!m_nodes[final_id].isLeaf());

so: every child in child order, the FIRST minimum wins (strict <), the descent stops at a node without children.  The children of a node
are in the order loadFromTextFile pushed them: ascending node id.  F::distance is the Hamming distance over the descriptor's bytes for the
binary classes and, for the float classes (FSurf64::distance and its kin), `sqd += (a[i] - b[i]) * (a[i] - b[i])` with float operands and
a double sum, i = 0, 1, ...

nid: the node chosen at depth L - levelsup.  When L - levelsup <= 0 it is 0.  When the leaf is reached above that depth DBoW2 leaves
*nid unwritten (the caller's variable is uninitialised); the oracle defines that case as 0, and so does this file.

FeatureVector: std::map<NodeId, vector<unsigned>>: nodes ascend by DBoW2 id, the features of a node ascend (addFeature is called for
i = 0, 1, ...), and only features whose word weight is > 0 enter.  BowVector: tests/_kfdb_ref.bow_vector.

Every rule has a switchable wrong alternative (`Rules`): tests/test_quant_ref_cpu.py proves that the scene built for a rule changes under it.
"""
import numpy as np

import _kfdb_ref

CHUNK = 16   # children a 16-lane row of the device kernels takes at a time; the trace names the chunk of a position, nothing here depends on it


class Rules:
    """the rules of the restatement; every default is DBoW2's, every other value a wrong alternative"""

    def __init__(self, last_minimum=False, float32_sum=False, reversed_sum=False, record_order=False, keep_stopped=False, nid_off=0):
        self.last_minimum = last_minimum    # '<=': the last minimum wins
        self.float32_sum = float32_sum      # the float distance accumulated in float32
        self.reversed_sum = reversed_sum    # ... accumulated from the last index down
        self.record_order = record_order    # FeatureVector nodes in breadth-first (record) order instead of id order
        self.keep_stopped = keep_stopped    # words of weight 0 enter the FeatureVector
        self.nid_off = nid_off              # nid taken at depth L - levelsup + nid_off


DBOW2 = Rules()


class Tree:
    """a vocabulary tree in DBoW2 terms: node i has parent[i] (node 0 = the root), a descriptor row, a weight; children in ascending id"""

    def __init__(self, k, L, parent, node_desc, weight, is_leaf):
        self.k, self.L = int(k), int(L)
        self.parent = [int(p) for p in parent]
        n = len(self.parent)
        self.node_desc = np.asarray(node_desc)
        self.is_float = self.node_desc.dtype.kind == "f"
        self.weight = [float(w) for w in weight]
        self.is_leaf = [bool(b) for b in is_leaf]
        self.children = [[] for _ in range(n)]
        for i in range(1, n):                      # loadFromTextFile: m_nodes[pid].children.push_back(nid), nid = 1, 2, ...
            self.children[self.parent[i]].append(i)
        self.word_id = [-1] * n                    # ... and words numbered in node order
        w = 0
        for i in range(n):
            if self.is_leaf[i]:
                self.word_id[i] = w
                w += 1
        self.depth = [0] * n
        self.record = []                           # breadth-first order from the root, children in child order
        frontier = [0]
        while frontier:
            nxt = []
            for p in frontier:
                self.record.append(p)
                for c in self.children[p]:
                    self.depth[c] = self.depth[p] + 1
                    nxt.append(c)
            frontier = nxt
        if not self.is_float:
            self._bits = [int.from_bytes(self.node_desc[i].tobytes(), "little") for i in range(n)]
        self._rows = {}

    def child_rows(self, node):
        if node not in self._rows:
            self._rows[node] = np.ascontiguousarray(self.node_desc[self.children[node]], np.float32)
        return self._rows[node]


def hamming(a, b):
    """DBoW2 FORB::distance and its kin over the bytes of the descriptor: the number of differing bits (a, b: the rows as integers)"""
    return bin(a ^ b).count("1")


def float_distances(feature, rows, rules=DBOW2):
    """FSurf64::distance for every row of `rows`: (a - b) * (a - b) in float32, accumulated in float64 in index order.  np.add.accumulate
    is the sequential recurrence out[i] = out[i - 1] + x[i] along the axis, in the dtype of its input"""
    d = feature[None, :] - rows                    # float32 - float32
    sq = d * d                                     # float32
    if rules.reversed_sum:
        sq = sq[:, ::-1]
    if rules.float32_sum:
        return np.add.accumulate(np.ascontiguousarray(sq), axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    return np.add.accumulate(sq.astype(np.float64), axis=1)[:, -1]


def descend(tree, feature, levelsup, rules=DBOW2, steps=None):
    """transform(feature, word_id, weight, nid, levelsup): (leaf node, nid).  steps (a list) receives one record per level: the child
    count, the winner's position and chunk, the positions that hold the minimum (more than one: a tie)"""
    nid_level = tree.L - levelsup + rules.nid_off
    nid = 0
    final_id, level = 0, 0
    fbits = None if tree.is_float else int.from_bytes(np.ascontiguousarray(feature, np.uint8).tobytes(), "little")
    while True:
        level += 1
        nodes = tree.children[final_id]
        if tree.is_float:
            dist = float_distances(feature, tree.child_rows(final_id), rules).tolist()
        else:
            dist = [hamming(fbits, tree._bits[c]) for c in nodes]
        pos, best = 0, dist[0]
        for c in range(1, len(nodes)):
            if dist[c] < best or (rules.last_minimum and dist[c] == best):
                pos, best = c, dist[c]
        final_id = nodes[pos]
        if steps is not None:
            tied = [c for c in range(len(nodes)) if dist[c] == best]
            steps.append({"count": len(nodes), "pos": pos, "chunk": pos // CHUNK, "tied": tied if len(tied) > 1 else []})
        if level == nid_level:
            nid = final_id
        if not tree.children[final_id]:
            break
    return final_id, (0 if nid_level <= 0 else nid)


def transform_nodes(tree, features, levelsup, rules=DBOW2, trace=None):
    """(leaf, nid) per feature as int32 arrays; trace (a list) receives the per-level records of every feature"""
    if tree.is_float:
        features = np.ascontiguousarray(features, np.float32)
    leaf, nid = np.zeros(len(features), np.int32), np.zeros(len(features), np.int32)
    for i in range(len(features)):
        steps = None if trace is None else []
        leaf[i], nid[i] = descend(tree, features[i], levelsup, rules, steps)
        if trace is not None:
            trace.append(steps)
    return leaf, nid


def feature_vector(tree, leaf, nid, rules=DBOW2):
    """[(node id, [feature indices ascending])], nodes ascending by DBoW2 id"""
    fv = {}
    for i in range(len(leaf)):
        if tree.weight[int(leaf[i])] > 0 or rules.keep_stopped:
            fv.setdefault(int(nid[i]), []).append(i)
    if rules.record_order:
        place = {node: r for r, node in enumerate(tree.record)}
        return sorted(fv.items(), key=lambda kv: place[kv[0]])
    return sorted(fv.items())


def bow_vector(tree, leaf):
    """{word: value}, ascending words, L1-normalised"""
    return _kfdb_ref.bow_vector([int(v) for v in leaf], tree.weight, tree.word_id)
