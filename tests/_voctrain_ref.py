"""Plain-Python restatement of DBoW2's TemplatedVocabulary::create for binary descriptors - the NORMATIVE semantics of afv_vocab_train
(include/afv_hip.h).  DBoW2 is an empty submodule in the reference (.gitmodules:1-3); create / HKmeansStep / initiateClustersKMpp /
createWords / setNodeWeights / FORB::meanValue / FORB::distance are restated from upstream DBoW2, parity unpinned.  The reference calls
it from src/createVocabulary.cpp:292-301 with k = 9, L = 3, TF_IDF, L1_NORM (:50-53).

Plain loops over Python ints; a descriptor row is one int (little-endian bytes), a distance is the popcount of an xor.  The per-bit
counts of the mean are summed with one big-int addition per member: every bit of a row is spread to a 32-bit field of its own (bit b at
position 32 * b), so the sum of the spread rows holds all counts side by side - integer additions, the same counts as a loop per bit.

Two deliberate differences from upstream (documented in DESIGN.md):
  * an EMPTY cluster keeps its previous centre (upstream releases it, the next distance then reads an empty matrix);
  * the seeding draws come from a counter-based generator, a pure function of (seed, path from the root, draw index), instead of rand().
Two parameters beyond upstream: max_iters (cap on the associate / mean rounds of a node, 0 = none) and init_centres (replaces the seeding
of the root only).
"""
import math

M64 = (1 << 64) - 1
DRAW_STEP = 0xD1342543DE82EF95
FIELD = 32


def sm(x):
    """splitmix64"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def root_key(seed):
    return sm(seed & M64)


def child_key(key, i):
    return sm(key ^ (i + 1))


def distance(a, b):
    """FORB::distance: Hamming"""
    return bin(a ^ b).count("1")


_SPREAD8 = []
for _v in range(256):
    _s = 0
    for _b in range(8):
        if (_v >> _b) & 1:
            _s |= 1 << (FIELD * _b)
    _SPREAD8.append(_s)


def spread(row, desc_bytes):
    s = 0
    for j in range(desc_bytes):
        s |= _SPREAD8[(row >> (8 * j)) & 255] << (FIELD * 8 * j)
    return s


def mean_value(members, spreads, rows, desc_bytes, trace=None):
    """FORB::meanValue: one member gives a copy; otherwise bit b is set iff count_b >= N / 2 + N % 2"""
    N = len(members)
    if N == 1:
        return rows[members[0]]
    total = 0
    for f in members:
        total += spreads[f]
    need = N // 2 + N % 2
    out = 0
    for b in range(8 * desc_bytes):
        cnt = (total >> (FIELD * b)) & 0xFFFFFFFF
        if trace is not None and (2 * cnt == N or 2 * cnt == N + 1 or 2 * cnt == N - 1):
            trace["majority_edge"].add((N % 2, 2 * cnt - N))
        if cnt >= need:
            out |= 1 << b
    return out


def seed_kmpp(feats, rows, k, key, trace=None):
    """initiateClustersKMpp with the generator replaced: the draw is weighted by the distance (not its square), as upstream"""
    n = len(feats)
    centres = [rows[feats[sm(key) % n]]]
    min_dist = [1 << 30] * n
    j = 0
    while len(centres) < k:
        j += 1
        last = centres[-1]
        for i in range(n):
            if min_dist[i] > 0:
                d = distance(rows[feats[i]], last)
                if d < min_dist[i]:
                    min_dist[i] = d
        dist_sum = 0
        for i in range(n):
            dist_sum += min_dist[i]
        if dist_sum == 0:
            if trace is not None:
                trace["seed_short"] += 1
            break
        cut = 1 + sm((key + j * DRAW_STEP) & M64) % dist_sum
        run = 0
        pick = n - 1
        for i in range(n):
            run += min_dist[i]
            if run >= cut:
                pick = i
                if trace is not None:
                    if run == cut:
                        trace["cut_on_boundary"] += 1
                    if cut == dist_sum:
                        trace["cut_is_sum"] += 1
                break
        centres.append(rows[feats[pick]])
    return centres


def associate(feats, rows, centres, trace=None):
    assoc, groups = [], [[] for _ in centres]
    for f in feats:
        best, bc = 1 << 30, 0
        tie = False
        for c in range(len(centres)):
            d = distance(rows[f], centres[c])
            if d < best:               # strictly smaller wins: the first minimum stays
                best, bc, tie = d, c, False
            elif d == best:
                tie = True
        if tie and trace is not None:
            trace["assoc_tie"] += 1
        assoc.append(bc)
        groups[bc].append(f)           # ascending feature order
    return assoc, groups


def new_trace():
    return {"seed_short": 0, "cut_on_boundary": 0, "cut_is_sum": 0, "assoc_tie": 0, "majority_edge": set(), "empty_cluster": 0,
            "trivial": 0, "capped_nodes": 0, "max_node_rounds": 0, "nodes": []}


def train(images, desc_bytes, k, L, seed=0, max_iters=0, init_centres=None, trace=None):
    """images: per image a sequence of rows (bytes-like / uint8 arrays of desc_bytes).  Returns a dict: parent, desc (bytes per node), is_leaf,
    ni (-1 for inner nodes), weight, rounds (per level: the most rounds a node of that level ran), capped."""
    rows, image_ptr = [], [0]
    for img in images:
        for r in img:
            rows.append(int.from_bytes(bytes(bytearray(r)), "little"))
        image_ptr.append(len(rows))
    spreads = [spread(r, desc_bytes) for r in rows]
    parent, desc, children = [0], [0], [[]]
    rounds = [0] * L
    state = {"capped": False}

    def hkmeans_step(parent_id, feats, level, key):
        if not feats:
            return
        node_rounds, node_capped = 0, False
        if len(feats) <= k:            # trivial case: one cluster per feature
            groups = [[f] for f in feats]
            centres = [rows[f] for f in feats]
            if trace is not None:
                trace["trivial"] += 1
        else:
            if level == 1 and init_centres is not None:
                centres = [int.from_bytes(bytes(bytearray(r)), "little") for r in init_centres]
            else:
                centres = seed_kmpp(feats, rows, k, key, trace)
            last = None
            while True:
                if node_rounds > 0:
                    for c in range(len(centres)):
                        if groups[c]:
                            centres[c] = mean_value(groups[c], spreads, rows, desc_bytes, trace)
                        elif trace is not None:    # the deviation: an empty cluster keeps its centre
                            trace["empty_cluster"] += 1
                assoc, groups = associate(feats, rows, centres, trace)
                node_rounds += 1
                if last is not None and assoc == last:
                    break
                if max_iters and node_rounds >= max_iters:
                    node_capped = True
                    break
                last = assoc
        rounds[level - 1] = max(rounds[level - 1], node_rounds)
        state["capped"] = state["capped"] or node_capped
        first = len(parent)
        for c in range(len(centres)):  # a node per cluster, empty ones too, before recursing
            parent.append(parent_id)
            desc.append(centres[c])
            children.append([])
            children[parent_id].append(first + c)
        if trace is not None:
            trace["capped_nodes"] += int(node_capped)
            trace["max_node_rounds"] = max(trace["max_node_rounds"], node_rounds)
            trace["nodes"].append({"id": parent_id, "level": level, "n": len(feats), "trivial": len(feats) <= k, "rounds": node_rounds,
                                   "capped": node_capped, "groups": [list(g) for g in groups], "centres": list(centres),
                                   "children": list(children[parent_id])})
        if level < L:
            for c in range(len(centres)):
                if len(groups[c]) > 1:
                    hkmeans_step(first + c, groups[c], level + 1, child_key(key, c))

    hkmeans_step(0, list(range(len(rows))), 1, root_key(seed))
    n = len(parent)
    is_leaf = [i > 0 and not children[i] for i in range(n)]
    # createWords: leaves get word ids in node-id order; setNodeWeights (TF-IDF): Ni = images with a feature whose DESCENT ends in the word
    ni = [0 if is_leaf[i] else -1 for i in range(n)]
    leaf_of = []
    nimages = len(image_ptr) - 1
    for im in range(nimages):
        seen = set()
        for f in range(image_ptr[im], image_ptr[im + 1]):
            w = descend(rows[f], desc, children)
            leaf_of.append(w)
            if w not in seen:
                seen.add(w)
                ni[w] += 1
    weight = [0.0] * n
    for i in range(n):
        if is_leaf[i] and ni[i] > 0:
            weight[i] = math.log(float(nimages) / float(ni[i]))
    return {"parent": parent, "desc": [d.to_bytes(desc_bytes, "little") for d in desc], "is_leaf": is_leaf, "ni": ni, "weight": weight,
            "rounds": rounds, "capped": state["capped"], "leaf_of": leaf_of, "children": children, "desc_int": desc}


def descend(row, desc, children):
    """TemplatedVocabulary::transform(feature, word_id): at every node the child of smallest distance, the first minimum"""
    node = 0
    while children[node]:
        best, bn = 1 << 30, 0
        for ch in children[node]:
            d = distance(row, desc[ch])
            if d < best:
                best, bn = d, ch
        node = bn
    return node
