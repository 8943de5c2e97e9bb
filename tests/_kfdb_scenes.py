"""Constructed place-recognition scenes: every scene is small, has a name, states the rule it exists for and names the flips of
tests/_kfdb_ref.py that must move its answer (tests/test_kfdb_ref_cpu.py proves that on the restatement alone; tests/test_gpu_kfdb_scenes.py
runs the scenes on the device and through both mirrors of KeyFrameDatabase).  Nothing here touches a kernel: the tree of
_bow_scenes.vocabulary is read as arrays, the leaves of the descriptor pool come from _bow_scenes.cpu_leaves.

Three families:
  (a) bow_scenes()      lists of leaf ids over the 10 000-word tree, each with a weight array (k_bowvec_build, afv_bow_vector);
  (b) score_scenes()    slot BowVectors and query BowVectors as host arrays (k_score_bow, afv_table_score_bow);
  (c) decision_scenes() operation scripts over hand-made BowVectors (KeyFrameDatabase in database.py and adapter/afv_adapter.hpp).
Values are dyadic wherever a rule needs an exact equality: for non-negative v, x the score term fabs(v - x) - v - x is -2 min(v, x), so the
score of two vectors is the sum of min(v, x) over the shared words, exact as long as the sum fits 53 bits."""
import numpy as np

import _bow_scenes as bs
import _kfdb_ref as ref

KIND = "orb32"
_cache = {}


# =====================================================================================================================================
# (a) BowVector scenes
# =====================================================================================================================================
N_POOL = 60000


def pool():
    """descriptors whose leaves are known: (desc uint8 [N_POOL, 32], leaf int32 [N_POOL], reach = the distinct leaves ascending,
    row_of = {leaf: first pool row that reaches it})"""
    if "pool" not in _cache:
        voc = bs.vocabulary(KIND)
        desc = np.random.RandomState(21).randint(0, 256, (N_POOL, 32)).astype(np.uint8)
        leaf = np.concatenate([bs.cpu_leaves(voc, desc[i:i + 4000]) for i in range(0, N_POOL, 4000)])
        reach, first = np.unique(leaf, return_index=True)
        _cache["pool"] = (desc, leaf, reach.astype(np.int32), dict(zip(reach.tolist(), first.tolist())))
    return _cache["pool"]


def descriptors_of(leaves):
    desc, _, _, row_of = pool()
    return np.ascontiguousarray(desc[[row_of[int(l)] for l in leaves]]).reshape(-1, 32)


def tree():
    """(weight, word_id, is_leaf) of the scene tree"""
    if "tree" not in _cache:
        v = bs.vocabulary(KIND)
        _cache["tree"] = (v.weight.copy(), v.word_id.copy(), v.is_leaf.copy())
    return _cache["tree"]


def weights(key):
    """the weight arrays of the scenes, one per key (a Vocabulary is built with them in place of its own):
    mixed         full 53-bit mantissas times 2^-40 .. 2^10: sums of them round at every addition, in an order-dependent way
    half_stopped  mixed, every second word (odd word id) stopped
    all_stopped   zeros"""
    if ("w", key) not in _cache:
        _, word_id, is_leaf = tree()
        n = len(word_id)
        rng = np.random.RandomState(7)
        w = (1.0 + rng.random_sample(n)) * np.ldexp(1.0, rng.randint(-40, 11, n))
        w[~is_leaf] = 0.0
        if key == "half_stopped":
            w[is_leaf & (word_id % 2 == 1)] = 0.0
        elif key == "all_stopped":
            w[:] = 0.0
        elif key != "mixed":
            raise KeyError(key)
        _cache[("w", key)] = w
    return _cache[("w", key)]


class BowScene:
    """leaves: the features' leaf nodes in feature order; flips: the flips of ref.bow_vector that must move the answer.  A scene with
    flips == () is a size edge whose answer holds no arithmetic to get wrong (at most one entry: {} or {word: 1.0}); it says so in
    `rule` and the CPU test checks that claim instead"""

    def __init__(self, name, rule, leaves, weight_key="mixed", flips=("norm_reversed",)):
        self.name, self.rule, self.leaves, self.weight_key, self.flips = name, rule, np.asarray(leaves, np.int32), weight_key, tuple(flips)

    @property
    def weight(self):
        return weights(self.weight_key)

    def want(self, flip=None):
        return ref.bow_vector(self.leaves.tolist(), self.weight, tree()[1], flip=flip)


def _draw(rng, n, nleaves):
    """n features over the first `nleaves` reachable leaves, every leaf at least once when n allows it, in random order"""
    reach = pool()[2]
    base = reach[:min(n, nleaves)]
    extra = reach[rng.randint(0, nleaves, max(0, n - len(base)))]
    return rng.permutation(np.concatenate([base, extra]))


def bow_scenes():
    if "bow" in _cache:
        return _cache["bow"]
    reach = pool()[2]
    assert len(reach) >= 8192, "the pool reaches %d leaves" % len(reach)
    rng = np.random.RandomState(33)
    S = []
    S.append(BowScene("n_0", "no feature: an empty vector, no launch", [], flips=()))
    S.append(BowScene("n_1", "one feature: P = 64 with 63 pads, one entry of value 1.0", reach[4000:4001], flips=()))
    # feature counts around the bitonic pad P (64, 1024, 8192) and the 1024-thread stretches; two to four features per word
    for n in (63, 64, 65, 1023, 1024, 1025, 4097, 8192):
        S.append(BowScene("n_%d" % n, "feature count %d: the pad P and the stretches per thread at this size" % n, _draw(rng, n, n // 2 if n < 1000 else n // 4),
                          flips=("norm_reversed", "count_times_weight") if n >= 1023 else ("norm_reversed",)))
    # distinct-word counts around the 1024-entry chunks of the norm
    for m in (1024, 1025, 2049, 8192):
        S.append(BowScene("words_%d" % m, "%d distinct words, each once: the norm is summed by one lane in chunks of 1024" % m,
                          rng.permutation(reach[:m])))
    S.append(BowScene("one_word_8192", "one word hit 8192 times and nothing else: one entry, value / norm = 1.0 whatever the value",
                      np.full(8192, reach[77]), flips=()))
    heavy = np.concatenate([np.full(8190, reach[77]), reach[[5, 6000]]])
    S.append(BowScene("heavy_word", "one word hit 8190 times next to two single words: the repeated addition over a run that crosses "
                      "1024 threads' stretches of 8 keys", rng.permutation(heavy), flips=("count_times_weight",)))
    # runs of 3, 9 and 1 keys in ascending word order: a cycle is 13 keys long, 13 is odd, so over 630 cycles the runs of 3 and of 9 start
    # at every offset modulo the 8 keys of a thread's stretch (P = 8192, 1024 threads); 8192 = 630 * 13 + 2
    counts = ([3, 9, 1] * 630) + [1, 1]
    runs = np.repeat(reach[:len(counts)], counts)
    assert len(runs) == 8192
    S.append(BowScene("runs_3_9", "runs of 3 and 9 equal keys at every offset modulo a stretch of 8", rng.permutation(runs),
                      flips=("norm_reversed", "count_times_weight")))
    S.append(BowScene("half_stopped_8192", "every second word stopped, no pad: the stopped keys sort behind the words",
                      _draw(rng, 8192, 3000), "half_stopped", flips=("norm_reversed", "count_times_weight")))
    S.append(BowScene("half_stopped_4097", "every second word stopped and 4095 pads behind them", _draw(rng, 4097, 1500), "half_stopped"))
    S.append(BowScene("all_stopped", "every leaf stopped: n = 0 entries, the norm is not > 0, nothing is divided", _draw(rng, 300, 100),
                      "all_stopped", flips=()))
    _cache["bow"] = S
    return S


# =====================================================================================================================================
# (b) score scenes
# =====================================================================================================================================
# afv_launch_score_bow (csrc/k_bowvec.hip) gives a workgroup of four wavefronts
#     slots_per_wg = clamp(nq * nsets / 4096, 4, 64) & ~3       (integer division)
# slots; wavefront w takes the slots s_begin + w, s_begin + w + 4, ...  With 4 every wavefront runs its loop once.
def slots_per_wg(nq, nsets):
    return min(max((nq * nsets) // 4096, 4), 64) & ~3


NO_BOW = "no_bow"     # a slot that holds features but no BowVector
EMPTY = "empty"       # a slot that holds nothing


class ScoreScene:
    """slots[i]: a {word: value} dict, NO_BOW or EMPTY; queries: dicts, or ("slot", i) for the BowVector of slot i; mask: uint8 per slot
    (never names a NO_BOW slot: that is an error by contract); flips: those of ref.l1_score that must move at least one cell;
    facts: [(query row, slot, (common, score, first_common))] worked out by hand"""

    def __init__(self, name, rule, slots, queries, mask, flips=("sum_reversed", "sum_pairwise"), facts=()):
        self.name, self.rule, self.slots, self.queries, self.flips, self.facts = name, rule, slots, queries, tuple(flips), list(facts)
        self.mask = np.asarray(mask, np.uint8)
        assert len(self.mask) == len(slots) and not any(m and s == NO_BOW for m, s in zip(self.mask, slots))

    @property
    def nsets(self):
        return len(self.slots)

    @property
    def cap(self):
        return max([1] + [len(s) for s in self.slots if isinstance(s, dict)])

    def query_bow(self, q):
        return self.slots[q[1]] if isinstance(q, tuple) else q

    def want(self, mask=None, flip=None):
        """(common, score, first_common) [nq, nsets]: the restatement, once per distinct (query, slot) pair"""
        nq, ns = len(self.queries), self.nsets
        common = np.full((nq, ns), -1, np.int32); score = np.zeros((nq, ns), np.float64); first = np.full((nq, ns), -1, np.int32)
        memo = {}
        for r, q in enumerate(self.queries):
            qb = self.query_bow(q)
            for s, sb in enumerate(self.slots):
                if not isinstance(sb, dict) or (mask is not None and not mask[s]):
                    continue
                key = (id(qb), id(sb))
                if key not in memo:
                    memo[key] = ref.l1_score(qb, sb, flip=flip)
                common[r, s], score[r, s], first[r, s] = memo[key]
        return common, score, first


def _mixed(rng, n):
    """values of mixed magnitude with full mantissas: every addition of score terms rounds"""
    return ((1.0 + rng.random_sample(n)) * np.ldexp(1.0, rng.randint(-30, 1, n))).tolist()


def _slot_sharing(rng, size, shared):
    """a slot of `size` words against the query {3 i}: entry i is word 3 i when i is in `shared` (the query has it), else 3 i + 1"""
    vals = _mixed(rng, size)
    return {3 * i + (0 if i in shared else 1): vals[i] for i in range(size)}


def _chunk_edges():
    rng = np.random.RandomState(41)
    q = dict(zip(range(0, 3 * 200, 3), _mixed(rng, 200)))
    slots = [
        {},                                              # 0  BowVector present but empty: common 0, score +0.0
        _slot_sharing(rng, 1, {0}),                      # 1  one word, shared, and it is word id 0
        _slot_sharing(rng, 1, set()),                    # 2  one word, not shared
        _slot_sharing(rng, 63, {62}),                    # 3  the last lane of a partial chunk
        _slot_sharing(rng, 64, {63}),                    # 4  only lane 63
        _slot_sharing(rng, 64, {0}),                     # 5  only lane 0
        _slot_sharing(rng, 65, {64}),                    # 6  an empty ballot first (continue), then lane 0 of the second chunk
        _slot_sharing(rng, 129, {128}),                  # 7  two empty ballots, then the single lane of the third chunk
        _slot_sharing(rng, 129, set(range(5, 129, 2))),  # 8  terms in all three chunks: the sum runs across lanes and chunks
        _slot_sharing(rng, 130, set(range(130))),        # 9  everything shared
        _slot_sharing(rng, 64, set()),                   # 10 a full chunk, nothing shared
        NO_BOW,                                          # 11
        EMPTY,                                           # 12
        _slot_sharing(rng, 65, {0, 63, 64}),             # 13 lanes 0 and 63 of the first chunk and lane 0 of the second
    ]
    mask = [1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1]
    facts = [(0, 0, (0, 0.0, -1)), (0, 2, (0, 0.0, -1)), (0, 10, (0, 0.0, -1)), (0, 11, (-1, 0.0, -1)), (0, 12, (-1, 0.0, -1))]
    for s, (cnt, first) in {1: (1, 0), 3: (1, 186), 4: (1, 189), 5: (1, 0), 6: (1, 192), 7: (1, 384), 9: (130, 0), 13: (3, 0)}.items():
        facts.append((0, s, (cnt, None, first)))
    queries = [q, ("slot", 8), ("slot", 9), ("slot", 0), {}]
    return ScoreScene("chunk_edges", "slot sizes 0, 1, 63, 64, 65, 129 and the placement of the shared words inside the 64-lane chunks",
                      slots, queries, mask, facts=facts)


def _query_edges():
    rng = np.random.RandomState(43)
    big = dict(zip(range(0, 2 * 8192, 2), _mixed(rng, 8192)))            # 8192 words: the LDS list at its limit, 13 search steps
    vals = _mixed(rng, 400)
    slots = [
        {w: vals[k] for k, w in enumerate([0, 1, 2, 4095 * 2, 8191, 8191 * 2, 8191 * 2 + 1, 20000])},   # 0 both ends of the big query
        {w: vals[10 + k] for k, w in enumerate(range(1000, 1300))},                                   # 1 300 words, every second one shared
        {w: vals[k] for k, w in enumerate(range(16384, 16384 + 70))},                                  # 2 entirely above the big query
        {w: vals[k] for k, w in enumerate(range(500, 570))},                                           # 3
        {w: big[w] * 0.5 for w in list(big)[:4096]},                                                   # 4 a slot at the table's largest capacity, 4096 words
    ]
    one_hit, one_miss = {1001: 0.375}, {999: 0.375}
    below = {w: vals[k] for k, w in enumerate(range(100, 140))}          # every word below slot 3's: lo == qn on every lane
    above = {w: vals[k] for k, w in enumerate(range(600, 640))}          # every word above slot 3's: lo == 0 on every lane
    queries = [big, {}, one_hit, one_miss, below, above, ("slot", 4), ("slot", 1)]
    facts = [(0, 0, (4, None, 0)), (0, 1, (150, None, 1000)), (0, 2, (0, 0.0, -1)), (1, 1, (0, 0.0, -1)), (2, 1, (1, None, 1001)), (3, 1, (0, 0.0, -1)), (4, 3, (0, 0.0, -1)), (5, 3, (0, 0.0, -1)), (6, 4, (4096, None, 0)), (0, 4, (4096, None, 0))]
    return ScoreScene("query_edges", "queries of 0, 1 and 8192 words (host arrays: a table slot holds at most 4096), a query entirely below or above a slot's words", slots, queries,
                      [1, 1, 1, 0, 1], facts=facts)


def _signed_values():
    rng = np.random.RandomState(47)
    v = _mixed(rng, 80)
    q = {w: (v[w] if w % 3 else -v[w]) for w in range(40)}
    q[40], q[41], q[42] = 0.0, 0.5, -0.25
    slots = [
        {w: (-v[40 + w] if w % 2 else v[40 + w]) for w in range(0, 40)},   # 0 mixed signs: terms of both kinds, a long sum
        {40: 0.0, 41: -0.25, 42: 0.5},                                      # 1 shared words, every term zero: 0 - 0 - 0 and |0.75| - 0.5 - 0.25
        {40: 3.5, 100: 1.0},                                                # 2 one shared word whose query value is zero: |3.5| - 0 - 3.5
        {100: -1.0, 101: 0.0},                                              # 3 nothing shared
        {41: 0.5, 42: -0.25, 43: 7.0},                                      # 4 equal values of either sign: -2 |v| each
    ]
    # a cell with shared words whose terms are all +0 scores -(+0) / 2 = -0.0; a cell with nothing shared scores +0.0
    facts = [(0, 1, (3, -0.0, 40)), (0, 2, (1, -0.0, 40)), (0, 3, (0, 0.0, -1)), (0, 4, (2, 0.75, 41))]
    return ScoreScene("signed_values", "negative and zero values: the sign of a zero score", slots, [q, ("slot", 1), ("slot", 0)],
                      [1, 1, 0, 1, 1], facts=facts)


def _batch(name, nsets, nq, want_per):
    """many queries against many slots: a handful of distinct vectors of at most 40 words, so the restatement runs once per distinct pair.
    Neighbouring slots of one wavefront (s, s + 4, s + 8 ...) differ in kind: whatever a wavefront carried over from a slot would show"""
    assert slots_per_wg(nq, nsets) == want_per and nsets % want_per != 0 and want_per > 4
    rng = np.random.RandomState(nsets)
    vocab = list(range(0, 240, 2))
    distinct = []
    for k in range(11):
        words = sorted(rng.choice(vocab, 5 + 3 * k, replace=False).tolist())
        distinct.append(dict(zip(words, _mixed(rng, len(words)))))
    distinct.append({1: 0.5, 3: 0.25})                                      # shares nothing with any query (odd words)
    distinct.append({})                                                     # present but empty
    qdistinct = []
    for k in range(5):
        words = sorted(rng.choice(vocab, 12 + 7 * k, replace=False).tolist())
        qdistinct.append(dict(zip(words, _mixed(rng, len(words)))))
    qdistinct.append({})
    slots, mask = [], []
    for s in range(nsets):
        if s % 17 == 5:
            slots.append(NO_BOW)
        elif s % 19 == 7:
            slots.append(EMPTY)
        else:
            slots.append(distinct[(s // 4 * 5 + s * 3) % len(distinct)])   # s and s + 4 never hold the same vector
        mask.append(0 if slots[-1] == NO_BOW or s % 5 == 2 else 1)
    queries = []
    for r in range(nq):
        if r % 11 == 3:
            s = (r * 7) % nsets
            while not isinstance(slots[s], dict):
                s = (s + 1) % nsets
            queries.append(("slot", s))
        else:
            queries.append(qdistinct[(r * 5 + r // 6) % len(qdistinct)])
    return ScoreScene(name, "slots_per_wg = %d: %d slots x %d queries, every wavefront loops over %d slots, the last group holds %d"
                      % (want_per, nsets, nq, want_per // 4, nsets % want_per), slots, queries, mask)


def score_scenes():
    if "score" not in _cache:
        _cache["score"] = [_chunk_edges(), _query_edges(), _signed_values(), _batch("batch_8", 130, 256, 8), _batch("batch_64", 515, 512, 64)]
    return _cache["score"]


# =====================================================================================================================================
# (c) decision scenes
# =====================================================================================================================================
class DecisionScene:
    """bows: {slot: BowVector} of every keyframe that ever sits in the table (nsets slots); covis: {slot: ids} (GetBestCovisibilityKeyFrames);
    ops: ("add", s) | ("erase", s) | ("reloc", bow) | ("loop", s, minScore or None = the last minscore result, connected) |
    ("minscore", s, connected).  Ids outside the table may stand among the covisibles and the connected: they name no keyframe.  flip: the flip that must change the list of answers; counter: the trace counter that must be met"""

    def __init__(self, name, rule, flip, counter, nsets, bows, covis, ops):
        self.name, self.rule, self.flip, self.counter, self.nsets, self.bows, self.covis, self.ops = name, rule, flip, counter, nsets, bows, covis, ops

    def best_covisibles(self, s):
        return self.covis.get(int(s), [])


def run_ref(scene, flip=None, traces=None):
    """the script on KeyFrameDatabaseRef: one answer per query op (a list of slots, or the float32 of minscore)"""
    db = ref.KeyFrameDatabaseRef()
    out, last_ms = [], np.float32(1)
    for op in scene.ops:
        tr = {}
        if op[0] == "add":
            db.add(op[1], scene.bows[op[1]])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "reloc":
            out.append(db.detect_relocalization_candidates(op[1], scene.best_covisibles, tr, flip=flip))
        elif op[0] == "loop":
            ms = last_ms if op[2] is None else op[2]
            out.append(db.detect_loop_candidates(scene.bows[op[1]], ms, op[3], scene.best_covisibles, tr, flip=flip))
        elif op[0] == "minscore":
            last_ms = ref.min_score_to_connected(scene.bows[op[1]], [scene.bows[c] for c in op[2] if c in scene.bows])
            out.append(last_ms)
        else:
            raise ValueError(op)
        if traces is not None and tr:
            traces.append(tr)
    return out


def run_db(scene, db):
    """the same script on a mirror with database.py's methods (add, erase, DetectRelocalizationCandidates, DetectLoopCandidates,
    min_score_to_connected); a reloc query goes in as (word, value) host arrays"""
    out, last_ms = [], np.float32(1)
    for op in scene.ops:
        if op[0] == "add":
            db.add(op[1])
        elif op[0] == "erase":
            db.erase(op[1])
        elif op[0] == "reloc":
            q = (np.array(list(op[1].keys()), np.int32), np.array(list(op[1].values()), np.float64))
            out.append(db.DetectRelocalizationCandidates(q, scene.best_covisibles))
        elif op[0] == "loop":
            ms = last_ms if op[2] is None else op[2]
            out.append(db.DetectLoopCandidates(op[1], ms, op[3], scene.best_covisibles))
        elif op[0] == "minscore":
            last_ms = db.min_score_to_connected(op[1], op[2])
            out.append(last_ms)
    return out


def script_text(scene):
    """the scene as the operation-script input of adapter/kfdb_selftest (values as hexadecimal floats)"""
    def bow_line(b):
        return " ".join(["%d" % len(b)] + ["%d %s" % (w, float(v).hex()) for w, v in b.items()])
    cap = max(len(b) for b in scene.bows.values())
    lines = ["script %d %d" % (scene.nsets, cap)]
    for s in range(scene.nsets):
        lines.append(bow_line(scene.bows[s]) if s in scene.bows else "-1")
    for s in range(scene.nsets):
        cv = scene.best_covisibles(s)
        lines.append(" ".join(str(v) for v in [len(cv)] + list(cv)))
    for op in scene.ops:
        if op[0] in ("add", "erase"):
            lines.append("%s %d" % (op[0], op[1]))
        elif op[0] == "reloc":
            lines.append("reloc " + bow_line(op[1]))
        elif op[0] == "loop":
            ms = "last" if op[2] is None else float(np.float32(op[2])).hex()
            lines.append(" ".join(["loop", str(op[1]), ms, str(len(op[3]))] + [str(c) for c in op[3]]))
        elif op[0] == "minscore":
            lines.append(" ".join(["minscore", str(op[1]), str(len(op[2]))] + [str(c) for c in op[2]]))
    return "\n".join(lines) + "\n"


def parse_script_output(text):
    out = []
    for line in text.strip().splitlines():
        kind, rest = line.split(":", 1)
        out.append(np.float32(float.fromhex(rest.strip())) if kind == "minscore" else [int(v) for v in rest.split()])
    return out


def _v(vals, base=0, extra=None):
    """words base, base + 1, ... with the given values, plus the words of `extra`"""
    b = {base + i: float(x) for i, x in enumerate(vals)}
    b.update(extra or {})
    return dict(sorted(b.items()))


Q8 = _v([0.125] * 8)              # the query of most scenes: words 0 .. 7 at 1/8; a keyframe's score is the sum of min(1/8, its value)
P24, P25 = 2.0 ** -24, 2.0 ** -25


def decision_scenes():
    if "dec" in _cache:
        return _cache["dec"]
    S = []
    # ---- the > minCommonWords gate at equality: maxCommonWords 5, int(5 * 0.8f) = 4; B shares exactly 4
    S.append(DecisionScene(
        "common_gate_equality", "commonWords > minCommonWords: 4 words against a gate of 4 do not pass", "common_ge", "common_eq", 6,
        {1: _v([0.125] * 5, extra={100: 0.375}), 3: _v([0.125] * 4, extra={101: 0.5})}, {},
        [("add", 3), ("add", 1), ("reloc", Q8)]))
    # ---- int(maxCommonWords * 0.8f) truncates: 7 * 0.8f = 5.6 -> 5 (rounded: 6); B shares 6
    S.append(DecisionScene(
        "common_gate_truncation", "int(7 * 0.8f) is 5, not 6: a keyframe with 6 words passes", "common_round", None, 4,
        {2: _v([0.125] * 7), 0: _v([0.125] * 6, extra={50: 0.25}), 3: Q8}, {},
        [("add", 2), ("add", 0), ("reloc", Q8), ("loop", 3, 0.0, [])]))
    # ---- si >= minScore at equality; the connected keyframe 4 gives minScore = 0.5 exactly, shares words, is a covisible of 1 and still
    #      is neither candidate nor addend
    S.append(DecisionScene(
        "min_score_equality", "si >= minScore: a score equal to minScore passes; a connected keyframe that is also a covisible",
        "min_score_gt", "min_score_eq", 6,
        {5: _v([0.5, 0.5]), 1: _v([0.25, 0.25, 0.5]), 4: _v([0.5], extra={9: 0.5})}, {1: [4, 77, -1]},
        [("add", 4), ("add", 1), ("minscore", 5, [4, 77, -1]), ("loop", 5, None, [4, -1, 77])]))
    # ---- acc > 0.75f * best at equality: A scores 1.0, B 0.75 with 7 words (gate int(8 * 0.8f) = 6)
    S.append(DecisionScene(
        "retain_equality", "accScore > 0.75f * bestAccScore: 0.75 against a best of 1.0 is dropped", "retain_ge", "retain_eq", 8,
        {6: Q8, 2: _v([0.125] * 5 + [0.0625] * 2, extra={50: 0.25})}, {6: [99], 2: [-1]},
        [("add", 6), ("add", 2), ("reloc", Q8)]))
    # ---- the strict > of the takeover: A and B score 0.5 alike, B is A's covisible and does not take A's entry over; D (0.375) has A as
    #      covisible and A does take D's entry
    half, d = _v([0.0625] * 8, extra={100: 0.5}), _v([0.046875] * 8, extra={101: 0.625})
    S.append(DecisionScene(
        "takeover_strict", "a neighbour takes an entry over only with a strictly better score", "takeover_ge", "takeover_eq", 8,
        {4: half, 1: dict(half), 6: d}, {4: [1], 6: [4]},
        [("add", 4), ("add", 6), ("add", 1), ("reloc", Q8)]))
    # ---- float accumulation in the order of the covisibles: 0.5f + 2^-25 (half an ulp, tie to even: stays) + 2^-24 = 0.5 + 1 ulp;
    #      reversed: 0.5 + 1 ulp, + half an ulp (tie to even: up) = 0.5 + 2 ulp; in double: 0.5 + 1.5 ulp rounds to 2 ulp.
    #      0.75f * best is 0.375 + 2 ulp(0.375) or + 3 ulp; E scores 0.375 + 3 ulp: kept by the reference, dropped otherwise
    S.append(DecisionScene(
        "accumulation_order", "accScore is a float, added to in the order of the covisibles", "acc_reversed", None, 8,
        {3: _v([0.0625] * 8), 7: _v([2.0 ** -28] * 8), 5: _v([2.0 ** -27] * 8), 0: _v([0.0625] * 6 + [P25, P24])}, {3: [7, 5]},
        [("add", 3), ("add", 7), ("add", 5), ("add", 0), ("reloc", Q8)]))
    S.append(DecisionScene(
        "accumulation_float", "accScore is a float: every addition rounds", "acc_double", None, 8,
        S[-1].bows, S[-1].covis, S[-1].ops))
    # ---- the stale mRelocScore: N is scored by the first query (0.5); in the second it shares one word (below the gate, not scored) and
    #      still adds its old 0.5 to A's entry and takes it over.  X was scored alike and erased since: it adds nothing
    q1 = _v([0.125] * 8, base=20)
    S.append(DecisionScene(
        "stale_reloc_score", "a neighbour that shares words adds its mRelocScore even when this query did not score it (:273-276); an "
        "erased covisible and one outside the table add nothing", "reloc_fresh_scores", "stale_used", 8,
        {5: _v([0.0625] * 8, base=20, extra={0: 0.125}), 2: _v([0.0625] * 8, base=20, extra={1: 0.125}), 6: _v([0.03125] * 8), 1: _v([0.0625] * 8)},
        {6: [2, 99, 5, -1]},
        [("add", 5), ("add", 6), ("add", 2), ("add", 1), ("reloc", q1), ("erase", 2), ("reloc", Q8)]))
    # ---- the loop side: N holds a loop score from an earlier query; in this one it shares a word, stays below the gate and adds nothing (:159)
    S.append(DecisionScene(
        "loop_gated_neighbour", "DetectLoopCandidates: a neighbour below the common-word gate adds nothing", "loop_counts_ungated",
        "below_gate_neighbour", 8,
        {5: _v([0.0625] * 8, base=20, extra={0: 0.125}), 6: _v([0.03125] * 8), 1: _v([0.0390625] * 8), 3: q1, 7: Q8}, {6: [5]},
        [("add", 5), ("add", 6), ("add", 1), ("loop", 3, 0.0, []), ("loop", 7, 0.125, [])]))
    # ---- candidate order = (smallest shared word, add sequence), not slot order; erase + add moves a keyframe to the end
    same = _v([0.125] * 7, base=1)
    S.append(DecisionScene(
        "order_by_add_sequence", "lKFsSharingWords is ordered by the first shared word, then by the order of add", "order_by_slot", None, 8,
        {5: dict(same), 2: dict(same), 7: Q8, 0: dict(same), 6: Q8}, {},
        [("add", 5), ("add", 2), ("add", 7), ("add", 0), ("reloc", Q8), ("loop", 6, 0.0, []), ("erase", 5), ("add", 5), ("reloc", Q8),
         ("loop", 6, 0.0, [2, 99, -1])]))
    _cache["dec"] = S
    return S
